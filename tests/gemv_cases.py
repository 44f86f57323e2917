"""Shared data for the exact decode-GEMV layout tests (test_decode_gpu.py,
test_decode_w8_gpu.py) and the inputs every skinny-GEMM front end rejects."""
import torch


def _check_front_end_rejects(M, w8, w16=None):
    """Calls the shared front end of ``ops.gemm`` does not cover, at a family's
    smallest covered shape (M rows, N = 64, K = 1024): ``w8`` is the family's
    int8 function, ``w16`` its 16-bit one if it has one.  Each returns None."""
    bf = dict(device="cuda", dtype=torch.bfloat16)
    x = torch.zeros(M, 1024, **bf)
    q = torch.zeros(64, 1024, device="cuda", dtype=torch.int8)
    s = torch.ones(64, device="cuda")
    b2 = torch.zeros(128, **bf)[::2]                   # 64 elements, not contiguous
    xs = torch.zeros(M, 1028, **bf)[:, :1024]          # row stride no multiple of 8
    assert not b2.is_contiguous() and xs.stride(0) % 8 and xs.data_ptr() % 16 == 0
    assert w8(x, q, s) is not None                     # the covered twin
    assert w8(x, q, None) is None
    assert w8(x, q, s.half()) is None                  # scale dtype
    assert w8(x, q, s, b2) is None
    assert w8(xs, q, s) is None
    if w16 is not None:
        w = torch.zeros(64, 1024, **bf)
        assert w16(x, w) is not None
        assert w16(x, w, b2) is None
        assert w16(xs, w) is None


def _int_case(M, N, K, seed):
    """Integer x [M, K], int8 q [N, K], bias and residual, and the float64
    result ``x q^T 2^-7 + b``.  Every partial sum is an integer < 2^24, so fp32
    accumulation is exact in any order and a kernel's output must equal the
    float64 result rounded once."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    q = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
    b = torch.randint(-8, 9, (N,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double()
    acc = x @ q.double().t()
    assert float(acc.abs().max()) < 2 ** 24
    return x, q, b, res, acc * 2.0 ** -7 + b
