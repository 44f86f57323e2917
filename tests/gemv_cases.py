"""Shared data for the exact decode-GEMV layout tests (test_decode_gpu.py,
test_decode_w8_gpu.py)."""
import torch


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
