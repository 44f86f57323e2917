"""The skinny GEMM of the 17..64-row decode step (csrc/kernels/decode_gemm.hip,
ops.gemm.decode_gemm / _w8 / _w4): exact layout tests on integer data for the
three weight formats, every launch shape, the QKV scatter, row independence,
random epilogues against fp32 torch and the calls it does not cover."""
import functools

import pytest
import torch

from tests.gemv_cases import _check_front_end_rejects, _int_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(nt, ks) for nt in (1, 2, 4) for ks in (4, 8)]   # every pair the library has


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """``_int_case`` (weight q * 2^-7: exact in both dtypes, fp32 sums exact in
    any order) and, on the same integer x, an int4 weight: q4 in [-8, 7] with
    group scales 2^-4 .. 2^-8 [K / 256, N].  Every int4 term is a multiple of
    2^-8 and sum |x| |q4| s < 2^13, so every partial sum in any order has at most
    21 bits: exact in fp32.  Shared: callers leave the tensors unchanged."""
    x, q, b, res, ref = _int_case(M, N, K, M + N + K)
    g = torch.Generator().manual_seed(M * N + K)
    q4 = torch.randint(-8, 8, (N, K), generator=g).to(torch.int8)
    G = K // 256
    s4 = torch.pow(2.0, -(4.0 + (3 * torch.arange(G)[:, None] + torch.arange(N)[None, :]) % 5))
    w4 = (q4.double().view(N, G, 256) * s4.double().t()[:, :, None]).view(N, K)
    assert float((x.abs() @ w4.abs().t()).max()) < 2 ** 13
    return x, q, b, res, ref, q4, s4.float(), x @ w4.t() + b


def _check_exact(dtype, M, N, K, shape=None, admits=lambda fmt: True):
    """The three formats at one shape, epilogues none / bias / bias + residual,
    against the float64 result rounded once."""
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    x, q, b, res, ref, q4, s4, ref4 = _case(M, N, K)
    xd, bd, rd = x.to(DEV, dtype), b.to(DEV, dtype), res.to(DEV, dtype)
    w = (q.double() * 2.0 ** -7).to(dtype)
    assert torch.equal(w.double(), q.double() * 2.0 ** -7)
    s8 = torch.full((N,), 2.0 ** -7, device=DEV)
    calls = {"w16": (lambda *a, **k: G.decode_gemm(xd, w.to(DEV), *a, **k), ref),
             "int8": (lambda *a, **k: G.decode_gemm_w8(xd, q.to(DEV), s8, *a, **k), ref),
             "int4": (lambda *a, **k: G.decode_gemm_w4(xd, ops.pack_int4(q4).to(DEV), s4.to(DEV),
                                                       *a, **k), ref4)}
    for fmt, (f, want) in calls.items():
        if not admits(fmt):
            assert f(bd, G.GV_BIAS, shape=shape) is None
            continue
        y = f(bd, G.GV_BIAS, shape=shape)
        assert y is not None and y.dtype == dtype and y.shape == (M, N), fmt
        assert torch.equal(y.cpu(), want.to(dtype)), fmt
        assert torch.equal(f(bd, G.GV_RES, res=rd, shape=shape).cpu(), (want + res).to(dtype)), fmt
        assert torch.equal(f(shape=shape).cpu(), (want - b).to(dtype)), fmt


# a last row tile of one row, N no multiple of 8 / 16 / 64, N under one block,
# one int4 group per wave (K = 1024), an odd group count (K = 3072)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(17, 1000, 1024), (33, 96, 2048), (48, 200, 3072),
                                   (64, 1000, 4096)])
def test_decode_gemm_exact_three_formats(dtype, M, N, K):
    _check_exact(dtype, M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nt,ks", SHAPES)
def test_decode_gemm_every_launch_shape(dtype, nt, ks):
    # int4 has no 4 x 4 tile (two fp32 tiles per (nt, mt) do not fit the registers)
    _check_exact(dtype, 64, 1000, 2048, (nt, ks), lambda fmt: not (fmt == "int4" and nt == 4))


def test_decode_gemm_pinned_shape_not_admitted():
    from fleetx_amd.ops import gemm as G
    x = torch.zeros(20, 1024, device=DEV, dtype=torch.bfloat16)
    p = torch.zeros(64, 512, device=DEV, dtype=torch.uint8)
    s = torch.ones(4, 64, device=DEV)
    assert G.decode_gemm_w4(x, p, s, shape=(1, 4)) is not None
    assert G.decode_gemm_w4(x, p, s, shape=(1, 8)) is None     # 128 k per wave: half a scale group
    assert G.decode_gemm(x, torch.zeros(64, 1024, device=DEV, dtype=torch.bfloat16),
                         shape=(3, 4)) is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("H,D", [(5, 64), (3, 128)])
@pytest.mark.parametrize("mapped", [False, True])
def test_decode_gemm_exact_qkv_scatter(dtype, M, H, D, mapped):
    from fleetx_amd.ops import gemm as G
    N, K, L = 3 * H * D, 1024, 24
    x, q, b, _, ref = _case(M, N, K)[:5]
    w = (q.double() * 2.0 ** -7).to(dtype)
    ar = torch.arange(M)
    if mapped:      # M rows over 8 cache rows: (m % 8, m // 8 * 3 + 1) is distinct per m
        rows, pos, R = (ar % 8).to(DEV, torch.int32), (ar // 8 * 3 + 1).to(DEV), 8
    else:
        rows, pos, R = None, ((ar * 7 + 3) % L).to(DEV), M
    kc = torch.zeros(R, L, H, D, device=DEV, dtype=dtype)
    vc = torch.zeros_like(kc)
    out = G.decode_gemm(x.to(DEV, dtype), w.to(DEV), b.to(DEV, dtype), G.GV_QKV,
                        qkv_cache=(kc, vc, pos) if rows is None else (kc, vc, pos, rows))
    assert out is not None and out.shape == (M, H * D)
    r = ref.to(dtype).view(M, H, 3, D)
    cr = ar.to(DEV) if rows is None else rows.long()
    assert torch.equal(out.view(M, H, D).cpu(), r[:, :, 0])
    assert torch.equal(kc[cr, pos].cpu(), r[:, :, 1])
    assert torch.equal(vc[cr, pos].cpu(), r[:, :, 2])
    mask = torch.ones(R, L, dtype=torch.bool, device=DEV)
    mask[cr, pos] = False
    assert int(mask.sum()) == R * L - M
    assert kc[mask].abs().max().item() == 0 and vc[mask].abs().max().item() == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_gemm_row_independence(dtype):
    """Row 5 of a 17-row call and the same x row at index 60 of a 64-row call
    with other rows around it: the same bits, in every format."""
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    N, K = 520, 2048
    g = torch.Generator(device=DEV).manual_seed(7)
    xa = torch.randn(17, K, device=DEV, generator=g).to(dtype)
    xb = torch.randn(64, K, device=DEV, generator=g).to(dtype)
    xb[60] = xa[5]
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    for f, wq in ((G.decode_gemm, (w,)), (G.decode_gemm_w8, ops.quantize_weight_int8(w)),
                  (G.decode_gemm_w4, ops.quantize_weight_int4(w))):
        ya, yb = f(xa, *wq, b, G.GV_GELU), f(xb, *wq, b, G.GV_GELU)
        assert ya is not None and yb is not None
        assert torch.equal(ya[5], yb[60]), f.__name__


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(17, 2048, 1024), (64, 1000, 4096)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_decode_gemm_epilogues(dtype, M, N, K, epi):
    from fleetx_amd.ops import gemm as G
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + epi)
    x = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    res = torch.randn(M, N, device=DEV, generator=g).to(dtype) if epi == G.GV_RES else None
    y = G.decode_gemm(x, w, b, epi, res=res)
    assert y is not None
    ref = x.float() @ w.float().t() + b.float()
    if epi == G.GV_GELU:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if epi == G.GV_RES:
        ref = ref + res.float()
    tol = 8e-3 if dtype == torch.bfloat16 else 2e-3
    assert _rel(y, ref) < tol


def test_decode_gemm_uncovered_calls_return_none():
    from fleetx_amd.ops import gemm as G
    bf = dict(device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(64, 1024, **bf)
    assert G.decode_gemm(torch.zeros(17, 1024, **bf), w) is not None   # the covered twin
    assert G.decode_gemm(torch.zeros(16, 1024, **bf), w) is None
    assert G.decode_gemm(torch.zeros(65, 1024, **bf), w) is None
    assert G.decode_gemm(torch.zeros(20, 1536, **bf), torch.zeros(64, 1536, **bf)) is None
    assert G.decode_gemm(torch.zeros(20, 1024, device=DEV), w) is None            # fp32 x
    x = torch.zeros(20, 1024, **bf)
    assert G.decode_gemm(x, w.half()) is None                          # weight dtype != x dtype
    assert G.decode_gemm_w8(x, w, torch.ones(64, device=DEV)) is None  # not int8
    with pytest.raises(AssertionError):                                # never reaches the binding
        G.decode_gemm(x, w, None, G.GV_RES)
    _check_front_end_rejects(17, G.decode_gemm_w8, G.decode_gemm)
