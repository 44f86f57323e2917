"""The quantised prefill GEMM (csrc/kernels/prefill_gemm.hip, ops.gemm.
prefill_gemm_w8 / _w4 / _mx4, 65 rows and more): exact layout tests on integer
data for the three weight formats, every pinned launch shape, row independence,
random epilogues against fp32 torch and the calls it does not cover."""
import functools

import pytest
import torch

from tests.gemv_cases import _check_front_end_rejects, _int_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FMTS = ["int8", "int4", "mxfp4"]
SHAPES = [(mt, nt) for mt in (4, 8) for nt in (1, 2, 4)]   # every pair the library has


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _op(fmt):
    from fleetx_amd.ops import gemm as G
    return {"int8": G.prefill_gemm_w8, "int4": G.prefill_gemm_w4, "mxfp4": G.prefill_gemm_mx4}[fmt]


def _quant(fmt, w):
    from fleetx_amd import ops
    return getattr(ops, "quantize_weight_" + fmt)(w), getattr(ops, "dequantize_weight_" + fmt)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """``_int_case`` (integer x, int8 q with the scale 2^-7) and on the same x
    an int4 weight (q4 in [-8, 7], group scales 2^-4 .. 2^-8: every term a
    multiple of 2^-8, sum |x| |w| < 2^13, 21 bits) and an MXFP4 weight (codes
    0..15, group exponents 2^-2 .. 2^2: every term a multiple of 2^-3, sum |x|
    |w| <= 96 K < 2^20, under 24 bits).  fp32 accumulation is then exact in any
    order and the output is the float64 result of the dequantised weight
    rounded once.  {fmt: (packed weight, scale, float64 reference)} on the
    device, with x, bias, residual; shared, callers leave them unchanged."""
    from fleetx_amd import ops
    x, q, b, res, _ = _int_case(M, N, K, M + N + K)
    g = torch.Generator().manual_seed(M * N + K)
    q4 = torch.randint(-8, 8, (N, K), generator=g).to(torch.int8)
    s4 = torch.pow(2.0, -(4.0 + (3 * torch.arange(K // 256)[:, None] + torch.arange(N)[None, :]) % 5))
    codes = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    e = (3 * torch.arange(K // 32)[None, :] + torch.arange(N)[:, None]) % 5 - 2
    packed = {"int8": (q, torch.full((N,), 2.0 ** -7)),
              "int4": (ops.pack_int4(q4), s4.float()),
              "mxfp4": ops.pack_mxfp4(codes, (e + 127).to(torch.uint8))}
    bound = {"int8": 2.0 ** 24 * 2.0 ** -7, "int4": 2.0 ** 13, "mxfp4": 2.0 ** 20}
    out = {}
    for fmt, (p, s) in packed.items():
        w = getattr(ops, "dequantize_weight_" + fmt)(p, s, torch.float64)  # exact in its fp32
        assert float((x.abs() @ w.abs().t()).max()) < bound[fmt]
        out[fmt] = (p.to(DEV), s.to(DEV), x @ w.t() + b)
    return x, b, res, out


def _check_exact(dtype, M, N, K, shape=None, admits=lambda fmt: True):
    """The three formats at one shape, epilogues none / bias / bias + residual,
    against the float64 result rounded once."""
    from fleetx_amd.ops import gemm as G
    x, b, res, per = _case(M, N, K)
    xd, bd, rd = x.to(DEV, dtype), b.to(DEV, dtype), res.to(DEV, dtype)
    for fmt, (p, s, want) in per.items():
        f = _op(fmt)
        y = f(xd, p, s, bd, G.GV_BIAS, shape=shape)
        if not admits(fmt):
            assert y is None, fmt
            continue
        assert y is not None and y.dtype == dtype and y.shape == (M, N), fmt
        assert torch.equal(y.cpu(), want.to(dtype)), fmt
        assert torch.equal(f(xd, p, s, bd, G.GV_RES, res=rd, shape=shape).cpu(),
                           (want + res).to(dtype)), fmt
        assert torch.equal(f(xd, p, s, shape=shape).cpu(), (want - b).to(dtype)), fmt


# one row in the second row tile and ragged N; N under one block; an odd group
# count; several row blocks; N % 8 != 0 (the scalar form of the epilogue: y rows,
# and the residual's, are not 16-byte aligned)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(65, 1000, 1024), (129, 96, 2048), (200, 200, 3072),
                                   (300, 1000, 4096), (70, 1001, 1024)])
def test_prefill_gemm_exact_three_formats(dtype, M, N, K):
    _check_exact(dtype, M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mt,nt", SHAPES)
def test_prefill_gemm_every_launch_shape(dtype, mt, nt):
    # int4 has no 8 x 4 tile (two fp32 tiles per (nt, mt))
    _check_exact(dtype, 200, 1000, 2048, (mt, nt),
                 lambda fmt: not (fmt == "int4" and (mt, nt) == (8, 4)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_prefill_gemm_row_independence(dtype, fmt):
    """Row 5 of a 65-row call and the same x row at index 250 of a 300-row call
    with other rows around it, under two different launch shapes: the same bits."""
    from fleetx_amd.ops import gemm as G
    N, K = 520, 2048
    g = torch.Generator(device=DEV).manual_seed(7)
    xa = torch.randn(65, K, device=DEV, generator=g).to(dtype)
    xb = torch.randn(300, K, device=DEV, generator=g).to(dtype)
    xb[250] = xa[5]
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    wq = _quant(fmt, w)[0]
    ya = _op(fmt)(xa, *wq, b, G.GV_GELU, shape=(4, 1))
    yb = _op(fmt)(xb, *wq, b, G.GV_GELU, shape=(8, 2))
    assert ya is not None and yb is not None
    assert torch.equal(ya[5], yb[250])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K", [(65, 2048, 1024), (300, 1000, 4096)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_prefill_gemm_epilogues(dtype, fmt, M, N, K, epi):
    from fleetx_amd.ops import gemm as G
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + epi)
    x = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    res = torch.randn(M, N, device=DEV, generator=g).to(dtype) if epi == G.GV_RES else None
    wq, deq = _quant(fmt, w)
    y = _op(fmt)(x, *wq, b, epi, res=res)
    assert y is not None
    ref = x.float() @ deq(*wq).t() + b.float()
    if epi == G.GV_GELU:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if epi == G.GV_RES:
        ref = ref + res.float()
    err = _rel(y, ref)
    print("rel err %.3g" % err)
    assert err < (8e-3 if dtype == torch.bfloat16 else 2e-3)


def test_prefill_gemm_uncovered_calls_return_none():
    from fleetx_amd.ops import gemm as G
    bf = dict(device=DEV, dtype=torch.bfloat16)
    q, s = torch.zeros(64, 1024, device=DEV, dtype=torch.int8), torch.ones(64, device=DEV)
    assert G.prefill_gemm_w8(torch.zeros(65, 1024, **bf), q, s) is not None   # the covered twin
    assert G.prefill_gemm_w8(torch.zeros(64, 1024, **bf), q, s) is None
    assert G.prefill_gemm_w8(torch.zeros(65, 1536, **bf),
                             torch.zeros(64, 1536, device=DEV, dtype=torch.int8), s) is None
    assert G.prefill_gemm_w8(torch.zeros(65, 1024, device=DEV), q, s) is None    # fp32 x
    assert G.prefill_gemm_w8(torch.zeros(65, 1024, **bf), q, s, None, G.GV_QKV) is None
    p = torch.zeros(64, 512, device=DEV, dtype=torch.uint8)
    assert G.prefill_gemm_w4(torch.zeros(65, 1024, **bf), p, torch.ones(64, 4, device=DEV)) is None
    assert G.prefill_gemm_mx4(torch.zeros(65, 1024, **bf), p,
                              torch.full((64, 16), 127, device=DEV, dtype=torch.uint8)) is None
    _check_front_end_rejects(65, G.prefill_gemm_w8)
