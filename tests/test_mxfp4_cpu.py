"""MXFP4 weight format on the host (fleetx_amd/ops/quant.py): the storage
layout's round trip, exact quantisation of representable data, the scale rule
and the rounding bound."""
import pytest
import torch

from fleetx_amd import ops

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (5, 1024 + 96), generator=g).to(torch.uint8)
    exps = torch.randint(1, 255, (5, 35), generator=g).to(torch.uint8)
    packed, scale = ops.pack_mxfp4(codes, exps)
    assert packed.shape == (5, 560) and scale.shape == (5, 35)
    c2, e2 = ops.unpack_mxfp4(packed, scale)
    assert torch.equal(c2, codes) and torch.equal(e2, exps)


def test_representable_matrix_is_exact():
    """Every group holds +-6 X, so its scale is X: the matrix comes back."""
    g = torch.Generator().manual_seed(1)
    n, k = 6, 2048
    val = E2M1[torch.randint(0, 8, (n, k // 32, 32), generator=g)]
    val[:, :, 0] = 6.0
    val = val * (1 - 2 * torch.randint(0, 2, val.shape, generator=g))
    e = torch.randint(-13, 14, (n, k // 32, 1), generator=g)
    w = torch.ldexp(val, e).view(n, k)
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(ops.dequantize_weight_mxfp4(*ops.quantize_weight_mxfp4(w), dtype),
                           w.to(dtype))


def test_scale_rule_and_rounding_bound():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(9, 1024, generator=g) * torch.logspace(-3, 3, 9)[:, None]
    w[4, 64:96] = 0
    packed, scale = ops.quantize_weight_mxfp4(w)
    _, exps = ops.unpack_mxfp4(packed, scale)
    X = torch.ldexp(torch.ones(9, 32), exps.int() - 127)
    amax = w.view(9, 32, 32).abs().amax(2)
    nz = amax > 0
    assert (amax <= 6 * X).all() and (6 * X < 2 * amax)[nz].all() and (exps[~nz] == 127).all()
    # half the e2m1 spacing at |w| / X: 0.5 below 2, 1 below 4, 2 up to 6
    v = w.view(9, 32, 32).abs() / X[:, :, None]
    half = torch.where(v < 2, 0.25, torch.where(v < 4, 0.5, 1.0)) * X[:, :, None]
    err = (w - ops.dequantize_weight_mxfp4(packed, scale)).view(9, 32, 32).abs()
    assert (err <= half).all()


def test_k_not_a_multiple_of_32_raises():
    with pytest.raises(ValueError):
        ops.quantize_weight_mxfp4(torch.zeros(4, 48))
