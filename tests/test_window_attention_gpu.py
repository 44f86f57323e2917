"""Window decode attention (W causal queries per sample over one KV cache):
the kernel against its fp32 formula branch, exact slot invariance, and the
formula branch for shapes the kernel does not hold."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXLEN = 720


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _case(dtype, D, W, B, H, lens, nan_from):
    """Random q and caches; NaN in every cache row at or beyond
    ``lens[b] + nan_from``."""
    g = torch.Generator(device=DEV).manual_seed(W * 131 + D + H)
    q = torch.randn(B * W, H, D, device=DEV, generator=g).to(dtype)
    k, v = (torch.randn(B, MAXLEN, H, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    lens = torch.tensor(lens, device=DEV, dtype=torch.int32)
    mask = torch.arange(MAXLEN, device=DEV)[None, :] >= (lens[:, None] + nan_from)
    k[mask], v[mask] = float("nan"), float("nan")
    return q, k, v, lens


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("BH", [(2, 4), (2, 32)])
@pytest.mark.parametrize("first", [0, 1])
def test_window_decode_attention_kernel(dtype, D, W, BH, first):
    """Kernel vs the fp32 formula: a window at position 0 (query 0 sees exactly
    one key), a window that ends with the cache, splits that end up empty, both
    workgroup widths, and NaN in every cache row at or beyond ``lens + W``."""
    from fleetx_amd import ops
    from fleetx_amd.ops.attention import _window_attention_formula
    B, H = BH
    lens = [0, 693] if first == 0 else [MAXLEN - W, 1]
    q, k, v, lens = _case(dtype, D, W, B, H, lens, W)
    ref = _window_attention_formula(q.float(), k, v, lens, W, D ** -0.5)
    assert torch.isfinite(ref).all()
    for nsplit in (1, None, 7):
        for waves in (4, 8):
            out = ops.window_decode_attention(q, k, v, lens, nsplit=nsplit, waves=waves)
            assert out.dtype == dtype and out.shape == (B * W, H, D)
            assert torch.isfinite(out).all(), (nsplit, waves)
            assert _rel(out, ref) < 1e-2, (nsplit, waves)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nsplit", [1, None, 7])
@pytest.mark.parametrize("waves", [4, 8])
def test_window_slot_invariance_exact(dtype, D, nsplit, waves):
    """The W = 5 result of slot j, bit for bit, from the same query in slot 0
    of a W = 5 window that starts j keys later on the same cache contents
    (the same instantiation and split count; the other four slots of that call
    carry other queries).  347 + j straddles a split boundary at nsplit 7."""
    from fleetx_amd import ops
    W, B, H = 5, 2, 4
    # rows up to lens + 2W - 1 are loaded by the shifted windows: NaN from there on
    q, k, v, lens = _case(dtype, D, W, B, H, [0, 347], 2 * W)
    out = ops.window_decode_attention(q, k, v, lens, nsplit=nsplit, waves=waves)
    assert torch.isfinite(out).all()
    g = torch.Generator(device=DEV).manual_seed(5)
    for j in range(W):
        q2 = torch.randn(B * W, H, D, device=DEV, generator=g).to(dtype)
        q2[0::W] = q[j::W]
        out2 = ops.window_decode_attention(q2, k, v, lens + j, nsplit=nsplit, waves=waves)
        assert torch.equal(out2[0::W], out[j::W]), j


def test_window_nine_queries_use_formula():
    """More queries than the kernel holds run the formula branch, not an error."""
    from fleetx_amd import ops
    B, W, H, D = 1, 9, 2, 64
    q = torch.randn(B * W, H, D, device=DEV).bfloat16()
    k, v = (torch.randn(B, 40, H, D, device=DEV).bfloat16() for _ in range(2))
    lens = torch.tensor([20], device=DEV, dtype=torch.int32)
    out = ops.window_decode_attention(q, k, v, lens)
    ref = ops.window_decode_attention(q.cpu().float(), k.cpu(), v.cpu(), lens.cpu())
    assert out.shape == (B * W, H, D) and _rel(out.cpu(), ref) < 1e-2


def test_window_cpu_matches_formula():
    """A CPU call is the formula; checked here against per-query softmax."""
    from fleetx_amd import ops
    from fleetx_amd.ops.attention import _window_attention_formula
    B, W, H, D, L = 2, 3, 2, 16, 12
    q = torch.randn(B * W, H, D)
    k, v = torch.randn(B, L, H, D), torch.randn(B, L, H, D)
    lens = torch.tensor([0, 5], dtype=torch.int32)
    for b in range(B):
        k[b, int(lens[b]) + W:] = float("nan")
        v[b, int(lens[b]) + W:] = float("nan")
    out = ops.window_decode_attention(q, k, v, lens)
    assert torch.equal(out, _window_attention_formula(q, k, v, lens, W, D ** -0.5))
    for b in range(B):
        for j in range(W):
            n = int(lens[b]) + j + 1
            s = torch.einsum("hd,lhd->hl", q[b * W + j], k[b, :n]) * D ** -0.5
            ref = torch.einsum("hl,lhd->hd", torch.softmax(s, -1), v[b, :n])
            assert torch.allclose(out[b * W + j], ref, atol=1e-5)
