"""The pieces of the window decode step on the GPU: the cache-row map of the
QKV GEMV epilogue (16-bit, int8 and int4 weights) and ``_window_step`` against
W plain decode steps fed the same tokens one at a time."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _linear(policy, x, w, b, epi, **kw):
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    if policy == "w16":
        return G.decode_linear(x, w, b, epi, **kw)
    if policy == "w8":
        return G.decode_linear_w8(x, *ops.quantize_weight_int8(w), b, epi, **kw)
    return G.decode_linear_w4(x, *ops.quantize_weight_int4(w), b, epi, **kw)


@pytest.mark.parametrize("policy", ["w16", "w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,D", [(5, 64), (3, 128)])
def test_qkv_scatter_with_row_map(policy, dtype, H, D):
    """M = 15 rows into 3 cache rows x 5 positions and M = 2 into cache row 1
    only.  The reference is the same kernel's no-map output: q is the same, and
    K/V row m of the no-map call sits, bit for bit, at cache[rows[m], pos[m]];
    nothing else is written.  The no-map call itself equals the GV_BIAS output
    of the same GEMV scattered in torch (the addressing of the 3-tuple form)."""
    from fleetx_amd.ops import gemm as G
    K, L, N = 1024, 24, 3 * H * D
    g = torch.Generator(device=DEV).manual_seed(H * D)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    for M, rows, pos in ((15, [0] * 5 + [1] * 5 + [2] * 5, [3, 4, 5, 6, 7, 0, 1, 2, 3, 4] + [19, 20, 21, 22, 23]),
                         (2, [1, 1], [7, 8])):
        x = torch.randn(M, K, device=DEV, generator=g).to(dtype)
        rows = torch.tensor(rows, device=DEV, dtype=torch.int32)
        pos = torch.tensor(pos, device=DEV)
        ar = torch.arange(M, device=DEV)
        # no map: today's addressing cache[m, pos[m]]
        kc0 = torch.zeros(M, L, H, D, device=DEV, dtype=dtype)
        vc0 = torch.zeros_like(kc0)
        q0 = _linear(policy, x, w, b, G.GV_QKV, qkv_cache=(kc0, vc0, pos))
        y = _linear(policy, x, w, b, G.GV_BIAS)
        assert q0 is not None and y is not None
        y5 = y.view(M, H, 3, D)
        assert torch.equal(q0.view(M, H, D), y5[:, :, 0])
        assert torch.equal(kc0[ar, pos], y5[:, :, 1]) and torch.equal(vc0[ar, pos], y5[:, :, 2])
        mask = torch.ones(M, L, dtype=torch.bool, device=DEV)
        mask[ar, pos] = False
        assert kc0[mask].abs().max().item() == 0 and vc0[mask].abs().max().item() == 0
        # with the map
        kc = torch.zeros(3, L, H, D, device=DEV, dtype=dtype)
        vc = torch.zeros_like(kc)
        q1 = _linear(policy, x, w, b, G.GV_QKV, qkv_cache=(kc, vc, pos, rows))
        assert q1 is not None and torch.equal(q1, q0)
        want_k, want_v = torch.zeros_like(kc), torch.zeros_like(vc)
        want_k[rows.long(), pos] = kc0[ar, pos]
        want_v[rows.long(), pos] = vc0[ar, pos]
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v)


def _big_model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return cfg, GPTForPretraining(cfg).cuda().eval()


@pytest.mark.parametrize("fused,quant", [(True, None), (True, "int8"), (False, None)])
def test_window_step_matches_sequential_steps(fused, quant):
    """B = 3, W = 5, cur = [3, 0, 40]: the window step's logits rows and appended
    K/V rows against W ``_decode_step`` calls fed the same tokens one at a
    time; cache rows outside the window stay as they were."""
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = _big_model()
    B, W, H, D, L = 3, 5, 8, 128, 64
    gen = gmod.GPTForGeneration(model, {"fused_decode": fused, "weight_quant": quant}).eval()
    if quant is not None:
        assert gen.requantize() is True
    g = torch.Generator(device=DEV).manual_seed(7)
    cache = gmod.KVCache(cfg.num_layers, B, L, H, D, torch.bfloat16, DEV)
    for li in range(cfg.num_layers):
        cache.k[li].normal_(generator=g)
        cache.v[li].normal_(generator=g)
    seq = gmod.KVCache(cfg.num_layers, B, L, H, D, torch.bfloat16, DEV)
    for li in range(cfg.num_layers):
        seq.k[li].copy_(cache.k[li])
        seq.v[li].copy_(cache.v[li])
    before = [c.clone() for c in cache.k + cache.v]
    cur = torch.tensor([3, 0, 40], device=DEV)
    tok = torch.randint(0, 1024, (B, W), device=DEV, generator=g)
    ar = torch.arange(W, device=DEV)
    pos = (cur[:, None] + ar[None, :]).reshape(-1)
    rows = torch.arange(B, device=DEV, dtype=torch.int32).repeat_interleave(W)
    calls = []
    orig = gmod._layer_decode_fused
    gmod._layer_decode_fused = lambda *a: calls.append(orig(*a)) or calls[-1]
    try:
        with torch.no_grad():
            lg = gen._window_step(tok.reshape(-1), pos, rows, cur.to(torch.int32), cache)
    finally:
        gmod._layer_decode_fused = orig
    if fused:
        assert len(calls) == cfg.num_layers and all(c is not None for c in calls)  # fused ran
    else:
        assert not calls
    assert lg.shape == (B * W, 1024) and lg.dtype == torch.float32
    with torch.no_grad():
        ref = torch.stack([gen._decode_step(tok[:, j].contiguous(), cur + j, seq)
                           for j in range(W)], 1)                       # [B, W, V]
    worst = max(_rel(lg.view(B, W, -1)[:, j], ref[:, j]) for j in range(W))
    print("window step vs sequential steps (fused %s, %s): worst logits rel %.3g"
          % (fused, quant, worst))
    assert worst < 2e-2
    inside = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    inside[rows.long(), pos] = True
    for got, want, old in zip(cache.k + cache.v, seq.k + seq.v, before):
        assert _rel(got[inside], want[inside]) < 2e-2
        assert torch.equal(got[~inside], old[~inside])
