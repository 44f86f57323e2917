"""Weight-only MXFP4 decode (csrc/kernels/decode_gemv_mx4.hip, GM4 of
decode_gemm.hip, ops.gemm.decode_linear_mx4 / decode_gemm_mx4, ``weight_quant:
mxfp4``): exact layout tests on integer data for the GEMV and the skinny GEMM,
the LayerNorm prologue, uncovered calls, the fused decode step and generation."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Integer x in [-4, 4], codes uniform over all 16, group scales 2^-1 ..
    2^-5 varying per (row, group) (a wrong nibble, byte, group or row changes
    the result), bias and residual in [-8, 8] and the float64 result.  Every
    term is a multiple of 2^-6 and sum |x| |w| <= 12 K < 2^16: 22 bits, so fp32
    is exact in any order and the output must equal the result rounded once.
    Returns device operands; shared, callers leave them unchanged."""
    from fleetx_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    codes = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    e = -(1 + (3 * torch.arange(K // 32)[None, :] + torch.arange(N)[:, None]) % 5)
    b = torch.randint(-8, 9, (N,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double()
    w = E2M1[(codes & 7).long()] * (1 - 2 * (codes >> 3).double())
    w = (w.view(N, K // 32, 32) * torch.pow(2.0, e.double())[:, :, None]).view(N, K)
    assert float((x.abs() @ w.abs().t()).max()) <= 12 * K < 2 ** 16
    p, s = ops.pack_mxfp4(codes, (e + 127).to(torch.uint8))
    return x.to(DEV), p.to(DEV), s.to(DEV), b, res, x @ w.t() + b


def _check_exact(f, dtype, M, N, K, **kw):
    """Epilogues bias / bias + residual / none against the rounded float64."""
    from fleetx_amd.ops import gemm as G
    x, p, s, b, res, ref = _case(M, N, K)
    xd, bd, rd = x.to(dtype), b.to(DEV, dtype), res.to(DEV, dtype)
    y = f(xd, p, s, bd, G.GV_BIAS, **kw)
    assert y is not None and y.dtype == dtype and y.shape == (M, N)
    assert torch.equal(y.cpu(), ref.to(dtype))
    assert torch.equal(f(xd, p, s, bd, G.GV_RES, res=rd, **kw).cpu(), (ref + res).to(dtype))
    assert torch.equal(f(xd, p, s, **kw).cpu(), (ref - b).to(dtype))


# ragged N and one chunk per wave; 8 waves; three chunks per wave (odd: one
# chunk per batch, both parities of the scale dword); four (two per batch)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(3, 1001, 1024), (16, 96, 2048), (5, 200, 3072),
                                   (1, 2000, 4096)])
def test_mx4_gemv_exact(dtype, M, N, K):
    from fleetx_amd.ops import gemm as G
    _check_exact(G.decode_linear_mx4, dtype, M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(17, 1000, 1024), (33, 96, 2048), (48, 200, 3072),
                                   (64, 1000, 4096)])
def test_mx4_gemm_exact(dtype, M, N, K):
    from fleetx_amd.ops import gemm as G
    _check_exact(G.decode_gemm_mx4, dtype, M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nt", [1, 2, 4])
@pytest.mark.parametrize("ks", [4, 8])
def test_mx4_gemm_every_launch_shape(dtype, nt, ks):
    from fleetx_amd.ops import gemm as G
    _check_exact(G.decode_gemm_mx4, dtype, 64, 1000, 2048, shape=(nt, ks))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("H,D", [(5, 64), (3, 128)])
@pytest.mark.parametrize("mapped", [False, True])
def test_mx4_exact_qkv_scatter(dtype, M, H, D, mapped):
    from fleetx_amd.ops import gemm as G
    N, K, L = 3 * H * D, 1024, 24
    x, p, s, b, _, ref = _case(M, N, K)
    ar = torch.arange(M, device=DEV)
    if mapped:      # M rows over 4 cache rows: (m % 4, m // 4 * 3 + 1) is distinct per m
        rows, pos, R = (ar % 4).int(), ar // 4 * 3 + 1, 4
    else:
        rows, pos, R = None, (ar * 7 + 3) % L, M
    kc = torch.zeros(R, L, H, D, device=DEV, dtype=dtype)
    vc = torch.zeros_like(kc)
    out = G.decode_linear_mx4(x.to(dtype), p, s, b.to(DEV, dtype), G.GV_QKV,
                              qkv_cache=(kc, vc, pos) if rows is None else (kc, vc, pos, rows))
    assert out is not None and out.shape == (M, H * D)
    r = ref.to(dtype).view(M, H, 3, D)
    cr = ar if rows is None else rows.long()
    assert torch.equal(out.view(M, H, D).cpu(), r[:, :, 0])
    assert torch.equal(kc[cr, pos].cpu(), r[:, :, 1])
    assert torch.equal(vc[cr, pos].cpu(), r[:, :, 2])
    mask = torch.ones(R, L, dtype=torch.bool, device=DEV)
    mask[cr, pos] = False
    assert int(mask.sum()) == R * L - M
    assert kc[mask].abs().max().item() == 0 and vc[mask].abs().max().item() == 0


@pytest.mark.parametrize("M,N,K", [(1, 960, 2048), (4, 960, 3072)])
@pytest.mark.parametrize("epi", [1, 3])
def test_mx4_fused_layernorm(M, N, K, epi):
    """The comparison and the bound of test_w4_fused_layernorm: 16-bit operands,
    fp32 accumulation, one rounding, against fp32 torch on the dequantised weight."""
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    g = torch.Generator(device=DEV).manual_seed(M + N + K + epi)
    x = (3.0 + torch.randn(M, K, device=DEV, generator=g)).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, device=DEV, generator=g).bfloat16()
    lw = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).bfloat16()
    lb = (0.1 * torch.randn(K, device=DEV, generator=g)).bfloat16()
    p, s = ops.quantize_weight_mxfp4(w)
    xn = torch.nn.functional.layer_norm(x.float(), (K,), lw.float(), lb.float(), 1e-5)
    ref = xn.bfloat16().float() @ ops.dequantize_weight_mxfp4(p, s).t() + b.float()
    H, D, L = N // 192, 64, 8
    kc = torch.zeros(M, L, H, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    pos = torch.arange(M, device=DEV) % L
    kw = dict(qkv_cache=(kc, vc, pos)) if epi == G.GV_QKV else {}
    y = G.decode_linear_mx4(x, p, s, b, epi, ln=(lw, lb, 1e-5), **kw)
    assert y is not None
    if epi == G.GV_GELU:
        assert _rel(y, torch.nn.functional.gelu(ref, approximate="tanh")) < 8e-3
    else:
        r = ref.view(M, H, 3, D)
        ar = torch.arange(M, device=DEV)
        assert _rel(y.view(M, H, D), r[:, :, 0]) < 8e-3
        assert _rel(kc[ar, pos], r[:, :, 1]) < 8e-3
        assert _rel(vc[ar, pos], r[:, :, 2]) < 8e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_mx4_gemm_row_independence(dtype):
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    N, K = 520, 2048
    g = torch.Generator(device=DEV).manual_seed(7)
    xa = torch.randn(17, K, device=DEV, generator=g).to(dtype)
    xb = torch.randn(64, K, device=DEV, generator=g).to(dtype)
    xb[60] = xa[5]
    wq = ops.quantize_weight_mxfp4(torch.randn(N, K, device=DEV, generator=g) * K ** -0.5)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    ya, yb = G.decode_gemm_mx4(xa, *wq, b, G.GV_GELU), G.decode_gemm_mx4(xb, *wq, b, G.GV_GELU)
    assert ya is not None and yb is not None
    assert torch.equal(ya[5], yb[60])


def test_mx4_uncovered_calls_return_none():
    from fleetx_amd.ops import gemm as G
    bf = dict(device=DEV, dtype=torch.bfloat16)
    u8 = dict(device=DEV, dtype=torch.uint8)
    p, s = torch.zeros(64, 512, **u8), torch.full((64, 32), 127, **u8)
    for f, m, over in ((G.decode_linear_mx4, 2, 17), (G.decode_gemm_mx4, 20, 65)):
        assert f(torch.zeros(m, 1024, **bf), p, s) is not None                 # the covered twin
        assert f(torch.zeros(over, 1024, **bf), p, s) is None                  # M out of range
        assert f(torch.zeros(m, 1024, device=DEV), p, s) is None               # fp32 x
        assert f(torch.zeros(m, 1024, **bf), p.to(torch.int8), s) is None      # not uint8
        assert f(torch.zeros(m, 1024, **bf), p, s.float()) is None             # scale dtype
        assert f(torch.zeros(m, 1024, **bf), p, s.t().contiguous()) is None    # scale shape
        assert f(torch.zeros(m, 1536, **bf), torch.zeros(64, 768, **u8),
                 torch.full((64, 48), 127, **u8)) is None                      # K % 1024 != 0


# ----------------------------------------------------------------------------
# the decode step and generation with weight_quant / spec_draft: mxfp4 (the
# small_model pattern and the 2e-2 of test_decode_w4_gpu.py)
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return cfg, GPTForPretraining(cfg).cuda().eval()


def _pair(model, rows):
    """(mxfp4 fused generator, unfused generator on the dequantised weights; the
    16-bit table still serves its embedding lookup, the dequantised one its head)."""
    from fleetx_amd import ops
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    a = GPTForGeneration(model, {"weight_quant": "mxfp4", "fused_decode_rows": rows}).eval()
    assert a.requantize() is True
    twin = copy.deepcopy(model)
    dq = lambda w: ops.dequantize_weight_mxfp4(*ops.quantize_weight_mxfp4(w), w.dtype)  # noqa: E731
    with torch.no_grad():
        for layer in twin.gpt.layers:
            for lin in (layer.attn.qkv_proj, layer.attn.out_proj, layer.mlp.fc1, layer.mlp.fc2):
                lin.weight.copy_(dq(lin.weight))
        head = dq(twin.gpt.embeddings.word_embeddings.weight)
    b = GPTForGeneration(twin, {"fused_decode": False}).eval()
    b._logits = lambda h, q8=None: torch.nn.functional.linear(h, head).float()
    return a, b


@pytest.mark.parametrize("B,name", [(6, "decode_linear_mx4"), (20, "decode_gemm_mx4")])
def test_mx4_fused_decode_step_matches_dequantised_unfused(small_model, monkeypatch, B, name):
    from fleetx_amd.models.language_model.gpt.generation import KVCache
    from fleetx_amd.ops import gemm as G
    cfg, model = small_model
    orig, ran = getattr(G, name), []

    def counted(*a, **k):
        y = orig(*a, **k)
        ran.append(y is not None)
        return y
    monkeypatch.setattr(G, name, counted)
    outs = []
    for gen in _pair(model, 16 if B <= 16 else 64):
        cache = KVCache(cfg.num_layers, B, 64, 8, 128, torch.bfloat16, DEV)
        g = torch.Generator(device=DEV).manual_seed(5)
        for L in range(cfg.num_layers):
            cache.k[L].normal_(generator=g)
            cache.v[L].normal_(generator=g)
        nxt = torch.randint(0, 1024, (B,), device=DEV, generator=g)
        cur = (torch.arange(B, device=DEV) * 11 + 3) % 64
        with torch.no_grad():
            lg = gen._decode_step(nxt, cur, cache)
        outs.append([lg] + [c.clone() for c in cache.k + cache.v])
    # every layer GEMM and the LM head ran the kernel (None: a LayerNorm prologue over > 4 rows)
    assert sum(ran) == 4 * cfg.num_layers + 1
    for a, b in zip(*outs):
        assert _rel(a, b) < 2e-2


def test_mx4_greedy_generation_requantize_and_draft(small_model):
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    cfg, model = small_model
    model = copy.deepcopy(model)  # a weight is changed below
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 1024, (3, 11), device=DEV, generator=g)
    lens = torch.tensor([11, 4, 8], device=DEV)
    conf = {"decode_strategy": "greedy_search", "max_dec_len": 12, "eos_token_id": None,
            "pad_token_id": 0}
    # a 16-bit target drafted on its mxfp4 copies emits the plain greedy ids
    plain = GPTForGeneration(model, conf).generate(prompt, lens)[0]
    spec = GPTForGeneration(model, dict(conf, spec_draft="mxfp4", spec_tokens=3))
    assert torch.equal(spec.generate(prompt, lens)[0], plain)
    assert spec.last_spec_stats["drafted"] > 0
    # the mxfp4 target: graph replay equals eager, and requantize() follows a weight change
    gens = [GPTForGeneration(model, dict(conf, weight_quant="mxfp4", use_hip_graph=graph))
            for graph in (True, False)]
    ids = [gen.generate(prompt, lens)[0] for gen in gens]
    assert ids[0].shape == (3, 12) and torch.equal(ids[0], ids[1])
    with torch.no_grad():
        model.gpt.layers[1].mlp.fc1.weight.mul_(-1.5)
    assert gens[1].requantize() is True
    fresh = GPTForGeneration(model, dict(conf, weight_quant="mxfp4", use_hip_graph=False))
    changed = gens[1].generate(prompt, lens)[0]
    assert torch.equal(changed, fresh.generate(prompt, lens)[0])
    assert not torch.equal(changed, ids[1])
