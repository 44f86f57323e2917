"""Weight-only int4 decode with group scales (csrc/kernels/decode_gemv_w4.hip,
ops.gemm.decode_linear_w4, ``weight_quant: int4_g256``): an exact layout test
on integer data, real-valued numerics against the dequantised formula, the
LayerNorm prologue, the fused decode step (greedy and beam) and greedy
generation.  The twin of test_decode_w8_gpu.py."""
import copy

import pytest
import torch

from tests.gemv_w4_cases import _int4_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


# ----------------------------------------------------------------------------
# 1. exact layout test: integer data and power-of-two group scales, every
#    partial sum exact in fp32 in any order (tests/gemv_w4_cases.py), so the
#    output must equal the float64 result rounded once.  Shapes: ragged N with
#    8 columns per block and one chunk per wave (4 waves); 8 waves with one and
#    two chunks; 16 columns per block with four chunks; three and five chunks
#    (an odd count ends on the single-batch tail); eight chunks (the steady
#    loop body runs three times).
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(3, 1001, 1024), (16, 96, 2048), (2, 2000, 4096),
                                   (1, 4096, 4096), (1, 2064, 3072), (1, 2064, 5120),
                                   (1, 2064, 8192)])
def test_w4_exact_bias_and_residual(dtype, M, N, K):
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    x, q, scale, b, res, ref = _int4_case(M, N, K, M + N + K)
    xd, bd, rd = x.to(DEV, dtype), b.to(DEV, dtype), res.to(DEV, dtype)
    pd, sd = ops.pack_int4(q).to(DEV), scale.to(DEV)
    y = G.decode_linear_w4(xd, pd, sd, bd, G.GV_BIAS)
    assert y is not None and y.dtype == dtype and y.shape == (M, N)
    assert torch.equal(y.cpu(), ref.to(dtype))
    y = G.decode_linear_w4(xd, pd, sd, bd, G.GV_RES, res=rd)
    assert y is not None
    assert torch.equal(y.cpu(), (ref + res).to(dtype))
    # no bias: the scaled group sums alone
    y = G.decode_linear_w4(xd, pd, sd)
    assert torch.equal(y.cpu(), (ref - b).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(3, 1024), (16, 2048), (1, 4096)])
@pytest.mark.parametrize("H,D", [(5, 64), (3, 128)])
def test_w4_exact_qkv_scatter(dtype, M, K, H, D):
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    N, L = 3 * H * D, 24
    x, q, scale, b, _, ref = _int4_case(M, N, K, M + K + D)
    kc = torch.zeros(M, L, H, D, device=DEV, dtype=dtype)
    vc = torch.zeros_like(kc)
    pos = ((torch.arange(M) * 7 + 3) % L).to(DEV)          # distinct for M <= 16 (7 coprime to 24)
    assert pos.unique().numel() == M
    out = G.decode_linear_w4(x.to(DEV, dtype), ops.pack_int4(q).to(DEV), scale.to(DEV),
                             b.to(DEV, dtype), G.GV_QKV, qkv_cache=(kc, vc, pos))
    assert out is not None and out.shape == (M, H * D)
    r = ref.to(dtype).view(M, H, 3, D)
    ar = torch.arange(M, device=DEV)
    assert torch.equal(out.view(M, H, D).cpu(), r[:, :, 0])
    assert torch.equal(kc[ar, pos].cpu(), r[:, :, 1])
    assert torch.equal(vc[ar, pos].cpu(), r[:, :, 2])
    mask = torch.ones(M, L, dtype=torch.bool, device=DEV)
    mask[ar, pos] = False
    assert kc[mask].abs().max().item() == 0 and vc[mask].abs().max().item() == 0


# ----------------------------------------------------------------------------
# 2. real-valued numerics (the recipe, shapes and tolerances of
#    test_decode_w8_gpu.py::test_w8_epilogues; the kernel rounds in the same
#    places: exact integer conversion, fp32 scale and accumulation, one
#    rounding at the store)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (3, 1000, 1024), (16, 12288, 2048),
                                   (16, 50304, 1024), (2, 96, 1024)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_w4_epilogues(dtype, M, N, K, epi):
    from fleetx_amd import ops
    from fleetx_amd.ops import gemm as G
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + epi)
    x = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=DEV, generator=g).to(dtype)
    res = torch.randn(M, N, device=DEV, generator=g).to(dtype) if epi == G.GV_RES else None
    p, scale = ops.quantize_weight_int4(w)
    y = G.decode_linear_w4(x, p, scale, b, epi, res=res)
    assert y is not None
    ref = x.float() @ ops.dequantize_weight_int4(p, scale).t() + b.float()
    if epi == G.GV_GELU:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if epi == G.GV_RES:
        ref = ref + res.float()
    tol = 8e-3 if dtype == torch.bfloat16 else 2e-3
    err = _rel(y, ref)
    print("rel err %.3g" % err)
    assert err < tol


def test_w4_uncovered_calls_return_none():
    from fleetx_amd.ops import gemm as G
    bf = dict(device=DEV, dtype=torch.bfloat16)
    p = torch.zeros(64, 768, device=DEV, dtype=torch.uint8)
    x = torch.zeros(2, 1536, **bf)
    assert G.decode_linear_w4(x, p, torch.ones(6, 64, device=DEV)) is None   # K % 1024 != 0
    p = torch.zeros(64, 512, device=DEV, dtype=torch.uint8)
    s = torch.ones(4, 64, device=DEV)
    assert G.decode_linear_w4(torch.zeros(2, 1024, **bf), p, s) is not None  # the covered twin
    assert G.decode_linear_w4(torch.zeros(17, 1024, **bf), p, s) is None     # M = 17
    assert G.decode_linear_w4(torch.zeros(2, 1024, device=DEV), p, s) is None      # fp32 x
    assert G.decode_linear_w4(torch.zeros(2, 1024, **bf), p.to(torch.int8), s) is None  # not uint8
    assert G.decode_linear_w4(torch.zeros(2, 1024, **bf), p, torch.ones(64, 4, device=DEV)) is None
    assert G.decode_linear_w4(torch.zeros(2, 1024, **bf), p, torch.ones(64, device=DEV)) is None


# ----------------------------------------------------------------------------
# 3. LayerNorm prologue (the cases of test_w8_fused_layernorm with M <= 4, one
#    with M > 4 that is not covered, and the large-LDS opt-in boundary)
# ----------------------------------------------------------------------------
_LN_CASES = [(1, 8192, 2048), (1, 6144, 2048), (1, 12288, 4096), (3, 1000, 1024), (4, 3072, 2048),
             (4, 4096, 4096), (5, 3072, 2048)]


def _ln_case(M, N, K, seed):
    from fleetx_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (3.0 + torch.randn(M, K, device=DEV, generator=g)).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, device=DEV, generator=g).bfloat16()
    lw = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).bfloat16()
    lb = (0.1 * torch.randn(K, device=DEV, generator=g)).bfloat16()
    p, scale = ops.quantize_weight_int4(w)
    xn = torch.nn.functional.layer_norm(x.float(), (K,), lw.float(), lb.float(), 1e-5)
    ref = xn.bfloat16().float() @ ops.dequantize_weight_int4(p, scale).t() + b.float()
    return x, p, scale, b, lw, lb, ref


@pytest.mark.parametrize("M,N,K", _LN_CASES)
@pytest.mark.parametrize("epi", [1, 3])
def test_w4_fused_layernorm(M, N, K, epi):
    from fleetx_amd.ops import gemm as G
    if epi == G.GV_QKV and N % 192:
        N = 960  # QKV needs N = 3 * heads * 64
    x, p, scale, b, lw, lb, ref = _ln_case(M, N, K, M + N + K + epi)
    H, D, L = N // 192, 64, 8
    kc = torch.zeros(M, L, H, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    pos = torch.arange(M, device=DEV) % L
    kw = dict(qkv_cache=(kc, vc, pos)) if epi == G.GV_QKV else {}
    y = G.decode_linear_w4(x, p, scale, b, epi, ln=(lw, lb, 1e-5), **kw)
    if M > 4:  # more than 4 rows take the LayerNorm kernel: the caller falls back
        assert y is None
        assert kc.abs().max().item() == 0
        return
    assert y is not None
    if epi == G.GV_GELU:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
        assert _rel(y, ref) < 8e-3, _rel(y, ref)
    else:
        r = ref.view(M, H, 3, D)
        ar = torch.arange(M, device=DEV)
        assert _rel(y.view(M, H, D), r[:, :, 0]) < 8e-3
        assert _rel(kc[ar, pos], r[:, :, 1]) < 8e-3
        assert _rel(vc[ar, pos], r[:, :, 2]) < 8e-3


def test_w4_fused_layernorm_lds_opt_in_boundary():
    """M = 3, K = 10240: the normalised rows take 61488 B of dynamic LDS, under
    64 KiB alone but over it with the kernel's static 8192 B, so the launch
    needs the large-LDS opt-in (recipe and bound of test_w4_fused_layernorm)."""
    from fleetx_amd.ops import gemm as G
    M, N, K = 3, 96, 10240
    assert M * (K + 8) * 2 <= 65536 < M * (K + 8) * 2 + 8192
    x, p, scale, b, lw, lb, ref = _ln_case(M, N, K, M + N + K + G.GV_GELU)
    ref = torch.nn.functional.gelu(ref, approximate="tanh")
    y = G.decode_linear_w4(x, p, scale, b, G.GV_GELU, ln=(lw, lb, 1e-5))
    assert y is not None
    assert _rel(y, ref) < 8e-3, _rel(y, ref)   # .item() inside waits for the kernel


# ----------------------------------------------------------------------------
# 4 / 5. the decode step and greedy generation with weight_quant: int4_g256
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return cfg, GPTForPretraining(cfg).cuda().eval()


def _dequantised_twin(model):
    """A copy of ``model`` whose four GEMV weights per layer hold
    dequantize(quantize(w)) in the model dtype, and the dequantised LM head."""
    from fleetx_amd import ops
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for layer in twin.gpt.layers:
            for lin in (layer.attn.qkv_proj, layer.attn.out_proj, layer.mlp.fc1, layer.mlp.fc2):
                p, s = ops.quantize_weight_int4(lin.weight)
                lin.weight.copy_(ops.dequantize_weight_int4(p, s, lin.weight.dtype))
        table = twin.gpt.embeddings.word_embeddings.weight
        head = ops.dequantize_weight_int4(*ops.quantize_weight_int4(table), table.dtype)
    return twin, head


def _pair(model, extra=None):
    """(int4 fused generator, unfused generator on the dequantised weights; the
    16-bit table still serves its embedding lookup, the dequantised one its head)."""
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    a = GPTForGeneration(model, dict(extra or {}, weight_quant="int4_g256")).eval()
    assert a.requantize() is True
    twin, head = _dequantised_twin(model)
    b = GPTForGeneration(twin, dict(extra or {}, fused_decode=False)).eval()
    b._logits = lambda h, q8=None: torch.nn.functional.linear(h, head).float()
    return a, b


class _CountW4:
    """Counts the calls of decode_linear_w4 that ran the int4 kernel."""

    def __enter__(self):
        from fleetx_amd.ops import gemm as G
        self.G, self.orig, self.ran = G, G.decode_linear_w4, 0

        def wrapped(*a, **k):
            y = self.orig(*a, **k)
            self.ran += y is not None
            return y
        G.decode_linear_w4 = wrapped
        return self

    def __exit__(self, *exc):
        self.G.decode_linear_w4 = self.orig


def test_w4_fused_decode_step_matches_dequantised_unfused(small_model):
    from fleetx_amd.models.language_model.gpt.generation import KVCache
    cfg, model = small_model
    B = 6
    outs = []
    with _CountW4() as cnt:
        for gen in _pair(model):
            cache = KVCache(cfg.num_layers, B, 64, 8, 128, torch.bfloat16, DEV)
            g = torch.Generator(device=DEV).manual_seed(5)
            for L in range(cfg.num_layers):
                cache.k[L].normal_(generator=g)
                cache.v[L].normal_(generator=g)
            nxt = torch.randint(0, 1024, (B,), device=DEV, generator=g)
            cur = torch.tensor([3, 10, 0, 63, 20, 41], device=DEV)
            with torch.no_grad():
                lg = gen._decode_step(nxt, cur, cache)
            outs.append((lg, [c.clone() for c in cache.k], [c.clone() for c in cache.v]))
    assert cnt.ran == 4 * cfg.num_layers + 1  # four GEMVs in every layer and the LM head
    assert _rel(outs[0][0], outs[1][0]) < 2e-2
    for a, b in zip(outs[0][1] + outs[0][2], outs[1][1] + outs[1][2]):
        assert _rel(a, b) < 2e-2


def test_w4_beam_decode_step_matches_dequantised_unfused(small_model):
    from fleetx_amd.models.language_model.gpt.generation import BeamKVCache
    cfg, model = small_model
    B, nb, S, Gn, t = 2, 3, 12, 6, 2
    outs = []
    with _CountW4() as cnt:
        for gen in _pair(model, {"decode_strategy": "beam_search", "num_beams": nb}):
            cache = BeamKVCache(cfg.num_layers, B, nb, S, Gn, 8, 128, torch.bfloat16, DEV)
            g = torch.Generator(device=DEV).manual_seed(9)
            for L in range(cfg.num_layers):
                cache.k[L].normal_(generator=g)
                cache.v[L].normal_(generator=g)
                cache.kg[L][:, :t].normal_(generator=g)
                cache.vg[L][:, :t].normal_(generator=g)
            cache.plens.copy_(torch.tensor([12, 7]))
            anc = torch.randint(0, nb, (B * nb, Gn), device=DEV, generator=g).int()
            anc[:, t] = cache._self.repeat(B)
            cache.anc.copy_(anc)
            slot = torch.full((B * nb,), t, dtype=torch.long, device=DEV)
            glens = torch.full((B,), t + 1, dtype=torch.int32, device=DEV)
            nxt = torch.randint(0, 1024, (B * nb,), device=DEV, generator=g)
            pos = cache.plens.long().repeat_interleave(nb) + t
            with torch.no_grad():
                lg = gen._beam_decode_step(nxt, pos, cache, slot, glens)
            outs.append((lg, [c[:, t].clone() for c in cache.kg],
                         [c[:, t].clone() for c in cache.vg]))
    assert cnt.ran == 4 * cfg.num_layers + 1
    assert outs[0][0].shape == (B * nb, 1024)
    assert _rel(outs[0][0], outs[1][0]) < 2e-2
    for a, b in zip(outs[0][1] + outs[0][2], outs[1][1] + outs[1][2]):
        assert _rel(a, b) < 2e-2


def _probe_logits(gen, cfg):
    """Logits of one decode step on a fixed cache state."""
    from fleetx_amd.models.language_model.gpt.generation import KVCache
    B = 2
    cache = KVCache(cfg.num_layers, B, 32, 8, 128, torch.bfloat16, DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    for L in range(cfg.num_layers):
        cache.k[L].normal_(generator=g)
        cache.v[L].normal_(generator=g)
    nxt = torch.randint(0, 1024, (B,), device=DEV, generator=g)
    with torch.no_grad():
        return gen._decode_step(nxt, torch.tensor([5, 17], device=DEV), cache).clone()


def test_w4_greedy_generation_and_requantize(small_model):
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    cfg, model = small_model
    model = copy.deepcopy(model)  # a weight is changed below
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 1024, (3, 11), device=DEV, generator=g)
    lens = torch.tensor([11, 4, 8], device=DEV)
    conf = {"decode_strategy": "greedy_search", "max_dec_len": 16, "eos_token_id": None,
            "weight_quant": "int4_g256"}
    gens = {graph: GPTForGeneration(model, dict(conf, use_hip_graph=graph)) for graph in (True, False)}
    with _CountW4() as cnt:
        ids_g, sc_g = gens[True].generate(prompt, lens)
        ran_graph = cnt.ran
        ids_e, sc_e = gens[False].generate(prompt, lens)
    assert ids_g.shape == (3, 16)
    per_step = 4 * cfg.num_layers + 1  # every decode GEMV of a step ran the int4 kernel
    assert ran_graph >= per_step and ran_graph % per_step == 0
    assert cnt.ran - ran_graph >= 15 * per_step and (cnt.ran - ran_graph) % per_step == 0
    assert torch.equal(ids_g, ids_e)
    assert torch.allclose(sc_g, sc_e, atol=1e-3, rtol=0)
    # an in-place change of one layer weight is picked up by the next generate()
    gen = gens[False]
    before = _probe_logits(gen, cfg)
    with torch.no_grad():
        model.gpt.layers[1].mlp.fc1.weight.mul_(1.5)
    assert torch.equal(_probe_logits(gen, cfg), before)  # int4 copies are refreshed by generate()
    gen.generate(prompt, lens)
    after = _probe_logits(gen, cfg)
    assert not torch.equal(after, before)
    fresh = GPTForGeneration(model, conf)
    assert fresh.requantize() is True
    assert torch.equal(after, _probe_logits(fresh, cfg))
