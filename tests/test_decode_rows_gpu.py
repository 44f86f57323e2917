"""``fused_decode_rows: 64``: decode steps of 17..64 rows run the fused layer on
the skinny GEMM (ops.gemm.decode_gemm*), in 16-bit, int8 and int4, and the
speculative loop engages at 20 rows."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return GPTForPretraining(cfg).cuda().eval()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _step(gen, B):
    """One decode step of ``B`` rows on a seeded cache: logits and the caches."""
    from fleetx_amd.models.language_model.gpt.generation import KVCache
    L = gen.gpt.cfg.num_layers
    cache = KVCache(L, B, 64, 8, 128, torch.bfloat16, DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    for li in range(L):
        cache.k[li].normal_(generator=g)
        cache.v[li].normal_(generator=g)
    nxt = torch.randint(0, 1024, (B,), device=DEV, generator=g)
    cur = (torch.arange(B, device=DEV) * 11 + 3) % 64
    with torch.no_grad():
        lg = gen._decode_step(nxt, cur, cache)
    return [lg] + list(cache.k) + list(cache.v)


def _unfused(model, quant):
    """The unfused generator; with ``quant`` on a copy whose four GEMM weights
    per layer and LM head hold dequantize(quantize(w)) as 16-bit weights (the
    16-bit table still serves the embedding lookup)."""
    from fleetx_amd import ops
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    if quant is None:
        return GPTForGeneration(model, {"fused_decode": False}).eval()
    q, dq = ((ops.quantize_weight_int8, ops.dequantize_weight_int8) if quant == "int8"
             else (ops.quantize_weight_int4, ops.dequantize_weight_int4))
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for layer in twin.gpt.layers:
            for lin in (layer.attn.qkv_proj, layer.attn.out_proj, layer.mlp.fc1, layer.mlp.fc2):
                lin.weight.copy_(dq(*q(lin.weight), lin.weight.dtype))
        table = twin.gpt.embeddings.word_embeddings.weight
        head = dq(*q(table), table.dtype)
    gen = GPTForGeneration(twin, {"fused_decode": False}).eval()
    gen._logits = lambda h, q8=None: torch.nn.functional.linear(h, head).float()
    return gen


@pytest.mark.parametrize("quant", [None, "int8", "int4_g256"])
@pytest.mark.parametrize("B", [20, 64])
def test_fused_step_above_16_rows_matches_unfused(model, B, quant):
    from fleetx_amd.models.language_model.gpt import generation as gmod
    want = _step(_unfused(model, quant), B)
    gen = gmod.GPTForGeneration(model, {"fused_decode_rows": 64, "weight_quant": quant}).eval()
    assert quant is None or gen.requantize() is True
    from fleetx_amd.ops import gemm as G
    calls, ran, orig = [], {}, gmod._layer_decode_fused
    gmod._layer_decode_fused = lambda *a: calls.append(orig(*a)) or calls[-1]
    names = ("decode_gemm", "decode_gemm_w8", "decode_gemm_w4")
    saved = {n: getattr(G, n) for n in names}

    def counted(n):
        def f(*a, **k):
            y = saved[n](*a, **k)
            ran[n] = ran.get(n, 0) + (y is not None)
            return y
        return f
    try:
        for n in names:
            setattr(G, n, counted(n))
        got = _step(gen, B)
    finally:
        gmod._layer_decode_fused = orig
        for n in names:
            setattr(G, n, saved[n])
    assert len(calls) == 3 and all(c is not None for c in calls)   # the fused layer ran
    # 13 GEMMs (four per layer and the LM head): a quantised step runs every one on
    # its own kernel and never lands on the 16-bit one; in 16-bit the launch table
    # may leave FFN2 to the vendor GEMM
    own = gmod._WEIGHT_QUANT[quant][3] if quant else "decode_gemm"
    assert (ran[own] == 13 if quant else 10 <= ran[own] <= 13), ran
    assert all(v == 0 for n, v in ran.items() if n != own), ran
    for a, b in zip(got, want):
        assert _rel(a, b) < 2e-2


def test_speculation_engages_at_20_rows(model):
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    conf = {"decode_strategy": "greedy_search", "max_dec_len": 16, "eos_token_id": None,
            "pad_token_id": 0, "fused_decode_rows": 64}
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 1024, (4, 11), device=DEV, generator=g)
    lens = torch.tensor([11, 4, 8, 6], device=DEV)
    plain, _ = GPTForGeneration(model, conf).generate(prompt, lens)
    gen = GPTForGeneration(model, dict(conf, spec_draft="int4_g256", spec_tokens=4))
    ids, _ = gen.generate(prompt, lens)
    st = gen.last_spec_stats
    assert st is not None and st["drafted"] == 4 * st["rounds"] * 4     # the window step ran
    assert torch.equal(ids, plain)
