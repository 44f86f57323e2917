"""``Generation.weight_quant_prefill``: the prefill (one pass and chunked) on the
quantised copies against the unfused 16-bit path on the dequantised weights
(the model and the twin recipe of tests/test_decode_w8_gpu.py)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def small_model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return cfg, GPTForPretraining(cfg).cuda().eval()


def _pair(model, quant, extra):
    """(generator prefilling on the quantised copies, unfused generator on the
    dequantised weights with the dequantised head; the 16-bit table still
    serves both embedding lookups)."""
    from fleetx_amd import ops
    from fleetx_amd.models.language_model.gpt import generation as gmod
    a = gmod.GPTForGeneration(model, dict(extra, weight_quant=quant,
                                          weight_quant_prefill=True)).eval()
    assert a.requantize() is True
    qname = gmod._WEIGHT_QUANT[quant][0]
    quantise, dequantise = getattr(ops, qname), getattr(ops, "de" + qname)
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for layer in twin.gpt.layers:
            for lin in (layer.attn.qkv_proj, layer.attn.out_proj, layer.mlp.fc1, layer.mlp.fc2):
                lin.weight.copy_(dequantise(*quantise(lin.weight), lin.weight.dtype))
        table = twin.gpt.embeddings.word_embeddings.weight
        head = dequantise(*quantise(table), table.dtype)
    b = gmod.GPTForGeneration(twin, dict(extra, fused_decode=False)).eval()
    b._logits = lambda h, q8=None: torch.nn.functional.linear(h, head).float()
    return a, b


class _Count:
    """Counts the calls of ops.gemm.<name> that ran the kernel and the linears
    that fell back to their 16-bit weight (generation._ulin)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from fleetx_amd.models.language_model.gpt import generation as gmod
        from fleetx_amd.ops import gemm as G
        self.G, self.gmod = G, gmod
        self.orig, self.ulin, self.ran, self.fell = getattr(G, self.name), gmod._ulin, 0, 0

        def wrapped(*a, **k):
            y = self.orig(*a, **k)
            self.ran += y is not None
            return y

        def fell(*a, **k):
            self.fell += 1
            return self.ulin(*a, **k)
        setattr(G, self.name, wrapped)
        gmod._ulin = fell
        return self

    def __exit__(self, *exc):
        setattr(self.G, self.name, self.orig)
        self.gmod._ulin = self.ulin


@pytest.mark.parametrize("quant", ["int8", "int4_g256", "mxfp4"])
@pytest.mark.parametrize("chunk,S", [(0, 96), (64, 160)])
def test_quant_prefill_matches_dequantised_unfused(small_model, quant, chunk, S):
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = small_model
    B = 3
    g = torch.Generator(device=DEV).manual_seed(13)
    ids = torch.randint(0, 1024, (B, S), device=DEV, generator=g)
    lens = torch.tensor([S, 70, 33], device=DEV)
    a, b = _pair(model, quant, {"prefill_chunk": chunk})
    outs = []
    with _Count(gmod._WEIGHT_QUANT[quant][4]) as cnt:
        for gen in (a, b):
            cache = gmod.KVCache(cfg.num_layers, B, S, 8, 128, torch.bfloat16, DEV)
            with torch.no_grad():
                lg = gen._prompt_logits(ids, lens, cache, lens.int())
            outs.append((lg, cache.k + cache.v))
    passes = -(-S // chunk) if chunk else 1      # every pass has more than 64 rows (B * 32 = 96)
    assert cnt.ran == 4 * cfg.num_layers * passes and cnt.fell == 0
    assert outs[0][0].dtype == torch.float32 and outs[0][0].shape == (B, 1024)
    assert _rel(outs[0][0], outs[1][0]) < 2e-2
    for ca, cb in zip(outs[0][1], outs[1][1]):
        for r in range(B):
            n = int(lens[r])
            assert _rel(ca[r, :n], cb[r, :n]) < 2e-2


def test_quant_prefill_needs_weight_quant(small_model):
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    with pytest.raises(ValueError):
        GPTForGeneration(small_model[1], {"weight_quant_prefill": True})
