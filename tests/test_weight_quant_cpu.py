"""Weight-only int8 for decoding, the parts that need no GPU: the per-row
quantiser (ops.quantize_weight_int8) and the ``weight_quant`` generation key."""
import warnings

import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G


def _weight():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(1000, 1024, generator=g) * 1024 ** -0.5).bfloat16()
    w[17] = 0
    return w


def test_quantizer_range_and_scale():
    w = _weight()
    q, s = ops.quantize_weight_int8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and q.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (1000,)
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    nz = torch.ones(1000, dtype=torch.bool)
    nz[17] = False
    assert torch.equal(q[nz].abs().amax(1), torch.full((999,), 127, dtype=torch.int8))
    assert torch.equal(s[nz], w[nz].float().abs().amax(1) / 127)
    assert int(q[17].abs().max()) == 0 and float(s[17]) == 1.0


def test_quantizer_error_is_half_a_step():
    w = _weight()
    q, s = ops.quantize_weight_int8(w)
    err = (w.float() - q.float() * s[:, None]).abs() / s[:, None]
    print("worst |w - q*scale| / scale = %.6f" % float(err.max()))
    assert float(err.max()) <= 0.5001
    # the dequantiser is that formula, rounded once
    assert torch.equal(ops.dequantize_weight_int8(q, s, torch.float32), q.float() * s[:, None])
    assert torch.equal(ops.dequantize_weight_int8(q, s, torch.bfloat16),
                       (q.float() * s[:, None]).bfloat16())


def test_quantizer_takes_any_float_dtype():
    w = _weight()
    q, s = ops.quantize_weight_int8(w)
    for dt in (torch.float32, torch.float16):
        # bf16 -> fp32 is exact; fp16 rounds the values, so only the contract is checked
        q2, s2 = ops.quantize_weight_int8(w.to(dt))
        assert q2.dtype == torch.int8 and s2.dtype == torch.float32
        if dt == torch.float32:
            assert torch.equal(q2, q) and torch.equal(s2, s)


def _model():
    torch.manual_seed(2)
    cfg = GPTConfig(vocab_size=97, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=64, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    return GPTForPretraining(cfg).eval()


def test_weight_quant_rejects_unknown_value():
    m = _model()
    with pytest.raises(ValueError, match="weight_quant"):
        G.GPTForGeneration(m, {"weight_quant": "int4"})
    assert G.GPTForGeneration(m, {}).weight_quant is None
    assert G.GPTForGeneration(m, {"weight_quant": "int8"}).weight_quant == "int8"


def test_weight_quant_is_ignored_on_cpu_with_one_warning():
    m = _model()
    ids = torch.randint(0, 97, (3, 9), generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([9, 4, 6])
    cfg = {"decode_strategy": "greedy_search", "max_dec_len": 8, "eos_token_id": None}
    ref, ref_scores = G.GPTForGeneration(m, cfg).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(cfg, weight_quant="int8"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out, scores = gen.generate(ids, lens)
        out2, _ = gen.generate(ids, lens)
    assert len([r for r in rec if "weight_quant" in str(r.message)]) == 1
    assert torch.equal(out, ref) and torch.equal(out2, ref) and torch.equal(scores, ref_scores)
    assert gen.requantize() is False


def test_int8_config_file(tmp_path, monkeypatch):
    """The shipped int8 generation config builds a module that runs (on CPU the
    key is accepted and ignored)."""
    import os
    from tests.test_generation import _tiny_bpe
    from fleetx_amd.utils import config as C
    from fleetx_amd.models import build_module
    monkeypatch.setenv("FLEETX_TOKENIZER_DIR", str(_tiny_bpe(tmp_path / "tok")))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt", "generation_gpt_345M_int8.yaml"),
        overrides=["Model.hidden_size=64", "Model.num_layers=2", "Model.num_attention_heads=4",
                   "Model.max_position_embeddings=64", "Global.device=cpu",
                   "Model.vocab_size=264", "Generation.max_dec_len=5"], nranks=1)
    module = build_module(cfg)
    assert module.model.weight_quant == "int8" and module.model.decode_strategy == "sampling"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = module.generate("hello world")
    assert isinstance(out, list) and isinstance(out[0], str)
