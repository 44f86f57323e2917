"""``Generation.prefill_act_quant`` and ``ops.quantize_rows_int8``, the parts
that need no GPU: the key's checks, the CPU formula on planted rows, and that a
CPU run ignores the key under ``weight_quant``'s one warning."""
import warnings

import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G

ON = {"weight_quant": "int8", "weight_quant_prefill": True, "prefill_act_quant": "int8"}


def _model():
    torch.manual_seed(2)
    cfg = GPTConfig(vocab_size=97, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=64, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    return GPTForPretraining(cfg).eval()


@pytest.mark.parametrize("conf", [dict(ON, prefill_act_quant="fp8"), dict(ON, prefill_act_quant=True),
                                  dict(ON, weight_quant="mxfp4"),
                                  {"weight_quant": "int8", "prefill_act_quant": "int8"}])
def test_prefill_act_quant_rejected(conf):
    with pytest.raises(ValueError, match="prefill_act_quant"):
        G.GPTForGeneration(_model(), conf)
    assert G.GPTForGeneration(_model(), {}).prefill_act_quant is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_rows_cpu_formula(dtype):
    """sx = 2^-3 with elements on the ties 0.5 / 1.5 / 2.5 sx (to even), an
    all-zero row, a row whose largest element is negative."""
    x = torch.zeros(3, 16)
    x[0, :7] = torch.tensor([15.875, .0625, .1875, .3125, -.0625, -.1875, -.3125])
    x[2, :3] = torch.tensor([1.0, -4.0, 2.0])
    q, s = ops.quantize_rows_int8(x.to(dtype))
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert torch.equal(s, torch.tensor([0.125, 1.0, 4.0]) / torch.tensor([1.0, 1.0, 127.0]))
    assert q[0, :7].tolist() == [127, 0, 2, 2, 0, -2, -2] and not q[1].any()
    assert q[2, :3].tolist() == [32, -127, 64]


def test_prefill_act_quant_is_ignored_on_cpu_with_the_one_warning():
    m = _model()
    ids = torch.randint(0, 97, (3, 9), generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([9, 4, 6])
    cfg = {"decode_strategy": "greedy_search", "max_dec_len": 8, "eos_token_id": None}
    ref, ref_scores = G.GPTForGeneration(m, cfg).generate(ids, lens)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out, scores = G.GPTForGeneration(m, dict(cfg, **ON)).generate(ids, lens)
    assert len([r for r in rec if "weight_quant" in str(r.message)]) == 1
    assert torch.equal(out, ref) and torch.equal(scores, ref_scores)
