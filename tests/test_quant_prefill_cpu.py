"""``Generation.weight_quant_prefill``, the parts that need no GPU: the key's
checks and that a CPU run ignores it under ``weight_quant``'s one warning."""
import warnings

import pytest
import torch

from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G


def _model():
    torch.manual_seed(2)
    cfg = GPTConfig(vocab_size=97, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=64, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    return GPTForPretraining(cfg).eval()


@pytest.mark.parametrize("conf", [{"weight_quant_prefill": True},
                                  {"weight_quant": "int8", "weight_quant_prefill": "yes"}])
def test_weight_quant_prefill_rejected(conf):
    with pytest.raises(ValueError, match="weight_quant_prefill"):
        G.GPTForGeneration(_model(), conf)
    assert G.GPTForGeneration(_model(), {}).weight_quant_prefill is False


def test_weight_quant_prefill_is_ignored_on_cpu_with_the_one_warning():
    m = _model()
    ids = torch.randint(0, 97, (3, 9), generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([9, 4, 6])
    cfg = {"decode_strategy": "greedy_search", "max_dec_len": 8, "eos_token_id": None}
    ref, ref_scores = G.GPTForGeneration(m, cfg).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(cfg, weight_quant="int8", weight_quant_prefill=True))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out, scores = gen.generate(ids, lens)
    assert len([r for r in rec if "weight_quant" in str(r.message)]) == 1
    assert torch.equal(out, ref) and torch.equal(scores, ref_scores)
