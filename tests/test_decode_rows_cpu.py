"""``Generation.fused_decode_rows``: the values it takes, and the speculative
loop's row limit, which follows it."""
import warnings

import pytest
import torch

from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining

CONF = {"decode_strategy": "greedy_search", "spec_draft": "int4_g256", "spec_tokens": 7}


@pytest.fixture(scope="module")
def model():
    return GPTForPretraining(GPTConfig(vocab_size=64, hidden_size=32, num_layers=1,
                                       num_attention_heads=2, max_position_embeddings=32)).eval()


def test_key_values(model):
    assert GPTForGeneration(model, {}).fused_decode_rows == 16
    for ok in (16, 64):
        assert GPTForGeneration(model, {"fused_decode_rows": ok}).fused_decode_rows == ok
    for bad in (32, True, "64"):
        with pytest.raises(ValueError, match="fused_decode_rows"):
            GPTForGeneration(model, {"fused_decode_rows": bad})


@pytest.mark.parametrize("rows,refused", [(16, True), (64, False)])
def test_speculation_row_limit_follows_the_key(model, rows, refused):
    gen = GPTForGeneration(model, dict(CONF, fused_decode_rows=rows))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert gen._spec_drafter(3, torch.device("cpu")) is None    # 3 x 8 = 24 rows
    msg = str(rec[0].message)
    said = "batch * (spec_tokens + 1) = 24 rows exceed the 16 of the decode GEMV" in msg
    assert said == refused and ("rows exceed" in msg) == refused, msg
