"""``split=True`` and ``Generation.sampler_split`` off the GPU: CPU tensors
take the formula path, so nothing changes, and the key is validated."""
import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G
from tests import device_loop_cases as C
from tests.test_generation import _model

CFG = {"decode_strategy": "sampling", "top_k": 20, "top_p": 0.9, "temperature": 0.8,
       "max_dec_len": 10, "repetition_penalty": 1.3, "eos_token_id": None, "pad_token_id": 0}


@pytest.mark.parametrize("extra", [{}, {"device_loop": True}, {"sampler": "coupled"},
                                   {"sampler": "coupled", "device_loop": True}],
                         ids=["host", "device_loop", "coupled", "coupled_device_loop"])
def test_sampler_split_generates_the_same_tokens_on_cpu(extra):
    m = C.varied(_model(0))
    ids = torch.randint(4, 97, (3, 9), generator=torch.Generator().manual_seed(3))
    off = G.GPTForGeneration(m, dict(CFG, sampler_split=False, **extra)).generate(ids, seed=7)
    on = G.GPTForGeneration(m, dict(CFG, sampler_split=True, **extra)).generate(ids, seed=7)
    assert on[0].shape == (3, 10)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


@pytest.mark.parametrize("bad", [1, 0, "true", None])
def test_sampler_split_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="sampler_split"):
        G.GPTForGeneration(_model(0), dict(CFG, sampler_split=bad))


def test_split_on_cpu_tensors_takes_the_formula():
    lg = 3 * torch.randn(3, 257, generator=torch.Generator().manual_seed(1))
    a, b = [ops.fused_sample(lg, 0.8, 20, 0.9, generator=torch.Generator().manual_seed(2),
                             return_probs=True, split=s) for s in (False, True)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    steps = torch.tensor([0, 4, 9], dtype=torch.int32)
    a, b = [ops.coupled_sample(lg, 0.8, 20, 0.9, 11, steps, split=s) for s in (False, True)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    u = torch.rand(C.N_STEPS, 3, generator=torch.Generator().manual_seed(4))
    sts = []
    for s in (False, True):
        logits, _, st, _ = C.build("penalty", 257, 3, greedy=False, sample=(0.8, 20, 0.9), u=u)
        ops.select_token(logits, st, split=s)
        sts.append(st)
    assert torch.equal(sts[0].out, sts[1].out) and torch.equal(sts[0].scores, sts[1].scores)
