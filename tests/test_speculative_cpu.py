"""Speculative greedy decoding, the parts that need no GPU: the round logic of
``GPTForGeneration._speculative`` on an fp32 model with the formula attention
and drafters injected through ``set_drafter``, against the plain greedy loop."""
import os
import warnings

import pytest
import torch

from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G

V, GAMMA, MAXPOS = 97, 4, 64


def _model():
    torch.manual_seed(2)
    cfg = GPTConfig(vocab_size=V, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=MAXPOS, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    m = GPTForPretraining(cfg).eval()
    # the default init decodes into one repeated token; wider matrices give varied text
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    return m


def _prompts(S=9, lens=(9, 5, 7)):
    g = torch.Generator().manual_seed(3)
    return torch.randint(4, V, (len(lens), S), generator=g), torch.tensor(lens)


class RandomDrafter:
    def __init__(self, seed=0):
        self.g = torch.Generator().manual_seed(seed)
        self.calls = 0

    def propose(self, last, cur, cache, k):
        self.calls += 1
        return torch.randint(0, V, (last.shape[0], k), generator=self.g)


class ReplayDrafter:
    """Proposes the tokens of a known continuation ``ids`` [B, T] (token i of a
    row sits at position ``lens + i``); zeros past its end."""

    def __init__(self, ids, lens):
        self.ids, self.lens = ids, lens

    def propose(self, last, cur, cache, k):
        B, T = self.ids.shape
        i = (cur - self.lens)[:, None] + 1 + torch.arange(k)[None, :]
        return torch.where(i < T, self.ids.gather(1, i.clamp(max=T - 1)), torch.zeros_like(i))


BASE = {"decode_strategy": "greedy_search", "max_dec_len": 14, "pad_token_id": 0}
CASES = {
    "plain": {},
    "penalty": {"repetition_penalty": 1.3},
    "min_len_eos": {"min_dec_len": 5, "eos_token_id": None},     # eos filled in below
    "forced_bos": {"forced_bos_token_id": 11},
    "forced_eos": {"forced_eos_token_id": 12, "eos_token_id": 12},
}


def _cfg(name, m, ids, lens):
    c = dict(BASE, **CASES[name])
    if name == "min_len_eos":
        # an EOS the unconstrained run emits early: min length must push it back
        free, _ = G.GPTForGeneration(m, dict(BASE)).generate(ids, lens)
        c["eos_token_id"] = int(free[0, 1])
    return c


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("drafter", ["random", "perfect"])
def test_speculative_equals_plain_greedy(name, drafter):
    m = _model()
    ids, lens = _prompts()
    c = _cfg(name, m, ids, lens)
    want, want_scores = G.GPTForGeneration(m, c).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA))
    gen.set_drafter(RandomDrafter(7) if drafter == "random" else ReplayDrafter(want, lens))
    got, scores = gen.generate(ids, lens)
    assert torch.equal(got, want)
    assert torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    st = gen.last_spec_stats
    assert st["rounds"] >= 1 and st["drafted"] == GAMMA * ids.shape[0] * st["rounds"]
    if name == "min_len_eos":
        assert (want[:, :5] != c["eos_token_id"]).all()
    if drafter == "perfect" and name == "plain":
        T = want.shape[1]
        assert st["rounds"] == -(-(T - 1) // (GAMMA + 1))


def test_speculative_stops_at_eos_inside_a_window():
    """EOS = a token the eos-free output holds mid-sequence: the row is cut
    after its first occurrence and padded, also when the EOS sits inside an
    accepted window (the perfect draft accepts whole windows)."""
    m = _model()
    ids, lens = _prompts()
    free, _ = G.GPTForGeneration(m, dict(BASE)).generate(ids, lens)
    # the (row, token) whose first occurrence is latest: past slot 0 of the first window
    firsts = [(r.tolist().index(t), b, t) for b, r in enumerate(free) for t in set(r.tolist())]
    k, b, eos = max(firsts)
    assert k >= 2
    c = dict(BASE, eos_token_id=eos, pad_token_id=0)
    want, want_scores = G.GPTForGeneration(m, c).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA))
    gen.set_drafter(ReplayDrafter(free, lens))
    got, scores = gen.generate(ids, lens)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    row = free[b].tolist()
    assert got[b].tolist() == (row[:k + 1] + [0] * len(row))[:got.shape[1]]


@pytest.mark.parametrize("drafter", ["random", "perfect"])
def test_speculative_end_of_position_range(drafter):
    """A prompt that ends GAMMA - 1 positions short of max_position_embeddings:
    the window reaches past the range, its slots there are never emitted."""
    m = _model()
    S = MAXPOS - (GAMMA - 1)
    ids, lens = _prompts(S, (S, S - 6, S - 2))
    want, want_scores = G.GPTForGeneration(m, dict(BASE)).generate(ids, lens)
    assert want.shape[1] == GAMMA - 1
    gen = G.GPTForGeneration(m, dict(BASE, spec_tokens=GAMMA))
    gen.set_drafter(RandomDrafter(1) if drafter == "random" else ReplayDrafter(want, lens))
    got, scores = gen.generate(ids, lens)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)


def test_constructor_errors():
    m = _model()
    ok = {"decode_strategy": "greedy_search", "spec_draft": "int4_g256"}
    G.GPTForGeneration(m, ok)
    for bad in ({"decode_strategy": "sampling"},
                {"decode_strategy": "beam_search", "num_beams": 2},
                {"device_loop": True},
                {"num_return_sequences": 2},
                {"weight_quant": "int4_g256"},
                {"spec_draft": "int3"},
                {"spec_tokens": 0},
                {"spec_tokens": 8}):
        with pytest.raises(ValueError):
            G.GPTForGeneration(m, dict(ok, **bad))
    # defaults: off, gamma 4
    gen = G.GPTForGeneration(m, {"decode_strategy": "greedy_search"})
    assert gen.spec_draft is None and gen.spec_tokens == 4
    with pytest.raises(ValueError):
        G.GPTForGeneration(m, {"decode_strategy": "sampling"}).set_drafter(RandomDrafter())


def test_spec_draft_on_cpu_without_drafter_warns_once_and_runs_plain():
    m = _model()
    ids, lens = _prompts()
    want, _ = G.GPTForGeneration(m, dict(BASE)).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(BASE, spec_draft="int8"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, _ = gen.generate(ids, lens)
        b, _ = gen.generate(ids, lens)
    assert torch.equal(a, want) and torch.equal(b, want)
    assert len([r for r in rec if "speculative" in str(r.message)]) == 1
    assert gen.last_spec_stats is None


def test_too_many_window_rows_warn_once_and_run_plain():
    m = _model()
    ids, lens = _prompts()                                  # B = 3: 3 * 8 rows > 16
    want, _ = G.GPTForGeneration(m, dict(BASE)).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(BASE, spec_tokens=7))
    d = RandomDrafter()
    gen.set_drafter(d)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, _ = gen.generate(ids, lens)
        gen.generate(ids, lens)
    assert torch.equal(a, want) and d.calls == 0
    assert len([r for r in rec if "speculative" in str(r.message)]) == 1


def test_speculative_config_file_loads_with_the_keys_set():
    from fleetx_amd.utils import config as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt",
                     "generation_gpt_345M_speculative.yaml"),
        overrides=["Global.device=cpu"], nranks=1)
    g = cfg["Generation"]
    assert g["spec_draft"] == "int4_g256" and g["spec_tokens"] == 4
    assert g["decode_strategy"] == "greedy_search"
    G.GPTForGeneration(_model(), dict(g))
