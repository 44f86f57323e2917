"""On-device verify of speculative decoding, the parts that need no GPU: the
PyTorch formula branch of ``ops.spec_verify`` against a per-row Python
reference, and the round logic of ``GPTForGeneration._speculative_device``
(``spec_device_loop``) against the plain greedy loop, on the model, prompts,
drafters and processor cases of test_speculative_cpu.py."""
import warnings

import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G
from tests import spec_verify_cases as C
from tests import test_speculative_cpu as S

GAMMA = S.GAMMA


# ------------------------------------------------------------ ops.spec_verify
@pytest.mark.parametrize("name", C.CASES)
@pytest.mark.parametrize("B,W", [(1, 2), (3, 5), (2, 8)])
@pytest.mark.parametrize("V", [1000, 1057])
def test_formula_against_the_per_row_reference(V, B, W, name):
    logits, hist, st, conf = C.build(name, V, B, W)
    before, keep = C.snapshot(st), logits.clone()
    want, gain, bound, emitted = C.reference(logits, hist, before, conf, V, W)
    assert ops.spec_verify(logits, st) is None
    got = C.snapshot(st)
    assert torch.equal(logits, keep)
    for k in C.INT_STATE:
        assert torch.equal(got[k], want[k]), k
    err = (got["scores"] - before["scores"] - gain).abs()
    print("score err", err.max().item(), "bound", bound.tolist())
    assert bool((err <= bound).all())
    inactive = torch.tensor([not e for e in emitted])
    assert torch.equal(got["scores"][inactive], before["scores"][inactive])
    C.check(name, got, want, emitted, B, W, V)
    # the whole bitmap: history + emitted, no rejected draft
    unpacked = ops.sampling.unpack_seen(got["seen"], V)
    for b in range(B):
        assert set(unpacked[b].nonzero().flatten().tolist()) == \
            set(hist[b].tolist()) | set(emitted[b])
    # a call after every row finished changes nothing
    st.unfinished.zero_()
    st.any_active.zero_()
    done = C.snapshot(st)
    ops.spec_verify(logits, st)
    again = C.snapshot(st)
    for k in C.ALL_STATE:
        assert torch.equal(again[k], done[k]), k


def test_out_of_range_drafts_count_as_not_seen():
    logits, hist, st, conf = C.build("none_accepted", 1057, 2, 5)
    st.tok.view(2, 5)[0, 1:] = torch.tensor([-3, 1057, 2 ** 40, -2 ** 40])
    before = C.snapshot(st)
    want, _, _, emitted = C.reference(logits, hist, before, conf, 1057, 5)
    ops.spec_verify(logits, st)
    got = C.snapshot(st)
    for k in C.INT_STATE:
        assert torch.equal(got[k], want[k]), k


def test_state_and_shape_errors():
    logits, _, st, _ = C.build("all_accepted", 1000, 2, 5)
    with pytest.raises(ValueError):
        ops.spec_verify(logits[:-1], st)
    ids, lens = torch.zeros(2, 4, dtype=torch.long), torch.tensor([4, 4])
    for window in (0, 9):
        with pytest.raises(ValueError):
            ops.SpecState(ids, lens, 100, 8, window)
    with pytest.raises(ValueError):
        ops.SpecState(torch.zeros(65, 4, dtype=torch.long), torch.full((65,), 4), 100, 8, 2)


# ------------------------------------------------------------------ generate()
def _run(m, c, ids, lens, drafter, **kw):
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA, spec_device_loop=True, **kw))
    gen.set_drafter(drafter)
    got, scores = gen.generate(ids, lens)
    return got, scores, gen.last_spec_stats


@pytest.mark.parametrize("name", sorted(S.CASES))
@pytest.mark.parametrize("drafter", ["random", "perfect"])
def test_device_verify_equals_plain_greedy(name, drafter):
    m = S._model()
    ids, lens = S._prompts()
    c = S._cfg(name, m, ids, lens)
    want, want_scores = G.GPTForGeneration(m, c).generate(ids, lens)
    d = S.RandomDrafter(7) if drafter == "random" else S.ReplayDrafter(want, lens)
    got, scores, st = _run(m, c, ids, lens, d)
    assert torch.equal(got, want)
    assert torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    assert st["rounds"] >= 1 and st["drafted"] == GAMMA * ids.shape[0] * st["rounds"]
    assert 0 <= st["accepted"] <= st["drafted"]
    if name == "min_len_eos":
        assert (want[:, :5] != c["eos_token_id"]).all()
    if drafter == "perfect" and name == "plain":
        T = want.shape[1]
        assert st["rounds"] == -(-(T - 1) // (GAMMA + 1))
    # and the host speculative loop agrees on the statistics
    host = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA))
    host.set_drafter(S.RandomDrafter(7) if drafter == "random" else S.ReplayDrafter(want, lens))
    host.generate(ids, lens)
    assert host.last_spec_stats == st


def test_eos_inside_an_accepted_window():
    m = S._model()
    ids, lens = S._prompts()
    free, _ = G.GPTForGeneration(m, dict(S.BASE)).generate(ids, lens)
    firsts = [(r.tolist().index(t), b, t) for b, r in enumerate(free) for t in set(r.tolist())]
    k, b, eos = max(firsts)
    assert k >= 2
    c = dict(S.BASE, eos_token_id=eos, pad_token_id=0)
    want, want_scores = G.GPTForGeneration(m, c).generate(ids, lens)
    got, scores, _ = _run(m, c, ids, lens, S.ReplayDrafter(free, lens))
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    row = free[b].tolist()
    assert got[b].tolist() == (row[:k + 1] + [0] * len(row))[:got.shape[1]]


@pytest.mark.parametrize("drafter", ["random", "perfect"])
def test_end_of_position_range(drafter):
    m = S._model()
    n = S.MAXPOS - (GAMMA - 1)
    ids, lens = S._prompts(n, (n, n - 6, n - 2))
    want, want_scores = G.GPTForGeneration(m, dict(S.BASE)).generate(ids, lens)
    assert want.shape[1] == GAMMA - 1
    d = S.RandomDrafter(1) if drafter == "random" else S.ReplayDrafter(want, lens)
    got, scores, _ = _run(m, dict(S.BASE), ids, lens, d)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)


def test_poll_interval_does_not_change_the_output():
    m = S._model()
    ids, lens = S._prompts()
    c = S._cfg("min_len_eos", m, ids, lens)
    a = _run(m, c, ids, lens, S.RandomDrafter(7), spec_poll=1)
    b = _run(m, c, ids, lens, S.RandomDrafter(7), spec_poll=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_constructor_errors():
    m = S._model()
    ok = {"decode_strategy": "greedy_search", "spec_device_loop": True}
    gen = G.GPTForGeneration(m, ok)
    assert gen.spec_device_loop and gen.spec_poll == 1
    for bad in ({"decode_strategy": "sampling"}, {"device_loop": True},
                {"num_return_sequences": 2}):
        with pytest.raises(ValueError):
            G.GPTForGeneration(m, dict(ok, **bad))
    off = G.GPTForGeneration(m, {"decode_strategy": "sampling"})
    assert off.spec_device_loop is False


def test_without_a_drafter_the_plain_loop_runs():
    m = S._model()
    ids, lens = S._prompts()
    want, want_scores = G.GPTForGeneration(m, dict(S.BASE)).generate(ids, lens)
    gen = G.GPTForGeneration(m, dict(S.BASE, spec_device_loop=True))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, scores = gen.generate(ids, lens)
    assert torch.equal(got, want) and torch.equal(scores, want_scores)
    assert gen.last_spec_stats is None


def test_config_file_loads_with_the_keys_set():
    import os
    from fleetx_amd.utils import config as Cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Cfg.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt",
                     "generation_gpt_345M_speculative_device_loop.yaml"),
        overrides=["Global.device=cpu"], nranks=1)
    g = cfg["Generation"]
    assert g["spec_device_loop"] is True and g["spec_draft"] == "int4_g256"
    assert g["decode_strategy"] == "greedy_search"
    G.GPTForGeneration(S._model(), dict(g))
