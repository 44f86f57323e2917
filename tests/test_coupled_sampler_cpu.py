"""The coupled sampler, the parts that need no GPU: the noise hash against a
plain-Python evaluation, the distribution and the coupling of the formula
(``ops.coupled_sample`` on CPU tensors), and speculative decoding under
sampling (``sampler: coupled``) against the plain coupled loop on the fp32
model, prompts and drafters of ``test_speculative_cpu``."""
import math
import os

import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G
from fleetx_amd.parallel import rng
from tests.test_speculative_cpu import GAMMA, RandomDrafter, ReplayDrafter, _model, _prompts

M64 = (1 << 64) - 1
N_DRAWS = 20000


# ------------------------------------------------------------------ the hash
def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _lb32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _h(seed, t, b, i):
    key = _mix64(_mix64((seed + 0x9E3779B97F4A7C15) & M64) ^ ((t << 32) | b))
    return _lb32(_lb32(i ^ (key & 0xFFFFFFFF)) ^ (key >> 32))


def test_noise_matches_a_plain_python_hash():
    V = 300
    for seed, t, b in ((0, 0, 0), (1, 0, 0), (1234567890123, 7, 2), (2 ** 63 + 5, 255, 15),
                       (-3, 1, 1)):
        h = rng.coupled_hash(seed, t, b, V)
        g = rng.coupled_noise(seed, t, b, V)
        g64 = rng.coupled_noise(seed, t, b, V, dtype=torch.float64)
        assert h.shape == (1, V)
        for i in (0, 1, 31, 32, 257, V - 1):
            want = _h(seed & M64, t, b, i)
            assert int(h[0, i]) == want
            u = ((want >> 9) + 0.5) * 2.0 ** -23
            ref = -math.log(-math.log(u))
            assert abs(float(g64[0, i]) - ref) <= 1e-12 * max(1.0, abs(ref))
            assert abs(float(g[0, i]) - ref) <= 1e-5 * max(1.0, abs(ref))
    # a tensor seed and tensor indices give the rows of the scalar calls
    hs = rng.coupled_hash(torch.tensor([77]), torch.tensor([3, 4]), torch.tensor([0, 1]), V)
    assert torch.equal(hs[0], rng.coupled_hash(77, 3, 0, V)[0])
    assert torch.equal(hs[1], rng.coupled_hash(77, 4, 1, V)[0])
    assert not torch.equal(hs[0], hs[1])


def test_uniform_stays_inside_the_open_interval():
    h = torch.tensor([0, 2 ** 32 - 1, 511, 512], dtype=torch.int64)
    u = rng.coupled_uniform(h)
    assert u.dtype == torch.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert float(u[0]) == 2.0 ** -24 and float(u[1]) == 1.0 - 2.0 ** -24   # exact in fp32
    g = -torch.log(-torch.log(u))
    assert torch.isfinite(g).all() and -2.9 < float(g.min()) and float(g.max()) < 16.7


# ---------------------------------------------------------- the distribution
P8 = torch.tensor([0.30, 0.22, 0.15, 0.12, 0.09, 0.06, 0.04, 0.02])


@pytest.mark.parametrize("name,top_k,top_p,kept", [
    ("full", 0, 1.0, range(8)),
    ("top_k_3", 3, 1.0, range(3)),
    ("top_p_0.6", 0, 0.6, range(3)),      # 0.30 + 0.22 <= 0.6 < 0.30 + 0.22 + 0.15
])
def test_draws_follow_the_filtered_distribution(name, top_k, top_p, kept):
    """20 000 rows under one seed: every token's frequency within 4 binomial
    standard deviations of its filtered probability, none outside the kept set."""
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])                  # not sorted by index
    p = P8[perm]
    logits = torch.log(p)[None, :].repeat(N_DRAWS, 1)
    ids, lse = ops.coupled_sample(logits, 1.0, top_k, top_p, 20261, torch.zeros(N_DRAWS),
                                  torch.arange(N_DRAWS))
    keep = torch.zeros(8, dtype=torch.bool)
    keep[[int((perm == k).nonzero()) for k in kept]] = True
    q = torch.where(keep, p, torch.zeros_like(p))
    q = q / q.sum()
    freq = torch.bincount(ids, minlength=8).double() / N_DRAWS
    sd = torch.sqrt(q * (1 - q) / N_DRAWS).double()
    print(name, "z", ((freq - q) / sd.clamp(min=1e-12)).tolist())
    assert bool((freq[~keep] == 0).all())
    assert bool(((freq - q).abs() <= 4 * sd)[keep].all())
    assert torch.allclose(lse, torch.zeros(N_DRAWS), atol=1e-6)


def test_token_indices_and_rows_draw_independently():
    """Steps in place of rows give another 20 000 draws of the same law, and the
    two differ (the noise depends on t and on b)."""
    logits = torch.log(P8)[None, :].repeat(N_DRAWS, 1)
    a, _ = ops.coupled_sample(logits, 1.0, 0, 1.0, 9, torch.arange(N_DRAWS), torch.zeros(N_DRAWS))
    b, _ = ops.coupled_sample(logits, 1.0, 0, 1.0, 9, torch.zeros(N_DRAWS), torch.arange(N_DRAWS))
    for ids in (a, b):
        freq = torch.bincount(ids, minlength=8).double() / N_DRAWS
        assert bool(((freq - P8).abs() <= 4 * torch.sqrt(P8 * (1 - P8) / N_DRAWS)).all())
    same = (a == b).double().mean().item()
    indep = float((P8 * P8).sum())
    assert abs(same - indep) <= 4 * math.sqrt(indep * (1 - indep) / N_DRAWS)


def test_shared_noise_couples_two_distributions():
    """P and Q = P's logits + 0.2 randn over V = 50: the draws with shared noise
    agree at least (1 - TV) / (1 + TV) of the time, the coupling's guarantee;
    0.02 covers four standard deviations of the estimate (one is at most
    sqrt(0.25 / 20000) = 0.0035)."""
    g = torch.Generator().manual_seed(4)
    V = 50
    lp = 2.5 * torch.randn(V, generator=g)
    lq = lp + 0.2 * torch.randn(V, generator=g)
    tv = 0.5 * (torch.softmax(lp, -1) - torch.softmax(lq, -1)).abs().sum().item()
    steps, rows = torch.zeros(N_DRAWS), torch.arange(N_DRAWS)
    a, _ = ops.coupled_sample(lp[None].repeat(N_DRAWS, 1), 1.0, 0, 1.0, 31, steps, rows)
    b, _ = ops.coupled_sample(lq[None].repeat(N_DRAWS, 1), 1.0, 0, 1.0, 31, steps, rows)
    agree = (a == b).double().mean().item()
    print("TV %.4f, 1 - TV %.4f, bound %.4f, agreement %.4f"
          % (tv, 1 - tv, (1 - tv) / (1 + tv), agree))
    assert agree >= (1 - tv) / (1 + tv) - 0.02
    assert agree <= 1 - tv + 0.02                                   # no coupling beats 1 - TV


# ---------------------------------------------------------------- the states
def test_state_constructors_choose_the_pick():
    ids, lens = torch.zeros(2, 4, dtype=torch.long), torch.tensor([4, 4])
    st = ops.SelectState(ids, lens, 100, 8, greedy=False, seed=5)
    assert st.coupled and not st.greedy and st.seed.dtype == torch.int64 and st.seed.item() == 5
    u = torch.rand(8, 2)
    st = ops.SelectState(ids, lens, 100, 8, greedy=False, u=u, seed=5)       # u wins: inverse CDF
    assert not st.coupled and st.seed is None
    assert not ops.SelectState(ids, lens, 100, 8).coupled
    with pytest.raises(ValueError):
        ops.SelectState(ids, lens, 100, 8, greedy=False)
    assert ops.SpecState(ids, lens, 100, 8, 3).greedy
    sp = ops.SpecState(ids, lens, 100, 8, 3, greedy=False, seed=torch.tensor([9]))
    assert sp.coupled and sp.seed.item() == 9
    for kw in ({}, {"u": u}, {"u": u, "seed": 1}):
        with pytest.raises(ValueError):
            ops.SpecState(ids, lens, 100, 8, 3, greedy=False, **kw)
    with pytest.raises(ValueError):
        ops.coupled_sample(torch.zeros(2, 5), 1.0, 0, 1.0, 1, [0])
    with pytest.raises(ValueError):
        ops.coupled_sample(torch.zeros(2, 5), 1.0, 0, 1.0, torch.tensor([1.0]), [0, 0])


def test_select_token_and_spec_verify_take_the_coupled_pick():
    """The CPU formulas: ``select_token`` mode coupled picks ``coupled_sample``
    of the processed logits at ``(step, row)``; ``spec_verify`` slot ``j`` picks
    it at ``(step + j, row)`` and accepts the drafts that equal the picks."""
    V, B, W = 61, 3, 4
    g = torch.Generator().manual_seed(8)
    hist = torch.randint(0, V, (B, 6), generator=g)
    lens = torch.tensor([6, 6, 6])
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, penalty=1.3, greedy=False, seed=11)
    st = ops.SelectState(hist, lens, V, 9, **kw)
    st.step.fill_(2)
    lg = 2.0 * torch.randn(B, V, generator=g)
    x = ops.sampling.processed_logits(lg, st)
    want, _ = ops.coupled_sample(x, 0.8, 20, 0.9, 11, torch.full((B,), 2))
    assert torch.equal(ops.select_token(lg, st), want)
    sp = ops.SpecState(hist, lens, V, 9, W, **kw)
    sp.step.fill_(2)
    sp.cur.copy_(lens + 1)
    sp.start_window()
    wl = 2.0 * torch.randn(B * W, V, generator=g)
    # drafts: the true picks of slots 0 and 1, then a miss
    seen = ops.sampling.unpack_seen(sp.seen, V)
    picks = []
    for j in range(W):
        xj = ops.sampling.processed_logits(wl.view(B, W, V)[:, j], sp, sp.step.long() + j, seen)
        pj, _ = ops.coupled_sample(xj, 0.8, 20, 0.9, 11, torch.full((B,), 2 + j))
        picks.append(pj)
        if j < W - 1:
            d = pj if j < 2 else (pj + 1) % V
            sp.tok.view(B, W)[:, j + 1] = d
            seen = seen.clone()
            seen[torch.arange(B), d] = True
    ops.spec_verify(wl, sp)
    assert torch.equal(sp.picks.long(), torch.stack(picks, 1))
    assert sp.accepted.tolist() == [2] * B and sp.step.tolist() == [5] * B
    assert torch.equal(sp.out[:, 2:5], torch.stack(picks[:3], 1))


# ----------------------------------------------------- generation, end to end
T = 14
SAMPLING = {"decode_strategy": "sampling", "sampler": "coupled", "temperature": 0.8, "top_k": 20,
            "top_p": 0.9, "max_dec_len": T, "pad_token_id": 0}
SEED = 7
CASES = {
    "plain": {},
    "penalty": {"repetition_penalty": 1.3},
    "min_len_eos": {"min_dec_len": 5, "eos_token_id": None},     # eos filled in below
    "forced_eos": {"forced_eos_token_id": 12, "eos_token_id": 12},
}


class KeyGap:
    """While active, every ``ops.coupled_sample`` call also evaluates the
    formula's keys and asserts that the best two of each row are more than
    ``gap`` apart: the run it watches does not hinge on a rounding."""

    def __init__(self, gap=1e-3):
        self.gap, self.calls, self.least = gap, 0, float("inf")

    def __enter__(self):
        self._saved = ops.coupled_sample

        def watched(logits, *a, **k):
            ids, lse, keys = self._saved(logits, *a, **dict(k, return_keys=True))
            top = torch.topk(keys, 2, dim=-1).values
            self.least = min(self.least, float((top[:, 0] - top[:, 1]).min()))
            self.calls += 1
            assert self.least > self.gap, "top two keys %.3g apart" % self.least
            return ids, lse
        ops.coupled_sample = watched
        return self

    def __exit__(self, *exc):
        ops.coupled_sample = self._saved


def _reference(m, c, ids, lens, seed=SEED):
    """The plain coupled host loop under ``seed``, watched by ``KeyGap``."""
    with KeyGap() as kg:
        out = G.GPTForGeneration(m, c).generate(ids, lens, seed=seed)
    assert kg.calls >= 1
    return out


def _cfg(name, m, ids, lens):
    c = dict(SAMPLING, **CASES[name])
    if name == "min_len_eos":
        # an EOS the unconstrained run emits early: min length must push it back
        free, _ = G.GPTForGeneration(m, dict(SAMPLING)).generate(ids, lens, seed=SEED)
        c["eos_token_id"] = int(free[0, 1])
    return c


@pytest.fixture(scope="module")
def refs():
    """Per case: config, the watched reference run, and the same run GAMMA
    tokens longer (the perfect drafter's continuation past ``max_dec_len``)."""
    m = _model()
    ids, lens = _prompts()
    out = {}
    for name in CASES:
        c = _cfg(name, m, ids, lens)
        want, scores = _reference(m, c, ids, lens)
        longer, _ = G.GPTForGeneration(m, dict(c, max_dec_len=T + GAMMA)).generate(
            ids, lens, seed=SEED)
        out[name] = (c, want, scores, longer)
    return m, ids, lens, out


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("drafter", ["random", "perfect"])
def test_speculative_sampling_equals_the_plain_coupled_loop(refs, name, drafter, device_loop):
    """Ids equal and scores within 1e-4, whatever the drafter, in the host loop
    and with the verify formula of ``spec_device_loop``.  ``perfect`` replays
    the reference; where no row meets an EOS (the statistics count a finished
    row's drafts as drafted but never as accepted) and the continuation past
    ``max_dec_len`` is the longer run's, every draft is accepted and the run
    takes ceil((T - 1) / (GAMMA + 1)) rounds."""
    m, ids, lens, cases = refs
    c, want, want_scores, longer = cases[name]
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA, spec_device_loop=device_loop))
    no_eos = c.get("eos_token_id") is None
    replay = longer if no_eos else want
    if no_eos:
        assert torch.equal(longer[:, :T], want)
    gen.set_drafter(RandomDrafter(7) if drafter == "random" else ReplayDrafter(replay, lens))
    got, scores = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(got, want)
    assert torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    st = gen.last_spec_stats
    assert st["rounds"] >= 1 and st["drafted"] == GAMMA * ids.shape[0] * st["rounds"]
    if name == "min_len_eos":
        assert (want[:, :5] != c["eos_token_id"]).all()
    if name == "forced_eos":
        assert want.shape[1] == T and (want[:, -1][want[:, :-1].ne(12).all(1)] == 12).all()
    if drafter == "perfect" and no_eos:
        assert want.shape[1] == T
        assert st["accepted"] == st["drafted"]
        assert st["rounds"] == -(-(T - 1) // (GAMMA + 1))
    if drafter == "random":
        assert st["accepted"] < st["drafted"]


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
def test_speculative_sampling_stops_at_eos_inside_a_window(refs, device_loop):
    """EOS = a token the eos-free run holds mid-sequence: the row is cut after
    its first occurrence and padded, also inside an accepted window."""
    m, ids, lens, cases = refs
    c, free, _, _ = cases["plain"]
    firsts = [(r.tolist().index(t), b, t) for b, r in enumerate(free) for t in set(r.tolist())]
    k, b, eos = max(firsts)
    assert k >= 2
    c = dict(c, eos_token_id=eos)
    want, want_scores = _reference(m, c, ids, lens)
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA, spec_device_loop=device_loop))
    gen.set_drafter(ReplayDrafter(free, lens))
    got, scores = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    row = free[b].tolist()
    assert got[b].tolist() == (row[:k + 1] + [0] * len(row))[:got.shape[1]]


def test_host_and_device_speculative_loops_agree_on_statistics(refs):
    m, ids, lens, cases = refs
    c = cases["penalty"][0]
    runs = []
    for dl in (False, True):
        gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA, spec_device_loop=dl))
        gen.set_drafter(RandomDrafter(3))
        out = gen.generate(ids, lens, seed=SEED)
        runs.append((out, gen.last_spec_stats))
    assert torch.equal(runs[0][0][0], runs[1][0][0])
    assert runs[0][1] == runs[1][1]


def test_seeds_differ_and_an_unseeded_run_draws_its_seed_from_torch(refs):
    m, ids, lens, cases = refs
    c, want, _, _ = cases["plain"]
    gen = G.GPTForGeneration(m, c)
    other, _ = gen.generate(ids, lens, seed=SEED + 1)
    assert not torch.equal(other, want)
    torch.manual_seed(5)
    a, _ = gen.generate(ids, lens)
    b, _ = gen.generate(ids, lens)
    torch.manual_seed(5)
    a2, _ = gen.generate(ids, lens)
    assert torch.equal(a, a2) and not torch.equal(a, b)


class PickDrafter:
    """A drafter with ``propose_coupled``: drafts with ``pick`` on logits of its
    own (here noise), and counts how it was asked."""

    def __init__(self, V):
        self.V, self.plain, self.coupled, self.index = V, 0, 0, []
        self.g = torch.Generator().manual_seed(1)

    def propose(self, last, cur, cache, k):
        self.plain += 1
        return torch.zeros(last.shape[0], k, dtype=torch.long)

    def propose_coupled(self, last, cur, cache, k, pick):
        self.coupled += 1
        self.index.append(pick.step.clone())
        return torch.stack([pick(torch.randn(last.shape[0], self.V, generator=self.g), i)
                            for i in range(1, k + 1)], 1)


@pytest.mark.parametrize("device_loop", [False, True], ids=["host", "device"])
def test_propose_coupled_is_called_with_the_pick(refs, device_loop):
    m, ids, lens, cases = refs
    c, want, want_scores, _ = cases["plain"]
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA, spec_device_loop=device_loop))
    d = PickDrafter(want.max().item() + 1)
    gen.set_drafter(d)
    got, scores = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)
    assert d.coupled == gen.last_spec_stats["rounds"] and d.plain == 0
    assert d.index[0].tolist() == [1] * ids.shape[0]               # token 0 came from the prefill
    # under greedy search the same drafter is asked through propose
    gen = G.GPTForGeneration(m, {"decode_strategy": "greedy_search", "max_dec_len": T,
                                 "pad_token_id": 0, "spec_tokens": GAMMA})
    d = PickDrafter(5)
    gen.set_drafter(d)
    gen.generate(ids, lens)
    assert d.plain >= 1 and d.coupled == 0


def test_a_perfect_draft_model_is_always_accepted(refs):
    """A drafter that runs the target itself and draws with ``pick`` proposes
    exactly the target's tokens: the coupling accepts every draft of a draft
    model that equals the target."""
    m, ids, lens, cases = refs
    c, want, _, longer = cases["plain"]

    class SelfDrafter:
        def propose_coupled(self, last, cur, cache, k, pick):
            emitted = pick.step
            out = []
            hist = [torch.cat([ids[b, :lens[b]], longer[b, :emitted[b]]]) for b in range(len(lens))]
            for i in range(1, k + 1):
                col = []
                for b in range(len(lens)):
                    lg = m(hist[b][None])[0, -1][None]
                    # the noise row is b: pick one row at a time from a batch that holds it
                    full = lg.repeat(len(lens), 1)
                    col.append(pick(full, i)[b])
                col = torch.stack(col)
                out.append(col)
                hist = [torch.cat([h, t[None]]) for h, t in zip(hist, col)]
            return torch.stack(out, 1)

        def propose(self, *a):
            raise AssertionError("propose_coupled must be preferred")

    gen = G.GPTForGeneration(m, dict(c, spec_tokens=GAMMA))
    gen.set_drafter(SelfDrafter())
    with torch.no_grad():
        got, _ = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(got, want)
    st = gen.last_spec_stats
    assert st["accepted"] == st["drafted"] and st["rounds"] == -(-(T - 1) // (GAMMA + 1))


# ------------------------------------------------------------ the plain loops
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_loop_equals_host_loop_under_the_coupled_sampler(refs, name):
    m, ids, lens, cases = refs
    c, want, want_scores, _ = cases[name]
    got, scores = G.GPTForGeneration(m, dict(c, device_loop=True)).generate(ids, lens, seed=SEED)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)


def test_return_sequences_use_the_expanded_row_index(refs):
    m, ids, lens, cases = refs
    c, want, _, _ = cases["plain"]
    got, _ = G.GPTForGeneration(m, dict(c, num_return_sequences=2)).generate(ids, lens, seed=SEED)
    assert got.shape[0] == 2 * ids.shape[0]
    assert torch.equal(got[0], want[0])                            # row 0 keeps its index
    assert all(not torch.equal(got[2 * b], got[2 * b + 1]) for b in range(ids.shape[0]))


def test_sessions_draw_with_the_coupled_sampler(refs):
    m, ids, lens, cases = refs
    c, want, want_scores, _ = cases["plain"]
    gen = G.GPTForGeneration(m, c)
    s = gen.new_session(ids.shape[0])
    got, scores = gen.generate(ids, lens, seed=SEED, session=s)
    assert torch.equal(got, want) and torch.allclose(scores, want_scores, atol=1e-4, rtol=0)


def test_ignored_speculation_runs_the_plain_coupled_loop(refs):
    """24 window rows: one warning, and the seed gives the plain loop's text."""
    import warnings
    m, ids, lens, cases = refs
    c, want, _, _ = cases["plain"]
    gen = G.GPTForGeneration(m, dict(c, spec_tokens=7))
    d = RandomDrafter()
    gen.set_drafter(d)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, _ = gen.generate(ids, lens, seed=SEED)
        b, _ = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(a, want) and torch.equal(b, want) and d.calls == 0
    assert len([r for r in rec if "speculative" in str(r.message)]) == 1
    gen = G.GPTForGeneration(m, dict(c, spec_draft="int8"))        # CPU without a drafter
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        a, _ = gen.generate(ids, lens, seed=SEED)
    assert torch.equal(a, want) and gen.last_spec_stats is None


def test_the_default_sampler_is_untouched():
    """``sampler: inverse_cdf`` (the default) draws what torch.multinomial draws
    from the same generator, as before."""
    m = _model()
    ids, lens = _prompts()
    c = {k: v for k, v in SAMPLING.items() if k != "sampler"}
    a, _ = G.GPTForGeneration(m, c).generate(ids, lens, seed=3)
    b, _ = G.GPTForGeneration(m, dict(c, sampler="inverse_cdf")).generate(ids, lens, seed=3)
    coupled, _ = G.GPTForGeneration(m, dict(c, sampler="coupled")).generate(ids, lens, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, coupled)
    assert G.GPTForGeneration(m, c).sampler == "inverse_cdf"


# ---------------------------------------------------------------- constructor
def test_constructor_accepts_sampling_with_the_coupled_sampler_only():
    m = _model()
    spec = {"decode_strategy": "sampling", "spec_draft": "int4_g256"}
    for conf in (spec, dict(spec, sampler="inverse_cdf"),
                 {"decode_strategy": "sampling", "spec_device_loop": True}):
        with pytest.raises(ValueError):
            G.GPTForGeneration(m, conf)
    with pytest.raises(ValueError):
        G.GPTForGeneration(m, {"decode_strategy": "sampling"}).set_drafter(RandomDrafter())
    ok = dict(spec, sampler="coupled")
    G.GPTForGeneration(m, ok)
    G.GPTForGeneration(m, dict(ok, spec_device_loop=True))
    G.GPTForGeneration(m, {"decode_strategy": "sampling", "sampler": "coupled"}).set_drafter(
        RandomDrafter())
    for bad in ({"sampler": "gumbel"}, {"sampler": None},
                dict(ok, device_loop=True), dict(ok, num_return_sequences=2),
                {"decode_strategy": "beam_search", "num_beams": 2, "sampler": "coupled",
                 "spec_draft": "int8"}):
        with pytest.raises(ValueError):
            G.GPTForGeneration(m, bad)
    # a session still refuses speculation
    gen = G.GPTForGeneration(m, ok)
    ids, lens = _prompts()
    with pytest.raises(ValueError):
        gen.generate(ids, lens, session=gen.new_session(3))


def test_speculative_sampling_config_file_loads_with_the_keys_set():
    from fleetx_amd.utils import config as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt",
                     "generation_gpt_345M_speculative_sampling.yaml"),
        overrides=["Global.device=cpu"], nranks=1)
    g = cfg["Generation"]
    assert g["decode_strategy"] == "sampling" and g["sampler"] == "coupled"
    assert g["top_k"] == 50 and g["top_p"] == 0.75
    assert g["spec_draft"] == "int4_g256" and g["spec_device_loop"] is True
    gen = G.GPTForGeneration(_model(), dict(g))
    assert gen._coupled() and gen.spec_tokens == 4
