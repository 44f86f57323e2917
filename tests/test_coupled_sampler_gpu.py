"""The coupled sampler's kernels on the GPU: ``coupled_sample_kernel`` against
float64 keys from ``rng.coupled_noise``, ``select_kernel`` mode 2 and the
coupled ``spec_pick_kernel`` against ``coupled_sample`` on torch-processed
logits, and all three under HIP-graph replay with changed indices and seed."""
import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.parallel import rng
from tests import device_loop_cases as DC
from tests import spec_verify_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
VOCABS = (257, 1000, 4133)        # fewer elements than threads, a partial stride, five strides
SETTINGS = [(1.0, 0, 1.0), (0.8, 20, 0.9), (1.0, 50, 0.75)]
SEED = 90210


def _seed(v=SEED):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# ------------------------------------------------- coupled_sample against keys
@pytest.mark.parametrize("tkp", SETTINGS)
@pytest.mark.parametrize("V", VOCABS)
def test_coupled_sample_against_float64_keys(V, tkp):
    """The pick is in ``fused_sample``'s kept set (same threshold phases on the
    same logits) and its float64 key is within 2^-18 max(1, max |key|) of the
    best kept key: 32 fp32 ulps of the largest key, a key being two rounded
    logf, one product and one sum.  Eight (step, row) pairs per row of logits."""
    temp, top_k, top_p = tkp
    g = torch.Generator(device=DEV).manual_seed(V)
    logits = 2.5 * torch.randn(B, V, device=DEV, generator=g)
    _, lse_ref, probs = ops.fused_sample(logits, temp, top_k, top_p, return_probs=True)
    kept = probs > 0
    if top_k:
        assert int(kept.sum(1).max()) <= top_k
    out, worst = 0, 0.0
    for rep in range(8):
        steps = torch.tensor([rep, 3 * rep + 1, 1000 + rep], dtype=torch.int32, device=DEV)
        rows = torch.tensor([0, rep % 3, 15 - rep], dtype=torch.int32, device=DEV)
        ids, lse = ops.coupled_sample(logits, temp, top_k, top_p, _seed(), steps, rows)
        noise = rng.coupled_noise(SEED, steps, rows, V, device=DEV, dtype=torch.float64)
        keys = logits.double() / temp + noise
        keys = torch.where(kept, keys, torch.full_like(keys, float("-inf")))
        assert bool(kept.gather(1, ids[:, None]).all())
        best = keys.max(1).values
        short = best - keys.gather(1, ids[:, None]).squeeze(1)
        bound = 2.0 ** -18 * keys[kept].abs().max().clamp(min=1.0)
        out += int((short > bound).sum())
        worst = max(worst, float(short.max()))
        assert torch.equal(lse, lse_ref)                  # the same softmax_stats
    print("V %d %r: worst shortfall %.3g, rows out of bound %d" % (V, tkp, worst, out))
    assert out == 0


def test_rows_default_to_the_row_index_and_the_int_seed_is_wrapped():
    logits = torch.randn(B, 1000, device=DEV)
    steps = torch.tensor([4, 4, 4], dtype=torch.int32, device=DEV)
    a, _ = ops.coupled_sample(logits, 0.8, 20, 0.9, _seed(), steps)
    b, _ = ops.coupled_sample(logits, 0.8, 20, 0.9, SEED, steps, torch.arange(B))
    assert torch.equal(a, b)
    c, _, keys = ops.coupled_sample(logits, 0.8, 20, 0.9, SEED, steps, return_keys=True)
    assert torch.equal(a, c) and keys.shape == logits.shape
    top = torch.topk(keys, 2, dim=-1).values
    if bool((top[:, 0] - top[:, 1] > 1e-3).all()):        # the formula agrees off a near tie
        assert torch.equal(keys.argmax(-1), a)
    d, _ = ops.coupled_sample(logits.cpu(), 0.8, 20, 0.9, SEED, steps.cpu())
    if bool((top[:, 0] - top[:, 1] > 1e-3).all()):
        assert torch.equal(d, a.cpu())


# ------------------------------------------------------- select_token, mode 2
def _couple(st, tkp, seed):
    """Turn a built greedy state into a coupled one (the shared ``build`` has
    no seed argument); temperature, top-k and top-p are already the case's."""
    st.greedy, st.coupled, st.seed = False, True, seed
    assert (st.temperature, st.top_k, st.top_p) == tkp


@pytest.mark.parametrize("tkp", SETTINGS)
@pytest.mark.parametrize("name", sorted(DC.CASES))
@pytest.mark.parametrize("V", VOCABS)
def test_select_token_mode_2(V, name, tkp):
    """``coupled_sample`` on the torch-processed logits and ``select_token`` on
    the raw ones pick the same tokens under the same (seed, step, row); the
    bookkeeping is the host loop's."""
    logits, hist, st, c = DC.build(name, V, B, DEV, sample=tkp)
    _couple(st, tkp, _seed())
    x = DC.torch_processed(logits, hist, c)
    steps = torch.full((B,), c["step"], dtype=torch.int32, device=DEV)
    pick, _ = ops.coupled_sample(x, tkp[0], tkp[1], tkp[2], _seed(), steps)
    before, keep = DC.snapshot(st), logits.clone()
    ops.select_token(logits, st)
    assert torch.equal(logits, keep)
    tok = DC.check_step(st, before, x, pick, hist, c, V)
    if name == "min_len_before":
        assert DC.EOS not in tok.tolist()
    if name == "forced_bos":
        assert tok.tolist() == [DC.BOS] * B
    if name == "forced_eos":
        assert tok.tolist() == [DC.EOS] * B
    if name == "finished_row":
        assert tok[1] == DC.PAD and st.finish_len[1] == 2 and st.unfinished[1] == 0


# ------------------------------------------------------- spec_verify, coupled
SPEC_CASES = [n for n in SC.CASES if n != "tie"]          # "tie" plants two equal greedy maxima


class FeedPicks:
    """While active, the CPU formula's race returns keys whose argmax is the
    given pick of the slot (call ``j`` is slot ``j``): the formula's
    bookkeeping runs on the GPU's picks."""

    def __init__(self, picks):
        self.picks, self.j = picks.cpu().long(), 0

    def __enter__(self):
        self._saved = ops.sampling.coupled_keys

        def fed(x, *a, **k):
            keys = torch.full_like(x, float("-inf"))
            keys.scatter_(1, self.picks[:, self.j:self.j + 1], 0.0)
            self.j += 1
            return keys
        ops.sampling.coupled_keys = fed
        return self

    def __exit__(self, *exc):
        ops.sampling.coupled_keys = self._saved


@pytest.mark.parametrize("scale", [1.0, 0.2], ids=["planted", "damped"])
@pytest.mark.parametrize("tkp", SETTINGS)
@pytest.mark.parametrize("name", SPEC_CASES)
@pytest.mark.parametrize("V,W", [(257, 2), (1000, 5), (4133, 8)])
def test_spec_verify_coupled(V, W, name, tkp, scale):
    """``picks`` bitwise equal to one ``coupled_sample`` per slot on the
    torch-processed slot logits (history plus d_1 .. d_j, token index step + j),
    ``logp`` within 1e-6 of it, and the full state equal to the CPU formula fed
    the GPU's picks.  ``damped`` scales the logits by 0.2, which brings the
    cases' planted logits down to the noise, so that acceptance varies."""
    logits, hist, cpu, conf = SC.build(name, V, B, W)
    _, _, st, _ = SC.build(name, V, B, W, DEV)
    logits = logits * scale
    for s in (cpu, st):
        s.temperature, s.top_k, s.top_p = tkp
        s.greedy, s.coupled = False, True
    cpu.seed, st.seed = _seed().cpu(), _seed()
    before = SC.snapshot(st)
    dlogits = logits.to(DEV)
    keep = dlogits.clone()
    ops.spec_verify(dlogits, st)
    got = SC.snapshot(st)
    assert torch.equal(dlogits, keep)
    # ---- one coupled_sample per slot
    active = (before["unfinished"] != 0) & (before["step"] < SC.N_STEPS)
    d = before["tok"].view(B, W)[:, 1:]
    rows = torch.arange(B, dtype=torch.int32, device=DEV)
    for j in range(W):
        x = torch.stack([SC._processed(
            dlogits[b * W + j],
            torch.cat([hist[b], torch.tensor([t for t in d[b, :j].tolist() if 0 <= t < V],
                                             dtype=torch.long)]).to(DEV),
            conf, int(before["step"][b]) + j) for b in range(B)])
        pick, lse = ops.coupled_sample(x, tkp[0], tkp[1], tkp[2], _seed(),
                                       before["step"].to(DEV) + j, rows)
        lp = x.gather(1, pick[:, None]).squeeze(1) - lse
        assert torch.equal(got["picks"][active, j].long(), pick.cpu()[active]), j
        assert bool(((got["logp"][:, j] - lp.cpu()).abs() <= 1e-6)[active].all()), j
    # ---- the bookkeeping: the CPU formula on the GPU's picks
    with FeedPicks(got["picks"]) as fp:
        ops.spec_verify(logits, cpu)
    assert fp.j == W
    want = SC.snapshot(cpu)
    for k in SC.INT_STATE:
        assert torch.equal(got[k], want[k]), k
    emitted = want["step"] - before["step"]
    # per emitted token the bound on fused_sample's lse, 1e-4 + 1e-5 |lse|, with |lse| < 60
    err = (got["scores"] - want["scores"]).abs()
    assert bool((err <= emitted * 7e-4).all())
    assert torch.equal(got["scores"][~active], before["scores"][~active])
    n = got["accepted"] - before["accepted"]
    print(name, "accepted", n.tolist(), "emitted", emitted.tolist())
    assert bool(((n >= 0) & (n <= W - 1)).all())
    if name == "finished_row":
        assert emitted[1] == 0 and got["finish_len"][1] == 2


# ----------------------------------------------------------------- graph replay
def test_graph_replay_follows_step_and_seed():
    """A captured ``coupled_sample``, ``select_token`` mode 2 and coupled
    ``spec_verify`` read the indices and the seed from device memory: after
    they change, a replay gives the new indices' picks."""
    V, W = 1000, 5
    tkp = (0.8, 20, 0.9)
    logits = 2.5 * torch.randn(B, V, device=DEV)
    steps = torch.zeros(B, dtype=torch.int32, device=DEV)
    rows = torch.arange(B, dtype=torch.int32, device=DEV)
    seed = _seed(1)
    out = torch.zeros(B, dtype=torch.long, device=DEV)
    _, hist, st, c = DC.build("penalty", V, B, DEV, sample=tkp)
    _couple(st, tkp, seed)
    wl, _, sp, conf = SC.build("none_accepted", V, B, W, DEV)
    wl = wl * 0.2
    sp.temperature, sp.top_k, sp.top_p = tkp
    sp.greedy, sp.coupled, sp.seed = False, True, seed
    sp0 = {k: v.to(DEV) for k, v in SC.snapshot(sp).items()}

    def body():
        out.copy_(ops.coupled_sample(logits, *tkp, seed, steps, rows)[0])
        ops.select_token(logits, st)
        ops.spec_verify(wl, sp)

    body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    seen = []
    for new_seed, new_step in ((1, 2), (77, 2), (77, 5)):
        seed.fill_(new_seed)
        steps.fill_(new_step)
        st.step.fill_(new_step)
        for k in SC.ALL_STATE:                             # the round starts over at new_step
            getattr(sp, k).copy_(sp0[k])
        sp.step.fill_(new_step)
        x = ops.sampling.processed_logits(logits, st)
        want_sel, _ = ops.coupled_sample(x, *tkp, _seed(new_seed), steps.clone(), rows)
        want, _ = ops.coupled_sample(logits, *tkp, _seed(new_seed), steps.clone(), rows)
        x0 = ops.sampling.processed_logits(wl.view(B, W, V)[:, 0], sp)
        want_slot0, _ = ops.coupled_sample(x0, *tkp, _seed(new_seed), steps.clone(), rows)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert torch.equal(st.out[:, new_step], want_sel)
        assert torch.equal(sp.picks[:, 0].long(), want_slot0)
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) or not torch.equal(seen[1], seen[2])
