"""The vocabulary-split sampling kernels (``split=True``; sampling_split.inc)
against a float64 reference: kept set and probabilities, the inverse-CDF draw,
the coupled pick, and ``select_token`` against the one-workgroup kernel on the
device-loop cases, also under graph replay.

V 1000 is one partial slice, 2056 a second slice of 8 entries, 50304 is 25
slices with a tail."""
import pytest
import torch

from fleetx_amd import ops
from tests import device_loop_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCABS = (1000, 2056, 50304)
TKP = [(1.0, 1, 1.0), (0.7, 50, 0.75), (1.0, 64, 1.0), (1.0, 50, 1e-6)]
SEED = 4242
FIELDS = ("seen", "step", "unfinished", "finish_len", "out", "nxt", "cur", "scores")


def kept64(x, T, k, p):
    """Float64 reference of one row: the kept mask (``x >= x_(k)``, then the
    mass of the strictly larger survivors ``<= p``), the softmax of ``x / T``,
    and the least distance from ``p`` of a survivor's mass-above (a mass of
    exactly 0, nothing above, is kept in any arithmetic and does not count)."""
    x = x.double()
    pr = torch.softmax(x / T, -1)
    keep = x >= torch.topk(x, k).values[-1]
    idx = keep.nonzero().squeeze(1)
    xs, o = torch.sort(x[idx], descending=True, stable=True)
    c = torch.cumsum(pr[idx][o], 0) - pr[idx][o]
    above = c[torch.searchsorted(-xs, -xs)]           # of the first of each run of equals
    if p < 1.0:
        keep[idx[o][above > p]] = False
    far = (above - p).abs()[above > 0]
    return keep, pr, float(far.min()) if far.numel() else 1.0


def make_rows(variant, V, R, k):
    """fp32 logits [R, V] on the CPU: ``random``; ``ties``: values rounded
    through bf16 with the k-th largest planted again in another slice;
    ``masked``: -inf on the middle third (whole slices at V 50304);
    ``equal``: one value, so every slice overflows and the fallback runs."""
    g = torch.Generator().manual_seed(SEED + V + R)
    x = 3.0 * torch.randn(R, V, generator=g)
    if variant == "ties":
        x = x.bfloat16().float()
        top = torch.topk(x, k, -1)
        at = top.indices[:, -1]
        x[torch.arange(R), torch.where(at < V - 8, V - 3, 5)] = top.values[:, -1]
    if variant == "masked":
        x[:, V // 3:2 * V // 3] = float("-inf")
    if variant == "equal":
        x = torch.full((R, V), 1.5)
    return x


@pytest.mark.parametrize("tkp", TKP)
@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("variant,dtype", [("random", torch.float32), ("ties", torch.float32),
                                           ("ties", torch.bfloat16), ("masked", torch.float32),
                                           ("equal", torch.float32)])
def test_kept_set(variant, dtype, V, R, tkp):
    """``probs`` is nonzero exactly on the float64 kept set and within 1e-6
    (relative) of the float64 softmax there; ``lse`` within 1e-4 + 1e-5 |lse|.
    No token of these seeds lies within 1e-5 of ``top_p`` (asserted)."""
    T, k, p = tkp
    x = make_rows(variant, V, R, k).to(DEV)
    ids, lse, probs = ops.fused_sample(x.to(dtype), T, k, p, return_probs=True, split=True)
    torch.cuda.synchronize()
    for r in range(R):
        keep, pr, margin = kept64(x[r], T, k, p)
        assert margin > 1e-5
        assert torch.equal(probs[r] > 0, keep)
        assert bool(keep[ids[r]])
        rel = ((probs[r].double() - pr).abs() / pr)[keep].max().item()
        ref = torch.logsumexp(x[r].double(), -1)
        print("kept %d, p rel err %.3g, lse err %.3g" % (keep.sum(), rel, abs(lse[r] - ref)))
        assert rel <= 1e-6
        assert abs(lse[r].double() - ref) <= 1e-4 + 1e-5 * abs(ref)


def near_step(x, T, k, p, u):
    """Float64 inverse CDF in index order over the kept set of the row ``x``
    for the uniforms ``u`` [n]: the ids, and which ``u * Z`` lie within 1e-5
    of a CDF step."""
    keep, pr, _ = kept64(x, T, k, p)
    idx = keep.nonzero().squeeze(1)
    c = torch.cumsum(pr[idx], 0)
    target = u.double() * c[-1]
    ids = idx[torch.searchsorted(c, target, right=True).clamp(max=idx.numel() - 1)]
    return ids, ((target[:, None] - c[None, :]).abs() < 1e-5).any(1)


@pytest.mark.parametrize("tkp", TKP)
@pytest.mark.parametrize("V", VOCABS)
def test_draw_is_the_float64_inverse_cdf(V, tkp):
    """64 draws from one row with a seeded generator: each id is the float64
    inverse CDF of the same uniform; at most 1 row in 64 may sit on a step."""
    x = make_rows("random", V, 1, tkp[1]).to(DEV)
    g, g2 = [torch.Generator(device=DEV).manual_seed(SEED + V) for _ in range(2)]
    ids, _ = ops.fused_sample(x.expand(64, V).contiguous(), *tkp, generator=g, split=True)
    want, skip = near_step(x[0], *tkp, torch.rand(64, device=DEV, generator=g2))
    print("rows on a CDF step:", int(skip.sum()))
    assert int(skip.sum()) <= 1
    assert torch.equal(ids[~skip], want[~skip])


@pytest.mark.parametrize("tkp", TKP)
@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("V", VOCABS)
def test_coupled_pick(V, R, tkp):
    """The float64 key of the pick is within 2^-18 max(1, max |key|) of the
    best kept key of ``coupled_keys`` (the bound of test_coupled_sampler_gpu),
    and the pick is the one-workgroup kernel's: same kept set, same keys."""
    x = make_rows("random", V, R, tkp[1]).to(DEV)
    rws = torch.arange(R, dtype=torch.int32, device=DEV)
    for rep in range(4):
        steps = (rws * 7 + rep).to(torch.int32)
        ids, lse = ops.coupled_sample(x, *tkp, SEED, steps, rws, split=True)
        old, lse_old = ops.coupled_sample(x, *tkp, SEED, steps, rws)
        keys = ops.coupled_keys(x, *tkp, SEED, steps, rws, dtype=torch.float64)
        short = keys.max(1).values - keys.gather(1, ids[:, None]).squeeze(1)
        assert bool((short <= 2.0 ** -18 * keys[keys > float("-inf")].abs().max().clamp(min=1.0))
                    .all())
        assert torch.equal(ids, old)
        assert bool(((lse - lse_old).abs() <= 1e-4 + 1e-5 * lse_old.abs()).all())


# ------------------------------------------------------------- select_token
def _state(st):
    return {k: getattr(st, k).clone() for k in FIELDS}


def _same(a, b, rows, lse):
    """Two states equal on ``rows``; the scores, which accumulate ``lse``,
    within its bound 1e-4 + 1e-5 |lse| (the split statistics sum in another
    order, so the last bits of ``lse`` differ)."""
    for k in FIELDS[:-1]:
        assert torch.equal(a[k][rows], b[k][rows]), k
    err = (a["scores"] - b["scores"]).abs()
    print("score diff %.3g" % err.max())
    assert bool((err <= 1e-4 + 1e-5 * lse.abs())[rows].all())


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("tkp", [(0.7, 50, 0.75), (1.0, 64, 1.0)])
@pytest.mark.parametrize("name", sorted(DC.CASES))
@pytest.mark.parametrize("V,B", [(1000, 3), (2056, 1), (50304, 3)])
def test_select_token_matches_the_one_workgroup_kernel(V, B, name, tkp, mode):
    """``split=True`` and ``split=False`` leave the same ``SelectState``; in
    mode 1 a row whose ``u * Z`` sits within 1e-5 of a CDF step is exempt."""
    got = []
    for split in (False, True):
        g = torch.Generator(device=DEV).manual_seed(V + B)
        u = torch.rand(DC.N_STEPS, B, device=DEV, generator=g)
        logits, _, st, c = DC.build(name, V, B, DEV, greedy=mode == 2, sample=tkp,
                                    u=u if mode == 1 else None)
        if mode == 2:                                     # build() has no seed argument
            st.greedy, st.coupled, st.seed = False, True, ops.sampling.seed_tensor(SEED, DEV)
        x = ops.sampling.processed_logits(logits, st)
        ops.select_token(logits, st, split=split)
        got.append(_state(st))
    ok = torch.ones(B, dtype=torch.bool, device=DEV)
    if mode == 1:
        for r in range(B):
            ok[r] = not bool(near_step(x[r], *tkp, u[c["step"], r].view(1))[1])
    print("rows compared:", int(ok.sum()), "of", B)
    _same(got[0], got[1], ok, torch.logsumexp(x.double(), -1))


def test_graph_replay_follows_u_and_step():
    """A captured split selection (mode 1, then mode 2 on a second state)
    reads ``u``, ``step`` and the seed from device memory: two replays with
    changed inputs equal the eager split calls on the same inputs."""
    V, B, tkp = 2056, 3, (0.7, 50, 0.75)
    u = torch.rand(DC.N_STEPS, B, device=DEV)
    sts = []
    for _ in range(2):                                    # [graph, eager] x [mode 1, mode 2]
        logits, _, s1, _ = DC.build("penalty", V, B, DEV, greedy=False, sample=tkp, u=u.clone())
        _, _, s2, _ = DC.build("penalty", V, B, DEV, sample=tkp)
        s2.greedy, s2.coupled, s2.seed = False, True, ops.sampling.seed_tensor(SEED, DEV)
        sts.append((s1, s2))
    start = [_state(s) for s in sts[0]]

    def body(pair):
        for s in pair:
            ops.select_token(logits, s, split=True)

    body(sts[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body(sts[0])
    picks = []
    for step, seed in ((2, 5), (5, 6)):
        new_u = torch.rand(DC.N_STEPS, B, device=DEV)
        for pair in sts:
            for s, s0 in zip(pair, start):
                for k in FIELDS:
                    getattr(s, k).copy_(s0[k])
                s.step.fill_(step)
            pair[0].u.copy_(new_u)
            pair[1].seed.fill_(seed)
        graph.replay()
        body(sts[1])
        torch.cuda.synchronize()
        for a, b in zip(*sts):
            for k in FIELDS:
                assert torch.equal(getattr(a, k), getattr(b, k)), k
            assert bool((a.out[:, step] != DC.PAD).any())
        picks.append(torch.cat([s.nxt for s in sts[0]]))
    assert not torch.equal(picks[0], picks[1])


@pytest.mark.parametrize("device_loop", (False, True))
def test_generate_with_sampler_split(device_loop):
    """``sampler_split`` under the coupled sampler, host loop and graphed
    device loop: the split pick is the one-workgroup pick, so the ids are."""
    from fleetx_amd.models.language_model.gpt import generation as G
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=256, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = DC.varied(GPTForPretraining(cfg)).cuda().eval()
    prompt = torch.randint(4, 1024, (3, 9), device=DEV)
    conf = {"decode_strategy": "sampling", "sampler": "coupled", "top_k": 20, "top_p": 0.9,
            "temperature": 0.8, "max_dec_len": 12, "eos_token_id": None, "pad_token_id": 0,
            "device_loop": device_loop}
    off = G.GPTForGeneration(model, conf).generate(prompt, seed=3)
    with DC.Spy() as spy:
        on = G.GPTForGeneration(model, dict(conf, sampler_split=True)).generate(prompt, seed=3)
    assert spy.select_graph == (11 if device_loop else 0)
    assert on[0].shape == (3, 12) and torch.equal(on[0], off[0])
    assert torch.allclose(on[1], off[1], rtol=0, atol=12 * 2e-4)
