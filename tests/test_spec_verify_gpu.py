"""On-device verify of speculative decoding on the GPU: ``spec_pick_kernel`` /
``spec_accept_kernel`` against the CPU formula of ``ops.spec_verify``, and
``Generation.spec_device_loop`` against the host speculative loop on the model
of test_speculative_gpu.py."""
import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G
from tests import spec_verify_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, GAMMA, B = 24, 4, 3
CONF = {"decode_strategy": "greedy_search", "max_dec_len": T, "eos_token_id": None,
        "pad_token_id": 0, "spec_tokens": GAMMA}


# -------------------------------------------------- kernels against the formula
@pytest.mark.parametrize("name", C.CASES)
@pytest.mark.parametrize("B,W", [(1, 2), (3, 5), (2, 8)])
@pytest.mark.parametrize("V", [1000, 1057, 50304])
def test_kernels_against_the_cpu_formula(V, B, W, name):
    logits, hist, cpu, conf = C.build(name, V, B, W)
    _, _, st, _ = C.build(name, V, B, W, DEV)
    before = C.snapshot(cpu)
    for k, v in C.snapshot(st).items():
        assert torch.equal(v, before[k]), k                # both start from the same state
    _, _, bound, emitted = C.reference(logits, hist, before, conf, V, W)
    ops.spec_verify(logits, cpu)
    want = C.snapshot(cpu)
    dlogits = logits.to(DEV)
    keep = dlogits.clone()
    ops.spec_verify(dlogits, st)
    got = C.snapshot(st)
    assert torch.equal(dlogits, keep)                      # read-only
    for k in C.INT_STATE:
        assert torch.equal(got[k], want[k]), k
    err = (got["scores"] - want["scores"]).abs()
    print("score err", err.max().item(), "bound", bound.tolist())
    assert bool((err <= bound).all())
    inactive = torch.tensor([not e for e in emitted])
    assert torch.equal(got["scores"][inactive], before["scores"][inactive])
    C.check(name, got, want, emitted, B, W, V)
    # a second call after every row finished changes nothing
    st.unfinished.zero_()
    st.any_active.zero_()
    done = C.snapshot(st)
    ops.spec_verify(dlogits, st)
    again = C.snapshot(st)
    for k in C.ALL_STATE:
        assert torch.equal(again[k], done[k]), k


def test_out_of_range_drafts_index_no_memory():
    logits, _, cpu, _ = C.build("none_accepted", 1057, 2, 5)
    _, _, st, _ = C.build("none_accepted", 1057, 2, 5, DEV)
    bad = torch.tensor([-3, 1057, 2 ** 40, -2 ** 40])
    cpu.tok.view(2, 5)[0, 1:] = bad
    st.tok.view(2, 5)[0, 1:] = bad.to(DEV)
    ops.spec_verify(logits, cpu)
    ops.spec_verify(logits.to(DEV), st)
    want, got = C.snapshot(cpu), C.snapshot(st)
    for k in C.INT_STATE:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------ generate()
class RandomDrafter:
    def __init__(self):
        self.g = torch.Generator(device=DEV).manual_seed(11)

    def propose(self, last, cur, cache, k):
        return torch.randint(0, 1024, (last.shape[0], k), device=DEV, generator=self.g)


class ReplayDrafter:
    """Proposes the tokens of a known continuation ``ids`` [B, n] (token i of a
    row sits at position ``lens + i``)."""

    def __init__(self, ids, lens):
        self.ids, self.lens = ids, lens

    def propose(self, last, cur, cache, k):
        n = self.ids.shape[1]
        i = (cur - self.lens)[:, None] + 1 + torch.arange(k, device=DEV)[None, :]
        return torch.where(i < n, self.ids.gather(1, i.clamp(max=n - 1)), torch.zeros_like(i))


class Spy:
    """Counts, while active, the calls that tell the device verify from the
    host speculative loop: ``ops.spec_verify`` (through ``generation``'s
    reference), the round graph, the host loop's ``_spec_process`` and its
    graphed window step."""

    def __enter__(self):
        self.verify = self.rounds = self.process = self.host_window = 0
        self._saved = (ops.spec_verify, G._GraphedSpecRound.__call__,
                       G.GPTForGeneration._spec_process, G._GraphedWindowStep.__call__)
        ver, rnd, proc, win = self._saved

        def spec_verify(*a, **k):
            self.verify += 1
            return ver(*a, **k)

        def round_graph(step, *a, **k):
            self.rounds += 1
            return rnd(step, *a, **k)

        def spec_process(gen, *a, **k):
            self.process += 1
            return proc(gen, *a, **k)

        def host_window(step, *a, **k):
            self.host_window += 1
            return win(step, *a, **k)
        ops.spec_verify = spec_verify
        G._GraphedSpecRound.__call__ = round_graph
        G.GPTForGeneration._spec_process = spec_process
        G._GraphedWindowStep.__call__ = host_window
        return self

    def __exit__(self, *exc):
        (ops.spec_verify, G._GraphedSpecRound.__call__, G.GPTForGeneration._spec_process,
         G._GraphedWindowStep.__call__) = self._saved


@pytest.fixture(scope="module")
def setup():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = GPTForPretraining(cfg).cuda().eval()
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 1024, (B, 11), device=DEV, generator=g)
    lens = torch.tensor([11, 4, 8], device=DEV)
    return model, prompt, lens


def _generate(setup, conf, drafter=None):
    model, prompt, lens = setup
    gen = G.GPTForGeneration(model, dict(CONF, **conf))
    if drafter is not None:
        gen.set_drafter(drafter)
    with Spy() as spy:
        ids, scores = gen.generate(prompt, lens)
    return ids, scores, gen.last_spec_stats, spy


def _same(a, b, n):
    """ids equal, scores within n * 2e-4 (under |lse| <= 10 per step), stats equal."""
    assert torch.equal(a[0], b[0])
    assert float(b[1].abs().max()) / n < 10               # the bound's premise
    print("score err", (a[1] - b[1]).abs().max().item(), "T", n)
    assert torch.allclose(a[1], b[1], rtol=0, atol=n * 2e-4)
    assert a[2] == b[2]


@pytest.fixture(scope="module")
def host_run(setup):
    return _generate(setup, {"spec_draft": "int4_g256"})


@pytest.fixture(scope="module")
def device_run(setup):
    return _generate(setup, {"spec_draft": "int4_g256", "spec_device_loop": True})


def test_device_loop_equals_the_host_loop(host_run, device_run):
    assert device_run[0].shape == (B, T)
    _same(device_run, host_run, T)


def _eos_of(free):
    firsts = [(r.tolist().index(t), b, t) for b, r in enumerate(free) for t in set(r.tolist())]
    k, _, eos = max(f for f in firsts if f[0] < T - 1)
    assert k >= 1
    return eos


@pytest.mark.parametrize("case", ["penalty", "min_len_eos", "forced_eos"])
def test_processor_runs_equal_the_host_loop(setup, host_run, case):
    conf = {"penalty": {"repetition_penalty": 1.3},
            "min_len_eos": {"min_dec_len": 5},
            "forced_eos": {"forced_eos_token_id": 12, "eos_token_id": 12}}[case]
    conf = dict(conf, spec_draft="int4_g256")
    if case == "min_len_eos":
        conf["eos_token_id"] = _eos_of(host_run[0])
    host = _generate(setup, conf)
    dev = _generate(setup, dict(conf, spec_device_loop=True))
    assert dev[3].verify > 0 and dev[3].process == 0
    _same(dev, host, host[0].shape[1])


def test_output_does_not_depend_on_the_drafter(setup, device_run):
    _, _, lens = setup
    ids, scores, st, _ = device_run
    assert st["drafted"] == GAMMA * st["rounds"] * B and 0 <= st["accepted"] <= st["drafted"]
    longer = _generate(setup, {"spec_draft": "int4_g256", "spec_device_loop": True,
                               "max_dec_len": T + GAMMA})[0]
    assert torch.equal(longer[:, :T], ids)
    dl = {"spec_device_loop": True}
    runs = {"int8": _generate(setup, dict(dl, spec_draft="int8")),
            "random": _generate(setup, dl, RandomDrafter()),
            "perfect": _generate(setup, dl, ReplayDrafter(longer, lens))}
    assert float(scores.abs().max()) / T < 10
    for name, (i2, s2, st2, spy) in runs.items():
        print(name, st2, "score err", (s2 - scores).abs().max().item())
        assert torch.equal(i2, ids), name
        assert torch.allclose(s2, scores, atol=T * 2e-4, rtol=0), name
        assert spy.verify > 0 and spy.process == 0 and spy.host_window == 0
    stp = runs["perfect"][2]
    assert stp["accepted"] == stp["drafted"]
    assert stp["rounds"] == -(-(T - 1) // (GAMMA + 1))


def test_graph_replay_equals_eager(setup, device_run):
    ids, scores, st, _ = device_run
    e = _generate(setup, {"spec_draft": "int4_g256", "spec_device_loop": True,
                          "use_hip_graph": False})
    assert torch.equal(e[0], ids) and torch.equal(e[1], scores) and e[2] == st


def test_device_path_ran(host_run, device_run, setup):
    """The round graph and ``ops.spec_verify`` produced the ``spec_device_loop``
    result: one round-graph call per round (the first runs eagerly and
    captures, the rest replay), no ``_spec_process``, no host window step."""
    spy, st = device_run[3], device_run[2]
    assert st["rounds"] > 1
    assert spy.rounds == st["rounds"] and spy.verify == 2   # the warm-up and the capture
    assert spy.process == 0 and spy.host_window == 0
    hspy = host_run[3]                                       # and the spy does see the host loop
    assert hspy.verify == 0 and hspy.rounds == 0 and hspy.host_window == host_run[2]["rounds"]
    e = _generate(setup, {"spec_draft": "int4_g256", "spec_device_loop": True,
                          "use_hip_graph": False})
    assert e[3].verify == e[3].rounds == st["rounds"]


def test_poll_interval_rounds_up_the_rounds_issued(setup, device_run):
    """With ``spec_poll`` 4 the loop issues the smallest multiple of 4 rounds
    that covers the rounds needed; the extra rounds change nothing."""
    need = device_run[2]["rounds"]
    p = _generate(setup, {"spec_draft": "int4_g256", "spec_device_loop": True, "spec_poll": 4})
    assert p[3].rounds == -(-need // 4) * 4
    assert torch.equal(p[0], device_run[0]) and torch.equal(p[1], device_run[1])
    assert p[2] == device_run[2]
