"""On-device token selection on the GPU: ``select_kernel`` against the torch
logits processors (+ ``argmax`` / ``fused_sample``), and
``Generation.device_loop`` against the default host loop."""
import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from tests import device_loop_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
# fewer elements than threads, a partial stride, a partial bitmap word, the real head
SHAPES = [(V, B) for V in (97, 1000, 1057, 50304) for B in (1, 5)]


def _named(tok, name, V, B, st):
    if name == "tie":
        assert tok.tolist() == [V // 3] * B               # the lower of two equal maxima
    if name == "min_len_before":
        assert C.EOS not in tok.tolist()
    if name == "min_len_at":
        assert tok.tolist() == [C.EOS] * B and not st.unfinished.any()
    if name == "forced_bos":
        assert tok.tolist() == [C.BOS] * B
    if name == "forced_eos":
        assert tok.tolist() == [C.EOS] * B
    if name == "finished_row" and B > 1:
        assert tok[1] == C.PAD and st.finish_len[1] == 2 and st.unfinished[1] == 0


@pytest.mark.parametrize("name", sorted(C.CASES))
@pytest.mark.parametrize("V,B", SHAPES)
def test_kernel_greedy(V, B, name):
    logits, hist, st, c = C.build(name, V, B, DEV)
    x = C.torch_processed(logits, hist, c)                # the torch processors, on the GPU
    pick = torch.argmax(x, -1)
    before, keep = C.snapshot(st), logits.clone()
    ops.select_token(logits, st)
    assert torch.equal(logits, keep)                      # read-only
    tok = C.check_step(st, before, x, pick, hist, c, V)
    _named(tok, name, V, B, st)


@pytest.mark.parametrize("tkp", [(0.7, 0, 0.9), (0.8, 40, 0.8)])
@pytest.mark.parametrize("name", sorted(C.CASES))
@pytest.mark.parametrize("V,B", SHAPES)
def test_kernel_sampling(V, B, name, tkp):
    """``fused_sample`` on the torch-processed logits and ``select_token`` on the
    raw ones, fed the same uniforms, pick the same tokens."""
    g, g2 = [torch.Generator(device=DEV).manual_seed(11) for _ in range(2)]
    step = C.CASES[name]["step"]
    u = torch.full((C.N_STEPS, B), float("nan"), device=DEV)
    u[step] = torch.rand(B, device=DEV, generator=g2)
    logits, hist, st, c = C.build(name, V, B, DEV, greedy=False, sample=tkp, u=u)
    x = C.torch_processed(logits, hist, c)
    pick, _ = ops.fused_sample(x, tkp[0], tkp[1], tkp[2], generator=g)
    before = C.snapshot(st)
    ops.select_token(logits, st)
    tok = C.check_step(st, before, x, pick, hist, c, V)
    if name != "tie":
        _named(tok, name, V, B, st)


def test_step_past_the_table_is_a_no_op():
    logits, hist, st, c = C.build("penalty", 1057, 5, DEV)
    st.step.fill_(C.N_STEPS)
    before = [t.clone() for t in (st.out, st.seen, st.scores, st.nxt, st.cur, st.step)]
    ops.select_token(logits, st)
    for a, b in zip(before, (st.out, st.seen, st.scores, st.nxt, st.cur, st.step)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ generate()
T = 24
CFG = {"decode_strategy": "greedy_search", "max_dec_len": T, "repetition_penalty": 1.3,
       "min_dec_len": 2, "pad_token_id": 0}
# the model of test_hip_graph_decode_matches_eager; one wide enough for the fused GEMVs, also int8
MODELS = {"h256": (256, 4, 4, None), "h1024": (1024, 3, 16, None),
          "h1024_int8": (1024, 3, 16, "int8")}


@pytest.fixture(scope="module", params=sorted(MODELS))
def runs(request):
    """Host loop and device loop (graph and eager) on one model, same EOS."""
    hidden, layers, heads, wq = MODELS[request.param]
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=hidden, num_layers=layers,
                    num_attention_heads=heads, max_position_embeddings=256,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    dtype=torch.bfloat16)
    model = C.varied(GPTForPretraining(cfg)).cuda().eval()
    prompt = torch.randint(4, 1024, (3, 17), device=DEV)
    lens = torch.tensor([17, 9, 12], device=DEV)
    base = dict(CFG, weight_quant=wq)

    def run(**kw):
        with C.Spy() as spy:
            ids, scores = G.GPTForGeneration(model, dict(base, **kw)).generate(prompt, lens)
        return ids.cpu(), scores.cpu(), spy
    free = run(eos_token_id=None)[0]
    eos = C.pick_eos(free)
    off = run(eos_token_id=eos)
    hit = [(row.index(eos) if eos in row else None) for row in off[0].tolist()]
    early = [h is not None and 3 <= h <= 6 for h in hit]
    assert any(early) and not all(early), hit
    on = run(eos_token_id=eos, device_loop=True)
    eager = run(eos_token_id=eos, device_loop=True, use_hip_graph=False)
    return off, on, eager, eos


def test_device_path_ran(runs):
    """The device loop, not the host loop, produced the ``device_loop`` results:
    every token after the first came from the graphed select step (graph run)
    or from one eager ``select_token`` per selection (eager run)."""
    off, on, eager, eos = runs
    done = bool((on[0] == eos).any(1).all())
    n = C.selections(on[0].shape[1], T, 8, done)
    assert n >= on[0].shape[1] > 1
    spy = on[2]
    assert spy.select_graph == n - 1 and spy.host_graph == 0 and spy.fused_sample == 0
    assert spy.select == 3                   # selection 0, the warm-up, the capture
    spy = eager[2]
    assert spy.select == n and spy.select_graph == 0 and spy.host_graph == 0
    spy = off[2]                             # and the spy does see the host loop
    assert spy.select == 0 and spy.select_graph == 0
    assert spy.host_graph == off[0].shape[1] - (1 if done else 0)


def test_generate_parity(runs):
    (ref_ids, ref_scores, _), (ids, scores, _), _, _ = runs
    assert torch.equal(ids, ref_ids)
    n = ref_ids.shape[1]
    assert float(ref_scores.abs().max()) / n < 10     # |lse| <= 10 per step, the bound's premise
    print("score err", (scores - ref_scores).abs().max().item(), "T", n)
    assert torch.allclose(scores, ref_scores, rtol=0, atol=n * 2e-4)


def test_graph_matches_eager(runs):
    _, (ids, scores, _), (eids, escores, _), _ = runs
    assert torch.equal(ids, eids) and torch.equal(scores, escores)


def test_sampling_reproducible_under_graph():
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=256, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = C.varied(GPTForPretraining(cfg)).cuda().eval()
    prompt = torch.randint(4, 1024, (3, 9), device=DEV)
    conf = {"decode_strategy": "sampling", "top_k": 20, "top_p": 0.9, "temperature": 0.8,
            "max_dec_len": 12, "eos_token_id": None, "pad_token_id": 0, "device_loop": True}
    with C.Spy() as spy:
        a = G.GPTForGeneration(model, conf).generate(prompt, seed=3)
    assert spy.select_graph == 11 and spy.select == 3 and spy.fused_sample == 0
    assert spy.host_graph == 0
    b = G.GPTForGeneration(model, conf).generate(prompt, seed=3)
    e = G.GPTForGeneration(model, dict(conf, use_hip_graph=False)).generate(prompt, seed=3)
    assert a[0].shape == (3, 12)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], e[0]) and torch.equal(a[1], e[1])
