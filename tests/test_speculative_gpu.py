"""Speculative greedy decoding on the GPU: the output does not depend on the
drafter, HIP-graph replay, every emitted token against an fp32 teacher-forced
oracle, EOS inside a window, and the fallback to the plain loop."""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, GAMMA, B = 24, 4, 3
# Shortfall of the chosen token below the fp32 oracle's best logit, worst over
# all rows and positions, measured on the plain greedy path (16-bit weights,
# this model and these prompts; that path is the same code before and after the
# window step was added): 0.00276351 (logit units; both paths are bf16 roundings
# of the same logits).  The allowance is twice that.
TAU_MEASURED = 0.00276351
TAU = 2 * TAU_MEASURED
CONF = {"decode_strategy": "greedy_search", "max_dec_len": T, "eos_token_id": None,
        "pad_token_id": 0}


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
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    model, prompt, lens = setup
    gen = GPTForGeneration(model, dict(CONF, spec_tokens=GAMMA, **conf))
    if drafter is not None:
        gen.set_drafter(drafter)
    ids, scores = gen.generate(prompt, lens)
    return ids, scores, gen.last_spec_stats


@pytest.fixture(scope="module")
def int4_run(setup):
    return _generate(setup, {"spec_draft": "int4_g256"})


def test_output_does_not_depend_on_the_drafter(setup, int4_run):
    """int4 draft, int8 draft, random tokens and a perfect draft give the same
    ids and scores.  The perfect drafter replays the int4 run's ids; for the
    slots past ``max_dec_len`` in its last round it needs the continuation,
    taken from the same run at ``max_dec_len + GAMMA`` (whose first T tokens
    are asserted to be the first run's)."""
    _, _, lens = setup
    ids, scores, st = int4_run
    assert ids.shape == (B, T)
    assert st["drafted"] == GAMMA * st["rounds"] * B and 0 <= st["accepted"] <= st["drafted"]
    longer, _, _ = _generate(setup, {"spec_draft": "int4_g256", "max_dec_len": T + GAMMA})
    assert torch.equal(longer[:, :T], ids)
    runs = {"int8": _generate(setup, {"spec_draft": "int8"}),
            "random": _generate(setup, {}, RandomDrafter()),
            "perfect": _generate(setup, {}, ReplayDrafter(longer, lens))}
    for name, (i2, s2, st2) in runs.items():
        print(name, st2)
        assert torch.equal(i2, ids), name
        assert torch.allclose(s2, scores, atol=1e-3, rtol=0), name
    st8, stp = runs["int8"][2], runs["perfect"][2]
    assert st8["drafted"] == GAMMA * st8["rounds"] * B
    assert stp["accepted"] == stp["drafted"]
    assert stp["rounds"] == -(-(T - 1) // (GAMMA + 1))


def test_graph_replay_equals_eager(setup, int4_run):
    ids, scores, _ = int4_run
    i2, s2, _ = _generate(setup, {"spec_draft": "int4_g256", "use_hip_graph": False})
    assert torch.equal(i2, ids) and torch.allclose(s2, scores, atol=1e-3, rtol=0)


def test_every_token_is_the_targets_greedy_choice(setup, int4_run):
    """Teacher-force the fp32 copy of the model over prompt + emitted ids: at
    every emitted position the chosen token's logit is within TAU of the
    oracle's maximum.  The plain greedy loop runs under the same assertion as
    the control.  Measured: plain 0.00276351 (hence TAU = 0.00552702),
    speculative (int4 draft, 16-bit target) 0.00153112."""
    model, prompt, lens = setup
    oracle = copy.deepcopy(model).float().cpu()
    plain, _, none = _generate(setup, {})
    assert none is None

    def shortfall(ids):
        worst = 0.0
        for r in range(B):
            n = int(lens[r])
            full = torch.cat([prompt[r, :n], ids[r]])[None].cpu()
            with torch.no_grad():
                lg = oracle(full)[0, n - 1:-1]
            gap = lg.max(-1).values - lg.gather(1, ids[r].cpu()[:, None]).squeeze(1)
            worst = max(worst, gap.max().item())
        return worst

    sp, ss = shortfall(plain), shortfall(int4_run[0])
    print("shortfall below the fp32 oracle's maximum: plain %.6g, speculative %.6g, tau %.6g"
          % (sp, ss, TAU))
    assert sp <= TAU
    assert ss <= TAU


def test_eos_inside_a_window(setup, int4_run):
    """EOS = a token the eos-free output holds mid-sequence: every row equals
    its eos-free row cut after the first EOS and padded."""
    free = int4_run[0]
    firsts = [(r.tolist().index(t), b, t) for b, r in enumerate(free) for t in set(r.tolist())]
    k, _, eos = max(f for f in firsts if f[0] < T - 1)
    assert k >= 1
    ids, _, _ = _generate(setup, {"spec_draft": "int4_g256", "eos_token_id": eos})
    want = torch.zeros_like(free)
    width = 0
    for b in range(B):
        row = free[b].tolist()
        n = row.index(eos) + 1 if eos in row else T
        want[b, :n] = free[b, :n]
        width = max(width, n)
    assert torch.equal(ids, want[:, :width])


def test_too_many_rows_fall_back_to_the_plain_loop(setup):
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    model, prompt, lens = setup
    plain, _ = GPTForGeneration(model, dict(CONF)).generate(prompt, lens)
    gen = GPTForGeneration(model, dict(CONF, spec_draft="int4_g256", spec_tokens=7))  # 24 rows
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, _ = gen.generate(prompt, lens)
        b, _ = gen.generate(prompt, lens)
    assert torch.equal(a, plain) and torch.equal(b, plain) and gen.last_spec_stats is None
    assert len([r for r in rec if "speculative" in str(r.message)]) == 1
