"""Beam search on the GPU: the ancestor-indexed decode attention kernel against
its fp32 formula branch, the beam decode step against the plain decode step on
materialised caches, HIP-graph replay, and the reported scores against a
teacher-forced forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _anc(pattern, B, nb, G, g):
    if pattern == "random":
        return torch.randint(0, nb, (B * nb, G), device=DEV, generator=g).to(torch.int32)
    if pattern == "shared":  # every beam descends from one row per slot
        one = torch.randint(0, nb, (B, 1, G), device=DEV, generator=g)
        return one.expand(B, nb, G).reshape(B * nb, G).to(torch.int32).contiguous()
    return torch.arange(nb, device=DEV, dtype=torch.int32).repeat(B)[:, None].expand(B * nb, G) \
        .contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nb", [1, 3, 4, 8])
@pytest.mark.parametrize("nsplit", [1, None, 7])
@pytest.mark.parametrize("BH", [(2, 4), (2, 32)])
@pytest.mark.parametrize("case", [("random", (700, 17)), ("shared", (700, 17)),
                                  ("identity", (700, 17)), ("random", (1, 700))])
def test_beam_decode_attention_kernel(dtype, D, nb, nsplit, BH, case):
    """Kernel vs the fp32 formula: ragged prefix and generated lengths, splits
    that end up empty, and NaN in every cache row the result must not touch."""
    _check_kernel(dtype, D, nb, nsplit, BH, case)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nb", [2, 5, 6, 7])
@pytest.mark.parametrize("waves", [4, 8])
def test_beam_decode_attention_other_beam_counts(dtype, D, nb, waves):
    """The remaining beam counts (5 and 7 run the 6- and 8-beam code with a
    repeated beam that is not stored) on both workgroup widths."""
    _check_kernel(dtype, D, nb, 7, (2, 4), ("random", (700, 17)), waves)


def _check_kernel(dtype, D, nb, nsplit, BH, case, waves=0):
    from fleetx_amd import ops
    from fleetx_amd.ops.attention import _beam_attention_formula
    (B, H), S, G = BH, 700, 40
    pattern, pl = case
    R = B * nb
    g = torch.Generator(device=DEV).manual_seed(nb * 131 + D + H)
    q = torch.randn(R, H, D, device=DEV, generator=g).to(dtype)
    kp, vp = (torch.randn(B, S, H, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    kg, vg = (torch.randn(R, G, H, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    plens = torch.tensor(pl, device=DEV, dtype=torch.int32)
    glens = torch.tensor([40, 1], device=DEV, dtype=torch.int32)
    anc = _anc(pattern, B, nb, G, g)
    # NaN wherever the kernel must not look
    nan = float("nan")
    pmask = torch.arange(S, device=DEV)[None, :] >= plens[:, None]
    kp[pmask], vp[pmask] = nan, nan
    valid = torch.arange(G, device=DEV)[None, :] < glens.repeat_interleave(nb)[:, None]   # [R, G]
    rows = (torch.arange(R, device=DEV) // nb * nb)[:, None] + anc.long()
    used = torch.zeros(R, G, dtype=torch.bool, device=DEV)
    slots = torch.arange(G, device=DEV)[None, :].expand(R, G)
    used[rows[valid], slots[valid]] = True
    kg[~used], vg[~used] = nan, nan
    out = ops.beam_decode_attention(q, kp, vp, plens, kg, vg, glens, anc, nsplit=nsplit,
                                    waves=waves)
    assert out.dtype == dtype and out.shape == (R, H, D)
    ref = _beam_attention_formula(q.float(), kp, vp, plens, kg, vg, glens, anc, D ** -0.5)
    assert torch.isfinite(ref).all()
    assert torch.isfinite(out).all()
    assert _rel(out, ref) < 1e-2


def test_beam_decode_attention_many_beams_use_formula():
    """More beams than the kernel holds run the formula branch, not an error."""
    from fleetx_amd import ops
    B, nb, H, D, S, G = 1, 9, 2, 64, 33, 4
    q = torch.randn(B * nb, H, D, device=DEV).bfloat16()
    kp, vp = (torch.randn(B, S, H, D, device=DEV).bfloat16() for _ in range(2))
    kg, vg = (torch.randn(B * nb, G, H, D, device=DEV).bfloat16() for _ in range(2))
    plens = torch.tensor([33], device=DEV, dtype=torch.int32)
    glens = torch.tensor([3], device=DEV, dtype=torch.int32)
    anc = torch.randint(0, nb, (B * nb, G), device=DEV).to(torch.int32)
    out = ops.beam_decode_attention(q, kp, vp, plens, kg, vg, glens, anc)
    ref = ops.beam_decode_attention(q.cpu().float(), kp.cpu(), vp.cpu(), plens.cpu(), kg.cpu(),
                                    vg.cpu(), glens.cpu(), anc.cpu())
    assert _rel(out.cpu(), ref) < 1e-2


def _big_model():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=1024, num_layers=3, num_attention_heads=8,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    return cfg, GPTForPretraining(cfg).cuda().eval()


@pytest.mark.parametrize("fused", [True, False])
def test_beam_decode_step_matches_plain_step(fused):
    """One beam decode step on random cache contents equals ``_decode_step`` on
    a plain cache of B*nb rows materialised by gathers; it writes slot t and
    nothing else."""
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = _big_model()
    B, nb, t, S, G, H, D = 2, 4, 5, 20, 8, 8, 128
    R = B * nb
    gen = gmod.GPTForGeneration(model, {"fused_decode": fused}).eval()
    g = torch.Generator(device=DEV).manual_seed(5)
    cache = gmod.BeamKVCache(cfg.num_layers, B, nb, S, G, H, D, torch.bfloat16, DEV)
    for li in range(cfg.num_layers):
        for c in (cache.k[li], cache.v[li], cache.kg[li], cache.vg[li]):
            c.normal_(generator=g)
    plens = torch.tensor([20, 9], device=DEV)
    cache.plens.copy_(plens)
    cache.anc.copy_(torch.randint(0, nb, (R, G), device=DEV, generator=g))
    cache.anc[:, t] = torch.arange(nb, device=DEV, dtype=torch.int32).repeat(B)
    nxt = torch.randint(0, 1024, (R,), device=DEV, generator=g)
    rpl = plens.repeat_interleave(nb)
    # the same contents as a plain cache: prefix, then each row's ancestors
    plain = gmod.KVCache(cfg.num_layers, R, S + G, H, D, torch.bfloat16, DEV)
    rows = (torch.arange(R, device=DEV) // nb * nb)[:, None] + cache.anc[:, :t].long()
    for li in range(cfg.num_layers):
        for dst, pre, gn in ((plain.k[li], cache.k[li], cache.kg[li]),
                             (plain.v[li], cache.v[li], cache.vg[li])):
            for r in range(R):
                p = int(rpl[r])
                dst[r, :p] = pre[r // nb, :p]
                dst[r, p:p + t] = gn[rows[r], torch.arange(t, device=DEV)]
    before = [[c.clone() for c in lst] for lst in (cache.k, cache.v, cache.kg, cache.vg)]
    slot = torch.full((R,), t, device=DEV, dtype=torch.long)
    glens = torch.full((B,), t + 1, device=DEV, dtype=torch.int32)
    calls = []
    orig = gmod._layer_decode_fused
    gmod._layer_decode_fused = lambda *a: calls.append(orig(*a)) or calls[-1]
    try:
        with torch.no_grad():
            lg = gen._beam_decode_step(nxt, rpl + t, cache, slot, glens)
    finally:
        gmod._layer_decode_fused = orig
    if fused:
        assert len(calls) == cfg.num_layers and all(c is not None for c in calls)  # fused ran
    else:
        assert not calls
    with torch.no_grad():
        ref = gen._decode_step(nxt, rpl + t, plain)
    assert _rel(lg, ref) < 2e-2
    ar = torch.arange(R, device=DEV)
    keep = torch.ones(G, dtype=torch.bool, device=DEV)
    keep[t] = False
    for li in range(cfg.num_layers):
        assert _rel(cache.kg[li][:, t], plain.k[li][ar, rpl + t]) < 2e-2
        assert _rel(cache.vg[li][:, t], plain.v[li][ar, rpl + t]) < 2e-2
        assert torch.equal(cache.k[li], before[0][li]) and torch.equal(cache.v[li], before[1][li])
        assert torch.equal(cache.kg[li][:, keep], before[2][li][:, keep])
        assert torch.equal(cache.vg[li][:, keep], before[3][li][:, keep])


def test_beam_search_hip_graph_matches_eager():
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=1024, hidden_size=256, num_layers=4, num_attention_heads=4,
                    max_position_embeddings=256, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = GPTForPretraining(cfg).cuda().eval()
    prompt = torch.randint(0, 1024, (3, 17), device=DEV)
    lens = torch.tensor([17, 9, 12], device=DEV)
    outs = []
    for graph in (False, True):
        gen = GPTForGeneration(model, {"max_dec_len": 24, "decode_strategy": "beam_search",
                                       "num_beams": 3, "num_return_sequences": 3,
                                       "eos_token_id": None, "use_hip_graph": graph})
        ids, scores = gen.generate(prompt, lens)
        outs.append((ids.cpu(), scores.cpu()))
    assert outs[0][0].shape == (9, 24)
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.allclose(outs[0][1], outs[1][1], atol=1e-3)


def test_beam_scores_are_teacher_forced_logprobs():
    """The reported scores (length_penalty 0) are the summed log-probabilities
    of the returned tokens under the ordinary training forward.  Yardstick: the
    same discrepancy of ``greedy_search`` on the same prompts; beam search,
    whose maximum runs over nb times as many rows, may reach 4x that.  A wrong
    ancestor is off by order 1 per token, rounding by around 1e-2."""
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    cfg, model = _big_model()
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 1024, (4, 21), device=DEV, generator=g)
    lens = torch.tensor([21, 9, 16, 5], device=DEV)
    T, nb = 24, 4

    def discrepancy(conf, per):
        gen = GPTForGeneration(model, dict(conf, max_dec_len=T, eos_token_id=None,
                                           length_penalty=0.0))
        ids, scores = gen.generate(prompt, lens)
        assert ids.shape == (4 * per, T)
        worst = 0.0
        for r in range(4 * per):
            n = int(lens[r // per])
            full = torch.cat([prompt[r // per, :n], ids[r]])[None]
            with torch.no_grad():
                logp = torch.log_softmax(model(full)[0, n - 1:-1].float(), -1)
            tf = logp.gather(1, ids[r][:, None]).sum().item()
            worst = max(worst, abs(tf - scores[r].item()))
        return worst

    greedy = discrepancy({"decode_strategy": "greedy_search"}, 1)
    beam = discrepancy({"decode_strategy": "beam_search", "num_beams": nb,
                        "num_return_sequences": nb}, nb)
    print("teacher-forced score discrepancy: greedy %.4g, beam search %.4g" % (greedy, beam))
    assert beam <= 4 * greedy
