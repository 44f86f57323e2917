"""Beam search (``decode_strategy: beam_search``) on the CPU paths: the cached
search on a ``BeamKVCache`` against a brute-force oracle that keeps no cache,
and ``ops.beam_decode_attention``'s formula branch against
``ops.decode_attention`` on materialised caches."""
import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G

V = 97
GAP = 1e-4


def _model(seed=0):
    torch.manual_seed(seed)
    cfg = GPTConfig(vocab_size=V, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=64, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    m = GPTForPretraining(cfg)
    with torch.no_grad():  # non-trivial LN/bias so the check is meaningful
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.eval()


def _oracle_sample(model, prompt, nb, max_new, eos=None, lp=0.0, early=False, seen=None):
    """Beam search for one unpadded prompt by full recomputation: ``model(ids)``
    for every beam at every step, no cache.  Returns the pool
    ``[(score, tokens)]``, best first.  ``seen``: list that receives the tokens
    of the top ``nb`` candidates of every step."""
    beams = [([], 0.0)]
    pool = []

    def add(score, toks):
        pool.append((score, toks))
        pool.sort(key=lambda e: -e[0])  # stable: the earlier entry wins a tie
        del pool[nb:]

    for t in range(max_new):
        rows = []
        for toks, sc in beams:
            ids = torch.cat([prompt, torch.tensor(toks, dtype=torch.long)])[None]
            with torch.no_grad():
                logp = torch.log_softmax(model(ids)[0, -1].float(), -1)
            rows.append(sc + logp)
        cand = torch.cat(rows).tolist()  # flat (beam, token) index
        order = sorted(range(len(cand)), key=lambda i: (-cand[i], i))[:2 * nb + 1]
        top = [cand[i] for i in order]
        # the test is only meaningful where rounding cannot reorder the candidates
        assert all(a - b > GAP for a, b in zip(top, top[1:])), (t, top)
        if seen is not None:
            seen.append([i % V for i in order[:nb]])
        new = []
        for rank, i in enumerate(order[:2 * nb]):
            b, tok = divmod(i, V)
            if eos is not None and tok == eos:
                if rank < nb:
                    add(cand[i] / float(t + 1) ** lp, beams[b][0] + [tok])
            elif len(new) < nb:
                new.append((beams[b][0] + [tok], cand[i]))
        beams = new
        if len(pool) == nb and (early or pool[-1][0] >= beams[0][1] / float(t + 1) ** lp):
            return pool
    for toks, sc in beams:
        add(sc / float(max_new) ** lp, toks)
    return pool


def _oracle(model, prompts, nb, max_new, nret=None, pad=0, **kw):
    nret = nret or nb
    hyps = [h for p in prompts for h in _oracle_sample(model, p, nb, max_new, **kw)[:nret]]
    T = max(len(toks) for _, toks in hyps)
    ids = torch.tensor([toks + [pad] * (T - len(toks)) for _, toks in hyps], dtype=torch.long)
    return ids, torch.tensor([s for s, _ in hyps])


def _batch(prompts, pad=0):
    S = max(len(p) for p in prompts)
    ids = torch.stack([torch.cat([p, torch.full((S - len(p),), pad, dtype=torch.long)])
                       for p in prompts])
    return ids, torch.tensor([len(p) for p in prompts])


def _prompts(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(4, V, (n,), generator=g) for n in (7, 4, 9)]


@pytest.mark.parametrize("nb", [2, 3])
def test_beam_search_matches_bruteforce_oracle(nb):
    m = _model(3)
    prompts = _prompts(11)
    gen = G.GPTForGeneration(m, {"decode_strategy": "beam_search", "num_beams": nb,
                                 "num_return_sequences": nb, "max_dec_len": 7,
                                 "eos_token_id": None})
    out, scores = gen.generate(*_batch(prompts))
    ref_ids, ref_scores = _oracle(m, prompts, nb, 7)
    assert out.shape == (3 * nb, 7)
    assert torch.equal(out, ref_ids)
    assert torch.allclose(scores, ref_scores, atol=1e-4, rtol=0)


def test_one_beam_is_greedy():
    m = _model(1)
    ids, lens = _batch(_prompts(5))
    cfg = {"max_dec_len": 8, "eos_token_id": None, "length_penalty": 0.0}
    beam = G.GPTForGeneration(m, dict(cfg, decode_strategy="beam_search", num_beams=1))
    greedy = G.GPTForGeneration(m, dict(cfg, decode_strategy="greedy_search"))
    out, scores = beam.generate(ids, lens)
    ref, ref_scores = greedy.generate(ids, lens)
    assert torch.equal(out, ref)
    assert torch.allclose(scores, ref_scores, atol=1e-4, rtol=0)


@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_beam_search_eos(early, lp):
    m = _model(3)
    prompts = _prompts(11)
    nb, max_new, pad = 3, 8, 0
    # an EOS id that the search meets: a top-nb candidate of sample 0 at step 2
    seen = []
    _oracle_sample(m, prompts[0], nb, max_new, seen=seen)
    eos = seen[2][1]
    ref_ids, ref_scores = _oracle(m, prompts, nb, max_new, pad=pad, eos=eos, lp=lp, early=early)
    finished = (ref_ids == eos).any(-1)
    assert finished.any(), "the chosen EOS never finished a hypothesis"
    gen = G.GPTForGeneration(m, {"decode_strategy": "beam_search", "num_beams": nb,
                                 "num_return_sequences": nb, "max_dec_len": max_new,
                                 "eos_token_id": eos, "pad_token_id": pad, "length_penalty": lp,
                                 "early_stopping": early})
    out, scores = gen.generate(*_batch(prompts, pad))
    assert torch.equal(out, ref_ids)
    assert torch.allclose(scores, ref_scores, atol=1e-4, rtol=0)
    # finished rows: nothing but padding after the EOS
    for row in out[finished]:
        end = row.tolist().index(eos)
        assert (row[end + 1:] == pad).all()


def test_beam_search_configuration():
    m = _model(3)
    prompts = _prompts(11)
    base = {"decode_strategy": "beam_search", "num_beams": 3, "max_dec_len": 6,
            "eos_token_id": None}
    out, scores = G.GPTForGeneration(m, dict(base, num_return_sequences=2)).generate(
        *_batch(prompts))
    ref_ids, ref_scores = _oracle(m, prompts, 3, 6, nret=2)
    assert out.shape == (6, 6)
    assert torch.equal(out, ref_ids)
    assert torch.allclose(scores, ref_scores, atol=1e-4, rtol=0)
    assert (scores.view(3, 2)[:, 0] >= scores.view(3, 2)[:, 1]).all()
    with pytest.raises(ValueError):
        G.GPTForGeneration(m, dict(base, num_return_sequences=4))
    with pytest.raises(ValueError, match="not supported"):
        G.GPTForGeneration(m, dict(base, num_beams=4, num_beam_groups=2))


def test_beam_decode_attention_cpu_matches_materialised():
    g = torch.Generator().manual_seed(0)
    B, nb, H, D, S, Gn = 3, 3, 2, 16, 11, 6
    R = B * nb
    q = torch.randn(R, H, D, generator=g)
    kp, vp = torch.randn(B, S, H, D, generator=g), torch.randn(B, S, H, D, generator=g)
    kg, vg = torch.randn(R, Gn, H, D, generator=g), torch.randn(R, Gn, H, D, generator=g)
    plens = torch.tensor([11, 1, 5], dtype=torch.int32)
    glens = torch.tensor([6, 3, 1], dtype=torch.int32)
    anc = torch.randint(0, nb, (R, Gn), generator=g).to(torch.int32)
    out = ops.beam_decode_attention(q, kp, vp, plens, kg, vg, glens, anc)
    kc, vc = torch.zeros(R, S + Gn, H, D), torch.zeros(R, S + Gn, H, D)
    lens = torch.zeros(R, dtype=torch.int32)
    for r in range(R):
        b = r // nb
        p, n = int(plens[b]), int(glens[b])
        rows = b * nb + anc[r, :n].long()
        kc[r, :p], vc[r, :p] = kp[b, :p], vp[b, :p]
        kc[r, p:p + n], vc[r, p:p + n] = kg[rows, torch.arange(n)], vg[rows, torch.arange(n)]
        lens[r] = p + n
    ref = ops.decode_attention(q, kc, vc, lens)
    assert torch.allclose(out, ref, atol=1e-5, rtol=1e-5)


def test_beam_search_config_file(tmp_path, monkeypatch):
    """The shipped beam-search config builds a generation module that runs."""
    import os
    from tests.test_generation import _tiny_bpe
    from fleetx_amd.utils import config as C
    from fleetx_amd.models import build_module
    monkeypatch.setenv("FLEETX_TOKENIZER_DIR", str(_tiny_bpe(tmp_path / "tok")))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt",
                     "generation_gpt_345M_beam_search.yaml"),
        overrides=["Model.hidden_size=64", "Model.num_layers=2", "Model.num_attention_heads=4",
                   "Model.max_position_embeddings=64", "Global.device=cpu",
                   "Model.vocab_size=264", "Generation.max_dec_len=5"], nranks=1)
    module = build_module(cfg)
    assert module.model.decode_strategy == "beam_search" and module.model.num_beams == 4
    out = module.generate("hello world")
    assert isinstance(out, list) and isinstance(out[0], str)
