"""Chunked prefill (``Generation.prefill_chunk``) and multi-turn sessions
(``GPTForGeneration.new_session`` / ``generate(..., session=)``) on the CPU in
fp32, against full recompute (``_naive_greedy`` of tests/test_generation.py)."""
import pytest
import torch

from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G
from tests.test_generation import _naive_greedy

V = 97


def _model(seed=0, max_pos=256):
    """tests/test_generation.py::_model with room for prompts beyond 64 tokens."""
    torch.manual_seed(seed)
    cfg = GPTConfig(vocab_size=V, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=max_pos, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    m = GPTForPretraining(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.eval()


def _gen(m, **kw):
    cfg = {"decode_strategy": "greedy_search", "max_dec_len": 6, "eos_token_id": None}
    cfg.update(kw)
    return G.GPTForGeneration(m, cfg)


def _ragged(lens, seed=1):
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randint(1, V, (n,), generator=g) for n in lens]
    ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return ids, torch.tensor(lens), rows


def _naive_scores(m, row, toks):
    """Sum of the log-probabilities of ``toks`` after ``row`` under full recompute."""
    cur, s = row[None, :], 0.0
    for t in toks.tolist():
        with torch.no_grad():
            lp = torch.log_softmax(m(cur)[:, -1].float(), -1)
        s += float(lp[0, t])
        cur = torch.cat([cur, torch.tensor([[t]])], 1)
    return s


def test_prefill_chunk_values():
    m = _model()
    for bad in (1, 63, 100, -64, 64.0, "64", True):
        with pytest.raises(ValueError):
            _gen(m, prefill_chunk=bad)
    assert _gen(m).prefill_chunk == 0
    assert _gen(m, prefill_chunk=128).prefill_chunk == 128


@pytest.mark.parametrize("strategy", ["greedy_search", "beam_search"])
def test_chunked_prefill_matches_recompute(strategy):
    """Prompts of 150 and 37 tokens in chunks of 64: row 1 is empty in chunks 1
    and 2.  Greedy ids equal full recompute; one beam is greedy too."""
    m = _model()
    ids, lens, rows = _ragged([150, 37])
    gen = _gen(m, prefill_chunk=64, decode_strategy=strategy, num_beams=1)
    out, _ = gen.generate(ids, lens)
    for b, r in enumerate(rows):
        assert torch.equal(out[b], _naive_greedy(m, r[None, :], 6)[0]), b


def test_short_prompt_is_the_default_path():
    """S <= prefill_chunk: the one-pass prefill, bit for bit."""
    m = _model(1)
    ids, lens, _ = _ragged([50, 20])
    a, sa = _gen(m).generate(ids, lens)
    b, sb = _gen(m, prefill_chunk=64).generate(ids, lens)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_chunked_cache_and_logits_match_one_pass():
    m = _model(2)
    ids, lens, _ = _ragged([150, 37])
    one, chk = _gen(m), _gen(m, prefill_chunk=64)
    s1, s2 = one.new_session(2), chk.new_session(2)
    one.generate(ids, lens, max_length=1, session=s1)
    chk.generate(ids, lens, max_length=1, session=s2)
    assert s1.logits.dtype == torch.float32 and s1.logits.shape == (2, V)
    assert float((s1.logits - s2.logits).abs().max()) <= 1e-5
    for li in range(2):
        for b, n in enumerate(lens.tolist()):
            for c1, c2 in ((s1.cache.k, s2.cache.k), (s1.cache.v, s2.cache.v)):
                assert float((c1[li][b, :n] - c2[li][b, :n]).abs().max()) <= 1e-5
    assert s2.lens.tolist() == [150, 37] and (s2.pending >= 0).all()


@pytest.mark.parametrize("chunk", [0, 64])
def test_two_turn_session_matches_recompute(chunk):
    m = _model(3)
    gen = _gen(m, prefill_chunk=chunk, max_dec_len=5)
    ids1, lens1, rows1 = _ragged([70, 9], seed=4)
    ids2, lens2, rows2 = _ragged([3, 80], seed=5)
    s = gen.new_session(2)
    out1, sc1 = gen.generate(ids1, lens1, session=s)
    assert s.lens.tolist() == [70 + 4, 9 + 4]
    assert s.pending.tolist() == out1[:, -1].tolist()
    out2, sc2 = gen.generate(ids2, lens2, session=s)
    for b in range(2):
        ref1 = _naive_greedy(m, rows1[b][None, :], 5)[0]
        assert torch.equal(out1[b], ref1), b
        assert abs(float(sc1[b]) - _naive_scores(m, rows1[b], ref1)) <= 1e-4
        transcript = torch.cat([rows1[b], ref1, rows2[b]])
        ref2 = _naive_greedy(m, transcript[None, :], 5)[0]
        assert torch.equal(out2[b], ref2), b
        assert abs(float(sc2[b]) - _naive_scores(m, transcript, ref2)) <= 1e-4
        full = torch.cat([transcript, ref2])
        n = int(s.lens[b]) + 1
        assert n == len(full) and torch.equal(s.tokens[b, :n], full)
    # a turn without new tokens continues from the pending token
    out3, _ = gen.generate(torch.zeros(2, 0, dtype=torch.long), torch.tensor([0, 0]), session=s)
    for b in range(2):
        full = torch.cat([rows1[b], out1[b], rows2[b], out2[b]])
        assert torch.equal(out3[b], _naive_greedy(m, full[None, :], 5)[0])
    s.reset()
    assert s.lens.tolist() == [0, 0] and s.pending.tolist() == [-1, -1] and s.logits is None
    again, _ = gen.generate(ids1, lens1, session=s)
    assert torch.equal(again, out1)


def test_session_eos_row_stops_early():
    """EOS = the token row 0 emits at step 2 of a dry run: its transcript ends
    at the EOS, pads are not in it, the other row goes on."""
    m = _model(4)
    ids1, lens1, rows1 = _ragged([20, 33], seed=6)
    dry, _ = _gen(m, max_dec_len=6).generate(ids1, lens1)
    eos = int(dry[0, 2])
    k1 = dry[1].tolist().index(eos) + 1 if eos in dry[1].tolist() else 6
    k0 = dry[0].tolist().index(eos) + 1          # <= 3
    gen = _gen(m, max_dec_len=6, eos_token_id=eos, pad_token_id=0)
    s = gen.new_session(2)
    out1, _ = gen.generate(ids1, lens1, session=s)
    assert out1[0, :k0].tolist() == dry[0, :k0].tolist()
    assert out1[0, k0:].tolist() == [0] * (out1.shape[1] - k0)
    assert s.lens.tolist() == [20 + k0 - 1, 33 + k1 - 1]
    assert s.pending.tolist() == [eos, int(dry[1, k1 - 1])]
    assert s.tokens[0, :20 + k0].tolist() == rows1[0].tolist() + dry[0, :k0].tolist()
    hist = s.history()
    assert hist.shape[1] == max(20 + k0, 33 + k1)
    assert hist[0, 20 + k0:].tolist() == [int(rows1[0][0])] * (hist.shape[1] - 20 - k0)
    # turn 2 continues each transcript after its own end
    ids2, lens2, rows2 = _ragged([5, 2], seed=7)
    gen2 = _gen(m, max_dec_len=4)
    out2, _ = gen2.generate(ids2, lens2, session=s)
    for b, k in enumerate((k0, k1)):
        transcript = torch.cat([rows1[b], dry[b, :k], rows2[b]])
        assert torch.equal(out2[b], _naive_greedy(m, transcript[None, :], 4)[0]), b


def test_session_repetition_penalty_covers_the_transcript():
    m = _model(5)
    pen = 1.7
    gen = _gen(m, max_dec_len=4, repetition_penalty=pen)
    ids1, lens1, rows1 = _ragged([12, 30], seed=8)
    ids2, lens2, rows2 = _ragged([6, 3], seed=9)
    s = gen.new_session(2)
    out1, _ = gen.generate(ids1, lens1, session=s)
    out2, _ = gen.generate(ids2, lens2, session=s)

    def naive(row, n):
        cur, out = row, []
        for _ in range(n):
            with torch.no_grad():
                lg = m(cur[None, :])[0, -1].float()
            seen = torch.unique(cur)
            lg[seen] = torch.where(lg[seen] < 0, lg[seen] * pen, lg[seen] / pen)
            out.append(int(lg.argmax()))
            cur = torch.cat([cur, torch.tensor(out[-1:])])
        return out
    plain = _gen(m, max_dec_len=4)
    differs = False
    for b in range(2):
        assert out1[b].tolist() == naive(rows1[b], 4), b
        transcript = torch.cat([rows1[b], out1[b], rows2[b]])
        assert out2[b].tolist() == naive(transcript, 4), b
        differs |= out2[b].tolist() != _naive_greedy(m, transcript[None, :], 4)[0].tolist()
    assert differs, "the penalty changed nothing: the test shows nothing"
    assert plain.repetition_penalty == 1.0


def test_session_errors():
    m = _model(6, max_pos=128)
    gen = _gen(m)
    ids, lens, _ = _ragged([10, 4])
    s = gen.new_session(2, max_len=64)
    assert s.cache.max_len == 64 and gen.new_session(1, max_len=10 ** 6).cache.max_len == 128

    def untouched():
        assert s.lens.tolist() == [0, 0] and s.pending.tolist() == [-1, -1]
        assert s.logits is None and int(s.tokens.abs().sum()) == 0
    with pytest.raises(ValueError):                       # batch size
        gen.generate(ids[:1], lens[:1], session=s)
    with pytest.raises(ValueError):                       # a row with nothing to prefill
        gen.generate(ids, torch.tensor([10, 0]), session=s)
    big, blens, _ = _ragged([65, 4])
    with pytest.raises(ValueError):                       # does not fit 64 rows
        gen.generate(big, blens, session=s)
    untouched()
    for kw in ({"decode_strategy": "beam_search", "num_beams": 2}, {"device_loop": True},
               {"spec_draft": "int8"}, {"spec_device_loop": True},
               {"num_return_sequences": 2, "decode_strategy": "sampling"}):
        with pytest.raises(ValueError):
            _gen(m, **kw).generate(ids, lens, session=s)
    drafted = _gen(m)
    drafted.set_drafter(object())
    with pytest.raises(ValueError):
        drafted.generate(ids, lens, session=s)
    untouched()
    # the second turn must fit as well: 10 + 6 - 1 in the cache, pending + 50 do not fit
    gen.generate(ids, lens, session=s)
    before = (s.lens.clone(), s.pending.clone())
    more, mlens, _ = _ragged([50, 50])
    with pytest.raises(ValueError):
        gen.generate(more, mlens, session=s)
    assert torch.equal(s.lens, before[0]) and torch.equal(s.pending, before[1])


def test_sampling_session_runs():
    m = _model(7)
    gen = _gen(m, decode_strategy="sampling", top_k=5, max_dec_len=4)
    s = gen.new_session(2)
    ids, lens, _ = _ragged([9, 70])
    a, _ = gen.generate(ids, lens, seed=3, session=s)
    b, _ = gen.generate(ids[:, :2], torch.tensor([2, 1]), seed=4, session=s)
    assert a.shape == (2, 4) and b.shape == (2, 4)
    assert s.lens.tolist() == [9 + 4 + 2 + 3, 70 + 4 + 1 + 3]


def test_module_passes_a_session_through():
    from fleetx_amd.models.language_model.language_module import GPTGenerationModule

    class Tok:
        eos_token_id = 0

        def encode(self, t):
            return [1 + (ord(ch) % (V - 1)) for ch in t]

        def convert_ids_to_string(self, row):
            return " ".join(str(t) for t in row)
    mod = GPTGenerationModule.__new__(GPTGenerationModule)
    torch.nn.Module.__init__(mod)
    mod.model = _gen(_model(8), max_dec_len=3)
    mod.tokenizer = Tok()
    s = mod.new_session(2)
    assert isinstance(s, G.GenerationSession) and s.batch_size == 2
    first = mod.generate(["hello there", "hi"], session=s)
    assert s.lens.tolist() == [11 + 2, 2 + 2]
    second = mod.generate(["and", "then what"], session=s)
    assert s.lens.tolist() == [13 + 1 + 3 + 2, 4 + 1 + 9 + 2]
    assert len(first) == 2 and len(second) == 2
    assert mod.generate(["hello there", "hi"]) == first       # no session: the plain call
