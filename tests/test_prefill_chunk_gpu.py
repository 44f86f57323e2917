"""Chunked prefill and session turns on the MI355X in bf16 / fp16: the logits
of the chunked / offset prefill (``fa_fwd_qoff_kernel``) against the one-pass
prefill (``fa_fwd_kernel``, today's path), each measured against the same
weights run in fp32 through the formula path on the CPU.

  E_one = max |one-pass logits - fp32 logits|
  E_new = max |chunked / offset logits - fp32 logits|
  required: E_new <= 2 E_one

Both are 16-bit evaluations of the same math that differ only in GEMM row
grouping and attention tiling; 2x is the margin for the maximum over a few
hundred values of two independent roundings.  The measured pairs are in
profiles/prefill_over_cache/README.md."""
import pytest
import torch

from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 1024
PROMPTS, CHUNK, TURN2 = [150, 37], 64, 70


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fleetx_amd.ops import _lib
    _lib.kernels()
    torch.manual_seed(0)


def _models(hidden, dtype):
    """A 2-layer, 2-head model in ``dtype`` on the GPU and the same (rounded)
    weights in fp32 on the CPU."""
    torch.manual_seed(hidden)
    kw = dict(vocab_size=V, hidden_size=hidden, num_layers=2, num_attention_heads=2,
              max_position_embeddings=512, hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0)
    m16 = GPTForPretraining(GPTConfig(dtype=dtype, **kw))
    with torch.no_grad():
        for _, p in m16.named_parameters():
            if p.ndim == 1:
                p.add_((0.05 * torch.randn(p.shape)).to(device=p.device, dtype=p.dtype))
    m32 = GPTForPretraining(GPTConfig(dtype=torch.float32, **kw))
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16.to(DEV).eval(), m32.cpu().eval()


def _gen(m, **kw):
    cfg = {"decode_strategy": "greedy_search", "max_dec_len": 0, "eos_token_id": None}
    cfg.update(kw)
    return G.GPTForGeneration(m, cfg)


def _ragged(lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, V, (n,), generator=g)
    return ids, torch.tensor(lens)


def _prefill_logits(gen, session, ids, lens, dev):
    """Prefill only (``max_dec_len`` 0): nothing is emitted, nothing pending."""
    out, _ = gen.generate(ids.to(dev), lens.to(dev), session=session)
    assert out.shape == (len(lens), 0)
    return session.logits.float().cpu()


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_chunked_and_offset_prefill_error(dtype, hidden):
    m16, m32 = _models(hidden, dtype)
    ids1, lens1 = _ragged(PROMPTS, 1)
    ids2, lens2 = _ragged([TURN2, TURN2], 2)
    both = torch.zeros(2, max(PROMPTS) + TURN2, dtype=torch.long)
    for b, n in enumerate(PROMPTS):
        both[b, :n] = ids1[b, :n]
        both[b, n:n + TURN2] = ids2[b]
    blens = lens1 + TURN2
    one, new, ref = _gen(m16), _gen(m16, prefill_chunk=CHUNK), _gen(m32)
    # turn 1: one pass (today's flash call) against chunks of 64
    s_new, s_ref = new.new_session(2), ref.new_session(2)
    f1 = _prefill_logits(ref, s_ref, ids1, lens1, "cpu")
    a1 = _prefill_logits(one, one.new_session(2), ids1, lens1, DEV)
    b1 = _prefill_logits(new, s_new, ids1, lens1, DEV)
    # turn 2: the whole transcript in one pass against 70 tokens at offsets 150 / 37
    f2 = _prefill_logits(ref, s_ref, ids2, lens2, "cpu")
    a2 = _prefill_logits(one, one.new_session(2), both, blens, DEV)
    b2 = _prefill_logits(new, s_new, ids2, lens2, DEV)
    assert s_new.lens.tolist() == [n + TURN2 for n in PROMPTS] == s_ref.lens.tolist()
    assert s_new.pending.tolist() == [-1, -1]
    f2_one = _prefill_logits(ref, ref.new_session(2), both, blens, "cpu")
    assert float((f2 - f2_one).abs().max()) <= 1e-4      # the fp32 reference itself
    for turn, f, a, b in ((1, f1, a1, b1), (2, f2, a2, b2)):
        e_one, e_new = float((a - f).abs().max()), float((b - f).abs().max())
        print("E %s hidden %d turn %d: E_one %.4e E_new %.4e ratio %.3f"
              % (str(dtype)[6:], hidden, turn, e_one, e_new, e_new / e_one))
        assert e_one > 0.0
        assert e_new <= 2.0 * e_one, (turn, e_one, e_new)


@pytest.mark.parametrize("hidden,dtype", [(128, torch.bfloat16), (256, torch.float16)])
def test_decode_after_chunked_prefill(hidden, dtype):
    """Graph-replayed decode steps after a chunked prefill and after an offset
    turn: shapes, ``lens`` / ``pending`` bookkeeping, the cache rows below
    ``lens`` finite."""
    m16, _ = _models(hidden, dtype)
    gen = _gen(m16, prefill_chunk=CHUNK, max_dec_len=5, use_hip_graph=True)
    s = gen.new_session(2)
    ids1, lens1 = _ragged(PROMPTS, 3)
    out1, sc1 = gen.generate(ids1.to(DEV), lens1.to(DEV), session=s)
    assert out1.shape == (2, 5) and sc1.shape == (2,) and bool(torch.isfinite(sc1).all())
    assert s.lens.tolist() == [n + 4 for n in PROMPTS]
    assert s.pending.tolist() == out1[:, -1].tolist()
    ids2, lens2 = _ragged([TURN2, 9], 4)
    out2, _ = gen.generate(ids2.to(DEV), lens2.to(DEV), session=s)
    assert out2.shape == (2, 5)
    want = [PROMPTS[0] + 4 + 1 + TURN2 + 4, PROMPTS[1] + 4 + 1 + 9 + 4]
    assert s.lens.tolist() == want and s._lens == want
    assert s.pending.tolist() == out2[:, -1].tolist()
    for b, n in enumerate(want):
        assert s.tokens[b, n - 5:n + 1].tolist()[1:] == out2[b].tolist()
        for li in range(2):
            assert bool(torch.isfinite(s.cache.k[li][b, :n].float()).all())
            assert bool(torch.isfinite(s.cache.v[li][b, :n].float()).all())
