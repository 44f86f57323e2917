"""``fa_fwd_qoff_split_kernel`` + ``fa_split_combine_kernel`` through
``ops.prefill_attention(..., nsplit=)`` on the MI355X, held to the float64
embedded reference and a-priori bounds of tests/test_prefill_attention_cpu.py
(fp32 partials, one rounding at the combine: the unsplit kernel's bounds).
Measured E pairs of ``test_session_turn_error``: profiles/prefill_split/README.md."""
import math

import pytest
import torch

from tests import test_attention_edges_gpu as A
from tests import test_prefill_attention_cpu as C
from tests import test_prefill_chunk_gpu as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fleetx_amd.ops import _lib
    _lib.kernels()  # fail loudly if the extension is missing
    torch.manual_seed(0)


def check(St, Sq, q_starts, D, dtype, inputs, kv_lens=None, **split):
    from fleetx_amd import ops
    c, qb, k, v, lens, ref = C.embedded(DEV, St, Sq, q_starts, D, dtype, inputs,
                                        kv_lens or [St] * len(q_starts))
    qs = torch.tensor(q_starts, dtype=torch.int32, device=DEV)
    out, lse = ops.prefill_attention(qb, k, v, qs, lens, scale=c.scale, return_lse=True, **split)
    C.compare(ref, out, lse, dtype, "%r Sq=%d q_starts=%s %s" % (c, Sq, q_starts, split))
    return out, lse


@pytest.mark.parametrize("nsplit", [2, 3, 5])
@pytest.mark.parametrize("D", [64, 88, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_embedded(dtype, D, nsplit):
    """4 tiles: nsplit 5 leaves empty splits, position 0 all but one; Sq 129 has
    waves above a split's range.  D 88: the 96 x 3 row, and 96 x 4 at Sq 200."""
    for inputs in ("peaked", "probe"):
        for Sq, q_starts in C.SHAPES + ([(200, [0, 0])] if D == 88 else []):
            check(C.ST, Sq, q_starts, D, dtype, inputs, nsplit=nsplit)
            check(C.ST, Sq, q_starts, D, dtype, inputs, nsplit=nsplit,
                  kv_lens=C.diagonal_binds(C.ST, Sq, q_starts))


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_three_query_blocks(D, dtype):
    """A block's diagonal tiles fall into two splits; min_split_tiles clips trailing splits."""
    for inputs in ("peaked", "probe"):
        check(640, 300, [1, 340], D, dtype, inputs, nsplit=3)
        check(640, 300, [1, 340], D, dtype, inputs, nsplit=5, min_split_tiles=4)


@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (128, torch.bfloat16)])
def test_empty_sample_and_padding_chunk(D, dtype):
    out, lse = check(C.ST, 33, [0, 40], D, dtype, "random", kv_lens=[0, 100], nsplit=3)
    assert int(torch.count_nonzero(out[0])) == 0
    assert bool((lse[0] == math.inf).all())
    out, _ = check(C.ST, 50, [150, 10], D, dtype, "peaked", kv_lens=[120, 200], nsplit=3)
    assert bool(torch.isfinite(out.float()).all())


def _raw(K, q, k, v, out, lse, qs, kl, ws_o, ws_ml, nsplit, min_tiles=1):
    from fleetx_amd.ops import _lib, attention as OA
    B, Sq, H, D = q.shape
    p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
    return K.flash_fwd_qoff_split(_lib.dt_code(q.dtype), p(q), p(k), p(v), p(out), p(lse),
                                  OA._strides(q), OA._strides(k), OA._strides(v),
                                  OA._strides(out), p(qs), p(kl), B, H, Sq, k.shape[1], D,
                                  1.0 / math.sqrt(D), p(ws_o), p(ws_ml), nsplit, min_tiles,
                                  _lib.stream())


@pytest.mark.parametrize("D,dtype", [(88, torch.bfloat16), (128, torch.float16)])
def test_workspace_and_cache_hygiene(D, dtype):
    """NaN in both workspaces and in every cache row at or past kv_len; O and lse
    carved out of sentinel buffers, which the reject codes leave intact."""
    from fleetx_amd.ops import _lib
    K = _lib.kernels()
    Sq, q_starts, G, ns = 129, [0, 64], 64, 5
    c, qb, k, v, lens, ref = C.embedded(DEV, C.ST, Sq, q_starts, D, dtype, "peaked", [150, C.ST])
    B, H = c.B, c.H
    kc = torch.full((B, 256, H, D), math.nan, device=DEV, dtype=dtype)
    vc = torch.full((B, 256, H, D), math.nan, device=DEV, dtype=dtype)
    for b in range(B):
        kc[b, :int(lens[b])], vc[b, :int(lens[b])] = k[b, :int(lens[b])], v[b, :int(lens[b])]
    big = torch.full((B, Sq + 2, H, D + 8), 3.0, device=DEV, dtype=dtype)
    stat = torch.full((G + B * H * Sq + G,), -7777.0, device=DEV)
    out, lse = big[:, 1:Sq + 1, :, :D], stat[G:G + B * H * Sq]
    ws_o = torch.full((B * H * ns * Sq * (96 if D == 88 else 128),), math.nan, device=DEV)
    ws_ml = torch.full((B * H * ns * Sq * 2,), math.nan, device=DEV)
    qs = torch.tensor(q_starts, dtype=torch.int32, device=DEV)
    inner = torch.zeros(B, Sq + 2, H, D + 8, dtype=torch.bool, device=DEV)
    inner[:, 1:Sq + 1, :, :D] = True

    assert _raw(K, qb, kc, vc, out, lse, qs, lens, ws_o, ws_ml, 1) == -2
    assert _raw(K, qb, kc, vc, out, lse, qs, lens, ws_o, ws_ml, ns, min_tiles=0) == -2
    assert _raw(K, qb, kc, vc, out, lse, None, lens, ws_o, ws_ml, ns) == -5
    assert _raw(K, qb, kc, vc, out, lse, qs, lens, None, ws_ml, ns) == -6
    assert _raw(K, qb, kc, vc, out, lse, qs, lens, ws_o, None, ns) == -6
    torch.cuda.synchronize()
    assert bool((big == 3.0).all()) and bool((stat == -7777.0).all())
    assert _raw(K, qb, kc, vc, out, lse, qs, lens, ws_o, ws_ml, ns) == 0
    torch.cuda.synchronize()
    assert bool((big[~inner] == 3.0).all()), "guard elements written"
    assert bool((stat[:G] == -7777.0).all()) and bool((stat[-G:] == -7777.0).all())
    C.compare(ref, out, lse.view(B, H, Sq), dtype, "sentinels")


def test_graph_replay_reads_the_arrays():
    """One captured nsplit 3 call follows q, q_starts and kv_lens: ranges are device-side."""
    from fleetx_amd import ops
    Sq, D, dtype = 70, 64, torch.bfloat16
    c, qa, k, v, lens, ref_a = C.embedded(DEV, C.ST, Sq, [65, 130], D, dtype, "random",
                                          [C.ST, C.ST])
    _, qb, k2, v2, _, ref_b = C.embedded(DEV, C.ST, Sq, [3, 90], D, dtype, "random", [C.ST, 150])
    assert torch.equal(k, k2) and torch.equal(v, v2)
    q = qa.clone()
    qs = torch.tensor([65, 130], dtype=torch.int32, device=DEV)
    kl = torch.tensor([C.ST, C.ST], dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.prefill_attention(q, k, v, qs, kl, scale=c.scale, nsplit=3)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = ops.prefill_attention(q, k, v, qs, kl, scale=c.scale, return_lse=True, nsplit=3)
    for qn, starts, lens_n, ref in ((qa, [65, 130], [C.ST, C.ST], ref_a),
                                    (qb, [3, 90], [C.ST, 150], ref_b)):
        q.copy_(qn)
        qs.copy_(torch.tensor(starts, dtype=torch.int32))
        kl.copy_(torch.tensor(lens_n, dtype=torch.int32))
        for _ in range(2):
            graph.replay()
            C.compare(ref, out, lse, dtype, "replay %s" % starts)


def test_rule():
    from fleetx_amd import ops
    from fleetx_amd.ops.attention import prefill_splits
    assert all(prefill_splits(2, 3, Sq, maxlen, 128) == 1
               for maxlen in (200, 256, 512, 640) for Sq in (1, 65, 129, 512))
    for maxlen in (640, 4096, 8192):
        assert prefill_splits(8, 32, 65, maxlen, 128) == 1       # 256 blocks
        assert prefill_splits(1, 32, 1024, maxlen, 64) == 1
    assert prefill_splits(1, 16, 65, 4096, 128) > 1
    c, qb, k, v, lens, _ = C.embedded(DEV, C.ST, 70, [65, 130], 64, torch.bfloat16, "peaked",
                                      [C.ST, C.ST])
    qs = torch.tensor([65, 130], dtype=torch.int32, device=DEV)
    one = ops.prefill_attention(qb, k, v, qs, lens, scale=c.scale, return_lse=True, nsplit=1)
    auto = ops.prefill_attention(qb, k, v, qs, lens, scale=c.scale, return_lse=True)
    assert torch.equal(one[0], auto[0]) and torch.equal(one[1], auto[1])


def _models(hidden, dtype):  # PC._models with a 2048-row session cache, so that the rule splits
    torch.manual_seed(hidden)
    kw = dict(vocab_size=PC.V, hidden_size=hidden, num_layers=2, num_attention_heads=2,
              max_position_embeddings=2048, hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0)
    m16 = PC.GPTForPretraining(PC.GPTConfig(dtype=dtype, **kw))
    with torch.no_grad():
        for p in (p for p in m16.parameters() if p.ndim == 1):
            p.add_((0.05 * torch.randn(p.shape)).to(device=p.device, dtype=p.dtype))
    m32 = PC.GPTForPretraining(PC.GPTConfig(dtype=torch.float32, **kw))
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16.to(DEV).eval(), m32.cpu().eval()


@pytest.mark.parametrize("prompts", [PC.PROMPTS, [700, 330]])
@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_session_turn_error(dtype, hidden, prompts):
    """A 70-token turn on a session takes the split path: E_new <= 2 E_one against
    the one-pass prefill of the transcript (tests/test_prefill_chunk_gpu.py).  The
    rule's 4 splits of at least 4 tiles: 220 keys lie in the first, 770 in all four."""
    from fleetx_amd.ops import attention as OA
    m16, m32 = _models(hidden, dtype)
    ids1, lens1 = PC._ragged(prompts, 1)
    ids2, lens2 = PC._ragged([PC.TURN2, PC.TURN2], 2)
    both = torch.zeros(2, max(prompts) + PC.TURN2, dtype=torch.long)
    for b, n in enumerate(prompts):
        both[b, :n] = ids1[b, :n]
        both[b, n:n + PC.TURN2] = ids2[b]
    one, ref = PC._gen(m16), PC._gen(m32)
    s_new, s_ref = one.new_session(2), ref.new_session(2)
    assert OA.prefill_splits(2, 2, PC.TURN2, s_new.max_len, hidden // 2) > 1
    PC._prefill_logits(ref, s_ref, ids1, lens1, "cpu")
    PC._prefill_logits(one, s_new, ids1, lens1, DEV)
    f2 = PC._prefill_logits(ref, s_ref, ids2, lens2, "cpu")
    a2 = PC._prefill_logits(one, one.new_session(2), both, lens1 + PC.TURN2, DEV)
    b2 = PC._prefill_logits(one, s_new, ids2, lens2, DEV)
    e_one, e_new = float((a2 - f2).abs().max()), float((b2 - f2).abs().max())
    print("E %s hidden %d prompts %s: E_one %.4e E_new %.4e"
          % (str(dtype)[6:], hidden, prompts, e_one, e_new))
    assert 0.0 < e_one and e_new <= 2.0 * e_one, (e_one, e_new)
