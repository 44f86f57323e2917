"""Element-exact edge tests of the cross-entropy, embedding, GeLU, dropout and
LayerNorm kernels (MI355X only) against float64 references computed from the
same 16-bit inputs: odd sizes, tails, more than one block, both 16-bit types.

Every ``check_*`` function takes the device, so tests/test_eltwise_edges_cpu.py
holds the PyTorch formula branches of the wrappers (which also serve GPU
tensors the vector kernels cannot address) to the same references.

Tolerance of an elementwise result (``assert_elementwise``): one ulp of the
16-bit output type plus an absolute floor.  One rounding to the output type
is 0.5 ulp and the fp32 evaluation error in front of it can flip that
rounding; where the fp32 formula cancels (``1 + tanh(u)`` for negative u,
``softmax - onehot``, ``x / (1 - p) + r``) the fp32 error is absolute --
2^-24 relative to the terms of the add, a few operations deep -- and a
near-zero result's 16-bit ulps cannot express it.  Hence the floor
``2^-22 * (sum of the magnitudes of the terms of the last fp32 add)``,
``2^-20`` for gradients, which multiply by ``dy`` or ``g`` on top.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
_MANT = {torch.bfloat16: 7, torch.float16: 10}
_MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
K0, K1 = 0.7978845608028654, 0.044715


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fleetx_amd.ops import _lib
    _lib.kernels()  # fail loudly if the extension is missing
    torch.manual_seed(0)


# ------------------------------------------------------------------ helpers
def ulp(ref, dtype):
    """Spacing of ``dtype`` at ``ref`` (float64):
    ``2^(floor(log2 max(|ref|, smallest_normal)) - mant)``."""
    a = ref.double().abs().clamp_min(_MIN_NORMAL[dtype])
    _, e = torch.frexp(a)            # a = m * 2^e with m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 1 - _MANT[dtype])


def assert_elementwise(got, ref64, dtype, floor, what=""):
    """Every element: ``|got - ref| <= 1 ulp(ref) + floor``."""
    assert got.dtype == dtype, (what, got.dtype)
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    ref64 = ref64.double()
    err = (got.detach().double() - ref64).abs()
    tol = ulp(ref64, dtype) + floor
    bad = ~(err <= tol)              # a NaN is bad
    nbad = int(bad.sum())
    if nbad:
        over = torch.where(bad, torch.nan_to_num(err / tol, nan=math.inf), torch.zeros_like(err))
        i = int(over.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(
            "%s: %d of %d elements off; worst at %s: got %r ref %r err %.3e tol %.3e (ulp %.3e)"
            % (what, nbad, err.numel(), idx, float(got.detach().reshape(-1)[i]),
               float(ref64.reshape(-1)[i]), float(err.reshape(-1)[i]),
               float(tol.reshape(-1)[i]), float(ulp(ref64, dtype).reshape(-1)[i])))


def _rel_rows(got, ref):
    """Largest row-wise relative l2 error (never one norm over the tensor)."""
    g = got.detach().double().reshape(-1, got.shape[-1])
    r = ref.double().reshape(-1, ref.shape[-1])
    return float(((g - r).norm(dim=1) / (r.norm(dim=1) + 1e-12)).max())


def assert_colsum(got, terms64, dtype, what=""):
    """A 16-bit (or fp32) column sum against the float64 sum of its ``terms64``
    [rows, cols]: 1 ulp of the output type plus ``2^-22 * sum|terms|`` (fp32
    accumulation in another order)."""
    ref = terms64.sum(0)
    floor = 2.0 ** -22 * terms64.abs().sum(0)
    if got.dtype == torch.float32:
        err = (got.double() - ref).abs()
        tol = floor + 2.0 ** -23 * ref.abs()
        bad = ~(err <= tol)
        assert not bool(bad.any()), (what, int(bad.sum()), float((err - tol).max()))
    else:
        assert_elementwise(got, ref, dtype, floor, what)


# ------------------------------------------------------------ cross entropy
CE_ROWS = 67
CE_VS = [5, 8, 37, 2040, 2047, 2048, 2056, 2059, 4099]


def _ce_columns(V):
    cand = [0, 7, 8, 2047, 2048, V - V % 8 - 1, V - V % 8, V - 1]
    return [min(max(c, 0), V - 1) for c in cand]


def make_ce_case(V, dtype, dev, ignore_index=None):
    """randn logits [67, V] with a +6 peak per row on a column that cycles
    through the vector / tail boundaries, labels that visit the same columns
    (so a missed column moves the loss by far more than the tolerance)."""
    gen = torch.Generator().manual_seed(1000 + V)
    x = torch.randn(CE_ROWS, V, generator=gen)
    cols = _ce_columns(V)
    r = torch.arange(CE_ROWS)
    peak = torch.tensor(cols)[r % 8]
    x[r, peak] += 6.0
    labels = torch.tensor(cols)[(r + r // 8) % 8]
    if ignore_index is not None:
        labels[[0, 1, CE_ROWS - 1]] = ignore_index
    g = torch.rand(CE_ROWS, generator=gen) + 0.05
    return x.to(dtype).to(dev), labels.to(dev), g.to(dev)


def ce_reference(x, labels, g, vocab_start=0, ignore_index=-100):
    """float64 loss and logits gradient of one vocab shard (the whole
    vocabulary with ``vocab_start`` 0 and labels inside ``[0, V)``)."""
    x64 = x.double()
    rows, V = x64.shape
    lse = torch.logsumexp(x64, -1)
    local = labels - vocab_start
    inr = (local >= 0) & (local < V) & (labels != ignore_index)
    tg = torch.where(inr, x64.gather(1, local.clamp(0, V - 1)[:, None])[:, 0],
                     torch.zeros_like(lse))
    live = labels != ignore_index
    loss = torch.where(live, lse - tg, torch.zeros_like(lse))
    p = torch.exp(x64 - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[inr, local[inr]] = 1.0
    grad = (p - onehot) * (g.double() * live)[:, None]
    return loss, grad


def ce_loss_limit(x, labels, ref_loss, ignore_index):
    """8 x the deviation of torch's own float32 cross_entropy from the float64
    value on the same inputs (room for ``__expf``), floor 1e-5."""
    safe = torch.where(labels == ignore_index, torch.full_like(labels, -100), labels)
    f32 = F.cross_entropy(x.float(), safe, reduction="none", ignore_index=-100)
    r64 = F.cross_entropy(x.double(), safe, reduction="none", ignore_index=-100)
    assert torch.allclose(r64, ref_loss, rtol=0, atol=1e-12)
    return max(8.0 * float((f32.double() - r64).abs().max()), 1e-5)


def check_ce(dev, V, dtype, inplace, ignore_index):
    from fleetx_amd import ops
    x, labels, g = make_ce_case(V, dtype, dev, ignore_index)
    ref_loss, ref_grad = ce_reference(x, labels, g, 0, ignore_index)
    limit = ce_loss_limit(x, labels, ref_loss, ignore_index)
    leaf = x.clone().requires_grad_()
    loss = ops.softmax_cross_entropy(leaf.clone(), labels, ignore_index=ignore_index,
                                     inplace_backward=inplace)
    assert loss.dtype == torch.float32
    err = float((loss.detach().double() - ref_loss).abs().max())
    assert err <= limit, (err, limit)
    (loss * g).sum().backward()
    floor = (2.0 ** -20 * g.double())[:, None].expand_as(ref_grad)
    assert_elementwise(leaf.grad, ref_grad, dtype, floor, "dlogits V=%d" % V)
    ign = labels == ignore_index
    assert int(ign.sum()) == 3
    assert int(torch.count_nonzero(leaf.grad[ign])) == 0, "ignored rows must get exactly 0"


@pytest.mark.parametrize("ignore_index", [-100, -1])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", CE_VS)
def test_cross_entropy_edges(V, dtype, inplace, ignore_index):
    check_ce(DEV, V, dtype, inplace, ignore_index)


def check_ce_shards(dev, V, dtype):
    """A [67, 2V] vocabulary as two shards: the (max, sum, target) statistics
    combined as the wrapper combines them across ranks, and the public op on
    each shard with its ``vocab_start``."""
    from fleetx_amd import ops
    from fleetx_amd.ops.loss_embed import ce_local_stats
    x, labels, g = make_ce_case(2 * V, dtype, dev, -100)
    ref_loss, _ = ce_reference(x, labels, g)
    limit = ce_loss_limit(x, labels, ref_loss, -100)
    shards = [x[:, s * V:(s + 1) * V].contiguous() for s in (0, 1)]
    stats = [ce_local_stats(xs, labels, s * V, -100) for s, xs in enumerate(shards)]
    gmx = torch.maximum(stats[0][0], stats[1][0])
    sm = sum(st[1] * torch.exp(st[0] - gmx) for st in stats)
    tg = stats[0][2] + stats[1][2]
    loss = torch.where(labels == -100, torch.zeros_like(gmx), torch.log(sm) + gmx - tg)
    err = float((loss.detach().double() - ref_loss).abs().max())
    assert err <= limit, (err, limit)
    inside = [int((((labels - s * V) >= 0) & ((labels - s * V) < V)).sum()) for s in (0, 1)]
    assert min(inside) > 0, inside       # labels inside and outside each shard
    for s, xs in enumerate(shards):
        ref_l, ref_g = ce_reference(xs, labels, g, s * V, -100)
        # a label outside the shard has no torch cross_entropy; the target logit
        # is exact either way, so the float32 deviation is that of the
        # log-sum-exp: measured with every label on column 0
        zero = torch.zeros_like(labels)
        lim = ce_loss_limit(xs, zero, ce_reference(xs, zero, g)[0], -100)
        leaf = xs.clone().requires_grad_()
        out = ops.softmax_cross_entropy(leaf.clone(), labels, vocab_start=s * V)
        e = float((out.detach().double() - ref_l).abs().max())
        assert e <= lim, (s, e, lim)
        (out * g).sum().backward()
        floor = (2.0 ** -20 * g.double())[:, None].expand_as(ref_g)
        assert_elementwise(leaf.grad, ref_g, dtype, floor, "shard %d dlogits" % s)
        assert int(torch.count_nonzero(leaf.grad[labels == -100])) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", CE_VS)
def test_cross_entropy_vocab_shards(V, dtype):
    check_ce_shards(DEV, V, dtype)


# -inf logits (masked vocabulary) at V 4099: nv = 512 vectors, thread t owns
# vectors t and t + 256, threads 0..2 the scalar tail 4096..4098
NEG_INF_COLUMNS = {
    "first_vectors": list(range(0, 16)),
    "both_vectors_of_one_thread": list(range(24, 32)) + list(range(2072, 2080)),
    "scalar_tail": [4096, 4097, 4098],
}


def check_ce_neg_inf(dev, dtype, where, inplace=True):
    from fleetx_amd import ops
    V = 4099
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(CE_ROWS, V, generator=gen)
    r = torch.arange(CE_ROWS)
    peak = 100 + 7 * r
    x[r, peak] += 6.0
    labels = torch.where(r % 2 == 0, peak, 3000 + r)
    cols = torch.tensor(NEG_INF_COLUMNS[where])
    x[:, cols] = -math.inf
    g = torch.rand(CE_ROWS, generator=gen) + 0.05
    x, labels, g, cols = x.to(dtype).to(dev), labels.to(dev), g.to(dev), cols.to(dev)
    ref_loss, ref_grad = ce_reference(x, labels, g)
    assert bool(torch.isfinite(ref_loss).all())
    limit = ce_loss_limit(x, labels, ref_loss, -100)
    leaf = x.clone().requires_grad_()
    loss = ops.softmax_cross_entropy(leaf.clone(), labels, inplace_backward=inplace)
    err = (loss.detach().double() - ref_loss).abs()
    assert bool(torch.isfinite(loss).all()), "non-finite loss on rows %s" % (
        (~torch.isfinite(loss)).nonzero().reshape(-1).tolist()[:8],)
    assert float(err.max()) <= limit, (float(err.max()), limit)
    (loss * g).sum().backward()
    floor = (2.0 ** -20 * g.double())[:, None].expand_as(ref_grad)
    assert_elementwise(leaf.grad, ref_grad, dtype, floor, "dlogits -inf " + where)
    assert int(torch.count_nonzero(leaf.grad[:, cols])) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", sorted(NEG_INF_COLUMNS))
def test_cross_entropy_neg_inf_logits(where, dtype):
    check_ce_neg_inf(DEV, dtype, where)


# ---------------------------------------------------------------- embedding
EMB_HS = [8, 200, 512, 520, 1032]       # 520 / 1032: a second pass with idle lanes
EMB_RAGGED_HS = [13, 1001]              # routed: the forward kernel moves 8-wide vectors
EMB_NTOK = [1, 3, 5, 130]               # 4 tokens per block


def check_embedding_fwd(dev, h, dtype, with_pos):
    from fleetx_amd import ops
    V, NP = 50, 131
    gen = torch.Generator().manual_seed(h)
    W = torch.randn(V, h, generator=gen).to(dtype).to(dev)
    P = torch.randn(NP, h, generator=gen).to(dtype).to(dev)
    for ntok in EMB_NTOK:
        ids = torch.randint(0, V, (ntok,), generator=gen).to(dev)
        pos = torch.randint(0, NP, (ntok,), generator=gen).to(dev)
        if with_pos:
            out = ops.embedding(ids, W, pos, P)
            full = (W.float()[ids] + P.float()[pos]).to(dtype)
        else:
            out = ops.embedding(ids, W)
            full = W[ids]
        assert out.shape == (ntok, h) and out.dtype == dtype
        assert torch.equal(out, full), (h, ntok)
        # vocab shard [20, 40): rows outside it are the position rows alone (or 0)
        Ws = W[20:40].contiguous()
        inr = ((ids >= 20) & (ids < 40))[:, None]
        if with_pos:
            out2 = ops.embedding(ids, Ws, pos, P, vocab_start=20)
            ref2 = torch.where(inr, full, P[pos])
        else:
            out2 = ops.embedding(ids, Ws, vocab_start=20)
            ref2 = torch.where(inr, full, torch.zeros_like(full))
        assert torch.equal(out2, ref2), (h, ntok, "shard")


@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", EMB_HS + EMB_RAGGED_HS)
def test_embedding_forward_bitwise(h, dtype, with_pos):
    check_embedding_fwd(DEV, h, dtype, with_pos)


def check_embedding_bwd(dev, h, dtype, one_id):
    from fleetx_amd import ops
    V, NP, ntok = 200, 131, 130          # at most 130 of 200 rows referenced
    gen = torch.Generator().manual_seed(h + 1)
    W = torch.randn(V, h, generator=gen).to(dtype).to(dev).requires_grad_()
    P = torch.randn(NP, h, generator=gen).to(dtype).to(dev).requires_grad_()
    ids = torch.full((ntok,), 7) if one_id else torch.randint(0, V, (ntok,), generator=gen)
    pos = torch.randint(0, NP - 1, (ntok,), generator=gen)    # row NP - 1 never referenced
    ids, pos = ids.to(dev), pos.to(dev)
    out = ops.embedding(ids.view(2, 65), W, pos.view(2, 65), P)
    d = torch.randn(2, 65, h, generator=gen).to(dtype).to(dev)
    out.backward(d)
    d64 = d.double().reshape(ntok, h)
    for grad, idx, n in ((W.grad, ids, V), (P.grad, pos, NP)):
        ref = torch.zeros(n, h, dtype=torch.float64, device=dev).index_add_(0, idx, d64)
        mag = torch.zeros(n, h, dtype=torch.float64, device=dev).index_add_(0, idx, d64.abs())
        assert_elementwise(grad, ref, dtype, 2.0 ** -22 * mag, "embedding grad h=%d" % h)
        unused = torch.ones(n, dtype=torch.bool, device=dev)
        unused[idx] = False
        assert int(unused.sum()) > 0
        assert int(torch.count_nonzero(grad[unused])) == 0


@pytest.mark.parametrize("det", ["0", "1"])
@pytest.mark.parametrize("one_id", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [8, 200, 520, 13, 1001])
def test_embedding_backward(h, dtype, one_id, det, monkeypatch):
    if det == "1":
        monkeypatch.setenv("FLEETX_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("FLEETX_DETERMINISTIC", raising=False)
    check_embedding_bwd(DEV, h, dtype, one_id)


# -------------------------------------------------------------- bias + GeLU
# 136: one active column group in the second 128-column tile; 17 rows: one past
# the 16-row tile; 13 / 1001: ragged widths (routed to the formula branch)
GELU_SHAPES = [(1, 8), (3, 136), (17, 128), (33, 1000), (5, 2056), (5, 13), (33, 1001)]
PLANTED = [0.0, 0.75, -0.75, 6.0, -6.0, 12.0, -12.0, 30.0, -30.0, 100.0, -100.0]


def _place(t, dtype, dev, misalign=False):
    """``t`` as a contiguous ``dtype`` tensor on ``dev``; ``misalign``: a view
    that starts 8 bytes into its buffer (off the 16-byte vector boundary)."""
    t = t.to(dtype)
    if not misalign:
        return t.to(dev)
    buf = torch.empty(t.numel() + 4, dtype=dtype, device=dev)
    v = buf[4:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def make_gelu_case(rows, cols, dtype, dev, with_bias, misalign=False):
    gen = torch.Generator().manual_seed(rows * 10007 + cols)
    x = 2.0 * torch.randn(rows, cols, generator=gen)
    flat = x.view(-1)
    n = min(flat.numel(), len(PLANTED))
    flat[:n] = torch.tensor(PLANTED[:n])
    if flat.numel() >= 2 * len(PLANTED):      # and in the last vector of the last row
        flat[-len(PLANTED):] = torch.tensor(PLANTED)
    b = 0.1 * torch.randn(cols, generator=gen) if with_bias else None
    dy = torch.randn(rows, cols, generator=gen)
    x = _place(x, dtype, dev, misalign)
    dy = _place(dy, dtype, dev, misalign)
    if b is not None:
        b = _place(b, dtype, dev, misalign)
    return x, b, dy


def gelu_reference(t, erf):
    """float64 GeLU and derivative at ``t`` with, for each, the sum of the
    magnitudes of the terms of its last add (the floor's scale)."""
    if erf:
        e = torch.erf(t / math.sqrt(2.0))
        second = t * 0.3989422804014327 * torch.exp(-0.5 * t * t)
    else:
        u = K0 * (t + K1 * t ** 3)
        e = torch.tanh(u)
        second = 0.5 * t * (1.0 - e * e) * K0 * (1.0 + 3.0 * K1 * t * t)
    y = 0.5 * t * (1.0 + e)
    ymag = 0.5 * t.abs() * (1.0 + e.abs())
    d = 0.5 * (1.0 + e) + second
    dmag = 0.5 * (1.0 + e.abs()) + second.abs()
    return y, ymag, d, dmag


def check_bias_gelu(dev, rows, cols, dtype, erf, with_bias, misalign=False):
    from fleetx_amd import ops
    x, b, dy = make_gelu_case(rows, cols, dtype, dev, with_bias, misalign)
    x.requires_grad_()
    if b is not None:
        b.requires_grad_()
    t = x.detach().double() + (b.detach().double() if b is not None else 0.0)
    y64, ymag, d64, dmag = gelu_reference(t, erf)
    y = ops.bias_gelu(x, b, approximate=not erf)
    assert_elementwise(y, y64, dtype, 2.0 ** -22 * ymag, "gelu fwd")
    y.backward(dy)
    dy64 = dy.double()
    assert_elementwise(x.grad, dy64 * d64, dtype, 2.0 ** -20 * dy64.abs() * dmag, "gelu dx")
    if b is not None:
        # the bias gradient is the column sum of the dx that was returned
        assert_colsum(b.grad, x.grad.double(), dtype, "gelu dbias")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("erf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", GELU_SHAPES)
def test_bias_gelu_edges(rows, cols, dtype, erf, with_bias):
    check_bias_gelu(DEV, rows, cols, dtype, erf, with_bias)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_gelu_misaligned_view(dtype):
    """A view that starts off the 16-byte boundary takes the formula branch."""
    check_bias_gelu(DEV, 17, 128, dtype, False, True, misalign=True)


def check_gelu_plain_and_grad(dev, rows, cols, dtype, erf):
    from fleetx_amd.ops.elementwise import gelu_plain, gelu_grad
    x, _, dy = make_gelu_case(rows, cols, dtype, dev, False)
    y64, ymag, d64, dmag = gelu_reference(x.double(), erf)
    assert_elementwise(gelu_plain(x, erf), y64, dtype, 2.0 ** -22 * ymag, "gelu_plain")
    dy64 = dy.double()
    dx = gelu_grad(dy, x, erf)
    assert_elementwise(dx, dy64 * d64, dtype, 2.0 ** -20 * dy64.abs() * dmag, "gelu_grad")
    terms = dx.double()
    for acc in (False, True):
        dst = torch.full((cols,), 3.0, dtype=torch.float32, device=dev)   # finite sentinel
        dx2 = gelu_grad(dy, x, erf, colsum=(dst, acc))
        assert torch.equal(dx2, dx)
        ref = terms.sum(0) + (3.0 if acc else 0.0)
        tol = 2.0 ** -22 * (terms.abs().sum(0) + 3.0)
        err = (dst.double() - ref).abs()
        assert bool((err <= tol).all()), (acc, float((err - tol).max()))


@pytest.mark.parametrize("erf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", GELU_SHAPES)
def test_gelu_plain_and_grad_colsum(rows, cols, dtype, erf):
    check_gelu_plain_and_grad(DEV, rows, cols, dtype, erf)


# ------------------------------------------------------------------ dropout
def _away_from_zero(shape, gen):
    """Magnitudes in [1, 2) with random signs: a kept element can never be
    mistaken for a dropped one (0, or the bare residual)."""
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2.0 - 1.0
    return (sign * (1.0 + torch.rand(shape, generator=gen).double())).float()


def check_dropout(dev, shape, dtype, p):
    from fleetx_amd import ops
    from fleetx_amd.parallel import rng
    numel = math.prod(shape)
    key = 0x1234567 + numel
    gen = torch.Generator().manual_seed(numel)
    x = _away_from_zero(shape, gen).to(dtype).to(dev).requires_grad_()
    dy = _away_from_zero(shape, gen).to(dtype).to(dev)
    keep = rng.keep_mask(shape, p, key, dev)
    y = ops.dropout(x, p, key)
    y.backward(dy)
    for got, src, what in ((y, x.detach(), "dropout fwd"), (x.grad, dy, "dropout bwd")):
        assert got.shape == tuple(shape)
        assert torch.equal(got == 0, ~keep), what + ": dropped set differs from the mask"
        s64 = src.double()
        ref = torch.where(keep, s64 / (1.0 - p), torch.zeros_like(s64))
        assert_elementwise(got, ref, dtype, 2.0 ** -22 * s64.abs() / (1.0 - p), what)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1,), (7,), (8,), (9,), (16389,), (3, 5)])
def test_dropout_edges(shape, dtype, p):
    check_dropout(DEV, shape, dtype, p)


def check_bias_dropout_add(dev, rows, cols, dtype, p, with_bias, with_res, misalign=False):
    from fleetx_amd import ops
    from fleetx_amd.parallel import rng
    key = 0x5EED0000 + rows * 131071 + cols
    gen = torch.Generator().manual_seed(rows * 7919 + cols)
    x = _place(_away_from_zero((rows, cols), gen), dtype, dev, misalign).requires_grad_()
    b = r = None
    if with_bias:      # |b| < 0.5: |x + b| stays above 0.5
        b = _place((0.1 * torch.randn(cols, generator=gen)).clamp(-0.4, 0.4), dtype, dev,
                   misalign).requires_grad_()
    if with_res:
        r = _place(torch.randn(rows, cols, generator=gen), dtype, dev, misalign).requires_grad_()
    dy = _place(_away_from_zero((rows, cols), gen), dtype, dev, misalign)
    keep = rng.keep_mask((rows, cols), p, key, dev)
    out = ops.bias_dropout_add(x, b, r, p, key)
    x64 = x.detach().double()
    b64 = b.detach().double() if with_bias else torch.zeros(cols, dtype=torch.float64, device=dev)
    r64 = r.detach().double() if with_res else torch.zeros_like(x64)
    base = r.detach() if with_res else torch.zeros_like(out)
    # dropped outputs are the residual itself (or exactly 0), kept ones never are
    assert torch.equal(out == base, ~keep), "dropped set differs from the mask"
    ref = torch.where(keep, (x64 + b64) / (1.0 - p), torch.zeros_like(x64)) + r64
    floor = 2.0 ** -22 * (x64.abs() + b64.abs()) / (1.0 - p) + 2.0 ** -22 * r64.abs()
    assert_elementwise(out, ref, dtype, floor, "bias_dropout_add fwd")
    out.backward(dy)
    dy64 = dy.double()
    assert torch.equal(x.grad == 0, ~keep), "dx: dropped set differs from the mask"
    assert_elementwise(x.grad, torch.where(keep, dy64 / (1.0 - p), torch.zeros_like(dy64)), dtype,
                       2.0 ** -22 * dy64.abs() / (1.0 - p), "bias_dropout_add dx")
    if with_res:
        assert torch.equal(r.grad, dy)
    if with_bias:
        assert_colsum(b.grad, x.grad.double(), dtype, "bias_dropout_add dbias")


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1, 8), (17, 136), (33, 1000), (5, 13)])
def test_bias_dropout_add_edges(rows, cols, dtype, with_bias, with_res):
    check_bias_dropout_add(DEV, rows, cols, dtype, 0.1, with_bias, with_res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_dropout_add_misaligned_view(dtype):
    check_bias_dropout_add(DEV, 17, 136, dtype, 0.1, True, True, misalign=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_bwd_colsum_four_rows_in_flight(dtype):
    """(1300, 8192) gives each split more than 64 rows, so a thread of
    ``dropout_bwd_colsum_kernel`` runs its 4-rows-in-flight loop and then the
    single-row remainder."""
    from fleetx_amd.ops import _lib
    rows, cols = 1300, 8192
    splits = _lib.kernels().coltile_splits(rows, cols)
    assert -(-rows // splits) > 64, splits
    check_bias_dropout_add(DEV, rows, cols, dtype, 0.1, True, True)


# ---------------------------------------------------------------- LayerNorm
def _assert_cols(got, terms64, bound, what):
    """Per column: error of a column sum relative to the l2 norm of the terms
    that column sums (for one row: the plain relative error)."""
    err = (got.detach().double() - terms64.sum(0)).abs()
    lim = bound * terms64.norm(dim=0)
    bad = ~(err <= lim + 1e-300)
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / (lim + 1e-300)).max()))


def check_layer_norm(dev, rows, h, dtype, fused, misalign=False):
    """``layer_norm`` (``fused`` False) or ``add_layer_norm`` with bias,
    residual and dropout, against float64 autograd: the bounds of
    tests/test_kernels_gpu.py (1e-2 forward, 2e-2 backward) per row and, for
    dgamma / dbeta / dbias, per column."""
    from fleetx_amd import ops
    from fleetx_amd.parallel import rng
    eps, p, key = 1e-5, 0.1, 987654321 + h
    gen = torch.Generator().manual_seed(rows * 4099 + h)

    def mk(t):
        return _place(t, dtype, dev, misalign).requires_grad_()
    x = mk(torch.randn(rows, h, generator=gen))
    w = mk(1.0 + 0.1 * torch.randn(h, generator=gen))
    b = mk(0.1 * torch.randn(h, generator=gen))
    gy = _place(torch.randn(rows, h, generator=gen), dtype, dev, misalign)
    w64, b64 = w.detach().double(), b.detach().double()
    if fused:
        bias = mk(0.1 * torch.randn(h, generator=gen))
        res = mk(torch.randn(rows, h, generator=gen))
        gs = _place(torch.randn(rows, h, generator=gen), dtype, dev, misalign)
        keep = rng.keep_mask((rows, h), p, key, dev)
        s, y = ops.add_layer_norm(x, bias, res, w, b, eps, p, key)
        s64 = torch.where(keep, (x.detach().double() + bias.detach().double()) / (1.0 - p),
                          torch.zeros(rows, h, dtype=torch.float64, device=dev)) \
            + res.detach().double()
        assert s.dtype == dtype and _rel_rows(s, s64) < 1e-2
        # y = LN(s) of the sum as stored: the reference normalises the returned s
        sin = s.detach().double().requires_grad_()
    else:
        y = ops.layer_norm(x, w, b, eps)
        sin = x.detach().double().requires_grad_()
    y64 = F.layer_norm(sin, (h,), w64, b64, eps)
    assert y.dtype == dtype and _rel_rows(y, y64.detach()) < 1e-2
    y64.backward(gy.double())
    ds64 = sin.grad
    if fused:
        torch.autograd.backward([s, y], [gs, gy])
        ds64 = ds64 + gs.double()
        assert _rel_rows(res.grad, ds64) < 2e-2
        dx64 = torch.where(keep, ds64 / (1.0 - p), torch.zeros_like(ds64))
        assert torch.equal(x.grad == 0, ~keep | (dx64 == 0))
        _assert_cols(bias.grad, dx64, 2e-2, "dbias")
    else:
        y.backward(gy)
        dx64 = ds64
    assert _rel_rows(x.grad, dx64) < 2e-2
    sd = sin.detach()
    mean = sd.mean(-1, keepdim=True)
    xhat = (sd - mean) * torch.rsqrt(((sd - mean) ** 2).mean(-1, keepdim=True) + eps)
    _assert_cols(w.grad, gy.double() * xhat, 2e-2, "dgamma")
    _assert_cols(b.grad, gy.double(), 2e-2, "dbeta")


def check_col_sum(dev, rows, cols, dtype):
    from fleetx_amd.ops.norm import col_sum, col_sum_f32
    gen = torch.Generator().manual_seed(rows * 31 + cols)
    x = torch.randn(rows, cols, generator=gen).to(dtype).to(dev)
    x64 = x.double()
    assert_colsum(col_sum(x, cols), x64, dtype, "col_sum")
    for acc in (False, True):
        dst = torch.full((cols,), 3.0, dtype=torch.float32, device=dev)   # finite sentinel
        col_sum_f32(x, dst, accumulate=acc)
        err = (dst.double() - x64.sum(0) - (3.0 if acc else 0.0)).abs()
        tol = 2.0 ** -22 * (x64.abs().sum(0) + 3.0)
        assert bool((err <= tol).all()), (acc, float((err - tol).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1, 8), (17, 136), (33, 1000), (5, 13), (33, 1001)])
def test_col_sum_edges(rows, cols, dtype):
    check_col_sum(DEV, rows, cols, dtype)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("h", [13, 1001])
def test_layer_norm_ragged_width(h, rows, dtype, fused):
    check_layer_norm(DEV, rows, h, dtype, fused)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("rows", [5, 37])
@pytest.mark.parametrize("h", [1024, 1408, 4104])
def test_layer_norm_fp16(h, rows, fused):
    check_layer_norm(DEV, rows, h, torch.float16, fused)


def test_layer_norm_misaligned_view():
    check_layer_norm(DEV, 5, 1024, torch.bfloat16, True, misalign=True)
