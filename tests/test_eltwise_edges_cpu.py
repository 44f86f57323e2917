"""The PyTorch formula branches of the cross-entropy, embedding, GeLU, dropout
and LayerNorm wrappers against the float64 references and tolerances of
tests/test_eltwise_edges_gpu.py.  These branches serve CPU tensors and every
GPU tensor the 16-byte-vector kernels cannot address (ragged width, buffer off
a 16-byte boundary), so they are held to the same element-exact checks."""
import pytest
import torch

from tests import test_eltwise_edges_gpu as E

DTYPES = E.DTYPES
CPU = "cpu"


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


# ------------------------------------------------------------------ helpers
def test_ulp_matches_the_number_formats():
    for dtype in DTYPES:
        fi = torch.finfo(dtype)
        v = torch.tensor([1.0, 1.5, 2.0, 0.75, 100.0, -6.0, 0.0, fi.tiny, fi.tiny / 4],
                         dtype=torch.float64)
        u = E.ulp(v, dtype)
        assert float(u[0]) == fi.eps and float(u[1]) == fi.eps and float(u[2]) == 2 * fi.eps
        assert float(u[3]) == fi.eps / 2
        nxt = torch.nextafter(torch.tensor(100.0, dtype=dtype), torch.tensor(200.0, dtype=dtype))
        assert float(u[4]) == float(nxt) - 100.0
        assert float(u[5]) == 4 * fi.eps
        # at and below the smallest normal: the subnormal spacing
        assert float(u[6]) == float(u[7]) == float(u[8]) == fi.tiny * fi.eps


def test_assert_elementwise_sees_one_wrong_element():
    ref = torch.randn(67, 50, dtype=torch.float64)
    got = ref.to(torch.bfloat16)
    zero = torch.zeros_like(ref)
    E.assert_elementwise(got, ref, torch.bfloat16, zero)
    bad = got.clone()
    bad[66, 49] = torch.nextafter(torch.nextafter(bad[66, 49], torch.tensor(9.0).bfloat16()),
                                  torch.tensor(9.0).bfloat16())
    with pytest.raises(AssertionError, match=r"1 of 3350 elements off; worst at \(66, 49\)"):
        E.assert_elementwise(bad, ref, torch.bfloat16, zero)
    bad = got.clone()
    bad[3, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \(3, 0\)"):
        E.assert_elementwise(bad, ref, torch.bfloat16, zero)


# ------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("ignore_index", [-100, -1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", E.CE_VS)
def test_cross_entropy_cpu(V, dtype, ignore_index):
    E.check_ce(CPU, V, dtype, False, ignore_index)


def test_cross_entropy_ignored_row_gets_zero_gradient_under_sum():
    """``softmax_cross_entropy(x, labels).sum().backward()``: upstream gradient
    1 on every row, ignored rows included."""
    from fleetx_amd import ops
    x = torch.randn(6, 37).requires_grad_()
    labels = torch.tensor([3, -100, 36, 0, -100, 8])
    ops.softmax_cross_entropy(x, labels).sum().backward()
    xr = x.detach().clone().requires_grad_()
    torch.nn.functional.cross_entropy(xr, labels, reduction="none", ignore_index=-100).sum().backward()
    assert int(torch.count_nonzero(x.grad[labels == -100])) == 0
    assert torch.allclose(x.grad, xr.grad, atol=1e-6, rtol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [5, 37, 2047, 2056])
def test_cross_entropy_vocab_shards_cpu(V, dtype):
    E.check_ce_shards(CPU, V, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", sorted(E.NEG_INF_COLUMNS))
def test_cross_entropy_neg_inf_logits_cpu(where, dtype):
    E.check_ce_neg_inf(CPU, dtype, where)


def test_lm_head_ce_ignored_rows_cpu():
    """The chunked LM head's CPU branch: an ignored row whose mask is 1 adds
    nothing to the hidden-state gradient or to the tied weight's gradient."""
    from fleetx_amd.ops import lm_head_ce
    T, H, V = 10, 16, 37
    h2 = torch.randn(T, H).requires_grad_()
    W = torch.nn.Parameter(0.3 * torch.randn(V, H))
    W.main_grad = torch.zeros(V, H)
    W._fx_fused_wgrad, W._fx_fresh = True, True
    labels = torch.randint(0, V, (T,))
    labels[[0, 4, 9]] = -100
    mask = torch.ones(T)
    lm_head_ce.declare_grad_scale(None, 1)
    loss = lm_head_ce.lm_head_cross_entropy(h2, W, labels, mask, chunk=4)
    loss.backward()
    lm_head_ce.check()
    hr, Wr = h2.detach().clone().requires_grad_(), W.detach().clone().requires_grad_()
    ref = torch.nn.functional.cross_entropy(hr @ Wr.t(), labels, reduction="sum",
                                            ignore_index=-100) / T
    ref.backward()
    assert torch.allclose(loss, ref, atol=1e-5)
    assert int(torch.count_nonzero(h2.grad[labels == -100])) == 0
    assert torch.allclose(h2.grad, hr.grad, atol=1e-5)
    assert torch.allclose(W.main_grad, Wr.grad, atol=1e-5)


# ---------------------------------------------------------------- embedding
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [8, 520] + E.EMB_RAGGED_HS)
def test_embedding_forward_cpu(h, dtype, with_pos):
    E.check_embedding_fwd(CPU, h, dtype, with_pos)


@pytest.mark.parametrize("one_id", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [8] + E.EMB_RAGGED_HS)
def test_embedding_backward_cpu(h, dtype, one_id):
    E.check_embedding_bwd(CPU, h, dtype, one_id)


# ----------------------------------------------------- GeLU, dropout, LayerNorm
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("erf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", E.GELU_SHAPES)
def test_bias_gelu_cpu(rows, cols, dtype, erf, with_bias):
    E.check_bias_gelu(CPU, rows, cols, dtype, erf, with_bias)


@pytest.mark.parametrize("erf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(3, 136), (5, 13), (33, 1001)])
def test_gelu_plain_and_grad_colsum_cpu(rows, cols, dtype, erf):
    E.check_gelu_plain_and_grad(CPU, rows, cols, dtype, erf)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1,), (7,), (9,), (16389,), (3, 5)])
def test_dropout_cpu(shape, dtype, p):
    E.check_dropout(CPU, shape, dtype, p)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(17, 136), (5, 13), (33, 1001)])
def test_bias_dropout_add_cpu(rows, cols, dtype, with_bias, with_res):
    E.check_bias_dropout_add(CPU, rows, cols, dtype, 0.1, with_bias, with_res)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("h", [13, 1001, 1024])
def test_layer_norm_cpu(h, rows, dtype, fused):
    E.check_layer_norm(CPU, rows, h, dtype, fused)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(17, 136), (5, 13), (33, 1001)])
def test_col_sum_cpu(rows, cols, dtype):
    E.check_col_sum(CPU, rows, cols, dtype)


# ------------------------------------------------------- the routing guard
class _FakeGpuTensor:
    """What ``vec8_ok`` looks at, without a GPU."""

    def __init__(self, ptr, cuda=True):
        self.is_cuda, self._ptr = cuda, ptr

    def data_ptr(self):
        return self._ptr


def test_vec8_ok_routes_ragged_widths_and_misaligned_buffers():
    from fleetx_amd.ops import _lib
    a, b = _FakeGpuTensor(4096), _FakeGpuTensor(4096 + 16)
    assert _lib.vec8_ok(8, a, None, b) and _lib.vec8_ok(1000, a)
    for width in (13, 1001, 1, 7, 12):
        assert not _lib.vec8_ok(width, a, b)
    for off in (2, 4, 8, 14):
        assert not _lib.vec8_ok(1024, a, _FakeGpuTensor(4096 + off))
    assert not _lib.vec8_ok(1024, a, _FakeGpuTensor(4096, cuda=False))
    assert not _lib.vec8_ok(8, torch.zeros(8))


def test_wrappers_consult_the_guard(monkeypatch):
    """Every wrapper of a 16-byte-vector kernel asks ``vec8_ok`` with the row
    width before it would launch: with CPU tensors the guard is the only
    thing between the call and a kernel launch, so the widths it was asked
    about are the record."""
    from fleetx_amd import ops
    from fleetx_amd.ops import _lib, norm
    from fleetx_amd.ops.elementwise import gelu_plain, gelu_grad
    seen = []
    real = _lib.vec8_ok

    def spy(width, *ts):
        seen.append(width)
        return real(width, *ts)
    monkeypatch.setattr(_lib, "vec8_ok", spy)
    x = torch.randn(5, 13).bfloat16().requires_grad_()
    b = torch.randn(13).bfloat16().requires_grad_()
    w = torch.ones(13).bfloat16().requires_grad_()

    def used(fn):
        del seen[:]
        fn()
        assert seen and all(wd == 13 for wd in seen), seen
    used(lambda: ops.bias_gelu(x, b).sum().backward())
    used(lambda: gelu_plain(x.detach()))
    used(lambda: gelu_grad(x.detach(), x.detach()))
    used(lambda: ops.bias_dropout_add(x, b, x.detach(), 0.1, 5).sum().backward())
    used(lambda: ops.layer_norm(x, w, b).sum().backward())
    used(lambda: sum(t.sum() for t in ops.add_layer_norm(x, b, x.detach(), w, b)).backward())
    used(lambda: norm.col_sum(x.detach(), 13))
    used(lambda: norm.col_sum_f32(x.detach(), torch.zeros(13)))
    used(lambda: ops.embedding(torch.tensor([1, 2]), x.detach()))
