"""The gradient sink (``parallel.grad_sink``): the protocol by which an op
writes a parameter gradient straight into ``main_grad``, checked on its own,
through the formula branches of every producer, and through the two hooks."""
import pytest
import torch

DTYPES = [torch.float32, torch.bfloat16]
ROWS = 24


def _param(shape, dtype=torch.float32, fused=True, ready=True):
    """A hand-made parameter as a gradient buffer would leave it: ``main_grad``
    holds stale 7.0, the step is fresh, readiness reports are recorded."""
    p = torch.nn.Parameter(torch.randn(*shape).to(dtype))
    p.main_grad = torch.full(shape, 7.0)
    p._fx_fresh = True
    p._fx_fused_wgrad = fused
    p.fired = []
    if ready:
        p._fx_grad_ready = lambda: p.fired.append(1)
    return p


# ------------------------------------------------------------------ the protocol
@pytest.mark.parametrize("dtype", DTYPES)
def test_open_close_overwrites_then_accumulates(dtype):
    from fleetx_amd.parallel import grad_sink as sink
    p = _param((5,), dtype)
    g = torch.arange(5.0)
    mg, acc = sink.open_write(p)
    assert mg is p.main_grad and acc is False and p._fx_fresh   # open changes nothing
    sink.store_or_add(mg, g, acc)
    sink.close_write(p)
    assert torch.equal(p.main_grad, g)                           # the 7.0 is gone
    assert p._fx_fresh is False and len(p.fired) == 1
    mg, acc = sink.open_write(p)
    assert acc is True
    sink.store_or_add(mg, g, acc)
    sink.close_write(p)
    assert torch.equal(p.main_grad, 2 * g) and len(p.fired) == 2


def test_close_without_notify_reports_later():
    from fleetx_amd.parallel import grad_sink as sink
    p = _param((3,))
    sink.close_write(p, notify=False)
    assert p._fx_fresh is False and p.fired == []
    sink.grad_part_done(p)
    assert len(p.fired) == 1


def test_tied_weight_reports_after_its_last_part():
    from fleetx_amd.parallel import grad_sink as sink
    p = _param((3,))
    p._fx_grad_parts = 2
    for closes in range(1, 5):
        sink.close_write(p)
        assert len(p.fired) == closes // 2
        if closes % 2 == 0:
            assert p._fx_parts_seen == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_deliver(dtype):
    from fleetx_amd.parallel import grad_sink as sink
    g = torch.arange(5.0) / 3
    p = _param((5,), dtype)
    assert sink.deliver(p, g, dtype) is None
    assert torch.equal(p.main_grad, g) and len(p.fired) == 1 and not p._fx_fresh
    # a parameter that does not take fused gradients, and a CPU gradient under
    # the on_gpu condition: returned for autograd, nothing else happens
    for p, kw in ((_param((5,), dtype, fused=False), {}), (_param((5,), dtype), {"on_gpu": True})):
        out = sink.deliver(p, g, dtype, **kw)
        assert out.dtype == dtype and torch.equal(out, g.to(dtype))
        assert torch.equal(p.main_grad, torch.full((5,), 7.0))
        assert p.fired == [] and p._fx_fresh


def test_named_predicates_differ_from_the_default():
    from fleetx_amd.parallel import grad_sink as sink
    p = _param((4,))
    assert sink.fused(p) and sink.in_buffer(p) and sink.fused(p, fp32_contiguous=True)
    assert not sink.fused(None) and not sink.in_buffer(None)
    # in a buffer without having opted into fused gradients (the fused MLP's FC1 bias)
    q = _param((4,), fused=False)
    assert not sink.fused(q) and sink.in_buffer(q)
    # fused but outside a buffer: no readiness callback
    q = _param((4,), ready=False)
    assert sink.fused(q) and not sink.in_buffer(q)
    # 16-bit gradient storage
    q = _param((4,))
    q.main_grad = q.main_grad.bfloat16()
    assert sink.fused(q) and not sink.fused(q, fp32_contiguous=True)
    # a strided main_grad
    q = _param((4,))
    q.main_grad = torch.full((4, 2), 7.0)[:, 0]
    assert sink.fused(q) and not sink.fused(q, fp32_contiguous=True)
    # the gradient's device
    assert not sink.fused(p, on_gpu=torch.zeros(1))


# ------------------------------------------------------------------ through the ops
# Each producer's formula branch runs on the same input with plain parameters
# (the gradient arrives in ``.grad``) and with parameters that take direct
# writes.  ``direct`` names those whose ``main_grad`` the op itself writes on
# the CPU; add_layer_norm and bias_dropout_add write it on the GPU only, on
# the CPU they hand their tensor to the buffer's hook, so those two run
# through a FlatParamGradBuffer (``direct`` empty).
def _linear(w, dtype, mk):
    from fleetx_amd.parallel.linear import linear
    x = torch.randn(2, ROWS // 2, w).to(dtype)
    prm = {"weight": mk((w, w)), "bias": mk((w,))}
    return prm, lambda: linear(x, prm["weight"], prm["bias"])


def _fused_mlp(w, dtype, mk):
    from fleetx_amd.parallel.linear import fused_mlp
    x = torch.randn(ROWS, w).to(dtype).requires_grad_()
    # FC1's bias lives in the buffer without having opted into fused gradients
    prm = {"w1": mk((2 * w, w)), "b1": mk((2 * w,), fused=False), "w2": mk((w, 2 * w))}
    return prm, lambda: fused_mlp(x, prm["w1"], prm["b1"], prm["w2"])


def _embedding(w, dtype, mk):
    from fleetx_amd.ops.loss_embed import embedding
    ids = torch.randint(0, 11, (2, ROWS // 2))
    pos = torch.arange(ROWS // 2).expand(2, -1)
    prm = {"word": mk((11, w)), "pos": mk((ROWS // 2, w))}
    return prm, lambda: embedding(ids, prm["word"], pos, prm["pos"])


def _add_layer_norm(w, dtype, mk):
    from fleetx_amd.ops.norm import add_layer_norm
    x, res = torch.randn(ROWS, w).to(dtype), torch.randn(ROWS, w).to(dtype)
    prm = {"bias": mk((w,)), "ln_w": mk((w,)), "ln_b": mk((w,))}

    def fwd():
        s, y = add_layer_norm(x, prm["bias"], res, prm["ln_w"], prm["ln_b"], 1e-5, 0.1, 4321)
        return s * 0.5 + y
    return prm, fwd


def _bias_dropout_add(w, dtype, mk):
    from fleetx_amd.ops.elementwise import bias_dropout_add
    x, res = torch.randn(ROWS, w).to(dtype), torch.randn(ROWS, w).to(dtype)
    prm = {"bias": mk((w,))}
    return prm, lambda: bias_dropout_add(x, prm["bias"], res, 0.1, 4321)


def _backward(fwd):
    """Upstream gradient in eighths: the embedding's scatter-add, the one
    producer that always accumulates onto ``main_grad``, then sums exactly, so
    that a second backward doubles it bitwise whatever the order of its adds."""
    y = fwd()
    torch.manual_seed(1)
    y.backward((torch.randint(-8, 9, y.shape) / 8).to(y.dtype))


PRODUCERS = [(_linear, True), (_fused_mlp, True), (_embedding, True),
             (_add_layer_norm, False), (_bias_dropout_add, False)]


@pytest.mark.parametrize("width", [16, 13])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("producer,direct", PRODUCERS, ids=[f.__name__[1:] for f, _ in PRODUCERS])
def test_fused_gradients_match_plain_through_the_ops(producer, direct, dtype, width):
    from fleetx_amd.parallel.grad_buffer import FlatParamGradBuffer

    def plain(shape, fused=True):
        return torch.nn.Parameter(torch.randn(*shape).to(dtype))

    def sinked(shape, fused=True):
        if direct:
            return _param(shape, dtype, fused=fused)
        p = plain(shape)
        p._fx_fused_wgrad_ok = fused
        return p

    torch.manual_seed(0)
    ref, fwd = producer(width, dtype, plain)
    _backward(fwd)
    torch.manual_seed(0)
    prm, fwd = producer(width, dtype, sinked)
    if not direct:
        buf = FlatParamGradBuffer(list(prm.items()))
        buf.grad_flat.fill_(7.0)
        for p in prm.values():
            p.fired = []
            p._fx_grad_ready = (lambda p, cb: lambda: (p.fired.append(1), cb()))(p, p._fx_grad_ready)
    _backward(fwd)
    once = {}
    for name, p in prm.items():
        # fp32: the plain gradient itself; bf16: both are roundings of one fp32 value
        assert p.grad is None, name                      # nothing was left to autograd
        assert torch.equal(p.main_grad.to(dtype), ref[name].grad), name
        assert p.fired == [1] and not p._fx_fresh, name
        once[name] = p.main_grad.clone()
    _backward(fwd)                                       # no zero_grad: accumulates
    for name, p in prm.items():
        assert torch.equal(p.main_grad, 2 * once[name]), name
        assert p.fired == [1, 1], name


def test_fused_mlp_bias_outside_a_buffer_goes_to_autograd():
    torch.manual_seed(0)
    ref, fwd = _fused_mlp(16, torch.bfloat16, lambda s, fused=True: torch.nn.Parameter(
        torch.randn(*s).bfloat16()))
    _backward(fwd)
    torch.manual_seed(0)
    prm, fwd = _fused_mlp(16, torch.bfloat16, lambda s, fused=True: _param(
        s, torch.bfloat16, fused=fused, ready=fused))
    _backward(fwd)
    b1 = prm["b1"]                                      # main_grad, but no readiness callback
    assert b1.grad.dtype == torch.bfloat16 and torch.equal(b1.grad, ref["b1"].grad)
    assert torch.equal(b1.main_grad, torch.full_like(b1.main_grad, 7.0)) and b1._fx_fresh


# ------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("dtype", DTYPES)
def test_buffer_hook_absorbs_and_sweep_zero_fills(dtype):
    from fleetx_amd.parallel.grad_buffer import FlatParamGradBuffer
    a = torch.nn.Parameter(torch.randn(6).to(dtype))
    b = torch.nn.Parameter(torch.randn(5).to(dtype))
    buf = FlatParamGradBuffer([("a", a), ("b", b)])
    buf.grad_flat.fill_(7.0)
    fired = []
    a._fx_grad_ready = (lambda cb: lambda: (fired.append(1), cb()))(a._fx_grad_ready)
    x = torch.arange(6.0).to(dtype)
    for micro in (1, 2):                                 # b receives no gradient
        (a * x).sum().backward()
        assert a.grad is None and a._fx_fresh is False and len(fired) == micro
        assert torch.equal(a.main_grad, micro * x.float())
    assert b._fx_fresh and torch.equal(b.main_grad, torch.full((5,), 7.0))
    buf.finish()
    assert not b._fx_fresh and torch.equal(b.main_grad, torch.zeros(5))
    assert torch.equal(a.main_grad, 2 * x.float())
    buf.zero_grad()
    assert a._fx_fresh and b._fx_fresh


def test_absorb_is_the_hook_body():
    """``sharding._accum_hook`` is ``absorb`` alone; ``grad_buffer``'s hook
    also drops the wgrad epilogue's norm partials."""
    from fleetx_amd.parallel import grad_sink as sink
    p = _param((4,), torch.bfloat16)
    sink.absorb(p)                                       # no .grad: a fused producer wrote
    assert p._fx_fresh and p.fired == []
    for n in (1, 2):
        p.grad = torch.ones(4, dtype=torch.bfloat16)
        sink.absorb(p)
        assert p.grad is None and not p._fx_fresh and len(p.fired) == n
        assert torch.equal(p.main_grad, torch.full((4,), float(n)))
