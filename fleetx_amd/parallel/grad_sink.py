"""The gradient sink: how an op writes a parameter gradient straight into the
flat buffer's ``p.main_grad`` instead of handing a tensor to autograd.

The protocol, in the order every producer follows it:

1. ask :func:`fused` whether the parameter takes direct writes;
2. :func:`open_write` -> ``(main_grad, accumulate)``: the first write of a
   step overwrites (``_fx_fresh``), later ones accumulate;
3. write (a kernel given ``main_grad.data_ptr()``, or :func:`store_or_add`);
4. :func:`close_write`: clears ``_fx_fresh`` and
5. reports :func:`grad_part_done` to the bucket / ZeRO unit (a tied weight
   only after its last part; ``notify=False`` defers the report).

:func:`deliver` is steps 1-5 for a gradient a PyTorch formula produced,
:func:`absorb` for one autograd left in ``.grad``.  Three producers ask another
question than the default predicate: ``on_gpu`` / ``fp32_contiguous`` of
:func:`fused`, and :func:`in_buffer`.  ``grad_buffer`` / ``sharding`` install
and reset the ``_fx_*`` attributes; a producer calls open, then close, and
touches none of them itself.  A leaf module: it imports nothing but torch.
"""
import torch


def fused(p, on_gpu=None, fp32_contiguous=False):
    """May a producer write ``p.main_grad`` directly?  (the default predicate)

    ``on_gpu`` (the gradient): only when it lives on the GPU -- a formula
    branch on the CPU returns its tensor so that the autograd hook adds it.
    ``fp32_contiguous``: only a contiguous fp32 ``main_grad`` -- the one-pass
    LayerNorm backward hands its kernel a raw fp32 pointer."""
    if p is None or not getattr(p, "_fx_fused_wgrad", False) or not hasattr(p, "main_grad"):
        return False
    if on_gpu is not None and not on_gpu.is_cuda:
        return False
    return not fp32_contiguous or (p.main_grad.dtype == torch.float32
                                   and p.main_grad.is_contiguous())


def in_buffer(p):
    """``p`` lives in a gradient buffer, whether or not it opted into fused
    gradients: the fused MLP writes FC1's bias gradient (``skip_bias_add``, so
    never ``_fx_fused_wgrad``) into ``main_grad`` from its dGeLU pass anyway."""
    return p is not None and hasattr(p, "main_grad") and \
        getattr(p, "_fx_grad_ready", None) is not None


def open_write(p):
    """``(main_grad, accumulate)``; reads only."""
    return p.main_grad, not getattr(p, "_fx_fresh", False)


def close_write(p, notify=True):
    """The write opened on ``p`` is issued; ``notify=False``: the caller
    reports :func:`grad_part_done` itself, later."""
    p._fx_fresh = False
    if notify:
        grad_part_done(p)


def grad_part_done(p):
    """One fused contribution to ``p.main_grad`` is in.  A weight used twice in
    a step (the tied word embedding: lookup + LM head, ``_fx_grad_parts = 2``)
    is reported ready to the gradient buffer only after its last part."""
    parts = getattr(p, "_fx_grad_parts", 1)
    if parts > 1:
        p._fx_parts_seen = getattr(p, "_fx_parts_seen", 0) + 1
        if p._fx_parts_seen < parts:
            return
        p._fx_parts_seen = 0
    cb = getattr(p, "_fx_grad_ready", None)
    if cb is not None:
        cb()


def store_or_add(dst, src, accumulate):
    """``dst (+)= src``."""
    if accumulate:
        dst.add_(src)
    else:
        dst.copy_(src)


def deliver(p, g32, dtype, on_gpu=False):
    """A gradient computed by a PyTorch formula: into ``main_grad`` (returns
    None) when ``p`` qualifies (``on_gpu``: see :func:`fused`), else returned
    in ``dtype`` for autograd."""
    if not fused(p, on_gpu=g32 if on_gpu else None):
        return g32.to(dtype)
    mg, accumulate = open_write(p)
    store_or_add(mg, g32, accumulate)
    close_write(p)
    return None


def absorb(param):
    """Body of the post-accumulate hooks: move ``param.grad`` into
    ``main_grad``.  Without a ``.grad`` a fused producer already wrote
    ``main_grad`` and reported it."""
    if param.grad is None:
        return
    mg, accumulate = open_write(param)
    store_or_add(mg, param.grad, accumulate)
    param.grad = None
    close_write(param)
