"""Launch state travels with each launch, never in the kernel library: the
AdamW entry point takes its kernel shape and learning-rate source per call,
an optimizer's device learning rate is its own, and the dropout launchers
take the graph-mode salt from ``parallel/rng.py`` at launch time."""
import functools
import gc

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------- fx_adamw
# two full passes of the wide shape (1024 threads x 4 float4 groups) on one
# workgroup, a partial group of four, and a scalar tail of 3
N = 2 * 1024 * 4 * 4 + 5 * 4 + 3
SHAPES = [(0, 1, 0), (0, 0, 0), (1, 1, 1), (3, 1, 0)]  # (workgroup cap, non-temporal, wide)
FLAGS = [(torch.bfloat16, f) for f in range(4)] + [(torch.float16, f) for f in range(2)]


@functools.lru_cache(maxsize=None)
def _adamw_inputs(dtype):
    gen = torch.Generator().manual_seed(11)
    master = torch.randn(N, generator=gen)
    m = 0.1 * torch.randn(N, generator=gen)
    v = 0.01 * torch.rand(N, generator=gen)
    g16 = (0.1 * torch.randn(N, generator=gen)).to(dtype)  # exact in 16 bits and in fp32
    return tuple(t.to(DEV) for t in (master, m, v, g16))


def _adamw(dtype, flags, shape=(0, 1, 0), skip=0, lr=1e-3, lr_dev=None):
    """One launch on fresh copies of the inputs: (rc, buffers before, buffers
    after), buffers = [master storage, m, v, 16-bit parameters]."""
    from fleetx_amd.ops import _lib
    k, st = _lib.kernels(), _lib.stream()
    master, m, v, g16 = (t.clone() for t in _adamw_inputs(dtype))
    grad = g16 if flags & 1 else g16.float()
    if flags & 2:  # packed: the low halves + the bf16 parameters (= the high halves)
        p16 = torch.empty(N, dtype=torch.bfloat16, device=DEV)
        store = torch.empty(N, dtype=torch.int16, device=DEV)
        k.pk_split(master.data_ptr(), p16.data_ptr(), store.data_ptr(), N, st)
    else:
        p16 = torch.zeros(N, dtype=dtype, device=DEV)
        store = master
    gs = torch.tensor([0.5], device=DEV)
    sk = torch.tensor([skip], dtype=torch.int32, device=DEV)
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    bufs = [store, m, v, p16]
    before = [t.clone() for t in bufs]
    rc = k.adamw(_lib.dt_code(dtype), flags, store.data_ptr(), grad.data_ptr(), m.data_ptr(),
                 v.data_ptr(), p16.data_ptr(), N, lr, 0.9, 0.95, 1e-8, 0.1, 0.01, gs.data_ptr(),
                 sk.data_ptr(), step.data_ptr(), _lib.ptr(lr_dev), *shape, st)
    torch.cuda.synchronize()
    return rc, before, bufs


@pytest.mark.parametrize("dtype,flags", FLAGS)
def test_adamw_launch_shapes_skip_and_device_lr(dtype, flags):
    """Every launch shape runs ``adamw_elem`` on every element: bitwise the
    same master, m, v and parameters.  skip = 1 changes nothing; a device
    learning rate replaces the host value."""
    rc, before, ref = _adamw(dtype, flags, SHAPES[0])
    assert rc == 0
    assert not any(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, ref))
    for shape in SHAPES[1:]:
        rc, _, got = _adamw(dtype, flags, shape)
        assert rc == 0 and _same(got, ref), shape
    rc, before, got = _adamw(dtype, flags, skip=1)
    assert rc == 0 and _same(got, before)
    lr_dev = torch.tensor([2.5e-3], device=DEV)
    _, _, got = _adamw(dtype, flags, lr=1e-3, lr_dev=lr_dev)
    _, _, want = _adamw(dtype, flags, lr=2.5e-3)
    assert _same(got, want) and not _same(got, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_adamw_gradient_and_master_layouts_agree(dtype):
    """A gradient that is exact in 16 bits gives the same update from either
    storage; the packed master decodes to the fp32 master's bits."""
    from fleetx_amd.ops import _lib
    _, _, f32 = _adamw(dtype, 0)
    _, _, g16 = _adamw(dtype, 1)
    assert _same(f32, g16)
    if dtype != torch.bfloat16:
        return
    _, _, pk = _adamw(dtype, 2)
    _, _, pk16 = _adamw(dtype, 3)
    assert _same(pk, pk16)
    lo, m, v, hi = pk
    x = torch.empty(N, dtype=torch.float32, device=DEV)
    _lib.kernels().pk_join(hi.data_ptr(), lo.data_ptr(), x.data_ptr(), N, _lib.stream())
    torch.cuda.synchronize()
    assert _same([x, m, v], f32[:3])


@pytest.mark.parametrize("flags", [2, 3])
def test_adamw_packed_master_refuses_fp16(flags):
    rc, before, got = _adamw(torch.float16, flags)
    assert rc == -1 and _same(got, before)


# ---------------------------------------------------------------- no cross-talk
class _Toy(nn.Module):
    """Two layer units (the forward-overlapped update runs unit by unit), each
    weight three wide workgroups long."""

    def __init__(self):
        super().__init__()
        self.emb = nn.Parameter((torch.randn(96, 64) * 0.05).bfloat16())
        self.layers = nn.ModuleList([nn.Linear(192, 192, dtype=torch.bfloat16) for _ in range(2)])


def _make(lr):
    from fleetx_amd.parallel.grad_buffer import FlatParamGradBuffer
    from fleetx_amd.optims.optimizer import FusedAdamW, ClipGradByGlobalNorm
    torch.manual_seed(0)
    m = _Toy().cuda()
    buf = FlatParamGradBuffer(m.named_parameters())
    opt = FusedAdamW(lr, buf, grad_clip=ClipGradByGlobalNorm(1.0), weight_decay=0.1)
    return m, buf, opt, torch.Generator(device=DEV).manual_seed(1)


def _step(run):
    m, buf, opt, gen = run
    for _, p in m.named_parameters():
        p.main_grad.copy_(torch.randn(p.shape, device=DEV, generator=gen) * 0.1)
        p._fx_fresh = False
    buf.finish()
    opt.step()
    opt.clear_grad()


def _state(run):
    run[2].sync_state()
    torch.cuda.synchronize()
    return [p.detach().clone() for p in run[0].parameters()] + [x.clone() for x in run[2].master]


def _alone(lr, steps=3):
    run = _make(lr)
    for _ in range(steps):
        _step(run)
    return _state(run)


def test_optimizers_do_not_share_launch_state(monkeypatch):
    from fleetx_amd.ops import _lib
    for name in ("FLEETX_ADAMW_OVERLAP_GRID", "FLEETX_ADAMW_OVERLAP_WIDE", "FLEETX_ADAMW_NT"):
        monkeypatch.delenv(name, raising=False)
    k = _lib.kernels()
    real, calls = k.adamw, []

    def spy(*a):
        calls.append((a[17], tuple(a[18:21])))  # (lr_dev, (grid, nt, wide))
        return real(*a)
    monkeypatch.setattr(k, "adamw", spy)
    slow, fast = _alone(3e-3), _alone(7e-3)
    assert not _same(slow, fast)

    # one optimizer reads its learning rate from the device, the other from the host
    a, b = _make(3e-3), _make(3e-3)
    a[2].lr_dev = torch.tensor([7e-3], device=DEV)
    del calls[:]
    for _ in range(3):
        _step(a)
        _step(b)
    assert _same(_state(a), fast)   # follows its tensor
    assert _same(_state(b), slow)   # bitwise the run made alone
    assert {c[0] for c in calls} == {a[2].lr_dev.data_ptr(), 0}

    # a capped, wide overlapped update on one optimizer, then the serial one on the other
    c, d = _make(3e-3), _make(3e-3)
    c[2].overlap_grid, c[2].overlap_wide = 1, True
    assert c[2].enable_forward_overlap(c[0])
    for _ in range(3):
        del calls[:]
        _step(c)
        assert calls and {s for _, s in calls} == {(1, 1, 1)}
        del calls[:]
        _step(d)
        assert calls and {s for _, s in calls} == {(0, 1, 0)}
    assert _same(_state(d), slow)
    assert _same(_state(c), slow)


# ---------------------------------------------------------------- dropout salt
P = 0.1
KEY = 0x5EED0000 + 64 * 131071 + 1032
M64 = 0xFFFFFFFFFFFFFFFF


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _salt_key(key, salt):
    """``salt_key`` of csrc/kernels/fx_common.h in Python integers."""
    return _mix64(key ^ _mix64((salt + 0x9E3779B97F4A7C15) & M64)) & 0x7FFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def _keep(key):
    from fleetx_amd.parallel import rng
    return rng.keep_mask((64, 1032), P, key, DEV)


def _away_from_zero(shape, gen):
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2.0 - 1.0
    return sign * (1.0 + torch.rand(shape, generator=gen))


def _dropout_masks(op, dtype):
    """(forward keep mask, backward keep mask) of one dropout-bearing op: the
    inputs are away from zero, so a kept element is never 0."""
    from fleetx_amd import ops
    gen = torch.Generator().manual_seed(7)
    x = _away_from_zero((64, 1032), gen).to(dtype).to(DEV).requires_grad_()
    dy = _away_from_zero((64, 1032), gen).to(dtype).to(DEV)
    if op == "dropout":
        y = ops.dropout(x, P, KEY)
    elif op == "bias_dropout_add":
        b = torch.zeros(1032, dtype=dtype, device=DEV, requires_grad=True)
        y = ops.bias_dropout_add(x, b, None, P, KEY)  # (the bias: the column-sum backward)
    else:
        w = torch.ones(1032, dtype=dtype, device=DEV, requires_grad=True)
        lb = torch.zeros(1032, dtype=dtype, device=DEV, requires_grad=True)
        y, _ = ops.add_layer_norm(x, None, None, w, lb, p=P, key=KEY)  # y = s = dropout(x)
    y.backward(dy)  # (LayerNorm: only s carries a gradient, so ds = dy exactly)
    torch.cuda.synchronize()
    return y.detach() != 0, x.grad != 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("op", ["dropout", "bias_dropout_add", "add_layer_norm",
                                "add_layer_norm_row_bwd"])
def test_dropout_salt_is_read_at_launch(op, dtype, monkeypatch):
    from fleetx_amd.parallel import rng
    if op == "add_layer_norm_row_bwd":  # the row kernel + column passes instead of the one-pass
        monkeypatch.setenv("FLEETX_LN_BWD_FUSED", "0")
    rng.set_device_salt(None)
    try:
        fwd, bwd = _dropout_masks(op, dtype)
        assert torch.equal(fwd, _keep(KEY)) and torch.equal(bwd, _keep(KEY))
        salt = torch.tensor([5], dtype=torch.int64, device=DEV)
        rng.set_device_salt(salt)
        for s in (5, 6):
            salt.fill_(s)  # in place: no other call
            fwd, bwd = _dropout_masks(op, dtype)
            want = _keep(_salt_key(KEY, s))
            assert torch.equal(fwd, want) and torch.equal(bwd, want), s
        assert not torch.equal(_keep(_salt_key(KEY, 5)), _keep(_salt_key(KEY, 6)))
        assert not torch.equal(_keep(_salt_key(KEY, 5)), _keep(KEY))
        del salt
        gc.collect()
        fwd, bwd = _dropout_masks(op, dtype)
        assert torch.equal(fwd, _keep(KEY)) and torch.equal(bwd, _keep(KEY))
    finally:
        rng.set_device_salt(None)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_attention_dropout_salt_is_read_at_launch():
    from fleetx_amd import ops
    from fleetx_amd.parallel import rng
    torch.manual_seed(0)
    B, S, H, D = 1, 128, 2, 64
    qkv0 = (0.5 * torch.randn(B, S, H, 3, D, device=DEV)).bfloat16()
    g = torch.randn(B, S, H, D, device=DEV)

    @functools.lru_cache(maxsize=None)
    def reference(key):
        x = qkv0.float().requires_grad_()
        out = ops.attention_reference(x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2], causal=True,
                                      dropout_p=P, key=key)
        out.backward(g)
        return out.detach(), x.grad

    def check(key):
        """Forward and backward both drew the masks of ``key``."""
        qkv = qkv0.clone().requires_grad_()
        out = ops.flash_attention_qkvpacked(qkv, causal=True, dropout_p=P, key=KEY)
        out.backward(g.bfloat16())
        ref, ref_grad = reference(key)
        assert _rel(out, ref) < 2e-2, _rel(out, ref)
        for i in range(3):
            e = _rel(qkv.grad[:, :, :, i], ref_grad[:, :, :, i])
            assert e < 3e-2, (i, e)

    rng.set_device_salt(None)
    try:
        check(KEY)
        salt = torch.tensor([5], dtype=torch.int64, device=DEV)
        rng.set_device_salt(salt)
        check(_salt_key(KEY, 5))
        salt.fill_(6)
        check(_salt_key(KEY, 6))
        # (the tolerance tells the masks apart: another key's output is far off)
        assert _rel(reference(_salt_key(KEY, 6))[0], reference(_salt_key(KEY, 5))[0]) > 0.1
        assert _rel(reference(KEY)[0], reference(_salt_key(KEY, 5))[0]) > 0.1
        del salt
        gc.collect()
        check(KEY)
    finally:
        rng.set_device_salt(None)
