"""Symmetric abs-max fake quantisation with a straight-through estimator.

Reference P11 / K23: paddleslim QAT with ``abs_max`` weight quantisation and
``moving_average_abs_max`` activation quantisation at 8 bits
(``pretrain_gpt_345M_mp8_qat.yaml:35-44``).

Also the per-row weight-only int8 quantiser whose output the decode GEMV
consumes (``quantize_weight_int8`` / ``ops.gemm.decode_linear_w8``), and the
int4 quantiser with one scale per k-group of 256 (``quantize_weight_int4`` /
``ops.gemm.decode_linear_w4``).
"""
import torch

from . import _lib


def absmax(x):
    if x.is_cuda:
        out = torch.zeros(1, device=x.device, dtype=torch.float32)
        _lib.kernels().absmax(_lib.dt_code(x.dtype), x.contiguous().data_ptr(), x.numel(),
                              out.data_ptr(), _lib.stream())
        return out
    return x.detach().abs().max().float().reshape(1)


class _FakeQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, bits):
        if x.is_cuda:
            xc = x.contiguous()
            y = torch.empty_like(xc)
            _lib.kernels().fake_quant_fwd(_lib.dt_code(x.dtype), xc.data_ptr(), y.data_ptr(),
                                          scale.data_ptr(), int(bits), x.numel(), _lib.stream())
            return y
        qmax = float(2 ** (bits - 1) - 1)
        s = scale.clamp_min(1e-8)
        return (torch.clamp(torch.round(x.float() / s * qmax), -qmax, qmax) * s / qmax).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None


def fake_quant(x, scale, bits=8):
    """Quantise-dequantise ``x`` with the per-tensor ``scale`` (device scalar)."""
    return _FakeQuant.apply(x, scale.float().reshape(1), bits)


# ----------------------------------------------------------------------------
# weight-only int8 for decoding (consumed by ops.gemm.decode_linear_w8)
# ----------------------------------------------------------------------------
def quantize_weight_int8(w):
    """Symmetric int8 quantisation of ``w [N, K]`` with one scale per output
    row: ``scale[n] = max|w[n, :]| / 127`` (fp32; 1 for an all-zero row) and
    ``q = clamp(rint(w / scale), -127, 127)``.  Returns ``(q int8 [N, K]
    contiguous, scale fp32 [N])``.  Plain torch ops: it runs once per weight."""
    assert w.dim() == 2 and w.is_floating_point()
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(wf / scale[:, None]), -127, 127).to(torch.int8)
    return q.contiguous(), scale.contiguous()


def dequantize_weight_int8(q, scale, dtype=torch.float32):
    """``q * scale[:, None]`` computed in fp32 and rounded once to ``dtype``."""
    return (q.float() * scale.float()[:, None]).to(dtype)


# ----------------------------------------------------------------------------
# weight-only int4, group size 256 (consumed by ops.gemm.decode_linear_w4)
# ----------------------------------------------------------------------------
INT4_GROUP = 256


def pack_int4(qint):
    """Pack int8 ``qint [N, K]`` with values in [-8, 7] (K % 8 == 0) into uint8
    ``[N, K / 2]``.

    Layout (shared only with ``unpack_int4`` and csrc/kernels/decode_gemv_w4.hip):
    each aligned run of 8 values ``q[8i .. 8i+7]`` of a row is the 4 bytes
    ``4i .. 4i+3``; byte ``j`` holds ``q[8i + j]`` in its low nibble and
    ``q[8i + j + 4]`` in its high nibble, both as 4-bit two's complement.  A
    dword masked with 0xF0F0F0F0 -- as it is, and shifted left by 4 -- is then
    two vectors of four int8 ``16 * q`` in element order, which the kernel
    converts like int8 weights."""
    assert qint.dim() == 2 and qint.dtype == torch.int8 and qint.shape[1] % 8 == 0
    n, k = qint.shape
    u = (qint.view(n, k // 8, 2, 4).to(torch.int16) & 0xF)
    return (u[:, :, 0] | (u[:, :, 1] << 4)).to(torch.uint8).reshape(n, k // 2).contiguous()


def unpack_int4(packed):
    """The exact inverse of ``pack_int4``: uint8 ``[N, K / 2]`` -> int8 ``[N, K]``
    with values in [-8, 7]."""
    assert packed.dim() == 2 and packed.dtype == torch.uint8 and packed.shape[1] % 4 == 0
    n, kb = packed.shape
    b = packed.view(n, kb // 4, 4).to(torch.int16)
    u = torch.stack((b & 0xF, b >> 4), dim=2)          # [n, runs, low / high nibble, 4]
    return ((u ^ 8) - 8).to(torch.int8).reshape(n, kb * 2).contiguous()


def quantize_weight_int4(w):
    """Symmetric int4 quantisation of ``w [N, K]`` (K % 256 == 0, else
    ValueError) with one scale per group of 256 k and output row:
    ``scale[g, n] = max|w[n, 256g : 256g + 256]| / 7`` (fp32; 1 for an all-zero
    group) and ``q = clamp(rint(w / scale), -7, 7)``.  Returns ``(packed uint8
    [N, K / 2] contiguous, scale fp32 [K / 256, N] contiguous)``; the scale is
    group-major so that the kernel lane that owns four adjacent output columns
    reads its four scales of a group from adjacent addresses.  Plain torch
    ops: it runs once per weight."""
    assert w.dim() == 2 and w.is_floating_point()
    n, k = w.shape
    if k % INT4_GROUP:
        raise ValueError("quantize_weight_int4: K = %d is no multiple of the group size %d"
                         % (k, INT4_GROUP))
    wf = w.detach().float().view(n, k // INT4_GROUP, INT4_GROUP)
    amax = wf.abs().amax(dim=2)
    scale = torch.where(amax > 0, amax / 7.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(wf / scale[:, :, None]), -7, 7).to(torch.int8).view(n, k)
    return pack_int4(q), scale.t().contiguous()


def dequantize_weight_int4(packed, scale, dtype=torch.float32):
    """``q * scale`` of each value's group, computed in fp32 and rounded once
    to ``dtype``; ``[N, K]``."""
    q = unpack_int4(packed)
    n, k = q.shape
    wf = q.view(n, k // INT4_GROUP, INT4_GROUP).float() * scale.float().t()[:, :, None]
    return wf.view(n, k).to(dtype)
