"""Symmetric abs-max fake quantisation with a straight-through estimator.

Reference P11 / K23: paddleslim QAT with ``abs_max`` weight quantisation and
``moving_average_abs_max`` activation quantisation at 8 bits
(``pretrain_gpt_345M_mp8_qat.yaml:35-44``).

Also the per-row weight-only int8 quantiser whose output the decode GEMV
consumes (``quantize_weight_int8`` / ``ops.gemm.decode_linear_w8``), and the
int4 quantiser with one scale per k-group of 256 (``quantize_weight_int4`` /
``ops.gemm.decode_linear_w4``), and the MXFP4 quantiser (e2m1 elements, one
power-of-two scale per 32 k; ``quantize_weight_mxfp4`` /
``ops.gemm.decode_linear_mx4``).
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


def quantize_rows_int8(x):
    """``quantize_weight_int8``'s formula on the rows of an activation ``x
    [M, K]``: ``sx[m] = max|x[m, :]| / 127`` (fp32, an IEEE division; 1 for an
    all-zero row) and ``xq = clamp(rint(x / sx), -127, 127)``, ties to even.
    Returns ``(xq int8 [M, K] contiguous, sx fp32 [M])``, the operands of
    ``ops.gemm.prefill_gemm_w8a8``.  A bf16 / fp16 GPU tensor with ``K % 1024
    == 0``, ``K <= 65536`` and rows that admit 16-byte loads runs
    csrc/kernels/prefill_gemm_i8.hip (one read of ``x``); everything else the
    torch formula, which gives the same bytes.  Inputs are trusted finite."""
    assert x.dim() == 2 and x.is_floating_point()
    M, K = x.shape
    if x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and M >= 1 and K % 1024 == 0 \
            and 0 < K <= 65536 and x.stride(1) == 1 and x.stride(0) % 8 == 0 \
            and x.stride(0) >= K and x.data_ptr() % 16 == 0 and not x.requires_grad:
        xq = torch.empty(M, K, device=x.device, dtype=torch.int8)
        sx = torch.empty(M, device=x.device, dtype=torch.float32)
        if _lib.kernels().quant_rows_i8(_lib.dt_code(x.dtype), M, K, x.data_ptr(), x.stride(0),
                                        xq.data_ptr(), sx.data_ptr(), _lib.stream()):
            _lib.maybe_sync()
            return xq, sx
    return quantize_weight_int8(x)


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


# ----------------------------------------------------------------------------
# weight-only MXFP4 (OCP microscaling: e2m1 elements, groups of 32 k, one e8m0
# scale per group; consumed by ops.gemm.decode_linear_mx4)
# ----------------------------------------------------------------------------
MXFP4_GROUP = 32
# the value of code c (bit 3: sign, bits 2..0: e2m1 magnitude)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_MX_BLOCK = 16  # scale bytes per storage block: 512 k, two of the kernel's 256-k chunks


def _mx_scale_order(groups):
    """Stored position -> group index of a row's scale bytes.  Whole blocks of
    16 groups (512 k) are ordered [lane group g of 4][chunk c of 2][half j of
    2] = group ``8 c + 2 g + j`` of the block, so the dword at byte ``4 g`` of
    a block holds what the kernel lane that streams k ``64 g .. 64 g + 63`` of
    either 256-k chunk needs; groups past the last whole block keep their
    order (the kernels take K % 1024 == 0 only)."""
    idx = torch.arange(groups)
    full = groups // _MX_BLOCK * _MX_BLOCK
    g, c, j = torch.meshgrid(torch.arange(4), torch.arange(2), torch.arange(2), indexing="ij")
    blk = (8 * c + 2 * g + j).reshape(-1)
    idx[:full] = (torch.arange(0, full, _MX_BLOCK)[:, None] + blk[None, :]).reshape(-1)
    return idx


def pack_mxfp4(codes, exps):
    """Store uint8 e2m1 ``codes [N, K]`` (values 0..15, K % 32 == 0) and their
    biased group exponents ``exps`` uint8 ``[N, K / 32]`` as the kernels read
    them: ``(packed uint8 [N, K / 2], scale uint8 [N, K / 32])``.

    Layout (shared only with ``unpack_mxfp4``, csrc/kernels/decode_gemv_mx4.hip
    and GM4 of decode_gemm.hip): byte ``i`` of a packed row holds code ``2i``
    in its low nibble and code ``2i + 1`` in its high nibble, the order in
    which ``v_cvt_scalef32_pk_*_fp4`` unpacks a byte; the scale bytes of a row
    are permuted by ``_mx_scale_order``."""
    assert codes.dim() == 2 and codes.dtype == torch.uint8 and codes.shape[1] % MXFP4_GROUP == 0
    n, k = codes.shape
    assert exps.shape == (n, k // MXFP4_GROUP) and exps.dtype == torch.uint8
    c = codes.view(n, k // 2, 2)
    packed = (c[:, :, 0] | (c[:, :, 1] << 4)).contiguous()
    order = _mx_scale_order(k // MXFP4_GROUP).to(exps.device)
    return packed, exps[:, order].contiguous()


def unpack_mxfp4(packed, scale):
    """The exact inverse of ``pack_mxfp4``: ``(codes uint8 [N, K], exps uint8
    [N, K / 32])``."""
    assert packed.dim() == 2 and packed.dtype == torch.uint8 and scale.dtype == torch.uint8
    n, kb = packed.shape
    assert scale.shape == (n, kb * 2 // MXFP4_GROUP)
    codes = torch.stack((packed & 0xF, packed >> 4), dim=2).reshape(n, kb * 2).contiguous()
    exps = torch.empty_like(scale)
    exps[:, _mx_scale_order(scale.shape[1]).to(scale.device)] = scale
    return codes, exps


def quantize_weight_mxfp4(w):
    """MXFP4 quantisation of ``w [N, K]`` (K % 32 == 0, else ValueError).  Per
    (row, group of 32 k) the scale is ``X = 2^e``, the smallest power of two
    with ``amax <= 6 X``, so no element saturates; stored as the e8m0 byte
    ``e + 127`` clamped to [1, 254] (127 for an all-zero group).  This rounds
    the scale up where the OCP specification's conversion rounds it down
    (``2^(floor(log2 amax) - 2)``, which saturates elements above ``6 X``);
    the stored format is the same.  Elements are ``w / X`` rounded to nearest,
    ties to even, onto the e2m1 values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}.

    Returns ``(packed uint8 [N, K / 2], scale uint8 [N, K / 32])`` in the
    layout of ``pack_mxfp4``.  fp16 models: the kernels convert exactly while
    every ``code * X`` is a normal fp16, ``2^-13 <= X <= 2^13``; scales
    outside that range are not covered there (bf16 holds them all).  Plain
    torch ops: it runs once per weight."""
    assert w.dim() == 2 and w.is_floating_point()
    n, k = w.shape
    if k % MXFP4_GROUP:
        raise ValueError("quantize_weight_mxfp4: K = %d is no multiple of the group size %d"
                         % (k, MXFP4_GROUP))
    wf = w.detach().float().view(n, k // MXFP4_GROUP, MXFP4_GROUP)
    amax = wf.abs().amax(dim=2)
    # amax = m 2^ex, m in [0.5, 1): 6 * 2^(ex - 3) = 0.75 * 2^ex covers m <= 0.75
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-126, 127)
    v = torch.ldexp(wf.abs(), -e[:, :, None])
    mag = torch.where(v < 2, torch.round(v * 2),
                      torch.where(v < 4, torch.round(v) + 2, torch.round(v / 2) + 4)).clamp(max=7)
    codes = mag.to(torch.uint8) | (((wf < 0) & (mag > 0)).to(torch.uint8) << 3)
    return pack_mxfp4(codes.view(n, k), (e + 127).to(torch.uint8))


def dequantize_weight_mxfp4(packed, scale, dtype=torch.float32):
    """``value(code) * 2^(e - 127)`` of each element's group: exact in fp32
    and bf16, rounded once to ``dtype`` otherwise; ``[N, K]``."""
    codes, exps = unpack_mxfp4(packed, scale)
    n, k = codes.shape
    lut = torch.tensor(_E2M1 + tuple(-x for x in _E2M1), device=codes.device)
    val = lut[codes.long()].view(n, k // MXFP4_GROUP, MXFP4_GROUP)
    return torch.ldexp(val, exps.int()[:, :, None] - 127).view(n, k).to(dtype)
