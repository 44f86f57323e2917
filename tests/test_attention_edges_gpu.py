"""Element-wise edge tests of the training attention kernels (MI355X only):
``fa_fwd_kernel``, ``fa_bwd_dq_kernel`` and the two dK/dV kernels of
csrc/kernels/flash_attn.hip, against a float64 reference computed from the
same 16-bit inputs.  Every element of O, lse, delta, dQ, dK and dV is checked
and the number of elements out of tolerance must be 0: no norm over a tensor,
no share of elements left out.

Every ``check_*`` function takes the device, so tests/test_attention_edges_cpu.py
holds the PyTorch formula branch of ``ops.flash_attention`` to the same
reference and bounds (which shows that the reference satisfies them), and
shows without any kernel that the checker has teeth.

Why not a norm.  tests/test_kernels_gpu.py asserts one Frobenius norm per
tensor (2e-2 for O, 3e-2 for the gradients).  A float64 model at B*H = 8,
S = 384, D = 64, randn inputs gave: a causal mask that admits one extra key on
the last row of each 64-key tile moves O by 0.0071; the last key of the
sequence dropped for every row moves O by 0.0012.  Both pass a 0.02 limit.
``test_checker_*`` in the CPU module shows that each fails here.

Reference (``reference``), float64, ``T`` the 16-bit type, [B, H, S, D]:
  s      = scale * q k^T + key_bias;  -inf where key > query (causal, top-left
           aligned also for Sq != Sk) or key >= min(kv_lens[b], Sk)
  P      = softmax(s);  a row without an unmasked key has P = 0, lse = +inf
  keep   = parallel.rng.attention_keep_mask(B*H, Sq, Sk, p, key)
  Pd     = P o keep / (1 - p);             O  = Pd v
  dP     = (dO v^T) o keep / (1 - p);      delta_i = sum_d dO_id O_id
  dS     = P o (dP - delta)
  dQ     = scale dS k;   dK = scale dS^T q;   dV = Pd^T dO

Tolerances: a-priori rounding bounds built from the reference's own
intermediates, never measured on a kernel.  ``e = 2^-mant(T)`` (2^-7 bf16,
2^-10 fp16), ``A_i = sum_d |dO_id O_id|``:
  O[i,d]   1 ulp_T(ref) + e sum_j Pd_ij |v_jd|
  dV[j,d]  1 ulp_T(ref) + e sum_i Pd_ij |dO_id|
  dQ[i,d]  1 ulp_T(ref) + scale e (sum_j |dS_ij| |k_jd| + A_i sum_j P_ij |k_jd|)
  dK[j,d]  1 ulp_T(ref) + scale e (sum_i |dS_ij| |q_id| + sum_i A_i P_ij |q_id|)
Derivation: the kernels round P to T as an MFMA operand (forward, dV) and dS
to T (dQ, dK); each rounding is at most e/2 relative to the operand, so e/2
times the magnitude sum of the products.  delta is formed from the stored
16-bit O, so it is off by at most (e/2) A_i, which enters dS as P_ij times
that.  The factor 2 (e instead of e/2) covers the fp32 score, exp2, row sum
and accumulation order: at these score magnitudes (|s| < 2^5, fp32 spacing
2^-19) orders of magnitude below e.  The 1 ulp is the rounding of the result
to T (0.5 ulp) and the shift of that rounding by the error in front of it.
fp16 only: a 16-bit operand below 2^-14 is rounded at the absolute spacing
2^-24, so each sum gets 2^-24 times the magnitude sum of the other factor
over the unmasked (and kept, scaled by 1 / (1 - p)) pairs; the forward's P is
relative to a running max at or below the row max, so its row sum is >= 1 and
the spacing does not grow under the normalisation.  Where the reference is
exactly 0 (masked key, dropped pair, one-hot probe) every term is 0 and the
bound is the bare ulp floor of T at its smallest normal: the kernel must
produce 0.

lse and delta are fp32:
  lse_i    D 2^-23 scale max_j sum_d |q_id k_jd|  +  2^-20 (1 + |lse_i|)
           the fp32 dot product of D terms (2^-24 per add, both orders, at
           the largest score magnitude of the row), then the exp2 / log2
           units (2^-22 relative each) and the fp32 row sum and the final
           multiply, on |lse| and on the O(1) log of the row sum.
           +inf (no unmasked key) must match exactly.
  delta_i  (e/2 + 2^-20) A_i  +  (1/2) sum_d |dO_id| tO_id,
           tO_id = e sum_j Pd_ij |v_jd| (+ the fp16 term), O's own bound
           the rounding of O to T moves it by at most e/2 of its value; the
           fp32 sum of D products adds 2^-20 A_i at most (D <= 128).  The
           second term is the rounding of P to T as the forward's MFMA
           operand, which the stored O carries: (e/2) sum_j Pd_ij |v_jd| per
           element, i.e. half of O's own bound.  (The first term alone was
           the bound at first.  With one-hot dO and V, delta_i is the single
           product dO_ic O_ic with O_ic = Pd_ij rounded twice, as operand and
           as output, and the MI355X kernels exceeded e/2 on such rows by up
           to 1.8x; under a sum of D random products it does not show.)
A stacked broadcast gradient (the stride-0 K/V head) is the sum over heads
of gradients that each obey their bound, rounded once more by the summation:
sum of the per-head tolerances plus 1 ulp of the sum.

Inputs (``make_inputs``), each from a fixed ``torch.Generator`` seed:
  random  0.5 randn q and k, randn v and dO.
  probe   v one-hot over a window of D keys [j0, j0 + D): O[i,c] = Pd[i, j0+c],
          the probability matrix itself (with p > 0 an element-exact check of
          the kernel's keep mask, both keys of a hash pair, several (b, h));
          dO one-hot over a query window: dV[j,c] = Pd[i0+c, j].  One window
          pair per (b, h), across the tile boundaries (``_windows``).
  peaked  random plus one shared direction in the last 8 head dims of every
          query and of chosen keys, so that those keys score 6 natural-log
          units above the rest (``make_ce_case``'s peaks): keys 32m-1, 32m,
          32m+1 (the row's own key j = i for the rows around every wave /
          half-tile / tile boundary, the first key of each 64-key tile and of
          its second half), kv_len-1, kv_len (masked: a leak is loud), Sk-1.

Template coverage.  The production build launches, for T in {bf16, fp16},
mode in {causal, plain, key bias} and drop in {no, yes} (all twelve per row):

  kernel                         tile D  NW   reached by
  fa_fwd_kernel                  64      4    test_config_sweep D 64 (8, 40 too)
  fa_fwd_kernel                  64      8    test_forward_eight_waves_child
  fa_fwd_kernel                  96      3    test_config_sweep D 96, S 33/65/129
  fa_fwd_kernel                  96      4    test_config_sweep D 96, S 193/300
  fa_fwd_kernel                  128     4    test_config_sweep D 128 (100, 120)
  fa_fwd_kernel                  128     8    test_forward_eight_waves_child
  fa_bwd_dq_kernel               64      4    test_config_sweep D 64
  fa_bwd_dq_kernel               96      3    test_config_sweep D 96, S 33/65/129
  fa_bwd_dq_kernel               96      4    test_config_sweep D 96, S 193/300
  fa_bwd_dq_kernel               128     4    test_config_sweep D 128
  fa_bwd_dkdv_q64v_kernel        64      4    test_config_sweep D 64
  fa_bwd_dkdv_q64v_kernel        96      3    test_config_sweep D 96, S 33/65/129
  fa_bwd_dkdv_q64v_kernel        96      4    test_config_sweep D 96, S 193/300
  fa_bwd_dkdv_kernel             128     4    test_config_sweep D 128

``waves_for(S)`` picks 3 waves at S 33, 65, 129 and 4 at 193, 300; the causal
forward of every row runs the paired grid (one block at S <= 32 NW, a pair,
and at nq = 3 a pair plus the middle block alone), the unpaired grid runs in
test_forward_unpaired_grid_child.  test_config_sweep runs all 2 x 3 x 2 of
(T, mode, drop) for each of its head dims.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
_MANT = {torch.bfloat16: 7, torch.float16: 10}
_MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}

SEQ_ALL = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 193, 257, 300]
SEQ_PRUNED = [33, 65, 129, 193, 300]
HEAD_DIMS = [64, 96, 128, 8, 40, 72, 88, 120, 100]
MODES = ["causal", "plain", "kbias"]


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


def assert_fp32(got, ref64, tol, what=""):
    """An fp32 row statistic: every finite element within ``tol``, every
    infinite one equal."""
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape)
    g = got.double()
    inf = torch.isinf(ref64)
    err = torch.where(inf, torch.zeros_like(ref64), (g - ref64).abs())
    bad = torch.where(inf, g != ref64, ~(err <= tol))
    nbad = int(bad.sum())
    if nbad:
        over = torch.where(bad, torch.nan_to_num(err / tol, nan=math.inf) + 1.0,
                           torch.zeros_like(err))
        i = int(over.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(
            "%s: %d of %d elements off; worst at %s: got %r ref %r err %.3e tol %.3e"
            % (what, nbad, err.numel(), idx, float(g.reshape(-1)[i]), float(ref64.reshape(-1)[i]),
               float(err.reshape(-1)[i]), float(tol.reshape(-1)[i])))


# -------------------------------------------------------------------- cases
class Case:
    """One attention problem.  ``mode``: causal / plain / kbias (plain with a
    key bias); ``kv_lens``: per-batch list; ``bias``: "pad1e4" (-1e4 on the keys
    at and past ``bias_lens[b]``) or "imagen" (-1e9 on a random key mask, 0 on
    the three trailing latent keys); ``layout``: plain, packed3, packed2, sp
    (the sequence-parallel [s, b, h, 3, d].transpose(0, 1) view) or mqa (one
    K/V head broadcast by a stride-0 view)."""

    def __init__(self, Sq, Sk=None, D=64, dtype=torch.bfloat16, mode="plain", p=0.0, B=2, H=3,
                 inputs="random", kv_lens=None, bias=None, bias_lens=None, layout="plain"):
        self.Sq, self.Sk = Sq, Sq if Sk is None else Sk
        self.D, self.dtype, self.p, self.B, self.H = D, dtype, p, B, H
        self.causal = mode == "causal"
        self.inputs, self.kv_lens, self.layout = inputs, kv_lens, layout
        self.bias = bias if bias is not None else ("pad1e4" if mode == "kbias" else None)
        self.bias_lens = bias_lens
        self.scale = 1.0 / math.sqrt(D)
        self.key = 0x0123456789ABCDE + 977 * self.Sq + 131 * self.Sk + D
        self.seed = (self.Sq * 1009 + self.Sk) * 257 + D

    def __repr__(self):
        return "Case(Sq=%d Sk=%d D=%d %s causal=%s p=%s B=%d H=%d %s kv_lens=%s bias=%s %s)" % (
            self.Sq, self.Sk, self.D, str(self.dtype)[6:], self.causal, self.p, self.B, self.H,
            self.inputs, self.kv_lens, self.bias, self.layout)


def peaked_keys(Sk, kv_len):
    ks = {kv_len - 1, kv_len, Sk - 1}
    for m in range(0, Sk + 32, 32):
        ks.update((m - 1, m, m + 1))
    return sorted(j for j in ks if 0 <= j < Sk)


def _windows(S, D):
    """Window starts for the one-hot probes, one per (b, h): the start, an odd
    start inside the first tile, across the 128 and 192 boundaries (the second
    from an odd key), the last D rows, and a window that runs off the end."""
    return [max(0, min(w, S - 1)) for w in
            (0, 33, 128 - D // 2, 193 - D // 2, S - D, S - D // 2)]


def make_inputs(c, dev):
    """16-bit q, k, v, dO in [B, S, H, D] (k, v with one head for ``mqa``),
    kv_lens (int32) and key bias (fp32) or None."""
    gen = torch.Generator().manual_seed(c.seed)
    B, H, Sq, Sk, D = c.B, c.H, c.Sq, c.Sk, c.D
    Hk = 1 if c.layout == "mqa" else H
    q = 0.5 * torch.randn(B, Sq, H, D, generator=gen)
    k = 0.5 * torch.randn(B, Sk, Hk, D, generator=gen)
    v = torch.randn(B, Sk, Hk, D, generator=gen)
    dO = torch.randn(B, Sq, H, D, generator=gen)
    lens = None
    if c.kv_lens is not None:
        assert len(c.kv_lens) == B
        lens = torch.tensor(c.kv_lens, dtype=torch.int32)
    if c.inputs == "peaked":
        n8 = min(8, D)
        val = math.sqrt(6.0 * math.sqrt(D) / n8)      # scale * n8 * val^2 = 6
        q[..., D - n8:] = val
        for b in range(B):
            kl = min(c.kv_lens[b], Sk) if c.kv_lens is not None else Sk
            k[b, peaked_keys(Sk, kl), :, D - n8:] = val
    elif c.inputs == "probe":
        v.zero_()
        dO.zero_()
        kw, qw = _windows(Sk, D), _windows(Sq, D)
        cols = torch.arange(D)
        for b in range(B):
            for h in range(H):
                j = kw[(b * H + h) % len(kw)] + cols
                i = qw[(b * H + h + 2) % len(qw)] + cols
                v[b, j[j < Sk], h, cols[j < Sk]] = 1.0
                dO[b, i[i < Sq], h, cols[i < Sq]] = 1.0
    else:
        assert c.inputs == "random", c.inputs
    bias = None
    if c.bias == "pad1e4":
        bl = c.bias_lens if c.bias_lens is not None else [max(1, Sk - 5), max(1, Sk // 2)]
        bias = torch.zeros(B, Sk)
        for b in range(B):
            bias[b, bl[b % len(bl)]:] = -1e4
    elif c.bias == "imagen":
        keep = torch.rand(B, Sk, generator=gen) < 0.7
        keep[:, -3:] = True
        bias = torch.where(keep, 0.0, -1e9).float()
    q, k, v, dO = (t.to(c.dtype).to(dev) for t in (q, k, v, dO))
    return q, k, v, dO, (lens.to(dev) if lens is not None else None), \
        (bias.to(dev) if bias is not None else None)


# ---------------------------------------------------------------- reference
def reference(q, k, v, dO, causal, p, key, scale, kv_lens=None, key_bias=None, wrong=None):
    """float64 attention forward and backward from the 16-bit inputs, with the
    per-element tolerance terms (module docstring).  Returns a dict of
    [B, S, H, D] tensors ``O dQ dK dV`` and their ``t*`` bounds (the part on top
    of 1 ulp), and [B, H, Sq] ``lse delta`` with ``tlse tdelta``.

    ``wrong`` plants a mask mistake (the checker's self-test only):
    "extra_key" (causal admits key i + 1 on rows i = 63 mod 64), "drop_last"
    (the last valid key masked for every row), "swap_keep" (the keep mask with
    even and odd keys swapped)."""
    from fleetx_amd.parallel import rng
    dtype, dev = q.dtype, q.device
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    q64 = q.double().permute(0, 2, 1, 3)
    k64 = k.double().permute(0, 2, 1, 3).expand(B, H, Sk, D)
    v64 = v.double().permute(0, 2, 1, 3).expand(B, H, Sk, D)
    g64 = dO.double().permute(0, 2, 1, 3)
    s = torch.matmul(q64, k64.transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias.double().view(B, 1, 1, Sk)
    qi = torch.arange(Sq, device=dev).view(Sq, 1)
    kj = torch.arange(Sk, device=dev).view(1, Sk)
    masked = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool, device=dev)
    if causal:
        lim = torch.where(qi % 64 == 63, qi + 1, qi) if wrong == "extra_key" else qi
        masked = masked | (kj > lim)
    klen = torch.full((B,), Sk, dtype=torch.int64, device=dev)
    if kv_lens is not None:
        klen = kv_lens.to(dev).long().clamp(max=Sk)
    if wrong == "drop_last":
        klen = klen - 1
    masked = (masked | (kj.view(1, 1, 1, Sk) >= klen.view(B, 1, 1, 1))).expand(B, H, Sq, Sk)
    valid = (~masked).double()
    s = s.masked_fill(masked, -math.inf)
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)                              # no unmasked key
    ex = torch.exp(s - torch.where(dead, torch.zeros_like(m), m))
    l = ex.sum(-1, keepdim=True)
    P = ex / torch.where(dead, torch.ones_like(l), l)
    lse = torch.where(dead, torch.full_like(m, math.inf),
                      m + torch.log(torch.where(dead, torch.ones_like(l), l)))[..., 0]
    z = torch.ones_like(P)
    if p > 0.0:
        keep = rng.attention_keep_mask(B * H, Sq, Sk, p, key, dev).view(B, H, Sq, Sk)
        if wrong == "swap_keep":
            keep = keep[..., (torch.arange(Sk, device=dev) ^ 1).clamp(max=Sk - 1)]
        z = keep.double() / (1.0 - p)
    Pd = P * z
    O = torch.matmul(Pd, v64)
    dP = torch.matmul(g64, v64.transpose(-1, -2)) * z
    delta = (g64 * O).sum(-1)
    A = (g64 * O).abs().sum(-1, keepdim=True)
    dS = P * (dP - delta[..., None])
    dQ = scale * torch.matmul(dS, k64)
    dK = scale * torch.matmul(dS.transpose(-1, -2), q64)
    dV = torch.matmul(Pd.transpose(-1, -2), g64)

    e = 2.0 ** -_MANT[dtype]
    sub = 2.0 ** -24 if dtype == torch.float16 else 0.0   # fp16 operands below 2^-14
    qa, ka, va, ga = q64.abs(), k64.abs(), v64.abs(), g64.abs()
    vz = valid * z
    tO = e * torch.matmul(Pd, va) + sub * torch.matmul(vz, va)
    tdV = e * torch.matmul(Pd.transpose(-1, -2), ga) + sub * torch.matmul(vz.transpose(-1, -2), ga)
    tdQ = scale * (e * (torch.matmul(dS.abs(), ka) + A * torch.matmul(P, ka))
                   + sub * torch.matmul(valid, ka))
    tdK = scale * (e * (torch.matmul(dS.abs().transpose(-1, -2), qa)
                        + torch.matmul((P * A).transpose(-1, -2), qa))
                   + sub * torch.matmul(valid.transpose(-1, -2), qa))
    smag = torch.matmul(qa, ka.transpose(-1, -2)).amax(-1)
    tlse = D * 2.0 ** -23 * scale * smag + 2.0 ** -20 * (1.0 + torch.nan_to_num(lse.abs(), posinf=0.0))
    tdelta = (e / 2 + 2.0 ** -20) * A[..., 0] + 0.5 * (ga * tO).sum(-1)
    R = {"lse": lse, "delta": delta, "tlse": tlse, "tdelta": tdelta, "dead": dead[..., 0],
         "klen": klen}
    for name, t in (("O", O), ("dQ", dQ), ("dK", dK), ("dV", dV),
                    ("tO", tO), ("tdQ", tdQ), ("tdK", tdK), ("tdV", tdV)):
        R[name] = t.permute(0, 2, 1, 3)                # [B, S, H, D]
    return R


def compare(R, got, dtype, what=""):
    """``got``: any of O, dQ, dK, dV ([B, S, H, D] 16-bit) and lse, delta
    ([B, H, Sq] fp32) against the reference dict, every element."""
    for name in ("O", "dQ", "dK", "dV"):
        if name not in got:
            continue
        ref, tol = R[name], R["t" + name]
        if got[name].shape[2] == 1 and ref.shape[2] != 1:
            # a broadcast K/V head: the per-head gradients summed by autograd
            tol = (tol + ulp(ref, dtype)).sum(2, keepdim=True)
            ref = ref.sum(2, keepdim=True)
        assert_elementwise(got[name], ref, dtype, tol, "%s %s" % (what, name))
    if "lse" in got:
        assert_fp32(got["lse"], R["lse"], R["tlse"], what + " lse")
    if "delta" in got:
        assert_fp32(got["delta"], R["delta"], R["tdelta"], what + " delta")


# ------------------------------------------------------------- running the op
def run_ops(c, q, k, v, dO, lens, bias, backward=True):
    """O (and dQ, dK, dV) through ``ops.flash_attention`` /
    ``ops.flash_attention_qkvpacked`` in the case's layout."""
    from fleetx_amd import ops
    kw = dict(causal=c.causal, dropout_p=c.p, key=c.key, kv_lens=lens, key_bias=bias)
    if c.layout in ("plain", "mqa"):
        ql, kl, vl = (t.clone().requires_grad_(backward) for t in (q, k, v))
        if c.layout == "mqa":
            B, Sk, _, D = k.shape
            out = ops.flash_attention(ql, kl.expand(B, Sk, c.H, D), vl.expand(B, Sk, c.H, D), **kw)
        else:
            out = ops.flash_attention(ql, kl, vl, **kw)
        got = {"O": out.detach()}
        if backward:
            out.backward(dO)
            got.update(dQ=ql.grad, dK=kl.grad, dV=vl.grad)
        return got
    pd = 2 if c.layout == "packed2" else 3
    qkv = torch.stack([q, k, v], dim=pd)
    if c.layout == "sp":
        leaf = qkv.transpose(0, 1).contiguous().requires_grad_(backward)    # [s, b, h, 3, d]
        view = leaf.transpose(0, 1)
        assert not view.is_contiguous() or c.B == 1
    else:
        leaf = qkv.requires_grad_(backward)
        view = leaf
    out = ops.flash_attention_qkvpacked(view, pack_dim=pd, **kw)
    got = {"O": out.detach()}
    if backward:
        out.backward(dO)
        g = leaf.grad.transpose(0, 1) if c.layout == "sp" else leaf.grad
        assert g.shape == qkv.shape
        got.update(dQ=g.select(pd, 0), dK=g.select(pd, 1), dV=g.select(pd, 2))
    return got


def flash_raw(q, k, v, dO, causal, p, key, scale, kv_lens=None, key_bias=None, bufs=None,
              backward=True):
    """The ``flash_fwd`` / ``flash_bwd`` bindings called the way ``_FlashAttn``
    calls them: returns out, lse, and with ``backward`` delta, dq, dk, dv.
    ``bufs`` may hold preallocated (strided) output views by those names."""
    from fleetx_amd.ops import _lib
    from fleetx_amd.ops import attention as A
    from fleetx_amd.parallel import rng
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    bufs = dict(bufs or {})

    def buf(name, shape, dtype):
        if name not in bufs:
            bufs[name] = torch.empty(shape, device=q.device, dtype=dtype)
        assert tuple(bufs[name].shape) == tuple(shape) and bufs[name].dtype == dtype
        return bufs[name]
    K, dt, st = _lib.kernels(), _lib.dt_code(q.dtype), A._strides
    out = buf("out", (B, Sq, H, D), q.dtype)
    lse = buf("lse", (B * H * Sq,), torch.float32)
    kl = kv_lens.to(torch.int32).contiguous() if kv_lens is not None else None
    kb = A._padded_bias(key_bias, B, Sk, q.device)
    kbw = kb.shape[1] if kb is not None else 0
    rc = K.flash_fwd(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                     st(q), st(k), st(v), st(out), _lib.ptr(kl), _lib.ptr(kb), kbw,
                     B, H, Sq, Sk, D, int(causal), float(scale), float(p), key,
                     rng.device_salt_ptr(), _lib.stream())
    assert rc == 0, rc
    if not backward:
        return bufs
    g = torch.empty_strided(out.shape, out.stride(), device=q.device, dtype=q.dtype)
    g.copy_(dO)                      # dO shares out's strides
    dq = buf("dq", (B, Sq, H, D), q.dtype)
    dk = buf("dk", (B, Sk, H, D), q.dtype)
    dv = buf("dv", (B, Sk, H, D), q.dtype)
    assert dk.stride() == dv.stride()
    delta = buf("delta", (B * H * Sq,), torch.float32)
    rc = K.flash_bwd(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), g.data_ptr(),
                     lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                     st(q), st(k), st(v), st(out), st(dq), st(dk), _lib.ptr(kl), _lib.ptr(kb), kbw,
                     B, H, Sq, Sk, D, int(causal), float(scale), float(p), key,
                     rng.device_salt_ptr(), _lib.stream())
    assert rc == 0, rc
    return bufs


def check_case(dev, c, backward=True):
    """Reference, the op in the case's layout, every element; on the GPU also
    lse and delta through the bindings (native head dims)."""
    q, k, v, dO, lens, bias = make_inputs(c, dev)
    R = reference(q, k, v, dO, c.causal, c.p, c.key, c.scale, lens, bias)
    got = run_ops(c, q, k, v, dO, lens, bias, backward)
    compare(R, got, c.dtype, repr(c))
    if c.kv_lens is not None:
        # rows without a key, and keys past kv_len: exactly 0, not merely small
        dead = R["dead"].permute(0, 2, 1)               # [B, Sq, H]
        assert int(torch.count_nonzero(got["O"][dead])) == 0, c
        if backward:
            assert int(torch.count_nonzero(got["dQ"][dead])) == 0, c
            past = torch.arange(c.Sk, device=dev).view(1, c.Sk) >= R["klen"].view(c.B, 1)
            assert int(torch.count_nonzero(got["dK"][past])) == 0, c
            assert int(torch.count_nonzero(got["dV"][past])) == 0, c
    if torch.device(dev).type == "cuda" and c.D % 8 == 0:
        B, H, Sk, D = c.B, c.H, c.Sk, c.D
        ke, ve = (t.expand(B, Sk, H, D) for t in (k, v))
        raw = flash_raw(q, ke, ve, dO, c.causal, c.p, c.key, c.scale, lens, bias,
                        backward=backward)
        assert torch.equal(raw["out"], got["O"]), c
        stats = {"lse": raw["lse"].view(B, H, c.Sq)}
        if backward:
            stats["delta"] = raw["delta"].view(B, H, c.Sq)
        compare(R, stats, c.dtype, repr(c))


# ----------------------------------------------------------------- the tests
@pytest.mark.parametrize("inputs,p", [("random", 0.0), ("peaked", 0.1)])
@pytest.mark.parametrize("mode", ["causal", "plain"])
def test_every_sequence_length(mode, inputs, p):
    """nq = 1, 2, 3 of the paired causal grid, every partial wave and half tile."""
    for S in SEQ_ALL:
        check_case(DEV, Case(S, D=64, mode=mode, p=p, inputs=inputs))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_config_sweep(D, dtype, mode, p):
    """Every production template (module docstring): tile dims, the native
    non-tile dims (columns past D read as zero, never stored) and the padded
    copy route of D 100."""
    for S in SEQ_PRUNED:
        check_case(DEV, Case(S, D=D, dtype=dtype, mode=mode, p=p, inputs="peaked"))


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 96, 128])
def test_probability_probes(D, dtype, mode, p):
    """One-hot V and dO: O and dV are windows of the probability matrix, with
    p > 0 of the kernel's keep mask (exact zeros where masked or dropped)."""
    for S in (129, 300):
        check_case(DEV, Case(S, D=D, dtype=dtype, mode=mode, p=p, inputs="probe"))


def kv_len_groups(Sk):
    """Per-batch kv_lens, two batches at a time: 0 (the all-masked batch), the
    tile edges, Sk + 5 (clamped), and 10 (key blocks wholly past kv_len)."""
    return [[0, 1], [63, 64], [65, Sk - 1], [Sk, Sk + 5], [10, Sk // 2]]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16),
                                     (88, torch.bfloat16)])
def test_kv_lens(D, dtype, mode, p):
    """``kv_lens`` with and without the causal mask (the prefill of
    generation.py is causal with Sq = Sk)."""
    for S in (129, 300):
        for lens in kv_len_groups(S):
            check_case(DEV, Case(S, D=D, dtype=dtype, mode=mode, p=p, inputs="peaked",
                                 kv_lens=lens))


CROSS_SHAPES = [(33, 129), (129, 33), (1, 1), (257, 70)]


@pytest.mark.parametrize("bias", [None, "imagen", "pad1e4"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", CROSS_SHAPES)
def test_cross_attention(Sq, Sk, D, dtype, bias):
    """Sq != Sk with and without a key bias (Imagen cross attention): the
    Imagen mask pattern, and -1e4 padding with one batch whose every key
    carries -1e4."""
    for inputs in ("random", "peaked"):
        check_case(DEV, Case(Sq, Sk, D=D, dtype=dtype, p=0.1 if D == 64 else 0.0, inputs=inputs,
                             bias=bias, bias_lens=[max(1, Sk - 5), 0]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention_broadcast_kv_head(dtype):
    check_case(DEV, Case(33, 129, D=64, dtype=dtype, layout="mqa"))
    check_case(DEV, Case(257, 70, D=128, dtype=dtype, layout="mqa", bias="imagen"))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(97, 200), (200, 97)])
def test_causal_cross_attention_top_left(Sq, Sk, D, dtype, p):
    """Causal with Sq != Sk masks key > query (top-left aligned), as
    ``attention_reference`` does."""
    for inputs in ("peaked", "probe"):
        check_case(DEV, Case(Sq, Sk, D=D, dtype=dtype, mode="causal", p=p, inputs=inputs))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [64, 88, 128])
@pytest.mark.parametrize("layout", ["packed3", "packed2", "sp"])
def test_layouts(layout, D, mode):
    for dtype in DTYPES:
        check_case(DEV, Case(129, D=D, dtype=dtype, mode=mode, p=0.1, inputs="peaked",
                             layout=layout))


@pytest.mark.parametrize("layout", ["plain", "packed3"])
@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("D", [128, 88])
def test_row_store_fallback_elementwise(D, mode, layout, monkeypatch):
    """FLEETX_FA_ROW16=0 (read per call): the 8-byte row stores."""
    monkeypatch.setenv("FLEETX_FA_ROW16", "0")
    for S in (129, 300):
        check_case(DEV, Case(S, D=D, mode=mode, p=0.1, inputs="peaked", layout=layout))


@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [88, 128])
def test_no_stray_writes(D, dtype, mode):
    """Outputs carved out of sentinel-filled buffers with a guard row before
    and after every batch and 8 guard columns past D: the forward (O, lse),
    dQ (dQ, delta) and dK/dV kernels leave every guard element alone at the
    tail shape S = 129."""
    c = Case(129, D=D, dtype=dtype, mode=mode, p=0.1, inputs="peaked")
    B, H, S, G = c.B, c.H, 129, 64
    q, k, v, dO, lens, bias = make_inputs(c, DEV)
    R = reference(q, k, v, dO, c.causal, c.p, c.key, c.scale)
    big = {n: torch.full((B, S + 2, H, D + 8), 3.0, device=DEV, dtype=dtype)
           for n in ("out", "dq", "dk", "dv")}
    stat = {n: torch.full((G + B * H * S + G,), -7777.0, device=DEV) for n in ("lse", "delta")}
    bufs = {n: t[:, 1:S + 1, :, :D] for n, t in big.items()}
    bufs.update({n: t[G:G + B * H * S] for n, t in stat.items()})
    flash_raw(q, k, v, dO, c.causal, c.p, c.key, c.scale, bufs=bufs)
    torch.cuda.synchronize()
    inner = torch.zeros(B, S + 2, H, D + 8, dtype=torch.bool, device=DEV)
    inner[:, 1:S + 1, :, :D] = True
    for n, t in big.items():
        assert bool((t[~inner] == 3.0).all()), "%s: guard elements written" % n
    for n, t in stat.items():
        assert bool((t[:G] == -7777.0).all()) and bool((t[-G:] == -7777.0).all()), n
    compare(R, {"O": bufs["out"], "dQ": bufs["dq"], "dK": bufs["dk"], "dV": bufs["dv"],
                "lse": bufs["lse"].view(B, H, S), "delta": bufs["delta"].view(B, H, S)},
            dtype, repr(c))


def test_rejected_calls_launch_nothing():
    """The return codes of ``flash_fwd`` / ``flash_bwd``: -1 for a head dim
    that is no multiple of 8, -2 for a key bias with the causal mask, -3 for an
    unknown dtype code; and a rejected call launches nothing: every output
    buffer keeps its sentinel.  The tensors are real (B 1, H 1, S 32, head dim
    16, a [1, 128] key bias), so even a wrong launch would stay inside memory
    this test owns."""
    from fleetx_amd.ops import _lib
    from fleetx_amd.ops import attention as A
    from fleetx_amd.parallel import rng
    K, st = _lib.kernels(), A._strides
    B, H, S, D = 1, 1, 32, 16
    q, k, v, g = (torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16) for _ in range(4))
    kb = torch.zeros(1, 128, device=DEV)
    o16 = {n: torch.full((B, S, H, D), 3.0, device=DEV, dtype=torch.bfloat16)
           for n in ("out", "dq", "dk", "dv")}
    f32 = {n: torch.full((B * H * S,), -7777.0, device=DEV) for n in ("lse", "delta")}
    out, dq, dk, dv = (o16[n] for n in ("out", "dq", "dk", "dv"))
    lse, delta = f32["lse"], f32["delta"]

    def fwd(dt, d, causal, bias):
        return K.flash_fwd(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                           lse.data_ptr(), st(q), st(k), st(v), st(out), 0, _lib.ptr(bias),
                           bias.shape[1] if bias is not None else 0, B, H, S, S, d, causal,
                           0.25, 0.0, 1, rng.device_salt_ptr(), _lib.stream())

    def bwd(dt, d, causal, bias):
        return K.flash_bwd(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                           g.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                           dk.data_ptr(), dv.data_ptr(), st(q), st(k), st(v), st(out), st(dq),
                           st(dk), 0, _lib.ptr(bias), bias.shape[1] if bias is not None else 0,
                           B, H, S, S, d, causal, 0.25, 0.0, 1, rng.device_salt_ptr(),
                           _lib.stream())

    for call in (fwd, bwd):
        assert call(0, 12, 0, None) == -1, call.__name__
        assert call(0, D, 1, kb) == -2, call.__name__
        assert call(2, D, 0, None) == -3, call.__name__
    torch.cuda.synchronize()
    for n, t in o16.items():
        assert bool((t == 3.0).all()), "%s written by a rejected call" % n
    for n, t in f32.items():
        assert bool((t == -7777.0).all()), "%s written by a rejected call" % n


# ------------------------------------------------- per-process switches (children)
def _child_main(argv):
    """Forward checks (O, lse) in a process whose environment carries one of
    the switches that flash_attn.hip caches on first use.  Exit 1 on a failure."""
    name, value, dims = argv[0], argv[1], [int(d) for d in argv[2].split(",")]
    assert os.environ.get(name) == value, (name, os.environ.get(name))
    n = 0
    try:
        for D in dims:
            for dtype in DTYPES:
                for mode in MODES:
                    for p in (0.0, 0.1):
                        for S in (129, 257, 300):
                            check_case(DEV, Case(S, D=D, dtype=dtype, mode=mode, p=p,
                                                 inputs="peaked"), backward=False)
                            n += 1
    except AssertionError as exc:
        print("FAILED after %d cases: %s" % (n, exc))
        return 1
    torch.cuda.synchronize()
    print("attention child ok: %d cases" % n)
    return 0


def _run_child(name, value, dims):
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, "-m", "tests.test_attention_edges_gpu", name, value, dims],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "attention child ok" in r.stdout, r.stdout[-4000:]


def test_forward_eight_waves_child():
    """FLEETX_FA_FWD_WAVES=8: the 256-query forward workgroup, D 64 and 128."""
    _run_child("FLEETX_FA_FWD_WAVES", "8", "64,128")


def test_forward_unpaired_grid_child():
    """FLEETX_FA_PAIR=0: one causal query block per workgroup in LPT order."""
    _run_child("FLEETX_FA_PAIR", "0", "64,96,128")


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1:]))
