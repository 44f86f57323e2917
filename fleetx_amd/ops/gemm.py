"""Linear-layer GEMMs on the hand-written gfx950 MFMA kernel (csrc/kernels/gemm.hip).

Three entry points cover the three GEMMs of a linear layer ``y = x W^T (+b)``
with the weight stored ``[out, in]``, each in its NATIVE layout (no transposed
copies):

* :func:`linear_fwd`   ``y = x W^T (+ b)``, optionally with the tanh/erf GeLU
  epilogue (returns ``(gelu(h), h)``; ``h`` is the pre-activation kept for the
  backward pass).  A = x ``[M][K]`` (k-contiguous), B = W ``[N][K]``.
* :func:`linear_dgrad` ``dx = dy W``, optionally times ``gelu'(h)`` in the
  epilogue (FC2's data gradient becomes FC1's dH directly).  A = dy
  ``[M][N]``, B = W read as ``[K=N][n=in]`` (mn-contiguous, hardware
  transposed LDS reads).
* :func:`linear_wgrad` ``main_grad (+)= dy^T x`` in fp32 (beta 0/1).  Both
  operands token-major (mn-contiguous).

Each returns ``None`` when the kernel does not cover the shape (K not a
multiple of 64, odd extents, non-unit inner strides, fp32 tensors); the
caller then uses hipBLASLt.  ``FLEETX_GEMM=hip`` routes every covered GEMM
here, ``blas`` none, ``auto`` (default) the kinds in ``FLEETX_GEMM_AUTO``.

Parity: the reference's ``FusedLinear`` / ``fused_gemm_epilogue``
(``gpt/dygraph/single_model.py:29,81,375``; ``language_model/utils.py:30-36``).
"""
import os

import torch

from . import _lib

LAY_KC, LAY_MC = 0, 1
EPI_STORE, EPI_BIAS_GELU, EPI_DGELU, EPI_F32, EPI_BIAS_GELU_ERF, EPI_DGELU_ERF, EPI_F32B, \
    EPI_F32BT = range(8)

_MODE = os.environ.get("FLEETX_GEMM", "auto")


def enabled():
    return _MODE != "blas"


def set_mode(mode):
    """'hip' (default), 'blas' (hipBLASLt everywhere) or 'auto' (per-kind table)."""
    global _MODE
    _MODE = mode


# GEMM kinds routed to the MFMA kernel under FLEETX_GEMM=auto.  The
# hand-scheduled 4-wave kernel (csrc/kernels/gemm5.hip) takes
#  * wgrad: the fp32-accumulating weight gradient in its native token-major
#    layout -- 1.23-1.43 PF against 1.01-1.18 PF for hipBLASLt's TN path plus
#    the two transposes it needs (profiles/r3_gemm/);
#  * dgrad (opt-in): the data gradient with the weight read in place
#    (hardware transposed LDS reads) -- 1.37-1.54 PF against 1.41-1.48 PF for
#    the TN path with its weight transpose in isolation, but 4 ms/step slower
#    in the 6.7B step on the same box (profiles/r3_step/routing_ab.txt);
#  * dgrad_act / fwd_act (opt-in): the GEMMs with a fused GeLU' / bias+GeLU
#    epilogue.  Measured in the 6.7B step they lose: the GeLU math runs with
#    the matrix pipe idle at one workgroup per CU (0.97 ms vs 0.77 ms for the
#    plain GEMM on FC2's data gradient, more than the 0.16 ms elementwise
#    pass they retire), and a forward GEMM that holds whole CUs starves the
#    forward-overlapped AdamW (profiles/r3_step/);
# forward GEMMs stay on hipBLASLt, whose TN kernels tie or lead there.
# Only shapes whose output fills the chip go to the kernel: >= 192 tiles of
# 128 x 128 (the kernel itself runs 256 x 256 tiles when there are >= 192 of
# those, else 128 x 128 tiles at two workgroups per CU, which is what the
# hidden 1024-2048 models and ViT-g use); FLEETX_GEMM_AUTO="kind,kind"
# replaces the set.
_DEFAULT_AUTO = "wgrad"


def default_auto_kinds():
    """The process default: ``FLEETX_GEMM_AUTO`` or the built-in table."""
    return os.environ.get("FLEETX_GEMM_AUTO", _DEFAULT_AUTO)


AUTO_KINDS = set(k for k in default_auto_kinds().split(",") if k)
MIN_TILES = int(os.environ.get("FLEETX_GEMM_MIN_TILES", "192"))
# weight gradients whose tiles underfill the chip run split along K
# (gemm5.hip g5_split_plan), so they may take smaller shapes
WGRAD_MIN_TILES = int(os.environ.get("FLEETX_GEMM_WGRAD_MIN_TILES", "64"))


def set_auto_kinds(kinds):
    """Replace the kinds routed under ``auto`` ('wgrad,dgrad' or a list)."""
    if isinstance(kinds, str):
        kinds = [k.strip() for k in kinds.split(",")]
    AUTO_KINDS.clear()
    AUTO_KINDS.update(k for k in kinds if k)


def _tiles(r, c, t=128):
    return ((r + t - 1) // t) * ((c + t - 1) // t)


def out_tiles(kind, a, b, t=128):
    """t x t output tiles of GEMM ``kind`` on operands (a, b) as passed to
    :func:`use`: fwd (x, w) -> [M, N]; dgrad (dy, w) -> [M, K]; wgrad (dy, x)
    -> [N, K]."""
    M = a.numel() // a.shape[-1]
    if kind.startswith("fwd"):
        return _tiles(M, b.shape[0], t)
    if kind.startswith("dgrad"):
        return _tiles(M, b.shape[1], t)
    return _tiles(a.shape[-1], b.shape[-1], t)


# ----------------------------------------------------------------------------
# Shipped GEMM plan (reproducible routing; reference parity: the fused path is
# chosen at config time, ``models/language_model/utils.py:30-36,67-71``).
# ``gemm_plan_gfx950.json`` (tools/gemm_plan.py: many interleaved launches per
# candidate on an MI355X) holds, per (kind, dtype, M, N, K) of the model zoo's
# layer shapes, the route (MFMA kernel or vendor) and the tile-order M-group
# height, so one tree runs the same kernels with the same tile orders on
# every box, on every rank, inside and outside stream capture and under a
# profiler.  Nothing is timed at run time: a forward or data gradient the plan
# does not route runs on hipBLASLt.
# Which of the two is faster depends on the shape (GPT-3 6.7B with the tuned
# tile order: QKV forward 1466 vs 1331 TF/s, FC1 forward 1414 vs 1521; data
# gradients of QKV / out / FC1 lead, FC2 trails; profiles/r4_gm/), so the tool
# writes a data gradient's route when the kernel wins by 3 %.
# Forward routes are written by hand (tools/gemm_plan.py --fwd-route) after a
# step A/B: their isolated timing misleads in the step.  Beside the
# forward-overlapped AdamW a gemm5 wave takes its SIMD's whole register file,
# so the update cannot share those CUs: with the QKV forward on gemm5 (10 %
# faster alone) the 6.7B step takes 316-317 ms vs 293-295 (three interleaved
# runs each; ViT-g 461 vs 465 img/s; the forward A/B in profiles/r4_route/).
# Even without the overlapped update (345M in its graph) the isolated winners
# (out-proj, FC2 forward) made the step 0.1-0.3 ms slower (the 345M A/B in
# profiles/r4_route/).  The shipped plan routes no forward.
# Key convention: M = rows of the activation (tokens), N = output columns,
# K = reduction; wgrad: M = tokens, N = out features, K = in features.
# ----------------------------------------------------------------------------
PLAN_FILE = os.environ.get("FLEETX_GEMM_PLAN",
                           os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                        "gemm_plan_gfx950.json"))
_PLAN = None  # {(kind, dtype, M, N, K): entry}
_ROUTE = {}   # (kind, M, N, K, dtype) -> (kernel?, "plan" | "default"), per loaded plan


def _deterministic():
    return os.environ.get("FLEETX_DETERMINISTIC", "0") == "1"


_KIND_LAYOUT = {"fwd": (LAY_KC, LAY_KC, 0), "fwd_act": (LAY_KC, LAY_KC, 0),
                "dgrad": (LAY_KC, LAY_MC, 0), "dgrad_act": (LAY_KC, LAY_MC, 0),
                "wgrad": (LAY_MC, LAY_MC, 1)}


def kernel_shape(kind, M, N, K):
    """(la, lb, fp32 out, M, N, K) of the kernel launch for a plan key."""
    la, lb, f32 = _KIND_LAYOUT[kind]
    if kind == "wgrad":
        return la, lb, f32, N, K, M
    return la, lb, f32, M, N, K


def load_plan(path=None, force=False):
    """Read the plan (once) and preload its tile orders into the kernel
    library; returns {key: entry}.  A missing / foreign-arch plan is empty."""
    global _PLAN
    if _PLAN is not None and not force:
        return _PLAN
    import json
    plan = {}
    path = path or PLAN_FILE
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    arch = doc.get("arch", "gfx950")
    ok_arch = True
    if torch.cuda.is_available():
        name = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "") or ""
        ok_arch = not name or name.split(":")[0] == arch
    if ok_arch:
        for e in doc.get("entries", []):
            key = (e["kind"], e.get("dtype", "bf16"), int(e["M"]), int(e["N"]), int(e["K"]))
            plan[key] = e
    _PLAN = plan
    _ROUTE.clear()
    if plan and _lib.available() and torch.cuda.is_available():
        k = _lib.kernels()
        for (kind, dt, M, N, K), e in plan.items():
            if e.get("gm"):
                k.gemm_set_tuned(*kernel_shape(kind, M, N, K), int(e["gm"]))
    if _deterministic() and _lib.available():
        _lib.kernels().gemm_set_tune(0)
    return plan


def _plan_entry(plan, kind, dtype, M, N, K):
    """The plan entry of a shape; fp16 shapes the plan lacks take the bf16
    entry (same kernels, same MFMA cycle counts, same tile orders: the fp16
    O2 step otherwise put the QKV data gradient on hipBLASLt plus a
    transpose, +16 ms per 6.7B step, profiles/r6_fp16/)."""
    e = plan.get((kind, "bf16" if dtype == torch.bfloat16 else "fp16", M, N, K))
    if e is None and dtype == torch.float16:
        e = plan.get((kind, "bf16", M, N, K))
    return e


def plan_route(kind, M, N, K, dtype):
    """True / False when the plan fixes the route of this shape, else None."""
    e = _plan_entry(load_plan(), kind, dtype, M, N, K)
    if e is None or "route" not in e:
        return None
    return e["route"] == "kernel"


def route(mode, auto_kinds, plan, kind, dtype, M, N, K):
    """(MFMA kernel?, source) of one GEMM, from its arguments alone: the mode,
    then the kind table (output tiles against ``MIN_TILES``; the plan is not
    consulted), then the plan's ``route`` of a forward / data gradient, else
    the vendor library."""
    if mode != "auto":
        return mode != "blas", "mode"
    if kind in auto_kinds:
        if kind == "wgrad":
            return _tiles(N, K) >= WGRAD_MIN_TILES, "kind"
        return _tiles(M, N) >= MIN_TILES, "kind"
    if kind in ("fwd", "dgrad"):
        e = _plan_entry(plan, kind, dtype, M, N, K)
        if e is not None and "route" in e:
            return e["route"] == "kernel", "plan"
    return False, "default"


def route_table():
    """{(kind, M, N, K): True if the MFMA kernel takes it} of the forwards and
    data gradients the plan (or its silence) has decided so far."""
    return {k[:4]: v[0] for k, v in _ROUTE.items()}


def kernel_routes():
    """{"kind MxNxK": "plan"} of every forward / data-gradient shape routed to
    the MFMA kernel so far, for the bench line."""
    return dict(sorted(("%s %dx%dx%d" % k[:4], v[1]) for k, v in _ROUTE.items() if v[0]))


def use(kind, a, b=None):
    """Whether GEMM ``kind`` ('fwd' | 'fwd_act' | 'dgrad' | 'dgrad_act' |
    'wgrad'; ``_act`` = with the GeLU / GeLU' epilogue) on these operands goes
    to the MFMA kernel (the kernel itself may still decline the shape)."""
    if not a.is_cuda or a.dtype not in (torch.bfloat16, torch.float16):
        return False
    if _MODE != "auto":
        return _MODE != "blas"
    if b is None:
        return False
    M = a.numel() // a.shape[-1]
    if kind.startswith("fwd"):
        N, K = b.shape[0], b.shape[1]
    elif kind.startswith("dgrad"):
        N, K = b.shape[1], b.shape[0]
    else:
        N, K = a.shape[-1], b.shape[-1]
    plan = load_plan()  # also preloads the tile orders before a first launch
    key = (kind, M, N, K, a.dtype)
    # only what the plan decides is cached: the kind table may change under it
    r = _ROUTE.get(key) if kind not in AUTO_KINDS else None
    if r is None:
        r = route(_MODE, AUTO_KINDS, plan, kind, a.dtype, M, N, K)
        if kind in ("fwd", "dgrad") and r[1] != "kind":
            _ROUTE[key] = r
    return r[0]


def _ok(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or t.dtype not in (torch.bfloat16, torch.float16) or t.dim() != 2 \
                or t.stride(1) != 1 or t.data_ptr() % 16 or t.stride(0) % 8:
            return False
    return True


def _launch(dt, la, lb, epi, M, N, K, A, lda, B, ldb, C, ldc, bias=None, aux=None, ldaux=0,
            beta=0, sq=None, ws=None):
    return _lib.kernels().gemm(dt, la, lb, epi, M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb,
                               C.data_ptr(), ldc, _lib.ptr(bias), _lib.ptr(aux), ldaux, int(beta),
                               _lib.stream(), _lib.ptr(sq), _lib.ptr(ws))


def _splitk_ws(M, N, K, device):
    """Scratch for the split-K slices of an fp32 weight-gradient GEMM whose
    tiles do not fill whole waves of the chip (gemm5.hip ``g5_split_plan``:
    the leftover tiles are cut along K and summed in slice order by a combine
    launch); None when the shape runs unsplit."""
    n = _lib.kernels().gemm_ws_bytes(EPI_F32, M, N, K)
    return torch.empty(n // 4, device=device, dtype=torch.float32) if n else None


def sq_slots(n, k):
    """fp32 slots :func:`linear_wgrad` may write with ``sq`` for an [n, k]
    weight gradient: one per wave of every 128 x 128 tile (the 256-tile
    geometry uses the first quarter; slots it does not write keep their
    zero)."""
    return 4 * ((n + 127) // 128) * ((k + 127) // 128)


def linear_fwd(x2, w, bias=None, act=None, out=None):
    """``x2 [M,K] @ w[N,K]^T (+ bias)``; ``act`` in (None, 'gelu', 'gelu_erf').
    Returns ``y`` or ``(gelu(h), h)``; ``None`` if not covered."""
    if not enabled() or not _ok(x2, w) or w.dtype != x2.dtype:
        return None
    if bias is not None and (bias.dtype != x2.dtype or not bias.is_contiguous()):
        return None
    M, K = x2.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("linear_fwd: shape mismatch {} x {}".format(tuple(x2.shape), tuple(w.shape)))
    y = out if out is not None else torch.empty(M, N, device=x2.device, dtype=x2.dtype)
    h = None
    if act is None:
        epi = EPI_STORE
    else:
        epi = EPI_BIAS_GELU if act == "gelu" else EPI_BIAS_GELU_ERF
        h = torch.empty(M, N, device=x2.device, dtype=x2.dtype)
    rc = _launch(_lib.dt_code(x2.dtype), LAY_KC, LAY_KC, epi, M, N, K, x2, x2.stride(0), w,
                 w.stride(0), y, N, bias, h, N)
    if rc != 0:
        return None
    _lib.maybe_sync()
    return y if act is None else (y, h)


def linear_dgrad(dy2, w, act_input=None, act="gelu", out=None):
    """``dy2 [M,N] @ w [N,K]`` (times ``gelu'(act_input)`` when given), into
    ``out`` (a contiguous [M, K] block) when given."""
    if not enabled() or not _ok(dy2, w, act_input) or w.dtype != dy2.dtype:
        return None
    M, N = dy2.shape
    K = w.shape[1]
    if w.shape[0] != N:
        raise ValueError("linear_dgrad: shape mismatch")
    if out is not None and (out.shape != (M, K) or not out.is_contiguous()
                            or out.dtype != dy2.dtype or out.data_ptr() % 16):
        return None
    dx = out if out is not None else torch.empty(M, K, device=dy2.device, dtype=dy2.dtype)
    epi = EPI_STORE
    ld_aux = 0
    if act_input is not None:
        epi = EPI_DGELU if act == "gelu" else EPI_DGELU_ERF
        ld_aux = act_input.stride(0)
    # C[M, K] = sum_n A[m, n] B[n, k]: A = dy (k-contig over n), B = w stored [n][k]
    rc = _launch(_lib.dt_code(dy2.dtype), LAY_KC, LAY_MC, epi, M, K, N, dy2, dy2.stride(0), w,
                 w.stride(0), dx, K, None, act_input, ld_aux)
    if rc != 0:
        return None
    _lib.maybe_sync()
    return dx


# 16-bit weight gradients wider than tall through the transposed product
# (linear_wgrad): 6.7B FC2 1365 -> 1460-1474 TF/s, step -1.1 to -2.3 ms,
# bitwise the plain order (profiles/r5_wgrad_t/).  FLEETX_GEMM_WGRAD_T=0 keeps
# the plain order.
WGRAD_T = os.environ.get("FLEETX_GEMM_WGRAD_T", "1") == "1"


def covers_wgrad(dy2, x2):
    """Whether :func:`linear_wgrad` takes ``dy2^T x2`` (same checks as the
    kernel: 16-bit token-major operands, tokens a multiple of 64, extents of
    8)."""
    if not enabled() or not _ok(dy2, x2) or dy2.dtype != x2.dtype:
        return False
    M, N = dy2.shape
    return M % 64 == 0 and M >= 64 and N % 8 == 0 and x2.shape[1] % 8 == 0 and N >= 8 \
        and x2.shape[1] >= 8


def linear_wgrad(dy2, x2, out32, accumulate, sq=None):
    """``out32[N,K] (+)= dy2[M,N]^T @ x2[M,K]`` in fp32.  Returns True if done.

    ``out32`` may also be 16-bit (the bf16 / fp16 gradient storage of
    ``Distributed.comm.grad_dtype``): fp32 accumulation, one rounding in the
    epilogue; with ``accumulate`` (micro-batches, pipeline schedules) the
    stored value joins the fp32 sum before that rounding.

    ``sq`` (fp32, :func:`sq_slots` long): the epilogue also writes the sums of
    squares of the values it stores (of the fp32 values for a 16-bit output),
    so the global gradient norm needs no second pass over this weight's
    gradient (parallel/grad_buffer.py, ``enable_fused_norm``).  Returns False
    when the kernel cannot (the caller then computes without it)."""
    if not enabled() or not _ok(dy2, x2) or dy2.dtype != x2.dtype:
        return False
    out16 = out32.dtype == dy2.dtype
    if (out32.dtype != torch.float32 and not out16) or not out32.is_contiguous():
        return False
    M, N = dy2.shape
    K = x2.shape[1]
    if out32.shape != (N, K):
        raise ValueError("linear_wgrad: out shape {} != {}".format(tuple(out32.shape), (N, K)))
    # C[N, K] = sum_m A[n, m] B[m, k]: A = dy stored [m][n], B = x stored [m][k]
    if sq is not None and (sq.dtype != torch.float32 or sq.numel() < sq_slots(N, K)):
        raise ValueError("linear_wgrad: sq needs {} fp32 slots".format(sq_slots(N, K)))
    rc = -1
    if out16 and N < K and WGRAD_T and not accumulate:
        # wide gradient (FC2: [4096, 16384]): run the transposed product
        # x^T dy, the FC1 operand order, and store it transposed.  The FC2 order
        # takes 46 % more L2 misses (profiles/r5_gemm_pmc/); -7 = the shape
        # would split along K, where only the plain order exists
        rc = _launch(_lib.dt_code(dy2.dtype), LAY_MC, LAY_MC, EPI_F32BT, K, N, M, x2,
                     x2.stride(0), dy2, dy2.stride(0), out32, K, sq=sq,
                     ws=_splitk_ws(K, N, M, dy2.device))
    if rc != 0:
        rc = _launch(_lib.dt_code(dy2.dtype), LAY_MC, LAY_MC, EPI_F32B if out16 else EPI_F32, N,
                     K, M, dy2, dy2.stride(0), x2, x2.stride(0), out32, K, beta=accumulate, sq=sq,
                     ws=_splitk_ws(N, K, M, dy2.device))
    if rc == 0:
        _lib.maybe_sync()
    return rc == 0


def wgrad_16(dy2, x2):
    """``dy2^T @ x2`` returned in the 16-bit input dtype (no main_grad)."""
    if not enabled() or not _ok(dy2, x2) or dy2.dtype != x2.dtype:
        return None
    M, N = dy2.shape
    K = x2.shape[1]
    out = torch.empty(N, K, device=dy2.device, dtype=dy2.dtype)
    rc = _launch(_lib.dt_code(dy2.dtype), LAY_MC, LAY_MC, EPI_STORE, N, K, M, dy2, dy2.stride(0),
                 x2, x2.stride(0), out, K)
    return out if rc == 0 else None


# ----------------------------------------------------------------------------
# decode-time skinny GEMM (csrc/kernels/decode_gemv.h: one kernel template over
# the weight operand -- decode_gemv.hip 16-bit, decode_gemv_w8.hip int8,
# decode_gemv_w4.hip int4 with a scale per group of 256 k)
# ----------------------------------------------------------------------------
GV_BIAS, GV_GELU, GV_RES, GV_QKV = range(4)


def _decode_gemv(x, w, wscale, bias, epi, res, qkv_cache, ln, int4=False):
    """The body of ``decode_linear`` (``wscale`` None: ``w`` is a 16-bit weight
    of ``x.dtype``), ``decode_linear_w8`` (``w`` int8, ``wscale`` fp32 [N]) and
    ``decode_linear_w4`` (``int4``: ``w`` packed uint8 [N, K / 2], ``wscale``
    fp32 [K / 256, N]): the checks, the QKV unpacking, the output and the call.
    None for a call the kernel does not cover; malformed caches / residual
    assert."""
    if not x.is_cuda or x.dim() != 2 or x.shape[0] < 1 or x.shape[0] > 16 \
            or x.dtype not in (torch.bfloat16, torch.float16):
        return None
    M, K = x.shape
    wdtype = x.dtype if wscale is None else torch.uint8 if int4 else torch.int8
    if w.dim() != 2 or w.dtype != wdtype or not w.is_cuda or w.shape[1] * (2 if int4 else 1) != K:
        return None
    N = w.shape[0]
    if w.stride(1) != 1 or x.stride(1) != 1 or K % 1024 or x.stride(0) % 8 \
            or (w.stride(0) * w.element_size()) % 16 or w.data_ptr() % 16 or x.data_ptr() % 16:
        return None
    if wscale is not None and (wscale.dtype != torch.float32 or not wscale.is_cuda
                               or (wscale.shape != (K // 256, N) if int4
                                   else wscale.numel() != N)
                               or not wscale.is_contiguous()):
        return None
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N
                             or not bias.is_contiguous()):
        return None
    if ln is not None and (ln[0].dtype != x.dtype or ln[1] is None or ln[1].dtype != x.dtype
                           or not ln[0].is_contiguous() or not ln[1].is_contiguous()
                           or ln[0].numel() != K or ln[1].numel() != K
                           or epi not in (GV_GELU, GV_QKV)):
        return None
    k = _lib.kernels()
    kc = vc = pos = rows = None
    heads = hd = maxlen = 0
    if epi == GV_QKV:
        kc, vc, pos = qkv_cache[:3]
        rows = qkv_cache[3] if len(qkv_cache) > 3 else None
        maxlen, heads, hd = kc.shape[1], kc.shape[2], kc.shape[3]
        assert N == 3 * heads * hd and kc.is_contiguous() and vc.is_contiguous()
        assert kc.shape == vc.shape and kc.dtype == x.dtype == vc.dtype
        assert pos.dtype == torch.int64 and pos.numel() == M and pos.is_contiguous()
        if rows is None:
            assert kc.shape[0] >= M
        else:
            # rows.max() < kc.shape[0] is the caller's to keep (no sync to check it)
            assert rows.dtype == torch.int32 and rows.numel() == M and rows.is_contiguous() \
                and rows.is_cuda
        y = torch.empty(M, heads * hd, device=x.device, dtype=x.dtype)
    else:
        y = torch.empty(M, N, device=x.device, dtype=x.dtype)
    if epi == GV_RES:
        assert res is not None and res.shape == (M, N) and res.stride(1) == 1 \
            and res.dtype == x.dtype
    head = (_lib.dt_code(x.dtype), int(epi), M, N, K, x.data_ptr(), x.stride(0),
            w.data_ptr(), w.stride(0))
    tail = (_lib.ptr(bias), _lib.ptr(res) if epi == GV_RES else 0,
            res.stride(0) if epi == GV_RES else 0, y.data_ptr(), y.stride(0),
            _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(pos), _lib.ptr(rows), heads, hd, maxlen,
            _lib.ptr(ln[0]) if ln is not None else 0, _lib.ptr(ln[1]) if ln is not None else 0,
            float(ln[2]) if ln is not None else 0.0, _lib.stream())
    if wscale is None:
        nb = k.decode_gemv(*head, *tail)
    elif int4:
        nb = k.decode_gemv_w4(*head, wscale.data_ptr(), *tail)
    else:
        nb = k.decode_gemv_w8(*head, wscale.data_ptr(), *tail)
    if nb == 0:
        return None
    _lib.maybe_sync()
    return y


def decode_linear(x, weight, bias=None, epi=GV_BIAS, res=None, qkv_cache=None, ln=None):
    """``x [M, K] @ weight[N, K]^T`` for M <= 16 rows on the weight-streaming
    MFMA GEMV, with the epilogue ``epi``: GV_BIAS (+b), GV_GELU (gelu_tanh(+b)),
    GV_RES (+b + res[M, N]) or GV_QKV (``qkv_cache = (k_cache, v_cache, pos)``:
    the packed [heads][3][head_dim] output is scattered -- q returned as [M, H*D],
    k/v written into the caches [M, maxlen, H, D] at ``pos`` [M]; with
    ``qkv_cache = (k_cache, v_cache, pos, rows)``, ``rows`` int32 [M], row ``m``
    is written to ``cache[rows[m], pos[m]]``, so one call appends several
    positions of one sample: the caches are then [B, maxlen, H, D] and
    ``rows.max() < B`` is trusted, not checked).

    ``ln = (weight, bias, eps)`` (GV_GELU / GV_QKV): ``x`` is the residual
    stream and its LayerNorm is fused into the GEMV as a prologue (the
    decoder layer's LN1 / LN2 then cost no launch of their own).

    Returns the output, or None when the kernel does not cover the call (the
    caller then uses the general GEMM)."""
    return _decode_gemv(x, weight, None, bias, epi, res, qkv_cache, ln)


def decode_linear_w8(x, wq, wscale, bias=None, epi=GV_BIAS, res=None, qkv_cache=None, ln=None):
    """``decode_linear`` with a weight-only int8 weight: ``x [M, K] @ (wq[N, K]
    * wscale[N, None])^T`` with ``wq`` int8 and ``wscale`` fp32 from
    ``ops.quantize_weight_int8``; the int8 values are converted to ``x.dtype``
    in registers (exactly), the products accumulate in fp32 and ``wscale``
    multiplies the accumulator before the bias.

    Returns the output, or None when the kernel does not cover the call (the
    caller then uses the 16-bit weight)."""
    if wscale is None:
        return None
    return _decode_gemv(x, wq, wscale, bias, epi, res, qkv_cache, ln)


def decode_linear_w4(x, wq, wscale, bias=None, epi=GV_BIAS, res=None, qkv_cache=None, ln=None):
    """``decode_linear`` with a weight-only int4 weight of group size 256:
    ``wq`` packed uint8 [N, K / 2] and ``wscale`` fp32 [K / 256, N] from
    ``ops.quantize_weight_int4``.  The int4 values are converted to ``x.dtype``
    in registers (exactly), every group of 256 k accumulates in fp32 from zero
    and enters the accumulator times its scale; the bias and the epilogue
    follow as in ``decode_linear``.

    Returns the output, or None when the kernel does not cover the call (the
    caller then uses the 16-bit weight)."""
    if wscale is None:
        return None
    return _decode_gemv(x, wq, wscale, bias, epi, res, qkv_cache, ln, int4=True)
