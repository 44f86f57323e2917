"""``fa_fwd_qoff_kernel`` (csrc/kernels/flash_attn.hip) through
``ops.prefill_attention`` on the MI355X: the embedded reference, bounds and
cases of tests/test_prefill_attention_cpu.py, every element of O and lse, zero
elements out of bounds.

Kernel rows reached: tile 64 x 4 waves (D 64), 96 x 3 (D 88, Sq 33 / 70 / 129),
96 x 4 (D 88, Sq 200 / 300), 128 x 4 (D 128); bf16 and fp16 each.  Grids: one
block, a pair, a pair plus the unpaired middle block (Sq 300), and the unpaired
grid in a child process (``FLEETX_FA_PAIR=0`` is read once per process)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import test_attention_edges_gpu as A
from tests import test_prefill_attention_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = A.ROOT


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fleetx_amd.ops import _lib
    _lib.kernels()  # fail loudly if the extension is missing
    torch.manual_seed(0)


@pytest.mark.parametrize("inputs", ["random", "peaked", "probe"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_embedded(dtype, D, inputs):
    for Sq, q_starts in C.SHAPES:
        C.check_embedded(DEV, C.ST, Sq, q_starts, D, dtype, inputs)
        C.check_embedded(DEV, C.ST, Sq, q_starts, D, dtype, inputs,
                         kv_lens=C.diagonal_binds(C.ST, Sq, q_starts))


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_tile_96(dtype):
    """D 88 on the 96 tile, 3 waves (Sq 33, 70, 129) and 4 (Sq 200)."""
    for Sq, q_starts in C.SHAPES + [(200, [0, 0])]:
        C.check_embedded(DEV, C.ST, Sq, q_starts, 88, dtype, "peaked")


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (88, torch.float16),
                                     (128, torch.bfloat16)])
def test_three_query_blocks(D, dtype):
    """Sq 300 over 640 keys: a pair plus the unpaired middle block, at an odd
    and at a long offset."""
    for inputs in ("peaked", "probe"):
        C.check_embedded(DEV, 640, 300, [1, 340], D, dtype, inputs)


@pytest.mark.parametrize("D", [64, 128])
def test_plain_causal_is_the_flash_forward(D):
    """q_starts 0 over the whole sequence: plain causal, the bits of
    ``flash_attention`` (same tiles in the same order)."""
    from fleetx_amd import ops
    out, _ = C.check_embedded(DEV, C.ST, 200, [0, 0], D, torch.bfloat16, "peaked")
    c, qb, k, v, lens, _ = C.embedded(DEV, C.ST, 200, [0, 0], D, torch.bfloat16, "peaked",
                                      [C.ST, C.ST])
    assert torch.equal(out, ops.flash_attention(qb, k, v, causal=True, scale=c.scale))


@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (128, torch.bfloat16)])
def test_empty_sample_and_padding_chunk(D, dtype):
    out, lse = C.check_embedded(DEV, C.ST, 33, [0, 40], D, dtype, "random", kv_lens=[0, 100])
    assert int(torch.count_nonzero(out[0])) == 0
    assert bool((lse[0] == math.inf).all())
    # both items of a pair empty
    out, lse = C.check_embedded(DEV, C.ST, 150, [0, 40], D, dtype, "random", kv_lens=[0, 200])
    assert int(torch.count_nonzero(out[0])) == 0 and bool((lse[0] == math.inf).all())
    # a padding chunk: q_start 150 past kv_len 120, every row sees the 120 keys
    out, _ = C.check_embedded(DEV, C.ST, 50, [150, 10], D, dtype, "peaked", kv_lens=[120, 200])
    assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_cache_view_and_packed_q(D, dtype):
    """K/V as the first 200 valid rows of a [B, 256, H, D] cache (the rows past
    kv_len hold NaN), q as the select view of a packed [B, Sq, H, 3, D] tensor."""
    from fleetx_amd import ops
    Sq, q_starts = 70, [65, 130]
    c, qb, k, v, lens, ref = C.embedded(DEV, C.ST, Sq, q_starts, D, dtype, "peaked", [180, 200])
    B, H = c.B, c.H
    kc = torch.full((B, 256, H, D), math.nan, device=DEV, dtype=dtype)
    vc = torch.full((B, 256, H, D), math.nan, device=DEV, dtype=dtype)
    kc[:, :C.ST], vc[:, :C.ST] = k, v
    for b in range(B):
        kc[b, int(lens[b]):], vc[b, int(lens[b]):] = math.nan, math.nan
    qkv = torch.randn(B, Sq, H, 3, D, device=DEV).to(dtype)
    qkv[:, :, :, 0] = qb
    qv = qkv.select(3, 0)
    assert not qv.is_contiguous()
    qs = torch.tensor(q_starts, dtype=torch.int32, device=DEV)
    out, lse = ops.prefill_attention(qv, kc, vc, qs, lens, scale=c.scale, return_lse=True)
    C.compare(ref, out, lse, dtype, "cache view")


def _raw(K, q, k, v, out, lse, qs, kl, dt=None, D=None):
    from fleetx_amd.ops import _lib
    from fleetx_amd.ops import attention as OA
    B, Sq, H, Dq = q.shape
    return K.flash_fwd_qoff(_lib.dt_code(q.dtype) if dt is None else dt, q.data_ptr(),
                            k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                            OA._strides(q), OA._strides(k), OA._strides(v), OA._strides(out),
                            qs.data_ptr() if qs is not None else 0,
                            kl.data_ptr() if kl is not None else 0, B, H, Sq, k.shape[1],
                            Dq if D is None else D, 1.0 / math.sqrt(Dq), _lib.stream())


@pytest.mark.parametrize("D,dtype", [(88, torch.bfloat16), (128, torch.float16)])
def test_no_stray_writes(D, dtype):
    """O and lse carved out of sentinel buffers (a guard row before and after
    every sample, 8 guard columns, 64 guard floats): Sq 129, the tail shape."""
    from fleetx_amd.ops import _lib
    Sq, q_starts, G = 129, [0, 64], 64
    c, qb, k, v, lens, ref = C.embedded(DEV, C.ST, Sq, q_starts, D, dtype, "peaked", [C.ST, C.ST])
    B, H = c.B, c.H
    big = torch.full((B, Sq + 2, H, D + 8), 3.0, device=DEV, dtype=dtype)
    stat = torch.full((G + B * H * Sq + G,), -7777.0, device=DEV)
    out, lse = big[:, 1:Sq + 1, :, :D], stat[G:G + B * H * Sq]
    qs = torch.tensor(q_starts, dtype=torch.int32, device=DEV)
    assert _raw(_lib.kernels(), qb, k, v, out, lse, qs, lens) == 0
    torch.cuda.synchronize()
    inner = torch.zeros(B, Sq + 2, H, D + 8, dtype=torch.bool, device=DEV)
    inner[:, 1:Sq + 1, :, :D] = True
    assert bool((big[~inner] == 3.0).all()), "guard elements written"
    assert bool((stat[:G] == -7777.0).all()) and bool((stat[-G:] == -7777.0).all())
    C.compare(ref, out, lse.view(B, H, Sq), dtype, "sentinels")


def test_rejected_calls_launch_nothing():
    """``fa_params()``'s codes (-1 head dim, -3 dtype), -5 without q_starts or
    kv_lens; every output keeps its sentinel."""
    from fleetx_amd.ops import _lib
    K = _lib.kernels()
    B, H, S, D = 1, 1, 32, 16
    q, k, v = (torch.randn(B, S, H, D, device=DEV).to(torch.bfloat16) for _ in range(3))
    out = torch.full((B, S, H, D), 3.0, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B * H * S,), -7777.0, device=DEV)
    z = torch.zeros(B, dtype=torch.int32, device=DEV)
    kl = torch.full((B,), S, dtype=torch.int32, device=DEV)
    assert _raw(K, q, k, v, out, lse, z, kl, D=12) == -1
    assert _raw(K, q, k, v, out, lse, z, kl, D=136) == -1
    assert _raw(K, q, k, v, out, lse, z, kl, dt=2) == -3
    assert _raw(K, q, k, v, out, lse, None, kl) == -5
    assert _raw(K, q, k, v, out, lse, z, None) == -5
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((lse == -7777.0).all())
    assert _raw(K, q, k, v, out, lse, z, kl) == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).any())


def test_formula_branches_and_checks():
    """Head dim 100 (GPU) and CPU tensors take the formula, held to the same
    reference; dtype and layout errors follow the decode wrappers."""
    from fleetx_amd import ops
    C.check_embedded(DEV, C.ST, 70, [65, 130], 100, torch.bfloat16, "peaked")
    C.check_embedded("cpu", C.ST, 70, [65, 130], 64, torch.bfloat16, "peaked")
    q = torch.randn(2, 8, 2, 64, device=DEV).to(torch.bfloat16)
    kc = torch.randn(2, 32, 2, 64, device=DEV).to(torch.bfloat16)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        ops.prefill_attention(q, kc, kc.half(), z, z + 8)
    with pytest.raises(ValueError):
        ops.prefill_attention(q, kc, kc.transpose(1, 2).contiguous().transpose(1, 2), z, z + 8)
    with pytest.raises(ValueError):
        ops.prefill_attention(q.clone().requires_grad_(), kc, kc, z, z + 8)


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_short_blocks_agree_with_window_formula(D, dtype):
    """Sq <= 8 on the same cache as the window decode formula (``lens =
    q_starts``, ``kv_lens = lens + W``): both round fp32 math once, the kernel
    also rounds P to 16 bits as its MFMA operand, hence O's own bound: 1 ulp
    plus ``e sum_j P_ij |v_j|`` <= 1 ulp + e max|v|."""
    from fleetx_amd.ops import attention as OA
    B, H, L = 2, 3, 160
    g = torch.Generator().manual_seed(5)
    kc = torch.randn(B, L, H, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(B, L, H, D, generator=g).to(dtype).to(DEV)
    lens = torch.tensor([17, 130], dtype=torch.int32, device=DEV)
    for W in (1, 5, 8):
        q = (0.5 * torch.randn(B, W, H, D, generator=g)).to(dtype).to(DEV)
        out = OA.prefill_attention(q, kc, vc, lens, lens + W)
        ref = OA._window_attention_formula(q.reshape(B * W, H, D), kc, vc, lens, W,
                                           1.0 / math.sqrt(D))
        e = 2.0 ** -A._MANT[dtype]
        floor = torch.full_like(ref, e * float(vc.float().abs().max()), dtype=torch.float64)
        A.assert_elementwise(out.reshape(B * W, H, D), ref.double(), dtype, floor, "W=%d" % W)


def test_graph_replay_reads_the_arrays():
    """q_starts / kv_lens are read by the kernel: one captured call replayed
    after the arrays changed gives the new offsets' result."""
    from fleetx_amd import ops
    Sq, D, dtype = 70, 64, torch.bfloat16
    # random inputs: K / V do not depend on kv_lens, so both cases share them
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
        ops.prefill_attention(q, k, v, qs, kl, scale=c.scale)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = ops.prefill_attention(q, k, v, qs, kl, scale=c.scale, return_lse=True)
    graph.replay()
    C.compare(ref_a, out, lse, dtype, "replay a")
    q.copy_(qb)
    qs.copy_(torch.tensor([3, 90], dtype=torch.int32))
    kl.copy_(torch.tensor([C.ST, 150], dtype=torch.int32))
    graph.replay()
    C.compare(ref_b, out, lse, dtype, "replay b")


# ------------------------------------------------- FLEETX_FA_PAIR=0 (child)
def _child_main():
    assert os.environ.get("FLEETX_FA_PAIR") == "0"
    n = 0
    try:
        for D in (64, 88, 128):
            for dtype in A.DTYPES:
                for Sq, q_starts in C.SHAPES:
                    C.check_embedded(DEV, C.ST, Sq, q_starts, D, dtype, "peaked")
                    n += 1
                C.check_embedded(DEV, 640, 300, [1, 340], D, dtype, "peaked")
                C.check_embedded(DEV, C.ST, 150, [0, 40], D, dtype, "random", kv_lens=[0, 200])
                n += 2
    except AssertionError as exc:
        print("FAILED after %d cases: %s" % (n, exc))
        return 1
    torch.cuda.synchronize()
    print("prefill attention child ok: %d cases" % n)
    return 0


def test_unpaired_grid_child():
    """FLEETX_FA_PAIR=0: one query block per workgroup in LPT order."""
    env = dict(os.environ)
    env["FLEETX_FA_PAIR"] = "0"
    r = subprocess.run([sys.executable, "-m", "tests.test_prefill_attention_gpu"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "prefill attention child ok" in r.stdout, r.stdout[-4000:]


if __name__ == "__main__":
    sys.exit(_child_main())
