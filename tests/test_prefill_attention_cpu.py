"""``ops.prefill_attention`` on CPU tensors (the fp32 formula branch) against
the float64 reference and a-priori bounds of tests/test_attention_edges_gpu.py.

Reference by embedding: a causal SELF-attention of ``St`` tokens is built
(``A.Case(St, mode="causal", kv_lens=...)``); the block of ``Sq`` queries that
starts at ``q_starts[b]`` must reproduce rows ``q_starts[b] .. q_starts[b] +
Sq - 1`` of that reference (O with the ``tO`` slice, lse with ``tlse``), every
element, zero elements out of bounds.  tests/test_prefill_attention_gpu.py runs
the same checks on the kernel.

The two self-checks show that the comparison separates the offset diagonal
from its neighbours without any kernel: the top-left aligned result of
``attention_reference`` (today's causal mask for Sq != Sk) and a diagonal
shifted by one key must both fail.  They need the diagonal, not ``kv_len``, to
be the binding limit, so ``kv_lens`` is the whole sequence there."""
import math

import pytest
import torch

from tests import test_attention_edges_gpu as A

CPU = "cpu"
ST = 200
# (Sq, q_starts): a block across two 64-key tiles, single rows at both ends,
# a block below one wave, and one of more than a 128-row query block
SHAPES = [(70, [65, 130]), (1, [0, 199]), (33, [31, 127]), (129, [0, 64])]


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def embedded(dev, St, Sq, q_starts, D, dtype, inputs, kv_lens, H=3):
    """The causal self-attention case and its reference, the query block of
    every sample, and the reference rows that block must reproduce."""
    c = A.Case(St, D=D, dtype=dtype, mode="causal", inputs=inputs, kv_lens=kv_lens, H=H)
    q, k, v, dO, lens, _ = A.make_inputs(c, dev)
    R = A.reference(q, k, v, dO, True, 0.0, c.key, c.scale, lens)
    qb = torch.stack([q[b, s:s + Sq] for b, s in enumerate(q_starts)])
    ref = {"O": torch.stack([R["O"][b, s:s + Sq] for b, s in enumerate(q_starts)]),
           "tO": torch.stack([R["tO"][b, s:s + Sq] for b, s in enumerate(q_starts)]),
           "lse": torch.stack([R["lse"][b, :, s:s + Sq] for b, s in enumerate(q_starts)]),
           "tlse": torch.stack([R["tlse"][b, :, s:s + Sq] for b, s in enumerate(q_starts)])}
    return c, qb, k, v, lens, ref


def compare(ref, out, lse, dtype, what):
    A.assert_elementwise(out, ref["O"], dtype, ref["tO"], what + " O")
    A.assert_fp32(lse, ref["lse"], ref["tlse"], what + " lse")


def check_embedded(dev, St, Sq, q_starts, D, dtype, inputs, kv_lens=None):
    from fleetx_amd import ops
    kv = kv_lens if kv_lens is not None else [St] * len(q_starts)
    c, qb, k, v, lens, ref = embedded(dev, St, Sq, q_starts, D, dtype, inputs, kv)
    qs = torch.tensor(q_starts, dtype=torch.int32, device=dev)
    out, lse = ops.prefill_attention(qb, k, v, qs, lens, scale=c.scale, return_lse=True)
    compare(ref, out, lse, dtype, "%r Sq=%d q_starts=%s" % (c, Sq, q_starts))
    return out, lse


def diagonal_binds(St, Sq, q_starts):
    return [min(St, s + Sq + 5) for s in q_starts]


@pytest.mark.parametrize("inputs", ["random", "peaked", "probe"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,q_starts", SHAPES)
def test_formula_embedded(Sq, q_starts, dtype, D, inputs):
    check_embedded(CPU, ST, Sq, q_starts, D, dtype, inputs)


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,q_starts", SHAPES)
def test_formula_diagonal_binds(Sq, q_starts, dtype):
    check_embedded(CPU, ST, Sq, q_starts, 64, dtype, "peaked",
                   kv_lens=diagonal_binds(ST, Sq, q_starts))


def test_formula_other_cases():
    """D 88 and 100, three query blocks, plain causal, a padding chunk."""
    check_embedded(CPU, ST, 70, [65, 130], 88, torch.bfloat16, "peaked")
    check_embedded(CPU, ST, 70, [65, 130], 100, torch.float16, "peaked")
    check_embedded(CPU, 640, 300, [1, 340], 64, torch.bfloat16, "peaked")
    check_embedded(CPU, ST, 200, [0, 0], 64, torch.float16, "peaked")
    # padding chunk: every row of sample 0 lies past kv_len and sees all 120 keys,
    # which is what the embedded reference gives rows past kv_len
    check_embedded(CPU, ST, 50, [150, 10], 64, torch.bfloat16, "peaked", kv_lens=[120, 200])


def test_formula_empty_sample_and_masked_nan():
    """kv_len 0: exact zeros and +inf.  Keys no row sees may hold NaN."""
    from fleetx_amd import ops
    out, lse = check_embedded(CPU, ST, 33, [0, 40], 64, torch.bfloat16, "random",
                              kv_lens=[0, 100])
    assert int(torch.count_nonzero(out[0])) == 0
    assert bool((lse[0] == math.inf).all())
    c, qb, k, v, lens, ref = embedded(CPU, ST, 33, [31, 127], 64, torch.float16, "random",
                                      [80, 150])
    k, v = k.clone(), v.clone()
    k[0, 80:], v[0, 80:] = math.nan, math.nan       # past kv_len
    k[1, 160:], v[1, 160:] = math.nan, math.nan     # past the last row's diagonal (and kv_len)
    out, lse = ops.prefill_attention(qb, k, v, torch.tensor([31, 127]), lens, scale=c.scale,
                                     return_lse=True)
    compare(ref, out, lse, torch.float16, "NaN in masked keys")


@pytest.mark.parametrize("inputs", ["random", "peaked", "probe"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,q_starts", SHAPES)
def test_checker_rejects_top_left(Sq, q_starts, dtype, D, inputs):
    """Today's causal mask for Sq != Sk (``attention_reference``) fails in every case."""
    from fleetx_amd import ops
    c, qb, k, v, lens, ref = embedded(CPU, ST, Sq, q_starts, D, dtype, inputs, [ST, ST])
    out = ops.attention_reference(qb, k, v, causal=True, scale=c.scale, kv_lens=lens)
    with pytest.raises(AssertionError):
        A.assert_elementwise(out, ref["O"], dtype, ref["tO"], "top left")


@pytest.mark.parametrize("inputs", ["random", "peaked", "probe"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,q_starts", [s for s in SHAPES if s[0] > 1])
def test_checker_rejects_diagonal_plus_one(Sq, q_starts, dtype, D, inputs):
    """A diagonal shifted by one key fails in every case with Sq > 1 (the
    single row at position 199 of 200 has no further key to admit)."""
    from fleetx_amd import ops
    c, qb, k, v, lens, ref = embedded(CPU, ST, Sq, q_starts, D, dtype, inputs, [ST, ST])
    out = ops.prefill_attention(qb, k, v, torch.tensor(q_starts) + 1, lens, scale=c.scale)
    with pytest.raises(AssertionError):
        A.assert_elementwise(out, ref["O"], dtype, ref["tO"], "diagonal + 1")


def test_agrees_with_window_formula():
    """Sq <= 8: the window decode formula on the same cache."""
    from fleetx_amd.ops import attention as OA
    B, W, H, D, L = 2, 5, 3, 64, 96
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, W, H, D, generator=g)
    kc, vc = torch.randn(B, L, H, D, generator=g), torch.randn(B, L, H, D, generator=g)
    lens = torch.tensor([17, 64])
    scale = 1.0 / math.sqrt(D)
    out = OA.prefill_attention(q, kc, vc, lens, lens + W, scale=scale)
    ref = OA._window_attention_formula(q.reshape(B * W, H, D), kc, vc, lens, W, scale)
    assert float((out.reshape(B * W, H, D) - ref).abs().max()) <= 2e-6


def test_argument_checks():
    from fleetx_amd import ops
    q = torch.randn(2, 4, 3, 64)
    kc, vc = torch.randn(2, 16, 3, 64), torch.randn(2, 16, 3, 64)
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.prefill_attention(q.clone().requires_grad_(), kc, vc, z, z + 4)
    with pytest.raises(ValueError):
        ops.prefill_attention(q, kc.clone().requires_grad_(), vc, z, z + 4)
    with pytest.raises(ValueError):
        ops.prefill_attention(q, kc, vc[:, :8], z, z + 4)
    with pytest.raises(ValueError):
        ops.prefill_attention(q, kc, vc, z[:1], z + 4)
    out = ops.prefill_attention(q, kc, vc, z, z + 4)
    assert out.shape == q.shape and out.dtype == q.dtype
