"""The PyTorch formula branch of ``ops.flash_attention`` (CPU tensors;
``attention_reference``: fp32, output rounded once) against the float64
reference and the a-priori bounds of tests/test_attention_edges_gpu.py, and
the checker's self-test.

The first part shows that the references and bounds are satisfied by a
correct implementation that shares no code with the kernels.  The second
shows without any kernel that the comparison has teeth: outputs computed from
a deliberately wrong mask must raise.  The motivation is the two measurements
of the GPU module's docstring (float64 model, B*H = 8, S = 384, D = 64, randn
inputs): one extra key on the last row of each 64-key tile moves O by 0.0071
in the Frobenius norm, the last key dropped for every row by 0.0012, and the
norm tests of tests/test_kernels_gpu.py pass anything below 0.02."""
import pytest
import torch

from tests import test_attention_edges_gpu as A

Case = A.Case
CPU = "cpu"
BF16, FP16 = torch.bfloat16, torch.float16


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


# ------------------------------------------- the formula branch, same checks
@pytest.mark.parametrize("inputs,p", [("random", 0.0), ("peaked", 0.1)])
@pytest.mark.parametrize("mode", ["causal", "plain"])
def test_every_sequence_length_cpu(mode, inputs, p):
    for S in A.SEQ_ALL:
        A.check_case(CPU, Case(S, D=64, mode=mode, p=p, inputs=inputs))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("D", [64, 128, 8, 88, 100])
def test_config_sweep_cpu(D, dtype, mode, p):
    for S in (33, 129, 300):
        A.check_case(CPU, Case(S, D=D, dtype=dtype, mode=mode, p=p, inputs="peaked"))


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, FP16)])
def test_probability_probes_cpu(D, dtype, mode, p):
    A.check_case(CPU, Case(300, D=D, dtype=dtype, mode=mode, p=p, inputs="probe"))


def test_probes_are_the_probability_matrix():
    """What the probe construction promises: O[i, c] = Pd[i, j0 + c] and
    dV[j, c] = Pd[i0 + c, j], exact zeros where masked or dropped."""
    from fleetx_amd.parallel import rng
    c = Case(300, D=64, mode="causal", p=0.5, inputs="probe")
    q, k, v, dO, _, _ = A.make_inputs(c, CPU)
    R = A.reference(q, k, v, dO, True, c.p, c.key, c.scale)
    keep = rng.attention_keep_mask(c.B * c.H, 300, 300, c.p, c.key).view(c.B, c.H, 300, 300)
    kw, qw = A._windows(300, 64), A._windows(300, 64)
    for b in range(c.B):
        for h in range(c.H):
            j0, i0 = kw[(b * c.H + h) % 6], qw[(b * c.H + h + 2) % 6]
            n = min(64, 300 - j0)
            O = R["O"][b, :, h, :n]                              # [Sq, n]
            live = keep[b, h, :, j0:j0 + n] & (torch.arange(j0, j0 + n).view(1, n)
                                              <= torch.arange(300).view(300, 1))
            assert torch.equal(O != 0, live)
            assert float(R["tO"][b, :, h, :n][~live].abs().max()) == 0.0
            m = min(64, 300 - i0)
            dV = R["dV"][b, :, h, :m]                            # [Sk, m]
            live = keep[b, h, i0:i0 + m, :].t() & (torch.arange(300).view(300, 1)
                                                   <= torch.arange(i0, i0 + m).view(1, m))
            assert torch.equal(dV != 0, live)
    assert {j0 % 2 for j0 in kw} == {0, 1}                       # both keys of a hash pair lead


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", ["causal", "plain"])
@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, FP16)])
def test_kv_lens_cpu(D, dtype, mode, p):
    for lens in A.kv_len_groups(300):
        A.check_case(CPU, Case(300, D=D, dtype=dtype, mode=mode, p=p, inputs="peaked",
                               kv_lens=lens))


@pytest.mark.parametrize("bias", [None, "imagen", "pad1e4"])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,Sk", A.CROSS_SHAPES)
def test_cross_attention_cpu(Sq, Sk, dtype, bias):
    for inputs in ("random", "peaked"):
        A.check_case(CPU, Case(Sq, Sk, D=64, dtype=dtype, p=0.1, inputs=inputs, bias=bias,
                               bias_lens=[max(1, Sk - 5), 0]))


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_cross_attention_broadcast_kv_head_cpu(dtype):
    A.check_case(CPU, Case(33, 129, D=64, dtype=dtype, layout="mqa"))


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("Sq,Sk", [(97, 200), (200, 97)])
def test_causal_cross_attention_top_left_cpu(Sq, Sk, dtype):
    for inputs in ("peaked", "probe"):
        A.check_case(CPU, Case(Sq, Sk, D=64, dtype=dtype, mode="causal", p=0.1, inputs=inputs))


@pytest.mark.parametrize("layout", ["packed3", "packed2", "sp"])
def test_layouts_cpu(layout):
    A.check_case(CPU, Case(129, D=88, mode="causal", p=0.1, inputs="peaked", layout=layout))


def test_key_bias_with_causal_is_rejected():
    from fleetx_amd import ops
    q = torch.zeros(1, 4, 1, 8, dtype=BF16)
    with pytest.raises(ValueError, match="non-causal"):
        ops.flash_attention(q, q, q, causal=True, key_bias=torch.zeros(1, 4))


# ------------------------------------------------------ the checker has teeth
def test_peaked_keys_cover_the_boundaries():
    ks = A.peaked_keys(300, 137)
    for j in (0, 31, 32, 33, 63, 64, 65, 96, 128, 136, 137, 192, 256, 288, 299):
        assert j in ks
    assert len(ks) < 40 and A.peaked_keys(1, 1) == [0]


def _outputs(c, wrong):
    """The float64 reference and, rounded to the 16-bit type as a perfect
    kernel would return them, the outputs of the same math under a wrong mask."""
    q, k, v, dO, lens, bias = A.make_inputs(c, CPU)
    R = A.reference(q, k, v, dO, c.causal, c.p, c.key, c.scale, lens, bias)
    W = A.reference(q, k, v, dO, c.causal, c.p, c.key, c.scale, lens, bias, wrong=wrong)
    exact = {n: R[n].to(c.dtype) for n in ("O", "dQ", "dK", "dV")}
    exact.update(lse=R["lse"].float(), delta=R["delta"].float())
    got = {n: W[n].to(c.dtype) for n in ("O", "dQ", "dK", "dV")}
    got.update(lse=W["lse"].float(), delta=W["delta"].float())
    return R, exact, got


@pytest.mark.parametrize("wrong,mode,p", [("extra_key", "causal", 0.0),
                                          ("drop_last", "plain", 0.0),
                                          ("swap_keep", "plain", 0.1),
                                          ("swap_keep", "causal", 0.5)])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("inputs", ["random", "peaked", "probe"])
def test_checker_sees_a_wrong_mask(inputs, dtype, wrong, mode, p):
    """The rounded reference passes; the same math with one mask mistake fails
    on the output alone, on each gradient of K and V alone, and on lse where
    the mistake changes the row sum."""
    c = Case(300, D=64, dtype=dtype, mode=mode, p=p, inputs=inputs)
    R, exact, got = _outputs(c, wrong)
    A.compare(R, exact, dtype)
    for name in ("O", "dK", "dV"):
        with pytest.raises(AssertionError, match=r"elements off; worst at"):
            A.compare(R, {name: got[name]}, dtype)
    if wrong != "swap_keep":
        with pytest.raises(AssertionError, match=r"lse: \d+ of"):
            A.compare(R, {"lse": got["lse"]}, dtype)


def test_checker_points_at_the_row_and_key():
    """The extra key on rows 63 and 127 shows up on those rows and no other."""
    c = Case(129, D=64, mode="causal", inputs="probe", B=1, H=1)
    R, _, got = _outputs(c, "extra_key")
    # (b, h) = (0, 0) probes keys 0..63 on columns 0..63: the leaked keys 64 and
    # 128 lie outside that window, the rows that admit them lose that mass
    bad = ~((got["O"].double() - R["O"]).abs() <= A.ulp(R["O"], c.dtype) + R["tO"])
    rows = bad.nonzero()[:, 1].unique().tolist()
    assert rows == [63, 127], rows
    with pytest.raises(AssertionError, match=r"worst at \(0, (63|127), 0, \d+\)"):
        A.compare(R, {"O": got["O"]}, c.dtype)


def test_assert_fp32_needs_matching_infinities():
    ref = torch.tensor([1.0, float("inf")], dtype=torch.float64)
    tol = torch.full((2,), 1e-3, dtype=torch.float64)
    A.assert_fp32(torch.tensor([1.0005, float("inf")]), ref, tol)
    for bad in ([1.0, 3e38], [1.0, float("-inf")], [1.002, float("inf")],
                [float("nan"), float("inf")]):
        with pytest.raises(AssertionError):
            A.assert_fp32(torch.tensor(bad), ref, tol)
