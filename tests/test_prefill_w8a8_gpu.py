"""W8A8 prefill (csrc/kernels/prefill_gemm_i8.hip): the row quantiser bit for bit
against the torch formula, one-hot probes of both MFMA operands at every launch
shape, random int8 against the float64 result of the exact integer sum, the K
split's bit invariance, and ``Generation.prefill_act_quant``."""
import copy
import functools

import pytest
import torch

from tests.test_quant_prefill_gpu import _rel, small_model  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(mt, nt, ks) for mt in (4, 8) for nt in (1, 2, 4) for ks in (1, 2, 4)]  # all the library has


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(1, 1024), (67, 1024), (1, 3072), (67, 3072)])
def test_quantize_rows_bit_exact(dtype, M, K):
    """Row 0: sx = 2^-3 exactly and elements on the ties 0.5 / 1.5 / 2.5 sx; row 1
    all zero; row 2 with its largest element negative; contiguous and strided."""
    from fleetx_amd import ops
    x = torch.randn(M, K + 64, generator=torch.Generator().manual_seed(K + M)).clamp(-3, 3)
    x[0, 0], x[0, 1:7] = 15.875, torch.tensor([.0625, .1875, .3125, -.0625, -.1875, -.3125])
    if M > 2:
        x[1] = 0
        x[2, 9] = -5.0
    x = x.to(dtype)
    for xd in (x[:, :K].contiguous().to(DEV), x.to(DEV)[:, :K]):
        want_q, want_s = ops.quantize_weight_int8(x[:, :K])       # the formula, on the CPU
        q, s = ops.quantize_rows_int8(xd)
        assert q.dtype == torch.int8 and q.is_contiguous() and s.dtype == torch.float32
        assert torch.equal(s.cpu(), want_s) and int((q.cpu() != want_q).sum()) == 0
        assert s[0] == 0.125 and q[0, :7].tolist() == [127, 0, 2, 2, 0, -2, -2]
        if M > 2:
            assert s[1] == 1 and not q[1].any() and q[2, 9] == -127


def _positions(K):
    """Every residue mod 128 in the first and in the last chunk, and both sides
    of every boundary of a K split in 2 or 4."""
    return list(range(128)) + list(range(K - 128, K)) + \
        [K * j // 4 + d for j in (1, 2, 3) for d in (-1, 0)]


@functools.lru_cache(maxsize=None)
def _rand_i8(rows, K):
    g = torch.Generator().manual_seed(rows * 31 + K)
    return torch.randint(-127, 128, (rows, K), generator=g, dtype=torch.int8).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [40, 200])
@pytest.mark.parametrize("K", [1024, 3072])
@pytest.mark.parametrize("mt,nt,ks", SHAPES)
def test_operand_layout_probes(dtype, N, K, mt, nt, ks):
    """One-hot x rows must return columns of wq, one-hot weight rows columns of
    xq, exactly (integers up to 127 are exact in bf16 and fp16)."""
    from fleetx_amd.ops import gemm as G
    pos = _positions(K)
    for M in sorted({65, 16 * mt + 1}):
        one_m, one_n = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
        wq, xq = _rand_i8(N, K), _rand_i8(M, K)
        for i in range(0, len(pos), M):
            km = torch.tensor([pos[(i + m) % len(pos)] for m in range(M)], device=DEV)
            hot = torch.zeros(M, K, device=DEV, dtype=torch.int8)
            hot[torch.arange(M, device=DEV), km] = 1
            y = G.prefill_gemm_w8a8(hot, one_m, wq, one_n, out_dtype=dtype, shape=(mt, nt, ks))
            assert y is not None and y.dtype == dtype
            assert torch.equal(y, wq[:, km].t().to(dtype))
        for i in range(0, len(pos), N):
            kn = torch.tensor([pos[(i + n) % len(pos)] for n in range(N)], device=DEV)
            hot = torch.zeros(N, K, device=DEV, dtype=torch.int8)
            hot[torch.arange(N, device=DEV), kn] = 1
            y = G.prefill_gemm_w8a8(xq, one_m, hot, one_n, out_dtype=dtype, shape=(mt, nt, ks))
            assert torch.equal(y, xq[:, kn].to(dtype))


@functools.lru_cache(maxsize=None)
def _random_case(M, N, K):
    """Full-range int8 operands with +-127 planted, real scales, and the float64
    product ``sum * (sx * sw)`` from the exact integer sum.  The fp32 error of
    the epilogue is at most 2^-24 (2 |product| + |result|) (sx * sw and the
    multiply round relative to the product), so the bound below, 2^-21
    |result|, is a bound for an element only while |product| <= 3.5 |result|.
    The data keeps that for every element: the bias is zero on even columns and
    6 to 7 times the column's largest |product| on odd ones, and a residual has
    the sign of product + bias.  Shared; callers leave it unchanged."""
    g = torch.Generator().manual_seed(M + N + K)
    xq, wq = (torch.randint(-127, 128, (r, K), generator=g, dtype=torch.int8) for r in (M, N))
    xq[:, 0], wq[:, 0], wq[1, :] = 127, -127, 127
    sx = torch.rand(M, generator=g) * 0.02 + 0.01
    sw = torch.rand(N, generator=g) * 2e-4 + 1e-4
    acc = xq.double() @ wq.double().t()                 # exact: |sum| < 2^53
    ref = acc * (sx.double()[:, None] * sw.double()[None, :])
    bias = ref.abs().amax(0) * (6 + torch.rand(N, generator=g)) * (torch.arange(N) % 2) \
        * (1 - 2 * (torch.arange(N) % 4 // 2))
    res = torch.randn(M, N, generator=g).abs() * torch.sign(ref + bias.bfloat16().double())
    return tuple(t.to(DEV) for t in (xq, sx, wq, sw, bias.float(), res.float(), ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(65, 40, 1024), (129, 200, 3072)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_random_int8_against_float64(dtype, M, N, K, epi):
    """Bias / residual: half an ulp of the output type at the reference plus
    2^-21 |ref| (four fp32 roundings: int-to-float, sx * sw, the product, the
    bias add).  GeLU: the bound of tests/test_prefill_gemm_gpu.py's epilogues."""
    from fleetx_amd.ops import gemm as G
    xq, sx, wq, sw, bias, res, ref = _random_case(M, N, K)
    b, r = bias.to(dtype), res.to(dtype)
    y = G.prefill_gemm_w8a8(xq, sx, wq, sw, b, epi, res=r if epi == G.GV_RES else None)
    assert y is not None and y.dtype == dtype and y.shape == (M, N)
    ref = ref + b.double()
    if epi == G.GV_GELU:
        err = _rel(y, torch.nn.functional.gelu(ref, approximate="tanh"))
        print("rel err %.3g" % err)
        assert err < (8e-3 if dtype == torch.bfloat16 else 2e-3)
        return
    if epi == G.GV_RES:
        ref = ref + r.double()
    e = torch.frexp(ref.abs())[1] - 1                    # floor(log2 |ref|)
    if dtype == torch.float16:
        e = e.clamp_min(-14)
    half_ulp = torch.ldexp(torch.ones_like(ref), e - (8 if dtype == torch.bfloat16 else 11))
    over = (y.double() - ref).abs() - (half_ulp + 2.0 ** -21 * ref.abs())
    print("worst excess over the bound %.3g" % over.max().item())
    assert int((over > 0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mt,nt,ks", SHAPES)
def test_split_invariance(dtype, mt, nt, ks):
    """Every pinned launch gives the default launch's bits, each epilogue."""
    from fleetx_amd.ops import gemm as G
    xq, sx, wq, sw, bias, res, _ = _random_case(129, 200, 3072)
    b, r = bias.to(dtype), res.to(dtype)
    for epi in (G.GV_BIAS, G.GV_GELU, G.GV_RES):
        want = G.prefill_gemm_w8a8(xq, sx, wq, sw, b, epi, res=r)
        got = G.prefill_gemm_w8a8(xq, sx, wq, sw, b, epi, res=r, shape=(mt, nt, ks))
        assert want is not None and got is not None and torch.equal(want, got)


def _reference(model, dev, dtype, conf):
    """The unfused generator on a twin whose four layer linears read
    dequant(wq) and see their input rows through quantize_rows_int8's formula;
    the head reads its dequantised copy with 16-bit activations."""
    from fleetx_amd import ops
    from fleetx_amd.models.language_model.gpt import generation as gmod
    twin = copy.deepcopy(model).to(dev, dtype)

    def rows(mod, args):
        q, s = ops.quantize_weight_int8(args[0].reshape(-1, args[0].shape[-1]))
        return (ops.dequantize_weight_int8(q, s, args[0].dtype).view_as(args[0]),)
    with torch.no_grad():
        for layer in twin.gpt.layers:
            for lin in (layer.attn.qkv_proj, layer.attn.out_proj, layer.mlp.fc1, layer.mlp.fc2):
                lin.weight.copy_(ops.dequantize_weight_int8(*ops.quantize_weight_int8(lin.weight)))
                lin.register_forward_pre_hook(rows)
        table = twin.gpt.embeddings.word_embeddings.weight
        head = ops.dequantize_weight_int8(*ops.quantize_weight_int8(table)).to(dev, dtype)
    gen = gmod.GPTForGeneration(twin, dict(conf, fused_decode=False)).eval()
    gen._logits = lambda h, q8=None: torch.nn.functional.linear(h, head).float()
    return gen


@pytest.mark.parametrize("chunk,S", [(0, 96), (64, 160)])
def test_generation_prefill_act_quant(small_model, chunk, S):
    """Logits and the written K / V against the reference in fp32 (CPU).  The
    tolerance is the quantised-prefill test's 2e-2, or twice the spread between
    that reference in fp32 and in the model's dtype where the spread is larger:
    an input near a rounding tie quantises one step apart in the two."""
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = small_model
    B, conf = 3, {"prefill_chunk": chunk}
    ids = torch.randint(0, 1024, (B, S), generator=torch.Generator().manual_seed(13))
    lens = torch.tensor([S, 70, 33])
    a = gmod.GPTForGeneration(model, dict(conf, weight_quant="int8", weight_quant_prefill=True,
                                          prefill_act_quant="int8")).eval()
    assert a.requantize() is True
    runs = [(a, DEV, torch.bfloat16), (_reference(model, DEV, torch.bfloat16, conf), DEV,
                                       torch.bfloat16),
            (_reference(model, "cpu", torch.float32, conf), "cpu", torch.float32)]
    outs = []
    for gen, dev, dt in runs:
        cache = gmod.KVCache(cfg.num_layers, B, S, 8, 128, dt, dev)
        with torch.no_grad():
            lg = gen._prompt_logits(ids.to(dev), lens.to(dev), cache, lens.to(dev).int())
        outs.append([lg.cpu()] + [c[r, :int(lens[r])].cpu() for c in cache.k + cache.v
                                  for r in range(B)])
    spread = max(_rel(x, y) for x, y in zip(outs[1], outs[2]))
    err = max(_rel(x, y) for x, y in zip(outs[0], outs[2]))
    print("spread fp32 / bf16 reference %.3g, kernel path against fp32 %.3g" % (spread, err))
    assert err < max(2e-2, 2 * spread)


def test_generation_64_rows_keep_the_key_off_bits(small_model):
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = small_model
    ids = torch.randint(0, 1024, (2, 32), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    lens = torch.tensor([32, 20], device=DEV)
    outs = []
    for extra in ({}, {"prefill_act_quant": "int8"}):
        gen = gmod.GPTForGeneration(model, dict(extra, weight_quant="int8",
                                                weight_quant_prefill=True)).eval()
        assert gen.requantize() is True
        cache = gmod.KVCache(cfg.num_layers, 2, 32, 8, 128, torch.bfloat16, DEV)
        with torch.no_grad():
            outs.append([gen._prompt_logits(ids, lens, cache, lens.int())] + cache.k + cache.v)
    assert all(torch.equal(x, y) for x, y in zip(*outs))
