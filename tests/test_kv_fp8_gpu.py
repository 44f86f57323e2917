"""``kv_append_fp8_kernel`` and ``decode_attn_fp8_kernel`` (csrc/kernels/kv_fp8.hip)
on the MI355X: the append bit for bit against torch's e4m3 cast, the attention
against the float64 reference over the dequantised bytes with the a-priori bound
of tests/test_prefill_split_gpu.py (fp32 partials, one 16-bit rounding), and
``Generation.kv_cache_dtype: fp8_e4m3`` end to end."""
import pytest
import torch

from tests import test_attention_edges_gpu as A
from tests import test_kv_fp8_cpu as C
from tests.test_quant_prefill_gpu import _rel, small_model  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bytes(x):  # the issue's formula, on the CPU: independent of the device's converts
    return x.cpu().float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


@pytest.mark.parametrize("form", ["decode", "prefill", "unaligned"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_append_bit_exact(dtype, D, form):
    """decode: S 1 at pos, one row at maxlen (dropped); prefill: S 5 from 0 into 4
    rows (the fifth dropped); unaligned: the views start 8 bytes off a 16-byte
    boundary, which the host refuses and the wrapper's formula serves."""
    from fleetx_amd import ops
    B, H = 3, 2
    S, L = (1, 7) if form == "decode" else (5, 4)
    qkv = C.planted_qkv(B, S, H, D, dtype, DEV)
    if form == "unaligned":
        buf = torch.empty(qkv.numel() + 4, dtype=dtype, device=DEV)
        buf[4:] = qkv.reshape(-1)
        qkv = buf[4:].view(B, S, H, 3, D)
        assert qkv.data_ptr() % 16 == 8
    pos = torch.tensor([0, 4, L], dtype=torch.int32, device=DEV) if form == "decode" else None
    kc = torch.full((B, L, H, D), 0x55, dtype=torch.uint8, device=DEV)
    vc = kc.clone()
    ops.kv_append_fp8(qkv[:, :, :, 1], qkv[:, :, :, 2], kc, vc, pos)
    want_k = torch.full((B, L, H, D), 0x55, dtype=torch.uint8)
    want_v = want_k.clone()
    for b in range(B):
        p0 = int(pos[b]) if pos is not None else 0
        n = max(0, min(S, L - p0))
        want_k[b, p0:p0 + n] = _bytes(qkv[b, :n, :, 1])
        want_v[b, p0:p0 + n] = _bytes(qkv[b, :n, :, 2])
    assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v)


@pytest.mark.parametrize("nw", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_attention_against_float64(dtype, D, nw):
    """Lengths around one step's extent E = (64 / LPK) * NW * U of the pinned
    instantiation, one across the first split boundary that leaves the last of
    three splits empty, and the whole cache; NaN bytes at and past lens[b]."""
    from fleetx_amd import ops
    H, E = 2, (64 // (D // 16)) * nw * 4
    L = E + 70
    chunk = -(-L // 3)
    lens = torch.tensor([0, 1, E - 1, E, E + 1, chunk + 3, L], dtype=torch.int32, device=DEV)
    B = lens.numel()
    g = torch.Generator().manual_seed(D + nw)
    q = (0.5 * torch.randn(B, H, D, generator=g)).to(dtype).to(DEV)
    kb = _bytes(0.5 * torch.randn(B, L, H, D, generator=g)).to(DEV)
    vb = _bytes(torch.randn(B, L, H, D, generator=g)).to(DEV)
    dead = torch.arange(L, device=DEV).view(1, L) >= lens.view(B, 1)
    kb[dead], vb[dead] = 0x7F, 0x7F
    ref, tol = C.attention_ref(q, kb, vb, lens, dtype)
    for nsplit in (1, 3):
        out = ops.decode_attention_fp8(q, kb, vb, lens, nsplit=nsplit, nw=nw)
        assert int(torch.count_nonzero(out[0])) == 0
        A.assert_elementwise(out, ref, dtype, tol, "nsplit %d" % nsplit)
    auto = ops.decode_attention_fp8(q, kb, vb, lens, nsplit=1)  # the rule: 14 workgroups, NW 16
    assert torch.equal(auto, ops.decode_attention_fp8(q, kb, vb, lens, nsplit=1, nw=16))
    with pytest.raises(NotImplementedError):
        ops.decode_attention_fp8(q[:, :, :32].contiguous(), kb[..., :32].contiguous(),
                                 vb[..., :32].contiguous(), lens)


def _round_through_e4m3(cache):
    for t in cache.k + cache.v:
        t.copy_(t.float().clamp(-448, 448).to(torch.float8_e4m3fn).to(t.dtype))


def test_generation_end_to_end(small_model):  # noqa: F811
    """Prefill and four fused decode steps on the e4m3 cache against the unfused
    16-bit generator whose cache is rounded through e4m3 after every call; then
    the device loop (one graph replay per token) against the host loop."""
    from fleetx_amd.models.language_model.gpt import generation as gmod
    cfg, model = small_model
    B, S = 3, 96
    ids = torch.randint(0, 1024, (B, S), device=DEV,
                        generator=torch.Generator(device=DEV).manual_seed(13))
    lens = torch.tensor([S, 70, 33], device=DEV)
    a = gmod.GPTForGeneration(model, {"kv_cache_dtype": "fp8_e4m3", "fused_decode": True}).eval()
    b = gmod.GPTForGeneration(model, {"fused_decode": False}).eval()
    ca = a._new_cache(B, S + 8, torch.bfloat16, DEV)
    cb = b._new_cache(B, S + 8, torch.bfloat16, DEV)
    with torch.no_grad():
        la, lb = (g._prompt_logits(ids, lens, c, lens.int()) for g, c in ((a, ca), (b, cb)))
        _round_through_e4m3(cb)
        assert _rel(la, lb) < 2e-2
        cur = lens.clone()
        for step in range(4):
            nxt = lb.argmax(-1)
            la, lb = a._decode_step(nxt, cur, ca), b._decode_step(nxt, cur, cb)
            _round_through_e4m3(cb)
            r = _rel(la, lb)
            print("step %d rel %.3e" % (step, r))
            assert r < 2e-2
            cur += 1
    gcfg = {"kv_cache_dtype": "fp8_e4m3", "decode_strategy": "greedy_search", "max_dec_len": 6}
    host = gmod.GPTForGeneration(model, gcfg).eval().generate(ids, lens)[0]
    dev = gmod.GPTForGeneration(model, dict(gcfg, device_loop=True)).eval().generate(ids, lens)[0]
    assert host.shape == (B, 6) and torch.equal(host, dev)
