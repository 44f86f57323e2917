"""Weight-only int4 (group size 256) for decoding, the parts that need no GPU:
the nibble packing, the grouped quantiser (ops.quantize_weight_int4) and the
``weight_quant: int4_g256`` generation key."""
import os
import warnings

import pytest
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
from fleetx_amd.models.language_model.gpt import generation as G


def _weight(dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(37, 1024, generator=g) * 1024 ** -0.5).to(dtype)
    w[17, 256:512] = 0          # one all-zero group
    return w


def test_pack_unpack_round_trip_all_codes():
    g = torch.Generator().manual_seed(1)
    q = torch.arange(-8, 8, dtype=torch.int8).repeat(5, 16)          # [5, 256], every code
    q = q[:, torch.randperm(256, generator=g)]
    assert sorted(set(q.flatten().tolist())) == list(range(-8, 8))
    p = ops.pack_int4(q)
    assert p.dtype == torch.uint8 and p.shape == (5, 128) and p.is_contiguous()
    back = ops.unpack_int4(p)
    assert back.dtype == torch.int8 and torch.equal(back, q)
    # every byte value unpacks and packs back to itself: the map is a bijection
    allb = torch.arange(256, dtype=torch.uint8).view(1, 256)
    assert torch.equal(ops.pack_int4(ops.unpack_int4(allb)), allb)


def test_quantizer_shapes_range_and_scale():
    w = _weight()
    p, s = ops.quantize_weight_int4(w)
    assert p.dtype == torch.uint8 and p.shape == (37, 512) and p.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (4, 37) and s.is_contiguous()
    q = ops.unpack_int4(p)
    assert int(q.min()) >= -7 and int(q.max()) <= 7
    amax = w.float().view(37, 4, 256).abs().amax(2).t()               # [4, 37]
    nz = torch.ones(4, 37, dtype=torch.bool)
    nz[1, 17] = False
    assert torch.equal(s[nz], (amax / 7.0)[nz])
    assert torch.allclose(s[nz] * 7, amax[nz], rtol=2e-7, atol=0)
    assert torch.equal(q.view(37, 4, 256).abs().amax(2).t()[nz], torch.full((147,), 7, dtype=torch.int8))
    assert float(s[1, 17]) == 1.0 and int(q[17, 256:512].abs().max()) == 0


def test_quantizer_error_is_half_a_step_of_its_group():
    w = _weight()
    p, s = ops.quantize_weight_int4(w)
    d = ops.dequantize_weight_int4(p, s)
    step = s.t()[:, :, None]                                           # [37, 4, 1]
    err = (w.float() - d).view(37, 4, 256).abs() / step
    print("worst |w - q*scale| / scale = %.6f" % float(err.max()))
    assert float(err.max()) <= 0.5001
    # the dequantiser is q * scale in fp32, rounded once
    q = ops.unpack_int4(p).view(37, 4, 256).float()
    assert torch.equal(d, (q * step).view(37, 1024))
    assert torch.equal(ops.dequantize_weight_int4(p, s, torch.bfloat16), (q * step).view(37, 1024).bfloat16())


def test_quantizer_rejects_k_not_multiple_of_256():
    with pytest.raises(ValueError):
        ops.quantize_weight_int4(torch.zeros(4, 384))
    with pytest.raises(ValueError):
        ops.quantize_weight_int4(torch.zeros(4, 64))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantizer_takes_any_float_dtype(dtype):
    p, s = ops.quantize_weight_int4(_weight(dtype))
    assert p.dtype == torch.uint8 and p.shape == (37, 512)
    assert s.dtype == torch.float32 and s.shape == (4, 37)
    if dtype == torch.float32:  # bf16 -> fp32 is exact: the same codes and scales
        p2, s2 = ops.quantize_weight_int4(_weight(torch.bfloat16))
        w32 = _weight(torch.bfloat16).float()
        p3, s3 = ops.quantize_weight_int4(w32)
        assert torch.equal(p2, p3) and torch.equal(s2, s3)


def _model():
    torch.manual_seed(2)
    cfg = GPTConfig(vocab_size=97, hidden_size=64, num_layers=2, num_attention_heads=4,
                    max_position_embeddings=64, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0)
    return GPTForPretraining(cfg).eval()


def test_weight_quant_int4_g256_constructs_and_is_ignored_on_cpu():
    m = _model()
    gen = G.GPTForGeneration(m, {"weight_quant": "int4_g256"})
    assert gen.weight_quant == "int4_g256"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert gen.requantize() is False
        assert gen.requantize() is False
    assert len([r for r in rec if "weight_quant" in str(r.message)]) == 1
    # the accepted values are listed when an unknown one is rejected
    with pytest.raises(ValueError, match="weight_quant.*int8.*int4_g256"):
        G.GPTForGeneration(m, {"weight_quant": "int3"})


def test_int4_config_file_loads_with_the_key_set():
    from fleetx_amd.utils import config as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.get_config(
        os.path.join(root, "fleetx_amd", "configs", "nlp", "gpt", "generation_gpt_345M_int4.yaml"),
        overrides=["Global.device=cpu"], nranks=1)
    assert cfg["Generation"]["weight_quant"] == "int4_g256"
