"""Hot-path ops: HIP/CDNA4 kernels on GPU tensors, reference math on CPU."""
from .norm import add_layer_norm, layer_norm, layer_norm_keep_input, FusedLayerNorm, col_sum  # noqa: F401
from .elementwise import bias_gelu, bias_dropout_add, dropout  # noqa: F401
from .attention import (flash_attention, flash_attention_qkvpacked, attention_reference,  # noqa: F401
                        decode_attention, beam_decode_attention, window_decode_attention,
                       prefill_attention)
from .loss_embed import softmax_cross_entropy, embedding  # noqa: F401
from .quant import fake_quant, quantize_weight_int8, dequantize_weight_int8  # noqa: F401
from .quant import (quantize_weight_int4, dequantize_weight_int4, pack_int4,  # noqa: F401
                    unpack_int4)
from .sampling import fused_sample, select_token, SelectState  # noqa: F401
from .sampling import spec_verify, SpecState  # noqa: F401
from .sampling import coupled_sample, coupled_keys  # noqa: F401
from .softmax import (fused_softmax, softmax_mask_fuse,  # noqa: F401
                      softmax_mask_fuse_upper_triangle)
from . import _lib  # noqa: F401
from .groupnorm import group_norm_silu, GroupNormSiLU  # noqa: F401,E402
