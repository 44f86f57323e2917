// Weight-only int4 decode GEMV (W4A16, group size 256):
//   y[M, N] = x[M, K] (q[N, K] * s[K / 256, N])^T,  M <= 16, 16-bit x and y,
// symmetric int4 weights with one fp32 scale per (k-group of 256, output row)
// (fleetx_amd/ops/quant.py: quantize_weight_int4): a quarter of the weight
// bytes per token of the 16-bit GEMV, on a decode step that is bound by the
// weight stream.
//
// Packed layout (only pack_int4 / unpack_int4 in ops/quant.py and this file
// know it).  A row of K weights is K / 2 bytes.  Each aligned run of 8 weights
// q[8i .. 8i+7] is the 4 bytes 4i .. 4i+3: byte j holds q[8i + j] in its low
// nibble and q[8i + j + 4] in its high nibble, both as 4-bit two's complement.
// A lane's 32 contiguous bytes of a chunk are thus its aligned 64-weight run,
// one dword per MFMA k-step, and a dword becomes its operand with two masks:
//   (v << 4) & 0xF0F0F0F0   bytes = 16 * q[8i + 0..3]   (int8, exact)
//    v       & 0xF0F0F0F0   bytes = 16 * q[8i + 4..7]
// which are int8 operands for the W8 conversion (cvt8 in decode_gemv.h).  The
// factor 16 is exact in bf16 and fp16 (|16 q| <= 128) and leaves with the
// scale: the chunk sum is multiplied by scale / 16.
//
// The kernel, its launch ladder and the host entry are decode_gemv.h's; this
// file is the int4 weight operand with the grouped scale (W::GROUPED):
//  * CHUNK = 256 = one scale group: every lane loads 32 contiguous bytes (64
//    weights) of one row and the matching 64 x elements, for the chunk's eight
//    MFMA k-steps, and the four scales scale[chunk, n] of its accumulator
//    columns in the same batch;
//  * the eight MFMAs of a chunk start from C = 0; the chunk sum then enters the
//    accumulator as fma(sum, scale / 16, acc), so nothing is left for the
//    epilogue (SCALED = false);
//  * conversion cost (hipcc -S, bf16 and fp16 alike): per dword 3 mask / shift
//    ops, 8 sign-extending byte converts and 4 packs = 15 VALU ops per 8
//    weights, ~1.9 per weight;
//  * loads run in batches of U = 1 chunk on two register sets, in the
//    branch-free steady K loop.  The x operand of a chunk is 32 VGPRs, so two
//    chunks per batch take 238-254 VGPRs (1-2 waves per SIMD, 1 with the
//    LayerNorm prologue) against 122-148 (3-4 waves); one chunk measured
//    faster at M <= 4 on most shapes and 15-21 % faster per generated token.
// FLEETX_GEMV_W4_KS (4 / 8 waves) and FLEETX_GEMV_W4_ROWS (8 / 16 columns per
// block) pin the launch shape for tools/bench_gemv.py sweeps; the shapes were
// measured in profiles/decode_w4/ (tools/bench_gemv.py --w4).
#include "decode_gemv.h"
#include "fx_api.h"

namespace {

// eight int4 (one dword, layout above) -> one MFMA operand holding 16 * q
template <typename T>
__device__ __forceinline__ short8 cvt8n(uint32_t v) {
  return cvt8<T>((v << 4) & 0xF0F0F0F0u, v & 0xF0F0F0F0u);
}

struct W4 {
  typedef uint8_t elt;
  typedef uintx4 reg;
  struct Ptrs {
    const uint8_t* w;
    const float* scale;  // [K / 256, N]
    bool valid() const { return (uintptr_t)w % 16 == 0 && scale != nullptr; }
  };
  static constexpr int CHUNK = 256, PACK = 2;
  static constexpr bool SCALED = false, GROUPED = true;
  static constexpr int U = 1, U_MIN = 1;
  static constexpr bool STEADY_LOOP = true;
  static constexpr const char* PIN_KS = "FLEETX_GEMV_W4_KS";
  static constexpr const char* PIN_U = nullptr;
  static constexpr const char* PIN_ROWS = "FLEETX_GEMV_W4_ROWS";
  template <typename T, int U>
  static __device__ __forceinline__ void mma_batch(floatx4& acc, const uintx4 (&wv)[U][2],
                                                   const short8 (&xv)[U][8],
                                                   const floatx4 (&sv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      floatx4 t = {0.f, 0.f, 0.f, 0.f};
      t = mma16<T>(cvt8n<T>(wv[u][0].x), xv[u][0], t);
      t = mma16<T>(cvt8n<T>(wv[u][0].y), xv[u][1], t);
      t = mma16<T>(cvt8n<T>(wv[u][0].z), xv[u][2], t);
      t = mma16<T>(cvt8n<T>(wv[u][0].w), xv[u][3], t);
      t = mma16<T>(cvt8n<T>(wv[u][1].x), xv[u][4], t);
      t = mma16<T>(cvt8n<T>(wv[u][1].y), xv[u][5], t);
      t = mma16<T>(cvt8n<T>(wv[u][1].z), xv[u][6], t);
      t = mma16<T>(cvt8n<T>(wv[u][1].w), xv[u][7], t);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(t[j], sv[u][j] * 0.0625f, acc[j]);
    }
  }
};

}  // namespace

extern "C" int fx_decode_gemv_w4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                 const uint8_t* wq, long ldw, const float* wscale,
                                 const void* bias, const void* res, long ldres, void* y, long ldy,
                                 void* kc, void* vc, const long* pos, const int* rows, int heads, int head_dim,
                                 int maxlen, const void* ln_w, const void* ln_b, float ln_eps,
                                 hipStream_t s) {
  return gemv_entry<W4>(dt, epi, M, N, K, x, ldx, W4::Ptrs{wq, wscale}, ldw, bias, res, ldres, y,
                        ldy, kc, vc, pos, rows, heads, head_dim, maxlen, ln_w, ln_b, ln_eps, s);
}
