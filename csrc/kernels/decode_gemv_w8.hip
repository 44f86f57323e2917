// Weight-only int8 decode GEMV (W8A16): y[M, N] = x[M, K] (q[N, K] * s[N])^T,
// M <= 16, 16-bit x and y, int8 weights with one fp32 scale per output row
// (fleetx_amd/ops/quant.py): half the weight bytes per token of the 16-bit
// GEMV, on a decode step that is bound by the weight stream.
//
// The kernel, its launch ladder and the host entry are decode_gemv.h's; this
// file is the int8 weight operand, converted in registers:
//  * per 128-k chunk every lane loads 32 contiguous bytes of one q row and the
//    matching 32 x elements, for the chunk's four MFMA k-steps;
//  * each int8 is sign-extended and converted to fp32 (cvt8 in decode_gemv.h,
//    shared with the int4 operand), then packed to the
//    activation dtype (bf16: the upper half of the fp32, exact for |q| <= 127;
//    fp16: cvt_pkrtz, exact too) right before its MFMA -- ~1.5 VALU lane-ops
//    per element;
//  * loads run in batches of U = 2 chunks (1 where a wave's K range holds an
//    odd number) on two register sets, in the branch-free steady K loop;
//  * the epilogue multiplies the accumulator by the row scale before the bias.
// FLEETX_GEMV_W8_KS (4 / 8 waves), FLEETX_GEMV_W8_U (1: one chunk per batch)
// and FLEETX_GEMV_W8_ROWS (8 / 16 columns per block) pin the launch shape for
// tools/bench_gemv.py sweeps; the shapes were measured in profiles/decode_w8/
// (tools/bench_gemv.py --w8).
#include "decode_gemv.h"
#include "fx_api.h"

namespace {

struct W8 {
  typedef int8_t elt;
  typedef uintx4 reg;
  struct Ptrs {
    const int8_t* w;
    const float* scale;
    bool valid() const { return (uintptr_t)w % 16 == 0 && scale != nullptr; }
  };
  static constexpr int CHUNK = 128, PACK = 1;
  static constexpr bool SCALED = true, GROUPED = false;
  static constexpr int U = 2, U_MIN = 1;
  static constexpr bool STEADY_LOOP = true;
  static constexpr const char* PIN_KS = "FLEETX_GEMV_W8_KS";
  static constexpr const char* PIN_U = "FLEETX_GEMV_W8_U";
  static constexpr const char* PIN_ROWS = "FLEETX_GEMV_W8_ROWS";
  template <typename T, int U>
  static __device__ __forceinline__ void mma_batch(floatx4& acc, const uintx4 (&wv)[U][2],
                                                   const short8 (&xv)[U][4]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc = mma16<T>(cvt8<T>(wv[u][0].x, wv[u][0].y), xv[u][0], acc);
      acc = mma16<T>(cvt8<T>(wv[u][0].z, wv[u][0].w), xv[u][1], acc);
      acc = mma16<T>(cvt8<T>(wv[u][1].x, wv[u][1].y), xv[u][2], acc);
      acc = mma16<T>(cvt8<T>(wv[u][1].z, wv[u][1].w), xv[u][3], acc);
    }
  }
};

}  // namespace

extern "C" int fx_decode_gemv_w8(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                 const int8_t* wq, long ldw, const float* wscale,
                                 const void* bias, const void* res, long ldres, void* y, long ldy,
                                 void* kc, void* vc, const long* pos, const int* rows, int heads, int head_dim,
                                 int maxlen, const void* ln_w, const void* ln_b, float ln_eps,
                                 hipStream_t s) {
  return gemv_entry<W8>(dt, epi, M, N, K, x, ldx, W8::Ptrs{wq, wscale}, ldw, bias, res, ldres, y,
                        ldy, kc, vc, pos, rows, heads, head_dim, maxlen, ln_w, ln_b, ln_eps, s);
}
