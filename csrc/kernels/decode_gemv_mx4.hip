// Weight-only MXFP4 decode GEMV (W4A16, OCP microscaling FP4):
//   y[M, N] = x[M, K] (fp4[N, K] * 2^(e[N, K / 32] - 127))^T,  M <= 16,
// 16-bit x and y, e2m1 weights (sign, two exponent bits, one mantissa bit:
// +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}) with one e8m0 power-of-two scale per (row,
// group of 32 k) (fleetx_amd/ops/quant.py: quantize_weight_mxfp4): 4.25 bits
// per weight.
//
// gfx950 converts this format in hardware: v_cvt_scalef32_pk_{bf16,f16}_fp4
// takes a dword, a byte selector and an fp32 scale and returns the byte's two
// fp4 values times the scale as two packed 16-bit floats -- half an MFMA
// operand register.  A dword of eight weights becomes one short8 A operand in
// four VALU ops (0.5 per weight, int4's mask / convert / pack sequence takes
// 15) with the group scale already applied, so the eight MFMAs of a chunk
// accumulate straight into acc: no zero tile per chunk, no accumulator fma,
// nothing for the epilogue (SCALED = GROUPED = false, OPSCALED = true).
//
// Packed layout (only pack_mxfp4 / unpack_mxfp4 in ops/quant.py, this file and
// GM4 in decode_gemm.hip know it).  Weights: a row of K weights is K / 2
// bytes, byte i holds weight 2i in its low nibble and weight 2i + 1 in its
// high nibble -- the order in which the convert instruction unpacks a byte
// (selector j: byte j of the dword; result: low nibble, high nibble).  A lane's
// 32 contiguous bytes of a chunk are its 64-weight run in k order, one dword
// per MFMA k-step.  Scales: one byte e per group, value 2^(e - 127), and the
// fp32 scale operand is e << 23 (e in 1..254).  A row's K / 32 scale bytes are
// stored in blocks of 16 (512 k, a pair of 256-k chunks) ordered [lane group
// g][chunk of the pair][half]: the dword at byte 4 g of a block is lane group
// g's two scales of the even chunk (k 64 g .. 64 g + 63 of it: two groups) and
// its two of the odd chunk.  A lane so fetches the scales of two chunks in one
// dword load, from the row it streams, in the batch that loads the weights.
//
// The kernel, its launch ladder and the host entry are decode_gemv.h's.
//  * CHUNK = 256: 32 contiguous bytes per lane, the matching 64 x elements,
//    eight MFMA k-steps -- the weight stream of the int4 policy;
//  * per chunk and lane: 32 converts, two shifts (e << 23, after one shift of
//    the dword by the chunk's parity in its pair) and an and;
//  * loads run in batches of U = 1 chunk on two register sets in the
//    branch-free steady loop, as int4's: 90-128 VGPRs, 3-5 waves per SIMD.
//    Two chunks per batch (145-218 VGPRs, 2-3 waves; one scale load per pair)
//    measured 5-9 % faster at M = 16 on the 1.3B shapes but 10-19 % slower on
//    the 6.7B FFN2 and LM head; one chunk is never more than 9 % behind int4
//    and up to 17 % ahead (profiles/decode_mx4/README.md).
// fp16 models: the conversion is exact while code * scale is a normal fp16,
// 2^-13 <= scale <= 2^13; bf16 holds every scale of the format.
// FLEETX_GEMV_MX4_KS (4 / 8 waves) and FLEETX_GEMV_MX4_ROWS (8 / 16 columns per
// block) pin the launch shape for tools/bench_gemv.py --mx4 sweeps.
//
// Built without packed fp32 VALU, as all new HIP code here (FX_NO_PK32,
// fx_common.h).  The kernel is the shared header's, so the attribute is applied
// to every function of this file's device pass instead of to the kernel, with
// flatten, so that the runtime's header functions still inline.
#include <hip/hip_runtime.h>
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#pragma clang attribute push(__attribute__((flatten)), apply_to = function)
#endif
#include "decode_gemv.h"
#include "fx_api.h"

namespace {

struct WMX4 {
  typedef uint8_t elt;
  typedef uintx4 reg;
  struct Ptrs {
    const uint8_t* w;
    const uint8_t* scale;  // [N, K / 32] e8m0, block order above
    bool valid() const { return (uintptr_t)w % 16 == 0 && scale != nullptr &&
                                (uintptr_t)scale % 16 == 0; }
  };
  static constexpr int CHUNK = 256, PACK = 2;
  static constexpr bool SCALED = false, GROUPED = false, OPSCALED = true;
  static constexpr int U = 1, U_MIN = 1;
  static constexpr bool STEADY_LOOP = true;
  static constexpr const char* PIN_KS = "FLEETX_GEMV_MX4_KS";
  static constexpr const char* PIN_U = nullptr;
  static constexpr const char* PIN_ROWS = "FLEETX_GEMV_MX4_ROWS";
  // ev[u]: the lane's scale dword of chunk u's pair; par: parity in its pair
  // of the batch's first chunk (an even U starts on an even chunk)
  template <typename T, int U>
  static __device__ __forceinline__ void mma_batch(floatx4& acc, const uintx4 (&wv)[U][2],
                                                   const short8 (&xv)[U][8],
                                                   const uint32_t (&ev)[U], int par) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t e = U % 2 == 0 ? ev[u] >> (16 * (u & 1)) : ev[u] >> (16 * ((par + u) & 1));
      const float s0 = mx4_scale(e), s1 = mx4_scale(e >> 8);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][0].x, s0), xv[u][0], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][0].y, s0), xv[u][1], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][0].z, s0), xv[u][2], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][0].w, s0), xv[u][3], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][1].x, s1), xv[u][4], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][1].y, s1), xv[u][5], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][1].z, s1), xv[u][6], acc);
      acc = mma16<T>(mx4_cvt8<T>(wv[u][1].w, s1), xv[u][7], acc);
    }
  }
};

}  // namespace

extern "C" int fx_decode_gemv_mx4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                  const uint8_t* wq, long ldw, const uint8_t* wscale,
                                  const void* bias, const void* res, long ldres, void* y, long ldy,
                                  void* kc, void* vc, const long* pos, const int* rows, int heads,
                                  int head_dim, int maxlen, const void* ln_w, const void* ln_b,
                                  float ln_eps, hipStream_t s) {
  return gemv_entry<WMX4>(dt, epi, M, N, K, x, ldx, WMX4::Ptrs{wq, wscale}, ldw, bias, res, ldres,
                          y, ldy, kc, vc, pos, rows, heads, head_dim, maxlen, ln_w, ln_b, ln_eps, s);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#pragma clang attribute pop
#endif
