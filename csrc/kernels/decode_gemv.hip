// Skinny GEMM for decoding: y[M, N] = x[M, K] W[N, K]^T, M <= 16, with the
// decoder layer's element-wise work fused into the epilogue.
//
// Reference K19 / N-12: the inference program's
// fused_multi_transformer (`core/engine/inference_engine.py:103-109,127-129`).
// At decode batch sizes a decoder layer is four weight-streaming GEMVs; every
// weight byte is read once per token, so the layer is bound by HBM bandwidth
// and the goal is to stream W at the roofline while the small activations
// come from L2.  Epilogues (GV_BIAS / GELU / RES / QKV scatter) turn each GEMV
// into a whole sub-layer.
//
// The kernel, its launch ladder and the host entry are decode_gemv.h's; this
// file is the 16-bit weight operand:
//  * per 64-k chunk every lane loads 32 contiguous bytes (16 elements) of one
//    W row, which are the A operands of the chunk's two MFMA k-steps as loaded;
//  * loads run in batches of U = 4 chunks on two register sets, in the
//    guarded K loop.  (Batches of 8 chunks spilled and 4 columns per block lost
//    everywhere; both were removed, see profiles/r2_decode/README.md.)
// FLEETX_GEMV_KS (4 / 8 waves) and FLEETX_GEMV_ROWS (8 / 16 columns per block)
// pin the launch shape for tools/bench_gemv.py sweeps.
#include "decode_gemv.h"
#include "fx_api.h"

namespace {

struct W16 {
  typedef uint16_t elt;
  typedef short8 reg;
  struct Ptrs {
    const uint16_t* w;
    bool valid() const { return (uintptr_t)w % 16 == 0; }
  };
  static constexpr int CHUNK = 64, PACK = 1;
  static constexpr bool SCALED = false, GROUPED = false;
  static constexpr int U = 4, U_MIN = 4;
  static constexpr bool STEADY_LOOP = false;
  static constexpr const char* PIN_KS = "FLEETX_GEMV_KS";
  static constexpr const char* PIN_U = nullptr;
  static constexpr const char* PIN_ROWS = "FLEETX_GEMV_ROWS";
  template <typename T, int U>
  static __device__ __forceinline__ void mma_batch(floatx4& acc, const short8 (&wv)[U][2],
                                                   const short8 (&xv)[U][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc = mma16<T>(wv[u][0], xv[u][0], acc);
      acc = mma16<T>(wv[u][1], xv[u][1], acc);
    }
  }
};

}  // namespace

extern "C" int fx_decode_gemv(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                              const void* w, long ldw, const void* bias, const void* res,
                              long ldres, void* y, long ldy, void* kc, void* vc, const long* pos, const int* rows,
                              int heads, int head_dim, int maxlen, const void* ln_w,
                              const void* ln_b, float ln_eps, hipStream_t s) {
  return gemv_entry<W16>(dt, epi, M, N, K, x, ldx, W16::Ptrs{(const uint16_t*)w}, ldw, bias, res,
                         ldres, y, ldy, kc, vc, pos, rows, heads, head_dim, maxlen, ln_w, ln_b, ln_eps,
                         s);
}
