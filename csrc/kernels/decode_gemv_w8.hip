// Weight-only int8 decode GEMV (W8A16): y[M, N] = x[M, K] (q[N, K] * s[N])^T,
// M <= 16, 16-bit x and y, int8 weights with one fp32 scale per output row
// (fleetx_amd/ops/quant.py).  The operation, the epilogues (EPI_BIAS / GELU /
// RES / QKV scatter) and the optional LayerNorm prologue are those of
// decode_gemv.hip; only the weight operand differs: half the bytes per token.
//
// A decode step is bound by the weight stream, so the kernel keeps the
// structure of the 16-bit GEMV (cdna_hip_programming.md §5, "GEMV / M <= 16
// decode weights": straight to VGPRs, deep unroll, late waits) and converts
// in registers:
//  * a block owns 16 (or 8) output columns and splits K over its waves; each
//    wave runs v_mfma_f32_16x16x32 with A = 16 W rows, B = 16 x rows;
//  * per 128-k chunk every lane loads 32 CONTIGUOUS bytes of one q row (lane
//    group g = lane/16 covers bytes 32g..32g+31: the instruction pair reads 16
//    full 128-byte row segments) and the matching 32 x elements; the four
//    MFMA k-steps use that permutation of k on both operands (a sum is
//    order-free in k);
//  * each int8 is sign-extended and converted to fp32, then packed to the
//    activation dtype (bf16: the upper half of the fp32, exact for |q| <= 127;
//    fp16: cvt_pkrtz, exact too) right before its MFMA -- ~1.5 VALU lane-ops
//    per element;
//  * loads run in batches of U 128-k chunks on two register sets;
//  * the wave partials are summed through LDS; the epilogue multiplies by the
//    row scale, then bias / GeLU / residual / scatter, one rounding at the store.
//
// The argument struct, load_x, ln_prologue and the epilogue are copies of
// decode_gemv.hip's, adapted to the 128-k chunk; that file is left as it is,
// so its code generation cannot change.  Launch shapes measured in
// profiles/decode_w8/ (tools/bench_gemv.py --w8).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "fx_api.h"
#include "fx_common.h"

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

enum { GV_BIAS = 0, GV_GELU = 1, GV_RES = 2, GV_QKV = 3 };

struct GemvW8Args {
  const uint16_t* x;
  const int8_t* wq;
  const float* wscale;
  const uint16_t* bias;
  const uint16_t* res;
  uint16_t* y;
  long ldx, ldw, ldy, ldres;
  int M, N, K;
  // QKV scatter
  uint16_t* kc;
  uint16_t* vc;
  const long* pos;
  int heads, head_dim, maxlen;
  // optional LayerNorm of x fused as a prologue (LN1 -> QKV, LN2 -> FFN1)
  const uint16_t* ln_w;
  const uint16_t* ln_b;
  float ln_eps;
};

template <typename T>
__device__ __forceinline__ floatx4 mma16(const short8& a, const short8& b, const floatx4& c) {
  if constexpr (std::is_same<T, bf16>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// two int8 (bytes B0 and B1 of v) -> two packed 16-bit floats.  Every integer
// in [-128, 127] is exact in bf16 (8 significant bits) and fp16.
template <typename T, int B0, int B1>
__device__ __forceinline__ uint32_t cvt2(uint32_t v) {
  const float f0 = (float)(int8_t)(v >> (8 * B0));
  const float f1 = (float)(int8_t)(v >> (8 * B1));
  if constexpr (std::is_same<T, bf16>::value) {
    // an exact small integer: the low 16 fp32 bits are zero, truncation is exact
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, f1),
                                 __builtin_bit_cast(uint32_t, f0), 0x07060302u);
  } else {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f0, f1));
  }
}
// eight int8 (two dwords) -> one MFMA operand, element order = byte order
template <typename T>
__device__ __forceinline__ short8 cvt8(uint32_t lo, uint32_t hi) {
  uint4 o;
  o.x = cvt2<T, 0, 1>(lo);
  o.y = cvt2<T, 2, 3>(lo);
  o.z = cvt2<T, 0, 1>(hi);
  o.w = cvt2<T, 2, 3>(hi);
  return __builtin_bit_cast(short8, o);
}

template <int U>
__device__ __forceinline__ void load_w(uintx4 (&wv)[U][2], const int8_t* wp, int c) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uintx4* p = reinterpret_cast<const uintx4*>(wp + (c + u) * 128);
    wv[u][0] = __builtin_nontemporal_load(p);
    wv[u][1] = __builtin_nontemporal_load(p + 1);
  }
}
// x operand: global (L2-resident activations) or, with the fused LayerNorm,
// the normalised rows staged in LDS (address space 3 -> ds_read_b128)
template <int U, bool XL>
__device__ __forceinline__ void load_x(short8 (&xv)[U][4], const uint16_t* xp, int c) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (XL) {
      const __attribute__((address_space(3))) short8* p =
          (const __attribute__((address_space(3))) short8*)(xp + (c + u) * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[u][i] = p[i];
    } else {
      const short8* p = reinterpret_cast<const short8*>(xp + (c + u) * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[u][i] = p[i];
    }
  }
}
template <int U, bool XL>
__device__ __forceinline__ void load_batch(uintx4 (&wv)[U][2], short8 (&xv)[U][4],
                                           const int8_t* wp, const uint16_t* xp, int c) {
  load_w<U>(wv, wp, c);
  load_x<U, XL>(xv, xp, c);
}

// Fused LayerNorm prologue: rows m < M of x [M, K] normalised (fp32 math,
// shifted one-pass moments: the row's first element is subtracted before the
// sums, so E[d^2] - E[d]^2 does not cancel) and stored as 16-bit rows in LDS.
template <typename T, int NT, int MR>
__device__ __forceinline__ void ln_prologue(const GemvW8Args& a, uint16_t* xs, float* scratch) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  constexpr int NW = NT / 64;
  const int K = a.K, nch = K / 8, M = a.M;
  float sh[MR], s1[MR], s2[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    sh[m] = m < M ? Elt<T>::to_f(a.x[(long)m * a.ldx]) : 0.f;
    s1[m] = s2[m] = 0.f;
  }
  for (int c = t; c < nch; c += NT) {
    uint4 raw[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < M) raw[m] = *reinterpret_cast<const uint4*>(a.x + (long)m * a.ldx + c * 8);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m >= M) continue;
      float v[8];
      unpack8<T>(raw[m], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[j] - sh[m];
        s1[m] += d;
        s2[m] += d * d;
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m >= M) continue;
    const float r1 = wave_sum(s1[m]), r2 = wave_sum(s2[m]);
    if (lane == 0) {
      scratch[(2 * m) * NW + w] = r1;
      scratch[(2 * m + 1) * NW + w] = r2;
    }
  }
  __syncthreads();
  float mean[MR], rstd[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    float r1 = 0.f, r2 = 0.f;
    if (m < M) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        r1 += scratch[(2 * m) * NW + i];
        r2 += scratch[(2 * m + 1) * NW + i];
      }
    }
    const float md = r1 / K;
    mean[m] = sh[m] + md;
    rstd[m] = rsqrtf(fmaxf(r2 / K - md * md, 0.f) + a.ln_eps);
  }
  for (int c = t; c < nch; c += NT) {
    float gw[8], gb[8];
    load8<T>(a.ln_w + c * 8, gw);
    load8<T>(a.ln_b + c * 8, gb);
    uint4 raw[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < M) raw[m] = *reinterpret_cast<const uint4*>(a.x + (long)m * a.ldx + c * 8);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m >= M) continue;
      float v[8];
      unpack8<T>(raw[m], v);
      short8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (short)Elt<T>::from_f((v[j] - mean[m]) * rstd[m] * gw[j] + gb[j]);
      *(__attribute__((address_space(3))) short8*)(xs + (long)m * (K + 8) + c * 8) = o;
    }
  }
  __syncthreads();
}

template <typename T, int U>
__device__ __forceinline__ void mma_batch(floatx4& acc, const uintx4 (&wv)[U][2],
                                          const short8 (&xv)[U][4]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    acc = mma16<T>(cvt8<T>(wv[u][0].x, wv[u][0].y), xv[u][0], acc);
    acc = mma16<T>(cvt8<T>(wv[u][0].z, wv[u][0].w), xv[u][1], acc);
    acc = mma16<T>(cvt8<T>(wv[u][1].x, wv[u][1].y), xv[u][2], acc);
    acc = mma16<T>(cvt8<T>(wv[u][1].z, wv[u][1].w), xv[u][3], acc);
  }
}

// U: 128-k chunks per load batch; GV_KS: waves (K slices) per block; RW:
// output columns per block; LNR: rows of the LayerNorm prologue (0 = none)
template <typename T, int EPI, int U, int GV_KS, int RW, int LNR>
__global__ __launch_bounds__(64 * GV_KS) void gemv_w8_kernel(GemvW8Args a) {
  constexpr bool LN = LNR > 0;
  __shared__ float red[GV_KS * 256];
  extern __shared__ __attribute__((aligned(16))) uint16_t xs_dyn[];  // LN: normalised x [M][K]
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  // RW = 8: rows r and r + 8 of the MFMA are the same q row (the coalescer
  // merges the duplicate lanes), so a narrow layer spreads over twice the blocks
  const int n0 = blockIdx.x * RW;
  const int r = lane & 15, g = lane >> 4;
  const int kw = a.K / GV_KS;  // multiple of 128 * U (host check)
  const int kb = w * kw;
  const int nrow = min(n0 + (r % RW), a.N - 1);
  const int8_t* wp = a.wq + (long)nrow * a.ldw + kb + 32 * g;
  // x rows >= M read row M-1 (their D rows are never stored); LN rows in LDS
  // are K + 8 elements apart, so the 16 lanes' rows fall on different banks
  const uint16_t* xp = LN ? xs_dyn + (long)min(r, a.M - 1) * (a.K + 8) + kb + 32 * g
                          : a.x + (long)min(r, a.M - 1) * a.ldx + kb + 32 * g;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  const int nch = kw / 128;
  // two register sets: batch c+1's loads are in flight under batch c's MFMAs
  uintx4 wa[U][2], wb[U][2];
  short8 xa[U][4], xb[U][4];
  // The steady loop has no branch around its loads, so the compiler counts
  // vmcnt exactly and batch c+1 really stays in flight under batch c's MFMAs
  // (a conditional load ahead of a wait makes it wait for the newest loads).
  int c = 0;
  bool done = false;
  if constexpr (LN) {
    // the first weight batches stream while the LayerNorm statistics are taken
    load_w<U>(wa, wp, 0);
    if (U < nch) load_w<U>(wb, wp, U);
    ln_prologue<T, 64 * GV_KS, LNR>(a, xs_dyn, red);
    load_x<U, true>(xa, xp, 0);
    if (U < nch) {
      load_x<U, true>(xb, xp, U);
      mma_batch<T, U>(acc, wa, xa);
      if (2 * U < nch) load_batch<U, LN>(wa, xa, wp, xp, 2 * U);
      else done = true;
      mma_batch<T, U>(acc, wb, xb);
      c = 2 * U;
    }
  } else {
    load_batch<U, false>(wa, xa, wp, xp, 0);
  }
  if (!done) {
    // set a holds batch c
    for (; c + 2 * U < nch; c += 2 * U) {
      load_batch<U, LN>(wb, xb, wp, xp, c + U);
      mma_batch<T, U>(acc, wa, xa);
      load_batch<U, LN>(wa, xa, wp, xp, c + 2 * U);
      mma_batch<T, U>(acc, wb, xb);
    }
    if (c + U < nch) {
      load_batch<U, LN>(wb, xb, wp, xp, c + U);
      mma_batch<T, U>(acc, wa, xa);
      mma_batch<T, U>(acc, wb, xb);
    } else {
      mma_batch<T, U>(acc, wa, xa);
    }
  }
  if constexpr (LN) __syncthreads();  // red[] doubled as the LN scratch
  // D[n][m]: lane holds n = 4g + j, m = r
#pragma unroll
  for (int j = 0; j < 4; ++j) red[w * 256 + (4 * g + j) * 16 + r] = acc[j];
  __syncthreads();
  const int t = threadIdx.x;  // (nn, m) = (t / 16, t % 16)
  if (t >= 256) return;
  const int nn = t >> 4, m = t & 15;
  const int n = n0 + nn;
  if (nn >= RW || m >= a.M || n >= a.N) return;
  float v = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < GV_KS; ++s2) v += red[s2 * 256 + t];
  v *= a.wscale[n];
  if (a.bias != nullptr) v += Elt<T>::to_f(a.bias[n]);
  if constexpr (EPI == GV_GELU) v = gelu_tanh(v);
  if constexpr (EPI == GV_RES) v += Elt<T>::to_f(a.res[(long)m * a.ldres + n]);
  const uint16_t o = Elt<T>::from_f(v);
  if constexpr (EPI == GV_QKV) {
    // packed [heads][3][head_dim] columns
    const int D = a.head_dim;
    const int h = n / (3 * D), tq = (n / D) % 3, d = n % D;
    if (tq == 0) {
      a.y[(long)m * a.ldy + h * D + d] = o;
    } else {
      uint16_t* cache = tq == 1 ? a.kc : a.vc;
      cache[(((long)m * a.maxlen + a.pos[m]) * a.heads + h) * D + d] = o;
    }
  } else {
    a.y[(long)m * a.ldy + n] = o;
  }
}

template <typename T, int EPI, int RW, int LNR>
void launch_u(const GemvW8Args& a, int u, int ks, hipStream_t s) {
  const dim3 grid((a.N + RW - 1) / RW);
  const size_t lds = LNR > 0 ? (size_t)a.M * (a.K + 8) * 2 : 0;
  auto go = [&](void (*k)(GemvW8Args), int threads) {
    if (lds > 65536 - sizeof(float) * 256 * 8)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(threads), lds, s, a);
  };
  if (ks == 8) {
    if (u >= 2) go(gemv_w8_kernel<T, EPI, 2, 8, RW, LNR>, 512);
    else go(gemv_w8_kernel<T, EPI, 1, 8, RW, LNR>, 512);
  } else {
    if (u >= 2) go(gemv_w8_kernel<T, EPI, 2, 4, RW, LNR>, 256);
    else go(gemv_w8_kernel<T, EPI, 1, 4, RW, LNR>, 256);
  }
}

template <typename T, int EPI, int LNR>
void launch_rw(const GemvW8Args& a, int u, int ks, int rw, hipStream_t s) {
  if (rw <= 8) launch_u<T, EPI, 8, LNR>(a, u, ks, s);
  else launch_u<T, EPI, 16, LNR>(a, u, ks, s);
}

// LayerNorm-fused GEMV: row-count bucket of the unrolled prologue
template <typename T, int EPI>
void launch_ln(const GemvW8Args& a, int u, int ks, int rw, hipStream_t s) {
  if (a.M == 1) launch_rw<T, EPI, 1>(a, u, ks, rw, s);
  else launch_rw<T, EPI, 4>(a, u, ks, rw, s);  // M <= 4 (host check)
}

int env_int(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : 0;
}

}  // namespace

extern "C" {

// y = x (wq * wscale[:, None])^T with the epilogues and the optional LayerNorm
// prologue of fx_decode_gemv.  Returns the number of blocks launched (0 =
// shape not supported: M > 16, K % 1024 != 0, unaligned rows).
// FLEETX_GEMV_W8_KS (4 / 8 waves), FLEETX_GEMV_W8_U (1: one chunk per batch)
// and FLEETX_GEMV_W8_ROWS (8 / 16 columns per block) pin the launch shape for
// tools/bench_gemv.py sweeps.
int fx_decode_gemv_w8(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                      const int8_t* wq, long ldw, const float* wscale, const void* bias,
                      const void* res, long ldres, void* y, long ldy, void* kc, void* vc,
                      const long* pos, int heads, int head_dim, int maxlen, const void* ln_w,
                      const void* ln_b, float ln_eps, hipStream_t s) {
  if (M < 1 || M > 16 || N < 1 || K < 1024 || K % 1024 != 0 || (ldx % 8) || (ldw % 16) ||
      ((uintptr_t)wq % 16) || ((uintptr_t)x % 16) || wscale == nullptr)
    return 0;
  if (epi < GV_BIAS || epi > GV_QKV) return 0;
  if (epi == GV_RES && res == nullptr) return 0;
  if (epi == GV_QKV && (kc == nullptr || vc == nullptr || pos == nullptr || head_dim < 1 ||
                        N != 3 * heads * head_dim))
    return 0;
  const bool ln = ln_w != nullptr;
  // fused LayerNorm for up to 4 rows, as in fx_decode_gemv
  if (ln && (ln_b == nullptr || (epi != GV_GELU && epi != GV_QKV) || M > 4 ||
             (long)M * (K + 8) * 2 > 96 * 1024))
    return 0;
  static const int pin_ks = env_int("FLEETX_GEMV_W8_KS");
  static const int pin_u = env_int("FLEETX_GEMV_W8_U");
  static const int pin_rw = env_int("FLEETX_GEMV_W8_ROWS");
  // as in the 16-bit GEMV: the narrow layers take 8 waves on shorter K ranges
  // and 8 columns per block, so that every CU streams
  int ks = (N <= 2048 && K % 2048 == 0) ? 8 : 4;
  if ((pin_ks == 4 || pin_ks == 8) && K % (128 * pin_ks) == 0) ks = pin_ks;
  // a wave's K range is a multiple of 256 for every K % 1024 == 0 at 4 waves
  // (two 128-k chunks per batch); 8 waves at K = 1024 leave one chunk
  int u = (K / (128 * ks)) % 2 == 0 ? 2 : 1;
  if (pin_u == 1) u = 1;
  int rw = N <= 2048 ? 8 : 16;
  if (pin_rw == 8 || pin_rw == 16) rw = pin_rw;
  GemvW8Args a;
  a.x = (const uint16_t*)x; a.wq = wq; a.wscale = wscale; a.bias = (const uint16_t*)bias;
  a.res = (const uint16_t*)res; a.y = (uint16_t*)y;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldres = ldres;
  a.M = M; a.N = N; a.K = K;
  a.kc = (uint16_t*)kc; a.vc = (uint16_t*)vc; a.pos = pos;
  a.heads = heads; a.head_dim = head_dim; a.maxlen = maxlen;
  a.ln_w = (const uint16_t*)ln_w; a.ln_b = (const uint16_t*)ln_b; a.ln_eps = ln_eps;
#define FX_GV(T)                                                  \
  switch (epi) {                                                              \
    case GV_GELU:                                                             \
      if (ln) launch_ln<T, GV_GELU>(a, u, ks, rw, s);                         \
      else launch_rw<T, GV_GELU, 0>(a, u, ks, rw, s);                         \
      break;                                                                  \
    case GV_RES: launch_rw<T, GV_RES, 0>(a, u, ks, rw, s); break;             \
    case GV_QKV:                                                              \
      if (ln) launch_ln<T, GV_QKV>(a, u, ks, rw, s);                          \
      else launch_rw<T, GV_QKV, 0>(a, u, ks, rw, s);                          \
      break;                                                                  \
    default: launch_rw<T, GV_BIAS, 0>(a, u, ks, rw, s); break;                \
  }
  if (dt == 0) { FX_GV(bf16) } else { FX_GV(f16) }
#undef FX_GV
  return (N + rw - 1) / rw;
}

}  // extern "C"
