// Decode GEMV, shared by every weight format: y[M, N] = x[M, K] W[N, K]^T,
// M <= 16, with the decoder layer's element-wise work fused into the epilogue
// and an optional LayerNorm of x fused as a prologue.  This header holds the
// kernel, the launch ladder and the host entry once; a weight format is a
// small policy type W (decode_gemv.hip: 16-bit, decode_gemv_w8.hip: int8 with
// a scale per output row, decode_gemv_w4.hip: int4 with a scale per k-group
// and output row) that supplies
//   elt, reg      weight element type and the 16-byte per-lane register type
//   PACK          weights per elt (1; int4: 2 per byte)
//   Ptrs          the weight pointer block of the argument struct: w (const
//                 elt*), with SCALED or GROUPED scale (const float*), and valid(), the
//                 host check of the block
//   CHUNK         k elements per chunk: every lane loads 32 contiguous bytes
//                 (reg[2]) of one W row per chunk, so CHUNK / 4 k per lane and
//                 CHUNK / 32 x vectors (MFMA k-steps) per chunk
//   mma_batch<T, U>  the MFMAs of U loaded chunks: registers -> the A operand
//                 of each of a chunk's k-steps (as loaded, or converted)
//   SCALED        accumulator times Ptrs::scale[n] before the bias
//   GROUPED       one chunk is one scale group: Ptrs::scale is [K / CHUNK, N],
//                 the lane's four scales of a chunk are loaded with the chunk's
//                 weights and mma_batch takes them as a fourth argument (it
//                 sums the chunk from zero and adds sum * scale to acc)
//   U, U_MIN      chunks per load batch: U, or U_MIN when a wave's K range is
//                 no multiple of U chunks
//   STEADY_LOOP   which of the kernel's two K-loop schedules runs
//   PIN_KS / PIN_U / PIN_ROWS   environment variables that pin the launch
//                 shape for tools/bench_gemv.py sweeps (nullptr: no such pin)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "fx_common.h"

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

//   GV_BIAS      y = acc + b                               (out-proj, LM head)
//   GV_GELU      y = gelu_tanh(acc + b)                    (FFN1)
//   GV_RES       y = acc + b + res                         (FFN2 + residual)
//   GV_QKV       acc + b scattered to q[M, H, D] and the KV cache at this
//                token's position (k/v_cache[M, maxlen, H, D])   (QKV + cache append);
//                with a row map, row m goes to cache row rows[m] (several
//                consecutive tokens of one sample in one call)
enum { GV_BIAS = 0, GV_GELU = 1, GV_RES = 2, GV_QKV = 3 };

template <typename W>
struct GemvArgs {
  const uint16_t* x;
  typename W::Ptrs wp;
  const uint16_t* bias;
  const uint16_t* res;
  uint16_t* y;
  long ldx, ldw, ldy, ldres;
  int M, N, K;
  // QKV scatter
  uint16_t* kc;
  uint16_t* vc;
  const long* pos;
  const int* rows;  // cache row of x row m; nullptr: row m
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

// int8 weight operands (W8; W4 after it has spread its nibbles into bytes)
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

template <typename W, int U>
__device__ __forceinline__ void load_w(typename W::reg (&wv)[U][2], const typename W::elt* wp,
                                       int c) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const typename W::reg* p =
        reinterpret_cast<const typename W::reg*>(wp + (c + u) * (W::CHUNK / W::PACK));
    wv[u][0] = __builtin_nontemporal_load(p);
    wv[u][1] = __builtin_nontemporal_load(p + 1);
  }
}
// x operand: global (L2-resident activations) or, with the fused LayerNorm,
// the normalised rows staged in LDS (address space 3 -> ds_read_b128)
template <typename W, int U, bool XL>
__device__ __forceinline__ void load_x(short8 (&xv)[U][W::CHUNK / 32], const uint16_t* xp, int c) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (XL) {
      const __attribute__((address_space(3))) short8* p =
          (const __attribute__((address_space(3))) short8*)(xp + (c + u) * W::CHUNK);
#pragma unroll
      for (int i = 0; i < W::CHUNK / 32; ++i) xv[u][i] = p[i];
    } else {
      const short8* p = reinterpret_cast<const short8*>(xp + (c + u) * W::CHUNK);
#pragma unroll
      for (int i = 0; i < W::CHUNK / 32; ++i) xv[u][i] = p[i];
    }
  }
}
template <typename W, int U, bool XL>
__device__ __forceinline__ void load_batch(typename W::reg (&wv)[U][2],
                                           short8 (&xv)[U][W::CHUNK / 32],
                                           const typename W::elt* wp, const uint16_t* xp, int c) {
  load_w<W, U>(wv, wp, c);
  load_x<W, U, XL>(xv, xp, c);
}

// GROUPED: the four scales scale[chunk, n] of the lane's accumulator columns
// (nj: their clamped column numbers).  Four dword loads: a row of scales is N
// floats, so no alignment beyond 4 bytes holds.
template <typename W, int U>
__device__ __forceinline__ void load_s(floatx4 (&sv)[U], const float* sp, int N,
                                       const int (&nj)[4], int c) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float* p = sp + (long)(c + u) * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) sv[u][j] = p[nj[j]];
  }
}

// The kernel's load and MFMA steps; with W::GROUPED they carry the chunk scales
// (sa / sb beside wa / wb).  Macros, not functions: a further level of inlining
// around these calls moves the code generation of every instantiation.
#define GV_LOAD_W(w, s, c)                                        \
  do {                                                            \
    load_w<W, U>(w, wp, c);                                       \
    if constexpr (W::GROUPED) load_s<W, U>(s, sp, a.N, nj, c);    \
  } while (0)
#define GV_LOAD_BATCH(XL, w, x, s, c)                             \
  do {                                                            \
    load_batch<W, U, XL>(w, x, wp, xp, c);                        \
    if constexpr (W::GROUPED) load_s<W, U>(s, sp, a.N, nj, c);    \
  } while (0)
#define GV_MMA(w, x, s)                                           \
  do {                                                            \
    if constexpr (W::GROUPED) W::template mma_batch<T, U>(acc, w, x, s); \
    else W::template mma_batch<T, U>(acc, w, x);                  \
  } while (0)

// Fused LayerNorm prologue: rows m < M of x [M, K] normalised (fp32 math,
// shifted one-pass moments: the row's first element is subtracted before the
// sums, so E[d^2] - E[d]^2 does not cancel) and stored as 16-bit rows in LDS.
// Every block recomputes the statistics of the same few rows (K * M * 2 bytes
// from L2) -- cheaper than a separate LayerNorm launch at decode sizes.
template <typename W, typename T, int NT, int MR>
__device__ __forceinline__ void ln_prologue(const GemvArgs<W>& a, uint16_t* xs, float* scratch) {
  // MR >= M rows (1 / 4, chosen on the host); the loops over rows are
  // unrolled so the loads of every row are in flight together
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

// CDNA4 mapping (cdna_hip_programming.md §5, "GEMV / M <= 16 decode weights":
// operand streamed once per block -> straight to VGPRs, deep unroll):
//  * a block owns RW output columns (rows of W) and splits K over its GV_KS
//    waves; each wave runs v_mfma_f32_16x16x32 with A = 16 W rows, B = 16 x
//    rows (rows >= M repeat row M-1 and are never stored).  (A cross-block
//    K split with an agent-scope slab reduction measured 2-10x SLOWER here:
//    the release/acquire pair per block costs more than the latency it
//    hides -- tools/bench_gemv.py, profiles/r2_decode/);
//  * per chunk every lane loads 32 CONTIGUOUS bytes of one W row (lane group
//    g = lane/16 covers bytes 32g..32g+31), so one wave instruction pair reads
//    16 full 128-byte row segments; the MFMA k-steps use the matching
//    permutation of k for x (a sum is order-free in k);
//  * the wave partials are summed through LDS and the epilogue runs one
//    output element per thread, with one rounding at the store.
// U: chunks per load batch; GV_KS: waves (K slices) per block; RW: output
// columns per block; LNR: rows of the LayerNorm prologue (0 = none)
template <typename W, typename T, int EPI, int U, int GV_KS, int RW, int LNR>
__global__ __launch_bounds__(64 * GV_KS) void gemv_kernel(GemvArgs<W> a) {
  constexpr bool LN = LNR > 0;
  __shared__ float red[GV_KS * 256];
  extern __shared__ __attribute__((aligned(16))) uint16_t xs_dyn[];  // LN: normalised x [M][K]
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  // RW = 8: the MFMA still takes 16 W rows, rows r and r + 8 are the same row
  // (the coalescer merges the duplicate lanes), so a narrow layer (N = 2048)
  // spreads over 256 blocks instead of 128 and every CU streams
  const int n0 = blockIdx.x * RW;
  const int r = lane & 15, g = lane >> 4;
  const int kw = a.K / GV_KS;  // multiple of CHUNK * U (host check)
  const int kb = w * kw;
  const int nrow = min(n0 + (r % RW), a.N - 1);
  const typename W::elt* wp =
      a.wp.w + (long)nrow * a.ldw + kb / W::PACK + W::CHUNK / 4 / W::PACK * g;
  // x rows >= M read row M-1 (no per-load select: their D rows are never stored)
  // LN rows in LDS are K + 8 elements apart: the 16 lanes' rows fall on different banks
  const uint16_t* xp = LN ? xs_dyn + (long)min(r, a.M - 1) * (a.K + 8) + kb + W::CHUNK / 4 * g
                          : a.x + (long)min(r, a.M - 1) * a.ldx + kb + W::CHUNK / 4 * g;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  const int nch = kw / W::CHUNK;
  // The wave's K range: nch chunks in batches of U on two register sets, so
  // that batch c+1's loads are in flight under batch c's MFMAs.  With the
  // LayerNorm prologue the first weight batches stream while the statistics
  // are taken.
  // Two schedules of the same sum, kept apart and in the kernel body (not in
  // functions) only so that sharing this header moved no code generation; see
  // profiles/decode_gemv_shared/README.md before merging or moving them.
  typename W::reg wa[U][2], wb[U][2];
  short8 xa[U][W::CHUNK / 32], xb[U][W::CHUNK / 32];
  // GROUPED: chunk scales of the two register sets, the scale rows of this
  // wave's K range and the lane's accumulator columns D[n = 4g + j]
  floatx4 sa[W::GROUPED ? U : 1], sb[W::GROUPED ? U : 1];
  const float* sp = nullptr;
  int nj[4];
  if constexpr (W::GROUPED) {
    sp = a.wp.scale + (long)(kb / W::CHUNK) * a.N;
#pragma unroll
    for (int j = 0; j < 4; ++j) nj[j] = min(n0 + (4 * g + j) % RW, a.N - 1);
  }
  if constexpr (W::STEADY_LOOP) {
    // Branch-free steady loop with peeled head and tail: no branch around the
    // loads, so the compiler counts vmcnt exactly and batch c+1 really stays in
    // flight under batch c's MFMAs (a conditional load ahead of a wait makes it
    // wait for the newest loads).
    int c = 0;
    bool done = false;
    if constexpr (LN) {
      GV_LOAD_W(wa, sa, 0);
      if (U < nch) GV_LOAD_W(wb, sb, U);
      ln_prologue<W, T, 64 * GV_KS, LNR>(a, xs_dyn, red);
      load_x<W, U, true>(xa, xp, 0);
      if (U < nch) {
        load_x<W, U, true>(xb, xp, U);
        GV_MMA(wa, xa, sa);
        if (2 * U < nch) GV_LOAD_BATCH(LN, wa, xa, sa, 2 * U);
        else done = true;
        GV_MMA(wb, xb, sb);
        c = 2 * U;
      }
    } else {
      GV_LOAD_BATCH(false, wa, xa, sa, 0);
    }
    if (!done) {
      // set a holds batch c
      for (; c + 2 * U < nch; c += 2 * U) {
        GV_LOAD_BATCH(LN, wb, xb, sb, c + U);
        GV_MMA(wa, xa, sa);
        GV_LOAD_BATCH(LN, wa, xa, sa, c + 2 * U);
        GV_MMA(wb, xb, sb);
      }
      if (c + U < nch) {
        GV_LOAD_BATCH(LN, wb, xb, sb, c + U);
        GV_MMA(wa, xa, sa);
        GV_MMA(wb, xb, sb);
      } else {
        GV_MMA(wa, xa, sa);
      }
    }
  } else {
    // Guarded loop with break: every load sits behind a bounds test.
    if constexpr (LN) {
      GV_LOAD_W(wa, sa, 0);
      if (U < nch) GV_LOAD_W(wb, sb, U);
      ln_prologue<W, T, 64 * GV_KS, LNR>(a, xs_dyn, red);
      load_x<W, U, true>(xa, xp, 0);
      if (U < nch) load_x<W, U, true>(xb, xp, U);
    } else {
      GV_LOAD_BATCH(false, wa, xa, sa, 0);
    }
    for (int c = 0; c < nch; c += 2 * U) {
      if (!LN || c > 0)
        if (c + U < nch) GV_LOAD_BATCH(LN, wb, xb, sb, c + U);
      GV_MMA(wa, xa, sa);
      if (c + U >= nch) break;
      if (c + 2 * U < nch) GV_LOAD_BATCH(LN, wa, xa, sa, c + 2 * U);
      GV_MMA(wb, xb, sb);
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
  if constexpr (W::SCALED) v *= a.wp.scale[n];
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
      const long cr = a.rows != nullptr ? a.rows[m] : m;
      cache[((cr * a.maxlen + a.pos[m]) * a.heads + h) * D + d] = o;
    }
  } else {
    a.y[(long)m * a.ldy + n] = o;
  }
}

// launch ladder: run-time (u, ks, rw, LayerNorm rows, epilogue) -> instantiation
template <typename W, typename T, int EPI, int RW, int LNR>
void launch_u(const GemvArgs<W>& a, int u, int ks, hipStream_t s) {
  const dim3 grid((a.N + RW - 1) / RW);
  const size_t lds = LNR > 0 ? (size_t)a.M * (a.K + 8) * 2 : 0;
  auto go = [&](void (*k)(GemvArgs<W>), int threads) {
    // the dynamic rows and the static red[] (up to 8 KiB) share the 64 KiB default
    if (lds > 65536 - sizeof(float) * 256 * 8)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(threads), lds, s, a);
  };
  if (ks == 8) {
    if (u == W::U) go(gemv_kernel<W, T, EPI, W::U, 8, RW, LNR>, 512);
    else go(gemv_kernel<W, T, EPI, W::U_MIN, 8, RW, LNR>, 512);
  } else {
    if (u == W::U) go(gemv_kernel<W, T, EPI, W::U, 4, RW, LNR>, 256);
    else go(gemv_kernel<W, T, EPI, W::U_MIN, 4, RW, LNR>, 256);
  }
}

template <typename W, typename T, int EPI, int LNR>
void launch_rw(const GemvArgs<W>& a, int u, int ks, int rw, hipStream_t s) {
  if (rw <= 8) launch_u<W, T, EPI, 8, LNR>(a, u, ks, s);
  else launch_u<W, T, EPI, 16, LNR>(a, u, ks, s);
}

// row-count bucket of the unrolled LayerNorm prologue (0 = none)
template <typename W, typename T, int EPI>
void launch_ln(const GemvArgs<W>& a, bool ln, int u, int ks, int rw, hipStream_t s) {
  if constexpr (EPI == GV_GELU || EPI == GV_QKV) {
    if (ln && a.M == 1) return launch_rw<W, T, EPI, 1>(a, u, ks, rw, s);
    if (ln) return launch_rw<W, T, EPI, 4>(a, u, ks, rw, s);  // M <= 4 (host check)
  }
  launch_rw<W, T, EPI, 0>(a, u, ks, rw, s);
}

template <typename W, typename T>
void launch_epi(const GemvArgs<W>& a, int epi, bool ln, int u, int ks, int rw, hipStream_t s) {
  switch (epi) {
    case GV_GELU: launch_ln<W, T, GV_GELU>(a, ln, u, ks, rw, s); break;
    case GV_RES: launch_ln<W, T, GV_RES>(a, ln, u, ks, rw, s); break;
    case GV_QKV: launch_ln<W, T, GV_QKV>(a, ln, u, ks, rw, s); break;
    default: launch_ln<W, T, GV_BIAS>(a, ln, u, ks, rw, s); break;
  }
}

inline int env_int(const char* name) {
  const char* e = name ? getenv(name) : nullptr;
  return e ? atoi(e) : 0;
}

// Host entry of every weight format: validates the call, chooses the launch
// shape and launches.  Returns the number of blocks launched (0 = call not
// covered: M > 16, K % 1024 != 0, unaligned rows, an epilogue without its
// operands, a LayerNorm prologue over more than 4 rows or 96 KiB).
// ln_w / ln_b (optional, GELU and QKV epilogues): y = LayerNorm(x) W^T ... with
// the LayerNorm fused as a prologue (normalised rows staged in LDS).
template <typename W>
int gemv_entry(int dt, int epi, int M, int N, int K, const void* x, long ldx,
               const typename W::Ptrs& wp, long ldw, const void* bias, const void* res,
               long ldres, void* y, long ldy, void* kc, void* vc, const long* pos, const int* rows,
               int heads, int head_dim, int maxlen, const void* ln_w, const void* ln_b, float ln_eps,
               hipStream_t s) {
  if (M < 1 || M > 16 || N < 1 || K < 1024 || K % 1024 != 0 || (ldx % 8) ||
      (ldw * sizeof(typename W::elt) % 16) || ((uintptr_t)x % 16) || !wp.valid())
    return 0;
  if (epi < GV_BIAS || epi > GV_QKV) return 0;
  if (epi == GV_RES && res == nullptr) return 0;
  if (epi == GV_QKV && (kc == nullptr || vc == nullptr || pos == nullptr || head_dim < 1 ||
                        N != 3 * heads * head_dim))
    return 0;
  const bool ln = ln_w != nullptr;
  // fused LayerNorm for up to 4 rows (small-batch decode, where the separate
  // launch dominates: 1.3B decode 1.27 / 1.38 / 1.43 -> 1.11 / 1.30 / 1.38 ms per
  // token at batch 1 / 2 / 4); more rows take the LayerNorm kernel (a 16-row
  // prologue measured 1.38 -> 2.13 ms at batch 8)
  if (ln && (ln_b == nullptr || (epi != GV_GELU && epi != GV_QKV) || M > 4 ||
             (long)M * (K + 8) * 2 > 96 * 1024))
    return 0;
  static const int pin_ks = env_int(W::PIN_KS);
  static const int pin_u = env_int(W::PIN_U);
  static const int pin_rw = env_int(W::PIN_ROWS);
  // measured (tools/bench_gemv.py, M = 1, HBM-streamed weights): 4 waves win
  // on every GPT-3 1.3B / 6.7B layer and the LM head (16-bit 1.3B FFN1 12.2 ->
  // 8.8 us, LM head 57 -> 40 us = 5.2 TB/s); only the narrow N <= 2048 layers
  // prefer 8 waves on shorter K ranges and 8 columns per block, so that every
  // CU streams (1.3B out-proj / FC2: 5.1 -> 4.7 / 14.2 -> 12.4 us)
  int ks = (N <= 2048 && K % 2048 == 0) ? 8 : 4;
  if ((pin_ks == 4 || pin_ks == 8) && K % (W::CHUNK * W::U_MIN * pin_ks) == 0) ks = pin_ks;
  // With the default ks a wave's K range is always a multiple of U chunks; only
  // the int8 FLEETX_GEMV_W8_KS=8 pin at K an odd multiple of 1024 leaves an odd
  // number of chunks and takes U_MIN (for W16, U_MIN == U); int4 has odd counts
  // at the default ks too (K = 1024: one chunk per wave)
  int u = (K / (W::CHUNK * ks)) % W::U == 0 ? W::U : W::U_MIN;
  if (pin_u == W::U_MIN) u = W::U_MIN;
  int rw = N <= 2048 ? 8 : 16;
  if (pin_rw == 8 || pin_rw == 16) rw = pin_rw;
  GemvArgs<W> a;
  a.x = (const uint16_t*)x; a.wp = wp; a.bias = (const uint16_t*)bias;
  a.res = (const uint16_t*)res; a.y = (uint16_t*)y;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldres = ldres;
  a.M = M; a.N = N; a.K = K;
  a.kc = (uint16_t*)kc; a.vc = (uint16_t*)vc; a.pos = pos; a.rows = rows;
  a.heads = heads; a.head_dim = head_dim; a.maxlen = maxlen;
  a.ln_w = (const uint16_t*)ln_w; a.ln_b = (const uint16_t*)ln_b; a.ln_eps = ln_eps;
  if (dt == 0) launch_epi<W, bf16>(a, epi, ln, u, ks, rw, s);
  else launch_epi<W, f16>(a, epi, ln, u, ks, rw, s);
  return (N + rw - 1) / rw;
}

#undef GV_LOAD_W
#undef GV_LOAD_BATCH
#undef GV_MMA

}  // namespace
