// W8A8 prefill: int8 activations, quantised per row, times the int8 weights the
// decode steps stream, on v_mfma_i32_16x16x64_i8.
//
//   quant_rows_i8_kernel:  x[M, K] (bf16 / fp16, row stride) -> xq int8 [M, K]
//                          contiguous and sx fp32 [M]
//   prefill_gemm_i8_kernel + prefill_i8_finish_kernel:
//     y[M, N] = epi( float(sum_k xq[m, k] wq[n, k]) * (sx[m] * sw[n]) + bias[n] )
//
// M >= 65, K % 1024 == 0, K <= 65536 (K * 127 * 127 < 2^31: the int32 sum
// cannot overflow), any N; wq [N, K] / sw [N] are what quantize_weight_int8
// makes and decode_linear_w8 / prefill_gemm_w8 read, nothing is repacked; y is
// 16-bit; the epilogues are GV_BIAS / GV_GELU / GV_RES of weight_operand.h.
//
// Row quantiser.  amax = max_k |float(x[m, k])|, sx = amax > 0 ? amax / 127 : 1
// (an IEEE division), xq = clamp(rintf(float(x) / sx), -127, 127), ties to
// even: ops.quantize_weight_int8's formula per activation row, so the torch
// formula gives the same bytes.  One block per row; a thread keeps its V
// 16-byte vectors of the row in registers between the absmax reduction and the
// rounding, so x is read once (add_ln_fwd_kernel's scheme); 16-byte loads,
// 8-byte stores.  Inputs are trusted finite.
//
// GEMM, prefill_gemm_kernel's geometry with the conversion gone:
//  * a 4-wave workgroup owns 16 MT rows and 64 NT columns, MT in {4, 8}, NT in
//    {1, 2, 4}; wave w owns the columns [n0 + 16 NT w, n0 + 16 NT (w + 1)) and
//    all the block's rows;
//  * weights are stationary in registers.  Lane (r, g) = (lane % 16, lane / 16)
//    loads the 16 contiguous bytes k in [16 g, 16 g + 16) of weight row r of a
//    64-k step: that load IS the MFMA A operand, zero VALU ops per weight.  A
//    chunk is 128 k (two steps); two register sets, chunk c + 1 in flight under
//    chunk c's MFMAs;
//  * the activations go through LDS by global_load_lds, 16 bytes per lane: a
//    row of the stage is the chunk's 128 bytes, a wave instruction 8 rows, two
//    stages of 16 MT * 128 bytes, one workgroup barrier per chunk.  The LDS
//    side is lane-linear, so the bank swizzle sits on the global source
//    address: slot s of row m holds the row's 16-byte piece s ^ f(m), f(m) =
//    (m >> 1) & 7.  The B fragment of step i is ONE ds_read_b128 per lane,
//    piece 4 i + g of row 16 mt + r: 4 cycles per wave instruction, the ideal
//    (tools/lds_bank_sim.py --prefill-gemm-i8);
//  * the operand k order of the MFMA does not matter as long as A and B agree:
//    both hold bytes [16 g, 16 g + 16) of their row in the same register order,
//    and an integer sum has no order.  D[n][m]: the lane holds n = 4 g + j,
//    m = r (tests/test_prefill_w8a8_gpu.py probes both operands);
//  * x rows >= M repeat row M - 1, columns >= N clamp the weight row; neither
//    is stored;
//  * K split KS in {1, 2, 4} across blocks: split s sums the chunks [s, s + 1)
//    K / (128 KS) and stores its int32 partial to slab s of [KS, M, ldp] (ldp =
//    N rounded up to 8); prefill_i8_finish_kernel sums the slabs in int32 and
//    applies the epilogue.  No float enters a partial, no atomics.  KS = 1
//    applies the epilogue in the GEMM kernel;
//  * epilogue from the accumulators through LDS (each wave its own 16 MT x 16
//    ints per column tile, in the x stages' memory): a thread has 8 consecutive
//    columns of one row, one rounding, one 16-byte store.  N % 8 != 0 or
//    unaligned operands take the scalar form.  Plain vector stores;
//  * grid: ceil(N / (64 NT)) * KS * ceil(M / (16 MT)) blocks in one dimension,
//    remapped per XCD so that the row blocks of one weight panel run on one XCD.
//
// Summation -- the contract.  The sum over k is an int32 sum and exact, and
// the float part of the epilogue is one function (pi8_epilogue, compiled
// without contraction) of (the sum, sx[m], sw[n], bias[n], res[m, n]).  So the
// bits of an output row do not depend on MT, NT, KS, M or the row's index.
//
// Built without packed fp32 VALU, as all new HIP code here.  Resources and
// measurements: profiles/prefill_w8a8/README.md.
#include "fx_api.h"
#include "weight_operand.h"

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int PI8_CHUNK = 128;  // k per chunk and bytes per stage row: two 64-k MFMA steps

// ---------------------------------------------------------------------------
// row quantiser
// ---------------------------------------------------------------------------
// NTH threads on one row, V 16-byte vectors (8 elements) per thread, vector c =
// threadIdx.x + NTH v; NTH * V * 8 >= K (host).
template <typename T, int NTH, int V>
__global__ __launch_bounds__(NTH) FX_NO_PK32 void quant_rows_i8_kernel(
    const uint16_t* __restrict__ x, long ldx, int8_t* __restrict__ xq, float* __restrict__ sx,
    int K) {
  __shared__ float part[NTH / 64];
  const int m = blockIdx.x, t = threadIdx.x, nvec = K / 8;
  const uint16_t* xr = x + (long)m * ldx;
  uint4 raw[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = t + NTH * v;
    raw[v] = c < nvec ? *reinterpret_cast<const uint4*>(xr + 8 * c) : uint4{0u, 0u, 0u, 0u};
  }
  float amax = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float f[8];
    unpack8<T>(raw[v], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  }
  amax = wave_max(amax);
  if ((t & 63) == 0) part[t >> 6] = amax;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NTH / 64; ++i) amax = fmaxf(amax, part[i]);
  const float s = amax > 0.f ? amax / 127.f : 1.f;
  if (t == 0) sx[m] = s;
  int8_t* qr = xq + (long)m * K;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = t + NTH * v;
    if (c >= nvec) continue;
    float f[8];
    unpack8<T>(raw[v], f);
    uint32_t b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      b[j] = (uint32_t)(int)fminf(fmaxf(rintf(f[j] / s), -127.f), 127.f) & 0xFFu;
    uintx2 o;
    o.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    o.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    *reinterpret_cast<uintx2*>(qr + 8 * c) = o;
  }
}

template <typename T, int NTH, int V>
void quant_rows_go(const void* x, long ldx, int8_t* xq, float* sx, int M, int K, hipStream_t s) {
  hipLaunchKernelGGL((quant_rows_i8_kernel<T, NTH, V>), dim3(M), dim3(NTH), 0, s,
                     (const uint16_t*)x, ldx, xq, sx, K);
}
template <typename T>
void quant_rows_launch(const void* x, long ldx, int8_t* xq, float* sx, int M, int K,
                       hipStream_t s) {
  const int nvec = K / 8;  // a multiple of 128
  if (nvec <= 128) return quant_rows_go<T, 128, 1>(x, ldx, xq, sx, M, K, s);
  if (nvec <= 256) return quant_rows_go<T, 256, 1>(x, ldx, xq, sx, M, K, s);
  if (nvec <= 512) return quant_rows_go<T, 256, 2>(x, ldx, xq, sx, M, K, s);
  if (nvec <= 1024) return quant_rows_go<T, 256, 4>(x, ldx, xq, sx, M, K, s);
  if (nvec <= 2048) return quant_rows_go<T, 256, 8>(x, ldx, xq, sx, M, K, s);
  if (nvec <= 4096) return quant_rows_go<T, 256, 16>(x, ldx, xq, sx, M, K, s);
  return quant_rows_go<T, 256, 32>(x, ldx, xq, sx, M, K, s);
}

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
struct PI8Args {
  const int8_t* xq;
  const float* sx;
  const int8_t* w;
  const float* sw;
  const uint16_t* bias;
  const uint16_t* res;
  uint16_t* y;
  int* slab;  // KS > 1: [KS, M, ldp] int32 partials
  long ldx, ldw, ldy, ldres, ldp;
  int M, N, K, epi;
  int nbm;  // row blocks
  int ks;   // K splits
  int vec;  // every epilogue operand admits 16-byte accesses at n % 8 == 0
};

// bank swizzle of the x stage: 16-byte slot s of row m holds piece s ^ pi8_swz(m)
__device__ __forceinline__ int pi8_swz(int m) { return (m >> 1) & 7; }

// Epilogue of 8 consecutive columns n .. n + 7 (those < N) of row m from their
// exact integer sums: the one place a float is made.  No contraction, so the
// GEMM kernel and the finish kernel give the same bits.
template <typename T>
__device__ __forceinline__ void pi8_epilogue(const PI8Args& a, int m, int n, const int (&s)[8]) {
#pragma clang fp contract(off)
  const int cnt = min(8, a.N - n);
  const bool full = a.vec && cnt == 8;
  const int epi = a.epi;
  float b[8], rs[8], v[8];
  EPI8_LOAD(b, rs);
  const float sxm = a.sx[m];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sc = sxm * a.sw[min(n + j, a.N - 1)];
    v[j] = (float)s[j] * sc;
    if (a.bias != nullptr) v[j] = v[j] + b[j];
    if (epi == GV_GELU) v[j] = gelu_tanh(v[j]);
    if (epi == GV_RES) v[j] = v[j] + rs[j];
  }
  EPI8_STORE(v);
}

// SPLIT: the block stores its int32 partial to its slab (T is not used)
template <typename T, int MT, int NT, bool SPLIT>
__global__ __launch_bounds__(256) FX_NO_PK32 void prefill_gemm_i8_kernel(PI8Args a) {
  constexpr int BM = 16 * MT;
  constexpr int STAGE = BM * PI8_CHUNK;  // bytes of one x stage: BM rows of 128 bytes
  constexpr int NI = BM / 32;            // global_load_lds instructions per wave and chunk
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  // consecutive ids = the row blocks of one (weight panel, K split)
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (lid % a.nbm) * BM;
  const int rest = lid / a.nbm;
  const int split = rest % a.ks;
  const int n0 = (rest / a.ks) * (64 * NT) + 16 * NT * w;
  const int nck = a.K / PI8_CHUNK / a.ks;  // chunks of this split: even (host check)
  const long k0 = (long)split * nck * PI8_CHUNK;
  const int8_t* wp[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    wp[nt] = a.w + (long)min(n0 + 16 * nt + r, a.N - 1) * a.ldw + k0 + 16 * g;
  // x stage: 1 KiB piece p (8 rows) is one wave instruction; wave w loads
  // pieces w NI .. w NI + NI - 1; lane l writes slot l % 8 of row 8 p + l / 8
  const int8_t* xs[NI];
#pragma unroll
  for (int u = 0; u < NI; ++u) {
    const int row = 8 * (w * NI + u) + (lane >> 3);
    xs[u] = a.xq + (long)min(m0 + row, a.M - 1) * a.ldx + k0 + 16 * ((lane & 7) ^ pi8_swz(row));
  }
  // B fragment of row tile mt, step i: piece 4 i + g of row 16 mt + r
  const int xr0 = 128 * r + 16 * (g ^ pi8_swz(r)), xr1 = xr0 ^ 64;
  // D[n][m] of tile (nt, mt): the lane holds n = 4 g + j, m = r
  intx4 acc[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = intx4{0, 0, 0, 0};
  intx4 wv[2][NT][2];

// chunk c of the split: weights into register set S, x into LDS stage S
#define PI8_LOAD(S, c)                                                           \
  do {                                                                           \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                          \
      const intx4* p = reinterpret_cast<const intx4*>(wp[nt] + (long)(c) * PI8_CHUNK); \
      wv[S][nt][0] = p[0];                                                       \
      wv[S][nt][1] = p[4];                                                       \
    }                                                                            \
    _Pragma("unroll") for (int u = 0; u < NI; ++u)                               \
        __builtin_amdgcn_global_load_lds(                                        \
            (const void*)(xs[u] + (long)(c) * PI8_CHUNK),                        \
            (__attribute__((address_space(3))) void*)(lds + (S) * STAGE + (w * NI + u) * 1024), \
            16, 0, 0);                                                           \
  } while (0)
// chunk c on set / stage S.  The wait and the barrier: chunk c's weights and
// this wave's part of its x tile have landed, every wave's part is visible, and
// every wave is done with chunk c - 1, whose stage chunk c + 1 is then loaded
// into, under chunk c's MFMAs.
#define PI8_STEP(S, c, NEXT)                                                     \
  do {                                                                           \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             \
    __syncthreads();                                                             \
    if (NEXT) PI8_LOAD(1 - (S), (c) + 1);                                        \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                          \
      const char* xt = lds + (S) * STAGE + mt * 2048;                            \
      const intx4 b0 = *reinterpret_cast<const intx4*>(xt + xr0);                \
      const intx4 b1 = *reinterpret_cast<const intx4*>(xt + xr1);                \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                        \
        acc[nt][mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[S][nt][0], b0, acc[nt][mt], 0, 0, 0); \
        acc[nt][mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv[S][nt][1], b1, acc[nt][mt], 0, 0, 0); \
      }                                                                          \
    }                                                                            \
  } while (0)

  PI8_LOAD(0, 0);
  for (int c = 0; c < nck; c += 2) {
    const bool more = c + 2 < nck;
    PI8_STEP(0, c, true);
    PI8_STEP(1, c + 1, more);
  }

#undef PI8_STEP
#undef PI8_LOAD

  // NT rounds of 16 columns: the wave's own red[m][n] (16 MT x 16 ints, a
  // quarter of the x stages), then 8 consecutive n of one row per thread and
  // pass.  The barriers order one round's reads before the next one's writes.
  int* red = reinterpret_cast<int*>(lds) + w * (BM * 16);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      *reinterpret_cast<intx4*>(&red[(16 * mt + r) * 16 + 4 * g]) = acc[nt][mt];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MT / 2; ++it) {
      const int idx = 64 * it + lane;
      const int oct = idx & 1, ml = idx >> 1;
      const int m = m0 + ml, n = n0 + 16 * nt + 8 * oct;
      if (m < a.M && n < a.N) {
        const intx4* p = reinterpret_cast<const intx4*>(&red[ml * 16 + 8 * oct]);
        const intx4 p0 = p[0], p1 = p[1];
        if constexpr (SPLIT) {
          // n % 8 == 0 and ldp % 8 == 0: aligned, and n + 7 < ldp
          intx4* d = reinterpret_cast<intx4*>(a.slab + ((long)split * a.M + m) * a.ldp + n);
          d[0] = p0;
          d[1] = p1;
        } else {
          int v[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = p0[j];
            v[4 + j] = p1[j];
          }
          pi8_epilogue<T>(a, m, n, v);
        }
      }
    }
  }
}

// one thread per (row, 8 columns): the int32 sum of the KS slabs, the epilogue
template <typename T>
__global__ __launch_bounds__(256) FX_NO_PK32 void prefill_i8_finish_kernel(PI8Args a) {
  const int noct = (int)(a.ldp / 8);
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.M * noct) return;
  const int m = (int)(idx / noct), n = 8 * (int)(idx % noct);
  intx4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
  for (int s = 0; s < a.ks; ++s) {
    const intx4* p = reinterpret_cast<const intx4*>(a.slab + ((long)s * a.M + m) * a.ldp + n);
    s0 += p[0];
    s1 += p[1];
  }
  int v[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = s0[j];
    v[4 + j] = s1[j];
  }
  pi8_epilogue<T>(a, m, n, v);
}

template <typename T, int MT, int NT>
void pi8_go(const PI8Args& a, hipStream_t s) {
  const dim3 grid(((a.N + 64 * NT - 1) / (64 * NT)) * a.ks * a.nbm);
  if (a.ks == 1) {
    hipLaunchKernelGGL((prefill_gemm_i8_kernel<T, MT, NT, false>), grid, dim3(256), 0, s, a);
  } else {
    // the partial kernel does not depend on the output type
    hipLaunchKernelGGL((prefill_gemm_i8_kernel<bf16, MT, NT, true>), grid, dim3(256), 0, s, a);
    const long nthr = (long)a.M * (a.ldp / 8);
    hipLaunchKernelGGL((prefill_i8_finish_kernel<T>), dim3((unsigned)((nthr + 255) / 256)),
                       dim3(256), 0, s, a);
  }
}
template <typename T, int MT>
void pi8_launch_nt(const PI8Args& a, int nt, hipStream_t s) {
  if (nt == 1) return pi8_go<T, MT, 1>(a, s);
  if (nt == 2) return pi8_go<T, MT, 2>(a, s);
  pi8_go<T, MT, 4>(a, s);
}
template <typename T>
void pi8_launch(const PI8Args& a, int mt, int nt, hipStream_t s) {
  if (mt == 4) return pi8_launch_nt<T, 4>(a, nt, s);
  pi8_launch_nt<T, 8>(a, nt, s);
}

// Launch shape from (M, N, K), from the sweep in profiles/prefill_w8a8/README.md
// (the four layer shapes of 1.3B and 6.7B and the LM head at 65 / 128 / 512 /
// 2048 rows, every tile and split, weights streamed from HBM; medians of three
// child processes, old-versus-old spread 0.9 % in the median, 10.4 % at most).
// b = ceil(N / 64) * ceil(M / 64), the blocks of the smallest tile:
//  * 64 rows per block while the grid is small; 128 rows from b >= 1024 (4-6 %
//    at b = 1024; at b = 768 and K = 2048 the small tile is 10 % ahead), and
//    from b >= 256 where K >= 4096 (a longer K loop pays for the taller tile);
//  * 128 columns only for K >= 4096 and 2048 <= b < 6144: 5 % and 14 % in two
//    of the three cases there, level in the third; at K = 2048 and on the
//    largest grids 64 columns are 8-18 % ahead in four cases and level in two.
//    The LM head shape at 65 / 128 rows would gain 4-8 % from 128 columns and
//    does not get them: the prefill does not run the head on this kernel;
//  * the K split raises the grid to 512 blocks, and to 1024 where K >= 4096:
//    at b <= 128 a split in 4 is 1.35-2.6x faster than none.
// Against the best shape of each of the 36 cases the rule is level (within 6 %)
// in 34 and 8 % and 9 % behind in two (LM head at 128 rows, 6.7B FFN2 at 512).
void prefill_i8_rule(int M, int N, int K, int& mt, int& nt, int& ks) {
  const long b = (long)((N + 63) / 64) * ((M + 63) / 64);
  const bool longk = K >= 4096;
  mt = (b >= 1024 || (longk && b >= 256)) ? 8 : 4;
  nt = (longk && b >= 2048 && b < 6144) ? 2 : 1;
  ks = 1;
  while (ks < 4 && b * ks < (longk ? 1024 : 512)) ks *= 2;
}

}  // namespace

// Rows of x [M, K] (dt 0: bf16, 1: fp16; row stride ldx elements) to int8 with
// one fp32 scale per row.  Returns the blocks launched, 0 for a call not
// covered: K % 1024 != 0, K > 65536, rows that do not admit 16-byte loads.
extern "C" int fx_quant_rows_i8(int dt, int M, int K, const void* x, long ldx, int8_t* xq,
                                float* sx, hipStream_t s) {
  if (M < 1 || K < 1024 || K % 1024 != 0 || K > 65536 || ldx % 8 || ldx < K || !al16(x) ||
      !al16(xq) || xq == nullptr || sx == nullptr)
    return 0;
  if (dt == 0) quant_rows_launch<bf16>(x, ldx, xq, sx, M, K, s);
  else quant_rows_launch<f16>(x, ldx, xq, sx, M, K, s);
  return M;
}

// the launch shape prefill_i8_rule gives: out[0..2] = mt, nt, ks
extern "C" void fx_prefill_i8_rule(int M, int N, int K, int* out) {
  prefill_i8_rule(M, N, K, out[0], out[1], out[2]);
}

// The W8A8 prefill GEMM.  mt = nt = ks = 0: prefill_i8_rule; else the pinned
// launch shape.  slab: KS * M * ldp int32 of workspace for ks > 1, ldp = N
// rounded up to 8 (slab_elems is checked; with the rule the caller provides for
// ks = 4).  Returns the GEMM blocks launched, 0 for a call not covered: M < 65,
// K % 1024 != 0, K > 65536, unaligned rows, an epilogue outside GV_BIAS /
// GV_GELU / GV_RES or without its operands, a shape the library does not have,
// a workspace too small.
extern "C" int fx_prefill_gemm_w8a8(int dt, int epi, int M, int N, int K, const int8_t* xq,
                                    long ldx, const float* sx, const int8_t* wq, long ldw,
                                    const float* wscale, const void* bias, const void* res,
                                    long ldres, void* y, long ldy, int* slab, long slab_elems,
                                    int mt, int nt, int ks, hipStream_t s) {
  if (M < 65 || N < 1 || K < 1024 || K % 1024 != 0 || K > 65536 || ldx % 16 || ldw % 16 ||
      ldx < K || ldw < K || !al16(xq) || !al16(wq) || xq == nullptr || wq == nullptr ||
      y == nullptr || sx == nullptr || wscale == nullptr)
    return 0;
  if (epi < GV_BIAS || epi > GV_RES) return 0;
  if (epi == GV_RES && res == nullptr) return 0;
  if (mt == 0 && nt == 0 && ks == 0) {
    prefill_i8_rule(M, N, K, mt, nt, ks);
  } else if ((mt != 4 && mt != 8) || (nt != 1 && nt != 2 && nt != 4) ||
             (ks != 1 && ks != 2 && ks != 4)) {
    return 0;
  }
  PI8Args a;
  a.xq = xq; a.sx = sx; a.w = wq; a.sw = wscale;
  a.bias = (const uint16_t*)bias; a.res = (const uint16_t*)res; a.y = (uint16_t*)y;
  a.slab = slab;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldres = ldres; a.ldp = (long)(N + 7) / 8 * 8;
  a.M = M; a.N = N; a.K = K; a.epi = epi;
  a.nbm = (M + 16 * mt - 1) / (16 * mt);
  a.ks = ks;
  if (ks > 1 && (slab == nullptr || !al16(slab) || slab_elems < (long)ks * M * a.ldp))
    return 0;
  a.vec = al16(y) && ldy % 8 == 0 && al16(bias) &&
          (epi != GV_RES || (al16(res) && ldres % 8 == 0));
  if (dt == 0) pi8_launch<bf16>(a, mt, nt, s);
  else pi8_launch<f16>(a, mt, nt, s);
  return ((N + 64 * nt - 1) / (64 * nt)) * ks * a.nbm;
}
