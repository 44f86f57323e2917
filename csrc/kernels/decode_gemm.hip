// Skinny GEMM for batched decoding: y[M, N] = x[M, K] W[N, K]^T, 17 <= M <= 64,
// K % 1024 == 0, any N, 16-bit x and y, with the decoder layer's element-wise
// work fused into the epilogue (GV_BIAS / GV_GELU / GV_RES / GV_QKV of
// weight_operand.h).  The twin of gemv_kernel for the rows it does not take: the
// step is still bound by the weight stream, so the weights are streamed once,
// straight to VGPRs, and every weight operand is reused from registers by all
// row tiles.  Weight operands: 16-bit, int8 with a scale per output row, int4
// (decode_gemv_w4.hip's packing) with a scale per (group of 256 k, output row),
// MXFP4 (decode_gemv_mx4.hip's packing) with an e8m0 scale per (row, 32 k).
//
// Register tiling:
//  * a block owns 16 * NT output columns (rows of W) and all 16 * MT x rows,
//    MT = ceil(M / 16) in 2..4, NT in {1, 2, 4}; its KS = 4 or 8 waves split K
//    (no cross-block K split: decode_gemv.h records it as 2-10x slower).
//    NT > 1 because a block re-reads M * K * 2 bytes of x from L2: at NT = 1,
//    M = 64 that is four times its 16-bit weight bytes; NT = 4 brings the
//    ratio back to that of gemv_kernel at M = 16;
//  * a chunk is 64 k.  Lane (r, g) = (lane % 16, lane / 16) loads the 16
//    contiguous k [16 g, 16 g + 16) of weight row r of each of its NT row tiles
//    (32 / 16 / 8 bytes for 16-bit / int8 / int4, nontemporal) and the same k
//    of x row r of each of its MT row tiles (x rows >= M repeat row M - 1 and
//    are never stored).  16 k per lane and chunk, not the 32 bytes of
//    gemv_kernel: the x operand of a chunk is 8 * MT VGPRs per 16 k, and with
//    32 int8 / 64 int4 weights per lane the two x register sets alone would
//    take 128 / 256 VGPRs at MT = 4;
//  * a quantised chunk becomes its two short8 A operands ONCE (cvt8 of
//    weight_operand.h; int4: the two-mask spread to 16 q first) and each feeds MT
//    MFMAs v_mfma_f32_16x16x32, so the conversion is paid per weight, not per
//    weight and row tile;
//  * two register sets: chunk c + 1 is in flight under chunk c's MFMAs, in a
//    branch-free loop over groups of PB chunks with the last group peeled (no
//    branch around a load, so vmcnt is counted exactly -- the W8 loop's reason).
//    int4: a group is one scale group (PB = 4 chunks = 256 k), summed from
//    C = 0 per (nt, mt) tile and entered as fma(sum, scale / 16, acc), with the
//    group's scales loaded ahead of its chunks;
//    MXFP4: the hardware conversion applies the scale to the operand, so the
//    MFMAs go straight into acc -- one fp32 tile per (nt, mt), which admits
//    the 4 x 4 tile int4 has no registers for.  A lane's 16 k of a chunk lie
//    in one scale group; a loop group is 256 k (PB = 4) and the 16 scale bytes
//    of its 512-k block are one load per weight row, taken a loop group ahead;
//  * x is not staged in LDS: every wave reads a different K range, nothing is
//    shared inside a block;
//  * the wave partials are summed through LDS in NT rounds of 16 columns (KS *
//    MT KiB, at most 32 KiB static), and in each round 32 * MT threads produce 8
//    consecutive n of one row each: int8 row scale, bias, GeLU / residual, one
//    rounding, one 16-byte store to y, q or a K / V cache row (D % 8 == 0: a run
//    of 8 never crosses q / k / v).  N % 8 and unaligned operands take the
//    scalar form of the same code.  No atomics.
//
// Summation order: a row's sum is the MFMA chain over its wave's chunks in
// order, then the waves in order.  KS is a function of (N, K, format) only and
// NT / MT do not enter, so the bits of an output row depend on that x row
// alone, not on its index, on M or on the other rows.
//
// Built without packed fp32 VALU, as all new HIP code here (FX_NO_PK32,
// fx_common.h).  Resources and measurements: profiles/decode_rows/README.md.
#include "fx_api.h"
#include "weight_operand.h"

namespace {

constexpr int DG_CHUNK = 64;  // k per chunk: 16 per lane, two MFMA k-steps

// Weight operand policies (weight_operand.h) with what this kernel owns: PB =
// chunks per loop group, FMT = the format's column of the launch table, load()
// = a lane's raw of one row and chunk, streamed.
struct G16 : Op16 {
  static constexpr int PB = 2, FMT = 0;
  static __device__ __forceinline__ raw load(const elt* p) {
    const short8* q = reinterpret_cast<const short8*>(p);
    raw o;
    o.v[0] = __builtin_nontemporal_load(q);
    o.v[1] = __builtin_nontemporal_load(q + 1);
    return o;
  }
};
struct G8 : Op8 {
  static constexpr int PB = 2, FMT = 1;
  static __device__ __forceinline__ raw load(const elt* p) { return load_w<raw, true>(p); }
};
struct G4 : Op4 {
  static constexpr int PB = 4, FMT = 2;
  static __device__ __forceinline__ raw load(const elt* p) { return load_w<raw, true>(p); }
};
// MXFP4 shares int4's column of the launch table until its own sweep is taken
struct GM4 : OpM4 {
  static constexpr int PB = 4, FMT = 2;
  static __device__ __forceinline__ raw load(const elt* p) { return load_w<raw, true>(p); }
};

template <typename W>
struct GemmArgs {
  const uint16_t* x;
  const typename W::elt* w;
  const typename W::sc* scale;  // G8: [N]; G4: [K / 256, N]; GM4: [N, K / 32] bytes
  const uint16_t* bias;
  const uint16_t* res;
  uint16_t* y;
  long ldx, ldw, ldy, ldres;  // ldw in elt (G4: bytes)
  int M, N, K, epi;
  // QKV scatter, as in GemvArgs
  uint16_t* kc;
  uint16_t* vc;
  const long* pos;
  const int* rows;
  int heads, head_dim, maxlen;
  int vec;  // every epilogue operand admits 16-byte accesses at n % 8 == 0
};

template <typename W, typename T, int KS, int NT, int MT>
__global__ __launch_bounds__(64 * KS) FX_NO_PK32 void decode_gemm_kernel(GemmArgs<W> a) {
  __shared__ __attribute__((aligned(16))) float red[KS * MT * 256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int kw = a.K / KS;  // multiple of PB chunks (host check)
  const int kb = w * kw;
  const typename W::elt* wp[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    wp[nt] = a.w + (long)min(n0 + 16 * nt + r, a.N - 1) * a.ldw + (kb + 16 * g) / W::PACK;
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xp[mt] = a.x + (long)min(16 * mt + r, a.M - 1) * a.ldx + kb + 16 * g;
  // D[n][m] of tile (nt, mt): the lane holds n = 4 g + j, m = r
  floatx4 acc[NT][MT], t[W::GROUPED ? NT : 1][W::GROUPED ? MT : 1];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
  typename W::raw wv[2][NT];
  short8 xv[2][MT][2];
  floatx4 sv[W::GROUPED ? NT : 1];
  const float* sp = nullptr;
  if constexpr (W::GROUPED) sp = a.scale + (long)(kb / 256) * a.N;
  // OPSCALED: per weight row the 16 scale bytes of a 512-k block (dword i:
  // chunk i of either 256-k half) of this loop group (ev) and the next (en),
  // and the lane's byte in a dword: 2 * (half of the block) + g / 2
  uintx4 ev[W::OPSCALED ? NT : 1], en[W::OPSCALED ? NT : 1];
  const uint8_t* ep[W::OPSCALED ? NT : 1];
  int q0 = 0;  // the wave's first loop group in units of 256 k
  if constexpr (W::OPSCALED) {
    q0 = kb / 256;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      ep[nt] = reinterpret_cast<const uint8_t*>(a.scale) +
               (long)min(n0 + 16 * nt + r, a.N - 1) * (a.K / 32);
      en[nt] = *reinterpret_cast<const uintx4*>(ep[nt] + (q0 >> 1) * 16);
    }
  }
  const int nb = kw / DG_CHUNK;

#define DG_LOAD(S, c)                                                        \
  do {                                                                       \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                        \
        wv[S][nt] = W::load(wp[nt] + (long)(c) * (DG_CHUNK / W::PACK));      \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                      \
      const short8* p = reinterpret_cast<const short8*>(xp[mt] + (long)(c) * DG_CHUNK); \
      xv[S][mt][0] = p[0];                                                   \
      xv[S][mt][1] = p[1];                                                   \
    }                                                                        \
  } while (0)
#define DG_MMA(S, I, dst)                                                    \
  do {                                                                       \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                      \
      short8 av[2];                                                          \
      if constexpr (W::OPSCALED)                                             \
        W::template ops<T>(wv[S][nt], mx4_scale(ev[nt][I] >> esh), av);      \
      else                                                                   \
        W::template ops<T>(wv[S][nt], av);                                   \
      _Pragma("unroll") for (int i = 0; i < 2; ++i)                          \
          _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                  \
              dst[nt][mt] = mma16<T>(av[i], xv[S][mt][i], dst[nt][mt]);      \
    }                                                                        \
  } while (0)
// chunk c (the I-th of its loop group) on set S; chunk c + 1 is loaded into the
// other set first
#define DG_STEP(S, I, c, NEXT)                                               \
  do {                                                                       \
    if (NEXT) DG_LOAD(1 - S, (c) + 1);                                       \
    if constexpr (W::GROUPED) DG_MMA(S, I, t);                               \
    else DG_MMA(S, I, acc);                                                  \
  } while (0)
// PB chunks from c (set 0 holds chunk c); MORE: chunk c + PB exists
#define DG_GROUP(c, MORE)                                                    \
  do {                                                                       \
    if constexpr (W::GROUPED) {                                              \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                    \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                        \
            sv[nt][j] = sp[min(n0 + 16 * nt + 4 * g + j, a.N - 1)];          \
        _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                    \
            t[nt][mt] = floatx4{0.f, 0.f, 0.f, 0.f};                         \
      }                                                                      \
      sp += a.N;                                                             \
    }                                                                        \
    int esh = 0;                                                             \
    if constexpr (W::OPSCALED) {                                             \
      const int q = q0 + (c) / W::PB;                                        \
      esh = 16 * (q & 1) + 8 * (g >> 1);                                     \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                    \
        ev[nt] = en[nt];                                                     \
        if (MORE)                                                            \
          en[nt] = *reinterpret_cast<const uintx4*>(ep[nt] + ((q + 1) >> 1) * 16); \
      }                                                                      \
    }                                                                        \
    DG_STEP(0, 0, c, true);                                                  \
    if constexpr (W::PB == 4) {                                              \
      DG_STEP(1, 1, (c) + 1, true);                                          \
      DG_STEP(0, 2, (c) + 2, true);                                          \
      DG_STEP(1, 3, (c) + 3, MORE);                                          \
    } else {                                                                 \
      DG_STEP(1, 1, (c) + 1, MORE);                                          \
    }                                                                        \
    if constexpr (W::GROUPED) {                                              \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                      \
          _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                  \
              _Pragma("unroll") for (int j = 0; j < 4; ++j)                  \
                  acc[nt][mt][j] =                                           \
                      __builtin_fmaf(t[nt][mt][j], sv[nt][j] * 0.0625f, acc[nt][mt][j]); \
    }                                                                        \
  } while (0)

  DG_LOAD(0, 0);
  int c = 0;
  for (; c + W::PB < nb; c += W::PB) DG_GROUP(c, true);
  DG_GROUP(c, false);

#undef DG_GROUP
#undef DG_STEP
#undef DG_MMA
#undef DG_LOAD

  // NT rounds of 16 columns: red[wave][mt][m][n], 32 * MT threads with 8 n each
  const int tt = threadIdx.x;
  const int oct = tt & 1, ml = (tt >> 1) & 15, tm = tt >> 5;
  const int m = 16 * tm + ml;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (nt > 0) __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      *reinterpret_cast<floatx4*>(&red[((w * MT + mt) * 16 + r) * 16 + 4 * g]) = acc[nt][mt];
    __syncthreads();
    const int n = n0 + 16 * nt + 8 * oct;
    if (tm < MT && m < a.M && n < a.N) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        const floatx4* p =
            reinterpret_cast<const floatx4*>(&red[((s2 * MT + tm) * 16 + ml) * 16 + 8 * oct]);
        const floatx4 p0 = p[0], p1 = p[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] += p0[j];
          v[4 + j] += p1[j];
        }
      }
      row_epilogue8<W, T, true>(a, m, n, v);
    }
  }
}

// int4 keeps two fp32 tiles live per (nt, mt), the group sum and the
// accumulator: 4 x 3 and 4 x 4 tiles do not fit the register file (they spill)
// and are not instantiated.  MXFP4 keeps one and has every tile.
template <typename W, int NT, int MT>
constexpr bool gemm_tile_ok = !(W::GROUPED && NT * MT > 8);

// launch ladder: run-time (dtype, ks, nt, mt) -> instantiation
template <typename W, typename T, int KS, int NT, int MT>
bool gemm_go(const GemmArgs<W>& a, hipStream_t s) {
  if constexpr (gemm_tile_ok<W, NT, MT>) {
    hipLaunchKernelGGL((decode_gemm_kernel<W, T, KS, NT, MT>),
                       dim3((a.N + 16 * NT - 1) / (16 * NT)), dim3(64 * KS), 0, s, a);
    return true;
  }
  return false;
}
template <typename W, typename T, int KS, int NT>
bool gemm_launch_mt(const GemmArgs<W>& a, int mt, hipStream_t s) {
  if (mt == 2) return gemm_go<W, T, KS, NT, 2>(a, s);
  if (mt == 3) return gemm_go<W, T, KS, NT, 3>(a, s);
  return gemm_go<W, T, KS, NT, 4>(a, s);
}
template <typename W, typename T, int KS>
bool gemm_launch_nt(const GemmArgs<W>& a, int nt, int mt, hipStream_t s) {
  if (nt == 1) return gemm_launch_mt<W, T, KS, 1>(a, mt, s);
  if (nt == 2) return gemm_launch_mt<W, T, KS, 2>(a, mt, s);
  return gemm_launch_mt<W, T, KS, 4>(a, mt, s);
}
template <typename W, typename T>
bool gemm_launch(const GemmArgs<W>& a, int ks, int nt, int mt, hipStream_t s) {
  if (ks == 8) return gemm_launch_nt<W, T, 8>(a, nt, mt, s);
  return gemm_launch_nt<W, T, 4>(a, nt, mt, s);
}

// Launch table, filled from the sweep in profiles/decode_rows/ (medians of three
// per figure): per measured (N, K) and format {16-bit, int8, int4; MXFP4 takes
// int4's column, its own sweep is not taken yet} the wave
// count ks -- one per (N, K, format), it fixes the order of a row's sum; the
// 16-bit column keeps gemv_kernel's rule, so that a row has the bits the GEMV
// gives it and a speculative window step repeats the plain loop's logits -- and
// the 16-column tiles per block nt for MT = 2, 3, 4.  nt = 0 (16-bit only): the
// vendor GEMM with its separate epilogue launches measured faster there; the
// call is not covered and the caller runs it unfused.  A quantised format is
// never left to the vendor GEMM, which would read the 16-bit weight: the
// weights a model decodes with must not depend on the row count.
struct GemmRule {
  int N, K;
  struct { int ks, nt[3]; } f[3];
};
const GemmRule GEMM_RULES[] = {
    { 6144,  2048, {{4, {2, 0, 0}}, {4, {2, 2, 2}}, {4, {2, 2, 2}}}},  // 1.3B QKV
    { 2048,  2048, {{8, {1, 1, 1}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 1.3B out-proj
    { 8192,  2048, {{4, {2, 2, 0}}, {4, {2, 2, 2}}, {4, {2, 2, 2}}}},  // 1.3B FFN1
    { 2048,  8192, {{8, {0, 0, 0}}, {8, {1, 1, 1}}, {8, {1, 1, 1}}}},  // 1.3B FFN2
    {12288,  4096, {{4, {0, 0, 0}}, {4, {4, 4, 4}}, {4, {4, 2, 2}}}},  // 6.7B QKV
    { 4096,  4096, {{4, {1, 0, 0}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 6.7B out-proj
    {16384,  4096, {{4, {0, 0, 0}}, {4, {4, 4, 4}}, {4, {4, 2, 2}}}},  // 6.7B FFN1
    { 4096, 16384, {{4, {0, 0, 0}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 6.7B FFN2
    {50304,  2048, {{4, {0, 0, 0}}, {4, {2, 4, 4}}, {4, {2, 2, 2}}}},  // LM head 1.3B
    {50304,  4096, {{4, {0, 0, 0}}, {4, {2, 4, 4}}, {4, {2, 2, 2}}}},  // LM head 6.7B
    { 3072,  1024, {{4, {1, 1, 1}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 345M QKV
    { 1024,  1024, {{4, {1, 1, 1}}, {4, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 345M out-proj
    { 4096,  1024, {{4, {1, 1, 1}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 345M FFN1
    { 1024,  4096, {{8, {1, 0, 0}}, {8, {1, 1, 1}}, {4, {1, 1, 1}}}},  // 345M FFN2
    {50304,  1024, {{4, {0, 0, 0}}, {4, {2, 4, 4}}, {4, {2, 2, 2}}}},  // LM head 345M
};

// Host entry of every weight format: validates the call, chooses the launch
// shape (nt / ks = 0: the rule below; else pinned by the caller) and launches.
// Returns the number of blocks launched, 0 for a call not covered: M outside
// 17..64, K % 1024 != 0, unaligned rows, an epilogue without its operands, a
// pinned shape the library does not have or K does not admit, or (no pin) a
// shape the launch table leaves to the vendor GEMM.
template <typename W>
int gemm_entry(int dt, int epi, int M, int N, int K, const void* x, long ldx, const void* w,
               long ldw, const typename W::sc* scale, const void* bias, const void* res, long ldres,
               void* y, long ldy, void* kc, void* vc, const long* pos, const int* rows, int heads,
               int head_dim, int maxlen, int nt, int ks, hipStream_t s) {
  if (M < 17 || M > 64 || N < 1 || K < 1024 || K % 1024 != 0 || (ldx % 8) ||
      (ldw * sizeof(typename W::elt) % 16) || !al16(x) || !al16(w) || y == nullptr ||
      ((W::SCALED || W::GROUPED) && scale == nullptr) ||
      (W::OPSCALED && (scale == nullptr || !al16(scale))))
    return 0;
  if (epi < GV_BIAS || epi > GV_QKV) return 0;
  if (epi == GV_RES && res == nullptr) return 0;
  if (epi == GV_QKV && (kc == nullptr || vc == nullptr || pos == nullptr || head_dim < 1 ||
                        N != 3 * heads * head_dim))
    return 0;
  const int mt = (M + 15) / 16;
  // A wave's K range is whole loop groups (int4: whole scale groups).  The
  // wave count is a function of (N, K, format) only: the table's, else
  // gemv_kernel's rule.
  const GemmRule* rule = nullptr;
  for (const GemmRule& r : GEMM_RULES)
    if (r.N == N && r.K == K) rule = &r;
  const int group = DG_CHUNK * W::PB;
  if (ks == 0) ks = rule ? rule->f[W::FMT].ks : (N <= 2048 && K % (8 * 256) == 0) ? 8 : 4;
  else if ((ks != 4 && ks != 8) || K % (ks * group) != 0) return 0;
  // Columns per block: the table's; a shape it does not hold gets the trend
  // of the sweep (narrow layers need every CU streaming, wide ones the x reuse
  // of a wide tile) and is never left to the vendor GEMM; int4 stays within
  // the tiles it has (gemm_tile_ok).
  if (nt == 0) {
    if (rule) {
      nt = rule->f[W::FMT].nt[mt - 2];
      if (nt == 0) return 0;
    } else {
      nt = N >= 12288 ? 4 : N >= 6144 ? 2 : 1;
      if (W::GROUPED && nt * mt > 8) nt = 2;
    }
  } else if (nt != 1 && nt != 2 && nt != 4) {
    return 0;
  }
  GemmArgs<W> a;
  a.x = (const uint16_t*)x; a.w = (const typename W::elt*)w; a.scale = scale;
  a.bias = (const uint16_t*)bias; a.res = (const uint16_t*)res; a.y = (uint16_t*)y;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldres = ldres;
  a.M = M; a.N = N; a.K = K; a.epi = epi;
  a.kc = (uint16_t*)kc; a.vc = (uint16_t*)vc; a.pos = pos; a.rows = rows;
  a.heads = heads; a.head_dim = head_dim; a.maxlen = maxlen;
  a.vec = al16(y) && ldy % 8 == 0 && al16(bias) &&
          (epi != GV_RES || (al16(res) && ldres % 8 == 0)) &&
          (epi != GV_QKV || (head_dim % 8 == 0 && al16(kc) && al16(vc)));
  const bool ok = dt == 0 ? gemm_launch<W, bf16>(a, ks, nt, mt, s)
                          : gemm_launch<W, f16>(a, ks, nt, mt, s);
  if (!ok) return 0;
  return (N + 16 * nt - 1) / (16 * nt);
}

}  // namespace

extern "C" int fx_decode_gemm(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                              const void* w, long ldw, const void* bias, const void* res,
                              long ldres, void* y, long ldy, void* kc, void* vc, const long* pos,
                              const int* rows, int heads, int head_dim, int maxlen, int nt, int ks,
                              hipStream_t s) {
  return gemm_entry<G16>(dt, epi, M, N, K, x, ldx, w, ldw, nullptr, bias, res, ldres, y, ldy, kc,
                         vc, pos, rows, heads, head_dim, maxlen, nt, ks, s);
}

extern "C" int fx_decode_gemm_w8(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                 const int8_t* wq, long ldw, const float* wscale,
                                 const void* bias, const void* res, long ldres, void* y, long ldy,
                                 void* kc, void* vc, const long* pos, const int* rows, int heads,
                                 int head_dim, int maxlen, int nt, int ks, hipStream_t s) {
  return gemm_entry<G8>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y, ldy, kc,
                        vc, pos, rows, heads, head_dim, maxlen, nt, ks, s);
}

extern "C" int fx_decode_gemm_w4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                 const uint8_t* wq, long ldw, const float* wscale,
                                 const void* bias, const void* res, long ldres, void* y, long ldy,
                                 void* kc, void* vc, const long* pos, const int* rows, int heads,
                                 int head_dim, int maxlen, int nt, int ks, hipStream_t s) {
  return gemm_entry<G4>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y, ldy, kc,
                        vc, pos, rows, heads, head_dim, maxlen, nt, ks, s);
}

extern "C" int fx_decode_gemm_mx4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                  const uint8_t* wq, long ldw, const uint8_t* wscale,
                                  const void* bias, const void* res, long ldres, void* y, long ldy,
                                  void* kc, void* vc, const long* pos, const int* rows, int heads,
                                  int head_dim, int maxlen, int nt, int ks, hipStream_t s) {
  return gemm_entry<GM4>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y, ldy, kc,
                         vc, pos, rows, heads, head_dim, maxlen, nt, ks, s);
}
