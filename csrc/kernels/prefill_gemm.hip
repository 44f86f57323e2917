// Weight-only quantised prefill GEMM: y[M, N] = x[M, K] dequant(W[N, K])^T,
// M >= 65, K % 1024 == 0, any N, 16-bit x and y (bf16 / fp16), fp32
// accumulation, with the decoder layer's element-wise work fused into the
// epilogue (GV_BIAS / GV_GELU / GV_RES of weight_operand.h; no GV_QKV scatter).
// The sibling of gemv_kernel (1..16 rows) and decode_gemm_kernel (17..64 rows)
// for the rows they do not take, on the SAME packed copies -- nothing is
// repacked: int8 q[N, K] with an fp32 scale [N]; int4 nibbles as pack_int4
// stores them with an fp32 scale [K / 256, N]; MXFP4 bytes as pack_mxfp4 stores
// them with the e8m0 scale bytes in _mx_scale_order (fleetx_amd/ops/quant.py).
//
// Tile geometry:
//  * a 4-wave workgroup owns 16 * MT x rows and 4 * 16 * NT output columns
//    (rows of W), MT in {4, 8}, NT in {1, 2, 4}.  Wave w owns the columns
//    [n0 + 16 NT w, n0 + 16 NT (w + 1)) and ALL the block's rows, so no wave
//    converts a weight another wave also converts: the conversion is paid once
//    per weight and block, not once per row tile;
//  * weights are stationary in registers.  A chunk is 64 k; lane (r, g) =
//    (lane % 16, lane / 16) loads the 16 contiguous k [16 g, 16 g + 16) of
//    weight row r of each of its NT column tiles (decode_gemm_kernel's lane
//    map: 16 / 8 / 8 bytes for int8 / int4 / MXFP4) straight to VGPRs, turns
//    them into two short8 MFMA A operands ONCE (cvt8; int4: the two-mask spread
//    first; MXFP4: mx4_cvt8 with the group scale from mx4_scale) and feeds each
//    to MT MFMAs v_mfma_f32_16x16x32.  Two register sets: chunk c + 1 is in
//    flight under chunk c's MFMAs.  The loads are nontemporal only while the
//    grid has ONE row block; with more, the other row blocks re-read the panel
//    from L2;
//  * the activations go through LDS: all four waves need the same 16 MT x 64
//    x tile of a chunk.  It is staged HBM -> LDS with global_load_lds, 16 bytes
//    per lane (a wave instruction is 8 rows of 128 bytes), in two stages of
//    16 MT * 128 bytes, one workgroup barrier per chunk.  The LDS side of that
//    load is lane-linear, so the bank swizzle is applied to the global source
//    address: slot s of row m holds the row's 16-byte piece s ^ f(m), f(m) =
//    bit 1 of m | bit 2 of m << 2.  The B fragments are read back with 16-byte
//    LDS reads, lane (r, g) pieces 2 g and 2 g + 1 of row 16 mt + r: 4 cycles
//    per wave instruction, the ideal (tools/lds_bank_sim.py --prefill-gemm).
//    x rows >= M repeat row M - 1 and are never stored; columns >= N clamp the
//    weight row and are never stored (decode_gemm_kernel's rules);
//  * scales.  int8: the row scale multiplies the accumulator in the epilogue.
//    int4: a group of 256 k (4 chunks) is summed from C = 0 per (nt, mt) tile
//    and entered as fma(sum, s / 16, acc), the group's scales loaded ahead of
//    its chunks.  MXFP4: the hardware conversion applies the scale, one fp32
//    tile per (nt, mt); the 16 scale bytes of a 512-k block are one load per
//    weight row, taken a loop group (256 k) ahead;
//  * epilogue from the accumulators, staged through LDS (each wave its own
//    16 MT x 16 floats per column tile, in the x stages' memory) so that a
//    thread handles 8 consecutive columns of one row: row scale, bias, GeLU or
//    residual, one rounding, one 16-byte store.  N % 8 != 0 or unaligned
//    operands take the scalar form of the same code.  Plain vector stores, no
//    atomics;
//  * grid: ceil(N / (64 NT)) * ceil(M / (16 MT)) blocks in one dimension;
//    blockIdx is remapped (xcd_remap) so that the row blocks of one weight
//    panel run on one XCD, next to each other in time, and share the panel in
//    that XCD's L2.
//
// Summation order -- the contract.  There is no K split: a row's sum is ONE
// MFMA chain over the chunks in k order (per chunk: the lane-map's first 8 k
// of every 16, then the second 8; int4: per group from zero, then the groups
// in order).  MT and NT do not enter the order, so the bits of an output row
// depend on that row of x alone: not on its index, on M, on the other rows or
// on the launch shape.  They are NOT the bits gemv_kernel or
// decode_gemm_kernel give the same row: those split K over their waves and sum
// the wave partials afterwards.
//
// Built without packed fp32 VALU, as all new HIP code here (FX_NO_PK32,
// fx_common.h).  Resources and measurements: profiles/quant_prefill/README.md.
#include "fx_api.h"
#include "weight_operand.h"

namespace {

constexpr int PG_CHUNK = 64;  // k per chunk: 16 per lane, two MFMA k-steps
constexpr int PG_PB = 4;      // chunks per loop group: 256 k, one int4 scale group

// Weight operand policies (weight_operand.h); the kernel chooses the load: the
// panel is streamed (load_w<raw, true>) only while it is read once, by one row
// block.  The names are this kernel's template arguments.
struct P8 : Op8 {};
struct P4 : Op4 {};
struct PM4 : OpM4 {};

template <typename W>
struct PrefillArgs {
  const uint16_t* x;
  const typename W::elt* w;
  const typename W::sc* scale;  // P8: [N]; P4: [K / 256, N]; PM4: [N, K / 32] bytes
  const uint16_t* bias;
  const uint16_t* res;
  uint16_t* y;
  long ldx, ldw, ldy, ldres;  // ldw in elt (P4 / PM4: bytes)
  int M, N, K, epi;
  int nbm;  // row blocks
  int vec;  // every epilogue operand admits 16-byte accesses at n % 8 == 0
};

// bank swizzle of the x stage: 16-byte slot s of row m holds piece s ^ pg_swz(m)
__device__ __forceinline__ int pg_swz(int m) { return ((m >> 1) & 1) | (((m >> 2) & 1) << 2); }

template <typename W, typename T, int MT, int NT, bool ST>
__global__ __launch_bounds__(256) FX_NO_PK32 void prefill_gemm_kernel(PrefillArgs<W> a) {
  constexpr int BM = 16 * MT;
  constexpr int STAGE = BM * 2 * PG_CHUNK;  // bytes of one x stage: BM rows of 128 bytes
  constexpr int NI = BM / 32;               // global_load_lds instructions per wave and chunk
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  // consecutive ids = the row blocks of one weight panel
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (lid % a.nbm) * BM;
  const int n0 = (lid / a.nbm) * (64 * NT) + 16 * NT * w;
  const typename W::elt* wp[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    wp[nt] = a.w + (long)min(n0 + 16 * nt + r, a.N - 1) * a.ldw + 16 * g / W::PACK;
  // x stage: 1 KiB piece p (8 rows) is one wave instruction; wave w loads
  // pieces w NI .. w NI + NI - 1; lane l writes slot l % 8 of row 8 p + l / 8
  const uint16_t* xs[NI];
#pragma unroll
  for (int u = 0; u < NI; ++u) {
    const int row = 8 * (w * NI + u) + (lane >> 3);
    xs[u] = a.x + (long)min(m0 + row, a.M - 1) * a.ldx + 8 * ((lane & 7) ^ pg_swz(row));
  }
  // B fragment of row tile mt, k-step i: piece 2 g + i of row 16 mt + r
  const int xr0 = 128 * r + 16 * ((2 * g) ^ pg_swz(r)), xr1 = xr0 ^ 16;
  // D[n][m] of tile (nt, mt): the lane holds n = 4 g + j, m = r
  floatx4 acc[NT][MT], t[W::GROUPED ? NT : 1][W::GROUPED ? MT : 1];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
  typename W::raw wv[2][NT];
  floatx4 sv[W::GROUPED ? NT : 1];
  const float* sp = nullptr;
  if constexpr (W::GROUPED) sp = a.scale;
  // OPSCALED: per weight row the 16 scale bytes of a 512-k block (dword i:
  // chunk i of either 256-k half) of this loop group (ev) and the next (en),
  // and the lane's byte in a dword: 2 * (half of the block) + g / 2
  uintx4 ev[W::OPSCALED ? NT : 1], en[W::OPSCALED ? NT : 1];
  const uint8_t* ep[W::OPSCALED ? NT : 1];
  if constexpr (W::OPSCALED) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      ep[nt] = reinterpret_cast<const uint8_t*>(a.scale) +
               (long)min(n0 + 16 * nt + r, a.N - 1) * (a.K / 32);
      en[nt] = *reinterpret_cast<const uintx4*>(ep[nt]);
    }
  }
  const int nb = a.K / PG_CHUNK;  // a multiple of 16 (host check)

// chunk c: weights into register set S, x into LDS stage S
#define PG_LOAD(S, c)                                                            \
  do {                                                                           \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                            \
        wv[S][nt] = load_w<typename W::raw, ST>(wp[nt] + (long)(c) * (PG_CHUNK / W::PACK)); \
    _Pragma("unroll") for (int u = 0; u < NI; ++u)                               \
        __builtin_amdgcn_global_load_lds(                                        \
            (const void*)(xs[u] + (long)(c) * PG_CHUNK),                         \
            (__attribute__((address_space(3))) void*)(lds + (S) * STAGE + (w * NI + u) * 1024), \
            16, 0, 0);                                                           \
  } while (0)
// chunk c (the I-th of its loop group) on set / stage S.  The wait and the
// barrier: chunk c's weights and this wave's part of its x tile have landed,
// every wave's part is visible, and every wave is done with chunk c - 1, whose
// stage chunk c + 1 is then loaded into, under chunk c's MFMAs.
#define PG_STEP(S, I, c, NEXT, dst)                                              \
  do {                                                                           \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             \
    __syncthreads();                                                             \
    if (NEXT) PG_LOAD(1 - (S), (c) + 1);                                         \
    short8 av[NT][2];                                                            \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                          \
      if constexpr (W::OPSCALED)                                                 \
        W::template ops<T>(wv[S][nt], mx4_scale(ev[nt][I] >> esh), av[nt]);      \
      else                                                                       \
        W::template ops<T>(wv[S][nt], av[nt]);                                   \
    }                                                                            \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                          \
      const char* xt = lds + (S) * STAGE + mt * 2048;                            \
      const short8 b0 = *reinterpret_cast<const short8*>(xt + xr0);              \
      const short8 b1 = *reinterpret_cast<const short8*>(xt + xr1);              \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                        \
        dst[nt][mt] = mma16<T>(av[nt][0], b0, dst[nt][mt]);                      \
        dst[nt][mt] = mma16<T>(av[nt][1], b1, dst[nt][mt]);                      \
      }                                                                          \
    }                                                                            \
  } while (0)
#define PG_GROUP_STEPS(dst)                                                      \
  do {                                                                           \
    PG_STEP(0, 0, c, true, dst);                                                 \
    PG_STEP(1, 1, c + 1, true, dst);                                             \
    PG_STEP(0, 2, c + 2, true, dst);                                             \
    PG_STEP(1, 3, c + 3, more, dst);                                             \
  } while (0)

  PG_LOAD(0, 0);
  for (int c = 0; c < nb; c += PG_PB) {
    const bool more = c + PG_PB < nb;
    int esh = 0;
    if constexpr (W::GROUPED) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[nt][j] = sp[min(n0 + 16 * nt + 4 * g + j, a.N - 1)];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) t[nt][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
      sp += a.N;
    }
    if constexpr (W::OPSCALED) {
      const int q = c / PG_PB;  // this loop group in units of 256 k
      esh = 16 * (q & 1) + 8 * (g >> 1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        ev[nt] = en[nt];
        if (more) en[nt] = *reinterpret_cast<const uintx4*>(ep[nt] + ((q + 1) >> 1) * 16);
      }
    }
    (void)esh;
    if constexpr (W::GROUPED) {
      PG_GROUP_STEPS(t);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[nt][mt][j] = __builtin_fmaf(t[nt][mt][j], sv[nt][j] * 0.0625f, acc[nt][mt][j]);
    } else {
      PG_GROUP_STEPS(acc);
    }
  }

#undef PG_GROUP_STEPS
#undef PG_STEP
#undef PG_LOAD

  // NT rounds of 16 columns: the wave's own red[m][n] (16 MT x 16 floats, a
  // quarter of the x stages), then 8 consecutive n of one row per thread and
  // pass.  The barriers order one round's reads before the next one's writes.
  float* red = reinterpret_cast<float*>(lds) + w * (BM * 16);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      *reinterpret_cast<floatx4*>(&red[(16 * mt + r) * 16 + 4 * g]) = acc[nt][mt];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MT / 2; ++it) {
      const int idx = 64 * it + lane;
      const int oct = idx & 1, ml = idx >> 1;
      const int m = m0 + ml, n = n0 + 16 * nt + 8 * oct;
      if (m < a.M && n < a.N) {
        const floatx4* p = reinterpret_cast<const floatx4*>(&red[ml * 16 + 8 * oct]);
        const floatx4 p0 = p[0], p1 = p[1];
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = p0[j];
          v[4 + j] = p1[j];
        }
        row_epilogue8<W, T, false>(a, m, n, v);
      }
    }
  }
}

// int4 keeps two fp32 tiles live per (nt, mt), the group sum and the
// accumulator: its 8 x 4 tile (256 accumulator registers before anything else)
// is not instantiated.  Every other combination compiles with scratch 0
// (profiles/quant_prefill/README.md).
template <typename W, int MT, int NT>
constexpr bool prefill_tile_ok = !(W::GROUPED && MT * NT > 16);

template <typename W, typename T, int MT, int NT>
bool prefill_go(const PrefillArgs<W>& a, hipStream_t s) {
  if constexpr (prefill_tile_ok<W, MT, NT>) {
    const dim3 grid(((a.N + 64 * NT - 1) / (64 * NT)) * a.nbm);
    // MT = 4 never has one row block (M >= 65)
    if (MT == 8 && a.nbm == 1)
      hipLaunchKernelGGL((prefill_gemm_kernel<W, T, MT, NT, MT == 8>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((prefill_gemm_kernel<W, T, MT, NT, false>), grid, dim3(256), 0, s, a);
    return true;
  }
  return false;
}
template <typename W, typename T, int MT>
bool prefill_launch_nt(const PrefillArgs<W>& a, int nt, hipStream_t s) {
  if (nt == 1) return prefill_go<W, T, MT, 1>(a, s);
  if (nt == 2) return prefill_go<W, T, MT, 2>(a, s);
  return prefill_go<W, T, MT, 4>(a, s);
}
template <typename W, typename T>
bool prefill_launch(const PrefillArgs<W>& a, int mt, int nt, hipStream_t s) {
  if (mt == 4) return prefill_launch_nt<W, T, 4>(a, nt, s);
  return prefill_launch_nt<W, T, 8>(a, nt, s);
}

// Launch shape from (M, N) and the format, from the sweep in
// profiles/quant_prefill/README.md (the four layer shapes of 1.3B and 6.7B and
// the LM head at 65 / 128 / 512 / 2048 rows, every tile, weights streamed from
// HBM).  b = ceil(N / 64) * ceil(M / 64), the blocks of the smallest tile:
//  * 64 columns and 64 rows per block win while the grid is small: wider
//    tiles lower the occupancy by more than their x reuse saves;
//  * from about a thousand blocks on, 128 rows per block, which halve the
//    times a panel is converted and re-read, are ahead -- int8 from b > 1024;
//    int4 and MXFP4 from b >= 1024 but only above 128 rows (a single row block
//    gains nothing from the tall tile: the LM head at 65 / 128 rows);
//  * MXFP4 alone, whose conversion is the cheapest and whose 8 x 2 tile still
//    runs two waves per SIMD, gains 15-35 % from 128 columns once b >= 2048.
// Against the best tile of each of the 36 cases the rule is within 10 % (int8),
// 5 % (int4) and 3 % (MXFP4).  Every format has the tiles its rule names.
template <typename W>
void prefill_rule(int M, int N, int& mt, int& nt) {
  const long b = (long)((N + 63) / 64) * ((M + 63) / 64);
  if (W::SCALED) mt = b > 1024 ? 8 : 4;
  else mt = (b >= 1024 && M > 128) ? 8 : 4;
  nt = (W::OPSCALED && mt == 8 && b >= 2048) ? 2 : 1;
}

// Host entry of every weight format: validates the call as gemm_entry<W> of
// decode_gemm.hip does, chooses the launch shape (mt = 0: the rule above; else
// pinned by the caller) and launches.  Returns the number of blocks launched,
// 0 for a call not covered: M < 65, K % 1024 != 0, unaligned rows, an epilogue
// outside GV_BIAS / GV_GELU / GV_RES or without its operands, a pinned shape
// the library does not have.
template <typename W>
int prefill_gemm_entry(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                       const void* w, long ldw, const typename W::sc* scale, const void* bias,
                       const void* res, long ldres, void* y, long ldy, int mt, int nt,
                       hipStream_t s) {
  if (M < 65 || N < 1 || K < 1024 || K % 1024 != 0 || (ldx % 8) ||
      (ldw * sizeof(typename W::elt) % 16) || !al16(x) || !al16(w) || y == nullptr ||
      scale == nullptr || (W::OPSCALED && !al16(scale)))
    return 0;
  if (epi < GV_BIAS || epi > GV_RES) return 0;
  if (epi == GV_RES && res == nullptr) return 0;
  if (mt == 0 && nt == 0) {
    prefill_rule<W>(M, N, mt, nt);
  } else if ((mt != 4 && mt != 8) || (nt != 1 && nt != 2 && nt != 4)) {
    return 0;
  }
  PrefillArgs<W> a;
  a.x = (const uint16_t*)x; a.w = (const typename W::elt*)w; a.scale = scale;
  a.bias = (const uint16_t*)bias; a.res = (const uint16_t*)res; a.y = (uint16_t*)y;
  a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldres = ldres;
  a.M = M; a.N = N; a.K = K; a.epi = epi;
  a.nbm = (M + 16 * mt - 1) / (16 * mt);
  a.vec = al16(y) && ldy % 8 == 0 && al16(bias) &&
          (epi != GV_RES || (al16(res) && ldres % 8 == 0));
  const bool ok = dt == 0 ? prefill_launch<W, bf16>(a, mt, nt, s)
                          : prefill_launch<W, f16>(a, mt, nt, s);
  if (!ok) return 0;
  return ((N + 64 * nt - 1) / (64 * nt)) * a.nbm;
}

}  // namespace

extern "C" int fx_prefill_gemm_w8(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                  const int8_t* wq, long ldw, const float* wscale,
                                  const void* bias, const void* res, long ldres, void* y,
                                  long ldy, int mt, int nt, hipStream_t s) {
  return prefill_gemm_entry<P8>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y,
                                ldy, mt, nt, s);
}

extern "C" int fx_prefill_gemm_w4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                  const uint8_t* wq, long ldw, const float* wscale,
                                  const void* bias, const void* res, long ldres, void* y,
                                  long ldy, int mt, int nt, hipStream_t s) {
  return prefill_gemm_entry<P4>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y,
                                ldy, mt, nt, s);
}

extern "C" int fx_prefill_gemm_mx4(int dt, int epi, int M, int N, int K, const void* x, long ldx,
                                   const uint8_t* wq, long ldw, const uint8_t* wscale,
                                   const void* bias, const void* res, long ldres, void* y,
                                   long ldy, int mt, int nt, hipStream_t s) {
  return prefill_gemm_entry<PM4>(dt, epi, M, N, K, x, ldx, wq, ldw, wscale, bias, res, ldres, y,
                                 ldy, mt, nt, s);
}
