// Decode attention over a KV cache: single-token, beam (nb queries per sample
// over a shared prompt) and window (W causal queries per sample).
//
// Parity: reference K18/K19 (generation decode with a KV cache,
// `single_model.py:109-114`, Paddle fused_multi_transformer decode path).
//
// Decode attention is memory bound (few query rows per (batch, head)): split-K
// over the cached keys (see decode_attn_split_kernel).  The beam and window
// kernels share one multi-query core (MQ and decode_attn_mq_*.inc) and all
// three share decode_attn_combine_kernel.
#include "fx_api.h"
#include "fx_common.h"

namespace {

// Split-K ("flash-decoding") single-token attention over a KV cache.
// q: [B, H, D] (strides sqb, sqh); caches: [B, maxlen, H, D] (skb, sks, skh);
// out: [B, H, D] (sob, D contiguous, head stride D).
// Pass 1: grid = B*H*nsplit workgroups; split s of (b, h) scores keys
//   [s*chunk, min((s+1)*chunk, len)): D/8 lanes cover one key row with 16-byte
//   loads, each lane group keeps 4 keys in flight per step (the kernel is HBM
//   bound: every cached byte is read once), online softmax per lane group,
//   merged through LDS into one partial (m, l, o[D]) per workgroup.
// Pass 2: one workgroup per (b, h) merges the nsplit partials.
// Small-batch long-context decode thus spreads over B*H*nsplit >= ~2 waves of
// workgroups instead of B*H (a few CUs out of 256).
// merge another online-softmax state (m2, l2, o2) into (m, l, o)
__device__ __forceinline__ void merge_state(float& m, float& l, float* o, float m2, float l2,
                                            const float* o2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  const float a = __expf(m - M), c = __expf(m2 - M);
  l = l * a + l2 * c;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = o[j] * a + o2[j] * c;
  m = M;
}

template <typename T, int D, int NW>
__global__ __launch_bounds__(64 * NW) void decode_attn_split_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const int* __restrict__ lens, float* __restrict__ ws,
    int H, int nsplit, int chunk, long sqb, long sqh, long skb, long sks, long skh, float scale,
    uint16_t* __restrict__ out, long sob) {
  constexpr int LPK = D / 8;        // lanes per key row
  constexpr int KPW = 64 / LPK;     // key rows per wave instruction
  constexpr int U = 4;              // key rows per lane group per step
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPK, c = (lane % LPK) * 8;
  const int len = lens[b];
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  float qv[8];
  load8<T>(q + b * sqb + hd * sqh + c, qv);
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] *= scale;
  float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
  const uint16_t* kb = kc + b * skb + hd * skh + c;
  const uint16_t* vb = vc + b * skb + hd * skh + c;
  // wave w, step: keys k0 + u*KPW*NW + w*KPW + sub, u < U.  NW = 16 for few
  // (batch, head) pairs: a whole short context is one step (one memory round
  // trip) of one workgroup instead of several steps of 4 waves
  for (int k0 = k_lo; k0 < k_hi; k0 += NW * KPW * U) {
    float sc[U];
    int key[U];
    // K and V rows of the step are loaded together (V does not depend on the
    // scores): one memory round trip per step instead of two
    uint4 kraw[U], vraw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      key[u] = k0 + (u * NW + w) * KPW + sub;
      const int kk = key[u] < k_hi ? key[u] : k_lo;  // in-range dummy row
      kraw[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * sks);
      vraw[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * sks);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kv[8];
      unpack8<T>(kraw[u], kv);
      sc[u] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sc[u] += kv[j] * qv[j];
    }
#pragma unroll
    for (int off = LPK / 2; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u) sc[u] += __shfl_xor(sc[u], off, 64);
    float mx = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (key[u] >= k_hi) sc[u] = -INFINITY;
      mx = fmaxf(mx, sc[u]);
    }
    if (mx == -INFINITY) continue;
    const float a = __expf(m - mx);
    l *= a;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= a;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (key[u] >= k_hi) continue;
      const float p = __expf(sc[u] - mx);
      float vv[8];
      unpack8<T>(vraw[u], vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += p * vv[j];
      l += p;
    }
    m = mx;
  }
  // merge: the KPW lane groups of a wave share each column slice -> lane
  // shuffles; then one state per (wave, slice) through LDS, NW-way
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
    float o2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o2[j] = __shfl_xor(o[j], off, 64);
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    merge_state(m, l, o, m2, l2, o2);
  }
  __shared__ float sm_m[NW * LPK], sm_l[NW * LPK], sm_o[NW * LPK][8];
  if (lane < LPK) {
    sm_m[w * LPK + lane] = m;
    sm_l[w * LPK + lane] = l;
#pragma unroll
    for (int j = 0; j < 8; ++j) sm_o[w * LPK + lane][j] = o[j];
  }
  __syncthreads();
  if (threadIdx.x < LPK) {
    float M = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; ++i) M = fmaxf(M, sm_m[i * LPK + threadIdx.x]);
    float L = 0.f, O[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) O[j] = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int t = i * LPK + threadIdx.x;
        if (sm_m[t] == -INFINITY) continue;
        const float a = __expf(sm_m[t] - M);
        L += sm_l[t] * a;
#pragma unroll
        for (int j = 0; j < 8; ++j) O[j] += sm_o[t][j] * a;
      }
    }
    if (nsplit == 1) {  // one split: normalise and store the output directly
      const float inv = L > 0.f ? 1.f / L : 0.f;
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = O[j] * inv;
      store8<T>(out + b * sob + hd * D + threadIdx.x * 8, r);
      return;
    }
    float* wp = ws + (long)blockIdx.x * (D + 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) wp[threadIdx.x * 8 + j] = O[j];
    if (threadIdx.x == 0) {
      wp[D] = M;
      wp[D + 1] = L;
    }
  }
}

template <typename T, int D>
__global__ __launch_bounds__(D) void decode_attn_combine_kernel(const float* __restrict__ ws,
                                                               uint16_t* __restrict__ out, int H,
                                                               int nsplit, long sob) {
  const int bh = blockIdx.x, b = bh / H, hd = bh % H, d = threadIdx.x;
  const float* base = ws + (long)bh * nsplit * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * (D + 2) + D]);
  float L = 0.f, O = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float* wp = base + s * (D + 2);
      if (wp[D] == -INFINITY) continue;
      const float a = __expf(wp[D] - M);
      L += wp[D + 1] * a;
      O += wp[d] * a;
    }
  }
  out[b * sob + hd * D + d] = Elt<T>::from_f(L > 0.f ? O / L : 0.f);
}

// Sum over the LPK (8 or 16) consecutive lanes that share a key row, on every
// lane of the group.  DPP lane permutes (xor 1, xor 2, mirror within 8, mirror
// within 16): one VALU add each and no LDS-pipeline round trip, which
// __shfl_xor costs.  With nb beams per key the score reductions are the bulk
// of the cross-lane traffic of beam_decode_attn_kernel.
template <int LPK>
__device__ __forceinline__ float group_sum(float v) {
  static_assert(LPK == 8 || LPK == 16, "lane group of 8 or 16");
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  if (LPK == 16)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

// ---- Multi-query core: the beam and window kernels are built from it.
// One workgroup of NW waves owns all nq <= NQ query rows row0 .. row0+nq-1 of one
// (sample, head, split): a K/V row is loaded once (16-byte loads, U rows in
// flight per lane group) and scored against every query, so a cache is streamed
// once per sample and not once per query.  NQ queries are held in registers (5
// and 7 run the 6 and 8 query code with query 0 repeated and not stored): per
// lane 8*NQ floats of q and of o, so U shrinks as NQ grows (measured for the
// beam kernel, carried over to the window kernel and not measured again).
// The core is MQ (the constants) and three parts that a kernel includes in
// this order: decode_attn_mq_init.inc (the state and its initialisation),
// decode_attn_mq_stream.inc ("stream rows [lo, hi) of one K/V cache"; which
// queries see a key is the kernel's choice: all of them, or query j sees key k
// iff k <= len0 + j) and decode_attn_mq_finish.inc (merge and epilogue).  Each
// part lists the names it takes from the kernel.
// Contracts, relied on by the kernels below and their callers:
// - Straight-line steps.  The per-query blocks of a step are straight-line
//   code: a masked key is selected away, not branched around, so the compiler
//   interleaves the queries' reduce / exp chains, which a wave cannot hide
//   behind other waves at 2 waves per SIMD.  A masked key enters as 0 * v:
//   every row that is loaded must hold finite values.
// - Finite NEG.  The running max starts at a large finite negative, so
//   exp(m - mx) never sees inf - inf.  The finish step turns a state that saw
//   no key into (-inf, 0, 0), as merge_state and the combine pass expect.
// - Rows read.  The stream over [lo, hi) loads rows [lo, hi) only (a lane
//   without a row in a step loads row lo again) and nothing if the range is
//   empty.
// - Slot invariance.  A query's result depends only on its q row and the keys
//   it sees, not on its slot j, provided the kernel's split bounds do not depend
//   on the lengths: the key -> (step, wave, lane group, u) map is a function
//   of the absolute key index and lo, and a step in which a query sees no key
//   leaves its state as it is (the score is NEG, so mx = m, exp(m - mx) = 1
//   and every product added is 0).
// Partials go to ws as [(row*H + h)*nsplit + split][D+2]:
// decode_attn_combine_kernel merges them with its "batch" = the number of rows.
//
// The parts are text included in the kernel's body, not functions, because
// here the results are a function of the instruction stream: the compiler
// contracts a * b + c to an FMA after it has vectorised, and one source line
// comes out fused in one unrolled copy and unfused in the next (merge_state's
// l in the two shuffle rounds at D 128, NQ 4).  Behind any function boundary,
// even one forwarding wrapper around a whole kernel body, the body is optimised
// on its own before it is inlined: all 96 instantiations then compile
// differently, and with other FMAs.  Included as text they compile to the
// instruction streams that the two separate copies had
// (profiles/decode_attn_core/README.md).
template <int D_, int NQ_, int NW_>
struct MQ {
  static constexpr int D = D_, NQ = NQ_, NW = NW_;
  static constexpr int LPK = D / 8;                        // lanes per key row
  static constexpr int KPW = 64 / LPK;                     // key rows per wave instruction
  static constexpr int U = NQ <= 2 ? 4 : NQ <= 4 ? 2 : 1;  // rows per lane group per step
  static constexpr int RB = NQ * NW <= 32 ? NQ : (32 / NW > 0 ? 32 / NW : 1);  // queries per merge round
  static constexpr int STEP = NW * KPW * U;                // rows per workgroup per step
  static constexpr float NEG = -1e30f;                     // "no key yet"
};

// Beam-search decode attention: nb beams per sample share the prompt.
// q / out: [B*nb, H, D]; prefix caches kp / vp: [B, S, H, D] (spb, sps, sph),
// plens [B]; generated caches kg / vg: [B*nb, G, H, D] (sgb, sgs, sgh), glens
// [B] valid slots; anc [B*nb, G] (row stride sab): row b*nb + anc[b*nb+j, s]
// holds in slot s the key of beam j's ancestor from step s.  anc is trusted to
// be in [0, nb).
// The key axis of row b*nb+j is the prefix [0, plens[b]) followed by the
// glens[b] generated slots; split-K over that axis exactly as above.  The
// prefix goes through the multi-query core (every beam sees every prefix key).
// Generated slots are loaded per beam through anc (short; sibling beams that
// share an ancestor hit the same lines), in the core's straight-line form.
// Prefix rows at or beyond plens[b] and slots at or beyond glens[b] are never
// read.
template <typename T, int D, int NB, int NW>
__global__ __launch_bounds__(64 * NW) void beam_decode_attn_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const int* __restrict__ plens,
    const uint16_t* __restrict__ kg, const uint16_t* __restrict__ vg,
    const int* __restrict__ glens, const int* __restrict__ anc, float* __restrict__ ws,
    uint16_t* __restrict__ out, int H, int nb, int nsplit, int chunk, long sqb, long sqh, long spb,
    long sps, long sph, long sgb, long sgs, long sgh, long sab, long sob, float scale) {
  using C = MQ<D, NB, NW>;
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / C::LPK, c = (lane % C::LPK) * 8;
  const int plen = plens[b], len = plen + glens[b];
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  const int lo = k_lo, hi = min(k_hi, plen);                    // prefix keys [lo, hi)
  const int g_lo = max(k_lo, plen) - plen, g_hi = k_hi - plen;  // generated slots [g_lo, g_hi)
  const long row0 = (long)b * nb;
  const int nq = nb;
#include "decode_attn_mq_init.inc"
  // ---- prefix: each K/V row is loaded once and scored against all beams
  const uint16_t* kb = kp + b * spb + hd * sph + c;
  const uint16_t* vb = vp + b * spb + hd * sph + c;
  const long ks = sps;
  constexpr bool causal = false;  // every beam sees every prefix key
  const int len0 = 0;
#include "decode_attn_mq_stream.inc"
  // ---- generated slots: beam j reads slot s from its ancestor's row
  for (int s0 = g_lo; s0 < g_hi; s0 += NW * C::KPW) {
    const int s = s0 + w * C::KPW + sub;
    const bool ok = s < g_hi;
    const int ss = ok ? s : g_lo;  // in-range dummy slot
    const long soff = (long)ss * sgs + hd * sgh + c;
    uint4 graw[NB], hraw[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const long row = row0 + anc[(row0 + (j < nb ? j : 0)) * sab + ss];
      graw[j] = *reinterpret_cast<const uint4*>(kg + row * sgb + soff);
      hraw[j] = *reinterpret_cast<const uint4*>(vg + row * sgb + soff);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float kv[8], vv[8];
      unpack8<T>(graw[j], kv);
      unpack8<T>(hraw[j], vv);
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) sc += kv[i] * qv[j][i];
      const float t = group_sum<C::LPK>(sc);
      sc = ok ? t : C::NEG;
      const float mx = fmaxf(m[j], sc);
      const float a = __expf(m[j] - mx), p = ok ? __expf(sc - mx) : 0.f;
      l[j] = l[j] * a + p;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[j][i] = o[j][i] * a + p * vv[i];
      m[j] = mx;
    }
  }
#include "decode_attn_mq_finish.inc"
}

// Window decode attention: W consecutive causal queries per sample over one
// KV cache (the verify step of speculative decoding).
// q / out: [B*W, H, D] (row strides sqb / sob); caches [B, maxlen, H, D] (skb,
// sks, skh); lens [B]: keys before the window.  The window's own K/V rows are
// in the cache at lens[b] .. lens[b]+W-1; row b*W + j attends to keys
// [0, lens[b] + j].  lens[b] + W <= maxlen is trusted.  Every row below
// lens[b] + W is loaded and enters masked queries as 0 * v, so those rows must
// hold finite values; rows at or beyond lens[b] + W are never read.
// The whole key axis goes through the multi-query core; the causal limit is its
// per-(query, key) select.  Slot invariance holds: the split bounds are
// multiples of chunk, a function of maxlen and nsplit.
template <typename T, int D, int NQ, int NW>
__global__ __launch_bounds__(64 * NW) void window_decode_attn_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const int* __restrict__ lens, float* __restrict__ ws,
    uint16_t* __restrict__ out, int H, int W, int nsplit, int chunk, long sqb, long sqh, long skb,
    long sks, long skh, long sob, float scale) {
  using C = MQ<D, NQ, NW>;
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / C::LPK, c = (lane % C::LPK) * 8;
  const int len0 = lens[b];
  const int lo = split * chunk, hi = min(len0 + W, lo + chunk);
  const long row0 = (long)b * W;
  const int nq = W;
#include "decode_attn_mq_init.inc"
  const uint16_t* kb = kc + b * skb + hd * skh + c;
  const uint16_t* vb = vc + b * skb + hd * skh + c;
  const long ks = sks;
  constexpr bool causal = true;
#include "decode_attn_mq_stream.inc"
#include "decode_attn_mq_finish.inc"
}

// Host dispatch of a multi-query kernel family K (K::fn<T, D, NQ, NW>): dtype
// 0 bf16 / 1 fp16, D 64 / 128, rows 1..8 -> NQ in {1, 2, 3, 4, 6, 8}, wide -> 8
// waves else 4; g workgroups.  Then the combine pass over B*rows*H outputs if
// nsplit > 1.  The caller has checked dt, D and rows.
struct BeamKernels {
  template <typename T, int D, int NQ, int NW>
  static constexpr auto fn = beam_decode_attn_kernel<T, D, NQ, NW>;
};
struct WindowKernels {
  template <typename T, int D, int NQ, int NW>
  static constexpr auto fn = window_decode_attn_kernel<T, D, NQ, NW>;
};

template <typename K, typename T, int D, int NQ, typename... A>
void mq_launch_nq(bool wide, int g, hipStream_t st, A... a) {
  if (wide) hipLaunchKernelGGL((K::template fn<T, D, NQ, 8>), g, 512, 0, st, a...);
  else hipLaunchKernelGGL((K::template fn<T, D, NQ, 4>), g, 256, 0, st, a...);
}

template <typename K, typename T, int D, typename... A>
void mq_launch_td(int rows, bool wide, int g, hipStream_t st, A... a) {
  switch (rows) {
    case 1: mq_launch_nq<K, T, D, 1>(wide, g, st, a...); break;
    case 2: mq_launch_nq<K, T, D, 2>(wide, g, st, a...); break;
    case 3: mq_launch_nq<K, T, D, 3>(wide, g, st, a...); break;
    case 4: mq_launch_nq<K, T, D, 4>(wide, g, st, a...); break;
    case 5:
    case 6: mq_launch_nq<K, T, D, 6>(wide, g, st, a...); break;
    default: mq_launch_nq<K, T, D, 8>(wide, g, st, a...); break;
  }
}

template <typename K, typename... A>
void mq_launch(int dt, int D, int rows, bool wide, int g, hipStream_t st, A... a) {
  if (dt == 0) {
    if (D == 128) mq_launch_td<K, bf16, 128>(rows, wide, g, st, a...);
    else mq_launch_td<K, bf16, 64>(rows, wide, g, st, a...);
  } else {
    if (D == 128) mq_launch_td<K, f16, 128>(rows, wide, g, st, a...);
    else mq_launch_td<K, f16, 64>(rows, wide, g, st, a...);
  }
}

void mq_combine(int dt, int D, int n, const float* ws, void* out, int H, int nsplit, long sob,
                hipStream_t st) {
  uint16_t* o = (uint16_t*)out;
  if (dt == 0) {
    if (D == 128) decode_attn_combine_kernel<bf16, 128><<<n, 128, 0, st>>>(ws, o, H, nsplit, sob);
    else decode_attn_combine_kernel<bf16, 64><<<n, 64, 0, st>>>(ws, o, H, nsplit, sob);
  } else {
    if (D == 128) decode_attn_combine_kernel<f16, 128><<<n, 128, 0, st>>>(ws, o, H, nsplit, sob);
    else decode_attn_combine_kernel<f16, 64><<<n, 64, 0, st>>>(ws, o, H, nsplit, sob);
  }
}

}  // namespace

// dt: 0 bf16 / 1 fp16; ws: fp32 workspace of B*H*nsplit*(D+2); chunk = keys per split
extern "C" int fx_decode_attn(int dt, const void* q, const void* kc, const void* vc, void* out,
                              const int* lens, int B, int H, int D, int maxlen, int nsplit,
                              float* ws, long sqb, long sqh, long skb, long sks, long skh,
                              long sob, float scale, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (nsplit < 1) return -2;
  const int chunk = (maxlen + nsplit - 1) / nsplit;
  const int g = B * H * nsplit;
  // few workgroups (small batch x heads): 16 waves each, so a short context
  // is one load step; many: 4 waves
  const bool wide = g < 256;
#define FX_DEC(TT, DD)                                                                           \
  do {                                                                                           \
    if (wide)                                                                                    \
      decode_attn_split_kernel<TT, DD, 16><<<g, 1024, 0, st>>>(                                  \
          (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, ws, H, nsplit,     \
          chunk, sqb, sqh, skb, sks, skh, scale, (uint16_t*)out, sob);                           \
    else                                                                                         \
      decode_attn_split_kernel<TT, DD, 4><<<g, 256, 0, st>>>(                                    \
          (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, ws, H, nsplit,     \
          chunk, sqb, sqh, skb, sks, skh, scale, (uint16_t*)out, sob);                           \
    if (nsplit > 1)                                                                              \
      decode_attn_combine_kernel<TT, DD><<<B * H, DD, 0, st>>>(ws, (uint16_t*)out, H, nsplit, sob); \
  } while (0)
  if (dt == 0) {
    if (D == 128) FX_DEC(bf16, 128); else FX_DEC(bf16, 64);
  } else if (dt == 1) {
    if (D == 128) FX_DEC(f16, 128); else FX_DEC(f16, 64);
  } else {
    return -3;
  }
#undef FX_DEC
  return 0;
}

// Beam decode attention (see beam_decode_attn_kernel).  dt: 0 bf16 / 1 fp16;
// S / G: allocated prefix rows / generated slots; chunk = keys per split of the
// S + G key axis; ws: fp32 workspace of B*nb*H*nsplit*(D+2); nw: waves per
// workgroup, 4 or 8, 0 = by the number of workgroups.
extern "C" int fx_beam_decode_attn(int dt, const void* q, const void* kp, const void* vp,
                                   const int* plens, const void* kg, const void* vg,
                                   const int* glens, const int* anc, void* out, float* ws, int B,
                                   int nb, int H, int D, int S, int G, int nsplit, long sqb,
                                   long sqh, long spb, long sps, long sph, long sgb, long sgs,
                                   long sgh, long sab, long sob, float scale, int nw,
                                   hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (nsplit < 1) return -2;
  if (dt != 0 && dt != 1) return -3;
  if (nb < 1 || nb > 8) return -4;
  if (nw != 0 && nw != 4 && nw != 8) return -5;
  const int chunk = (S + G + nsplit - 1) / nsplit;
  const int g = B * H * nsplit;
  // up to one workgroup per CU: 8 waves each (one resident round covers the
  // CUs with half the partials of 4-wave workgroups); more: 4 waves, of which
  // 2-3 workgroups fit a CU
  const bool wide = nw == 8 || (nw == 0 && g <= 256);
  mq_launch<BeamKernels>(dt, D, nb, wide, g, st, (const uint16_t*)q, (const uint16_t*)kp,
                         (const uint16_t*)vp, plens, (const uint16_t*)kg, (const uint16_t*)vg,
                         glens, anc, ws, (uint16_t*)out, H, nb, nsplit, chunk, sqb, sqh, spb, sps,
                         sph, sgb, sgs, sgh, sab, sob, scale);
  if (nsplit > 1) mq_combine(dt, D, B * nb * H, ws, out, H, nsplit, sob, st);
  return 0;
}

// Window decode attention (see window_decode_attn_kernel).  dt: 0 bf16 / 1 fp16;
// W: queries per sample, 1..8; chunk = keys per split of the maxlen key axis; ws:
// fp32 workspace of B*W*H*nsplit*(D+2); nw: waves per workgroup, 4 or 8, 0 = by
// the number of workgroups (the beam launcher's rule).
extern "C" int fx_window_decode_attn(int dt, const void* q, const void* kc, const void* vc,
                                     const int* lens, void* out, float* ws, int B, int W, int H,
                                     int D, int maxlen, int nsplit, long sqb, long sqh, long skb,
                                     long sks, long skh, long sob, float scale, int nw,
                                     hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (nsplit < 1) return -2;
  if (dt != 0 && dt != 1) return -3;
  if (W < 1 || W > 8) return -4;
  if (nw != 0 && nw != 4 && nw != 8) return -5;
  const int chunk = (maxlen + nsplit - 1) / nsplit;
  const int g = B * H * nsplit;
  const bool wide = nw == 8 || (nw == 0 && g <= 256);
  mq_launch<WindowKernels>(dt, D, W, wide, g, st, (const uint16_t*)q, (const uint16_t*)kc,
                           (const uint16_t*)vc, lens, ws, (uint16_t*)out, H, W, nsplit, chunk,
                           sqb, sqh, skb, sks, skh, sob, scale);
  if (nsplit > 1) mq_combine(dt, D, B * W * H, ws, out, H, nsplit, sob, st);
  return 0;
}
