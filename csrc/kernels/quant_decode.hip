// QAT fake-quant (abs-max, symmetric int-N) and single-token decode attention
// over a KV cache.
//
// Parity: reference K23 (paddleslim QAT: abs_max weights / moving-average
// abs_max activations, 8 bit; `pretrain_gpt_345M_mp8_qat.yaml:35-44`) and
// K18/K19 (generation decode with a KV cache, `single_model.py:109-114`,
// Paddle fused_multi_transformer decode path).
//
// Decode attention is memory bound (one query row per (batch, head)): split-K
// over the cached keys (see decode_attn_split_kernel).
#include "fx_api.h"
#include "fx_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void absmax_kernel(const uint16_t* __restrict__ x, long n,
                                                     float* __restrict__ out) {
  float m = 0.f;
  const long n8 = n / 8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float a[8];
    load8<T>(x + i * 8, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(a[j]));
  }
  for (long i = n8 * 8 + blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    m = fmaxf(m, fabsf(Elt<T>::to_f(x[i])));
  m = wave_max(m);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<unsigned int*>(out), __float_as_uint(m));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fake_quant_kernel(const uint16_t* __restrict__ x,
                                                         uint16_t* __restrict__ y,
                                                         const float* __restrict__ scale, int bits,
                                                         long n) {
  const float s = fmaxf(*scale, 1e-8f);
  const float qmax = (float)((1 << (bits - 1)) - 1);
  const float inv = qmax / s, deq = s / qmax;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float v = Elt<T>::to_f(x[i]);
    float q = fminf(fmaxf(rintf(v * inv), -qmax), qmax);
    y[i] = Elt<T>::from_f(q * deq);
  }
}

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

// Beam-search decode attention: nb beams per sample share the prompt.
// q / out: [B*nb, H, D]; prefix caches kp / vp: [B, S, H, D] (spb, sps, sph),
// plens [B]; generated caches kg / vg: [B*nb, G, H, D] (sgb, sgs, sgh), glens
// [B] valid slots; anc [B*nb, G] (row stride sab): row b*nb + anc[b*nb+j, s]
// holds in slot s the key of beam j's ancestor from step s.  anc is trusted to
// be in [0, nb).
// The key axis of row b*nb+j is the prefix [0, plens[b]) followed by the
// glens[b] generated slots; split-K over that axis exactly as above.  One
// workgroup owns all nb queries of one (b, h, split): a prefix K/V row is
// loaded once (16-byte loads, U rows in flight per lane group) and scored
// against every beam, so the prompt is streamed once per sample and not once
// per beam.  Generated slots are loaded per beam through anc (short; sibling
// beams that share an ancestor hit the same lines).
// NB >= nb beams are held in registers (5 and 7 beams run the 6 and 8 beam
// code with beam 0 repeated and not stored): per lane 8*NB floats of q and of
// o, so U shrinks as NB grows.  The per-beam blocks of a step are straight-line
// code (masked keys are selected away, not branched around; the running max
// starts at a large finite negative so no inf - inf arises): the compiler
// interleaves the beams' reduce / exp chains, which a wave cannot hide behind
// other waves at 2 waves per SIMD.  The waves are merged through LDS in rounds
// of RB beams (static LDS stays far below 64 KB also for 16 waves).
// Partials go to ws as [(row*H + h)*nsplit + split][D+2]: decode_attn_combine_kernel
// merges them with its "batch" = B*nb.
template <typename T, int D, int NB, int NW>
__global__ __launch_bounds__(64 * NW) void beam_decode_attn_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const int* __restrict__ plens,
    const uint16_t* __restrict__ kg, const uint16_t* __restrict__ vg,
    const int* __restrict__ glens, const int* __restrict__ anc, float* __restrict__ ws,
    uint16_t* __restrict__ out, int H, int nb, int nsplit, int chunk, long sqb, long sqh, long spb,
    long sps, long sph, long sgb, long sgs, long sgh, long sab, long sob, float scale) {
  constexpr int LPK = D / 8;                     // lanes per key row
  constexpr int KPW = 64 / LPK;                  // key rows per wave instruction
  constexpr int U = NB <= 2 ? 4 : NB <= 4 ? 2 : 1;  // prefix rows per lane group per step
  constexpr int RB = NB * NW <= 32 ? NB : (32 / NW > 0 ? 32 / NW : 1);  // beams per merge round
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPK, c = (lane % LPK) * 8;
  const int plen = plens[b], len = plen + glens[b];
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  const int p_hi = min(k_hi, plen);                      // prefix keys [k_lo, p_hi)
  const int g_lo = max(k_lo, plen) - plen, g_hi = k_hi - plen;  // generated slots [g_lo, g_hi)
  constexpr float NEG = -1e30f;  // "no key yet": finite, so exp(m - mx) never sees inf - inf
  const long row0 = (long)b * nb;
  float qv[NB][8], o[NB][8], m[NB], l[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    load8<T>(q + (row0 + (j < nb ? j : 0)) * sqb + hd * sqh + c, qv[j]);
    m[j] = NEG;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qv[j][i] *= scale;
      o[j][i] = 0.f;
    }
  }
  // ---- prefix: each K/V row is loaded once and scored against all beams
  const uint16_t* kb = kp + b * spb + hd * sph + c;
  const uint16_t* vb = vp + b * spb + hd * sph + c;
  // software pipeline: the rows of step i+1 are requested before step i is
  // scored, so a wave overlaps its own memory round trip with its math (with
  // nb beams the math per row is long, and few waves fit per SIMD)
  constexpr int STEP = NW * KPW * U;
  uint4 kraw[U], vraw[U], knext[U], vnext[U];
  if (k_lo < p_hi) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = k_lo + (u * NW + w) * KPW + sub;
      const int kk = key < p_hi ? key : k_lo;  // in-range dummy row
      kraw[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * sps);
      vraw[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * sps);
    }
  }
  for (int k0 = k_lo; k0 < p_hi; k0 += STEP) {
    const bool more = k0 + STEP < p_hi;
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = k0 + STEP + (u * NW + w) * KPW + sub;
        const int kk = key < p_hi ? key : k_lo;
        knext[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * sps);
        vnext[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * sps);
      }
    }
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ok[u] = k0 + (u * NW + w) * KPW + sub < p_hi;
    float kv[U][8], vv[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unpack8<T>(kraw[u], kv[u]);
      unpack8<T>(vraw[u], vv[u]);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float sc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sc[u] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[u] += kv[u][i] * qv[j][i];
      }
      float mx = m[j];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float t = group_sum<LPK>(sc[u]);
        sc[u] = ok[u] ? t : NEG;
        mx = fmaxf(mx, sc[u]);
      }
      const float a = __expf(m[j] - mx);
      l[j] *= a;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[j][i] *= a;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = ok[u] ? __expf(sc[u] - mx) : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[j][i] += p * vv[u][i];
        l[j] += p;
      }
      m[j] = mx;
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        kraw[u] = knext[u];
        vraw[u] = vnext[u];
      }
    }
  }
  // ---- generated slots: beam j reads slot s from its ancestor's row
  for (int s0 = g_lo; s0 < g_hi; s0 += NW * KPW) {
    const int s = s0 + w * KPW + sub;
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
      const float t = group_sum<LPK>(sc);
      sc = ok ? t : NEG;
      const float mx = fmaxf(m[j], sc);
      const float a = __expf(m[j] - mx), p = ok ? __expf(sc - mx) : 0.f;
      l[j] = l[j] * a + p;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[j][i] = o[j][i] * a + p * vv[i];
      m[j] = mx;
    }
  }
  // a state that saw no key is (-inf, 0, 0), as merge_state and the combine pass expect
#pragma unroll
  for (int j = 0; j < NB; ++j) m[j] = l[j] > 0.f ? m[j] : -INFINITY;
  // ---- merge: lane groups of a wave by shuffles, then the waves through LDS
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) {
      float o2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o2[i] = __shfl_xor(o[j][i], off, 64);
      const float m2 = __shfl_xor(m[j], off, 64), l2 = __shfl_xor(l[j], off, 64);
      merge_state(m[j], l[j], o[j], m2, l2, o2);
    }
  }
  __shared__ float sm_m[RB][NW * LPK], sm_l[RB][NW * LPK], sm_o[RB][NW * LPK][8];
#pragma unroll
  for (int r0 = 0; r0 < NB; r0 += RB) {
    if (r0 > 0) __syncthreads();
    if (lane < LPK) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if (r0 + r >= NB) continue;
        sm_m[r][w * LPK + lane] = m[r0 + r];
        sm_l[r][w * LPK + lane] = l[r0 + r];
#pragma unroll
        for (int i = 0; i < 8; ++i) sm_o[r][w * LPK + lane][i] = o[r0 + r][i];
      }
    }
    __syncthreads();
    // thread t merges beam r0 + t / LPK, column slice t % LPK
    const int r = threadIdx.x / LPK, sl = threadIdx.x % LPK, j = r0 + r;
    if (r < RB && j < nb) {
      float M = -INFINITY, L = 0.f, O[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) O[i] = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i)
        merge_state(M, L, O, sm_m[r][i * LPK + sl], sm_l[r][i * LPK + sl], sm_o[r][i * LPK + sl]);
      if (nsplit == 1) {  // one split: normalise and store the output directly
        const float inv = L > 0.f ? 1.f / L : 0.f;
        float res[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) res[i] = O[i] * inv;
        store8<T>(out + (row0 + j) * sob + hd * D + sl * 8, res);
      } else {
        float* wp = ws + (((row0 + j) * H + hd) * nsplit + split) * (D + 2);
#pragma unroll
        for (int i = 0; i < 8; ++i) wp[sl * 8 + i] = O[i];
        if (sl == 0) {
          wp[D] = M;
          wp[D + 1] = L;
        }
      }
    }
  }
}

// Window decode attention: W consecutive causal queries per sample over one
// KV cache (the verify step of speculative decoding).
// q / out: [B*W, H, D] (row strides sqb / sob); caches [B, maxlen, H, D] (skb,
// sks, skh); lens [B]: keys before the window.  The window's own K/V rows are
// in the cache at lens[b] .. lens[b]+W-1; row b*W + j attends to keys
// [0, lens[b] + j].  lens[b] + W <= maxlen is trusted.  Every row below
// lens[b] + W is loaded and enters masked queries as 0 * v, so those rows must
// hold finite values; rows at or beyond lens[b] + W are never read.
// One workgroup owns all W queries of one (b, h, split), as the beam kernel
// owns its beams: a K/V row is loaded once (16-byte loads, U rows in flight per
// lane group, the next step's rows requested before this step is scored) and
// scored against every query.  The causal limit is a per-(query, key) select.
// NQ >= W queries are held in registers (5 and 7 run the 6 and 8 query code
// with query 0 repeated and not stored).  U per NQ is the beam kernel's choice,
// carried over and not measured again for this kernel.
// Slot invariance: a query's result depends only on its q row and the keys it
// sees, not on its slot j.  The split bounds are multiples of chunk (a function
// of maxlen and nsplit), the key -> (step, wave, lane group, u) map is a
// function of the absolute key index, and a step in which a query sees no key
// leaves its state as it is: the score is NEG (finite), so mx = m, exp(m - mx)
// = 1 and every product added is 0.
// Partials go to ws as [(row*H + h)*nsplit + split][D+2]: decode_attn_combine_kernel
// merges them with its "batch" = B*W.
template <typename T, int D, int NQ, int NW>
__global__ __launch_bounds__(64 * NW) void window_decode_attn_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const int* __restrict__ lens, float* __restrict__ ws,
    uint16_t* __restrict__ out, int H, int W, int nsplit, int chunk, long sqb, long sqh, long skb,
    long sks, long skh, long sob, float scale) {
  constexpr int LPK = D / 8;                     // lanes per key row
  constexpr int KPW = 64 / LPK;                  // key rows per wave instruction
  constexpr int U = NQ <= 2 ? 4 : NQ <= 4 ? 2 : 1;  // rows per lane group per step
  constexpr int RB = NQ * NW <= 32 ? NQ : (32 / NW > 0 ? 32 / NW : 1);  // queries per merge round
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPK, c = (lane % LPK) * 8;
  const int len0 = lens[b];
  const int k_lo = split * chunk, k_hi = min(len0 + W, k_lo + chunk);
  constexpr float NEG = -1e30f;  // "no key yet": finite, so exp(m - mx) never sees inf - inf
  const long row0 = (long)b * W;
  float qv[NQ][8], o[NQ][8], m[NQ], l[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    load8<T>(q + (row0 + (j < W ? j : 0)) * sqb + hd * sqh + c, qv[j]);
    m[j] = NEG;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qv[j][i] *= scale;
      o[j][i] = 0.f;
    }
  }
  const uint16_t* kb = kc + b * skb + hd * skh + c;
  const uint16_t* vb = vc + b * skb + hd * skh + c;
  constexpr int STEP = NW * KPW * U;
  uint4 kraw[U], vraw[U], knext[U], vnext[U];
  if (k_lo < k_hi) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = k_lo + (u * NW + w) * KPW + sub;
      const int kk = key < k_hi ? key : k_lo;  // in-range dummy row
      kraw[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * sks);
      vraw[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * sks);
    }
  }
  for (int k0 = k_lo; k0 < k_hi; k0 += STEP) {
    const bool more = k0 + STEP < k_hi;
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = k0 + STEP + (u * NW + w) * KPW + sub;
        const int kk = key < k_hi ? key : k_lo;
        knext[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * sks);
        vnext[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * sks);
      }
    }
    // key u is visible to query j iff it lies in this split and key <= len0 + j,
    // i.e. j >= jmin[u] (NQ for a key outside the split)
    int jmin[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = k0 + (u * NW + w) * KPW + sub;
      jmin[u] = key < k_hi ? key - len0 : NQ;
    }
    float kv[U][8], vv[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unpack8<T>(kraw[u], kv[u]);
      unpack8<T>(vraw[u], vv[u]);
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      float sc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sc[u] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[u] += kv[u][i] * qv[j][i];
      }
      float mx = m[j];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float t = group_sum<LPK>(sc[u]);
        sc[u] = j >= jmin[u] ? t : NEG;
        mx = fmaxf(mx, sc[u]);
      }
      const float a = __expf(m[j] - mx);
      l[j] *= a;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[j][i] *= a;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = j >= jmin[u] ? __expf(sc[u] - mx) : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[j][i] += p * vv[u][i];
        l[j] += p;
      }
      m[j] = mx;
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        kraw[u] = knext[u];
        vraw[u] = vnext[u];
      }
    }
  }
  // a state that saw no key is (-inf, 0, 0), as merge_state and the combine pass expect
#pragma unroll
  for (int j = 0; j < NQ; ++j) m[j] = l[j] > 0.f ? m[j] : -INFINITY;
  // ---- merge: lane groups of a wave by shuffles, then the waves through LDS
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) {
      float o2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o2[i] = __shfl_xor(o[j][i], off, 64);
      const float m2 = __shfl_xor(m[j], off, 64), l2 = __shfl_xor(l[j], off, 64);
      merge_state(m[j], l[j], o[j], m2, l2, o2);
    }
  }
  __shared__ float sm_m[RB][NW * LPK], sm_l[RB][NW * LPK], sm_o[RB][NW * LPK][8];
#pragma unroll
  for (int r0 = 0; r0 < NQ; r0 += RB) {
    if (r0 > 0) __syncthreads();
    if (lane < LPK) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if (r0 + r >= NQ) continue;
        sm_m[r][w * LPK + lane] = m[r0 + r];
        sm_l[r][w * LPK + lane] = l[r0 + r];
#pragma unroll
        for (int i = 0; i < 8; ++i) sm_o[r][w * LPK + lane][i] = o[r0 + r][i];
      }
    }
    __syncthreads();
    // thread t merges query r0 + t / LPK, column slice t % LPK
    const int r = threadIdx.x / LPK, sl = threadIdx.x % LPK, j = r0 + r;
    if (r < RB && j < W) {
      float M = -INFINITY, L = 0.f, O[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) O[i] = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i)
        merge_state(M, L, O, sm_m[r][i * LPK + sl], sm_l[r][i * LPK + sl], sm_o[r][i * LPK + sl]);
      if (nsplit == 1) {  // one split: normalise and store the output directly
        const float inv = L > 0.f ? 1.f / L : 0.f;
        float res[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) res[i] = O[i] * inv;
        store8<T>(out + (row0 + j) * sob + hd * D + sl * 8, res);
      } else {
        float* wp = ws + (((row0 + j) * H + hd) * nsplit + split) * (D + 2);
#pragma unroll
        for (int i = 0; i < 8; ++i) wp[sl * 8 + i] = O[i];
        if (sl == 0) {
          wp[D] = M;
          wp[D + 1] = L;
        }
      }
    }
  }
}

}  // namespace

extern "C" void fx_absmax(int dtype, const void* x, long n, float* out, hipStream_t st) {
  long g = (n / 8 + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  if (dtype == 0) absmax_kernel<bf16><<<(int)g, 256, 0, st>>>((const uint16_t*)x, n, out);
  else absmax_kernel<f16><<<(int)g, 256, 0, st>>>((const uint16_t*)x, n, out);
}

extern "C" int fx_fake_quant_fwd(int dtype, const void* x, void* y, const float* scale, int bits,
                                 long n, hipStream_t st) {
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  if (dtype == 0)
    fake_quant_kernel<bf16><<<(int)g, 256, 0, st>>>((const uint16_t*)x, (uint16_t*)y, scale, bits, n);
  else
    fake_quant_kernel<f16><<<(int)g, 256, 0, st>>>((const uint16_t*)x, (uint16_t*)y, scale, bits, n);
  return 0;
}

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
#define FX_BEAM(TT, DD, NBB)                                                                     \
  do {                                                                                           \
    if (wide)                                                                                    \
      beam_decode_attn_kernel<TT, DD, NBB, 8><<<g, 512, 0, st>>>(                                \
          (const uint16_t*)q, (const uint16_t*)kp, (const uint16_t*)vp, plens,                   \
          (const uint16_t*)kg, (const uint16_t*)vg, glens, anc, ws, (uint16_t*)out, H, nb,       \
          nsplit, chunk, sqb, sqh, spb, sps, sph, sgb, sgs, sgh, sab, sob, scale);               \
    else                                                                                         \
      beam_decode_attn_kernel<TT, DD, NBB, 4><<<g, 256, 0, st>>>(                                \
          (const uint16_t*)q, (const uint16_t*)kp, (const uint16_t*)vp, plens,                   \
          (const uint16_t*)kg, (const uint16_t*)vg, glens, anc, ws, (uint16_t*)out, H, nb,       \
          nsplit, chunk, sqb, sqh, spb, sps, sph, sgb, sgs, sgh, sab, sob, scale);               \
  } while (0)
#define FX_BEAM_NB(TT, DD)                                                                       \
  do {                                                                                           \
    switch (nb) {                                                                                \
      case 1: FX_BEAM(TT, DD, 1); break;                                                         \
      case 2: FX_BEAM(TT, DD, 2); break;                                                         \
      case 3: FX_BEAM(TT, DD, 3); break;                                                         \
      case 4: FX_BEAM(TT, DD, 4); break;                                                         \
      case 5:                                                                                    \
      case 6: FX_BEAM(TT, DD, 6); break;                                                         \
      default: FX_BEAM(TT, DD, 8); break;                                                        \
    }                                                                                            \
    if (nsplit > 1)                                                                              \
      decode_attn_combine_kernel<TT, DD><<<B * nb * H, DD, 0, st>>>(ws, (uint16_t*)out, H,       \
                                                                    nsplit, sob);                \
  } while (0)
  if (dt == 0) {
    if (D == 128) FX_BEAM_NB(bf16, 128); else FX_BEAM_NB(bf16, 64);
  } else {
    if (D == 128) FX_BEAM_NB(f16, 128); else FX_BEAM_NB(f16, 64);
  }
#undef FX_BEAM_NB
#undef FX_BEAM
  return 0;
}

// Window decode attention (see window_decode_attn_kernel).  dt: 0 bf16 / 1 fp16;
// W: queries per sample, 1..8; chunk = keys per split of the maxlen key axis; ws:
// fp32 workspace of B*W*H*nsplit*(D+2); nw: waves per workgroup, 4 or 8, 0 = by
// the number of workgroups.
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
#define FX_WIN(TT, DD, NQQ)                                                                      \
  do {                                                                                           \
    if (wide)                                                                                    \
      window_decode_attn_kernel<TT, DD, NQQ, 8><<<g, 512, 0, st>>>(                              \
          (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, ws,                \
          (uint16_t*)out, H, W, nsplit, chunk, sqb, sqh, skb, sks, skh, sob, scale);             \
    else                                                                                         \
      window_decode_attn_kernel<TT, DD, NQQ, 4><<<g, 256, 0, st>>>(                              \
          (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, ws,                \
          (uint16_t*)out, H, W, nsplit, chunk, sqb, sqh, skb, sks, skh, sob, scale);             \
  } while (0)
#define FX_WIN_NQ(TT, DD)                                                                        \
  do {                                                                                           \
    switch (W) {                                                                                 \
      case 1: FX_WIN(TT, DD, 1); break;                                                          \
      case 2: FX_WIN(TT, DD, 2); break;                                                          \
      case 3: FX_WIN(TT, DD, 3); break;                                                          \
      case 4: FX_WIN(TT, DD, 4); break;                                                          \
      case 5:                                                                                    \
      case 6: FX_WIN(TT, DD, 6); break;                                                          \
      default: FX_WIN(TT, DD, 8); break;                                                         \
    }                                                                                            \
    if (nsplit > 1)                                                                              \
      decode_attn_combine_kernel<TT, DD><<<B * W * H, DD, 0, st>>>(ws, (uint16_t*)out, H,        \
                                                                   nsplit, sob);                 \
  } while (0)
  if (dt == 0) {
    if (D == 128) FX_WIN_NQ(bf16, 128); else FX_WIN_NQ(bf16, 64);
  } else {
    if (D == 128) FX_WIN_NQ(f16, 128); else FX_WIN_NQ(f16, 64);
  }
#undef FX_WIN_NQ
#undef FX_WIN
  return 0;
}
