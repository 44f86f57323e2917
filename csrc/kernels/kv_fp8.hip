// FP8 (OCP e4m3) KV cache for decode: the quantising append and the single-token
// split-K attention over the one-byte cache.
//
// Format: the cache is a plain e4m3 image of the 16-bit cache, uint8
// [B, maxlen, H, D], no scales.  The byte of a 16-bit value x is
// fp8(clamp(float(x), -448, 448)): round to nearest even, subnormals kept
// (torch.float8_e4m3fn).  Inputs are trusted finite, so with the clamp in front
// the NaN bytes 0x7F / 0xFF are never written.  Dequantisation to fp32 is exact
// (v_cvt_pk_f32_fp8), and every e4m3 value is exact in bf16 and fp16.
//
// kv_append_fp8_kernel serves the prefill (S rows per sample from position 0)
// and the decode step (S = 1 at pos[b]); decode_attn_fp8_kernel has the
// interface, the split-K scheme and the partial layout of
// decode_attn_split_kernel (decode_attn.hip), whose combine kernel merges its
// partials (fx_decode_attn_combine), with a lane map of its own: 16 elements
// of a key row per lane instead of 8.
//
// Built without packed fp32 VALU, as all new HIP code here (FX_NO_PK32,
// fx_common.h).  Plain vector stores, no atomics.  Resources and measurements:
// profiles/kv_fp8/README.md.
#include "fx_api.h"
#include "fx_common.h"

namespace {

typedef float kv_float2 __attribute__((ext_vector_type(2)));

// 16 e4m3 bytes -> 16 fp32, exactly: eight v_cvt_pk_f32_fp8
__device__ __forceinline__ void unpack16_fp8(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const kv_float2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const kv_float2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// 16 fp32 -> 16 e4m3 bytes: clamp to the finite range (v_med3_f32; the convert
// alone would turn 1000 into NaN), then eight v_cvt_pk_fp8_f32
__device__ __forceinline__ uint4 pack16_fp8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = __builtin_amdgcn_fmed3f(f[4 * i + j], -448.f, 448.f);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], p, true);
    w[i] = (uint32_t)p;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// Append R = B*S source rows of [H, D] 16-bit K and V (row stride ssr, head
// stride ssh, in elements: the k / v views of the packed QKV output, no copy)
// to the uint8 caches [B, maxlen, H, D] (strides scb, scs, sch in bytes).
// Source row r belongs to cache row r / S at position (pos ? pos[r / S] : 0) +
// r % S; a position at or past maxlen is dropped.  pos is read on the device,
// so a captured launch follows it.  A thread converts 16 elements of K and of
// V: two 16-byte loads and one 16-byte store each, tpr = H*D/16 threads a row.
template <typename T>
__global__ __launch_bounds__(256) FX_NO_PK32 void kv_append_fp8_kernel(
    const uint16_t* __restrict__ k_src, const uint16_t* __restrict__ v_src, long ssr, long ssh,
    int S, const int* __restrict__ pos, uint8_t* __restrict__ k_cache,
    uint8_t* __restrict__ v_cache, long scb, long scs, long sch, int maxlen, int D, int tpr,
    long nthreads) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nthreads) return;
  const long r = idx / tpr;
  const int e = (int)(idx - r * tpr) * 16;
  const int hd = e / D, d = e - hd * D;
  const long b = r / S;
  const int p = (pos ? pos[b] : 0) + (int)(r - b * S);
  if (p < 0 || p >= maxlen) return;
  const long so = r * ssr + hd * ssh + d;
  const long co = b * scb + (long)p * scs + hd * sch + d;
  float kf[16], vf[16];
  load8<T>(k_src + so, kf);
  load8<T>(k_src + so + 8, kf + 8);
  load8<T>(v_src + so, vf);
  load8<T>(v_src + so + 8, vf + 8);
  *reinterpret_cast<uint4*>(k_cache + co) = pack16_fp8(kf);
  *reinterpret_cast<uint4*>(v_cache + co) = pack16_fp8(vf);
}

// Sum over the LPK (4 or 8) consecutive lanes that share a key row, on every
// lane of the group: DPP quad permutes (xor 1, xor 2) and, at 8, the mirror
// within a half row; log2(LPK) VALU adds, no LDS round trip.
template <int LPK>
__device__ __forceinline__ float group_sum_fp8(float v) {
  static_assert(LPK == 4 || LPK == 8, "lane group of 4 or 8");
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  if (LPK == 8)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  return v;
}

// merge another online-softmax state (m2, l2, o2[16]) into (m, l, o[16])
__device__ __forceinline__ void merge_state16(float& m, float& l, float* o, float m2, float l2,
                                              const float* o2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  const float a = __expf(m - M), c = __expf(m2 - M);
  l = l * a + l2 * c;
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = o[j] * a + o2[j] * c;
  m = M;
}

// Split-K single-token attention over the e4m3 cache.  q: [B, H, D] 16-bit
// (strides sqb, sqh); caches: uint8 [B, maxlen, H, D] (skb, sks, skh in bytes);
// out: [B, H, D] 16-bit (sob, head stride D).  grid = B*H*nsplit; split s of
// (b, h) scores keys [s*chunk, min((s+1)*chunk, lens[b])) and writes one
// partial (o[D], m, l) at ws[blockIdx.x * (D + 2)], or with one split the
// normalised output.
// Lane map: LPK = D/16 lanes cover a key row, 16 bytes (16 elements) each, so
// a wave instruction covers 64/LPK rows (8 at D 128, 16 at D 64); q (scaled)
// and o are 16 fp32 a lane.  A lane group keeps U rows of K and of V in
// flight, requested together: one step of the workgroup is (64/LPK)*NW*U keys
// and one memory round trip.  Out-of-range lanes load the split's first row,
// so no row at or past lens[b] is ever read; lens[b] == 0 gives zeros.
template <typename T, int D, int NW>
__global__ __launch_bounds__(64 * NW) FX_NO_PK32 void decode_attn_fp8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc,
    const uint8_t* __restrict__ vc, const int* __restrict__ lens, float* __restrict__ ws, int H,
    int nsplit, int chunk, int maxlen, long sqb, long sqh, long skb, long sks, long skh,
    float scale, uint16_t* __restrict__ out, long sob) {
  constexpr int LPK = D / 16;       // lanes per key row
  constexpr int KPW = 64 / LPK;     // key rows per wave instruction
  constexpr int U = 4;              // key rows per lane group per step
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPK, c = (lane % LPK) * 16;
  const int len = min(lens[b], maxlen);
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  float qv[16];
  const uint16_t* qp = q + b * sqb + hd * sqh + c;
  load8<T>(qp, qv);
  load8<T>(qp + 8, qv + 8);
#pragma unroll
  for (int j = 0; j < 16; ++j) qv[j] *= scale;
  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = 0.f;
  const uint8_t* kb = kc + b * skb + hd * skh + c;
  const uint8_t* vb = vc + b * skb + hd * skh + c;
  // wave w, step: keys k0 + (u*NW + w)*KPW + sub, u < U
  for (int k0 = k_lo; k0 < k_hi; k0 += NW * KPW * U) {
    float sc[U];
    int key[U];
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
      float kv[16];
      unpack16_fp8(kraw[u], kv);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += kv[j] * qv[j];
      sc[u] = group_sum_fp8<LPK>(s);
    }
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
    for (int j = 0; j < 16; ++j) o[j] *= a;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (key[u] >= k_hi) continue;
      const float p = __expf(sc[u] - mx);
      float vv[16];
      unpack16_fp8(vraw[u], vv);
#pragma unroll
      for (int j = 0; j < 16; ++j) o[j] += p * vv[j];
      l += p;
    }
    m = mx;
  }
  // merge: the KPW lane groups of a wave share each column slice -> lane
  // shuffles; then one state per (wave, slice) through LDS, NW-way
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
    float o2[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o2[j] = __shfl_xor(o[j], off, 64);
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    merge_state16(m, l, o, m2, l2, o2);
  }
  __shared__ float sm_m[NW * LPK], sm_l[NW * LPK], sm_o[NW * LPK][16];
  if (lane < LPK) {
    sm_m[w * LPK + lane] = m;
    sm_l[w * LPK + lane] = l;
#pragma unroll
    for (int j = 0; j < 16; ++j) sm_o[w * LPK + lane][j] = o[j];
  }
  __syncthreads();
  if (threadIdx.x < LPK) {
    float M = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; ++i) M = fmaxf(M, sm_m[i * LPK + threadIdx.x]);
    float L = 0.f, O[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) O[j] = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int t = i * LPK + threadIdx.x;
        if (sm_m[t] == -INFINITY) continue;
        const float a = __expf(sm_m[t] - M);
        L += sm_l[t] * a;
#pragma unroll
        for (int j = 0; j < 16; ++j) O[j] += sm_o[t][j] * a;
      }
    }
    if (nsplit == 1) {  // one split: normalise and store the output directly
      const float inv = L > 0.f ? 1.f / L : 0.f;
      float r[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) r[j] = O[j] * inv;
      uint16_t* op = out + b * sob + hd * D + threadIdx.x * 16;
      store8<T>(op, r);
      store8<T>(op + 8, r + 8);
      return;
    }
    float* wp = ws + (long)blockIdx.x * (D + 2);
#pragma unroll
    for (int j = 0; j < 16; ++j) wp[threadIdx.x * 16 + j] = O[j];
    if (threadIdx.x == 0) {
      wp[D] = M;
      wp[D + 1] = L;
    }
  }
}

}  // namespace

// dt: 0 bf16 / 1 fp16.  k_src / v_src: R = B*S rows of [H, D] with row stride
// ssr and head stride ssh (elements); pos: int32 [B] on the device, or null
// (position 0); caches: uint8 with strides scb, scs, sch (bytes).  Nonzero for
// a call the 16-byte vectors cannot address (the caller then uses the formula).
extern "C" int fx_kv_append_fp8(int dt, const void* k_src, const void* v_src, long ssr, long ssh,
                                int B, int S, int H, int D, const int* pos, void* k_cache,
                                void* v_cache, long scb, long scs, long sch, int maxlen,
                                hipStream_t st) {
  if (dt != 0 && dt != 1) return -3;
  if (D < 16 || D % 16 || B < 1 || S < 1 || H < 1 || maxlen < 1) return -1;
  if (!al16(k_src) || !al16(v_src) || ssr % 8 || ssh % 8) return -4;
  if (!al16(k_cache) || !al16(v_cache) || scb % 16 || scs % 16 || sch % 16) return -4;
  const int tpr = H * D / 16;
  const long n = (long)B * S * tpr;
  const int g = fx_cdiv(n, 256);
#define FX_APP(TT)                                                                              \
  kv_append_fp8_kernel<TT><<<g, 256, 0, st>>>((const uint16_t*)k_src, (const uint16_t*)v_src,   \
                                              ssr, ssh, S, pos, (uint8_t*)k_cache,              \
                                              (uint8_t*)v_cache, scb, scs, sch, maxlen, D, tpr, n)
  if (dt == 0) FX_APP(bf16); else FX_APP(f16);
#undef FX_APP
  return 0;
}

// dt: 0 bf16 / 1 fp16 (q and out); caches: uint8 e4m3; ws: fp32 workspace of
// B*H*nsplit*(D+2); chunk = keys per split; nw: waves per workgroup, 4 or 16,
// 0 = by the number of workgroups (16 under 256 workgroups: the 16-bit kernel's
// rule, carried over).
extern "C" int fx_decode_attn_fp8(int dt, const void* q, const void* kc, const void* vc, void* out,
                                  const int* lens, int B, int H, int D, int maxlen, int nsplit,
                                  float* ws, long sqb, long sqh, long skb, long sks, long skh,
                                  long sob, float scale, int nw, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (nsplit < 1) return -2;
  if (dt != 0 && dt != 1) return -3;
  if (!al16(q) || sqb % 8 || sqh % 8 || !al16(out) || sob % 8) return -4;
  if (!al16(kc) || !al16(vc) || skb % 16 || sks % 16 || skh % 16) return -4;
  if (nw != 0 && nw != 4 && nw != 16) return -5;
  const int chunk = (maxlen + nsplit - 1) / nsplit;
  const int g = B * H * nsplit;
  const bool wide = nw ? nw == 16 : g < 256;
#define FX_DEC8(TT, DD)                                                                          \
  do {                                                                                           \
    if (wide)                                                                                    \
      decode_attn_fp8_kernel<TT, DD, 16><<<g, 1024, 0, st>>>(                                    \
          (const uint16_t*)q, (const uint8_t*)kc, (const uint8_t*)vc, lens, ws, H, nsplit,       \
          chunk, maxlen, sqb, sqh, skb, sks, skh, scale, (uint16_t*)out, sob);                   \
    else                                                                                         \
      decode_attn_fp8_kernel<TT, DD, 4><<<g, 256, 0, st>>>(                                      \
          (const uint16_t*)q, (const uint8_t*)kc, (const uint8_t*)vc, lens, ws, H, nsplit,       \
          chunk, maxlen, sqb, sqh, skb, sks, skh, scale, (uint16_t*)out, sob);                   \
  } while (0)
  if (dt == 0) {
    if (D == 128) FX_DEC8(bf16, 128); else FX_DEC8(bf16, 64);
  } else {
    if (D == 128) FX_DEC8(f16, 128); else FX_DEC8(f16, 64);
  }
#undef FX_DEC8
  if (nsplit > 1) fx_decode_attn_combine(dt, D, B * H, ws, out, H, nsplit, sob, st);
  return 0;
}
