// What the kernels over the quantised weight copies share: the decode GEMV
// (decode_gemv.h), the 17..64-row skinny GEMM (decode_gemm.hip), the weight-only
// prefill GEMM (prefill_gemm.hip) and the W8A8 prefill (prefill_gemm_i8.hip).
//  * the epilogue codes GV_*, the MFMA step and the conversions of a loaded
//    weight register to MFMA operands;
//  * the "16 k per lane and chunk" weight operand policies of the two GEMMs;
//  * the epilogue of 8 consecutive columns of one output row.
// Sharing these moved no code generation: profiles/skinny_shared/README.md has
// the check and what it took; read it before adding a level of inlining here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fx_common.h"

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));
typedef uint32_t uintx2 __attribute__((ext_vector_type(2)));

//   GV_BIAS      y = acc + b                               (out-proj, LM head)
//   GV_GELU      y = gelu_tanh(acc + b)                    (FFN1)
//   GV_RES       y = acc + b + res                         (FFN2 + residual)
//   GV_QKV       acc + b scattered to q[M, H, D] and the KV cache at this
//                token's position (k/v_cache[M, maxlen, H, D])   (QKV + cache append);
//                with a row map, row m goes to cache row rows[m] (several
//                consecutive tokens of one sample in one call)
enum { GV_BIAS = 0, GV_GELU = 1, GV_RES = 2, GV_QKV = 3 };

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

// MXFP4 weight operands (WMX4; OpM4 below)
// an e8m0 scale byte (the low byte of v; 1..254) -> the fp32 2^(e - 127)
__device__ __forceinline__ float mx4_scale(uint32_t v) {
  return __builtin_bit_cast(float, (v & 0xFFu) << 23);
}
// eight e2m1 (one dword: byte j = elements 2j, 2j + 1 in its low, high nibble)
// times scale -> one MFMA operand in element order: v_cvt_scalef32_pk_*_fp4,
// one instruction per byte.  Exact: a code times a power of two is a 16-bit
// float (fp16: while it is a normal one).
template <typename T>
__device__ __forceinline__ short8 mx4_cvt8(uint32_t v, float scale) {
  uint4 o;
  if constexpr (std::is_same<T, bf16>::value) {
    o.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 0));
    o.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 1));
    o.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 2));
    o.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 3));
  } else {
    o.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, 0));
    o.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, 1));
    o.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, 2));
    o.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, 3));
  }
  return __builtin_bit_cast(short8, o);
}

// ---------------------------------------------------------------------------
// Weight operand policies of the two GEMMs, 16 k per lane and chunk of 64 k:
// elt = the stored element, raw = a lane's 16 weights of one row and chunk as
// loaded, sc = the scale's element, PACK = weights per elt, ops() = the two
// MFMA A operands of a raw.  SCALED: the accumulator times scale[n] in the
// epilogue; GROUPED: scale [K / 256, N], a group of 256 k is summed from zero
// and enters the accumulator times its scale; OPSCALED: ops() takes the fp32
// scale of the lane's group of 32 k.  A kernel derives its own policy type and
// adds what it owns (decode_gemm.hip: G16 / G8 / G4 / GM4, prefill_gemm.hip:
// P8 / P4 / PM4).
// ---------------------------------------------------------------------------
struct Op16 {
  typedef uint16_t elt;
  struct raw { short8 v[2]; };
  typedef float sc;
  static constexpr int PACK = 1;
  static constexpr bool SCALED = false, GROUPED = false, OPSCALED = false;
  template <typename T>
  static __device__ __forceinline__ void ops(const raw& v, short8 (&a)[2]) {
    a[0] = v.v[0];
    a[1] = v.v[1];
  }
};

struct Op8 {
  typedef int8_t elt;
  typedef uintx4 raw;
  typedef float sc;
  static constexpr int PACK = 1;
  static constexpr bool SCALED = true, GROUPED = false, OPSCALED = false;
  template <typename T>
  static __device__ __forceinline__ void ops(const raw& v, short8 (&a)[2]) {
    a[0] = cvt8<T>(v.x, v.y);
    a[1] = cvt8<T>(v.z, v.w);
  }
};

struct Op4 {
  typedef uint8_t elt;
  typedef uintx2 raw;
  typedef float sc;
  static constexpr int PACK = 2;
  static constexpr bool SCALED = false, GROUPED = true, OPSCALED = false;
  // a dword is 8 weights: byte j = q[j] (low nibble), q[j + 4] (high nibble);
  // two masks spread them to int8 operands holding 16 q (decode_gemv_w4.hip)
  template <typename T>
  static __device__ __forceinline__ void ops(const raw& v, short8 (&a)[2]) {
    a[0] = cvt8<T>((v.x << 4) & 0xF0F0F0F0u, v.x & 0xF0F0F0F0u);
    a[1] = cvt8<T>((v.y << 4) & 0xF0F0F0F0u, v.y & 0xF0F0F0F0u);
  }
};

// MXFP4 (decode_gemv_mx4.hip): a dword is 8 weights in k order, byte j = weights
// 2j, 2j + 1; s: the fp32 scale of the lane's group
struct OpM4 {
  typedef uint8_t elt;
  typedef uintx2 raw;
  typedef uint8_t sc;
  static constexpr int PACK = 2;
  static constexpr bool SCALED = false, GROUPED = false, OPSCALED = true;
  template <typename T>
  static __device__ __forceinline__ void ops(const raw& v, float s, short8 (&a)[2]) {
    a[0] = mx4_cvt8<T>(v.x, s);
    a[1] = mx4_cvt8<T>(v.y, s);
  }
};

// one raw of a quantised policy; ST: the weights are read once -> streaming load
template <typename R, bool ST>
__device__ __forceinline__ R load_w(const void* p) {
  if constexpr (ST) return __builtin_nontemporal_load(reinterpret_cast<const R*>(p));
  else return *reinterpret_cast<const R*>(p);
}

// ---------------------------------------------------------------------------
// Epilogue of 8 consecutive columns n .. n + 7 (those < N, cnt of them) of
// output row m.  a: the kernel's argument struct (bias, res, ldres, y, ldy, N,
// epi, vec = every epilogue operand admits 16-byte accesses at n % 8 == 0).
// full = a.vec && cnt == 8: the 16-byte form, else the scalar form of the same
// code.  The operand loads and the plain store are shared with the int8
// epilogue (prefill_gemm_i8.hip), which makes its floats under its own rule.
// Macros, not functions: as functions (one more level of inlining inside the
// epilogue) they moved the code generation of every kernel that has one.
// ---------------------------------------------------------------------------
// bias and residual of the 8 columns as floats b / rs; zeros where there is none
#define EPI8_LOAD(b, rs)                                                              \
  do {                                                                                \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) b[j] = rs[j] = 0.f;                 \
    if (full) {                                                                       \
      if (a.bias != nullptr) load8<T>(a.bias + n, b);                                 \
      if (epi == GV_RES) load8<T>(a.res + (long)m * a.ldres + n, rs);                 \
    } else {                                                                          \
      for (int j = 0; j < cnt; ++j) {                                                 \
        if (a.bias != nullptr) b[j] = Elt<T>::to_f(a.bias[n + j]);                    \
        if (epi == GV_RES) rs[j] = Elt<T>::to_f(a.res[(long)m * a.ldres + n + j]);    \
      }                                                                               \
    }                                                                                 \
  } while (0)
// one rounding of v and the store to y[m, n ..]
#define EPI8_STORE(v)                                                                 \
  do {                                                                                \
    uint16_t* dst = a.y + (long)m * a.ldy + n;                                        \
    if (full) {                                                                       \
      store8<T>(dst, v);                                                              \
    } else {                                                                          \
      for (int j = 0; j < cnt; ++j) dst[j] = Elt<T>::from_f(v[j]);                    \
    }                                                                                 \
  } while (0)

// The 16-bit kernels' epilogue: v holds the summed fp32 accumulators.  Row
// scale (W::SCALED), bias, GeLU or residual, one rounding.  QKV: the kernel has
// the GV_QKV scatter and `a` the cache block of GemvArgs; without it the
// kernel carries no scatter code and no cache pointers.
template <typename W, typename T, bool QKV, typename A>
__device__ __forceinline__ void row_epilogue8(const A& a, int m, int n, float (&v)[8]) {
  const int cnt = min(8, a.N - n);
  const bool full = a.vec && cnt == 8;
  const int epi = a.epi;
  float b[8], rs[8];
  EPI8_LOAD(b, rs);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (W::SCALED) v[j] *= a.scale[min(n + j, a.N - 1)];
    if (a.bias != nullptr) v[j] += b[j];
    if (epi == GV_GELU) v[j] = gelu_tanh(v[j]);
    if (epi == GV_RES) v[j] += rs[j];
  }
  if constexpr (QKV) {
    // where column c of row m goes
    auto dst = [&](int c) -> uint16_t* {
      if (epi != GV_QKV) return a.y + (long)m * a.ldy + c;
      // packed [heads][3][head_dim] columns
      const int D = a.head_dim;
      const int h = c / (3 * D), tq = (c / D) % 3, d = c % D;
      if (tq == 0) return a.y + (long)m * a.ldy + h * D + d;
      const long cr = a.rows != nullptr ? a.rows[m] : m;
      return (tq == 1 ? a.kc : a.vc) + ((cr * a.maxlen + a.pos[m]) * a.heads + h) * D + d;
    };
    if (full) {
      store8<T>(dst(n), v);
    } else {
      for (int j = 0; j < cnt; ++j) *dst(n + j) = Elt<T>::from_f(v[j]);
    }
  } else {
    EPI8_STORE(v);
  }
}

}  // namespace
