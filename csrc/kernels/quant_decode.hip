// QAT fake-quant (abs-max, symmetric int-N).
//
// Parity: reference K23 (paddleslim QAT: abs_max weights / moving-average
// abs_max activations, 8 bit; `pretrain_gpt_345M_mp8_qat.yaml:35-44`).
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
