// Vocabulary-split sampling for small-batch decode (included by sampling.hip).
//
// sample_kernel, coupled_sample_kernel and select_kernel give one row to one
// workgroup, which sweeps the 200 KB row about ten times; at batch 1 one CU of
// 256 works.  For rows with 1 <= top_k <= 64 the work is split over the row
// here, in two launches on one stream (no grid-wide sync, no global atomics,
// plain vector stores):
//
//   part kernel, grid R * G, 256 threads: workgroup (r, s) owns slice s of row
//   r, a fixed run of SLICE = 2048 vocabulary indices (G = ceil(V / 2048), the
//   bounds depend on V only).  A thread reads 8 consecutive logits once (two
//   16-byte loads for fp32, one for bf16, scalar in the tail and for processed
//   logits) and keeps them in registers.  It leaves in the slice's workspace
//   slot (SLOT dwords):
//     [0..3]  max and sum-exp of x / T, max and sum-exp of x;
//     [4]     the number of candidates;
//     [5..]   CAP x values, then CAP indices: every x >= the slice's k-th
//             largest x, in index order.
//   The k-th largest comes from a 4-pass radix select over the registers on
//   an order-preserving integer image of x (histogram of 256 bins in LDS, the
//   bin found by a block scan with one bin per thread); the candidates are
//   compacted through a block prefix count.  More than CAP candidates can
//   only come from ties at the threshold: the count is stored, no pair is.
//   A token that is no candidate of its slice has k strictly larger tokens
//   in the slice alone, so it is below the row's k-th largest.  -inf entries
//   (probability 0) are never candidates.
//
//   finish kernel, grid R, 1024 threads: merges the G statistics in slice
//   order, loads the at most G * CAP candidates into LDS, sorts them by
//   (x descending, index ascending) with a bitonic network on 64-bit keys and
//   reads the kept set off the sorted run:
//     top-k   x >= x_(k), ties kept;
//     top-p   kept iff the fp32 mass of the survivors with strictly larger x
//             is <= top_p (top_p_filter's rule, ties grouped);
//   then the pick with sample_row's / coupled_row's argument meanings: the
//   inverse-CDF draw in index order (a second, short sort by index) or the
//   Gumbel race with race_token's key, coupled_key and coupled_gumbel
//   unchanged.  The kept set is defined on x where the one-workgroup kernels
//   define it on fp32 probability bits; the two differ only where distinct
//   logits collapse to one fp32 probability.
//
//   Fallback: a row with an overflowed slice, a top_k outside 1..64 or more
//   than NSORT / CAP slices (V > 86016) runs sample_row / coupled_row in the
//   finish kernel, which is why that is 1024 threads wide; the host never
//   looks at a device flag.
//
// Probabilities are exp(fma(x, 1/T, -m)) / se with the accurate expf, one
// rounding in the exponent, so a kept p is within 1e-6 of the float64 softmax.
// Built without packed fp32 VALU.  Resources and measurements:
// profiles/sample_split/README.md.

namespace {

constexpr int PT = 256;                 // part kernel: threads
constexpr int PE = 8;                   // logits per thread
constexpr int SLICE = PT * PE;          // vocabulary indices per slice
constexpr int CAP = 96;                 // candidate slots per slice
constexpr int SLOT = 4 + 1 + 2 * CAP;   // workspace dwords per slice
constexpr int MAXK = 64;                // largest top_k of the split path
constexpr int NSORT = 4096;             // sort capacity of the finish kernel
constexpr int MAXG = NSORT / CAP;       // most slices whose candidates fit
static_assert(PT == 256, "one histogram bin per thread");

// fp32 -> uint32 with the same order (-0 is normalised away before)
__device__ __forceinline__ unsigned int order_key(float x) {
  const unsigned int b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float order_val(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k);
}

// ---- logit loaders: raw rows (vector loads) or ProcLoad (scalar, as it is)
template <typename T>
struct RawLoad {
  const T* lg;
  __device__ __forceinline__ float operator()(int i) const { return ld<T>(lg, i); }
};

// x[j] = load(i0 + j), -inf past the row's end
template <typename L>
__device__ __forceinline__ void load_run(const L& load, int i0, int V, float* x) {
#pragma unroll
  for (int j = 0; j < PE; ++j) x[j] = i0 + j < V ? load(i0 + j) : -INFINITY;
}
__device__ __forceinline__ void load_run(const RawLoad<float>& load, int i0, int V, float* x) {
  const float* p = load.lg + i0;
  if (i0 + PE <= V && ((uintptr_t)p & 15) == 0) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
    x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < PE; ++j) x[j] = i0 + j < V ? p[j] : -INFINITY;
  }
}
__device__ __forceinline__ void load_run(const RawLoad<uint16_t>& load, int i0, int V,
                                         float* x) {
  const uint16_t* p = load.lg + i0;
  if (i0 + PE <= V && ((uintptr_t)p & 15) == 0) {
    unpack8<bf16>(*reinterpret_cast<const uint4*>(p), x);
  } else {
#pragma unroll
    for (int j = 0; j < PE; ++j) x[j] = i0 + j < V ? bf16_bits_to_float(p[j]) : -INFINITY;
  }
}

// ------------------------------------------------------------- part kernel
struct PartShared {
  float red[4][PT / 64];
  unsigned int hist[256];
  unsigned int wtot[PT / 64];
  unsigned int sel_bin, sel_need;
};

// inclusive prefix sum of `v` over the 256 threads, and the total
__device__ __forceinline__ unsigned int part_scan(unsigned int v, PartShared& q,
                                                  unsigned int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();
  if (lane == 63) q.wtot[w] = incl;
  __syncthreads();
  unsigned int before = 0u;
  total = 0u;
#pragma unroll
  for (int i = 0; i < PT / 64; ++i) {
    const unsigned int t = q.wtot[i];
    if (i < w) before += t;
    total += t;
  }
  return incl + before;
}

template <typename L>
__device__ __forceinline__ void split_part(const L& load, int V, int slice, float inv_temp,
                                           int top_k, float* __restrict__ slot, PartShared& q) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i0 = slice * SLICE + tid * PE;
  float x[PE];
  load_run(load, i0, V, x);
  // (a) statistics
  float mt = -INFINITY, mr = -INFINITY;
#pragma unroll
  for (int j = 0; j < PE; ++j) {
    x[j] += 0.f;  // -0 -> +0: equal logits, one integer image
    mt = fmaxf(mt, x[j] * inv_temp);
    mr = fmaxf(mr, x[j]);
  }
  mt = wave_max(mt);
  mr = wave_max(mr);
  if (lane == 0) q.red[0][w] = mt, q.red[1][w] = mr;
  __syncthreads();
  mt = q.red[0][0], mr = q.red[1][0];
#pragma unroll
  for (int i = 1; i < PT / 64; ++i) mt = fmaxf(mt, q.red[0][i]), mr = fmaxf(mr, q.red[1][i]);
  float st = 0.f, sr = 0.f;
  if (mr > -INFINITY) {  // else the slice is all -inf (or past the row): sums 0
#pragma unroll
    for (int j = 0; j < PE; ++j) {
      st += expf(__fmaf_rn(x[j], inv_temp, -mt));
      sr += expf(x[j] - mr);
    }
  }
  st = wave_sum(st);
  sr = wave_sum(sr);
  if (lane == 0) q.red[2][w] = st, q.red[3][w] = sr;
  __syncthreads();
  if (tid == 0) {
    st = sr = 0.f;
#pragma unroll
    for (int i = 0; i < PT / 64; ++i) st += q.red[2][i], sr += q.red[3][i];
    slot[0] = mt, slot[1] = st, slot[2] = mr, slot[3] = sr;
  }
  int* islot = reinterpret_cast<int*>(slot);
  if (top_k < 1 || top_k > MAXK) {  // the finish kernel takes the fallback
    if (tid == 0) islot[4] = 0;
    return;
  }
  // (b) the slice's k-th largest key: radix select over the registers
  unsigned int key[PE];
#pragma unroll
  for (int j = 0; j < PE; ++j) key[j] = order_key(x[j]);
  unsigned int prefix = 0u, need = (unsigned)top_k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    q.hist[tid] = 0u;
    __syncthreads();
    const unsigned int hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
#pragma unroll
    for (int j = 0; j < PE; ++j)
      if ((key[j] & hmask) == prefix) atomicAdd(&q.hist[(key[j] >> shift) & 0xffu], 1u);
    __syncthreads();
    // thread t holds bin 255 - t: the scan counts the keys in higher bins
    const unsigned int h = q.hist[255 - tid];
    unsigned int total;
    const unsigned int incl = part_scan(h, q, total);
    if (incl - h < need && need <= incl) {  // one thread: SLICE keys >= need
      q.sel_bin = 255u - tid;
      q.sel_need = need - (incl - h);
    }
    __syncthreads();
    prefix |= q.sel_bin << shift;
    need = q.sel_need;
  }
  // candidates: key >= the k-th largest, -inf never
  const unsigned int ninf = order_key(-INFINITY);
  unsigned int c = 0u;
#pragma unroll
  for (int j = 0; j < PE; ++j) c += (key[j] >= prefix && key[j] > ninf) ? 1u : 0u;
  unsigned int total;
  unsigned int pos = part_scan(c, q, total) - c;
  if (total <= (unsigned)CAP) {
#pragma unroll
    for (int j = 0; j < PE; ++j) {
      if (key[j] >= prefix && key[j] > ninf) {
        slot[5 + pos] = x[j];
        islot[5 + CAP + pos] = i0 + j;
        ++pos;
      }
    }
  }
  if (tid == 0) islot[4] = (int)total;
}

template <typename T>
__global__ __launch_bounds__(PT) FX_NO_PK32 void sample_part_kernel(
    const T* __restrict__ logits, long ld_row, int V, int G, float inv_temp, int top_k,
    float* __restrict__ ws) {
  __shared__ PartShared q;
  const int row = blockIdx.x / G, slice = blockIdx.x - row * G;
  RawLoad<T> load{logits + row * ld_row};
  split_part(load, V, slice, inv_temp, top_k, ws + (long)blockIdx.x * SLOT, q);
}

// select_kernel's processed-logit loader for row `row` at step `step`
__device__ __forceinline__ ProcLoad select_load(const SelectArgs& a, int row, int step) {
  ProcLoad load;
  load.lg = a.logits + row * a.ld_row;
  load.seen = a.seen + (long)row * a.words;
  load.mask_eos = (a.eos >= 0 && step < a.min_len) ? a.eos : -1;
  load.force = (a.feos >= 0 && step == a.feos_step) ? a.feos
               : (a.bos >= 0 && step == 0)          ? a.bos
                                                    : -1;
  load.use_pen = a.use_pen;
  load.pen = a.pen;
  load.inv_pen = a.inv_pen;
  return load;
}

__global__ __launch_bounds__(PT) FX_NO_PK32 void select_part_kernel(SelectArgs a, int G,
                                                                    float* __restrict__ ws) {
  __shared__ PartShared q;
  const int row = blockIdx.x / G, slice = blockIdx.x - row * G;
  const int step = a.step[row];
  if (step >= a.n_steps || !a.unfinished[row]) return;  // the finish kernel picks nothing
  const ProcLoad load = select_load(a, row, step);
  split_part(load, a.V, slice, a.inv_temp, a.top_k, ws + (long)blockIdx.x * SLOT, q);
}

// ----------------------------------------------------------- finish kernel
struct FinishShared {
  unsigned long long key[NSORT];  // (~order_key(x), index), later (index, p bits)
  float p[NSORT];                 // p of the sorted run, later its running sum in index order
  float sm[MAXG], sse[MAXG], rm[MAXG], rse[MAXG];
  int cnt[MAXG], off[MAXG];
  float m, mraw, inv_se, lse;
  int n, nk, np;
};

// ascending bitonic sort of key[0 .. n), n a power of two
__device__ __forceinline__ void bitonic_sort(unsigned long long* key, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += ST) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long a = key[i], b = key[l];
        if ((a > b) == ((i & k) == 0)) key[i] = b, key[l] = a;
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ float wave_scan_sum(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// The pick of one row from its G workspace slots; every thread returns it (0
// when nothing survives), `lse` is the logsumexp of load(i).  `coupled`: the
// race of token index `t`, row `b` under `seed`; else the draw with `u`.
template <typename L>
__device__ __forceinline__ int split_finish(const L& load, const float* __restrict__ ws, int G,
                                            int V, float inv_temp, int top_k, float top_p,
                                            bool coupled, float u, uint64_t seed, int t, int b,
                                            float* __restrict__ probs_row, Shared& s,
                                            FinishShared& q, float& lse) {
  const int tid = threadIdx.x;
  const bool fast = top_k >= 1 && top_k <= MAXK && G <= MAXG;
  int over = 0;
  if (fast && tid < G) {
    const float* sl = ws + (long)tid * SLOT;
    q.sm[tid] = sl[0], q.sse[tid] = sl[1], q.rm[tid] = sl[2], q.rse[tid] = sl[3];
    const int c = reinterpret_cast<const int*>(sl)[4];
    q.cnt[tid] = c;
    over = c > CAP;
  }
  if (!fast || __syncthreads_or(over)) {
    if (coupled) return coupled_row(load, V, inv_temp, top_k, top_p, seed, t, b, s, lse);
    return sample_row(load, V, inv_temp, top_k, top_p, u, probs_row, s, lse);
  }
  if (probs_row)
    for (int i = tid; i < V; i += ST) probs_row[i] = 0.f;
  // ---- the G statistics: rescaled in parallel, summed in slice order
  if (tid < 64) {
    const bool in = tid < G;
    const float a = in ? q.sm[tid] : -INFINITY, r = in ? q.rm[tid] : -INFINITY;
    const float M = wave_max(a), R = wave_max(r);
    if (in) {
      q.sse[tid] = a > -INFINITY ? q.sse[tid] * expf(a - M) : 0.f;
      q.rse[tid] = r > -INFINITY ? q.rse[tid] * expf(r - R) : 0.f;
    }
    if (tid == 0) q.m = M, q.mraw = R;
  }
  __syncthreads();
  if (tid == 0) {
    float se = 0.f, sr = 0.f;
    int n = 0;
    for (int g = 0; g < G; ++g) {
      se += q.sse[g];
      sr += q.rse[g];
      q.off[g] = n;
      n += q.cnt[g];
    }
    q.inv_se = 1.f / se;
    q.lse = q.mraw + __logf(sr);
    q.n = n;
  }
  __syncthreads();
  lse = q.lse;
  const int n = q.n;  // <= G * CAP <= NSORT
  if (n == 0) return 0;
  // ---- candidates into LDS, sorted by (x descending, index ascending)
  int npad = 64;
  while (npad < n) npad <<= 1;
  for (int e = tid; e < G * CAP; e += ST) {
    const int g = e / CAP, j = e - g * CAP;
    if (j < q.cnt[g]) {
      const float* base = ws + (long)g * SLOT + 5;
      const unsigned int idx = reinterpret_cast<const unsigned int*>(base)[CAP + j];
      q.key[q.off[g] + j] = ((unsigned long long)~order_key(base[j]) << 32) | idx;
    }
  }
  for (int e = n + tid; e < npad; e += ST) q.key[e] = ~0ull;
  __syncthreads();
  bitonic_sort(q.key, npad);
  // ---- top-k: the run x >= x_(k)
  const unsigned int hk = (unsigned int)(q.key[min(top_k, n) - 1] >> 32);
  for (int j = tid; j < n; j += ST)
    if ((unsigned int)(q.key[j] >> 32) <= hk &&
        (j + 1 == n || (unsigned int)(q.key[j + 1] >> 32) > hk))
      q.nk = j + 1;
  __syncthreads();
  const int nk = q.nk;
  const float m = q.m, inv_se = q.inv_se;
  for (int j = tid; j < nk; j += ST) {
    const float x = order_val(~(unsigned int)(q.key[j] >> 32));
    q.p[j] = expf(__fmaf_rn(x, inv_temp, -m)) * inv_se;
  }
  if (tid == 0) q.np = nk;
  __syncthreads();
  // ---- top-p: kept iff the mass of the strictly larger x is <= top_p (wave 0)
  if (top_p < 1.f && tid < 64) {
    float carry = 0.f, cstart = -1.f;
    int np = 0;
    for (int base = 0; base < nk; base += 64) {
      const int j = base + tid;
      const bool in = j < nk;
      const float incl = wave_scan_sum(in ? q.p[j] : 0.f, tid);
      const float prev = __shfl_up(incl, 1, 64);
      const float excl = carry + (tid ? prev : 0.f);
      const bool start =
          in && (j == 0 || (unsigned int)(q.key[j - 1] >> 32) != (unsigned int)(q.key[j] >> 32));
      // the mass above an element is the one above the first of its equals
      float v = start ? excl : -1.f;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float w = __shfl_up(v, o, 64);
        if (tid >= o) v = fmaxf(v, w);
      }
      v = fmaxf(v, cstart);
      np += __popcll(__ballot(in && v <= top_p));
      carry += __shfl(incl, 63, 64);
      cstart = __shfl(v, 63, 64);
    }
    if (tid == 0) q.np = np;
  }
  __syncthreads();
  const int np = q.np;  // >= 1: nothing is above the first
  if (probs_row)
    for (int j = tid; j < np; j += ST) probs_row[(unsigned int)q.key[j]] = q.p[j];
  if (coupled) {
    // race_token over the kept run
    const uint64_t key = coupled_key(seed, t, b);
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
    float best = -INFINITY;
    int first = V;
    for (int j = tid; j < np; j += ST) {
      const int i = (int)(unsigned int)q.key[j];
      const float x = order_val(~(unsigned int)(q.key[j] >> 32));
      const float k = __fmaf_rn(x, inv_temp, coupled_gumbel(klo, khi, i));
      if (k > best || (k == best && i < first)) best = k, first = i;
    }
    const float mx = block_max(best, s);
    if (tid == 0) s.pick = V;
    __syncthreads();
    if (first < V && best == mx) atomicMin(&s.pick, first);
    __syncthreads();
    return s.pick < V ? s.pick : 0;
  }
  // ---- the draw: the kept run in index order, its running mass, u * total
  int np2 = 64;
  while (np2 < np) np2 <<= 1;
  for (int j = tid; j < np2; j += ST)  // entry j is read and written by its own thread
    q.key[j] = j < np ? ((q.key[j] & 0xffffffffull) << 32) | __float_as_uint(q.p[j]) : ~0ull;
  __syncthreads();
  bitonic_sort(q.key, np2);
  if (tid < 64) {
    float carry = 0.f;
    for (int base = 0; base < np; base += 64) {
      const int j = base + tid;
      const float incl = wave_scan_sum(j < np ? __uint_as_float((unsigned int)q.key[j]) : 0.f, tid);
      if (j < np) q.p[j] = carry + incl;
      carry += __shfl(incl, 63, 64);
    }
    const float target = u * carry;
    int r = 0;  // the first entry whose running mass passes the target
    for (int base = 0; base < np; base += 64) {
      const int j = base + tid;
      r += __popcll(__ballot(j < np && q.p[j] <= target));
    }
    if (tid == 0) s.pick = (int)(q.key[min(r, np - 1)] >> 32);  // rounding: past the end
  }
  __syncthreads();
  return s.pick;
}

template <typename T>
__global__ __launch_bounds__(ST) FX_NO_PK32 void sample_finish_kernel(
    const T* __restrict__ logits, long ld_row, int V, int G, float inv_temp, int top_k,
    float top_p, const float* __restrict__ uniforms, const float* __restrict__ ws,
    int64_t* __restrict__ out_ids, float* __restrict__ out_lse, float* __restrict__ out_probs) {
  __shared__ Shared s;
  __shared__ FinishShared q;
  const long row = blockIdx.x;
  RawLoad<T> load{logits + row * ld_row};
  float lse;
  const int pick = split_finish(load, ws + row * G * SLOT, G, V, inv_temp, top_k, top_p, false,
                                uniforms[row], 0, 0, 0,
                                out_probs ? out_probs + row * (long)V : nullptr, s, q, lse);
  if (threadIdx.x == 0) {
    if (out_lse) out_lse[row] = lse;
    out_ids[row] = pick;
  }
}

__global__ __launch_bounds__(ST) FX_NO_PK32 void coupled_finish_kernel(
    const float* __restrict__ logits, long ld_row, int V, int G, float inv_temp, int top_k,
    float top_p, const int* __restrict__ steps, const int* __restrict__ rows,
    const int64_t* __restrict__ seed, const float* __restrict__ ws,
    int64_t* __restrict__ out_ids, float* __restrict__ out_lse) {
  __shared__ Shared s;
  __shared__ FinishShared q;
  const long row = blockIdx.x;
  RawLoad<float> load{logits + row * ld_row};
  float lse;
  const int pick = split_finish(load, ws + row * G * SLOT, G, V, inv_temp, top_k, top_p, true,
                                0.f, (uint64_t)seed[0], steps[row], rows ? rows[row] : (int)row,
                                nullptr, s, q, lse);
  if (threadIdx.x == 0) {
    if (out_lse) out_lse[row] = lse;
    out_ids[row] = pick;
  }
}

// select_kernel in sampling modes 1 and 2 with the pick from the workspace
__global__ __launch_bounds__(ST) FX_NO_PK32 void select_finish_kernel(
    SelectArgs a, int G, const float* __restrict__ ws) {
  __shared__ Shared s;
  __shared__ FinishShared q;
  const int row = blockIdx.x;
  const int step = a.step[row];
  if (step >= a.n_steps) return;  // out / u hold n_steps columns
  const int unf = a.unfinished[row];
  const ProcLoad load = select_load(a, row, step);
  int pick = 0;
  float lse = 0.f;
  if (unf)  // a finished row emits pad: nothing to pick
    pick = split_finish(load, ws + (long)row * G * SLOT, G, a.V, a.inv_temp, a.top_k, a.top_p,
                        a.sampling == 2, a.sampling == 2 ? 0.f : a.u[(long)step * a.B + row],
                        a.sampling == 2 ? (uint64_t)a.seed[0] : 0, step, row, nullptr, s, q, lse);
  if (threadIdx.x == 0)
    select_bookkeep(a, load, a.seen + (long)row * a.words, row, step, unf, pick, lse);
}

// the part launch is skipped where every row takes the fallback
inline bool split_serves(int V, int top_k) {
  return top_k >= 1 && top_k <= MAXK && fx_cdiv(V, SLICE) <= MAXG;
}

}  // namespace

extern "C" long fx_sample_split_ws(int R, int V) {
  return (long)R * fx_cdiv(V, SLICE) * SLOT;
}

extern "C" int fx_sample_split(int dtype, const void* logits, long ld_row, int B, int V,
                               float inv_temp, int top_k, float top_p, const float* uniforms,
                               int64_t* out_ids, float* out_lse, float* out_probs, float* ws,
                               hipStream_t st) {
  if (B <= 0 || V <= 0) return 0;
  if (!ws || (dtype != 2 && dtype != 0)) return -1;
  const int G = fx_cdiv(V, SLICE);
  if (dtype == 2) {
    const float* lg = (const float*)logits;
    if (split_serves(V, top_k))
      sample_part_kernel<float><<<B * G, PT, 0, st>>>(lg, ld_row, V, G, inv_temp, top_k, ws);
    sample_finish_kernel<float><<<B, ST, 0, st>>>(lg, ld_row, V, G, inv_temp, top_k, top_p,
                                                  uniforms, ws, out_ids, out_lse, out_probs);
  } else {
    const uint16_t* lg = (const uint16_t*)logits;
    if (split_serves(V, top_k))
      sample_part_kernel<uint16_t><<<B * G, PT, 0, st>>>(lg, ld_row, V, G, inv_temp, top_k, ws);
    sample_finish_kernel<uint16_t><<<B, ST, 0, st>>>(lg, ld_row, V, G, inv_temp, top_k, top_p,
                                                     uniforms, ws, out_ids, out_lse, out_probs);
  }
  return 0;
}

extern "C" int fx_coupled_sample_split(const float* logits, long ld_row, int R, int V,
                                       float inv_temp, int top_k, float top_p, const int* steps,
                                       const int* rows, const int64_t* seed, int64_t* out_ids,
                                       float* out_lse, float* ws, hipStream_t st) {
  if (R <= 0 || V <= 0) return 0;
  if (!logits || !steps || !seed || !out_ids || !ws) return -1;
  const int G = fx_cdiv(V, SLICE);
  if (split_serves(V, top_k))
    sample_part_kernel<float><<<R * G, PT, 0, st>>>(logits, ld_row, V, G, inv_temp, top_k, ws);
  coupled_finish_kernel<<<R, ST, 0, st>>>(logits, ld_row, V, G, inv_temp, top_k, top_p, steps,
                                          rows, seed, ws, out_ids, out_lse);
  return 0;
}

// fx_select with the sampling pick split over the vocabulary; the greedy pick
// has no split form and runs select_kernel
extern "C" int fx_select_split(const float* logits, long ld_row, int B, int V, int sampling,
                               float inv_temp, int top_k, float top_p, const float* u,
                               int n_steps, int eos, int pad, int min_len, float pen,
                               float inv_pen, int bos, int feos, int feos_step,
                               unsigned int* seen, int words, int* step, int* unfinished,
                               int* finish_len, float* scores, int64_t* out, int64_t* nxt,
                               int64_t* cur, const int64_t* lens, hipStream_t st,
                               const int64_t* seed, float* ws) {
  if (sampling == 0)
    return fx_select(logits, ld_row, B, V, sampling, inv_temp, top_k, top_p, u, n_steps, eos, pad,
                     min_len, pen, inv_pen, bos, feos, feos_step, seen, words, step, unfinished,
                     finish_len, scores, out, nxt, cur, lens, st, seed);
  if (B <= 0 || V <= 0 || n_steps <= 0) return 0;
  if (sampling < 0 || sampling > 2 || !ws) return -1;
  if (words < (V + 31) / 32 || (sampling == 1 && !u) || (sampling == 2 && !seed)) return -1;
  if (pad < 0 || pad >= V || eos >= V || bos >= V || feos >= V) return -2;
  SelectArgs a;
  a.logits = logits, a.ld_row = ld_row, a.V = V, a.B = B;
  a.sampling = sampling, a.inv_temp = inv_temp, a.top_k = top_k, a.top_p = top_p;
  a.u = u, a.n_steps = n_steps;
  a.eos = eos, a.pad = pad, a.min_len = min_len;
  a.use_pen = pen != 1.f, a.pen = pen, a.inv_pen = inv_pen;
  a.bos = bos, a.feos = feos, a.feos_step = feos_step;
  a.seen = seen, a.words = words, a.step = step, a.unfinished = unfinished;
  a.finish_len = finish_len, a.scores = scores, a.out = out, a.nxt = nxt, a.cur = cur;
  a.lens = lens, a.seed = seed;
  const int G = fx_cdiv(V, SLICE);
  if (split_serves(V, top_k)) select_part_kernel<<<B * G, PT, 0, st>>>(a, G, ws);
  select_finish_kernel<<<B, ST, 0, st>>>(a, G, ws);
  return 0;
}
