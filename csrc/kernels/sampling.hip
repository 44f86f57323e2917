// Fused top-k / top-p (nucleus) sampling over the vocabulary (K18).
//
// The reference samples with a chain of framework ops per decode step
// (softmax, topk, sort + cumsum + scatter for top-p, multinomial,
// log_softmax + gather for the score: single_model.py:907-988).  Here one
// workgroup of 1024 threads (16 wave64s) owns one batch row and does all of
// it in a single launch, never sorting:
//
//   1. row max / sum-exp of logits/T (softmax denominators) and the
//      logsumexp of the raw logits (for the token's log-prob score);
//   2. top-k threshold by 4-pass radix select (8 bits per pass) on the fp32
//      probability bits (non-negative floats order like their bit patterns);
//      histogram in LDS, keep p >= p_(k)  (ties kept, as topk + ">=" does);
//   3. top-p threshold by the same radix walk over probability MASS: the
//      largest T with mass(p >= T) > top_p, computed on the top-k survivors
//      without renormalising -- exactly the keep rule of
//      models/language_model/gpt/generation.py:top_p_filter (keep a token iff
//      the mass ranked strictly above it is <= top_p);
//   4. inverse-CDF draw in index order with the row's uniform u: per-thread
//      contiguous chunks, block exclusive scan of chunk masses, the owning
//      thread walks its chunk.
//
// The coupled sampler (coupled_row) replaces phase 4 by a Gumbel race over the
// same kept set: argmax_i (x_i / T + g_i) with noise g that depends only on
// (seed, token index t, row b, vocabulary index i).  Whoever picks token t of
// row b -- a draft step, a window slot, the plain loop -- draws with the same
// noise, so speculative decoding under sampling accepts a draft iff it equals
// the target's pick, as the greedy loop does.
//
// Every pass re-reads the row from global memory (a 50k-entry fp32 row is
// 200 KB: L2-resident, larger than LDS); decode batches are small, so the
// kernel is latency- not bandwidth-bound and one launch replaces ~15.
#include "fx_api.h"
#include "fx_common.h"

namespace {

constexpr int ST = 1024;          // threads per row
constexpr int SW = ST / 64;       // waves

struct Shared {
  float red[SW];
  float red2[SW];
  unsigned int hist[256];
  float mass[256];
  float scan[ST];
  unsigned int sel_prefix;
  float sel_above;
  unsigned int sel_k;
  int pick;
};

template <typename T>
__device__ __forceinline__ float ld(const T* p, long i);
template <>
__device__ __forceinline__ float ld<float>(const float* p, long i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<uint16_t>(const uint16_t* p, long i) {
  return bf16_bits_to_float(p[i]);
}

__device__ __forceinline__ float block_max(float v, Shared& s) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s.red[w] = v;
  __syncthreads();
  float r = s.red[0];
#pragma unroll
  for (int i = 1; i < SW; ++i) r = fmaxf(r, s.red[i]);
  return r;
}
__device__ __forceinline__ float block_sum(float v, Shared& s) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s.red2[w] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < SW; ++i) r += s.red2[i];
  return r;
}

// ---- the four phases, over a logit loader `load(i)` (raw logits in
// sample_kernel, processed logits in select_kernel: one text for both)

// 1. softmax denominators of load(i)/T (max `m`, 1/sum-exp `inv_se`) and the
//    logsumexp of load(i) itself
template <typename L>
__device__ __forceinline__ void softmax_stats(const L& load, int V, float inv_temp, Shared& s,
                                              float& m_out, float& inv_se, float& lse) {
  const int tid = threadIdx.x;
  float m = -INFINITY, mraw = -INFINITY;
  for (int i = tid; i < V; i += ST) {
    const float x = load(i);
    m = fmaxf(m, x * inv_temp);
    mraw = fmaxf(mraw, x);
  }
  m = block_max(m, s);
  const float mr = block_max(mraw, s);
  float se = 0.f, ser = 0.f;
  for (int i = tid; i < V; i += ST) {
    const float x = load(i);
    se += __expf(x * inv_temp - m);
    ser += __expf(x - mr);
  }
  se = block_sum(se, s);
  ser = block_sum(ser, s);
  m_out = m;
  inv_se = 1.f / se;
  lse = mr + __logf(ser);
}

// 2. top-k threshold (radix select on the probability bits): keep p_bits >= kth
template <typename P>
__device__ __forceinline__ unsigned int topk_threshold(const P& prob, int V, int top_k,
                                                       Shared& s) {
  const int tid = threadIdx.x;
  unsigned int kth = 0u;
  if (top_k > 0 && top_k < V) {
    if (tid == 0) {
      s.sel_prefix = 0u;
      s.sel_k = (unsigned)top_k;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
      __syncthreads();
      for (int b = tid; b < 256; b += ST) s.hist[b] = 0u;
      __syncthreads();
      const unsigned int prefix = s.sel_prefix;
      const unsigned int hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
      for (int i = tid; i < V; i += ST) {
        const unsigned int key = __float_as_uint(prob(i));
        if ((key & hmask) == (prefix & hmask)) atomicAdd(&s.hist[(key >> shift) & 0xffu], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned int need = s.sel_k, cum = 0u;
        int b = 255;
        for (; b > 0; --b) {
          if (cum + s.hist[b] >= need) break;
          cum += s.hist[b];
        }
        s.sel_k = need - cum;
        s.sel_prefix = prefix | ((unsigned)b << shift);
      }
    }
    __syncthreads();
    kth = s.sel_prefix;
  }
  return kth;
}

// 3. top-p threshold over the top-k survivors' mass
template <typename P>
__device__ __forceinline__ unsigned int topp_threshold(const P& prob, int V, float top_p,
                                                       unsigned int kth, Shared& s) {
  const int tid = threadIdx.x;
  unsigned int pth = 0u;
  if (top_p < 1.f) {
    if (tid == 0) {
      s.sel_prefix = 0u;
      s.sel_above = 0.f;
      s.sel_k = 0u;  // 0: searching, 1: keep all, 2: stop at the current prefix
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
      __syncthreads();
      for (int b = tid; b < 256; b += ST) s.mass[b] = 0.f;
      __syncthreads();
      const unsigned int prefix = s.sel_prefix;
      const unsigned int hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
      for (int i = tid; i < V; i += ST) {
        const float p = prob(i);
        const unsigned int key = __float_as_uint(p);
        if (key >= kth && (key & hmask) == (prefix & hmask))
          atomicAdd(&s.mass[(key >> shift) & 0xffu], p);
      }
      __syncthreads();
      if (tid == 0) {
        float above = s.sel_above;
        int b = 255;
        bool found = false;
        for (; b >= 0; --b) {
          if (above + s.mass[b] > top_p) {
            found = true;
            break;
          }
          above += s.mass[b];
        }
        if (!found) {
          // total mass <= top_p: nothing is cut (first level), or float
          // rounding between levels -- keep the bin selected so far
          s.sel_k = shift == 24 ? 1u : 2u;
        } else {
          s.sel_above = above;
          s.sel_prefix = prefix | ((unsigned)b << shift);
        }
      }
      __syncthreads();
      if (s.sel_k != 0u) break;
    }
    __syncthreads();
    pth = s.sel_k == 1u ? 0u : s.sel_prefix;
  }
  return pth;
}

// 4. inverse-CDF draw in index order with the uniform `u`; every thread
//    returns the pick (0 when nothing survives)
template <typename P>
__device__ __forceinline__ int draw_token(const P& prob, int V, unsigned int thr, float u,
                                          float* __restrict__ probs_row, Shared& s) {
  const int tid = threadIdx.x;
  const int chunk = (V + ST - 1) / ST;
  const int lo = min(V, tid * chunk), hi = min(V, lo + chunk);
  float part = 0.f;
  int last = -1;
  for (int i = lo; i < hi; ++i) {
    const float p = prob(i);
    const bool keep = __float_as_uint(p) >= thr;
    if (keep) {
      part += p;
      last = i;
    }
    if (probs_row) probs_row[i] = keep ? p : 0.f;
  }
  s.scan[tid] = part;
  if (tid == 0) s.pick = -1;
  __syncthreads();
  // Hillis-Steele inclusive scan over 1024 chunk masses
  for (int off = 1; off < ST; off <<= 1) {
    const float v = tid >= off ? s.scan[tid - off] : 0.f;
    __syncthreads();
    s.scan[tid] += v;
    __syncthreads();
  }
  const float total = s.scan[ST - 1];
  const float target = u * total;
  const float excl = s.scan[tid] - part;
  if (part > 0.f && target >= excl && target < excl + part) {
    float c = excl;
    int pick = last;
    for (int i = lo; i < hi; ++i) {
      const float p = prob(i);
      if (__float_as_uint(p) < thr) continue;
      c += p;
      if (target < c) {
        pick = i;
        break;
      }
    }
    atomicMax(&s.pick, pick);
  }
  __syncthreads();
  if (s.pick < 0 && last >= 0) atomicMax(&s.pick, last);  // rounding: u*total past the end
  __syncthreads();
  return s.pick < 0 ? 0 : s.pick;
}

// ---- the coupled pick: shared Gumbel noise instead of a uniform
// The key of token index `t` in row `b`; must match parallel/rng.py:coupled_key.
__device__ __forceinline__ uint64_t coupled_key(uint64_t seed, int t, int b) {
  const uint64_t tb = ((uint64_t)(uint32_t)t << 32) | (uint32_t)b;
  return fx_mix64(fx_mix64(seed + 0x9E3779B97F4A7C15ull) ^ tb);
}
// g_i = -log(-log(U)), U = ((h >> 9) + 0.5) * 2^-23 in (0, 1): 23 bits are exact
// in fp32 (24 would round the top value to 1 and g to +inf).  The accurate
// logf: E = -log(U) reaches 6e-8, where an absolute error is a large relative one.
__device__ __forceinline__ float coupled_gumbel(uint32_t klo, uint32_t khi, int i) {
  const uint32_t h = lowbias32(lowbias32((uint32_t)i ^ klo) ^ khi);
  const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

// 4'. Gumbel race over the kept set: the index of the largest
//     key_i = fma(load(i), inv_temp, g_i), the lowest index among equal keys;
//     every thread returns the pick (0 when nothing survives)
template <typename L, typename P>
__device__ __forceinline__ int race_token(const L& load, const P& prob, int V, unsigned int thr,
                                          float inv_temp, uint64_t key, Shared& s) {
  const int tid = threadIdx.x;
  const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
  float best = -INFINITY;
  int first = V;
  for (int i = tid; i < V; i += ST) {
    if (thr != 0u && __float_as_uint(prob(i)) < thr) continue;
    const float k = __fmaf_rn(load(i), inv_temp, coupled_gumbel(klo, khi, i));
    if (k > best) {  // ascending i: the lowest index of the thread's maximum
      best = k;
      first = i;
    }
  }
  const float m = block_max(best, s);
  if (tid == 0) s.pick = V;
  __syncthreads();
  if (first < V && best == m) atomicMin(&s.pick, first);
  __syncthreads();
  return s.pick < V ? s.pick : 0;
}

// phases 1-3 and the race on load(i) for token index `t` of row `b`; returns
// the pick, `lse` is the logsumexp of load(i).  The kept set is sample_row's.
template <typename L>
__device__ __forceinline__ int coupled_row(const L& load, int V, float inv_temp, int top_k,
                                           float top_p, uint64_t seed, int t, int b, Shared& s,
                                           float& lse) {
  float m, inv_se;
  softmax_stats(load, V, inv_temp, s, m, inv_se, lse);
  auto prob = [&](int i) { return __expf(load(i) * inv_temp - m) * inv_se; };
  const unsigned int kth = topk_threshold(prob, V, top_k, s);
  const unsigned int pth = topp_threshold(prob, V, top_p, kth, s);
  return race_token(load, prob, V, kth > pth ? kth : pth, inv_temp, coupled_key(seed, t, b), s);
}

// phases 1-4 on load(i); returns the pick, `lse` is the logsumexp of load(i)
template <typename L>
__device__ __forceinline__ int sample_row(const L& load, int V, float inv_temp, int top_k,
                                          float top_p, float u, float* __restrict__ probs_row,
                                          Shared& s, float& lse) {
  float m, inv_se;
  softmax_stats(load, V, inv_temp, s, m, inv_se, lse);
  auto prob = [&](int i) { return __expf(load(i) * inv_temp - m) * inv_se; };
  const unsigned int kth = topk_threshold(prob, V, top_k, s);
  const unsigned int pth = topp_threshold(prob, V, top_p, kth, s);
  return draw_token(prob, V, kth > pth ? kth : pth, u, probs_row, s);
}

template <typename T>
__global__ __launch_bounds__(ST) void sample_kernel(const T* __restrict__ logits, long ld_row,
                                                   int V, float inv_temp, int top_k, float top_p,
                                                   const float* __restrict__ uniforms,
                                                   int64_t* __restrict__ out_ids,
                                                   float* __restrict__ out_lse,
                                                   float* __restrict__ out_probs) {
  __shared__ Shared s;
  const long row = blockIdx.x;
  const T* lg = logits + row * ld_row;
  auto load = [&](int i) { return ld<T>(lg, i); };
  float lse;
  const int pick = sample_row(load, V, inv_temp, top_k, top_p, uniforms[row],
                              out_probs ? out_probs + row * (long)V : nullptr, s, lse);
  if (threadIdx.x == 0) {
    if (out_lse) out_lse[row] = lse;
    out_ids[row] = pick;
  }
}

// The coupled pick of R rows of raw logits: row r chooses token index steps[r]
// of noise row rows[r] (r itself without `rows`).  Steps, rows and the seed are
// read from device memory, so a captured launch follows them under replay.
__global__ __launch_bounds__(ST) void coupled_sample_kernel(
    const float* __restrict__ logits, long ld_row, int V, float inv_temp, int top_k, float top_p,
    const int* __restrict__ steps, const int* __restrict__ rows,
    const int64_t* __restrict__ seed, int64_t* __restrict__ out_ids,
    float* __restrict__ out_lse) {
  __shared__ Shared s;
  const int row = blockIdx.x;
  const float* lg = logits + row * ld_row;
  auto load = [&](int i) { return lg[i]; };
  float lse;
  const int pick = coupled_row(load, V, inv_temp, top_k, top_p, (uint64_t)seed[0], steps[row],
                               rows ? rows[row] : row, s, lse);
  if (threadIdx.x == 0) {
    if (out_lse) out_lse[row] = lse;
    out_ids[row] = pick;
  }
}

// ---------------------------------------------------------------- selection
// One decode step's token selection, state in device memory (K18, K19): the
// logits processors applied on the load, the pick (greedy or phases 1-4
// above), then the bookkeeping the host loop does between two decode steps.
// A row belongs to one block, so the epilogue is one thread's plain stores.
struct SelectArgs {
  const float* logits;      // [B, V] fp32, read-only
  long ld_row;
  int V, B;
  int sampling;             // 0: greedy, 1: top-k / top-p sampling, 2: the coupled pick
  float inv_temp;
  int top_k;
  float top_p;
  const float* u;           // [n_steps, B] uniforms (sampling)
  int n_steps;
  int eos, pad;             // eos < 0: none
  int min_len;              // 0: off
  int use_pen;
  float pen, inv_pen;
  int bos;                  // forced at step 0 (< 0: off)
  int feos, feos_step;      // forced at step == feos_step (feos < 0: off)
  unsigned int* seen;       // [B, words] bitmap of each row's history
  int words;
  int* step;                // [B]
  int* unfinished;          // [B]
  int* finish_len;          // [B]
  float* scores;            // [B]
  int64_t* out;             // [B, n_steps]
  int64_t* nxt;             // [B] the decode graph's static inputs
  int64_t* cur;
  const int64_t* lens;      // [B]
  const int64_t* seed;      // [1] (sampling == 2)
};

// the processed logit x'(i), in the order of GPTForGeneration._processors()
struct ProcLoad {
  const float* lg;
  const unsigned int* seen;
  int mask_eos;   // min length active: this index gets -1e9 (< 0: off)
  int force;      // forced BOS / EOS: this index gets 0, the rest -1e9 (< 0: off)
  int use_pen;
  float pen, inv_pen;
  __device__ __forceinline__ bool in_seen(int i) const {
    return (seen[i >> 5] >> (i & 31)) & 1u;
  }
  // `hist(i)`: is token i in the row's history (asked only under a penalty)
  template <typename H>
  __device__ __forceinline__ float proc(int i, const H& hist) const {
#pragma clang fp contract(off)
    if (force >= 0) return i == force ? 0.f : -1e9f;
    float x = lg[i];
    if (i == mask_eos) x = -1e9f;
    // rounded products (never contracted into a consumer's add): bitwise torch's
    // GPU `x * pen` and `x / pen`, the latter being `x * fp32(1 / pen)` there
    if (use_pen && hist(i))
      x = x < 0.f ? x * pen : x * inv_pen;
    return x;
  }
  __device__ __forceinline__ float operator()(int i) const {
    return proc(i, [&](int t) { return in_seen(t); });
  }
};

// ProcLoad for slot j of a speculative window: the history is the row's bitmap
// plus the drafts d_1 .. d_j, which are held in registers (a rejected draft
// must never reach the bitmap).  Unused entries and ids outside the
// vocabulary are -1 and match no index.
constexpr int MAXW = 8;  // window slots: spec_tokens + 1
struct DraftLoad : ProcLoad {
  int d[MAXW - 1];
  __device__ __forceinline__ float operator()(int i) const {
    return proc(i, [&](int t) {
      bool h = in_seen(t);
#pragma unroll
      for (int k = 0; k < MAXW - 1; ++k) h |= d[k] == t;
      return h;
    });
  }
};

// the greedy pick on load(i): the max, the lowest index that holds it, and
// lse = m + log(sum exp(x - m)); every thread returns the pick
template <typename L>
__device__ __forceinline__ int greedy_row(const L& load, int V, Shared& s, float& lse) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int i = tid; i < V; i += ST) m = fmaxf(m, load(i));
  m = block_max(m, s);
  if (tid == 0) s.pick = V;
  __syncthreads();
  float se = 0.f;
  int first = V;
  for (int i = tid; i < V; i += ST) {
    const float x = load(i);
    se += __expf(x - m);
    if (x == m) first = min(first, i);
  }
  se = block_sum(se, s);
  if (first < V) atomicMin(&s.pick, first);
  __syncthreads();
  lse = m + __logf(se);
  return s.pick < V ? s.pick : 0;
}

__global__ __launch_bounds__(ST) void select_kernel(SelectArgs a) {
  __shared__ Shared s;
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int step = a.step[row];
  if (step >= a.n_steps) return;  // out / u hold n_steps columns
  const int unf = a.unfinished[row];
  unsigned int* seen = a.seen + (long)row * a.words;
  ProcLoad load;
  load.lg = a.logits + row * a.ld_row;
  load.seen = seen;
  load.mask_eos = (a.eos >= 0 && step < a.min_len) ? a.eos : -1;
  load.force = (a.feos >= 0 && step == a.feos_step) ? a.feos
               : (a.bos >= 0 && step == 0)          ? a.bos
                                                    : -1;
  load.use_pen = a.use_pen;
  load.pen = a.pen;
  load.inv_pen = a.inv_pen;
  int pick = 0;
  float lse = 0.f;
  if (unf) {  // a finished row emits pad: nothing to pick
    if (a.sampling == 2) {
      pick = coupled_row(load, a.V, a.inv_temp, a.top_k, a.top_p, (uint64_t)a.seed[0], step, row,
                         s, lse);
    } else if (a.sampling) {
      pick = sample_row(load, a.V, a.inv_temp, a.top_k, a.top_p, a.u[(long)step * a.B + row],
                        nullptr, s, lse);
    } else {
      pick = greedy_row(load, a.V, s, lse);
    }
  }
  if (tid == 0) {
    const int tok = unf ? pick : a.pad;
    if (unf) a.scores[row] += load(pick) - lse;
    a.out[(long)row * a.n_steps + step] = tok;
    if (tok >= 0 && tok < a.V) seen[tok >> 5] |= 1u << (tok & 31);
    if (unf && tok == a.eos) {
      a.unfinished[row] = 0;
      a.finish_len[row] = step + 1;
    }
    a.nxt[row] = tok;
    a.cur[row] = a.lens[row] + step;
    a.step[row] = step + 1;
  }
}

// ------------------------------------------------------ speculative verify
// One round of speculative decoding after the window step, state in device
// memory: spec_pick_kernel takes the target's pick of every window slot (the
// greedy one, or the coupled one under sampling), spec_accept_kernel does the bookkeeping the host loop does
// between two window steps.  Two launches on one stream, so the second sees
// all picks without a grid-wide sync; a row's state belongs to one thread.
struct SpecArgs {
  const float* logits;      // [B*W, V] fp32, read-only; row b*W + j is slot j of sample b
  long ld_row;
  int V, B, W;              // W = spec_tokens + 1 <= MAXW
  int n_steps;
  int eos;                  // < 0: none
  int min_len;              // 0: off
  int use_pen;
  float pen, inv_pen;
  int feos, feos_step;      // forced at step == feos_step (feos < 0: off)
  unsigned int* seen;       // [B, words]
  int words;
  int* step;                // [B] tokens emitted so far (>= 1)
  int* unfinished;          // [B]
  int* finish_len;          // [B]
  float* scores;            // [B]
  int64_t* out;             // [B, n_steps]
  int64_t* nxt;             // [B] the last emitted token
  int64_t* cur;             // [B] its position
  int64_t* tok;             // [B*W] the window's tokens: nxt, then the drafts d_1 .. d_g
  int64_t* pos;             // [B*W]
  int* wlens;               // [B] keys before the window
  int* picks;               // [B, W]
  float* logp;              // [B, W]
  int* rounds;              // [B]
  int* accepted;            // [B]
  int* any_active;          // [1]
  float inv_temp;           // the coupled pick's sampler settings and seed [1]
  int top_k;
  float top_p;
  const int64_t* seed;
};

// Workgroup (b, j): the processed logits of slot j, which chooses token
// step[b] + j from the history plus the drafts d_1 .. d_j, and their greedy
// pick (COUPLED: their coupled pick with token index step[b] + j, row b).  A row that no longer emits is skipped.  Slots at or past n_steps are
// picked as well (they are never emitted): the acceptance count covers them,
// as the host loop's does.
template <bool COUPLED>
__global__ __launch_bounds__(ST) void spec_pick_kernel(SpecArgs a) {
  __shared__ Shared s;
  const int b = blockIdx.x / a.W, j = blockIdx.x % a.W;
  const int step = a.step[b];
  if (!a.unfinished[b] || step >= a.n_steps) return;
  const int sj = step + j;
  DraftLoad load;
  load.lg = a.logits + (long)blockIdx.x * a.ld_row;
  load.seen = a.seen + (long)b * a.words;
  load.mask_eos = (a.eos >= 0 && sj < a.min_len) ? a.eos : -1;
  load.force = (a.feos >= 0 && sj == a.feos_step) ? a.feos : -1;  // step >= 1: never BOS
  load.use_pen = a.use_pen;
  load.pen = a.pen;
  load.inv_pen = a.inv_pen;
#pragma unroll
  for (int k = 0; k < MAXW - 1; ++k) {
    load.d[k] = -1;
    if (k < j) {
      const int64_t t = a.tok[(long)b * a.W + 1 + k];
      if (t >= 0 && t < a.V) load.d[k] = (int)t;
    }
  }
  float lse;
  int pick;
  if constexpr (COUPLED)
    pick = coupled_row(load, a.V, a.inv_temp, a.top_k, a.top_p, (uint64_t)a.seed[0], sj, b, s,
                       lse);
  else
    pick = greedy_row(load, a.V, s, lse);
  if (threadIdx.x == 0) {
    a.picks[blockIdx.x] = pick;
    a.logp[blockIdx.x] = load(pick) - lse;
  }
}

// Thread b: accept the longest prefix of row b's drafts that the picks agree
// with plus the target's next token, cut at n_steps and at the first EOS, and
// write the next round's window inputs.
__global__ __launch_bounds__(64) void spec_accept_kernel(SpecArgs a) {
  const int b = threadIdx.x;
  int live = 0;
  if (b < a.B) {
    const int W = a.W, step = a.step[b];
    if (a.unfinished[b] && step < a.n_steps) {
      const int64_t* d = a.tok + (long)b * W;  // d[i] = d_i, i in 1..W-1
      const int* picks = a.picks + b * W;
      int n = 0;
      while (n < W - 1 && d[n + 1] == (int64_t)picks[n]) ++n;
      int m = min(n + 1, a.n_steps - step);
      int unf = 1;
      if (a.eos >= 0) {
        for (int j = 0; j < m; ++j) {
          if (picks[j] == a.eos) {
            m = j + 1;
            unf = 0;
            a.unfinished[b] = 0;
            a.finish_len[b] = step + m;
            break;
          }
        }
      }
      unsigned int* seen = a.seen + (long)b * a.words;
      float sc = a.scores[b];
      for (int j = 0; j < m; ++j) {
        const int t = picks[j];  // in [0, V): the result of greedy_row / coupled_row
        a.out[(long)b * a.n_steps + step + j] = t;
        seen[t >> 5] |= 1u << (t & 31);
        sc += a.logp[b * W + j];
      }
      a.scores[b] = sc;
      const int64_t last = picks[m - 1];
      const int64_t cur = a.cur[b] + m;
      a.nxt[b] = last;
      a.step[b] = step + m;
      a.cur[b] = cur;
      a.rounds[b] += 1;
      a.accepted[b] += n;
      a.tok[(long)b * W] = last;
      for (int j = 0; j < W; ++j) a.pos[(long)b * W + j] = cur + j;
      a.wlens[b] = (int)cur;
      live = unf && step + m < a.n_steps;
    }
  }
  const int any = __syncthreads_or(live);
  if (threadIdx.x == 0) a.any_active[0] = any != 0;
}

}  // namespace

extern "C" int fx_sample(int dtype, const void* logits, long ld_row, int B, int V, float inv_temp,
                         int top_k, float top_p, const float* uniforms, int64_t* out_ids,
                         float* out_lse, float* out_probs, hipStream_t st) {
  if (B <= 0 || V <= 0) return 0;
  if (dtype == 2)
    sample_kernel<float><<<B, ST, 0, st>>>((const float*)logits, ld_row, V, inv_temp, top_k,
                                           top_p, uniforms, out_ids, out_lse, out_probs);
  else if (dtype == 0)
    sample_kernel<uint16_t><<<B, ST, 0, st>>>((const uint16_t*)logits, ld_row, V, inv_temp,
                                              top_k, top_p, uniforms, out_ids, out_lse,
                                              out_probs);
  else
    return -1;
  return 0;
}

extern "C" int fx_coupled_sample(const float* logits, long ld_row, int R, int V, float inv_temp,
                                 int top_k, float top_p, const int* steps, const int* rows,
                                 const int64_t* seed, int64_t* out_ids, float* out_lse,
                                 hipStream_t st) {
  if (R <= 0 || V <= 0) return 0;
  if (!logits || !steps || !seed || !out_ids) return -1;
  coupled_sample_kernel<<<R, ST, 0, st>>>(logits, ld_row, V, inv_temp, top_k, top_p, steps, rows,
                                          seed, out_ids, out_lse);
  return 0;
}

extern "C" int fx_select(const float* logits, long ld_row, int B, int V, int sampling,
                         float inv_temp, int top_k, float top_p, const float* u, int n_steps,
                         int eos, int pad, int min_len, float pen, float inv_pen, int bos,
                         int feos, int feos_step, unsigned int* seen, int words, int* step,
                         int* unfinished, int* finish_len, float* scores, int64_t* out,
                         int64_t* nxt, int64_t* cur, const int64_t* lens, hipStream_t st,
                         const int64_t* seed) {
  if (B <= 0 || V <= 0 || n_steps <= 0) return 0;
  if (sampling < 0 || sampling > 2) return -1;
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
  select_kernel<<<B, ST, 0, st>>>(a);
  return 0;
}

extern "C" int fx_spec_verify(const float* logits, long ld_row, int B, int W, int V, int n_steps,
                              int eos, int pad, int min_len, float pen, float inv_pen, int feos,
                              int feos_step, unsigned int* seen, int words, int* step,
                              int* unfinished, int* finish_len, float* scores, int64_t* out,
                              int64_t* nxt, int64_t* cur, int64_t* tok, int64_t* pos, int* wlens,
                              int* picks, float* logp, int* rounds, int* accepted,
                              int* any_active, hipStream_t st, int coupled, float inv_temp,
                              int top_k, float top_p, const int64_t* seed) {
  if (B <= 0 || V <= 0 || n_steps <= 0) return 0;
  if (words < (V + 31) / 32 || (coupled && !seed)) return -1;
  if (pad < 0 || pad >= V || eos >= V || feos >= V) return -2;
  if (W < 1 || W > MAXW || B > 64) return -3;
  SpecArgs a;
  a.logits = logits, a.ld_row = ld_row, a.V = V, a.B = B, a.W = W, a.n_steps = n_steps;
  a.eos = eos, a.min_len = min_len;
  a.use_pen = pen != 1.f, a.pen = pen, a.inv_pen = inv_pen;
  a.feos = feos, a.feos_step = feos_step;
  a.seen = seen, a.words = words, a.step = step, a.unfinished = unfinished;
  a.finish_len = finish_len, a.scores = scores, a.out = out, a.nxt = nxt, a.cur = cur;
  a.tok = tok, a.pos = pos, a.wlens = wlens, a.picks = picks, a.logp = logp;
  a.rounds = rounds, a.accepted = accepted, a.any_active = any_active;
  a.inv_temp = inv_temp, a.top_k = top_k, a.top_p = top_p, a.seed = seed;
  if (coupled)
    spec_pick_kernel<true><<<B * W, ST, 0, st>>>(a);
  else
    spec_pick_kernel<false><<<B * W, ST, 0, st>>>(a);
  spec_accept_kernel<<<1, 64, 0, st>>>(a);
  return 0;
}
