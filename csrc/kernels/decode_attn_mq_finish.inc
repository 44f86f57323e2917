// Multi-query decode attention core, part 3 of 3: merge the workgroup's states
// per query and write rows row0 .. row0+nq-1, the normalised output at
// nsplit == 1, else the partial of this split.
//
// Names the including kernel provides, besides those of parts 1 and 2:
//   lane, H, split, nsplit, ws, out, sob
  // a state that saw no key is (-inf, 0, 0), as merge_state and the combine pass expect
#pragma unroll
  for (int j = 0; j < C::NQ; ++j) m[j] = l[j] > 0.f ? m[j] : -INFINITY;
  // ---- merge: lane groups of a wave by shuffles, then the waves through LDS
#pragma unroll
  for (int j = 0; j < C::NQ; ++j) {
#pragma unroll
    for (int off = C::LPK; off < 64; off <<= 1) {
      float o2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o2[i] = __shfl_xor(o[j][i], off, 64);
      const float m2 = __shfl_xor(m[j], off, 64), l2 = __shfl_xor(l[j], off, 64);
      merge_state(m[j], l[j], o[j], m2, l2, o2);
    }
  }
  // in rounds of RB queries: static LDS stays far below 64 KB also for 16 waves
  __shared__ float sm_m[C::RB][C::NW * C::LPK], sm_l[C::RB][C::NW * C::LPK],
      sm_o[C::RB][C::NW * C::LPK][8];
#pragma unroll
  for (int r0 = 0; r0 < C::NQ; r0 += C::RB) {
    if (r0 > 0) __syncthreads();
    if (lane < C::LPK) {
#pragma unroll
      for (int r = 0; r < C::RB; ++r) {
        if (r0 + r >= C::NQ) continue;
        sm_m[r][w * C::LPK + lane] = m[r0 + r];
        sm_l[r][w * C::LPK + lane] = l[r0 + r];
#pragma unroll
        for (int i = 0; i < 8; ++i) sm_o[r][w * C::LPK + lane][i] = o[r0 + r][i];
      }
    }
    __syncthreads();
    // thread t merges query r0 + t / LPK, column slice t % LPK
    const int r = threadIdx.x / C::LPK, sl = threadIdx.x % C::LPK, j = r0 + r;
    if (r < C::RB && j < nq) {
      float M = -INFINITY, L = 0.f, O[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) O[i] = 0.f;
#pragma unroll
      for (int i = 0; i < C::NW; ++i)
        merge_state(M, L, O, sm_m[r][i * C::LPK + sl], sm_l[r][i * C::LPK + sl],
                    sm_o[r][i * C::LPK + sl]);
      if (nsplit == 1) {  // one split: normalise and store the output directly
        const float inv = L > 0.f ? 1.f / L : 0.f;
        float res[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) res[i] = O[i] * inv;
        store8<T>(out + (row0 + j) * sob + hd * C::D + sl * 8, res);
      } else {
        float* wp = ws + (((row0 + j) * H + hd) * nsplit + split) * (C::D + 2);
#pragma unroll
        for (int i = 0; i < 8; ++i) wp[sl * 8 + i] = O[i];
        if (sl == 0) {
          wp[C::D] = M;
          wp[C::D + 1] = L;
        }
      }
    }
  }
