// Multi-query decode attention core, part 2 of 3: stream rows [lo, hi) of one
// K/V cache into the state of part 1 (decode_attn_mq_init.inc).
//
// Names the including kernel provides, besides those of part 1:
//   w, sub        wave, lane group within the wave
//   kb, vb, ks    the lane's (sample, head, column) K / V base, row stride
//   lo, hi        the rows to stream
//   causal, len0  constexpr bool: query j sees key k iff k <= len0 + j; false: every
//                 query sees every key of the range
  {
    // software pipeline: the rows of step i+1 are requested before step i is
    // scored, so a wave overlaps its own memory round trip with its math (with
    // several queries the math per row is long, and few waves fit per SIMD)
    uint4 kraw[C::U], vraw[C::U], knext[C::U], vnext[C::U];
    if (lo < hi) {
#pragma unroll
      for (int u = 0; u < C::U; ++u) {
        const int key = lo + (u * C::NW + w) * C::KPW + sub;
        const int kk = key < hi ? key : lo;  // in-range dummy row
        kraw[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * ks);
        vraw[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * ks);
      }
    }
    for (int k0 = lo; k0 < hi; k0 += C::STEP) {
      const bool more = k0 + C::STEP < hi;
      if (more) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
          const int key = k0 + C::STEP + (u * C::NW + w) * C::KPW + sub;
          const int kk = key < hi ? key : lo;
          knext[u] = *reinterpret_cast<const uint4*>(kb + (long)kk * ks);
          vnext[u] = *reinterpret_cast<const uint4*>(vb + (long)kk * ks);
        }
      }
      // key u is visible to query j iff it lies in [lo, hi) and, if causal,
      // key <= len0 + j, i.e. iff j >= jmin[u] (NQ for a key outside the range)
      int jmin[C::U];
#pragma unroll
      for (int u = 0; u < C::U; ++u) {
        const int key = k0 + (u * C::NW + w) * C::KPW + sub;
        jmin[u] = key < hi ? (causal ? key - len0 : 0) : C::NQ;
      }
      float kv[C::U][8], vv[C::U][8];
#pragma unroll
      for (int u = 0; u < C::U; ++u) {
        unpack8<T>(kraw[u], kv[u]);
        unpack8<T>(vraw[u], vv[u]);
      }
#pragma unroll
      for (int j = 0; j < C::NQ; ++j) {
        float sc[C::U];
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
          sc[u] = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) sc[u] += kv[u][i] * qv[j][i];
        }
        float mx = m[j];
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
          const float t = group_sum<C::LPK>(sc[u]);
          sc[u] = j >= jmin[u] ? t : C::NEG;
          mx = fmaxf(mx, sc[u]);
        }
        const float a = __expf(m[j] - mx);
        l[j] *= a;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[j][i] *= a;
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
          const float p = j >= jmin[u] ? __expf(sc[u] - mx) : 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) o[j][i] += p * vv[u][i];
          l[j] += p;
        }
        m[j] = mx;
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
          kraw[u] = knext[u];
          vraw[u] = vnext[u];
        }
      }
    }
  }
