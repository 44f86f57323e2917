// Multi-query decode attention core, part 1 of 3: the per-query state and its
// initialisation.  See "Multi-query core" in decode_attn.hip for the design,
// the contracts and why the parts are text included in a kernel's body.
//
// Names the including kernel provides:
//   T, C = MQ<D, NQ, NW>           element type, the core's constants
//   q, row0, nq, sqb, sqh, hd, c   query j is row row0 + (j < nq ? j : 0) of q; c: the
//                                  lane's first column
//   scale
// Names it leaves behind: the state qv, o, m, l [NQ] (m is C::NEG until a key is seen).
  float qv[C::NQ][8], o[C::NQ][8], m[C::NQ], l[C::NQ];
#pragma unroll
  for (int j = 0; j < C::NQ; ++j) {
    load8<T>(q + (row0 + (j < nq ? j : 0)) * sqb + hd * sqh + c, qv[j]);
    m[j] = C::NEG;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qv[j][i] *= scale;
      o[j][i] = 0.f;
    }
  }
