// pybind11 entry points for the HIP kernel library (module fleetx_amd._C._kernels).
// Tensors cross the boundary as raw device addresses (uintptr_t) plus the
// current HIP stream handle; shape checks live in fleetx_amd/ops/*.py.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <stdint.h>
#include <string>
#include <stdexcept>
#include <vector>

namespace py = pybind11;
typedef uintptr_t ptr;

#include "fx_api.h"

#define P(x) reinterpret_cast<void*>(x)
#define CP(x) reinterpret_cast<const void*>(x)
#define S(x) reinterpret_cast<hipStream_t>(x)
#define F(x) reinterpret_cast<float*>(x)

static std::vector<long> v3(const std::vector<long>& a) {
  std::vector<long> r(a);
  r.resize(3, 0);
  return r;
}

PYBIND11_MODULE(_kernels, m) {
  m.doc() = "FleetX-AMD HIP kernels (gfx950)";
  m.def("coltile_splits", &fx_coltile_splits);
  m.def("add_ln_fwd", [](int dt, ptr x, ptr bias, ptr res, ptr g, ptr b, ptr s_out, ptr y,
                         ptr mean, ptr rstd, int rows, int h, float eps, float p, uint64_t key,
                         ptr salt, ptr st) {
    fx_add_ln_fwd(dt, CP(x), CP(bias), CP(res), CP(g), CP(b), P(s_out), P(y), F(mean), F(rstd),
                  rows, h, eps, p, key, CP(salt), S(st));
  });
  m.def("ln_bwd_row", [](int dt, ptr dy, ptr s, ptr mean, ptr rstd, ptr g, ptr ds_in, ptr ds_out,
                         ptr dx_out, int rows, int h, float p, uint64_t key, ptr salt, ptr st) {
    fx_ln_bwd_row(dt, CP(dy), CP(s), F(mean), F(rstd), CP(g), CP(ds_in), P(ds_out), P(dx_out),
                  rows, h, p, key, CP(salt), S(st));
  });
  // LayerNorm backward with dgamma / dbeta (/ dbias of the fused residual's
  // linear) column sums in the same pass; returns -1 if h is not covered
  m.def("ln_bwd_cols_blocks", &fx_ln_bwd_cols_blocks);
  m.def("ln_bwd_cols", [](int dt, ptr dy, ptr s, ptr mean, ptr rstd, ptr g, ptr ds_in, ptr ds_out,
                          ptr dx_out, int rows, int h, float p, uint64_t key, ptr part,
                          int with_dbias, ptr fg, ptr tg, int accg, ptr fb, ptr tb, int accb,
                          ptr fx, ptr tx, int accx, ptr salt, ptr st) {
    return fx_ln_bwd_cols(dt, CP(dy), CP(s), F(mean), F(rstd), CP(g), CP(ds_in), P(ds_out),
                          P(dx_out), rows, h, p, key, F(part), with_dbias, F(fg), P(tg), accg,
                          F(fb), P(tb), accb, F(fx), P(tx), accx, CP(salt), S(st));
  }, py::arg("dt"), py::arg("dy"), py::arg("s"), py::arg("mean"), py::arg("rstd"), py::arg("g"),
     py::arg("ds_in"), py::arg("ds_out"), py::arg("dx_out"), py::arg("rows"), py::arg("h"),
     py::arg("p"), py::arg("key"), py::arg("part"), py::arg("with_dbias"), py::arg("fg") = 0,
     py::arg("tg") = 0, py::arg("accg") = 0, py::arg("fb") = 0, py::arg("tb") = 0,
     py::arg("accb") = 0, py::arg("fx") = 0, py::arg("tx") = 0, py::arg("accx") = 0,
     py::arg("salt") = 0, py::arg("st") = 0);
  // column-sum producers: cnt != 0 fuses the finalize (last workgroup of a
  // column tile sums the splits into f*/t* outputs); cnt == 0: the caller
  // runs coltile_finalize
  m.def("coltile_partial", [](int dt, int mode, ptr a, ptr b, ptr mean, ptr rstd, ptr p0, ptr p1,
                              int rows, int cols, int splits, ptr st, ptr cnt, ptr f0, ptr t0,
                              int acc0, ptr f1, ptr t1, int acc1) {
    fx_coltile_partial(dt, mode, CP(a), CP(b), F(mean), F(rstd), F(p0), F(p1), rows, cols, splits,
                       S(st), reinterpret_cast<int*>(cnt), F(f0), P(t0), acc0, F(f1), P(t1),
                       acc1);
  }, py::arg("dt"), py::arg("mode"), py::arg("a"), py::arg("b"), py::arg("mean"), py::arg("rstd"),
     py::arg("p0"), py::arg("p1"), py::arg("rows"), py::arg("cols"), py::arg("splits"),
     py::arg("st"), py::arg("cnt") = 0, py::arg("f0") = 0, py::arg("t0") = 0, py::arg("acc0") = 0,
     py::arg("f1") = 0, py::arg("t1") = 0, py::arg("acc1") = 0);
  m.def("coltile_finalize", [](int dt, ptr part, int splits, int cols, ptr out_f32, ptr out_t,
                               int accumulate, ptr st) {
    fx_coltile_finalize(dt, F(part), splits, cols, F(out_f32), P(out_t), accumulate, S(st));
  });
  m.def("bias_gelu_fwd", [](int dt, int erf, ptr x, ptr bias, ptr y, long n, int cols, ptr st) {
    fx_bias_gelu_fwd(dt, erf, CP(x), CP(bias), P(y), n, cols, S(st));
  });
  m.def("bias_gelu_bwd", [](int dt, int erf, ptr dy, ptr x, ptr bias, ptr dx, ptr part, int rows,
                            int cols, int splits, ptr st, ptr cnt, ptr out_f32, ptr out_t,
                            int acc) {
    fx_bias_gelu_bwd(dt, erf, CP(dy), CP(x), CP(bias), P(dx), F(part), rows, cols, splits, S(st),
                     reinterpret_cast<int*>(cnt), F(out_f32), P(out_t), acc);
  }, py::arg("dt"), py::arg("erf"), py::arg("dy"), py::arg("x"), py::arg("bias"), py::arg("dx"),
     py::arg("part"), py::arg("rows"), py::arg("cols"), py::arg("splits"), py::arg("st"),
     py::arg("cnt") = 0, py::arg("out_f32") = 0, py::arg("out_t") = 0, py::arg("acc") = 0);
  m.def("bias_dropout_add_fwd", [](int dt, ptr x, ptr bias, ptr res, ptr out, long n, int cols,
                                   float p, uint64_t key, ptr salt, ptr st) {
    fx_bias_dropout_add_fwd(dt, CP(x), CP(bias), CP(res), P(out), n, cols, p, key, CP(salt),
                            S(st));
  });
  m.def("dropout_bwd_colsum", [](int dt, ptr dout, ptr dx, ptr part, int rows, int cols,
                                 int splits, float p, uint64_t key, ptr salt, ptr st, ptr cnt,
                                 ptr out_f32, ptr out_t, int acc) {
    fx_dropout_bwd_colsum(dt, CP(dout), P(dx), F(part), rows, cols, splits, p, key, CP(salt), S(st),
                          reinterpret_cast<int*>(cnt), F(out_f32), P(out_t), acc);
  }, py::arg("dt"), py::arg("dout"), py::arg("dx"), py::arg("part"), py::arg("rows"),
     py::arg("cols"), py::arg("splits"), py::arg("p"), py::arg("key"), py::arg("salt"),
     py::arg("st"), py::arg("cnt") = 0, py::arg("out_f32") = 0, py::arg("out_t") = 0,
     py::arg("acc") = 0);
  m.def("dropout_fwd", [](int dt, ptr x, ptr y, long n, float p, uint64_t key, ptr salt,
                          ptr st) {
    fx_dropout_fwd(dt, CP(x), P(y), n, p, key, CP(salt), S(st));
  });
  m.def("ce_stats", [](int dt, ptr logits, ptr labels, int rows, int V, long vstart, ptr mx,
                       ptr sm, ptr tg, int ignore, ptr st) {
    fx_ce_stats(dt, CP(logits), reinterpret_cast<const int64_t*>(labels), rows, V, vstart, F(mx),
                F(sm), F(tg), ignore, S(st));
  });
  m.def("ce_bwd", [](int dt, ptr logits, ptr dx, ptr labels, ptr lse, ptr g, int rows, int V,
                     long vstart, int ignore, ptr st) {
    fx_ce_bwd(dt, CP(logits), P(dx), reinterpret_cast<const int64_t*>(labels), F(lse), F(g), rows,
              V, vstart, ignore, S(st));
  });
  m.def("sumsq_blocks", &fx_sumsq_blocks);
  m.def("sumsq_chunks", [](ptr addr, ptr len, int n, ptr partial, ptr st) {
    fx_sumsq_chunks(reinterpret_cast<const int64_t*>(addr), reinterpret_cast<const int64_t*>(len),
                    n, F(partial), S(st));
  });
  m.def("sumsq_f32", [](ptr x, long n, ptr partial, int blocks, ptr st) {
    fx_sumsq_f32(F(x), n, F(partial), blocks, S(st));
  });
  m.def("sumsq_16", [](int dt, ptr x, long n, ptr partial, int blocks, ptr st) {
    fx_sumsq_16(dt, CP(x), n, F(partial), blocks, S(st));
  });
  // flags: bit 0 = 16-bit gradient, bit 1 = packed master (p = the master's low halves,
  // p16 = the bf16 parameters); lr_dev: device learning rate (0 = lr); grid / nt / wide: the
  // launch shape (loss_optim_embed.hip fx_adamw)
  m.def("adamw", [](int dt, int flags, ptr p, ptr g, ptr mm, ptr vv, ptr p16, long n, float lr,
                    float b1, float b2, float eps, float wd, float l2, ptr gscale, ptr skip,
                    ptr step, ptr lr_dev, int grid, int nt, int wide, ptr st) {
    return fx_adamw(dt, flags, P(p), CP(g), F(mm), F(vv), P(p16), n, lr, b1, b2, eps, wd, l2,
                    F(gscale), reinterpret_cast<const int*>(skip),
                    reinterpret_cast<const int*>(step), F(lr_dev), grid, nt, wide, S(st));
  });
  m.def("pk_split", [](ptr x, ptr hi, ptr lo, long n, ptr st) {
    fx_pk_split(F(x), P(hi), P(lo), n, S(st));
  });
  m.def("pk_join", [](ptr hi, ptr lo, ptr x, long n, ptr st) {
    fx_pk_join(CP(hi), CP(lo), F(x), n, S(st));
  });
  m.def("cast_f32", [](int dt, ptr x, ptr y, long n, ptr st) {
    fx_cast_f32(dt, F(x), P(y), n, S(st));
  });
  m.def("accum_f32", [](int dt, ptr acc, ptr x, long n, int overwrite, ptr st) {
    fx_accum_f32(dt, F(acc), CP(x), n, overwrite, S(st));
  });
  m.def("embedding_fwd", [](int dt, ptr ids, ptr pos, ptr W, ptr Pw, ptr out, int ntok, int h,
                            long vstart, long vsize, ptr st) {
    fx_embedding_fwd(dt, reinterpret_cast<const int64_t*>(ids),
                     reinterpret_cast<const int64_t*>(pos), CP(W), CP(Pw), P(out), ntok, h, vstart,
                     vsize, S(st));
  });
  m.def("embedding_bwd", [](int dt, ptr ids, ptr dout, ptr dW, int ntok, int h, long vstart,
                            long vsize, ptr st) {
    fx_embedding_bwd(dt, reinterpret_cast<const int64_t*>(ids), CP(dout), F(dW), ntok, h, vstart,
                     vsize, S(st));
  });
  m.def("embedding_bwd_sorted", [](int dt, ptr sid, ptr perm, ptr dout, ptr dW, int ntok, int h,
                                   long vstart, long vsize, ptr st) {
    fx_embedding_bwd_sorted(dt, reinterpret_cast<const int64_t*>(sid),
                            reinterpret_cast<const int64_t*>(perm), CP(dout), F(dW), ntok, h,
                            vstart, vsize, S(st));
  });
  m.def("fa_set_stamps", [](ptr p) { return fx_fa_set_stamps(P(p)); });  // lab builds: stamps
  m.def("fa_lab", &fx_fa_lab);  // 1 in tools/fa_lab builds (per-wave stamps compiled in)
  m.def("flash_fwd", [](int dt, ptr q, ptr k, ptr v, ptr out, ptr lse, std::vector<long> qs,
                        std::vector<long> ks, std::vector<long> vs, std::vector<long> os,
                        ptr kv_lens, ptr kbias, long kb_stride, int B, int H, int Sq, int Sk, int D,
                        int causal, float scale, float p, uint64_t key, ptr salt, ptr st) {
    auto a = v3(qs), b = v3(ks), c = v3(vs), d = v3(os);
    return fx_flash_fwd(dt, CP(q), CP(k), CP(v), P(out), F(lse), a.data(), b.data(), c.data(),
                        d.data(), reinterpret_cast<const int*>(kv_lens), F(kbias), kb_stride, B, H,
                        Sq, Sk, D, causal, scale, p, key, CP(salt), S(st));
  });
  m.def("flash_fwd_qoff", [](int dt, ptr q, ptr k, ptr v, ptr out, ptr lse, std::vector<long> qs,
                             std::vector<long> ks, std::vector<long> vs, std::vector<long> os,
                             ptr q_starts, ptr kv_lens, int B, int H, int Sq, int Sk, int D,
                             float scale, ptr st) {
    auto a = v3(qs), b = v3(ks), c = v3(vs), d = v3(os);
    return fx_flash_fwd_qoff(dt, CP(q), CP(k), CP(v), P(out), F(lse), a.data(), b.data(),
                             c.data(), d.data(), reinterpret_cast<const int*>(q_starts),
                             reinterpret_cast<const int*>(kv_lens), B, H, Sq, Sk, D, scale,
                             S(st));
  });
  m.def("flash_bwd", [](int dt, ptr q, ptr k, ptr v, ptr o, ptr dout, ptr lse, ptr delta, ptr dq,
                        ptr dk,
                        ptr dv, std::vector<long> qs, std::vector<long> ks, std::vector<long> vs,
                        std::vector<long> os, std::vector<long> dqs, std::vector<long> dks,
                        ptr kv_lens, ptr kbias, long kb_stride, int B, int H, int Sq, int Sk, int D,
                        int causal, float scale, float p, uint64_t key, ptr salt, ptr st) {
    auto a = v3(qs), b = v3(ks), c = v3(vs), d = v3(os), e = v3(dks), f = v3(dqs);
    return fx_flash_bwd(dt, CP(q), CP(k), CP(v), CP(o), CP(dout), F(lse), F(delta), P(dq), P(dk),
                        P(dv), a.data(), b.data(), c.data(), d.data(), f.data(), e.data(),
                        reinterpret_cast<const int*>(kv_lens), F(kbias), kb_stride, B, H, Sq, Sk,
                        D, causal, scale, p, key, CP(salt), S(st));
  });
  m.def("gn_nseg", [](long rows, long hw) { return fx_gn_nseg(rows, hw); });
  m.def("gn_fwd", [](int dt, ptr x, ptr gamma, ptr beta, ptr scale, ptr shift, ptr y, ptr part,
                     ptr mean, ptr rstd, int B, int C, int G, long hw, int nseg, float eps,
                     int silu, ptr st) {
    return fx_gn_fwd(dt, CP(x), F(gamma), F(beta), F(scale), F(shift), P(y),
                     reinterpret_cast<double*>(part), F(mean), F(rstd), B, C, G, hw, nseg, eps,
                     silu, S(st));
  });
  m.def("gn_bwd_reduce", [](int dt, ptr x, ptr dy, ptr mean, ptr rstd, ptr gamma, ptr beta,
                            ptr scale, ptr shift, ptr part, int B, int C, int G, long hw, int nseg,
                            int silu, ptr st) {
    return fx_gn_bwd_reduce(dt, CP(x), CP(dy), F(mean), F(rstd), F(gamma), F(beta), F(scale),
                            F(shift), F(part), B, C, G, hw, nseg, silu, S(st));
  });
  m.def("gn_bwd_apply", [](int dt, ptr x, ptr dy, ptr mean, ptr rstd, ptr gamma, ptr beta,
                           ptr scale, ptr shift, ptr g1, ptr g2, ptr dx, int B, int C, int G,
                           long hw, int nseg, int silu, ptr st) {
    return fx_gn_bwd_apply(dt, CP(x), CP(dy), F(mean), F(rstd), F(gamma), F(beta), F(scale),
                           F(shift), F(g1), F(g2), P(dx), B, C, G, hw, nseg, silu, S(st));
  });
  m.def("fake_quant_fwd", [](int dt, ptr x, ptr y, ptr scale, int bits, long n, ptr st) {
    return fx_fake_quant_fwd(dt, CP(x), P(y), F(scale), bits, n, S(st));
  });
  m.def("absmax", [](int dt, ptr x, long n, ptr out, ptr st) {
    fx_absmax(dt, CP(x), n, F(out), S(st));
  });
  m.def("transpose16", [](int dt, ptr x, ptr y, ptr part, int R, int C, long ldx, long ldy,
                          ptr st) { return fx_transpose16(dt, CP(x), P(y), F(part), R, C, ldx, ldy, S(st)); });
  m.def("sample", [](int dt, ptr logits, long ld, int B, int V, float inv_temp, int top_k,
                     float top_p, ptr u, ptr ids, ptr lse, ptr probs, ptr st) {
    return fx_sample(dt, CP(logits), ld, B, V, inv_temp, top_k, top_p, F(u),
                     reinterpret_cast<int64_t*>(ids), F(lse), F(probs), S(st));
  });
  m.def("select", [](ptr logits, long ld, int B, int V, int sampling, float inv_temp, int top_k,
                     float top_p, ptr u, int n_steps, int eos, int pad, int min_len, float pen,
                     float inv_pen, int bos, int feos, int feos_step, ptr seen, int words,
                     ptr step, ptr unfinished, ptr finish_len, ptr scores, ptr out, ptr nxt,
                     ptr cur, ptr lens, ptr st, ptr seed) {
    return fx_select(F(logits), ld, B, V, sampling, inv_temp, top_k, top_p, F(u), n_steps, eos,
                     pad, min_len, pen, inv_pen, bos, feos, feos_step,
                     reinterpret_cast<unsigned int*>(seen), words, reinterpret_cast<int*>(step),
                     reinterpret_cast<int*>(unfinished), reinterpret_cast<int*>(finish_len),
                     F(scores), reinterpret_cast<int64_t*>(out), reinterpret_cast<int64_t*>(nxt),
                     reinterpret_cast<int64_t*>(cur), reinterpret_cast<const int64_t*>(lens),
                     S(st), reinterpret_cast<const int64_t*>(seed));
  });
  m.def("coupled_sample", [](ptr logits, long ld, int R, int V, float inv_temp, int top_k,
                             float top_p, ptr steps, ptr rows, ptr seed, ptr ids, ptr lse,
                             ptr st) {
    return fx_coupled_sample(F(logits), ld, R, V, inv_temp, top_k, top_p,
                             reinterpret_cast<const int*>(steps),
                             reinterpret_cast<const int*>(rows),
                             reinterpret_cast<const int64_t*>(seed),
                             reinterpret_cast<int64_t*>(ids), F(lse), S(st));
  });
  m.def("spec_verify", [](ptr logits, long ld, int B, int W, int V, int n_steps, int eos, int pad,
                          int min_len, float pen, float inv_pen, int feos, int feos_step, ptr seen,
                          int words, ptr step, ptr unfinished, ptr finish_len, ptr scores, ptr out,
                          ptr nxt, ptr cur, ptr tok, ptr pos, ptr wlens, ptr picks, ptr logp,
                          ptr rounds, ptr accepted, ptr any_active, ptr st, int coupled,
                          float inv_temp, int top_k, float top_p, ptr seed) {
    auto I = [](ptr p) { return reinterpret_cast<int*>(p); };
    auto L = [](ptr p) { return reinterpret_cast<int64_t*>(p); };
    return fx_spec_verify(F(logits), ld, B, W, V, n_steps, eos, pad, min_len, pen, inv_pen, feos,
                          feos_step, reinterpret_cast<unsigned int*>(seen), words, I(step),
                          I(unfinished), I(finish_len), F(scores), L(out), L(nxt), L(cur), L(tok),
                          L(pos), I(wlens), I(picks), F(logp), I(rounds), I(accepted),
                          I(any_active), S(st), coupled, inv_temp, top_k, top_p, L(seed));
  });
  m.def("decode_attn", [](int dt, ptr q, ptr kc, ptr vc, ptr out, ptr lens, int B, int H, int D,
                          int maxlen, int nsplit, ptr ws, long sqb, long sqh, long skb, long sks,
                          long skh, long sob, float scale, ptr st) {
    return fx_decode_attn(dt, CP(q), CP(kc), CP(vc), P(out), reinterpret_cast<const int*>(lens), B,
                          H, D, maxlen, nsplit, F(ws), sqb, sqh, skb, sks, skh, sob, scale, S(st));
  });
  m.def("beam_decode_attn", [](int dt, ptr q, ptr kp, ptr vp, ptr plens, ptr kg, ptr vg, ptr glens,
                               ptr anc, ptr out, ptr ws, int B, int nb, int H, int D, int S, int G,
                               int nsplit, long sqb, long sqh, long spb, long sps, long sph,
                               long sgb, long sgs, long sgh, long sab, long sob, float scale,
                               int nw, ptr st) {
    return fx_beam_decode_attn(dt, CP(q), CP(kp), CP(vp), reinterpret_cast<const int*>(plens),
                               CP(kg), CP(vg), reinterpret_cast<const int*>(glens),
                               reinterpret_cast<const int*>(anc), P(out), F(ws), B, nb, H, D, S, G,
                               nsplit, sqb, sqh, spb, sps, sph, sgb, sgs, sgh, sab, sob, scale,
                               nw, S(st));
  });
  m.def("window_decode_attn", [](int dt, ptr q, ptr kc, ptr vc, ptr lens, ptr out, ptr ws, int B,
                                 int W, int H, int D, int maxlen, int nsplit, long sqb, long sqh,
                                 long skb, long sks, long skh, long sob, float scale, int nw,
                                 ptr st) {
    return fx_window_decode_attn(dt, CP(q), CP(kc), CP(vc), reinterpret_cast<const int*>(lens),
                                 P(out), F(ws), B, W, H, D, maxlen, nsplit, sqb, sqh, skb, sks,
                                 skh, sob, scale, nw, S(st));
  });
  m.def("softmax_fwd", [](int dt, int mdt, ptr x, ptr mask, ptr y, long rows, int Sq, int Sk,
                          long mask_div, float scale, int causal, ptr st) {
    return fx_softmax_fwd(dt, mdt, CP(x), CP(mask), P(y), rows, Sq, Sk, mask_div, scale, causal,
                          S(st));
  });
  m.def("gemm", [](int dt, int la, int lb, int epi, int M, int N, int K, ptr A, long lda, ptr B,
                   long ldb, ptr C, long ldc, ptr bias, ptr aux, long ldaux, int beta, ptr st,
                   ptr sq, ptr ws) {
    return fx_gemm(dt, la, lb, epi, M, N, K, CP(A), lda, CP(B), ldb, P(C), ldc, CP(bias), P(aux),
                   ldaux, beta, S(st), F(sq), F(ws));
  }, py::arg("dt"), py::arg("la"), py::arg("lb"), py::arg("epi"), py::arg("M"), py::arg("N"),
     py::arg("K"), py::arg("A"), py::arg("lda"), py::arg("B"), py::arg("ldb"), py::arg("C"),
     py::arg("ldc"), py::arg("bias"), py::arg("aux"), py::arg("ldaux"), py::arg("beta"),
     py::arg("st"), py::arg("sq") = 0, py::arg("ws") = 0);
  m.def("gemm_ws_bytes", &fx_gemm_ws_bytes);
  m.def("gemm_set_gm", &fx_gemm_set_gm);
  m.def("gemm_set_geom", &fx_gemm_set_geom);
  m.def("gemm_set_tuned", &fx_gemm_set_tuned);
  m.def("gemm_set_tune", &fx_gemm_set_tune);
  m.def("gemm_set_persist", &fx_gemm_set_persist);
  m.def("gemm_set_xrect", &fx_gemm_set_xrect);
  m.def("gemm_tuned", []() {
    std::vector<long> buf(7 * 512);
    const int n = fx_gemm_tuned(buf.data(), (int)buf.size());
    py::list rows;
    for (int i = 0; i < n; ++i)
      rows.append(py::make_tuple(buf[7 * i], buf[7 * i + 1], buf[7 * i + 2], buf[7 * i + 3],
                                 buf[7 * i + 4], buf[7 * i + 5], buf[7 * i + 6]));
    return rows;
  });
  // decode-time skinny GEMM with fused sub-layer epilogues (decode_gemv.hip)
  m.def("decode_gemv", [](int dt, int epi, int M, int N, int K, ptr x, long ldx, ptr w, long ldw,
                          ptr bias, ptr res, long ldres, ptr y, long ldy, ptr kc, ptr vc, ptr pos,
                          ptr rows, int heads, int head_dim, int maxlen, ptr ln_w, ptr ln_b,
                          float ln_eps, ptr st) {
    return fx_decode_gemv(dt, epi, M, N, K, CP(x), ldx, CP(w), ldw, CP(bias), CP(res), ldres, P(y),
                          ldy, P(kc), P(vc), reinterpret_cast<const long*>(pos),
                          reinterpret_cast<const int*>(rows), heads, head_dim, maxlen, CP(ln_w), CP(ln_b), ln_eps, S(st));
  });
  // the same with int8 weights and one fp32 scale per output row (decode_gemv_w8.hip)
  m.def("decode_gemv_w8", [](int dt, int epi, int M, int N, int K, ptr x, long ldx, ptr wq, long ldw,
                             ptr wscale, ptr bias, ptr res, long ldres, ptr y, long ldy, ptr kc,
                             ptr vc, ptr pos, ptr rows, int heads, int head_dim, int maxlen,
                             ptr ln_w, ptr ln_b, float ln_eps, ptr st) {
    return fx_decode_gemv_w8(dt, epi, M, N, K, CP(x), ldx, reinterpret_cast<const int8_t*>(wq), ldw,
                             reinterpret_cast<const float*>(wscale), CP(bias), CP(res), ldres,
                             P(y), ldy, P(kc), P(vc), reinterpret_cast<const long*>(pos),
                             reinterpret_cast<const int*>(rows), heads, head_dim, maxlen, CP(ln_w), CP(ln_b), ln_eps, S(st));
  });
  // the same with packed int4 weights (ldw in bytes) and one fp32 scale per k-group of 256
  // and output row, [K / 256, N] (decode_gemv_w4.hip)
  m.def("decode_gemv_w4", [](int dt, int epi, int M, int N, int K, ptr x, long ldx, ptr wq, long ldw,
                             ptr wscale, ptr bias, ptr res, long ldres, ptr y, long ldy, ptr kc,
                             ptr vc, ptr pos, ptr rows, int heads, int head_dim, int maxlen,
                             ptr ln_w, ptr ln_b, float ln_eps, ptr st) {
    return fx_decode_gemv_w4(dt, epi, M, N, K, CP(x), ldx, reinterpret_cast<const uint8_t*>(wq), ldw,
                             reinterpret_cast<const float*>(wscale), CP(bias), CP(res), ldres,
                             P(y), ldy, P(kc), P(vc), reinterpret_cast<const long*>(pos),
                             reinterpret_cast<const int*>(rows), heads, head_dim, maxlen, CP(ln_w), CP(ln_b), ln_eps, S(st));
  });
  // CU-masked stream (streams.hip): returns (stream handle, CUs selected)
  m.def("cumask_stream_create", [](int ncu) {
    int got = 0;
    hipStream_t s = fx_cumask_stream_create(ncu, &got);
    return py::make_tuple(reinterpret_cast<ptr>(s), got);
  });
  m.def("stream_destroy", [](ptr s) { return fx_stream_destroy(S(s)); });
  // intra-node one-shot all-reduce over IPC-mapped peer memory (comm.hip)
  m.def("comm_max_world", &fx_comm_max_world);
  m.def("comm_max_blocks", &fx_comm_max_blocks);
  m.def("comm_alloc", [](long slot_granules) {
    return reinterpret_cast<ptr>(fx_comm_alloc(slot_granules));
  });
  m.def("comm_free", [](ptr p) { return fx_comm_free(P(p)); });
  m.def("comm_ipc_handle", [](ptr p) {
    char h[64];
    const int r = fx_comm_ipc_handle(P(p), h);
    if (r != 0) throw std::runtime_error("hipIpcGetMemHandle failed: " + std::to_string(r));
    return py::bytes(h, 64);
  });
  m.def("comm_ipc_open", [](py::bytes h) {
    std::string s = h;
    if (s.size() != 64) throw std::runtime_error("IPC handle must be 64 bytes");
    return reinterpret_cast<ptr>(fx_comm_ipc_open(s.data()));
  });
  m.def("comm_ipc_close", [](ptr p) { return fx_comm_ipc_close(P(p)); });
  m.def("comm_allreduce", [](int dt, int op, ptr in, ptr out, long n, int rank, int world,
                             std::vector<uint64_t> peers, ptr epochs, ptr err, long slot,
                             unsigned long long timeout_ticks, ptr st) {
    if ((int)peers.size() != world) throw std::runtime_error("need one receive base per rank");
    return fx_comm_allreduce(dt, op, CP(in), P(out), n, rank, world, peers.data(),
                             reinterpret_cast<unsigned int*>(epochs),
                             reinterpret_cast<unsigned int*>(err), slot, timeout_ticks, S(st));
  });
  m.def("softmax_bwd", [](int dt, ptr y, ptr dy, ptr dx, long rows, int Sq, int Sk, float scale,
                          int causal, ptr st) {
    return fx_softmax_bwd(dt, CP(y), CP(dy), P(dx), rows, Sq, Sk, scale, causal, S(st));
  });
}
