// The extern "C" ABI of the HIP kernel library: every fx_* entry point, declared
// once.  bindings.cpp calls through these prototypes and each .hip file that
// defines an entry includes them, so a definition that drifts from its
// prototype is a compile error ("conflicting types") instead of a silent
// mis-call.  dtype codes: 0 = bf16, 1 = fp16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
int fx_coltile_splits(int rows, int cols);
void fx_add_ln_fwd(int, const void*, const void*, const void*, const void*, const void*, void*,
                   void*, float*, float*, int, int, float, float, uint64_t, const void*,
                   hipStream_t);
void fx_ln_bwd_row(int, const void*, const void*, const float*, const float*, const void*,
                   const void*, void*, void*, int, int, float, uint64_t, const void*, hipStream_t);
int fx_ln_bwd_cols_blocks(int, int, int);
int fx_ln_bwd_cols(int, const void*, const void*, const float*, const float*, const void*,
                   const void*, void*, void*, int, int, float, uint64_t, float*, int, float*, void*,
                   int, float*, void*, int, float*, void*, int, const void*, hipStream_t);
void fx_coltile_partial(int, int, const void*, const void*, const float*, const float*, float*,
                        float*, int, int, int, hipStream_t, int*, float*, void*, int, float*,
                        void*, int);
void fx_coltile_finalize(int, const float*, int, int, float*, void*, int, hipStream_t);
void fx_bias_gelu_fwd(int, int, const void*, const void*, void*, long, int, hipStream_t);
void fx_bias_gelu_bwd(int, int, const void*, const void*, const void*, void*, float*, int, int, int,
                      hipStream_t, int*, float*, void*, int);
void fx_bias_dropout_add_fwd(int, const void*, const void*, const void*, void*, long, int, float,
                             uint64_t, const void*, hipStream_t);
void fx_dropout_bwd_colsum(int, const void*, void*, float*, int, int, int, float, uint64_t,
                           const void*, hipStream_t, int*, float*, void*, int);
void fx_dropout_fwd(int, const void*, void*, long, float, uint64_t, const void*, hipStream_t);
void fx_ce_stats(int, const void*, const int64_t*, int, int, long, float*, float*, float*, int,
                 hipStream_t);
void fx_ce_bwd(int, const void*, void*, const int64_t*, const float*, const float*, int, int, long,
               int, hipStream_t);
int fx_sumsq_blocks(long n);
void fx_sumsq_f32(const float*, long, float*, int, hipStream_t);
void fx_sumsq_16(int, const void*, long, float*, int, hipStream_t);
void fx_sumsq_chunks(const int64_t*, const int64_t*, int, float*, hipStream_t);
// flags: bit 0 = 16-bit gradient, bit 1 = packed master (master = the low
// halves, p16 = the bf16 parameters; bf16 only, else -1 and no launch).
// lr_dev: device learning rate (null = lr).  grid_cap > 0 caps the workgroups;
// wide = 1024-thread blocks x 4 groups, else 256 x 2; nt = non-temporal accesses.
int fx_adamw(int dtype, int flags, void* master, const void* grad, float* m, float* v, void* p16,
             long n, float lr, float beta1, float beta2, float eps, float wd, float l2,
             const float* gscale, const int* skip, const int* step, const float* lr_dev,
             int grid_cap, int nt, int wide, hipStream_t st);
void fx_pk_split(const float*, void*, void*, long, hipStream_t);
void fx_pk_join(const void*, const void*, float*, long, hipStream_t);
void fx_cast_f32(int, const float*, void*, long, hipStream_t);
void fx_accum_f32(int, float*, const void*, long, int, hipStream_t);
void fx_embedding_fwd(int, const int64_t*, const int64_t*, const void*, const void*, void*, int,
                      int, long, long, hipStream_t);
void fx_embedding_bwd(int, const int64_t*, const void*, float*, int, int, long, long,
                      hipStream_t);
int fx_fa_lab();
int fx_fa_set_stamps(void*);
int fx_flash_fwd(int, const void*, const void*, const void*, void*, float*, const long*, const long*,
                 const long*, const long*, const int*, const float*, long, int, int, int, int, int,
                 int, float, float, uint64_t, const void*, hipStream_t);
int fx_flash_fwd_qoff(int, const void*, const void*, const void*, void*, float*, const long*,
                      const long*, const long*, const long*, const int*, const int*, int, int, int,
                      int, int, float, hipStream_t);
int fx_flash_bwd(int, const void*, const void*, const void*, const void*, const void*, const float*,
                 float*, void*, void*, void*, const long*, const long*, const long*, const long*,
                 const long*, const long*, const int*, const float*, long, int, int, int, int, int,
                 int, float, float, uint64_t, const void*, hipStream_t);
int fx_fake_quant_fwd(int, const void*, void*, const float*, int, long, hipStream_t);
void fx_absmax(int, const void*, long, float*, hipStream_t);
int fx_gn_nseg(long, long);
int fx_gn_fwd(int, const void*, const float*, const float*, const float*, const float*, void*,
              double*, float*, float*, int, int, int, long, int, float, int, hipStream_t);
int fx_gn_bwd_reduce(int, const void*, const void*, const float*, const float*, const float*,
                     const float*, const float*, const float*, float*, int, int, int, long, int,
                     int, hipStream_t);
int fx_gn_bwd_apply(int, const void*, const void*, const float*, const float*, const float*,
                    const float*, const float*, const float*, const float*, const float*, void*,
                    int, int, int, long, int, int, hipStream_t);
int fx_transpose16(int, const void*, void*, float*, int, int, long, long, hipStream_t);
int fx_sample(int, const void*, long, int, int, float, int, float, const float*, int64_t*, float*,
              float*, hipStream_t);
int fx_select(const float* logits, long ld_row, int B, int V, int sampling, float inv_temp,
              int top_k, float top_p, const float* u, int n_steps, int eos, int pad, int min_len,
              float pen, float inv_pen, int bos, int feos, int feos_step, unsigned int* seen,
              int words, int* step, int* unfinished, int* finish_len, float* scores,
              int64_t* out, int64_t* nxt, int64_t* cur, const int64_t* lens, hipStream_t,
              const int64_t* seed);
int fx_coupled_sample(const float* logits, long ld_row, int R, int V, float inv_temp, int top_k,
                      float top_p, const int* steps, const int* rows, const int64_t* seed,
                      int64_t* out_ids, float* out_lse, hipStream_t);
int fx_spec_verify(const float* logits, long ld_row, int B, int W, int V, int n_steps, int eos,
                   int pad, int min_len, float pen, float inv_pen, int feos, int feos_step,
                   unsigned int* seen, int words, int* step, int* unfinished, int* finish_len,
                   float* scores, int64_t* out, int64_t* nxt, int64_t* cur, int64_t* tok,
                   int64_t* pos, int* wlens, int* picks, float* logp, int* rounds, int* accepted,
                   int* any_active, hipStream_t, int coupled, float inv_temp, int top_k,
                   float top_p, const int64_t* seed);
int fx_decode_attn(int, const void*, const void*, const void*, void*, const int*, int, int, int,
                   int, int, float*, long, long, long, long, long, long, float, hipStream_t);
int fx_beam_decode_attn(int, const void*, const void*, const void*, const int*, const void*,
                        const void*, const int*, const int*, void*, float*, int, int, int, int, int,
                        int, int, long, long, long, long, long, long, long, long, long, long, float,
                        int, hipStream_t);
int fx_window_decode_attn(int, const void*, const void*, const void*, const int*, void*, float*,
                          int, int, int, int, int, int, long, long, long, long, long, long, float,
                          int, hipStream_t);
void fx_embedding_bwd_sorted(int, const int64_t*, const int64_t*, const void*, float*, int, int,
                             long, long, hipStream_t);
int fx_softmax_fwd(int, int, const void*, const void*, void*, long, int, int, long, float, int,
                   hipStream_t);
int fx_softmax_bwd(int, const void*, const void*, void*, long, int, int, float, int, hipStream_t);
int fx_gemm(int, int, int, int, int, int, int, const void*, long, const void*, long, void*, long,
            const void*, void*, long, int, hipStream_t, float*, float*);
long fx_gemm_ws_bytes(int, int, int, int);
void fx_gemm_set_gm(int);
void fx_gemm_set_geom(int, int);
int fx_gemm_tuned(long*, int);
void fx_gemm_set_tuned(int, int, int, int, int, int, int);
void fx_gemm_set_tune(int);
void fx_gemm_set_persist(int);
void fx_gemm_set_xrect(int);
int fx_decode_gemv(int, int, int, int, int, const void*, long, const void*, long, const void*,
                   const void*, long, void*, long, void*, void*, const long*, const int*, int, int, int,
                   const void*, const void*, float, hipStream_t);
int fx_decode_gemv_w8(int, int, int, int, int, const void*, long, const int8_t*, long, const float*,
                      const void*, const void*, long, void*, long, void*, void*, const long*, const int*, int,
                      int, int, const void*, const void*, float, hipStream_t);
int fx_decode_gemv_w4(int, int, int, int, int, const void*, long, const uint8_t*, long, const float*,
                      const void*, const void*, long, void*, long, void*, void*, const long*, const int*, int,
                      int, int, const void*, const void*, float, hipStream_t);
hipStream_t fx_cumask_stream_create(int, int*);
int fx_stream_destroy(hipStream_t);
int fx_comm_max_world();
int fx_comm_max_blocks();
void* fx_comm_alloc(long);
int fx_comm_free(void*);
int fx_comm_ipc_handle(void*, char*);
void* fx_comm_ipc_open(const char*);
int fx_comm_ipc_close(void*);
int fx_comm_allreduce(int, int, const void*, void*, long, int, int, const uint64_t*, unsigned int*,
                      unsigned int*, long, unsigned long long, hipStream_t);
}
