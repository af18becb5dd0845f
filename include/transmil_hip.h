/* C ABI of libtransmil_hip.so -- the MI355X (gfx950) TransMIL hot path.
 *
 * The reference has no native boundary: its plugin surface is Python
 * (`models.TransMIL` imported by ModelInterface.load_model,
 * code/models/model_interface.py:1256-1293, and the third-party
 * `nystrom_attention.NystromAttention`, code/models/TransMIL.py:5,26-34,47).
 * This ABI is what the drop-in Python module (transmil_deepgraft_amd/models/
 * TransMIL.py and transmil_deepgraft_amd/nystrom_attention.py) binds through
 * ctypes; each entry point below names the reference op it replaces.
 *
 * Conventions (all entry points):
 *   - device pointers are caller-owned; nothing is allocated inside;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream);
 *   - no host synchronisation, so every call is hipGraph-capturable -- with ONE documented
 *     exception, tm_conv1x1_tune (a host-timed algorithm search, refused during capture);
 *   - deterministic: no float atomics, fixed reduction orders -- every result is a function of
 *     the inputs alone, with ONE documented exception: tm_conv1x1 after tm_conv1x1_tune runs the
 *     algorithm the tune call timed fastest IN THIS PROCESS, so two processes that tuned may
 *     round the C5 encoder features differently (the Python encoder skips the tune under
 *     torch.use_deterministic_algorithms(True) or TM_CONV1X1_TUNE=0: heuristic first choice);
 *   - return 0 on success, 1 on a bad argument, 2 on a launch error;
 *     tm_last_error() returns the thread-local message.
 *   - dtype enum: TM_F32 = 0, TM_BF16 = 1 (activations / MFMA operands).
 */
#ifndef TRANSMIL_HIP_H
#define TRANSMIL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors / build info ---------------------------------------------- */
const char* tm_last_error(void);
const char* tm_build_info(void);

/* ---- dense GEMM with fused epilogues (gemm.hip) -----------------------
 * C[m,n] = epi(alpha * sum_k A(m,k) B(k,n)),
 *   A(m,k) = a_trans ? A[k*lda+m] : A[m*lda+k];  B(k,n) = b_kn ? B[k*ldb+n] : B[n*ldb+k].
 * Replaces the nn.Linear call sites of _fc1 (code/models/TransMIL.py:128-133),
 * NystromAttention.to_qkv / to_out (SURVEY.md App. A eq. 2, 10) and their
 * backward products. */
enum { TM_EPI_PLAIN = 0, TM_EPI_QKV = 1, TM_EPI_SPLITK = 2 };
typedef struct tm_gemm_args {
  int M, N, K;
  int lda, ldb, ldc;
  int a_trans, b_kn;
  int ab_dtype, c_dtype;
  int splits, k_per_split;
  int mode;            /* TM_EPI_* */
  float alpha;
  const float* bias;   /* [N] fp32 or NULL */
  int gelu;            /* exact erf GELU after bias */
  void* pre;           /* pre-activation store (c_dtype), row m, ld_pre; or NULL */
  int ld_pre;
  float drop_p, drop_scale;
  uint64_t seed;
  const float* resid;  /* fp32 residual added last, indexed like C; or NULL */
  int accumulate;      /* C += result */
  /* output row map (grp_in > 0): bag = m / grp_in, t = m % grp_in - skip;
   * t < 0 -> not stored; row = bag*grp_out + out_off + t; if t < dup_n also
   * stored at bag*grp_out + dup_off + t (TransMIL grid padding, :177-180) */
  int grp_in, skip, grp_out, out_off, dup_n, dup_off;
  /* TM_EPI_QKV: m = bag*seq + t, n = which*(nh*dh) + head*dh + d ->
   * C[((which*nbags + bag)*nh + head)*seq + t][d]; q (which==0) scaled by qscale */
  int nbags, nh, dh, seq;
  float qscale;
  /* dropout seed read from device memory when non-NULL: seed = *seed_ptr * 0x9E3779B97F4A7C15 + seed
   * (keeps a hipGraph replay drawing a fresh mask every step) */
  const uint64_t* seed_ptr;
  /* bf16 weight-gradient split-K (a_trans = 1, TM_EPI_SPLITK, K and k_per_split multiples of 64)
   * only, else NULL: colsum[z][m] = sum over split z's k of A[k][m] (the bias gradient of the same
   * dY, summed by the workgroups of the first column tile while they stage A) -- [splits][M] fp32 */
  float* colsum;
  /* 1: the pre-activation store (pre) is bf16 whatever c_dtype (the bf16 step's _fc1: the GELU
   * backward reads it back in bf16, tm_fc1_gelu_bwd with TM_BF16); 0: c_dtype */
  int pre_bf16;
  /* TM_EPI_SPLITK with bf16 operands: 1 = the split slabs are written bf16 (each split's partial
   * rounded once; tm_splitk_reduce_bf16 sums them in fp32); 0: fp32 slabs (c_dtype TM_F32) */
  int slab_bf16;
} tm_gemm_args;

int tm_gemm(const void* A, const void* B, void* C, const tm_gemm_args* args, void* stream);
/* Two independent products as ONE launch.  Between tm_gemm_pair_begin(stream) and
 * tm_gemm_pair_end(stream) the calling thread's tm_gemm calls on that stream (two at most) are
 * checked as usual but only held (pointers and a copy of the arguments: the caller keeps owning
 * every buffer, which must stay valid until `end` returns); `end` launches them.  A bf16 split-K
 * weight gradient (a_trans = b_kn = 1, TM_EPI_SPLITK) and a bf16 plain data gradient (a_trans = 0,
 * b_kn = 1, no split, plain epilogue), in either call order, both on the 128 x 128 ring (K and
 * k_per_split multiples of 64, the k-strided extents multiples of 8), run as one grid of the same
 * tiles: every output bit-identical to the separate launches.  Anything else held (one call, a
 * shape off the ring, fp32 operands, another epilogue) is launched separately in call order; no
 * call held: `end` does nothing.  The caller asserts that neither product reads the other's output,
 * and issues nothing else that launches on `stream` between begin and end (reductions deferred to a
 * tm_reduce_queue are fine: they launch at the flush).
 * The held state is host-side and per calling THREAD (one open pair per thread, bound to the stream
 * given to begin; tm_gemm calls on other streams launch at once).  An error at begin (a pair already
 * open), at a held tm_gemm (bad arguments, a third call) or at end (another stream) closes the pair
 * and drops what was held: nothing stays held after a non-zero return, and an `end` that finds no
 * open pair returns 0.  No device state, no synchronisation: capturable like tm_gemm. */
int tm_gemm_pair_begin(void* stream);
int tm_gemm_pair_end(void* stream);
/* Deferred parameter-gradient reductions. A tm_reduce_queue is a caller-owned host object
 * (no device memory, no stream): every entry point below that ends in a split-K / slab sum takes
 * `tm_reduce_queue* rq`.  rq == NULL launches the sum now on `stream`; otherwise the (slab, out)
 * pair is only appended to *rq, and tm_reduce_flush(rq, stream) sums every queued pair in ONE
 * launch (same fixed split order, so bit-identical to the immediate form).  The library keeps no
 * deferral state of its own: two engines on two streams, or two threads, each pass their own
 * queue.  A queue must not be used by two threads at once; nothing may read a queued output (or
 * free its slab) before the flush.  A full queue (48 entries) is flushed on the appending call's
 * stream.  Replaces the DDP-reducer-era fixed-bucket gradient pass (code/train.py:184). */
typedef struct tm_reduce_queue tm_reduce_queue;
tm_reduce_queue* tm_reduce_queue_create(void);          /* NULL + tm_last_error() on failure */
void tm_reduce_queue_destroy(tm_reduce_queue* rq);      /* entries still queued are dropped */
int tm_reduce_queue_pending(const tm_reduce_queue* rq); /* queued entries, -1 if rq is invalid */
int tm_reduce_flush(tm_reduce_queue* rq, void* stream);
int tm_splitk_reduce(const float* slab, float* out, int splits, long long count, float alpha,
                     int accumulate, tm_reduce_queue* rq, void* stream);
/* the same over bf16 slabs (tm_gemm_args.slab_bf16): the splits summed in fp32 in index order */
int tm_splitk_reduce_bf16(const void* slab, float* out, int splits, long long count, float alpha,
                          int accumulate, tm_reduce_queue* rq, void* stream);
long long tm_colsum_workspace(int rows, int cols, int rows_per_chunk);
int tm_colsum(const void* X, int dtype, int rows, int cols, int ld, int rows_per_chunk,
              float* work, float* out, int accumulate, tm_reduce_queue* rq, void* stream);

/* ---- LayerNorm / head (layernorm.hip) ----------------------------------
 * TransLayer.norm (code/models/TransMIL.py:23,47) and the final norm + _fc
 * head (:154-155, 202-204).  x rows are [B*S, D] fp32; y is written into the
 * front-padded [B, n_pad, D] layout (rows b*n_pad + pad + i; pad rows zeroed). */
int tm_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, int rows, int D,
                     int S, int n_pad, int pad, int dtype, void* y, float* mean, float* rstd, void* stream);
long long tm_layernorm_bwd_workspace(int rows, int D, int rows_per_block);
/* dx_accum[r] += LN'(dy) (dy read from the padded layout); dgamma/dbeta written */
/* resid_cls_only != 0: dx_accum holds the residual gradient only at the class rows (row % S == 0);
 * the other rows are written (=) without being read (the last layer's dL/dH, clsrow.hip) */
int tm_layernorm_bwd(const void* dy, int dtype, const float* x, const float* gamma, const float* mean,
                     const float* rstd, int rows, int D, int S, int n_pad, int pad, int rows_per_block,
                     int resid_cls_only, float* dx_accum, float* work, float* dgamma, float* dbeta,
                     tm_reduce_queue* rq, void* stream);
/* tm_layernorm_bwd with a per-segment addend on dy: row t of bag b reads dy + seg_add[b][(pad + t) /
 * seg_len] (+ seg_add[b][nseg] at t = 0, the class row); seg_add is [B][seg_rows][D] fp32 (the
 * scale * Aq Wq rows of tm_cls_q_rows' products, seg_rows = 288, nseg = 256) */
int tm_layernorm_bwd_seg(const void* dy, int dtype, const float* x, const float* gamma, const float* mean,
                         const float* rstd, int rows, int D, int S, int n_pad, int pad, int rows_per_block,
                         int resid_cls_only, const float* seg_add, int seg_len, int nseg, int seg_rows,
                         float* dx_accum, float* work, float* dgamma, float* dbeta, tm_reduce_queue* rq,
                         void* stream);
int tm_head_fwd(const float* h, int B, int S, int D, const float* gamma, const float* beta, float eps,
                const float* W, const float* bias, int C, float* logits, float* xhat, float* rstd,
                void* stream);
/* writes dh[b*S*D + :D] (row 0 of each bag); other rows untouched */
int tm_head_bwd(const float* dlogits, int B, int C, int S, int D, const float* xhat, const float* rstd,
                const float* gamma, const float* beta, const float* W, float* dW, float* dbias,
                float* dgamma, float* dbeta, float* dh, void* stream);
/* The training step's head and loss in one launch each way (replaces tm_head_fwd + tm_ce_fwd and
 * tm_ce_bwd + tm_head_bwd on the fused TransMILTask path): forward = tm_head_fwd, then
 * CrossEntropyLoss(logits, one_hot(label).float()) / Y_prob / Y_hat / class stats as tm_ce_fwd
 * (code/models/model_interface.py:339-356); backward: dlogits = gloss (prob - one_hot) / B
 * (+ dlogits_in, nullable), then tm_head_bwd.  scratch: B*C floats (may be null if B == 1, C <= 4). */
int tm_head_ce_fwd(const float* h, int B, int S, int D, const float* gamma, const float* beta, float eps,
                   const float* W, const float* bias, int C, const long long* label, float* logits, float* xhat,
                   float* rstd, float* loss, float* prob, long long* yhat, int* class_stats, void* stream);
int tm_head_ce_bwd(const float* prob, const long long* label, const float* gloss, const float* dlogits_in, int B,
                   int C, int S, int D, const float* xhat, const float* rstd, const float* gamma,
                   const float* beta, const float* W, float* dW, float* dbias, float* dgamma, float* dbeta,
                   float* dh, float* scratch, void* stream);

/* ---- NystromAttention core (nystrom.hip) --------------------------------
 * SURVEY.md App. A eq. 4-9 of the third-party nystrom_attention package
 * (call site code/models/TransMIL.py:47).  dim_head = 64, 256 landmarks.
 * q/k/v: [B*h, n, 64] (T), n a multiple of 256; landmarks [B*h, 256, 64]. */
int tm_nys_landmarks(int dtype, const void* q, const void* k, int nbh, int n, float* ql, float* kl,
                     void* ql_t, void* kl_t, void* stream);
int tm_nys_sim2_softmax(const float* ql, const float* kl, int nbh, float* a2, void* stream);
int tm_softmax_bwd_rows256(const float* a, const float* da, float* ds, int rows, void* stream);
long long tm_nys_a3_workspace(int nbh, int n);
/* W = softmax(ql k^T) v  [B*h,256,64] fp32, lse3 [B*h,256] */
/* bf16: w = lse3 = NULL leaves the tm_nys_a3_partials(nbh, n) key-split partials in work for
 * tm_pinv_fwd_split_a3 to combine */
long long tm_nys_a3_partials(int nbh, int n);
int tm_nys_a3_fwd(int dtype, const float* ql, const void* k, const void* v, int nbh, int n, float* work,
                  float* w, float* lse3, void* stream);
/* bf16 only: tm_nys_a3_fwd(TM_BF16, ..., w = NULL, lse3 = NULL) and tm_nys_sim2_softmax_split(ql, kl,
 * nbh, a2, a2s) in ONE launch (the A3 workgroups also write the A2 rows, bit-identical to the
 * separate kernel; two launches where the key split does not tile the 256 rows).  Both replace
 * NystromAttention.forward's attn2 / attn3 softmaxes (code/models/TransMIL.py:47; App. A eq. 5-6). */
int tm_nys_a3_fwd_sim2(const float* ql, const float* kl, const void* k, const void* v, int nbh, int n,
                       float* work, float* a2, void* a2s, void* stream);
/* merged[b][t][head*64+d] = softmax(q kl^T) y + conv33(v); lse1 [B*h, n]; kl_t, y_t: T copies */
int tm_nys_a1_fwd(int dtype, const void* q, const void* v, const void* kl_t, const void* y_t,
                  const float* wconv, int nbh, int nh, int n, void* merged, float* lse1, void* stream);
int tm_cast_f32(int dtype, const float* x, void* y, long long count, void* stream);
long long tm_nys_conv_bwd_workspace(int nbags, int nh, int n);
/* dv [B*h, n, 64] in the step's dtype T (bf16 in the bf16 mode: the fused A3 backward reads it once) */
int tm_nys_conv_bwd(int dtype, const void* dmerged, const void* merged, const void* v, const float* wconv,
                    int nbh, int nh, int n, void* dv, float* d1, float* work, float* dwconv,
                    tm_reduce_queue* rq, void* stream);
long long tm_nys_a1_bwd_workspace(int nbh, int n, int queries_per_wg);
/* A1 product backward: dq [B*h, n, 64] fp32 written, dkl / dy [B*h, 256, 64] from per-workgroup
 * partial slabs in work.  queries_per_wg: a multiple of 32 that divides n; the fp32 kernel gives each
 * workgroup that many query rows, the bf16 kernel splits the rows evenly itself and stages at most
 * 256 per workgroup, so TM_BF16 with queries_per_wg > 256 is refused (returns 1). */
int tm_nys_a1_bwd(int dtype, const void* q, const void* dmerged, const void* kl_t, const void* y_t,
                  const float* lse1, const float* d1, int nbh, int nh, int n, int queries_per_wg,
                  float* dq, float* work, float* dkl, float* dy, int accumulate, tm_reduce_queue* rq,
                  void* stream);
/* bf16 only: tm_nys_a1_bwd with dq written as bf16(dq_scale * dq) into the q part of dqkv
 * ([B][n][3*nh*64], bf16, the columns of each head) instead of fp32 [B*h][n][64] rows (half the
 * bytes, no fp32 round trip); tm_nys_assemble_q_slab_inplace then adds the landmark term there. */
int tm_nys_a1_bwd_dqkv(const void* q, const void* dmerged, const void* kl_t, const void* y_t, const float* lse1,
                       const float* d1, int nbh, int nh, int n, void* dqkv, float dq_scale, float* work, float* dkl,
                       float* dy, tm_reduce_queue* rq, void* stream);
long long tm_nys_a3_bwd_workspace(int nbh, int n);
/* d3 (here and in tm_nys_a3_bwd_fused): D = rowsum(dW o W) as [2][B*h][256] partials, the two
 * 32-column halves of dW (tm_bmm_job.Rd of the dW = Z^T dY product); the kernels sum them */
int tm_nys_a3_bwd(int dtype, const void* ql_t, const void* dw_t, const void* k, const void* v,
                  const float* lse3, const float* d3, int nbh, int nh, int n, float* dk, float* dv,
                  float* work, float* dql, int accumulate, tm_reduce_queue* rq, void* stream);
/* Row `row` of the return_attn product attn1 Z attn3 (App. A eq. 11; read by
 * code/visualize_mil.py:580-581 as cls_attention[0,:,padding+1,...]) for every bag and
 * head, without the [n, n] matrix: out [B*h, n] fp32 from the forward's q, k (T, q
 * pre-scaled), ql / kl [B*h,256,64], Z [B*h,256,256] and lse3 [B*h,256] (fp32). */
int tm_nys_attn_row(int dtype, const void* q, const void* k, const float* ql, const float* kl, const float* z,
                    const float* lse3, int nbh, int n, int row, float* out, void* stream);
int tm_nys_assemble_dqkv(int dtype, const float* dq, const float* dql, const float* dk, const float* dkl,
                         const float* dv, int nbags, int nh, int n, float scale, void* dqkv, void* stream);
/* bf16 mode, fused key side: the A3 backward writes the final bf16 k / v parts of dqkv
 * (k = dK + dk~[t/l]/l, v = dv_conv + dV) and dql (=) from its slabs; then tm_nys_assemble_q_slab
 * writes the q part, scale * (dq + (dql + sum_p slab[p])[t/l]/l).  dv_conv (bf16, as tm_nys_conv_bwd /
 * tm_cls_a1_row_bwd write it in the bf16 mode) is read only for rows
 * [dv_lo, dv_hi) (zero elsewhere; 0, n = dense); dq_row >= 0: dq is zero outside that row.
 * dql = NULL: the dq~ partial slab is left in work ([tm_nys_a3_bwd_slabs][B*h][256][64] bf16, each
 * partial rounded once; the consumers sum them in fp32) for tm_nys_assemble_q_slab, which reduces it
 * while writing the q part (one launch fewer). */
int tm_nys_a3_bwd_fused(const void* ql_t, const void* dw_t, const void* k, const void* v, const float* lse3,
                        const float* d3, int nbh, int nh, int n, const void* dv_conv, int dv_lo, int dv_hi,
                        const float* dkl, float* work, float* dql, void* dqkv, tm_reduce_queue* rq,
                        void* stream);
/* partial slabs the bf16 A3 backward writes (tm_nys_a3_bwd_fused's work) */
int tm_nys_a3_bwd_slabs(int nbh, int n);
/* q part of dqkv, scale * (dq + (dql + sum_p slab[p])[t/l]/l), the slab sum in the same launch
 * (nh <= 8; slab [slabs][nbags*nh][256][64] bf16 as tm_nys_a3_bwd_fused(dql = NULL) leaves it) */
int tm_nys_assemble_q_slab(int dtype, const float* dq, int dq_row, const float* dql, const void* slab, int slabs,
                           int nbags, int nh, int n, float scale, void* dqkv, void* stream);
/* bf16, after tm_nys_a1_bwd_dqkv: q += scale * (dql + sum_p slab[p])[t/l]/l in place in dqkv */
int tm_nys_assemble_q_slab_inplace(const float* dql, const void* slab, int slabs, int nbags, int nh, int n,
                                   float scale, void* dqkv, void* stream);

/* ---- geometry-generic NystromAttention core, fp32 (nystrom_geo.hip) --------
 * The same stages as the tm_nys_* / tm_pinv_* entry points above for the TransMIL widths other than
 * 512: (dh, nl) = (dim_head, landmarks) in {(32, 128), (48, 192)} (out_features 256 / 384; TransLayer
 * builds dim_head = dim / 8, landmarks = dim / 2, code/models/TransMIL.py:26-31).  fp32 operands,
 * fp32 FMA arithmetic and accumulation; q, k, v [B*h][n][dh] (q pre-scaled), landmarks / W / Y
 * [B*h][nl][dh], A2 / Z [B*h][nl][nl], merged / dmerged [B][n][h*dh]; n a positive multiple of nl.
 * Every entry point refuses an unsupported (dh, nl), a bad n and null pointers before any device
 * work; the *_workspace / *_floats queries return -1 for them.  (64, 256) stays on the entry points
 * above. */
int tm_nysg_landmarks(int dh, int nl, const float* q, const float* k, int nbh, int n, float* ql, float* kl,
                      void* stream);
long long tm_nysg_a3_workspace(int dh, int nl, int nbh, int n);   /* bytes */
/* W = softmax(ql k^T) v [B*h][nl][dh] and lse3 [B*h][nl], key-split in blocks of nl keys */
int tm_nysg_a3_fwd(int dh, int nl, const float* ql, const float* k, const float* v, int nbh, int n, float* work,
                   float* w, float* lse3, void* stream);
int tm_nysg_sim2_softmax(int dh, int nl, const float* ql, const float* kl, int nbh, float* a2, void* stream);
int tm_nysg_softmax_bwd_rows(int dh, int nl, const float* a, const float* da, float* ds, long long rows,
                             void* stream);
long long tm_nysg_pinv_saved_floats(int dh, int nl, int nbh, int iters);
/* as tm_pinv_fwd (prec 0): the abs-sum maxima are taken over ALL bags and heads; iters >= 1 */
int tm_nysg_pinv_fwd(int dh, int nl, const float* X, int nbh, int iters, float* saved, void* stream);
long long tm_nysg_pinv_bwd_workspace_floats(int dh, int nl, int nbh);
int tm_nysg_pinv_bwd(int dh, int nl, const float* X, int nbh, int iters, const float* saved, float* dZ,
                     float* work, float* dX, void* stream);
/* C = op(A) B + e1 E1 per head: A [nl][nl] (ta = 1: transposed), B, C, E1 (or NULL) [nl][dh]:
 * Y = Z W, dW = Z^T dY, dq~ = dS2 k~ + dq~3, dk~ = dS2^T q~ + dk~ */
int tm_nysg_mm(int dh, int nl, const float* A, int ta, const float* B, const float* E1, float e1, float* C,
               int nbh, void* stream);
/* merged = softmax(q kl^T) y + conv33(v) (fp32 [B][n][h*dh]), lse1 [B*h][n] */
int tm_nysg_a1_fwd(int dh, int nl, const float* q, const float* v, const float* kl, const float* y,
                   const float* wconv, int nbh, int nh, int n, float* merged, float* lse1, void* stream);
long long tm_nysg_conv_bwd_workspace(int dh, int nl, int nbags, int nh, int n);   /* bytes */
int tm_nysg_conv_bwd(int dh, int nl, const float* dmerged, const float* merged, const float* v,
                     const float* wconv, int nbh, int nh, int n, float* dv, float* d1, float* work,
                     float* dwconv, tm_reduce_queue* rq, void* stream);
long long tm_nysg_a1_bwd_workspace(int dh, int nl, int nbh, int n);   /* bytes */
/* dq (=) [B*h][n][dh]; dkl, dy (=) [B*h][nl][dh] summed from the workspace's slabs (deferred into rq) */
int tm_nysg_a1_bwd(int dh, int nl, const float* q, const float* dmerged, const float* kl, const float* y,
                   const float* lse1, const float* d1, int nbh, int nh, int n, float* dq, float* work,
                   float* dkl, float* dy, tm_reduce_queue* rq, void* stream);
long long tm_nysg_a3_bwd_workspace(int dh, int nl, int nbh, int n);   /* bytes */
/* dk (=), dv (+=: it holds the conv backward's dv) [B*h][n][dh]; dql (=) from the slabs;
 * D = rowsum(dw o w) is computed by the kernel */
int tm_nysg_a3_bwd(int dh, int nl, const float* ql, const float* dw, const float* w, const float* k,
                   const float* v, const float* lse3, int nbh, int n, float* dk, float* dv, float* work,
                   float* dql, tm_reduce_queue* rq, void* stream);
/* dqkv [B][n][3*h*dh] in `dtype` as tm_nys_assemble_dqkv */
int tm_nysg_assemble_dqkv(int dh, int nl, int dtype, const float* dq, const float* dql, const float* dk,
                          const float* dkl, const float* dv, int nbags, int nh, int n, float scale, void* dqkv,
                          void* stream);
/* tm_nys_attn_row for this family (fp32 q, k) */
int tm_nysg_attn_row(int dh, int nl, const float* q, const float* k, const float* ql, const float* kl,
                     const float* z, const float* lse3, int nbh, int n, int row, float* out, void* stream);

/* ---- exact softmax attention (attention.hip) ------------------------------
 * TransformerMIL's ViT blocks (code/models/_transformer.py:33-43): softmax(q k^T * scale) v, dh = 64,
 * no mask, not causal, no dropout on the probabilities.  q, k, v, out, dout, dqkv are fp32 in memory.
 * Element (b, t, h, d) of q / k / v is at base[(b*n + t)*row_stride + h*64 + d], so the packed to_qkv
 * output [B, n, 3*H*64] is passed as three base pointers with row_stride = 3*H*64.
 * compute = TM_F32: fp32 MFMA products (exact fmaf chains).  TM_BF16: operands rounded to bf16 while
 * they are staged, bf16 MFMA, fp32 accumulation; fp32 softmax statistics in both.
 * out [B, n, H*64] (heads merged, what to_out reads), lse [B*H, n] = log sum_j exp(scale * q.k_j).
 * Online softmax over 64-key chunks: no n x n matrix is written, any n >= 1.  Arguments are checked
 * before any device work (n, B, H > 0, B*H <= 65535, row_stride >= H*64 and a multiple of 4, pointers
 * non-null and 16-byte aligned). */
int tm_attn_fwd(int compute, const float* q, const float* k, const float* v, int B, int H, int n,
                long long row_stride, float scale, float* out, float* lse, void* stream);
/* bytes of tm_attn_bwd's work: D = rowsum(dout o out) as [B*H, n] fp32, linear in B*H*n */
long long tm_attn_bwd_workspace(int B, int H, int n);
/* dqkv [B, n, 3*H*64] packed (written, not accumulated): the dY that to_qkv's backward GEMMs read.
 * P = exp(scale*S - lse) is recomputed; dV = P^T dout and dK = scale * dS^T q come from a pass that owns
 * its key rows, dQ = scale * dS k from a pass that owns its query rows: no atomics, one writer and one
 * summation order per element. */
int tm_attn_bwd(int compute, const float* q, const float* k, const float* v, const float* out,
                const float* lse, const float* dout, int B, int H, int n, long long row_stride,
                float scale, void* work, float* dqkv, void* stream);

/* ---- pseudo-inverse + small fp32 batched products (pinv.hip) -------------
 * moore_penrose_iter_pinv of nystrom_attention (App. A eq. 7).
 * C = diag*I + alpha*(op(A) op(B) [+ op(A2) op(B2)]) + e1*E1 + e2*E2, batched;
 * op(X) = X^T when the t-flag is set; E1/E2 share C's layout. */
typedef struct tm_bmm_job {
  const float* A; const float* B; int ta, tb; int lda, ldb; long long sa, sb;
  const float* A2; const float* B2; int ta2, tb2; int lda2, ldb2; long long sa2, sb2;
  const float* E1; float e1; const float* E2; float e2;
  float alpha, diag;
  float* C; int ldc; long long sc;
  int M, N, K;
  /* optional second output of the same product (C's layout): C2 = c2_alpha*(products)
   * + c2_diag*I + c2_e1*E1 (null: none) */
  float* C2; float c2_alpha, c2_diag, c2_e1;
  /* optional bf16 form of C (C's layout, written beside it): ct_mode 1 = bf16(C) at Ct,
   * 2 = split planes hi = bf16(C) at Ct and lo = bf16(C - hi) at Ct + ct_plane elements
   * (the operand format of tm_pinv_bwd_split), 0 = none */
  void* Ct; long long ct_plane; int ct_mode; int ct_reserved;
  /* optional partial row dots of C with Rw (C's layout), one per 32-column tile:
   * Rd[(n / 32) * nbatch + b][m] = sum over that tile's columns of C[b][m][n] * Rw[b][m][n]
   * (null: none).  D = rowsum(dW o W) of the A3 backward as N / 32 = 2 partials. */
  float* Rd; const float* Rw;
} tm_bmm_job;
/* prec 0: exact fp32 MFMA; prec 1: bf16x3 (hi/lo split, ~16-bit operands, fp32 accumulate) */
int tm_bmm(const tm_bmm_job* jobs, int njobs, int nbatch, int prec, void* stream);
long long tm_pinv_saved_floats(int nbh, int iters);
int tm_pinv_fwd(const float* X, int nbh, int iters, int prec, float* saved, void* stream);
long long tm_pinv_bwd_workspace_floats(int nbh);
int tm_pinv_bwd(const float* X, int nbh, int iters, int prec, const float* saved, float* dZ, float* work,
                float* dX, void* stream);

/* ---- pseudo-inverse on split operands, bf16 (bench) mode (pinv_split.hip) --
 * Same function as tm_pinv_fwd / tm_pinv_bwd with prec 1, restructured for MI355X: every chain
 * matrix is kept as bf16 hi / lo planes (hi = bf16(M), lo = bf16(M - hi); the lo plane follows the
 * hi plane at + nbh*256*256 elements), products are hi*hi + hi*lo + lo*hi on the bf16 MFMA with
 * fp32 accumulation, 64x64 output tiles fed by LDS-DMA; 14 launches forward.
 * A2 = softmax(ql kl^T) with its split planes (replaces tm_nys_sim2_softmax on this path): */
int tm_nys_sim2_softmax_split(const float* ql, const float* kl, int nbh, float* a2, void* a2s, void* stream);
/* saved: Z_iters fp32 at saved[0 .. nbh*65536), then the split chain matrices, sums and maxima */
long long tm_pinv_split_saved_floats(int nbh, int iters);
int tm_pinv_fwd_split(const float* X, const void* Xs, int nbh, int iters, float* saved, void* stream);
/* tm_pinv_fwd_split with the A3 forward's partial combine in the chain's last launch (its idle CUs):
 * a3_work / a3_parts = the partials tm_nys_a3_fwd(TM_BF16, ..., w = NULL, lse3 = NULL) left,
 * a3_parts = tm_nys_a3_partials(nbh, n); writes W [B*h,256,64] and lse3 [B*h,256] as tm_nys_a3_fwd. */
int tm_pinv_fwd_split_a3(const float* X, const void* Xs, int nbh, int iters, float* saved, const float* a3_work,
                         int a3_parts, float* w, float* lse3, void* stream);
/* work: the gradient w.r.t. Z_iters as split planes at work[0 .. nbh*65536) on entry (tm_split_f32);
 * out = dL/dX (softmax == 0) or the backward of A2 = softmax(.) through X (softmax != 0), fp32 */
long long tm_pinv_bwd_split_workspace_floats(int nbh);
int tm_pinv_bwd_split(const float* X, const void* Xs, int nbh, int iters, const float* saved, float* work,
                      int softmax, float* out, void* stream);
/* fp32 -> split planes: y[i] = bf16(x[i]), y[count + i] = bf16(x[i] - y[i]); count % 8 == 0 */
int tm_split_f32(const float* x, void* y, long long count, void* stream);

/* ---- PPEG (ppeg.hip) -- code/models/TransMIL.py:60-75 -------------------- *
 * wfold [49][D] tap-major (the three depthwise kernels + identity folded into one 7x7), bfold [D] */
int tm_ppeg_fold(const float* w7, const float* b7, const float* w5, const float* b5, const float* w3,
                 const float* b3, int D, float* wfold, float* bfold, void* stream);
/* x, y [B, 1 + G*G, D] fp32, D % 32 == 0; y must not alias x; x, y, wfold, bfold 16-byte aligned */
int tm_ppeg_fwd(const float* x, int B, int G, int D, const float* wfold, const float* bfold, float* y,
                void* stream);
long long tm_ppeg_bwd_workspace(int B, int G, int D);
/* dx (=) must alias neither dy nor x (the weight-gradient blocks read x while the stencil blocks of
 * the same launch write dx); x, dy, dx, wfold, work and dout 16-byte aligned; work and the six
 * gradients are required.
 * dout (nullable): also writes the padded to_out-dropout gradient of the TransLayer below from dx
 * (as tm_dropout_bwd_pad with the same dtype / n_pad / pad / p / seed / seed_ptr: rows [0, pad)
 * zero, rows pad + S .. n_pad - 1 left alone).  The weight
 * gradients (=) are summed from the workspace's slabs by tm_splitk_reduce: deferred into rq when
 * it is non-null (final after tm_reduce_flush), else summed before return */
int tm_ppeg_bwd(const float* x, const float* dy, int B, int G, int D, const float* wfold, float* dx,
                float* work, float* dw7, float* db7, float* dw5, float* db5, float* dw3, float* db3,
                int dtype, void* dout, int n_pad, int pad, float p, uint64_t seed,
                const uint64_t* seed_ptr, tm_reduce_queue* rq, void* stream);

/* ---- AttMIL gated attention pooling (attmil.hip) -- code/models/AttMIL.py:88-110 ----
 * Z [N, 2D] = H [Wv;Wu]^T + [bv;bu] (caller's GEMM), H [N, L], w [D] / b [1] = attention_weights,
 * Wc [C, L] / bc [C] = classifier.  Forward writes a [N] scores, p [N] softmax weights, M [L] pooled
 * bag and logits [C]; backward writes dZ [N, 2D], dH [N, L] = p dM (the caller's GEMM then adds
 * dZ [Wv;Wu]), dM [L], dw [D], db [1], dWc [C, L], dbc [C].  fp32; work sized by the queries. */
long long tm_attmil_fwd_workspace(int N, int L);
int tm_attmil_fwd(const float* Z, const float* H, const float* w, const float* b, const float* Wc,
                  const float* bc, int N, int L, int D, int C, float* work, float* a, float* p, float* M,
                  float* logits, void* stream);
long long tm_attmil_bwd_workspace(int N, int L, int D);
int tm_attmil_bwd(const float* Z, const float* H, const float* w, const float* p, const float* M,
                  const float* Wc, const float* dlogits, int N, int L, int D, int C, float* work,
                  float* dZ, float* dH, float* dM, float* dw, float* db, float* dWc, float* dbc, void* stream);

/* The typed pooling: the same mathematics with Z [N, 2D], H [N, L] and dZ [N, 2D] stored as dtype
 * (TM_F32 or TM_BF16: the model's bf16 compute mode); every other tensor and all arithmetic fp32.
 * Forward (two launches: a row pass of tm_attmil_pool_rows_per_block() rows per workgroup, then the
 * flash-style merge of its block partials) writes a [N], stats [2] = {max a, sum exp(a - max)}, M [L]
 * and logits [C]; backward (three launches) recomputes p from a and stats and writes dZ (dtype),
 * dH [N, L] = p dM (fp32; the caller's GEMM then adds dZ [Wv;Wu]), dw [D], db [1], dWc [C, L],
 * dbc [C].  No float atomics: results repeat bitwise.  Refused before any device work: N < 1, L not
 * a multiple of 8 or > 4096, D not a multiple of 8 or > 512, C outside [1, 256], a null pointer, or
 * one of Z, H, w, a, M, Wc, work, dZ, dH, dw, dWc not 16-byte aligned.  work sized by the queries
 * (0 for a refused shape). */
int tm_attmil_pool_rows_per_block(void);
long long tm_attmil_pool_fwd_workspace(int N, int L);
int tm_attmil_pool_fwd(int dtype, const void* Z, const void* H, const float* w, const float* b,
                       const float* Wc, const float* bc, int N, int L, int D, int C, float* work,
                       float* a, float* stats, float* M, float* logits, void* stream);
long long tm_attmil_pool_bwd_workspace(int N, int L, int D);
int tm_attmil_pool_bwd(int dtype, const void* Z, const void* H, const float* w, const float* a,
                       const float* stats, const float* M, const float* Wc, const float* dlogits,
                       int N, int L, int D, int C, float* work, void* dZ, float* dH, float* dw,
                       float* db, float* dWc, float* dbc, void* stream);

/* ---- Chowder scores, two-sided top-R and head (chowder.hip) -- code/models/Chowder.py:19-50 ----
 * x [B, N, L] contiguous of dtype TM_F32 / TM_BF16 (all arithmetic fp32), w [L] / b [1] = the 1x1
 * Conv1d f1, W1 [H1, 2R] / b1, W2 [H2, H1] / b2, W3 [C, H2] / b3 = the three Linear layers of f2.
 * Limits: L a multiple of 8 and <= 4096, 1 <= R <= 32, N >= R, 1 <= B <= 65535, H1 / H2 / C in
 * [1, 1024]; anything else returns non-zero with a tm_last_error() text and launches nothing.
 * Forward (two launches): s[b,n] = x[b,n,:] . w + b, summed in an order that depends on L only (a
 * row gives the same bits wherever it stands); scores (nullable) [B, N] receives s.
 * vals [B, 2R] = (R smallest ascending, then R largest descending), the layout of
 * torch.cat((topk(largest=False).values, topk.values)); idx [B, 2R] int32 the instance indices.  Among
 * equal scores the lower index is selected first, in both selections.  With N < 2R an instance can
 * stand in both selections; it then appears twice.  Non-finite scores are out of contract: the
 * selection is then unspecified, but every idx is in [0, N) and nothing is read or written out of
 * bounds.  hid [B, H1 + H2] = (h1 = W1 vals + b1, h2 = W2 h1 + b2), logits [B, C] = W3 h2 + b3.
 * Backward (two launches and, with dx, one memset): from dlogits [B, C] the six head gradients,
 * dw [L] = sum_b sum_j dvals[b,j] x[b, idx[b,j], :] and db [1] = sum dvals, every sum in the fixed
 * order b, then j (no float atomics: bitwise repeatable).  dx (nullable) [B, N, L] fp32 is
 * zero-filled and row idx[b,j] receives dvals[b,j] w, an instance selected twice the sum of both.
 * An idx outside [0, N) is skipped.  work is sized by the queries (0 for a shape outside the limits). */
long long tm_chowder_fwd_workspace(int B, int N, int L, int R);
int tm_chowder_fwd(int dtype, const void* x, int B, int N, int L, const float* w, const float* b, int R,
                   const float* W1, const float* b1, int H1, const float* W2, const float* b2, int H2,
                   const float* W3, const float* b3, int C, void* work, float* scores, float* vals,
                   int* idx, float* hid, float* logits, void* stream);
long long tm_chowder_bwd_workspace(int B, int L, int R, int H1, int H2, int C);
int tm_chowder_bwd(int dtype, const void* x, int B, int N, int L, const float* w, int R, const float* W1,
                   int H1, const float* W2, int H2, const float* W3, int C, const float* vals,
                   const int* idx, const float* hid, const float* dlogits, void* work, float* dw,
                   float* db, float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                   float* dx, void* stream);

/* ---- CLAM_MB gated attention pooling, instance selection and instance loss (clam.hip) --
 * code/models/model_clam.py:195-268 ----
 * fp32.  Z [N, 2D] = h [Wa;Wb]^T + [ba;bb] and h [N, L] = ReLU(x W1^T + b1) come from the caller's
 * GEMMs; Wc [K, D] / bc [K] = attention_c, Wcls [K, L] / bcls [K] = the K Linear(L, 1) bag classifiers
 * stacked, Wic [K, 2, L] / bic [K, 2] = the K instance classifiers stacked.  Limits: L == 512, D a
 * multiple of 4 and <= 512, 1 <= K <= 8, 1 <= k_sample <= 32, N >= k_sample; anything else returns
 * non-zero with a tm_last_error() text and launches nothing.
 * tm_clam_fwd (two launches): A_raw [K, N] the scores a[c,i] = Wc[c] . (tanh(Z[i,:D]) sigmoid(Z[i,D:]))
 * + bc[c]; stats [K, 2] = {max_i a[c,i], sum_i exp(a[c,i] - max)}; M [K, L] = softmax_N(a) h;
 * logits [K] = Wcls[c] . M[c] + bcls[c].  label (nullable, a DEVICE int64, read by the kernel only)
 * switches the instance evaluation on: class y = label takes the k_sample largest scores of a[y,:]
 * in descending order (targets 1), then the k_sample smallest in ascending order (targets 0); with
 * subtyping every other class takes its k_sample largest (targets 0); among equal scores the lower
 * index first.  idx / preds / targets [K, 2 k_sample] int32 (-1 in the slots of a class that is not
 * evaluated and in the second half of an out-of-class row), dil [K, 2 k_sample, 2] =
 * d inst_loss / d il, inst_loss [1] = sum over the evaluated classes of the mean cross entropy of
 * il = h[idx] Wic[c]^T + bic[c] (divided by K with subtyping).  Non-finite scores are out of contract:
 * every idx still lies in [0, N).  tm_clam_scores: A_raw alone (one launch).
 * tm_clam_bwd (three launches): from dlogits [K] and dloss [1] (both nullable: zero) writes dZ [N, 2D],
 * dH [N, L] = sum_c p dM[c] plus the instance classifiers' contributions to the selected rows (the
 * caller's GEMM then adds dZ [Wa;Wb]), dWc [K, D], dbc [K], dWcls [K, L], dbcls [K] and, with idx
 * (nullable: no instance evaluation), dWic [K, 2, L] and dbic [K, 2].  Every sum has one fixed order
 * (no float atomics): bitwise repeatable.  work is sized by the queries (0 for a shape outside the
 * limits). */
long long tm_clam_fwd_workspace(int N, int K);
int tm_clam_scores(const float* Z, int N, int D, int K, const float* Wc, const float* bc, float* A_raw,
                   void* stream);
int tm_clam_fwd(const float* Z, const float* H, int N, int L, int D, int K, const float* Wc,
                const float* bc, const float* Wcls, const float* bcls, const float* Wic, const float* bic,
                const long long* label, int k_sample, int subtyping, float* work, float* A_raw,
                float* stats, float* M, float* logits, float* inst_loss, int* idx, int* preds,
                int* targets, float* dil, void* stream);
long long tm_clam_bwd_workspace(int N, int D, int K, int k_sample);
int tm_clam_bwd(const float* Z, const float* H, const float* A_raw, const float* stats, const float* M,
                int N, int L, int D, int K, const float* Wc, const float* Wcls, const float* Wic,
                const int* idx, const float* dil, int k_sample, const float* dlogits, const float* dloss,
                float* work, float* dZ, float* dH, float* dWc, float* dbc, float* dWcls, float* dbcls,
                float* dWic, float* dbic, void* stream);

/* ---- DTFD-MIL double-tier pseudo-bag pooling (dtfd.hip) -- code/models/model_interface_dtfd.py:174-279,
 * code/models/DTFDMIL.py:14-109 ----
 * fp32.  H [G S, L] = ReLU(xg W1^T) and Z [G S, 2D] = H [Wv;Wu]^T + [bv;bu] are the caller's GEMMs over
 * the G S gathered rows (pseudo-bag g = rows g S .. g S + S - 1).  Limits: L == 512, D a multiple of 4
 * and <= 512, 1 <= C <= 8, 1 <= S <= 1024, 1 <= G <= 64; anything else is refused before a launch.
 * tm_dtfd_fwd (two launches): tier 1 per pseudo-bag, a_i = w . (tanh(Z[i, :D]) * sigmoid(Z[i, D:])) + b,
 * p1 [G, S] = softmax_S(a) (max-shifted), M [G, L] = sum_i p_i h_i, sub [G, C] = M Wc^T + bc and, when
 * cam is not NULL, cam [G, S, C] = p_i (h_i . Wc[c]); tier 2 over the rows of M with the attCls
 * parameters (Wv2 / Wu2 [D, L], bv2 / bu2 [D], w2 [D], b2 [1], Wc2 [C, L], bc2 [C]): Z2 [G, 2D] (the gate
 * pre-activations, saved for the backward), p2 [G] = softmax_G, F [L] = sum_g p2_g M_g, slide [C] =
 * Wc2 F + bc2, yprob [C] = softmax(slide), yhat [1] = the first argmax; with label (device int64 [1],
 * nullable) losses [2] = {mean_g CE(sub_g, y), CE(slide, y)}, NaN for a label outside [0, C).
 * tm_dtfd_bwd: from dsub [G, C], dslide [C], gsub [1], gslide [1] (the gradients of sub, slide and the
 * two losses; each nullable: zero).  need_t2: the attCls gradients dWv2, dbv2, dWu2, dbu2, dw2, db2,
 * dWc2, dbc2 (one launch).  need_t1: dZ [G S, 2D], dH [G S, L] = p_i dM_g (the caller's GEMM then adds
 * dZ [Wv;Wu]), dw [D], db [1], dWc [C, L], dbc [C] (two more launches).  Neither: no launch.  Every sum
 * has one fixed order (no float atomics): bitwise repeatable.  work is sized by the query (0 for a
 * shape outside the limits). */
int tm_dtfd_fwd(const float* Z, const float* H, int G, int S, int L, int D, int C, const float* w,
                const float* b, const float* Wc, const float* bc, const float* Wv2, const float* bv2,
                const float* Wu2, const float* bu2, const float* w2, const float* b2, const float* Wc2,
                const float* bc2, const long long* label, float* p1, float* M, float* sub, float* cam,
                float* Z2, float* p2, float* F, float* slide, float* losses, float* yprob,
                long long* yhat, void* stream);
long long tm_dtfd_bwd_workspace(int G, int D, int C);
int tm_dtfd_bwd(const float* Z, const float* H, const float* p1, const float* M, const float* p2,
                const float* Z2, const float* F, const float* sub, const float* slide,
                const long long* label, int G, int S, int L, int D, int C, const float* w, const float* Wc,
                const float* Wv2, const float* Wu2, const float* w2, const float* Wc2, const float* dsub,
                const float* dslide, const float* gsub, const float* gslide, int need_t1, int need_t2,
                float* work, float* dZ, float* dH, float* dw, float* db, float* dWc, float* dbc,
                float* dWv2, float* dbv2, float* dWu2, float* dbu2, float* dw2, float* db2, float* dWc2,
                float* dbc2, void* stream);

/* ---- feature-bag sampling (bags.hip) -- code/datasets/feature_dataloader.py:335-431 ----
 * dst[r] = src[i0[r]] (i1 NULL or i1[r] < 0), (src[i0[r]] * wa[r]) + (src[i1[r]] * wb[r]) (mixup),
 * or 0 (i0[r] < 0); src [*, F] and dst [nrows, F] of dtype TM_F32 / TM_BF16, i0/i1 int64 row
 * ids into src (device), nrows <= 65535.  Replaces the per-item indexing of
 * FeatureBagLoader.__getitem__ (:346-362) and data_interface.simple_collate's stack (:238-246). */
int tm_gather_rows(int dtype, const void* src, int F, const long long* i0, const long long* i1,
                   const float* wa, const float* wb, int nrows, void* dst, void* stream);
/* The inverse, fp32: dst[idx[r]] = src[r] for nrows rows of F floats by plain stores (idx int64 on the
 * device, distinct; a row id outside [0, N) is skipped). */
int tm_scatter_rows(const float* src, const long long* idx, int nrows, int F, long long N, float* dst,
                    void* stream);

/* ---- tile-bag ingest (tiles.hip) -- code/datasets/jpg_dataloader.py:164-171, 229-293 ----
 * dst[r][c][h][w] = lut[c][src[idx[r]][h][w][c]] rounded to dtype (ToTensor + Normalize as a
 * [3][256] fp32 table the caller computes), or an all-zero tile where idx[r] < 0 or >= ntiles
 * (to_fixed_size_bag's zero padding; an index can never read outside the slab).  src is a uint8
 * slab [ntiles][H][W][3] (tile t at byte t*H*W*3, a tile < 2 GiB), idx int64 [n] and lut on the
 * device, dst of dtype TM_F32 / TM_BF16 addressed by the element strides dn, dc, dh, dw (> 0:
 * NCHW, channels-last or any other non-overlapping layout).  64-bit addressing throughout; any
 * n < 2^31 in one launch; n == 0 returns 0 without a launch.  Dword loads and 16-B stores where W
 * is a multiple of 16 B / sizeof(dtype), src is 4-B and dst 16-B aligned and the strides are those
 * of planes (dw == 1) or of channels-last pixels (dc == 1, dw == 3) with 16-B-aligned rows; the
 * same bits otherwise. */
int tm_gather_tiles_u8(int dtype, const void* src, long long ntiles, int H, int W, const long long* idx,
                       long long n, const float* lut, void* dst, long long dn, long long dc, long long dh,
                       long long dw, void* stream);

/* ---- glue (glue.hip) -- code/models/TransMIL.py:177-186 ------------------ */
int tm_put_cls(const float* cls, int B, int S, int D, float* H, void* stream);
/* CrossEntropyLoss(logits, one_hot(label).float()) mean over B rows + softmax + argmax in one
 * launch (code/models/model_interface.py:339-347); backward dlogits = g[0] (prob - one_hot) / B.
 * label int64 [B] on the device, values in [0, C); an out-of-range label makes the loss NaN and is
 * left out of class_stats (no out-of-bounds access).  class_stats
 * (nullable, int32 [C][2]) accumulates per-class count / correct (:350-356). */
int tm_ce_fwd(const float* logits, const long long* label, int B, int C, float* loss, float* prob,
              long long* yhat, int* class_stats, void* stream);
int tm_ce_bwd(const float* prob, const long long* label, int B, int C, const float* g, float* dlogits,
              void* stream);
/* out [B, n_pad, D] T, n_pad >= pad + S: rows [0, pad) of a bag zero, row pad + i =
 * T(keep(b*S + i, c) / (1 - p) * dH[b*S + i][c]) for i < S; rows pad + S .. n_pad - 1 have no input
 * row and are left alone (as tm_layernorm_fwd and the fused store of tm_ppeg_bwd leave them) */
int tm_dropout_bwd_pad(int dtype, const float* dH, int B, int S, int n_pad, int pad, int D, float p,
                       uint64_t seed, const uint64_t* seed_ptr, void* out, void* stream);
/* NystromAttention eq. 1 for a raw input: [B*S, D] fp32 -> front-padded [B, n_pad, D] T (rows
 * [0, pad) zero, rows pad + S .. n_pad - 1 left alone) */
int tm_pad_rows(int dtype, const float* x, int B, int S, int n_pad, int pad, int D, void* y, void* stream);
/* _fc1 GELU backward + grid-pad fold: dpre (dtype T) = (dH[token] + dH[dup]) * GELU'(pre); `pre` is the
 * forward's pre-activation in the same T (fp32 for TM_F32, bf16 for TM_BF16: tm_gemm_args.pre_bf16) */
int tm_fc1_gelu_bwd(int dtype, const float* dH, const void* pre, int B, int N, int S, int add, int D,
                    void* dpre, float* dcls, void* stream);
/* dpre = dy * GELU'(pre) elementwise (fp32 dy / pre, dpre in dtype): the backward of the inner
 * Linear + GELU of the in_features = 2048 _fc1 branch (code/models/TransMIL.py:100-111) */
int tm_gelu_bwd(int dtype, const float* dy, const float* pre, long long count, void* dpre, void* stream);
/* the same with pre and dpre both stored as dtype (the pre-activation a tm_gemm epilogue kept with
 * pre_bf16); count % 8 == 0, 16-B aligned */
int tm_gelu_bwd_pre(int dtype, const float* dy, const void* pre, long long count, void* dpre, void* stream);
/* y = max(a + b, 0) elementwise (the C5 encoder's residual add + ReLU, Bottleneck.forward,
 * code/models/ResNet.py:97-124); 16-B aligned, y may alias a */
int tm_add_relu(int dtype, const void* a, const void* b, void* y, long long count, void* stream);
/* y[r, c] = act(y[r, c] + bias[c]) in place over rows x C channels-last (C % 8 == 0; act = ReLU
 * when relu != 0): a 3x3 convolution's folded conv+BN bias + ReLU (ResNet.py:95-104) in one pass */
int tm_bias_act(int dtype, void* y, const void* bias, long long rows, int C, int relu, void* stream);
/* fp32 ReLU passes in place over count elements (a multiple of 4, 16-B aligned): h = max(h, 0), the
 * ReLU of a Linear without a bias, and its backward dh = h > 0 ? dh : 0 */
int tm_relu(float* h, long long count, void* stream);
int tm_relu_bwd(float* dh, const float* h, long long count, void* stream);
/* ResNet stem tail (ResNet.py:240-245, BN folded into the convolution's bias): out[N, OH, OW, C] =
 * maxpool3x3/2 pad 1 (relu(y + bias)) over the raw channels-last bf16 stem output y[N, H, W, C],
 * OH = (H - 1) / 2 + 1; one pass instead of the in-place bias + ReLU and a max-pool launch */
int tm_bias_relu_maxpool(const void* y, const void* bias, void* out, int N, int H, int W, int C, void* stream);
/* the same with train-mode BatchNorm: each tap bf16(relu(y * scale + shift)) (tm_bn_apply's
 * arithmetic, scale / shift fp32 [C] from tm_bn_train_stats), then the window max */
int tm_bn_relu_maxpool(const void* y, const float* scale, const float* shift, void* out, int N, int H, int W, int C,
                       void* stream);
/* The whole eval-mode stem in one pass (code/models/ResNet.py:240-245, BN folded): out[N, PH, PW, 64]
 * = maxpool3x3/2 pad 1(relu(conv7x7/2 pad 3(x, w) + bias)), x bf16 [N, 3, H, W] at element strides
 * (sn, sc, sh, sw) (NCHW or channels-last),
 * wp the folded weights packed bf16 [64][7][8][4] (w[o, c, ky, kx] at [o][ky][kx][c]; kx = 7 and
 * c = 3 zero), bias bf16 [64]; CH = (H - 1) / 2 + 1, PH = (CH - 1) / 2 + 1 (same for W).  fp32
 * accumulation, one bf16 rounding after the ReLU; the convolution output never reaches HBM. */
int tm_stem_conv_pool(const void* x, const void* wp, const void* bias, void* out, int N, int H, int W, long long sn,
                      long long sc, long long sh, long long sw, void* stream);
/* The train-mode stem (batch-statistics bn1, code/models/model_interface.py:303-309 feeding the
 * frozen encoder in train mode) in two passes over the tiles, the convolution recomputed instead of
 * stored: tm_stem_bn_stats runs the convolution and reduces its bf16-rounded outputs per channel
 * (per-workgroup count / mean / M2, merged in workgroup order in fp64: deterministic), then writes
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale (biased variance) and updates the
 * running statistics with the unbiased variance and the momentum (nn.BatchNorm2d);
 * workspace >= tm_stem_bn_stats_workspace() doubles.  tm_stem_conv_pool_bn then writes
 * maxpool(bf16(relu(bf16(conv) * scale + shift))) (tm_bn_apply's arithmetic).  N may be the whole
 * bag: tiles are addressed with 64-bit bases. */
long long tm_stem_bn_stats_workspace(void);
int tm_stem_bn_stats(const void* x, const void* wp, int N, int H, int W, long long sn, long long sc, long long sh,
                     long long sw, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, float* scale, float* shift, double* workspace, long long ws_doubles,
                     void* stream);
int tm_stem_conv_pool_bn(const void* x, const void* wp, const float* scale, const float* shift, void* out, int N,
                         int H, int W, long long sn, long long sc, long long sh, long long sw, void* stream);
/* out[n, i, j, :] = x[n, s*i, s*j, :] for channels-last x [N, H, W, C] (bf16 / fp32, C * elem % 16
 * == 0): the input of a stride-s 1x1 downsample convolution (code/models/ResNet.py:130-135). */
int tm_subsample2d(int dtype, const void* x, void* out, int N, int H, int W, int C, int stride, void* stream);
/* C5 encoder 1x1 convolution over channels-last rows (code/models/ResNet.py:95-117 conv1 / conv3
 * / downsample with BN folded): y[rows, cout] = act(x[rows, cin] . w[cout, cin]^T (+ bias[cout])
 * (+ residual[rows, cout])), one hipBLASLt GEMM with the bias / residual / ReLU epilogue.
 * bias / residual may be NULL; residual must not alias y.  workspace: caller-owned device scratch
 * of ws_bytes, stream-ordered on `stream` (NULL / 0: workspace-free algorithms only; up to
 * tm_conv1x1_workspace_bytes() is used).  Library state: a per-device hipBLASLt handle and a
 * per-shape plan cache (host objects behind a mutex, immutable once built -- no device scratch is
 * shared between calls).  No host synchronisation.  Returns 3 on a hipBLASLt error. */
long long tm_conv1x1_workspace_bytes(void);
int tm_conv1x1(int dtype, const void* x, const void* w, const void* bias, const void* residual, void* y,
               long long rows, int cin, int cout, int relu, void* workspace, long long ws_bytes, void* stream);
/* THE EXCEPTION to "no host synchronisation": times every hipBLASLt heuristic candidate for this
 * shape on the given operands (y is overwritten) and waits on timing events, then keeps the fastest
 * for later tm_conv1x1 calls of the shape (the hipBLASLt analogue of MIOpen find).  Call once per
 * shape, outside stream capture (refused with status 1 while `stream` is capturing); without it
 * tm_conv1x1 uses the heuristic's first choice. */
int tm_conv1x1_tune(int dtype, const void* x, const void* w, const void* bias, const void* residual, void* y,
                    long long rows, int cin, int cout, int relu, void* workspace, long long ws_bytes,
                    void* stream);
/* ResNet-18 BasicBlock 3x3 convolution (pad 1, stride 1 or 2; BN folded into w / bias) over
 * channels-last activations, a hand-written implicit GEMM on the MFMA units (conv3x3.hip):
 * y[n, ho, wo, cout] = act(conv3x3(x[n, h, wd, cin], w) (+ bias[cout]) (+ residual[n, ho, wo, cout])),
 * ho = (h - 1) / stride + 1, wo = (wd - 1) / stride + 1, act = ReLU when relu != 0.
 * w is [cout][3][3][cin] (a [cout, cin, 3, 3] tensor contiguous in channels_last).  dtype TM_BF16
 * (bf16 MFMA, fp32 accumulation, one rounding) or TM_F32 (f32 MFMA) for x, w, bias, residual, y.
 * cin, cout multiples of 64 up to 512; h, wd in 1..32768; n >= 1; x and y addressed with 64-bit
 * offsets (no 2^31 limit); every pointer 16-byte aligned; bias / residual may be NULL; y must not
 * alias x.  Bitwise reproducible (no atomics).  Every refusal's message begins "conv3x3:". */
int tm_conv3x3(int dtype, const void* x, const void* w, const void* bias, const void* residual, void* y,
               long long n, int h, int wd, int cin, int cout, int stride, int relu, void* stream);
/* One convolution stage of the `simple` tile backbone (code/models/model_interface.py:270-281:
 * Conv2d(3, 20, 5) / Conv2d(20, 50, 5), each + ReLU + MaxPool2d(2, 2)) in one pass (conv5x5.hip):
 *   out[n, pr, pc, c] = maxpool2x2/2(relu(conv5x5_valid(x, w) + bias))[n, c, pr, pc],
 * stride 1, no padding, floor-mode pool: ph = (h - 4) / 2, pw = (w - 4) / 2 (an odd convolution output
 * drops its last row / column); the convolution output never reaches HBM.  Implicit GEMM on the MFMA
 * units in both modes: dtype TM_BF16 (bf16 x, wp, out; fp32 accumulation, one rounding after the
 * pool) or TM_F32.  (cin, cout) = (3, 20) or (20, 50) only; h, w in 6..32768; n >= 1, x and out
 * addressed with 64-bit offsets (no 2^31 limit).
 *   x     (3, 20):  [n, 3, h, w] at element strides (sn, sc, sh, sw): NCHW or channels-last.
 *         (20, 50): the first stage's output layout: channels-last pixels of 24 channels, 20 .. 23
 *                   zero (sc = 1, sw = 24, sh and sn multiples of 8, 16-byte aligned).
 *   wp    the weights packed on the host in MFMA fragment order, dtype elements
 *         [NS][NU][2][32][8]: element j of fragment f = 2 s + hf of output channel 32 u + r at
 *         [s][u][hf][r][j], zero where no weight is named.
 *         (3, 20):  NS = 8, NU = 1; f = 3 ky + sub, j = 4 (kx - 2 sub) + c  (kx = 5, c = 3: zero).
 *         (20, 50): NS = 38, NU = 2; f = 3 (5 ky + kx) + sub, j = c - 8 sub  (c >= 20: zero).
 *   bias  fp32 [cout].
 *   out   tile n at out + n * so; pixel (pr, pc) holds cpo channels (cpo even, cout <= cpo <= 32 NU;
 *         channels cout .. cpo - 1 are written as zeros), and the `tail` elements after a tile's
 *         ph * pw * cpo are written as zeros (so even, so >= ph * pw * cpo + tail).  The second stage
 *         with cpo = 50, so = 140480, tail = 30 writes the rows of the Linear's K-padded A matrix.
 * Bitwise reproducible (no atomics).  Every refusal's message begins "conv5x5:". */
int tm_conv5x5_relu_pool(int dtype, const void* x, const void* wp, const float* bias, void* out, long long n, int h,
                         int w, int cin, int cout, long long sn, long long sc, long long sh, long long sw,
                         long long so, int cpo, int tail, void* stream);
/* Train-mode BatchNorm2d over a channels-last activation given as npieces (1..64) row pieces
 * xs[p] of [rows[p], C] (host arrays; C a power of two, 8..2048; nn.BatchNorm2d.forward in
 * training, code/models/ResNet.py:95-117 under model.train()): batch statistics over all pieces
 * (biased variance for the normalisation) -> scale = gamma / sqrt(var + eps), shift = beta -
 * mean * scale (fp32 [C]); running_mean / running_var (may be NULL) updated with the unbiased
 * variance and momentum.  workspace >= tm_bn_train_workspace(C) floats. */
long long tm_bn_train_workspace(int C);
int tm_bn_train_stats(int dtype, const void* const* xs, const long long* rows, int npieces, int C,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, float* scale, float* shift, float* workspace, long long ws_floats,
                      void* stream);
/* y = act(y * scale[c] + shift[c] (+ residual | + residual * rscale[c] + rshift[c])) in place over
 * rows x C channels-last (C % 8 == 0): BN apply + ReLU, or bn3 + (BN'd) identity + ReLU, one pass */
int tm_bn_apply(int dtype, void* y, const float* scale, const float* shift, const void* residual,
                const float* rscale, const float* rshift, long long rows, int C, int relu, void* stream);

/* ---- class-row specialisation of the last TransLayer (clsrow.hip) -- code/models/TransMIL.py:195-203 ----
 * The logits read layer 2 only through the class token (norm(h)[:, 0]), which sits at row r = pad of
 * the front-padded attention input.  Forward: merged[b][r] = A1 row + conv33 (lse1[bh][r] written),
 * then H3[b*S] = H2[b*S] + dropout(merged[b][r] Wo^T + bo) (other H3 rows are not written).
 * Backward (dL/dH3 zero outside the class rows): dWo, dbo (=), dmerged [B][D] (dtype) rows; then
 * dq row r (the caller zero-fills dq), dk~ / dY (=) [nbh][256][64], the conv33 dv window rows
 * r-16..r+16 (caller zero-fills dv) and dwconv (=) [nh][33]. */
int tm_cls_a1_row_fwd(int dtype, const void* q, const void* v, const void* kl_t, const void* y_t, const float* wconv,
                      int nbh, int nh, int n, int r, void* merged, float* lse1, void* stream);
int tm_cls_out_fwd(int dtype, const void* merged, const void* wo, const float* bo, const float* H2, int B, int n, int r,
                   int S, int D, float p, uint64_t seed, const uint64_t* seed_ptr, float* H3, void* stream);
int tm_cls_out_bwd(int dtype, const float* dH, const void* merged, const void* wo, int B, int n, int r, int S, int D,
                   float p, uint64_t seed, const uint64_t* seed_ptr, float* dwo, float* dbo, void* dmerged,
                   void* stream);
/* tm_head_ce_bwd's one-bag fast path (B = 1, C <= 4, D = 512, no extra logits gradient) folded
 * into tm_cls_out_bwd: every block recomputes dL/dH3 at the class row from the saved softmax, x^
 * and rstd; dH's class row and the head / norm gradients are written as tm_head_ce_bwd writes
 * them.  One launch instead of two on the training step's tail (code/models/TransMIL.py:202-204,
 * model_interface.py:346-347 backward). */
int tm_cls_head_out_bwd(int dtype, const float* prob, const long long* label, const float* gloss, int C,
                        const float* xhat, const float* rstd, const float* gamma, const float* beta, const float* W,
                        float* dW, float* dbias, float* dgamma, float* dbeta, float* dH, const void* merged,
                        const void* wo, int n, int r, int S, int D, float p, uint64_t seed, const uint64_t* seed_ptr,
                        float* dwo, float* dbo, void* dmerged, void* stream);
int tm_cls_a1_row_bwd(int dtype, const void* dmerged, const void* q, const void* v, const void* kl_t, const void* y_t,
                      const float* lse1, const float* wconv, int B, int nh, int n, int r, float* dq, float* dkl,
                      float* dy, void* dv, float* dwconv, void* stream);   /* dv: the 33-row window, in T */
/* bf16 mode: layer 2's q enters the loss only through its landmark means q~ (App. A eq. 4) and the
 * class row r, so dL/dq = dq~[t / l] / l on every row t plus the class row's own term, and the q
 * part of to_qkv's backward is two small products instead of a dense q block in dqkv:
 *   dWq = scale * Aq^T Xs,   dxn[t] += scale * (Aq Wq)[t / l] (+ row NL at t = r)
 * (tm_bmm, then tm_layernorm_bwd_seg).  This writes their operands, [B][288][nh*64] fp32 each:
 *   Aq rows j < 256: (dql + sum_p slab[p])[b*nh + h][j][d] / l at column h*64 + d (slab: the
 *   nslabs [B*nh][256][64] partials tm_nys_a3_bwd_fused leaves in its work), row 256: dq[b*nh+h][r][d];
 *   Xs rows j < 256: sum over the segment's rows of xn[b] (bf16 [B][n][nh*64], pad rows zero),
 *   row 256: xn[b][r]; rows 257..287 of both: zeros (operand rows to a multiple of 32). */
int tm_cls_q_rows(const float* dql, const void* slab, int nslabs, const float* dq, const void* xn, int B, int nh,
                  int n, int r, float* Aq, float* Xs, void* stream);

/* fp32 -> dtype copies of up to 8 tensors (per-step bf16 GEMM weight operands) in one launch;
 * offset[] = prefix sums of the element counts, offset[0] = 0 */
#define TM_CAST_MAX 8
typedef struct tm_cast_table {
  int count;
  int reserved;
  const float* src[TM_CAST_MAX];
  void* dst[TM_CAST_MAX];
  long long offset[TM_CAST_MAX + 1];
} tm_cast_table;
int tm_cast_f32_many(int dtype, const tm_cast_table* table, void* stream);
/* One launch per forward: the cast table (as tm_cast_f32_many, 0..8 tensors), the PPEG fold
 * (as tm_ppeg_fold; skipped when w7 is NULL), when counter is non-NULL counter[0] += 1 with the
 * new value written to seed_out[0] (the dropout stream of a captured step), and when cls is
 * non-NULL the class-token rows H[b*S][0..D) = cls (as tm_put_cls). */
int tm_step_prepare(int dtype, const tm_cast_table* table, const float* w7, const float* b7,
                    const float* w5, const float* b5, const float* w3, const float* b3, int D,
                    float* wfold, float* bfold, long long* counter, long long* seed_out,
                    const float* cls, float* H, int B, int S, void* stream);

/* ---- evaluation record and epoch metrics (evalrec.hip) --------------------
 * validation_step / test_step and their epoch ends (code/models/model_interface.py:432-607,
 * 609-860) without a host sync per step.  The epoch record is five caller-owned arrays of
 * `capacity` rows (logits / prob fp32 [capacity][C], y_hat / label int64, nll fp32) plus a device
 * int `cursor` (rows appended so far) and class_stats (int32 [C][2] count / correct, as tm_ce_fwd;
 * may be NULL).
 * tm_eval_record: one launch per step; for bag b row cursor + b receives the logits, their
 * max-subtracted fp32 softmax, the first argmax, the label and nll = logsumexp(logits) -
 * logits[label]; class_stats[label] is bumped and cursor advances by B.  A row >= capacity is not
 * written (the cursor still counts, so the host sees the overflow at the epoch end); a label
 * outside [0, C) gives a NaN nll, no stats update and no out-of-bounds read. */
int tm_eval_record(const float* logits, const long long* label, int B, int C, int capacity, int* cursor,
                   float* rec_logits, float* rec_prob, long long* rec_yhat, long long* rec_label,
                   float* rec_nll, int* class_stats, void* stream);
/* Per patient p in [0, P) over the first M record rows (patient: int32 [M] ids; other ids are
 * ignored), in record order: target = the label of the first slide, score[C] = the fp32 mean of the
 * slides' prob (with positive_rule: over the slides with y_hat == 1 only when there is one, :539-544),
 * pred = score[1] > 0.5 for C == 2, else the first argmax; nslides = the slide count (a patient
 * without slides: score 0, target -1). */
int tm_eval_patients(const float* rec_prob, const long long* rec_yhat, const long long* rec_label,
                     const int* patient, int M, int C, int P, int positive_rule, float* score,
                     long long* pred, long long* target, int* nslides, void* stream);
/* cm[target][pred] as int32 [C][C] (= ; out-of-range entries skipped) and, when nll is non-NULL,
 * nll_sum[0] = the sum of nll[0..M) accumulated in double in a fixed order. */
int tm_eval_confusion(const long long* pred, const long long* target, int M, int C, int* cm,
                      const float* nll, double* nll_sum, void* stream);
/* One-vs-rest Mann-Whitney counts per class c over scores [M][C]: over every (i, j) with
 * target[i] == c != target[j], wins2[c] = sum 2 [s_i > s_j] + [s_i == s_j], npairs[c] = the pair
 * count (both uint64 [C], = ).  AUROC_c = wins2 / (2 npairs): the trapezoidal ROC area with ties
 * counted half.  Integer adds only: exact, independent of order. */
int tm_eval_auc_pairs(const float* scores, const long long* target, int M, int C,
                      unsigned long long* wins2, unsigned long long* npairs, void* stream);

/* ---- optimizer step (optim.hip) ----------------------------------------
 * torch.optim.RAdam (L2 decay, code/MyOptimizer/optim_factory.py:77-79) + the
 * Lookahead sync (code/MyOptimizer/lookahead.py, wrapped at optim_factory.py:118-121)
 * over up to 40 parameter tensors in one launch.  exp_avg / exp_avg_sq / slow are
 * flat 16-B aligned fp32 buffers indexed by the table's offsets (prefix sums of numel, each
 * rounded up to a multiple of 4); counters (int32[tm_radam_counters_len(total)], device,
 * zero-initialised; total = the table's last offset) hold one (RAdam step, Lookahead step) pair per
 * workgroup of the launch, each advanced by its workgroup in the same launch (no tick launch);
 * the pairs stay equal as long as the table's total is fixed, and pair 0 is the one to checkpoint.
 * lookahead_k == 0 disables the sync (plain RAdam). */
#define TM_OPTIM_MAX_TENSORS 40
typedef struct tm_optim_tensor {
  float* param;
  const float* grad;
  long long numel;
  float lr;
  float weight_decay;
} tm_optim_tensor;
typedef struct tm_optim_table {
  int count;
  int reserved;
  long long offset[TM_OPTIM_MAX_TENSORS + 1];
  tm_optim_tensor t[TM_OPTIM_MAX_TENSORS];
  /* device [count][2] fp32 (lr, weight_decay) read by the kernel in place of t[i].lr /
   * t[i].weight_decay, or NULL.  A captured hipGraph replays the kernel arguments it was captured
   * with; reading the hyper-parameters from device memory lets an LR scheduler (ReduceLROnPlateau,
   * model_interface.py:862-877) act on a replayed step (the caller rewrites the buffer). */
  const float* hyper;
} tm_optim_table;
long long tm_radam_counters_len(long long total_elements);
int tm_radam_lookahead_step(const tm_optim_table* table, float* exp_avg, float* exp_avg_sq, float* slow,
                            int* counters, float beta1, float beta2, float eps, int lookahead_k,
                            float lookahead_alpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSMIL_HIP_H */
