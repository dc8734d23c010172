/*
 * nrv.h -- C ABI of the MI355X-native ViT encoder-block hot path (libnrv_hip.so).
 *
 * Drop-in boundary for RandallBalestriero/noise-robust-vit's ViT / SimpleViT module API.
 * The reference has NO native/FFI layer (it is pure PyTorch): every entry
 * point below replaces a run of ATen ops dispatched by a reference nn.Module.forward (and its
 * autograd backward); the replaced call site is cited as <file>:<lines> relative to
 * /root/reference/vit_pytorch_robust/.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless stated; the caller owns every buffer,
 *     including workspaces and saved-for-backward tensors.  Nothing here allocates, frees or
 *     synchronises.  All work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - bf16 tensors are raw uint16 storage (bfloat16 bit pattern), row-major, leading dimension
 *     in ELEMENTS.  "stream" tensors (the residual stream) are fp32 or bf16, selected by dtype.
 *   - Return value: 0 = ok; < 0 = argument/shape error detected on the host before any launch
 *     (NRV_ERR_*); > 0 = hipError_t from the launch.  No exceptions cross the ABI.
 *   - Re-entrant; no mutable globals except ONE process-wide planning knob, nrv_set_reserved_cus() (below): it changes
 *     the tile / split plans of every later GEMM launch of the process, whichever thread or stream issues it.
 *   - Built for gfx950 only (wave64, MFMA 16x16x32 bf16, buffer_load...lds, ds_read_b64_tr_b16).
 */
#ifndef NRV_H_
#define NRV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRV_ABI_VERSION 19

/* dtype codes */
#define NRV_F32 0
#define NRV_BF16 1
#define NRV_U8 2                 /* the 8-bit gelu' stream of NRV_EPI_BIAS_GELU_Q8 / NRV_EPI_DGELU_Q8 only */

/* error codes */
#define NRV_OK 0
#define NRV_ERR_NULL (-1)        /* required pointer is NULL */
#define NRV_ERR_SHAPE (-2)       /* shape/stride not supported (see each entry) */
#define NRV_ERR_DTYPE (-3)       /* unknown dtype code */
#define NRV_ERR_WORKSPACE (-4)   /* workspace too small */
#define NRV_ERR_ALIGN (-5)       /* pointer / leading dimension not 16-byte aligned */
#define NRV_ERR_EPILOGUE (-6)    /* unknown epilogue or missing epilogue operand */

/* GEMM epilogues (fused into the MFMA kernel's store phase) */
#define NRV_EPI_NONE 0           /* C = acc                                                     */
#define NRV_EPI_BIAS 1           /* C = acc + bias[n]                                           */
#define NRV_EPI_BIAS_GELU 2      /* u = acc + bias[n]; aux_out = bf16(gelu_erf'(u)) (optional); C = gelu_erf(u) */
#define NRV_EPI_BIAS_RESIDUAL 3  /* C = acc + bias[n] (bias optional) + aux[m % aux_row_mod][n] */
#define NRV_EPI_DGELU 4          /* C = acc * aux[m][n]     (aux = the bf16 gelu' saved by NRV_EPI_BIAS_GELU) */
#define NRV_EPI_BIAS_GELU_Q8 5   /* NRV_EPI_BIAS_GELU with aux_out as bytes: q = round(202 gelu_erf'(u)) + 26  (bf16 C only)      */
#define NRV_EPI_DGELU_Q8 6       /* C = acc * (aux[m][n] - 26) / 202   (aux = the NRV_U8 stream saved by NRV_EPI_BIAS_GELU_Q8; bf16 C) */

int nrv_abi_version(void);
const char* nrv_error_string(int code);

/* ------------------------------------------------------------------------------------------
 * LayerNorm  (replaces nn.LayerNorm at simple_vit.py:38,54,65 / vit.py:104,115,167 and its backward)
 *   y = (x - mean) * rstd * gamma + beta, biased variance, eps inside the sqrt.
 *   x [rows, dim] (x_dtype fp32|bf16, contiguous), y bf16 [rows, dim], mean/rstd fp32 [rows].
 *   dim % 8 == 0 and dim <= 4096.
 * ---------------------------------------------------------------------------------------- */
int nrv_layernorm_fwd(const void* x, int x_dtype, const float* gamma, const float* beta,
                      void* y_bf16, float* mean, float* rstd,
                      int64_t rows, int dim, float eps, void* stream);

/* dx = dres + LN'(dy); dgamma/dbeta = column reductions (deterministic two-pass).
 *   dy bf16 [rows, dim]; dres optional residual-stream gradient (dres_dtype fp32|bf16) or NULL;
 *   dx_f32 / dx_bf16: either or both may be given (the bf16 copy feeds the next MFMA GEMM);
 *   dgamma/dbeta fp32 [dim]: written (accumulate=0) or added to (accumulate=1).
 *   workspace: nrv_layernorm_bwd_workspace(rows, dim) bytes. */
size_t nrv_layernorm_bwd_workspace(int64_t rows, int dim);
int nrv_layernorm_bwd(const void* dy_bf16, const void* x, int x_dtype, const float* gamma,
                      const float* mean, const float* rstd,
                      const void* dres, int dres_dtype,
                      float* dx_f32, void* dx_bf16,
                      float* dgamma, float* dbeta, int accumulate,
                      void* workspace, size_t workspace_bytes,
                      int64_t rows, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * GEMM "NT":  C[M,N] = A[M,K] . B[N,K]^T  (+ epilogue), bf16 operands, fp32 MFMA accumulate.
 *   Replaces nn.Linear forward (simple_vit.py:39,41,61,62,130; vit.py MLP :40-47; utils.py:115,579)
 *   and, with B = W^T, the input-gradient matmul of its backward.
 *   A [M,K] bf16 lda; B [N,K] bf16 ldb; C [M,N] c_dtype (fp32|bf16) ldc.
 *   K % 8 == 0; lda, ldb % 8 == 0; ldc*sizeof(C) % 16 == 0; all base pointers 16-byte aligned.
 *   bias fp32 [N] (may be NULL where optional).
 *   aux: epilogue operand [*, N] of aux_dtype with ld_aux; aux_row_mod > 0 makes the aux row
 *        index m % aux_row_mod (broadcast of a [tokens, dim] positional table over the batch,
 *        simple_vit.py:142-143); 0 means row m.
 *   aux_out: optional bf16 [M,N] (ldc_aux) receiving gelu'(pre-activation) for NRV_EPI_BIAS_GELU: the backward's
 *        NRV_EPI_DGELU epilogue is then one multiply, no second erf/exp evaluation.
 *        The _Q8 pair keeps the same stream in one byte per element (gelu_erf' lies in [-0.129, 1.129]; step 1/202, i.e. an
 *        absolute error <= 0.0025 -- what bf16 leaves on values in [0.5, 1)): aux_dtype = NRV_U8 on the way back.  The byte stream is
 *        private to the pair and stored in ROW PAIRS, byte (m, n) at (m >> 1) * 2 ld + (n >> 6) * 128 + (m & 1) * 64 + (n & 63)
 *        (the 2 x 64 bytes a wave touches are one 128-byte line): N % 64 == 0, ld % 16 == 0, ld >= N, and the buffer holds M rounded up
 *        to an even number of rows of ld bytes.
 *   Output row remap (class-token slot, vit.py:341-342): if out_group > 0 the result row m is
 *   stored at row (m / out_group) * out_group_stride + (m % out_group) + out_row_offset of C
 *   (and of aux, when aux_row_mod == 0).  The remap and aux_row_mod ride on NRV_EPI_BIAS_RESIDUAL (the patch
 *   embedding: bias + positional table, optionally with the class-token slot); with any other epilogue
 *   they are refused (NRV_ERR_EPILOGUE).
 *   Rows >= M and columns >= N of a tile are never written; ldc, ld_aux * 1280 bytes must stay below 2^31
 *   (a wave addresses its 160-row block with 32-bit offsets).
 * ---------------------------------------------------------------------------------------- */
int nrv_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb,
                     void* C, int c_dtype, int64_t ldc,
                     int64_t M, int64_t N, int64_t K,
                     int epilogue, const float* bias,
                     const void* aux, int aux_dtype, int64_t ld_aux, int64_t aux_row_mod,
                     void* aux_out, int64_t ld_aux_out,
                     int64_t out_group, int64_t out_group_stride, int64_t out_row_offset,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * GEMM "TN":  C[M,N] (fp32) = beta * C + sum_t A[t,M] * B[t,N]   -- the weight-gradient matmul
 *   dW = dY^T . X of nn.Linear's backward (contraction over tokens), split over the token axis
 *   with a deterministic slab reduction.
 *   A [T,M] bf16 lda; B [T,N] bf16 ldb; C fp32 ldc; beta is 0 or 1.
 *   M % 8 == 0, N % 8 == 0; a_group/a_group_stride/a_row_offset remap the rows of A exactly as
 *   the NT output remap does (0 = identity) so that dY laid out with a class-token slot can be used.
 *   dbias (optional, fp32 [M]): the bias gradient of the same Linear, dbias[m] = dbias_beta*dbias[m] + sum_t A[t,m],
 *   computed on the MFMA from the A tiles the kernel already streams (no second pass over dY).
 *   workspace: nrv_gemm_tn_workspace(M, N, T) bytes.
 * ---------------------------------------------------------------------------------------- */
size_t nrv_gemm_tn_workspace(int64_t M, int64_t N, int64_t T);
int nrv_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb,
                     float* C, int64_t ldc, int64_t M, int64_t N, int64_t T, float beta,
                     int64_t a_group, int64_t a_group_stride, int64_t a_row_offset,
                     float* dbias, float dbias_beta,
                     void* workspace, size_t workspace_bytes, void* stream);

/* All weight gradients of a layer in ONE launch (ABI 11): up to 4 problems C_i[M_i,N_i] = beta_i * C_i + sum_t A_i[t,:]^T B_i[t,:]
 * over the same T token rows (dWqkv, dWo, dW1, dW2 of an encoder block: utils.py:693-706, simple_vit.py:39-41,61-62), optional
 * dbias_i[m] = dbias_beta_i * dbias_i[m] + sum_t A_i[t,m].  One workgroup per CU, all with the same number of K-steps of 64 token
 * rows: cohorts of one workgroup per 256 x 256 tile that sweep the same token range in step (operand rows are shared through
 * L2 / Infinity Cache as in a split-K launch) + a stream-K remainder; partial tiles go through `workspace` and are added in K
 * order (deterministic per CU count).  Same operand rules as nrv_gemm_tn_bf16 (no row remap).  `problems` is a HOST array, read
 * during the call.  nrv_gemm_tn_grouped_workspace returns 0 for a group the kernel does not take (fewer than 8 K-steps of work
 * per CU, more tiles than CUs): issue nrv_gemm_tn_bf16 per problem then. */
typedef struct nrv_tn_problem {
    const void* A; int64_t lda;          /* bf16 [T, M] */
    const void* B; int64_t ldb;          /* bf16 [T, N] */
    float* C; int64_t ldc;               /* fp32 [M, N] */
    int64_t M, N;
    float beta;                          /* 0 or 1 */
    float* dbias; float dbias_beta;      /* optional fp32 [M]; beta 0 or 1 */
} nrv_tn_problem;
size_t nrv_gemm_tn_grouped_workspace(const nrv_tn_problem* problems, int nprob, int64_t T);
int nrv_gemm_tn_grouped_bf16(const nrv_tn_problem* problems, int nprob, int64_t T,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch-plan queries (ABI 18).  Read-only: they launch nothing, touch no device memory and are callable without a GPU (the
 * library then plans for 256 CUs).  They report what nrv_gemm_nt_bf16 / nrv_gemm_tn_bf16 WOULD launch for the same arguments
 * under the current nrv_set_reserved_cus() value; the launches and the queries go through one planning function, so the answer
 * is the launch's own decision, not a copy of it.  Operand pointers, leading dimensions and dtypes do not enter a plan.
 * Return 0 and fill *plan, or NRV_ERR_NULL / NRV_ERR_SHAPE / NRV_ERR_EPILOGUE by the rules of the launch (N % 8, K % 8, the
 * remap only with NRV_EPI_BIAS_RESIDUAL, the _Q8 epilogues only with N % 64 == 0, beta 0 or 1).
 *   nrv_gemm_nt_plan: `remap` != 0 when the launch passes out_group > 0 or aux_row_mod > 0.
 *     tile_m x tile_n : the tile configuration (256 / 320 / 192 / 128 rows x 256 columns, or 384 x 128);
 *     phased          : 1 = the phased persistent kernel (K % 64 == 0 and K >= 192: workgroup b walks the tiles b, b + grid, ...),
 *                       0 = the plain kernel, one tile per workgroup;
 *     tiles, grid     : output tiles and workgroups launched (grid == tiles on the plain kernel).
 *   nrv_gemm_tn_plan: `a_group` != 0 when the launch remaps the rows of A, `dbias` != 0 when it asks for the bias gradient.
 *     tiles           : 256 x 256 output tiles; the grid is tiles * splits workgroups;
 *     splits, kt_q, kt_r : token splits and the K-tiles (64 token rows) of a split: kt_q, the first kt_r splits one more;
 *     phased          : 1 = the phased kernel (no row remap and kt_q >= 3), 0 = the plain one;
 *     direct          : 1 = one split and beta == 0: the kernel stores into C with the caller's ldc; 0 = fp32 slabs in the workspace;
 *     reduce          : 1 = the reduction kernel runs (slabs, or the bias gradient of a direct launch).
 * ---------------------------------------------------------------------------------------- */
typedef struct nrv_nt_plan { int tile_m, tile_n, phased, tiles, grid; } nrv_nt_plan;
typedef struct nrv_tn_plan { int tiles, splits, kt_q, kt_r, phased, direct, reduce; } nrv_tn_plan;
int nrv_gemm_nt_plan(int64_t M, int64_t N, int64_t K, int epilogue, int remap, nrv_nt_plan* plan);
int nrv_gemm_tn_plan(int64_t M, int64_t N, int64_t T, int a_group, float beta, int dbias, nrv_tn_plan* plan);

/* ------------------------------------------------------------------------------------------
 * The split-K reduction as a side job of the NT launch that follows (added without an ABI bump: the ABI stays 19 and every
 * prototype, plan answer and workspace size above is unchanged).
 *
 * A weight-gradient launch leaves fp32 slabs (and bias column sums) that a small, latency-bound reduction kernel adds up.  The
 * persistent NT kernel lets the workgroups that have one tile fewer than the busiest ones start late; with a job attached they
 * reduce equal contiguous shares of the slabs first, in place of (part of) that wait.  No workgroup waits for another: stream
 * order guarantees that the slabs are complete.  The arithmetic and its order are those of the reduction kernel, so C and dbias
 * are bit-identical whichever way a job is run.
 *   nrv_gemm_tn_bf16_deferred: nrv_gemm_tn_bf16 without the reduction launch.  Same checks, plan and kernel; fills *job, whose
 *     `pending` is 1 when slabs or a bias gradient remain to be reduced (0: a direct plan without dbias, C is complete).  The
 *     workspace, C and dbias must stay valid until the job has run.  nrv_gemm_tn_bf16 is this call followed by nrv_splitk_reduce.
 *   nrv_splitk_reduce: the stand-alone reduction of a job (nothing when pending == 0).
 *   nrv_gemm_nt_bf16_side: nrv_gemm_nt_bf16 that also completes `job` on the same stream.  When the admission rule holds the
 *     GEMM launch carries the job (*fused = 1); otherwise nrv_splitk_reduce runs first and the plain GEMM after it (*fused = 0).
 *     The GEMM's operands must not alias the job's C, dbias or workspace.
 *   nrv_gemm_nt_side_plan: read-only like nrv_gemm_nt_plan (no GPU needed).  `job_bytes`: the slab bytes of the job
 *     (splits * M * N * 4; 0 for a job of bias sums only).
 *     late        : workgroups that would take shares = grid - tiles % grid; 0 on the plain kernel, with a row remap, with
 *                   tiles <= grid and with tiles % grid == 0;
 *     share_bytes : slab bytes per share, ceil(job_bytes / late) (0 when late == 0);
 *     admitted    : late > 0 and share_bytes <= B * (K / 64) * tile_m / 256, B the library's measured bytes per K-step.
 * ---------------------------------------------------------------------------------------- */
typedef struct nrv_reduce_job {
    const float* slabs; int64_t slab_stride;   /* [splits] slabs of M x N fp32 (NULL: a direct plan), elements between slabs */
    float* C; int64_t ldc;                      /* C = beta * C + sum of the slabs */
    const float* bias_ws; float* dbias;         /* [splits][M] column sums (NULL: no bias gradient) -> dbias */
    int64_t M, N;
    int splits;
    float beta, dbias_beta;
    int pending;
} nrv_reduce_job;
typedef struct nrv_nt_side_plan { int late, admitted; int64_t share_bytes; } nrv_nt_side_plan;
int nrv_gemm_tn_bf16_deferred(const void* A, int64_t lda, const void* B, int64_t ldb,
                              float* C, int64_t ldc, int64_t M, int64_t N, int64_t T, float beta,
                              int64_t a_group, int64_t a_group_stride, int64_t a_row_offset,
                              float* dbias, float dbias_beta,
                              void* workspace, size_t workspace_bytes, nrv_reduce_job* job, void* stream);
int nrv_splitk_reduce(const nrv_reduce_job* job, void* stream);
int nrv_gemm_nt_bf16_side(const void* A, int64_t lda, const void* B, int64_t ldb,
                          void* C, int c_dtype, int64_t ldc,
                          int64_t M, int64_t N, int64_t K,
                          int epilogue, const float* bias,
                          const void* aux, int aux_dtype, int64_t ld_aux, int64_t aux_row_mod,
                          void* aux_out, int64_t ld_aux_out,
                          int64_t out_group, int64_t out_group_stride, int64_t out_row_offset,
                          const nrv_reduce_job* job, int* fused, void* stream);
int nrv_gemm_nt_side_plan(int64_t M, int64_t N, int64_t K, int epilogue, int remap, int64_t job_bytes, nrv_nt_side_plan* plan);

/* Column sum (bias gradient of nn.Linear's backward): out[n] = beta*out[n] + sum_t X[t,n].
 *   X bf16 [T,N] ld; N % 8 == 0.  workspace: nrv_colsum_workspace(T, N) bytes. */
size_t nrv_colsum_workspace(int64_t T, int64_t N);
int nrv_colsum_bf16(const void* X, int64_t ld, float* out, int64_t T, int64_t N, float beta,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head self-attention (replaces simple_vit.py:68-75 -- chunk/rearrange, q k^T * scale,
 * Softmax(-1), attn v, rearrange -- and the intended SDPA of utils.py:207-232,568-577).
 *   qkv bf16 [B, N, 3*H*dh] exactly as the QKV projection writes it (feature index =
 *   which*(H*dh) + h*dh + d, simple_vit.py:67-68); out bf16 [B, N, H*dh] ('b h n d -> b n (h d)');
 *   lse fp32 [B, H, N] = log(sum_j exp(scale * q.k_j)) saved for the backward.
 *   Shapes: dh == 64 and 1 <= N <= 256 run the single-pass kernels (the [N,N] score matrix never leaves the CU);
 *   any other N with dh in {32, 64, 80, 96, 128} runs the streaming kernels (online softmax over 64-key tiles:
 *   vit_h_14, 384-px checkpoints, SimpleViT(dim_head=...)); everything else returns NRV_ERR_SHAPE.
 *   layout (ABI 11): 0 = the row-major tensors above.  NRV_ATTN_QKV_BLOCKED: qkv (and dqkv) as [3*H][B*N][dh] -- the 3 H
 *   column blocks of dh features of the projection's [B*N, 3*H*dh] output each stored as their own contiguous [B*N, dh]
 *   matrix, so that the q / k / v slice of one (batch, head) is ONE contiguous N*dh*2 bytes instead of N segments of dh*2
 *   bytes at a 3*H*dh*2-byte stride.  NRV_ATTN_OUT_BLOCKED: out (and dout) as [H][B*N][dh] likewise.  The blocked forms are
 *   what nrv_gemm_nt_bf16 writes with c_block / reads with a_block; single-pass shapes (dh 64, N <= 256) only. */
#define NRV_ATTN_QKV_BLOCKED 1
#define NRV_ATTN_OUT_BLOCKED 2
int nrv_attn_fwd(const void* qkv_bf16, void* out_bf16, float* lse,
                 int B, int N, int H, int dh, float scale, int layout, void* stream);

/* Backward: dqkv bf16 [B, N, 3*H*dh] from dout bf16 [B, N, H*dh]; recomputes P from q,k and lse.
 *   delta_ws: fp32 [B*H*N] scratch (row sums of dout*out). */
int nrv_attn_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                 void* dqkv_bf16, float* delta_ws,
                 int B, int N, int H, int dh, float scale, int layout, void* stream);

/* Introspection only (Recorder-style attention maps, recorder.py:24-31; never on the training path):
 *   probs fp32 [B, H, N, N] = exp(scale * q.k - lse), i.e. the softmax the fused kernels keep on chip. */
int nrv_attn_probs(const void* qkv_bf16, const float* lse, float* probs,
                   int B, int N, int H, int dh, float scale, int layout, void* stream);

/* Attention-weight dropout inside nrv_attn_fwd / _bwd's kernels (vit.py:108: F.dropout(softmax(...), p), with the mask drawn
 * here and regenerated in the backward; nothing of size N^2 is written).  Entry points added under ABI 19.
 *   P = softmax(scale q k^T);  Pd = P o keep / (1 - p_eff);  out = Pd v.  lse, the row maximum and the row sum are those of the
 *   undropped row (bit-identical to nrv_attn_fwd's); P o keep is rounded to bf16 as the MFMA operand and 1 / (l (1 - p_eff)) is
 *   applied in fp32 at the end.  Backward with M = keep / (1 - p_eff): dV = (P o M)^T dO, dS = P o (M o (dO v^T) - delta),
 *   delta = rowsum(dO o out) as without dropout.  A query whose keys are all dropped has out and dq exactly zero.
 *   Shapes and pointers as nrv_attn_fwd / _bwd with layout 0 (row-major only).  seed_dev: 64 bits in DEVICE memory (8-byte
 *   aligned), read by the kernels when they run, so a captured graph draws a new mask per replay.
 *
 *   Decisions.  T = nrv_attn_drop_threshold(p) = floor(p * 2^16 + 1/2) (p taken as the float it is passed as), p_eff = T / 2^16;
 *   T = 0 runs the plain kernels (bit-identical results).  keep(seed, g, q, k) for g = b * H + h is a stateless function of
 *   exactly these four values; all arithmetic is on uint32, wrapping:
 *     fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16          (murmur3's finaliser)
 *     head(c) = fmix(fmix(fmix(seed_lo + c) ^ seed_hi) + g)           seed_lo / seed_hi = the low / high 32 bits of the seed
 *     row keys of query q:  a0 = fmix(head(0x9E3779B9) ^ q),  a1 = fmix(head(0x7F4A7C15) ^ q)
 *     word of (q, key pair kp = k >> 1):
 *         t = a0 + kp * 0x9E3779B9;  t ^= t >> 16;  t *= 0x85EBCA6B;  t ^= a1;  t ^= t >> 13;  t *= 0xC2B2AE35;  t ^= t >> 16
 *     r(q, k) = bits 16 (k & 1) .. 16 (k & 1) + 15 of the word;   keep  <=>  r >= T
 *   The row keys cost eight multiplies once per (query, kernel); a word costs two multiplies and decides two keys of one
 *   query.  The query-owner kernels (forward, dQ) draw two words per four keys of a lane; the key-owner kernels (dK / dV), whose
 *   lanes hold four queries of one key, read the row keys from LDS and draw four words per four elements.
 *   nrv_attn_drop_mask writes the decisions themselves, uint8 [B, H, N, N] (1 = kept), for tests and for the composed path.
 *   Errors before any launch: NRV_ERR_NULL, NRV_ERR_SHAPE (shape; p < 0, p >= 1, NaN, or a T of 65536), NRV_ERR_ALIGN. */
int nrv_attn_drop_threshold(float p);   /* T in [0, 65535], or NRV_ERR_SHAPE */
int nrv_attn_drop_fwd(const void* qkv_bf16, void* out_bf16, float* lse, const uint64_t* seed_dev, float p,
                      int B, int N, int H, int dh, float scale, void* stream);
int nrv_attn_drop_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                      void* dqkv_bf16, float* delta_ws, const uint64_t* seed_dev, float p,
                      int B, int N, int H, int dh, float scale, void* stream);
int nrv_attn_drop_mask(const uint64_t* seed_dev, float p, unsigned char* keep, int B, int H, int N, void* stream);

/* Attention with memory keys and a score mask (ABI 14; learnable_memory_vit.py:64-86, the Adapter's attention).
 *   Queries: the Nq token rows of qkv bf16 [B, Nq, 3*H*dh] (same layout as nrv_attn_fwd).  Keys / values: those Nq rows
 *   followed by M memory rows, Nk = Nq + M; memory row r of sample b is row b*mem_bstride + r of mem_kv bf16 [*, 2*H*dh]
 *   (k features h*dh + d, v features H*dh + h*dh + d); mem_bstride = 0 (one set for every sample) or M (one set per sample).
 *   mask (optional, NULL = every pair): bit (key & 31) of the 32-bit word b*mask_bstride + h*mask_hstride + q*W + (key >> 5),
 *   W = ceil(Nk / 32), 1 = may attend; strides in words, 0 = broadcast.  A masked score is -FLT_MAX (masked_fill of the
 *   reference), so a query whose keys are all masked gets uniform weights over the Nk keys; its lse is written as -FLT_MAX.
 *   dh in {32, 64, 80, 96, 128}, any Nq >= 1, M >= 0; out bf16 [B, Nq, H*dh]; lse fp32 [B, H, Nq] (natural log).
 *   Backward: dqkv bf16 [B, Nq, 3*H*dh] (token rows); dmem fp32 [B*M, 2*H*dh] per-sample gradient of the memory rows' k / v;
 *   dmem_sum (optional, shared memories only) fp32 [M, 2*H*dh] = that gradient summed over the batch in a fixed order (groups
 *   of 16 samples, then the groups); dmem is then its scratch and holds partial sums afterwards.
 *   delta_ws fp32 [B*H*Nq] scratch.  Deterministic (no atomics). */
int nrv_attn_mem_fwd(const void* qkv_bf16, const void* mem_kv_bf16, int64_t mem_bstride, int M,
                     const uint32_t* mask, int64_t mask_bstride, int64_t mask_hstride,
                     void* out_bf16, float* lse, int B, int Nq, int H, int dh, float scale, void* stream);
int nrv_attn_mem_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                     const void* mem_kv_bf16, int64_t mem_bstride, int M,
                     const uint32_t* mask, int64_t mask_bstride, int64_t mask_hstride,
                     void* dqkv_bf16, float* dmem_f32, float* dmem_sum_f32, float* delta_ws,
                     int B, int Nq, int H, int dh, float scale, void* stream);
/* bool / uint8 [rows, cols] (non-zero = 1) -> the bit words above: uint32 [rows, ceil(cols / 32)] */
int nrv_mask_pack_bits(const void* mask_u8, uint32_t* bits, int64_t rows, int cols, void* stream);

/* "robust" attention (robust=True): softmax followed by Sinkhorn normalisation -- 3 x (row /, column /) and a final
 * row / -- utils.py:1025-1037, wired at simple_vit.py:56-57.  Same layouts as nrv_attn_fwd.
 *   scalings fp32 [B, H, 7, N]: the row / column scaling vectors a1 b1 a2 b2 a3 b3 a4 (cumulative: after step t, P = diag(a_t) softmax(S) diag(b_t); the final matrix is diag(a4) softmax(S) diag(b3)),
 *   saved with lse for the backward.  dh == 64, N <= 256 (the head's [N,N] matrix stays on chip); other shapes return
 *   NRV_ERR_SHAPE -- the host side composes them from nrv_bgemm + nrv_sinkhorn_fwd / bwd (kernels.attn_sinkhorn_*).
 *   The backward is one kernel and needs no scratch (ABI 8). */
int nrv_attn_sinkhorn_fwd(const void* qkv_bf16, void* out_bf16, float* lse, float* scalings,
                          int B, int N, int H, int dh, float scale, void* stream);
int nrv_attn_sinkhorn_bwd(const void* qkv_bf16, const void* dout_bf16, const float* lse, const float* scalings,
                          void* dqkv_bf16, int B, int N, int H, int dh, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Shifted-window attention of the Swin Transformer (ABI 15; swin.py:165-267 between the QKV and output Linears: torch.roll,
 * window partition, q * dh^-0.5 @ k^T, + relative-position bias, + the -100 shift mask, softmax or Sinkhorn (swin.py:239-246),
 * @ v, reverse partition, reverse roll).
 *   The grid is the PADDED map pH x pW (multiples of Wh, Ww); its tokens are rows b*pH*pW + y*pW + x.
 *   qkv bf16 [B*pH*pW, 3C] as the QKV GEMM writes it: feature which*C + h*dh + d (swin.py:187-189), dh = C / heads.
 *   Slot (i, j) of window (wy, wx) is token ((wy*Wh + i + sh) mod pH, (wx*Ww + j + sw) mod pW); out bf16 [B*pH*pW, C] is written
 *   to the same token rows, so the roll and the partition and their reverses are index arithmetic (no permuted copy).
 *   table fp32 [(2Wh-1)(2Ww-1), heads] (relative_position_bias_table, indexed (dy + Wh-1)(2Ww-1) + dx + Ww-1 for the coordinate
 *   difference query - key, swin.py:330-347).  sh, sw: the shift AFTER the reference's rule that zeroes it on an axis the window
 *   covers (swin.py:157-161); the -100 mask between shift regions (swin.py:203-236) is applied when sh + sw > 0.
 *   robust = 0: softmax; 1: softmax, 3 x (row /, column /), row / over the window matrix (padded slots take part).
 *   stats fp32 [B*pH*pW, heads, S]: S = 1 (softmax: the row lse) or 8 (robust: lse, a1, b1, a2, b2, a3, b3, a4 -- the cumulative
 *   scalings of nrv_attn_sinkhorn_fwd, a_t of the token as a query, b_t as a key).  Saved for the backward; nothing of size
 *   [windows, heads, N, N] is stored.
 *   Shapes: dh in {32, 64}, Wh * Ww <= 64, (2Wh-1)(2Ww-1) <= 225, 0 <= sh < Wh, 0 <= sw < Ww; else NRV_ERR_SHAPE.
 *   qkv / out / dout / dqkv 16-byte aligned.
 * Backward: dqkv bf16 [B*pH*pW, 3C] (every row written), dtable fp32 [(2Wh-1)(2Ww-1), heads] = the score gradient summed over
 *   batch and windows and folded through the index: per-workgroup partials over fixed chunks of 8 windows in `workspace`
 *   (nrv_window_attn_bwd_workspace bytes), then a fixed-order sum per entry.  Deterministic (no atomics). */
int nrv_window_attn_fwd(const void* qkv_bf16, const float* table, void* out_bf16, float* stats,
                        int B, int pH, int pW, int C, int heads, int Wh, int Ww, int sh, int sw, int robust, void* stream);
size_t nrv_window_attn_bwd_workspace(int B, int pH, int pW, int C, int heads, int Wh, int Ww);
int nrv_window_attn_bwd(const void* qkv_bf16, const float* table, const void* dout_bf16, const float* stats,
                        void* dqkv_bf16, float* dtable, void* workspace, size_t workspace_bytes,
                        int B, int pH, int pW, int C, int heads, int Wh, int Ww, int sh, int sw, int robust, void* stream);

/* Stochastic depth, row mode (ABI 15; torchvision StochasticDepth(p, "row") at swin.py:519,532-533): one factor per sample,
 * f = keep[r / rows_per_sample] / survival (keep fp32 [samples], 0 or 1, the caller's data; survival = 1 - p > 0).
 *   nrv_sd_add_f32   : out = x + y * f          fp32 [rows, dim] (out may alias x or y)
 *   nrv_sd_scale_bf16: out_bf16 = bf16(dy * f)  the branch gradient of the same add (feeds the branch's GEMMs)
 *   dim % 4 == 0, rows % rows_per_sample == 0. */
int nrv_sd_add_f32(const float* x, const float* y, const float* keep, float* out, float survival,
                   int64_t rows, int64_t rows_per_sample, int dim, void* stream);
int nrv_sd_scale_bf16(const float* dy, const float* keep, void* out_bf16, float survival,
                      int64_t rows, int64_t rows_per_sample, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * LeViT (ABI 16; levit.py).  Every Conv2d / Linear of LeViT is followed by a BatchNorm in training mode that normalises over
 * all token rows; the stem keeps its activations as NHWC rows, so Conv2d_BN (levit.py:57-100) and Linear_BN (:103-134) are
 * both "GEMM on rows (nrv_gemm_nt_bf16, fp32 out) -> BN over rows".
 *
 * Batch norm over rows, y fp32 [T, C] contiguous (replaces BatchNorm2d / BatchNorm1d at levit.py:70-71,106-107,133 and their
 * backward).  C % 4 == 0, T <= 2^24; y, residual, out_f32 16-byte aligned, out_bf16 8-byte aligned.
 *   nrv_bn_stats : per column mean and biased variance from per-chunk (count, mean, M2) partials merged in a fixed order (Chan);
 *                  mean, invstd = 1 / sqrt(var + eps) [C]; stat [3, C] = the combined (count, mean, M2) (what a cross-rank
 *                  all-reduce would merge); running_mean / running_var (both or neither) updated with `momentum` and the
 *                  unbiased variance.  workspace: nrv_bn_workspace(T, C) bytes.
 *   nrv_bn_apply : z = gamma (y - mean) * inv + beta, inv = scale (scale_is_var = 0: invstd of nrv_bn_stats) or
 *                  1 / sqrt(scale + eps) (scale_is_var = 1: the running variance, eval mode); act 1: z = hardswish(z);
 *                  keep (optional, fp32 [T / rows_per_sample]): z *= keep[r / rows_per_sample] / survival (row-mode drop-path,
 *                  levit.py:187-193); residual (optional, fp32 [T, C]): z += residual.  Stores out_f32 and / or out_bf16.
 *   nrv_bn_bwd   : dz = upstream (dz_dtype fp32|bf16 [T, C]) * hardswish'(z) (act 1) * keep factor; dgamma = sum dz x^,
 *                  dbeta = sum dz (fixed-order partials); dy_bf16 = gamma inv (dz - mean(dz) - x^ mean(dz x^)) (training = 1) or
 *                  gamma inv dz (training = 0).  Same workspace.  Deterministic (no atomics). */
size_t nrv_bn_workspace(int64_t T, int C);
int nrv_bn_stats(const float* y, int64_t T, int C, float eps, float momentum,
                 float* mean, float* invstd, float* stat, float* running_mean, float* running_var,
                 void* workspace, size_t workspace_bytes, void* stream);
int nrv_bn_apply(const float* y, const float* mean, const float* scale, int scale_is_var, float eps,
                 const float* gamma, const float* beta, int act,
                 const float* residual, const float* keep, float survival, int64_t rows_per_sample,
                 float* out_f32, void* out_bf16, int64_t T, int C, void* stream);
int nrv_bn_bwd(const void* dz, int dz_dtype, int act, const float* keep, float survival, int64_t rows_per_sample,
               const float* y, const float* mean, const float* scale, int scale_is_var, float eps,
               const float* gamma, const float* beta, int training,
               float* dgamma, float* dbeta, void* dy_bf16,
               void* workspace, size_t workspace_bytes, int64_t T, int C, void* stream);

/* Convolution as unfold + GEMM (the b16 stem, levit.py:166-175: Conv2d(ks 3, stride 2, pad 1, no bias)).
 *   nrv_conv_unfold: src = NCHW image (src_layout NRV_CONV_NCHW, fp32|bf16) or NHWC rows bf16 [B*H*W, C] (NRV_CONV_NHWC) ->
 *                    cols bf16 [B*Ho*Wo, KP], feature (ky, kx, c), KP = ks*ks*C rounded up to 8, zero padding and zero
 *                    columns >= ks*ks*C.  The GEMM weight image is the Conv2d weight permuted to [Cout, ks, ks, C].
 *   nrv_conv_fold  : the input gradient, dx fp32 NHWC rows [B*H*W, C] from dcols bf16 [B*Ho*Wo, KP], in gather form: each
 *                    input element sums its (ky, kx) contributions in ky-then-kx order (no scatter, no atomics).
 *   Ho = (H + 2 pad - ks) / stride + 1; ks <= 7, pad < ks.  cols 16-byte aligned (and src for NHWC).
 *   nrv_conv_unfold / nrv_conv_fold and nrv_soft_split_fwd / nrv_soft_split_bwd (below) are one unfold / fold kernel pair
 *   (csrc/nrv_misc.hip) with two feature orders: tap-major (ky, kx, c) here, channel-major (c, ky, kx) there. */
#define NRV_CONV_NCHW 0
#define NRV_CONV_NHWC 1
int nrv_conv_unfold(const void* src, int src_dtype, int src_layout, void* cols_bf16,
                    int B, int C, int H, int W, int ks, int stride, int pad, void* stream);
int nrv_conv_fold(const void* dcols_bf16, float* dx, int B, int C, int H, int W, int ks, int stride, int pad, void* stream);

/* LeViT attention with a learned offset bias (levit.py:240-258 Attention, :380-403 AttentionSubsample, between qkv / q, kv and
 * proj): S = kd^-0.5 q k^T + table[h, idx[i, j]]; robust = 0: softmax; 1: softmax, 3 x (row /, column /), row /; O = P V;
 * act = hardswish(O) (the proj's activation, levit.py:229-232).
 *   q / k / v: bf16 rows of sample b, token i, head h at base + (b * Nq|Nk + i) * ld + h * hstride (elements; ld, hstride % 8
 *   == 0, bases 16-byte aligned): Attention's qkv [B*N, H*(2kd + d)] is q = qkv, k = qkv + kd, v = qkv + 2kd, hstride 2kd + d;
 *   AttentionSubsample's q [B*Nq, H*kd] and kv [B*Nk, H*(kd + d)].  table fp32 [H, n_offsets] (attention_biases);
 *   idx int32 [Nq, Nk] (attention_bias_idxs).  out, act bf16 [B*Nq, H*d] (column h*d + j, levit.py:256).
 *   stats fp32 [B*H, nrv_bias_attn_stats_size(Nq, Nk, robust)]: lse [Nq]; Sinkhorn adds a1..a4 [4][Nq] and b1..b3 [3][Nk].
 *   Shapes: Nq <= Nk <= 256, kd in {16, 32}, d in {32, 64, 128}, n_offsets <= 256, Nq * (Nk + 1) <= 39 424 (the fp32 score
 *   matrix of one (sample, head) in LDS); else NRV_ERR_SHAPE.
 * Backward: dact bf16 [B*Nq, H*d] = gradient of act (Hardswish' of the saved out applied on load); dq / dk / dv written in the
 *   layouts of q / k / v (same ld and hstride; every row of every head written).  dtable fp32 [H, n_offsets] = dS summed over the
 *   batch and folded through idx: inv_ptr int32 [n_offsets + 1] / inv_pos int32 [Nq*Nk] list the flat positions i*Nk + j of each
 *   entry; per-(head, entry, sample) partials in workspace (nrv_bias_attn_bwd_workspace bytes), then a fixed-order sum over the
 *   samples.  Deterministic (no atomics). */
size_t nrv_bias_attn_stats_size(int Nq, int Nk, int robust);
int nrv_bias_attn_fwd(const void* q, int64_t ldq, int hq, const void* k, int64_t ldk, int hk,
                      const void* v, int64_t ldv, int hv, const float* table, const int32_t* idx,
                      void* out_bf16, void* act_bf16, float* stats,
                      int B, int heads, int Nq, int Nk, int kd, int dv, int n_offsets, int robust, void* stream);
size_t nrv_bias_attn_bwd_workspace(int B, int heads, int n_offsets);
int nrv_bias_attn_bwd(const void* q, int64_t ldq, int hq, const void* k, int64_t ldk, int hk,
                      const void* v, int64_t ldv, int hv, const float* table, const int32_t* idx,
                      const int32_t* inv_ptr, const int32_t* inv_pos,
                      const void* out_bf16, const void* dact_bf16, const float* stats,
                      void* dq, void* dk, void* dv_out, float* dtable, void* workspace, size_t workspace_bytes,
                      int B, int heads, int Nq, int Nk, int kd, int dv, int n_offsets, int robust, void* stream);

/* ------------------------------------------------------------------------------------------
 * PatchConvNet (ABI 17; patch_convnet.py).  Token-major rows [B*H*W, C]: row b*H*W + y*W + x is the reference's
 * x.transpose(-1, -2).reshape(B, C, H, W) (patch_convnet.py:239-243), so the NCHW convolutions of Conv_blocks_se run on the GEMM's
 * rows without a permuted copy.  C % 8 == 0 and bf16 row pointers 16-byte aligned everywhere.  Every reduction is a fixed-order
 * sum of per-tile partials (no atomics): reruns are bit-identical.
 *
 * Depthwise 3x3 convolution, zero padding, stride 1 (Conv_blocks_se qkv_pos[2:4], patch_convnet.py:229-231):
 *   nrv_dwconv3x3_fwd : d = bf16(gelu_erf(dwconv3x3(a) + bias)), a / d bf16 rows [B*H*W, C]; w fp32 [C, 9] (the Conv2d weight
 *                       [C, 1, 3, 3] viewed flat); sq fp32 [B, C] = per-(sample, channel) sums of the fp32 d: the SE squeeze.
 *   nrv_dwconv3x3_bwd : dd = (dg s[b] + dmean[b] / (H W)) gelu'(pre), pre recomputed from a (nine FMAs); da = the gather of dd
 *                       through the taps, times the 1x1 conv's gelu' when gelu_stream is given (NRV_BF16 [rows, C] of
 *                       NRV_EPI_BIAS_GELU, or NRV_U8 of NRV_EPI_BIAS_GELU_Q8 with C % 64 == 0; NULL: none), stored bf16 so that it
 *                       feeds the 1x1 conv's TN / NT GEMMs directly.  dw fp32 [C, 9], db fp32 [C] (per-sample partials, then the
 *                       samples in order).  workspace: nrv_dwconv3x3_bwd_workspace(B, H, W, C) bytes (fp32 dd and the partials).
 *   B <= 65535, H * W <= 2^24; else NRV_ERR_SHAPE.
 * Squeeze-and-excitation (utils.py:1148-1184), rd = round(C / 4) hidden units, C <= 4096, rd <= 1024, B <= 65535:
 *   nrv_se_fwd   : mean = sq / HW; hid fp32 [B, rd] = relu(W_r mean + b_r) (kept for the backward); s fp32 [B, C] =
 *                  sigmoid(W_e hid + b_e).  W_r fp32 [rd, C], W_e fp32 [C, rd] (the 1x1 Conv2d weights viewed flat).
 *   nrv_se_apply : g = bf16(d s[b]): the A operand of the block's last 1x1 conv.  s 16-byte aligned.
 *   nrv_se_bwd   : ds = sum over the H W rows of dg d (fixed order), dz = ds s (1 - s), dp = relu'(hid) W_e^T dz; dmean fp32
 *                  [B, C] = W_r^T dp (the gradient of the mean, consumed by nrv_dwconv3x3_bwd); dW_e = sum_b dz hid^T,
 *                  db_e = sum_b dz, dW_r = sum_b dp mean^T, db_r = sum_b dp, each over the samples in order.
 *                  workspace: nrv_se_bwd_workspace(B, C, rd) bytes.
 * LayerScale residual (patch_convnet.py:211-217, 262-265) with row-mode drop path, f = keep[r / rows_per_sample] / survival
 * (keep fp32 [rows / rows_per_sample], optional: NULL means f = 1), C % 4 == 0, x / y / gamma / out 16-byte aligned:
 *   nrv_ls_add_f32 : out = x + f gamma y (fp32 rows; out may alias x).
 *   nrv_ls_bwd     : dz_bf16 = bf16(dy f gamma); dgamma = sum over rows of dy f y (per-128-row partials, then in order).
 *                    workspace: nrv_ls_bwd_workspace(rows, C) bytes; rows <= 128 * 65535.
 * nrv_dgelu_rows : out_bf16 = dx gelu'(stream), dx fp32 [rows, C], the stream as in nrv_dwconv3x3_bwd (the ConvStem's GELUs, whose
 *                  derivative has to follow nrv_conv_fold).
 * Class attention (Learned_Aggregation_Layer, patch_convnet.py:88-101): per (sample b, head h) one query q against Nk = 1 + Np
 *   keys, S_j = scale q.k_j, P = softmax(S), o = sum_j P_j v_j; lse fp32 [B * heads] = log-sum-exp of S.  Key / value 0 is the
 *   class row of sample b (kc / vc: row b), keys 1 .. Np are its patch rows (kp / vp: rows b*Np .. b*Np + Np - 1): the
 *   cat((x_cls, x)) of patch_convnet.py:215 is never formed.  Head h of a row is columns h*dh .. h*dh + dh - 1; q, out: [B, ld].
 *   Backward: dq (layout of q), dkc / dkp / dvc / dvp (layouts and leading dimensions of kc / kp / vc / vp) as bf16 from dout:
 *   dS = P (dP - sum_j P_j dP_j), dP_j = dout.v_j.  Shapes: dh % 8 == 0, dh <= 1024, Nk <= 4096, every ld >= heads * dh and
 *   % 8 == 0; else NRV_ERR_SHAPE.  kp / vp may be NULL when Np == 0.
 * ---------------------------------------------------------------------------------------- */
int nrv_dwconv3x3_fwd(const void* a, const float* w, const float* bias, void* d_bf16, float* sq,
                      int B, int H, int W, int C, void* stream);
size_t nrv_dwconv3x3_bwd_workspace(int B, int H, int W, int C);
int nrv_dwconv3x3_bwd(const void* a, const float* w, const float* bias, const void* dg, const float* s, const float* dmean,
                      const void* gelu_stream, int gelu_dtype, void* da_bf16, float* dw, float* db,
                      void* workspace, size_t workspace_bytes, int B, int H, int W, int C, void* stream);
int nrv_se_fwd(const float* sq, int HW, const float* wr, const float* br, const float* we, const float* be,
               float* hid, float* s, int B, int C, int rd, void* stream);
int nrv_se_apply(const void* d, const float* s, void* g_bf16, int B, int HW, int C, void* stream);
size_t nrv_se_bwd_workspace(int B, int C, int rd);
int nrv_se_bwd(const void* dg, const void* d, const float* sq, int HW, const float* s, const float* hid,
               const float* wr, const float* we, float* dmean, float* dwr, float* dbr, float* dwe, float* dbe,
               void* workspace, size_t workspace_bytes, int B, int C, int rd, void* stream);
int nrv_ls_add_f32(const float* x, const float* y, const float* gamma, const float* keep, float survival, float* out,
                   int64_t rows, int64_t rows_per_sample, int C, void* stream);
size_t nrv_ls_bwd_workspace(int64_t rows, int C);
int nrv_ls_bwd(const float* dy, const float* y, const float* gamma, const float* keep, float survival, void* dz_bf16,
               float* dgamma, void* workspace, size_t workspace_bytes, int64_t rows, int64_t rows_per_sample, int C, void* stream);
int nrv_dgelu_rows(const float* dx, const void* gelu_stream, int gelu_dtype, void* out_bf16, int64_t rows, int C, void* stream);
int nrv_cls_attn_fwd(const void* q, int64_t ldq, const void* kc, int64_t ldkc, const void* kp, int64_t ldkp,
                     const void* vc, int64_t ldvc, const void* vp, int64_t ldvp, void* out_bf16, int64_t ldo, float* lse,
                     int B, int heads, int Np, int dh, float scale, void* stream);
int nrv_cls_attn_bwd(const void* q, int64_t ldq, const void* kc, int64_t ldkc, const void* kp, int64_t ldkp,
                     const void* vc, int64_t ldvc, const void* vp, int64_t ldvp, const void* dout_bf16, int64_t ldo,
                     const float* lse, void* dq, void* dkc, void* dkp, void* dvc, void* dvp,
                     int B, int heads, int Np, int dh, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone SinkhornAttention(scores)  (the reference's exported module, utils.py:1025-1037, applied to a MATERIALISED
 * score tensor; the training path uses the fused nrv_attn_sinkhorn_* above and never materialises scores):
 *   P = softmax(S, -1); iters x { P /= rowsum(P); P /= colsum(P) }; P /= rowsum(P)        (reference default iters = 3)
 *   scores / out / dout / dscores: fp32 [G, R, C] contiguous (G = product of the leading dimensions), R, C <= 4096.
 *   Saved for the backward: lse fp32 [G, R] (row log-sum-exp of S), avec fp32 [G, iters + 1, R] and bvec fp32 [G, iters, C]:
 *   the cumulative row / column scalings after every step (P = diag(avec[iters]) softmax(S) diag(bvec[iters - 1])).
 *   dscores also serves as the backward's working matrix (it may not alias dout).
 * ---------------------------------------------------------------------------------------- */
int nrv_sinkhorn_fwd(const float* scores, float* out, float* lse, float* avec, float* bvec,
                     int64_t G, int R, int C, int iters, void* stream);
int nrv_sinkhorn_bwd(const float* scores, const float* dout, const float* lse, const float* avec, const float* bvec,
                     float* dscores, int64_t G, int R, int C, int iters, void* stream);

/* ------------------------------------------------------------------------------------------
 * Talking-heads attention on materialised matrices (added to ABI 17 without changing an existing prototype, so the version number stays; cait.py:107-120, CaiT's Attention): the scores of all heads are
 * mixed by mix_heads_pre_attn before the normalisation and the weights by mix_heads_post_attn after it.  With S = q k^T * scale
 * (nrv_bgemm), W1 = mix_heads_pre_attn, W2 = mix_heads_post_attn (fp32 [H, H], indexed [h, g]):
 *     T[b,g] = sum_h W1[h,g] S[b,h]   (cait.py:107-109)     P = attend(T)   (:111)     A[b,g] = sum_h W2[h,g] P[b,h]   (:114-116)
 * and A meets v in nrv_bgemm (:118).  All matrices [B, H, Nq, Nk] contiguous; S, P, dA, dS, in, dout, din fp32; A / out fp32 or
 * bf16 (a_dtype / out_dtype).  1 <= H <= 16, Nq >= 1, 1 <= Nk <= 1025, no divisibility requirement; anything else returns
 * NRV_ERR_SHAPE before a launch.  fp32 arithmetic; no atomics: the parameter gradients are sums of per-workgroup partials
 * (workspace) added in index order by a second kernel, so reruns are bit-identical.
 *   nrv_th_softmax_fwd   attend = softmax(dim = -1) in one pass: reads S once, writes P (kept for the backward) and A.
 *   nrv_th_softmax_bwd   from dA (= dO v^T, nrv_bgemm), P, S: dS = W1-mix of dT, dT = P (dP - <P, dP>), dP = W2-mix of dA;
 *                        dW2[h,g] = sum P[b,h,i,j] dA[b,g,i,j],  dW1[h,g] = sum S[b,h,i,j] dT[b,g,i,j]  (fp32 [H, H]).
 *   nrv_head_mix_fwd     out[b,g] = sum_h W[h,g] in[b,h] alone.  robust=True (SinkhornAttention, utils.py:1025-1037, normalises rows
 *                        AND columns, so it cannot be row-local): nrv_head_mix_fwd(W1) -> nrv_sinkhorn_fwd -> nrv_head_mix_fwd(W2).
 *   nrv_head_mix_bwd     din[b,h] = sum_g W[h,g] dout[b,g];  dW[h,g] = sum in[b,h,i,j] dout[b,g,i,j].
 * ---------------------------------------------------------------------------------------- */
int nrv_th_softmax_fwd(const float* S, const float* W1, const float* W2, float* P, void* A, int a_dtype,
                       int B, int H, int Nq, int Nk, void* stream);
size_t nrv_th_softmax_bwd_workspace(int B, int H, int Nq, int Nk);
int nrv_th_softmax_bwd(const float* dA, const float* P, const float* S, const float* W1, const float* W2, float* dS,
                       float* dW1, float* dW2, void* workspace, size_t workspace_bytes, int B, int H, int Nq, int Nk, void* stream);
int nrv_head_mix_fwd(const float* in, const float* W, void* out, int out_dtype, int B, int H, int Nq, int Nk, void* stream);
size_t nrv_head_mix_bwd_workspace(int B, int H, int Nq, int Nk);
int nrv_head_mix_bwd(const float* dout, const float* in, const float* W, float* din, float* dW, void* workspace,
                     size_t workspace_bytes, int B, int H, int Nq, int Nk, void* stream);

/* ------------------------------------------------------------------------------------------
 * Re-attention on materialised matrices (added to ABI 19 without changing an existing prototype, so the version number stays;
 * deepvit.py:47-53, 67-74, DeepViT's Attention): the attention weights of all heads are mixed by reattn_weights and then normalised
 * by a LayerNorm over the H heads at every (query, key) position.  With S = q k^T * scale (nrv_bgemm), W = reattn_weights (fp32
 * [H, H], indexed [h, g]), gamma / beta = reattn_norm.1.{weight, bias} (fp32 [H]):
 *     P = softmax(S)   (deepvit.py:67-69)     M[b,g] = sum_h W[h,g] P[b,h]   (:73)
 *     mu = mean_g M,  var = mean_g (M - mu)^2  (two-pass),  A[b,g] = (M[b,g] - mu) rsqrt(var + eps) gamma[g] + beta[g]   (:49-53, 74)
 * and A meets v in nrv_bgemm (:78).  All matrices [B, H, Nq, Nk] contiguous; S, P, dA, dS, dP fp32; A fp32 or bf16 (a_dtype).
 * 1 <= H <= 16, Nq >= 1, 1 <= Nk <= 1025, eps > 0, no divisibility requirement; anything else returns NRV_ERR_SHAPE before a
 * launch.  fp32 arithmetic; mu and rstd are never stored (the backward recomputes them from P); no atomics: dW, dgamma, dbeta are
 * sums of per-workgroup partials (workspace, H H + 2 H doubles each) added in index order by a second kernel, so reruns are
 * bit-identical.
 *   nrv_reattn_softmax_fwd   one pass: reads S once, writes P (kept for the backward) and A.
 *   nrv_reattn_softmax_bwd   from dA (= dO v^T, nrv_bgemm) and P: with x^ = (M - mu) rstd and dx^ = dA gamma,
 *                            dM[g] = rstd (dx^[g] - mean_g dx^ - x^[g] mean_g (dx^ x^)),  dP[h] = sum_g W[h,g] dM[g],
 *                            dS = P (dP - <P, dP>_row);  dW[h,g] = sum P[b,h,i,j] dM[b,g,i,j],  dgamma[g] = sum dA x^,
 *                            dbeta[g] = sum dA.
 *   nrv_reattn_norm_fwd/bwd  mixing + LayerNorm alone, for robust=True (SinkhornAttention normalises rows AND columns, so it cannot
 *                            be row-local): nrv_sinkhorn_fwd -> nrv_reattn_norm_fwd, and nrv_reattn_norm_bwd -> dP -> nrv_sinkhorn_bwd.
 * ---------------------------------------------------------------------------------------- */
int nrv_reattn_softmax_fwd(const float* S, const float* W, const float* gamma, const float* beta, float* P, void* A, int a_dtype,
                           int B, int H, int Nq, int Nk, float eps, void* stream);
size_t nrv_reattn_softmax_bwd_workspace(int B, int H, int Nq, int Nk);
int nrv_reattn_softmax_bwd(const float* dA, const float* P, const float* W, const float* gamma, float* dS, float* dW,
                           float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                           int B, int H, int Nq, int Nk, float eps, void* stream);
int nrv_reattn_norm_fwd(const float* P, const float* W, const float* gamma, const float* beta, void* A, int a_dtype,
                        int B, int H, int Nq, int Nk, float eps, void* stream);
size_t nrv_reattn_norm_bwd_workspace(int B, int H, int Nq, int Nk);
int nrv_reattn_norm_bwd(const float* dA, const float* P, const float* W, const float* gamma, float* dP, float* dW,
                        float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                        int B, int H, int Nq, int Nk, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched small GEMM with arbitrary strides (bf16 MFMA, fp32 accumulation): for every (g1 < G1, g2 < G2)
 *   C[g1,g2][m,n] = alpha * sum_k A[g1,g2][m,k] * B[g1,g2][k,n],   element (g1, g2, row, col) of an operand at
 *   base + g1 * b1 + g2 * b2 + row * rs + col * cs  (ELEMENT strides; dtype fp32 or bf16 per operand; operands are rounded to
 *   bf16 when staged).  The matrix products of robust=True attention at the shapes the fused nrv_attn_sinkhorn_* kernels do
 *   not take (N > 256 or dh != 64) -- the reference's own structure there: q k^T * scale (simple_vit.py:70), SinkhornAttention on
 *   the materialised scores (utils.py:1031-1037 = nrv_sinkhorn_fwd / bwd), attn v (simple_vit.py:74), and their backward --
 *   read head slices of the packed projection and write slices of dqkv in place through the strides.  ABI 11.
 * ---------------------------------------------------------------------------------------- */
int nrv_bgemm(const void* A, int a_dtype, int64_t a_rs, int64_t a_cs, int64_t a_b1, int64_t a_b2,
              const void* B, int b_dtype, int64_t b_rs, int64_t b_cs, int64_t b_b1, int64_t b_b2,
              void* C, int c_dtype, int64_t c_rs, int64_t c_cs, int64_t c_b1, int64_t c_b2,
              int G1, int G2, int M, int N, int K, float alpha, void* stream);

/* Launch-plan query of nrv_bgemm (ABI 19).  Read-only like nrv_gemm_nt_plan: it launches nothing, reads no memory and is
 * callable without a GPU; the pointers are only inspected for alignment.  nrv_bgemm takes every host-side decision from the
 * same function, so the answer is the launch's own, and the return code is the one nrv_bgemm gives for the same arguments
 * (NRV_ERR_NULL also for a null `plan`; NRV_ERR_SHAPE for a non-positive dimension or more than 2^31 - 1 workgroups;
 * NRV_ERR_DTYPE).
 *   a_vec, b_vec : the operand is staged by 16-byte vectors (8 bf16 / 4 fp32) along its unit stride: one of its two matrix strides
 *                  is 1 and the address is dword-aligned (bf16: not both strides 1, and the other matrix stride and both batch
 *                  strides even); 0 = element by element.  Two vector operands run the register-double-buffered K loop.
 *   c_vec        : 4 consecutive columns of a C row go out as one store (c_cs == 1, dword-aligned base; bf16: c_rs, c_b1, c_b2 even).
 *   tiles_m, tiles_n : 64 x 64 tiles of C;  blocks = tiles_m * tiles_n * G1 * G2 workgroups. */
typedef struct { int a_vec, b_vec, c_vec, tiles_m, tiles_n; long long blocks; } nrv_bgemm_plan_t;
int nrv_bgemm_plan(const void* A, int a_dtype, int64_t a_rs, int64_t a_cs, int64_t a_b1, int64_t a_b2,
                   const void* B, int b_dtype, int64_t b_rs, int64_t b_cs, int64_t b_b1, int64_t b_b2,
                   const void* C, int c_dtype, int64_t c_rs, int64_t c_cs, int64_t c_b1, int64_t c_b2,
                   int G1, int G2, int M, int N, int K, nrv_bgemm_plan_t* plan);

/* ------------------------------------------------------------------------------------------
 * Patch unfold (replaces einops Rearrange 'b c (h p1) (w p2) -> b h w (p1 p2 c)' simple_vit.py:126-129,
 * and the im2col implied by Conv2d(k=s=p) vit.py:237-242,323).
 *   img [B,C,H,W] (img_dtype fp32|bf16) -> patches bf16 [B*(H/p)*(W/p), FP], FP = C*p*p rounded up to a multiple of 8
 *   (the GEMM's K granularity); columns >= C*p*p are written as zero (vit_h_14, vit.py:512-519: p = 14, 588 -> 592)
 *   layout 0: feature order (p1, p2, c)   [SimpleViT Linear weight order]
 *   layout 1: feature order (c, p1, p2)   [Conv2d weight.reshape(D,-1) order]
 * ---------------------------------------------------------------------------------------- */
#define NRV_PATCH_P1P2C 0
#define NRV_PATCH_CP1P2 1
int nrv_patch_unfold(const void* img, int img_dtype, void* patches_bf16,
                     int B, int C, int H, int W, int p, int layout, void* stream);

/* Weight staging: w fp32 [R,C] -> w_bf16 [R,C] and (optional) wT_bf16 [C,R]; once per optimizer step. */
int nrv_cast_transpose(const float* w, void* w_bf16, void* wT_bf16, int64_t R, int64_t C, void* stream);

/* The same for many matrices in one launch.  jobs_dev: DEVICE array of njobs entries, sorted by tile_start;
 * a matrix of R x C occupies ceil(R/64) * ceil(C/64) consecutive tile numbers starting at tile_start (tiles_c =
 * ceil(C/64)); total_tiles = the sum.  wT_bf16 may be NULL per job.  The caller fills the table (host-side arithmetic only). */
typedef struct nrv_cast_job {
    const float* w;
    void* w_bf16;
    void* wT_bf16;
    int64_t R, C;
    int64_t tile_start;
    int64_t tiles_c;
} nrv_cast_job;
int nrv_cast_transpose_batched(const nrv_cast_job* jobs_dev, int njobs, int64_t total_tiles, void* stream);

/* Elementwise cast fp32 -> bf16 (n % 8 == 0 not required). */
int nrv_cast_f32_bf16(const float* x, void* y_bf16, int64_t n, void* stream);

/* Dropout with p > 0 (training; reference: nn.Dropout at vit.py:100-101 (MLPBlock), :112,125 (EncoderBlock), :154,175 (Encoder)).
 * The keep mask is the caller's data: one byte per element (0 = dropped), n % 8 == 0, 8-byte aligned; scale = 1 / (1 - p).
 *   nrv_dropout_add_f32:  out = x + y * (keep ? scale : 0)   fp32 residual stream x, fp32 branch output y (out may alias x or y)
 *   nrv_mask_mul_bf16:    out = a * (keep ? scale : 0)       bf16 (out may alias a): GELU output, gelu' stream, branch gradient
 *   nrv_mask_mul_f32:     the same on fp32, any n: attention_dropout (vit.py:108, utils.py dropout on the attention weights) is
 *                         COMPOSED -- scores (nrv_bgemm), softmax / Sinkhorn on the materialised matrix (nrv_sinkhorn_fwd), this mask,
 *                         P v (nrv_bgemm) -- not fused into the attention kernels: correct, and as slow as materialising [B,H,N,N]. */
int nrv_dropout_add_f32(const float* x, const float* y, const unsigned char* keep, float* out, float scale, int64_t n, void* stream);
int nrv_mask_mul_bf16(const void* a_bf16, const unsigned char* keep, void* out_bf16, float scale, int64_t n, void* stream);
int nrv_mask_mul_f32(const float* a, const unsigned char* keep, float* out, float scale, int64_t n, void* stream);

/* Row gather / scatter-add of the residual stream (MAE token selection, mae.py:75-76 and its backward):
 *   fwd: out[r, :] = src[index[r], :]   (rows_out rows, dim % 4 == 0, fp32; src has rows_src rows)
 *   bwd: dsrc[index[r], :] += dout[r, :] (indices unique per call => plain stores into a zeroed dsrc of rows_src rows)
 *   index is DEVICE data: an entry outside [0, rows_src) never becomes an address -- the gather writes a zero row for it,
 *   the scatter drops it (ABI 11: the bound is part of the call, a wrong index cannot fault the GPU). */
int nrv_gather_rows_f32(const float* src, const int64_t* index, float* out,
                        int64_t rows_out, int64_t rows_src, int dim, void* stream);
int nrv_scatter_rows_f32(const float* dout, const int64_t* index, float* dsrc,
                         int64_t rows_out, int64_t rows_src, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step on flat fp32 buffers (replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step of the reference
 * harness: examples/CIFAR100.py:90-97,191-192, baseline.py:127).
 *   nrv_sumsq_f32 : out[0] = sum_i x[i]^2 (deterministic two-stage reduction; workspace nrv_sumsq_workspace(n) bytes); x fp32 or bf16
 *   nrv_adamw_f32 : for every i:  g = grad[i] * c,  c = min(1, max_norm / (sqrt(gnorm_sq[0]) + 1e-6))  (c = 1 when gnorm_sq
 *                   is NULL or max_norm <= 0);  p *= 1 - lr * weight_decay;  m = beta1 m + (1 - beta1) g;
 *                   v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *                   -- torch.optim.AdamW (amsgrad = False, maximize = False) arithmetic, step >= 1.  A NaN gnorm_sq gives
 *                   c = NaN (the min lets it through): every p, m and v becomes NaN, as after clip_grad_norm_; +inf gives c = 0.
 *   Hyper-parameters are doubles (1 - beta and the bias corrections are formed in double, then rounded, as torch does).
 *   p, m, v: fp32 [n], 16-byte aligned; grad: fp32 or (ABI 11) bf16 [n] -- the reduced slabs of a bf16 gradient exchange are read in
 *   place, no conversion pass back into an fp32 buffer; gnorm_sq: DEVICE pointer to one float (no host round trip).
 *   step_scalars (optional, DEVICE pointer to 3 floats): { 1 - lr * weight_decay, lr / (1 - beta1^step),
 *   1 / sqrt(1 - beta2^step) } read by the kernel INSTEAD of the values derived from lr / weight_decay / step -- a captured
 *   HIP graph replays one launch with every step's learning rate and bias corrections (the caller refreshes the 3 floats).
 * ---------------------------------------------------------------------------------------- */
size_t nrv_sumsq_workspace(int64_t n);
int nrv_sumsq_f32(const void* x, int x_dtype, int64_t n, float* out, void* workspace, size_t workspace_bytes, void* stream);
int nrv_adamw_f32(float* p, const void* grad, int grad_dtype, float* m, float* v, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                  const float* gnorm_sq, float max_norm, const float* step_scalars, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tokens-to-token pieces (T2T-ViT, t2t.py:58-93; added to ABI 17, no existing prototype changed).
 *   nrv_soft_split_fwd: nn.Unfold(ks, stride, pad) on token-major rows.  src = NCHW image (NRV_SPLIT_NCHW, fp32|bf16; ld_src
 *                    ignored) or bf16 token rows [B*H*W, ld_src] (NRV_SPLIT_ROWS, ld_src >= C: RearrangeImage is the
 *                    addressing) -> cols bf16 [B*Ho*Wo, KP], feature c*ks*ks + ky*ks + kx (nn.Unfold's order; nrv_conv_unfold
 *                    writes (ky, kx, c)), KP = ks*ks*C rounded up to 8.  Taps outside the image and columns >= ks*ks*C are
 *                    zeros.  A copy: bf16 sources arrive bit-exact, fp32 ones rounded to nearest even.  The channel-major
 *                    instantiation of the unfold / fold kernel pair behind nrv_conv_unfold / nrv_conv_fold.
 *   nrv_soft_split_bwd: its input gradient, a fold in gather form: dx fp32 rows [B*H*W, ld_dx] (ld_dx >= C; columns >= C
 *                    are written as zeros) from dcols bf16 [B*Ho*Wo, KP].  Each element sums the at most ceil(ks / stride)^2
 *                    windows that cover it, ky then kx ascending: no scatter, no atomics, reruns are bit-identical.
 *   Ho = (H + 2 pad - ks) / stride + 1; ks <= 7, pad < ks; else NRV_ERR_SHAPE.  cols 16-byte aligned.
 *   nrv_layernorm_pad_fwd / _bwd: nn.LayerNorm over the first n columns of rows stored with stride ld (n <= 4096, ld >= n,
 *                    ld % 8 == 0, ld <= 2^20; else NRV_ERR_SHAPE): statistics over n, gamma / beta / dgamma / dbeta fp32 [n],
 *                    columns n .. ld - 1 of y / dx written as zeros (the zero pad columns of odd feature widths: 147 in 152,
 *                    1323 in 1328).  Otherwise the arguments of nrv_layernorm_fwd / _bwd; dgamma / dbeta are per-slab column
 *                    sums added in slab order (deterministic).  workspace: nrv_layernorm_pad_bwd_workspace(rows, n) bytes.
 *   nrv_attn_wide_fwd / _bwd: the streaming softmax attention of nrv_attn_fwd / _bwd (same tensors, online softmax over
 *                    64-key tiles, LSE saved, P recomputed in the backward, no atomics) for head dims 128 < dh <= 192 with
 *                    dh % 8 == 0 and any N: the [N, N] matrix is never written.  The upper limit is the 64 KB of static
 *                    LDS (two [64][192] bf16 tiles + statistics = 49 664 bytes; 256 columns would need 66 048).  Anything
 *                    else returns NRV_ERR_SHAPE before a launch; wider heads run the composed path (nrv_bgemm +
 *                    nrv_sinkhorn_fwd with 0 iterations).  delta_ws: fp32 [B*H*N] scratch.
 * ---------------------------------------------------------------------------------------- */
#define NRV_SPLIT_NCHW 0
#define NRV_SPLIT_ROWS 1
int nrv_soft_split_fwd(const void* src, int src_dtype, int src_layout, int64_t ld_src, void* cols_bf16,
                       int B, int C, int H, int W, int ks, int stride, int pad, void* stream);
int nrv_soft_split_bwd(const void* dcols_bf16, float* dx, int64_t ld_dx, int B, int C, int H, int W, int ks, int stride,
                       int pad, void* stream);
int nrv_layernorm_pad_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y_bf16, float* mean,
                          float* rstd, int64_t rows, int n, int64_t ld, float eps, void* stream);
size_t nrv_layernorm_pad_bwd_workspace(int64_t rows, int n);
int nrv_layernorm_pad_bwd(const void* dy_bf16, const void* x, int x_dtype, const float* gamma, const float* mean,
                          const float* rstd, const void* dres, int dres_dtype, float* dx_f32, void* dx_bf16,
                          float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes,
                          int64_t rows, int n, int64_t ld, void* stream);
int nrv_attn_wide_fwd(const void* qkv_bf16, void* out_bf16, float* lse, int B, int N, int H, int dh, float scale,
                      void* stream);
int nrv_attn_wide_bwd(const void* qkv_bf16, const void* out_bf16, const void* dout_bf16, const float* lse,
                      void* dqkv_bf16, float* delta_ws, int B, int N, int H, int dh, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * RvT (ABI 18, added entry points; rvt.py).  Three memory-bound families: every lane moves 16 bytes, the arithmetic is fp32 in
 * registers with ONE bf16 rounding on the store, every sum runs in a fixed order (no atomics): reruns are bit-identical.
 * Shapes are checked first (NRV_ERR_SHAPE), then pointers (NRV_ERR_NULL), then alignment, all before any launch.
 *
 * 2-D axial rotary embedding (rvt.py:12-44, 130-147), in place on the packed qkv bf16 [B*N, 3*H*dh]:
 *   nrv_rotary_fwd : for the token rows t >= lead of every sample (lead = 0 or 1 class rows) and the q block and the k block of
 *                    every head, the first dr features are rotated pairwise: out[2m] = x[2m] c - x[2m+1] s, out[2m+1] =
 *                    x[2m+1] c + x[2m] s with s / c = entry (t - lead, m) of the fp32 tables sin / cos [N - lead, dr / 2] (the
 *                    reference's '(d j)' repeat is this pairing and is never materialised).  Features dr .. dh - 1, the class
 *                    rows and the whole v block keep their bits.
 *   nrv_rotary_bwd : the transposed rotation (s -> -s) on dqkv, same arguments.
 *   dh % 8 == 0, dr % 2 == 0, 2 <= dr <= dh, lead in {0, 1}, N > lead; else NRV_ERR_SHAPE.  qkv and the tables 16-byte aligned.
 * Depthwise ks x ks convolution, ks in {3, 5, 7}, stride 1, zero padding ks / 2, no bias, no activation (SpatialConv's
 * DepthWiseConv2d.net[0], rvt.py:46-78) on token-major bf16 rows [B*(lead + H*W), C]: patch token (y, x) of sample b is row
 * b*(lead + H*W) + lead + y*W + x.  The lead class rows of a sample are never read as neighbours.
 *   nrv_dwconv_fwd : out(p) = bf16(sum_t w[c, t] a(p + off_t)), t = ky * ks + kx ascending; w fp32 [C, ks*ks] (the Conv2d weight
 *                    [C, 1, ks, ks] viewed flat).  The class rows of out are NOT written.
 *   nrv_dwconv_bwd : da = the gather of dout through the flipped taps, bf16, its class rows written as zeros; dw fp32
 *                    [C, ks*ks] = per-sample partials (tokens in row-major order) summed over the samples in index order.
 *                    workspace: nrv_dwconv_bwd_workspace(B, H, W, C, ks) bytes (the partials).
 *   C % 8 == 0, B <= 65535, H * W <= 2^24, lead in {0, 1}; any H, W (planes smaller than the kernel radius included; planes
 *   larger than the 14 x 14 token tile staged in LDS run several tiles); else NRV_ERR_SHAPE.
 * GEGLU (rvt.py:80-83): u bf16 [rows, ld_u] holds [x | g] in its first 2 * hidden columns (the fc1 output with NRV_EPI_BIAS; the
 * gate is the SECOND half).
 *   nrv_geglu_fwd : h bf16 [rows, hidden] = bf16(x gelu_erf(g)).
 *   nrv_geglu_bwd : du bf16 [rows, 2 * hidden]: du[:, :hidden] = dh gelu(g), du[:, hidden:] = dh x gelu'(g), both recomputed
 *                   from u (no saved stream).
 *   hidden % 8 == 0, ld_u >= 2 * hidden, ld_u % 8 == 0; else NRV_ERR_SHAPE.
 * ---------------------------------------------------------------------------------------- */
int nrv_rotary_fwd(void* qkv_bf16, const float* sin_t, const float* cos_t, int B, int N, int lead, int H, int dh, int dr,
                   void* stream);
int nrv_rotary_bwd(void* dqkv_bf16, const float* sin_t, const float* cos_t, int B, int N, int lead, int H, int dh, int dr,
                   void* stream);
int nrv_dwconv_fwd(const void* a, const float* w, void* out_bf16, int B, int H, int W, int lead, int C, int ks, void* stream);
size_t nrv_dwconv_bwd_workspace(int B, int H, int W, int C, int ks);
int nrv_dwconv_bwd(const void* a, const float* w, const void* dout, void* da_bf16, float* dw, void* workspace,
                   size_t workspace_bytes, int B, int H, int W, int lead, int C, int ks, void* stream);
int nrv_geglu_fwd(const void* u_bf16, int64_t ld_u, void* h_bf16, int64_t rows, int hidden, void* stream);
int nrv_geglu_bwd(const void* u_bf16, int64_t ld_u, const void* dh_bf16, void* du_bf16, int64_t rows, int hidden,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * PiT (added to ABI 19 without changing an existing prototype, so the version number stays; pit.py).
 *
 * Pooled depthwise convolution (Pool.downsample.net[0], pit.py:90-106): Conv2d(C, 2C, 3, stride 2, padding 1, groups = C, bias)
 * on token-major rows of the fp32 residual stream x [B*(lead + H*W), C], lead = 0 or 1 class rows in front of every sample's
 * plane (never read as neighbours).  Output planes are Ho = (H - 1) / 2 + 1 by Wo = (W - 1) / 2 + 1; output channel o reads
 * input channel o / 2 (PyTorch's grouping).  w fp32 [2C, 9] (the Conv2d weight [2C, 1, 3, 3] viewed flat), bias fp32 [2C].
 *   nrv_pool_dwconv_fwd : out bf16 [B*Ho*Wo, 2C], dense, no class rows (the A operand of the 1 x 1 convolution's GEMM):
 *                         out = bf16(bias[o] + sum_t w[o, t] x(2 oy - 1 + ky, 2 ox - 1 + kx, o / 2)), t = 3 ky + kx ascending,
 *                         fp32 in registers, one rounding.
 *   nrv_pool_dwconv_bwd : dx fp32 [B*(lead + H*W), C] in gather form: every input element sums the at most 2 x 2 windows that
 *                         cover it times the two output channels of its group, ky then kx then o = 2c, 2c + 1 ascending; the
 *                         class rows of dx are written as zeros.  dw fp32 [2C, 9] and dbias fp32 [2C] = per-sample partials
 *                         (output tokens in row-major order) summed over the samples in index order.  No atomics.
 *                         workspace: nrv_pool_dwconv_bwd_workspace(B, H, W, C) bytes (the partials).
 *   C % 8 == 0, B <= 65535, H * W <= 2^24, lead in {0, 1}, any H, W >= 1; else NRV_ERR_SHAPE.  Shapes are checked first, then
 *   pointers (NRV_ERR_NULL), then the workspace size and the 16-byte alignment of every pointer, all before any launch.
 * Overlapped patch unfold (to_patch_embedding[0]):
 *   nrv_unfold_patches : nn.Unfold(ks, stride) on an NCHW image (fp32 | bf16), no padding, 1 <= stride <= ks <= 32.  cols bf16
 *                        [B*Ho*Wo, KP], feature c ks^2 + ky ks + kx, KP = ks^2 C rounded up to 8, columns >= ks^2 C zeros.
 *                        fp32 sources are rounded to nearest even, bf16 sources are copied.  The kernel of nrv_soft_split_fwd
 *                        (which keeps ks <= 7).  cols 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int nrv_pool_dwconv_fwd(const float* x_f32, const float* w, const float* bias, void* out_bf16, int B, int H, int W, int lead, int C,
                        void* stream);
size_t nrv_pool_dwconv_bwd_workspace(int B, int H, int W, int C);
int nrv_pool_dwconv_bwd(const float* x_f32, const float* w, const void* dout_bf16, float* dx_f32, float* dw, float* dbias,
                        void* workspace, size_t workspace_bytes, int B, int H, int W, int lead, int C, void* stream);
int nrv_unfold_patches(const void* img, int img_dtype, void* cols_bf16, int B, int C, int H, int W, int ks, int stride,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * CCT (added to ABI 19 without changing an existing prototype, so the version number stays; cct.py).
 *
 * ReLU + MaxPool2d on NHWC token rows (Tokenizer, cct.py:182-191).  y [B*H*W, C] is a convolution's output (y_dtype fp32 | bf16),
 * C % 8 == 0; the pool is (pk, ps, pp) with pk in {2, 3}, 1 <= ps <= pk, pp <= pk / 2, H + 2 pp >= pk (likewise W), else
 * NRV_ERR_SHAPE.  Ho = (H + 2 pp - pk) / ps + 1, likewise Wo.
 *   nrv_relu_maxpool_fwd : out_f32 and / or out_bf16 [B*Ho*Wo, C] (at least one) and idx u8 [B*Ho*Wo, C]: the tap ky pk + kx of
 *                          the FIRST maximum among the in-bounds taps, ky then kx ascending; with relu != 0 the mark 255 when
 *                          that maximum is <= 0 (the output is then 0 and no gradient flows): autograd's rule for
 *                          max_pool2d(relu(x)).  Values are copied: the fp32 output of an fp32 input is bit-exact, a bf16 output
 *                          of an fp32 input is one round-to-nearest-even.
 *   nrv_relu_maxpool_bwd : dy bf16 [B*H*W, C] from dout fp32 [B*Ho*Wo, C] and idx, in gather form: every input element sums, oy
 *                          then ox ascending, the dout of the windows that cover it and whose idx names it; fp32 sum, one
 *                          rounding; an element nobody selected is an exact zero.  No atomics.
 *   Shapes first, then pointers (NRV_ERR_NULL), the dtype, then the 16-byte alignment of every pointer, all before any launch.
 * LayerNorm with the fp32 stream on both sides (the post-norm `src = norm1(src)`, cct.py:139, and the head's norm):
 *   nrv_layernorm_f32_fwd : x fp32 [rows, dim] -> y_f32, y_bf16 (optional copy, one rounding of y_f32), mean, rstd [rows];
 *                           two-pass statistics, biased variance, eps inside the sqrt.
 *   nrv_layernorm_f32_bwd : dy fp32 -> dx_f32, dx_bf16 (optional), dgamma, dbeta [dim].  A wave walks max(8, ceil(rows / 4096))
 *                           consecutive rows; the four waves of a workgroup add their column sums in order and write one
 *                           partial row of dgamma / dbeta into the workspace
 *                           (nrv_layernorm_f32_bwd_workspace(rows, dim) bytes); the partial rows are summed in a fixed order.
 *   dim % 8 == 0, 8 <= dim <= 4096, rows >= 1.
 * Sequence pooling (cct.py:286-288): y fp32 [B*n, D], a fp32 [D] (attention_pool.weight), bias fp32 [1] (a device pointer).
 *   nrv_seqpool_fwd : w fp32 [B, n] = softmax over a sample's n tokens of y_n . a + bias (max-subtracted), out fp32 [B, D] =
 *                     sum_n w_n y_n, n ascending.  One workgroup per sample.
 *   nrv_seqpool_bwd : from dout [B, D]: t_n = dout . y_n, dl_n = w_n (t_n - sum_m w_m t_m), dy_n = w_n dout + dl_n a,
 *                     da = sum_b sum_n dl_n y_n, dbias = sum_b sum_n dl_n; per-sample partials in the workspace
 *                     (nrv_seqpool_bwd_workspace(B, D) bytes) summed in a fixed order (lane r of 64 adds samples r, r + 64, ...,
 *                     then the lanes in order: index order for B <= 64).
 *   1 <= n <= 4096, D % 8 == 0, 8 <= D <= 4096, B >= 1.
 * ---------------------------------------------------------------------------------------- */
int nrv_relu_maxpool_fwd(const void* y, int y_dtype, int relu, float* out_f32, void* out_bf16, void* idx_u8, int B, int H, int W,
                         int C, int pk, int ps, int pp, void* stream);
int nrv_relu_maxpool_bwd(const float* dout, const void* idx_u8, void* dy_bf16, int B, int H, int W, int C, int pk, int ps, int pp,
                         void* stream);
int nrv_layernorm_f32_fwd(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_bf16, float* mean,
                          float* rstd, int64_t rows, int dim, float eps, void* stream);
size_t nrv_layernorm_f32_bwd_workspace(int64_t rows, int dim);
int nrv_layernorm_f32_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                          float* dx_f32, void* dx_bf16, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                          int64_t rows, int dim, void* stream);
int nrv_seqpool_fwd(const float* y, const float* a, const float* bias, float* w, float* out, int B, int n, int D, void* stream);
size_t nrv_seqpool_bwd_workspace(int B, int D);
int nrv_seqpool_bwd(const float* dout, const float* y, const float* a, const float* w, float* dy, float* da, float* dbias,
                    void* workspace, size_t workspace_bytes, int B, int n, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Twins-SVT (added to ABI 19 without changing an existing prototype, so the version number stays; twins_svt.py).
 *
 * Sub-sampled global attention (GlobalAttention, twins_svt.py:123-154): every query of a map against the few pooled keys of
 * its sample.  q: bf16 row-major view [B*Nq, ldq] whose first column is head 0's q, head h at column h*dh; k, v: bf16 views
 * [B*Nk, ldk] / [B*Nk, ldv], head-major likewise (separate pointers: the two halves of one to_kv output work).
 *   nrv_subattn_fwd  : out bf16 [B*Nq, H*dh] = softmax(scale q k^T) v, lse fp32 [B, H, Nq].  bf16 operands, fp32 accumulation;
 *                      e = exp(scale s - max) is rounded to bf16 once for the product with v, the row sum adds the unrounded e,
 *                      one rounding on the store.
 *   nrv_subattn_bwd  : from q, k, v, dout bf16 [B*Nq, H*dh] and lse (NOT out: with every key of a row on chip
 *                      dS = P (dP - rowsum(P dP)) needs no saved delta).  dq laid out like q; dk / dv laid out like k / v.
 *                      P and dS are rounded to bf16 once, before dV = P^T dO and dQ = scale dS K, dK = scale dS^T Q.  dK and dV
 *                      are accumulated in fp32 over a workgroup's chunk of query rows, one fp32 partial per chunk goes to the
 *                      workspace (nrv_subattn_bwd_workspace bytes) and a second kernel adds the chunks in index order.  No
 *                      atomics; the chunk length is a constant of the library, so reruns and machines agree bit for bit.
 *   nrv_subattn_plan : chunk = query rows per workgroup, chunks = ceil(Nq / chunk), nk_pad = keys staged on chip (Nk rounded
 *                      up to 32; keys >= Nk are masked, never read).  Read-only, needs no GPU.
 *   dh in {32, 64}, 1 <= Nk <= 128, Nq >= 1, B, H in [1, 65535], ld* >= H*dh and ld* % 8 == 0; else NRV_ERR_SHAPE.  Shapes are
 *   checked first, then pointers (NRV_ERR_NULL), then the workspace size, then the 16-byte alignment of every bf16 base and the
 *   workspace, all before any launch.
 * PEG (twins_svt.py:81-87): x + Conv2d(C, C, ks, padding ks / 2, groups = C)(x) on token-major rows of the fp32 residual
 * stream [B*H*W, C].  w fp32 [C, ks*ks] (the Conv2d weight [C, 1, ks, ks] viewed flat), bias fp32 [C].
 *   nrv_peg_fwd : out fp32 = x + bias[c] + sum_t w[c, t] x(p + off_t), t = ky * ks + kx ascending, taps outside the plane skipped.
 *   nrv_peg_bwd : dx fp32 = dy + the gather of dy through the flipped taps; dw fp32 [C, ks*ks] and dbias fp32 [C] = per-sample
 *                 partials (tokens in row-major order) summed over the samples in index order.  No atomics.
 *                 workspace: nrv_peg_bwd_workspace(B, H, W, C, ks) bytes (the partials).
 *   ks in {3, 5, 7}, C % 8 == 0, B <= 65535, H * W <= 2^24, any H, W >= 1; else NRV_ERR_SHAPE; then NRV_ERR_NULL, the workspace
 *   size and the 16-byte alignment of x / out / dy / dx / bias / workspace.
 * ---------------------------------------------------------------------------------------- */
typedef struct { int chunk, chunks, nk_pad; } nrv_subattn_plan_t;
int nrv_subattn_plan(int Nq, int Nk, int dh, nrv_subattn_plan_t* plan);
int nrv_subattn_fwd(const void* q_bf16, int64_t ldq, const void* k_bf16, int64_t ldk, const void* v_bf16, int64_t ldv,
                    void* out_bf16, float* lse, int B, int H, int Nq, int Nk, int dh, float scale, void* stream);
size_t nrv_subattn_bwd_workspace(int B, int H, int Nq, int Nk, int dh);
int nrv_subattn_bwd(const void* q_bf16, int64_t ldq, const void* k_bf16, int64_t ldk, const void* v_bf16, int64_t ldv,
                    const void* dout_bf16, const float* lse, void* dq_bf16, void* dk_bf16, void* dv_bf16, void* workspace,
                    size_t workspace_bytes, int B, int H, int Nq, int Nk, int dh, float scale, void* stream);
int nrv_peg_fwd(const float* x_f32, const float* w, const float* bias, float* out_f32, int B, int H, int W, int C, int ks,
                void* stream);
size_t nrv_peg_bwd_workspace(int B, int H, int W, int C, int ks);
int nrv_peg_bwd(const float* x_f32, const float* w, const float* dy_f32, float* dx_f32, float* dw, float* dbias, void* workspace,
                size_t workspace_bytes, int B, int H, int W, int C, int ks, void* stream);

/* CUs the GEMM launches leave free (process-wide; default 0; returns the previous value, or a negative error code when n is
 * negative or leaves fewer than 8 CUs).  The NT GEMM is persistent (one workgroup per CU for the whole launch) and the TN
 * GEMM sizes its token splits to one round of the CUs: with a collective's kernels resident on some CUs (RCCL all-reduce
 * overlapped with the backward, parallel.GradReducer) a grid sized for ALL CUs runs its last workgroups in a second round,
 * i.e. takes twice as long.  With n > 0 both kernels plan for (CUs - n).  Single-GPU runs never call this.
 * A different value changes the TN split count, hence the summation order of weight gradients (deterministic per value). */
int nrv_set_reserved_cus(int n);

/* Hardware-assumption probes used by tests/test_kernels_gpu.py (test_probe_*) (MFMA lane maps, transposed LDS read,
 * LDS-DMA layout and out-of-range zero fill).  out: fp32 scratch written by a single wave. */
int nrv_probe(int which, const void* in, void* out, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NRV_H_ */
