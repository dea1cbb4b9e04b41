/*
 * mca_hip.h — C ABI of libmca_hip.so: the gfx950 (MI355X) kernels behind the MCA / MMA fusion
 * training step.
 *
 * The reference (josiahbjorgaard/mca-paper) has no FFI: its hot path is stock ATen ops called from
 * Python.  Each entry point below therefore names the reference Python lines whose
 * arithmetic it replaces.  Conventions:
 *   - plain pointers to DEVICE memory, sizes as integers, `stream` is a hipStream_t passed as void*;
 *   - caller allocates every output and workspace; nothing is allocated, freed or synchronised here,
 *     so every call is stream-ordered and graph-capturable;
 *   - return value 0 = launched, negative = argument error (MCA_E_*), nothing launched;
 *   - bf16 tensors are uint16_t (raw bits, round-to-nearest-even); all accumulation is fp32.
 *   - "ld" = leading dimension in ELEMENTS of a row-major matrix.
 */
#ifndef MCA_HIP_H
#define MCA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mca_stream_t;

#define MCA_OK 0
#define MCA_E_BADARG (-1)
#define MCA_E_ALIGN (-2)
#define MCA_E_UNSUPPORTED (-3)
#define MCA_E_LAUNCH (-4)

/* version / build info: returns a static string */
const char* mca_version(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM  (all Linear layers: encoders.py:190, model.py:49-51,69-71; their autograd backward)
 * --------------------------------------------------------------------------------------------- */
/* C[M,N] = A[M,K] · B[N,K]^T (+ bias[N]) (+ residual[M,N]).   K % 64 == 0, lda/ldb % 8 == 0.
 * out_bf16 != 0: C is bf16, else fp32.  bias / residual may be NULL.  residual rows are indexed
 * row % res_period when res_period > 0 (broadcast over batch), else row.                         */
int mca_gemm_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb,
                void* C, int64_t ldc, int out_bf16,
                const float* bias, const float* residual, int64_t ldres, int64_t res_period,
                int64_t M, int64_t N, int64_t K, mca_stream_t stream);

/* The same product, bf16, stored COLUMN-BLOCKED: column n of row m at C + (n / 64) * cbs + m * 64 + n % 64, i.e. N / 64 slabs of
 * [M][64], cbs >= M * 64 elements apart - the head-major form the attention kernels read in place (mca_attn_layout).  Exactly the
 * values mca_gemm_nt writes for the same operands; nothing outside rows 0 .. M - 1 of a slab is touched.  Shapes of the 256 x 256
 * persistent kernel only: M >= 2048, N % 256 == 0, K >= 192, K % 32 == 0, C % 16 == 0, cbs % 8 == 0 (MCA_E_UNSUPPORTED otherwise:
 * the caller keeps mca_gemm_nt and the row-major layout; mca_dbg_plan_gemm_nt_cb answers without a launch).                     */
int mca_gemm_nt_cb(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t cbs,
                   int64_t M, int64_t N, int64_t K, mca_stream_t stream);

/* C[M,N] (fp32) = A[M,K]·B[N,K]^T + LayerNorm(x)[M,N], the LayerNorm (model.py:24-31, beta = 0) recomputed in the epilogue
 * as (x - mean[m]) * rstd[m] * gamma[n] from the saved pre-norm tensor and the statistics mca_layernorm_fwd wrote: the
 * residual branches x = Attn(LN(x)) + LN(x), x = FF(LN(x)) + LN(x) of MCALayer.forward (model.py:117-122) without the normed
 * fp32 tensor ever being stored.  M >= 2048, N % 128 == 0, K >= 512 (MCA_E_UNSUPPORTED otherwise: use mca_gemm_nt).      */
int mca_gemm_nt_lnres(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                      const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                      int64_t M, int64_t N, int64_t K, mca_stream_t stream);

/* Fused data-gradient GEMM + GEGLU backward (model.py:35-54 autograd): dg = A[M,K]·B[ip,K]^T is never stored;
 * dh[:, n] = dg*gelu(gate), dh[:, ip+n] = dg*a*gelu'(gate) with h = [a | gate].  h, dh: bf16 [M, 2*ip], row stride ldh. */
int mca_gemm_nt_geglu_bwd(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* h,
                          uint16_t* dh, int64_t ldh, int64_t ip, int64_t M, int64_t K, mca_stream_t stream);

/* Fused FF1 GEMM + GEGLU forward (model.py:35-38,49-54): h[M, 2*ip] = A[M,K]·W1[2*ip,K]^T (bf16, both halves kept for the
 * backward) and g[M, ip] = h[:, :ip] * gelu(h[:, ip:]) in one pass (h is not read back).  ip % 64 == 0, ldh >= 2*ip,
 * ldg >= ip, both % 8 == 0.                                                                                          */
int mca_gemm_nt_geglu_fwd(const uint16_t* A, int64_t lda, const uint16_t* W1, int64_t ldb, uint16_t* h, int64_t ldh,
                          uint16_t* g, int64_t ldg, int64_t ip, int64_t M, int64_t K, mca_stream_t stream);

/* The saved-factor forms of the two fusions above: the forward keeps the two factors its backward multiplies by instead
 * of h, in h's place (same shape [M, 2*ip], bf16, same strides):
 *     s[:, 0:ip]    = bf16(gelu(gate_b))
 *     s[:, ip:2*ip] = bf16(a_b * gelu'(gate_b))
 * with a_b, gate_b the bf16-rounded halves of A·W1^T, i.e. exactly what the unsaved form stores as h; g is bit for bit
 * the g of the unsaved form.  Where both halves of h are zero (the padded columns ip > I) both factors are zero.
 * The backward is then dh[:, n] = bf16(dg * s[:, n]), dh[:, ip+n] = bf16(dg * s[:, ip+n]): no gelu is evaluated again,
 * at one more bf16 rounding (2^-9 relative) per element of dh than the unsaved pair.  Arguments, their rules, the kernels'
 * grids and the fall-backs are those of the siblings, s in the place of h; an s must only ever meet a _saved backward. */
int mca_gemm_nt_geglu_fwd_saved(const uint16_t* A, int64_t lda, const uint16_t* W1, int64_t ldb, uint16_t* s, int64_t lds,
                                uint16_t* g, int64_t ldg, int64_t ip, int64_t M, int64_t K, mca_stream_t stream);
int mca_gemm_nt_geglu_bwd_saved(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* s,
                                uint16_t* dh, int64_t ldh, int64_t ip, int64_t M, int64_t K, mca_stream_t stream);

/* Data-gradient GEMM + LayerNorm backward in one launch (model.py:24-31 autograd behind a Linear's): dy[M,N] = A[M,K]·B[N,K]^T
 * (+ residual[M,N], may be NULL) is never stored; a workgroup owns whole rows of it and runs the row body of mca_layernorm_bwd's
 * trunk form on them: dx (fp32) and dx_bf16 = rstd*(g - mean(g) - xhat*mean(g*xhat)) with g = dy*gamma, xhat = (x - mean)*rstd,
 * and dgamma += sum_rows dy*xhat (fp32 atomics, one per column and workgroup).  dx, its bf16 copy and the statistics' use are
 * bit for bit those of mca_gemm_nt (fp32, residual) followed by mca_layernorm_bwd; dgamma differs by the order of the atomic adds.
 * dx may alias residual.  N == 512 and K >= 96 (MCA_E_UNSUPPORTED otherwise), K % 32 == 0, any M >= 1; lda/ldb/ld_bf16 % 8 == 0,
 * ldres/ldx/lddx % 4 == 0, every base 16-byte aligned (MCA_E_ALIGN).                                                          */
int mca_gemm_nt_res_lnbwd(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual, int64_t ldres,
                          const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                          float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16, float* dgamma,
                          int64_t M, int64_t N, int64_t K, mca_stream_t stream);
/* The same call with the tile height chosen for the device: a workgroup owns 160 whole rows instead of 128 where that saves a
 * round of workgroups over the CUs (rounds x rows per tile, ties to 128: M = 81,216 on 256 CUs is 508 tiles in two rounds instead
 * of 635 in three), and the call above unchanged everywhere else.  Same arguments, same rules, same return codes in the same
 * order; dx and dx_bf16 are the same bits from either tile, dgamma differs by the order of the atomic adds.              */
int mca_gemm_nt_res_lnbwd_tall(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual, int64_t ldres,
                               const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                               float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16, float* dgamma,
                               int64_t M, int64_t N, int64_t K, mca_stream_t stream);

/* C[N,K] += A[R,N]^T · B[R,K]   (weight gradient: reduction over the R token rows; fp32 atomics
 * into C, which the caller zeroes once per step).  lda/ldb % 8 == 0; N and K are arbitrary but the
 * rows of A / B must be readable up to the next multiple of 8 columns (lda >= roundup8(N) etc.).  */
int mca_gemm_tn_acc(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb,
                    float* C, int64_t ldc, int64_t R, int64_t N, int64_t K, mca_stream_t stream);

/* Several weight gradients over the same R token rows in one launch: C_i[N_i,K_i] += A_i[R,N_i]^T · B_i[R,K_i] for
 * i < n <= MCA_TN_MAX_GROUP (the four nn.Linear weight gradients of an MCALayer backward, model.py:109-131: to_q/to_kv,
 * to_out, feedforward[0] (two halves) and feedforward[2]).  Same operand rules as mca_gemm_tn_acc per member; members may
 * not alias each other's C.  Groups the kernel does not suit run as n single launches (same results).              */
#define MCA_TN_MAX_GROUP 8
typedef struct mca_tn_desc {
  const uint16_t* A; int64_t lda;
  const uint16_t* B; int64_t ldb;
  float* C; int64_t ldc;
  int64_t N, K;
} mca_tn_desc;
int mca_gemm_tn_acc_group(const mca_tn_desc* d, int n, int64_t R, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm (model.py:24-31; nn.LayerNorm in encoders.py:51,189,192)
 * --------------------------------------------------------------------------------------------- */
/* y = LN(x)*gamma (+beta), eps; one row = `cols` contiguous floats at x + row*ldx.
 * Optional outputs (NULL to skip): y (fp32) at y + (row / period)*y_bstride + (row % period)*ldy
 * (period <= 0: row*ldy); y_bf16 at row*ld_bf16, zero-filled up to cols_pad.
 * rowmask (u8, 1 = padded row): the row's output is `add` only (fp32) / zeros (bf16) and its stats
 * are (0, 0).  add (fp32 [period, cols]) is added after masking (positional table).
 * mean/rstd: per-row statistics saved for the backward.                                          */
int mca_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta,
                      const uint8_t* rowmask, const float* add, int64_t period,
                      float* y, int64_t ldy, int64_t y_bstride,
                      uint16_t* y_bf16, int64_t ld_bf16, int cols_pad,
                      float* mean, float* rstd, int64_t rows, int cols, float eps, mca_stream_t stream);

/* Backward of the above.  dy is read with the same (period, ldy, y_bstride) row mapping as y was
 * written; masked rows have zero gradient.  dx / dx_bf16 optional.  dgamma/dbeta (fp32[cols]) are
 * ACCUMULATED (atomics).  dxsum (fp32[cols], may be NULL): += the column sums of dx, i.e. the bias
 * gradient of the nn.Linear whose output this norm takes (encoders.py:189-192: Linear -> LayerNorm),
 * without a second pass over dx.                                                                 */
int mca_layernorm_bwd(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period,
                      const float* x, int64_t ldx, const float* gamma,
                      const float* mean, const float* rstd, const uint8_t* rowmask,
                      float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16,
                      float* dgamma, float* dbeta, float* dxsum, int64_t rows, int cols, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GEGLU (model.py:35-38): h = [a | gate] (two halves of width ip, ld 2*ip) -> g = gelu(gate)*a
 * --------------------------------------------------------------------------------------------- */
int mca_geglu_fwd(const uint16_t* h, uint16_t* g, int64_t rows, int ip, mca_stream_t stream);
int mca_geglu_bwd(const uint16_t* dg, const uint16_t* h, uint16_t* dh, int64_t rows, int ip,
                  mca_stream_t stream);
/* The stand-alone siblings of the saved-factor GEMM forms above (their fall-back for small or oddly shaped problems).
 * Forward: s holds h = [a | gate] on entry and the factors [gelu(gate) | a * gelu'(gate)] on return, IN PLACE; g as the
 * unsaved kernel writes it.  Backward: dh = [dg * s_lo | dg * s_hi].                                              */
int mca_geglu_fwd_saved(uint16_t* s, uint16_t* g, int64_t rows, int ip, mca_stream_t stream);
int mca_geglu_bwd_saved(const uint16_t* dg, const uint16_t* s, uint16_t* dh, int64_t rows, int ip,
                        mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * small data-movement helpers
 * --------------------------------------------------------------------------------------------- */
/* dst[bf16, rows_pad x cols_pad, ld] = src[fp32, rows x cols, lds] (transposed if transpose != 0:
 * dst[c][r] = src[r][c]); padding is zero-filled.  Used to refresh the bf16 weight copies.       */
int mca_cast_pad_bf16(const float* src, int64_t lds, int64_t rows, int64_t cols,
                      uint16_t* dst, int64_t ldd, int64_t rows_pad, int64_t cols_pad, int transpose,
                      mca_stream_t stream);
/* the same for n tensors in ONE launch; descs_dev is a device array (built once by the caller)   */
/* scale: every element is multiplied by it before rounding (0 is read as 1; used to fold scale * log2(e) into W_q)  */
typedef struct { const void* src; void* dst; int64_t lds, rows, cols, ldd, rows_pad, cols_pad; int32_t transpose; float scale; } mca_cast_desc;
int mca_cast_pad_bf16_multi(const mca_cast_desc* descs_dev, int n, mca_stream_t stream);
/* dst[r*ldd + c] = bf16(src[r*lds + c] * scale) */
int mca_f32_to_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t rows, int64_t cols,
                    float scale, mca_stream_t stream);
/* dst[(i/period)*dst_bstride + (i%period)*ldd + c] = src[(i % period)*lds + c]  for i < rows
 * (broadcast learned tokens over the batch: model.py:460,472)                                    */
int mca_bcast_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t dst_bstride,
                   int64_t period, int64_t rows, int cols, mca_stream_t stream);
/* dst[(i % period)*ldd + c] += sum over i of src[(i/period)*src_bstride + (i%period)*lds + c]
 * (period == 1: plain column sum -> bias gradients)                                              */
int mca_reduce_rows(const float* src, int64_t lds, int64_t src_bstride, int64_t period,
                    float* dst, int64_t ldd, int64_t rows, int cols, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * TabularEncoder (encoders.py:17-96): nn.Embedding(max_norm=1) in-place row renormalisation;
 * ContinuousValueEncoder front end Linear(1,D)+ReLU on min(x, max_value), and its backward.
 * --------------------------------------------------------------------------------------------- */
int mca_embedding_renorm(float* weight, int64_t rows, int cols, float max_norm, mca_stream_t stream);
/* h1[r, :] = relu(min(x[r], max_value) * w1 + b1) as bf16 (rows x cols); padmask[r] = (x[r] == padding_value) */
int mca_tab_value_fwd(const float* x, const float* w1, const float* b1, uint16_t* h1, uint8_t* padmask,
                      int64_t rows, int cols, float max_value, float padding_value, mca_stream_t stream);
/* dw1 += sum_r dh1*[h1>0]*min(x,max_value);  db1 += sum_r dh1*[h1>0]   (dh1 fp32, ld in elements)            */
int mca_tab_value_bwd(const float* dh1, int64_t ld, const uint16_t* h1, const float* x, float* dw1, float* db1,
                      int64_t rows, int cols, float max_value, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Token tables (encoders.py:17-37 as SequenceEncoder :145-166 and SparseTabularEncoder :100-120 use them): rows looked up
 * by index.  idx: `rows` integers of idx_bytes = 8 or 4 each.  An index outside [0, vocab) is never dereferenced.
 * --------------------------------------------------------------------------------------------- */
/* For i < rows:  dst[(i/period)*dst_bstride + (i%period)*ldd + c]  =  (accumulate ? its old value : 0) + (table[idx[i]][c] +
 * add[(i%period)*cols + c])   (add may be NULL; cols % 4 == 0, 16-byte aligned pointers and strides, else MCA_E_ALIGN).
 * Before any row is read, the rows that occur in idx, and only those, are renormalised in place as nn.Embedding(max_norm)
 * does on every forward: a row with L2 norm > max_norm is multiplied by max_norm / (norm + 1e-7), once however many tokens name
 * it; every other row keeps its bits.  Three launches on the stream: mark, renormalise the marked rows, gather.
 * marker: vocab int32 words owned by the caller, all zero on entry, all zero again when the call's launches have run (the
 * kernels clear what they set: no memset).  An index out of range contributes no table row (the output row is the add part
 * alone) and ORs oob_bit into *flag (flag may be NULL), the word of the finite check below.                              */
int mca_embedding_lookup(float* table, int64_t vocab, int cols, float max_norm, const void* idx, int idx_bytes,
                         int64_t rows, int64_t period, const float* add, float* dst, int64_t ldd, int64_t dst_bstride,
                         int accumulate, int32_t* marker, int32_t* flag, int oob_bit, mca_stream_t stream);
/* dtable[idx[i]][c] += dy[(i/period)*y_bstride + (i%period)*ldy + c] for every i < rows whose index is in range and is not
 * padding_idx (negative: counted from the end, as nn.Embedding does; vocab: no padding row).  fp32 atomics, one wavefront
 * instruction per 256 contiguous bytes of one table row; dtable is packed (vocab, cols).                                 */
int mca_embedding_scatter_add(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period, const void* idx, int idx_bytes,
                              int64_t rows, float* dtable, int64_t vocab, int cols, int64_t padding_idx, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PatchEncoder front end (encoders.py:247-251,260-262,273; mode "matrix"): patch gather + LayerNorm(P) + pad mask, one pass.
 * --------------------------------------------------------------------------------------------- */
/* Element (s, r, c) of values is at values + s*v_bstride + r*ldv + c.  Row t = s*n + i*(W/p2) + j, n = (H/p1)*(W/p2), is patch
 * (i, j): its P = p1*p2 elements in (row-in-patch, column-in-patch) order.
 *   xp[t*P ...]        the gathered patch, fp32 (what mca_layernorm_bwd reads as x in the backward); NULL to skip
 *   xn_bf16[t*ld_bf16] bf16(LN(patch)*gamma + beta), zero-filled from P to cols_pad
 *   mean[t], rstd[t]   the row's statistics
 *   padmask[t]         1 if every element == pad_value (exact float compare; NaN is not equal), else 0
 * A row with padmask 1 is written as its exact value: xn = bf16(beta), mean = pad_value, rstd = rsqrt(eps) (LayerNorm of a
 * constant row multiplies any rounding of the mean by rsqrt(eps) = 316).
 * Returns non-zero, launching nothing, for H % p1, W % p2, P > 1024, cols_pad < P, ld_bf16 < cols_pad, ldv < W or a NULL
 * required pointer (every pointer but xp).                                                                               */
int mca_patch_ln_fwd(const float* values, int64_t v_bstride, int64_t ldv, int batch, int H, int W, int p1, int p2,
                     const float* gamma, const float* beta, float pad_value, float eps,
                     float* xp, uint16_t* xn_bf16, int64_t ld_bf16, int cols_pad,
                     float* mean, float* rstd, uint8_t* padmask, mca_stream_t stream);

/* The same pass over a (b, C, T, H, W) batch cut into (pt, p1, p2) patches (ImagePatchEncoder: T = pt = 1; VideoPatchEncoder).
 * Element (s, c, t, r, w) of values is at values + s*v_bstride + c*v_cstride + t*v_fstride + r*ldv + w, so planes and frames may
 * be framed apart.  With gt = T/pt, gh = H/p1, gw = W/p2, row ((s*gt + ti)*gh + hi)*gw + wi is patch (ti, hi, wi) of sample s, and
 * its element ((c*pt + dt)*p1 + r)*p2 + col is values[s, c, ti*pt + dt, hi*p1 + r, wi*p2 + col]; P = C*pt*p1*p2.
 * Outputs and all-pad semantics as mca_patch_ln_fwd: a row has padmask 1 only when every element of every channel and frame of
 * the patch == pad_value.  With C = T = pt = 1 the outputs equal mca_patch_ln_fwd's bit for bit.
 * Returns non-zero, launching nothing, for T % pt, H % p1, W % p2, P > 1024, cols_pad < P, ld_bf16 < cols_pad, ldv < W, a frame
 * stride (T > 1) below (H-1)*ldv + W, a channel stride (C > 1) below (T-1)*v_fstride + (H-1)*ldv + W, a batch stride (batch > 1)
 * below (C-1)*v_cstride + that, or a NULL required pointer (every pointer but xp).                                              */
int mca_patch_nd_ln_fwd(const float* values, int64_t v_bstride, int64_t v_cstride, int64_t v_fstride, int64_t ldv,
                        int batch, int C, int T, int H, int W, int pt, int p1, int p2,
                        const float* gamma, const float* beta, float pad_value, float eps,
                        float* xp, uint16_t* xn_bf16, int64_t ld_bf16, int cols_pad,
                        float* mean, float* rstd, uint8_t* padmask, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Block-masked fused attention (model.py:73-105 as used by MCALayer :119 and attn_pool :472-473)
 * --------------------------------------------------------------------------------------------- */
/* Packing of the per-modality attention masks (model.py:455-466; encoders.py:196-214 for the row masks): ONE launch
 * instead of ~8 small tensor ops per modality.  For every modality i < n_mod, mask i is (b, n_i) of 1-byte (bool) or
 * 8-byte (int64) elements, non-zero = padded:
 *   padding[s, offset_i + j] = mask_i[s, j] != 0;   rowmask_i[s*n_i + j] = the same (dense copy, skipped when NULL);
 *   present[s] bit i = any token of modality i valid in sample s (MCA.forward's modality_sample_mask);
 *   padding[s, n_tokens - n_fusion ...] = 0 (fusion tokens are never padded).                                        */
#define MCA_MAX_MODALITIES 16
typedef struct { const void* mask; uint8_t* rowmask; int32_t elem_bytes, n, offset, pad_; } mca_mask_desc;
typedef struct { mca_mask_desc m[MCA_MAX_MODALITIES]; int32_t n_mod, batch, n_tokens, n_fusion; } mca_pack_masks_args;
int mca_pack_masks(const mca_pack_masks_args* args, uint8_t* padding, int32_t* present, mca_stream_t stream);

/* mca_pack_masks with a per-step MODALITY DROPOUT drawn on the device (the reference's dead BatchDropout, utils/dataset.py).
 * For local sample s, global sample g = sample0 + s, descriptor i and t = *step (read on the device, so a captured step draws
 * new masks at every replay once the counter moves: mca_counter_add):
 *   u(g, i, t) = top 24 bits of fmix64(seed ^ fmix64(t ^ fmix64((g << 32) | i))) * 2^-24   (fmix64: the murmur3 finaliser; the
 *                draw of the MLP probe's dropout, mca_probe_nt_f32 act 2, with row = g and unit = i);
 *   want_i = u < p[i] in float32 (p = 0 never drops, p = 1 always);   raw_i = mask i has a valid token in sample s;
 *   keep_one != 0, some raw_i, and want_i for every i with raw_i: the raw-present modality with the largest u is rescued
 *                (ties: the lowest i); a sample without a raw-present modality stays empty.
 * A modality with want_i that is not rescued is DROPPED: every padding byte of its range and every byte of its rowmask is 1,
 * present bit i is 0 and dropped[s] bit i is 1 (set whether or not raw_i; dropped may be NULL).  Everything else, fusion columns
 * included, is what mca_pack_masks writes; with every p[i] == 0 the outputs are mca_pack_masks' byte for byte.  The input masks
 * are only read.  On top of mca_pack_masks' checks: MCA_E_BADARG for drop or step NULL or any of the MCA_MAX_MODALITIES p[i]
 * NaN or outside [0, 1] (zero the entries past n_mod); MCA_E_ALIGN for a step pointer that is not 8-byte aligned.               */
typedef struct { float p[MCA_MAX_MODALITIES]; uint64_t seed; int64_t sample0; int32_t keep_one, pad_; } mca_modality_drop_args;
int mca_pack_masks_drop(const mca_pack_masks_args* args, const mca_modality_drop_args* drop, const int64_t* step,
                        uint8_t* padding, int32_t* present, int32_t* dropped, mca_stream_t stream);
/* *counter += inc by one thread of a kernel (never a memset / copy node of a captured step).  MCA_E_BADARG: counter NULL;
 * MCA_E_ALIGN: not 8-byte aligned.                                                                                              */
int mca_counter_add(int64_t* counter, int64_t inc, mca_stream_t stream);

/* Finite check of encoder inputs / pooled outputs without a host sync (encoders.py:197-198,206-213: the reference raises
 * after `.sum()` syncs).  *flag |= bit if any of the n[i] floats at p[i], i < count, is Inf or NaN.  The caller zeroes the
 * flag word, reads it once per step and passes it to mca_adamw_step as skip_flag.                                       */
typedef struct { const float* p[MCA_MAX_MODALITIES]; int64_t n[MCA_MAX_MODALITIES]; int32_t count, pad_; } mca_finite_args;
int mca_nonfinite_flag(const mca_finite_args* args, int32_t* flag, int bit, mca_stream_t stream);
/* *host_pinned = *flag, by a kernel (host_pinned: pinned, device-visible host memory): the host polls it after an event,
 * no copy node in a captured step                                                                                        */
int mca_flag_to_host(const int32_t* flag, int32_t* host_pinned, mca_stream_t stream);

/* keyinfo[b, nk_pad] = padded ? 31 : kgroup[j]; entries >= nk are 31.
 * ktile_flags[b, n_ktiles] = 0 no valid key in the 64-key tile, 1 mixed, 2 all valid.
 * padding: u8 (b, nk), 1 = padded key (model.py:465-466).                                       */
int mca_build_keyinfo(const uint8_t* padding, const uint8_t* kgroup, uint8_t* keyinfo,
                      uint8_t* ktile_flags, int batch, int nk, int nk_pad, mca_stream_t stream);

/* khot[b, nk_pad, 16] (bf16) = one-hot of min(keyinfo, 15): the B^T operand of the MASK PRODUCT.  A structure with at most
 * 15 key groups lets the attention kernels add -32768 * (query may not see the key's group | key padded) to the scores on
 * the matrix pipe (one 32x32x16 MFMA per 32-key block: S += Khot . Qblk^T, Qblk[i][g] = bit g of qmask[i] ? 0 : -32768,
 * Qblk[i][15] = -32768) instead of ~4 vector instructions per score; exp2 of such a score is exactly 0, a row whose every
 * key is blocked ends with a running maximum below -16384 and takes the uniform-row path.                               */
int mca_build_keyhot(const uint8_t* keyinfo, uint16_t* khot, int batch, int nk_pad, mca_stream_t stream);

/* vmean[b, h*64+d] = mean over ALL nk keys of V  (value of a fully-masked softmax row); fixed summation order:
 * bitwise reproducible                                                                            */
int mca_attn_vmean(const uint16_t* V, int64_t kv_bstride, int64_t kv_ld, float* vmean,
                   int batch, int nk, int heads, mca_stream_t stream);
/* the same, skipping the samples whose presence bits (mca_pack_masks: bit m = modality m has a valid token) equal full_bits:
 * with every modality present no query row of the fusion / EAO structures is fully masked, vmean[b] is never read and is
 * left as it was                                                                                                        */
int mca_attn_vmean_if_needed(const uint16_t* V, int64_t kv_bstride, int64_t kv_ld, float* vmean, int batch, int nk,
                             int heads, const int32_t* present, int32_t full_bits, mca_stream_t stream);

typedef struct {
  const uint16_t* q; int64_t q_bstride; int64_t q_ld;     /* q[b*q_bstride + i*q_ld + h*64 + d]   */
  const uint16_t* k; const uint16_t* v; int64_t kv_bstride; int64_t kv_ld;
  uint16_t* o; int64_t o_bstride; int64_t o_ld;
  float* lse;                       /* (b, heads, nq) log2-domain; +inf marks a uniform row       */
  const uint32_t* qmask;            /* (nq) allowed key groups per query row                       */
  const uint8_t* keyinfo;           /* (b, nk_pad)                                                 */
  const uint8_t* ktile_flags;       /* (b, n_ktiles)                                               */
  const int32_t* q_ptr; const uint32_t* q_kt; const int32_t* q_order;   /* q_kt: key-tile index | (full << 31) */
  const float* vmean;               /* (b, heads*64)                                               */
  int batch, heads, nq, nk, nk_pad, n_qtiles, n_ktiles;
  float scale;                      /* dim_head ** -0.5                                            */
  int flags;                        /* MCA_ATTN_* bits                                             */
  const uint16_t* khot;             /* optional (mca_build_keyhot): one-hot key groups, the mask as a matrix product */
} mca_attn_fwd_args;
/* q already carries scale * log2(e) (folded into the bf16 copy of to_q.weight by mca_cast_pad_bf16_multi's per-tensor
 * scale): the kernels then take q.k as the log2-domain logit and never multiply a score.  lse, o, dq, dk, dv keep their
 * meaning (dq is the gradient w.r.t. the UNSCALED q, so the data- and weight-gradient GEMMs are unchanged).              */
#define MCA_ATTN_Q_PRESCALED 1
/* mca_attn_fwd only: LAZY softmax reference.  The score accumulators start from -m (the MFMA C operand) and m moves only when
 * a score exceeds it by more than 12 (log2 units) or a row meets its first real key, instead of following every new row maximum:
 * a third fewer vector instructions per tile (CMU b = 32: 304 against 336 us per layer).  Same contract (o, lse, uniform rows) and
 * the same distance from the exact softmax; P is rounded to bf16 against another reference, so results differ from the textbook
 * form by rounding (2-3e-3 rel-L2 of o).  The engine sets it by default since round 5: over 8 data seeds x {MCA, MMA} the two
 * forms are statistically indistinguishable in their distance to the fp64 oracle (profiles/r05_lazy_softmax_seed_study.txt).   */
#define MCA_ATTN_LAZY_REFERENCE 2
/* dim_head is fixed at 64; query tile 128 rows, key tile 64.                                     */
int mca_attn_fwd(const mca_attn_fwd_args* args, mca_stream_t stream);

/* Where the heads of q and of k | v lie, for operands that are not (rows, heads*64) matrices: head h starts q_hstride (kv_hstride)
 * elements behind head 0, 0 = 64.  The column-blocked output of mca_gemm_nt_cb, [block][T][64] with cbs elements between the blocks,
 * is q_bstride = kv_bstride = n*64, q_ld = kv_ld = 64, q_hstride = kv_hstride = cbs, with q, k and v pointing at blocks 0, heads and
 * 2*heads: a (sample, head) is then n contiguous 128-byte rows.  Strides % 8 == 0.  The argument structs above and below keep their
 * fields: the layout travels beside them.                                                                                        */
typedef struct { int64_t q_hstride, kv_hstride; } mca_attn_layout;
/* mca_attn_fwd / mca_attn_vmean_if_needed on such operands (layout NULL or all zero: exactly those calls; same kernels, same bits) */
int mca_attn_fwd_hm(const mca_attn_fwd_args* args, const mca_attn_layout* layout, mca_stream_t stream);
int mca_attn_vmean_if_needed_hm(const uint16_t* V, int64_t kv_bstride, int64_t kv_ld, int64_t kv_hstride, float* vmean, int batch, int nk,
                                int heads, const int32_t* present, int32_t full_bits, mca_stream_t stream);

/* Attention READOUT (model.py:87-103: Attention.forward with return_attn=True returns softmax(q·k^T) after its two
 * masked_fill; here the (b, h, nq, nk) matrix is never written).  One launch per attention, after mca_attn_fwd on the same
 * operands (same conventions: head = 64 contiguous bf16, q_bstride 0 for the pooling query, MCA_ATTN_Q_PRESCALED required,
 * the forward's 128 x 64 tile lists).  lse is the array the forward wrote and is not recomputed: p[i][j] = exp2(q_i·k_j - lse[i]) for a key j the row may see
 * ((qmask[i] >> keyinfo[b][j]) & 1), exactly 0 for every other key.
 *   mass[b, h, i, g] (fp32, every element written) = sum of p[i][j] over the keys j with keyinfo[b][j] == g: the share of row
 *     i's softmax on key group g < n_groups (1 <= n_groups <= 31).  A uniform row (lse = +inf) gets uniform_mass[g], which the
 *     caller sets to (keys with static group g) / nk: the reference's softmax of a fully masked row is uniform over ALL nk
 *     keys, padded and blocked ones included.
 *   probs[b, h, r, j] (fp32, optional: NULL to skip) = p[row0 + r][j] for r < n_rows and every j < nk, every element written
 *     (keys of tiles the schedule skips included: 0); 1 / nk on a uniform row.  The window need not be aligned.
 * fp32 sums in a fixed order, no atomics: bitwise repeatable.  row0 / n_rows are read only when probs is given.             */
typedef struct {
  const uint16_t* q; int64_t q_bstride; int64_t q_ld;     /* q[b*q_bstride + i*q_ld + h*64 + d]   */
  const uint16_t* k; int64_t kv_bstride; int64_t kv_ld;
  const float* lse;                 /* (b, heads, nq) log2-domain, as written by the forward         */
  const uint32_t* qmask;            /* (nq)                                                          */
  const uint8_t* keyinfo;           /* (b, nk_pad)                                                   */
  const uint8_t* ktile_flags;       /* (b, n_ktiles)                                                 */
  const int32_t* q_ptr; const uint32_t* q_kt; const int32_t* q_order;
  int batch, heads, nq, nk, nk_pad, n_qtiles, n_ktiles;
  float scale;                      /* dim_head ** -0.5 (already folded into q)                      */
  int flags;                        /* MCA_ATTN_Q_PRESCALED                                          */
  int n_groups;
  const float* uniform_mass;        /* (n_groups)                                                    */
  float* mass;                      /* (b, heads, nq, n_groups)                                      */
  float* probs;                     /* (b, heads, n_rows, nk) or NULL                                */
  int row0, n_rows;
} mca_attn_readout_args;
int mca_attn_readout(const mca_attn_readout_args* args, mca_stream_t stream);

/* ---- EAO baseline (model.py:481-596): every modality alone and every combination of modalities is one SEGMENT of a
 * super-sequence; the attention kernels' key groups make the attention block-diagonal over segments.
 * dst[b, r, :] (+)= src[b, r, :], r < rows: replicates a modality's encoded token block into its segments (accumulate = 0)
 * and sums the gradients of the replicas back (accumulate = 1); strides in floats.                                        */
int mca_rows_copy_add(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int64_t rows, int cols,
                      int batch, int accumulate, mca_stream_t stream);
/* MeanTokenProjectionPool without token types / projection (model.py:255-276): out[b, s, :] = mean of the un-padded rows
 * seg_start[s] .. seg_start[s+1]-1 of x[b] (zeros if none); counts[b, s] = their number.  Fixed summation order.          */
int mca_segment_mean_fwd(const float* x, const uint8_t* padding, const int32_t* seg_start, int n_seg, float* out,
                         int32_t* counts, int batch, int n_tokens, int cols, mca_stream_t stream);
/* dx[b, r, :] = padded(b, r) ? 0 : d_out[b, seg_of_row[r], :] / counts[b, seg_of_row[r]]                                  */
int mca_segment_mean_bwd(const float* d_out, const uint8_t* padding, const uint8_t* seg_of_row, const int32_t* counts,
                         int n_seg, float* dx, int batch, int n_tokens, int cols, mca_stream_t stream);

/* MX-fp8 operands of the fusion attention forward (BASELINE configs[4], "fp8 MFMA attention"): OCP e4m3 elements with one
 * E8M0 power-of-two scale byte per 32 elements along the contraction (d for Q and K; keys 0..31 | 32..63 of a 64-key tile
 * for V^T), the operand format of v_mfma_scale_f32_32x32x64_f8f6f4.  npad = n_ktiles * 64 token rows per (sample, head), rows >= n are zero.
 *   q8, k8 : [batch][heads][npad][64]            qs, ks : [batch][heads][npad][2]
 *   v8t    : [batch][heads][n_ktiles][64 d][64]  V transposed per 64-key tile; position p of a row holds key
 *            32 (p >> 5) + 8 ((p >> 2) & 3) + 4 ((p >> 4) & 1) + (p & 3) of the tile (the order in which the S^T
 *            accumulators of the forward kernel hold a query's keys);      vs : [batch][heads][n_ktiles][64 d][2]          */
typedef struct { uint8_t* q8; uint8_t* qs; uint8_t* k8; uint8_t* ks; uint8_t* v8t; uint8_t* vs; int n_ktiles; } mca_attn_fp8_operands;
/* q | k | v (bf16, strides as in mca_attn_fwd_args; q pre-scaled by scale * log2 e) -> the operands above              */
int mca_attn_quant_mxfp8(const uint16_t* q, int64_t q_bstride, int64_t q_ld, const uint16_t* k, const uint16_t* v,
                         int64_t kv_bstride, int64_t kv_ld, const mca_attn_fp8_operands* f, int batch, int heads, int n,
                         mca_stream_t stream);
/* mca_attn_fwd with Q K^T and P V on the block-scaled fp8 matrix instruction (self-attention, MCA_ATTN_Q_PRESCALED only;
 * the q / k / v pointers of args are not read).  o (bf16) and lse as mca_attn_fwd; the backward stays in bf16.            */
int mca_attn_fwd_fp8(const mca_attn_fwd_args* args, const mca_attn_fp8_operands* f, mca_stream_t stream);

/* Backward of the fusion attention with the two score recomputes (S = Q K^T, dP = dO V^T: 4 of the 7 matrix products of
 * the two-pass backward) on the block-scaled fp8 matrix instruction (BASELINE configs[4]; autograd of model.py:87-99).
 * Operands: e4m3 copies of q, k, v, dO, all [batch][heads][npad][64] with [batch][heads][npad][2] E8M0 scale bytes (blocks of
 * 32 ALONG d, the contraction of both products), npad = n_ktiles * 64, rows >= n zero.  q8 / k8 are the arrays of
 * mca_attn_quant_mxfp8, so S is bit for bit the S of mca_attn_fwd_fp8 and P = 2^(S - lse) is consistent with its lse.   */
typedef struct { uint8_t* q8; uint8_t* qs; uint8_t* k8; uint8_t* ks; uint8_t* v8; uint8_t* vs; uint8_t* do8; uint8_t* dos; int n_ktiles; } mca_attn_fp8_bwd_operands;
/* which: bit 0 q, bit 1 k, bit 2 v, bit 3 dO are quantised by this call (15 = all; 12 = v and dO when f->q8 / f->k8 point at
 * the arrays the forward's mca_attn_quant_mxfp8 wrote for the same layer)                                              */
int mca_attn_quant_bwd_mxfp8(const uint16_t* q, int64_t q_bstride, int64_t q_ld, const uint16_t* k, const uint16_t* v,
                             int64_t kv_bstride, int64_t kv_ld, const uint16_t* d_o, int64_t o_bstride, int64_t o_ld,
                             const mca_attn_fp8_bwd_operands* f, int which, int batch, int heads, int n, mca_stream_t stream);
/* mca_attn_bwd_dq / mca_attn_bwd_dkv (arguments as documented below) with those operands; self-attention,
 * MCA_ATTN_Q_PRESCALED and the mask product (khot / qblk) required, kblock_keys = 128 for the dkv pass; the q / v pointers
 * of args are read only by the dkv pass (bf16 Q tile of the dK product); dQ, dK, dV products stay bf16 / fp32.            */
/* delta[b,h,i] = sum_d dO*O ; dvmean[b,h*64+d] = (1/nk) * sum over uniform rows i of dO          */
int mca_attn_bwd_prep(const uint16_t* o, const uint16_t* d_o, int64_t o_bstride, int64_t o_ld,
                      const float* lse, float* delta, float* dvmean,
                      int batch, int heads, int nq, int nk, mca_stream_t stream);

/* The backward runs in two passes WITHOUT atomics (float atomics run at ~1.3 TB/s chip-wide on MI355X: the 0.9 GB of fp32 dQ
 * adds per layer put a 690 us floor under a one-pass kernel, which left the library in round 3): every output element has
 * one owner, results are bitwise reproducible.  MCA_ATTN_Q_PRESCALED is required (MCA_E_UNSUPPORTED otherwise).
 *   mca_attn_bwd_dq : one workgroup per 128-row query tile, key tiles of 64 (the forward's schedule); dq written once,
 *                     bf16 (dq_f32 == 0) or fp32, no pre-zeroing.  Needs q_ptr / q_kt / q_order, n_qtiles128, n_ktiles64.
 *   mca_attn_bwd_dkv: one workgroup per 256- or 128-key block (kblock_keys), query steps of 64; dk, dv bf16.  Needs k_qt
 *                     (per key block the list of 64-row query tiles | full << 31), k_wg (per launch slot the four int32
 *                     {key block, first list entry, number of entries, query tile of the first entry}: one 16-byte load at
 *                     workgroup start), n_qtiles64, n_kblocks256, dvmean.
 * Both need mca_attn_bwd_prep's delta (and dvmean).  The two launches are independent of each other.                     */
typedef struct {
  const uint16_t* q; int64_t q_bstride; int64_t q_ld;
  const uint16_t* k; const uint16_t* v; int64_t kv_bstride; int64_t kv_ld;
  const uint16_t* d_o; int64_t o_bstride; int64_t o_ld;
  const float* lse; const float* delta; const float* dvmean;
  void* dq; int64_t dq_bstride; int64_t dq_ld; int dq_f32;
  uint16_t* dk; uint16_t* dv; int64_t dkv_bstride; int64_t dkv_ld;
  const uint32_t* qmask; const uint8_t* keyinfo; const uint8_t* ktile_flags;
  const int32_t* q_ptr; const uint32_t* q_kt; const int32_t* q_order; int n_qtiles128, n_ktiles64;
  const int32_t* k_wg; const uint32_t* k_qt; int n_qtiles64, n_kblocks256;
  int batch, heads, nq, nk, nk_pad;
  float scale;
  int flags;
  /* optional, both or neither: the mask as a matrix product (see mca_build_keyhot).  qblk[nq, 16] bf16 is the static query
   * side: qblk[i][g] = bit g of qmask[i] ? 0 : -32768 for g < 15, qblk[i][15] = -32768                                  */
  const uint16_t* khot; const uint16_t* qblk;
  /* keys per workgroup of the dkv pass: 0 / 256 (8 wavefronts) or 128 (4 wavefronts, two workgroups per CU: a few % faster
   * for short sequences, slower for long ones); k_wg / k_qt / n_kblocks256 describe key blocks of THIS size              */
  int kblock_keys;
} mca_attn_bwd2_args;
int mca_attn_bwd_dq(const mca_attn_bwd2_args* args, mca_stream_t stream);
int mca_attn_bwd_dkv(const mca_attn_bwd2_args* args, mca_stream_t stream);
int mca_attn_bwd_dq_fp8(const mca_attn_bwd2_args* args, const mca_attn_fp8_bwd_operands* f, mca_stream_t stream);
int mca_attn_bwd_dkv_fp8(const mca_attn_bwd2_args* args, const mca_attn_fp8_bwd_operands* f, mca_stream_t stream);

/* ONE-PASS backward of the fusion self-attention (autograd of model.py:87-99 as called by MCALayer.forward :119), the five
 * matrix products the gradient needs instead of the two passes' seven, still without atomics: ONE workgroup owns a whole
 * (sample, head), walks its key blocks (<= 256 keys: dK / dV in registers) in order and inside a block the query tiles
 * (<= 64 rows) the structure allows; dQ of a tile is summed over its key blocks by a private fp32 read-modify-write in dq_acc
 * (first visit starts from zero, last visit writes bf16 dq): fixed order, bitwise reproducible.  Needs the mask product
 * operands (khot / qblk: at most 15 key groups), MCA_ATTN_Q_PRESCALED, nq == nk == n.  Tables (structure.build_onepass_schedule):
 *   qt_desc[n_qtiles]  = {first row, rows (1..64)}                       query tiles, a partition of 0..n-1
 *   kb_desc[n_kblocks] = {first key, keys (1..256), first entry, entries} key blocks, a partition of 0..n-1, 16-byte aligned
 *   kb_qt[]            = per key block its query tiles | (every pair structurally allowed << 31); the order inside a block's
 *                        list is free (a tile's first / last visit is decided per key block): the generator emits serpentine
 *   visit[n_kblocks][n_qtiles] = 1 where the block lists the tile;  max_list = longest list (<= 250), n_entries = all lists
 * rowc (b, heads, n_qtiles + 1, 2, 64) fp32: -lse | -delta of the tile's rows (mca_attn_bwd_prep_onepass; positions past a
 * tile's rows, and the whole last tile - the NULL tile every key block's sweep ends on - hold -inf | 0, written once by the caller).  dq_acc: workspace of
 * batch * heads * max(1, split) * (n_qtiles + 1) * 4096 floats (the last slot of a (sample, head) belongs to the null tile:
 * written, never read back into a result), contents irrelevant on entry.  dq, dk, dv bf16, every element written.  n_qtiles < 256, n_kblocks <= 64, max_list <= 250, else MCA_E_UNSUPPORTED
 * (the caller keeps the two-pass form).                                                                                  */
typedef struct {
  const uint16_t* q; int64_t q_bstride; int64_t q_ld;           /* q[b*q_bstride + head*q_hstride + i*q_ld + d]                       */
  const uint16_t* k; const uint16_t* v; int64_t kv_bstride; int64_t kv_ld;
  const uint16_t* d_o; int64_t o_bstride; int64_t o_ld;        /* d_o[b*o_bstride + head*o_hstride + i*o_ld + d]                     */
  int64_t q_hstride, o_hstride;                                /* elements between heads: 64 in a (b, n, heads*64) matrix (0 = 64);   */
                                                               /* n*64 in the head-major packed copies of mca_attn_bwd_prep_onepass  */
  const float* rowc; const float* dvmean;
  uint16_t* dq; int64_t dq_bstride; int64_t dq_ld;
  uint16_t* dk; uint16_t* dv; int64_t dkv_bstride; int64_t dkv_ld;
  float* dq_acc;
  const uint8_t* keyinfo; const uint8_t* ktile_flags; const uint16_t* khot; const uint16_t* qblk;
  const int32_t* qt_desc; const int32_t* kb_desc; const uint32_t* kb_qt; const uint8_t* visit;
  int n_qtiles, n_kblocks, max_list;
  int n_entries;                                               /* length of kb_qt: n_entries + 4 * n_kblocks <= 768                 */
  int batch, heads, n, nk_pad, n_ktiles64;
  float scale;
  int flags;
  int split;                                                   /* 0 / 1: one workgroup per (sample, head).  S = 2..8 (small batches): S workgroups per  */
                                                               /* (sample, head), key block kb swept by workgroup kb mod S, dq_acc holds S slices  */
                                                               /* per (sample, head) (slice-major; total size: see dq_acc above), summed in            */
                                                               /* slice order by a second launch of the same call: still no atomics, bitwise repeatable  */
} mca_attn_bwd1_args;
int mca_attn_bwd_onepass(const mca_attn_bwd1_args* args, mca_stream_t stream);
/* mca_attn_bwd_prep for the one-pass form: rowc in tile order (row_slot[q] = tile * 64 + position) instead of delta; dvmean as
 * mca_attn_bwd_prep.  Optional (q_hm and do_hm both or neither): head-major packed copies q_hm / do_hm [batch][heads][n][64] of
 * q (read with q_bstride / q_ld) and d_o - the one-pass kernel then reads a 64-row tile of a head as 8 KiB of contiguous memory
 * (pass them as its q / d_o with q_bstride = heads*n*64, q_hstride = n*64, q_ld = 64: the form the pipelined kernel takes; other
 * strides run the plain form of the same algorithm).  Both buffers need 64 rows (8 KiB) of slack behind the last row that hold
 * FINITE values of ordinary magnitude (the engine zero-fills them once): the pipelined kernel reads whole 64-row tiles without
 * clamping to a tile's rows, and the rows past them (the next tile's, the next head's, or the slack) enter the products behind row
 * constants of -inf, i.e. with P = 0 and dS = 0 * (finite) = 0 - a NaN or an Inf there would poison dK / dV (0 * NaN).  Their
 * values do not change a result bit (tests/test_attention_edges_gpu.py runs zeros against randn).                          */
int mca_attn_bwd_prep_onepass(const uint16_t* o, const uint16_t* d_o, int64_t o_bstride, int64_t o_ld, const float* lse,
                              const int32_t* row_slot, float* rowc, float* dvmean, int batch, int heads, int n, int n_qtiles,
                              const uint16_t* q, int64_t q_bstride, int64_t q_ld, uint16_t* q_hm, uint16_t* do_hm,
                              mca_stream_t stream);
/* The one-pass backward on head-major operands that need no packed copies: q and d_o as written by mca_gemm_nt_cb (the struct's own
 * q_hstride / o_hstride say so already), k | v through layout->kv_hstride (q_hstride of the layout is not read).  layout NULL or
 * zero: mca_attn_bwd_onepass.  The slack rule of the packed copies holds for the buffers q and d_o lie in: 64 finite rows behind the
 * last slab that is read as q or d_o (a tile's over-read inside the buffer lands in the next sample or slab).                   */
int mca_attn_bwd_onepass_hm(const mca_attn_bwd1_args* args, const mca_attn_layout* layout, mca_stream_t stream);
/* Its prep launch: rowc and dvmean as mca_attn_bwd_prep_onepass writes them (delta summed by the same lanes in the same order: the
 * same bits), o row-major, d_o[b*do_bstride + head*do_hstride + i*do_ld + d] (do_hstride 0 = 64), and no copy of anything.      */
int mca_attn_bwd_prep_onepass_hm(const uint16_t* o, int64_t o_bstride, int64_t o_ld, const uint16_t* d_o, int64_t do_bstride,
                                 int64_t do_hstride, int64_t do_ld, const float* lse, const int32_t* row_slot, float* rowc,
                                 float* dvmean, int batch, int heads, int n, int n_qtiles, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * All-pairs contrastive loss with temperature
 * (model.py:175-233 + torchmultimodal ContrastiveLossWithTemperature, formula per
 *  utils/contrastive_loss_with_temperature.py:40-108,178-195)
 * --------------------------------------------------------------------------------------------- */
typedef struct { int32_t slot_a, slot_b; uint32_t and_bits, or_bits; } mca_loss_term;
/* pooled_all: (B, R, D) fp32, all ranks concatenated rank-major; present_all: (B) u32 bit m = modality
 * m present in the sample.  Local rows are [row0, row0+b).
 * Outputs: term_loss[T] (NaN where a term has no valid row on this rank), loss[1] (NaN-aware mean),
 * d_pooled (b,R,D) = d(sum over ranks of loss_r)/d(local pooled) given every rank's n_valid/n_terms
 * are computed here from present_all; d_logit_scale[1] = d loss_local / d logit_scale.
 * workspace: >= mca_contrastive_workspace_bytes(...)                                              */
int64_t mca_contrastive_workspace_bytes(int B, int T);
int mca_contrastive_fwd_bwd(const float* pooled_all, const uint32_t* present_all,
                            const mca_loss_term* terms, int T, const float* logit_scale,
                            int B, int b_local, int row0, int R, int D,
                            float* term_loss, float* loss, float* d_pooled, float* d_logit_scale,
                            void* workspace, mca_stream_t stream);
/* The same loss, outputs and meaning (model.py:175-233; utils/contrastive_loss_with_temperature.py:40-108,178-195) in a
 * STREAMING form for gathered batches of thousands of rows (mca-paper_amd/cached.py): the Gram product and both gradient
 * products run tile by tile on the fp32-input MFMA (exact fp32 products, fp32 accumulation) and the logits are recomputed in
 * the gradient pass, so no (B, B) matrix is ever stored.  The workspace holds per-row statistics only (9 T B floats); no word
 * of it is read before the same call has written it.  No atomics: every sum has a fixed order given by the shapes, two calls
 * give the same bytes.  d_pooled (b_local, R, D) is written at every element, zeros in the slots no term names.
 * Accepted: every B >= 1 with b_local | B, every T, R <= 65535 and 1 <= D <= 512.  MCA_E_UNSUPPORTED, nothing launched: D > 512
 * (the caller uses mca_contrastive_fwd_bwd).  MCA_E_BADARG, nothing launched: the dense form's refusals, or workspace_bytes <
 * mca_contrastive_stream_workspace_bytes(B, T, R, D).                                                                       */
int64_t mca_contrastive_stream_workspace_bytes(int B, int T, int R, int D);
int mca_contrastive_stream_fwd_bwd(const float* pooled_all, const uint32_t* present_all,
                                   const mca_loss_term* terms, int T, const float* logit_scale,
                                   int B, int b_local, int row0, int R, int D,
                                   float* term_loss, float* loss, float* d_pooled, float* d_logit_scale,
                                   void* workspace, int64_t workspace_bytes, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * clip_grad_norm_ + AdamW over one flat buffer (train_accel_gpu.py:116-118; torch AdamW defaults)
 * --------------------------------------------------------------------------------------------- */
/* sqnorm[0] = sum g^2, sqnorm[MCA_SQNORM_WORDS - 1] = its square root (the total gradient norm, train_accel_gpu.py:116).
 * sqnorm points at MCA_SQNORM_WORDS floats: words 1 .. MCA_SQNORM_WORDS - 2 are scratch for the per-block partial sums, added
 * in a fixed order (the same bits on every launch and on every data-parallel replica); the library itself holds no state,
 * calls on different buffers may overlap.                                                          */
#define MCA_SQNORM_WORDS 1026
int mca_grad_sqnorm(const float* g, int64_t n, float* sqnorm, mca_stream_t stream);
/* grads scaled by min(1, max_norm/(sqrt(sqnorm)+1e-6)) when max_norm > 0, then decoupled AdamW.
 * skip_flag (may be NULL): device word written by mca_nonfinite_flag; non-zero = the step is skipped,
 * parameters and moments untouched (the reference raises before optimizer.step(), encoders.py:197-213). */
int mca_adamw_step(float* p, const float* g, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_corr1, float bias_corr2, float max_norm, const float* sqnorm,
                   const int32_t* skip_flag, const float* hyper, mca_stream_t stream);
/* hyper (may be NULL): three device floats {lr, bias_corr1, bias_corr2} that replace the scalar arguments, so that a step
 * captured in a hipGraph takes this step's learning rate and Adam bias corrections at REPLAY time; written by
 * mca_adamw_hyper, a one-thread kernel launched outside the graph (scalar arguments: no host buffer to race with).      */
int mca_adamw_hyper(float* hyper, float lr, float bias_corr1, float bias_corr2, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Downstream evaluation (lp_accel_gpu.py of the reference: utils/metrics.py:20-27,72-98 and its probe loop), fp32, no float
 * atomics: the same bits on every launch.  The tile-core products (cosine rank, pair sum, the probe's NT layer and TN
 * gradients) are one k-ordered fmaf chain per output; the row kernels (normalisation, probe head) add lane-strided partials
 * in a fixed xor tree (csrc/evaluate.hip).
 * --------------------------------------------------------------------------------------------- */
/* y[i] = x[i] / max(||x[i]||_2, 1e-8) for n rows of d (torch's cosine_similarity order: normalise, then dot).  y may be x. */
int mca_rows_normalize_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t n, int64_t d, mca_stream_t stream);
/* rank[r] = #{ j < nt : q[i].t[j] > q[i].t[i] } with i = qidx[r] (or r when qidx is NULL), for r < nq: the rank of the true
 * target among all targets, strict > (exact ties do not count).  s_true: nq floats of workspace, = q[i].t[i] by the same
 * fmaf chain as the tile.  Every qidx[r] must be a row of q and < nt (the caller checks).  Integer atomics only.           */
int mca_cosine_rank_f32(const float* q, int64_t ldq, const int32_t* qidx, int64_t nq, const float* t, int64_t ldt, int64_t nt,
                        int64_t d, float* s_true, int32_t* rank, mca_stream_t stream);
/* Top-k retrieval over the same scores.  s[r][j] = q[i].t[j], i = qidx[r] (or r when qidx is NULL): the tile's fmaf chain,
 * bitwise the value the rank kernel compares and the probe layer (act 0, no bias) stores.  The candidates of query r are the
 * targets j < nt with tvalid[j] != 0 (tvalid may be NULL: all), j != exclude[r] (exclude may be NULL; -1 excludes nothing)
 * and a score that is not NaN.  j comes before j' when s[r][j] > s[r][j'], or when the two compare equal (+0 and -0 do) and
 * j < j': a total order, so the result depends on no tile, arrival or chunk order.  For c < k, score[r * lds + c] and
 * index[r * ldi + c] are the c-th candidate in that order; columns past the number of candidates hold -inf and -1; nothing
 * else is stored.  nq == 0: nothing launched; nt == 0: every row is padding.  The (nq, nt) matrix is never stored; ws holds
 * the k best of every 1024-target chunk.  Integer LDS atomics only: two launches give the same bytes.
 * MCA_E_BADARG (nothing launched): k < 1, d < 1, negative sizes, ldq / ldt < d, lds / ldi < k, a NULL q, t (nt > 0), score or
 * index, a ws that is NULL or below the workspace query.  MCA_E_UNSUPPORTED: k > MCA_TOPK_MAX, nt > 65535 * 1024.          */
#define MCA_TOPK_MAX 64
/* bytes of workspace for a problem; host only, nothing launched; < 0 for an invalid problem (a size < 0, k outside 1..64) */
int64_t mca_cosine_topk_workspace(int64_t nq, int64_t nt, int k);
int mca_cosine_topk_f32(const float* q, int64_t ldq, const int32_t* qidx, int64_t nq, const float* t, int64_t ldt, int64_t nt,
                        int64_t d, const uint8_t* tvalid, const int32_t* exclude, int k, void* ws, int64_t ws_bytes,
                        float* score, int64_t lds, int32_t* index, int64_t ldi, mca_stream_t stream);
/* doubles of workspace mca_pair_gauss_sum_f32 needs for n rows */
int64_t mca_pair_gauss_workspace(int64_t n);
/* sum_out[0] = sum_{i<j} exp(-t * ||x_i - x_j||^2) (exp in fp32, the squared distance a direct-difference fmaf chain, fp64
 * per-tile partials added in a fixed order); value_out[0] = log(sum / (n (n - 1) / 2)) as float: lunif of the reference
 * (NaN for n < 2, -inf when every pair underflows).  Either output may be NULL.                                       */
int mca_pair_gauss_sum_f32(const float* x, int64_t ldx, int64_t n, int64_t d, float t, double* partials, int64_t n_partials,
                           double* sum_out, float* value_out, mca_stream_t stream);
/* Probe layer: y[m, n] = act(x[xidx[m]] . w[n] + bias[n]) (xidx may be NULL, bias may be NULL); act 0 none, 1 ReLU, 2 dropout
 * (keep when a hash of (seed, step, m, n) >= p, kept values scaled by 1/(1-p)) then ReLU.                                   */
int mca_probe_nt_f32(const float* x, int64_t ldx, const int32_t* xidx, const float* w, int64_t ldw, const float* bias, float* y,
                     int64_t ldy, int64_t M, int64_t N, int64_t K, int act, float p, uint64_t seed, int64_t step, mca_stream_t stream);
/* number of loss partials mca_probe_head_f32 writes for B rows */
int64_t mca_probe_head_blocks(int64_t B);
/* Probe head over B rows: z[r] = a[aidx[r]] . w[l] + bias[l] (w [L, K]), pred[r, l] = z; loss_type 0 L1, 1 MSE, 2 BCE with
 * logits against labels[yidx[r], l] (labels [*, L]); dz (may be NULL) = d(mean loss)/dz; da (may be NULL) [B, K] =
 * (dz . w)[r, k] * dact_scale where a[r, k] > 0, else 0 (ReLU + dropout backward of the MLP's stored hidden output);
 * loss_part[mca_probe_head_blocks(B)] = per-block sums of the element losses.  K <= 1024, L <= 64.                     */
int mca_probe_head_f32(const float* a, int64_t lda, const int32_t* aidx, int64_t K, const float* w, const float* bias, int64_t L,
                       const float* labels, const int32_t* yidx, int64_t B, int loss_type, float* pred, float* dz, float* da,
                       float dact_scale, float* loss_part, mca_stream_t stream);
/* floats of workspace mca_probe_tn_f32 needs */
int64_t mca_probe_tn_workspace(int64_t R, int64_t N, int64_t K);
/* gw[m, k] = sum_r a[r, m] * b[bidx[r], k] and gb[m] = sum_r a[r, m] over R rows (a weight and bias gradient; bidx may be
 * NULL): per-chunk partials of 128 rows, added in chunk order by a second launch.                                       */
int mca_probe_tn_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const int32_t* bidx, int64_t R, int64_t N, int64_t K,
                     float* partials, int64_t n_partials, float* gw, float* gb, mca_stream_t stream);
/* acc[0] += (sum of n loss partials, fixed order) / count */
int mca_probe_loss_accum(const float* loss_part, int64_t n, int64_t count, float* acc, mca_stream_t stream);

/* ---- Supervised task head over the pooled tokens (fine-tuning; finetune.py).  A linear head nn.Linear(D, L) reads ONE slot of the
 * (b, R, D) pooled tokens, x[s, :] = pooled[s, slot, :] (signed values: no activation gate), and an elementwise loss compares its
 * logits with a column window of a label matrix.  Row s is VALID iff any_bits == 0 or (present[s] & any_bits) != 0; n_valid counts
 * the valid rows and n = n_valid * L.
 *   pred[s, l]   = z[s, l] = x[s] . w[l] + bias[l], written for every row, valid or not
 *   loss[0]      = mean element loss over the n elements of the valid rows, NOT scaled by task_weight (0 when n_valid == 0);
 *   loss[1]      = n_valid.  Element loss by loss_type: 0 |z - y|, 1 (z - y)^2, 2 max(z, 0) - z y + log1p(exp(-|z|))
 *   dz[s, l]     = (d element loss / dz) * fl(task_weight / n) on valid rows (sign(0) = 0 for L1), 0 on invalid rows and when
 *                  n_valid == 0; the labels of an invalid row are never read
 *   gw[l, k]     = sum_s dz[s, l] x[s, k], gb[l] = sum_s dz[s, l]   (accumulate 0: overwritten, 1: added to)
 *   d_pooled[s, r, :] = base_weight * d_pooled_in[s, r, :] + (r == slot ? sum_l dz[s, l] w[l, :] : 0), one fused multiply-add per
 *                  element, every element written; d_pooled_in NULL: base_weight is ignored and the base is 0.
 * Two launches: one workgroup per 64 rows (one wave per row) stores its share of gw, gb and the loss into its slot of the
 * workspace, rows in order; the second launch adds the slots in block order.  No atomics: two calls on unchanged inputs give the
 * same bits.  Rows of pooled, w, d_pooled and gw move as 16-byte accesses.
 * MCA_E_BADARG: args or a required pointer NULL, b < 1, R < 1, D < 1, L < 1, slot outside [0, R), ld_labels < L, loss_type outside
 * 0 .. 2, accumulate not 0 / 1, present NULL with any_bits != 0, a NaN weight, workspace_bytes below the query.
 * MCA_E_UNSUPPORTED: D > 1024 or L > 64.  MCA_E_ALIGN: D % 4 != 0; pooled, w, d_pooled, d_pooled_in, gw or workspace not 16-byte
 * aligned; another pointer not 4-byte aligned.  Every check returns before anything is launched.                              */
typedef struct {
  const float* pooled;              /* (b, R, D) dense fp32                                          */
  const uint32_t* present;          /* (b) presence words of the step, or NULL (any_bits == 0)       */
  uint32_t any_bits;
  int b, R, D, slot;
  const float* w; const float* bias;          /* (L, D) row-major, (L)                               */
  int L;
  const float* labels;              /* y[s, l] = labels[s * ld_labels + l]                           */
  int64_t ld_labels;
  int loss_type;                    /* 0 L1, 1 MSE, 2 BCE with logits (mca_probe_head_f32's codes)   */
  float task_weight, base_weight;
  const float* d_pooled_in;         /* (b, R, D) or NULL                                             */
  float* pred;                      /* (b, L)                                                        */
  float* loss;                      /* [2]                                                           */
  float* d_pooled;                  /* (b, R, D); may alias d_pooled_in                              */
  float* gw; float* gb;             /* (L, D), (L)                                                   */
  int accumulate;
  float* workspace; int64_t workspace_bytes;
} mca_task_head_args;
/* bytes of workspace mca_task_head_fwd_bwd needs (host only): ceil(b / 64) slots of L*D + roundup4(L) + 4 floats; -1 for sizes the
 * entry point refuses (b < 1, L outside 1 .. 64, D outside 4 .. 1024 or D % 4 != 0)                                              */
int64_t mca_task_head_workspace_bytes(int b, int L, int D);
int mca_task_head_fwd_bwd(const mca_task_head_args* args, mca_stream_t stream);

/* ---- Softmax cross-entropy over class-index labels (csrc/class_head.hip): the classification twins of mca_probe_head_f32 and
 * mca_task_head_fwd_bwd.  One wavefront per row, one class per lane (C <= 64); the row maximum m is subtracted before expf, S is the
 * sum of the exponentials and the row's negative log-likelihood is (m + logf(S)) - z_y.  A label is a CLASS INDEX when it is an
 * integer value in [0, C); anything else (negative, >= C, fractional, NaN) is none and never indexes anything.
 *
 * Probe head, plain nn.CrossEntropyLoss(): the operands of mca_probe_head_f32 with C classes for its L outputs and ONE label a row,
 * y_r = labels[yidx[r] * ldy] (yidx may be NULL: row r), ldy >= 1.  pred[r, c] = z[r, c] = a[aidx[r]] . w[c] + bias[c];
 * row loss = -log softmax(z_r)[y_r]; dz (may be NULL) [B, C] = (softmax(z_r) - onehot(y_r)) / B; da (may be NULL) [B, K] as
 * mca_probe_head_f32 forms it from dz; loss_part[mca_probe_head_blocks(B)] = per-block sums of the row losses (the caller passes
 * count = B to mca_probe_loss_accum).  A row whose label is no class index gets loss 0 and dz 0; the divisor stays B.
 * MCA_E_BADARG: a required pointer NULL, B, K < 1, C < 2, lda < K, ldy < 1.  MCA_E_UNSUPPORTED: K > 1024 or C > 64.             */
int mca_probe_head_ce_f32(const float* a, int64_t lda, const int32_t* aidx, int64_t K, const float* w, const float* bias, int64_t C,
                          const float* labels, int64_t ldy, const int32_t* yidx, int64_t B, float* pred, float* dz, float* da,
                          float dact_scale, float* loss_part, mca_stream_t stream);

/* Class head over the pooled tokens (fine-tuning): mca_task_head_fwd_bwd with the softmax cross-entropy of C classes for its
 * elementwise losses.  x[s, :] = pooled[s, slot, :]; y_s = labels[s * ld_labels].  Row s is COUNTED iff it is valid by presence
 * (any_bits == 0 or (present[s] & any_bits) != 0) and y_s is a class index; a negative label marks an unlabelled row, and every
 * other label that is no class index is treated the same way.  The label of a row that is invalid by presence is never read.
 * With cw = class_weights (all ones when NULL), eps = label_smoothing, p_s = softmax(z_s) and W = sum of cw[y_s] over counted rows:
 *   pred[s, c]   = z[s, c] = x[s] . w[c] + bias[c], written for every row
 *   loss[0]      = (1 / W) sum_s [ (1 - eps) cw[y_s] (-log p_s[y_s]) + (eps / C) sum_c cw[c] (-log p_s[c]) ] over counted rows, NOT
 *                  scaled by task_weight: torch's cross_entropy(z, y, weight=cw, label_smoothing=eps, reduction="mean") over the
 *                  counted rows.  0 when W == 0 (nothing counted, or only classes of weight 0).
 *   loss[1]      = the number of counted rows;  loss[2] = W
 *   dz[s, c]     = fl(task_weight / W) * [ (1 - eps) cw[y_s] (p_s[c] - [c == y_s]) + (eps / C) (p_s[c] sum_k cw[k] - cw[c]) ] on
 *                  counted rows, 0 elsewhere and when W == 0
 *   gw, gb, d_pooled (base_weight, d_pooled_in, aliasing) and accumulate: exactly as in mca_task_head_fwd_bwd.
 * Two launches: one workgroup per 64 rows (one wave per row) stores its share of gw, gb and the loss into its slot of the
 * workspace, rows in order; the second launch adds the slots in block order.  Every workgroup forms the count and W itself, all by
 * the same order.  No atomics: two calls on unchanged inputs give the same bits.  Rows of pooled, w, d_pooled and gw move as
 * 16-byte accesses.
 * MCA_E_BADARG: args or a required pointer NULL, b < 1, R < 1, D < 1, C < 2, slot outside [0, R), ld_labels < 1, label_smoothing
 * outside [0, 1) or NaN, accumulate not 0 / 1, present NULL with any_bits != 0, a NaN weight, workspace_bytes below the query.
 * MCA_E_UNSUPPORTED: D > 1024 or C > 64.  MCA_E_ALIGN: D % 4 != 0; pooled, w, d_pooled, d_pooled_in, gw or workspace not 16-byte
 * aligned; another pointer not 4-byte aligned.  Every check returns before anything is launched.                              */
typedef struct {
  const float* pooled;              /* (b, R, D) dense fp32                                          */
  const uint32_t* present;          /* (b) presence words of the step, or NULL (any_bits == 0)       */
  uint32_t any_bits;
  int b, R, D, slot;
  const float* w; const float* bias;          /* (C, D) row-major, (C)                               */
  int C;
  const float* labels;              /* y_s = labels[s * ld_labels]: one fp32 class index a row       */
  int64_t ld_labels;
  const float* class_weights;       /* (C), or NULL for all ones                                     */
  float label_smoothing;            /* in [0, 1)                                                     */
  float task_weight, base_weight;
  const float* d_pooled_in;         /* (b, R, D) or NULL                                             */
  float* pred;                      /* (b, C) logits                                                 */
  float* loss;                      /* [3]                                                           */
  float* d_pooled;                  /* (b, R, D); may alias d_pooled_in                              */
  float* gw; float* gb;             /* (C, D), (C)                                                   */
  int accumulate;
  float* workspace; int64_t workspace_bytes;
} mca_class_head_args;
/* bytes of workspace mca_class_head_fwd_bwd needs (host only): ceil(b / 64) slots of C*D + roundup4(C) + 4 floats; -1 for sizes the
 * entry point refuses (b < 1, C outside 2 .. 64, D outside 4 .. 1024 or D % 4 != 0)                                             */
int64_t mca_class_head_workspace_bytes(int b, int C, int D);
int mca_class_head_fwd_bwd(const mca_class_head_args* args, mca_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deterministic mode: fixed-order forms of the six entry points whose parameter gradients are sums of
 * fp32 atomics ("Deterministic mode").  Each takes the arguments of its plain form plus
 * `scratch` (device, fp32) and its size in floats; the *_scratch queries (host only, nothing launched)
 * give the floats a problem needs.  A scratch that is NULL or too small: MCA_E_BADARG, nothing launched.
 * Every contributing workgroup STORES its partial into slot s of the scratch (s = its row split / slab
 * index, a function of the problem shape, the knob table and - grouped form only - the CU count; never
 * of timing or placement); a second launch on the same stream then computes, per destination element,
 *     dst = dst + (((p_0 + p_1) + p_2) + ... + p_{S-1})        sequentially in fp32,
 * with a plain read-modify-write: the caller orders calls that target the same tensor (stream order
 * does).  The scratch needs no zeroing and holds nothing between calls; calls on one stream may share it.
 * The partials are the plain forms' own (same tiles, same row ranges, same per-row arithmetic).
 *
 * Slot layouts (slot s at scratch + s * slot_stride, all packed fp32):
 *   mca_gemm_tn_acc_det        S = the plain form's row splits; slot = [N][K], slot_stride = N*K.
 *                              S == 1: the plain kernel runs, need 0, scratch unused.
 *   mca_gemm_tn_acc_group_det  grouped launch: S uniform row splits of every tile (S = CUs / tiles, at
 *                              least 128 rows each); slot = member 0's [N_0][K_0], then member 1's, ...;
 *                              slot_stride = sum N_i*K_i.  S == 1: need 0.  Groups the grouped kernel does
 *                              not take: one mca_gemm_tn_acc_det per member in order, each with its own
 *                              layout from scratch + 0; need = the largest member's.
 *   mca_layernorm_bwd_det      S = workgroups of the kernel form the call takes; slot = [3][cols]: dgamma,
 *                              dbeta, dxsum partials (rows of a NULL target are not written), slot_stride
 *                              = 3*cols.  The need is 3*cols * the largest S over the three kernel forms
 *                              for (rows, cols), so it does not depend on which pointers are NULL.
 *   mca_reduce_rows_det        S = row slabs; slot = [period][cols], slot_stride = period*cols.
 *   mca_tab_value_bwd_det      S = row slabs; slot = [2][cols]: dw1, db1; slot_stride = 2*cols.
 *   mca_embedding_scatter_add_det   no slots: the scratch holds two packed int32 arrays of `rows` words, the tokens sorted by
 *                              (table row, position) and their table rows (tokens that contribute nothing last), every
 *                              word written by the first launch.  The second launch computes, per touched element,
 *                              dtable = dtable + (((g_0 + g_1) + g_2) + ...), the row's tokens in position order: an
 *                              order that depends on the index values and the shapes only.  rows, vocab < 2^31.
 * (S and the partition for a weight gradient: mca_dbg_plan_gemm_tn_det / _group_det, mca_hip_debug.h.)
 * cus: CU count to plan the grouped form for, 0 = the current device's.
 * --------------------------------------------------------------------------------------------- */
int64_t mca_gemm_tn_acc_det_scratch(int64_t R, int64_t N, int64_t K);
int mca_gemm_tn_acc_det(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                        int64_t R, int64_t N, int64_t K, float* scratch, int64_t scratch_floats, mca_stream_t stream);
int64_t mca_gemm_tn_acc_group_det_scratch(const int64_t* N, const int64_t* K, int n, int64_t R, int cus);
int mca_gemm_tn_acc_group_det(const mca_tn_desc* d, int n, int64_t R, float* scratch, int64_t scratch_floats, mca_stream_t stream);
int64_t mca_layernorm_bwd_det_scratch(int64_t rows, int cols);
int mca_layernorm_bwd_det(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period,
                          const float* x, int64_t ldx, const float* gamma,
                          const float* mean, const float* rstd, const uint8_t* rowmask,
                          float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16,
                          float* dgamma, float* dbeta, float* dxsum, int64_t rows, int cols,
                          float* scratch, int64_t scratch_floats, mca_stream_t stream);
int64_t mca_reduce_rows_det_scratch(int64_t rows, int64_t period, int cols);
int mca_reduce_rows_det(const float* src, int64_t lds, int64_t src_bstride, int64_t period, float* dst, int64_t ldd,
                        int64_t rows, int cols, float* scratch, int64_t scratch_floats, mca_stream_t stream);
int64_t mca_tab_value_bwd_det_scratch(int64_t rows, int cols);
int mca_tab_value_bwd_det(const float* dh1, int64_t ld, const uint16_t* h1, const float* x, float* dw1, float* db1,
                          int64_t rows, int cols, float max_value, float* scratch, int64_t scratch_floats, mca_stream_t stream);
int64_t mca_embedding_scatter_add_det_scratch(int64_t rows);
int mca_embedding_scatter_add_det(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period, const void* idx, int idx_bytes,
                                  int64_t rows, float* dtable, int64_t vocab, int cols, int64_t padding_idx,
                                  float* scratch, int64_t scratch_floats, mca_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
