/*
 * mca_hip_debug.h — measurement hooks of libmca_hip.so.  NOT part of the drop-in ABI (include/mca_hip.h): these entry
 * points exist for the A/B tools under tools/ and for the tests that compare the production kernels with their
 * conservative forms.  The knob table is process-global; production code never sets it, and every test that does restores
 * it in a fixture finaliser (tests/conftest.py).
 */
#ifndef MCA_HIP_DEBUG_H
#define MCA_HIP_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* knob[key] = value for key in [0, 16); returns 0.  All knobs are 0 in production.  What the library reads them for:
 *    0  persistent NT GEMMs: 8 = s_memtime stamps of workgroup 0 (tools/trace_persist.py), 32 * P = P row panels per tile group
 *    1  = 1: the 128 x 128 NT kernel for every shape;   2  bit 1: weight-gradient 128 x 128 kernel without its atomics (timing)
 *    3  > 0: number of (uniform) row splits of the weight-gradient kernels;   4  = 1: no residual prefetch in the fp32 + residual NT kernel
 *    6  = r + 1: the grouped weight-gradient launch gives its two-tile workgroups 32 r rows less than the others; -(r + 1): the
 *       same with a purely tile-major line (no owner segments)
 *    5  weight-gradient kernel: 1 = 128 x 128, 2 = 256 x 128 where 256 x 256 would be chosen
 *    7  1 = one-tile-per-workgroup NT kernels only, 3 = persistent kernel for fp32 + residual as well;   10  = 1: 256 x 128 persistent
 *       kernel where the 256 x 256 one would be chosen;   11  = 1: one launch per member of a weight-gradient group
 *    8 / 9  attention kernels (9 also the weight-gradient kernels), bit mask: 8 = s_memtime stamps / clock probe of the launch
 *       (trace build; gemm_tn_256x256_group_kernel in every build), 16 = launch order without the XCD remap, 32 = fp8 forward with
 *       register staging instead of LDS-DMA
 *   12  = 1: general LayerNorm kernels where the trunk forms would be chosen
 *   13  mca_patch_ln_fwd: +c = at most c patches per workgroup; -c = the same cap in the wavefront-per-patch form that reads
 *       each patch from global memory instead of staging strip rows through LDS (same results; profiles/patch_encoder.md).
 *       mca_patch_nd_ln_fwd: |c| caps the span the same way; it has no wavefront-per-patch form, the sign is ignored
 *   14  > 0: cap on the workgroups of the LayerNorm backward kernels (default 256) and of mca_reduce_rows (default 512)
 *   15  mca_gemm_nt_res_lnbwd_tall (and plan entry 7), the tile height: 1 = always 128 rows, 2 = always 160 rows; 0 = the height
 *       rule of csrc/gemm_plan.h (mca_nt_rows_height).  mca_gemm_nt_res_lnbwd does not read it
 *   (13 and 15, in their earlier use, selected / tuned the forward attention forms of round 4; gone with tools/overlays/fwd64)
 *   one-pass attention backward (attention_bwd1.hip), knob 9: 8 = s_memtime stamps (trace build, tools/trace_bwd1.py), 16 = launch
 *       order without the XCD remap, 64 = the plain (compiler-scheduled) kernel instead of the pipelined one (cross-check) */
int mca_debug_set(int key, int value);
/* every knob back to 0 */
int mca_debug_reset(void);

/* Which GEMM kernel a call would launch, with which grid, LDS size and integer arguments: the planners of csrc/gemm_plan.h (where
 * the structs are defined), as the entry points call them, with the current knob table.  cus: the CU count to plan for, 0 = ask the
 * runtime.  Nothing is launched and no device is touched.  Return 0 or the MCA_E_* code the entry point would refuse the shape with.
 *   mca_dbg_plan_gemm_nt        entry 0 = mca_gemm_nt, 1 = _lnres, 2 = _geglu_fwd, 3 = _geglu_bwd (the last three read M, N = ip, K only;
 *                               kernel 0 from entry 2: the unfused pair mca_gemm_nt + mca_geglu_fwd),
 *                               4 = _geglu_fwd_saved, 5 = _geglu_bwd_saved (the plans of entries 2 and 3 with the saved kernel),
 *                               6 = _res_lnbwd (reads M, N, K only: the full-row kernel, one workgroup per 128 rows),
 *                               7 = _res_lnbwd_tall (reads M, N, K and cus, and knob 15: the plan of entry 6, or kernel 160 =
 *                               gemm_nt_rows160_kernel with one workgroup per 160 rows where the height rule picks it; cus > 0
 *                               touches no device: the engine asks with it before it chooses the entry point)
 *   mca_dbg_plan_gemm_tn        mca_gemm_tn_acc (its rule does not read the CU count)
 *   mca_dbg_plan_gemm_tn_group  mca_gemm_tn_acc_group over n members of N[i] x K[i]: grouped or single launches, and the row partition
 *   mca_dbg_gemm_kernel_name    the template instantiation a plan's `kernel` value stands for */
struct mca_gemm_plan;
struct mca_nt_problem;
struct mca_tn_group_plan;
int mca_dbg_plan_gemm_nt(int entry, const struct mca_nt_problem* problem, int cus, struct mca_gemm_plan* out);
int mca_dbg_plan_gemm_tn(int64_t R, int64_t N, int64_t K, struct mca_gemm_plan* out);
int mca_dbg_plan_gemm_tn_group(const int64_t* N, const int64_t* K, int n, int64_t R, int cus, struct mca_tn_group_plan* out);
const char* mca_dbg_gemm_kernel_name(int kernel);
/* mca_gemm_nt_cb's plan for a C at address `C` with slab stride cbs: mca_gemm_nt's plan for the same shape with the column-blocked
 * kernel, or MCA_E_UNSUPPORTED where the entry point refuses (the current knob table included).  cus > 0 touches no device: the
 * engine asks with it before it chooses a layout. */
int mca_dbg_plan_gemm_nt_cb(int64_t M, int64_t N, int64_t K, uint64_t C, int64_t cbs, int cus, struct mca_gemm_plan* out);
/* The plans of the deterministic weight-gradient forms (mca_gemm_tn_acc_det, mca_gemm_tn_acc_group_det; structs in csrc/gemm_plan.h):
 * the launch, the slot count, the slot stride and the scratch floats, with the current knob table. */
struct mca_tn_det_plan;
struct mca_tn_group_det_plan;
int mca_dbg_plan_gemm_tn_det(int64_t R, int64_t N, int64_t K, struct mca_tn_det_plan* out);
int mca_dbg_plan_gemm_tn_group_det(const int64_t* N, const int64_t* K, int n, int64_t R, int cus, struct mca_tn_group_det_plan* out);
/* Which LayerNorm kernel a call would launch: the planners of csrc/ln_plan.h (where the structs and the forms are defined), as
 * mca_layernorm_fwd and mca_layernorm_bwd / _bwd_det call them, with the current knob table (12 and 14).  The problem carries every
 * pointer as an integer: only null-ness and alignment are read.  Nothing is launched and no device is touched.  Return 0, or
 * MCA_E_BADARG where the entry point would refuse (rows == 0 included: there is nothing to plan). */
struct mca_ln_fwd_problem;
struct mca_ln_fwd_plan;
struct mca_ln_bwd_problem;
struct mca_ln_bwd_plan;
int mca_dbg_plan_layernorm_fwd(const struct mca_ln_fwd_problem* problem, struct mca_ln_fwd_plan* out);
int mca_dbg_plan_layernorm_bwd(const struct mca_ln_bwd_problem* problem, struct mca_ln_bwd_plan* out);
/* The workspace of mca_contrastive_fwd_bwd for a gathered batch of B rows and T terms, in bytes from the workspace pointer:
 * out = {G offset, G bytes, stats offset, stats bytes, w offset, w bytes}.  G (T, B, B) fp32 holds dG after the call, stats is
 * (T, B, 4) fp32 = {lse of row i, lse of column i, ce_row + ce_col, dsum}, w is (T, W) fp32 with room for W = B ranks.  The entry
 * point and mca_contrastive_workspace_bytes (= w offset + w bytes + 256) place the regions by this function.  Pure host code. */
int mca_dbg_contrastive_layout(int B, int T, int64_t* out);
/* The tile constants and the workspace of mca_contrastive_stream_fwd_bwd: out[14] = {TI owner rows of a block, TJ other-side rows
 * of a tile step, TK columns of D staged per step, the largest D, then (byte offset, bytes) of lse (2, T, B) fp32 (direction 0:
 * rows, 1: columns), erat (2, T, B) = sum p l / sum p, diag (T, B) = l[i][i], the three (T, W) reduction arrays n / s / ds, and w
 * (T, W)}, each (T, W) array with room for W = B.  MCA_E_BADARG: out NULL or a non-positive size.  Pure host code. */
int mca_dbg_contrastive_stream_layout(int B, int T, int64_t* out);
#ifdef __cplusplus
}
#endif
#endif
