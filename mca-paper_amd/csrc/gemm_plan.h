// Which GEMM kernel runs, with which grid, LDS size and integer arguments: the decisions of gemm.hip's entry points as pure
// host functions.  No HIP includes, no global state, no runtime calls: the knob table and the CU count come in as arguments,
// so a host compiler alone builds this header (tests/gemm_plan_check.cpp) and the CPU tests ask the library for its plans
// (mca_dbg_plan_gemm_*, include/mca_hip_debug.h).  gemm.hip validates, calls a planner and launches what the plan says.
#pragma once
#include <stdint.h>

// ---- tile geometry shared by the kernels and the planners
#define BM 128          // gemm_nt_glds_kernel: 128 x 128 output tile
#define BN 128          // column tile of every NT kernel but the 256 x 256 one
#define BM2 256         // row tile of the 256-row NT kernels
#define BR 64           // reduction rows per step of gemm_tn_kernel / gemm_tn_256_kernel
#define BR2 32          // ... of the 256 x 256 weight-gradient kernels
#define P2_STAGE (512 * 32)          // gemm_nt_persist256_kernel, elements per stage: A image [256][32] then B image [256][32]
#define TN2_STAGE (BR2 * 512)        // 256 x 256 weight gradient, elements per stage: A image [32][256] then B image [32][256]
#define TN2_NSTAGE 5
// dynamic LDS of the kernels that need more than the static 64 KiB
#define NT256_LDS_BYTES (3 * (BM2 + BN) * 64 * 2)
#define NT256LN_LDS_BYTES (NT256_LDS_BYTES + 2048)
#define NTPS_LDS_BYTES (3 * (BM2 + BN) * 64 * 2 + 16384)
#define P2_LDS_BYTES (5 * P2_STAGE * 2)
#define TN256_LDS_BYTES (3 * BR * (256 + 128) * 2)
#define TN2_LDS_BYTES (TN2_NSTAGE * TN2_STAGE * 2)

// ---- the launchable kernels, one value per template instantiation.  The three six-member families are laid out as
// base + 3 * OUT_BF16 + RES (glds, 256) and base + 2 * MODE + BIAS (persist), which is how the planner names a member.
enum mca_gemm_kernel {
  MCA_GK_NONE = 0,                     // no fused kernel: mca_gemm_nt_geglu_fwd runs mca_gemm_nt + mca_geglu_fwd
  MCA_GK_NT_GLDS = 1,                  // gemm_nt_glds_kernel<OUT_BF16, RES, 64, 0>           6 values
  MCA_GK_NT_GLDS_GEGLU_BWD = 7,        // gemm_nt_glds_kernel<true, 0, 64, 1>
  MCA_GK_NT_256 = 8,                   // gemm_nt_256_kernel<OUT_BF16, RES, 0, 0>             6 values
  MCA_GK_NT_256_PF = 14,               // gemm_nt_256_kernel<false, 1, 1, 0>   residual tile prefetched
  MCA_GK_NT_256_LNRES = 15,            // gemm_nt_256_kernel<false, 1, 1, 2>   ... and LayerNorm recomputed
  MCA_GK_NT_256_GEGLU_BWD = 16,        // gemm_nt_256_kernel<true, 0, 0, 1>
  MCA_GK_NT_PERSIST = 17,              // gemm_nt_persist_kernel<MODE 0..2, BIAS>             6 values
  MCA_GK_NT_PERSIST_GEGLU_BWD = 23,    // gemm_nt_persist_kernel<3, false>
  MCA_GK_NT_PERSIST_GEGLU_FWD = 24,    // gemm_nt_persist_kernel<4, false>
  MCA_GK_NT_PERSIST256 = 25,           // gemm_nt_persist256_kernel<false>
  MCA_GK_NT_PERSIST256_GEGLU_FWD = 26, // gemm_nt_persist256_kernel<true>
  MCA_GK_TN = 27,                      // gemm_tn_kernel
  MCA_GK_TN_256 = 28,                  // gemm_tn_256_kernel
  MCA_GK_TN_256X256 = 29,              // gemm_tn_256x256_kernel
  MCA_GK_TN_256X256_GROUP = 30,        // gemm_tn_256x256_group_kernel
  MCA_GK_COUNT = 31,
  // The saved-factor GEGLU forms (mca_gemm_nt_geglu_fwd_saved / _bwd_saved): the value of the unsaved sibling + MCA_GK_SAVED.
  // They stand outside the table above (MCA_GK_COUNT counts the base forms), so no existing value, name or count moves.
  MCA_GK_SAVED = 64,
  MCA_GK_NT_GLDS_GEGLU_BWD_SAVED = MCA_GK_SAVED + MCA_GK_NT_GLDS_GEGLU_BWD,              // gemm_nt_glds_kernel<true, 0, 64, 3>
  MCA_GK_NT_256_GEGLU_BWD_SAVED = MCA_GK_SAVED + MCA_GK_NT_256_GEGLU_BWD,                // gemm_nt_256_kernel<true, 0, 0, 3>
  MCA_GK_NT_PERSIST_GEGLU_BWD_SAVED = MCA_GK_SAVED + MCA_GK_NT_PERSIST_GEGLU_BWD,        // gemm_nt_persist_kernel<5, false>
  MCA_GK_NT_PERSIST_GEGLU_FWD_SAVED = MCA_GK_SAVED + MCA_GK_NT_PERSIST_GEGLU_FWD,        // gemm_nt_persist_kernel<6, false>
  MCA_GK_NT_PERSIST256_GEGLU_FWD_SAVED = MCA_GK_SAVED + MCA_GK_NT_PERSIST256_GEGLU_FWD,  // gemm_nt_persist256_kernel<true, true>
  // The full-row form (mca_gemm_nt_res_lnbwd): a workgroup owns whole rows of C and runs the LayerNorm backward's row body on
  // them.  Outside the counted table like the saved forms.
  MCA_GK_NT_ROWS_LNBWD = 128,                                                             // gemm_nt_rows_kernel
  // ... and its 160-row sibling (mca_gemm_nt_res_lnbwd_tall, where the height rule below picks it)
  MCA_GK_NT_ROWS160_LNBWD = 160,                                                          // gemm_nt_rows160_kernel
  // The column-blocked store (mca_gemm_nt_cb): the 256 x 256 bf16 kernel writing C as [N / 64][M][64].  Outside the counted table too.
  MCA_GK_NT_PERSIST256_CB = 256                                                           // gemm_nt_persist256_kernel<false,false,true>
};

// the instantiation a value stands for, spelled as in gemm.hip without blanks
static inline const char* mca_gemm_kernel_name(int k) {
  static const char* const names[MCA_GK_COUNT] = {
      "none",
      "gemm_nt_glds_kernel<false,0,64,0>", "gemm_nt_glds_kernel<false,1,64,0>", "gemm_nt_glds_kernel<false,2,64,0>",
      "gemm_nt_glds_kernel<true,0,64,0>", "gemm_nt_glds_kernel<true,1,64,0>", "gemm_nt_glds_kernel<true,2,64,0>",
      "gemm_nt_glds_kernel<true,0,64,1>",
      "gemm_nt_256_kernel<false,0,0,0>", "gemm_nt_256_kernel<false,1,0,0>", "gemm_nt_256_kernel<false,2,0,0>",
      "gemm_nt_256_kernel<true,0,0,0>", "gemm_nt_256_kernel<true,1,0,0>", "gemm_nt_256_kernel<true,2,0,0>",
      "gemm_nt_256_kernel<false,1,1,0>", "gemm_nt_256_kernel<false,1,1,2>", "gemm_nt_256_kernel<true,0,0,1>",
      "gemm_nt_persist_kernel<0,false>", "gemm_nt_persist_kernel<0,true>", "gemm_nt_persist_kernel<1,false>",
      "gemm_nt_persist_kernel<1,true>", "gemm_nt_persist_kernel<2,false>", "gemm_nt_persist_kernel<2,true>",
      "gemm_nt_persist_kernel<3,false>", "gemm_nt_persist_kernel<4,false>",
      "gemm_nt_persist256_kernel<false>", "gemm_nt_persist256_kernel<true>",
      "gemm_tn_kernel", "gemm_tn_256_kernel", "gemm_tn_256x256_kernel", "gemm_tn_256x256_group_kernel"};
  switch (k) {
    case MCA_GK_NT_GLDS_GEGLU_BWD_SAVED: return "gemm_nt_glds_kernel<true,0,64,3>";
    case MCA_GK_NT_256_GEGLU_BWD_SAVED: return "gemm_nt_256_kernel<true,0,0,3>";
    case MCA_GK_NT_PERSIST_GEGLU_BWD_SAVED: return "gemm_nt_persist_kernel<5,false>";
    case MCA_GK_NT_PERSIST_GEGLU_FWD_SAVED: return "gemm_nt_persist_kernel<6,false>";
    case MCA_GK_NT_PERSIST256_GEGLU_FWD_SAVED: return "gemm_nt_persist256_kernel<true,true>";
    case MCA_GK_NT_ROWS_LNBWD: return "gemm_nt_rows_kernel";
    case MCA_GK_NT_ROWS160_LNBWD: return "gemm_nt_rows160_kernel";
    case MCA_GK_NT_PERSIST256_CB: return "gemm_nt_persist256_kernel<false,false,true>";
  }
  return k >= 0 && k < MCA_GK_COUNT ? names[k] : "?";
}

// What a launch needs beyond the caller's pointers, leading dimensions and M / N / K.
struct mca_gemm_plan {
  int kernel;                        // enum mca_gemm_kernel
  int grid_x, grid_y, block, lds_bytes;
  int n;                             // the N the kernel is given (the fused GEGLU forward passes ip, not 2 * ip)
  int tiles_n, nwg;                  // NT: column tiles and tiles in all, in the kernel's own tile size
  int tiles_k, rows_per_split;       // TN: tiles along K, rows of one split (grid_x = tiles, grid_y = splits)
  int dbg;                           // the knob word the kernel receives (NT persistent: knob 0, gemm_tn_kernel: knob 2, other TN: knob 9)
};

// ======================================================================================================================
// C[M,N] = A.B^T (+ bias, + residual)
// ======================================================================================================================
#define MCA_NT_BIG_M 2048           // rows from which the 256-row kernels are taken
// the k-loops the pipelined kernels are written for (their wait counts assume at least this many k-steps)
#define MCA_NT_P256_MIN_K 192       // gemm_nt_persist256_kernel: 6 steps of 32
#define MCA_NT_PERSIST_MIN_K 320    // gemm_nt_persist_kernel: 5 steps of 64
#define MCA_NT_PF_MIN_K 512         // gemm_nt_256_kernel with the residual prefetch (and the fused LayerNorm form built on it): 8 steps of 64
#define MCA_GEGLU_BWD_BIG_M 40960   // see mca_plan_gemm_nt_geglu_bwd

struct mca_nt_problem {
  int64_t M, N, K;
  int out_bf16;
  int64_t res_period;                // > 0 with a residual: residual row = row % res_period
  uint64_t C, bias, residual;        // addresses: only null-ness (bias, residual) and alignment are read
  int64_t ldc, ldres;
};

static inline int mca_min_int(int a, int b) { return a < b ? a : b; }

static inline mca_gemm_plan mca_plan_gemm_nt(const mca_nt_problem& p, const int* knobs, int cus) {
  const int64_t M = p.M, N = p.N, K = p.K;
  const bool out_bf16 = p.out_bf16 != 0, bias = p.bias != 0;
  const int tiles_n = (int)((N + BN - 1) / BN);
  const int res = !p.residual ? 0 : (p.res_period > 0 ? 2 : 1);
  const bool big = M >= MCA_NT_BIG_M && knobs[1] != 1;            // knob 1 = 1 forces the 128x128 kernel (A/B measurements)
  const int nwg2 = (int)((M + BM2 - 1) / BM2) * tiles_n;
  mca_gemm_plan pl = {};
  pl.n = (int)N; pl.tiles_n = tiles_n; pl.grid_y = 1;
  // persistent kernel for bf16 / plain fp32 outputs (knob 7, A/B measurements: 1 = one-tile-per-workgroup kernels only,
  // 3 = persistent kernel for fp32 + residual as well)
  const bool c16 = p.C % 16 == 0 && p.ldc % (out_bf16 ? 8 : 4) == 0;
  const bool res16 = p.ldres % 4 == 0 && p.residual % 16 == 0;
  // (fp32 output + residual: HBM-bound, the lock-step kernel with its residual prefetch measures 10-16 % faster: MODE 2 of
  // the persistent kernel is only used with knob 7 = 3)
  const bool ps_res = res == 1 && !out_bf16 && res16 && knobs[7] == 3;
  // bf16 output, N % 256 == 0: 256x256 tiles (knob 10 = 1: keep the 256x128 persistent kernel, A/B)
  if (big && knobs[7] == 0 && knobs[10] != 1 && out_bf16 && res == 0 && !bias && N % 256 == 0 && K >= MCA_NT_P256_MIN_K && K % 32 == 0 && c16) {
    pl.kernel = MCA_GK_NT_PERSIST256;
    pl.tiles_n = (int)(N / 256); pl.nwg = (int)((M + 255) / 256) * pl.tiles_n;
    pl.grid_x = mca_min_int(pl.nwg, cus); pl.block = 512; pl.lds_bytes = P2_LDS_BYTES; pl.dbg = knobs[0];
    return pl;
  }
  if (big && (knobs[7] == 0 || knobs[7] == 3) && N % BN == 0 && K >= MCA_NT_PERSIST_MIN_K && c16 && (res == 0 || ps_res) && (!bias || p.bias % 16 == 0)) {
    const int mode = out_bf16 ? 0 : res == 0 ? 1 : 2;
    pl.kernel = MCA_GK_NT_PERSIST + 2 * mode + (bias ? 1 : 0);
    pl.nwg = nwg2;
    pl.grid_x = mca_min_int(nwg2, cus); pl.block = 512; pl.lds_bytes = NTPS_LDS_BYTES; pl.dbg = knobs[0];
    return pl;
  }
  // fp32 + per-row residual: the residual tile prefetched into registers under the k-loop (knob 4 = 1: without, A/B)
  const bool pf = big && !out_bf16 && res == 1 && N % BN == 0 && K >= MCA_NT_PF_MIN_K && res16 && c16 && (!bias || p.bias % 4 == 0) && knobs[4] != 1;
  if (big) {
    pl.kernel = pf ? MCA_GK_NT_256_PF : MCA_GK_NT_256 + (out_bf16 ? 3 : 0) + res;
    pl.nwg = nwg2; pl.block = 512; pl.lds_bytes = NT256_LDS_BYTES;
  } else {
    pl.kernel = MCA_GK_NT_GLDS + (out_bf16 ? 3 : 0) + res;
    pl.nwg = (int)((M + BM - 1) / BM) * tiles_n; pl.block = 256;
  }
  pl.grid_x = pl.nwg;
  return pl;
}

// C = A.B^T (bf16) stored COLUMN-BLOCKED (mca_gemm_nt_cb): column n of row m at C + (n / 64) * cbs + m * 64 + n % 64, cbs >= M * 64
// elements between the 64-column slabs.  Only the 256 x 256 persistent kernel has the store, so the plan is mca_plan_gemm_nt's for a
// packed bf16 C of the same shape - same grid, block, LDS bytes and knob word, knobs 1, 7 and 10 included - with the kernel value
// swapped, wherever that plan is MCA_GK_NT_PERSIST256 and cbs keeps a lane's 16 bytes aligned.  false: refused (MCA_E_UNSUPPORTED).
static inline bool mca_plan_gemm_nt_cb(int64_t M, int64_t N, int64_t K, uint64_t C, int64_t cbs, const int* knobs, int cus, mca_gemm_plan* out) {
  const mca_nt_problem pr = {M, N, K, 1, 0, C, 0, 0, N, 0};
  mca_gemm_plan pl = mca_plan_gemm_nt(pr, knobs, cus);
  if (pl.kernel != MCA_GK_NT_PERSIST256 || cbs % 8 != 0 || cbs < M * 64) return false;
  pl.kernel = MCA_GK_NT_PERSIST256_CB;
  *out = pl;
  return true;
}

// C = A.B^T + LayerNorm(x): the fused form exists for the large-M residual-prefetch kernel only (mca_gemm_nt_lnres refuses
// M < MCA_NT_BIG_M, N % BN and K < MCA_NT_PF_MIN_K; callers keep the two-kernel form there)
static inline bool mca_nt_lnres_supported(int64_t M, int64_t N, int64_t K) {
  return M >= MCA_NT_BIG_M && M <= (1LL << 30) && N % BN == 0 && K >= MCA_NT_PF_MIN_K;
}
static inline mca_gemm_plan mca_plan_gemm_nt_lnres(int64_t M, int64_t N) {
  mca_gemm_plan pl = {};
  pl.kernel = MCA_GK_NT_256_LNRES;
  pl.n = (int)N; pl.tiles_n = (int)(N / BN); pl.nwg = (int)((M + BM2 - 1) / BM2) * pl.tiles_n;
  pl.grid_x = pl.nwg; pl.grid_y = 1; pl.block = 512; pl.lds_bytes = NT256LN_LDS_BYTES;
  return pl;
}

// dh = GEGLU'(h) applied to dg = A.B^T, N = ip.
// below ~40k rows (the data-parallel configs' 8 samples per GPU: 20,304 rows) the 128 x 128 kernel, two or three workgroups
// per CU whose epilogues (0.9 GB of h / dh traffic at b = 32) overlap each other's k-loops, beats the persistent 256 x 128
// one (65 against 75 us at b = 8; 308 against 282 at b = 32: tools/bench_step_gemms.py); knob 1 = 1 forces it (A/B)
static inline mca_gemm_plan mca_plan_gemm_nt_geglu_bwd(int64_t M, int64_t N, int64_t K, const int* knobs, int cus) {
  mca_gemm_plan pl = {};
  pl.n = (int)N; pl.tiles_n = (int)((N + BN - 1) / BN); pl.grid_y = 1;
  if (M >= MCA_GEGLU_BWD_BIG_M && knobs[1] != 1) {
    pl.nwg = (int)((M + BM2 - 1) / BM2) * pl.tiles_n; pl.block = 512;
    if (knobs[7] != 1 && N % BN == 0 && K >= MCA_NT_PERSIST_MIN_K) {
      pl.kernel = MCA_GK_NT_PERSIST_GEGLU_BWD;
      pl.grid_x = mca_min_int(pl.nwg, cus); pl.lds_bytes = NTPS_LDS_BYTES; pl.dbg = knobs[0];
    } else {
      pl.kernel = MCA_GK_NT_256_GEGLU_BWD;
      pl.grid_x = pl.nwg; pl.lds_bytes = NT256_LDS_BYTES;
    }
  } else {
    pl.kernel = MCA_GK_NT_GLDS_GEGLU_BWD;
    pl.nwg = (int)((M + BM - 1) / BM) * pl.tiles_n; pl.grid_x = pl.nwg; pl.block = 256;
  }
  return pl;
}

// h = A.W1^T ([a | gate]) and g = a * gelu(gate) in one pass, N = ip: a column tile is 128 (256 x 256 kernel) or 64 (MODE 4)
// "a" rows of W1 with the gate rows of the same columns.  MCA_GK_NONE: small or oddly shaped, the plain GEMM + mca_geglu_fwd.
static inline mca_gemm_plan mca_plan_gemm_nt_geglu_fwd(int64_t M, int64_t ip, int64_t K, const int* knobs, int cus) {
  mca_gemm_plan pl = {};
  if (M < MCA_NT_BIG_M || knobs[7] == 1) return pl;
  if (ip % 128 == 0 && K >= MCA_NT_P256_MIN_K && knobs[10] != 1) {
    pl.kernel = MCA_GK_NT_PERSIST256_GEGLU_FWD;
    pl.tiles_n = (int)(ip / 128); pl.lds_bytes = P2_LDS_BYTES;
  } else if (ip % 64 == 0 && K >= MCA_NT_PERSIST_MIN_K) {
    pl.kernel = MCA_GK_NT_PERSIST_GEGLU_FWD;
    pl.tiles_n = (int)(ip / 64); pl.lds_bytes = NTPS_LDS_BYTES;
  } else {
    return pl;
  }
  pl.n = (int)ip; pl.nwg = (int)((M + BM2 - 1) / BM2) * pl.tiles_n;
  pl.grid_x = mca_min_int(pl.nwg, cus); pl.grid_y = 1; pl.block = 512; pl.dbg = knobs[0];
  return pl;
}

// The saved-factor forms (mca_gemm_nt_geglu_fwd_saved / _bwd_saved, include/mca_hip.h): the sibling's plan - same grid, block,
// LDS bytes and integer arguments for every shape, knob table and CU count - with the kernel value swapped for the saved one.
// MCA_GK_NONE stays MCA_GK_NONE: the plain GEMM followed by mca_geglu_fwd_saved.
static inline mca_gemm_plan mca_plan_saved(mca_gemm_plan pl) {
  if (pl.kernel != MCA_GK_NONE) pl.kernel += MCA_GK_SAVED;
  return pl;
}
static inline mca_gemm_plan mca_plan_gemm_nt_geglu_fwd_saved(int64_t M, int64_t ip, int64_t K, const int* knobs, int cus) {
  return mca_plan_saved(mca_plan_gemm_nt_geglu_fwd(M, ip, K, knobs, cus));
}
static inline mca_gemm_plan mca_plan_gemm_nt_geglu_bwd_saved(int64_t M, int64_t N, int64_t K, const int* knobs, int cus) {
  return mca_plan_saved(mca_plan_gemm_nt_geglu_bwd(M, N, K, knobs, cus));
}

// ---- the full-row kernel (gemm_nt_rows_kernel): a workgroup computes ROWS_BM whole rows of C[M, ROWS_N] in k-steps of ROWS_BK
// through a ring of ROWS_NSTAGE stages of (A image [128][32], B image [512][32]); its epilogue moves the tile through the same LDS
// 32 rows at a time (row stride ROWS_CS_LD floats: + 4 so that the accumulator rows of the two lane halves, 4 rows apart, fall
// into different banks) and runs a LayerNorm row body on whole rows.
#define ROWS_BM 128
#define ROWS_N 512
#define ROWS_BK 32
#define ROWS_NSTAGE 3
#define ROWS_STAGE ((ROWS_BM + ROWS_N) * ROWS_BK)          // elements per stage
#define ROWS_CS_LD (ROWS_N + 4)
#define ROWS_LDS_BYTES (ROWS_NSTAGE * ROWS_STAGE * 2)      // 120 KiB; the epilogue's 32 x ROWS_CS_LD floats (64.5 KiB) fit inside
#define MCA_NT_ROWS_MIN_K (ROWS_NSTAGE * ROWS_BK)          // the prologue fills every stage of the ring

// mca_gemm_nt_res_lnbwd: one workgroup per 128 rows, any M >= 1 (rows past M are clamped on load and never stored).  < 0: the
// MCA_E_* code the entry point refuses the shape with (-3 = MCA_E_UNSUPPORTED, -2 = MCA_E_ALIGN).
static inline int mca_nt_rows_refusal(int64_t M, int64_t N, int64_t K) {
  if (N != ROWS_N || M > (1LL << 30)) return -3;
  if (K % ROWS_BK) return -2;
  if (K < MCA_NT_ROWS_MIN_K) return -3;
  return 0;
}
static inline mca_gemm_plan mca_plan_gemm_nt_res_lnbwd(int64_t M) {
  mca_gemm_plan pl = {};
  pl.kernel = MCA_GK_NT_ROWS_LNBWD;
  pl.n = ROWS_N; pl.tiles_n = 1; pl.nwg = (int)((M + ROWS_BM - 1) / ROWS_BM);
  pl.grid_x = pl.nwg; pl.grid_y = 1; pl.block = 512; pl.lds_bytes = ROWS_LDS_BYTES;
  return pl;
}

// ---- the tall form (gemm_nt_rows160_kernel, mca_gemm_nt_res_lnbwd_tall): the same kernel with ROWS160_BM rows per workgroup, a ring
// of three stages of (A image [160][32], B image [512][32]).  The epilogue's uses of the ring are those of the 128-row kernel.
#define ROWS160_BM 160
#define ROWS160_STAGE ((ROWS160_BM + ROWS_N) * ROWS_BK)          // elements per stage
#define ROWS160_LDS_BYTES (ROWS_NSTAGE * ROWS160_STAGE * 2)      // 126 KiB
#define MCA_KNOB_ROWS_HEIGHT 15                                  // 1 = always 128 rows, 2 = always 160 (include/mca_hip_debug.h)

// The height rule.  Model: one workgroup per CU at a time (either form's LDS allows no second one), every round of the launch
// lasts as long as one tile, and a tile's time follows its rows - the k-loop and the epilogue's streams alike.  A launch then
// costs rounds x rows per tile = ceil(ceil(M / h) / cus) * h row times on its busiest CU.  Ties go to 128, the form with the
// smaller tail.
static inline int64_t mca_nt_rows_cost(int64_t M, int h, int cus) {
  const int64_t tiles = (M + h - 1) / h;
  return (tiles + cus - 1) / cus * h;
}
static inline int mca_nt_rows_height(int64_t M, int cus) {
  if (cus < 1) cus = 1;
  return mca_nt_rows_cost(M, ROWS160_BM, cus) < mca_nt_rows_cost(M, ROWS_BM, cus) ? ROWS160_BM : ROWS_BM;
}
// mca_gemm_nt_res_lnbwd_tall: the plan of mca_gemm_nt_res_lnbwd where the height is 128, one workgroup per 160 rows otherwise.
// Refusals: mca_nt_rows_refusal.
static inline mca_gemm_plan mca_plan_gemm_nt_res_lnbwd_tall(int64_t M, const int* knobs, int cus) {
  const int forced = knobs[MCA_KNOB_ROWS_HEIGHT];
  const int h = forced == 1 ? ROWS_BM : forced == 2 ? ROWS160_BM : mca_nt_rows_height(M, cus);
  if (h == ROWS_BM) return mca_plan_gemm_nt_res_lnbwd(M);
  mca_gemm_plan pl = {};
  pl.kernel = MCA_GK_NT_ROWS160_LNBWD;
  pl.n = ROWS_N; pl.tiles_n = 1; pl.nwg = (int)((M + ROWS160_BM - 1) / ROWS160_BM);
  pl.grid_x = pl.nwg; pl.grid_y = 1; pl.block = 512; pl.lds_bytes = ROWS160_LDS_BYTES;
  return pl;
}

// ======================================================================================================================
// weight gradient C[N,K] += A[R,N]^T . B[R,K], the reduction split over rows (fp32 atomics)
// ======================================================================================================================
#define MCA_TN_BIG_N 512            // 256-row tiles from here ...
#define MCA_TN_BIG_R 4096           // ... when there are this many rows to reduce
#define MCA_TN_HUGE_MIN_K 512
// 256x256 tiles when the output has at least 8 of them (a 512x512 gradient has 4: the 256x128 kernel with half the
// splits, i.e. half the atomic bytes, measured 70 vs 93 us)
#define MCA_TN_HUGE_MIN_TILES 8

static inline mca_gemm_plan mca_plan_gemm_tn(int64_t R, int64_t N, int64_t K, const int* knobs) {
  const bool big = N >= MCA_TN_BIG_N && R >= MCA_TN_BIG_R && knobs[5] != 1;          // knob 5 = 1 forces the 128x128 kernel, 2 the 256x128 one
  const bool huge = big && K >= MCA_TN_HUGE_MIN_K && knobs[5] != 2 && ((N + 255) / 256) * ((K + 255) / 256) >= MCA_TN_HUGE_MIN_TILES;
  const int tiles_k = (int)(huge ? (K + 255) / 256 : (K + 127) / 128);
  const int tiles_n = big ? (int)((N + 255) / 256) : (int)((N + 127) / 128);
  const int tiles = tiles_n * tiles_k;
  // split the reduction: one (big: 1 WG/CU) or two (2 WGs/CU) full rounds of workgroups of a 256-CU chip; every split adds
  // N*K*4 bytes of fp32 atomics; at least 4 steps of 64 rows each
  int64_t splits = big ? (tiles <= 16 ? 256 / tiles : 512 / tiles) : (tiles <= 32 ? 512 / tiles : 1024 / tiles);
  if (huge) splits = 256 / tiles > 0 ? 256 / tiles : 1;
  if (knobs[3] > 0) splits = knobs[3];
  const int64_t max_splits = (R + 4 * BR - 1) / (4 * BR);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  if (splits > 65535) splits = 65535;
  int64_t rps = (R + splits - 1) / splits;
  rps = (rps + BR - 1) / BR * BR;
  splits = (R + rps - 1) / rps;
  mca_gemm_plan pl = {};
  pl.kernel = huge ? MCA_GK_TN_256X256 : big ? MCA_GK_TN_256 : MCA_GK_TN;
  pl.grid_x = tiles; pl.grid_y = (int)splits; pl.block = big ? 512 : 256;
  pl.lds_bytes = huge ? TN2_LDS_BYTES : big ? TN256_LDS_BYTES : 0;
  pl.n = (int)N; pl.tiles_k = tiles_k; pl.rows_per_split = (int)rps;
  pl.dbg = big ? knobs[9] : knobs[2];
  return pl;
}

// ---- several weight gradients over the SAME token rows in one launch (gemm_tn_256x256_group_kernel)
#define MCA_TN_GROUP_MIN_R 4096     // fewer rows: one launch per member
#define MCA_TN_GROUP_MIN_DIM 256    // a member narrower than one 256 x 256 tile either way is not taken
#define MCA_TN_GROUP_MIN_TILES 16   // a group too small to fill the chip goes through the single-problem entry point
#define TN_SPAN_RELIEF 1536         // rows a two-tile workgroup is relieved of (measured: tools/bench_tn_group.py)

// The row partition of a grouped launch.  Every workgroup reduces `unit` rows of one tile's worth of work.  The first
// n_full * tiles workgroups take whole (tile, split) cells of `unit` rows (the tiles of one split next to each other on an XCD, so
// that an operand row block is fetched into one L2 once); the rows left over, [n_full * unit, R) of every tile, form a second,
// tile-major line of tiles * (R - n_full * unit) row-units that the remaining workgroups cut into equal spans of `span` rows (a
// little less than `unit`): such a workgroup finishes one tile's rest and starts the next one's (two atomic epilogues).  Any
// number of tiles then fills the chip's one round of workgroups: 52 tiles are 4 full splits on 208 CUs + 48 spans, not 4 splits
// with 48 CUs idle (worth 7 % at b = 32, not 19 %: the launch is bound by the shared L2 -> LDS and atomic paths,
// tools/bench_tn_group.py).
// own > 0 (when the line's workgroups are at least half as many as the tiles): the first `own` of them each take the whole
// rest of "their" tile first - rows [n_full * unit, R) of tiles 0 .. own - 1, the SAME rows at the same time, so these segments
// share operand rows through L2 like the cells do - and only tiles own .. tiles - 1 form the line (spans of `span` rows)
struct mca_tn_partition {
  int tiles, R;
  int unit, n_full, span;          // rows of a whole cell, cells per tile, rows of a span of the line
  int own;
};

struct mca_tn_group_plan {
  int grouped;                     // 0: one mca_gemm_tn_acc launch per member;  1: one grouped launch;  < 0: that MCA_E_* code
  mca_gemm_plan launch;            // grouped launch: kernel, grid_x workgroups, LDS bytes, knob 9
  mca_tn_partition part;
};

// tiles of one member in the grouped kernel, 0 if it does not take the member
static inline int mca_tn_group_member_tiles(int64_t N, int64_t K) {
  if (N < MCA_TN_GROUP_MIN_DIM || K < MCA_TN_GROUP_MIN_DIM || N > (1 << 24) || K > (1 << 24)) return 0;
  return (int)((N + 255) / 256) * (int)((K + 255) / 256);
}

// tiles: the sum of mca_tn_group_member_tiles over the n members, or 0 if one of them is not taken.
// One full round of workgroups (1 per CU).  n_full whole splits of `unit` rows per tile + `spans` workgroups on the tile-major
// line of the rows left over.  A span workgroup pays two pipeline fills and two atomic epilogues, so it gets `relief` rows less
// than a cell: unit = (tiles * R + spans * relief) / CUs.  At least 4 steps of 32 rows per workgroup.
// knob 3 = s: s uniform splits and no line (the round-3 partition, A/B); knob 6 = r + 1: relief of 32 r rows, -(r + 1): the
// same without owner segments; knob 11 = 1: always one launch per member (A/B)
static inline mca_tn_group_plan mca_plan_gemm_tn_group(int tiles, int n, int64_t R, const int* knobs, int cus) {
  mca_tn_group_plan pl = {};
  if (knobs[11] == 1 || R < MCA_TN_GROUP_MIN_R || n == 1 || tiles < MCA_TN_GROUP_MIN_TILES || tiles > 65535) return pl;
  const int k6 = knobs[6];
  // (a FIXED relief: scaling it down with R - at most an eighth of a cell - was measured and is worse at small R: b = 2, 52 / 60 tiles
  //  73.6 / 78.0 us with 1,536 rows against 76.9 / 95.0 with 512; b = 16 within 2 % either way.  tools/bench_tn_group.py 2 8 16)
  const int64_t relief = k6 != 0 ? 32 * (int64_t)((k6 < 0 ? -k6 : k6) - 1) : TN_SPAN_RELIEF;
  int64_t n_full = cus / tiles, unit, rest, span = 0, spans = 0, own = 0;
  if (knobs[3] > 0) {
    unit = ((R + knobs[3] - 1) / knobs[3] + BR2 - 1) / BR2 * BR2;
    n_full = (R + unit - 1) / unit; rest = 0;                 // uniform splits: the last one is short
  } else {
    const int64_t sp0 = cus - n_full * tiles, left = tiles - sp0;          // line workgroups; tiles without an owner among them
    const bool owners = k6 >= 0 && n_full > 0 && sp0 > 0 && left > 0 && left <= sp0;
    if (owners) {
      // a line workgroup reduces rest + left * rest / sp0 rows, a cell `unit` = that + relief:  rest * f + relief = unit,
      // rest = R - n_full * unit,  f = 1 + left / sp0
      const double f = 1.0 + (double)left / (double)sp0;
      unit = (int64_t)(((double)R * f + (double)relief) / ((double)n_full * f + 1.0));
      if (unit < 4 * BR2) unit = 4 * BR2;
      unit = (unit + BR2 - 1) / BR2 * BR2;
      rest = R - n_full * unit;
    }
    if (owners && rest >= BR2) {
      own = sp0;
      span = (left * rest + sp0 - 1) / sp0;
      if (span < 4 * BR2) span = 4 * BR2;
      span = (span + BR2 - 1) / BR2 * BR2;
      spans = sp0;
    } else {
      for (;;) {
        const int64_t sp = cus - n_full * tiles;                // workgroups left for the line
        unit = ((int64_t)tiles * R + sp * relief + cus - 1) / cus;
        if (unit < 4 * BR2) unit = 4 * BR2;
        unit = (unit + BR2 - 1) / BR2 * BR2;
        rest = R - n_full * unit;
        if (rest >= 0 || n_full == 0) break;
        n_full--;                                               // (tiny R: fewer whole splits)
      }
      if (n_full == 0) { rest = R; }
      if (rest > 0) {
        const int64_t sp = cus - n_full * tiles > 0 ? cus - n_full * tiles : cus;
        span = ((int64_t)tiles * rest + sp - 1) / sp;
        if (span < 4 * BR2) span = 4 * BR2;
        span = (span + BR2 - 1) / BR2 * BR2;
        spans = ((int64_t)tiles * rest + span - 1) / span;
      }
    }
  }
  const int64_t grid = n_full * tiles + spans;
  if (grid <= 0 || grid > (1 << 30)) { pl.grouped = -3; return pl; }          // MCA_E_UNSUPPORTED
  pl.grouped = 1;
  pl.launch.kernel = MCA_GK_TN_256X256_GROUP;
  pl.launch.grid_x = (int)grid; pl.launch.grid_y = 1; pl.launch.block = 512; pl.launch.lds_bytes = TN2_LDS_BYTES; pl.launch.dbg = knobs[9];
  pl.part.tiles = tiles; pl.part.R = (int)R;
  pl.part.unit = (int)unit; pl.part.n_full = (int)n_full; pl.part.span = (int)span; pl.part.own = (int)own;
  return pl;
}

// The decode of that partition: the segments (tile, rows [r_begin, r_end)) of workgroup `lin`, each handed to emit().  This is a
// line-for-line HOST COPY of the segment loop of gemm_tn_256x256_group_kernel (gemm.hip) - sharing one function between the
// two changed the kernel's machine code - so a change to either is a change to both; tests/gemm_plan_check.cpp runs this one
// over every workgroup of a planned grid.
template <typename Emit>
static inline void mca_tn_group_segments(const mca_tn_partition& g, int lin, Emit emit) {
  const int n_cells = g.n_full * g.tiles;
  const int row0 = g.n_full * g.unit, rest = g.R - row0;          // rows [row0, R) of every tile
  const int line0 = g.own;
  int64_t s = 0, e = 0;
  bool own_pending = false;
  if (lin >= n_cells) {
    const int j = lin - n_cells;
    own_pending = j < g.own;
    s = (int64_t)j * g.span;
    e = s + g.span;
    const int64_t line = (int64_t)(g.tiles - line0) * rest;
    if (e > line) e = line;
  }
  for (;;) {
    int tile_all, r_begin, r_end;
    if (lin < n_cells) {
      tile_all = lin % g.tiles;
      r_begin = (lin / g.tiles) * g.unit; r_end = r_begin + g.unit;
    } else if (own_pending) {
      own_pending = false;
      tile_all = lin - n_cells;
      r_begin = row0; r_end = g.R;
    } else {
      if (s >= e) break;
      const int t = (int)(s / rest);
      tile_all = line0 + t;
      const int off = (int)(s - (int64_t)t * rest);
      int len = rest - off; if ((int64_t)len > e - s) len = (int)(e - s);
      r_begin = row0 + off; r_end = r_begin + len;
      s += len;
    }
    if (r_end > g.R) r_end = g.R;
    emit(tile_all, r_begin, r_end);
    if (lin < n_cells) break;
  }
}

// ======================================================================================================================
// Deterministic forms (mca_gemm_tn_acc_det, mca_gemm_tn_acc_group_det): the same tiles and row splits, but every split
// STORES its whole [N, K] partial into a slot of its own of the caller's scratch (slot = logical split index), and one
// reduce launch then adds the slots in ascending order into C.  The plans below say how many slots there are, how far
// apart they lie and how much scratch that takes.  slots == 1: one contributor per element already - the plain kernel
// runs (its one atomic add per element is dst + p_0) and no scratch is needed.
// ======================================================================================================================
struct mca_tn_det_plan {
  mca_gemm_plan launch;            // mca_plan_gemm_tn's launch, unchanged: grid_x tiles, grid_y = slots row splits
  int slots;                       // partial slabs [N, K] (packed, leading dimension K), slot s at scratch + s * slot_stride
  int64_t slot_stride;             // N * K floats
  int64_t scratch_floats;          // slots * slot_stride; 0 when slots == 1
};

static inline mca_tn_det_plan mca_plan_gemm_tn_det(int64_t R, int64_t N, int64_t K, const int* knobs) {
  mca_tn_det_plan d = {};
  d.launch = mca_plan_gemm_tn(R, N, K, knobs);
  d.slots = d.launch.grid_y;
  d.slot_stride = N * K;
  d.scratch_floats = d.slots > 1 ? d.slots * d.slot_stride : 0;
  return d;
}

// A group: the uniform-split partition the default planner has behind knob 3 (n_full = S cells of `unit` rows per tile, no
// tile-major line, no owner segments), so that every (tile, split) cell has exactly ONE workgroup and a slot is a split.
// S: the whole rounds of workgroups one per CU that the tiles allow, cus / tiles - what the default plan takes as n_full
// before it deals the remaining CUs out as spans; the deterministic form leaves those CUs idle instead (a span's partial
// would need a slot whose position depends on the balance).  At least 4 steps of 32 rows per cell, at least 1 split;
// knob 3 > 0 sets S as it sets the splits everywhere else.  A slot holds the members' [N_i, K_i] partials one after the
// other (member i at sum_{j < i} N_j * K_j, packed).  plan.grouped == 0: the default planner refuses the group (few rows,
// one member, few tiles, knob 11): one single-problem deterministic launch per member, each reusing the scratch, whose
// need is then the largest member's.
struct mca_tn_group_det_plan {
  mca_tn_group_plan plan;          // grouped == 1: part.n_full == slots, part.span == part.own == 0
  int slots;
  int64_t slot_stride;             // sum of N_i * K_i
  int64_t scratch_floats;
};

static inline mca_tn_group_det_plan mca_plan_gemm_tn_group_det(const int64_t* N, const int64_t* K, int n, int64_t R, const int* knobs, int cus) {
  mca_tn_group_det_plan d = {};
  int tiles = 0;
  bool all_taken = true;
  for (int i = 0; i < n; i++) {
    const int t = mca_tn_group_member_tiles(N[i], K[i]);
    all_taken = all_taken && t > 0;
    tiles += t;
    d.slot_stride += N[i] * K[i];
  }
  if (!all_taken) tiles = 0;
  int kn[16];
  for (int i = 0; i < 16; i++) kn[i] = knobs[i];
  if (kn[3] <= 0) {
    int64_t s = tiles > 0 ? cus / tiles : 1;
    const int64_t max_s = R / (4 * BR2);
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    kn[3] = (int)s;
  }
  d.plan = mca_plan_gemm_tn_group(tiles, n, R, kn, cus);
  if (d.plan.grouped == 1) {
    d.slots = d.plan.part.n_full;
    d.scratch_floats = d.slots > 1 ? d.slots * d.slot_stride : 0;
  } else if (d.plan.grouped == 0) {
    d.slots = 0; d.slot_stride = 0;
    for (int i = 0; i < n; i++) {
      const mca_tn_det_plan m = mca_plan_gemm_tn_det(R, N[i], K[i], knobs);
      if (m.scratch_floats > d.scratch_floats) d.scratch_floats = m.scratch_floats;
    }
  }
  return d;
}
