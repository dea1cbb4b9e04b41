// Which LayerNorm kernel a call launches, and with which grid: plain host C++ without HIP, as csrc/gemm_plan.h is for the GEMMs.
// elementwise.hip validates, calls a planner and launches what the plan says; the same planners answer the debug hooks
// (mca_dbg_plan_layernorm_fwd / _bwd, include/mca_hip_debug.h), so a test without a GPU can ask which kernel a case reaches.
// The problems carry every pointer as an integer: the rules read null-ness and alignment only.
#ifndef MCA_LN_PLAN_H
#define MCA_LN_PLAN_H
#include <stdint.h>

enum mca_ln_form {
  MCA_LN_NONE = 0,          // nothing to launch (backward with no output asked for)
  MCA_LN_NARROW = 1,        // ln_fwd_narrow_kernel: 16 lanes per row, 16 rows per workgroup and pass (width 0)
  MCA_LN_TRUNK = 2,         // ln_fwd_trunk_kernel<NI> / ln_bwd_trunk_kernel<NI>: two rows per wavefront (width NI = cols / 256)
  MCA_LN_GENERAL = 3,       // ln_fwd_kernel<VEC> / ln_bwd_kernel<VEC>: one row per wavefront (width VEC = 1 or 4)
  MCA_LN_PARAMS = 4,        // ln_bwd_params_kernel<CW>: a thread per column, a row slab per workgroup (width CW = 64 / 128 / 256)
};

struct mca_ln_fwd_problem {
  int64_t rows; int32_t cols, cols_pad;
  int64_t ldx, ldy, y_bstride, ld_bf16, period;
  uint64_t x, gamma, beta, rowmask, add, y, y_bf16;
};
struct mca_ln_fwd_plan {
  int32_t form, width;
  int64_t grid_x;
  int64_t passes;                 // the most passes a wavefront makes of its row loop (the trunk forward has no loop: 1)
};

struct mca_ln_bwd_problem {
  int64_t rows; int32_t cols, pad_;
  int64_t ldy, y_bstride, period, ldx, lddx, ld_bf16;
  uint64_t dy, x, gamma, rowmask, dx, dx_bf16, dgamma, dbeta, dxsum;
};
struct mca_ln_bwd_plan {
  int32_t form, width;
  int64_t grid_x, grid_y;
  int64_t rows_per_block;          // PARAMS: rows of a workgroup's slab; TRUNK / GENERAL: rows a workgroup takes per pass (8 / 4)
  int64_t slots;                   // workgroup slabs that end with one partial each: the deterministic form's slots
  int64_t passes;                  // the most passes of its row loop a wavefront (PARAMS: a thread, 256 / CW rows of the slab apart) makes
};

// ---- the grids of the three backward forms: one place for the launches and for the deterministic form's scratch need (a slot
// per workgroup slab).  Knob 14 as described in include/mca_hip_debug.h.
static inline int mca_ln_params_cw(int cols) { return cols <= 64 ? 64 : (cols <= 128 ? 128 : 256); }
static inline int64_t ln_bwd_params_slabs(int64_t rows, int cols, int64_t* rpb_out) {
  const int cw = mca_ln_params_cw(cols);
  const int chunks = (cols + cw - 1) / cw;
  int64_t slabs = 1024 / chunks;          // four rounds of workgroups at most (each ends with one atomic per column)
  if (slabs > (rows + 31) / 32) slabs = (rows + 31) / 32;
  if (slabs < 1) slabs = 1;
  const int64_t rpb = (rows + slabs - 1) / slabs;
  if (rpb_out) *rpb_out = rpb;
  return (rows + rpb - 1) / rpb;
}
static inline int64_t ln_bwd_trunk_blocks(int64_t rows, const int* knobs) {
  // one workgroup per CU at most: every workgroup ends with one atomic per column on dgamma, and 1024 of them on the same
  // 512 addresses cost more than the extra loads in flight bring (b = 8: 40.8 -> 28.5 us, b = 32: 108.7 -> 104.0 us;
  // knob 14 = another cap, tools/bench_ln.py)
  int64_t nb = (rows + 7) / 8;
  const int64_t cap = knobs[14] > 0 ? knobs[14] : 256;
  return nb > cap ? cap : nb;
}
static inline int64_t ln_bwd_general_blocks(int64_t rows, const int* knobs) {
  int64_t blocks = (rows + 3) / 4;
  // every workgroup ends with one atomic per column on the same dgamma / dbeta / dxsum addresses, and a wavefront has one row in
  // flight: few workgroups at few rows, up to four per CU at many (measured, tools/bench_ln_encoder.py: 3,600 rows 14.5 us at
  // 256 against 30.7 at 1,024; 48,000 rows 134 us at 256 against 70 at 1,024)
  int64_t bcap = rows / 32;
  if (bcap < 256) bcap = 256;
  if (bcap > 1024) bcap = 1024;
  if (knobs[14] > 0) bcap = knobs[14];
  return blocks > bcap ? bcap : blocks;
}

static inline bool mca_ln_trunk_cols(int cols) { return cols == 256 || cols == 512 || cols == 1024; }

// rows > 0 and 0 < cols <= 1024 (the entry point has refused anything else)
static inline mca_ln_fwd_plan mca_plan_layernorm_fwd(const mca_ln_fwd_problem& p, const int* knobs) {
  mca_ln_fwd_plan o = {MCA_LN_GENERAL, 1, 0, 0};
  if (!p.y && p.y_bf16 && !p.add && p.cols <= 256 && knobs[12] != 1) {          // narrow rows, bf16 output only (knob 12 = 1: general kernel)
    o.form = MCA_LN_NARROW; o.width = 0;
    o.grid_x = (p.rows + 15) / 16; if (o.grid_x > 4096) o.grid_x = 4096;
    o.passes = (p.rows + o.grid_x * 16 - 1) / (o.grid_x * 16);
    return o;
  }
  // 16-byte loads of x and stores of y, 8-byte stores of y_bf16 (gamma, beta and add are read as scalars)
  const bool vec = (p.cols % 4 == 0) && (p.ldx % 4 == 0) && (!p.y || (p.ldy % 4 == 0 && p.y_bstride % 4 == 0)) &&
                   (!p.y_bf16 || (p.ld_bf16 % 4 == 0 && p.y_bf16 % 8 == 0)) &&
                   (p.x % 16 == 0) && (!p.y || p.y % 16 == 0);
  if (vec && !p.beta && !p.rowmask && !p.add && !p.y && p.y_bf16 && p.cols_pad <= p.cols && mca_ln_trunk_cols(p.cols) &&
      p.gamma % 16 == 0 && knobs[12] != 1) {          // knob 12 = 1: general kernel (A/B); any row count, so that a given call form
                                                      // always takes the same arithmetic path
    o.form = MCA_LN_TRUNK; o.width = p.cols / 256;
    o.grid_x = (p.rows + 7) / 8;
    o.passes = 1;
    return o;
  }
  o.width = vec ? 4 : 1;
  o.grid_x = (p.rows + 3) / 4; if (o.grid_x > 8192) o.grid_x = 8192;
  o.passes = (p.rows + o.grid_x * 4 - 1) / (o.grid_x * 4);
  return o;
}

static inline mca_ln_bwd_plan mca_plan_layernorm_bwd(const mca_ln_bwd_problem& p, const int* knobs) {
  mca_ln_bwd_plan o = {MCA_LN_NONE, 0, 0, 1, 0, 0, 0};
  if (!p.dx && !p.dx_bf16 && !p.dxsum && knobs[12] != 1) {          // parameter gradients only
    if (!p.dgamma && !p.dbeta) return o;
    o.form = MCA_LN_PARAMS; o.width = mca_ln_params_cw(p.cols);
    o.grid_x = (p.cols + o.width - 1) / o.width;
    o.grid_y = ln_bwd_params_slabs(p.rows, p.cols, &o.rows_per_block);
    o.slots = o.grid_y;
    o.passes = (o.rows_per_block + 256 / o.width - 1) / (256 / o.width);
    return o;
  }
  // 16-byte loads of x and dy and stores of dx, 8-byte stores of dx_bf16
  const bool vec = (p.cols % 4 == 0) && (p.ldx % 4 == 0) && (p.ldy % 4 == 0) && (p.y_bstride % 4 == 0) &&
                   (!p.dx || p.lddx % 4 == 0) && (!p.dx_bf16 || (p.ld_bf16 % 4 == 0 && p.dx_bf16 % 8 == 0)) &&
                   (p.x % 16 == 0) && (p.dy % 16 == 0) && (!p.dx || p.dx % 16 == 0);
  if (vec && !p.rowmask && p.period <= 0 && !p.dbeta && !p.dxsum && p.dgamma && mca_ln_trunk_cols(p.cols) &&
      p.gamma % 16 == 0 && knobs[12] != 1) {          // knob 12 = 1: general kernel (A/B)
    o.form = MCA_LN_TRUNK; o.width = p.cols / 256;
    o.grid_x = ln_bwd_trunk_blocks(p.rows, knobs);
    o.rows_per_block = 8;
  } else {
    o.form = MCA_LN_GENERAL; o.width = vec ? 4 : 1;
    o.grid_x = ln_bwd_general_blocks(p.rows, knobs);
    o.rows_per_block = 4;
  }
  o.slots = o.grid_x;
  o.passes = (p.rows + o.grid_x * o.rows_per_block - 1) / (o.grid_x * o.rows_per_block);
  return o;
}

// the deterministic form's scratch: [slots][3][cols] floats, slots = the most any form a call of this size can take would write
static inline int64_t mca_plan_layernorm_bwd_det_scratch(int64_t rows, int cols, const int* knobs) {
  int64_t slots = ln_bwd_general_blocks(rows, knobs);
  const int64_t ps = ln_bwd_params_slabs(rows, cols, nullptr);
  if (ps > slots) slots = ps;
  if (mca_ln_trunk_cols(cols)) { const int64_t tb = ln_bwd_trunk_blocks(rows, knobs); if (tb > slots) slots = tb; }
  return slots * 3 * cols;
}
#endif
