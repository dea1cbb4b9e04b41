// The plans of the deterministic weight-gradient forms (mca_plan_gemm_tn_det, mca_plan_gemm_tn_group_det, csrc/gemm_plan.h):
// every (tile, row) must be reduced by exactly one workgroup, every workgroup must own exactly one (tile, split) cell - its slot -
// none of them empty, the slot count must be the grid's split count and the scratch slots x the floats of one partial.
// Stand-alone (host compiler, no HIP); tests/test_deterministic_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <vector>

#include "gemm_plan.h"

static int failures = 0;
static void fail(const char* what, long a, long b, long c, long d) {
  if (failures++ < 20) printf("FAIL %s (%ld, %ld, %ld, %ld)\n", what, a, b, c, d);
}

// single problem: split s of the grid reduces rows [s * rows_per_split, min(R, (s + 1) * rows_per_split))
static void check_single(int64_t R, int64_t N, int64_t K, const int* knobs) {
  const mca_tn_det_plan d = mca_plan_gemm_tn_det(R, N, K, knobs);
  const mca_gemm_plan ref = mca_plan_gemm_tn(R, N, K, knobs);
  if (d.launch.kernel != ref.kernel || d.launch.grid_x != ref.grid_x || d.launch.grid_y != ref.grid_y || d.launch.rows_per_split != ref.rows_per_split)
    fail("deterministic launch differs from the plain plan", R, N, K, 0);
  if (d.slots != d.launch.grid_y) fail("slots != splits", R, N, K, d.slots);
  if (d.slot_stride != N * K) fail("slot stride", R, N, K, d.slot_stride);
  if (d.scratch_floats != (d.slots > 1 ? d.slots * N * K : 0)) fail("scratch floats", R, N, K, d.scratch_floats);
  int64_t at = 0;
  for (int s = 0; s < d.slots; s++) {
    const int64_t b = (int64_t)s * d.launch.rows_per_split, e = b + d.launch.rows_per_split < R ? b + d.launch.rows_per_split : R;
    if (b != at || e <= b) fail("split empty or not adjacent", R, N, K, s);
    at = e;
  }
  if (at != R) fail("rows not covered", R, N, K, at);
}

static void check_group(const std::vector<int64_t>& N, const std::vector<int64_t>& K, int64_t R, const int* knobs, int cus) {
  const int n = (int)N.size();
  const mca_tn_group_det_plan d = mca_plan_gemm_tn_group_det(N.data(), K.data(), n, R, knobs, cus);
  int64_t sum = 0, largest = 0;
  for (int i = 0; i < n; i++) {
    sum += N[i] * K[i];
    const int64_t m = mca_plan_gemm_tn_det(R, N[i], K[i], knobs).scratch_floats;
    if (m > largest) largest = m;
  }
  if (d.plan.grouped == 0) {          // single deterministic launches, sharing the scratch
    if (d.scratch_floats != largest) fail("fallback scratch is not the largest member's", R, n, d.scratch_floats, largest);
    for (int i = 0; i < n; i++) check_single(R, N[i], K[i], knobs);
    return;
  }
  if (d.plan.grouped != 1) { fail("plan refused", R, n, d.plan.grouped, 0); return; }
  const mca_tn_partition& g = d.plan.part;
  if (g.span != 0 || g.own != 0) fail("not the uniform partition", R, n, g.span, g.own);
  if (d.slots != g.n_full || d.plan.launch.grid_x != g.n_full * g.tiles) fail("slots != splits of the grid", R, n, d.slots, d.plan.launch.grid_x);
  if (d.slot_stride != sum || d.scratch_floats != (d.slots > 1 ? d.slots * sum : 0)) fail("scratch floats", R, n, d.slot_stride, d.scratch_floats);
  if (knobs[3] == 0 && d.plan.launch.grid_x > cus && d.slots > 1) fail("more than one round of workgroups", R, n, d.plan.launch.grid_x, cus);
  std::vector<int> next_row(g.tiles, 0), count((size_t)g.tiles * g.n_full, 0);
  for (int lin = 0; lin < d.plan.launch.grid_x; lin++) {          // lin ascending = split-major: a tile's cells come in row order
    int segs = 0;
    mca_tn_group_segments(g, lin, [&](int tile, int r_begin, int r_end) {
      segs++;
      if (tile < 0 || tile >= g.tiles) { fail("tile out of range", R, n, tile, lin); return; }
      const int split = lin / g.tiles;          // the kernel's slot index
      if (tile != lin % g.tiles || split >= g.n_full) { fail("cell is not (lin % tiles, lin / tiles)", R, n, tile, lin); return; }
      count[(size_t)split * g.tiles + tile]++;
      if (r_begin != next_row[tile] || r_end <= r_begin) fail("cell empty or not adjacent", R, tile, r_begin, r_end);
      next_row[tile] = r_end;
    });
    if (segs != 1) fail("a workgroup with other than one segment", R, n, lin, segs);
  }
  for (int t = 0; t < g.tiles; t++) if (next_row[t] != R) fail("rows not covered", R, t, next_row[t], 0);
  for (int c : count) if (c != 1) fail("a (tile, split) cell without exactly one workgroup", R, n, c, 0);
}

int main() {
  int cases = 0;
  const int64_t rows_list[] = {16, 500, 777, 1000, 2048, 4096, 4100, 4160, 5000, 5076, 8200, 20304, 81216, 97408, 779264};
  const int64_t dims[][2] = {{512, 512}, {1365, 512}, {512, 1365}, {128, 74}, {200, 136}, {1024, 512}, {512, 256}, {1536, 512}, {74, 512}, {35, 512}};
  const int knob_list[][2] = {{0, 0}, {3, 0}, {0, 1}, {0, 2}, {1, 0}};          // (knob 3, knob 5)
  for (int64_t R : rows_list)
    for (const auto& nk : dims)
      for (const auto& kn : knob_list) {
        int knobs[16] = {0};
        knobs[3] = kn[0]; knobs[5] = kn[1];
        cases++;
        check_single(R, nk[0], nk[1], knobs);
      }
  const std::vector<std::vector<int64_t>> groups_n = {{1536, 1365, 1365, 512}, {1536, 1365, 1365, 512, 512}, {1536, 1365, 1365, 512, 512, 1024},
                                                      {512, 300, 1024, 256, 515}, {512, 100}, {1024, 512}, {512, 512}};
  const std::vector<std::vector<int64_t>> groups_k = {{512, 512, 512, 1365}, {512, 512, 512, 1365, 512}, {512, 512, 512, 1365, 512, 512},
                                                      {512, 700, 256, 256, 260}, {512, 512}, {512, 1024}, {512, 256}};
  const int cus_list[] = {64, 256, 304};
  for (size_t gi = 0; gi < groups_n.size(); gi++)
    for (int64_t R : rows_list)
      for (int cus : cus_list)
        for (int k3 : {0, 1, 3, 7}) {
          int knobs[16] = {0};
          knobs[3] = k3;
          cases++;
          check_group(groups_n[gi], groups_k[gi], R, knobs, cus);
        }
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
