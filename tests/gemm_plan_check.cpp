// The row partition of the grouped weight gradient (mca_plan_gemm_tn_group, csrc/gemm_plan.h), decoded for every workgroup of
// the planned grid by the host copy of the kernel's segment loop: each tile's segments must tile the rows [0, R) with no gap,
// overlap or empty segment, and one round of workgroups must not exceed the CU count.  Stand-alone (host compiler, no HIP);
// tests/test_gemm_plan_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "gemm_plan.h"

int main() {
  const int tiles_list[] = {16, 17, 48, 52, 60, 100, 128, 255, 256, 257, 300, 513};
  const int64_t rows_list[] = {4096, 4100, 8200, 20304, 40608, 81216, 324864, 1 << 20};
  const int cus_list[] = {64, 256, 304};
  const int knob_list[][2] = {{0, 0}, {3, 0}, {0, 1}, {0, 49}, {0, -49}, {0, -1}};          // (knob 3, knob 6)
  int cases = 0, failures = 0, max_grid_over_cus = 0;
  for (int tiles : tiles_list)
    for (int64_t R : rows_list)
      for (int cus : cus_list)
        for (const auto& kn : knob_list) {
          int knobs[16] = {0};
          knobs[3] = kn[0]; knobs[6] = kn[1];
          cases++;
          const mca_tn_group_plan pl = mca_plan_gemm_tn_group(tiles, 4, R, knobs, cus);
          auto fail = [&](const char* what, int tile, long a, long b) {
            if (failures++ < 20)
              printf("FAIL tiles=%d R=%ld cus=%d knob3=%d knob6=%d: %s (tile %d: %ld, %ld)\n", tiles, (long)R, cus, kn[0], kn[1], what, tile, a, b);
          };
          if (pl.grouped != 1) { fail("no grouped launch planned", -1, pl.grouped, 0); continue; }
          if (pl.part.tiles != tiles || pl.part.R != R) fail("partition of another problem", -1, pl.part.tiles, pl.part.R);
          if (knobs[3] == 0 && pl.launch.grid_x > cus) fail("more than one round of workgroups", -1, pl.launch.grid_x, cus);
          if (knobs[3] == 0) max_grid_over_cus = std::max(max_grid_over_cus, pl.launch.grid_x - cus);
          std::vector<std::vector<std::pair<int, int>>> seg(tiles);
          bool in_range = true;
          for (int lin = 0; lin < pl.launch.grid_x; lin++)
            mca_tn_group_segments(pl.part, lin, [&](int tile, int r_begin, int r_end) {
              if (tile < 0 || tile >= tiles) { if (in_range) fail("tile out of range", tile, r_begin, r_end); in_range = false; return; }
              seg[tile].push_back({r_begin, r_end});
            });
          for (int t = 0; t < tiles && in_range; t++) {
            std::sort(seg[t].begin(), seg[t].end());
            long at = 0;
            bool ok = true;
            for (const auto& s : seg[t]) {
              if (s.second <= s.first) { fail("empty segment", t, s.first, s.second); ok = false; break; }
              if (s.first != at) { fail(s.first > at ? "gap" : "overlap", t, at, s.first); ok = false; break; }
              at = s.second;
            }
            if (ok && at != R) fail("rows not covered to the end", t, at, (long)R);
            if (!ok) break;
          }
        }
  printf("%d cases, %d failures, largest grid - cus = %d\n", cases, failures, max_grid_over_cus);
  return failures ? 1 : 0;
}
