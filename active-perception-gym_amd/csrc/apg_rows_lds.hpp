// apg_rows_lds.hpp — the occupancy row source of the kernels that stage whole packed maps in LDS (k_scan_poses,
// k_move_poses): apg_scan.hpp's lidar_scan reads the map through it.
#pragma once
#include "apg_scan.hpp"

namespace apg {

// Bit rows staged in LDS ([h][wpr], padding bits cleared), read through a 64-column window at x0 as RowsGlobal reads
// global memory: zero outside the map, so segments that leave it need no special case.
struct RowsLds {
  typedef uint64_t word;
  const uint64_t *rows;
  int h, wpr, x0;
  APG_DEV uint64_t row(int y) const {
    if ((unsigned)y >= (unsigned)h) return 0ULL;
    return extract_window_row64(rows + y * wpr, wpr, x0);
  }
  APG_DEV uint64_t row_nw(int y) const { return row(y); }
  APG_DEV uint64_t or_rows(int j0, int j1, int) const {
    uint64_t acc = 0ULL;
    for (int j = j0; j <= j1; j++) acc |= row(j);
    return acc;
  }
};

}  // namespace apg
