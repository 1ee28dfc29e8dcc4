// ed_lockstep_groups.hpp — how ed_sector_lanc_tridiag_lockstep cuts nseed
// start vectors into groups that advance in lockstep.  Host-only, no HIP: it
// compiles under a plain C++ compiler (tests/test_lockstep_cpu.py).
//
// The block kernel k_spmv_mv exists for 8, 4, 2 and 1 vectors; the seeds are
// taken in order, the widest group first: 13 seeds -> 8 + 4 + 1.
#pragma once

namespace edg {

constexpr int kLockMaxWidth = 8;

// Width of the group that starts when `left` seeds remain (left >= 1): the
// largest of 8, 4, 2, 1 that fits.
inline int lockstep_width(int left) { return left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1; }

// The groups of nseed seeds as (first seed, width), in order.  Returns their
// number; first/width hold at least lockstep_max_groups(nseed) entries.
inline int lockstep_max_groups(int nseed) { return nseed / 8 + 3; }
inline int lockstep_groups(int nseed, int* first, int* width) {
  int n = 0;
  for (int q = 0; q < nseed;) {
    const int w = lockstep_width(nseed - q);
    first[n] = q;
    width[n] = w;
    n++;
    q += w;
  }
  return n;
}

}  // namespace edg
