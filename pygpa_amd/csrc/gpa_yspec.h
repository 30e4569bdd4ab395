// Index arithmetic of the y-spectral sweep: where pass B finds, in a row of spectrum stored in the spectral
// register layout, what the forward transform of the band-rotated row would have left in its registers.
//
// The row pre-pass stores register i of thread t of  Yhat = FFT_y(row)  at position  i * TPF + t  (TPF = L / 16 threads per
// row).  The spatial pass B multiplies the row by the rotation phasor exp(-2 pi i s y / 16) before its forward transform,
// which moves the spectrum DOWN by s blocks of L / 16 bins:  FFT(T rot)[k] = FFT(T)[k + s L / 16]  (forward kernel
// exp(-2 pi i k y / L)).  So register i of thread t wants the stored value whose bin is  spec_index(t, i) + s L / 16.
//   * 4096 points (three radix-16 passes): register i of every thread holds block i of 256 consecutive bins -> the same
//     thread, register (i + s) mod 16.
//   * 2048 points (16 x 16 x 8): a thread's registers i and i + 1 (i even) share a block of 256 bins, 8 bins apart; a shift by
//     an even s is the register shift above, an odd s lands on thread t ^ 8, two registers further when t & 8.
// GPA_HD: tests/host/yspec_emulator.cpp checks both against WgFFT::spec_index for every (s, t, i).
#pragma once
#include <algorithm>
#include <vector>

#include "gpa_fft.h"

namespace gpa {

// the row lengths the y-spectral path takes
GPA_HD bool yspec_lg_ok(int lg) { return lg == 11 || lg == 12; }

struct YspecSrc { int tid, reg; };   // stored at position reg * TPF + tid

GPA_HD YspecSrc yspec_source(int lg, int s, int tid, int reg) {
  const int odd = lg == 11 ? (s & 1) : 0;
  YspecSrc r;
  r.tid = odd ? (tid ^ 8) : tid;
  r.reg = (reg + s - odd + ((odd && (tid & 8)) ? 2 : 0)) & 15;
  return r;
}

// the stored registers (blocks of L / 16 positions) a peak with band rotation s and nbl live registers reads
GPA_HD unsigned yspec_blockmask(int lg, int s, int nbl) {
  unsigned m = 0;
  for (int i = 0; i < nbl; ++i) {
    m |= 1u << yspec_source(lg, s, 0, i).reg;
    m |= 1u << yspec_source(lg, s, 8, i).reg;
  }
  return m;
}

// Pass A's work list: the (plane, block) pairs whose mask bit is set, gathered by block into groups of at most
// gmax planes.  A workgroup of pass A loads a tile of Yhat once and filters it for every plane of its group, so a block read by
// n planes is fetched ceil(n / gmax) times instead of n times; a block read by more than gmax planes is cut into full groups
// and one remainder.  planes = the flat plane list, every group a contiguous run [first, first + count) of it, ascending.
// The groups are ordered by count, largest first (ties: by block): pass A's tile map starts the groups of an XCD in list order,
// so the long workgroups start first and the short ones fill the tail.  gmax = 1 gives the pairs themselves.
struct YspecGroup { int block, first, count; };
struct YspecGroups {
  std::vector<YspecGroup> groups;
  std::vector<int> planes;
};

inline YspecGroups yspec_groups(const unsigned* mask, int nplanes, int gmax) {
  YspecGroups r;
  if (gmax < 1) gmax = 1;
  for (int blk = 0; blk < 16; ++blk) {
    int run = 0;
    for (int q = 0; q < nplanes; ++q) {
      if (!((mask[q] >> blk) & 1)) continue;
      if (run == 0 || run == gmax) { r.groups.push_back({blk, (int)r.planes.size(), 0}); run = 0; }
      r.planes.push_back(q);
      ++r.groups.back().count;
      ++run;
    }
  }
  std::stable_sort(r.groups.begin(), r.groups.end(), [](const YspecGroup& a, const YspecGroup& b) { return a.count > b.count; });
  return r;
}

// The cap when YSPEC_GROUP is not set, measured at 4096^2, 3 peaks x 16 candidates (f32: blocks read by 12, 12, 4, 8, 12, 12, 12
// planes), pass A in us, rocprofv3 average of 23 launches (profiles/passA_groups.txt):
//   f32:  cap 1: 517   2: 360   3: 366   4: 312   6: 284   12: 313      (one plane per workgroup before the groups: 544)
//   f64:  cap 4: 1270  6: 1293  12: 984                                 (before: 1725)
// f32: an XCD's 32 CUs (one workgroup each) get 576 plane iterations; groups of 6 deal them out in 18 iterations' time, groups
// of 4 in 20 (4.5 rounds), groups of 12 in 24 -- and the times follow.  f64 does best with one group per block.
inline int yspec_group_default(int dtype) { return dtype == 0 ? 6 : 12; }

}  // namespace gpa
