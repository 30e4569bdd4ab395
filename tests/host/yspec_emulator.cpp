// The block-shift formula and the live-block masks of the y-spectral sweep (pygpa_amd/csrc/gpa_yspec.h) against the
// transform's own spec_index: for every band rotation s, thread and live register, the stored position pass B reads must hold
// the bin the forward transform of the rotated row would have left in that register, i.e. spec_index + s L / 16 (mod L).
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "gpa_yspec.h"

using namespace gpa;

template <int LG>
static void check() {
  using F = WgFFT<float, LG, 16>;
  constexpr int L = F::L, TPF = F::TPF;
  if (!yspec_lg_ok(LG)) { printf("lg %d not taken\n", LG); exit(1); }
  for (int nbl : {6, 8})
    for (int s = 0; s < 16; ++s) {
      const unsigned mask = yspec_blockmask(LG, s, nbl);
      unsigned used = 0;
      for (int t = 0; t < TPF; ++t)
        for (int i = 0; i < nbl; ++i) {
          const YspecSrc src = yspec_source(LG, s, t, i);
          if (src.tid < 0 || src.tid >= TPF || src.reg < 0 || src.reg >= 16) { printf("range L=%d s=%d t=%d i=%d\n", L, s, t, i); exit(1); }
          const int want = (F::spec_index(t, i) + s * (L / 16)) % L;
          const int got = F::spec_index(src.tid, src.reg);
          if (got != want) { printf("bin L=%d s=%d t=%d i=%d: %d != %d\n", L, s, t, i, got, want); exit(1); }
          if (!((mask >> src.reg) & 1)) { printf("mask misses L=%d s=%d nbl=%d reg=%d\n", L, s, nbl, src.reg); exit(1); }
          used |= 1u << src.reg;
        }
      if (used != mask) { printf("mask too wide L=%d s=%d nbl=%d: %x != %x\n", L, s, nbl, mask, used); exit(1); }
      // a band of nbl blocks: the mask holds nbl stored blocks (4096), or up to two more where an odd shift splits pairs (2048)
      const int bits = __builtin_popcount(mask);
      if (bits < nbl || bits > nbl + 2) { printf("mask size L=%d s=%d nbl=%d: %d\n", L, s, nbl, bits); exit(1); }
    }
  // sign of the shift: rotating a pure tone exp(2 pi i k0 y / L) by exp(-2 pi i s y / 16) leaves it in bin k0 - s L / 16; with
  // s = 0 the map is the identity
  for (int t = 0; t < TPF; ++t)
    for (int i = 0; i < 16; ++i) {
      const YspecSrc src = yspec_source(LG, 0, t, i);
      if (src.tid != t || src.reg != i) { printf("identity L=%d\n", L); exit(1); }
    }
}

int main() {
  check<11>();
  check<12>();
  printf("OK\n");
  return 0;
}
