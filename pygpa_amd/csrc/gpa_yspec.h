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

}  // namespace gpa
