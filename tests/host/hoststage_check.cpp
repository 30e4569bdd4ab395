// HostStage (pygpa_amd/csrc/gpa_hoststage.h) on the CPU: the primitives of gpa_devbuf.h are malloc / free / a counter / memcpy
// here, so "device" slots are host memory the checks can read and write.  Prints "OK <checks>" and exits 0, or the failed
// check and exits 1.
//   g++ -std=c++17 -DGPA_DEVBUF_HOST_SEAM -I pygpa_amd/csrc tests/host/hoststage_check.cpp
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gpa_hoststage.h"

using namespace gpa;

static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static DevBufSeam& S = g_devbuf_seam;

// sizes that are no multiples of 256: a wrong offset overlaps a neighbour
static const size_t kBytes[4] = {1, 240, 960, 257};
constexpr size_t GUARD = 64;
constexpr unsigned char GUARD_BYTE = 0xA5;

struct HostArray {   // `bytes` of payload, guard bytes behind it
  unsigned char b[1024 + GUARD];
  size_t bytes;
  void fill(size_t n, unsigned seed) {
    bytes = n;
    for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)(seed * 37 + i * 11 + 1);
    memset(b + n, GUARD_BYTE, GUARD);
  }
  bool guard_ok() const {
    for (size_t i = 0; i < GUARD; ++i)
      if (b[bytes + i] != GUARD_BYTE) return false;
    return true;
  }
  bool holds(unsigned seed) const {
    for (size_t i = 0; i < bytes; ++i)
      if (b[i] != (unsigned char)(seed * 37 + i * 11 + 1)) return false;
    return true;
  }
};

static void pattern(void* dev, size_t n, unsigned seed) {
  for (size_t i = 0; i < n; ++i) static_cast<unsigned char*>(dev)[i] = (unsigned char)(seed * 37 + i * 11 + 1);
}

// in(1) | out(240) | absent | in-out(960), upload off | in(257): layout, copies, guards, one drain
static int layout_and_copies() {
  S = DevBufSeam{};
  size_t counter = 0;
  DevBuf buf(&counter);
  HostArray h[4];
  for (int k = 0; k < 4; ++k) h[k].fill(kBytes[k], k);
  HostStage st(buf, nullptr);
  const int a = st.in(h[0].b, kBytes[0]), b = st.out(h[1].b, kBytes[1]), none = st.in(nullptr, 4096);
  const int c = st.inout(h[2].b, kBytes[2], false), d = st.in(h[3].b, kBytes[3]);
  CHECK(a == 0 && b == 1 && none == 2 && c == 3 && d == 4);
  CHECK(!st.dev(a) && !st.dev(d) && !buf.ptr && S.allocs == 0 && S.copies == 0);   // nothing before upload()
  CHECK(st.upload() == hipSuccess);
  CHECK(S.allocs == 1 && S.syncs == 0 && S.copies == 2);   // the two inputs; neither the absent operand nor the in-out
  CHECK(st.dev(none) == nullptr && st.dev(-1) == nullptr && st.dev(5) == nullptr);
  const int live[4] = {a, b, c, d};
  const unsigned char* base = buf.as<unsigned char>();
  size_t end = 0;
  for (int k = 0; k < 4; ++k) {
    const size_t off = (size_t)(st.as<unsigned char>(live[k]) - base);
    CHECK(off % 256 == 0 && off >= end);   // aligned, behind the slot before it
    CHECK(off == up256(end));              // ... and no further than that: the absent operand took no bytes
    end = off + kBytes[k];
  }
  CHECK(buf.cap == end && counter == end);   // the last slot ends with its last byte
  CHECK(!memcmp(st.dev(a), h[0].b, kBytes[0]) && !memcmp(st.dev(d), h[3].b, kBytes[3]));   // inputs intact
  // the "kernel" writes its outputs; the host arrays still hold what they held
  pattern(st.dev(b), kBytes[1], 7);
  pattern(st.dev(c), kBytes[2], 8);
  CHECK(h[1].holds(1) && h[2].holds(2));
  CHECK(st.download() == hipSuccess);
  CHECK(S.copies == 4 && S.syncs == 1);   // out and in-out, one drain
  CHECK(h[1].holds(7) && h[2].holds(8) && h[0].holds(0) && h[3].holds(3));
  for (int k = 0; k < 4; ++k) CHECK(h[k].guard_ok());   // exactly `bytes` each
  CHECK(!memcmp(st.dev(a), h[0].b, kBytes[0]) && !memcmp(st.dev(d), h[3].b, kBytes[3]));   // no slot reached into another
  return 0;
}

// an in-out operand with its upload on goes both ways
static int inout_uploaded() {
  S = DevBufSeam{};
  DevBuf buf;
  HostArray h;
  h.fill(240, 3);
  HostStage st(buf, nullptr);
  const int i = st.inout(h.b, 240);
  CHECK(st.upload() == hipSuccess && S.copies == 1 && !memcmp(st.dev(i), h.b, 240));
  pattern(st.dev(i), 240, 9);
  CHECK(st.download() == hipSuccess && S.copies == 2 && S.syncs == 1 && h.holds(9) && h.guard_ok());
  return 0;
}

// operands at addresses of the caller's: no bytes of the buffer, copies to and from there
static int caller_given_address() {
  S = DevBufSeam{};
  size_t counter = 0;
  DevBuf buf(&counter);
  HostArray hin, hout, hcell, dev_in, dev_out;
  hin.fill(960, 1);
  hout.fill(960, 2);
  hcell.fill(257, 3);
  dev_in.fill(960, 4);
  dev_out.fill(960, 5);
  HostStage st(buf, nullptr);
  const int i = st.in(hin.b, 960, dev_in.b), c = st.in(hcell.b, 257), o = st.out(hout.b, 960, dev_out.b);
  const int none = st.in(nullptr, 960, dev_in.b);   // absent wins over the address
  CHECK(st.upload() == hipSuccess && S.copies == 2);
  CHECK(st.dev(i) == dev_in.b && st.dev(o) == dev_out.b && st.dev(c) == buf.ptr && st.dev(none) == nullptr);
  CHECK(buf.cap == 257 && counter == 257);
  CHECK(dev_in.holds(1) && dev_in.guard_ok() && dev_out.holds(5) && !memcmp(st.dev(c), hcell.b, 257));
  pattern(dev_out.b, 960, 6);
  CHECK(st.download() == hipSuccess && S.copies == 3 && S.syncs == 1);
  CHECK(hout.holds(6) && hout.guard_ok() && hin.holds(1) && hcell.holds(3));
  return 0;
}

// one buffer under several calls: a call that fits allocates nothing, a larger one allocates once and drains before it frees
static int reuse_and_growth() {
  S = DevBufSeam{};
  size_t counter = 0;
  DevBuf buf(&counter);
  HostArray h[3];
  h[0].fill(960, 0);
  h[1].fill(240, 1);
  h[2].fill(1000, 2);
  {
    HostStage st(buf, nullptr);
    st.in(h[0].b, 960);
    st.out(h[1].b, 240);
    CHECK(st.upload() == hipSuccess && st.download() == hipSuccess);
  }
  CHECK(S.allocs == 1 && S.frees == 0 && S.syncs == 1 && buf.cap == 1024 + 240);
  void* const p0 = buf.ptr;
  {
    HostStage st(buf, nullptr);   // smaller: nothing moves
    const int i = st.in(h[1].b, 240);
    CHECK(st.upload() == hipSuccess && st.dev(i) == p0 && st.download() == hipSuccess);
  }
  CHECK(S.allocs == 1 && S.frees == 0 && S.syncs == 2 && buf.cap == 1024 + 240 && counter == buf.cap);
  {
    HostStage st(buf, nullptr);   // larger
    st.in(h[0].b, 960);
    st.in(h[2].b, 1000);
    const long s0 = S.syncs;
    CHECK(st.upload() == hipSuccess);
    CHECK(S.allocs == 2 && S.frees == 1 && S.syncs == s0 + 1 && buf.cap == 1024 + 1000 && counter == buf.cap);
    CHECK(st.download() == hipSuccess && S.syncs == s0 + 2);
  }
  return 0;
}

// a failed allocation: the error comes back, nothing was copied, the buffer is empty and no device pointer exists
static int failed_reserve() {
  S = DevBufSeam{};
  size_t counter = 0;
  DevBuf buf(&counter);
  HostArray h;
  h.fill(960, 0);
  {
    HostStage st(buf, nullptr);
    st.in(h.b, 100);
    CHECK(st.upload() == hipSuccess && S.copies == 1);
  }
  S.fail_at = 1;
  HostStage st(buf, nullptr);
  const int i = st.in(h.b, 960), o = st.out(h.b, 960);
  CHECK(st.upload() == hipErrorOutOfMemory);
  CHECK(S.copies == 1 && !buf.ptr && buf.cap == 0 && counter == 0 && !st.dev(i) && !st.dev(o));
  CHECK(S.syncs == 1 && S.frees == 1);   // the live buffer was drained and freed before the allocation failed
  return 0;
}

// the ninth operand is refused, and so is the upload; nothing is written behind the eight
static int operand_bound() {
  S = DevBufSeam{};
  DevBuf buf;
  HostArray h;
  h.fill(16, 0);
  struct { unsigned char before[64]; HostStage st; unsigned char after[64]; } box = {{0}, HostStage(buf, nullptr), {0}};
  memset(box.before, GUARD_BYTE, 64);
  memset(box.after, GUARD_BYTE, 64);
  for (int k = 0; k < HostStage::MAX_OPERANDS; ++k) CHECK(box.st.in(h.b, 16) == k);
  CHECK(box.st.in(h.b, 16) == -1 && box.st.out(h.b, 16) == -1 && box.st.inout(h.b, 16) == -1);
  for (int k = 0; k < 64; ++k) CHECK(box.before[k] == GUARD_BYTE && box.after[k] == GUARD_BYTE);
  CHECK(box.st.upload() == hipErrorInvalidValue && S.allocs == 0 && S.copies == 0 && !buf.ptr);
  CHECK(box.st.dev(0) == nullptr && box.st.dev(HostStage::MAX_OPERANDS) == nullptr);
  return 0;
}

// a smaller alignment packs the slots: two cells of doubles back to back
static int packed() {
  S = DevBufSeam{};
  DevBuf buf;
  HostArray r, w;
  r.fill(15 * 8, 0);
  w.fill(15 * 8, 1);
  HostStage st(buf, nullptr, sizeof(double));
  const int i = st.out(r.b, 15 * 8), j = st.out(w.b, 15 * 8);
  CHECK(st.upload() == hipSuccess && S.copies == 0);
  CHECK(st.as<unsigned char>(j) == st.as<unsigned char>(i) + 15 * 8 && buf.cap == 2 * 15 * 8);
  pattern(st.dev(i), 15 * 8, 4);
  pattern(st.dev(j), 15 * 8, 5);
  CHECK(st.download() == hipSuccess && r.holds(4) && w.holds(5) && r.guard_ok() && w.guard_ok());
  return 0;
}

int main() {
  if (layout_and_copies() || inout_uploaded() || caller_given_address() || reuse_and_growth() || failed_reserve() ||
      operand_bound() || packed())
    return 1;
  CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
  printf("OK %ld\n", g_checks);
  return 0;
}
