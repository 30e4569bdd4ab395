// DevBuf (pygpa_amd/csrc/gpa_devbuf.h) on the CPU: the header's allocate / free / drain primitives are malloc / free / a
// counter here, and the n-th allocation can be made to fail.  Prints "OK <checks>" and exits 0, or the failed check and exits 1.
//   g++ -std=c++17 -DGPA_DEVBUF_HOST_SEAM -I pygpa_amd/csrc tests/host/devbuf_check.cpp
#include <stdio.h>

#include <utility>
#include <vector>

#include "gpa_devbuf.h"

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

static size_t live_bytes(const std::vector<DevBuf>& b) {
  size_t s = 0;
  for (const DevBuf& x : b) s += x.ptr ? x.cap : 0;
  return s;
}
static long live_count(const std::vector<DevBuf>& b) {
  long n = 0;
  for (const DevBuf& x : b) n += x.ptr != nullptr;
  return n;
}

// about ten mixed reserves on three buffers that share one counter: (buffer, bytes); some grow, some fit, one asks for 0
static const struct { int buf; size_t bytes; } kSeq[] = {{0, 100}, {1, 40}, {0, 50},  {2, 0},   {0, 300}, {1, 40},
                                                         {1, 41},  {2, 16}, {2, 500}, {0, 299}, {1, 1000}};
static const int kSeqLen = (int)(sizeof(kSeq) / sizeof(kSeq[0]));

// the sequence with the fail_n-th allocation failing (0: none does)
static int run_sequence(int fail_n, int* allocations_tried) {
  S = DevBufSeam{};
  S.fail_at = fail_n;
  size_t counter = 0;
  int tried = 0;
  bool failed = false;
  {
    std::vector<DevBuf> b;
    for (int i = 0; i < 3; ++i) b.emplace_back(&counter);
    for (int i = 0; i < kSeqLen; ++i) {
      DevBuf& x = b[kSeq[i].buf];
      const size_t want = kSeq[i].bytes ? kSeq[i].bytes : 16;
      const bool fits = x.ptr && x.cap >= want, was_live = x.ptr != nullptr;
      const long a0 = S.allocs, s0 = S.syncs, f0 = S.frees;
      const size_t cap0 = x.cap, counter0 = counter;
      void* const p0 = x.ptr;
      tried += !fits;
      const bool fails_now = !fits && fail_n > 0 && tried == fail_n;
      const hipError_t e = x.reserve(kSeq[i].bytes, nullptr);
      if (fits) {   // sufficient capacity: neither allocates nor drains, nothing moves
        CHECK(e == hipSuccess && S.allocs == a0 && S.syncs == s0 && S.frees == f0 && x.ptr == p0 && x.cap == cap0);
      } else {
        CHECK(S.syncs == s0 + (was_live ? 1 : 0));   // one drain when a buffer was live, none from empty
        CHECK(S.frees == f0 + (was_live ? 1 : 0));
        if (fails_now) {
          failed = true;
          CHECK(e != hipSuccess && x.ptr == nullptr && x.cap == 0 && S.allocs == a0);
          CHECK(counter == counter0 - cap0);         // reduced by exactly the old capacity
        } else {
          CHECK(e == hipSuccess && x.ptr != nullptr && x.cap == want && S.allocs == a0 + 1);
        }
      }
      CHECK(counter == live_bytes(b));
      CHECK(S.frees + live_count(b) == S.allocs);
    }
    CHECK(failed == (fail_n > 0 && fail_n <= tried));
    // a later successful reserve recovers every buffer, the failed one included
    for (DevBuf& x : b) {
      CHECK(x.reserve(2000, nullptr) == hipSuccess && x.ptr && x.cap == 2000);
      static_cast<char*>(x.ptr)[1999] = 1;   // (the memory is there: the sanitizer build checks the bounds)
    }
    CHECK(counter == 3 * 2000 && S.frees + 3 == S.allocs);
  }
  CHECK(counter == 0 && S.frees == S.allocs);   // destruction frees and reports
  if (allocations_tried) *allocations_tried = tried;
  return 0;
}

static int lifetime() {
  S = DevBufSeam{};
  size_t counter = 0;
  {
    DevBuf a(&counter);
    CHECK(a.reserve(64, nullptr) == hipSuccess && counter == 64);
    a.release();
    CHECK(!a.ptr && a.cap == 0 && counter == 0 && S.frees == 1);
    a.release();   // twice is harmless
    CHECK(counter == 0 && S.frees == 1);
    CHECK(a.reserve(0, nullptr) == hipSuccess && a.cap == 16 && counter == 16);   // 0 bytes: the 16 of dmalloc
    DevBuf b(std::move(a));
    CHECK(!a.ptr && a.cap == 0 && b.ptr && b.cap == 16 && b.counted == &counter && counter == 16);
    DevBuf c(&counter);
    CHECK(c.reserve(32, nullptr) == hipSuccess && counter == 48);
    c = std::move(b);   // frees c's own 32 bytes, takes b's
    CHECK(!b.ptr && c.cap == 16 && counter == 16 && S.frees == 2);
    DevBuf pinned(nullptr, true), temp;   // uncounted ones
    CHECK(pinned.reserve(8, nullptr) == hipSuccess && temp.reserve(8, nullptr) == hipSuccess && counter == 16);
  }
  // a, b (moved from) freed nothing; c, pinned, temp one each
  CHECK(counter == 0 && S.allocs == 5 && S.frees == 5 && S.syncs == 0);
  return 0;
}

int main() {
  int tried = 0;
  if (run_sequence(0, &tried)) return 1;
  if (tried < 6) { printf("FAILED: the sequence allocates only %d times\n", tried); return 1; }
  for (int n = 1; n <= tried; ++n)
    if (run_sequence(n, nullptr)) return 1;
  if (lifetime()) return 1;
  printf("OK %ld\n", g_checks);
  return 0;
}
