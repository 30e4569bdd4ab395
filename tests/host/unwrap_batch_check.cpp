// Host check of pygpa_amd/csrc/gpa_unwrap_batch.h: the chunk size of a stack of unwraps under a byte budget and the
// weight plane a problem reads.  Prints "OK <checks>" and returns 0, or names the first failures and returns 1.
//   g++ -O2 -std=c++17 -I pygpa_amd/csrc tests/host/unwrap_batch_check.cpp -o unwrap_batch_check
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "gpa_unwrap_batch.h"

using namespace gpa;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++checks;                                                              \
    if (!(cond)) {                                                         \
      if (++failures <= 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                                      \
  } while (0)

int main() {
  static_assert(sizeof(size_t) == 8, "the offsets are 64-bit");
  // ---- ring ----
  CHECK(unwrap_ring_for(1) == 2);
  CHECK(unwrap_ring_for(2) == 2);
  CHECK(unwrap_ring_for(7) == 7);
  CHECK(unwrap_ring_for(10) == 10);
  CHECK(unwrap_ring_for(100) == 10);

  // ---- bytes of a problem: 5 arrays, ring - 2 further search directions, the fixed part ----
  const size_t npx = (size_t)64 * 64, fixed = 1572864 + 256;
  CHECK(unwrap_problem_bytes(npx, 4, 2, 0) == 5 * npx * 4);
  CHECK(unwrap_problem_bytes(npx, 8, 10, 0) == 13 * npx * 8);
  CHECK(unwrap_problem_bytes(npx, 8, 10, fixed) == 13 * npx * 8 + fixed);
  CHECK(unwrap_problem_bytes(npx, 4, 1, 0) == 5 * npx * 4);   // (never fewer than the two directions the workspace owns)

  // ---- budget edges ----
  for (size_t rsz : {(size_t)4, (size_t)8})
    for (int ring : {2, 3, 10}) {
      const size_t per = unwrap_problem_bytes(npx, rsz, ring, fixed);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 0) == 1);            // nothing fits: one problem still runs
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, per - 1) == 1);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, per) == 1);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 2 * per - 1) == 1);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 2 * per) == 2);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 2 * per + per / 2) == 2);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 3 * per - 1) == 2);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, 3 * per) == 3);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, (size_t)GPA_UNWRAP_BATCH_MAX * per - 1) == GPA_UNWRAP_BATCH_MAX - 1);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, (size_t)GPA_UNWRAP_BATCH_MAX * per) == GPA_UNWRAP_BATCH_MAX);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, (size_t)(GPA_UNWRAP_BATCH_MAX + 1) * per) == GPA_UNWRAP_BATCH_MAX);
      CHECK(unwrap_batch_chunk(npx, rsz, ring, fixed, ~(size_t)0) == GPA_UNWRAP_BATCH_MAX);
    }
  // the default budget of 2 GiB: 12 frames of 512^2 in one chunk, 2048^2 f32 at ring 10 nine at a time, 16384^2 alone
  const size_t GiB2 = (size_t)2 << 30;
  CHECK(unwrap_batch_chunk((size_t)512 * 512, 4, 10, fixed, GiB2) >= 12);
  CHECK(unwrap_batch_chunk((size_t)2048 * 2048, 4, 10, 0, GiB2) == 9);
  CHECK(unwrap_batch_chunk((size_t)16384 * 16384, 8, 10, fixed, GiB2) == 1);
  CHECK(unwrap_batch_chunk(0, 4, 2, 0, GiB2) == GPA_UNWRAP_BATCH_MAX);   // (no bytes per problem: no division by zero)

  // ---- a ragged last chunk: the loop of the entry point over nb = 5 with a budget of two and a half problems ----
  {
    const size_t per = unwrap_problem_bytes(npx, 8, 10, fixed);
    const int nb = 5, chunk = unwrap_batch_chunk(npx, 8, 10, fixed, 2 * per + per / 2);
    int sizes[8], n = 0, covered = 0;
    for (int c0 = 0; c0 < nb; c0 += chunk) {
      const int m = nb - c0 < chunk ? nb - c0 : chunk;
      sizes[n++] = m;
      covered += m;
    }
    CHECK(chunk == 2 && n == 3 && sizes[0] == 2 && sizes[1] == 2 && sizes[2] == 1 && covered == nb);
  }

  // ---- the three weight modes ----
  const size_t big = (size_t)16384 * 16384;   // 2^28 samples
  for (size_t pb = 0; pb < 64; ++pb) {
    CHECK(unwrap_weight_offset(pb, 1, npx) == (pb / 2) * npx);   // driver: 2i and 2i + 1 read the weight of image i
    CHECK(unwrap_weight_offset(pb, 0, npx) == pb * npx);         // own weights
    CHECK(unwrap_weight_offset(pb, 0, 0) == 0);                  // one weight for all
    CHECK(unwrap_weight_offset(pb, 1, 0) == 0);
  }
  CHECK(unwrap_weight_offset(1, 1, npx) == 0 && unwrap_weight_offset(2, 1, npx) == npx && unwrap_weight_offset(3, 1, npx) == npx);
  // own weights differ from the driver's map for every problem but the first: what a left-over `pb >> 1` would read
  for (size_t pb = 1; pb < 64; ++pb) CHECK(unwrap_weight_offset(pb, 0, npx) != unwrap_weight_offset(pb, 1, npx));

  // ---- 64-bit offsets: pb * npx >= 2^32 ----
  CHECK(unwrap_weight_offset(16, 0, big) == ((uint64_t)1 << 32));
  CHECK(unwrap_weight_offset(17, 0, big) == ((uint64_t)17 << 28));
  CHECK(unwrap_weight_offset(GPA_UNWRAP_BATCH_MAX - 1, 0, big) == (uint64_t)(GPA_UNWRAP_BATCH_MAX - 1) * big);
  CHECK(unwrap_weight_offset(GPA_UNWRAP_BATCH_MAX - 1, 0, big) > ((uint64_t)1 << 39));
  CHECK(unwrap_weight_offset(33, 1, big) == ((uint64_t)1 << 32));
  CHECK(unwrap_weight_offset(GPA_UNWRAP_BATCH_MAX - 1, 1, big) == (uint64_t)2047 * big);
  CHECK(unwrap_problem_bytes(big, 8, 10, 0) == (uint64_t)13 * 8 * big);   // 26 GiB: no 32-bit product on the way

  if (failures) {
    printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  printf("OK %d\n", checks);
  return 0;
}
