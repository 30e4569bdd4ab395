// The arithmetic of a stack of weighted unwraps solved as ONE set of launches (gpa_unwrap_batch_dev): how many problems a
// byte budget holds, and which weight plane a problem reads.  The kernels that read a weight (setup_kernel, pq_kernel,
// pq_small_kernel, rowidct_pq_kernel, pqdct_kernel) and the entry points (gpa_api_unwrap.hip) call these very functions.
// Plain C++17: no HIP header, no globals -- tests/host/unwrap_batch_check.cpp compiles it with g++ and
// tests/test_unwrap_stack_host.py runs the result.
#pragma once
#include <stddef.h>

#ifndef GPA_UNWRAP_BATCH_MAX
#define GPA_UNWRAP_BATCH_MAX 4096   // problems of one gpa_unwrap_batch[_dev] call (include/gpa_hip.h states the same)
#endif

namespace gpa {

// image-sized arrays every problem of a workspace owns whatever its solve keeps: r, p, p2, q, z (Impl; p and p2 are the
// first two search directions of the ring)
constexpr int UNWRAP_WS_PLANES = 5;
constexpr int UNWRAP_RING_MAX = 10;   // = RING_MAX (gpa_unwrap_impl.h)

// search directions a solve of kmax iterations keeps so that phi is written once per `ring` iterations (run_pcg)
constexpr int unwrap_ring_for(int kmax) { return kmax < 2 ? 2 : (kmax < UNWRAP_RING_MAX ? kmax : UNWRAP_RING_MAX); }

// device bytes of ONE problem: its image-sized arrays, the ring included, and `fixed` bytes of scalars, flags, partial
// sums and per-problem column-solve scratch
constexpr size_t unwrap_problem_bytes(size_t npx, size_t rsz, int ring, size_t fixed) {
  return (size_t)(UNWRAP_WS_PLANES + (ring > 2 ? ring - 2 : 0)) * npx * rsz + fixed;
}

// problems of one set of launches: as many as fit `budget` bytes, at least 1 (a single problem above the budget still
// runs), at most GPA_UNWRAP_BATCH_MAX
constexpr int unwrap_batch_chunk(size_t npx, size_t rsz, int ring, size_t fixed, size_t budget) {
  const size_t per = unwrap_problem_bytes(npx, rsz, ring, fixed);
  const size_t n = per ? budget / per : (size_t)GPA_UNWRAP_BATCH_MAX;
  return n < 1 ? 1 : (n > (size_t)GPA_UNWRAP_BATCH_MAX ? GPA_UNWRAP_BATCH_MAX : (int)n);
}

// Offset, in samples, of the weight plane problem pb reads:
//   wshift = 1, wstride = npx   problems 2i and 2i + 1 share the weight of image i (the two displacement components of
//                               the batched driver)
//   wshift = 0, wstride = npx   one weight per problem
//   wstride = 0                 one weight for all problems
// 64-bit throughout: pb * npx passes 2^32 from 16 problems of 16384^2 on.
constexpr size_t unwrap_weight_offset(size_t pb, int wshift, size_t wstride) { return (pb >> wshift) * wstride; }

}  // namespace gpa
