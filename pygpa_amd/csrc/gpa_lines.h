// Per-line medians and homogenize_per_axis (pyGPA/imagetools.py:112-125): everything integer or host-computable that the
// kernels of gpa_lines.hip and the entry points of gpa_api_lines.hip share.  No HIP code: tests/host/lines_check.cpp includes
// it with a host compiler.
//
// A median is a selection.  The samples of a line become unsigned keys whose integer order is the order of the values, the
// keys sit in LDS, and a radix selection (most significant byte first, 8 bits per pass) finds the key of rank (m - 1) / 2
// among the m valid ones; rank m / 2 follows from it (lines_upper_is_same).  np.nanmedian is v[m / 2] for odd m and
// (v[m / 2 - 1] + v[m / 2]) / 2 for even m -- one rounded addition and an exact halving -- so the result has NumPy's bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LINES_HD __host__ __device__ inline
#else
#define LINES_HD inline
#endif

namespace gpa {

// Longest line: its keys must fit the LDS one workgroup may declare (160 KiB): 16384 f64 keys are 128 KiB.
constexpr int LINES_MAX_N = 16384;
// threads of the selection kernel, and its waves (64 lanes): one private 256-bin histogram per wave
constexpr int LINES_THREADS = 256;
constexpr int LINES_WAVES = LINES_THREADS / 64;
// samples of a thread that are in flight together in the loops over a line
constexpr int LINES_BATCH = 4;
// frames of one call: the frame index is a grid dimension of every kernel
constexpr int LINES_MAX_FRAMES = 65535;
// largest radius of the profile filter: R = int(4 sigma + 0.5) with sigma <= 16384; indices i + k stay far below 2^30
constexpr double LINES_MAX_SIGMA = 16384.0;
// edge of the square LDS tile of the transpose, and its padded row
constexpr int LINES_TILE = 32;
constexpr int LINES_TILE_PITCH = LINES_TILE + 1;

// ---- keys ------------------------------------------------------------------------------------------------------------------
// A NaN is no sample: it gets the largest key, which no number has (all ones is the key of the bit pattern 0x7ff..f, itself
// a NaN), and is counted apart, so the ranks of the valid samples are their ranks among all keys of the line.
constexpr uint32_t LINES_NAN_KEY32 = 0xffffffffu;
constexpr uint64_t LINES_NAN_KEY64 = 0xffffffffffffffffull;

LINES_HD bool lines_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
LINES_HD bool lines_is_nan(uint64_t bits) { return (bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }

// IEEE bits -> key: negative numbers have all bits flipped (larger magnitude, smaller key), the others the sign bit set.
// -inf < ... < -subnormal < -0 < +0 < +subnormal < ... < +inf; -0 and +0 get neighbouring keys (their order does not
// matter to a median: they compare equal, and (-0 + +0) / 2 = +0 as in NumPy).
LINES_HD uint32_t lines_key(uint32_t bits) {
  if (lines_is_nan(bits)) return LINES_NAN_KEY32;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
LINES_HD uint64_t lines_key(uint64_t bits) {
  if (lines_is_nan(bits)) return LINES_NAN_KEY64;
  return (bits & 0x8000000000000000ull) ? ~bits : (bits | 0x8000000000000000ull);
}
// key -> IEEE bits; the NaN key gives a quiet NaN pattern (all ones without the sign would do as well: 0x7ff..f)
LINES_HD uint32_t lines_unkey(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }
LINES_HD uint64_t lines_unkey(uint64_t key) { return (key & 0x8000000000000000ull) ? (key & 0x7fffffffffffffffull) : ~key; }

// ---- ranks -----------------------------------------------------------------------------------------------------------------
// of m >= 1 valid samples sorted as v[0 .. m): the median is v[lo] (m odd, lo == hi) or (v[lo] + v[hi]) / 2
LINES_HD int lines_rank_lo(int m) { return (m - 1) / 2; }
LINES_HD int lines_rank_hi(int m) { return m / 2; }
// count_le = number of keys <= v[lo].  v[hi] is the same key when more than hi keys are <= it, else the smallest key above.
LINES_HD bool lines_upper_is_same(int count_le, int m) { return count_le > lines_rank_hi(m); }

// ---- LDS and route -----------------------------------------------------------------------------------------------------------
// dynamic LDS of one line of n samples with keys of key_bytes (4: f32, 8: f64), a multiple of 16 bytes: a short line takes
// what it needs, so several workgroups share a CU.  The histograms and the few words of the selection are static LDS.
LINES_HD size_t lines_lds_bytes(int n, int key_bytes) { return ((size_t)n * (size_t)key_bytes + 15) & ~(size_t)15; }
constexpr size_t LINES_STATIC_LDS = (size_t)LINES_WAVES * 256 * 4 + 64;
constexpr size_t LINES_LDS_LIMIT = 160 * 1024;
// dynamic LDS a kernel may take without having its limit raised; lines beyond it (f64 above 8192 samples) run the kernel's
// second instantiation, whose limit is raised once (lines_long_route)
constexpr size_t LINES_PLAIN_LDS = 64 * 1024;
LINES_HD bool lines_long_route(int n, int key_bytes) { return lines_lds_bytes(n, key_bytes) > LINES_PLAIN_LDS; }
// whether a line of n samples is served
LINES_HD bool lines_length_ok(int n) { return n >= 1 && n <= LINES_MAX_N; }
// rounds of the loops over a line: LINES_BATCH samples per thread and round
LINES_HD int lines_rounds(int n) { return (n + LINES_BATCH * LINES_THREADS - 1) / (LINES_BATCH * LINES_THREADS); }

// ---- the fold ----------------------------------------------------------------------------------------------------------------
// index i folded into [0, n) under scipy.ndimage's 'reflect' rule (d c b a | a b c d | d c b a, period 2 n); any i with
// |i| < 2^30, so the radius may exceed the line many times over (the default sigma = 200 gives R = 800)
LINES_HD int lines_fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}
LINES_HD int lines_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

// ---- transpose tiles ---------------------------------------------------------------------------------------------------------
LINES_HD int lines_tiles(int n) { return (n + LINES_TILE - 1) / LINES_TILE; }
// samples of tile t along an axis of n samples (the last one may be ragged)
LINES_HD int lines_tile_extent(int t, int n) {
  const int left = n - t * LINES_TILE;
  return left < 0 ? 0 : (left < LINES_TILE ? left : LINES_TILE);
}

}  // namespace gpa
