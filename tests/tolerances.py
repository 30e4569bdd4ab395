"""The stated tolerances of the displacement-field driver (README.md "Tolerances" quotes this file; the full-size
GPU tests of tests/test_gpu_configs.py assert exactly these numbers).

Reference: extract_displacement_field, geometric_phase_analysis.py:907-932, computes in complex128 / float64.
Errors are in PIXELS of displacement, after removing the free mean of each component (phase_unwrap.py:110-114),
on fields with |u| up to ~155 px (BASELINE configs[2]) -- i.e. max 0.02 px is 1.3e-4 relative.

f64 build vs the oracle (the reference's arithmetic):   index work bit-exact, u to rounding.
f32 build (BASELINE configs[1-2] name fp32) vs the f64 build and vs the oracle, with the reference's stopping test
(the library default; 10 + 10 PCG iterations at configs[2]):
    rms  |du| <= 1e-5 px      (measured 3.3e-6 at 4096^2, 2.7e-6 at 2048^2)
    max  |du| <= 0.02 px      (measured 0.009 at 4096^2 and 0.0044 at 2048^2: ONE winner flip at an amplitude tie each)
    kidx may differ from the f64 / oracle winner at <= 2.5e-7 of the pixels (measured: ONE pixel of 16.8 M at 4096^2 =
    6e-8, one of 4.2 M at 2048^2 = 2.4e-7), and only where the two candidates' amplitudes tie to <= 4e-6 of the largest
    amplitude (conftest.kidx_mismatch_is_tie).
Per-configuration bounds below are <= 2 x what was measured on MI355X (profiles/r02_accuracy.json, re-measured by
every run of the tests into gpurun_out/r02_accuracy.json; round 5's copy: profiles/r05_accuracy.json)."""

F64 = dict(max_px=2e-11, kidx_frac=0.0, tie_rel=1e-12)        # measured 6.8e-12 px (4096^2), 4.4e-12 (2048^2)
F32 = dict(rms_px=1e-5, max_px=0.02, kidx_frac=2.5e-7, tie_rel=4e-6, lockin_rel=1.6e-6)   # lockin_rel measured 7.9e-7
F32_C2 = dict(rms_px=5.5e-6, max_px=0.0089)                   # configs[1], 2048^2 3 x 8: measured 2.74e-6 / 0.00443
F32_C3 = dict(rms_px=6.6e-6, max_px=0.0181)                   # configs[2], 4096^2 3 x 16: measured 3.28e-6 / 0.00904
# configs[0], 512^2, one reference k-vector per peak (iterate_GPA route and a K = 1 driver call), against the
# reference's own outputs (tests/golden/config1_512.npz); |u| up to 19 px, phases up to ~20 rad
C1_F64 = dict(corr=1e-12, prs=1e-8, u=1e-9)
C1_F32 = dict(corr=2e-7, prs_rel=2e-5, u_px=2e-3, lockin_rel=2e-6)
# configs[3]'s image (8192^2, 3 x 16, |u| up to 310 px) through the WHOLE-IMAGE driver against the oracle at full size
# (round 6, tests/test_gpu_pins.py): measured rms 8.7e-6 px, max 0.0041 px, 2 winner flips in 67 M pixels (3e-8)
F32_C4 = dict(rms_px=1.8e-5, max_px=0.0083, kidx_frac=2.5e-7)
# Lawler-Fujita at the benchmark's displacement (4096^2, |u| up to 155 px) against the oracle: u_inv in px, the undistorted
# image relative to its maximum; measured f64 2.7e-13 / 2.4e-13, f32 1.2e-4 / 8.8e-5
LF_4096 = {'float64': dict(u_inv_px=1e-9, rec_rel=1e-9), 'float32': dict(u_inv_px=2.5e-4, rec_rel=1.8e-4)}
# ... and at 16384^2 with |u| up to 621 px in f32 against the equation that defines the inverse: sample coordinates up to
# 16384 carry an f32 ulp of 9.8e-4 px; measured residual 7.6e-4 px, reconstruction within 0.014 of a lattice of amplitude 3
LF_16384_F32 = dict(residual_px=2e-3, rec_abs=0.03)

# The weighted unwrap mode by mode (tests/test_gpu_unwrap_modes.py; the measure: tests/unwrap_modes.py).  Per case and check
# (U: one unweighted iteration, an exact Poisson solve; W2 / W3: weighted, kmax 2 / 3):
#     (spectral residual of the emulation in the case's precision, ratio device / emulation measured on MI355X, asserted ratio)
# The asserted ratio is 2 x the measured one (results are deterministic: the margin covers a change of compiler or of the FMA
# contraction), and never above UNWRAP_MODES_CAP: at 16 floors every planted fault of tests/test_unwrap_modes_host.py still
# reads.  A case that needs more is a finding, not a number to widen.  Measured: f32 0.21 .. 3.5 (median 1.06), f64 0.27 .. 5.9
# (median 1.45); the largest asserted ratio is 11.84 (f64 64 x 2048, W3).
#
# What these tests found, and what became of it (the numbers are those of the first measurement, before the fix).  The
# TRANSFORM-BASED COLUMN SOLVE of a packed pair of columns (colsolve_kernel, its mixed-radix form, g_colsolve_kernel) read
#     f64 columns of    63 (63 x 65: mixed radix, plain scheme, psi entry)   U 47 .. 48    W2 78 .. 80
#                      256 (256^2, COLSOLVE=fft)                             U 65          W2 90       W3 18
#                     1024 (1024 x 64; 1024 x 16 on the mixed-radix engine)  U 3100 / 2400 W2 560 / 210 W3 220 / 400
#                     8192 (8192 x 64)                                       U 60000       W2 6600     W3 3500
#     f32 columns of 16384 (16384 x 64)                                      U 62
#   i.e. (0.2 .. 3) x eps / |smallest eigenvalue of the column axis| = eps x O(n0^2), and 12 .. 15 floors on every f64 case with
#   64-point transform-solved columns, where the transform-free and streamed solves and the half-length column kernel read
#   0.4 .. 4 floors on the same shapes.  The pixel tests could not see it: 2.5e-10 of the right-hand side at 8192 points,
#   under their 1e-8.
#   Cause: the fused solve forms the coefficient of a low bin k twice -- as Re(w_k V_k) in the thread of bin k and as
#   -Im(w_(N-k) V_(N-k)) in the thread of bin N - k, each by cancellation from the packed spectrum -- and scales both by
#   1 / eigenvalue_k.  The two roundings differed (w_(N-k) of the f64 table was not -i conj(w_k) to the last bit, and cmul's
#   contraction was the compiler's choice), and the inverse transform of a packed pair turns their difference, already
#   multiplied by up to n0^2, into bin N - k of the PARTNER column, where the eigenvalue is O(4): on the device the largest
#   error coefficient was bin (n0 - 1, 1) -- (255, 1) at 256^2, (1022, 1) at 1024 x 64, (62, 1) at 63 x 65 -- ten times the
#   next.  A NumPy model of the formulas (tools/dbg/colsolve_pair_model.py) reads the same 66 and 2990 floors, and 1 floor with
#   every coefficient evaluated once.
#   Fix: dct_split_mul (gpa_dct.h) writes the two coefficients out as one rounded product and one fma each, the same
#   operations in either thread, and dct_mirror_exact_w (gpa_unwrap_tables.hip) builds the w tables of the column solves with
#   w_(N-k) = (s_k, -c_k) to the bit.  After it: f64 8192 x 64 U 0.76, 1024 x 64 U 0.82, 256^2 fft U 1.07, f32 16384 x 64 U 0.68.
UNWRAP_MODES_CAP = 16.0
UNWRAP_MODES = {
    'f32-64x64': {'U': (1.35e-06, 0.675, 1.35), 'W2': (2.15e-06, 1.53, 3.06), 'W3': (2.33e-06, 1.48, 2.96)},
    'f64-64x64': {'U': (2.28e-15, 0.897, 1.794), 'W2': (4.49e-15, 1.01, 2.02), 'W3': (3.15e-15, 1.75, 3.5)},
    'f32-64x512': {'U': (1.52e-06, 1.05, 2.1), 'W2': (4.02e-06, 1.02, 2.04), 'W3': (3.95e-06, 1.19, 2.38)},
    'f64-64x512': {'U': (3.52e-15, 0.717, 1.434), 'W2': (6.91e-15, 3.16, 6.32), 'W3': (9.12e-15, 2.39, 4.78)},
    'f32-1024x64': {'U': (1.79e-06, 0.8, 1.6), 'W2': (9.90e-06, 3.18, 6.36), 'W3': (1.46e-05, 0.531, 1.062)},
    'f64-1024x64': {'U': (3.14e-15, 0.824, 1.648), 'W2': (4.04e-14, 1.15, 2.3), 'W3': (2.16e-14, 1.82, 3.64)},
    'f32-64x64-NO_LAT=1': {'U': (1.35e-06, 0.675, 1.35), 'W2': (2.15e-06, 1.53, 3.06), 'W3': (2.33e-06, 1.48, 2.96)},
    'f64-64x64-NO_LAT=1': {'U': (2.28e-15, 0.897, 1.794), 'W2': (4.49e-15, 1.15, 2.3), 'W3': (3.15e-15, 1.8, 3.6)},
    'f32-64x64-stack': {'U': (1.35e-06, 0.84, 1.68), 'W2': (2.87e-06, 1.27, 2.54), 'W3': (3.05e-06, 1.13, 2.26)},
    'f64-64x64-stack': {'U': (3.87e-15, 0.583, 1.166), 'W2': (4.97e-15, 1.03, 2.06), 'W3': (4.29e-15, 1.45, 2.9)},
    'f32-64x1024': {'U': (1.88e-06, 1.12, 2.24), 'W2': (8.20e-06, 1.24, 2.48), 'W3': (4.80e-06, 1.14, 2.28)},
    'f64-64x1024': {'U': (4.71e-15, 0.651, 1.302), 'W2': (1.15e-14, 2.23, 4.46), 'W3': (6.55e-15, 3.08, 6.16)},
    'f32-64x2048': {'U': (1.80e-06, 0.736, 1.472), 'W2': (2.20e-05, 1.51, 3.02), 'W3': (1.37e-05, 1.34, 2.68)},
    'f64-64x2048': {'U': (4.55e-15, 0.701, 1.402), 'W2': (4.47e-14, 1.36, 2.72), 'W3': (3.68e-14, 5.92, 11.84)},
    'f32-64x4096': {'U': (1.97e-06, 0.974, 1.948), 'W2': (1.54e-05, 1.33, 2.66), 'W3': (1.09e-05, 1.55, 3.1)},
    'f32-64x4096-NO_ROWPERS=1': {'U': (1.97e-06, 0.974, 1.948), 'W2': (1.54e-05, 1.33, 2.66), 'W3': (1.09e-05, 1.55, 3.1)},
    'f64-64x4096': {'U': (4.09e-15, 1.11, 2.22), 'W2': (3.03e-14, 5.14, 10.28), 'W3': (1.98e-14, 4.85, 9.7)},
    'f32-64x8192': {'U': (2.49e-06, 0.918, 1.836), 'W2': (2.37e-05, 1.39, 2.78), 'W3': (5.15e-05, 0.864, 1.728)},
    'f32-64x8192-NO_ROWPERS=1': {'U': (2.49e-06, 0.918, 1.836), 'W2': (2.37e-05, 1.39, 2.78), 'W3': (5.15e-05, 0.864, 1.728)},
    'f64-64x8192': {'U': (4.46e-15, 1.05, 2.1), 'W2': (5.97e-14, 2, 4), 'W3': (7.19e-14, 4.16, 8.32)},
    'f32-64x16384': {'U': (4.07e-06, 0.463, 0.926), 'W2': (4.71e-05, 0.974, 1.948), 'W3': (1.09e-04, 1.02, 2.04)},
    'f32-64x16384-NO_ROWPERS=1': {'U': (4.07e-06, 0.463, 0.926), 'W2': (4.71e-05, 0.974, 1.948), 'W3': (1.09e-04, 1.02, 2.04)},
    'f64-64x16384': {'U': (4.55e-15, 0.869, 1.738), 'W2': (9.95e-14, 2.94, 5.88), 'W3': (2.59e-13, 3.07, 6.14)},
    'f32-8192x64': {'U': (2.84e-06, 0.704, 1.408), 'W2': (9.36e-05, 3.5, 7), 'W3': (6.23e-05, 1.86, 3.72)},
    'f32-16384x64': {'U': (3.10e-06, 0.68, 1.36), 'W2': (2.95e-04, 2.23, 4.46), 'W3': (2.68e-04, 1.87, 3.74)},
    'f64-8192x64': {'U': (4.25e-15, 0.761, 1.522), 'W2': (1.90e-13, 3.76, 7.52), 'W3': (9.16e-14, 1.62, 3.24)},
    'f64-16384x64': {'U': (4.36e-15, 1.11, 2.22), 'W2': (6.31e-13, 1.73, 3.46), 'W3': (3.88e-13, 2.14, 4.28)},
    'f32-64x64-COLSOLVE=tri': {'U': (1.35e-06, 0.574, 1.148), 'W2': (2.15e-06, 1.13, 2.26), 'W3': (2.33e-06, 1.33, 2.66)},
    'f32-1024x1024-COLSOLVE=tri': {'U': (3.88e-06, 0.342, 0.684), 'W2': (1.81e-05, 0.238, 0.476), 'W3': (1.29e-05, 0.409, 0.818)},
    'f64-512x512': {'U': (5.60e-15, 0.402, 0.804), 'W2': (9.55e-15, 1.4, 2.8), 'W3': (7.48e-15, 1.9, 3.8)},
    'f64-1024x1024': {'U': (4.50e-15, 0.649, 1.298), 'W2': (6.83e-14, 0.4, 0.8), 'W3': (3.64e-14, 1.03, 2.06)},
    'f64-256x256-COLSOLVE=fft': {'U': (3.54e-15, 1.07, 2.14), 'W2': (6.97e-15, 2.08, 4.16), 'W3': (5.29e-15, 2.34, 4.68)},
    'f32-256x256-COLSOLVE=stream': {'U': (1.67e-06, 0.697, 1.394), 'W2': (5.76e-06, 0.576, 1.152), 'W3': (4.72e-06, 0.906, 1.812)},
    'f64-256x256-COLSOLVE=stream': {'U': (3.54e-15, 3.23, 6.46), 'W2': (6.97e-15, 3.43, 6.86), 'W3': (5.29e-15, 2.11, 4.22)},
    'f32-256x256-COLSOLVE=stream-COLSTREAM_CHUNK=32': {'U': (1.67e-06, 0.697, 1.394), 'W2': (5.76e-06, 0.576, 1.152), 'W3': (4.72e-06, 0.906, 1.812)},
    'f64-256x256-COLSOLVE=stream-COLSTREAM_CHUNK=32': {'U': (3.54e-15, 3.23, 6.46), 'W2': (6.97e-15, 3.43, 6.86), 'W3': (5.29e-15, 2.11, 4.22)},
    'f32-2048x2048': {'U': (7.59e-06, 0.209, 0.418), 'W2': (2.49e-05, 0.695, 1.39)},
    'f32-60x36': {'U': (1.42e-06, 0.99, 1.98), 'W2': (2.44e-06, 1.04, 2.08), 'W3': (2.01e-06, 1.4, 2.8)},
    'f64-60x36': {'U': (3.26e-15, 0.705, 1.41), 'W2': (4.79e-15, 1.05, 2.1), 'W3': (3.83e-15, 1.57, 3.14)},
    'f32-36x36': {'U': (1.23e-06, 0.454, 0.908), 'W2': (2.73e-06, 1.04, 2.08), 'W3': (2.19e-06, 1.73, 3.46)},
    'f64-36x36': {'U': (2.40e-15, 0.624, 1.248), 'W2': (4.22e-15, 1.18, 2.36), 'W3': (3.36e-15, 1.45, 2.9)},
    'f32-63x65': {'U': (1.42e-06, 0.918, 1.836), 'W2': (2.72e-06, 1.15, 2.3), 'W3': (2.65e-06, 1.2, 2.4)},
    'f64-63x65': {'U': (3.05e-15, 0.801, 1.602), 'W2': (4.57e-15, 1.43, 2.86), 'W3': (4.11e-15, 1.72, 3.44)},
    'f32-250x250': {'U': (1.70e-06, 0.901, 1.802), 'W2': (4.33e-06, 1.1, 2.2), 'W3': (3.05e-06, 1.34, 2.68)},
    'f64-250x250': {'U': (4.26e-15, 0.624, 1.248), 'W2': (1.04e-14, 0.637, 1.274), 'W3': (6.43e-15, 1.14, 2.28)},
    'f32-36x36-COLSOLVE=fft': {'U': (1.23e-06, 0.611, 1.222), 'W2': (2.73e-06, 1.05, 2.1), 'W3': (2.19e-06, 1.37, 2.74)},
    'f64-36x36-COLSOLVE=fft': {'U': (2.40e-15, 0.796, 1.592), 'W2': (4.22e-15, 0.913, 1.826), 'W3': (3.36e-15, 1.55, 3.1)},
    'f32-360x360-COLSOLVE=stream': {'U': (1.91e-06, 0.516, 1.032), 'W2': (4.96e-06, 0.687, 1.374), 'W3': (3.84e-06, 1.11, 2.22)},
    'f64-360x360-COLSOLVE=stream': {'U': (4.39e-15, 2.77, 5.54), 'W2': (3.54e-14, 0.588, 1.176), 'W3': (8.12e-15, 2.36, 4.72)},
    'f32-68x68': {'U': (1.61e-06, 0.669, 1.338), 'W2': (2.73e-06, 1.33, 2.66), 'W3': (2.04e-06, 2.09, 4.18)},
    'f64-68x68': {'U': (2.94e-15, 1.51, 3.02), 'W2': (4.95e-15, 2.14, 4.28), 'W3': (3.31e-15, 2.94, 5.88)},
    'f32-97x101': {'U': (1.19e-06, 1.43, 2.86), 'W2': (2.94e-06, 1.36, 2.72), 'W3': (2.93e-06, 1.79, 3.58)},
    'f64-97x101': {'U': (3.08e-15, 1.57, 3.14), 'W2': (6.39e-15, 1.96, 3.92), 'W3': (5.44e-15, 2.08, 4.16)},
    'f32-63x65-NO_MR=1': {'U': (1.42e-06, 0.945, 1.89), 'W2': (2.72e-06, 1.39, 2.78), 'W3': (2.65e-06, 1.14, 2.28)},
    'f64-63x65-NO_MR=1': {'U': (3.05e-15, 1.38, 2.76), 'W2': (4.57e-15, 3.03, 6.06), 'W3': (4.11e-15, 2.22, 4.44)},
    'f32-4x4': {'U': (3.61e-07, 0.711, 1.422), 'W2': (9.93e-07, 0.719, 1.438), 'W3': (1.02e-06, 1.39, 2.78)},
    'f64-4x4': {'U': (3.33e-16, 1.61, 3.22), 'W2': (2.12e-15, 0.761, 1.522), 'W3': (4.62e-15, 0.274, 0.548)},
    'f32-4x512': {'U': (9.62e-07, 0.801, 1.602), 'W2': (1.02e-05, 0.92, 1.84), 'W3': (6.13e-06, 1.43, 2.86)},
    'f64-4x512': {'U': (1.53e-15, 1.41, 2.82), 'W2': (1.86e-14, 0.684, 1.368), 'W3': (9.21e-15, 1.74, 3.48)},
    'f32-1024x16': {'U': (1.53e-06, 0.814, 1.628), 'W2': (2.27e-05, 1.44, 2.88), 'W3': (1.67e-05, 1.49, 2.98)},
    'f64-1024x16': {'U': (2.60e-15, 1.62, 3.24), 'W2': (4.14e-14, 1.67, 3.34), 'W3': (2.69e-14, 1.73, 3.46)},
    'f32-16x1024': {'U': (1.63e-06, 1.05, 2.1), 'W2': (1.04e-05, 1.24, 2.48), 'W3': (6.45e-06, 1.33, 2.66)},
    'f64-16x1024': {'U': (2.88e-15, 1.14, 2.28), 'W2': (2.32e-14, 0.898, 1.796), 'W3': (1.34e-14, 2.56, 5.12)},
    'f32-16x2048': {'U': (1.53e-06, 1.02, 2.04), 'W2': (2.19e-05, 1.56, 3.12), 'W3': (1.55e-05, 1.17, 2.34)},
    'f64-16x2048': {'U': (4.58e-15, 0.634, 1.268), 'W2': (4.13e-14, 1.4, 2.8), 'W3': (2.86e-14, 3.44, 6.88)},
    'f32-32x4096': {'U': (1.83e-06, 0.967, 1.934), 'W2': (1.11e-04, 1.19, 2.38), 'W3': (6.53e-05, 1.3, 2.6)},
    'f64-32x4096': {'U': (3.24e-15, 1.12, 2.24), 'W2': (2.01e-13, 0.742, 1.484), 'W3': (9.69e-14, 1.88, 3.76)},
    'f32-32x8192': {'U': (1.80e-06, 0.851, 1.702), 'W2': (1.22e-04, 1.22, 2.44), 'W3': (7.29e-05, 1.35, 2.7)},
    'f32-8192x32': {'U': (1.87e-06, 0.911, 1.822), 'W2': (5.85e-05, 0.646, 1.292), 'W3': (2.22e-05, 1.36, 2.72)},
    'f32-64x1024-psi': {'U': (1.88e-06, 1.12, 2.24), 'W2': (8.20e-06, 1.24, 2.48), 'W3': (4.80e-06, 1.14, 2.28)},
    'f64-63x65-psi': {'U': (3.05e-15, 0.801, 1.602), 'W2': (4.57e-15, 1.43, 2.86), 'W3': (4.11e-15, 1.72, 3.44)},
    'f32-60x36-compat': {'U': (1.42e-06, 0.99, 1.98), 'W2': (1.71e-06, 1.12, 2.24), 'W3': (2.05e-06, 1.06, 2.12)},
    'f64-60x36-compat': {'U': (3.26e-15, 0.705, 1.41), 'W2': (3.47e-15, 1.37, 2.74), 'W3': (3.28e-15, 1.63, 3.26)},
}
