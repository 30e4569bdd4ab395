"""GPU parity tests of the weighted unwrap (a7, phase_unwrap.py:282-350) on LONG axes and of the streamed column
solve -- the kernel instantiations the 8192^2 and 16384^2 global solves of BASELINE configs[3] / [4] select.

The reference is one code path for every size; this build runs different kernels from 8192 points on (four-pass row
transforms, 4-wave rowidct_p, the streamed recursion down the columns).  Every one of them is held to the ORACLE here:
  * elongated images (64 x 16384, 16384 x 64, 96 x 8192, 8192 x 96, 128 x 8192 ...): the long-row kernels and the
    long-column DCT kernel against the oracle, which costs < 1 s at these shapes.  (Aspect ratios >= 2: the reference's
    swapped-axis eigenvalue table is singular there and its result NaN; device and oracle use the true eigenvalues,
    as in test_unwrap_elongated_images.)
  * square images: the streamed column solve (gpa_unwrap_colstream.hip) against the oracle at 256^2 ... 2048^2 in both
    precisions, ragged sizes included, and at 8192^2 (f32, 3 iterations: the oracle needs ~1 minute there);
    against the resident column kernels (DCT / transform-free) at 4096^2.
Which kernels ran is asserted through gpa_last_kernel_profile.

Tolerances (relative to max |phi|): f64 1e-8, f32 5e-5 (a 16384-point f32 transform carries ~1e-6 per pass)."""
import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def make_problem(shape, seed, rough=False):
    """wrapped noisy phase of a smooth field + a weight with structure; returns dx, dy (pre-differenced) and weight"""
    rng = np.random.default_rng(seed)
    n0, n1 = shape
    x = np.arange(n0)[:, None] / float(n0)
    y = np.arange(n1)[None, :] / float(n1)
    phi = 40.0 * x + 25.0 * y + 6.0 * np.sin(2 * np.pi * (1.5 * x + 0.5 * y)) * np.cos(2 * np.pi * 2.0 * y)
    psi = orc.wrap_to_pi(phi + (0.3 if rough else 0.05) * rng.normal(size=shape))
    weight = (0.05 + rng.random(shape)) if rough else (0.5 + 0.5 * np.cos(2 * np.pi * 3 * x) * np.cos(2 * np.pi * 2 * y) + 0.2 * rng.random(shape))
    weight = np.abs(weight) + 0.02
    return np.diff(psi, axis=1), np.diff(psi, axis=0), weight


def solve_profiled(shape, dtype, dx, dy, w, kmax):
    plan = _lib.Plan(shape, 1, dtype)
    plan.set_profiling(True)
    phi, it = plan.unwrap_prediff(dx, dy, w, kmax=kmax)
    prof = plan.last_kernel_profile()
    plan.close()
    return phi, it, prof


# f32 tolerance by the longest axis: the Poisson preconditioner divides the lowest modes by eigenvalues ~ (pi / N)^2, i.e.
# multiplies the f32 rounding of a row transform (~1e-7 per pass) by up to N^2 / pi^2 = 2.7e7 at N = 16384; the iteration
# corrects most of it, what is left is a smooth offset whose size is a matter of the rounding's luck: over 12 problems (seeds) the
# error at 64 x 16384 is 3e-4 .. 2.7e-3 of max|phi| (median 7e-4), at 128 x 8192 4e-5 .. 3.3e-4 (median 8e-5) -- the same
# distribution for the one-row-per-workgroup and the persistent row kernels (tools/dbg/halfpers_seeds.py, round 6).
# So these numbers are set by the amplification, not by the kernels, and an accuracy regression common to both kernel families
# would pass them: long f32 rows are held to a rounding-level bound in tests/test_gpu_unwrap_modes.py, per DCT mode with the
# amplification undone (64 x 8192 and 64 x 16384, persistent and one-row-per-workgroup: 0.5 .. 1.4 of a plain f32 solve).
F32_TOL = {8192: 6e-4, 16384: 4e-3}


# (both sides powers of two: the power-of-two kernels; 96 x 8192 / 8192 x 96 run the same long axes on the mixed-radix
#  engine, whose kernels share the profile names)
LONG_SHAPES = [((64, 16384), [np.float32]), ((16384, 64), [np.float32]),
               ((128, 8192), [np.float32, np.float64]), ((8192, 128), [np.float32, np.float64]),
               ((96, 8192), [np.float32]), ((8192, 96), [np.float32]), ((2048, 8192), [np.float32])]


@pytest.mark.parametrize('shape,dtypes', LONG_SHAPES)
def test_long_axis_unwrap_vs_oracle(shape, dtypes):
    """8192- and 16384-point rows / columns against the oracle, weighted, kmax 10: the four-pass rowdct_fused / rowidct_p
    instantiations (rows) and the long-column DCT kernel (columns)"""
    dx, dy, w = make_problem(shape, seed=shape[0] + shape[1])
    ref, ref_it = orc.unwrap_prediff(dx, dy, w, kmax=10, compat=False, return_iters=True)
    for dtype in dtypes:
        phi, it, prof = solve_profiled(shape, dtype, dx, dy, w, 10)
        tol = 1e-8 if dtype is np.float64 else F32_TOL[max(shape)]
        assert np.isfinite(phi).all()
        print('long axis', shape, np.dtype(dtype).name, 'rel err %.3e' % rel(phi, ref), 'iters', it, ref_it)
        assert rel(phi, ref) < tol, (shape, np.dtype(dtype).name, rel(phi, ref))
        if dtype is np.float64:
            assert it == ref_it
        # the fused iteration ran (rows up to 512 pixels: row kernel and stencil in one launch)
        want = ['rowdct_fused_kernel', 'colsolve_kernel', 'phi_flush_kernel']
        want += ['rowidct_pq_kernel'] if (shape[1] <= 512 and shape[0] & (shape[0] - 1) == 0 and shape[1] & (shape[1] - 1) == 0) else ['rowidct_p_kernel', 'pq_kernel']
        for k in want:
            assert k in prof and prof[k][0] >= 1, (k, sorted(prof))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n', [256, 500, 1000, 1024, 2048])
def test_streamed_column_solve_vs_oracle(n, dtype, gpa_option):
    """square images with the streamed column solve forced (COLSOLVE=stream): chunk sums -> scan -> recursions, against the
    oracle's dctn / idctn preconditioner; 500 and 1000 are ragged (last chunk short, columns not a multiple of 256)"""
    shape = (n, n)
    dx, dy, w = make_problem(shape, seed=n, rough=True)
    ref, ref_it = orc.unwrap_prediff(dx, dy, w, kmax=12, return_iters=True)
    gpa_option('COLSOLVE', 'stream')
    phi, it, prof = solve_profiled(shape, dtype, dx, dy, w, 12)
    for k in ('colstream_agg_kernel', 'colstream_scan_kernel', 'colstream_apply_kernel'):
        assert k in prof, sorted(prof)
    assert 'colsolve_kernel' not in prof and 'colsolve_tri_kernel' not in prof
    assert rel(phi, ref) < (1e-8 if dtype is np.float64 else 5e-5), rel(phi, ref)
    if dtype is np.float64:
        assert it == ref_it
    # unweighted, a different chunk height
    gpa_option('COLSTREAM_CHUNK', '32' if n >= 1024 else '64')
    ref_u = orc.unwrap_prediff(dx, dy, None, kmax=5)
    plan = _lib.Plan(shape, 1, dtype)
    phi_u, _ = plan.unwrap_prediff(dx, dy, None, kmax=5)
    plan.close()
    assert rel(phi_u, ref_u) < (1e-8 if dtype is np.float64 else 5e-5)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_streamed_column_solve_equals_resident_kernels_4096(dtype, gpa_option):
    """4096^2 (the headline size; the streamed solve is its default): same iterates as the resident column kernels --
    the DCT kernel and the transform-free recursion -- iteration counts equal in f64, phi within the PCG tolerance"""
    n = 4096
    dx, dy, w = make_problem((n, n), seed=7, rough=True)
    out = {}
    for mode in ('stream', 'tri', 'fft'):
        gpa_option('COLSOLVE', mode)
        phi, it, prof = solve_profiled((n, n), dtype, dx, dy, w, 10)
        out[mode] = (phi, it)
        want = {'stream': 'colstream_apply_kernel', 'tri': 'colsolve_tri_kernel', 'fft': 'colsolve_kernel'}[mode]
        assert want in prof, (mode, sorted(prof))
    gpa_option('COLSOLVE', None)
    phi, it, prof = solve_profiled((n, n), dtype, dx, dy, w, 10)
    assert 'colstream_apply_kernel' in prof            # the default at this size
    tol = 1e-9 if dtype is np.float64 else 5e-5
    for mode in ('tri', 'fft'):
        assert rel(out['stream'][0], out[mode][0]) < tol, (mode, rel(out['stream'][0], out[mode][0]))
        if dtype is np.float64:
            assert out['stream'][1] == out[mode][1]
    assert np.array_equal(phi, out['stream'][0])


def test_unwrap_8192_square_vs_oracle():
    """the 8192^2 global solve of BASELINE configs[3] against the ORACLE at full size (f32, weighted, 3 iterations: the
    oracle's 8192^2 DCTs take about a minute on the host): four-pass row kernels + the streamed column solve"""
    n = 8192
    dx, dy, w = make_problem((n, n), seed=11)
    ref = orc.unwrap_prediff(dx, dy, w, kmax=3, workers=-1)
    phi, it, prof = solve_profiled((n, n), np.float32, dx, dy, w, 3)
    assert it == 3
    for k in ('rowdct_fused_kernel', 'rowidct_p_kernel', 'colstream_agg_kernel', 'colstream_scan_kernel', 'colstream_apply_kernel'):
        assert k in prof, sorted(prof)
    assert rel(phi, ref) < 5e-5, rel(phi, ref)


@pytest.mark.parametrize('n', [8192, 16384])
def test_long_square_streamed_vs_resident_columns(n, gpa_option):
    """8192^2 and 16384^2 (f32): the streamed column solve against the resident transform-free kernel it replaces
    (16 rows per thread at 16384 points), 4 iterations; and the fused driver's iteration counts agree"""
    dx, dy, w = make_problem((n, n), seed=n)
    out = {}
    for mode in ('stream', 'tri'):
        gpa_option('COLSOLVE', mode)
        phi, it, prof = solve_profiled((n, n), np.float32, dx, dy, w, 4)
        out[mode] = phi
        assert ('colstream_apply_kernel' if mode == 'stream' else 'colsolve_tri_kernel') in prof, sorted(prof)
        assert it == 4
    assert rel(out['stream'], out['tri']) < 5e-5, rel(out['stream'], out['tri'])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n', [2048, 4096])
def test_stencil_fused_iteration_equals_separate_kernels(n, dtype, gpa_option):
    """rows of 2048 / 4096 points: the iteration with the stencil inside the row-transform launch (pqdct_kernel: q never
    reaches HBM, the residual update R -= alpha DCT_rows(q) rides in the column solve's first launch) against the same
    solve with separate stencil / row-transform / update kernels (NO_PQDCT): same iterates to rounding -- iteration counts
    equal, phi within the PCG tolerance -- and, at 2048^2, the oracle's phi"""
    dx, dy, w = make_problem((n, n), seed=n + 1, rough=True)
    phi_f, it_f, prof_f = solve_profiled((n, n), dtype, dx, dy, w, 12)
    assert 'pqdct_kernel' in prof_f and prof_f['pqdct_kernel'][0] == 11 and prof_f['pq_kernel'][0] == 1, sorted(prof_f.items())
    assert 'rowdct_fused_kernel' in prof_f and prof_f['rowdct_fused_kernel'][0] == 1      # iteration 0 only
    gpa_option('NO_PQDCT', '1')
    phi_s, it_s, prof_s = solve_profiled((n, n), dtype, dx, dy, w, 12)
    assert 'pqdct_kernel' not in prof_s and prof_s['pq_kernel'][0] == 12
    assert it_f == it_s
    assert rel(phi_f, phi_s) < (1e-10 if dtype is np.float64 else 3e-5), rel(phi_f, phi_s)
    # unweighted, few iterations (kmax 2: the fused kernel runs once)
    gpa_option('NO_PQDCT', None)
    pu_f, _, _ = solve_profiled((n, n), dtype, dx, dy, None, 2)
    gpa_option('NO_PQDCT', '1')
    pu_s, _, _ = solve_profiled((n, n), dtype, dx, dy, None, 2)
    assert rel(pu_f, pu_s) < (1e-10 if dtype is np.float64 else 3e-5)
    if n == 2048:
        ref, ref_it = orc.unwrap_prediff(dx, dy, w, kmax=12, return_iters=True)
        assert rel(phi_f, ref) < (1e-8 if dtype is np.float64 else 5e-5)
        if dtype is np.float64:
            assert it_f == ref_it


def test_stack_of_2048_frames_equals_single_images():
    """a stack of 2048^2 frames (blockIdx.z = problem) through the stencil-fused iteration and the streamed column solve:
    every frame's u and iteration counts equal the single-image driver's bit for bit (same kernels, same partial-sum order)"""
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
    n = 2048
    kvecs = hex_kvecs(0.1, 7.0)
    klists = np.stack(explicit_klists(kvecs, 0.04, 2, 2))
    imgs = np.stack([hex_moire((n, n), kvecs, (0.4 + 0.3 * i) * gaussian_bump_displacement((n, n)), noise=0.05, seed=i, dtype=np.float32)
                     for i in range(3)])
    plan = _lib.Plan((n, n), 12, np.float32)
    u_b, it_b = plan.extract_displacement_field_stack(imgs, kvecs, klists, 10, 20, kmax=10, chunk=3)
    for i in range(3):
        u, _, _, iters = plan.extract_displacement_field(imgs[i], kvecs, klists, 10, 20, kmax=10)
        assert np.array_equal(u_b[i], u), (i, float(np.abs(u_b[i] - u).max()))
        assert tuple(it_b[i]) == tuple(iters)
    plan.close()


@pytest.mark.parametrize('shape', [(4096, 4096), (2048, 4096), (64, 4096), (1024, 8192), (512, 16384)])
def test_persistent_row_kernels_equal_per_pair_kernels(shape, gpa_option):
    """round 5: the persistent, software-pipelined rowidct_p kernel of gpa_unwrap_rowpers.hip (4096-point f32 rows: LDS-DMA of
    the next row pair into the other LDS buffer while the current one is transformed) against the one-pair-per-workgroup
    kernel it replaces (NO_ROWPERS): the same arithmetic in the same order -- phi equal BIT FOR BIT, equal iteration
    counts, over bands of 4 / 2 / 1 row pairs per workgroup, weighted, kmax 10 and kmax 23 (two flushes of the ring);
    and the oracle's phi at 2048 x 4096.  Round 6: the same for the persistent half-length kernels of 8192- and 16384-point
    rows (gpa_unwrap_rowhalfpers.hip; bands of 2 / 1-2 rows per workgroup) against the one-row-per-workgroup kernels."""
    dx, dy, w = make_problem(shape, seed=shape[0] + 7)
    dx, dy, w = (np.ascontiguousarray(v, dtype=np.float32) for v in (dx, dy, w))
    for kmax in (10, 23):
        gpa_option('NO_ROWPERS', None)
        plan = _lib.Plan(shape, 1, np.float32)
        a, it_a = plan.unwrap_prediff(dx, dy, w, kmax=kmax)
        a2, _ = plan.unwrap_prediff(dx, dy, w, kmax=kmax)
        plan.close()
        gpa_option('NO_ROWPERS', '1')
        plan = _lib.Plan(shape, 1, np.float32)
        b, it_b = plan.unwrap_prediff(dx, dy, w, kmax=kmax)
        plan.close()
        gpa_option('NO_ROWPERS', None)
        assert np.isfinite(a).all()
        assert np.array_equal(a, a2)                       # run to run (no race between DMA, reads and exchanges)
        assert it_a == it_b == kmax
        assert np.array_equal(a, b), (shape, kmax, float(np.abs(a - b).max()))
    if shape == (2048, 4096):
        ref = orc.unwrap_prediff(dx.astype(np.float64), dy.astype(np.float64), w.astype(np.float64), kmax=10, compat=False)
        plan = _lib.Plan(shape, 1, np.float32)
        phi, _ = plan.unwrap_prediff(dx, dy, w, kmax=10)
        plan.close()
        assert rel(phi, ref) < 5e-5


def test_f32_stagnation_guard_fires_and_has_a_switch(golden, gpa_option):
    """VERDICT r05 item 8 / ADVICE r05: the f32-only stagnation stop (pcg_breakdown (2), gpa_unwrap_impl.h; not in the
    reference) on a case where it FIRES -- the 63 x 65 golden case at kmax = 100, which the f64 reference solves in 15
    iterations -- asserted against the oracle's iterate at the SAME iteration count; F32_STALL=0 switches it off (the solve
    then runs on like the reference's loop, phase_unwrap.py:326-349, and drifts: what the guard is for); and it never acts
    within kmax = 10 on the benchmark's kind of image (2048^2): the same bits with and without it."""
    g = golden('hex_63x65')
    wn = np.linalg.norm(g['a5_weights'], axis=0)
    dx, dy = g['a6_dudx'][0], g['a6_dudy'][0]
    plan = _lib.Plan(g['image'].shape, 1, np.float32)
    phi, it = plan.unwrap_prediff(dx, dy, wn, kmax=100)
    assert 10 < it < 40, it
    ref_it = orc.unwrap_prediff(dx, dy, wn, kmax=it)
    sc = np.abs(ref_it).max()
    assert np.abs(phi - ref_it).max() < 2.5e-5 * sc
    gpa_option('F32_STALL', '0')
    phi_off, it_off = plan.unwrap_prediff(dx, dy, wn, kmax=100)
    assert it_off > it
    ref_100 = orc.unwrap_prediff(dx, dy, wn, kmax=100)
    # without the guard the f32 iterate has drifted further from the reference's answer than with it
    assert np.abs(phi_off - ref_100).max() > np.abs(phi - ref_100).max()
    gpa_option('F32_STALL', '5')
    _, it5 = plan.unwrap_prediff(dx, dy, wn, kmax=100)
    assert it < it5 <= it_off
    gpa_option('F32_STALL', None)
    plan.close()
    # the benchmark's kind of image: 10 + 10 iterations, the guard is inert
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
    n = 2048
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire((n, n), kvecs, gaussian_bump_displacement((n, n)), noise=0.1, seed=100, dtype=np.float32)
    klists = np.stack(explicit_klists(kvecs, 0.04, 4, 4))
    plan = _lib.Plan((n, n), 48, np.float32)
    u, _, _, iters = plan.extract_displacement_field(img, kvecs, klists, 10, 20, 10)
    gpa_option('F32_STALL', '0')
    u_off, _, _, iters_off = plan.extract_displacement_field(img, kvecs, klists, 10, 20, 10)
    gpa_option('F32_STALL', None)
    plan.close()
    assert tuple(iters) == tuple(iters_off) == (10, 10)
    assert np.array_equal(u, u_off)


def test_shapes_without_unwrap_kernels_say_so():
    """the unwrap's size limits: a 16384-point axis beside an axis that is not a power of two has no kernels in
    f32 (the mixed-radix engine stops at 8192 points), nor has 300 x 8192 in f64 -- the call fails with GPA_ERR_STATE and names the
    limit instead of a bare HIP error string; 300 x 8192 in f32 runs."""
    rng = np.random.default_rng(1)
    for shape, dt, ok in (((300, 16384), np.float32, False), ((300, 8192), np.float64, False), ((300, 8192), np.float32, True)):
        dx = (0.1 * rng.standard_normal((shape[0], shape[1] - 1))).astype(dt)
        dy = (0.1 * rng.standard_normal((shape[0] - 1, shape[1]))).astype(dt)
        plan = _lib.Plan(shape, 1, dt)
        if ok:
            phi, it = plan.unwrap_prediff(dx, dy, None, kmax=2)
            assert np.isfinite(phi).all() and it == 2
        else:
            with pytest.raises(_lib.GPAError, match='no kernels for this shape'):
                plan.unwrap_prediff(dx, dy, None, kmax=2)
        plan.close()
