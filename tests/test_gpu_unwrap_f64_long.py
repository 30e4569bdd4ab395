"""GPU tests of the f64 weighted unwrap (a7, phase_unwrap.py:282-350) on 16384-point axes: the shapes BASELINE configs[4]
needs in the reference's own arithmetic.  Before this file's kernels an f64 plan with a 16384-point axis had no unwrap
workspace and every test below failed with GPAError.

  * rows of 16384 points (64 x 16384): rowdct_half_kernel<double, 14> / rowidct_p_half_kernel<double, 14>, which report
    under the names of the kernels they stand in for, against the oracle;
  * columns of 16384 points beside a shorter row axis (16384 x 64): colsolve_half_kernel (gpa_unwrap_colhalf.hip), one
    column per half-length transform, against the oracle;
  * 16384^2: the streamed and the resident transform-free column solves at n0 = 16384, whose tables exist for square images
    only, so this is the smallest shape that has them.  No oracle run at this size (its 16384^2 DCTs take minutes):
    (a) unweighted, against the equation the solve is defined by -- phi0 smooth, dx / dy its differences, the Poisson solve is
    exact and PCG stops after one iteration (the oracle's count at 512^2 and 1024^2 on this recipe, where its own error is
    9e-13 / 2.2e-12 of max|phi0 - mean|); (b) weighted, streamed against resident, each of which is held to the oracle at
    1e-8 at the smaller sizes of test_gpu_unwrap_long.py;
  * the limits that stay: no f64 sweep at 16384 points, no unwrap beside an axis that is not a power of two.

Tolerance (relative to max |phi|): f64 1e-8, the project's figure for long axes (test_gpu_unwrap_long.py).
Measured on MI355X (profiles/unwrap_f64_16384.txt has the figures of the run that was recorded)."""
import time

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


def test_rows_of_16384_points_f64_vs_oracle():
    """64 x 16384, f64, weighted, kmax 10: the half-length row kernels at 16384 points against the oracle"""
    shape = (64, 16384)
    dx, dy, w = make_problem(shape, seed=shape[0] + shape[1])
    ref, ref_it = orc.unwrap_prediff(dx, dy, w, kmax=10, compat=False, return_iters=True)
    phi, it, prof = solve_profiled(shape, np.float64, dx, dy, w, 10)
    assert np.isfinite(phi).all()
    print('f64 rows', shape, 'rel err %.3e' % rel(phi, ref), 'iters', it, ref_it)
    assert rel(phi, ref) < 1e-8, rel(phi, ref)
    assert it == ref_it
    for k in ('rowdct_fused_kernel', 'rowidct_p_kernel', 'pq_kernel'):
        assert k in prof and prof[k][0] >= 1, (k, sorted(prof))


def test_columns_of_16384_points_f64_vs_oracle():
    """16384 x 64, f64, weighted, kmax 10: colsolve_half_kernel -- the only column solve this shape has -- against the oracle"""
    shape = (16384, 64)
    dx, dy, w = make_problem(shape, seed=shape[0] + shape[1])
    ref, ref_it = orc.unwrap_prediff(dx, dy, w, kmax=10, compat=False, return_iters=True)
    phi, it, prof = solve_profiled(shape, np.float64, dx, dy, w, 10)
    assert np.isfinite(phi).all()
    print('f64 columns', shape, 'rel err %.3e' % rel(phi, ref), 'iters', it, ref_it)
    assert rel(phi, ref) < 1e-8, rel(phi, ref)
    assert it == ref_it
    assert 'colsolve_half_kernel' in prof and prof['colsolve_half_kernel'][0] >= 1, sorted(prof)
    for other in ('colsolve_kernel', 'colsolve_tri_kernel', 'colstream_apply_kernel'):
        assert other not in prof, sorted(prof)


# ---- 16384^2 -------------------------------------------------------------------------------------------------------
N = 16384
BLOCK = 1024


@pytest.fixture(scope='module')
def square():
    """the smooth field of make_problem at 16384^2 (no noise), its wrapped differences and a closed-form weight, built in row
    blocks from separable factors: no random draws, no 2 GiB temporaries beyond the arrays handed out"""
    t0 = time.time()
    x = np.arange(N) / float(N)
    y = np.arange(N) / float(N)
    # sin(2 pi (1.5 x + 0.5 y)) = sin(3 pi x) cos(pi y) + cos(3 pi x) sin(pi y)
    sa, ca = np.sin(3 * np.pi * x), np.cos(3 * np.pi * x)
    fb = 6.0 * np.cos(np.pi * y) * np.cos(4 * np.pi * y)
    gb = 6.0 * np.sin(np.pi * y) * np.cos(4 * np.pi * y)
    phi0 = np.empty((N, N))
    for r0 in range(0, N, BLOCK):
        s = slice(r0, r0 + BLOCK)
        np.multiply.outer(sa[s], fb, out=phi0[s])
        phi0[s] += np.multiply.outer(ca[s], gb)
        phi0[s] += (40.0 * x[s])[:, None]
        phi0[s] += (25.0 * y)[None, :]
    dx = np.empty((N, N - 1))
    dy = np.empty((N - 1, N))
    dxw = np.empty((N, N - 1))
    dyw = np.empty((N - 1, N))
    for r0 in range(0, N, BLOCK):
        r1 = min(r0 + BLOCK + 1, N)                      # one row of overlap for the differences along axis 0
        blk = phi0[r0:r1]
        psi = orc.wrap_to_pi(blk)
        dx[r0:r0 + BLOCK] = np.diff(blk[:BLOCK], axis=1)
        dxw[r0:r0 + BLOCK] = np.diff(psi[:BLOCK], axis=1)
        dy[r0:r1 - 1] = np.diff(blk, axis=0)
        dyw[r0:r1 - 1] = np.diff(psi, axis=0)
    weight = 0.6 + 0.5 * np.multiply.outer(np.cos(6 * np.pi * x), np.cos(4 * np.pi * y))
    print('16384^2 inputs built in %.1f s' % (time.time() - t0))
    return {'phi0': phi0, 'dx': dx, 'dy': dy, 'dxw': dxw, 'dyw': dyw, 'weight': weight}


def test_square_16384_f64_unweighted_solves_its_equation(square):
    """(a) dx, dy = the differences of a smooth phi0 (gradient <= 0.0073 rad/px: nothing wraps), no weight: the unwrap must
    return phi0 up to its mean, in ONE iteration -- the preconditioner is the exact inverse then -- through the streamed
    column solve, the default at this size"""
    t0 = time.time()
    phi0 = square['phi0']
    phi, it, prof = solve_profiled((N, N), np.float64, square['dx'], square['dy'], None, 5)
    assert it == 1, it
    assert 'colstream_apply_kernel' in prof, sorted(prof)
    for k in ('rowdct_fused_kernel', 'rowidct_p_kernel', 'pq_kernel'):
        assert k in prof, (k, sorted(prof))
    m0, m = phi0.mean(), phi.mean()
    err = scale = 0.0
    for r0 in range(0, N, BLOCK):
        s = slice(r0, r0 + BLOCK)
        ref = phi0[s] - m0
        err = max(err, float(np.abs((phi[s] - m) - ref).max()))
        scale = max(scale, float(np.abs(ref).max()))
    print('f64 16384^2 unweighted: rel err %.3e, iters %d, wall %.1f s' % (err / scale, it, time.time() - t0))
    assert err < 1e-8 * scale, err / scale


def test_square_16384_f64_streamed_equals_resident_columns(square, gpa_option):
    """(b) weighted (closed-form weight), the differences of the WRAPPED phi0, kmax 3: the streamed column solve against the
    resident transform-free kernel (16 rows per thread, 1024 chunks: its limit) -- equal iteration counts, phi within
    2e-8 (each mode is held to the oracle at 1e-8 at smaller sizes)"""
    t0 = time.time()
    out = {}
    for mode in ('stream', 'tri'):
        gpa_option('COLSOLVE', mode)
        phi, it, prof = solve_profiled((N, N), np.float64, square['dxw'], square['dyw'], square['weight'], 3)
        out[mode] = (phi, it)
        assert ('colstream_apply_kernel' if mode == 'stream' else 'colsolve_tri_kernel') in prof, (mode, sorted(prof))
        assert ('colsolve_tri_kernel' if mode == 'stream' else 'colstream_apply_kernel') not in prof, (mode, sorted(prof))
    assert out['stream'][1] == out['tri'][1], (out['stream'][1], out['tri'][1])
    err = scale = 0.0
    for r0 in range(0, N, BLOCK):
        s = slice(r0, r0 + BLOCK)
        err = max(err, float(np.abs(out['stream'][0][s] - out['tri'][0][s]).max()))
        scale = max(scale, float(np.abs(out['tri'][0][s]).max()))
    print('f64 16384^2 weighted: stream vs tri rel %.3e, iters %d, wall %.1f s' % (err / scale, out['tri'][1], time.time() - t0))
    assert np.isfinite(scale) and scale > 0
    assert err < 2e-8 * scale, err / scale


def test_f64_limits_that_stay():
    """the f64 sweep still stops at 8192 points (the plan exists and says so), and a 16384-point axis beside one that is not a
    power of two has no unwrap kernels"""
    plan = _lib.Plan((64, 16384), 1, np.float64)
    with pytest.raises(_lib.GPAError, match='too large for the sweep'):
        plan.lockin_batch(np.zeros((64, 16384)), np.zeros((1, 2)), 5.0)
    plan.close()
    shape = (300, 16384)
    rng = np.random.default_rng(1)
    dx = 0.1 * rng.standard_normal((shape[0], shape[1] - 1))
    dy = 0.1 * rng.standard_normal((shape[0] - 1, shape[1]))
    plan = _lib.Plan(shape, 1, np.float64)
    with pytest.raises(_lib.GPAError, match='no kernels for this shape'):
        plan.unwrap_prediff(dx, dy, None, kmax=2)
    plan.close()
