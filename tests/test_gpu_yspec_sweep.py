"""GPU tests of the y-spectral sweep: a row pre-pass leaves FFT_y(image - mean) (rowfft_kernel), pass A
filters its columns along x (the x filter commutes with a transform along y), the end strips come from the spatial pass A on
the columns within E of either row end (passA_strips_kernel), and the shared-forward pass B loads its live spectral blocks
instead of transforming the row.  Checked against the oracle and against the spatial path (NO_YSPEC=1) on the smallest shapes
that reach every index path -- (64, 2048): odd and even band rotations of the 16 x 16 x 8 transform; (96, 4096): a zero-padded
x axis -- with a plain 4 x 4 list, a list whose band wraps around block 15, and two peaks that share their x-planes
(tests/yspec_cases.py).  Semantics: geometric_phase_analysis.py:72-75 (lock-in), :679-684 (strict '>' in list order).

Case 4 (f32, both paths against the f64 oracle, over the pixels where both paths pick the oracle's winner, relative to the
largest |lock-in| of the oracle); measured on MI355X:

    shape       case / peak   max new    max spatial   rms new    rms spatial
    (64, 2048)  grid   / 0    4.89e-07   4.81e-07      1.43e-07   1.33e-07
    (96, 4096)  grid   / 0    5.88e-07   4.45e-07      1.73e-07   1.39e-07
    (64, 2048)  wrap   / 0    5.73e-07   5.42e-07      2.06e-07   1.89e-07
    (96, 4096)  wrap   / 0    5.68e-07   5.69e-07      1.65e-07   1.78e-07
    (64, 2048)  shared / 0    4.74e-07   4.31e-07      1.24e-07   1.31e-07
    (64, 2048)  shared / 1    5.41e-07   4.65e-07      1.39e-07   1.53e-07
    (96, 4096)  shared / 0    4.52e-07   4.93e-07      1.27e-07   1.31e-07
    (96, 4096)  shared / 1    4.59e-07   4.82e-07      1.22e-07   1.32e-07
The largest ratio new / spatial is 1.32 (max) and 1.24 (rms); the winners of the two paths agreed at every pixel.
Case 5, (256, 2048) f32 driver, new path against NO_YSPEC=1: rms 1.9e-06 px, max 5.9e-06 px, 10 + 10 iterations both.
"""
import numpy as np
import pytest

from pygpa_amd import _lib
from test_gpu_parity import TOL
from tolerances import F32
import yspec_cases as yc

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
NEW = ('rowfft_kernel', 'passA_strips_kernel')


def _run(name, shape, dtype):
    """(lock-ins (P, n0, n1), kidx (P, n0, n1), kernel profile) of one case: a single peak through the sweep entry point, two
    peaks through the fused driver"""
    img, kvecs, klists = yc.case(name, shape)
    P, K = klists.shape[:2]
    plan = _lib.Plan(shape, P * K, dtype)
    plan.set_profiling(True)
    if P == 1:
        lock, kidx, _ = plan.sweep(img - img.mean(), kvecs[0], klists[0], yc.SIGMA)
        lock, kidx = lock[None], kidx[None]
    else:
        _, lock, kidx, _ = plan.extract_displacement_field(img, kvecs, klists, yc.SIGMA, 2 * yc.SIGMA, kmax=2,
                                                           want_lockins=True, want_kidx=True)
    prof = plan.last_kernel_profile()
    plan.close()
    return lock, kidx, prof


def _took_new_path(prof):
    assert all(k in prof for k in NEW), sorted(prof)
    assert prof['passA_kernel'][0] == 1 and prof['rowfft_kernel'][0] == 1 and prof['passA_strips_kernel'][0] == 1, prof
    assert 'passB_shared_kernel' in prof, sorted(prof)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', yc.SHAPES)
@pytest.mark.parametrize('name', yc.CASES)
def test_yspec_vs_oracle_and_end_columns(name, shape, dtype):
    """cases 1 - 3: winner index identical to the oracle in f64 (amplitude ties only in f32), lock-ins within the bound of
    test_shared_passb_vs_oracle_and_end_columns everywhere and in the first / last 3 sigma columns on their own (the end fix
    reads the strips buffer); the band of 'wrap' (and of every f32 list here) straddles blocks 15 -> 0, the planes of 'shared'
    are read by two peaks with different rotations"""
    f32 = dtype is np.float32
    rots = [yc.band_rotation(kl, yc.SIGMA, f32) for kl in yc.case(name, shape)[2]]
    if name == 'wrap':
        assert rots[0][0] + rots[0][1] > 16, rots
    if name == 'shared':
        assert rots[0][0] != rots[1][0] and rots[1][0] + 8 <= 16, rots
    lock, kidx, prof = _run(name, shape, dtype)
    _took_new_path(prof)
    e3 = 3 * yc.SIGMA
    for p, (ref_lock, ref_kidx, amps) in enumerate(yc.oracle(name, shape)):
        same = kidx[p] == ref_kidx
        if not f32:
            assert same.all(), 'f64 winner index differs from the oracle at %d pixels' % int((~same).sum())
        else:
            a = np.take_along_axis(amps, np.maximum(kidx[p], 0)[None], 0)[0]
            b = np.take_along_axis(amps, ref_kidx[None], 0)[0]
            assert np.all(np.abs(a - b)[~same] <= TOL[dtype]['tie'] * amps.max()), 'kidx mismatches that are not amplitude ties'
        assert same.mean() > 0.9999
        d = np.where(same, np.abs(lock[p] - ref_lock), 0) / np.abs(ref_lock).max()
        assert d.max() < TOL[dtype]['lock'], (p, d.max())
        assert max(d[:, :e3].max(), d[:, -e3:].max()) < TOL[dtype]['lock']


@pytest.mark.parametrize('shape', yc.SHAPES)
@pytest.mark.parametrize('name', yc.CASES)
def test_f32_error_against_spatial_path(name, shape, gpa_option):
    """case 4: both f32 paths against the f64 oracle.  Both sum the same number of f32 roundings in a different order, so the
    new path's max and rms error may exceed the spatial path's by at most a factor 2; the winners may differ between the paths
    only where the oracle's two amplitudes agree to 1e-5 relative, at no more than 0.1 % of the pixels (the inputs' own share
    of such near-ties is below a tenth of that: tests/test_yspec_host.py)"""
    lock_n, kidx_n, prof_n = _run(name, shape, np.float32)
    gpa_option('NO_YSPEC', '1')
    lock_s, kidx_s, prof_s = _run(name, shape, np.float32)
    gpa_option('NO_YSPEC', None)
    _took_new_path(prof_n)
    assert not any(k in prof_s for k in NEW) and 'passB_shared_kernel' in prof_s, sorted(prof_s)
    for p, (ref_lock, ref_kidx, amps) in enumerate(yc.oracle(name, shape)):
        ok = (kidx_n[p] == ref_kidx) & (kidx_s[p] == ref_kidx)
        sc = np.abs(ref_lock).max()
        en, es = np.abs(lock_n[p] - ref_lock)[ok] / sc, np.abs(lock_s[p] - ref_lock)[ok] / sc
        fig = (en.max(), es.max(), np.sqrt(np.mean(en ** 2)), np.sqrt(np.mean(es ** 2)))
        print('yspec f32 error %s %-6s peak %d: max new %.3e spatial %.3e | rms new %.3e spatial %.3e' % ((shape, name, p) + fig))
        differ = kidx_n[p] != kidx_s[p]
        a = np.take_along_axis(amps, np.maximum(kidx_n[p], 0)[None], 0)[0]
        b = np.take_along_axis(amps, np.maximum(kidx_s[p], 0)[None], 0)[0]
        assert np.all(np.abs(a - b)[differ] <= 1e-5 * np.maximum(a, b)[differ]), 'winners differ away from near-ties'
        assert differ.mean() <= 1e-3
        assert fig[0] <= 2 * fig[1], fig
        assert fig[2] <= 2 * fig[3], fig


def test_fused_driver_against_spatial_path(gpa_option):
    """case 5: the fused driver on (256, 2048), f32, kmax 10 -- the same iteration counts as the spatial path and u within the
    f32 bounds of tests/tolerances.py (rms 1e-5 px, max 0.02 px, after removing the free mean of each component)"""
    shape = (256, 2048)
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
    from oracle import gpa_oracle as orc
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.2, seed=4)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 4, 4))
    plan = _lib.Plan(shape, 48, np.float32)
    plan.set_profiling(True)
    u_n, _, _, it_n = plan.extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma, kmax=10, want_kidx=True)
    prof_n = plan.last_kernel_profile()
    gpa_option('NO_YSPEC', '1')
    u_s, _, _, it_s = plan.extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma, kmax=10, want_kidx=True)
    prof_s = plan.last_kernel_profile()
    plan.close()
    _took_new_path(prof_n)
    assert not any(k in prof_s for k in NEW), sorted(prof_s)
    assert tuple(it_n) == tuple(it_s), (it_n, it_s)
    du = (u_n - u_n.mean(axis=(1, 2), keepdims=True)) - (u_s - u_s.mean(axis=(1, 2), keepdims=True))
    print('yspec driver (256, 2048): rms %.3e px, max %.3e px, iterations %s' % (np.sqrt(np.mean(du ** 2)), np.abs(du).max(), tuple(it_n)))
    assert np.sqrt(np.mean(du.astype(np.float64) ** 2)) <= F32['rms_px']
    assert np.abs(du).max() <= F32['max_px']


@pytest.mark.parametrize('dtype', DTYPES)
def test_kernel_names_of_both_paths(dtype, gpa_option):
    """case 6: the new path runs the row pre-pass, ONE pass A launch, the strips pass and the shared pass B; NO_YSPEC=1 runs
    neither new kernel.  Lists the shared pass B does not take (one candidate per x-plane) stay on the spatial path."""
    shape = (64, 2048)
    _took_new_path(_run('shared', shape, dtype)[2])
    img, kvecs, klists = yc.case('grid', shape)
    plan = _lib.Plan(shape, 16, dtype)
    plan.set_profiling(True)
    plan.sweep(img - img.mean(), kvecs[0], klists[0][::5], yc.SIGMA)     # four candidates on four x-planes
    prof = plan.last_kernel_profile()
    assert not any(k in prof for k in NEW) and 'passB_shared_kernel' not in prof, sorted(prof)
    gpa_option('NO_YSPEC', '1')
    plan.sweep(img - img.mean(), kvecs[0], klists[0], yc.SIGMA)
    prof = plan.last_kernel_profile()
    plan.close()
    assert not any(k in prof for k in NEW) and 'passB_shared_kernel' in prof and prof['passA_kernel'][0] == 1, sorted(prof)


@pytest.mark.parametrize('dtype', DTYPES)
def test_stack_equals_single_calls(dtype, gpa_option):
    """case 7: a stack of 3 frames of (64, 2048) through the batched driver equals three single calls bit for bit (both take
    the y-spectral path: the choice is made when the list is staged).  NO_LAT=1 as in
    test_gpu_hypothesis.py::test_stack_ragged_chunks_and_fallback: a single image up to 1024^2 otherwise unwraps with the
    latency-tuned kernel instantiations, whose f32 results equal the stack's to rounding only."""
    gpa_option('NO_LAT', '1')
    shape = (64, 2048)
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
    from oracle import gpa_oracle as orc
    kvecs = hex_kvecs(0.1, 7.0)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 4, 4))
    frames = np.stack([hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.2, seed=s) for s in (1, 2, 3)])
    plan = _lib.Plan(shape, 48, dtype)
    assert plan.lib.gpa_supports_batch(plan.handle)
    us, its = plan.extract_displacement_field_stack(frames, kvecs, klists, sigma, 2 * sigma, kmax=10, chunk=3)
    plan.set_profiling(True)
    for f in range(3):
        u, _, _, it = plan.extract_displacement_field(frames[f], kvecs, klists, sigma, 2 * sigma, kmax=10, want_kidx=True)
        _took_new_path(plan.last_kernel_profile())
        assert np.array_equal(us[f], u), f
        assert tuple(its[f]) == tuple(it), f
    plan.close()
