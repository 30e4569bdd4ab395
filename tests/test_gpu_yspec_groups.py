"""GPU tests of the grouped y-spectral pass A: a workgroup of passA_kernel loads its tile of Yhat once and filters
it for up to YSPEC_GROUP planes that read the tile's block.  The arithmetic of one (plane, tile) does not depend on the
schedule, so everything downstream is equal BIT FOR BIT between YSPEC_GROUP=1 (one plane per workgroup, the schedule before the
groups), caps that cut the blocks' plane lists unevenly, and the default.  No oracle here: equality with the one-plane schedule
is the whole claim, the oracle checks of the path are tests/test_gpu_yspec_sweep.py.

The three-peak hex lists give blocks read by 12 and by 4 planes on 2048-point rows (an odd band rotation splits register pairs
there) and by 12, 8 and 4 planes on 4096-point rows -- asserted from the host function (tests/host/yspec_groups_check.cpp), so
that the test cannot pass on uniform groups; a cap of 3 leaves a group of one plane behind every block of 4."""
import numpy as np
import pytest

from pygpa_amd import _lib
import yspec_cases as yc
from test_yspec_groups_host import build_exe, groups_of

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
CAPS = ['1', '3', '4', None]


def _hex_case(shape, seed=4):
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
    from oracle import gpa_oracle as orc
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.2, seed=seed)
    kw, sigma, _ = orc.derive_params(kvecs)
    return img, kvecs, np.stack(explicit_klists(kvecs, kw, 4, 4)), sigma


def _one_launch_each(prof):
    for k in ('rowfft_kernel', 'passA_kernel', 'passA_strips_kernel'):
        assert k in prof and prof[k][0] == 1, (k, prof)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,sizes', [((256, 2048), {4, 12}), ((64, 4096), {4, 8, 12})])
def test_fused_driver_equal_under_every_cap(shape, sizes, dtype, gpa_option, tmp_path):
    """lock-ins, winner indices and u of the fused driver (3 peaks x 4 x 4, kmax 2) under YSPEC_GROUP = 1, 3, 4 and the default"""
    img, kvecs, klists, sigma = _hex_case(shape)
    f32 = dtype is np.float32
    exe = build_exe(tmp_path)
    if exe is not None:
        rot = [yc.band_rotation(kl, sigma, f32)[0] for kl in klists]
        lg = 11 if shape[1] == 2048 else 12
        counts = {c for _, c in groups_of(exe, 6 if f32 else 8, 16, rot, lg)[1]}
        assert counts == sizes, counts
        assert 1 in {c for _, c in groups_of(exe, 6 if f32 else 8, 3, rot, lg)[1]}
    ref = None
    for cap in CAPS:
        gpa_option('YSPEC_GROUP', cap)
        plan = _lib.Plan(shape, 48, dtype)
        plan.set_profiling(True)
        u, lock, kidx, it = plan.extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma, kmax=2, want_lockins=True,
                                                            want_kidx=True)
        prof = plan.last_kernel_profile()
        plan.close()
        _one_launch_each(prof)
        if ref is None:
            ref = (u, lock, kidx, tuple(it))
            continue
        assert np.array_equal(lock, ref[1]), cap
        assert np.array_equal(kidx, ref[2]), cap
        assert np.array_equal(u, ref[0]), cap
        assert tuple(it) == ref[3], cap


@pytest.mark.parametrize('dtype', DTYPES)
def test_benchmark_instantiation_equal_under_every_cap(dtype, gpa_option):
    """plan.sweep of the single-peak 'grid' case at (4096, 2048): the 4096-point x axis takes the benchmark's instantiation of
    the kernel (f32: four columns per workgroup, four tiles per 128-byte line, tile in registers) and its plane rotation"""
    shape = (4096, 2048)
    img, kvecs, klists = yc.case('grid', shape)
    img0 = img - img.mean()
    ref = None
    for cap in ('1', '3', None):
        gpa_option('YSPEC_GROUP', cap)
        plan = _lib.Plan(shape, 16, dtype)
        plan.set_profiling(True)
        lock, kidx, _ = plan.sweep(img0, kvecs[0], klists[0], yc.SIGMA)
        prof = plan.last_kernel_profile()
        plan.close()
        _one_launch_each(prof)
        if ref is None:
            ref = (lock, kidx)
            continue
        assert np.array_equal(lock, ref[0]), cap
        assert np.array_equal(kidx, ref[1]), cap


def test_cap_is_read_when_a_sweep_is_staged(gpa_option):
    """one plan, the same list: changing YSPEC_GROUP between two calls re-cuts the groups (same bits either way)"""
    shape = (64, 2048)
    img, kvecs, klists = yc.case('shared', shape)
    plan = _lib.Plan(shape, 32, np.float32)
    out = []
    for cap in ('1', None, '5'):
        gpa_option('YSPEC_GROUP', cap)
        _, lock, kidx, _ = plan.extract_displacement_field(img, kvecs, klists, yc.SIGMA, 2 * yc.SIGMA, kmax=2, want_lockins=True,
                                                           want_kidx=True)
        out.append((lock, kidx))
    plan.close()
    for lock, kidx in out[1:]:
        assert np.array_equal(lock, out[0][0]) and np.array_equal(kidx, out[0][1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_stack_equals_single_calls(dtype, gpa_option):
    """a stack of 2 frames of (64, 2048) through the batched driver (blockIdx.z = frame) equals the single calls bit for bit
    under the default cap; NO_LAT=1 as in tests/test_gpu_yspec_sweep.py::test_stack_equals_single_calls"""
    gpa_option('NO_LAT', '1')
    shape = (64, 2048)
    _, kvecs, klists, sigma = _hex_case(shape)
    frames = np.stack([_hex_case(shape, seed=s)[0] for s in (1, 2)])
    plan = _lib.Plan(shape, 48, dtype)
    assert plan.lib.gpa_supports_batch(plan.handle)
    us, its = plan.extract_displacement_field_stack(frames, kvecs, klists, sigma, 2 * sigma, kmax=10, chunk=2)
    plan.set_profiling(True)
    for f in range(2):
        u, _, _, it = plan.extract_displacement_field(frames[f], kvecs, klists, sigma, 2 * sigma, kmax=10, want_kidx=True)
        _one_launch_each(plan.last_kernel_profile())
        assert np.array_equal(us[f], u), f
        assert tuple(its[f]) == tuple(it), f
    plan.close()
