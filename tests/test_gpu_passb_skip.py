"""The row-wise skip test of the shared pass B: a candidate whose spectral bound proves that it cannot win a pixel
of its rows is dropped before its transform.  Nothing may change: every case runs with the test (default) and without it
(NO_PB_SKIP=1) through Plan.sweep (compensated winners of one peak) and through the fused driver (raw winners of three peaks)
and the outputs are compared bit for bit -- lock-ins, kidx, u, iteration counts.  Plan.last_passb_skips() says how many
(row, candidate) pairs the kernel skipped; tools/passb_skip_model.py says how many the bound allows.

Which instantiations carry the test: all f32 ones, and the f64 ones of the y-spectral form (rows of 2048 / 4096 points).  The
f64 kernel of zero-padded rows has no registers for it (gpa_passb_shared.hip): there the count is 0 and only equality is checked."""
import os
import sys

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import passb_skip_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SHAPES = [(64, 2048), (64, 4096), (48, 1500)]
GRIDS = [(4, 4), (4, 2)]
KVECS = hex_kvecs(0.1, 7.0)
KW, SIGMA, _ = orc.derive_params(KVECS)


def has_test(shape, dtype):
    return dtype is np.float32 or shape[1] in (2048, 4096)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def run_both(shape, dtype, img, klists, gpa_option, peak=1, kvecs=KVECS):
    """sweep of one peak and the fused driver of all three, with the test and without: asserts bit equality, returns the
    (skipped, visited) counts of the sweep with the test, of the sweep without it, and of the driver with it"""
    img0 = img - img.mean()
    plan = _lib.Plan(shape, 3 * len(klists[0]), dtype)
    plan.set_profiling(True)
    out = {}
    for sw in (None, '1'):
        gpa_option('NO_PB_SKIP', sw)
        lock, kidx, _ = plan.sweep(img0, kvecs[peak], klists[peak], SIGMA)
        assert 'passB_shared_kernel' in plan.last_kernel_profile()
        cnt = plan.last_passb_skips()
        u, lk, kd, it = plan.extract_displacement_field(img, kvecs, np.stack(klists), SIGMA, 4, kmax=10, want_kidx=True)
        dcnt = plan.last_passb_skips()
        u2, lk2, kd2, it2 = plan.extract_displacement_field(img, kvecs, np.stack(klists), SIGMA, 4, kmax=10, want_kidx=True,
                                                            want_lockins=True)
        out[sw] = (lock, kidx, u, kd, list(it), lk2, kd2, u2, list(it2), cnt, dcnt)
    gpa_option('NO_PB_SKIP', None)
    plan.close()
    a, b = out[None], out['1']
    names = ('sweep lock-in', 'sweep kidx', 'driver u (raw winners)', 'driver kidx (raw)', 'iterations', 'driver lock-ins', 'driver kidx',
             'driver u', 'iterations')
    for name, va, vb in zip(names, a, b):
        assert (va == vb) if isinstance(va, list) else (va.shape == vb.shape and bits(va) == bits(vb)), name
    assert b[9][0] == 0 and b[10][0] == 0, 'NO_PB_SKIP=1 must skip nothing'
    assert a[9][1] == b[9][1] == shape[0] * len(klists[peak])
    assert a[10][1] == 3 * shape[0] * len(klists[0])
    return a[9], b[9], a[10]


_MODEL = {}


def model_of(key, img, klist, kref):
    """the NumPy model of one image and list, computed once for the precisions that share it"""
    if key not in _MODEL:
        m = model.skip_model(img - img.mean(), klist, kref, SIGMA)
        _MODEL[key] = (m['skipped'].copy(), m['wins'].copy())
    return _MODEL[key]


def carriers(shape, kvecs=KVECS, noise=0.01, seed=3):
    x = np.arange(shape[0])[:, None]
    y = np.arange(shape[1])[None, :]
    img = sum(np.cos(2 * np.pi * (k[0] * x + k[1] * y)) for k in kvecs)
    return img + noise * np.random.default_rng(seed).normal(size=shape)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_clean_carriers_skip_what_the_model_predicts(shape, grid, dtype, gpa_option):
    """(a) one clean carrier per peak at the reference vector plus 1 % noise: equal bits, and the kernel skips at least half of
    the (row, candidate) pairs the NumPy model (|X_k| magnitudes, f64) finds skippable for the peak that is swept; without the
    test it skips none"""
    klists = explicit_klists(KVECS, KW, *grid)
    img = carriers(shape)
    with_test, without, _ = run_both(shape, dtype, img, klists, gpa_option)
    predicted = int(model_of(('carriers', shape, grid), img, klists[1], KVECS[1])[0].sum())
    print('skipped %d of %d visited, model %d' % (with_test[0], with_test[1], predicted))
    assert predicted > 0
    if has_test(shape, dtype):
        assert with_test[0] > 0 and with_test[0] >= 0.5 * predicted, (with_test, predicted)
    else:
        assert with_test[0] == 0
    assert without[0] == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_bands_where_every_candidate_wins_somewhere(shape, grid, dtype, gpa_option):
    """(b) vertical bands of columns, band j carrying candidate j of every peak at equal amplitude: every candidate wins somewhere
    on every row, the model predicts no skip at all, and the results are equal"""
    klists = explicit_klists(KVECS, KW, *grid)
    K = len(klists[0])
    x = np.arange(shape[0])[:, None]
    y = np.arange(shape[1])[None, :]
    img = np.zeros(shape)
    for p in range(3):
        for j in range(K):
            sl = slice(j * shape[1] // K, (j + 1) * shape[1] // K)
            img[:, sl] += np.cos(2 * np.pi * (klists[p][j][0] * x + klists[p][j][1] * y[:, sl]))
    skipped, wins = model_of(('bands', shape, grid), img, klists[1], KVECS[1])
    assert not skipped.any() and wins.all()
    with_test, _, _ = run_both(shape, dtype, img, klists, gpa_option)
    assert with_test[0] == 0


def seam_burst(shape, grid, width=2, amp=4.0, background=0.3, noise=0.001):
    """the image of case (c): every peak's list (and reference vector) is shifted along y so that its LAST candidate sits at
    wy n1 = integer + 1/2; that candidate's carrier lives only in the `width` columns either side of the row seam, the candidate
    visited first carries a weak background everywhere.  Across the seam the burst's carrier jumps by pi: in the circular part
    g_b (*) T its two halves cancel, in the lock-in (circular part + Hankel correction) they add."""
    n0, n1 = shape
    klists = [kl.copy() for kl in explicit_klists(KVECS, KW, *grid)]
    kvecs = KVECS.copy()
    for p in range(3):
        wy = klists[p][-1][1]
        delta = (np.floor(wy * n1) + 0.5) / n1 - wy
        klists[p][:, 1] += delta
        kvecs[p, 1] += delta
    x = np.arange(n0)[:, None]
    y = np.arange(n1)[None, :]
    edge = ((y < width) | (y >= n1 - width)).astype(np.float64)
    img = np.zeros(shape)
    for p in range(3):
        ks = klists[p][-1]
        kb = klists[p][model.visiting_order(klists[p], kvecs[p])[0]]
        img += amp * edge * np.cos(2 * np.pi * (ks[0] * x + ks[1] * y)) + background * np.cos(2 * np.pi * (kb[0] * x + kb[1] * y))
    img += noise * np.random.default_rng(5).normal(size=shape)
    return img, klists, kvecs


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_end_correction_decides(shape, grid, dtype, gpa_option):
    """(c) a strong carrier that is not periodic in n1 (wy n1 = integer + 1/2) and lives only in the two columns either side of
    the seam, over a weak background: on some rows the bound of the circular part ALONE lies below the running best -- the
    model, which leaves the Hankel correction out, marks the pair skippable -- while the candidate wins pixels within E of the
    row ends through the correction.  The premise is asserted with the model first ((skipped & wins) is not empty for the peak
    that is swept); a kernel whose test ignored or underestimated the correction would skip those rows and lose their winners.
    Equal bits with and without the test."""
    img, klists, kvecs = seam_burst(shape, grid)
    key = ('seam', shape, grid)
    if key not in _MODEL:
        m = model.skip_model(img - img.mean(), klists[0], kvecs[0], SIGMA)
        _MODEL[key] = (m['skipped'].copy(), m['wins'].copy())
    skipped, wins = _MODEL[key]
    decided = skipped & wins
    print('rows x candidates the end correction decides: %d (model skips %d)' % (int(decided.sum()), int(skipped.sum())))
    assert decided.any(), 'the image does not exercise the end correction'
    run_both(shape, dtype, img, klists, gpa_option, peak=0, kvecs=kvecs)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_zero_row_nan_row_and_zero_image(shape, grid, dtype, gpa_option):
    """(d) a row of zeros, a row containing a NaN, and an image of zeros (winner -1 everywhere): equal bits; a NaN in the bound
    means "run\""""
    klists = explicit_klists(KVECS, KW, *grid)
    base = hex_moire(shape, KVECS, gaussian_bump_displacement(shape), noise=0.1, seed=11)
    zero_row = base.copy()
    zero_row[shape[0] // 3, :] = 0.0
    run_both(shape, dtype, zero_row, klists, gpa_option)
    zeros = np.zeros(shape)
    plan = _lib.Plan(shape, len(klists[0]), dtype)
    nan_row = base - base.mean()
    nan_row[shape[0] // 2, shape[1] // 5] = np.nan
    for img0 in (nan_row, zeros):
        res = []
        for sw in (None, '1'):
            gpa_option('NO_PB_SKIP', sw)
            lock, kidx, _ = plan.sweep(img0, KVECS[0], klists[0], SIGMA)
            res.append((lock, kidx))
        gpa_option('NO_PB_SKIP', None)
        assert bits(res[0][0]) == bits(res[1][0]) and np.array_equal(res[0][1], res[1][1])
        if img0 is zeros:
            assert np.all(res[0][1] == -1) and np.all(res[0][0] == 0)
    plan.close()


def _seeds(carrier, gpa_option):
    """20 seeds of unit noise (plus `carrier` times the peak's clean carrier) at (64, 2048), f32, one peak of 16 candidates: asserts
    equal bits with and without the test, returns the pairs skipped per seed"""
    shape = (64, 2048)
    klist = explicit_klists(KVECS, KW, 4, 4)[2]
    x = np.arange(shape[0])[:, None]
    y = np.arange(shape[1])[None, :]
    plan = _lib.Plan(shape, 16, np.float32)
    plan.set_profiling(True)
    skipped = []
    for seed in range(20):
        img0 = np.random.default_rng(1000 + seed).normal(size=shape) + carrier * np.cos(2 * np.pi * (KVECS[2][0] * x + KVECS[2][1] * y))
        img0 -= img0.mean()
        res = []
        for sw in (None, '1'):
            gpa_option('NO_PB_SKIP', sw)
            lock, kidx, _ = plan.sweep(img0, KVECS[2], klist, SIGMA)
            res.append((lock, kidx))
            if sw is None:
                skipped.append(plan.last_passb_skips()[0])
        gpa_option('NO_PB_SKIP', None)
        assert bits(res[0][0]) == bits(res[1][0]) and np.array_equal(res[0][1], res[1][1]), seed
    plan.close()
    return skipped


def test_noise_only_images_twenty_seeds(gpa_option):
    """(e) 20 seeds of noise without any carrier at (64, 2048), f32: equal bits.  (The bound allows no skip on such images -- the
    model finds none --, so this is the "never skip wrongly on noise" half; the next test is the half where the test does skip.)"""
    skipped = _seeds(0.0, gpa_option)
    print('noise only: %d pairs skipped over 20 seeds' % sum(skipped))


def test_weak_carrier_in_noise_twenty_seeds(gpa_option):
    """(e'), beside the issue's cases: the same 20 noise fields with the peak's carrier at amplitude 1 under them (one to one per
    pixel; the model finds about 390 of the 1024 pairs skippable with |X_k|): the kernel does skip on every seed, decisions
    made close to the noise floor, and the bits stay equal"""
    skipped = _seeds(1.0, gpa_option)
    print('carrier 1.0 in unit noise: pairs skipped per seed', skipped)
    assert min(skipped) > 0, skipped
