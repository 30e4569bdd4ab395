"""Host checks of the per-pixel weighted least squares (tests/lstsq_cases.py): the LAPACK restatement against the reference's own
function, the derived bound against a dtype-faithful NumPy emulation of the kernels' normal equations, the stability condition
with solve2's determinant test, and the minimum-norm claims of the oracle.  No GPU."""
import os
import re

import numpy as np
import pytest

import lstsq_cases as lc
from oracle import gpa_oracle as orc

SHAPE = (17, 70)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_fixtures_pin_lapack_to_the_reference(kset):
    """tests/golden/lstsq_<set>.npz hold what the reference's myweighed_lstsq returned (tools/make_lstsq_golden.py); the
    restatement gives the same to 1e-12 of ||x|| on the same inputs, and the inputs are the generators' own"""
    g = lc.load(kset)
    b, K, w = lc.fixture_inputs(kset)
    assert np.array_equal(g['b'], b) and np.array_equal(g['K'], K) and np.array_equal(g['w'], w)
    assert g['x'].shape == (2,) + lc.FIXTURE_SHAPE and g['K'].shape == (len(lc.KSETS[kset]), 2)
    x = lc.lapack(g['b'], g['K'], g['w'])
    d, size = lc.norm2(x - g['x']), lc.norm2(g['x'])
    assert np.all(d <= 1e-12 * size)
    zero = lc.FIXTURE_ROWS.index(('all_zero', None))
    assert np.all(g['x'][:, zero] == 0) and np.all(size[:zero] > 0)


def test_ksets_cover_every_P():
    assert sorted({len(k) for k in lc.KSETS.values()}) == [2, 3, 4, 5, 6, 7, 8]
    for name, pairs in lc.COLLINEAR.items():
        for i, j in pairs:
            assert np.array_equal(2 * lc.KSETS[name][i], lc.KSETS[name][j])
    # no other set holds a collinear pair: every 2 x 2 minor of two of its vectors is far from 0
    for name, k in lc.KSETS.items():
        for i in range(len(k)):
            for j in range(i + 1, len(k)):
                if (i, j) not in lc.COLLINEAR.get(name, []):
                    assert abs(k[i, 0] * k[j, 1] - k[i, 1] * k[j, 0]) > 0.2 * np.linalg.norm(k[i]) * np.linalg.norm(k[j]), (name, i, j)


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_coverage_and_margins(kset, dtype):
    """the graded-coverage condition of the header on the helper's own inputs, and the right-hand sides' distance from +-pi"""
    assert lc.check_coverage(kset, SHAPE, dtype) <= 0.1
    b = lc.rhs(kset, SHAPE, 'equal')
    assert np.abs(b).max() < np.pi - 0.5 > lc.SEAM_MARGIN


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_emulation_within_the_bound(kset, dtype):
    """the normal equations in the data's precision stay within the derived bound of LAPACK at every pixel of every bounded
    class (equal, every graded ratio, scaled, negative), and within the rank-1 bound on the rank-deficient ones: the reference
    alone never exceeds the bound, so a kernel that does is wrong.  Largest ratio seen: 0.6 (f32, graded 1e-3), 0.09 elsewhere."""
    for label, cls, r in lc.class_list(kset, dtype):
        if cls == 'beyond':
            continue
        c = lc.solve_case(kset, label, SHAPE, np.dtype(dtype).name)
        x, _ = lc.emulate(c['b'], c['K'], c['w'], dtype)
        assert np.isfinite(x).all()
        if cls == 'all_zero':
            assert not x.any() and not c['x_ref'].any()
            continue
        bnd = lc.bound(c['x_ref'], c['b'], c['K'], c['w'], dtype, deficient=cls in lc.DEFICIENT)
        assert lc.ratio(x, c['x_ref'], bnd) <= 1.0, (label, lc.ratio(x, c['x_ref'], bnd))


def test_scaled_weights_are_the_equal_answers():
    """the per-pixel normalisation: a pixel's weights times 1e-30 or 1e+30 give the answer of the unscaled weights to rounding,
    and in f32 w^4 neither underflows nor overflows on the way"""
    for dtype in lc.DTYPES:
        kset = 'hex3'
        c = lc.solve_case(kset, 'scaled', SHAPE, np.dtype(dtype).name)
        n = SHAPE[0] * SHAPE[1]
        s = np.asarray(lc.SCALES)[np.arange(n) % 2].reshape(SHAPE)
        w1 = c['w'] / s                     # the same weights without the factor, in float64 (not rounded again)
        x, _ = lc.emulate(c['b'], c['K'], c['w'], dtype)
        ref1 = lc.lapack(c['b'], c['K'], w1)
        assert np.isfinite(x).all() and lc.norm2(x).min() > 1e-4
        assert lc.ratio(x, ref1, lc.bound(ref1, c['b'], c['K'], w1, dtype)) <= 1.0


@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_emulation_stable_beyond_the_bound(kset):
    """f32, weights (1, r, r) with r = 1e-4 ... 1e-7, where u kappa^2 > 1 and the bound says nothing: with solve2's test
    det > 4 eps tr^2 every answer is finite and no larger than 2 max(||x_lapack||, ||x_rank1||).
    (With the constant used before, 1e-12 tr^2, the same emulation fails from r = 1e-4 on: 3.2 ... 4.1 times that size on these
    1190 pixels, 13.9 on 200 000 -- tools/lstsq_threshold.py.  The old constant is not run here.)"""
    for label, cls, r in lc.class_list(kset, np.float32):
        if cls != 'beyond':
            continue
        c = lc.solve_case(kset, label, SHAPE, 'float32')
        x, r1 = lc.emulate(c['b'], c['K'], c['w'], np.float32)
        assert lc.stability_ratio(x, c['x_ref'], c['x_r1']) <= 2.0, label
        assert r1.all()      # kappa >= 1 / r > 1 / sqrt(4 eps): every pixel keeps the dominant direction only


@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_min_norm_claims(kset):
    """rank-deficient pixels: LAPACK's answer is the minimum-norm one, r / tr, and oracle.weighted_lstsq (the comparison of every
    other GPU test of the solve) returns it to 1e-12; every weight 0 gives exactly 0"""
    for label in ('one_nonzero', 'collinear_pair', 'all_zero'):
        if label == 'collinear_pair' and kset not in lc.COLLINEAR:
            continue
        c = lc.solve_case(kset, label, SHAPE, 'float64')
        xo = orc.weighted_lstsq(c['b'], c['K'], c['w'])
        size = np.maximum(lc.norm2(c['x_ref']), 1e-300)
        assert np.all(lc.norm2(xo - c['x_ref']) <= 1e-12 * size), label
        assert np.all(lc.norm2(c['x_r1'] - c['x_ref']) <= 1e-12 * size), label
        if label == 'all_zero':
            assert not xo.any() and not c['x_ref'].any()
        else:
            assert size.min() > 1e-6


def test_oracle_is_unchanged_where_it_was_pinned():
    """on well-conditioned pixels (every graded ratio the f64 cases use) the oracle is within the f64 bound of LAPACK"""
    for kset in ('hex2', 'hex3', 'sq8'):
        for label, cls, r in lc.class_list(kset, np.float64):
            if cls not in lc.BOUND_CLASSES:
                continue
            c = lc.solve_case(kset, label, SHAPE, 'float64')
            xo = orc.weighted_lstsq(c['b'], c['K'], c['w'])
            assert lc.ratio(xo, c['x_ref'], lc.bound(c['x_ref'], c['b'], c['K'], c['w'], np.float64)) <= 1.0, (kset, label)


def test_constants_are_those_of_solve2():
    """lstsq_cases.TINY is what csrc/gpa_jacmath.h compiles and what the oracle uses"""
    src = open(os.path.join(ROOT, 'pygpa_amd', 'csrc', 'gpa_jacmath.h')).read()
    m = re.search(r'const T tiny = sizeof\(T\) == 4 \? T\(([0-9.e+-]+)\) : T\(([0-9.e+-]+)\);', src)
    assert m, 'solve2: the line of the determinant test has changed'
    assert float(m.group(1)) == lc.TINY[np.dtype(np.float32)] == 4 * np.finfo(np.float32).eps
    assert float(m.group(2)) == lc.TINY[np.dtype(np.float64)] == 4 * np.finfo(np.float64).eps
