"""The mode-by-mode measure of the weighted unwrap (tests/unwrap_modes.py) would catch a wrong kernel -- no GPU.

Each fault is planted in the emulation, in both of its precisions, at 64^2, 4 x 512, 63 x 65, 64 x 4096 and 32 x 16384, and must
read ABOVE the bound tests/test_gpu_unwrap_modes.py asserts for that class of case (precision x check: the largest asserted
ratio of tests/tolerances.py UNWRAP_MODES, at most the cap of 16 floors, which is asserted here as well); the clean emulation is
the floor itself, ratio 1, and must read below it.
  eig_one             one eigenvalue, away from the axes, off by a relative 1e-3               -> check U
  eig_shift           the axis-0 eigenvalue table shifted by one bin (the k <-> n0 - k kind)   -> U, W2, W3
  edge_last_col       the last column's edge weight from the last pixel, not the minimum       -> W2, W3
  first_row_interior  the stencil's first row treated as interior                              -> U (through alpha), W2, W3
  fwd_bin             one forward-transform output bin scaled by 1 + 1e-3                      -> check U
(A single wrong bin is judged on U, the check with the N-independent floor: after two or three weighted iterations on rows of
16384 points its reading drops to 2 .. 12 floors.  The stencil faults take their detection from kmax 2 and 3.)
Also here: properties of the reference and the measure themselves, and the self-check of the GPU cases' table."""
import numpy as np
import pytest

import tolerances as TOL
import unwrap_modes as um
from oracle import gpa_oracle as orc
from test_gpu_unwrap_modes import CASES, CHECKS

SHAPES = [(64, 64), (4, 512), (63, 65), (64, 4096), (32, 16384)]
REALS = {'f32': np.float32, 'f64': np.float64}
DETECTED_BY = {'eig_one': ('U',), 'eig_shift': CHECKS, 'edge_last_col': ('W2', 'W3'), 'first_row_interior': CHECKS, 'fwd_bin': ('U',)}


def class_bound(prec, check):
    """the largest ratio the GPU test asserts for a case of this precision and check"""
    return max(TOL.UNWRAP_MODES[c.id][check][2] for c in CASES if c.dtype == prec and check in c.checks)


_REF = {}


def reference(shape, prec, check):
    """(dx, dy, weight, kmax, phi_ref, r0, eig, floor): the reference one precision up and the clean emulation's reading, computed
    once and shared by the fault tests"""
    key = (shape, prec, check)
    if key not in _REF:
        real = REALS[prec]
        hi = um.hi_real(real)
        phi0, w = um.make_inputs(shape, 1)
        dx, dy, ww, kmax = um.check_args(phi0, w, check)
        ref, k, r0 = um.reference_pcg(dx, dy, ww, kmax, False, hi)
        assert k == kmax
        eig = um.eig_table(shape, False, hi)
        emu, k_emu, _ = um.emulate(dx, dy, ww, kmax, False, real)
        assert k_emu == kmax
        _REF[key] = (dx, dy, ww, kmax, ref, r0, eig, um.spectral_residual(emu, ref, r0, eig), um.mean_offset(emu, ref))
    return _REF[key]


def test_class_bounds_respect_the_cap():
    for prec in REALS:
        for check in CHECKS:
            assert 1.0 < class_bound(prec, check) <= TOL.UNWRAP_MODES_CAP == 16.0


@pytest.mark.parametrize('prec', list(REALS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_clean_emulation_is_the_floor(shape, prec):
    """the clean emulation reads ratio 1 by construction -- below every asserted bound -- and its floor is what the precision
    allows: check U within 64 eps at every shape (1.0e-6 .. 2.1e-6 in f32: it does not grow with N), the weighted checks
    within 1024 eps (up to 4.8e-5 in f32 on rows of 16384 points); the free mean far below the same figure"""
    eps = float(np.finfo(REALS[prec]).eps)
    for check in CHECKS:
        floor, mean = reference(shape, prec, check)[7:]
        print('floor', shape, prec, check, '%.3e' % floor, 'mean %.1e' % mean)
        assert 0 < floor < (64 if check == 'U' else 1024) * eps
        assert mean < floor
        assert 1.0 < class_bound(prec, check)


@pytest.mark.parametrize('prec', list(REALS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('fault', um.FAULTS)
def test_planted_fault_reads_above_the_asserted_bound(fault, shape, prec):
    real = REALS[prec]
    for check in DETECTED_BY[fault]:
        dx, dy, ww, kmax, ref, r0, eig, floor, _ = reference(shape, prec, check)
        phi, k, _ = um.emulate(dx, dy, ww, kmax, False, real, fault=fault)
        ratio = um.spectral_residual(phi, ref, r0, eig) / floor
        print('fault', fault, shape, prec, check, 'reads %.3g floors' % ratio)
        assert k == kmax
        assert ratio > TOL.UNWRAP_MODES_CAP, (fault, shape, prec, check, ratio)
        assert ratio > class_bound(prec, check)


@pytest.mark.parametrize('compat', [False, True])
@pytest.mark.parametrize('shape', [(20, 31), (24, 24)])
def test_reference_is_the_oracles_loop(shape, compat):
    """reference_pcg in float64 against oracle/gpa_oracle.py:unwrap_prediff on the oracle's own kind of input (wrapping
    differences, kmax 12): same iterates to rounding, same count -- and the eigenvalue table is the oracle's cos form"""
    rng = np.random.default_rng(5)
    psi = orc.wrap_to_pi(rng.normal(size=shape) * 2.0)
    w = 0.3 + rng.random(shape)
    dx, dy = np.diff(psi, axis=1), np.diff(psi, axis=0)
    want, k_want = orc.unwrap_prediff(dx, dy, w, kmax=12, compat=compat, return_iters=True)
    got, k, r0 = um.reference_pcg(dx, dy, w, 12, compat, np.float64)
    assert k == k_want == 12
    assert np.abs(got - want).max() < 1e-10 * np.abs(want).max()
    eig = um.eig_table(shape, compat, np.float64)
    assert np.abs(eig - orc.poisson_scale(shape, compat=compat)).max() < 1e-14


def test_inputs_are_exact_in_both_precisions():
    phi0, w = um.make_inputs((63, 65), 3)
    dx, dy = um.diffs(phi0)
    assert phi0.dtype == np.float32 and w.dtype == np.float32
    assert np.abs(phi0).max() <= 0.7 and w.min() >= 0.2 and w.max() <= 1.0
    for d in (dx, dy):
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d) and np.abs(d).max() < 1.4 < np.pi


def test_unweighted_single_iteration_is_an_exact_poisson_solve():
    """check U: phi0 minus its mean, to the reference's own rounding"""
    phi0, _ = um.make_inputs((48, 80), 2)
    dx, dy = um.diffs(phi0)
    phi, k, _ = um.reference_pcg(dx, dy, None, 1, False, np.longdouble)
    p = phi0.astype(np.longdouble)
    assert k == 1 and float(np.abs(phi - (p - p.mean())).max()) < 1e-15
