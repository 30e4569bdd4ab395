#!/usr/bin/env python
"""Fixtures of the phases -> Jacobian -> properties functions: runs the reference's own phases2J, calc_props_from_phases and
phys_props_from_Jac (pyGPA/property_extract.py:39-52, :181-217, :258-278, imported through oracle.make_golden._install_stubs)
on the cases of tests/jac_cases.py and writes tests/golden/jac_*.npz.

    python tools/make_jac_golden.py [--only NAME ...]

Nothing of the reference is replaced: myweighed_lstsq, wrapToPi, np.gradient and the LAPACK SVD are its own code path.
Stored per case: phases, weights, kvecs, nmperpixel, J = phases2J, props = calc_props_from_phases, and phys_props_from_Jac of
eye(2) + J without and with diff.  Data only.  The script asserts what the tests rely on (the seam margin and the share of
differences that wrap, jac_cases.SEAM_MARGIN / WRAP_SHARE); if a seed misses a condition, change the seed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import jac_cases as jc  # noqa: E402


def import_property_extract():
    from oracle.make_golden import _install_stubs, REF
    _install_stubs()
    import matplotlib
    matplotlib.use('Agg')
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pyGPA.property_extract as pe
    return pe


def make(pe, name):
    kvecs, phases, weights, nm = jc.phase_inputs(name)
    margin, share = jc.seam_margin_and_share(phases)
    wrapped = jc.CASES[name][2]
    assert margin >= jc.SEAM_MARGIN, (name, margin)
    assert share >= jc.WRAP_SHARE if wrapped else share == 0, (name, share)
    J = pe.phases2J(kvecs, phases, weights, nm)
    props = np.asarray(pe.calc_props_from_phases(kvecs, phases, weights, nm))
    Jac = np.eye(2) + J
    out = dict(kvecs=kvecs, phases=phases, weights=weights, nmperpixel=np.float64(nm), J=J, props=props,
               phys=np.asarray(pe.phys_props_from_Jac(Jac, poisson_ratio=jc.POISSON)),
               phys_diff=np.asarray(pe.phys_props_from_Jac(Jac, refangle=3.0, refscale=2.0, diff=True, poisson_ratio=jc.POISSON)))
    assert all(np.isfinite(v).all() for v in out.values()), name
    dev = np.abs(jc.phases2J_np(kvecs, phases, weights, nm) - J).max() / np.abs(J).max()
    kap = props[3]
    print('%-18s margin %.3f rad, %.1f %% of the differences wrap, max|J| %.3g, restatement - reference %.2e max|J|, '
          'kappa %.4g ... %.4g (%d of %d pixels above %g)' % (name, margin, 100 * share, np.abs(J).max(), dev, kap.min(), kap.max(),
                                                             (kap > jc.KAPPA_MIN).sum(), kap.size, jc.KAPPA_MIN))
    path = os.path.join(jc.GOLDEN, 'jac_%s.npz' % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    pe = import_property_extract()
    for name in jc.CASES:
        if a.only is None or name in a.only:
            make(pe, name)


if __name__ == '__main__':
    main()
