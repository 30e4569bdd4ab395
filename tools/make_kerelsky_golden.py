#!/usr/bin/env python
"""Fixtures of the per-pixel Kerelsky fits: runs the reference's own Kerelsky_J and Kerelsky_Jac (pyGPA/property_extract.py:707-883,
imported through oracle.make_golden._install_stubs) on the cases of tests/kerelsky_cases.py and writes tests/golden/kerelsky_*.npz.

    python tools/make_kerelsky_golden.py [--only NAME ...]

REPLACED, in this file only, before the reference module is imported:
  latticegen.transformations.rotation_matrix / strain_matrix / a_0_to_r_k and latticegen.generate_ks, which are not available,
      by their restatements in kerelsky_cases (a declared restatement);
  dask.array.as_gufunc  by a plain loop over the leading axes that calls the reference's worker once per pixel.
scipy.optimize.least_squares, the residual Jac_fit_diff, the two starts and the retry rule are the reference's own code path.

Each case is fitted twice: with the reference's defaults (lq_kwargs = {'max_nfev': 50}) and with xtol = ftol = gtol = 1e-15.  Stored
are the inputs, both results, both global fits, and both costs as the reference's Jac_fit_diff evaluates them.  Data only.
The script asserts what the tests rely on (kerelsky_cases.fixture_promises); if a seed misses a condition, change the seed.
"""
import argparse
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kerelsky_cases as kc  # noqa: E402


def _loop_gufunc(**kw):
    def deco(f):
        def run(JacA0, refest, lq_kwargs):
            JacA0 = np.asarray(JacA0)
            out = np.empty(JacA0.shape[:-2] + (4,))
            for idx in np.ndindex(*JacA0.shape[:-2]):
                out[idx] = f(JacA0[idx], refest, lq_kwargs)
            return out
        return run
    return deco


def import_property_extract():
    from oracle.make_golden import _install_stubs, REF
    _install_stubs()
    import matplotlib
    matplotlib.use('Agg')
    lgt = sys.modules['latticegen.transformations']
    lgt.rotation_matrix, lgt.strain_matrix, lgt.a_0_to_r_k = kc.rotation_matrix, kc.strain_matrix, kc.a_0_to_r_k
    sys.modules['latticegen'].generate_ks = kc.generate_ks
    sys.modules['dask.array'].as_gufunc = _loop_gufunc
    sys.modules['dask.array'].asarray = lambda a, **k: np.asarray(a)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pyGPA.property_extract as pe
    return pe


def ref_costs(pe, X, A):
    return np.array([0.5 * np.sum(pe.Jac_fit_diff(x, a) ** 2) for x, a in zip(X.reshape(-1, 4), A.reshape(-1, 2, 2))]).reshape(X.shape[:-1])


def make_field(pe, name):
    J, kvecs = kc.field_inputs(name)
    A0 = kc.a0_and_start(kvecs, kc.NMPERPIXEL, kc.A_0)[0]
    A = A0 + A0 @ J          # what the reference fits
    out = dict(J=J, kvecs=kvecs, nmperpixel=np.float64(kc.NMPERPIXEL), a_0=np.float64(kc.A_0), A0=A0)
    for tag, kw in (('default', kc.DEFAULT), ('tight', kc.TIGHT)):
        X, refest = pe.Kerelsky_J(J, kvecs, nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, lq_kwargs=dict(kw))
        out['X_' + tag], out['refest_' + tag], out['cost_' + tag] = X, np.asarray(refest), ref_costs(pe, X, A)
    root = kc.root_pixels(out)
    out['root_cost_max'] = np.float64(out['cost_default'][root].max())
    kc.fixture_promises(name, out)
    assert np.abs(kc.cost(out['X_default'], kc.form_A(A0, J)) - out['cost_default']).max() <= 1e-9 * (1 + out['cost_default'].max())
    rest = ~root
    print('%-14s root pixels %d / %d (%.0f %%)  largest default cost on them %.2e  on the rest: cost %.3g ... %.3g, default - tight <= %.2e, theta = 0 on %d' %
          (name, root.sum(), root.size, 100 * root.mean(), out['root_cost_max'],
           out['cost_default'][rest].min() if rest.any() else 0, out['cost_default'][rest].max() if rest.any() else 0,
           (out['cost_default'][rest] - out['cost_tight'][rest]).max() if rest.any() else 0, int((out['X_default'][..., 0] == 0).sum())))
    print('%-14s default vs tight on root pixels: %s' % ('', kc.param_dev(out['X_default'][root], out['X_tight'][root])))
    np.savez_compressed(os.path.join(kc.GOLDEN, 'kerelsky_%s.npz' % name), **out)


def make_ksets(pe):
    import scipy.optimize
    sets = kc.kset_inputs()
    out = dict(kvecs=np.stack([s[0] for s in sets]), sort=np.array([s[1] for s in sets]), symmetric=np.array([s[2] == 'symmetric' for s in sets]),
               nmperpixel=np.float64(kc.NMPERPIXEL), a_0=np.float64(kc.A_0))
    for tag in ('default', 'tight'):
        pe.least_squares = scipy.optimize.least_squares if tag == 'default' else functools.partial(
            scipy.optimize.least_squares, xtol=1e-15, ftol=1e-15, gtol=1e-15)
        X = np.stack([pe.Kerelsky_Jac(k, nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, sort=s, reference=r) for k, s, r in sets])
        out['X_' + tag] = X
        A = np.stack([kc.a0_and_start(k, kc.NMPERPIXEL, kc.A_0, sort=s)[0] for k, s, _ in sets])
        plain = X.copy()
        plain[out['symmetric'], 3] -= plain[out['symmetric'], 0] / 2
        out['cost_' + tag] = ref_costs(pe, plain, A)
    pe.least_squares = scipy.optimize.least_squares
    out['A0'] = A
    truth = np.array(kc.KSET_X + [e['x'] for e in kc.KSET_EXTRA])
    print('ksets: tight cost <= %.2e, default cost <= %.2e; tight vs generating x: %s; default vs tight %s' %
          (out['cost_tight'].max(), out['cost_default'].max(), kc.param_dev(plain, truth), kc.param_dev(out['X_default'], out['X_tight'])))
    assert out['cost_tight'].max() <= kc.ROOT_COST and np.isfinite(out['X_default']).all()
    np.savez_compressed(os.path.join(kc.GOLDEN, 'kerelsky_%s.npz' % kc.KSETS), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    pe = import_property_extract()
    for name in kc.FIELD_CASES:
        if a.only is None or name in a.only:
            make_field(pe, name)
    if a.only is None or kc.KSETS in a.only:
        make_ksets(pe)


if __name__ == '__main__':
    main()
