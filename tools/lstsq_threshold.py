#!/usr/bin/env python
"""Chooses the multiple m of solve2's determinant test, det > m eps tr^2 (csrc/gpa_jacmath.h): the smallest power of two for
which the dtype-faithful emulation of tests/lstsq_cases.py meets the stability condition
    every component finite,  ||x|| <= 2 max(||x_lapack||, ||x_rank1||)
on every pixel of the f32 `beyond` class (one weight 1, the others r U(0.5, 1), r = 1e-4 ... 1e-7), N pixels per ratio and
k-vector set, and returns LAPACK's minimum-norm answer within the rank-1 bound on the exactly rank-deficient classes
(`one_nonzero`, `collinear_pair`) in both precisions.  Prints, per multiple, the largest ratio met and the share of pixels that take the rank-1 branch.

    python tools/lstsq_threshold.py [--pixels 200000]

The LAPACK side is a batched float64 SVD with gelsd's cut (singular values below eps64 max(P, 2) smax count as zero), which is
what np.linalg.lstsq(rcond=None) does per pixel; tests/test_lstsq_host.py holds the two equal on the test's cases.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import lstsq_cases as lc  # noqa: E402


def lapack_batched(b, K, w):
    P = len(K)
    M = np.moveaxis(w, 0, -1)[..., :, None] * K
    rhs = np.moveaxis(w * b, 0, -1)
    U, s, Vt = np.linalg.svd(M, full_matrices=False)
    keep = s > np.finfo(np.float64).eps * max(P, 2) * s[..., :1]
    c = np.einsum('...pk,...p->...k', U, rhs) * np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)
    return np.moveaxis(np.einsum('...kc,...k->...c', Vt, c), -1, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pixels', type=int, default=200000)
    a = ap.parse_args()
    shape = (1, a.pixels)
    dt = np.float32
    cases = []
    for ks in lc.KSET_NAMES:
        K = lc.kmat(ks, dt)
        for r in lc.BEYOND:
            b = lc.rounded(lc.rhs(ks, shape, r), dt)
            w = lc.rounded(lc.weights('beyond', ks, shape, r), dt)
            cases.append((ks, r, b, K, w, lapack_batched(b, K, w), lc.rank1(b, K, w)))
    # exactly rank-deficient pixels, both precisions: error against LAPACK's minimum-norm answer over the rank-1 bound
    deficient = []
    for d in (np.float32, np.float64):
        for ks in lc.KSET_NAMES:
            for cls in ('one_nonzero', 'collinear_pair'):
                if cls == 'collinear_pair' and ks not in lc.COLLINEAR:
                    continue
                K = lc.kmat(ks, d)
                b = lc.rounded(lc.rhs(ks, shape, cls), d)
                w = lc.rounded(lc.weights(cls, ks, shape), d)
                x_ref = lc.rank1(b, K, w)       # = LAPACK's answer on these classes to 1e-15 (tests/test_lstsq_host.py)
                deficient.append((d, b, K, w, x_ref, lc.bound(x_ref, b, K, w, d, deficient=True)))
    chosen = None
    for m, name in [(None, '1e-12')] + [(m, '%d eps' % m) for m in (1, 2, 4, 8, 16, 32)]:
        tiny = lc.TINY_F32_BEFORE if m is None else m * lc.EPS[np.dtype(dt)]
        dworst = {np.float32: 0.0, np.float64: 0.0}
        for d, b, K, w, x_ref, bnd in deficient:
            t = (lc.TINY_F32_BEFORE if d is np.float32 else 1e-28) if m is None else m * lc.EPS[np.dtype(d)]
            dworst[d] = max(dworst[d], lc.ratio(lc.emulate(b, K, w, d, tiny=t)[0], x_ref, bnd))
        worst, where, share = 0.0, None, []
        for ks, r, b, K, w, x_ref, x_r1 in cases:
            x, r1 = lc.emulate(b, K, w, dt, tiny=tiny)
            q = lc.stability_ratio(x, x_ref, x_r1)
            share.append(r1.mean())
            if q > worst:
                worst, where = q, (ks, r)
        ok = worst <= 2.0 and max(dworst.values()) <= 1.0
        print('tiny = %-7s exact rank 1: error / bound = %.3g (f32), %.3g (f64; first line: 1e-28)' % (name, dworst[np.float32], dworst[np.float64]))
        print('tiny = %-7s largest ||x|| / max(||x_lapack||, ||x_rank1||) = %8.3f at %s; rank-1 share %.3f ... %.3f  %s' %
              (name, worst, where, min(share), max(share), 'passes' if ok else 'FAILS'))
        if ok and chosen is None and name != '1e-12':
            chosen = name
    print('smallest passing multiple:', chosen)


if __name__ == '__main__':
    main()
