#!/usr/bin/env python
"""Fixtures of the per-pixel weighted least squares: runs the reference's own myweighed_lstsq (pyGPA/geometric_phase_analysis.py:
98-113, imported through oracle.make_golden._import_reference, numba's njit / prange replaced by plain Python as there) on the
inputs of tests/lstsq_cases.fixture_inputs and writes tests/golden/lstsq_<set>.npz, one per k-vector set (P = 2 ... 8).

    python tools/make_lstsq_golden.py [--only SET ...]

Stored are b, K, w and the reference's x, numeric arrays only.  tests/test_lstsq_host.py holds lstsq_cases.lapack equal to x on
these inputs; the script asserts the same before it writes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import lstsq_cases as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--check', action='store_true', help='write nothing: compare with the committed arrays bit for bit')
    a = ap.parse_args()
    bad = 0
    from oracle.make_golden import _import_reference
    GPA, _ = _import_reference()
    for kset in lc.KSET_NAMES:
        if a.only is not None and kset not in a.only:
            continue
        b, K, w = lc.fixture_inputs(kset)
        x = GPA.myweighed_lstsq(b, K, w)
        mine = lc.lapack(b, K, w)
        dev = float((lc.norm2(mine - x) / np.maximum(lc.norm2(x), 1e-300)).max())
        assert dev <= 1e-12, (kset, dev)
        path = os.path.join(lc.GOLDEN, 'lstsq_%s.npz' % kset)
        if a.check:
            old = lc.load(kset)
            same = all(old[k].dtype == v.dtype and old[k].tobytes() == v.tobytes() for k, v in dict(b=b, K=K, w=w, x=x).items())
            print('%-5s %s' % (kset, 'identical arrays' if same else 'DIFFERS'))
            bad += not same
            continue
        np.savez_compressed(path, b=b, K=K, w=w, x=x)
        print('%-5s P = %d  %d pixels  restatement within %.1e of the reference  %d bytes' %
              (kset, len(K), x[0].size, dev, os.path.getsize(path)))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
