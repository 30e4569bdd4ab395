#!/usr/bin/env python
"""Fixtures of homogenize_per_axis: runs the reference's own `imagetools.homogenize_per_axis` (pyGPA/imagetools.py:112-125,
imported as tools/make_prep_golden.py imports the module) on the cases of tests/axis_cases.py and writes
tests/golden/axis_*.npz.

    python tools/make_axis_golden.py [--only NAME ...]

Data only: the f64 image (the f32 input is its cast), the mask, sigma, and per variant (f64 / f32 input, without / with the mask)
the reference's output and its two filtered profiles.  The profiles are captured from the reference's own calls of
scipy.ndimage.gaussian_filter, which is wrapped for the duration of a call and records what it returns.  The script also
prints what the cases promise: finite outputs, positive medians, every divisor q within 0.5 .. 1.
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import axis_cases as ac  # noqa: E402
from make_prep_golden import import_imagetools  # noqa: E402


def run_reference(it, image, sigma, mask):
    """(out, profile0, profile1) of the reference's call"""
    seen = []
    real = it.ndi.gaussian_filter

    def recording(*a, **k):
        r = real(*a, **k)
        seen.append(np.array(r, copy=True))
        return r
    it.ndi.gaussian_filter = recording
    try:
        with warnings.catch_warnings(), np.errstate(invalid='ignore', divide='ignore'):
            warnings.simplefilter('ignore', RuntimeWarning)
            out = it.homogenize_per_axis(image, sigma=sigma, mask=mask)
    finally:
        it.ndi.gaussian_filter = real
    assert len(seen) == 2 and seen[0].shape == (1, image.shape[1]) and seen[1].shape == (image.shape[0], 1)
    return out, seen[0].ravel(), seen[1].ravel()


def make_case(it, name):
    image, mask, sigma = ac.case_inputs(name)
    out = dict(image=image, mask=mask, sigma=np.float64(sigma))
    for variant in ac.VARIANTS:
        img, m = ac.variant_inputs(out, variant)
        res, p0, p1 = run_reference(it, img, sigma, m)
        assert res.dtype == p0.dtype == p1.dtype == img.dtype, (name, variant)
        if name == ac.NAN_CASE and m is not None:
            assert np.isnan(res).all(), name
        else:
            q0, q1 = p0 / p0.max(), p1 / p1.max()
            assert np.isfinite(res).all() and p0.min() > 0 and p1.min() > 0, (name, variant)
            assert 0.5 <= min(q0.min(), q1.min()) and max(q0.max(), q1.max()) <= 1.0, (name, variant)
            print('%-20s %-10s R %3d  q0 %.3f .. 1  q1 %.3f .. 1  out %.4f .. %.4f' %
                  (name, variant, ac.pc.radius(sigma), q0.min(), q1.min(), res.min(), res.max()))
        out['out_' + variant], out['p0_' + variant], out['p1_' + variant] = res, p0, p1
    if name == ac.NAN_CASE:
        print('%-20s masked: all %d pixels NaN' % (name, image.size))
    np.savez_compressed(os.path.join(ac.GOLDEN, name + '.npz'), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    it = import_imagetools()
    for name in list(ac.CASES) + [ac.NAN_CASE]:
        if a.only is None or name in a.only:
            make_case(it, name)


if __name__ == '__main__':
    main()
