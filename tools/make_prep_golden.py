#!/usr/bin/env python
"""Fixtures of the image preparation: runs the reference's own `imagetools` (pyGPA/imagetools.py:92-194, imported through
oracle.make_golden._install_stubs) on the cases of tests/prep_cases.py and writes tests/golden/prep_*.npz.

    python tools/make_prep_golden.py [--only NAME ...]

Two third-party pieces the reference imports are absent here and are REPLACED, in this file only:
  skimage.morphology.disk   by its restatement prep_cases.disk -- the (2r+1)^2 uint8 array X^2 + Y^2 <= r^2 of
                            np.meshgrid(arange(-r, r + 1), arange(-r, r + 1)), which is what skimage documents and computes;
  dask.array.any            by np.any wrapped so that the result has the .compute() the reference calls.
Everything else -- scipy.ndimage's gaussian_filter and binary_erosion, the loops -- is the reference's own code path.

Data only: inputs, sigma, r, mask_value, the reference's out for nan_scale None and 1, its VV and den, masks and lims.  The
script also prints what the cases promise: the uncovered fraction, the smallest den under the mask, the kept fractions.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import prep_cases as pc  # noqa: E402


class _Computed(np.ndarray):
    def compute(self):
        return np.asarray(self)


def import_imagetools():
    from oracle.make_golden import _install_stubs, REF
    _install_stubs()
    import matplotlib
    matplotlib.use('Agg')
    sys.modules['skimage.morphology'].disk = pc.disk
    sys.modules['dask.array'].any = lambda *a, **k: np.asarray(np.any(*a, **k)).view(_Computed)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pyGPA.imagetools as it
    return it


def make_homogenize(it, name):
    import scipy.ndimage as ndi
    image, mask, sigma = pc.homogenize_inputs(name)
    with np.errstate(invalid='ignore', divide='ignore'):
        out_none = it.gauss_homogenize2(image, mask, sigma)
        out_1 = it.gauss_homogenize3(image, mask, sigma)
        # VV and den as lines 99-102 compute them
        VV = ndi.gaussian_filter(np.where(mask, image, 0), sigma=sigma)
        den = ndi.gaussian_filter(mask.astype(image.dtype), sigma=sigma)
        VV /= den
    empty = pc.box_empty(mask, sigma)
    assert np.array_equal(np.isnan(VV), empty) and np.array_equal(den == 0, empty), name
    assert np.all(np.isfinite(image[mask])) and image[mask].min() >= 500 and image[mask].max() <= 4000
    print('%-22s R %3d  uncovered %.1f %%  NaN samples %d  min den under the mask %.4f  masked range %.0f .. %.0f' %
          (name, pc.radius(sigma), 100 * empty.mean(), int(np.isnan(image).sum()), den[mask].min(), image[mask].min(), image[mask].max()))
    np.savez_compressed(os.path.join(pc.GOLDEN, name + '.npz'), image=image, mask=mask, sigma=np.float64(sigma), out_none=out_none,
                        out_1=out_1, VV=VV, den=den)


def make_mask(it):
    stack = pc.mask_stack()
    frames = stack.astype(np.float64)
    out = dict(stack=stack, mask_value=np.float64(pc.MASK_VALUE), radii=np.array(pc.MASK_RADII))
    for r in pc.MASK_RADII:
        out['mask_r%d' % r] = it.generate_mask(frames, pc.MASK_VALUE, r)
        print('prep_mask r %3d: kept %.2f %%' % (r, 100 * out['mask_r%d' % r].mean()))
    print('prep_mask: %.2f %% of the pixels are hit' % (100 * (~out['mask_r0']).mean()))
    out['mask_nan_r20'] = it.generate_mask(frames, np.nan, 20)
    # the bounds cull_by_mask slices with, read off an index grid that went through it
    grid = np.stack(np.mgrid[:stack.shape[1], :stack.shape[2]])
    for r in (3, 20):
        c = it.cull_by_mask(grid, out['mask_r%d' % r])
        out['cull_lims_r%d' % r] = np.array([c[0, 0, 0], c[0, -1, 0] + 1, c[1, 0, 0], c[1, 0, -1] + 1])
    np.savez_compressed(os.path.join(pc.GOLDEN, 'prep_mask.npz'), **out)


def make_trim(it):
    out = {}
    for name in pc.TRIM_CASES:
        img = pc.trim_image(name)
        out[name + '_image'] = img
        out[name + '_trim_nans'] = it.trim_nans(img)
        try:
            t2, lims = it.trim_nans2(img, return_lims=True)
        except IndexError:      # an interior all-NaN line: the reference's window empties
            out[name + '_trim_nans2_empties'] = np.bool_(True)
            print('prep_trim %-8s %s -> trim_nans %s, trim_nans2 empties' % (name, img.shape, out[name + '_trim_nans'].shape))
            continue
        out[name + '_trim_nans2'] = t2
        out[name + '_lims'] = np.asarray(lims)
        print('prep_trim %-8s %s -> trim_nans %s, trim_nans2 %s lims %s' % (name, img.shape, out[name + '_trim_nans'].shape, t2.shape,
                                                                           np.asarray(lims).tolist()))
    np.savez_compressed(os.path.join(pc.GOLDEN, 'prep_trim.npz'), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    it = import_imagetools()

    def want(n):
        return a.only is None or n in a.only
    for name in pc.H_CASES:
        if want(name):
            make_homogenize(it, name)
    if want('prep_mask'):
        make_mask(it)
    if want('prep_trim'):
        make_trim(it)


if __name__ == '__main__':
    main()
