"""homogenize_per_axis: the cases of tests/golden/axis_*.npz, their seeded generators, a NumPy restatement of what the reference
computes (imagetools.py:112-125), and the derived bound of the GPU test.  A helper, not a test; tools/make_axis_golden.py uses
it too.

The restatement is written from the rules of NumPy, SciPy and the reference, not from the kernels:
    res = image.copy()
    for axis in (0, 1):
        line    = reducfunc(where(mask, res, nan), axis)                (np.nanmedian: an exact selection)
        profile = gaussian_filter(line, sigma) along the line            (taps of prep_cases.gauss_taps, 'reflect' fold, one f64
                                                                          sum, rounded once to the image's dtype; along the unit
                                                                          axis SciPy's second pass multiplies by sum(w) ~ 1)
        res     = res / (profile / profile.max())                        (np.max propagates NaN)
"""
import os

import numpy as np

import prep_cases as pc

GOLDEN = pc.GOLDEN
EPS = pc.EPS

# name: (shape, sigma, seed)
CASES = {
    'axis_48x80_s3': ((48, 80), 3.0, 41),        # R = 12
    'axis_33x150_s10': ((33, 150), 10.0, 42),    # R = 40 > n0; odd sizes; ragged transpose tiles
    'axis_64x64_s200': ((64, 64), 200.0, 43),    # the default sigma: R = 800, the fold repeats 12 times
    'axis_5x50_s2': ((5, 50), 2.0, 44),          # thin
    'axis_50x5_s2': ((50, 5), 2.0, 45),          # thin
    'axis_96x130_s25': ((96, 130), 25.0, 46),    # R = 100
    'axis_70x300_s1': ((70, 300), 1.0, 47),      # R = 4; a line longer than one round of a 256-thread load
}
THIN = ('axis_5x50_s2', 'axis_50x5_s2')
# one fully masked column: the reference returns NaN at every pixel, and so must the mirror
NAN_CASE = 'axis_nan_40x60_s2'
NAN_CASE_DEF = ((40, 60), 2.0, 48)
VARIANTS = ('f64_nomask', 'f64_mask', 'f32_nomask', 'f32_mask')


# ---- the bound -------------------------------------------------------------------------------------------------------------
# Relative deviations between the device and the reference, in units of the unit round-off u of the image's dtype (EPS),
# first order.  Every median of the cases is positive (checked with the fixtures), so every sum below is a sum of positive
# terms and its error is relative to its value; the median and the maximum are 1-Lipschitz, so relative perturbations of at
# most e of positive samples move them by at most e.  A = 2 R + 2.
#
# f64.  A profile is a sum of 2 R + 1 positive products: at most A roundings on the device (the sum, then nothing: it is
#   already f64), A in SciPy's pass along the line and about A more in its pass along the unit axis (the same taps times the one
#   repeated sample), and 3 for taps that differ in the last place of exp and of the normalisation:
#       e_p0  = 3 A + 3                      the axis-0 profile: its medians are the same numbers on both sides
#       e_q0  = 2 e_p0 + 2                   q = profile / max: the profile enters as numerator and as maximum; a division each
#       e_r0  = e_q0 + 2                     res = image / q0, a division on each side
#       e_m1  = e_r0 + 2 (+ m1_extra)        medians of res: 1-Lipschitz; the (a + b) / 2 of an even count rounds on each side
#       e_p1  = e_m1 + 3 A + 3
#       e_q1  = 2 e_p1 + 2
#       e_out = e_r0 + e_q1 + 2              out = res / q1        = 24 A + 44 (+ 2 m1_extra)
# f32.  Both sides accumulate the profile in f64 and round it ONCE to f32; the f64 part above is below 3e-5 u32 for R <= 800
#   and is covered by 1.  Two roundings of nearly the same number differ by at most an ulp = 2 u, so the chain is the one above
#   with 2 + 1 in place of 3 A + 3:
#       e_p0 = 3,  e_q0 = 8,  e_r0 = 10,  e_m1 = 12 (+ m1_extra),  e_p1 = 15,  e_q1 = 32,  e_out = 44 (+ 2 m1_extra)
# m1_extra: what a foreign reducfunc adds between the two sides' axis-1 lines beyond the perturbation of its input -- 2 n for
#   np.nanmean of n samples (n roundings on each side).
def bounds(sigma, dtype, m1_extra=0):
    """(e_p0, e_p1, e_out): relative bounds of the two profiles and of the output, in units of EPS[dtype]"""
    A = 2 * pc.radius(sigma) + 2
    if np.dtype(dtype) == np.float64:
        return 3 * A + 3, 9 * A + 15 + m1_extra, 24 * A + 44 + 2 * m1_extra
    return 3, 15 + m1_extra, 44 + 2 * m1_extra


# measured on the MI355X: max relative deviation / EPS per case and variant, (profile 0, profile 1, out);
# tests/test_gpu_axis.py prints the figures
C_MEASURED = {
    'axis_48x80_s3': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (2.102, 2.052, 5.712), 'f64_mask': (3.210, 3.987, 7.409)},
    'axis_33x150_s10': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (4.155, 3.134, 7.879), 'f64_mask': (4.242, 3.139, 7.898)},
    'axis_64x64_s200': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (14.787, 21.142, 23.684), 'f64_mask': (18.018, 13.763, 30.862)},
    'axis_5x50_s2': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (2.263, 2.061, 4.045), 'f64_mask': (2.296, 3.191, 5.881)},
    'axis_50x5_s2': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (1.089, 2.139, 3.855), 'f64_mask': (2.096, 4.080, 3.844)},
    'axis_96x130_s25': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (6.528, 8.637, 11.061), 'f64_mask': (6.525, 6.475, 11.002)},
    'axis_70x300_s1': {'f32_nomask': (0.000, 0.000, 0.000), 'f32_mask': (0.000, 0.000, 0.000), 'f64_nomask': (2.172, 3.995, 7.987), 'f64_mask': (2.241, 3.993, 11.610)},
}


# ---- generators ------------------------------------------------------------------------------------------------------------
def _case_def(name):
    return NAN_CASE_DEF if name == NAN_CASE else CASES[name]


def case_image(name):
    """a positive illumination field of about 2000 with per-row and per-column gain (+-10 %) plus N(0, 20) noise, float64"""
    shape, _, seed = _case_def(name)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[0], :shape[1]].astype(np.float64)
    cy, cx = 0.45 * shape[0], 0.55 * shape[1]
    illum = 0.85 + 0.15 * np.exp(-(((x - cx) / shape[1]) ** 2 + ((y - cy) / shape[0]) ** 2) / 0.5)
    rowgain = 1.0 + 0.1 * (2.0 * rng.random(shape[0]) - 1.0)
    colgain = 1.0 + 0.1 * (2.0 * rng.random(shape[1]) - 1.0)
    return 2000.0 * illum * rowgain[:, None] * colgain[None, :] + 20.0 * rng.standard_normal(shape)


def case_mask(name):
    """10 % random holes; on the full cases also a 4-row block, a column with exactly ONE valid sample and a row with exactly
    TWO; on the thin cases row 0 and column 0 are forced true, so that no line is empty; the NaN case masks column 17 out"""
    shape, _, seed = _case_def(name)
    rng = np.random.default_rng(seed + 500)
    mask = rng.random(shape) >= 0.10
    n0, n1 = shape
    if name in THIN:
        mask[0, :] = True
        mask[:, 0] = True
        return mask
    if name == NAN_CASE:
        mask[:, 17] = False
        return mask
    r0 = n0 // 3
    mask[r0:r0 + 4, n1 // 4:n1 // 4 + n1 // 3] = False
    c, j = n1 // 2 + 3, n0 // 2
    mask[:, c] = False
    mask[j, c] = True
    i = n0 - 6
    mask[i, :] = False
    mask[i, 2] = True
    mask[i, n1 - 5] = True
    return mask


def case_inputs(name):
    return case_image(name), case_mask(name), _case_def(name)[1]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def filter_line(line, sigma):
    """gaussian_filter of a 1-D line under 'reflect': one f64 sum per sample, rounded once to the line's dtype"""
    line = np.asarray(line)
    w = pc.gauss_taps(sigma)
    R = len(w) // 2
    n = line.size
    idx = pc.fold(np.arange(n)[:, None] + np.arange(-R, R + 1)[None, :], n)
    return (line.astype(np.float64)[idx] * w[None, :]).sum(axis=1).astype(line.dtype)


def restate(image, sigma, mask=None, reducfunc=np.nanmedian):
    """(out, profile0, profile1, res0) of homogenize_per_axis in the image's dtype; res0 is res after axis 0"""
    res = np.array(image, copy=True)
    profiles, res0 = [], None
    with np.errstate(invalid='ignore', divide='ignore'):
        for axis in (0, 1):
            src = res if mask is None else np.where(mask, res, np.nan)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)       # All-NaN slice
                line = np.asarray(reducfunc(src, axis=axis)).astype(res.dtype)
            prof = filter_line(line, sigma)
            q = prof / prof.max()
            res = res / (q[None, :] if axis == 0 else q[:, None])
            profiles.append(prof)
            if axis == 0:
                res0 = res
    return res, profiles[0], profiles[1], res0


def rel_dev(got, ref, dtype):
    """max |got - ref| / (|ref| EPS[dtype])"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) * EPS[np.dtype(dtype)])).max())


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def variant_inputs(z, variant):
    """(image in the variant's dtype, mask or None) of a loaded fixture"""
    dtype = np.float64 if variant.startswith('f64') else np.float32
    return z['image'].astype(dtype), (z['mask'] if variant.endswith('_mask') else None)


def lines_check(tmpdir, extra=()):
    """compile tests/host/lines_check.cpp against pygpa_amd/csrc/gpa_lines.h with the host compiler and run it: returns
    (compiler result, run result or None).  The program prints 'OK <checks>'."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), 'lines_check')
    cmd = [pc._host_cxx(), '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(root, 'pygpa_amd', 'csrc')] + list(extra)
    r = subprocess.run(cmd + [os.path.join(root, 'tests', 'host', 'lines_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    return r, subprocess.run([exe], capture_output=True, text=True, timeout=120)
