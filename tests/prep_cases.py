"""Image preparation: the cases of tests/golden/prep_*.npz, their seeded generators, and a NumPy restatement of what the
reference computes (imagetools.py:92-194).  A helper, not a test; tools/make_prep_golden.py uses it too.

The restatement is written from the rules of SciPy and of the reference, not from the kernels:
  gaussian_filter: taps exp(-k^2 / 2 sigma^2) / sum, k = -R .. R, R = int(4 sigma + 0.5), a correlation along axis 0 and then
  along axis 1 on the 'reflect' extension (d c b a | a b c d | d c b a);
  VV = G(where(mask, image, 0)) / G(mask), NaN exactly where the (2R+1)^2 box of the reflect-extended mask holds no true
  sample (box_empty);  disk(r) = X^2 + Y^2 <= r^2 on the (2r+1)^2 grid;  binary_erosion with border_value 0;  the loop of
  trim_nans2.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# ---- homogenisation ----------------------------------------------------------------------------------------------------
# name: (shape, sigma, seed)
H_CASES = {
    'prep_h_96x130_s3': ((96, 130), 3.0, 11),       # R = 12: the smallest FFT radius; ragged last segments; ~80 % uncovered
    'prep_h_40x300_s10': ((40, 300), 10.0, 12),     # R = 40 >= n0: the reflect extension repeats
    'prep_h_150x33_s25': ((150, 33), 2.5, 13),      # R = 10: the direct route by default; odd width
    'prep_h_64x64_full_s4': ((64, 64), 4.0, 14),    # mask all true, no NaN: VV is the plain filter
}

# The bound of the GPU test: |VV - VV_ref| <= C_VV eps M / den_ref wherever den_ref > 0, M the largest masked sample, eps the
# unit round-off (2^-24, 2^-53).  C_VV is derived, not measured: two transforms of at most 2^14 points at about 4 log2(L) eps
# each (56 eps at most, relative to the largest sample of the pair), the rounded tables, the multiply and the division.
C_VV = 128.0
EPS = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
# measured on the MI355X: max |VV - VV_ref| den_ref / (eps M) per case, (f32, f64), FFT route (GAUSS_FFT_MINR = 1) and direct
# route (GAUSS_FFT_MINR = 100000); tests/test_gpu_prep.py prints the figures
C_MEASURED = {
    'prep_h_96x130_s3': {'fft': (1.691, 1.786), 'direct': (0.963, 1.966)},
    'prep_h_40x300_s10': {'fft': (0.716, 0.975), 'direct': (0.419, 1.292)},
    'prep_h_150x33_s25': {'fft': (1.579, 3.086), 'direct': (1.000, 3.086)},
    'prep_h_64x64_full_s4': {'fft': (3.049, 3.072), 'direct': (0.697, 4.096)},
}
# tests/test_gpu_prep.py::test_longest_segments (12 x 70 under sigma = 600 in f32, 300 in f64; the split passes): 0.667, 6.105


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def fold(i, n):
    """index under the period-2n reflect rule, any integers"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gauss_taps(sigma):
    R = radius(sigma)
    k = np.arange(-R, R + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum()


def gauss1d(x, sigma, axis):
    """correlation with the taps along `axis` on the reflect extension"""
    w = gauss_taps(sigma)
    R = len(w) // 2
    n = x.shape[axis]
    x = np.moveaxis(x, axis, 0)
    out = np.zeros_like(x, dtype=np.float64)
    idx = np.arange(n)
    for k in range(-R, R + 1):
        out += w[k + R] * x[fold(idx + k, n)]
    return np.moveaxis(out, 0, axis)


def gauss2d(x, sigma):
    return gauss1d(gauss1d(np.asarray(x, dtype=np.float64), sigma, 0), sigma, 1)


def box_empty(mask, sigma):
    """True where no true sample of the reflect-extended mask lies within +-R along both axes"""
    R = radius(sigma)
    any_ = np.asarray(mask, dtype=bool)
    for axis in (0, 1):
        n = any_.shape[axis]
        a = np.moveaxis(any_, axis, 0)
        ext = a[fold(np.arange(-R, n + R), n)]                       # the walked extension
        c = np.concatenate([np.zeros((1,) + ext.shape[1:], int), np.cumsum(ext, axis=0)])
        any_ = np.moveaxis((c[2 * R + 1:] - c[:n]) > 0, 0, axis)
    return ~any_


def restate_homogenize(image, mask, sigma, nan_scale=None):
    """(out, VV, den) of gauss_homogenize2"""
    with np.errstate(invalid='ignore', divide='ignore'):
        num = gauss2d(np.where(mask, image, 0), sigma)
        den = gauss2d(mask.astype(np.float64), sigma)
        VV = num / den
        VV[box_empty(mask, sigma)] = np.nan
        if nan_scale is not None:
            VV = np.where(np.isnan(VV), nan_scale, VV)
        return image / VV, VV, den


def lattice_image(shape, seed):
    """a smooth illumination profile times a hexagonal lattice, values within [500, 4000]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[0], :shape[1]].astype(np.float64)
    cy, cx = 0.4 * shape[0], 0.6 * shape[1]
    illum = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * (0.8 * max(shape)) ** 2))
    lat = sum(np.cos(2 * np.pi * 0.11 * (np.cos(a) * x + np.sin(a) * y)) for a in (0.2, 0.2 + np.pi / 3, 0.2 + 2 * np.pi / 3))
    img = illum * (1.0 + 0.12 * lat) + 0.01 * rng.standard_normal(shape)
    img = (img - img.min()) / (img.max() - img.min())
    return 500.0 + 3500.0 * img


def _disk_at(shape, cy, cx, rad):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= rad * rad


def homogenize_inputs(name):
    """(image, mask, sigma) of a case: NaN at some samples OUTSIDE the mask"""
    shape, sigma, seed = H_CASES[name]
    rng = np.random.default_rng(seed + 1000)
    image = lattice_image(shape, seed)
    if name == 'prep_h_96x130_s3':
        mask = _disk_at(shape, 30, 40, 6) | _disk_at(shape, 93, 100, 5)     # the second blob touches the bottom edge
        mask[50, 112] = True                                                 # one isolated true pixel
    elif name == 'prep_h_40x300_s10':
        mask = _disk_at(shape, 12, 60, 9) | _disk_at(shape, 30, 150, 7)
        mask[2, 296] = True
    elif name == 'prep_h_150x33_s25':
        mask = _disk_at(shape, 40, 10, 8) | _disk_at(shape, 120, 30, 6)
        mask[80, 16] = True
    else:
        return image, np.ones(shape, dtype=bool), sigma
    nan_at = (rng.random(shape) < 0.03) & ~mask
    image[nan_at] = np.nan
    return image, mask, sigma


# ---- masks -----------------------------------------------------------------------------------------------------------
MASK_SHAPE = (5, 120, 140)
MASK_VALUE = 0.0
MASK_RADII = (0, 1, 3, 20, 200)     # 200: larger than the image, all false


def disk(r):
    """skimage.morphology.disk restated: the (2r+1)^2 array X^2 + Y^2 <= r^2, uint8"""
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= r * r, dtype=np.uint8)


def mask_stack(seed=21):
    """uint16 frames with the sentinel 0 sprinkled (about 0.3 % of the pixels are hit in some frame), away from a patch that
    survives the r = 20 erosion"""
    rng = np.random.default_rng(seed)
    B, n0, n1 = MASK_SHAPE
    stack = rng.integers(100, 4000, size=MASK_SHAPE).astype(np.uint16)
    y, x = np.mgrid[:n0, :n1]
    far = ((y - 62) ** 2 + (x - 75) ** 2) > 30 ** 2
    hit = (rng.random((n0, n1)) < 0.0042) & far
    ys, xs = np.nonzero(hit)
    stack[rng.integers(0, B, size=len(ys)), ys, xs] = 0
    return stack


def restate_erosion(mask, r):
    """binary_erosion(mask, disk(r)), border_value 0, by the row-distance decomposition"""
    mask = np.asarray(mask, dtype=bool)
    n0, n1 = mask.shape
    if r == 0:
        return mask.copy()
    pad = np.zeros((n0, n1 + 2), dtype=bool)
    pad[:, 1:-1] = mask
    big = n1 + 2
    pos = np.arange(n1 + 2)
    left = np.maximum.accumulate(np.where(~pad, pos, -big), axis=1)                       # nearest false at or before
    right = np.minimum.accumulate(np.where(~pad, pos, 2 * big)[:, ::-1], axis=1)[:, ::-1]   # ... at or after
    hd = np.minimum(pos - left, right - pos)[:, 1:-1]
    hdp = np.zeros((n0 + 2 * r, n1), dtype=hd.dtype)
    hdp[r:r + n0] = hd
    out = np.ones((n0, n1), dtype=bool)
    for dy in range(-r, r + 1):
        out &= hdp[r + dy:r + dy + n0] > int(np.floor(np.sqrt(r * r - dy * dy)))
    return out


def restate_generate_mask(stack, value, r):
    return restate_erosion(~np.any(np.asarray(stack) == value, axis=0), r)


def restate_bounds(mask):
    rows, cols = np.nonzero(mask.any(axis=1))[0], np.nonzero(mask.any(axis=0))[0]
    return np.array([rows.min(), rows.max() + 1, cols.min(), cols.max() + 1])


# ---- trims -----------------------------------------------------------------------------------------------------------
TRIM_CASES = ('borders', 'tie', 'inner')


def trim_image(name):
    rng = np.random.default_rng({'borders': 31, 'tie': 32, 'inner': 33}[name])
    if name == 'borders':       # ragged NaN borders of unequal widths on all four sides, as undistort_image leaves them
        img = rng.random((48, 56))
        x = np.arange(56)
        y = np.arange(48)
        top = (2 + 1.5 * np.sin(x / 7.0)).round().astype(int)
        bot = (5 + 2 * np.cos(x / 5.0)).round().astype(int)
        lef = (1 + 1.2 * np.sin(y / 6.0) ** 2).round().astype(int)
        rig = (7 + 2 * np.sin(y / 9.0)).round().astype(int)
        for j in range(56):
            img[:top[j], j] = np.nan
            img[48 - bot[j]:, j] = np.nan
        for i in range(48):
            img[i, :lef[i]] = np.nan
            img[i, 56 - rig[i]:] = np.nan
    elif name == 'tie':         # NaN specks in two opposite corners: r = c = [1, 1], a tie, and the columns lose
        img = rng.random((12, 9))
        img[0, 0] = np.nan
        img[11, 8] = np.nan
    else:                       # an interior all-NaN row and column, plus a border
        img = rng.random((20, 17))
        img[7] = np.nan
        img[:, 11] = np.nan
        img[0] = np.nan
        img[:, -1] = np.nan
        img[3, 5] = np.nan
    return img


def restate_trim_lims(image):
    """the loop of trim_nans2 on index bounds: [x0, x1, y0, y1]"""
    nan = np.isnan(image)
    x0, x1, y0, y1 = 0, image.shape[0], 0, image.shape[1]
    while x1 > x0 and y1 > y0:
        w = nan[x0:x1, y0:y1]
        r = w[[0, -1]].sum(axis=1)
        c = w[:, [0, -1]].sum(axis=0)
        if r.sum() == 0 and c.sum() == 0:
            break
        if r.sum() > c.sum():
            x0 += int(r[0] > 0)
            x1 -= int(r[1] > 0)
        else:
            y0 += int(c[0] > 0)
            y1 -= int(c[1] > 0)
    return np.array([x0, x1, y0, y1])


def restate_trim_nans(image):
    nan = np.isnan(image)
    return image[~nan.all(axis=1)][:, ~nan.all(axis=0)]


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def _host_cxx():
    import shutil
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None and os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        cxx = '/opt/rocm/lib/llvm/bin/clang++'
    assert cxx is not None, 'no host C++ compiler'
    return cxx


def host_compiler_links(tmpdir, flags):
    """whether the host compiler builds and runs an empty program with `flags` (the sanitizer runtimes are there)"""
    import subprocess
    src, exe = os.path.join(str(tmpdir), 'probe.cpp'), os.path.join(str(tmpdir), 'probe')
    with open(src, 'w') as f:
        f.write('int main() { return 0; }\n')
    r = subprocess.run([_host_cxx(), '-std=c++17'] + list(flags) + [src, '-o', exe], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


def prep_check(tmpdir, extra=()):
    """compile tests/host/prep_check.cpp against pygpa_amd/csrc/gpa_prep.h with the host compiler and run it: returns
    (compiler result, run result or None).  The program prints 'OK <checks>'."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _host_cxx()
    exe = os.path.join(str(tmpdir), 'prep_check')
    cmd = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(root, 'pygpa_amd', 'csrc')] + list(extra)
    r = subprocess.run(cmd + [os.path.join(root, 'tests', 'host', 'prep_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    return r, subprocess.run([exe], capture_output=True, text=True, timeout=120)
