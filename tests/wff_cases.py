"""Windowed Fourier filtering: the cases of tests/golden/wff_*.npz, a NumPy / SciPy restatement of the separable shared-sum
form the kernels compute, and the f32 bounds.  A helper, not a test; tools/make_wff_golden.py uses it too.

The restatement is written from the rules of the reference (geometric_phase_analysis.py:551-580), not from the kernels:
window s = round(2 sigma) (Python's round), offsets j = -s .. s - 1, g(j) = exp(-j^2 / 2 sigma^2), nrm = sum g^2;
kx(j) = g(j) e^(i wx j) along axis 1, ky(j) = g(j) e^(i wy j) / nrm along axis 0; true convolution, mode 'reflect';

    g_t = scale * sum_wx Cx[kx] ( sum_wy Cy[ky] ( T_t ( Cy[ky] ( Cx[kx] f ) ) ) ),   T_t: keep where |sf| >= thr_t
"""
import os

import numpy as np
import scipy.ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# name: (shape, sigma, wl, wu).  Thresholds are chosen by the generator (quantiles 0.5 and 0.9 of |sf|, each moved to the
# centre of the widest gap within +-2000 ranks) and stored in the fixture.
CASES = {
    'wff_40x56': ((40, 56), 3.0, -1.0, 1.0),          # s = 6, 7 x 7 pairs
    'wff_5x50': ((5, 50), 3.0, -1.0, 1.0),            # axis 0 shorter than s: the fold reflects twice
    'wff_50x5': ((50, 5), 3.0, -1.0, 1.0),            # ... axis 1
    'wff_33x47_s25': ((33, 47), 2.5, -1.0, 1.0),      # 2 sigma = 5.0: s = 5, an odd half-window
    'wff_36x44_asym': ((36, 44), 3.0, -0.7, 1.1),     # a list whose length depends on float rounding (recorded: nws)
}

# f32: the largest deviation of the restatement run in complex64 from the one in complex128, relative to the largest
# magnitude of the output, measured on the CPU by tools/make_wff_golden.py (printed as 'c64 restatement'); the bound is
# 8 x that -- the factor covers the kernels' f32 accumulation order and f32 taps.
F32_MEASURED = {
    'wff_40x56': 1.695e-07,
    'wff_5x50': 1.533e-07,
    'wff_50x5': 2.066e-07,
    'wff_33x47_s25': 1.794e-07,
    'wff_36x44_asym': 1.707e-07,
}
F32_FACTOR = 8.0


def f32_bound(name):
    return F32_FACTOR * F32_MEASURED[name]


def half_window(sigma):
    return round(2 * sigma)


def freq_list(sigma, wl, wu):
    wi = 1 / sigma
    return np.arange(wl, wu + wi / 2, wi)


def scale_of(sigma):
    wi = 1 / sigma
    return wi * wi / (4 * np.pi ** 2)


def taps(sigma, w, normalised):
    """k(j) = g(j) e^(i w j) (/ nrm), j = -s .. s - 1, as a complex128 array indexed by j + s"""
    s = half_window(sigma)
    j = np.arange(-s, s)
    g = np.exp(-j ** 2 / (2 * sigma ** 2))
    k = g * np.exp(1j * w * j)
    return k / (g ** 2).sum() if normalised else k


def cconv1d(f, k, axis):
    """out[i] = sum_j f[i - j] k(j) along `axis`, 'reflect' boundary, through ndi.convolve1d on real and imaginary parts;
    in the precision of f (complex64: float32 parts and float32 taps, rounded once per pass)"""
    rt = np.float32 if f.dtype == np.complex64 else np.float64
    fr, fi = np.ascontiguousarray(f.real, dtype=rt), np.ascontiguousarray(f.imag, dtype=rt)
    kr, ki = k.real.astype(rt), k.imag.astype(rt)

    def c(x, w):
        return ndi.convolve1d(x, w, axis=axis, mode='reflect')
    out = np.empty(f.shape, dtype=f.dtype)
    out.real = c(fr, kr) - c(fi, ki)
    out.imag = c(fr, ki) + c(fi, kr)
    return out


def spectra(image, sigma, wxs, wys, cdtype=np.complex128):
    """yields (ix, iy, sf) for every frequency pair, wx outer"""
    f = np.asarray(image).astype(cdtype)
    for ix, wx in enumerate(wxs):
        A = cconv1d(f, taps(sigma, wx, False), 1)
        for iy, wy in enumerate(wys):
            yield ix, iy, cconv1d(A, taps(sigma, wy, True), 0)


def restate(image, sigma, thresholds, wxs, wys, scale, cdtype=np.complex128):
    """the separable shared-sum form: (T,) + image.shape"""
    f = np.asarray(image).astype(cdtype)
    thresholds = np.asarray(thresholds, dtype=np.float64)
    out = np.zeros((len(thresholds),) + f.shape, dtype=cdtype)
    for wx in wxs:
        kx = taps(sigma, wx, False)
        A = cconv1d(f, kx, 1)
        B = np.zeros_like(out)
        for wy in wys:
            ky = taps(sigma, wy, True)
            sf = cconv1d(A, ky, 0)
            mag = np.abs(sf)
            for t, thr in enumerate(thresholds):
                B[t] += cconv1d(np.where(mag >= thr, sf, 0).astype(cdtype), ky, 0)
        for t in range(len(thresholds)):
            out[t] += cconv1d(B[t], kx, 1)
    return out * np.asarray(scale, dtype=out.real.dtype)


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def noisy_phasor(shape, seed):
    """exp(i (phi + noise)): a smooth phase with a carrier inside the +-1 rad / pixel range and 0.6 rad of white noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[0], :shape[1]].astype(np.float64)
    cy, cx = (shape[0] - 1) / 2, (shape[1] - 1) / 2
    phi = 0.35 * x - 0.2 * y + 2.5 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * (0.3 * max(shape)) ** 2))
    return np.exp(1j * (phi + 0.6 * rng.standard_normal(shape)))


_GEOM = {}


def geom_check(tmpdir, extra=()):
    """compile tests/host/wff_geom_check.cpp against pygpa_amd/csrc/gpa_wff.h with the host compiler and run it: returns
    (compiler result, run result or None).  The program prints 'OK <checks>' and the tile lines of tile_geometry()."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None and os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        cxx = '/opt/rocm/lib/llvm/bin/clang++'
    assert cxx is not None, 'no host C++ compiler'
    exe = os.path.join(str(tmpdir), 'wff_geom_check')
    cmd = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(root, 'pygpa_amd', 'csrc')] + list(extra)
    r = subprocess.run(cmd + [os.path.join(root, 'tests', 'host', 'wff_geom_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    return r, subprocess.run([exe], capture_output=True, text=True, timeout=120)


def tile_geometry(tmpdir):
    """{('f32' | 'f64', s): (columns, R)} of the column kernel's workgroup tile, as gpa_wff.h computes it"""
    if not _GEOM:
        r, out = geom_check(tmpdir)
        assert r.returncode == 0 and out is not None and out.returncode == 0, r.stderr[-2000:]
        for ln in out.stdout.splitlines():
            if ln.startswith('TILE '):
                _, dt, s, cols, R = ln.split()
                _GEOM[(dt, int(s))] = (int(cols), int(R))
    return _GEOM
