"""NumPy model (float64, no GPU) of the packed-pair Makhoul column solve of WgDCT::solve_combine_impl / mr_colsolve_kernel, on
the mode-by-mode measure of tests/unwrap_modes.py (check U; the rows by SciPy).  As the kernels evaluated it before dct_split_mul (gpa_dct.h) -- the coefficient of bin N - k
taken from the imaginary part of bin k's product, every bin rounding on its own -- it reads about eps / |smallest eigenvalue|
(66 floors at 256^2, 2990 at 1024 x 64: what tests/test_gpu_unwrap_modes.py measured on the device then); with every coefficient
evaluated once it reads about 1 floor, as the device does now.  See the comment above UNWRAP_MODES in tests/tolerances.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'tests'))
import numpy as np
import scipy.fft as sfft
import unwrap_modes as um


def col_solve(Rrow, shape, symmetrise):
    """Rrow: row-DCT'd residual (unnormalised scipy DCT-II along axis 1), float64.  Returns z rows-spectrum solved along columns."""
    n0, n1 = shape
    N = n0
    a, b = um.eig_parts(shape, False, np.float64)           # 2 sin^2
    am = 2 * np.sin(np.pi * (N - np.arange(N)) / (2.0 * N)) ** 2
    k = np.arange(N)
    w = np.exp(-1j * np.pi * k / (2.0 * N))
    m = np.arange(N)
    src = np.where(m < (N + 1) // 2, 2 * m, 2 * (N - 1 - m) + 1)
    out = np.empty_like(Rrow)
    cn = -0.5 / N
    for ja in range(0, n1, 2):
        jb = ja + 1
        c = Rrow[src, ja] + 1j * Rrow[src, jb]
        Z = np.fft.fft(c)
        zk, zm = Z, Z[(N - k) % N]
        va = 0.5 * (zk + np.conj(zm))
        vb = (zk - np.conj(zm)) / 2j
        ua, ub = w * va, w * vb
        if symmetrise:
            # the coefficient of bin N - k taken from bin N - k's own real part instead of this bin's imaginary part
            ua = ua.real + 1j * (-(ua.real[(N - k) % N]))
            ub = ub.real + 1j * (-(ub.real[(N - k) % N]))
            ua[0] = ua.real[0]
            ub[0] = ub.real[0]
        with np.errstate(divide='ignore'):
            sa, sb = cn / (a + b[ja]), cn / (a + b[jb])
            sam, sbm = cn / (am + b[ja]), cn / (am + b[jb])
        sam[0] = sbm[0] = 0
        if ja == 0:
            sa[0] = 1.0 / N
        ya = (sa * ua.real + 1j * sam * ua.imag) * np.conj(w)
        yb = (sb * ub.real + 1j * sbm * ub.imag) * np.conj(w)
        xn = ya + 1j * yb
        v = np.conj(np.fft.fft(np.conj(xn)))
        res = np.empty(N, complex)
        res[src] = v
        out[:, ja], out[:, jb] = res.real, res.imag
    return out


for shape in ((64, 64), (256, 256), (1024, 64)):
    phi0, _ = um.make_inputs(shape, shape[0] + 3 * shape[1])
    dx, dy = um.diffs(phi0)
    ref, k, r0 = um.reference_pcg(dx, dy, None, 1, False, np.longdouble)
    eig = um.eig_table(shape, False, np.longdouble)
    emu, _, _ = um.emulate(dx, dy, None, 1, False, np.float64)
    floor = um.spectral_residual(emu, ref, r0, eig)
    Rrow = sfft.dct(r0.astype(np.float64), axis=1)                       # rows, unnormalised
    for sym in (False, True):
        Zc = col_solve(Rrow, shape, sym)                                 # columns solved, still row spectra
        z = sfft.idct(Zc, axis=1)                                        # scipy idct = exact inverse of dct
        # alpha = 1 in exact arithmetic: phi = z
        print(shape, 'symmetrised' if sym else 'as the kernel', 'reads %.1f floors' % (um.spectral_residual(z, ref, r0, eig) / floor), flush=True)
