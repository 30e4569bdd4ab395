"""The weighted unwrap judged mode by mode (plain NumPy / SciPy, no GPU): the reference, the yardstick and the measure of
tests/test_unwrap_modes_host.py and tests/test_gpu_unwrap_modes.py.

A pixel max-norm comparison after a PCG run cannot see a kernel that is subtly wrong: the Poisson preconditioner multiplies
the rounding of the lowest modes by up to N^2 / pi^2, so its f32 tolerance is set by that amplification, and a fault confined
to some modes is divided by the square root of the number of modes in pixel space.  Here the difference to a reference one
precision up is taken PER DCT COEFFICIENT AND MULTIPLIED BY THE EIGENVALUE -- which undoes the amplification -- on a field with
a flat spectrum, relative to the rms of the right-hand side.  A plain f32 solve sits at 1e-6 .. 2.4e-6 on that measure at
every shape; one eigenvalue off by 1e-3 reads a hundred times that.

  reference_pcg   phase_unwrap.py:282-350 as oracle/gpa_oracle.py:unwrap_prediff restates it (operation order, edge weights
                  min(w^2), stopping test), in the arithmetic `real`: np.longdouble judges f64 results, np.float64 f32 results.
  emulate         the same loop in the precision under test (np.float32 / np.float64): inputs and state held in it, tables built
                  in double and then rounded (as gpa_unwrap_tables.hip builds them), dot products accumulated in double,
                  transforms scipy.fft.dctn / idctn(norm='ortho') in that precision.  What a correct solve in that precision
                  leaves on the measure: the yardstick.  `fault` plants one of FAULTS in it.
  spectral_residual, mean_offset   the measure, and the free mean on its own.
Eigenvalues are -4 (sin^2 + sin^2), the form of the device tables: no cos - 1 cancellation."""
import numpy as np
import scipy.fft as sfft

FAULTS = ('eig_one', 'eig_shift', 'edge_last_col', 'first_row_interior', 'fwd_bin')


def hi_real(real):
    """the arithmetic that judges results of precision `real`: one precision up"""
    return np.float64 if np.dtype(real) == np.float32 else np.longdouble


def _pi(real):
    return real(4) * np.arctan(real(1))


def effective_compat(shape, compat):
    """the device drops the reference's swapped-axis table where it is singular (one side at least twice the other)"""
    n0, n1 = shape
    return bool(compat) and not (n0 >= 2 * n1 or n1 >= 2 * n0)


def eig_parts(shape, compat, real=np.float64, shift0=0):
    """a[k] = 2 sin^2(pi k / 2 A0), b[j] = 2 sin^2(pi j / 2 A1), evaluated in `real`; compat: A0 = n1, A1 = n0
    (phase_unwrap.py:107-109).  shift0: the axis-0 table read one bin off (fault 'eig_shift')."""
    n0, n1 = shape
    A0, A1 = (n1, n0) if effective_compat(shape, compat) else (n0, n1)
    pi = _pi(real)
    a = 2 * np.sin(pi * (np.arange(n0) + shift0).astype(real) / real(2 * A0)) ** 2
    b = 2 * np.sin(pi * np.arange(n1).astype(real) / real(2 * A1)) ** 2
    return a, b


def eig_table(shape, compat, real, shift0=0):
    """-2 (a + b) = -4 (sin^2 + sin^2) in `real`, [0, 0] -> 1.  np.longdouble: evaluated in long double; otherwise the two
    one-dimensional tables are built in double, rounded to `real` and combined in `real`, as the device does."""
    build = np.longdouble if np.dtype(real) == np.longdouble else np.float64
    a, b = eig_parts(shape, compat, build, shift0)
    a, b = a.astype(real), b.astype(real)
    eig = real(-2) * (a[:, None] + b[None, :])
    eig[0, 0] = real(1)
    return eig


def make_inputs(shape, seed):
    """(phi0, weight), both float32.  phi0: uniform in [-0.7, 0.7] -- a flat spectrum -- on the grid of multiples of 2^-20, so
    phi0 AND its differences (below 1.4 in size: 22 bits) are exact in float32: the prediff entry, the psi entry's own
    differences and both precisions start from the same numbers, and no difference comes near +-pi, so the wrap inside the
    entry points can never flip.  weight: uniform in [0.2, 1]."""
    rng = np.random.default_rng(seed)
    u = rng.random(shape, dtype=np.float32).astype(np.float64)
    phi0 = (np.round((1.4 * u - 0.7) * 2.0 ** 20) / 2.0 ** 20).astype(np.float32)
    weight = (np.float32(0.2) + np.float32(0.8) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    return phi0, weight


def diffs(phi0):
    """dx (n0, n1 - 1), dy (n0 - 1, n1) of make_inputs' phi0, in float64 (exact, and exactly representable in float32)"""
    p = phi0.astype(np.float64)
    return np.diff(p, axis=1), np.diff(p, axis=0)


def fault_bin(shape):
    """the DCT bin of the single-bin faults: away from both axes, fixed by the shape"""
    n0, n1 = shape
    return max(1, n0 // 3), max(1, (2 * n1) // 3)


def _wrap(x, real):
    pi = _pi(real)
    return np.mod(x + pi, real(2) * pi) - pi


def _div(fx, fy, shape, real):
    r = np.zeros(shape, dtype=real)
    r[:, :-1] += fx
    r[:, 1:] -= fx
    r[:-1, :] += fy
    r[1:, :] -= fy
    return r


def _pcg(dx, dy, weight, kmax, compat, real, acc, fault, eps, workers):
    assert fault is None or fault in FAULTS, fault
    dx = _wrap(np.asarray(dx).astype(real), real)
    dy = _wrap(np.asarray(dy).astype(real), real)
    shape = (dx.shape[0], dy.shape[1])
    if weight is None:
        wwx, wwy = np.ones_like(dx), np.ones_like(dy)
    else:
        ww = np.asarray(weight).astype(real) ** 2
        wwx = np.minimum(ww[:, :-1], ww[:, 1:])
        wwy = np.minimum(ww[:-1, :], ww[1:, :])
        if fault == 'edge_last_col':      # the last column's edge takes the last pixel's weight, not the minimum
            wwx = wwx.copy()
            wwx[:, -1] = ww[:, -1]
    r = _div(wwx * dx, wwy * dy, shape, real)
    r0 = r.copy()
    eig = eig_table(shape, compat, real, shift0=1 if fault == 'eig_shift' else 0)
    kb = fault_bin(shape)
    if fault == 'eig_one':
        eig[kb] *= real(1 + 1e-3)

    def dot(u, v):
        return np.vdot(u.astype(acc), v.astype(acc))

    norm0 = np.sqrt(dot(r, r))
    phi = np.zeros(shape, dtype=real)
    k, rho_prev, p = 0, None, None
    while np.any(r != 0):
        R = sfft.dctn(r, norm='ortho', workers=workers)
        if fault == 'fwd_bin':            # one output bin of the forward transform scaled
            R[kb] *= real(1 + 1e-3)
        z = sfft.idctn(R / eig, norm='ortho', workers=workers)
        k += 1
        rho = dot(r, z)
        p = z if k == 1 else z + real(rho / rho_prev) * p
        rho_prev = rho
        q = _div(wwx * (p[:, 1:] - p[:, :-1]), wwy * (p[1:, :] - p[:-1, :]), shape, real)
        if fault == 'first_row_interior':  # the stencil's row 0 has an edge to a row above it (the image's last, as a wrapped index reads it)
            q[0, :] -= wwy[-1, :] * (p[0, :] - p[-1, :])
        alpha = real(rho / dot(p, q))
        phi = phi + alpha * p
        r = r - alpha * q
        if k >= kmax or np.sqrt(dot(r, r)) < eps * norm0:
            break
    assert phi.dtype == np.dtype(real) and r0.dtype == np.dtype(real)
    return phi, k, r0


def reference_pcg(dx, dy, weight, kmax, compat, real, eps=1e-9, workers=1):
    """(phi, iterations, r0) in the arithmetic `real` (np.longdouble or np.float64), dot products included"""
    return _pcg(dx, dy, weight, kmax, compat, real, real, None, eps, workers)


def emulate(dx, dy, weight, kmax, compat, real, fault=None, eps=1e-9, workers=1):
    """(phi, iterations, r0) of the same loop in the precision under test (np.float32 or np.float64); fault: one of FAULTS"""
    return _pcg(dx, dy, weight, kmax, compat, real, np.float64, fault, eps, workers)


def spectral_residual(phi, phi_ref, r0, eig, workers=1):
    """max_k |eig_k DCT(phi - phi_ref)_k| / rms(DCT(r0)), k = (0, 0) left out, in the arithmetic of phi_ref / eig (one precision
    above the code under test).  eig: the table the solve used (eig_table in that arithmetic).  The transform is
    orthonormal, so rms(DCT(r0)) = rms(r0)."""
    hi = phi_ref.dtype.type
    d = sfft.dctn(np.asarray(phi).astype(hi) - phi_ref, norm='ortho', workers=workers)
    num = np.abs(eig.astype(hi) * d)
    num[0, 0] = 0
    r0 = np.asarray(r0).astype(hi)
    return float(num.max() / np.sqrt(np.mean(r0 * r0)))


def mean_offset(phi, phi_ref):
    """|mean(phi) - mean(phi_ref)| / rms(phi_ref): the free mean, which the spectral measure leaves out"""
    hi = phi_ref.dtype.type
    return float(abs(np.mean(np.asarray(phi).astype(hi)) - np.mean(phi_ref)) / np.sqrt(np.mean(phi_ref * phi_ref)))


def check_args(phi0, weight, check):
    """(dx, dy, weight, kmax) of the three checks of a case: 'U' one unweighted iteration -- with the true eigenvalues an
    exact Poisson solve, phi0 minus its mean -- and 'W2' / 'W3', weighted, kmax 2 and 3"""
    dx, dy = diffs(phi0)
    return {'U': (dx, dy, None, 1), 'W2': (dx, dy, weight, 2), 'W3': (dx, dy, weight, 3)}[check]
