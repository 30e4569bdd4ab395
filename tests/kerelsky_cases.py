"""Cases, restatements and bounds of the per-pixel Kerelsky fits (pygpa_amd.property_extract.Kerelsky_J / Kerelsky_Jac), shared
by tools/make_kerelsky_golden.py, tests/test_kerelsky_host.py and tests/test_gpu_kerelsky.py.

The four `latticegen` functions the reference's fits call are not available; the forms below are a DECLARED RESTATEMENT
(DESIGN.md 2.14), consistent with calc_abcd's delta = 0.16 (property_extract.py:511-520):
    rotation_matrix(a)   [[cos a, -sin a], [sin a, cos a]], a in radians
    strain_matrix(eps)   diag(1 / (1 + eps), 1 / (1 - 0.16 eps))
    generate_ks(r_k, t)  six vectors of length r_k at t + 0, 60, ..., 300 degrees
    a_0_to_r_k(a_0)      1 / (a_0 sin 60 degrees)
"""
import os
import subprocess

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 0.16
FIELD_CASES = {'smooth_24x20': ((24, 20), 1e-4, 11), 'rough_16x16': ((16, 16), 0.03, 7)}     # shape, noise on A, seed
KSETS = 'ksets'
NMPERPIXEL, A_0 = 0.5, 0.246
GLOBAL_X = (1.1, 25.0, 0.004, 12.0)          # the deformation the k-vectors of the field cases carry
TIGHT = dict(max_nfev=1000, xtol=1e-15, ftol=1e-15, gtol=1e-15)
DEFAULT = dict(max_nfev=50)
# a root pixel: the tight fit reaches cost <= ROOT_COST and the default and the tight results agree within ROOT_ANGLE degrees
# (psi mod 180, xi mod 360) and ROOT_EPS
ROOT_COST, ROOT_ANGLE, ROOT_EPS = 1e-20, 1e-6, 1e-9
ROOT_SHARE = {'smooth_24x20': 1.0, 'rough_16x16': 0.6}
NONROOT_COST_SLACK = 1e-4                     # default cost - tight cost on the other pixels
COST_REL = 1e-6

# Largest deviation of the solver from the tight fixture on root pixels, per parameter (theta, psi, xi in degrees, eps),
# measured for the host-compiled gpa_kerelsky.h and for the device; the bound is 8 x the larger (the sincos of the two maths
# libraries differ).  Measured, over the two field cases and the ten k-vector sets, host and device alike to the
# digits shown: theta 1.21e-13, psi 1.33e-9 (the k-vector set with eps = 1e-5; 1.8e-11 on the fields), eps 1.59e-15, xi 6.48e-12.
# Written rounded up; the host test holds the host solver to its figures.
MEASURED_HOST = dict(theta=1.3e-13, psi=1.4e-9, eps=1.6e-15, xi=6.5e-12)
MEASURED_DEVICE = dict(theta=1.3e-13, psi=1.4e-9, eps=1.6e-15, xi=6.5e-12)
PARAMS = ('theta', 'psi', 'eps', 'xi')


def bounds():
    return {k: 8 * max(MEASURED_HOST[k], MEASURED_DEVICE[k]) for k in PARAMS}


# ---- the restated latticegen functions ---------------------------------------------------------------------------------------
def rotation_matrix(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s], [s, c]])


def strain_matrix(epsilon, delta=DELTA):
    return np.array([[1 / (1 + epsilon), 0.], [0., 1 / (1 - delta * epsilon)]])


def generate_ks(r_k, theta, kz=None, sym=6):
    ang = np.deg2rad(theta + np.arange(sym) * (360. / sym))
    return r_k * np.stack([np.cos(ang), np.sin(ang)], axis=1)


def a_0_to_r_k(a_0, symmetry=6):
    return 1 / (a_0 * np.sin(np.deg2rad(60.)))


# ---- the model in NumPy, over any leading shape --------------------------------------------------------------------------------
def _W(a_deg):
    a = np.deg2rad(a_deg)
    c, s = np.cos(a), np.sin(a)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def model(x):
    """V^T D V W(theta + xi) - W(xi) for x (..., 4)"""
    x = np.asarray(x, dtype=np.float64)
    th, ps, ep, xi = (x[..., i] for i in range(4))
    V = _W(ps)
    D = np.zeros(x.shape[:-1] + (2, 2))
    D[..., 0, 0] = 1 / (1 + ep)
    D[..., 1, 1] = 1 / (1 - DELTA * ep)
    return np.swapaxes(V, -1, -2) @ D @ V @ _W(th + xi) - _W(xi)


def cost(x, A):
    """|1000 vec(model(x) - A)|^2 / 2 over the leading shape; NaN where x is"""
    F = (model(x) - np.asarray(A, dtype=np.float64)) * 1000
    return 0.5 * (F * F).sum(axis=(-1, -2))


def form_A(A0, J):
    """A0 + A0 J, element by element in the order the kernel uses (no fused operation): (..., 2, 2)"""
    J = np.asarray(J)
    A = np.empty(J.shape, dtype=np.float64)
    for i in range(2):
        for j in range(2):
            A[..., i, j] = A0[i, j] + (A0[i, 0] * J[..., 0, j].astype(np.float64) + A0[i, 1] * J[..., 1, j].astype(np.float64))
    return A


def a0_and_start(kvecs, nmperpixel, a_0, sort=0):
    """A0 (2 x 2) and the start of the global fit as property_extract.py:827-842 compute them"""
    from pygpa_amd.mathtools import periodic_average, periodic_difference
    kvecs = np.asarray(kvecs, dtype=np.float64)
    angles = np.arctan2(kvecs[:, 1], kvecs[:, 0])
    lk = kvecs / (a_0_to_r_k(a_0) * nmperpixel)
    if sort != 0:
        lk = lk[np.argsort(sort * periodic_difference(angles, periodic_average(angles)))]
    A0 = np.linalg.lstsq(generate_ks(1, 0)[:3], lk, rcond=None)[0].T
    return A0, np.array([.01, 0., 0., np.rad2deg(np.arctan2(lk[0, 1], lk[0, 0])) % 360])


# ---- cases -----------------------------------------------------------------------------------------------------------------
def kvecs_of(x, nmperpixel=NMPERPIXEL, a_0=A_0):
    """the three k-vectors (per pixel) of a lattice deformed by x: kvecs = k0s A^T r_k0"""
    return generate_ks(1, 0)[:3] @ model(np.asarray(x, dtype=np.float64)).T * (a_0_to_r_k(a_0) * nmperpixel)


def field_inputs(name):
    """J (n0, n1, 2, 2) and kvecs (3, 2) of a field case: smooth theta, psi, eps, xi fields, A = model + noise, J = A0^-1 (A - A0)"""
    (n0, n1), noise, seed = FIELD_CASES[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:n0, :n1] / max(n0, n1)
    x = np.empty((n0, n1, 4))
    x[..., 0] = 1.15 + 0.8 * np.sin(2.1 * xx + 0.3) * np.cos(1.7 * yy)          # 0.3 ... 2 degrees
    x[..., 1] = 25 + 30 * np.sin(1.3 * yy - 0.5 * xx)
    x[..., 2] = 0.004 + 0.0035 * np.cos(2.5 * xx + 1.1 * yy)                     # up to 0.008
    x[..., 3] = 12 + 4 * np.cos(1.9 * xx) * np.sin(2.3 * yy + 0.4)
    A = model(x) + noise * rng.standard_normal((n0, n1, 2, 2))
    kvecs = kvecs_of(GLOBAL_X)
    A0 = a0_and_start(kvecs, NMPERPIXEL, A_0)[0]
    return np.linalg.solve(A0, A - A0), kvecs


KSET_X = [(0.1, 10., 1e-5, 3.), (0.5, 70., 1e-3, 20.), (1.0, 130., 5e-3, 45.), (2.0, 40., 1e-2, 0.5), (5.0, 100., 3e-2, 33.),
          (12.0, 160., 5e-2, 50.), (30.0, 20., 8e-2, 10.), (45.0, 85., 0.1, 25.)]
KSET_EXTRA = [dict(x=(1.5, 60., 8e-3, 15.), sort=1, reference=None), dict(x=(3.0, 35., 2e-2, 8.), sort=0, reference='symmetric')]


def kset_inputs():
    """[(kvecs, sort, reference)]: the eight plain sets, one with sort = 1 (given in scrambled order), one with reference='symmetric'"""
    sets = [(kvecs_of(x), 0, None) for x in KSET_X]
    for e in KSET_EXTRA:
        k = kvecs_of(e['x'])
        sets.append((k[[1, 2, 0]] if e['sort'] else k, e['sort'], e['reference']))
    return sets


def load(name):
    with np.load(os.path.join(GOLDEN, 'kerelsky_%s.npz' % name)) as z:
        return {k: z[k] for k in z.files}


def angle_diff(a, b, period):
    return np.abs((a - b + period / 2) % period - period / 2)


def param_dev(x, ref):
    """largest |x - ref| per parameter over the leading shape: psi mod 180, xi mod 360"""
    x, ref = np.asarray(x, dtype=np.float64).reshape(-1, 4), np.asarray(ref, dtype=np.float64).reshape(-1, 4)
    if len(x) == 0:
        return dict.fromkeys(PARAMS, 0.0)
    return dict(theta=float(np.abs(x[:, 0] - ref[:, 0]).max()), psi=float(angle_diff(x[:, 1], ref[:, 1], 180.).max()),
                eps=float(np.abs(x[:, 2] - ref[:, 2]).max()), xi=float(angle_diff(x[:, 3], ref[:, 3], 360.).max()))


def root_pixels(z):
    """the mask of root pixels of a loaded field fixture"""
    d, t = z['X_default'].reshape(-1, 4), z['X_tight'].reshape(-1, 4)
    ok = z['cost_tight'].ravel() <= ROOT_COST
    ok &= (np.abs(d[:, 0] - t[:, 0]) <= ROOT_ANGLE) & (angle_diff(d[:, 1], t[:, 1], 180.) <= ROOT_ANGLE)
    ok &= (np.abs(d[:, 2] - t[:, 2]) <= ROOT_EPS) & (angle_diff(d[:, 3], t[:, 3], 360.) <= ROOT_ANGLE)
    return ok.reshape(z['cost_tight'].shape)


def fixture_promises(name, z):
    """what the tests rely on, asserted by the generator and again by the host tests; returns the root mask"""
    root = root_pixels(z)
    assert root.mean() >= ROOT_SHARE[name], (name, root.mean())
    if (~root).any():
        assert (z['cost_default'][~root] - z['cost_tight'][~root]).max() <= NONROOT_COST_SLACK, name
    assert float(z['root_cost_max']) == float(z['cost_default'][root].max())
    return root


def check_solution(name, z, X, tol, label=''):
    """The acceptance checks of one field case for a solver's X (n0, n1, 4), inputs as stored: returns the measured deviations.
    tol: dict of per-parameter bounds, or None to measure only."""
    X = np.asarray(X, dtype=np.float64)
    root = root_pixels(z)
    assert np.isfinite(X).all() and (X[..., 0] >= 0).all() and (X[..., 2] >= 0).all(), name
    dev = param_dev(X[root], z['X_tight'][root])
    slack = param_dev(z['X_default'][root], z['X_tight'][root])
    dev_default = param_dev(X[root], z['X_default'][root])
    A = form_A(z['A0'], z['J'])
    c = cost(X, A)
    limit = z['cost_default'] * (1 + COST_REL) + float(z['root_cost_max'])
    worst = float((c - limit).max())
    print('%s %s: root %d / %d  dev from tight %s  largest cost %.3e  worst cost - limit %.3e' %
          (label, name, root.sum(), root.size, ' '.join('%s %.2e' % kv for kv in dev.items()), c.max(), worst))
    if tol is not None:
        for k in PARAMS:
            assert dev[k] <= tol[k], (name, k, dev[k], tol[k])
            assert dev_default[k] <= slack[k] + tol[k], (name, k, dev_default[k])
    assert (c <= limit).all(), (name, int((c > limit).sum()), worst)
    return dev


# ---- the host-compiled solver -------------------------------------------------------------------------------------------------
def build_check(tmpdir, extra=()):
    """compile tests/host/kerelsky_check.cpp against pygpa_amd/csrc/gpa_kerelsky.h with the host compiler: (result, exe)"""
    import prep_cases as pc
    exe = os.path.join(str(tmpdir), 'kerelsky_check')
    cmd = [pc._host_cxx(), '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc')] + list(extra)
    r = subprocess.run(cmd + [os.path.join(ROOT, 'tests', 'host', 'kerelsky_check.cpp'), '-o', exe], capture_output=True, text=True)
    return r, exe


def host_solve(exe, tmpdir, A, x0, max_nfev=50, retry_cost=1e-5, a0=None):
    """run the host program on pixels `A` (n, 2, 2) (or J with a0): (X (n, 4), cost (n,), nfev (n,))"""
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 4)
    fin, fout = os.path.join(str(tmpdir), 'in.bin'), os.path.join(str(tmpdir), 'out.bin')
    head = np.concatenate([[len(A), max_nfev, retry_cost, 0. if a0 is None else 1.], np.asarray(x0, dtype=np.float64).ravel(),
                           np.zeros(4) if a0 is None else np.asarray(a0, dtype=np.float64).ravel()])
    with open(fin, 'wb') as f:
        f.write(head.astype(np.float64).tobytes())
        f.write(A.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = np.fromfile(fout, dtype=np.float64).reshape(len(A), 6)
    return out[:, :4], out[:, 4], out[:, 5].astype(np.int64)
