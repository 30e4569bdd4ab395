"""Cases, restatements and bounds of the field / phases -> Jacobian functions of pygpa_amd.property_extract (u2J, phases2J,
calc_props_from_phases, phys_props_from_Jac), shared by tools/make_jac_golden.py, tests/test_jac_host.py and
tests/test_gpu_jac.py.

The phase fixtures are GPA phases of a displaced hexagonal carrier: phase_p = 2 pi k_p . u(r) with u a linear part plus a smooth
wave, taken through np.angle (the wrapped cases) or left as they are (the unwrapped case, kept within |phase| < 12 rad: an f32
phase of magnitude x carries x 2^-24 of rounding, which the solve divides by 2 pi |k| nmperpixel).  The doubled difference of two
wrapped phases jumps by 2 pi wherever a wrap lies between the two samples; those are the differences wrapToPi has to fold back.
"""
import os
import re

import numpy as np

from oracle import gpa_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'pygpa_amd', 'csrc', 'gpa_fieldjac.h')

# name -> shape, P, wrapped, pixel whose weights are all zero (or None), seed, gain on the displacement (the tiny frames need a
# steeper field to hold a wrap at all)
CASES = {
    'hex_37x70': ((37, 70), 3, True, None, 1, 1.0),
    'p2_2x9': ((2, 9), 2, True, None, 2, 2.5),
    'p2_9x2': ((9, 2), 2, True, None, 3, 2.5),
    'p3_3x300': ((3, 300), 3, True, None, 4, 1.0),
    'p8_24x20': ((24, 20), 8, True, None, 5, 1.0),
    'unwrapped_12x16': ((12, 16), 3, False, None, 6, 1.0),
    'zero_weight_13x11': ((13, 11), 3, True, (5, 7), 7, 1.0),
}
NMPERPIXEL = 3.7            # the reference's own default resolution (calc_moire_props_from_kvecs)
SEAM_MARGIN = 1e-3          # every wrapped argument stays this far from +-pi: no wrap decision can flip in f32
WRAP_SHARE = 0.05           # at least this share of the differences wraps in the wrapped cases
KAPPA_MIN = 1.001           # pixels whose anisotropy direction is compared
POISSON = 0.16

# u2J shapes of the GPU test beside the one read from the tile constants, and the spacings of the host test
U_SHAPES = [(2, 2), (2, 9), (9, 2), (3, 300), (300, 3), (37, 70)]
SPACINGS = [1, 0.5, 3.7, 0.37]


def j_bound(dtype):
    """the project's bound for this solve (tests/test_gpu_parity.py, test_f2_jacobian_and_props_golden), times max|J|"""
    return 2e-5 if np.dtype(dtype) == np.float32 else 1e-11


def tile_constants():
    """FJ_ROWS, FJ_LANES, FJ_VEC_BYTES of csrc/gpa_fieldjac.h"""
    src = open(HEADER).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % n, src).group(1)) for n in ('FJ_ROWS', 'FJ_LANES', 'FJ_VEC_BYTES'))


def ragged_shape():
    """two tiles and a ragged remainder along both axes, for the wider (f32) tile"""
    rows, lanes, vec_bytes = tile_constants()
    return 2 * rows + 5, 2 * lanes * (vec_bytes // 4) + 3


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def kvecs_of(P):
    if P <= 3:
        ang = np.deg2rad(7. + 60. * np.arange(3))[:P]
        r = 0.11 * np.ones(P)
    else:
        ang = np.deg2rad(7. + 180. / P * np.arange(P))
        r = 0.08 + 0.04 * (np.arange(P) % 3) / 2
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)


def displacement(shape, seed, gain=1.0):
    """a smooth displacement field (2, N, M) in pixels: a linear part and one wave"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing='ij')
    M = np.array([[0.45, -0.3], [0.35, 0.5]]) + 0.05 * rng.normal(size=(2, 2))
    amp, per, ph = 1.5 + rng.random(2), 35. + 10 * rng.random(2), 2 * np.pi * rng.random(2)
    wave = np.stack([amp[c] * np.sin(2 * np.pi * (x + 0.6 * y) / per[c] + ph[c]) for c in range(2)])
    off = 3 * rng.random(2)
    return gain * (np.stack([M[c, 0] * x + M[c, 1] * y + off[c] for c in range(2)]) + wave)


def phase_inputs(name, shape=None):
    """(kvecs, phases, weights, nmperpixel) of a case, f64; `shape` overrides the case's (the tile-sized GPU case)"""
    cshape, P, wrapped, zero_px, seed, gain = CASES[name]
    shape = cshape if shape is None else shape
    kvecs = kvecs_of(P)
    u = displacement(shape, seed, gain)
    if not wrapped:
        u = u - u.mean(axis=(1, 2), keepdims=True)
    phases = 2 * np.pi * np.einsum('pc,cnm->pnm', kvecs, u)
    if wrapped:
        phases = np.angle(np.exp(1j * phases))
    rng = np.random.default_rng(1000 + seed)
    x, y = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing='ij')
    weights = np.stack([0.6 + 0.35 * np.sin(0.21 * x + 0.13 * y + p) for p in range(P)]) + 0.05 * rng.random((P,) + tuple(shape))
    if zero_px is not None:
        weights[(slice(None),) + tuple(zero_px)] = 0.
    return kvecs, phases, weights, NMPERPIXEL


def field_input(shape, seed=0):
    """a displacement field (2, N, M) with no structure the stencil could hide behind"""
    return np.random.default_rng(seed).normal(size=(2,) + tuple(shape)) * 3.


# ---- restatements ------------------------------------------------------------------------------------------------------------
def wrap_to_pi(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


def edge_diff(f, axis):
    """f[i+1] - f[i-1] inside and the one-sided difference at the two ends of `axis`, and the sample distance of each (2 or 1)"""
    f = np.moveaxis(f, axis, 0)
    d = np.empty_like(f)
    d[1:-1] = f[2:] - f[:-2]
    d[0] = f[1] - f[0]
    d[-1] = f[-1] - f[-2]
    span = np.full(f.shape[0], 2)
    span[[0, -1]] = 1
    return np.moveaxis(d, 0, axis), span.reshape([-1 if a == axis % f.ndim else 1 for a in range(f.ndim)])


def u2J_np(U, h):
    """the edge rule of gpa_fieldjac.h in NumPy, in U's own precision: J[n, m, c, a] = (-U_c[hi] - -U_c[lo]) / T(h (hi - lo))"""
    U = np.asarray(U)
    T = U.dtype.type
    J = np.empty(U.shape[1:] + (2, 2), dtype=U.dtype)
    for a in range(2):
        d, span = edge_diff(-U, 1 + a)
        div = np.where(span == 2, T(2.0 * h), T(h)).astype(U.dtype)
        J[..., a] = np.moveaxis(d / div, 0, -1)
    return J


def u2J_gradient(U, h):
    """u2J as the reference writes it (property_extract.py:13-18)"""
    return np.moveaxis(np.stack(np.gradient(-U, h, axis=(1, 2)), axis=-1), 0, -2)


def doubled_differences(phases):
    """2 np.gradient(phases) along the two image axes: (2, P, N, M)"""
    out = []
    for axis in (1, 2):
        d, span = edge_diff(phases, axis)
        out.append(np.where(span == 2, d, 2 * d))
    return np.stack(out)


def seam_margin_and_share(phases):
    """(smallest distance of a doubled difference from the seam at +-pi, share of the differences that wrap)"""
    d = doubled_differences(np.asarray(phases, dtype=np.float64))
    t = (d + np.pi) % (2 * np.pi)
    return float(np.minimum(t, 2 * np.pi - t).min()), float((np.abs(d) >= np.pi).mean())


def phases2J_np(kvecs, phases, weights, nmperpixel):
    """phases2J (property_extract.py:39-52) on the oracle's weighted least squares"""
    K = 2 * np.pi * np.asarray(kvecs, dtype=np.float64)
    b = wrap_to_pi(doubled_differences(np.asarray(phases, dtype=np.float64))) / 2 / nmperpixel
    w = np.asarray(weights, dtype=np.float64)
    J = -np.stack([orc.weighted_lstsq(b[0], K, w), orc.weighted_lstsq(b[1], K, w)], axis=-1)
    return np.moveaxis(J, 0, -2)


def load(name):
    with np.load(os.path.join(GOLDEN, 'jac_%s.npz' % name)) as z:
        return {k: z[k] for k in z.files}


def pdiff(x, y, period):
    return (np.asarray(x) - y + period / 2) % period - period / 2


def check_props(props, ref, dtype, last='kappa', kappa=None):
    """the bounds of test_f2_jacobian_and_props_golden (tests/test_gpu_parity.py) for (angle, aniangle, alpha, kappa); with
    last='epsilon' the fourth map is held to kappa's relative bound times kappa.max(), as an absolute bound.  Prints each figure
    before it asserts."""
    f32 = np.dtype(dtype) == np.float32
    kap = ref[3] if kappa is None else kappa
    ok = kap > KAPPA_MIN
    tol_ani = (2e-5 if f32 else 1e-11) * (1 + 1 / (kap[ok] - 1)) * 57.3
    d_angle = np.abs(pdiff(props[0], ref[0], 360)).max()
    d_ani = (np.abs(pdiff(props[1], ref[1], 180))[ok] / tol_ani).max() if ok.any() else 0.
    atol_alpha = (2e-6 if f32 else 1e-13) * np.abs(ref[2] * kap).max()
    d_alpha = (np.abs(props[2] - ref[2]) / (atol_alpha + (1e-5 if f32 else 1e-12) * np.abs(ref[2]))).max()
    rtol_last = (2e-5 if f32 else 1e-11) * kap.max()
    if last == 'kappa':
        d_last = (np.abs(props[3] - ref[3]) / (1e-8 + rtol_last * np.abs(ref[3]))).max()
    else:
        d_last = (np.abs(props[3] - ref[3]) / rtol_last).max()
    print('%s: angle %.3g deg (bound %.3g), aniangle %.3g of its bound, alpha %.3g of its bound, %s %.3g of its bound'
          % (np.dtype(dtype).name, d_angle, 1e-4 if f32 else 1e-10, d_ani, d_alpha, last, d_last))
    assert props.shape == ref.shape
    assert d_angle <= (1e-4 if f32 else 1e-10)
    assert d_ani <= 1
    assert d_alpha <= 1
    assert d_last <= 1


# ---- the argument errors of the C ABI (include/gpa_hip.h), shared by the host and the GPU test -----------------------------------
def field_errors(P, buf):
    """(arguments of gpa_field_jacobian after `device`, the word its error must hold)"""
    u, J, props = P(buf['u']), P(buf['J']), P(buf['props'])
    ok = dict(dtype=1, nimg=1, n0=4, n1=5, u=u, nm=0.5, ident=0, J=J, props=props)
    cases = [(dict(dtype=7), 'dtype'), (dict(nimg=0), 'nimg'), (dict(n0=1), 'n0'), (dict(n1=1), 'n1'), (dict(u=None), 'u'),
             (dict(nm=0.0), 'nmperpixel'), (dict(nm=float('nan')), 'nmperpixel'), (dict(nm=float('inf')), 'nmperpixel'),
             (dict(J=None, props=None), 'both null'), (dict(J=u), 'J overlaps u'), (dict(props=u), 'props overlaps u'),
             (dict(props=J), 'props overlaps J')]
    for change, word in cases:
        a = dict(ok, **change)
        yield (a['dtype'], a['nimg'], a['n0'], a['n1'], a['u'], a['nm'], a['ident'], a['J'], a['props'], 0., 1., 0), word


def phases_errors(P, buf):
    ph, w, J, props, k = P(buf['ph']), P(buf['w']), P(buf['J']), P(buf['props']), P(buf['k'])
    ok = dict(dtype=1, n0=4, n1=5, P=3, k=k, ph=ph, w=w, nm=0.5, ident=0, J=J, props=props)
    cases = [(dict(dtype=-1), 'dtype'), (dict(n0=1), 'n0'), (dict(n1=0), 'n1'), (dict(P=1), 'P'), (dict(P=9), 'P'),
             (dict(k=None), 'kvecs'), (dict(k=P(np.full((3, 2), np.inf))), 'kvecs'), (dict(ph=None), 'phases'),
             (dict(w=None), 'weights'), (dict(nm=0.0), 'nmperpixel'), (dict(nm=float('nan')), 'nmperpixel'),
             (dict(J=None, props=None), 'both null'), (dict(J=ph), 'J overlaps phases'), (dict(J=w), 'J overlaps weights'),
             (dict(props=ph), 'props overlaps phases'), (dict(props=w), 'props overlaps weights'), (dict(props=J), 'props overlaps J')]
    for change, word in cases:
        a = dict(ok, **change)
        yield (a['dtype'], a['n0'], a['n1'], a['P'], a['k'], a['ph'], a['w'], a['nm'], a['ident'], a['J'], a['props'], 0., 1., 0), word


def phys_errors(P, buf):
    J, props = P(buf['J']), P(buf['props'])
    for args, word in [((7, 20, J, 0, 0., 1., 0, 0.16, props), 'dtype'), ((1, 20, None, 0, 0., 1., 0, 0.16, props), 'jac'),
                       ((1, 20, J, 0, 0., 1., 0, 0.16, None), 'props'), ((1, 20, J, 0, 0., 1., 0, float('nan'), props), 'poisson_ratio'),
                       ((1, 20, J, 0, 0., 1., 0, 0.16, J), 'props overlaps jac')]:
        yield args, word


def error_buffers():
    """the arrays the error tables point at, carved from one arena a slot apart: an output aimed at one input overlaps that input
    and nothing else, wherever the allocator puts things"""
    arena = np.zeros(6 * 1024)
    shapes = dict(u=(2, 4, 5), J=(4, 5, 2, 2), props=(4, 4, 5), ph=(3, 4, 5), w=(3, 4, 5))
    buf = {k: arena[1024 * i:1024 * i + int(np.prod(sh))].reshape(sh) for i, (k, sh) in enumerate(shapes.items())}
    buf['k'] = np.array([[0.1, 0.], [0., 0.1], [0.07, 0.07]])
    return buf


ERROR_TABLES = {'gpa_field_jacobian': field_errors, 'gpa_phases_jacobian': phases_errors, 'gpa_phys_props_from_jac': phys_errors}
