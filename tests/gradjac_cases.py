"""Inputs and the argument-error table of gpa_gradients_jacobian (phase gradients and weights of a stack -> J and lattice
properties in one pass), shared by tests/test_gradjac_host.py and tests/test_gpu_gradjac.py."""
import numpy as np

NMPERPIXEL = 0.5
# a single pixel, fewer pixels than a wave, a whole number of vectors, a ragged tail, several waves
SHAPES = [(1, 1), (3, 5), (7, 64), (9, 67), (64, 64)]
PEAKS = [2, 3, 8]


def kvecs_of(P):
    ang = np.deg2rad(7. + 180. / P * np.arange(P))
    r = 0.08 + 0.04 * (np.arange(P) % 3) / 2
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)


def dks_of(P):
    """a turn per k-vector large enough that g - 2 pi dk leaves (-pi, pi] on a share of the pixels"""
    rng = np.random.default_rng(100 + P)
    return 0.2 * rng.uniform(-1, 1, size=(P, 2))


def zero_pixel(shape, b):
    """the pixel of frame b whose weights are all 0 (another one in every frame)"""
    n = shape[0] * shape[1]
    return np.unravel_index((5 * b + 3) % n, shape)


def inputs(nimg, P, shape, dtype, seed=0):
    """(grads (nimg, P, N, M, 2) in (-pi, pi], weights (nimg, P, N, M) > 0 except one all-zero pixel per frame), in `dtype`;
    every frame its own random numbers"""
    rng = np.random.default_rng(1000 * seed + 10 * P + nimg)
    grads = -rng.uniform(-np.pi, np.pi, size=(nimg, P) + tuple(shape) + (2,))
    weights = 0.1 + rng.random((nimg, P) + tuple(shape))
    for b in range(nimg):
        weights[(b, slice(None)) + tuple(zero_pixel(shape, b))] = 0.
    return grads.astype(dtype), weights.astype(dtype)


# ---- the argument errors of the C ABI ------------------------------------------------------------------------------------------
def error_buffers():
    """the arrays the error table points at, carved from one arena a slot apart"""
    arena = np.zeros(6 * 1024)
    shapes = dict(g=(3, 4, 5, 2), w=(3, 4, 5), J=(4, 5, 2, 2), props=(4, 4, 5))
    buf = {k: arena[1024 * i:1024 * i + int(np.prod(sh))].reshape(sh) for i, (k, sh) in enumerate(shapes.items())}
    buf['k'] = np.array([[0.1, 0.], [0., 0.1], [0.07, 0.07]])
    buf['dk'] = np.zeros((3, 2))
    return buf


def gradients_errors(P, buf):
    """(arguments of gpa_gradients_jacobian after `device`, the word its error must hold)"""
    g, w, J, props, k, dk = (P(buf[n]) for n in ('g', 'w', 'J', 'props', 'k', 'dk'))
    ok = dict(dtype=1, nimg=1, n0=4, n1=5, P=3, k=k, dk=dk, g=g, w=w, nm=0.5, ident=0, J=J, props=props)
    cases = [(dict(dtype=7), 'dtype'), (dict(nimg=0), 'nimg'), (dict(n0=0), 'n0'), (dict(n1=-1), 'n1'), (dict(P=1), 'P'),
             (dict(P=9), 'P'), (dict(k=None), 'kvecs'), (dict(k=P(np.full((3, 2), np.inf))), 'kvecs'),
             (dict(dk=P(np.full((3, 2), np.nan))), 'dks'), (dict(g=None), 'grads'), (dict(w=None), 'weights'),
             (dict(nm=0.0), 'nmperpixel'), (dict(nm=float('nan')), 'nmperpixel'), (dict(nm=float('inf')), 'nmperpixel'),
             (dict(J=None, props=None), 'both null'), (dict(n0=1 << 16, n1=1 << 16), 'beyond one launch'),
             (dict(J=g), 'J overlaps grads'), (dict(J=w), 'J overlaps weights'), (dict(props=g), 'props overlaps grads'),
             (dict(props=w), 'props overlaps weights'), (dict(props=J), 'props overlaps J')]
    for change, word in cases:
        a = dict(ok, **change)
        yield (a['dtype'], a['nimg'], a['n0'], a['n1'], a['P'], a['k'], a['dk'], a['g'], a['w'], a['nm'], a['ident'], a['J'],
               a['props'], 0., 1., 0), word
