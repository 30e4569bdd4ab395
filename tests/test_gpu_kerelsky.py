"""Per-pixel Kerelsky fits on the device (gpa_kerelsky_fit[_dev], pygpa_amd.property_extract.Kerelsky_J / Kerelsky_Jac /
Kerelsky_J_dev) against the fixtures the reference wrote (tools/make_kerelsky_golden.py) and the bounds of tests/kerelsky_cases.py."""
import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.property_extract as pe

import kerelsky_cases as kc

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
_cache = {}


def fixture(name):
    if name not in _cache:
        z = kc.load(name)
        for v in z.values():
            v.setflags(write=False)
        _cache[name] = z
    return _cache[name]


def fit_case(name, dtype):
    """the device result of a whole field case, computed once per precision: (X (n0, n1, 4), cost (n0, n1))"""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        z = fixture(name)
        X, cost = _lib.kerelsky_fit(z['J'], z['refest_default'], a0=z['A0'], dtype=dtype)
        X.setflags(write=False)
        cost.setflags(write=False)
        _cache[key] = X, cost
    return _cache[key]


@pytest.mark.parametrize('name', list(kc.FIELD_CASES))
def test_parameters_and_cost_f64(name):
    z = fixture(name)
    X, cost = fit_case(name, np.float64)
    assert X.dtype == np.float64 and X.shape == z['X_tight'].shape and cost.dtype == np.float64
    dev = kc.check_solution(name, z, X, kc.bounds(), 'device f64')
    print('measured device deviations', dev)
    # the cost returned is the cost of what is returned
    A = kc.form_A(z['A0'], z['J'])
    assert np.abs(cost - kc.cost(X, A)).max() <= 1e-9 * (1 + cost.max())


@pytest.mark.parametrize('name', list(kc.FIELD_CASES))
def test_f32_build_is_the_f64_build_on_rounded_input(name):
    z = fixture(name)
    X32, cost32 = fit_case(name, np.float32)
    assert X32.dtype == np.float32 and cost32.dtype == np.float64
    J32 = z['J'].astype(np.float32)
    X64, cost64 = _lib.kerelsky_fit(J32.astype(np.float64), z['refest_default'], a0=z['A0'], dtype=np.float64)
    ulp = np.spacing(np.abs(X64.astype(np.float32)))
    assert (np.abs(X32.astype(np.float64) - X64) <= ulp).all()
    assert np.array_equal(cost32, cost64)
    assert (X32[..., 0] >= 0).all() and (X32[..., 2] >= 0).all()
    # (rounding theta to f32 alone moves the cost of a root pixel to about 1e-13, so the cost criterion is a statement about the
    # f64 output; for f32 the equality above carries it over.  The figure is printed.)
    c = kc.cost(X32, kc.form_A(z['A0'], J32))
    print('%s f32: cost of the rounded output - cost before rounding: max %.3e' % (name, (c - cost64).max()))


def test_ksets_global_fits():
    z = fixture(kc.KSETS)
    tol = kc.bounds()
    for i, (kvecs, sort, reference) in enumerate(kc.kset_inputs()):
        assert np.array_equal(kvecs, z['kvecs'][i])
        x = pe.Kerelsky_Jac(kvecs, nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, sort=sort, reference=reference)
        dev = kc.param_dev(x, z['X_tight'][i])
        slack = kc.param_dev(z['X_default'][i], z['X_tight'][i])
        dd = kc.param_dev(x, z['X_default'][i])
        print('kset %d: %s' % (i, dev))
        plain = x.copy()
        if reference == 'symmetric':
            plain[3] -= plain[0] / 2
        assert x[0] >= 0 and x[2] >= 0
        assert kc.cost(plain, z['A0'][i]) <= z['cost_default'][i] * (1 + kc.COST_REL) + z['cost_default'].max()
        for k in kc.PARAMS:
            assert dev[k] <= tol[k] and dd[k] <= slack[k] + tol[k], (i, k, dev[k], tol[k])


def test_mirror_is_the_library_call():
    z = fixture('smooth_24x20')
    X, refest = pe.Kerelsky_J(z['J'], z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0)
    tol = kc.bounds()
    dev = kc.param_dev(refest, z['refest_tight'])
    assert all(dev[k] <= tol[k] for k in kc.PARAMS), dev
    assert np.array_equal(X, _lib.kerelsky_fit(z['J'], refest, a0=z['A0'])[0])
    assert np.array_equal(pe.iterate_J_leastsq(kc.form_A(z['A0'], z['J']), refest, {'max_nfev': 50}), X)
    kc.check_solution('smooth_24x20', z, X, tol, 'mirror')


@pytest.mark.parametrize('dtype', DTYPES)
def test_indexing_and_divergence(dtype):
    """sub-ranges of one large call give the same bits, whatever the wave they fall in; a NaN pixel and a pixel that needs
    the second start leave their wave neighbours' bits alone (the rough case has pixels of both kinds side by side)"""
    z = fixture('rough_16x16')
    J = np.concatenate([z['J'].reshape(-1, 2, 2), fixture('smooth_24x20')['J'].reshape(-1, 2, 2)]).astype(dtype)
    x0 = z['refest_default']
    X, cost = _lib.kerelsky_fit(J, x0, a0=z['A0'], dtype=dtype)
    assert len(J) == 736 and np.isfinite(X).all()
    assert (cost[:256] > 1e-5).sum() >= 20 and (cost[:256] <= 1e-5).sum() >= 128     # both kinds of pixel
    for n in (1, 63, 64, 65, 257, 736):
        for off in (0, 3):
            Xn, cn = _lib.kerelsky_fit(J[off:off + n], x0, a0=z['A0'], dtype=dtype)
            assert np.array_equal(Xn, X[off:off + n]) and np.array_equal(cn, cost[off:off + n]), (n, off)
    Jn = J.copy()
    bad = [0, 70, 127, 128, 300]
    Jn[bad, 0, 1] = np.nan
    Jn[301, 1, 1] = np.inf
    Xb, cb = _lib.kerelsky_fit(Jn, x0, a0=z['A0'], dtype=dtype)
    keep = np.ones(len(J), dtype=bool)
    keep[bad + [301]] = False
    assert np.isnan(Xb[~keep]).all() and np.isnan(cb[~keep]).all()
    assert np.array_equal(Xb[keep], X[keep]) and np.array_equal(cb[keep], cost[keep])
    # the second start: without it (retry_cost inf) the pixels that needed it are worse or equal, the others keep their bits
    X1, c1 = _lib.kerelsky_fit(J, x0, a0=z['A0'], retry_cost=np.inf, dtype=dtype)
    one = c1 <= 1e-5
    assert np.array_equal(X1[one], X[one]) and np.array_equal(c1[one], cost[one]) and (c1[~one] >= cost[~one]).all()
    assert (c1[~one] > cost[~one]).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_consistency(dtype):
    z = fixture('rough_16x16')
    J = z['J'].astype(dtype).reshape(-1, 2, 2)
    x0, npx = z['refest_default'], 256
    X, cost = fit_case('rough_16x16', dtype)
    X, cost = X.reshape(-1, 4), cost.ravel()
    # run == run
    X2, c2 = _lib.kerelsky_fit(J, x0, a0=z['A0'], dtype=dtype)
    assert np.array_equal(X2, X) and np.array_equal(c2, cost)
    # _dev == host form, with and without the cost
    d_J, d_X, d_c = _lib.DeviceBuffer(J.nbytes), _lib.DeviceBuffer(X.nbytes), _lib.DeviceBuffer(8 * npx)
    d_J.upload(J)
    _lib.kerelsky_fit_dev(d_J.ptr, npx, x0, d_X.ptr, a0=z['A0'], cost_ptr=d_c.ptr, dtype=dtype)
    assert np.array_equal(d_X.download((npx, 4), dtype), X) and np.array_equal(d_c.download((npx,), np.float64), cost)
    d_X.upload(np.zeros_like(X))
    _lib.kerelsky_fit_dev(d_J.ptr, npx, x0, d_X.ptr, a0=z['A0'], dtype=dtype)
    assert np.array_equal(d_X.download((npx, 4), dtype), X)
    # a0 = NULL with A precomputed == a0 given with J (f64: A is formed in f64 and only an f64 array holds it)
    if dtype is np.float64:
        XA, cA = _lib.kerelsky_fit(kc.form_A(z['A0'], J), x0, dtype=dtype)
        assert np.array_equal(XA, X) and np.array_equal(cA, cost)
    else:
        XA, cA = _lib.kerelsky_fit(kc.form_A(z['A0'], J), x0, dtype=np.float64)
        assert np.array_equal(XA.astype(np.float32), X) and np.array_equal(cA, cost)
    # npx = 0 is a no-op
    assert _lib.kerelsky_fit(np.empty((0, 2, 2)), x0, dtype=dtype)[0].shape == (0, 4)
    for b in (d_J, d_X, d_c):
        b.free()


# The 64 x 64 golden's k-vectors (0.15 per pixel at 7, 67, 127 degrees) imply a twist of 2 asin(|k| / (2 r_k0)).  At 1 nm per
# pixel and a_0 = 0.246 nm that is 1.83 degrees, inside the 0.3 ... 2 degrees the fits are used at.  The image's J has a mean
# (J00: -1.6e-3), which moves the median twist by 0.36 % of the twist: 0.0066 degrees there.
CHAIN_NM, CHAIN_A0 = 1.0, 0.246


@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_chain(golden, dtype):
    g = golden('props_64')
    shape, npx = g['weights'].shape[1:], g['weights'][0].size
    plan = _lib.Plan(shape, 3, dtype)
    grads, w = np.ascontiguousarray(g['grads'], dtype=dtype), np.ascontiguousarray(g['weights'], dtype=dtype)
    esz = np.dtype(dtype).itemsize
    d_g, d_w, d_J, d_X = (_lib.DeviceBuffer(n) for n in (grads.nbytes, w.nbytes, 4 * npx * esz, 4 * npx * esz))
    d_g.upload(grads)
    d_w.upload(w)
    plan.phasegradient2J_dev(g['kvecs'], d_g.ptr, d_w.ptr, 1.0, d_J.ptr)        # dimensionless J
    refest = pe.Kerelsky_J_dev(d_J.ptr, npx, g['kvecs'], nmperpixel=CHAIN_NM, a_0=CHAIN_A0, dtype=dtype, out_ptr=d_X.ptr,
                               stream=plan.stream())
    plan.sync()
    X = d_X.download(shape + (4,), dtype)
    J = d_J.download(shape + (2, 2), dtype)
    Xh, refest_h = pe.Kerelsky_J(J, g['kvecs'], nmperpixel=CHAIN_NM, a_0=CHAIN_A0, dtype=dtype)
    assert np.array_equal(refest, refest_h) and np.array_equal(X, Xh) and np.isfinite(X).all()
    implied = np.rad2deg(2 * np.arcsin(np.linalg.norm(g['kvecs'], axis=1).mean() * CHAIN_A0 * np.sin(np.pi / 3) / CHAIN_NM / 2))
    print('twist: implied %.5f, global fit %.5f, median %.5f' % (implied, refest[0], np.median(X[..., 0])))
    assert abs(refest[0] - implied) <= 1e-2 and abs(np.median(X[..., 0]) - implied) <= 1e-2
    for b in (d_g, d_w, d_J, d_X):
        b.free()


def test_argument_errors_name_the_argument():
    lib = _lib.load()
    P = _lib._ptr
    a = np.zeros((4, 2, 2))
    x0, a0, out = np.array([1., 0., 0., 10.]), np.eye(2), np.zeros((4, 4))
    bad_x0 = [np.array([-1., 0., 0., 10.]), np.array([1., 0., -1e-3, 10.]), np.array([1., np.nan, 0., 10.]), np.array([1., 0., 7., 10.])]
    for sfx, tail in (('', ()), ('_dev', (None,))):
        f = getattr(lib, 'gpa_kerelsky_fit' + sfx)
        cases = [((0, 2, 4, P(a), P(a0), P(x0), 50, 1e-5, P(out), None), 'dtype'), ((0, 1, 4, None, P(a0), P(x0), 50, 1e-5, P(out), None), 'jac'),
                 ((0, 1, 4, P(a), P(a0), None, 50, 1e-5, P(out), None), 'x0'), ((0, 1, 4, P(a), P(a0), P(x0), 50, 1e-5, None, None), 'out'),
                 ((0, 1, 4, P(a), P(a0), P(x0), 0, 1e-5, P(out), None), 'max_nfev'),
                 ((0, 1, 4, P(a), P(a0), P(x0), 50, float('nan'), P(out), None), 'retry_cost'),
                 ((0, 1, 4, P(a), P(np.full((2, 2), np.inf)), P(x0), 50, 1e-5, P(out), None), 'a0'),
                 ((0, 1, 1 << 40, P(a), P(a0), P(x0), 50, 1e-5, P(out), None), 'npx')]
        cases += [((0, 1, 4, P(a), P(a0), P(b), 50, 1e-5, P(out), None), 'x0') for b in bad_x0]
        for args, word in cases:
            assert f(*(args + tail)) == -1
            assert word in _lib.last_error() and ('gpa_kerelsky_fit' + sfx + ':') in _lib.last_error(), (word, _lib.last_error())
    assert not out.any()
