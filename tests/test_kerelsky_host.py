"""The Kerelsky fits without a GPU: the fixtures the reference wrote against the NumPy restatement of tests/kerelsky_cases.py, the
solver header compiled for the host (tests/host/kerelsky_check.cpp, plain and under the host sanitizers -- an ordinary
executable) on every fixture pixel with the bounds the GPU tests use, the C ABI's symbols and argument errors, and the Python
mirror against a recording stand-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.property_extract as pe

import kerelsky_cases as kc
import prep_cases as pc

SYMBOLS = {'gpa_kerelsky_fit': 10, 'gpa_kerelsky_fit_dev': 11}
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def _cost_tol(c):
    """two evaluations of the same formula: each of the four elements of F carries a few roundings of numbers of size 1, times
    1000, say e = 2e-12; the costs then differ by at most 2 sqrt(2 c) e + 2 e^2"""
    e = 2e-12
    return 2 * np.sqrt(2 * c) * e + 2 * e * e


@pytest.mark.parametrize('name', list(kc.FIELD_CASES))
def test_field_fixture_promises_and_restatement(name):
    z = kc.load(name)
    shape = kc.FIELD_CASES[name][0]
    J, kvecs = kc.field_inputs(name)
    assert np.array_equal(z['J'], J) and np.array_equal(z['kvecs'], kvecs) and z['J'].shape == shape + (2, 2)
    assert float(z['nmperpixel']) == kc.NMPERPIXEL and float(z['a_0']) == kc.A_0
    assert os.path.getsize(os.path.join(kc.GOLDEN, 'kerelsky_%s.npz' % name)) < 1 << 20
    assert all(v.dtype.kind in 'fib' for v in z.values())                 # numeric arrays only
    A0, est = kc.a0_and_start(kvecs, kc.NMPERPIXEL, kc.A_0)
    assert np.array_equal(z['A0'], A0)
    root = kc.fixture_promises(name, z)
    print('%s: %d of %d root pixels' % (name, root.sum(), root.size))
    A = A0 + A0 @ J                                                       # what the reference fitted
    assert np.abs(kc.form_A(A0, J) - A).max() <= 4 * np.finfo(float).eps * np.abs(A0).sum() * (1 + np.abs(J).max())
    for tag in ('default', 'tight'):
        c = kc.cost(z['X_' + tag], A)
        assert (np.abs(c - z['cost_' + tag]) <= _cost_tol(z['cost_' + tag])).all(), tag
        assert (z['X_' + tag][..., 0] >= 0).all() and (z['X_' + tag][..., 2] >= 0).all()
    # the mirror's residual is the restatement
    x = z['X_default'][3, 5]
    assert 0.5 * np.sum(pe.Jac_fit_diff(x, A[3, 5]) ** 2) == pytest.approx(float(kc.cost(x, A[3, 5])), rel=1e-12, abs=1e-30)


def test_kset_fixture():
    z = kc.load(kc.KSETS)
    sets = kc.kset_inputs()
    assert len(sets) == 10 and z['kvecs'].shape == (10, 3, 2)
    truth = np.array(kc.KSET_X + [e['x'] for e in kc.KSET_EXTRA])
    assert truth[:8, 0].min() == 0.1 and truth[:8, 0].max() == 45 and truth[:8, 2].min() == 1e-5 and truth[:8, 2].max() == 0.1
    for i, (kvecs, sort, reference) in enumerate(sets):
        assert np.array_equal(z['kvecs'][i], kvecs) and z['sort'][i] == sort and bool(z['symmetric'][i]) == (reference == 'symmetric')
        assert np.array_equal(z['A0'][i], kc.a0_and_start(kvecs, kc.NMPERPIXEL, kc.A_0, sort=sort)[0])
    assert z['cost_tight'].max() <= kc.ROOT_COST
    plain = z['X_tight'].copy()
    plain[z['symmetric'], 3] -= plain[z['symmetric'], 0] / 2
    dev = kc.param_dev(plain, truth)     # the reference's fit returns the deformation the k-vectors were made with
    assert dev['theta'] <= 1e-9 and dev['psi'] <= 1e-6 and dev['eps'] <= 1e-12 and dev['xi'] <= 1e-9, dev
    assert (np.abs(kc.cost(plain, z['A0']) - z['cost_tight']) <= _cost_tol(z['cost_tight'])).all()


def test_bounds_are_eight_times_the_larger_measurement():
    b = kc.bounds()
    for k in kc.PARAMS:
        assert kc.MEASURED_HOST[k] > 0 and kc.MEASURED_DEVICE[k] > 0
        assert b[k] == 8 * max(kc.MEASURED_HOST[k], kc.MEASURED_DEVICE[k])
        # far inside what makes a root pixel: the bound separates roots, it does not blur them
        assert b[k] <= 0.1 * (kc.ROOT_EPS if k == 'eps' else kc.ROOT_ANGLE)


# ---- the header, compiled for the host --------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def check_exe(request, tmp_path_factory):
    extra = SANITIZE if request.param == 'sanitized' else []
    if extra and not pc.host_compiler_links(tmp_path_factory.mktemp('probe'), extra):
        pytest.skip('the host compiler has no sanitizer runtimes')
    r, exe = kc.build_check(tmp_path_factory.mktemp('kerelskycheck'), extra)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_header_self_check(check_exe):
    import subprocess
    out = subprocess.run([check_exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 40000


@pytest.mark.parametrize('name', list(kc.FIELD_CASES))
def test_host_solver_on_field_fixtures(check_exe, tmp_path, name):
    z = kc.load(name)
    X, cost, nfev = kc.host_solve(check_exe, tmp_path, z['J'], z['refest_default'], a0=z['A0'])
    shape = z['X_tight'].shape
    dev = kc.check_solution(name, z, X.reshape(shape), kc.bounds(), 'host')
    for k in kc.PARAMS:
        assert dev[k] <= kc.MEASURED_HOST[k], (k, dev[k])          # the figures written down are the figures
    A = kc.form_A(z['A0'], z['J']).reshape(-1, 2, 2)
    assert np.abs(cost - kc.cost(X, A)).max() <= 1e-9 * (1 + cost.max())
    assert nfev.min() >= 1 and nfev.max() <= 3 * 50
    print('%s: trial evaluations per pixel: mean %.2f, max %d' % (name, nfev.mean(), nfev.max()))
    # a0 = NULL with A itself is the same solve
    XA, cA, _ = kc.host_solve(check_exe, tmp_path, A, z['refest_default'])
    assert np.array_equal(XA, X) and np.array_equal(cA, cost)


def test_host_solver_on_ksets(check_exe, tmp_path):
    z = kc.load(kc.KSETS)
    tol = kc.bounds()
    for i, (kvecs, sort, reference) in enumerate(kc.kset_inputs()):
        A0, est = kc.a0_and_start(kvecs, kc.NMPERPIXEL, kc.A_0, sort=sort)
        X, cost, nfev = kc.host_solve(check_exe, tmp_path, A0[None], est, max_nfev=400, retry_cost=1e-20)
        assert cost[0] <= z['cost_default'][i] * (1 + kc.COST_REL) + z['cost_default'].max() and X[0, 0] >= 0 and X[0, 2] >= 0
        x = X[0].copy()
        if reference == 'symmetric':
            x[3] += x[0] / 2
        dev, slack, dd = kc.param_dev(x, z['X_tight'][i]), kc.param_dev(z['X_default'][i], z['X_tight'][i]), kc.param_dev(x, z['X_default'][i])
        for k in kc.PARAMS:
            assert dev[k] <= tol[k] and dd[k] <= slack[k] + tol[k] and dev[k] <= kc.MEASURED_HOST[k], (i, k, dev[k])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_signatures():
    header = open(os.path.join(kc.ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, n in SYMBOLS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        res, args = _lib.SIGNATURES[name]
        assert nargs == len(args) == n and res is _lib._i, name
    build = open(os.path.join(kc.ROOT, 'pygpa_amd', 'build.py')).read()
    assert "'gpa_kerelsky.hip'" in build and "'gpa_api_kerelsky.hip'" in build and "'gpa_kerelsky.hip': ['-ffp-contract=off']" in build


def test_library_argument_errors_need_no_device():
    lib = _lib.load()
    P = _lib._ptr
    a, x0, out = np.zeros((4, 2, 2)), np.array([1., 0., 0., 10.]), np.zeros((4, 4))
    for sfx, tail in (('', ()), ('_dev', (None,))):
        f = getattr(lib, 'gpa_kerelsky_fit' + sfx)
        for args, word in [((0, 7, 4, P(a), None, P(x0), 50, 1e-5, P(out), None), 'dtype'), ((0, 1, 4, None, None, P(x0), 50, 1e-5, P(out), None), 'jac'),
                           ((0, 1, 4, P(a), None, None, 50, 1e-5, P(out), None), 'x0'), ((0, 1, 4, P(a), None, P(x0), 50, 1e-5, None, None), 'out'),
                           ((0, 1, 4, P(a), None, P(x0), 0, 1e-5, P(out), None), 'max_nfev'),
                           ((0, 1, 4, P(a), None, P(x0), 50, float('nan'), P(out), None), 'retry_cost'),
                           ((0, 1, 4, P(a), P(np.full(4, np.nan)), P(x0), 50, 1e-5, P(out), None), 'a0'),
                           ((0, 1, 4, P(a), None, P(np.array([-1., 0., 0., 0.])), 50, 1e-5, P(out), None), 'x0')]:
            assert f(*(args + tail)) == -1
            assert word in _lib.last_error() and ('gpa_kerelsky_fit' + sfx + ':') in _lib.last_error(), (word, _lib.last_error())
        assert f(*((0, 1, 0, P(a), None, P(x0), 50, 1e-5, P(out), None) + tail)) == 0        # no pixels: nothing to do, no device
    assert not out.any()


# ---- the mirror against a recording stand-in -------------------------------------------------------------------------------
def _doubles(p, n):
    return None if not p else np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (n,)).copy()


class _RecordingLib:
    """gpa_kerelsky_fit[_dev] that records its scalar arguments and answers every pixel with `answer`"""

    def __init__(self, answer):
        self.calls, self.answer = [], answer

    def _record(self, kind, code, npx, a0, x0, max_nfev, retry):
        self.calls.append(dict(kind=kind, code=code, npx=npx, a0=_doubles(a0, 4), x0=_doubles(x0, 4), max_nfev=max_nfev, retry=retry))

    def gpa_kerelsky_fit(self, device, code, npx, jac, a0, x0, max_nfev, retry, out, cost):
        self._record('host', code, npx, a0 and a0.value, x0.value, max_nfev, retry)
        ct = C.c_float if code == _lib.GPA_F32 else C.c_double
        np.ctypeslib.as_array(C.cast(out.value, C.POINTER(ct)), (npx, 4))[:] = self.answer
        np.ctypeslib.as_array(C.cast(cost.value, C.POINTER(C.c_double)), (npx,))[:] = 0.0
        return 0

    def gpa_kerelsky_fit_dev(self, device, code, npx, jac, a0, x0, max_nfev, retry, out, cost, stream):
        self._record('dev', code, npx, a0 and a0.value, x0.value, max_nfev, retry)
        self.calls[-1].update(jac=jac.value, out=out.value, cost=cost and cost.value, stream=stream and stream.value)
        return 0


@pytest.fixture
def recording(monkeypatch):
    def install(answer=(1.25, 30., 0.004, 11.)):
        lib = _RecordingLib(np.asarray(answer, dtype=np.float64))
        monkeypatch.setattr(_lib, 'load', lambda: lib)
        return lib
    return install


def test_mirror_calls(recording):
    lib = recording()
    z = kc.load('smooth_24x20')
    A0, est = kc.a0_and_start(z['kvecs'], kc.NMPERPIXEL, kc.A_0)
    X, refest = pe.Kerelsky_J(z['J'], z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0)
    assert X.shape == (24, 20, 4) and X.dtype == np.float64 and np.array_equal(refest, lib.answer)
    g, p = lib.calls
    assert len(lib.calls) == 2                                   # the global fit with npx = 1, then one call for the field
    assert (g['kind'], g['npx'], g['a0'], g['max_nfev'], g['retry']) == ('host', 1, None, 50, 1e-20) and np.array_equal(g['x0'], est)
    assert est[0] == .01 and est[1] == 0 and est[2] == 0
    assert (p['kind'], p['npx'], p['max_nfev'], p['retry'], p['code']) == ('host', 480, 50, 1e-5, _lib.GPA_F64)
    assert np.array_equal(p['a0'], A0.ravel()) and np.array_equal(p['x0'], refest)          # as computed, not re-derived
    lib.calls.clear()
    X, _ = pe.Kerelsky_J(z['J'], z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, lq_kwargs={'max_nfev': 7}, dtype=np.float32)
    assert X.dtype == np.float32 and [c['max_nfev'] for c in lib.calls] == [7, 7] and lib.calls[1]['code'] == _lib.GPA_F32
    lib.calls.clear()
    # sort reorders the k-vectors before A0 and the start are formed
    for sort in (1, -1):
        k = z['kvecs'][[1, 2, 0]]
        A0s, ests = kc.a0_and_start(k, kc.NMPERPIXEL, kc.A_0, sort=sort)
        pe.Kerelsky_J(z['J'], k, nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, sort=sort)
        assert np.array_equal(lib.calls[-1]['a0'], A0s.ravel()) and np.array_equal(lib.calls[-2]['x0'], ests)
    assert np.array_equal(kc.a0_and_start(z['kvecs'][[1, 2, 0]], kc.NMPERPIXEL, kc.A_0, sort=1)[0], A0)
    assert not np.array_equal(kc.a0_and_start(z['kvecs'][[1, 2, 0]], kc.NMPERPIXEL, kc.A_0, sort=0)[0], A0)
    lib.calls.clear()
    # Kerelsky_Jac: the global fit alone, A0 as the matrix, scipy's default budget; 'symmetric' moves xi by theta / 2
    x = pe.Kerelsky_Jac(z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0)
    xs = pe.Kerelsky_Jac(z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, reference='symmetric')
    assert np.array_equal(x, lib.answer) and np.array_equal(xs, lib.answer + [0, 0, 0, 1.25 / 2])
    assert [(c['npx'], c['a0'], c['max_nfev'], c['retry']) for c in lib.calls] == [(1, None, 400, 1e-20)] * 2
    lib.calls.clear()
    # iterate_J_leastsq: the matrices themselves, the start as given
    Y = pe.iterate_J_leastsq(np.zeros((3, 5, 2, 2)), [1., 2., 0., 4.], {'max_nfev': 9})
    assert Y.shape == (3, 5, 4) and lib.calls[0]['a0'] is None and lib.calls[0]['npx'] == 15 and lib.calls[0]['retry'] == 1e-5
    assert np.array_equal(lib.calls[0]['x0'], [1., 2., 0., 4.]) and lib.calls[0]['max_nfev'] == 9
    lib.calls.clear()
    # the resident form: pointers go through untouched, refest comes back
    r = pe.Kerelsky_J_dev(0x1000, 77, z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, dtype=np.float32, out_ptr=0x2000, cost_ptr=0x3000, stream=0x40)
    d = lib.calls[1]
    assert np.array_equal(r, lib.answer) and (d['kind'], d['npx'], d['jac'], d['out'], d['cost'], d['stream'], d['code']) == ('dev', 77, 0x1000, 0x2000, 0x3000, 0x40, 0)
    assert np.array_equal(d['a0'], A0.ravel()) and np.array_equal(d['x0'], r)


def test_failed_global_fit_returns_nan_refest_alone(recording):
    lib = recording(answer=(np.nan,) * 4)
    z = kc.load('smooth_24x20')
    r = pe.Kerelsky_J(z['J'], z['kvecs'], nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0)
    assert isinstance(r, np.ndarray) and r.shape == (4,) and np.isnan(r).all() and len(lib.calls) == 1
    r = pe.Kerelsky_J_dev(0x1000, 77, z['kvecs'], out_ptr=0x2000)
    assert np.isnan(r).all() and len(lib.calls) == 2 and lib.calls[1]['kind'] == 'host'
    assert np.isnan(pe.Kerelsky_Jac(z['kvecs'])).all()


@pytest.mark.parametrize('kw, exc', [
    (dict(J=np.zeros((4, 4, 2, 3))), ValueError), (dict(J=np.zeros(4)), ValueError), (dict(kvecs=np.ones((2, 2))), ValueError),
    (dict(kvecs=np.full((3, 2), np.nan)), ValueError), (dict(nmperpixel=0.), ValueError), (dict(a_0=-1.), ValueError),
    (dict(reference='asymmetric'), ValueError), (dict(sort=2), ValueError), (dict(lq_kwargs={'max_nfev': 0}), ValueError),
    (dict(lq_kwargs={'max_nfev': 50, 'xtol': 1e-12}), NotImplementedError), (dict(lq_kwargs={'loss': 'huber'}), NotImplementedError),
    (dict(dtype=np.int32), ValueError)])
def test_argument_errors_before_the_library(recording, kw, exc):
    lib = recording()
    args = dict(J=np.zeros((4, 4, 2, 2)), kvecs=kc.kvecs_of(kc.GLOBAL_X), nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0, reference=None, sort=0,
                lq_kwargs={'max_nfev': 50}, dtype=None)
    args.update(kw)
    J = args.pop('J')
    with pytest.raises(exc) as e:
        pe.Kerelsky_J(J, args.pop('kvecs'), **args)
    assert not lib.calls
    if exc is NotImplementedError:
        assert [k for k in kw['lq_kwargs'] if k != 'max_nfev'][0] in str(e.value)


def test_twist_matrix_and_residual():
    assert np.allclose(pe.twist_matrix(3.0), kc._W(1.5) - kc._W(-1.5), rtol=0, atol=1e-16)
    x, A = np.array([1.2, 40., 0.01, 12.]), np.array([[0.01, -0.02], [0.02, 0.01]])
    V, D = kc.rotation_matrix(np.deg2rad(40.)), kc.strain_matrix(0.01)
    want = np.ravel(V.T @ D @ V @ kc.rotation_matrix(np.deg2rad(13.2)) - kc.rotation_matrix(np.deg2rad(12.)) - A) * 1000
    assert np.allclose(pe.Jac_fit_diff(x, A), want, rtol=0, atol=1e-12)
    assert pe.Jac_fit_diff(x, A).shape == (4,)


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gpa_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.GPAError):
        pe.Kerelsky_Jac(kc.kvecs_of(kc.GLOBAL_X), nmperpixel=kc.NMPERPIXEL, a_0=kc.A_0)
    with pytest.raises(_lib.GPAError):
        pe.iterate_J_leastsq(np.zeros((3, 2, 2)), [1., 0., 0., 10.])
