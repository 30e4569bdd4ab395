"""The field / phases -> Jacobian functions without a GPU: the fixtures the reference wrote against the NumPy restatement of
tests/jac_cases.py, the edge rule against np.gradient, the geometry header compiled for the host (tests/host/fieldjac_check.cpp,
plain and under the host sanitizers -- an ordinary executable), the C ABI's symbols and argument errors, and the Python mirror
against a recording stand-in."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.property_extract as pe

import jac_cases as jc
import prep_cases as pc

SYMBOLS = {'gpa_field_jacobian': 13, 'gpa_field_jacobian_dev': 14, 'gpa_phases_jacobian': 15, 'gpa_phases_jacobian_dev': 16,
           'gpa_phys_props_from_jac': 10, 'gpa_phys_props_from_jac_dev': 11}
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


# ---- fixtures and restatements --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(jc.CASES))
def test_fixture_promises_and_restatement(name):
    z = jc.load(name)
    shape, P, wrapped, zero_px = jc.CASES[name][:4]
    kvecs, phases, weights, nm = jc.phase_inputs(name)
    assert np.array_equal(z['kvecs'], kvecs) and np.array_equal(z['phases'], phases) and np.array_equal(z['weights'], weights)
    assert float(z['nmperpixel']) == nm and z['phases'].shape == (P,) + shape and z['J'].shape == shape + (2, 2)
    assert z['props'].shape == z['phys'].shape == z['phys_diff'].shape == (4,) + shape
    assert os.path.getsize(os.path.join(jc.GOLDEN, 'jac_%s.npz' % name)) < 1 << 20
    assert all(v.dtype.kind == 'f' for v in z.values())                 # numeric arrays only
    margin, share = jc.seam_margin_and_share(z['phases'])
    print('%s: seam margin %.3f rad, %.1f %% of the differences wrap' % (name, margin, 100 * share))
    assert margin >= jc.SEAM_MARGIN
    assert share >= jc.WRAP_SHARE if wrapped else (share == 0 and np.abs(z['phases']).max() < 12)
    J = jc.phases2J_np(z['kvecs'], z['phases'], z['weights'], nm)
    assert np.abs(J - z['J']).max() <= 1e-12 * np.abs(z['J']).max()
    if zero_px is not None:
        assert not z['weights'][(slice(None),) + zero_px].any() and not z['J'][zero_px].any() and not J[zero_px].any()
        assert (z['props'][3] > jc.KAPPA_MIN).sum() == z['props'][3].size - 1
    else:
        assert (z['props'][3] > jc.KAPPA_MIN).all()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edge_rule_is_np_gradient(dtype):
    """one rounded subtraction and one rounded division by the divisor rounded once to the dtype: np.gradient to the bit"""
    n = 0
    for shape in [(2, 2), (2, 9), (9, 2), (3, 300), (300, 3), (37, 70), (65, 257), (5, 2), (16, 17)]:
        U = jc.field_input(shape, seed=shape[0] * 1000 + shape[1]).astype(dtype)
        for h in jc.SPACINGS:
            J, want = jc.u2J_np(U, h), jc.u2J_gradient(U, h)
            assert J.dtype == want.dtype == dtype and J.shape == shape + (2, 2)
            np.testing.assert_array_equal(J, want)
            n += J.size
    assert n > 100000


def test_edge_rule_propagates_nan_like_np_gradient():
    U = jc.field_input((9, 11), seed=3)
    U[0, 4, 5] = np.nan
    U[1, 0, 0] = np.nan
    J, want = jc.u2J_np(U, 0.5), jc.u2J_gradient(U, 0.5)
    assert np.array_equal(np.isnan(J), np.isnan(want)) and np.isnan(J).sum() == 4 + 4   # four neighbours inside; the corner itself twice and its two neighbours
    np.testing.assert_array_equal(J, want)


# ---- the header, compiled for the host --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'sanitized'])
def test_geometry_header_on_the_host(kind, tmp_path):
    extra = SANITIZE if kind == 'sanitized' else []
    if extra and not pc.host_compiler_links(tmp_path, extra):
        pytest.skip('the host compiler has no sanitizer runtimes')
    exe = os.path.join(str(tmp_path), 'fieldjac_check')
    cmd = [pc._host_cxx(), '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-I',
           os.path.join(jc.ROOT, 'pygpa_amd', 'csrc')] + extra
    r = subprocess.run(cmd + [os.path.join(jc.ROOT, 'tests', 'host', 'fieldjac_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 1000000


def test_tile_constants_are_readable():
    rows, lanes, vec_bytes = jc.tile_constants()
    assert lanes == 64 and vec_bytes == 16 and rows >= 2
    assert jc.ragged_shape() == (2 * rows + 5, 2 * lanes * 4 + 3)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_signatures():
    header = open(os.path.join(jc.ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = _lib.load()
    for name, n in SYMBOLS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        res, args = _lib.SIGNATURES[name]
        assert nargs == len(args) == n and res is _lib._i, name
        assert hasattr(lib, name)
    build = open(os.path.join(jc.ROOT, 'pygpa_amd', 'build.py')).read()
    assert "'gpa_fieldjac.hip'" in build and "'gpa_api_fieldjac.hip'" in build
    assert "'gpa_fieldjac.hip':" not in build                 # the flags of gpa_reconstruct.hip: no per-file entry


def test_library_argument_errors_need_no_device():
    lib = _lib.load()
    buf = jc.error_buffers()
    for base, table in jc.ERROR_TABLES.items():
        for sfx, tail in (('', ()), ('_dev', (None,))):
            f = getattr(lib, base + sfx)
            n = 0
            for args, word in table(_lib._ptr, buf):
                assert f(*((0,) + args + tail)) == -1, (base + sfx, word)
                assert word in _lib.last_error() and (base + sfx + ':') in _lib.last_error(), (word, _lib.last_error())
                n += 1
            assert n >= 5
    # a device J is stored as whole matrices
    P = _lib._ptr
    J1 = buf['J'].ravel()[1:]
    assert lib.gpa_field_jacobian_dev(0, 1, 1, 4, 4, P(buf['u']), 0.5, 0, P(J1), None, 0., 1., 0, None) == -1 and 'aligned' in _lib.last_error()
    assert lib.gpa_phases_jacobian_dev(0, 1, 4, 4, 3, P(buf['k']), P(buf['ph']), P(buf['w']), 0.5, 0, P(J1), None, 0., 1., 0, None) == -1
    assert 'aligned' in _lib.last_error()
    assert lib.gpa_phys_props_from_jac(0, 1, 0, _lib._ptr(buf['J']), 0, 0., 1., 0, 0.16, _lib._ptr(buf['props'])) == 0   # no pixels
    assert not any(v.any() for k, v in buf.items() if k != 'k')


# ---- the mirror against a recording stand-in -------------------------------------------------------------------------------
class _RecordingLib:
    """the six entry points, recording their arguments; host forms fill their outputs with a constant"""

    def __init__(self):
        self.calls = []

    def _rec(self, name, **kw):
        self.calls.append(dict(name=name, **{k: (v.value if hasattr(v, 'value') else v) for k, v in kw.items()}))
        return 0

    def gpa_field_jacobian(self, device, code, nimg, n0, n1, u, nm, ident, J, props, refangle, refscale, diff):
        return self._rec('field', code=code, nimg=nimg, n0=n0, n1=n1, u=u, nm=nm, ident=ident, J=J, props=props, refangle=refangle,
                         refscale=refscale, diff=diff)

    def gpa_field_jacobian_dev(self, device, code, nimg, n0, n1, u, nm, ident, J, props, refangle, refscale, diff, stream):
        return self._rec('field_dev', code=code, nimg=nimg, n0=n0, n1=n1, u=u, nm=nm, ident=ident, J=J, props=props,
                         refangle=refangle, refscale=refscale, diff=diff, stream=stream)

    def gpa_phases_jacobian(self, device, code, n0, n1, P, k, ph, w, nm, ident, J, props, refangle, refscale, diff):
        kv = np.ctypeslib.as_array(C.cast(k.value, C.POINTER(C.c_double)), (P, 2)).copy()
        return self._rec('phases', code=code, n0=n0, n1=n1, P=P, kvecs=kv, ph=ph, w=w, nm=nm, ident=ident, J=J, props=props,
                         refangle=refangle, refscale=refscale, diff=diff)

    def gpa_phases_jacobian_dev(self, device, code, n0, n1, P, k, ph, w, nm, ident, J, props, refangle, refscale, diff, stream):
        return self._rec('phases_dev', code=code, n0=n0, n1=n1, P=P, ph=ph, w=w, nm=nm, ident=ident, J=J, props=props,
                         refangle=refangle, refscale=refscale, diff=diff, stream=stream)

    def gpa_phys_props_from_jac(self, device, code, npx, jac, ident, refangle, refscale, diff, poisson, props):
        return self._rec('phys', code=code, npx=npx, ident=ident, refangle=refangle, refscale=refscale, diff=diff, poisson=poisson)


@pytest.fixture
def recording(monkeypatch):
    lib = _RecordingLib()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    return lib


def _only(lib):
    assert len(lib.calls) == 1
    return lib.calls.pop()


def test_mirror_calls(recording):
    lib = recording
    z = jc.load('hex_37x70')
    U = jc.field_input((6, 7))
    J = pe.u2J(U, 0.5)
    c = _only(lib)
    assert J.shape == (6, 7, 2, 2) and J.dtype == np.float64
    assert (c['name'], c['code'], c['nimg'], c['n0'], c['n1'], c['nm'], c['ident'], c['props']) == ('field', 1, 1, 6, 7, 0.5, 0, None) and c['J']
    assert pe.u2Jac(U, 0.5, dtype=np.float32).dtype == np.float32
    c = _only(lib)
    assert (c['code'], c['ident'], c['nm']) == (0, 1, 0.5)
    Js = pe.u2J_stack(np.stack([U, U, U]), 3.7)
    c = _only(lib)
    assert Js.shape == (3, 6, 7, 2, 2) and (c['nimg'], c['n0'], c['n1'], c['nm']) == (3, 6, 7, 3.7)
    pe.u2J_dev(0x1000, (4, 2, 6, 7), 0.5, J_ptr=0x2000, props_ptr=0x3000, stream=0x40, dtype=np.float32, refangle=5.)
    c = _only(lib)
    assert (c['name'], c['u'], c['J'], c['props'], c['stream'], c['nimg'], c['code'], c['refangle']) == ('field_dev', 0x1000, 0x2000, 0x3000, 0x40, 4, 0, 5.)
    pe.u2J_dev(0x1000, (2, 6, 7), 0.5, props_ptr=0x3000)
    c = _only(lib)
    assert (c['J'], c['props'], c['stream'], c['nimg']) == (None, 0x3000, None, 1)

    args = (z['kvecs'], z['phases'], z['weights'], float(z['nmperpixel']))
    J = pe.phases2J(*args)
    c = _only(lib)
    assert J.shape == (37, 70, 2, 2) and (c['name'], c['P'], c['n0'], c['n1'], c['nm'], c['ident'], c['props']) == ('phases', 3, 37, 70, 3.7, 0, None)
    assert np.array_equal(c['kvecs'], z['kvecs'])                      # plain kvecs: the library forms 2 pi kvecs
    pe.phases2Jac(*args)
    assert _only(lib)['ident'] == 1
    # calc_props_from_phases: ONE fused call that stores no J, with the base angle of the k-vectors as refangle
    props = pe.calc_props_from_phases(*args)
    c = _only(lib)
    theta_0 = pe.get_initial_props(z['kvecs'])[1]
    assert props.shape == (4, 37, 70) and c['J'] is None and c['props'] and c['refangle'] == theta_0 and c['refscale'] == 1. and c['diff'] == 0
    assert c['ident'] == 0
    pe.phases2J_dev(z['kvecs'], 0x1000, 0x2000, (3, 37, 70), 3.7, J_ptr=0x3000, stream=0x50)
    c = _only(lib)
    assert (c['name'], c['ph'], c['w'], c['J'], c['props'], c['stream'], c['P']) == ('phases_dev', 0x1000, 0x2000, 0x3000, None, 0x50, 3)

    p = pe.phys_props_from_Jac(np.zeros((5, 4, 2, 2)), refangle=2., refscale=3, diff=True)
    c = _only(lib)
    assert p.shape == (4, 5, 4) and (c['npx'], c['refangle'], c['refscale'], c['diff'], c['poisson'], c['ident']) == (20, 2., 3., 1, 0.16, 0)


@pytest.mark.parametrize('call', [
    lambda: pe.u2J(np.zeros((3, 4, 5)), 0.5), lambda: pe.u2J(np.zeros((2, 1, 5)), 0.5), lambda: pe.u2J(np.zeros((2, 5, 1)), 0.5),
    lambda: pe.u2J(np.zeros((2, 2, 4, 5)), 0.5), lambda: pe.u2J_stack(np.zeros((2, 4, 5)), 0.5), lambda: pe.u2J_stack(np.zeros((0, 2, 4, 5)), 0.5),
    lambda: pe.u2J(np.zeros((2, 4, 5)), 0.), lambda: pe.u2J(np.zeros((2, 4, 5)), np.nan), lambda: pe.u2Jac(np.zeros((2, 4, 5)), np.inf),
    lambda: pe.u2J(np.zeros((2, 4, 5)), 0.5, dtype=np.int32), lambda: pe.u2J_dev(0x1000, (2, 4, 5), 0.5),
    lambda: pe.u2J_dev(0x1000, (2, 1, 5), 0.5, J_ptr=0x2000),
    lambda: pe.phases2J(np.zeros((3, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4, 4)), 0.5),          # weights must match phases
    lambda: pe.phases2J(np.zeros((3, 2)), np.zeros((3, 4, 5)), np.zeros((4, 5)), 0.5),
    lambda: pe.phases2J(np.zeros((2, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4, 5)), 0.5),
    lambda: pe.phases2J(np.zeros((1, 2)), np.zeros((1, 4, 5)), np.zeros((1, 4, 5)), 0.5),
    lambda: pe.phases2J(np.zeros((9, 2)), np.zeros((9, 4, 5)), np.zeros((9, 4, 5)), 0.5),
    lambda: pe.phases2J(np.zeros((3, 2)), np.zeros((3, 1, 5)), np.zeros((3, 1, 5)), 0.5),
    lambda: pe.phases2Jac(np.zeros((3, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4, 5)), 0.),
    lambda: pe.phases2J(np.full((3, 2), np.nan), np.zeros((3, 4, 5)), np.zeros((3, 4, 5)), 0.5),
    lambda: pe.phases2J_dev(np.zeros((3, 2)), 0x1000, 0x2000, (3, 4, 5), 0.5),
    lambda: pe.phys_props_from_Jac(np.zeros((4, 2, 3))), lambda: pe.phys_props_from_Jac(np.zeros((4, 2, 2)), poisson_ratio=np.nan)])
def test_argument_errors_before_the_library(recording, call):
    with pytest.raises(ValueError):
        call()
    assert not recording.calls


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gpa_device_count() > 0:
        pytest.skip('a GPU is visible')
    z = jc.load('p2_2x9')
    with pytest.raises(_lib.GPAError):
        pe.u2J(jc.field_input((4, 5)), 0.5)
    with pytest.raises(_lib.GPAError):
        pe.calc_props_from_phases(z['kvecs'], z['phases'], z['weights'], 3.7)
    with pytest.raises(_lib.GPAError):
        pe.phys_props_from_Jac(np.eye(2) + z['J'])
