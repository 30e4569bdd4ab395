"""phase_unwrap_stack / phase_unwrap_prediff_stack without a GPU: the mirror refuses wrong shape and dtype combinations with
ValueError before it touches the library; the entry points of the stack are declared in include/gpa_hip.h with the argument
counts and kinds of their ctypes prototypes; and the host-testable arithmetic of the stack (pygpa_amd/csrc/gpa_unwrap_batch.h:
chunk size under a byte budget, weight plane of a problem) passes its stand-alone check (tests/host/unwrap_batch_check.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.phase_unwrap as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to get a plan (and with it the library) fails the test"""
    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'get_plan', boom)
    monkeypatch.setattr(_lib, 'load', boom)


@pytest.mark.parametrize('psi_shape, w_shape', [
    ((32, 48), None),                    # wrong rank
    ((1, 4, 32, 48), None),
    ((48,), None),
    ((0, 32, 48), None),                 # B = 0
    ((4, 32, 48), (32, 47)),             # weight of another grid
    ((4, 32, 48), (48, 32)),
    ((4, 32, 48), (4, 32, 47)),
    ((4, 32, 48), (3, 32, 48)),          # (B', N, M) weights with B' != B
    ((4, 32, 48), (5, 32, 48)),
    ((4, 32, 48), (1, 32, 48)),
    ((4, 32, 48), (4, 1, 32, 48)),       # weight of the wrong rank
    ((4, 1, 48), None),                  # nothing to difference
])
def test_psi_combinations_raise_before_the_library(no_library, psi_shape, w_shape):
    w = None if w_shape is None else np.ones(w_shape, np.float32)
    with pytest.raises(ValueError):
        PU.phase_unwrap_stack(np.zeros(psi_shape, np.float32), weight=w)


@pytest.mark.parametrize('dx_shape, dy_shape, w_shape', [
    ((4, 32, 47), (4, 31, 47), None),            # dx/dy shapes that do not pair
    ((4, 32, 47), (4, 32, 48), None),
    ((4, 32, 47), (3, 31, 48), None),            # another B
    ((4, 32, 47), (31, 48), None),               # wrong rank
    ((32, 47), (31, 48), None),
    ((0, 32, 47), (0, 31, 48), None),            # B = 0
    ((4, 32, 47), (4, 31, 48), (32, 47)),        # weight of another grid (that of dx)
    ((4, 32, 47), (4, 31, 48), (3, 32, 48)),     # B' != B
])
def test_prediff_combinations_raise_before_the_library(no_library, dx_shape, dy_shape, w_shape):
    w = None if w_shape is None else np.ones(w_shape, np.float32)
    with pytest.raises(ValueError):
        PU.phase_unwrap_prediff_stack(np.zeros(dx_shape, np.float32), np.zeros(dy_shape, np.float32), weight=w)


def test_dtype_errors_raise_before_the_library(no_library):
    psi = np.zeros((2, 32, 48))
    with pytest.raises(ValueError):
        PU.phase_unwrap_stack(psi, dtype=np.float16)
    with pytest.raises(ValueError):
        PU.phase_unwrap_stack(psi, dtype=np.complex64)
    with pytest.raises(ValueError):
        PU.phase_unwrap_stack(psi.astype(np.complex128))
    with pytest.raises(ValueError):
        PU.phase_unwrap_stack(psi, weight=np.ones((32, 48), np.complex64))
    with pytest.raises(ValueError):
        PU.phase_unwrap_prediff_stack(np.zeros((2, 32, 47)), np.zeros((2, 31, 48), np.complex128))


def test_accepted_shapes():
    assert _lib.unwrap_stack_shapes((4, 32, 48)) == 4
    assert _lib.unwrap_stack_shapes((1, 32, 48), None, (32, 48)) == 1
    assert _lib.unwrap_stack_shapes((4, 32, 47), (4, 31, 48)) == 4
    assert _lib.unwrap_stack_shapes((4, 32, 47), (4, 31, 48), (32, 48)) == 4
    with pytest.raises(ValueError):
        _lib.unwrap_stack_shapes((4, 32, 48), None, (32, 32))
    assert _lib.unwrap_stack_weight_planes((32, 48), 4, (32, 48)) == 1
    assert _lib.unwrap_stack_weight_planes((4, 32, 48), 4, (32, 48)) == 4
    assert _lib.unwrap_stack_weight_planes((1, 32, 48), 1, (32, 48)) == 1


ENTRY_POINTS = (('gpa_unwrap_batch_dev', 10), ('gpa_unwrap_prediff_batch_dev', 11), ('gpa_unwrap_batch_finish', 3),
                ('gpa_unwrap_batch', 10), ('gpa_unwrap_prediff_batch', 11))


def test_entry_points_declared_with_matching_prototypes():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, nargs in ENTRY_POINTS:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, '%s is not declared in gpa_hip.h' % name
        params = [a.strip() for a in m.group(1).split(',')]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i
        assert len(args) == len(params)
        # pointers, ints and doubles sit where the prototype has them
        for prm, ct in zip(params, args):
            if '*' in prm:
                assert ct is _lib._vp, (name, prm)
            elif prm.startswith('int '):
                assert ct is _lib._i, (name, prm)
            elif prm.startswith('double '):
                assert ct is _lib._d, (name, prm)
            else:
                raise AssertionError('unexpected parameter %r of %s' % (prm, name))
    assert re.search(r'^#define GPA_UNWRAP_BATCH_MAX 4096\s*$', header, flags=re.M) and _lib.UNWRAP_BATCH_MAX == 4096
    # the internal header that sizes the chunks states the same limit
    internal = open(os.path.join(ROOT, 'pygpa_amd', 'csrc', 'gpa_unwrap_batch.h')).read()
    assert re.search(r'^#define GPA_UNWRAP_BATCH_MAX 4096\b', internal, flags=re.M)


def test_mirror_offers_the_stack_calls():
    for name in ('unwrap_stack', 'unwrap_prediff_stack', 'unwrap_batch_dev', 'unwrap_prediff_batch_dev', 'unwrap_batch_finish'):
        assert callable(getattr(_lib.Plan, name))
    for name in ('phase_unwrap_stack', 'phase_unwrap_prediff_stack'):
        assert callable(getattr(PU, name))
        assert 'phase_unwrap.py:' in getattr(PU, name).__doc__     # what the reference offers in its place


@pytest.fixture(scope='module')
def gxx():
    g = shutil.which('g++')
    if g is None:
        pytest.skip('g++ not available')
    return g


def test_batch_arithmetic_check_program(gxx, tmp_path):
    """chunk size (budget edges, a ragged last chunk), the three weight modes and the 64-bit offsets at pb * npx >= 2^32"""
    exe = str(tmp_path / 'unwrap_batch_check')
    src = os.path.join(ROOT, 'tests', 'host', 'unwrap_batch_check.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.startswith('OK ')
    assert int(out.stdout.split()[1]) > 400
