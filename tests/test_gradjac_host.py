"""gpa_gradients_jacobian[_dev] without a GPU: every bad argument is GPA_ERR_ARG, named in gpa_last_error, before a device is
touched; the mirror refuses bad shapes before the library; the pointwise geometry of gpa_fieldjac.h covers every pixel once."""
import os
import subprocess

import numpy as np
import pytest

import gradjac_cases as gc
from pygpa_amd import _lib
from pygpa_amd import property_extract as pe


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pointwise_geometry_on_the_host(tmp_path):
    """tests/host/gradjac_check.cpp: the index arithmetic of gradients_jacobian_kernel walked on the CPU over the shapes of the
    GPU test and the edges of a wave"""
    import prep_cases as pc
    exe = os.path.join(str(tmp_path), 'gradjac_check')
    cmd = [pc._host_cxx(), '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'host', 'gradjac_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 100000


def test_library_argument_errors_need_no_device():
    lib = _lib.load()
    buf = gc.error_buffers()
    for sfx, tail in (('', ()), ('_dev', (None,))):
        f = getattr(lib, 'gpa_gradients_jacobian' + sfx)
        n = 0
        for args, word in gc.gradients_errors(_lib._ptr, buf):
            assert f(*((0,) + args + tail)) == -1, (sfx, word)
            assert word in _lib.last_error() and ('gpa_gradients_jacobian' + sfx + ':') in _lib.last_error(), (word, _lib.last_error())
            n += 1
        assert n >= 20
    # a device J is stored as whole matrices, device gradients are read as whole pairs
    P = _lib._ptr
    ok = [0, 1, 1, 4, 5, 3, P(buf['k']), None, P(buf['g']), P(buf['w']), 0.5, 0, P(buf['J']), None, 0., 1., 0, None]
    for pos, arr in ((12, buf['J']), (8, buf['g'])):
        args = list(ok)
        args[pos] = P(arr.ravel()[1:])
        assert lib.gpa_gradients_jacobian_dev(*args) == -1 and 'aligned' in _lib.last_error()
    assert not any(v.any() for k, v in buf.items() if k != 'k')   # nothing was written


@pytest.mark.parametrize('call', [
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3)[:1], g, w, 0.5),                     # one k-vector
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3), g[..., :1], w, 0.5),                # no pairs
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3), g, w[:, :2], 0.5),                  # weights of another shape
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3), g, w, 0.5, dks=np.zeros((2, 2))),   # dks of another shape
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3), g, w, 0.5, want_J=False),           # nothing to compute
    lambda g, w: _lib.gradients_jacobian(gc.kvecs_of(3), g, w, 0.0),                         # no spacing
    lambda g, w: pe.phasegradient2J_stack(gc.kvecs_of(3), g[0], w[0], 0.5),                  # a single frame is no stack
])
def test_mirror_refuses_before_the_library(call, monkeypatch):
    g, w = gc.inputs(2, 3, (3, 5), np.float64)
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was reached'))
    with pytest.raises(ValueError):
        call(g, w)

