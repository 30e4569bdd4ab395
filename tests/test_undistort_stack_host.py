"""undistort_image_stack without a GPU: the mirror refuses wrong shape combinations with ValueError before it touches the
library, and the two entry points of the stack are declared in include/gpa_hip.h with the argument counts of their ctypes
prototypes."""
import os
import re

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to get a plan (and with it the library) fails the test"""
    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'get_plan', boom)
    monkeypatch.setattr(_lib, 'load', boom)


@pytest.mark.parametrize('frames_shape, u_shape', [
    ((4, 32, 48), (32, 48)),              # u of the wrong rank
    ((4, 32, 48), (2, 2, 2, 32, 48)),
    ((4, 32, 48), (3, 32, 48)),           # not two components
    ((4, 32, 48), (4, 3, 32, 48)),
    ((4, 32, 48), (3, 2, 32, 48)),        # 3 fields for 4 frames
    ((4, 32, 48), (5, 2, 32, 48)),
    ((4, 32, 48), (2, 32, 47)),           # another grid
    ((4, 32, 48), (4, 2, 48, 32)),
    ((32, 48), (2, 32, 48)),              # frames not 3-D
    ((1, 4, 32, 48), (2, 32, 48)),
    ((0, 32, 48), (2, 32, 48)),           # no frames
])
def test_shape_combinations_raise_before_the_library(no_library, frames_shape, u_shape):
    with pytest.raises(ValueError):
        GPA.undistort_image_stack(np.zeros(frames_shape, np.float32), np.zeros(u_shape, np.float32))


def test_accepted_shapes():
    assert _lib.stack_shapes((4, 32, 48), (2, 32, 48)) == (4, False)
    assert _lib.stack_shapes((4, 32, 48), (4, 2, 32, 48)) == (4, True)
    assert _lib.stack_shapes((2, 32, 48), (2, 2, 32, 48)) == (2, True)     # B = 2: four dimensions mean a field per frame
    assert _lib.stack_shapes((1, 32, 48), (1, 2, 32, 48), plan_shape=(32, 48)) == (1, True)
    with pytest.raises(ValueError):
        _lib.stack_shapes((4, 32, 48), (2, 32, 48), plan_shape=(32, 32))


def test_entry_points_declared_with_matching_argument_counts():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, nargs in (('gpa_undistort_image_batch_dev', 8), ('gpa_undistort_image_batch', 6)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, '%s is not declared in gpa_hip.h' % name
        params = [a.strip() for a in m.group(1).split(',')]
        assert len(params) == nargs
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(params)
        # ints and doubles sit where the prototype has them
        for prm, ct in zip(params, args):
            if '*' in prm:
                assert ct is _lib._vp, (name, prm)
            elif prm.startswith('int '):
                assert ct is _lib._i, (name, prm)
            elif prm.startswith('double '):
                assert ct is _lib._d, (name, prm)
    assert '#define GPA_UNDISTORT_MAX_FRAMES 65535' in header and _lib.UNDISTORT_MAX_FRAMES == 65535
