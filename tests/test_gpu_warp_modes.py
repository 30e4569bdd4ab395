"""GPU tests of the boundary modes 'reflect' / 'grid-mirror', 'mirror' and 'grid-wrap' of invert_u / invert_u_overlap
(invert_folded_kernel, gpa_warp.hip) against the same scipy.ndimage.map_coordinates calls the reference makes (oracle).

Bounds (those of tests/test_gpu_hypothesis.py::test_invert_u_modes_vs_scipy): error <= tol * max(1, max|ref|) with tol = 1e-10
in f64 and 3e-4 in f32, and no NaN anywhere in the output -- the folded modes never use cval.

Fields: smooth, with |grad u| <= 0.2 ('reflect', 'mirror') or <= 0.5 ('grid-wrap', a field of the frame's period): the fixed
point contracts, so that a perturbation of the field by one f32 rounding moves the result by about as much.  (A field with
|grad u| > 1 is chaotic under the iteration and compares nothing.)

'reflect' on axes shorter than 16 samples is held to the device's own 'grid-wrap' on the symmetric doubling of the field,
an exact identity of the half-sample symmetric spline: SciPy's 'reflect' prefilter is approximate on short axes (3.7e-6 of the
field at n = 4, rounding from n = 12), the device computes the exact extension."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 3e-4}
DTYPES = [np.float64, np.float32]
MODES = ['reflect', 'mirror', 'grid-wrap']
VARIANTS = ['overlap', 'plain']


def smooth_field(shape):
    n0, n1 = shape
    x, y = np.mgrid[:n0, :n1].astype(np.float64)
    return np.stack([0.08 * n0 * np.sin(1.7 * y / n1 + 0.3) * np.cos(2.3 * x / n0), 0.08 * n1 * np.cos(2.9 * x / n0 + 1.0) + 0.02 * y])


def periodic_field(shape):
    n0, n1 = shape
    x, y = np.mgrid[:n0, :n1].astype(np.float64)
    tx, ty = 2.0 * np.pi * x / n0, 2.0 * np.pi * y / n1
    return np.stack([0.08 * n0 * np.sin(ty + 0.3) * np.cos(tx), 0.08 * n1 * np.cos(tx + 1.0) * np.sin(ty)])


def step_field(shape):
    """multiples of 0.5: the sample points of the first round land on integers and half-integers (the fold points -0.5,
    n - 0.5, n - 1 and n among them)"""
    x, y = np.mgrid[:shape[0], :shape[1]]
    return np.stack([0.5 * ((3 * x + 5 * y) % 7) - 1.5, 0.5 * ((2 * x + 3 * y) % 5) - 1.0])


FIELDS = {'smooth': smooth_field, 'periodic': periodic_field, 'step': step_field}


def field_for(mode, shape):
    return periodic_field(shape) if mode == 'grid-wrap' else smooth_field(shape)


@functools.lru_cache(maxsize=None)
def oracle(kind, shape, mode, variant, iters, edge):
    """the reference's result, computed once and shared by the two precisions (read-only)"""
    fn = orc.invert_u_overlap if variant == 'overlap' else orc.invert_u
    ref = fn(FIELDS[kind](shape), iters=iters, edge=edge, mode=mode)
    ref.setflags(write=False)
    return ref


def device(us, mode, variant, iters, edge, dtype):
    fn = GPA.invert_u_overlap if variant == 'overlap' else GPA.invert_u
    return fn(us, iters=iters, edge=edge, mode=mode, dtype=dtype)


def check(out, ref, dtype, what):
    assert out.shape == ref.shape and out.dtype == dtype, what
    assert not np.isnan(out).any(), what
    assert not np.isnan(ref).any(), what
    err, scale = np.abs(out - ref).max(), max(1.0, np.abs(ref).max())
    print('%s: error %.3g, bound %.3g' % (what, err, TOL[dtype] * scale))
    assert err <= TOL[dtype] * scale, what


ROUNDS = [(6, 0), (4, 3), (5, 0), (35, 0), (6, 40)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('mode', MODES + ['grid-mirror'])
@pytest.mark.parametrize('shape', [(37, 50), (72, 90), (16, 4100)])
def test_modes_vs_oracle(shape, mode, variant, dtype):
    """(16, 4100): rows longer than one FIR workgroup of 2048 outputs -- the interior and the extension tile loader with every
    extension.  edge = 40 puts coordinates beyond a whole period of the 37-row shape."""
    kind = 'periodic' if mode == 'grid-wrap' else 'smooth'
    us = FIELDS[kind](shape)
    for iters, edge in ROUNDS:
        ref = oracle(kind, shape, mode, variant, iters, edge)
        check(device(us, mode, variant, iters, edge, dtype), ref, dtype, (shape, mode, variant, iters, edge))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [(4, 5), (5, 7)])
def test_tiny_shapes(shape, mode, variant, dtype):
    """axes of 4 to 7 samples (n < 4 + footprint: no pixel takes the interior path), edge 12: the grid reaches more than
    two periods outside, every tap folds.  'mirror' and 'grid-wrap' against the oracle; 'reflect' against the device's own
    'grid-wrap' on the symmetric doubling, cropped to the grid of the original frame"""
    n0, n1 = shape
    us = field_for(mode, shape)
    for edge in (0, 12):
        out = device(us, mode, variant, 6, edge, dtype)
        if mode == 'reflect':
            doubled = np.pad(us, ((0, 0), (0, n0), (0, n1)), mode='symmetric')
            ref = device(doubled, 'grid-wrap', variant, 6, edge, dtype)
            e2 = 2 * edge if variant == 'overlap' else 0
            ref = ref[:, :n0 + e2, :n1 + e2].astype(np.float64)
        else:
            ref = oracle('periodic' if mode == 'grid-wrap' else 'smooth', shape, mode, variant, 6, edge)
        check(out, ref, dtype, (shape, mode, variant, edge))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('mode', MODES)
def test_fold_points(mode, variant, dtype):
    """sample points within rounding of integers and half-integers, -0.5, n - 0.5, n - 1 and n included: either side of a fold
    gives the same value (a branch flip is harmless), an off-by-one fold does not"""
    shape = (18, 21)
    us = step_field(shape)
    for edge in (0, 3):
        ref = oracle('step', shape, mode, variant, 2, edge)
        check(device(us, mode, variant, 2, edge, dtype), ref, dtype, (mode, variant, edge))


@pytest.mark.parametrize('dtype', DTYPES)
def test_early_exit_equals_every_round(dtype, gpa_option):
    """tests/test_gpu_parity.py::test_f1_early_exit_equals_every_round for invert_folded_kernel: leaving the loop once every
    pixel of a wavefront is at a bitwise fixed point or in a cycle of two (member by the parity of the rounds left) is
    BIT-identical to running every round (LF_ALL_ROUNDS=1)"""
    shape = (72, 90)
    plan = _lib.Plan(shape, 1, dtype)
    for mode in MODES:
        us = field_for(mode, shape).astype(dtype)
        for variant in VARIANTS:
            fn = plan.invert_u_overlap if variant == 'overlap' else plan.invert_u
            for iters in (5, 6, 35):
                gpa_option('LF_ALL_ROUNDS', None)
                a = fn(us, iters=iters, edge=3, mode=mode)
                gpa_option('LF_ALL_ROUNDS', '1')
                b = fn(us, iters=iters, edge=3, mode=mode)
                gpa_option('LF_ALL_ROUNDS', None)
                assert not np.isnan(a).any()
                assert np.array_equal(a, b), (mode, variant, iters, int((a != b).sum()))
    plan.close()


class DeviceArray:
    """a device buffer through the HIP runtime itself (ctypes)"""
    _hip = None

    def __init__(self, host):
        if DeviceArray._hip is None:
            _lib.load()
            DeviceArray._hip = C.CDLL('libamdhip64.so')
        self.host = np.ascontiguousarray(host)
        p = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(p), C.c_size_t(self.host.nbytes)) == 0
        self.ptr = p.value
        assert self._hip.hipMemcpy(C.c_void_p(self.ptr), self.host.ctypes.data_as(C.c_void_p), C.c_size_t(self.host.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.host)
        assert self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    def __del__(self):
        try:
            self._hip.hipFree(C.c_void_p(self.ptr))
        except Exception:
            pass


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_entry_equals_host_entry(dtype):
    """Plan.invert_u_dev (device pointers, scale) against the host-pointer calls on +-u, bit for bit; and two windows of the
    output grid behind one prefilter: the windows of the whole-grid result, the rest of the buffer untouched"""
    shape = (72, 90)
    plan = _lib.Plan(shape, 1, dtype)
    for mode in MODES:
        u = field_for(mode, shape).astype(dtype)
        d_u = DeviceArray(u)
        for overlap, edge in ((True, 0), (True, 6), (False, 3)):
            host_fn = plan.invert_u_overlap if overlap else plan.invert_u
            for scale in (1.0, -1.0):
                host = host_fn(u if scale > 0 else -u, iters=7, edge=edge, mode=mode)
                d_out = DeviceArray(np.zeros_like(host))
                plan.invert_u_dev(d_u.ptr, d_out.ptr, scale=scale, iters=7, edge=edge, overlap=overlap, mode=mode)
                plan.sync()
                assert np.array_equal(d_out.get(), host), (mode, overlap, edge, scale)
        whole = plan.invert_u_overlap(u, iters=7, edge=6, mode=mode)
        d_out = DeviceArray(np.full_like(whole, -7.0))
        rects = [(0, 0, 30, 41), (55, 60, 29, 42)]          # the second reaches the last row and column of the 84 x 102 grid
        plan.invert_u_dev(d_u.ptr, d_out.ptr, iters=7, edge=6, overlap=True, mode=mode, rects=rects)
        plan.sync()
        part, inside = d_out.get(), np.zeros(whole.shape, bool)
        for r0, c0, h, w in rects:
            inside[:, r0:r0 + h, c0:c0 + w] = True
        assert np.array_equal(part[inside], whole[inside]), mode
        assert np.all(part[~inside] == -7.0), mode
    with pytest.raises(NotImplementedError):
        plan.invert_u_dev(0, 0, mode='wrap')        # (refused before any pointer is used)
    plan.close()


def test_c_level_mode_codes():
    """gpa_invert_u_mode refuses a code outside 0 .. 4 with GPA_ERR_ARG and names the codes"""
    shape = (8, 9)
    plan = _lib.Plan(shape, 1, np.float64)
    us, out = np.zeros((2,) + shape), np.zeros((2,) + shape)
    ok = plan.lib.gpa_invert_u_mode(plan.handle, _lib._ptr(us), 2, 0, 1, 4, _lib._ptr(out))
    assert ok == 0
    for bad in (5, -1):
        rc = plan.lib.gpa_invert_u_mode(plan.handle, _lib._ptr(us), 2, 0, 1, bad, _lib._ptr(out))
        msg = _lib.last_error()
        assert rc == -1, (bad, rc)             # GPA_ERR_ARG (include/gpa_hip.h)
        for word in ('nearest', 'constant', 'reflect', 'grid-mirror', 'mirror', 'grid-wrap', '0', '4'):
            assert word in msg, (bad, msg)
    plan.close()
