"""undistort_image of a whole stack of frames in one device call (gpa_undistort_image_batch[_dev],
GPA.undistort_image_stack) against the loop over the single-image entry points, BIT FOR BIT: every per-output sum of the
batched kernels keeps the order of the single-plane ones, so there is no tolerance here.  Run with `-m gpu` on an MI355X.

Shapes are chosen for where the kernels can go wrong: B = 5 is neither a multiple of the resampling kernel's NF = 4 frames
per pass nor below it (one full pass plus a tail), B = 1 is a tail alone, 2100 is longer than the 2048 outputs of one FIR
workgroup (rows) and spans many 32-row column tiles; 9 frames of 2100 x 20 are enough workgroups per frame that a thread
takes two passes of four frames in its loop (and the ninth frame goes to another workgroup row as a tail).  The fields are a smooth bump of a few pixels plus a shear, so that
some sample coordinates leave the image (cval) and the frames' edges matter."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA
from pygpa_amd.synthetic import hex_kvecs, hex_moire, explicit_klists

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
SHAPES = [(5, 96, 80), (1, 63, 65), (3, 20, 2100), (3, 2100, 20), (9, 2100, 20)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def field(shape, k=0):
    """bump number k (amplitude, centre and width vary with k) plus a shear of +-3 px across the image"""
    n0, n1 = shape
    x, y = np.mgrid[:n0, :n1].astype(np.float64)
    xn, yn = x / n0 - 0.5 - 0.05 * k, y / n1 - 0.5 + 0.04 * k
    bump = (2.5 + 0.6 * k) * np.exp(-0.5 * ((xn / (0.18 + 0.01 * k)) ** 2 + (yn / 0.15) ** 2))
    return np.stack([bump + 6.0 * (y / n1 - 0.5), -0.6 * bump + 5.0 * (x / n0 - 0.5)])


@functools.lru_cache(maxsize=None)
def case(shape3, dtype, per_frame):
    """frames, u and the loop over the single-image call (the reference of every test that shares the case); read-only"""
    B, shape = shape3[0], shape3[1:]
    kvecs = hex_kvecs(0.12, 11.0)
    frames = np.stack([hex_moire(shape, kvecs, noise=0.1, seed=10 + b) for b in range(B)]).astype(dtype)
    u = (np.stack([field(shape, b) for b in range(B)]) if per_frame else field(shape)).astype(dtype)
    plan = _lib.Plan(shape, 1, dtype)
    loop = np.stack([plan.undistort_image(frames[b], u[b] if per_frame else u) for b in range(B)])
    plan.close()
    for a in (frames, u, loop):
        a.setflags(write=False)
    return frames, u, loop


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape3', SHAPES)
def test_shared_field_equals_loop_bitwise(shape3, dtype):
    frames, u, loop = case(shape3, dtype, False)
    # some coordinates do leave the image (cval = 0 exactly) and most do not
    assert 0 < np.count_nonzero(loop == 0) < 0.5 * loop.size
    out = GPA.undistort_image_stack(frames, u, dtype=dtype)
    assert out.shape == frames.shape and out.dtype == np.dtype(dtype)
    for b in range(shape3[0]):
        assert same(out[b], loop[b]), 'frame %d' % b


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape3', [(5, 96, 80), (3, 20, 2100), (1, 63, 65)])
def test_per_frame_fields_equal_loop_bitwise(shape3, dtype):
    frames, u, loop = case(shape3, dtype, True)
    assert u.shape == (shape3[0], 2) + shape3[1:]
    out = GPA.undistort_image_stack(frames, u, dtype=dtype)
    for b in range(shape3[0]):
        assert same(out[b], loop[b]), 'frame %d' % b


def test_against_oracle():
    """the bound of the single-image parity test (tests/test_gpu_parity.py test_f1_reconstruction_like_reference): 1e-9 of
    the reference's largest magnitude, per frame"""
    frames, u, _ = case((5, 96, 80), np.float64, False)
    out = GPA.undistort_image_stack(frames, u)
    for b in range(5):
        ref = orc.undistort_image(frames[b], u)
        err = float(np.abs(out[b] - ref).max() / np.abs(ref).max())
        print('frame %d: rel err vs oracle %.3g' % (b, err))
        assert err < 1e-9


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_resident_chain(dtype):
    """extract_displacement_field_batch_dev's output, left on the device, undistorts the frames with per_frame=True and
    scale=-1: the same bits (result and u_inv) as the loop of undistort_image_dev(scale=-1) over the same device fields"""
    B, shape = 3, (128, 128)
    npx, item = shape[0] * shape[1], np.dtype(dtype).itemsize
    kvecs = hex_kvecs(0.12, 11.0)
    imgs = np.stack([hex_moire(shape, kvecs, field(shape, b), noise=0.1, seed=b) for b in range(B)])
    imgs = (imgs - imgs.mean(axis=(1, 2), keepdims=True)).astype(dtype)
    klists = np.stack(explicit_klists(kvecs, np.linalg.norm(kvecs, axis=1).mean() / 2.5, 2, 2))
    plan = _lib.Plan(shape, klists.shape[0] * klists.shape[1], dtype)
    d = {k: _lib.DeviceBuffer(n * npx * item) for k, n in (('img', B), ('u', 2 * B), ('rec', B), ('uinv', 2 * B), ('rec1', 1), ('uinv1', 2))}
    try:
        d['img'].upload(imgs)
        assert plan.lib.gpa_supports_batch(plan.handle)
        plan.extract_displacement_field_batch_dev(d['img'].ptr, B, kvecs, klists, 8, 16, 10, d['u'].ptr)
        plan.undistort_image_batch_dev(d['img'].ptr, B, d['u'].ptr, d['rec'].ptr, per_frame=True, scale=-1.0, uinv_ptr=d['uinv'].ptr)
        plan.sync()
        rec, uinv = d['rec'].download((B,) + shape, dtype), d['uinv'].download((B, 2) + shape, dtype)
        assert np.abs(uinv[np.isfinite(uinv)]).max() > 0.5      # (the fields are a few pixels: the chain did run)
        for b in range(B):
            plan.undistort_image_dev(d['img'].ptr + b * npx * item, d['u'].ptr + 2 * b * npx * item, d['rec1'].ptr,
                                     uinv_ptr=d['uinv1'].ptr, scale=-1.0)
            plan.sync()
            assert same(rec[b], d['rec1'].download(shape, dtype)), 'frame %d' % b
            assert same(uinv[b], d['uinv1'].download((2,) + shape, dtype)), 'u_inv of frame %d' % b
    finally:
        for b in d.values():
            b.free()
        plan.close()


@pytest.mark.parametrize('per_frame', [False, True])
def test_chunks_do_not_change_the_result(gpa_option, per_frame):
    """a scratch bound of two frames' spline planes: the 5 frames pass in three chunks (2 + 2 + 1), inside the library and
    -- the `chunk` argument -- as three library calls; both equal the one-chunk call"""
    frames, u, loop = case((5, 96, 80), np.float64, per_frame)
    n0, n1 = 96, 80
    elems = 4 * (n0 + 24) * (n1 + 24) + 3 * n0 * n1 if per_frame else 2 * n0 * n1     # scratch elements per frame
    plan = _lib.Plan((n0, n1), 1, np.float64)
    whole = plan.undistort_image_stack(frames, u)
    ws_whole = plan.workspace_bytes
    plan.close()
    gpa_option('LF_STACK_BYTES', str(2 * elems * 8 + 8))
    plan = _lib.Plan((n0, n1), 1, np.float64)
    chunked = plan.undistort_image_stack(frames, u)
    assert ws_whole - plan.workspace_bytes == 3 * elems * 8      # the workspace holds two frames' planes, not five
    gpa_option('LF_STACK_BYTES', None)
    calls = plan.undistort_image_stack(frames, u, chunk=2)
    plan.close()
    assert same(whole, loop) and same(chunked, whole) and same(calls, whole)


def test_frame_count_limits():
    plan = _lib.Plan((64, 64), 1, np.float32)
    buf = _lib.DeviceBuffer(4 * 64 * 64 * 4)
    try:
        for B in (0, 65536, -1):
            for rc in (plan.lib.gpa_undistort_image_batch_dev(plan.handle, C.c_void_p(buf.ptr), B, C.c_void_p(buf.ptr), 0, 1.0, None,
                                                              C.c_void_p(buf.ptr)),
                       plan.lib.gpa_undistort_image_batch(plan.handle, C.c_void_p(buf.ptr), B, C.c_void_p(buf.ptr), 0, C.c_void_p(buf.ptr))):
                assert rc == -1        # GPA_ERR_ARG
                assert '65535' in _lib.last_error() and 'B = %d' % B in _lib.last_error()
        assert plan.lib.gpa_undistort_image_batch_dev(plan.handle, None, 1, C.c_void_p(buf.ptr), 0, 1.0, None, C.c_void_p(buf.ptr)) == -1
        assert 'null' in _lib.last_error()
    finally:
        buf.free()
        plan.close()
