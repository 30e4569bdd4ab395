"""Mirror of pyGPA/imagetools.py: image preparation in front of the GPA chain, on the device.

Same names, positional order and defaults as the reference, plus the house ``dtype=None`` keyword (None: float64).  Inputs and
outputs are host NumPy arrays; the work runs in libgpa_hip.so and there is no CPU fallback.  The ``*_dev`` forms take a
``_lib.Plan`` and device pointers for callers that keep the image on the device between stages (undistort -> trim ...).

``homogenize_per_axis`` runs its default reducfunc, the per-line ``np.nanmedian`` (and ``np.median``), as a selection kernel on
the device; any other callable is evaluated on the host and only its lines go to the device.

Not mirrored: the plotting helpers (``fftplot``, ``indicate_k``) and ``to_KovesiRGB``.
"""
import numpy as np

from . import _lib
from ._lib import GPAError  # noqa: F401
from .geometric_phase_analysis import fftbounds  # noqa: F401

DEFAULT_DTYPE = np.float64
# frames of one upload of generate_mask: chunks of at most this many bytes (one frame at least)
MASK_CHUNK_BYTES = 256 << 20


def _real(dtype):
    dtype = np.dtype(DEFAULT_DTYPE if dtype is None else dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64')
    return dtype.type


def _image2d(image, what='image'):
    image = np.asarray(image)
    if image.ndim >= 3:
        raise NotImplementedError('%s has %d dimensions: colour images are not served, only 2-D arrays' % (what, image.ndim))
    if image.ndim != 2:
        raise ValueError('%s must be 2-D' % what)
    if image.dtype.kind not in 'fiub':
        raise TypeError('%s must be real' % what)
    return image


def _homogenize_args(image, mask, sigma):
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError('image must be 2-D')
    if image.dtype.kind not in 'fiub':
        raise TypeError('image must be real')
    mask = np.asarray(mask)
    if mask.dtype != np.bool_:
        raise TypeError('mask must have dtype bool (the reference takes any other mask as weights in one of its two filters '
                        'and as truth values in the other)')
    if mask.shape != image.shape:
        raise ValueError('mask %s does not match the image %s' % (mask.shape, image.shape))
    if np.ndim(sigma) != 0:
        raise ValueError('sigma must be one scalar')
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError('sigma must be positive and finite')
    if image.dtype.kind == 'f' and not np.all(np.isfinite(image[mask])):
        raise ValueError('image holds a non-finite sample under the mask')
    return image, mask, sigma


def gauss_homogenize2(image, mask, sigma, nan_scale=None, dtype=None):
    """image / VV, VV the Gaussian average of the image that ignores what mask excludes (imagetools.py:92-105):
    VV = gaussian_filter(where(mask, image, 0), sigma) / gaussian_filter(mask, sigma).  Where no true mask sample lies within
    the filter's box VV is NaN, or nan_scale when given -- the reference's pattern, exactly.

    image: 2-D real; mask: 2-D bool of the same shape (anything else raises TypeError); sigma: one positive finite scalar.
    A non-finite sample under the mask raises ValueError (outside the mask NaNs are ignored, as in the reference).
    Deviation: an integer image is converted to the plan's precision first; the reference would filter it in integers."""
    image, mask, sigma = _homogenize_args(image, mask, sigma)
    plan = _lib.get_plan(image.shape, 1, _real(dtype))
    return plan.gauss_homogenize(image, mask, sigma, nan_scale)


def gauss_homogenize3(image, mask, sigma, dtype=None):
    """gauss_homogenize2 with nan_scale=1 (imagetools.py:108-109): pixels out of the mask's reach are left as they are"""
    return gauss_homogenize2(image, mask, sigma, nan_scale=1, dtype=dtype)


def gauss_homogenize_dev(plan, image_ptr, mask_ptr, out_ptr, sigma, nan_scale=None, vv_ptr=None):
    """gauss_homogenize2 of an image that is resident on the device (`plan`: a _lib.Plan of its shape; image_ptr / out_ptr /
    vv_ptr: device pointers to n0 x n1 reals of the plan's precision; mask_ptr: n0 x n1 bytes, 0 is false): enqueued on the
    plan's stream, nothing comes to the host.  vv_ptr (optional) receives VV.  Nothing is checked on the host: a non-finite
    sample under the mask gives NaN on at least the (2R+1)^2 box the reference spreads it over."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError('sigma must be positive and finite')
    plan.gauss_homogenize_dev(image_ptr, mask_ptr, out_ptr, sigma, nan_scale, vv_ptr)


# frames of one device call of homogenize_per_axis_stack: chunks of at most this many bytes (one frame at least)
AXIS_CHUNK_BYTES = 256 << 20


def _per_axis_args(image, mask, sigma, what='image', ndim=2):
    image = np.asarray(image)
    if image.ndim != ndim:
        raise ValueError('%s must be %d-D' % (what, ndim))
    if image.dtype.kind not in 'fiub':
        raise TypeError('%s must be real' % what)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype != np.bool_:
            raise TypeError('mask must have dtype bool')
        if mask.shape != image.shape[-2:]:
            raise ValueError('mask %s does not match the image %s' % (mask.shape, image.shape[-2:]))
    if np.ndim(sigma) != 0:
        raise ValueError('sigma must be one scalar')
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError('sigma must be positive and finite')
    if min(image.shape[-2:]) < 4 or max(image.shape[-2:]) > _lib.LINES_MAX_N:
        raise ValueError('both axes must hold 4 .. %d samples, not %s' % (_lib.LINES_MAX_N, image.shape[-2:]))
    return image, mask, sigma


def homogenize_per_axis(image, sigma=200, mask=None, reducfunc=np.nanmedian, dtype=None):
    """Divide out a smooth profile per column, then per row (imagetools.py:112-125): for axis 0, then axis 1,
    profile = gaussian_filter(reducfunc(where(mask, res, nan), axis, keepdims=True), sigma); res /= profile / profile.max().
    Removes detector stripes and per-line gain, which a 2-D Gaussian average follows instead.

    reducfunc np.nanmedian (the default) and np.median are recognised by identity and run on the device: exact per-line
    selections with NumPy's bits, the second axis taken from the image after the first division without storing it.  Any
    other callable is called on the host exactly as the reference calls it, once per axis; its line goes to the device for
    the filter and the divisions.  That path costs a download of res per axis.
    A line without any valid sample has the median NaN, and max() spreads it: the whole result is NaN, as in the reference.

    image: 2-D real, both axes 4 .. 16384; mask: None or 2-D bool of the same shape; sigma: one positive finite scalar.
    Deviation: an integer image is converted to the plan's precision first (the reference fails on its in-place division)."""
    image, mask, sigma = _per_axis_args(image, mask, sigma)
    if not callable(reducfunc):
        raise TypeError('reducfunc must be callable')
    plan = _lib.get_plan(image.shape, 1, _real(dtype))
    if reducfunc is np.nanmedian or reducfunc is np.median:
        return plan.homogenize_per_axis(image, sigma, mask, propagate_nan=reducfunc is np.median)
    image = plan._img(image)
    line0 = _reduced(reducfunc, image, mask, 0)
    res = plan.homogenize_lines(image, sigma, line0)
    return plan.homogenize_lines(image, sigma, line0, _reduced(reducfunc, res, mask, 1))


def _reduced(reducfunc, res, mask, axis):
    src = res if mask is None else np.where(mask, res, np.nan)
    line = np.asarray(reducfunc(src, axis=axis, keepdims=True))
    want = (1, res.shape[1]) if axis == 0 else (res.shape[0], 1)
    if line.shape != want:
        raise ValueError('reducfunc returned the shape %s along axis %d, not %s' % (line.shape, axis, want))
    return line


def homogenize_per_axis_stack(frames, sigma=200, mask=None, dtype=None):
    """homogenize_per_axis (np.nanmedian) of every frame of a stack (B, n0, n1) that shares one mask: one device call per
    chunk of frames.  Frame b equals the single call bit for bit."""
    frames, mask, sigma = _per_axis_args(frames, mask, sigma, what='frames', ndim=3)
    if frames.shape[0] < 1:
        raise ValueError('frames must hold at least one frame')
    real = _real(dtype)
    plan = _lib.get_plan(frames.shape[1:], 1, real)
    per = max(1, AXIS_CHUNK_BYTES // max(1, frames.shape[1] * frames.shape[2] * np.dtype(real).itemsize))
    out = np.empty(frames.shape, dtype=real)
    for a in range(0, len(frames), per):
        out[a:a + per] = plan.homogenize_per_axis(frames[a:a + per], sigma, mask)
    return out


def homogenize_per_axis_dev(plan, image_ptr, mask_ptr, out_ptr, sigma, profiles_ptr=None):
    """homogenize_per_axis (np.nanmedian) of an image that is resident on the device (`plan`: a _lib.Plan of its shape;
    image_ptr / out_ptr: device pointers to n0 x n1 reals of the plan's precision; mask_ptr: n0 x n1 bytes, 0 is false, or
    None): enqueued on the plan's stream, nothing comes to the host.  profiles_ptr (optional) receives the two filtered
    profiles, n1 values then n0."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError('sigma must be positive and finite')
    plan.homogenize_per_axis_dev(image_ptr, mask_ptr, out_ptr, sigma, profiles_ptr=profiles_ptr)


def nanmedian_lines(image, axis, mask=None, keepdims=True, dtype=None):
    """np.nanmedian(where(mask, image, nan), axis=axis, keepdims=keepdims) on the device: an exact selection per line, NumPy's
    bits in both precisions.  image: 2-D real; axis 0 or 1 (the reduced axis holds at most 16384 samples); mask: None or 2-D
    bool.  An axis shorter than the plan's smallest (4) is served by repeating the image four times along it, which leaves
    every median as it is: each sample then occurs four times, and the two middle ranks hold what they held."""
    image = _image2d(image)
    if axis not in (0, 1, -1, -2):
        raise ValueError('axis must be 0 or 1')
    axis = axis % 2
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype != np.bool_:
            raise TypeError('mask must have dtype bool')
        if mask.shape != image.shape:
            raise ValueError('mask %s does not match the image %s' % (mask.shape, image.shape))
    if image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError('image is empty')
    if image.shape[axis] > _lib.LINES_MAX_N:
        raise ValueError('axis %d holds %d samples, more than %d' % (axis, image.shape[axis], _lib.LINES_MAX_N))
    real = _real(dtype)
    nlines = image.shape[1 - axis]
    reps = tuple(4 if n < 4 else 1 for n in image.shape)
    if reps != (1, 1):
        image = np.tile(image, reps)
        mask = None if mask is None else np.tile(mask, reps)
    med = _lib.get_plan(image.shape, 1, real).line_nanmedian(image, axis, mask)[:nlines]
    if not keepdims:
        return med
    return med.reshape((1, nlines) if axis == 0 else (nlines, 1))


def generate_mask(dataset, mask_value, r=20, dtype=None):
    """Boolean (n0, n1) mask that is False wherever any frame of `dataset` (B, n0, n1) equals mask_value, eroded with a disk
    of radius r (imagetools.py:178-185).  The frames go up in chunks and accumulate on the device.  The comparison runs in
    the plan's precision: with dtype=np.float32 frames and mask_value are rounded to float32 first.  A NaN mask_value hits
    nothing, as in NumPy."""
    dataset = np.asarray(dataset)
    if dataset.ndim != 3 or dataset.shape[0] < 1:
        raise ValueError('dataset must be a stack (B, n0, n1) with B >= 1, not %s' % (dataset.shape,))
    r = int(r)
    if r < 0 or r > _lib.PREP_MAX_R:
        raise ValueError('r must be within 0 .. %d' % _lib.PREP_MAX_R)
    real = _real(dtype)
    plan = _lib.get_plan(dataset.shape[1:], 1, real)
    per = max(1, MASK_CHUNK_BYTES // max(1, dataset.shape[1] * dataset.shape[2] * np.dtype(real).itemsize))
    hit = None
    for a in range(0, len(dataset), per):
        hit = plan.mask_any_equal(dataset[a:a + per], mask_value, hit)
    return plan.mask_erode_disk(hit, r, invert=True).astype(bool)


def cull_by_mask(data, mask):
    """data[..., rows, columns] without the edge rows and columns that mask (2-D) leaves fully False (imagetools.py:188-194).
    The bounds are computed on the device, the slice is taken on the host.  ValueError for an all-False mask."""
    data = np.asarray(data)
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError('mask must be 2-D')
    if data.ndim < 2 or data.shape[-2:] != mask.shape:
        raise ValueError('data %s does not end in the shape of the mask %s' % (data.shape, mask.shape))
    lims = _lib.get_plan(mask.shape, 1, DEFAULT_DTYPE).mask_bounds(mask != 0)
    return _cull(data, lims)


def _cull(data, lims):
    x0, x1, y0, y1 = (int(v) for v in lims)
    if x1 <= x0 or y1 <= y0:
        raise ValueError('mask has no true sample')
    return data[..., x0:x1, y0:y1]


def mask_bounds_dev(plan, mask_ptr):
    """[[first row, last row + 1], [first column, last column + 1]] with a true sample of a device-resident byte mask"""
    lims = plan.mask_bounds_dev(mask_ptr)
    if lims[1] <= lims[0] or lims[3] <= lims[2]:
        raise ValueError('mask has no true sample')
    return np.array([[lims[0], lims[1]], [lims[2], lims[3]]])


def trim_nans(image, dtype=None):
    """image without the rows and columns that hold only NaN, wherever they lie (imagetools.py:128-142).  2-D only."""
    image = _image2d(image)
    rows, cols = _lib.get_plan(image.shape, 1, _real(dtype)).nan_lines(image)
    return image[~rows][:, ~cols]


def _lims2(lims):
    x0, x1, y0, y1 = (int(v) for v in lims)
    if x1 <= x0 or y1 <= y0:
        raise ValueError('trim_nans2: nothing is left of the image (every window holds a NaN on its edge)')
    return np.array([[x0, x1], [y0, y1]])


def trim_nans2(image, return_lims=False, dtype=None):
    """Trim the outer rows and columns that hold a NaN, keeping as much area as possible (imagetools.py:145-175): the
    reference's loop, run on the device; four integers come back.  2-D only.  ValueError where the window empties (an all-NaN
    image; the reference fails with an IndexError there)."""
    image = _image2d(image)
    lims = _lims2(_lib.get_plan(image.shape, 1, _real(dtype)).nan_trim_lims(image))
    out = image[lims[0, 0]:lims[0, 1], lims[1, 0]:lims[1, 1]].copy()
    return (out, lims) if return_lims else out


def trim_nans2_dev(plan, image_ptr):
    """[[x0, x1], [y0, y1]] of trim_nans2 for an image that is resident on the device (n0 x n1 reals of the plan's precision)"""
    return _lims2(plan.nan_trim_lims_dev(image_ptr))
