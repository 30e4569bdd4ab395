"""Unit-cell averaging of images on the GPU: mirror of pyGPA/unit_cell_averaging.py.

``unit_cell_average`` folds every pixel of an image, displaced by ``u``, into one unit cell of the lattice spanned by
``ks`` (upscaled by ``z``), drizzle style; ``expand_unitcell`` paints such a cell back onto a full grid.  Both run in
libgpa_hip.so (pygpa_amd/csrc/gpa_ucell.hip); the small geometric helpers below are host NumPy, with the reference's
names, signatures and results, because the GPU entry points take the geometry they compute.

Differences from the reference, all at the cell's border: a pixel whose corner falls on index ``rsize`` (one past the
last bin) has that corner dropped, where the reference raises IndexError (numba: writes out of bounds).  A corner at
index -1 lands in the last row / column, as in the reference.
"""
import numpy as np

from . import _lib

__all__ = ['forward_transform', 'backward_transform', 'cart_in_uc', 'float_overlap', 'calc_ucell_parameters',
           'unit_cell_average', 'unit_cell_average_stack', 'add_to_position', 'expand_unitcell']


def forward_transform(vecs, ks):
    """Cartesian vectors (last axis) -> lattice coordinates, i.e. vecs @ ks.T"""
    return vecs @ np.asarray(ks).T


def backward_transform(vecs, ks):
    """Lattice coordinates (last axis) -> cartesian vectors, i.e. vecs @ inv(ks).T"""
    return vecs @ np.linalg.inv(ks).T


def cart_in_uc(vecs, ks, rmin=0):
    """Cartesian vectors (last axis) folded into the unit cell spanned by ks, relative to rmin.

    Per axis, as the kernels compute it: the lattice coordinates a_k = v0 ks[k, 0] + v1 ks[k, 1] reduced into [0, 1]
    (NumPy's remainder: a tiny negative coordinate gives exactly 1), mapped back with inv(ks)."""
    k = np.asarray(ks, dtype=np.float64)
    kinv = np.linalg.inv(k)
    v = np.asarray(vecs, dtype=np.float64)
    a0 = np.remainder(v[..., 0] * k[0, 0] + v[..., 1] * k[0, 1], 1.)
    a1 = np.remainder(v[..., 0] * k[1, 0] + v[..., 1] * k[1, 1], 1.)
    return np.stack([a0 * kinv[0, 0] + a1 * kinv[0, 1], a0 * kinv[1, 0] + a1 * kinv[1, 1]], axis=-1) - rmin


def float_overlap(f):
    """2 x 2 overlap areas of a unit pixel shifted by the fractions f = (f0, f1) with the bins it covers.

    Laid out as the reference lays it out: entry [li, lj] = (f0 if lj else 1 - f0) * (f1 if li else 1 - f1)."""
    f = np.asarray(f, dtype=np.float64)
    w = np.stack((1 - f, f))              # w[c, axis]
    return w[:, 0][None, :] * w[:, 1][:, None]


def calc_ucell_parameters(ks, z):
    """(rmin, rsize) of the cell spanned by ks upscaled by z: the cell's cartesian lower corner, and its bounding box in
    upscaled bins."""
    # the cell's four vertices in cartesian coordinates: 0, the two columns of inv(ks) and their sum
    e0, e1 = np.linalg.inv(np.asarray(ks, dtype=np.float64)).T
    vertices = np.stack([np.zeros(2), e1, e0, e0 + e1])
    lo, hi = vertices.min(axis=0), vertices.max(axis=0)
    bins = np.ceil(hi - np.floor(lo))        # whole pixels the cell's bounding box spans from the pixel below lo
    return lo, tuple(int(z * b) for b in bins)


def add_to_position(value, R, res, weights):
    """Host-side: add value at the (upscaled) cell position R to res and its overlap to weights, in place."""
    R = np.asarray(R, dtype=np.float64)
    base = np.floor(R)
    ov = float_overlap(R - base)
    i0, j0 = base.astype(np.int32)
    for li in range(2):
        for lj in range(2):
            res[i0 + li, j0 + lj] += value * ov[li, lj]
            weights[i0 + li, j0 + lj] += ov[li, lj]


def _geometry(ks, z):
    ks = np.asarray(ks, dtype=np.float64)[:2]
    if ks.shape != (2, 2):
        raise ValueError('ks must hold (at least) two 2-D k-vectors')
    rmin, rsize = calc_ucell_parameters(ks, z)
    return _lib.UcellGeom.make(ks, np.linalg.inv(ks), rmin, rsize, z)


def _dtype_of(a, dtype):
    if dtype is not None:
        return np.dtype(dtype)
    return np.dtype(np.float32) if np.asarray(a).dtype == np.float32 else np.dtype(np.float64)


def unit_cell_average(image, ks, u=None, z=1, only_generate_func=False, dtype=None):
    """Average `image` over all unit cells spanned by `ks`, following the displacement `u` (2, N, M), into a cell upscaled
    by `z`.  NaN pixels of the image are ignored (a mask).  Returns the cell as a float64 array of shape rsize
    (calc_ucell_parameters), NaN where no pixel landed, in cartesian (not lattice) coordinates.

    only_generate_func=True returns ``f(image, u)`` with u shaped (N, M, 2), as the reference's generated function takes
    it.  The precision follows the image (float32 images run the float32 build; the sums are float64 in both) unless
    `dtype` says otherwise."""
    geom = _geometry(ks, z)

    def average(img, uu):
        img = np.asarray(img)
        plan = _lib.get_plan(img.shape, 1, _dtype_of(img, dtype))
        return plan.unit_cell_average(img, geom, uu)

    if only_generate_func:
        return lambda img, uu: average(img, None if uu is None else np.moveaxis(np.asarray(uu), -1, 0))
    return average(image, u)


def unit_cell_average_stack(frames, ks, u=None, z=1, dtype=None, chunk=64):
    """unit_cell_average of every frame of `frames` (B, N, M), all with the same displacement `u` (2, N, M): the pixel
    lists are built once per `chunk` frames.  Returns (B,) + rsize float64; frame b equals
    unit_cell_average(frames[b], ks, u, z) bitwise."""
    frames = np.asarray(frames)
    if frames.ndim != 3:
        raise ValueError('frames must have shape (B, N, M)')
    dt = _dtype_of(frames, dtype)
    shape = frames.shape[1:]
    if u is not None and np.shape(u) != (2,) + shape:
        raise ValueError('u must have shape (2, N, M)')
    plan = _lib.get_plan(shape, 1, dt)
    geom = _geometry(ks, z)
    rs = tuple(geom.rsize)
    chunk = max(1, min(int(chunk), len(frames), _lib.UCELL_MAX_FRAMES))
    out = np.empty((len(frames),) + rs, dtype=np.float64)
    bufs = [_lib.DeviceBuffer(chunk * frames[0].size * dt.itemsize, plan.device),
            _lib.DeviceBuffer(chunk * out[0].nbytes, plan.device)]
    try:
        if u is not None:
            bufs.append(_lib.DeviceBuffer(2 * frames[0].size * dt.itemsize, plan.device))
            bufs[2].upload(np.ascontiguousarray(u, dtype=dt))
        for b0 in range(0, len(frames), chunk):
            nb = min(chunk, len(frames) - b0)
            bufs[0].upload(np.ascontiguousarray(frames[b0:b0 + nb], dtype=dt))
            plan.unit_cell_average_dev(bufs[0].ptr, geom, bufs[1].ptr, None if u is None else bufs[2].ptr, nframes=nb)
            plan.sync()
            bufs[1].download_into(out[b0:b0 + nb])
        return out
    finally:
        for b in bufs:
            b.free()


def expand_unitcell(unit_cell_image, ks, shape, z=1, z2=1, u=0, dtype=None):
    """Paint the cell `unit_cell_image` (as unit_cell_average returns it, upscaled by `z`) onto a grid of `shape`, sampled
    at r / z2 + u(r) (u: 0 or (2, *shape)), with an order-3 spline (NaN cells count as 0).  The precision follows `u` when
    it is a float32 array (float64 otherwise) unless `dtype` says otherwise."""
    shape = (int(shape[0]), int(shape[1]))
    geom = _geometry(ks, z)
    cell = np.asarray(unit_cell_image, dtype=np.float64)
    if cell.shape != tuple(geom.rsize):
        raise ValueError('unit_cell_image has shape %s, the cell of ks and z has %s' % (cell.shape, tuple(geom.rsize)))
    if np.isscalar(u) or np.ndim(u) == 0:
        uu = None if float(u) == 0.0 else np.full((2,) + shape, float(u))
    else:
        uu = np.asarray(u)
    plan = _lib.get_plan(shape, 1, _dtype_of(uu, dtype) if uu is not None else np.dtype(dtype or np.float64))
    return plan.expand_unitcell(cell, geom, z2, uu)
