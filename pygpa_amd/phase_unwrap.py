"""Host-side mirror of pyGPA/phase_unwrap.py (weighted least-squares unwrap)."""
import numpy as np

from . import _lib

DEFAULT_DTYPE = np.float64


def phase_unwrap(psi, weight=None, kmax=100, dtype=None):
    """Unwrap a wrapped phase image (phase_unwrap.py:141-208)."""
    psi = np.asarray(psi)
    plan = _lib.get_plan(psi.shape, 1, DEFAULT_DTYPE if dtype is None else dtype)
    return plan.unwrap(psi, weight, kmax=kmax)[0]


def phase_unwrap_prediff(dx, dy, weight=None, kmax=100, dtype=None):
    """Unwrap from pre-differenced gradients (phase_unwrap.py:282-350)."""
    dx = np.asarray(dx)
    dy = np.asarray(dy)
    plan = _lib.get_plan((dx.shape[0], dy.shape[1]), 1, DEFAULT_DTYPE if dtype is None else dtype)
    return plan.unwrap_prediff(dx, dy, weight, kmax=kmax)[0]


def _stack_args(a, dy, weight, dtype):
    """shapes and dtype of a stack call, checked before a plan or the library is touched: (B, grid, dtype)"""
    dt = np.dtype(DEFAULT_DTYPE if dtype is None else dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64, got %s' % dt)
    arrays = [np.asarray(x) for x in (a, dy, weight) if x is not None]
    for x in arrays:
        if x.dtype.kind not in 'fiub':
            raise ValueError('the stack, its gradients and its weights must be real arrays, got %s' % x.dtype)
    B = _lib.unwrap_stack_shapes(np.shape(a), None if dy is None else np.shape(dy))
    grid = np.shape(a)[1:] if dy is None else (np.shape(a)[1], np.shape(dy)[2])
    if weight is not None:
        _lib.unwrap_stack_weight_planes(np.shape(weight), B, grid)
    return B, tuple(int(n) for n in grid), dt.type


def phase_unwrap_stack(psis, weight=None, kmax=100, dtype=None):
    """Unwrap a stack of wrapped phase images psis (B, N, M) in one device call: phi (B, N, M).

    weight: None, one (N, M) map for all images, or (B, N, M), one each.  The reference has no stack form: a Python loop
    over phase_unwrap (phase_unwrap.py:141-208) gives the same numbers, one solve -- a chain of 4 - 5 dependent kernel
    launches per PCG iteration -- after the other; here the B solves share that chain, each with its own stopping test."""
    B, grid, dt = _stack_args(psis, None, weight, dtype)
    plan = _lib.get_plan(grid, 1, dt)
    return plan.unwrap_stack(psis, weight, kmax=kmax)[0]


def phase_unwrap_prediff_stack(dxs, dys, weight=None, kmax=100, dtype=None):
    """Unwrap a stack from pre-differenced gradients dxs (B, N, M - 1), dys (B, N - 1, M) in one device call: phi (B, N, M).

    weight as in phase_unwrap_stack.  In the reference: a Python loop over phase_unwrap_prediff (phase_unwrap.py:282-350)."""
    B, grid, dt = _stack_args(dxs, dys, weight, dtype)
    plan = _lib.get_plan(grid, 1, dt)
    return plan.unwrap_prediff_stack(dxs, dys, weight, kmax=kmax)[0]


# the reference's *_ref variants are the same algorithm without the precomputed
# scaling (phase_unwrap.py:26-78, :211-279); tests/test_phase_unwrap.py asserts equality
phase_unwrap_ref = phase_unwrap
phase_unwrap_ref_prediff = phase_unwrap_prediff


def _wrapToPi(x):
    return (x + np.pi) % (2 * np.pi) - np.pi
