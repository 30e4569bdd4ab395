"""Host-side mirror of the phase-gradient -> Jacobian -> lattice-properties chain of
pyGPA/property_extract.py: the immediate consumer of the
``'grad'`` output of ``wfr2_grad_opt``.

Same names, argument order and return layout as the reference.  The per-pixel work -- the
weighted least squares of the phase gradients and the 2x2 singular value decomposition --
runs in libgpa_hip.so (gpa_phasegradient2J / gpa_props_from_jac, include/gpa_hip.h); the
k-vector bookkeeping on P x 2 arrays stays on the host.  No CPU fallback.

J straight from a displacement field or from phases -- u2J, u2Jac, phases2J, phases2Jac, calc_props_from_phases, phys_props_from_Jac
(property_extract.py:13-52, :181-217, :258-278) and the stack form u2J_stack -- is one pass over the data (gpa_field_jacobian,
gpa_phases_jacobian, gpa_phys_props_from_jac): the difference stencil, the per-pixel solve and the 2 x 2 SVD in one
kernel, with J, the properties of 1 + J, or both as outputs; u2J_dev and phases2J_dev are the device-resident forms.  Differences:
u2Jac works (the reference's loses its spacing argument and raises TypeError); `weights` must have the shape of `phases`; shape
errors are ValueError before the library is touched.  The moire conversions (J_2_J_diff, moire_props_*, f2angle) are not provided.

phasegradient2J_stack, calc_props_from_phasegradient_stack and phasegradient2J_dev take the gradients and weights of a whole stack
(extract_displacement_field_stack(..., return_gs=True)) through one plan-free pass (gpa_gradients_jacobian): J, the properties of
1 + J, or both, frame b equal to the single functions bit for bit.  The single functions keep their two-kernel path.

The Kerelsky decomposition of the displacement-gradient field -- Kerelsky_Jac, Kerelsky_J and its per-pixel worker
iterate_J_leastsq (property_extract.py:696-883) -- runs in the same library (gpa_kerelsky_fit, one bounded Levenberg-Marquardt
solve per pixel and lane, csrc/gpa_kerelsky.h) in place of scipy.optimize.least_squares behind a dask gufunc; Kerelsky_J_dev is its
device-resident form.  The four `latticegen` functions behind the model are restated.  Differences, all stated at
the functions: `lq_kwargs` takes `max_nfev` only; a pixel with a non-finite Jacobian gives NaN where the reference raises; a global
fit counts as failed when its result is not finite.

Kerelsky, Kerelsky_plus and moire_amplitudes (fits of the k-vector lengths, no per-pixel work) and double_strain_decomp (marked
UNTESTED in the reference, prints from its loop) are out of scope.
"""
import numpy as np

from . import _lib
from .geometric_phase_analysis import DEFAULT_DTYPE, calc_diff_from_isotropic
from .mathtools import periodic_average, periodic_difference


def _dt(dtype):
    return DEFAULT_DTYPE if dtype is None else dtype


def phasegradient2J(kvecs, grads, weights, nmperpixel, iso_ref=True, sort=0, dtype=None):
    """J (N, M, 2, 2) directly from phase gradients (property_extract.py:69-101).

    With iso_ref the result is relative to ``kvecs + calc_diff_from_isotropic(kvecs)``.
    As in the reference, ``sort != 0`` reorders kvecs and grads but not weights."""
    kvecs = np.asarray(kvecs, dtype=np.float64).reshape(-1, 2)
    grads = np.asarray(grads)
    angles = np.arctan2(kvecs[:, 1], kvecs[:, 0])
    if sort == 0:
        lkvecs = kvecs
        order = np.arange(3)
    else:
        order = np.argsort(sort * periodic_difference(angles, periodic_average(angles)))
        lkvecs = kvecs[order]
    plan = _lib.get_plan(grads.shape[1:3], max(len(kvecs), 2), _dt(dtype))
    if iso_ref:
        dks = calc_diff_from_isotropic(lkvecs)
        return plan.phasegradient2J(lkvecs, grads[order], weights, nmperpixel, dks=dks)
    return plan.phasegradient2J(kvecs, grads, weights, nmperpixel)


def phasegradient2Jac(kvecs, grads, weights, nmperpixel, dtype=None):
    """Jac = 1 + J from phase gradients (property_extract.py:55-66).  The identity is added
    inside the device kernels where Jac is consumed; here it is added to the returned array."""
    J = phasegradient2J(kvecs, grads, weights, nmperpixel, dtype=dtype)
    return np.eye(2, dtype=J.dtype) + J


def props_from_Jac(Jac, refangle=0., refscale=1., diff=False, dtype=None, _add_identity=False):
    """(angle, aniangle, alpha, kappa) of a lattice from the Jacobian of its transformation
    (property_extract.py:137-178): array of shape (4,) + Jac.shape[:-2]."""
    return _lib.props_from_jac(Jac, add_identity=_add_identity, refangle=refangle, refscale=refscale, diff=diff,
                               dtype=_dt(dtype))


def props_from_J(J, refangle=0., refscale=1, dtype=None):
    """props_from_Jac(J + 1) (property_extract.py:220-221)."""
    return props_from_Jac(J, refangle=refangle, refscale=refscale, dtype=dtype, _add_identity=True)


def get_initial_props(ks, standardize=False):
    """(r_k, theta_0 [deg], symmetry) of a set of k-vectors (property_extract.py:491-503);
    ``standardize`` (mathtools.standardize_ks) is not provided."""
    if standardize:
        raise NotImplementedError('standardize_ks is outside the accelerated path')
    kvecs = np.asarray(ks, dtype=np.float64).reshape(-1, 2)
    symmetry = 2 * len(kvecs)
    r_k = np.linalg.norm(kvecs, axis=1).mean()
    theta_0 = np.rad2deg(periodic_average(np.arctan2(kvecs[:, 1], kvecs[:, 0]), 2 * np.pi / symmetry))
    hexa = np.arange(-180, 180, 60)
    diffind = np.argmin(np.abs(theta_0 + hexa - np.rad2deg(np.arctan2(kvecs[0, 1], kvecs[0, 0]))))
    return r_k, theta_0 + hexa[diffind], symmetry


def calc_props_from_phasegradient(kvecs, grads, weights, nmperpixel, dtype=None):
    """Lattice properties directly from the sweep's phase gradients
    (property_extract.py:234-255): props_from_Jac(1 + J) with the base angle of kvecs added."""
    J = phasegradient2J(kvecs, grads, weights, nmperpixel, dtype=dtype)
    _, theta_0, _ = get_initial_props(kvecs)
    return props_from_J(J, refangle=theta_0, dtype=dtype)


# ---- a stack of frames: gradients -> J and properties in one pass (gpa_gradients_jacobian, no plan) ----------------------------
def _stack_order(kvecs, grads, weights, sort, iso_ref):
    """(kvecs in solve order, grads[:, order], dks or None) of a stack: the bookkeeping of phasegradient2J"""
    kvecs = np.asarray(kvecs, dtype=np.float64).reshape(-1, 2)
    grads = np.asarray(grads)
    if grads.ndim != 5 or np.ndim(weights) != 4:
        raise ValueError('grads must have shape (B, P, N, M, 2) and weights (B, P, N, M)')
    if sort != 0 and iso_ref:   # (without iso_ref the single function solves in the given order, whatever `sort` says)
        angles = np.arctan2(kvecs[:, 1], kvecs[:, 0])
        order = np.argsort(sort * periodic_difference(angles, periodic_average(angles)))
        kvecs, grads = kvecs[order], grads[:, order]
    return kvecs, grads, (calc_diff_from_isotropic(kvecs) if iso_ref else None)


def phasegradient2J_stack(kvecs, grads, weights, nmperpixel, iso_ref=True, sort=0, dtype=None):
    """phasegradient2J of every frame of a stack in one call: grads (B, P, N, M, 2) and weights (B, P, N, M), e.g. the
    outputs of extract_displacement_field_stack(..., return_gs=True), -> J (B, N, M, 2, 2), frame b equal to
    phasegradient2J(kvecs, grads[b], weights[b], ...) bit for bit.  ``sort != 0`` reorders kvecs and grads[:, order] but not
    the weights, as the single function does."""
    lk, lg, dks = _stack_order(kvecs, grads, weights, sort, iso_ref)
    return _lib.gradients_jacobian(lk, lg, weights, nmperpixel, dks=dks, dtype=_dt(dtype))[0]


def calc_props_from_phasegradient_stack(kvecs, grads, weights, nmperpixel, dtype=None):
    """calc_props_from_phasegradient of every frame of a stack in one pass: (B, 4, N, M), frame b equal to the single function's
    bit for bit.  Only the properties are asked for, so J is never stored."""
    lk, lg, dks = _stack_order(kvecs, grads, weights, 0, True)
    _, theta_0, _ = get_initial_props(kvecs)
    return _lib.gradients_jacobian(lk, lg, weights, nmperpixel, dks=dks, want_J=False, want_props=True, refangle=theta_0,
                                   dtype=_dt(dtype))[1]


def phasegradient2J_dev(kvecs, grads_ptr, weights_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, iso_ref=True, stream=None,
                        add_identity=False, refangle=0., refscale=1., diff=False, dtype=None, device=0):
    """phasegradient2J_stack for gradients that are resident on the device (e.g. the grads and weights of
    Plan.extract_displacement_field_grad_batch_dev): grads_ptr holds `shape` = (P, N, M, 2) or (B, P, N, M, 2) values of `dtype`,
    weights_ptr that shape without its last axis.  J_ptr receives (B,) N x M x 2 x 2 values, props_ptr (B,) 4 x N x M --
    props_from_J of that J -- in the same pass; at least one of the two.  Asynchronous on `stream`."""
    kvecs = np.asarray(kvecs, dtype=np.float64).reshape(-1, 2)
    _lib.gradients_jacobian_dev(kvecs, grads_ptr, weights_ptr, shape, nmperpixel, J_ptr=J_ptr, props_ptr=props_ptr,
                                dks=calc_diff_from_isotropic(kvecs) if iso_ref else None, add_identity=add_identity,
                                refangle=refangle, refscale=refscale, diff=diff, dtype=_dt(dtype), device=device, stream=stream)


# ---- J and properties from a displacement field or from phases (property_extract.py:13-52, :181-217, :258-278) ---------------
def u2J(U, nmperpixel, dtype=None):
    """J (N, M, 2, 2) from the displacement field U (2, N, M) (property_extract.py:13-18): J[n, m, c, a] is
    np.gradient(-U[c], nmperpixel, axis=a), to the bit."""
    if np.ndim(U) != 3:
        raise ValueError('U must have shape (2, N, M); u2J_stack takes stacks')
    return _lib.field_jacobian(U, nmperpixel, dtype=_dt(dtype))[0]


def u2Jac(U, nmperpixel, dtype=None):
    """Jac = 1 + u2J(U, nmperpixel) (property_extract.py:21-26, where the call loses nmperpixel and raises TypeError); the identity
    is added in the kernel."""
    if np.ndim(U) != 3:
        raise ValueError('U must have shape (2, N, M)')
    return _lib.field_jacobian(U, nmperpixel, add_identity=True, dtype=_dt(dtype))[0]


def u2J_stack(us, nmperpixel, dtype=None):
    """u2J of every frame of a stack (B, 2, N, M) in one call: (B, N, M, 2, 2), frame b equal to u2J(us[b]) bit for bit."""
    if np.ndim(us) != 4:
        raise ValueError('us must have shape (B, 2, N, M)')
    return _lib.field_jacobian(us, nmperpixel, dtype=_dt(dtype))[0]


def u2J_dev(U_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, stream=None, add_identity=False, refangle=0., refscale=1.,
            diff=False, dtype=None, device=0):
    """u2J for a field that is resident on the device (e.g. the u of extract_displacement_field_stack): U_ptr holds `shape` =
    (2, N, M) or (B, 2, N, M) values of `dtype`.  J_ptr receives (B,) N x M x 2 x 2 values, props_ptr (B,) 4 x N x M --
    props_from_J of that J -- in the same pass; at least one of the two.  Asynchronous on `stream`."""
    _lib.field_jacobian_dev(U_ptr, shape, nmperpixel, J_ptr=J_ptr, props_ptr=props_ptr, add_identity=add_identity,
                            refangle=refangle, refscale=refscale, diff=diff, dtype=_dt(dtype), device=device, stream=stream)


def phases2J(kvecs, phases, weights, nmperpixel, dtype=None):
    """J (N, M, 2, 2) from phases (P, N, M), e.g. of iterate_GPA or phase_unwrap (property_extract.py:39-52): minus the per-pixel
    weighted least squares of wrapToPi(2 np.gradient(phases)) / 2 / nmperpixel against 2 pi kvecs.  `weights` must have the shape
    of `phases`."""
    return _lib.phases_jacobian(kvecs, phases, weights, nmperpixel, dtype=_dt(dtype))[0]


def phases2Jac(kvecs, phases, weights, nmperpixel, dtype=None):
    """Jac = 1 + phases2J (property_extract.py:29-36); the identity is added in the kernel."""
    return _lib.phases_jacobian(kvecs, phases, weights, nmperpixel, add_identity=True, dtype=_dt(dtype))[0]


def phases2J_dev(kvecs, phases_ptr, weights_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, stream=None, add_identity=False,
                 refangle=0., refscale=1., diff=False, dtype=None, device=0):
    """phases2J for phases and weights resident on the device, `shape` = (P, N, M) values of `dtype` each.  J_ptr receives
    N x M x 2 x 2 values, props_ptr 4 x N x M -- props_from_J of that J -- in the same pass; at least one of the two.
    Asynchronous on `stream`."""
    _lib.phases_jacobian_dev(kvecs, phases_ptr, weights_ptr, shape, nmperpixel, J_ptr=J_ptr, props_ptr=props_ptr,
                             add_identity=add_identity, refangle=refangle, refscale=refscale, diff=diff, dtype=_dt(dtype),
                             device=device, stream=stream)


def calc_props_from_phases(kvecs, phases, weights, nmperpixel, dtype=None):
    """Lattice properties directly from phases (property_extract.py:258-278): props_from_Jac(1 + phases2J) with the base angle of
    kvecs added, in one pass that never stores J."""
    _, theta_0, _ = get_initial_props(kvecs)
    return _lib.phases_jacobian(kvecs, phases, weights, nmperpixel, want_J=False, want_props=True, refangle=theta_0,
                                dtype=_dt(dtype))[1]


def phys_props_from_Jac(Jac, refangle=0., refscale=1, diff=False, poisson_ratio=0.16, dtype=None):
    """(angle, aniangle, alpha, epsilon) of a lattice from the Jacobian of its transformation, the heterostrain epsilon in place of
    the anisotropy kappa (property_extract.py:181-217): array of shape (4,) + Jac.shape[:-2]."""
    return _lib.phys_props_from_jac(Jac, refangle=refangle, refscale=refscale, diff=diff, poisson_ratio=poisson_ratio,
                                    dtype=_dt(dtype))


# ---- Kerelsky decomposition (property_extract.py:457-479, :696-883)----------------------------------------------------------
KERELSKY_DELTA = 0.16          # Poisson ratio of the strain matrix, as calc_abcd's delta (property_extract.py:511)


def _rot(angle_deg):
    a = np.deg2rad(angle_deg)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def twist_matrix(angle):
    """W(angle / 2) - W(-angle / 2), the transformation of a lattice twist over `angle` degrees (property_extract.py:457-479)."""
    return 2 * np.sin(np.deg2rad(angle / 2)) * np.array([[0., -1.], [1., 0.]])


def Jac_fit_diff(x, JacA0):
    """The residual the Kerelsky fits minimise (property_extract.py:696-704), on the host: for x = (theta, psi, epsilon, xi),
    angles in degrees, 1000 ravel(V^T D V W(theta + xi) - W(xi) - JacA0) with W the rotation, V = W(psi) and
    D = diag(1 / (1 + epsilon), 1 / (1 - 0.16 epsilon))."""
    theta, psi, epsilon, xi = x
    V = _rot(psi)
    D = np.diag([1 / (1 + epsilon), 1 / (1 - KERELSKY_DELTA * epsilon)])
    return np.ravel(V.T @ D @ V @ _rot(theta + xi) - _rot(xi) - JacA0) * 1000


def _fit_dtype(dtype):
    dtype = np.dtype(_dt(dtype))
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64')
    return dtype


def _max_nfev(lq_kwargs):
    if lq_kwargs is None:
        return 50
    for key in lq_kwargs:
        if key != 'max_nfev':
            raise NotImplementedError('lq_kwargs[%r]: the device solver takes max_nfev only (its tolerances are fixed at the '
                                      'precision of f64)' % (key,))
    n = lq_kwargs.get('max_nfev', 50)
    if n is None:
        return 400                                   # scipy's default, 100 * the number of parameters
    if int(n) != n or n < 1:
        raise ValueError('lq_kwargs["max_nfev"] must be an integer >= 1')
    return int(n)


def _kerelsky_a0(kvecs, nmperpixel, a_0, reference, sort):
    """A0 with k0s @ A0.T = kvecs / r_k0 for the unit vectors k0s at 0, 60, 120 degrees, and the start of the global fit
    (property_extract.py:748-762): every argument checked."""
    kvecs = np.asarray(kvecs, dtype=np.float64)
    if kvecs.shape != (3, 2):
        raise ValueError('kvecs must have shape (3, 2)')
    if not np.isfinite(kvecs).all():
        raise ValueError('kvecs must be finite')
    if not (np.isfinite(nmperpixel) and nmperpixel > 0 and np.isfinite(a_0) and a_0 > 0):
        raise ValueError('nmperpixel and a_0 must be positive')
    if reference not in (None, 'symmetric'):
        raise ValueError("reference must be None or 'symmetric'")
    if sort not in (-1, 0, 1):
        raise ValueError('sort must be -1, 0 or 1')
    angles = np.arctan2(kvecs[:, 1], kvecs[:, 0])
    r_k0 = nmperpixel / (a_0 * np.sin(np.deg2rad(60.)))
    lkvecs = kvecs / r_k0
    if sort != 0:
        lkvecs = lkvecs[np.argsort(sort * periodic_difference(angles, periodic_average(angles)))]
    k0 = np.deg2rad([0., 60., 120.])
    A0 = np.linalg.lstsq(np.stack([np.cos(k0), np.sin(k0)], axis=1), lkvecs, rcond=None)[0].T
    est = np.array([.01, 0., 0., np.rad2deg(np.arctan2(lkvecs[0, 1], lkvecs[0, 0])) % 360])
    return np.ascontiguousarray(A0), est


def _global_fit(A0, est, max_nfev, debug):
    """the fit of A0 itself, one pixel: starts est and est with psi = 90, the second whenever the first leaves a cost above 1e-20
    (property_extract.py:763-768)"""
    x, cost = _lib.kerelsky_fit(A0, est, max_nfev=max_nfev, retry_cost=1e-20, dtype=np.float64)
    if debug:
        print('Kerelsky global fit: x = %s, cost = %s' % (x, cost))
    return x if np.isfinite(x).all() else np.full(4, np.nan)


def iterate_J_leastsq(JacA0, refest, lq_kwargs=None, dtype=None):
    """The fit of every 2 x 2 matrix of JacA0 (..., 2, 2) from the start refest (property_extract.py:863-883): array (..., 4) of
    (theta, psi, epsilon, xi).  A second start at psi + 90 is tried where the first leaves a cost above 1e-5."""
    return _lib.kerelsky_fit(JacA0, refest, max_nfev=_max_nfev(lq_kwargs), retry_cost=1e-5, dtype=_fit_dtype(dtype))[0]


def Kerelsky_Jac(kvecs, nmperpixel=1., a_0=0.246, reference=None, debug=False, sort=0):
    """(theta, psi, epsilon, xi) of three k-vectors (unit cells per pixel), in degrees (property_extract.py:707-777), by the fit of
    JacA0 with k0s @ JacA0.T = kvecs.  reference='symmetric' adds theta / 2 to xi.  NaN when the fit fails, i.e. when its result
    is not finite."""
    A0, est = _kerelsky_a0(kvecs, nmperpixel, a_0, reference, sort)
    params = _global_fit(A0, est, 400, debug)
    if reference == 'symmetric':
        params[3] = params[3] + params[0] / 2
    return params


def Kerelsky_J(J, kvecs, nmperpixel=1., a_0=0.246, reference=None, debug=False, sort=0, lq_kwargs={'max_nfev': 50}, dtype=None):
    """Per-pixel (theta, psi, epsilon, xi) from the displacement-gradient field J (..., 2, 2) and the three k-vectors
    (property_extract.py:780-860): returns (X (..., 4), refest), X from the fit of A0 + A0 J at every pixel started at the global
    fit refest of A0; or the NaN refest alone when the global fit fails.  As in the reference, `reference` has no effect here.
    A pixel whose J is not finite gives NaN (the reference raises)."""
    max_nfev, dtype = _max_nfev(lq_kwargs), _fit_dtype(dtype)
    J = np.asarray(J)
    if J.ndim < 2 or J.shape[-2:] != (2, 2):
        raise ValueError('J must have shape (..., 2, 2)')
    A0, est = _kerelsky_a0(kvecs, nmperpixel, a_0, reference, sort)
    refest = _global_fit(A0, est, max_nfev, debug)
    if not np.isfinite(refest).all():
        return refest
    X, _ = _lib.kerelsky_fit(J, refest, a0=A0, max_nfev=max_nfev, retry_cost=1e-5, dtype=dtype)
    return X, refest


def Kerelsky_J_dev(J_ptr, npx, kvecs, nmperpixel=1., a_0=0.246, reference=None, debug=False, sort=0, lq_kwargs={'max_nfev': 50},
                   dtype=None, out_ptr=None, cost_ptr=None, device=0, stream=None):
    """Kerelsky_J for a J that is resident on the device (e.g. the output of Plan.phasegradient2J_dev): J_ptr holds npx x 2 x 2
    values of `dtype`, out_ptr receives npx x 4 of them (cost_ptr, optional, npx doubles); asynchronous on `stream`.  Returns
    refest; when the global fit fails refest is NaN and nothing is written."""
    max_nfev, dtype = _max_nfev(lq_kwargs), _fit_dtype(dtype)
    if out_ptr is None:
        raise ValueError('out_ptr is required')
    A0, est = _kerelsky_a0(kvecs, nmperpixel, a_0, reference, sort)
    refest = _global_fit(A0, est, max_nfev, debug)
    if np.isfinite(refest).all():
        _lib.kerelsky_fit_dev(J_ptr, npx, refest, out_ptr, a0=A0, max_nfev=max_nfev, retry_cost=1e-5, cost_ptr=cost_ptr,
                              dtype=dtype, device=device, stream=stream)
    return refest
