"""The per-pixel weighted least squares of a5 / a6 (csrc/gpa_reconstruct.hip through solve2 of csrc/gpa_jacmath.h): k-vector sets
for P = 2 ... 8, seeded weight classes, an independent LAPACK reference, a dtype-faithful NumPy emulation of the kernels' normal
equations, and the derived bound of tests/test_lstsq_host.py and tests/test_gpu_lstsq.py.  A helper, not a test;
tools/make_lstsq_golden.py uses it too.

The reference is the rule of myweighed_lstsq (geometric_phase_analysis.py:97-113), restated, not the kernels' algorithm:
    per pixel   x = np.linalg.lstsq((w * K.T).T, w * b, rcond=None)[0]          in float64
on inputs rounded to the dtype under test first (K = 2 pi kvecs included: the kernels convert it), so that both sides see the
same numbers.  tests/golden/lstsq_*.npz pin the restatement to the reference's own function at every P.

The bound.  M = diag(w) K (P x 2) has singular values smax >= smin, kappa = smax / smin; x minimises ||M x - w b||.  The kernels
solve A x = r with A = M^T M, r = M^T (w b), in the precision T of the data, unit round-off u.  First order in u:

  (1) forming A and r.  A term of a sum is ww k_i k_j or ww k_i b with ww = wn wn, wn = w / wmax.  Per term: 1 rounding in wn
      (the rounding of 1 / wmax is a common factor of all weights and drops out of x), counted twice because wn is squared, 1 for
      the square, 2 for the two products, and at most P - 1 for the P - 1 additions the term passes through: (P + 4) u =: g.
      (A fused multiply-add only removes roundings.)  So  |dA| <= g |M|^T |M|,  |dr| <= g |M|^T |w b|  and, with
      || |M|^T |M| ||_2 <= ||M||_F^2 <= 2 smax^2  and  || |M|^T |w b| || <= sqrt(2) smax ||w b||:
          ||dx|| <= ||A^-1|| (||dr|| + ||dA|| ||x||) <= g kappa^2 (2 ||x|| + sqrt(2) ||w b|| / smax)
                 <= 2 (P + 4) u kappa^2 (||x|| + ||w b|| / smax)
  (2) Cramer's rule.  det = a00 a11 - a01^2: three roundings on terms of size <= tr^2 / 4, and tr^2 / (4 det) =
      (kappa + 1 / kappa)^2 / 4 <= kappa^2, so |d det| / det <= 3 * 2 u kappa^2 / ... <= 6 u kappa^2, which moves x by
      6 u kappa^2 ||x|| per component.  A numerator a11 r0 - a01 r1 has three roundings and the division (1 / det, then the
      product) two more, on terms of size <= ||A|| ||r||, i.e. 5 u sqrt(2) kappa^2 ||w b|| / smax per component.  For the 2-norm
      of the two components, times sqrt(2):
          ||dx|| <= u kappa^2 (6 sqrt(2) ||x|| + 10 ||w b|| / smax) <= 10 u kappa^2 (||x|| + ||w b|| / smax)
  together  C(P) = 2 (P + 4) + 10 = 2 P + 18  roundings (22 at P = 2, 34 at P = 8).
  (3) what a kernel does to b before the solve (wraps, atan2) is an absolute error db of each b_p, given by the caller in units
      of u; it moves w b by at most db u ||w||, so x by  db u kappa ||w|| / smax.
  (4) LAPACK's own float64 error: gelsd is backward stable, 8 (P + 2) u64 kappa (||x|| + ||w b|| / smax) covers it generously.

      ||x_dev - x_lapack|| <= C(P) u kappa^2 (||x|| + ||w b|| / smax) + db u kappa ||w|| / smax + 8 (P + 2) u64 kappa (...)

kappa and smax come from a float64 SVD of M on the host.  The bound is first order: it means something where C u kappa^2 << 1.
Where C u kappa^2 >= 1 it exceeds ||x|| + ||w b|| / smax and a solve that drops the weak direction altogether satisfies it.

Graded coverage.  Asserted by check_coverage() on the helper's own inputs: C u kappa^2 <= 0.1 at every pixel of `equal`, `scaled`
and of `graded` down to the ratio COVERED[dtype].  In f64 that is every graded ratio.  In f32 the derived C(P) allows this down to
r = 1e-2 only (kappa <= 220); at r = 1e-3 kappa is 1300 ... 2600 by construction (one weight 1, the others r U(0.5, 1)) and
u kappa^2 alone is 0.1 ... 0.4, so no constant C >= 1 can meet the condition there.  The bound is asserted at every pixel of
every graded ratio all the same; nothing is left out.

Stability, where the bound says nothing (`beyond`, f32 only): every component finite and
      ||x_dev|| <= 2 max(||x_lapack||, ||x_rank1||),   x_rank1 = K^T (w^2 b) / trace(A)
at every pixel (x_rank1 is the minimum-norm answer along the dominant direction, what solve2's rank-1 branch returns).

Rank-deficient classes (`one_nonzero`, `collinear_pair`): LAPACK returns the minimum-norm solution.  In exact arithmetic that
is r / tr; the kernels' r / tr has P + 5 roundings on r, P + 4 on tr and one division, so ||x_dev - x_lapack|| <=
(2 P + 10) u ||x|| sqrt(2) <= C(P) u ||x|| -- the bound above with kappa = 1.  `all_zero`: exactly 0.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TWO_PI = 2 * np.pi
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
EPS = {k: 2 * v for k, v in U.items()}
DTYPES = [np.float64, np.float32]

# solve2's determinant test, det > TINY tr^2 (csrc/gpa_jacmath.h): 4 eps in both precisions, also the oracle's
TINY = {np.dtype(np.float32): 4 * 2.0 ** -23, np.dtype(np.float64): 4 * 2.0 ** -52}
# the constants before this file existed.  Both lie below the determinant's rounding noise: the f32 one fails the stability
# condition from r = 1e-4 on, and both return answers unrelated to LAPACK's on exactly rank-deficient pixels
TINY_BEFORE = {np.dtype(np.float32): 1e-12, np.dtype(np.float64): 1e-28}
TINY_F32_BEFORE = TINY_BEFORE[np.dtype(np.float32)]

# what each kernel does to a right-hand side before the solve, absolute, in units of u (term (3) of the bound)
DB = {
    'wlstsq': 0.,      # b is used as given
    'jacobian': 0.,    # no wrap without dks
    # wrap_to_pi(x), |x| < 5 pi:  t = x + pi (u |t| <= 19 u), floor exact away from the seams, t - 2 pi m (<= 6.3 u, the f32
    # constant 2 pi is 2.8 u off per turn, two turns), - pi (3.2 u and the constant's 1.4 u): 19 + 6.3 + 5.6 + 4.6 -> 40
    'prediff': 40.,
    # two atan2 of at most 2 ulp(pi) = 8 u each against np.angle of the same rounded lock-ins, the difference (exact or 6.3 u),
    # one wrap by comparisons with the T constant of 2 pi (2.8 u): 16 + 6.3 + 2.8 -> 28
    'reconstruct': 28.,
}

# roundings a kernel adds to every term of a sum before the solve starts (term (1) of the bound counts P + 4)
EXTRA = {
    'wlstsq': 0, 'jacobian': 0, 'prediff': 0,
    # the weight is |z| (mask + 1e-6): x^2, y^2, their sum and the root leave at most 3 u on |z|, the mask factor 1 more, and the
    # weight enters squared: 8
    'reconstruct': 8,
}

SEAM_MARGIN = 1e-3    # every wrapped argument of the f32 cases stays this far from +-pi


def C(P):
    """the count of roundings of the header, 2 P + 18"""
    return 2 * P + 18


# ---- k-vector sets -----------------------------------------------------------------------------------------------------------
def _hex():
    a = np.deg2rad(7.0 + 60.0 * np.arange(3))
    k = 0.1 * np.stack([np.cos(a), np.sin(a)], axis=1)
    second = np.stack([k[0] + k[1], k[1] + k[2], k[2] - k[0]])
    return k, second


def _square():
    a = np.deg2rad(11.0)
    k1 = 0.11 * np.array([np.cos(a), np.sin(a)])
    k2 = 0.11 * np.array([-np.sin(a), np.cos(a)])
    return k1, k2


def _ksets():
    k, second = _hex()
    k1, k2 = _square()
    sq4 = np.stack([k1, k2, k1 + k2, k1 - k2])
    sq7 = np.concatenate([sq4, np.stack([2 * k1, 2 * k2, 2 * (k1 + k2)])])
    return {
        'hex2': k[:2],
        'sq2': np.stack([k1, k2]),
        'hex3': k,
        'sq4': sq4,
        'hex5': np.concatenate([k, second])[:5],
        'hex6': np.concatenate([k, second]),
        'sq7': sq7,
        'sq8': np.concatenate([sq7, (2 * (k1 - k2))[None]]),
    }


KSETS = _ksets()
KSET_NAMES = list(KSETS)
# (index of k, index of 2 k) in the sets that hold collinear pairs
COLLINEAR = {'sq7': [(0, 4), (1, 5), (2, 6)], 'sq8': [(0, 4), (1, 5), (2, 6), (3, 7)]}


def kmat(kset, dtype):
    """K = 2 pi kvecs as the kernels use it: formed in float64 and rounded to the data's precision; returned as float64"""
    return (TWO_PI * KSETS[kset]).astype(dtype).astype(np.float64)


# ---- weight classes -------------------------------------------------------------------------------------------------------------
GRADED = {np.dtype(np.float32): (1e-1, 1e-2, 1e-3), np.dtype(np.float64): (1e-1, 1e-3, 1e-6)}
COVERED = {np.dtype(np.float32): 1e-2, np.dtype(np.float64): 1e-6}     # smallest graded ratio with C u kappa^2 <= 0.1
BEYOND = (1e-4, 1e-5, 1e-6, 1e-7)
SCALES = (1e-30, 1e+30)
BOUND_CLASSES = ('equal', 'graded', 'scaled', 'negative')
DEFICIENT = ('one_nonzero', 'collinear_pair', 'all_zero')


def class_list(kset, dtype, signed=True):
    """[(label, class, ratio)] for a k-vector set and a precision; signed: the entry point takes weights of either sign"""
    dtype = np.dtype(dtype)
    out = [('equal', 'equal', None)]
    out += [('graded_%g' % r, 'graded', r) for r in GRADED[dtype]]
    if dtype == np.float32:
        out += [('beyond_%g' % r, 'beyond', r) for r in BEYOND]
    out += [('one_nonzero', 'one_nonzero', None)]
    if kset in COLLINEAR:
        out += [('collinear_pair', 'collinear_pair', None)]
    out += [('all_zero', 'all_zero', None), ('scaled', 'scaled', None)]
    if signed:
        out += [('negative', 'negative', None)]
    return out


def _seed(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode())


def weights(cls, kset, shape, r=None, scales=SCALES, uniform=False):
    """(P, n0, n1) float64 weights of a class, seeded by (class, set, shape, ratio).  uniform: the peaks that carry weight in
    `one_nonzero` / `collinear_pair` are the same at every pixel (for lock-ins: a peak without amplitude has no phase, so a
    phase difference towards a pixel where it has none would be arbitrary)"""
    P = len(KSETS[kset])
    rng = np.random.default_rng(_seed('w', cls, kset, tuple(shape), r))
    n = shape[0] * shape[1]
    pick = (lambda hi: np.full(n, rng.integers(0, hi))) if uniform else (lambda hi: rng.integers(0, hi, n))
    if cls in ('equal', 'scaled', 'negative'):
        w = rng.uniform(0.5, 1.0, (P, n))
        if cls == 'scaled':
            w = w * np.asarray(scales)[np.arange(n) % len(scales)][None, :]
        if cls == 'negative':
            w = w * rng.choice([-1.0, 1.0], (P, n))
    elif cls in ('graded', 'beyond'):
        w = r * rng.uniform(0.5, 1.0, (P, n))
        w[rng.integers(0, P, n), np.arange(n)] = 1.0
    elif cls == 'one_nonzero':
        w = np.zeros((P, n))
        w[pick(P), np.arange(n)] = rng.uniform(0.5, 1.0, n)
    elif cls == 'collinear_pair':
        pairs = np.asarray(COLLINEAR[kset])[pick(len(COLLINEAR[kset]))]
        w = np.zeros((P, n))
        w[pairs[:, 0], np.arange(n)] = rng.uniform(0.5, 1.0, n)
        w[pairs[:, 1], np.arange(n)] = rng.uniform(0.5, 1.0, n)
    elif cls == 'all_zero':
        w = np.zeros((P, n))
    else:
        raise KeyError(cls)
    return w.reshape((P,) + tuple(shape))


def rhs(kset, shape, tag=0):
    """b = K x_true + 0.05 N(0, 1), |x_true| <= 0.5 per component: (P, n0, n1) float64, inside (-pi + 0.5, pi - 0.5)"""
    rng = np.random.default_rng(_seed('b', kset, tuple(shape), tag))
    K = TWO_PI * KSETS[kset]
    x = rng.uniform(-0.5, 0.5, (2,) + tuple(shape))
    b = np.einsum('pc,cnm->pnm', K, x) + 0.05 * np.clip(rng.standard_normal((len(K),) + tuple(shape)), -5, 5)
    assert np.abs(b).max() < np.pi - 0.5
    return b


def rounded(a, dtype):
    """the float64 values of `a` rounded to dtype"""
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def wrap_to_pi(x):
    """the reference's wrapToPi (mathtools.py:72-75): [-pi, pi), +pi -> -pi"""
    return (np.asarray(x, dtype=np.float64) + np.pi) % TWO_PI - np.pi


# ---- the reference -------------------------------------------------------------------------------------------------------------
def lapack(b, K, w):
    """per pixel np.linalg.lstsq((w * K.T).T, w * b, rcond=None)[0] in float64: b, w (P, ...), K (P, 2) -> (2, ...)"""
    b, w, K = np.asarray(b, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(K, dtype=np.float64)
    P, lead = b.shape[0], b.shape[1:]
    bf, wf = b.reshape(P, -1), w.reshape(P, -1)
    out = np.empty((2, bf.shape[1]))
    for i in range(bf.shape[1]):
        wloc = wf[:, i]
        out[:, i] = np.linalg.lstsq((wloc * K.T).T, wloc * bf[:, i], rcond=None)[0]
    return out.reshape((2,) + lead)


def rank1(b, K, w):
    """K^T (w^2 b) / trace(K^T W^2 K): the minimum-norm answer along the dominant direction; 0 where every weight is 0"""
    b, w, K = np.asarray(b, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(K, dtype=np.float64)
    wmax = np.abs(w).max(axis=0)
    wn = w / np.where(wmax > 0, wmax, 1.0)
    ww = wn * wn
    r = np.einsum('pc,p...->c...', K, ww * b)
    tr = np.einsum('p,p...->...', (K * K).sum(axis=1), ww)
    return np.where(tr > 0, r / np.where(tr > 0, tr, 1.0), 0.0)


def svd_stats(K, w):
    """(smax, smin) of diag(w) K per pixel, float64; the weights are normalised per pixel first (kappa does not change)"""
    w, K = np.asarray(w, dtype=np.float64), np.asarray(K, dtype=np.float64)
    wmax = np.abs(w).max(axis=0)
    wn = w / np.where(wmax > 0, wmax, 1.0)
    M = np.moveaxis(wn, 0, -1)[..., :, None] * K             # (..., P, 2)
    s = np.linalg.svd(M, compute_uv=False)
    return s[..., 0] * wmax, s[..., 1] * wmax


def norm2(x):
    return np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(axis=0))


def bound(x_ref, b, K, w, dtype, db=0.0, deficient=False, extra=0):
    """the per-pixel bound of the header on ||x - x_ref||; deficient: the rank-1 form (kappa = 1 along the one direction);
    extra: further roundings per term of a sum, for kernels that compute their weights (EXTRA), 2 in C for each"""
    P = len(K)
    u = U[np.dtype(dtype)]
    smax, smin = svd_stats(K, w)
    ok = smax > 0
    safe = np.where(ok, smax, 1.0)
    kappa = np.ones_like(smax) if deficient else smax / np.where(smin > 0, smin, np.nan)
    size = norm2(x_ref) + np.where(ok, norm2(np.asarray(w, dtype=np.float64) * b) / safe, 0.0)
    wn = np.where(ok, norm2(w) / safe, 0.0)
    return (C(P) + 2 * extra) * u * kappa ** 2 * size + db * u * kappa * wn + 8 * (P + 2) * U[np.dtype(np.float64)] * kappa * size


def kappa_of(K, w):
    smax, smin = svd_stats(K, w)
    return smax / smin


def ratio(x, x_ref, bnd):
    """max over pixels of ||x - x_ref|| / bound (0 / 0 counts as 0: all_zero pixels must be exact and are checked apart)"""
    d = norm2(np.asarray(x, dtype=np.float64) - x_ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(d == 0, 0.0, d / bnd)
    return float(np.max(q))


def stability_ratio(x, x_ref, x_r1):
    """max over pixels of ||x|| / max(||x_lapack||, ||x_rank1||); the condition is <= 2 with every component finite"""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return float('inf')
    den = np.maximum(norm2(x_ref), norm2(x_r1))
    return float(np.max(norm2(x) / den))


def check_coverage(kset, shape, dtype):
    """the graded-coverage condition on the helper's own inputs; returns the largest C u kappa^2 met"""
    dtype = np.dtype(dtype)
    K = kmat(kset, dtype)
    worst = 0.0
    todo = [('equal', None), ('scaled', None)] + [('graded', r) for r in GRADED[dtype] if r >= COVERED[dtype]]
    for cls, r in todo:
        kap = kappa_of(K, rounded(weights(cls, kset, shape, r, scales=scales_for(dtype)), dtype))
        worst = max(worst, float(C(len(K)) * U[dtype] * (kap ** 2).max()))
    assert worst <= 0.1, (kset, shape, dtype, worst)
    return worst


def scales_for(dtype, squared=False):
    """the factors of `scaled`.  squared: for the entry point that takes lock-ins and forms |z|^2 and (1e-6 |z|)^2 in the data's
    precision on the way to the weight and to wnorm: in f32 those squares must stay normal numbers, which 1e-30 does not allow;
    the normalisation is tested at 1e-12 and 1e+15 there"""
    if squared and np.dtype(dtype) == np.float32:
        return (1e-12, 1e+15)
    return SCALES


# ---- the emulation -----------------------------------------------------------------------------------------------------------
def emulate(b, K, w, dtype, tiny=None):
    """the kernels' normal equations in NumPy with every operation rounded to dtype: per-pixel normalisation by max |w|, sums in
    list order, solve2 with det > tiny tr^2 (default TINY[dtype]), r / tr below it, 0 where tr = 0.  No fused multiply-adds.
    Returns (x (2, ...) in dtype, rank1 mask)"""
    T = np.dtype(dtype).type
    tiny = T(TINY[np.dtype(dtype)] if tiny is None else tiny)
    b, w = np.asarray(b).astype(T), np.asarray(w).astype(T)
    K = np.asarray(K).astype(T)
    wmax = np.abs(w).max(axis=0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ws = np.where(wmax > 0, T(1) / np.where(wmax > 0, wmax, T(1)), T(0)).astype(T)
        a00 = np.zeros(b.shape[1:], T)
        a01, a11, r0, r1 = a00.copy(), a00.copy(), a00.copy(), a00.copy()
        for p in range(len(K)):
            wn = w[p] * ws
            ww = wn * wn
            a00 = a00 + ww * K[p, 0] * K[p, 0]
            a01 = a01 + ww * K[p, 0] * K[p, 1]
            a11 = a11 + ww * K[p, 1] * K[p, 1]
            r0 = r0 + ww * K[p, 0] * b[p]
            r1 = r1 + ww * K[p, 1] * b[p]
        det = a00 * a11 - a01 * a01
        tr = a00 + a11
        full = det > tiny * tr * tr
        inv = T(1) / np.where(full, det, T(1))
        x0 = np.where(full, (a11 * r0 - a01 * r1) * inv, np.where(tr > 0, r0 / np.where(tr > 0, tr, T(1)), T(0)))
        x1 = np.where(full, (a00 * r1 - a01 * r0) * inv, np.where(tr > 0, r1 / np.where(tr > 0, tr, T(1)), T(0)))
    assert x0.dtype == T
    return np.stack([x0, x1]), ~full & (tr > 0)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
FIXTURE_SHAPE = (6, 40)
# label -> (class, ratio): one row of the fixture each
FIXTURE_ROWS = [('equal', None), ('graded', 1e-2), ('graded', 1e-5), ('one_nonzero', None), ('collinear_pair', None), ('all_zero', None)]


def fixture_inputs(kset):
    """(b, K, w) of tests/golden/lstsq_<kset>.npz: one row of FIXTURE_SHAPE per class (collinear_pair: `equal` again on the
    sets without a collinear pair)"""
    shape = FIXTURE_SHAPE
    P = len(KSETS[kset])
    b = rhs(kset, shape, 'fixture')
    w = np.empty((P,) + shape)
    for i, (cls, r) in enumerate(FIXTURE_ROWS):
        if cls == 'collinear_pair' and kset not in COLLINEAR:
            cls = 'equal'
        w[:, i] = weights(cls, kset, (1, shape[1]), r)[:, 0]
    return b, TWO_PI * KSETS[kset], w


def load(kset):
    with np.load(os.path.join(GOLDEN, 'lstsq_%s.npz' % kset)) as z:
        return {k: z[k] for k in z.files}


# ---- inputs of the GPU test, with their references (computed once per process) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_case(kset, label, shape, dtype_name, squared=False):
    """dict(b, w, K, x_ref, x_r1) for one (set, class label, shape, dtype): b and w rounded to the dtype, float64 arrays;
    not to be modified"""
    dtype = np.dtype(dtype_name)
    cls, r = next((c, rr) for lab, c, rr in class_list(kset, np.float32) + class_list(kset, np.float64) if lab == label)
    K = kmat(kset, dtype)
    b = rounded(rhs(kset, shape, label), dtype)
    w = rounded(weights(cls, kset, shape, r, scales=scales_for(dtype, squared)), dtype)
    out = dict(cls=cls, r=r, b=b, w=w, K=K, x_ref=lapack(b, K, w), x_r1=rank1(b, K, w))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def smooth_phase(kset, shape):
    """phases (P, n0, n1) of a smooth displacement: K_p . X(i, j) with X linear plus one wave, plus 0.03 N(0, 1) per sample, so
    that the P differences of a pixel are not consistent with any x.  Neighbouring samples differ by less than 1.2 rad"""
    rng = np.random.default_rng(_seed('phi', kset, tuple(shape)))
    i, j = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing='ij')
    X = np.stack([0.31 * i - 0.22 * j + 0.8 * np.sin((i + 0.5 * j) / 9.0), 0.18 * i + 0.27 * j + 0.6 * np.cos((0.7 * i - j) / 11.0)])
    K = TWO_PI * KSETS[kset]
    return np.einsum('pc,cnm->pnm', K, X) + 0.03 * np.clip(rng.standard_normal((len(K),) + tuple(shape)), -5, 5)


@functools.lru_cache(maxsize=None)
def lockin_case(kset, label, shape, dtype_name):
    """lock-ins z = w exp(i phi) of a class, rounded to the complex type of the dtype, and what the reference makes of them in
    float64: phases np.angle(z), weights |z|, wrapped differences along both axes, the LAPACK answers dx (2, n0, n1 - 1) and
    dy (2, n0 - 1, n1) and the rank-1 answers.  The peaks of the rank-deficient classes are the same at every pixel.  Asserts
    that no difference lies within SEAM_MARGIN of +-pi.  Not to be modified"""
    dtype = np.dtype(dtype_name)
    cdtype = np.complex64 if dtype == np.float32 else np.complex128
    cls, r = next((c, rr) for lab, c, rr in class_list(kset, np.float32) + class_list(kset, np.float64) if lab == label)
    K = kmat(kset, dtype)
    w = weights(cls, kset, shape, r, scales=scales_for(dtype, squared=True), uniform=True)
    z = np.where(w != 0, w * np.exp(1j * smooth_phase(kset, shape)), 0).astype(cdtype)     # (0 times a phasor is a signed zero)
    zz = z.astype(np.complex128)
    ph, amp = np.angle(zz), np.abs(zz)
    bx, by = wrap_to_pi(np.diff(ph, axis=2)), wrap_to_pi(np.diff(ph, axis=1))
    wx, wy = amp[:, :, :-1], amp[:, :-1, :]
    assert max(np.abs(bx * (wx > 0)).max(), np.abs(by * (wy > 0)).max()) < np.pi - SEAM_MARGIN     # wherever a difference counts
    out = dict(cls=cls, r=r, z=z, K=K, amp=amp, bx=bx, by=by, wx=wx, wy=wy, dx=lapack(bx, K, wx), dy=lapack(by, K, wy),
               dx_r1=rank1(bx, K, wx), dy_r1=rank1(by, K, wy))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- measured on the MI355X ---------------------------------------------------------------------------------------------------
# tests/test_gpu_lstsq.py prints one 'CMEAS kernel P class dtype figure' line per check; the table holds, per key, the largest
# figure over shapes, k-vector sets of that P and ratios: error / bound for equal, graded, scaled, negative and the rank-deficient
# classes, ||x|| / max(||x_lapack||, ||x_rank1||) for beyond (the condition is <= 2).
# kernel -> dtype -> class -> {P: figure}; 'reconstruct' is reconstruct_kernel<T, P> through gpa_reconstruct_grad.  The bound holds
# with room to spare everywhere (largest: 0.48), every `beyond` pixel returns the rank-1 answer (1.000), every all_zero pixel 0.
# With the determinant test used before (1e-12 / 1e-28 tr^2) the same run gave: beyond 17.8 ... 21.8 in f32 (the condition is
# <= 2), one_nonzero and collinear_pair 9e5 ... 1.8e7 times the bound in f32 and 7e15 ... 2.8e16 times in f64.
C_MEASURED = {
    'wlstsq': {
        'float32': {
            'equal': {2: 0.067, 3: 0.076, 4: 0.064, 5: 0.037, 6: 0.063, 7: 0.034, 8: 0.046},
            'graded': {2: 0.340, 3: 0.319, 4: 0.285, 5: 0.257, 6: 0.053, 7: 0.232, 8: 0.041},
            'scaled': {2: 0.073, 3: 0.063, 4: 0.059, 5: 0.042, 6: 0.060, 7: 0.045, 8: 0.051},
            'negative': {2: 0.070, 3: 0.068, 4: 0.060, 5: 0.039, 6: 0.048, 7: 0.036, 8: 0.048},
            'beyond': {2: 1.000, 3: 1.000, 4: 1.000, 5: 1.000, 6: 1.000, 7: 1.000, 8: 1.000},
            'one_nonzero': {2: 0.054, 3: 0.044, 4: 0.045, 5: 0.041, 6: 0.038, 7: 0.036, 8: 0.037},
            'collinear_pair': {7: 0.047, 8: 0.040},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
        'float64': {
            'equal': {2: 0.081, 3: 0.075, 4: 0.061, 5: 0.039, 6: 0.053, 7: 0.034, 8: 0.040},
            'graded': {2: 0.022, 3: 0.031, 4: 0.028, 5: 0.046, 6: 0.051, 7: 0.039, 8: 0.040},
            'scaled': {2: 0.086, 3: 0.069, 4: 0.073, 5: 0.043, 6: 0.052, 7: 0.033, 8: 0.034},
            'negative': {2: 0.102, 3: 0.073, 4: 0.059, 5: 0.041, 6: 0.043, 7: 0.040, 8: 0.042},
            'one_nonzero': {2: 0.080, 3: 0.058, 4: 0.057, 5: 0.041, 6: 0.043, 7: 0.040, 8: 0.035},
            'collinear_pair': {7: 0.044, 8: 0.038},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
    },
    'prediff': {
        'float32': {
            'equal': {2: 0.262, 3: 0.251, 4: 0.221, 5: 0.168, 6: 0.208, 7: 0.172, 8: 0.201},
            'graded': {2: 0.352, 3: 0.318, 4: 0.284, 5: 0.273, 6: 0.052, 7: 0.232, 8: 0.078},
            'scaled': {2: 0.286, 3: 0.219, 4: 0.262, 5: 0.165, 6: 0.205, 7: 0.155, 8: 0.203},
            'negative': {2: 0.250, 3: 0.243, 4: 0.212, 5: 0.178, 6: 0.207, 7: 0.164, 8: 0.199},
            'beyond': {2: 1.000, 3: 1.000, 4: 1.000, 5: 1.000, 6: 1.000, 7: 1.000, 8: 1.000},
            'one_nonzero': {2: 0.343, 3: 0.334, 4: 0.328, 5: 0.324, 6: 0.313, 7: 0.304, 8: 0.302},
            'collinear_pair': {7: 0.262, 8: 0.262},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
        'float64': {
            'equal': {2: 0.078, 3: 0.047, 4: 0.040, 5: 0.032, 6: 0.034, 7: 0.027, 8: 0.028},
            'graded': {2: 0.024, 3: 0.037, 4: 0.030, 5: 0.036, 6: 0.052, 7: 0.039, 8: 0.041},
            'scaled': {2: 0.079, 3: 0.048, 4: 0.045, 5: 0.045, 6: 0.043, 7: 0.027, 8: 0.032},
            'negative': {2: 0.062, 3: 0.057, 4: 0.047, 5: 0.032, 6: 0.037, 7: 0.023, 8: 0.031},
            'one_nonzero': {2: 0.074, 3: 0.049, 4: 0.034, 5: 0.036, 6: 0.037, 7: 0.032, 8: 0.030},
            'collinear_pair': {7: 0.032, 8: 0.028},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
    },
    'jacobian': {
        'float32': {
            'equal': {2: 0.096, 3: 0.072, 4: 0.088, 5: 0.050, 6: 0.058, 7: 0.041, 8: 0.063},
            'graded': {2: 0.355, 3: 0.319, 4: 0.284, 5: 0.274, 6: 0.053, 7: 0.232, 8: 0.041},
            'scaled': {2: 0.082, 3: 0.065, 4: 0.064, 5: 0.049, 6: 0.069, 7: 0.056, 8: 0.054},
            'beyond': {2: 1.000, 3: 1.000, 4: 1.000, 5: 1.000, 6: 1.000, 7: 1.000, 8: 1.000},
            'one_nonzero': {2: 0.079, 3: 0.067, 4: 0.061, 5: 0.063, 6: 0.060, 7: 0.058, 8: 0.051},
            'collinear_pair': {7: 0.062, 8: 0.056},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
        'float64': {
            'equal': {2: 0.094, 3: 0.074, 4: 0.062, 5: 0.051, 6: 0.051, 7: 0.037, 8: 0.042},
            'graded': {2: 0.023, 3: 0.032, 4: 0.030, 5: 0.046, 6: 0.046, 7: 0.040, 8: 0.040},
            'scaled': {2: 0.090, 3: 0.081, 4: 0.066, 5: 0.046, 6: 0.059, 7: 0.039, 8: 0.039},
            'one_nonzero': {2: 0.079, 3: 0.065, 4: 0.052, 5: 0.054, 6: 0.045, 7: 0.040, 8: 0.034},
            'collinear_pair': {7: 0.039, 8: 0.044},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
    },
    'reconstruct': {
        'float32': {
            'equal': {2: 0.224, 3: 0.144, 4: 0.121, 5: 0.073, 6: 0.086, 7: 0.073, 8: 0.063},
            'graded': {2: 0.205, 3: 0.192, 4: 0.198, 5: 0.178, 6: 0.034, 7: 0.160, 8: 0.028},
            'scaled': {2: 0.157, 3: 0.118, 4: 0.100, 5: 0.079, 6: 0.064, 7: 0.045, 8: 0.056},
            'beyond': {2: 1.000, 3: 1.000, 4: 1.000, 5: 1.000, 6: 1.000, 7: 1.000, 8: 1.000},
            'one_nonzero': {2: 0.224, 3: 0.258, 4: 0.291, 5: 0.287, 6: 0.385, 7: 0.198, 8: 0.227},
            'collinear_pair': {7: 0.123, 8: 0.116},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
        'float64': {
            'equal': {2: 0.242, 3: 0.150, 4: 0.115, 5: 0.080, 6: 0.094, 7: 0.055, 8: 0.058},
            'graded': {2: 0.014, 3: 0.022, 4: 0.022, 5: 0.030, 6: 0.036, 7: 0.029, 8: 0.028},
            'scaled': {2: 0.209, 3: 0.150, 4: 0.093, 5: 0.063, 6: 0.071, 7: 0.036, 8: 0.062},
            'one_nonzero': {2: 0.389, 3: 0.484, 4: 0.410, 5: 0.379, 6: 0.407, 7: 0.206, 8: 0.279},
            'collinear_pair': {7: 0.113, 8: 0.112},
            'all_zero': {2: 0.000, 3: 0.000, 4: 0.000, 5: 0.000, 6: 0.000, 7: 0.000, 8: 0.000},
        },
    },
}
