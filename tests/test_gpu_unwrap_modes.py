"""The kernels of the weighted unwrap, route by route, held to a rounding-level bound mode by mode (tests/unwrap_modes.py has
the reference, the yardstick and the measure; the planted faults it catches: tests/test_unwrap_modes_host.py).

A case is a shape, a dtype, options, an entry point and the route it exists to reach.  The host half gives every case's
line to tests/host/unwrap_route_table.cpp and asserts the printed route, so a case that stops reaching its kernel after a
threshold moves fails without a GPU instead of quietly testing something else.  On the GPU the kernel names of
gpa_last_kernel_profile are asserted where they tell kernels apart (colsolve_tri / colsolve_half / colstream_* / pqdct /
rowidct_pq / g_*).

Three checks per case:
  U    unwrap_prediff(diff(phi0), weight=None, kmax=1, axes_compat=False): with the true eigenvalues one unweighted iteration
       is an exact Poisson solve -- one application each of set-up, forward row transform, column solve, inverse row
       transform, stencil dot product and flush -- and phi is phi0 minus its mean.  The sharp check for transforms and tables.
  W2, W3  weighted, kmax 2 and 3: the stencil, the edge weights, R -= alpha DCT(q), the beta recurrence and the second visit of
       every buffer.  Iteration counts equal kmax on both sides.
The asserted quantity is spectral_residual(GPU) / spectral_residual(emulate), both against the reference one precision up on
the same input: tests/tolerances.py UNWRAP_MODES holds, per case and check, the emulation's value, the ratio measured on an
MI355X and the asserted ratio (2 x measured), none above UNWRAP_MODES_CAP = 16 -- where every planted fault still reads.
The free mean, which the measure leaves out, is held to the same bound on its own.

Shapes: the smallest that reach each route ON THE DEVICE.  The power-of-two kernels take axes of 64 .. 16384 points
(unwrap_pow2_shape); 4 x 512, 1024 x 16, 16 x 2048, 32 x 4096, 32 x 8192 ... are generic shapes and run the mixed-radix
kernels -- they are cases here under that route -- so the short axis of every power-of-two case is 64, and the f32
one-row-per-workgroup half-length kernels, which 64 rows already hand to the persistent ones, are reached with NO_ROWPERS.
f64 results are judged in long double: 64 x 8192, 64 x 16384 and their transposes (2^19, 2^20 pixels) are the largest."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import tolerances as TOL
import unwrap_modes as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {'f32': np.float32, 'f64': np.float64}
CHECKS = ('U', 'W2', 'W3')
STACK = 5            # maps of the stack cases: more than 2 problems per launch take the lean kernels


class Case:
    def __init__(self, dtype, shape, route, opts=None, entry='prediff', compat=False, checks=CHECKS, workers=1, tag='',
                 declined=None):
        """declined: the column solve the device runs where the builder of the route's table declines the shape (the host tool
        takes every table as built; the route falls back as unwrap_route() says it does without the table)"""
        self.dtype, self.shape, self.route, self.opts = dtype, tuple(shape), route, dict(opts or {})
        self.entry, self.compat, self.checks, self.workers, self.declined = entry, compat, tuple(checks), workers, declined
        parts = [dtype, '%dx%d' % self.shape] + ['%s=%s' % kv for kv in sorted(self.opts.items())]
        parts += [entry] if entry != 'prediff' else []
        parts += ['compat'] if compat else []
        self.id = '-'.join(parts + ([tag] if tag else []))

    @property
    def route_line(self):
        """the case as tests/host/unwrap_route_table.cpp reads it (None: the plain scheme reads no route)"""
        if 'NO_MR' in self.opts:
            return None
        toks = [self.dtype, str(self.shape[0]), str(self.shape[1])]
        if self.entry == 'stack':
            toks.append('nprob=%d' % STACK)
        for k, v in sorted(self.opts.items()):
            if k in ('NO_LAT', 'NO_ROWPERS'):
                toks.append(k)
            elif k == 'COLSOLVE':
                toks.append('COLSOLVE=%s' % v)
            else:
                assert k == 'COLSTREAM_CHUNK', k      # (a table-time option: no part of the route)
        return ' '.join(toks)

    def kernels(self, kmax):
        """(names the profile must hold, names it must not) for this route"""
        if self.route is None:
            return ('g_rowdct_kernel', 'g_colsolve_kernel', 'g_rowidct_kernel'), ('rowdct_fused_kernel', 'colsolve_kernel')
        fwd, inv, cols, rowpq, fuse_pq = self.route[:5]
        cols = self.declined or cols
        colk = {'tri': ('colsolve_tri_kernel',), 'colhalf': ('colsolve_half_kernel',), 'dct': ('colsolve_kernel',), 'mr': ('colsolve_kernel',),
                'stream': ('colstream_agg_kernel', 'colstream_scan_kernel', 'colstream_apply_kernel')}
        want = ('rowdct_fused_kernel', 'phi_flush_kernel') + colk[cols]
        want += ('rowidct_pq_kernel',) if rowpq else ('rowidct_p_kernel', 'pq_kernel')
        want += ('pqdct_kernel',) if fuse_pq and kmax > 1 else ()
        every = set(sum(colk.values(), ())) | {'rowidct_pq_kernel', 'pqdct_kernel', 'g_rowdct_kernel', 'g_colsolve_kernel', 'g_rowidct_kernel'}
        return want, tuple(sorted(every - set(want)))


def _both(shape, r32, r64=None, **kw):
    return [Case('f32', shape, r32, **kw), Case('f64', shape, r64 if r64 is not None else r32, **kw)]


# route: (fwd, inv, cols, rowpq, fuse_pq, lat_rows, lat_cols, lat_pq) as the host tool prints it; inv '-': rowpq, no inverse row
# kernel is launched.  Written out here per case, not computed.
P, H, HP, PERS, MR = 'packed', 'half', 'halfpers', 'pers', 'mr'
CASES = []
# rowpq with the latency-tuned kernels; dct columns (f32) or tri (f64, square) -- 64 rows / columns beside 512 / 1024 points
CASES += _both((64, 64), (P, '-', 'dct', 1, 0, 1, 1, 1), (P, '-', 'tri', 1, 0, 1, 1, 1))
CASES += _both((64, 512), (P, '-', 'dct', 1, 0, 1, 1, 1))
CASES += _both((1024, 64), (P, '-', 'dct', 1, 0, 1, 1, 1))
# the lean forms of the same: NO_LAT, and more than two problems per launch
CASES += _both((64, 64), (P, P, 'dct', 0, 0, 0, 0, 0), (P, P, 'tri', 0, 0, 0, 0, 0), opts={'NO_LAT': 1})
CASES += _both((64, 64), (P, P, 'dct', 0, 0, 0, 0, 0), (P, P, 'tri', 0, 0, 0, 0, 0), entry='stack')
# rowidct_p + pq, latency-tuned, rows of 1024 points; lean packed rows of 2048 points
CASES += _both((64, 1024), (P, P, 'dct', 0, 0, 1, 1, 1))
CASES += _both((64, 2048), (P, P, 'dct', 0, 0, 0, 1, 1))
# rows of 4096 points: f32 persistent against packed; f64 forward half-length, inverse packed
CASES += [Case('f32', (64, 4096), (P, PERS, 'dct', 0, 0, 0, 1, 1)),
          Case('f32', (64, 4096), (P, P, 'dct', 0, 0, 0, 1, 1), opts={'NO_ROWPERS': 1}),
          Case('f64', (64, 4096), (H, P, 'dct', 0, 0, 0, 1, 1))]
# rows of 8192 and 16384 points: half-length kernels, one row per workgroup (f64; f32 with NO_ROWPERS) and persistent (f32)
for n1 in (8192, 16384):
    CASES += [Case('f32', (64, n1), (HP, HP, 'dct', 0, 0, 0, 1, 1)),
              Case('f32', (64, n1), (H, H, 'dct', 0, 0, 0, 1, 1), opts={'NO_ROWPERS': 1}),
              Case('f64', (64, n1), (H, H, 'dct', 0, 0, 0, 1, 1))]
# long dct columns; the half-length column kernel (f64, 16384 points)
CASES += [Case('f32', (8192, 64), (P, '-', 'dct', 1, 0, 1, 0, 1)), Case('f32', (16384, 64), (P, '-', 'dct', 1, 0, 1, 0, 1)),
          Case('f64', (8192, 64), (P, '-', 'dct', 1, 0, 1, 0, 1)), Case('f64', (16384, 64), (P, '-', 'colhalf', 1, 0, 1, 0, 1))]
# tri columns at both rows-per-thread settings (n0 <= 640: half as many rows per thread); the dct kernel on an f64 square
CASES += [Case('f32', (64, 64), (P, '-', 'tri', 1, 0, 1, 1, 1), opts={'COLSOLVE': 'tri'}),
          Case('f32', (1024, 1024), (P, P, 'tri', 0, 0, 1, 1, 1), opts={'COLSOLVE': 'tri'}),
          Case('f64', (512, 512), (P, '-', 'tri', 1, 0, 1, 1, 1)),
          Case('f64', (1024, 1024), (P, P, 'tri', 0, 0, 1, 1, 1)),
          Case('f64', (256, 256), (P, '-', 'dct', 1, 0, 1, 1, 1), opts={'COLSOLVE': 'fft'})]
# the streamed column solve: forced at 256^2, default chunk height and 32-row chunks; by default with fuse_pq at 2048^2
CASES += _both((256, 256), (P, '-', 'stream', 1, 0, 1, 1, 1), opts={'COLSOLVE': 'stream'})
CASES += _both((256, 256), (P, '-', 'stream', 1, 0, 1, 1, 1), opts={'COLSOLVE': 'stream', 'COLSTREAM_CHUNK': 32})
CASES += [Case('f32', (2048, 2048), (P, P, 'stream', 0, 1, 0, 0, 1), checks=('U', 'W2'), workers=16)]
# mixed radix: mr columns, tri on a square, the one-pixel instantiations (rows that are no whole 4-pixel vectors), mr columns
# forced on a square, the streamed solve on ragged chunks
CASES += _both((60, 36), (MR, MR, 'mr', 0, 0, 1, 1, 1))
CASES += _both((36, 36), (MR, MR, 'tri', 0, 0, 1, 1, 1))
CASES += _both((63, 65), (MR, MR, 'mr', 0, 0, 1, 1, 1))
# (f32 250^2: build_tritab declines rows that are no whole 16-byte vectors, 250 % 4 != 0 -- colsolve_kernel runs -- so the f32
#  case is the mixed-radix column kernel on a square, the f64 case the recursion on ragged chunks)
CASES += [Case('f32', (250, 250), (MR, MR, 'tri', 0, 0, 1, 1, 1), declined='mr'), Case('f64', (250, 250), (MR, MR, 'tri', 0, 0, 1, 1, 1))]
CASES += _both((36, 36), (MR, MR, 'mr', 0, 0, 1, 1, 1), opts={'COLSOLVE': 'fft'})
CASES += _both((360, 360), (MR, MR, 'stream', 0, 0, 1, 1, 1), opts={'COLSOLVE': 'stream'})
# chirp-z (sides with a prime factor above 13) on the mixed-radix engine
CASES += _both((68, 68), (MR, MR, 'tri', 0, 0, 1, 1, 1))
CASES += _both((97, 101), (MR, MR, 'mr', 0, 0, 1, 1, 1))
# the plain scheme (g_* kernels)
CASES += _both((63, 65), None, opts={'NO_MR': 1})
# power-of-two axes under 64 points: generic shapes, the mixed-radix kernels on short and on long axes
for shape in ((4, 4), (4, 512), (1024, 16), (16, 1024), (16, 2048), (32, 4096)):
    CASES += _both(shape, (MR, MR, 'tri' if shape[0] == shape[1] else 'mr', 0, 0, 1, 1, 1))
CASES += [Case('f32', (32, 8192), (MR, MR, 'mr', 0, 0, 0, 1, 1)), Case('f32', (8192, 32), (MR, MR, 'mr', 0, 0, 1, 0, 1))]
# through unwrap(psi): the set-up kernel's own differences; and the reference's swapped-axis table (aspect below 1.75)
CASES += [Case('f32', (64, 1024), (P, P, 'dct', 0, 0, 1, 1, 1), entry='psi'), Case('f64', (63, 65), (MR, MR, 'mr', 0, 0, 1, 1, 1), entry='psi')]
CASES += _both((60, 36), (MR, MR, 'mr', 0, 0, 1, 1, 1), compat=True)
BY_ID = {c.id: c for c in CASES}

# shapes with a 16384-point axis (f32) or an 8192- / 16384-point axis (f64) beside an axis under 64 points: generic shapes past
# the mixed-radix engine's length -- no kernels, so no case
NO_KERNELS = [('f32', (32, 16384)), ('f32', (16384, 32)), ('f64', (16, 8192)), ('f64', (16, 16384)), ('f64', (8192, 16)),
              ('f64', (16384, 16))]


# ---------------------------------------------------------------------------------------------------------------------
# host half
# ---------------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique():
    assert len(BY_ID) == len(CASES)


def test_every_case_reaches_its_route(tmp_path):
    """unwrap_route() for every case's line, against the route written beside the case"""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'unwrap_route_table')
    src = os.path.join(ROOT, 'tests', 'host', 'unwrap_route_table.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', exe], check=True)
    cases = [c for c in CASES if c.route_line is not None]
    out = subprocess.run([exe], input=''.join(c.route_line + '\n' for c in cases), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.strip().split('\n')
    assert len(lines) == len(cases)
    bad = []
    for c, line in zip(cases, lines):
        got = line.split()
        got = tuple(got[:3]) + tuple(int(v) for v in got[3:])
        want = c.route
        if c.route[0] == MR:          # (the mixed-radix kernels have no latency-tuned forms: lat_rows / lat_cols are not read)
            got, want = got[:5] + got[7:], want[:5] + want[7:]
        if got != want:
            bad.append((c.id, c.route_line, c.route, got))
    assert not bad, bad


def test_every_case_has_its_bound():
    """tests/tolerances.py UNWRAP_MODES: an entry (emulation, measured ratio, asserted ratio) per case and check, asserted =
    2 x measured, none above the cap"""
    assert set(TOL.UNWRAP_MODES) == set(BY_ID)
    for c in CASES:
        assert set(TOL.UNWRAP_MODES[c.id]) == set(c.checks), c.id
        for check, (emul, measured, asserted) in TOL.UNWRAP_MODES[c.id].items():
            assert emul > 0 and measured > 0
            assert asserted <= TOL.UNWRAP_MODES_CAP, (c.id, check, asserted)
            assert 2 * measured <= asserted <= 2.02 * measured, (c.id, check)


# ---------------------------------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _inputs(shape, seed):
    return um.make_inputs(shape, seed)


def _seed(case, b=0):
    return 1000 * b + case.shape[0] + 3 * case.shape[1]


def gpu_solve(case, check, set_option):
    """the case's check on the device: [(phi0, weight, phi, iterations)] per map (one, or STACK of them) and the kernel profile"""
    from pygpa_amd import _lib
    real = DTYPES[case.dtype]
    for k, v in case.opts.items():
        set_option(k, str(v))
    nb = STACK if case.entry == 'stack' else 1
    ins = [_inputs(case.shape, _seed(case, b)) for b in range(nb)]
    compat = case.compat and check != 'U'
    plan = _lib.Plan(case.shape, 1, real)
    try:
        plan.set_profiling(True)
        args = [um.check_args(phi0, w, check) for phi0, w in ins]
        kmax = args[0][3]
        if case.entry == 'stack':
            ws = None if args[0][2] is None else np.stack([a[2] for a in args])
            phis, its = plan.unwrap_prediff_stack(np.stack([a[0] for a in args]), np.stack([a[1] for a in args]), ws, kmax=kmax,
                                                  axes_compat=compat)
        elif case.entry == 'psi':
            phi, it = plan.unwrap(ins[0][0], args[0][2], kmax=kmax, axes_compat=compat)
            phis, its = [phi], [it]
        else:
            phi, it = plan.unwrap_prediff(args[0][0], args[0][1], args[0][2], kmax=kmax, axes_compat=compat)
            phis, its = [phi], [it]
        prof = plan.last_kernel_profile()
    finally:
        plan.close()
    return [(ins[b][0], ins[b][1], np.array(phis[b]), int(its[b])) for b in range(nb)], prof


def measure(case, check, set_option):
    """{'emul', 'gpu', 'ratio', 'mean', 'iters', 'profile'}: the spectral residual of the emulation and of the device against the
    reference one precision up (the worst map of a stack), and the device's free-mean offset"""
    real = DTYPES[case.dtype]
    hi = um.hi_real(real)
    compat = case.compat and check != 'U'
    maps, prof = gpu_solve(case, check, set_option)
    eig = um.eig_table(case.shape, compat, hi)
    out = dict(emul=0.0, gpu=0.0, mean=0.0, iters=[], profile=sorted(prof))
    for phi0, w, phi, it in maps:
        dx, dy, ww, kmax = um.check_args(phi0, w, check)
        ref, k_ref, r0 = um.reference_pcg(dx, dy, ww, kmax, compat, hi, workers=case.workers)
        emu, k_emu, _ = um.emulate(dx, dy, ww, kmax, compat, real, workers=case.workers)
        assert phi.dtype == real and np.isfinite(phi).all()
        out['emul'] = max(out['emul'], um.spectral_residual(emu, ref, r0, eig, workers=case.workers))
        out['gpu'] = max(out['gpu'], um.spectral_residual(phi, ref, r0, eig, workers=case.workers))
        out['mean'] = max(out['mean'], um.mean_offset(phi, ref))
        out['iters'].append((it, k_emu, k_ref, kmax))
    out['ratio'] = out['gpu'] / out['emul']
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case,check', [(c, ch) for c in CASES for ch in c.checks], ids=lambda v: v if isinstance(v, str) else v.id)
def test_unwrap_mode_by_mode(case, check, gpa_option):
    """(These cases found the packed-pair column solve at up to 60000 floors in f64 -- f64-8192x64 U -- before dct_split_mul and
    the mirror-exact w tables; the comment above UNWRAP_MODES in tests/tolerances.py has the figures.  Now 0.2 .. 5.9.)"""
    m = measure(case, check, gpa_option)
    emul_rec, measured, asserted = TOL.UNWRAP_MODES[case.id][check]
    print('unwrap modes %s %s: emulation %.3e (recorded %.3e) device %.3e ratio %.3f (measured %.3f, asserted %.3f) mean %.2e iters %s'
          % (case.id, check, m['emul'], emul_rec, m['gpu'], m['ratio'], measured, asserted, m['mean'], m['iters']))
    for it, k_emu, k_ref, kmax in m['iters']:
        assert it == k_emu == k_ref == kmax, m['iters']
    want, absent = case.kernels(m['iters'][0][3])
    if case.entry == 'stack':     # (a stack call records no kernel profile: its route is held on the CPU alone)
        assert m['profile'] == []
        want = absent = ()
    for k in want:
        assert k in m['profile'], (k, m['profile'])
    for k in absent:
        assert k not in m['profile'], (k, m['profile'])
    assert asserted <= TOL.UNWRAP_MODES_CAP
    assert m['ratio'] <= asserted, (case.id, check, m['ratio'], asserted)
    assert m['mean'] <= asserted * m['emul'], (case.id, check, m['mean'], asserted * m['emul'])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,shape', NO_KERNELS, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_short_axis_beside_a_long_one_has_no_kernels(dtype, shape):
    from pygpa_amd import _lib
    phi0, _ = um.make_inputs(shape, 1)
    dx, dy = um.diffs(phi0)
    plan = _lib.Plan(shape, 1, DTYPES[dtype])
    try:
        with pytest.raises(_lib.GPAError, match='no kernels for this shape'):
            plan.unwrap_prediff(dx, dy, None, kmax=1, axes_compat=False)
    finally:
        plan.close()
