"""Unwrapping a stack of phase maps: one stack call against the loop of single calls a user writes without it.

Resident on one GPU (phase maps, weights and results stay in device buffers), timed with HIP events on the plan's stream
(Plan.timer_start / timer_stop: the second event is synchronised on), profiling off.  Legs per shape and precision:
    loop    B x unwrap_dev(psi[b], weight[b], phi[b])          -- the single path, untouched by the stack call: each call waits
                                                                 for its solve (its iteration count is the call's result)
    stack   unwrap_batch_dev(psi, B, weight, B, phi)            -- the B solves as one set of launches per chunk, one wait
B maps with a weight each, kmax iterations at most.  Both legs are warmed up, then alternate leg by leg within each repetition;
median, quartiles and extremes per leg; `spread` is max - min of the loop over the repetitions, the yardstick the difference of
the medians is held against.  Before the timing the stack's phi and counts are compared with the loop's at the timed size (bit
for bit under NO_LAT=1, where both run the same kernels; to rounding with the default kernels, which are the ones timed).
After the timing one profiled run of each leg gives the per-kernel times (gpa_set_profiling; loop: one solve).
A library without the stack call (GPA_HIP_LIB=<its libgpa_hip.so>) runs the loop leg alone.

    python tools/unwrap_stack_timing.py [--sizes 256,512,1024,2048] [--dtypes f32,f64] [--maps 12] [--kmax 25] [--reps 20]
                                        [--label TEXT] [--out profiles/unwrap_stack_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STACK_SYMBOLS = ('gpa_unwrap_batch_dev', 'gpa_unwrap_prediff_batch_dev', 'gpa_unwrap_batch_finish', 'gpa_unwrap_batch',
                 'gpa_unwrap_prediff_batch', 'gpa_unwrap_batch_problem_bytes')


def stats(ts):
    a = np.sort(np.asarray(ts))
    q = lambda f: float(a[int(round(f * (len(a) - 1)))])   # noqa: E731
    return {'n': len(a), 'median_ms': q(0.5), 'q25_ms': q(0.25), 'q75_ms': q(0.75), 'min_ms': float(a[0]), 'max_ms': float(a[-1])}


def fmt(name, s):
    return '  %-6s n=%-3d median %9.3f ms   quartiles %9.3f .. %9.3f   min %9.3f  max %9.3f' % (
        name, s['n'], s['median_ms'], s['q25_ms'], s['q75_ms'], s['min_ms'], s['max_ms'])


def make_maps(B, n, seed=11):
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    rng = np.random.default_rng(seed)
    psi = np.empty((B, n, n))
    for i in range(B):
        a, b = rng.uniform(-0.4, 0.4, 2)
        ph = a * x + b * y + 1.5 * np.sin(x / 9 + y / 13) + 0.05 * rng.standard_normal((n, n))
        psi[i] = (ph + np.pi) % (2 * np.pi) - np.pi
    return psi, 0.3 + rng.random((B, n, n))


def profile_lines(title, prof):
    total = sum(ms for _, ms in prof.values())
    out = ['  per kernel, %s (%.3f ms in kernels):' % (title, total)]
    for name, (calls, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
        out.append('    %-22s %4d launches %9.3f ms' % (name, calls, ms))
    return out


def run_case(_lib, B, n, dt, kmax, reps, warmup, have_stack):
    shape, npx, item = (n, n), n * n, np.dtype(dt).itemsize
    psi, W = make_maps(B, n)
    plan = _lib.Plan(shape, 1, dt, device=0)
    d = {k: _lib.DeviceBuffer(B * npx * item) for k in ('psi', 'w', 'phi', 'ref')}
    d['psi'].upload(psi.astype(dt))
    d['w'].upload(W.astype(dt))

    def loop(out='phi'):
        return [plan.unwrap_dev(d['psi'].ptr + b * npx * item, d['w'].ptr + b * npx * item, d[out].ptr + b * npx * item, kmax=kmax)
                for b in range(B)]

    def stack():
        return plan.unwrap_batch_dev(d['psi'].ptr, B, d['w'].ptr, B, d['phi'].ptr, kmax=kmax)

    legs = [('loop', loop)]
    lines = ['%d maps of %d^2 %s, a weight each, kmax = %d' % (B, n, np.dtype(dt).name, kmax)]
    if have_stack:
        legs.append(('stack', stack))
        for no_lat in ('1', None):
            _lib.set_option('NO_LAT', no_lat)
            it_l = loop('ref')
            it_s = stack()
            ref, got = d['ref'].download((B,) + shape, dt), d['phi'].download((B,) + shape, dt)
            lines.append('  %-28s stack == loop bit for bit: %-5s  max |diff| / max |phi| %.2e  counts equal: %s  (counts %s)' % (
                'NO_LAT=1 (same kernels):' if no_lat else 'default kernels (timed):', np.array_equal(ref, got),
                float(np.abs(ref - got).max() / np.abs(ref).max()), list(it_l) == list(it_s), ' '.join(str(int(v)) for v in it_s)))
        lines.append('  chunk: %d problems per set of launches' % min(B, max(1, (2 << 30) // plan.unwrap_batch_problem_bytes(kmax))))
    for _ in range(warmup):
        for _, f in legs:
            f()
    plan.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, f in legs:
            plan.timer_start()
            f()
            times[name].append(plan.timer_stop())
    res = {name: stats(ts) for name, ts in times.items()}
    lines += [fmt(name, res[name]) for name, _ in legs]
    if have_stack:
        lp, st = res['loop'], res['stack']
        spread = lp['max_ms'] - lp['min_ms']
        gain = lp['median_ms'] - st['median_ms']
        lines.append('  median loop / median stack = %.2f   loop - stack = %+.3f ms   spread of the loop (max - min) = %.3f ms   -> %s' % (
            lp['median_ms'] / st['median_ms'], gain, spread,
            'stack faster by more than the spread' if gain > spread else
            ('stack slower by more than the spread' if -gain > spread else 'within the spread')))
    plan.set_profiling(True)
    plan.unwrap_dev(d['psi'].ptr, d['w'].ptr, d['ref'].ptr, kmax=kmax)
    lines += profile_lines('ONE single solve (map 0)', plan.last_kernel_profile())
    if have_stack:
        stack()
        lines += profile_lines('the stack call', plan.last_kernel_profile())
    plan.set_profiling(False)
    plan.close()
    for b in d.values():
        b.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256,512,1024,2048')
    ap.add_argument('--dtypes', default='f32,f64')
    ap.add_argument('--maps', type=int, default=12)
    ap.add_argument('--kmax', type=int, default=25)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--label', default='', help='what to call the library in the report')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unwrap_stack_timing.txt'))
    a = ap.parse_args()
    from pygpa_amd import _lib
    import ctypes
    have_stack = hasattr(ctypes.CDLL(_lib.LIB_PATH), STACK_SYMBOLS[0])
    if not have_stack:          # a library from before the stack call: bind what it has
        for name in STACK_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    lines = ['library: %s%s' % (a.label or _lib.LIB_PATH, '' if have_stack else '   (no stack call: loop leg only)')]
    for dt in a.dtypes.split(','):
        for n in a.sizes.split(','):
            lines += run_case(_lib, a.maps, int(n), {'f32': np.float32, 'f64': np.float64}[dt], a.kmax, a.reps, a.warmup, have_stack)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
