#!/usr/bin/env python
"""Timing of the field / phases -> Jacobian kernels on one GPU: resident gpa_field_jacobian_dev (u2J) and gpa_phases_jacobian_dev
(phases2J, P = 3) at 4096^2 and 1024^2, in f32 and f64, writing J only, the properties only, and both.

    python tools/jac_timing.py [--sizes 4096 1024] [--reps 7] [--no-counters] [--out profiles/jac_timing.txt]

Per case: ms of one call (HIP events on a plan's stream through gpa_timer_start / stop, device pointers, no copies; one warm-up
call, then the median of --reps), the byte model -- every input plane read once, every output element written once -- the time
that takes at the stream rate of 6300 GB/s, and the share of that rate the call reaches.  Then, from a counter run of its own
(this script started again under `rocprofv3 --pmc`, a pass for FETCH_SIZE and one for WRITE_SIZE, one launch per case of the
largest size, no tracing beside the counters), the bytes the L2 fetched and wrote per launch.  FETCH_SIZE is printed as the counter gives it and
doubled: on gfx950 it tallies the 128-byte requests of 16-byte-per-lane streaming loads at 64 bytes.  There is no pass mark, and
nothing on the parent commit to compare with.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

STREAM_GBS = 6300.0
DTYPES = {'f32': np.float32, 'f64': np.float64}
MODES = {'J': (True, False), 'props': (False, True), 'J+props': (True, True)}
NM = 3.7
KVECS = 0.11 * np.stack([np.cos(np.deg2rad([7., 67., 127.])), np.sin(np.deg2rad([7., 67., 127.]))], axis=1)


def inputs(n, dt, seed=3):
    """a smooth displacement field (2, n, n) of a few pixels and the wrapped GPA phases and weights (3, n, n) it gives"""
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing='ij')
    u = np.stack([0.4 * x - 0.3 * y + 2 * np.sin(2 * np.pi * (x + 0.6 * y) / 41.), 0.35 * x + 0.5 * y + 1.5 * np.cos(2 * np.pi * x / 37.)])
    phases = np.angle(np.exp(2j * np.pi * np.einsum('pc,cnm->pnm', KVECS, u)))
    weights = np.stack([0.6 + 0.35 * np.sin(0.021 * x + 0.013 * y + p) for p in range(3)])
    return (0.01 * u).astype(dt), phases.astype(dt), weights.astype(dt)


def cases(sizes, dtypes):
    for n in sizes:
        for name in dtypes:
            for kind in ('u2J', 'phases2J'):
                for mode in MODES:
                    yield n, name, kind, mode


def model_bytes(n, item, kind, mode):
    want_J, want_props = MODES[mode]
    return n * n * item * ((2 if kind == 'u2J' else 6) + 4 * want_J + 4 * want_props)


def run_all(sizes, dtypes, reps):
    """{case: [ms, ...]}: `reps` timed calls of every case after one warm-up (reps = 0: the warm-up alone, for the counter run)"""
    from pygpa_amd import _lib
    import pygpa_amd.property_extract as pe
    out = {}
    plan = _lib.Plan((64, 64), 1, np.float64)      # for its stream and timer only
    try:
        for n in sizes:
            for name in dtypes:
                dt = DTYPES[name]
                item = np.dtype(dt).itemsize
                u, ph, w = inputs(n, dt)
                bufs = {k: _lib.DeviceBuffer(v.nbytes) for k, v in (('u', u), ('ph', ph), ('w', w))}
                bufs['J'], bufs['p'] = _lib.DeviceBuffer(4 * n * n * item), _lib.DeviceBuffer(4 * n * n * item)
                try:
                    for k, v in (('u', u), ('ph', ph), ('w', w)):
                        bufs[k].upload(v)
                    for kind in ('u2J', 'phases2J'):
                        for mode, (want_J, want_props) in MODES.items():
                            kw = dict(J_ptr=bufs['J'].ptr if want_J else None, props_ptr=bufs['p'].ptr if want_props else None,
                                      stream=plan.stream(), dtype=dt)

                            def run():
                                if kind == 'u2J':
                                    pe.u2J_dev(bufs['u'].ptr, (2, n, n), NM, **kw)
                                else:
                                    pe.phases2J_dev(KVECS, bufs['ph'].ptr, bufs['w'].ptr, (3, n, n), NM, **kw)
                            run()
                            plan.sync()
                            ts = []
                            for _ in range(reps):
                                plan.timer_start()
                                run()
                                ts.append(plan.timer_stop())
                            out[(n, name, kind, mode)] = ts
                finally:
                    for b in bufs.values():
                        b.free()
    finally:
        plan.close()
    return out


def counter_run(n, dtypes):
    """{case: (FETCH_SIZE, WRITE_SIZE) in bytes}, from one launch per case under rocprofv3 in a child process; None without it"""
    prof = shutil.which('rocprofv3')
    if not prof:
        return None
    order = list(cases([n], dtypes))
    got = {}
    for counter in ('FETCH_SIZE', 'WRITE_SIZE'):          # a pass each
        tmp = tempfile.mkdtemp()
        cmd = [prof, '--pmc', counter, '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__),
               '--child', '--sizes', str(n), '--dtypes'] + list(dtypes)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError('counter run failed:\n' + (r.stdout + r.stderr)[-2000:])
        rows = {}
        for f in glob.glob(os.path.join(tmp, '**', '*counter_collection.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row['Kernel_Name']
                if 'field_jacobian_kernel' in name or 'phases_jacobian_kernel' in name:
                    rows[int(row['Dispatch_Id'])] = 1024 * float(row['Counter_Value'])      # the counter is in KiB
        shutil.rmtree(tmp, ignore_errors=True)
        if len(rows) != len(order):
            raise RuntimeError('expected %d launches under the profiler, found %d' % (len(order), len(rows)))
        got[counter] = [rows[d] for d in sorted(rows)]
    return {c: (got['FETCH_SIZE'][i], got['WRITE_SIZE'][i]) for i, c in enumerate(order)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[4096, 1024])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dtypes', nargs='*', default=['f32', 'f64'])
    ap.add_argument('--no-counters', action='store_true')
    ap.add_argument('--child', action='store_true', help='the counter run: one launch per case, nothing printed')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jac_timing.txt'))
    a = ap.parse_args()
    if a.child:
        run_all(a.sizes, a.dtypes, 0)
        return
    times = run_all(a.sizes, a.dtypes, a.reps)
    counters = None if a.no_counters else counter_run(max(a.sizes), a.dtypes)
    lines = ['u2J (gpa_field_jacobian_dev) and phases2J (gpa_phases_jacobian_dev, P = 3), resident; byte model: inputs once + outputs once, '
             'at the stream rate of %.0f GB/s' % STREAM_GBS]
    for case in cases(a.sizes, a.dtypes):
        n, name, kind, mode = case
        ts = times[case]
        ms = float(np.median(ts))
        mb = model_bytes(n, np.dtype(DTYPES[name]).itemsize, kind, mode) / 1e6
        t_model = mb / STREAM_GBS
        line = ('%s %5d^2 %-8s %-7s %8.4f ms (median of %d, min %.4f, max %.4f); byte model %6.0f MB = %.4f ms: %5.1f %% of the stream rate'
                % (name, n, kind, mode, ms, len(ts), min(ts), max(ts), mb, t_model, 100 * t_model / ms))
        if counters and case in counters:
            f, w = counters[case]
            line += '; FETCH_SIZE %.0f MB (x 2 = %.0f MB), WRITE_SIZE %.0f MB' % (f / 1e6, 2 * f / 1e6, w / 1e6)
        lines.append(line)
    if counters is None and not a.no_counters:
        lines.append('(rocprofv3 not found: no counter run)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
