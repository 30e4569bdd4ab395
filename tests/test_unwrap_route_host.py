"""The kernel choice of the weighted unwrap (pygpa_amd/csrc/gpa_unwrap_route.h), no GPU: unwrap_route() for a list of shapes
and options against rows written out here (read off the dispatchers the header replaced, not computed by a second copy of
the rules), and the coupling of the route with the table-availability functions over every power-of-two shape and option
combination (tests/host/unwrap_route_table.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (fwd, inv, cols, rowpq, fuse_pq, lat_rows, lat_cols, lat_pq); inv '-': rowpq, the inverse row kernel is not
# launched.  nprob = 1 and no option unless named; tables as the workspace builds them by default.  None: not compared (the
# mixed-radix kernels of the generic sizes have no latency-tuned forms).
ROWS = [
    ('f32 512 512',                       ('packed', '-', 'dct', 1, 0, 1, 1, 1)),
    ('f32 512 512 nprob=4',               ('packed', 'packed', 'dct', 0, 0, 0, 0, 0)),
    ('f32 512 512 nprob=2',               ('packed', '-', 'dct', 1, 0, 1, 1, 1)),
    ('f32 512 512 NO_LAT',                ('packed', 'packed', 'dct', 0, 0, 0, 0, 0)),
    ('f32 512 512 NO_ROWPQ',              ('packed', 'packed', 'dct', 0, 0, 1, 1, 1)),
    ('f64 512 512',                       ('packed', '-', 'tri', 1, 0, 1, 1, 1)),
    ('f64 1024 1024',                     ('packed', 'packed', 'tri', 0, 0, 1, 1, 1)),
    ('f32 1024 1024',                     ('packed', 'packed', 'dct', 0, 0, 1, 1, 1)),
    ('f32 2048 2048',                     ('packed', 'packed', 'stream', 0, 1, 0, 0, 1)),
    ('f32 2048 2048 NO_PQDCT',            ('packed', 'packed', 'stream', 0, 0, 0, 0, 1)),
    ('f32 2048 2048 COLSOLVE=fft',        ('packed', 'packed', 'dct', 0, 0, 0, 0, 1)),
    ('f32 2048 2048 COLSOLVE=tri',        ('packed', 'packed', 'tri', 0, 0, 0, 0, 1)),
    ('f32 256 256 COLSOLVE=stream',       ('packed', '-', 'stream', 1, 0, 1, 1, 1)),
    ('f32 256 256 COLSOLVE=tri',          ('packed', '-', 'tri', 1, 0, 1, 1, 1)),
    ('f32 4096 4096',                     ('packed', 'pers', 'stream', 0, 1, 0, 0, 1)),
    ('f32 4096 4096 NO_ROWPERS',          ('packed', 'packed', 'stream', 0, 1, 0, 0, 1)),
    ('f32 4096 4096 ROWHALF_MINLG=12',    ('half', 'half', 'stream', 0, 1, 0, 0, 1)),
    ('f32 64 4096',                       ('packed', 'pers', 'dct', 0, 0, 0, 1, 1)),
    ('f32 64 4096 NO_ROWPERS',            ('packed', 'packed', 'dct', 0, 0, 0, 1, 1)),
    ('f32 64 4096 ROWHALF_MINLG=12',      ('half', 'half', 'dct', 0, 0, 0, 1, 1)),
    ('f64 4096 4096',                     ('half', 'packed', 'stream', 0, 1, 0, 0, 1)),
    ('f64 4096 4096 NO_ROWHALF',          ('packed', 'packed', 'stream', 0, 1, 0, 0, 1)),
    # an explicitly set ROWHALF_MINLG, its default value included, switches the f64 4096-point forward special case off
    ('f64 4096 4096 ROWHALF_MINLG=13',    ('packed', 'packed', 'stream', 0, 1, 0, 0, 1)),
    ('f64 64 4096',                       ('half', 'packed', 'dct', 0, 0, 0, 1, 1)),
    ('f64 64 4096 NO_ROWHALF',            ('packed', 'packed', 'dct', 0, 0, 0, 1, 1)),
    ('f64 64 4096 ROWHALF_MINLG=13',      ('packed', 'packed', 'dct', 0, 0, 0, 1, 1)),
    ('f32 8192 8192',                     ('halfpers', 'halfpers', 'stream', 0, 0, 0, 0, 1)),
    ('f32 8192 8192 NO_ROWPERS',          ('half', 'half', 'stream', 0, 0, 0, 0, 1)),
    ('f32 8192 8192 NO_ROWHALF',          ('packed', 'packed', 'stream', 0, 0, 0, 0, 1)),
    ('f32 128 8192',                      ('halfpers', 'halfpers', 'dct', 0, 0, 0, 1, 1)),
    ('f32 128 8192 NO_ROWPERS',           ('half', 'half', 'dct', 0, 0, 0, 1, 1)),
    ('f32 128 8192 NO_ROWHALF',           ('packed', 'packed', 'dct', 0, 0, 0, 1, 1)),
    ('f32 8192 128',                      ('packed', '-', 'dct', 1, 0, 1, 0, 1)),
    ('f64 8192 8192',                     ('half', 'half', 'stream', 0, 0, 0, 0, 1)),
    ('f32 16384 16384',                   ('halfpers', 'halfpers', 'stream', 0, 0, 0, 0, 1)),
    ('f32 16384 16384 COLSOLVE=tri',      ('halfpers', 'halfpers', 'tri', 0, 0, 0, 0, 1)),
    ('f32 16384 16384 COLSOLVE=fft',      ('halfpers', 'halfpers', 'dct', 0, 0, 0, 0, 1)),
    ('f32 64 16384',                      ('halfpers', 'halfpers', 'dct', 0, 0, 0, 1, 1)),
    ('f64 16384 16384',                   ('half', 'half', 'stream', 0, 0, 0, 0, 1)),
    # NO_ROWHALF is ignored for f64 rows of 16384 points: they have no packed kernel
    ('f64 16384 16384 NO_ROWHALF',        ('half', 'half', 'stream', 0, 0, 0, 0, 1)),
    ('f64 16384 16384 COLSOLVE=tri',      ('half', 'half', 'tri', 0, 0, 0, 0, 1)),
    ('f64 16384 16384 COLSOLVE=fft',      ('half', 'half', 'colhalf', 0, 0, 0, 0, 1)),
    ('f64 64 16384',                      ('half', 'half', 'dct', 0, 0, 0, 1, 1)),
    ('f64 64 16384 NO_ROWHALF',           ('half', 'half', 'dct', 0, 0, 0, 1, 1)),
    ('f64 16384 64',                      ('packed', '-', 'colhalf', 1, 0, 1, 0, 1)),
    # COLSOLVE=stream where no stream table exists (not square): neither tri nor the default -- the transform kernel
    ('f64 1024 512 COLSOLVE=stream',      ('packed', '-', 'dct', 1, 0, 1, 1, 1)),
    ('f32 1000 1000 generic',             ('mr', 'mr', 'tri', 0, 0, None, None, 1)),
    ('f32 1000 1000 generic COLSOLVE=fft', ('mr', 'mr', 'mr', 0, 0, None, None, 1)),
    ('f32 3000 3000 generic',             ('mr', 'mr', 'stream', 0, 0, None, None, 1)),
    ('f32 96 8192 generic',               ('mr', 'mr', 'mr', 0, 0, None, None, 1)),
]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    out = str(tmp_path_factory.mktemp('route') / 'unwrap_route_table')
    src = os.path.join(ROOT, 'tests', 'host', 'unwrap_route_table.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', out], check=True)
    return out


def test_route_table(exe):
    out = subprocess.run([exe], input=''.join(c + '\n' for c, _ in ROWS), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.strip().split('\n')
    assert len(lines) == len(ROWS)
    bad = []
    for (case, want), line in zip(ROWS, lines):
        got = line.split()
        got = tuple(got[:3]) + tuple(int(v) for v in got[3:])
        if any(w is not None and w != g for w, g in zip(want, got)) or len(got) != len(want):
            bad.append((case, want, got))
    assert not bad, bad


def test_route_never_names_a_missing_table(exe):
    out = subprocess.run([exe, 'coupling'], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.startswith('OK ')
    assert int(out.stdout.split()[1]) > 1000
