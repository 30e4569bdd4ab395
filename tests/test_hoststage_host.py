"""The helper that stages the operands of a host-pointer call in one buffer (pygpa_amd/csrc/gpa_hoststage.h), no GPU: the
allocate / free / drain / copy primitives replaced by malloc / free / a counter / memcpy (GPA_DEVBUF_HOST_SEAM), so that slot
offsets, absent operands, in-out operands, caller-given addresses, reuse, growth, a failed allocation and the operand bound
can be checked on host memory (tests/host/hoststage_check.cpp).  Run plain and, where the host compiler has the runtimes, under
AddressSanitizer and UBSan -- an ordinary executable with its own main, nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path_factory, name, extra):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    out = str(tmp_path_factory.mktemp('hoststage') / name)
    src = os.path.join(ROOT, 'tests', 'host', 'hoststage_check.cpp')
    cmd = [gxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-DGPA_DEVBUF_HOST_SEAM', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc')]
    return subprocess.run(cmd + extra + [src, '-o', out], capture_output=True, text=True), out


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ')
    assert int(out.stdout.split()[1]) > 100


def test_hoststage(tmp_path_factory):
    r, exe = _build(tmp_path_factory, 'hoststage_check', [])
    assert r.returncode == 0, r.stderr[-2000:]
    _run(exe)


def test_hoststage_sanitized(tmp_path_factory):
    r, exe = _build(tmp_path_factory, 'hoststage_check_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the host compiler has no sanitizer runtimes')
    assert r.returncode == 0, r.stderr[-2000:]
    _run(exe)
