"""The half-length column solve of the unwrap (pygpa_amd/csrc/gpa_unwrap_colhalf.h: f64 columns of 16384 points) on the host:

  * a NumPy model of the single-column DCT-II / DCT-III through ONE complex FFT of half the length -- the identities the
    kernel is written from -- against scipy.fft.dct / idct at N = 16, 64 and 16384;
  * a NumPy model of the kernel's table layout (natural order over k = 0 .. N/2 - 1, each bin beside its partner N - k, bin
    0 beside bin N/2) and of the rows behind the transform's slots, through a whole column solve against
    idct(dct(r) / eigenvalues);
  * the header itself, thread by thread and phase by phase (tests/host/colhalf_emulator.cpp, as test_host_emulators.py).

These guard the index maps; the GPU tests (test_gpu_unwrap_f64_long.py) are the ones that need the kernel."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.fft import dct, idct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [16, 64, 16384]


def makhoul_src(n):
    m = np.arange(n)
    return np.where(m < (n + 1) // 2, 2 * m, 2 * (n - 1 - m) + 1)


def slot_rows(n):
    """rows of the column behind slot j of the half-length transform, as ColHalf::row_re / row_im: (v[2j], v[2j + 1])"""
    src = makhoul_src(n)
    return src[0::2], src[1::2]


def half_dct2(x):
    """SciPy's unnormalised DCT-II of one real sequence through an N/2-point complex FFT"""
    n = len(x)
    h = n // 2
    re, im = slot_rows(n)
    T = np.fft.fft(x[re] + 1j * x[im])
    k = np.arange(1, h)
    Tm = np.conj(T[h - k])
    ve, vo = 0.5 * (T[k] + Tm), -0.5j * (T[k] - Tm)
    U = np.exp(-0.5j * np.pi * k / n) * (ve + np.exp(-2j * np.pi * k / n) * vo)
    X = np.empty(n)
    X[0] = 2 * (T[0].real + T[0].imag)
    X[h] = np.sqrt(2.0) * (T[0].real - T[0].imag)
    X[k] = 2 * U.real
    X[n - k] = -2 * U.imag
    return X


def half_dct3(X):
    """the exact inverse of half_dct2 (SciPy's idct), again through one N/2-point complex FFT"""
    n = len(X)
    h = n // 2
    k = np.arange(1, h)
    V = np.empty(h, dtype=complex)
    V[0] = 0.5 * X[0]
    V[k] = np.exp(0.5j * np.pi * k / n) * 0.5 * (X[k] - 1j * X[n - k])
    vh = X[h] / np.sqrt(2.0)
    T = np.empty(h, dtype=complex)
    T[0] = 0.5 * (V[0].real + vh) + 0.5j * (V[0].real - vh)
    Vm = np.conj(V[h - k])
    T[k] = 0.5 * (V[k] + Vm) + 1j * 0.5 * np.exp(2j * np.pi * k / n) * (V[k] - Vm)
    t = np.fft.ifft(T)
    re, im = slot_rows(n)
    x = np.empty(n)
    x[re] = t.real
    x[im] = t.imag
    return x


@pytest.mark.parametrize('n', SIZES)
def test_half_length_dct_pair_equals_scipy(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + np.sin(np.arange(n) * 0.01)
    X = dct(x, type=2)
    scale = np.abs(X).max()
    assert np.abs(half_dct2(x) - X).max() < 1e-13 * scale
    assert np.abs(half_dct3(X) - idct(X, type=2)).max() < 1e-13 * np.abs(x).max()
    assert np.abs(half_dct3(half_dct2(x)) - x).max() < 1e-13 * np.abs(x).max()


@pytest.mark.parametrize('n', SIZES)
def test_slot_rows_are_a_permutation_in_fours(n):
    """slot j < N/4 holds rows (4j, 4j + 2), slot N/2 - 1 - j rows (4j + 3, 4j + 1): every row once"""
    re, im = slot_rows(n)
    assert sorted(np.concatenate([re, im]).tolist()) == list(range(n))
    j = np.arange(n // 4)
    assert np.array_equal(re[j], 4 * j) and np.array_equal(im[j], 4 * j + 2)
    assert np.array_equal(re[n // 2 - 1 - j], 4 * j + 3) and np.array_equal(im[n // 2 - 1 - j], 4 * j + 1)


def colhalf_tables(n0, a0):
    """the device tables as colhalf_tables() lays them out: k = 0 .. n0/2 - 1; ham[k] belongs to bin n0 - k, ham[0] to bin n0/2"""
    h = n0 // 2
    k = np.arange(h)
    km = np.where(k == 0, h, n0 - k)
    w = np.exp(-0.5j * np.pi * k / n0)
    e = np.exp(-2j * np.pi * k / n0)
    return w, e, 2 * np.sin(np.pi * k / (2.0 * a0)) ** 2, 2 * np.sin(np.pi * km / (2.0 * a0)) ** 2


def colhalf_solve(r, hb, first):
    """one column through the kernel's phases with the kernel's tables: z = idct(dct(r) / eig), and 2N <r, z>"""
    n = len(r)
    h = n // 2
    w, e, ha, ham = colhalf_tables(n, n)
    re, im = slot_rows(n)
    T = np.fft.fft(r[re] + 1j * r[im])
    k = np.arange(h)
    Tm = np.conj(T[(h - k) % h])
    U = w * (0.5 * (T + Tm) + e * (-0.5j) * (T - Tm))
    xlo, xhi = 2 * U.real, -2 * U.imag
    xlo[0] = 2 * (T[0].real + T[0].imag)
    xhi[0] = np.sqrt(2.0) * (T[0].real - T[0].imag)
    slo, shi = -0.5 / np.where(ha + hb == 0, 1.0, ha + hb), -0.5 / (ham + hb)
    if first:
        slo[0] = 1.0
    ylo, yhi = xlo * slo, xhi * shi
    c = np.where(k == 0, 0.5, 1.0)
    rho = float(np.sum(c * xlo * ylo + xhi * yhi))
    V = np.conj(w) * 0.5 * (ylo - 1j * yhi)
    v0, vh = 0.5 * ylo[0], yhi[0] / np.sqrt(2.0)
    Vm = np.conj(V[(h - k) % h])
    Tn = 0.5 * (V + Vm) + 0.5j * np.conj(e) * (V - Vm)
    Tn[0] = 0.5 * (v0 + vh) + 0.5j * (v0 - vh)
    t = np.fft.ifft(Tn)
    z = np.empty(n)
    z[re] = t.real
    z[im] = t.imag
    return z, rho


@pytest.mark.parametrize('first', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_table_layout_solves_a_column(n, first):
    """eigenvalues 2 (cos(pi k / N) + cos(pi j / M) - 2) = -2 (ha_k + hb_j), the DC bin of column 0 divided by 1
    (phase_unwrap.py:106-115)"""
    rng = np.random.default_rng(n + 1)
    r = rng.standard_normal(n)
    hb = 0.0 if first else 2 * np.sin(np.pi * 5 / (2.0 * 64)) ** 2
    kk = np.arange(n)
    eig = -2.0 * (2 * np.sin(np.pi * kk / (2.0 * n)) ** 2 + hb)
    if first:
        eig[0] = 1.0
    ref = idct(dct(r, type=2) / eig, type=2)
    z, rho = colhalf_solve(r, hb, first)
    assert np.abs(z - ref).max() < 1e-12 * np.abs(ref).max()
    assert abs(rho - 2.0 * n * float(r @ ref)) < 1e-10 * abs(2.0 * n * float(r @ ref))


def test_colhalf_emulator(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'colhalf_emulator')
    src = os.path.join(ROOT, 'tests', 'host', 'colhalf_emulator.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith('OK')
