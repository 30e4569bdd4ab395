"""Host-side bookkeeping of the mirror modules, on the CPU: the control flow that sits above the C ABI is
run with the device call replaced by the oracle's array functions, and compared with the vectors the
real reference produced (tests/golden/peaks.npz, oracle/make_golden.py)."""
import numpy as np
import pytest

from oracle import gpa_oracle as orc

PEAK_CASES = ['clean128', 'noisy200x240', 'weak96', 'harmonics256', 'aniso160', 'stripe128']


class _OraclePeaks:
    """stands in for _lib.Plan.find_peaks: (coords, values) in skimage order, from the oracle"""
    calls = 0

    def find_peaks(self, image, sigma, dog_sigma, threshold_rel, want_smooth=False, max_out=4096):
        _OraclePeaks.calls += 1
        smooth = orc.smoothed_spectrum(image, sigma, DoG=dog_sigma > 0)
        c = orc.peak_local_max(smooth, threshold_rel)
        return c.astype(np.intp), smooth[tuple(c.T)]


@pytest.mark.parametrize('name', PEAK_CASES)
def test_extract_primary_ks_relaxation_loop(golden, name, monkeypatch):
    """the relaxation loop of the mirror returns what the reference's recursion returns, through every
    branch (plain, threshold / sigma relaxation -- 12 levels for the stripe image --, triangle selection)"""
    import pygpa_amd.geometric_phase_analysis as GPA
    monkeypatch.setattr(GPA, '_plan', lambda image, batch, dtype: _OraclePeaks())
    g = golden('peaks')
    thr, dog = g[name + '_kw']
    _OraclePeaks.calls = 0
    pks, aks = GPA.extract_primary_ks(g[name + '_image'], threshold=float(thr), DoG=bool(dog))
    assert np.array_equal(pks, g[name + '_primary'])
    assert np.array_equal(aks, g[name + '_all'])
    if name == 'stripe128':
        assert _OraclePeaks.calls > 5


def test_k_vector_helpers_match_oracle():
    """remove_negative_duplicates / select_closest_to_triangle / threshold schedule against the oracle's
    restatement (itself pinned by the peaks golden vectors) on random grid frequencies, including exact
    +k / -k pairs, near duplicates and closed triangles that tie to rounding"""
    import pygpa_amd.geometric_phase_analysis as GPA
    from pygpa_amd.mathtools import remove_negative_duplicates
    rng = np.random.default_rng(12)
    for _ in range(400):
        n = int(rng.integers(0, 12))
        ks = rng.integers(-20, 21, size=(n, 2)) / rng.choice([64., 100., 37.])
        if n:
            extra = -ks[rng.integers(0, n, size=3)] + rng.normal(size=(3, 2)) * 1e-7
            ks = np.concatenate([ks, extra])
        assert np.array_equal(remove_negative_duplicates(ks), orc.remove_negative_duplicates(ks))
        if len(ks) >= 3:
            assert np.array_equal(GPA.select_closest_to_triangle(ks), orc.select_closest_to_triangle(ks))
            assert np.array_equal(GPA.smallest_sum(ks[:3]), orc.smallest_sum(ks[:3]))
    assert np.isnan(GPA.smallest_sum(np.zeros((2, 2))))
    for t in list(rng.random(200)) + [0.7, 0.2, 0.1999999, 0.001, 0.0005]:
        nxt = GPA._lower_threshold(t)
        assert (nxt is None and orc._decrease_threshold(t) == t) or nxt == orc._decrease_threshold(t)


def test_generate_klists_matches_reference(golden):
    """generate_klists (host bookkeeping for wfr3 / wfr4) against the list the reference produced"""
    import pygpa_amd.geometric_phase_analysis as GPA
    g = golden('variants_64')
    lists = GPA.generate_klists(g['kvecs'], kmax=1.12, kmin=0.9, sort_list=True)
    assert len(lists) == 3 and np.array_equal(lists[1], g['wfr4_ring'])
    # unsorted: the same points in grid order
    raw = GPA.generate_klists(g['kvecs'], kmax=1.12, kmin=0.9)[1]
    assert sorted(map(tuple, raw)) == sorted(map(tuple, g['wfr4_ring']))


class _FakePeaksLib:
    """stands in for libgpa_hip.so's two candidate-list entry points: the device's list is `cands` (rows of (row, col,
    value)) in an arbitrary atomic-append order; a call stores the first max_out of them and reports the full count"""

    def __init__(self, cands, dtype):
        self.cands, self.dtype, self.calls = cands, dtype, []

    def _store(self, max_out, coords, values, count):
        import ctypes as C
        n = min(len(self.cands), max_out)
        c = np.ctypeslib.as_array((C.c_int32 * (2 * max_out)).from_address(coords.value)).reshape(max_out, 2)
        v = np.frombuffer((C.c_char * (max_out * np.dtype(self.dtype).itemsize)).from_address(values.value), dtype=self.dtype)
        c[:n] = self.cands[:n, :2]
        v[:n] = self.cands[:n, 2]
        count._obj.value = len(self.cands)
        return 0

    def gpa_find_peaks_dev(self, handle, image, sigma, dog_sigma, thr, max_out, coords, values, count, smooth):
        self.calls.append(('dev', thr, max_out))
        return self._store(max_out, coords, values, count)

    def gpa_find_peaks_again(self, handle, thr, max_out, coords, values, count):
        self.calls.append(('again', thr, max_out))
        return self._store(max_out, coords, values, count)

    def gpa_plan_destroy(self, handle):
        pass


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_find_peaks_dev_fetches_every_candidate(dtype):
    """find_peaks_dev used to keep the first max_out candidates of a longer list -- the device's append
    order, an arbitrary subset.  A count above max_out must lead to a second fetch of `count` entries from the plan's
    smoothed spectrum (gpa_find_peaks_again at the same threshold), sorted like find_peaks (highest first, raster order
    among equals); a count within max_out is taken as it is"""
    from pygpa_amd import _lib
    rng = np.random.default_rng(3)
    rc = rng.choice(64 * 64, size=40, replace=False)
    vals = rng.integers(1, 8, size=40).astype(dtype)          # many equal values: the raster tie order matters
    cands = np.column_stack([rc // 64, rc % 64, vals]).astype(np.float64)
    plan = _lib.Plan.__new__(_lib.Plan)
    plan.handle, plan.shape, plan.rdtype = 1, (64, 64), dtype
    plan.lib = _FakePeaksLib(cands, dtype)
    coords, values = plan.find_peaks_dev(0x1000, 1.0, 0.0, 0.25, max_out=16)
    assert plan.lib.calls == [('dev', 0.25, 16), ('again', 0.25, 40)]
    order = np.lexsort((cands[:, 1], cands[:, 0], -cands[:, 2]))
    assert np.array_equal(coords, cands[order, :2].astype(np.intp)) and coords.dtype == np.intp
    assert np.array_equal(values, cands[order, 2].astype(dtype)) and values.dtype == dtype
    plan.lib.calls = []
    coords2, values2 = plan.find_peaks_dev(0x1000, 1.0, 0.0, 0.25, max_out=40)
    assert plan.lib.calls == [('dev', 0.25, 40)]
    assert np.array_equal(coords2, coords) and np.array_equal(values2, values)
    plan.handle = None
