"""ctypes binding of libgpa_hip.so (C ABI declared in include/gpa_hip.h).

The library is the product: if it cannot be loaded, or no GPU is visible, every
entry point raises -- there is no CPU fallback.
"""
import atexit
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPA_HIP_LIB selects another build of the same library (performance experiments, tools/variant.sh)
LIB_PATH = os.environ.get('GPA_HIP_LIB') or os.path.join(_HERE, 'libgpa_hip.so')

GPA_F32, GPA_F64 = 0, 1
UCELL_MAX_FRAMES = 65535     # frames of one gpa_unit_cell_average_batch_dev call
UNDISTORT_MAX_FRAMES = 65535     # frames of one gpa_undistort_image_batch[_dev] call
UNWRAP_BATCH_MAX = 4096          # problems of one gpa_unwrap_batch[_dev] call (GPA_UNWRAP_BATCH_MAX)
WFF_MAX_S, WFF_MAX_T = 40, 8     # half-window round(2 sigma) and thresholds of one gpa_wff[_dev] call
PREP_MAX_R, PREP_MAX_N1 = 254, 32768     # erosion radius of gpa_mask_erode_disk, row length of gpa_gauss_homogenize
LINES_MAX_N = 16384                      # longest line of gpa_line_nanmedian / gpa_homogenize_per_axis (GPA_LINES_MAX_N)
_DTYPES = {GPA_F32: (np.float32, np.complex64), GPA_F64: (np.float64, np.complex128)}

# every symbol of include/gpa_hip.h: name -> (restype, argtypes)
_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
_dp, _ip, _fp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
SIGNATURES = {
    'gpa_version': (_i, []),
    'gpa_last_error': (C.c_char_p, []),
    'gpa_device_count': (_i, []),
    'gpa_set_option': (_i, [C.c_char_p, C.c_char_p]),
    'gpa_plan_create': (_vp, [_i, _i, _i, _i, _i]),
    'gpa_plan_destroy': (None, [_vp]),
    'gpa_plan_sync': (_i, [_vp]),
    'gpa_plan_workspace_bytes': (_sz, [_vp]),
    'gpa_plan_stream': (_vp, [_vp]),
    'gpa_plan_fft_len': (_i, [_vp, _i]),
    'gpa_lockin_batch': (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    'gpa_lockin_batch_dev': (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    'gpa_sweep': (_i, [_vp, _vp, _vp, _vp, _i, _d, _vp, _vp, _vp]),
    'gpa_sweep_dev': (_i, [_vp, _vp, _vp, _vp, _i, _d, _vp, _vp, _vp]),
    'gpa_sweep_grad': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    'gpa_sweep_grad_dev': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    'gpa_sweep_gated': (_i, [_vp, _vp, _vp, _vp, _i, _d, _vp, _vp, _vp]),
    'gpa_reconstruct_prediff': (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    'gpa_invert_u': (_i, [_vp, _vp, _i, _i, _vp]),
    'gpa_invert_u_mode': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'gpa_invert_u_mode_dev': (_i, [_vp, _vp, _d, _i, _i, _i, _i, _vp, _i, _vp]),
    'gpa_undistort_image_dev': (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'gpa_undistort_image_scaled_dev': (_i, [_vp, _vp, _vp, _d, _vp, _i, _vp, _vp]),
    'gpa_undistort_image_batch_dev': (_i, [_vp, _vp, _i, _vp, _i, _d, _vp, _vp]),
    'gpa_undistort_image_batch': (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    'gpa_reconstruct_grad': (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    'gpa_reconstruct_grad_dev': (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    'gpa_weighted_lstsq': (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    'gpa_unwrap_prediff': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_prediff_dev': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_prediff_enqueue_dev': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _vp]),
    'gpa_unwrap_finish': (_i, [_vp, _vp]),
    'gpa_unwrap': (_i, [_vp, _vp, _vp, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_dev': (_i, [_vp, _vp, _vp, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_batch_dev': (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_prediff_batch_dev': (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_batch_finish': (_i, [_vp, _i, _vp]),
    'gpa_unwrap_batch': (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_prediff_batch': (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _d, _i, _vp, _vp]),
    'gpa_unwrap_batch_problem_bytes': (_sz, [_vp, _i]),
    'gpa_extract_displacement_field': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _vp, _vp, _vp, _vp]),
    'gpa_extract_displacement_field_dev': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _vp, _vp, _vp, _vp]),
    'gpa_extract_displacement_field_async': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _vp, _vp, _vp]),
    'gpa_last_iters': (_i, [_vp, _vp]),
    'gpa_extract_displacement_field_grad': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gpa_extract_displacement_field_grad_dev': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gpa_extract_displacement_field_grad_async': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'gpa_extract_displacement_field_batch_dev': (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _d, _i, _i, _vp, _vp]),
    'gpa_extract_displacement_field_grad_batch_dev': (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                                           _vp]),
    'gpa_last_batch_iters': (_i, [_vp, _i, _vp]),
    'gpa_supports_batch': (_i, [_vp]),
    'gpa_extract_gradients': (_i, [_vp, _vp, _vp, _i, _vp, _i, _d, _i, _vp, _vp, _vp]),
    'gpa_mean_dev': (_i, [_vp, _vp, _sz, _dp]),
    'gpa_tile_gradients_dev': (_i, [_vp, _vp, _sz, _i, _i, _d, _vp, _i, _vp, _i, _d, _i, _i, _i, _i, _i,
                                    _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz]),
    'gpa_tile_sums_dev': (_i, [_vp, _vp, _sz, _sz, _vp, _i, _i, _vp]),
    'gpa_tile_set_mean_dev': (_i, [_vp, _vp, _d]),
    'gpa_tile_gradients_meandev_dev': (_i, [_vp, _vp, _sz, _i, _i, _vp, _i, _vp, _i, _d, _i, _i, _i, _i, _i,
                                            _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _sz]),
    'gpa_stitch_tiles_dev': (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'gpa_plan_wait_stream': (_i, [_vp, _vp]),
    'gpa_stream_wait_plan': (_i, [_vp, _vp]),
    'gpa_invert_u_overlap': (_i, [_vp, _vp, _i, _i, _vp]),
    'gpa_undistort_image': (_i, [_vp, _vp, _vp, _vp]),
    'gpa_phasegradient2J': (_i, [_vp, _vp, _i, _vp, _vp, _d, _vp, _vp]),
    'gpa_phasegradient2J_dev': (_i, [_vp, _vp, _i, _vp, _vp, _d, _vp, _vp]),
    'gpa_lockin_weights_dev': (_i, [_vp, _vp, _i, _vp]),
    'gpa_props_from_jac': (_i, [_i, _i, _sz, _vp, _i, _d, _d, _i, _vp]),
    'gpa_props_from_jac_dev': (_i, [_i, _i, _sz, _vp, _i, _d, _d, _i, _vp, _vp]),
    'gpa_kerelsky_fit': (_i, [_i, _i, _sz, _vp, _vp, _vp, _i, _d, _vp, _vp]),
    'gpa_kerelsky_fit_dev': (_i, [_i, _i, _sz, _vp, _vp, _vp, _i, _d, _vp, _vp, _vp]),
    'gpa_field_jacobian': (_i, [_i, _i, _i, _i, _i, _vp, _d, _i, _vp, _vp, _d, _d, _i]),
    'gpa_field_jacobian_dev': (_i, [_i, _i, _i, _i, _i, _vp, _d, _i, _vp, _vp, _d, _d, _i, _vp]),
    'gpa_phases_jacobian': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _d, _i, _vp, _vp, _d, _d, _i]),
    'gpa_phases_jacobian_dev': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _d, _i, _vp, _vp, _d, _d, _i, _vp]),
    'gpa_gradients_jacobian': (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _d, _i, _vp, _vp, _d, _d, _i]),
    'gpa_gradients_jacobian_dev': (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _d, _i, _vp, _vp, _d, _d, _i, _vp]),
    'gpa_phys_props_from_jac': (_i, [_i, _i, _sz, _vp, _i, _d, _d, _i, _d, _vp]),
    'gpa_phys_props_from_jac_dev': (_i, [_i, _i, _sz, _vp, _i, _d, _d, _i, _d, _vp, _vp]),
    'gpa_fit_plane': (_i, [_vp, _vp, _i, _d, _dp, _ip]),
    'gpa_fit_plane_dev': (_i, [_vp, _vp, _i, _d, _dp, _ip]),
    'gpa_fit_planes_dev': (_i, [_vp, _vp, _i, _i, _d, _vp, _vp]),
    'gpa_lockin_polar_crop_dev': (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    'gpa_iterate_gpa_dev': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'gpa_iterate_gpa': (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'gpa_per_dft': (_i, [_vp, _vp, _vp]),
    'gpa_per_dft_dev': (_i, [_vp, _vp, _vp]),
    'gpa_per': (_i, [_vp, _vp, _i, _vp, _vp]),
    'gpa_gaussian_deconvolve': (_i, [_vp, _vp, _i, _d, _d, _vp]),
    'gpa_gaussian_deconvolve_dev': (_i, [_vp, _vp, _i, _d, _d, _vp]),
    'gpa_find_peaks': (_i, [_vp, _vp, _d, _d, _d, _i, _vp, _vp, _ip, _vp]),
    'gpa_find_peaks_dev': (_i, [_vp, _vp, _d, _d, _d, _i, _vp, _vp, _ip, _vp]),
    'gpa_find_peaks_again': (_i, [_vp, _d, _i, _vp, _vp, _ip]),
    'gpa_unit_cell_average': (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'gpa_unit_cell_average_dev': (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'gpa_unit_cell_average_batch_dev': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    'gpa_expand_unitcell': (_i, [_vp, _vp, _vp, _d, _vp, _vp]),
    'gpa_expand_unitcell_dev': (_i, [_vp, _vp, _vp, _d, _vp, _vp]),
    'gpa_wff': (_i, [_vp, _vp, _d, _vp, _i, _vp, _i, _vp, _i, _d, _vp]),
    'gpa_wff_dev': (_i, [_vp, _vp, _d, _vp, _i, _vp, _i, _vp, _i, _d, _vp]),
    'gpa_gauss_homogenize': (_i, [_vp, _vp, _vp, _d, _i, _d, _vp, _vp]),
    'gpa_gauss_homogenize_dev': (_i, [_vp, _vp, _vp, _d, _i, _d, _vp, _vp]),
    'gpa_mask_any_equal': (_i, [_vp, _vp, _i, _d, _i, _vp]),
    'gpa_mask_any_equal_dev': (_i, [_vp, _vp, _i, _d, _i, _vp]),
    'gpa_mask_erode_disk': (_i, [_vp, _vp, _i, _i, _vp]),
    'gpa_mask_erode_disk_dev': (_i, [_vp, _vp, _i, _i, _vp]),
    'gpa_mask_bounds': (_i, [_vp, _vp, _vp]),
    'gpa_mask_bounds_dev': (_i, [_vp, _vp, _vp]),
    'gpa_nan_lines': (_i, [_vp, _vp, _vp, _vp]),
    'gpa_nan_lines_dev': (_i, [_vp, _vp, _vp, _vp]),
    'gpa_nan_trim_lims': (_i, [_vp, _vp, _vp]),
    'gpa_nan_trim_lims_dev': (_i, [_vp, _vp, _vp]),
    'gpa_line_nanmedian': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'gpa_line_nanmedian_dev': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'gpa_homogenize_per_axis': (_i, [_vp, _vp, _vp, _d, _i, _i, _vp, _vp]),
    'gpa_homogenize_per_axis_dev': (_i, [_vp, _vp, _vp, _d, _i, _i, _vp, _vp]),
    'gpa_homogenize_lines': (_i, [_vp, _vp, _d, _vp, _vp, _vp, _vp]),
    'gpa_homogenize_lines_dev': (_i, [_vp, _vp, _d, _vp, _vp, _vp, _vp]),
    'gpa_timer_start': (_i, [_vp]),
    'gpa_timer_stop': (_i, [_vp, _vp]),
    'gpa_set_profiling': (_i, [_vp, _i]),
    'gpa_last_stage_ms': (_i, [_vp, _vp]),
    'gpa_last_kernel_profile': (_i, [_vp, C.c_char_p, _sz]),
    'gpa_last_passb_skips': (_i, [_vp, _vp, _vp]),
    'gpa_passb_visiting_order': (_i, [_vp, _vp, _i, _vp]),
    'gpa_download_async': (_i, [_vp, _vp, _vp, _sz, _i]),
    'gpa_download_wait': (_i, [_vp, _i]),
}

_lib = None
_lock = threading.Lock()


class UcellGeom(C.Structure):
    """gpa_ucell_geom: the geometry of unit_cell_average / expand_unitcell, computed on the host as the reference does"""
    _fields_ = [('ks', C.c_double * 4), ('kinv', C.c_double * 4), ('rmin', C.c_double * 2), ('rsize', C.c_int32 * 2),
                ('z', C.c_double)]

    @classmethod
    def make(cls, ks, kinv, rmin, rsize, z):
        g = cls()
        g.ks[:] = [float(v) for v in np.asarray(ks, dtype=np.float64).reshape(4)]
        g.kinv[:] = [float(v) for v in np.asarray(kinv, dtype=np.float64).reshape(4)]
        g.rmin[:] = [float(v) for v in np.asarray(rmin, dtype=np.float64).reshape(2)]
        g.rsize[:] = [int(v) for v in rsize]
        g.z = float(z)
        return g


class GPAError(RuntimeError):
    pass


def load():
    """Load libgpa_hip.so (once) and declare every prototype.  Raises GPAError if the
    library is missing -- build it with ``python -m pygpa_amd.build``."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GPAError('HIP extension %s is missing; build it with `python -m pygpa_amd.build`. '
                           'pygpa_amd has no CPU fallback.' % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        except OSError as e:
            raise GPAError('cannot load %s: %s' % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def passb_visiting_order(klist, kref):
    """list positions of `klist` (K x 2) in the order the shared pass B visits them for the reference vector `kref`
    (gpa_passb_visiting_order: the library's own rule, on the host)"""
    kl = np.ascontiguousarray(klist, dtype=np.float64).reshape(-1, 2)
    kr = np.ascontiguousarray(kref, dtype=np.float64).reshape(2)
    out = np.empty(len(kl), dtype=np.int32)
    check(load().gpa_passb_visiting_order(kl.ctypes.data, kr.ctypes.data, len(kl), out.ctypes.data), 'gpa_passb_visiting_order')
    return [int(v) for v in out]


def last_error():
    msg = load().gpa_last_error()
    return msg.decode() if msg else ''


def check(code, what):
    if code != 0:
        raise GPAError('%s failed (%d): %s' % (what, code, last_error()))


# scipy.ndimage boundary modes of invert_u / invert_u_overlap -> the mode codes of gpa_invert_u_mode[_dev]
_WARP_MODES = {'nearest': 0, 'constant': 1, 'reflect': 2, 'grid-mirror': 2, 'mirror': 3, 'grid-wrap': 4}
_WARP_REFUSED = {
    'wrap': "mode 'wrap' is scipy.ndimage's legacy mode (coordinates fold with period n - 1 over spline coefficients of "
            "period n; SciPy's documentation points to 'grid-wrap'): use mode='grid-wrap'",
    'grid-constant': "mode 'grid-constant' is not provided: with the cval = nan last round of invert_u_overlap SciPy pads "
                     "with NaN before the spline prefilter, and the reference returns all NaN",
}


def warp_mode_code(mode):
    """The library's code of a scipy.ndimage boundary mode of invert_u / invert_u_overlap: 0 'nearest', 1 'constant',
    2 'reflect' and its synonym 'grid-mirror', 3 'mirror', 4 'grid-wrap'.  Every other mode raises NotImplementedError
    (for 'wrap' and 'grid-constant' with the reason); needs no library."""
    try:
        return _WARP_MODES[mode]
    except (KeyError, TypeError):
        pass
    raise NotImplementedError(_WARP_REFUSED.get(mode if isinstance(mode, str) else None,
                                                'mode must be one of %s, not %r' % (', '.join(map(repr, _WARP_MODES)), mode)))


_OPTION_VALUES = {}     # what this process has set through set_option (name -> str); a name that is absent follows the
#                         library's start-up value, i.e. the GPA_<NAME> environment variable read once


def set_option(name, value):
    """gpa_set_option: a diagnostic / test switch of the library ('NO_LAT', 'COLSOLVE', 'F32_EPS_FLOOR', ...; the
    names of INTEGRATION.md).  value None clears it.  The library reads the GPA_<NAME> environment variables once, when
    it is first used; afterwards only this call changes a switch."""
    check(load().gpa_set_option(str(name).encode(), None if value is None else str(value).encode()), 'gpa_set_option')
    _OPTION_VALUES[str(name)] = None if value is None else str(value)


def get_option(name):
    """the value a switch currently has as far as this process can know: what set_option last gave it, else the GPA_<NAME>
    environment variable the library read at start-up (None: unset)"""
    name = str(name)
    if name in _OPTION_VALUES:
        return _OPTION_VALUES[name]
    return os.environ.get('GPA_' + name)


class options:
    """with options(NO_LAT=1, COLSOLVE='tri'): ...  -- switches set for the block; afterwards every one of them is back at the
    value it had before (an outer options() block's, the environment's, or unset), not simply cleared"""

    def __init__(self, **kw):
        self.kw = kw
        self.prev = {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.prev[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            set_option(k, self.prev.get(k))
        return False


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _peak_lists(kvecs, klists):
    """(kvecs (P, 2), P, klists (P, K, 2), K) as contiguous float64: the reference vectors and candidate lists of a sweep"""
    kvecs = _f64(kvecs).reshape(-1, 2)
    P = len(kvecs)
    klists = _f64(klists).reshape(P, -1, 2)
    return kvecs, P, klists, klists.shape[1]


def stack_shapes(frames_shape, u_shape, plan_shape=None):
    """The shapes undistort_image_stack takes: frames (B, N, M) with B >= 1, u (2, N, M) or (B, 2, N, M).  Returns
    (B, per_frame); ValueError for any other combination (and for frames that do not match plan_shape, when given)."""
    frames_shape, u_shape = tuple(frames_shape), tuple(u_shape)
    if len(frames_shape) != 3 or frames_shape[0] < 1:
        raise ValueError('frames must be a stack (B, N, M) with B >= 1, not %s' % (frames_shape,))
    B, shape = frames_shape[0], frames_shape[1:]
    if plan_shape is not None and shape != tuple(plan_shape):
        raise ValueError('frames %s do not match the plan %s' % (shape, tuple(plan_shape)))
    if u_shape == (2,) + shape:
        return B, False
    if len(u_shape) == 4 and u_shape[1:] == (2,) + shape:
        if u_shape[0] != B:
            raise ValueError('u holds %d fields for %d frames' % (u_shape[0], B))
        return B, True
    raise ValueError('u must be (2, N, M) or (B, 2, N, M) for frames (B, N, M) = %s, not %s' % (frames_shape, u_shape))


def unwrap_stack_shapes(a_shape, dy_shape=None, plan_shape=None):
    """B of a stack of phase maps (B, N, M) -- or, with dy_shape, of gradient pairs (B, N, M - 1) / (B, N - 1, M) -- on the
    grid plan_shape where given; ValueError for anything else.  Pure shape arithmetic: no array, no library."""
    a_shape = tuple(a_shape)
    if len(a_shape) != 3:
        raise ValueError('a stack must be three-dimensional (B, N, M), got %s' % (a_shape,))
    if a_shape[0] < 1:
        raise ValueError('the stack is empty')
    if dy_shape is None:
        grid = a_shape[1:]
    else:
        dy_shape = tuple(dy_shape)
        if len(dy_shape) != 3 or dy_shape[0] != a_shape[0] or dy_shape[1] + 1 != a_shape[1] or dy_shape[2] != a_shape[2] + 1:
            raise ValueError('dx %s and dy %s do not pair: need (B, N, M - 1) and (B, N - 1, M)' % (a_shape, dy_shape))
        grid = (a_shape[1], dy_shape[2])
    if grid[0] < 2 or grid[1] < 2:
        raise ValueError('the maps must be at least 2 x 2, got %s' % (grid,))
    if plan_shape is not None and tuple(plan_shape) != grid:
        raise ValueError('maps of %s do not match the plan %s' % (grid, tuple(plan_shape)))
    return a_shape[0]


def unwrap_stack_weight_planes(w_shape, B, grid):
    """1 for a weight (N, M) shared by the B maps of `grid`, B for (B, N, M); ValueError for anything else"""
    w_shape, grid = tuple(w_shape), tuple(grid)
    if w_shape == grid:
        return 1
    if w_shape == (B,) + grid:
        return B
    raise ValueError('weight must be %s or %s, got %s' % (grid, (B,) + grid, w_shape))


class Plan:
    """One device + stream + workspace for images of a fixed shape (wraps gpa_plan)."""

    def __init__(self, shape, max_batch, dtype=np.float64, device=0):
        self.lib = load()
        self.shape = (int(shape[0]), int(shape[1]))
        self.code = GPA_F32 if np.dtype(dtype) == np.float32 else GPA_F64
        self.rdtype, self.cdtype = _DTYPES[self.code]
        self.max_batch = int(max_batch)
        self.device = int(device)
        if self.lib.gpa_device_count() <= 0:
            raise GPAError('no MI355X/HIP device visible; pygpa_amd has no CPU fallback')
        self.handle = self.lib.gpa_plan_create(self.device, self.shape[0], self.shape[1], self.max_batch, self.code)
        if not self.handle:
            raise GPAError('gpa_plan_create failed: ' + last_error())

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.gpa_plan_destroy(self.handle)
            self.handle = None
        for name in ('_d_img', '_d_u'):
            buf = getattr(self, name, None)
            if buf is not None:
                buf.free()
                setattr(self, name, None)
        self._stage = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -----------------------------------------------------------
    def _img(self, image):
        image = np.ascontiguousarray(image, dtype=self.rdtype)
        if image.shape != self.shape:
            raise ValueError('image shape %s does not match the plan %s' % (image.shape, self.shape))
        return image

    @property
    def workspace_bytes(self):
        return self.lib.gpa_plan_workspace_bytes(self.handle)

    def fft_len(self, axis):
        return self.lib.gpa_plan_fft_len(self.handle, axis)

    def sync(self):
        check(self.lib.gpa_plan_sync(self.handle), 'gpa_plan_sync')

    # ---- host-pointer entry points ------------------------------------------
    def lockin_batch(self, image, kvecs, sigma):
        image = self._img(image)
        kvecs = _f64(kvecs).reshape(-1, 2)
        out = np.empty((len(kvecs),) + self.shape, dtype=self.cdtype)
        check(self.lib.gpa_lockin_batch(self.handle, _ptr(image), _ptr(kvecs), len(kvecs), float(sigma), _ptr(out)),
              'gpa_lockin_batch')
        return out

    def sweep(self, image, kref, klist, sigma, want_kidx=True, want_grad=False, grad_mode=0):
        image = self._img(image)
        kref = _f64(kref).reshape(2)
        klist = _f64(klist).reshape(-1, 2)
        lockin = np.empty(self.shape, dtype=self.cdtype)
        kidx = np.empty(self.shape, dtype=np.int32) if want_kidx else None
        grad = np.empty(self.shape + (2,), dtype=self.rdtype) if want_grad else None
        if want_grad and grad_mode:
            check(self.lib.gpa_sweep_grad(self.handle, _ptr(image), _ptr(kref), _ptr(klist), len(klist), float(sigma),
                                          int(grad_mode), _ptr(lockin), _ptr(kidx), _ptr(grad)), 'gpa_sweep_grad')
        else:
            check(self.lib.gpa_sweep(self.handle, _ptr(image), _ptr(kref), _ptr(klist), len(klist), float(sigma),
                                     _ptr(lockin), _ptr(kidx), _ptr(grad)), 'gpa_sweep')
        return lockin, kidx, grad

    def sweep_gated(self, image, kref, klist, sigma, gate):
        """wfr4's selection rule; gate: (K, K) bool, gate[j, k] = candidate k may replace the kept candidate j"""
        image = self._img(image)
        kref = _f64(kref).reshape(2)
        klist = _f64(klist).reshape(-1, 2)
        gate = np.ascontiguousarray(gate, dtype=np.uint8)
        if gate.shape != (len(klist), len(klist)):
            raise ValueError('gate must be (K, K)')
        lockin = np.empty(self.shape, dtype=self.cdtype)
        kidx = np.empty(self.shape, dtype=np.int32)
        check(self.lib.gpa_sweep_gated(self.handle, _ptr(image), _ptr(kref), _ptr(klist), len(klist), float(sigma),
                                       _ptr(gate), _ptr(lockin), _ptr(kidx)), 'gpa_sweep_gated')
        return lockin, kidx

    def reconstruct_prediff(self, grads, weights, kvecs):
        kvecs = _f64(kvecs).reshape(-1, 2)
        grads = np.ascontiguousarray(grads, dtype=self.rdtype)
        weights = np.ascontiguousarray(weights, dtype=self.rdtype)
        if grads.shape != (len(kvecs),) + self.shape + (2,) or weights.shape != grads.shape[:-1]:
            raise ValueError('grads must be (P,) + plan shape + (2,), weights (P,) + plan shape')
        n0, n1 = self.shape
        dudx = np.empty((2, n0, n1 - 1), dtype=self.rdtype)
        dudy = np.empty((2, n0 - 1, n1), dtype=self.rdtype)
        wnorm = np.empty((n0, n1), dtype=self.rdtype)
        check(self.lib.gpa_reconstruct_prediff(self.handle, _ptr(grads), _ptr(weights), _ptr(kvecs), len(kvecs),
                                               _ptr(dudx), _ptr(dudy), _ptr(wnorm)), 'gpa_reconstruct_prediff')
        return dudx, dudy, wnorm

    def invert_u(self, us, iters=35, edge=0, mode='nearest'):
        """invert_u of the reference on the plan's grid; mode: 'nearest', 'constant', 'reflect' / 'grid-mirror', 'mirror' or
        'grid-wrap' (warp_mode_code)"""
        us = np.ascontiguousarray(us, dtype=self.rdtype)
        if us.shape != (2,) + self.shape:
            raise ValueError('us must have shape (2,) + plan shape')
        code = warp_mode_code(mode)
        out = np.empty((2,) + self.shape, dtype=self.rdtype)
        check(self.lib.gpa_invert_u_mode(self.handle, _ptr(us), int(iters), int(edge), 0, code, _ptr(out)),
              'gpa_invert_u_mode')
        return out

    def reconstruct_grad(self, lockins, kvecs, mask_border):
        lockins = np.ascontiguousarray(lockins, dtype=self.cdtype)
        kvecs = _f64(kvecs).reshape(-1, 2)
        n0, n1 = self.shape
        dudx = np.empty((2, n0, n1 - 1), dtype=self.rdtype)
        dudy = np.empty((2, n0 - 1, n1), dtype=self.rdtype)
        wnorm = np.empty((n0, n1), dtype=self.rdtype)
        check(self.lib.gpa_reconstruct_grad(self.handle, _ptr(lockins), _ptr(kvecs), len(kvecs), int(mask_border),
                                            _ptr(dudx), _ptr(dudy), _ptr(wnorm)), 'gpa_reconstruct_grad')
        return dudx, dudy, wnorm

    def weighted_lstsq(self, b, weights, kvecs):
        b = np.ascontiguousarray(b, dtype=self.rdtype)
        weights = np.ascontiguousarray(weights, dtype=self.rdtype)
        kvecs = _f64(kvecs).reshape(-1, 2)
        if b.shape != (len(kvecs),) + self.shape or weights.shape != b.shape:
            raise ValueError('b / weights must have shape (P,) + plan shape')
        out = np.empty((2,) + self.shape, dtype=self.rdtype)
        check(self.lib.gpa_weighted_lstsq(self.handle, _ptr(b), _ptr(weights), _ptr(kvecs), len(kvecs), _ptr(out)),
              'gpa_weighted_lstsq')
        return out

    def invert_u_overlap(self, us, iters=35, edge=0, mode='nearest'):
        """invert_u_overlap of the reference, (2, n0 + 2 edge, n1 + 2 edge); mode as in invert_u.  Only 'constant' ends on a
        cval = nan round: the folded modes 'reflect' / 'mirror' / 'grid-wrap' give every coordinate a value"""
        us = np.ascontiguousarray(us, dtype=self.rdtype)
        if us.shape != (2,) + self.shape:
            raise ValueError('us must have shape (2,) + plan shape')
        code = warp_mode_code(mode)
        out = np.empty((2, self.shape[0] + 2 * edge, self.shape[1] + 2 * edge), dtype=self.rdtype)
        check(self.lib.gpa_invert_u_mode(self.handle, _ptr(us), int(iters), int(edge), 1, code, _ptr(out)),
              'gpa_invert_u_mode')
        return out

    def undistort_image(self, deformed, u):
        deformed = self._img(deformed)
        u = np.ascontiguousarray(u, dtype=self.rdtype)
        if u.shape != (2,) + self.shape:
            raise ValueError('u must have shape (2,) + plan shape')
        out = np.empty(self.shape, dtype=self.rdtype)
        check(self.lib.gpa_undistort_image(self.handle, _ptr(deformed), _ptr(u), _ptr(out)), 'gpa_undistort_image')
        return out

    def undistort_image_stack(self, frames, u, chunk=None):
        """undistort_image of every frame of `frames` (B, n0, n1) in one library call per `chunk` frames (default and
        upper limit: the 65535 frames a call takes).  u: (2, n0, n1), one field for all frames -- inverted once per call --
        or (B, 2, n0, n1), a field per frame.  Returns (B, n0, n1); frame b equals undistort_image(frames[b], u or u[b])
        bitwise."""
        frames, u = np.asarray(frames), np.asarray(u)
        B, per_frame = stack_shapes(frames.shape, u.shape, self.shape)
        chunk = UNDISTORT_MAX_FRAMES if chunk is None else max(1, min(int(chunk), UNDISTORT_MAX_FRAMES))
        if not per_frame:
            u = np.ascontiguousarray(u, dtype=self.rdtype)
        out = np.empty((B,) + self.shape, dtype=self.rdtype)
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            fr = np.ascontiguousarray(frames[b0:b0 + nb], dtype=self.rdtype)
            uu = np.ascontiguousarray(u[b0:b0 + nb], dtype=self.rdtype) if per_frame else u
            check(self.lib.gpa_undistort_image_batch(self.handle, _ptr(fr), nb, _ptr(uu), int(per_frame), _ptr(out[b0:b0 + nb])),
                  'gpa_undistort_image_batch')
        return out

    def undistort_image_batch_dev(self, frames_ptr, nframes, u_ptr, out_ptr, per_frame=False, scale=1.0, uinv_ptr=None):
        """undistort_image(frames[b], scale * u) of nframes plan-shaped frames (contiguous) on device pointers, enqueued on the
        plan's stream (no host sync).  per_frame False: u is one field (2 x n0 x n1) for all frames; True: nframes fields
        (nframes x 2 x n0 x n1), e.g. the output of extract_displacement_field_batch_dev with scale = -1.  uinv_ptr receives
        u_inv in the layout of u.  nframes: 1 .. 65535"""
        check(self.lib.gpa_undistort_image_batch_dev(self.handle, _ptr(int(frames_ptr)), int(nframes), _ptr(int(u_ptr)),
                                                     int(bool(per_frame)), float(scale), _ptr(uinv_ptr), _ptr(int(out_ptr))),
              'gpa_undistort_image_batch_dev')

    # ---- unit-cell averaging / expansion (unit_cell_averaging.py); geom: a UcellGeom -------------------------
    def unit_cell_average(self, image, geom, u=None, want_weights=False):
        """res (and weights) of unit_cell_average: rsize float64 arrays whatever the plan's precision"""
        image = self._img(image)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=self.rdtype)
            if u.shape != (2,) + self.shape:
                raise ValueError('u must have shape (2,) + plan shape')
        rs = tuple(geom.rsize)
        res = np.empty(rs, dtype=np.float64)
        w = np.empty(rs, dtype=np.float64) if want_weights else None
        check(self.lib.gpa_unit_cell_average(self.handle, _ptr(image), _ptr(u), C.byref(geom), _ptr(res), _ptr(w)),
              'gpa_unit_cell_average')
        return (res, w) if want_weights else res

    def unit_cell_average_dev(self, images_ptr, geom, res_ptr, u_ptr=None, weights_ptr=None, nframes=1):
        """unit_cell_average of nframes plan-shaped frames (contiguous) sharing u, on device pointers, enqueued on the plan's
        stream; res / weights: nframes x rsize doubles"""
        check(self.lib.gpa_unit_cell_average_batch_dev(self.handle, _ptr(int(images_ptr)), int(nframes),
                                                       _ptr(u_ptr), C.byref(geom),
                                                       _ptr(int(res_ptr)), _ptr(weights_ptr)),
              'gpa_unit_cell_average_batch_dev')

    def expand_unitcell(self, cell, geom, z2=1, u=None):
        """expand_unitcell onto the plan's grid: cell is rsize (taken as float64), out is plan-shaped in the plan's dtype"""
        cell = np.ascontiguousarray(cell, dtype=np.float64)
        if cell.shape != tuple(geom.rsize):
            raise ValueError('cell shape %s does not match rsize %s' % (cell.shape, tuple(geom.rsize)))
        if u is not None:
            u = np.ascontiguousarray(u, dtype=self.rdtype)
            if u.shape != (2,) + self.shape:
                raise ValueError('u must have shape (2,) + plan shape')
        out = np.empty(self.shape, dtype=self.rdtype)
        check(self.lib.gpa_expand_unitcell(self.handle, _ptr(cell), C.byref(geom), float(z2), _ptr(u), _ptr(out)),
              'gpa_expand_unitcell')
        return out

    def expand_unitcell_dev(self, cell_ptr, geom, out_ptr, z2=1, u_ptr=None):
        check(self.lib.gpa_expand_unitcell_dev(self.handle, _ptr(int(cell_ptr)), C.byref(geom), float(z2),
                                               _ptr(u_ptr), _ptr(int(out_ptr))),
              'gpa_expand_unitcell_dev')

    # ---- windowed Fourier filtering (geometric_phase_analysis.py:551-580) ----------------------------------
    def wff(self, image, sigma, wxs, wys, thresholds, scale):
        """gpa_wff: the filtered fields of up to WFF_MAX_T thresholds, (T,) + shape complex in the plan's precision; image is
        taken as complex, wxs / wys are the frequency lists along axis 1 / axis 0"""
        image = np.ascontiguousarray(image, dtype=self.cdtype)
        if image.shape != self.shape:
            raise ValueError('image shape %s does not match the plan %s' % (image.shape, self.shape))
        wxs, wys, thr = _f64(wxs).ravel(), _f64(wys).ravel(), _f64(thresholds).ravel()
        out = np.empty((len(thr),) + self.shape, dtype=self.cdtype)
        check(self.lib.gpa_wff(self.handle, _ptr(image), float(sigma), _ptr(wxs), len(wxs), _ptr(wys), len(wys), _ptr(thr),
                               len(thr), float(scale), _ptr(out)), 'gpa_wff')
        return out

    def wff_dev(self, image_ptr, out_ptr, sigma, wxs, wys, thresholds, scale):
        """gpa_wff_dev: image_ptr -> n0 x n1 complex, out_ptr -> T x n0 x n1 complex, both on the device in the plan's precision
        and not overlapping; enqueued on the plan's stream"""
        wxs, wys, thr = _f64(wxs).ravel(), _f64(wys).ravel(), _f64(thresholds).ravel()
        check(self.lib.gpa_wff_dev(self.handle, _ptr(int(image_ptr)), float(sigma), _ptr(wxs), len(wxs), _ptr(wys), len(wys),
                                   _ptr(thr), len(thr), float(scale), _ptr(int(out_ptr))), 'gpa_wff_dev')

    # ---- image preparation (imagetools.py:92-194) ----------------------------------------------------------
    def _mask(self, mask):
        """a mask as a C-contiguous uint8 plane of 0 / 1, by truth value (0.5 and 256 are true)"""
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != self.shape:
            raise ValueError('mask shape %s does not match the plan %s' % (mask.shape, self.shape))
        return mask

    @staticmethod
    def _nan_scale(nan_scale):
        return (0, 0.0) if nan_scale is None else (1, float(nan_scale))

    def gauss_homogenize(self, image, mask, sigma, nan_scale=None, want_vv=False):
        """gpa_gauss_homogenize: image / VV with VV the masked Gaussian average; mask is taken by truth value.  Returns out,
        or (out, VV) with want_vv"""
        image, mask = self._img(image), self._mask(mask)
        out = np.empty(self.shape, dtype=self.rdtype)
        vv = np.empty(self.shape, dtype=self.rdtype) if want_vv else None
        use, ns = self._nan_scale(nan_scale)
        check(self.lib.gpa_gauss_homogenize(self.handle, _ptr(image), _ptr(mask), float(sigma), use, ns, _ptr(out), _ptr(vv)),
              'gpa_gauss_homogenize')
        return (out, vv) if want_vv else out

    def gauss_homogenize_dev(self, image_ptr, mask_ptr, out_ptr, sigma, nan_scale=None, vv_ptr=None):
        """gpa_gauss_homogenize_dev: image_ptr / out_ptr / vv_ptr (optional) -> n0 x n1 reals of the plan's precision, mask_ptr ->
        n0 x n1 bytes, all on the device; out and vv overlap neither image nor mask; enqueued on the plan's stream"""
        use, ns = self._nan_scale(nan_scale)
        check(self.lib.gpa_gauss_homogenize_dev(self.handle, _ptr(int(image_ptr)), _ptr(int(mask_ptr)), float(sigma), use, ns,
                                                _ptr(int(out_ptr)), None if vv_ptr is None else _ptr(int(vv_ptr))),
              'gpa_gauss_homogenize_dev')

    def mask_any_equal(self, frames, value, hit=None):
        """gpa_mask_any_equal: hit | any(frames == value, axis=0) as a uint8 plane; frames (B, n0, n1), compared in the plan's
        precision; hit: the plane of an earlier chunk, or None"""
        frames = np.ascontiguousarray(frames, dtype=self.rdtype)
        if frames.ndim != 3 or frames.shape[0] < 1 or frames.shape[1:] != self.shape:
            raise ValueError('frames must be (B >= 1,) + %s, not %s' % (self.shape, frames.shape))
        acc = hit is not None
        hit = self._mask(hit).copy() if acc else np.empty(self.shape, dtype=np.uint8)
        check(self.lib.gpa_mask_any_equal(self.handle, _ptr(frames), len(frames), float(value), int(acc), _ptr(hit)),
              'gpa_mask_any_equal')
        return hit

    def mask_any_equal_dev(self, frames_ptr, B, value, hit_ptr, accumulate=False):
        check(self.lib.gpa_mask_any_equal_dev(self.handle, _ptr(int(frames_ptr)), int(B), float(value), int(bool(accumulate)),
                                              _ptr(int(hit_ptr))), 'gpa_mask_any_equal_dev')

    def mask_erode_disk(self, mask, r, invert=False):
        """gpa_mask_erode_disk: binary_erosion(~mask if invert else mask, disk(r)) as a uint8 plane"""
        mask = self._mask(mask)
        out = np.empty(self.shape, dtype=np.uint8)
        check(self.lib.gpa_mask_erode_disk(self.handle, _ptr(mask), int(bool(invert)), int(r), _ptr(out)), 'gpa_mask_erode_disk')
        return out

    def mask_erode_disk_dev(self, in_ptr, out_ptr, r, invert=False):
        check(self.lib.gpa_mask_erode_disk_dev(self.handle, _ptr(int(in_ptr)), int(bool(invert)), int(r), _ptr(int(out_ptr))),
              'gpa_mask_erode_disk_dev')

    def mask_bounds(self, mask):
        """gpa_mask_bounds: int32 [first row, last row + 1, first column, last column + 1] holding a true sample"""
        lims = np.empty(4, dtype=np.int32)
        check(self.lib.gpa_mask_bounds(self.handle, _ptr(self._mask(mask)), _ptr(lims)), 'gpa_mask_bounds')
        return lims

    def mask_bounds_dev(self, mask_ptr):
        lims = np.empty(4, dtype=np.int32)
        check(self.lib.gpa_mask_bounds_dev(self.handle, _ptr(int(mask_ptr)), _ptr(lims)), 'gpa_mask_bounds_dev')
        return lims

    def nan_lines(self, image):
        """gpa_nan_lines: (rows, cols) bool arrays, True where every sample of the line is NaN"""
        rows, cols = np.empty(self.shape[0], dtype=np.uint8), np.empty(self.shape[1], dtype=np.uint8)
        check(self.lib.gpa_nan_lines(self.handle, _ptr(self._img(image)), _ptr(rows), _ptr(cols)), 'gpa_nan_lines')
        return rows.astype(bool), cols.astype(bool)

    def nan_lines_dev(self, image_ptr):
        rows, cols = np.empty(self.shape[0], dtype=np.uint8), np.empty(self.shape[1], dtype=np.uint8)
        check(self.lib.gpa_nan_lines_dev(self.handle, _ptr(int(image_ptr)), _ptr(rows), _ptr(cols)), 'gpa_nan_lines_dev')
        return rows.astype(bool), cols.astype(bool)

    def nan_trim_lims(self, image):
        """gpa_nan_trim_lims: int32 [x0, x1, y0, y1], the window the loop of trim_nans2 ends with"""
        lims = np.empty(4, dtype=np.int32)
        check(self.lib.gpa_nan_trim_lims(self.handle, _ptr(self._img(image)), _ptr(lims)), 'gpa_nan_trim_lims')
        return lims

    def nan_trim_lims_dev(self, image_ptr):
        lims = np.empty(4, dtype=np.int32)
        check(self.lib.gpa_nan_trim_lims_dev(self.handle, _ptr(int(image_ptr)), _ptr(lims)), 'gpa_nan_trim_lims_dev')
        return lims

    # ---- per-line medians, homogenize_per_axis (imagetools.py:112-125) -------------------------------------
    def _mask_or_none(self, mask):
        return None if mask is None else self._mask(mask)

    def line_nanmedian(self, image, axis, mask=None, propagate_nan=False):
        """gpa_line_nanmedian: np.nanmedian(where(mask, image, nan), axis) (np.median with propagate_nan) as a 1-D array of
        the plan's precision: n1 column medians for axis 0, n0 row medians for axis 1"""
        image, mask = self._img(image), self._mask_or_none(mask)
        out = np.empty(self.shape[1 - int(axis)] if int(axis) in (0, 1) else 1, dtype=self.rdtype)
        check(self.lib.gpa_line_nanmedian(self.handle, _ptr(image), _ptr(mask), int(axis), int(bool(propagate_nan)), _ptr(out)),
              'gpa_line_nanmedian')
        return out

    def line_nanmedian_dev(self, image_ptr, mask_ptr, axis, out_ptr, propagate_nan=False):
        """gpa_line_nanmedian_dev: device pointers (mask_ptr may be None); enqueued on the plan's stream"""
        check(self.lib.gpa_line_nanmedian_dev(self.handle, _ptr(int(image_ptr)), None if mask_ptr is None else _ptr(int(mask_ptr)),
                                              int(axis), int(bool(propagate_nan)), _ptr(int(out_ptr))), 'gpa_line_nanmedian_dev')

    def homogenize_per_axis(self, frames, sigma, mask=None, propagate_nan=False, want_profiles=False):
        """gpa_homogenize_per_axis of one image (n0, n1) or a stack (B, n0, n1) sharing `mask`, in one device call.  Returns out,
        or (out, profile0, profile1) with want_profiles: the filtered profiles along axis 0 ((B,) n1 values) and axis 1 ((B,) n0)"""
        frames = np.ascontiguousarray(frames, dtype=self.rdtype)
        single = frames.ndim == 2
        if frames.ndim not in (2, 3) or frames.shape[-2:] != self.shape or frames.shape[0] < 1:
            raise ValueError('frames %s do not match the plan %s' % (frames.shape, self.shape))
        nb = 1 if single else frames.shape[0]
        mask = self._mask_or_none(mask)
        out = np.empty(frames.shape, dtype=self.rdtype)
        prof = np.empty((nb, self.shape[1] + self.shape[0]), dtype=self.rdtype) if want_profiles else None
        check(self.lib.gpa_homogenize_per_axis(self.handle, _ptr(frames), _ptr(mask), float(sigma), int(bool(propagate_nan)), nb,
                                               _ptr(out), _ptr(prof)), 'gpa_homogenize_per_axis')
        if not want_profiles:
            return out
        p0, p1 = prof[:, :self.shape[1]].copy(), prof[:, self.shape[1]:].copy()
        return (out, p0[0], p1[0]) if single else (out, p0, p1)

    def homogenize_per_axis_dev(self, image_ptr, mask_ptr, out_ptr, sigma, propagate_nan=False, nb=1, profiles_ptr=None):
        """gpa_homogenize_per_axis_dev: image_ptr / out_ptr -> nb x n0 x n1 reals of the plan's precision, mask_ptr (or None) ->
        n0 x n1 bytes, profiles_ptr (or None) -> nb x (n1 + n0) reals, all on the device; enqueued on the plan's stream"""
        check(self.lib.gpa_homogenize_per_axis_dev(self.handle, _ptr(int(image_ptr)), None if mask_ptr is None else _ptr(int(mask_ptr)),
                                                   float(sigma), int(bool(propagate_nan)), int(nb), _ptr(int(out_ptr)),
                                                   None if profiles_ptr is None else _ptr(int(profiles_ptr))),
              'gpa_homogenize_per_axis_dev')

    def homogenize_lines(self, image, sigma, line0, line1=None, want_profiles=False):
        """gpa_homogenize_lines: the filter and the divisions of homogenize_per_axis with the reduced lines given (line0: n1
        values, line1: n0 values or None for the image after axis 0 alone)"""
        image = self._img(image)
        line0 = np.ascontiguousarray(line0, dtype=self.rdtype).ravel()
        if line0.size != self.shape[1]:
            raise ValueError('line0 needs %d values' % self.shape[1])
        if line1 is not None:
            line1 = np.ascontiguousarray(line1, dtype=self.rdtype).ravel()
            if line1.size != self.shape[0]:
                raise ValueError('line1 needs %d values' % self.shape[0])
        out = np.empty(self.shape, dtype=self.rdtype)
        prof = np.empty(self.shape[1] + (0 if line1 is None else self.shape[0]), dtype=self.rdtype) if want_profiles else None
        check(self.lib.gpa_homogenize_lines(self.handle, _ptr(image), float(sigma), _ptr(line0), _ptr(line1), _ptr(out), _ptr(prof)),
              'gpa_homogenize_lines')
        if not want_profiles:
            return out
        return out, prof[:self.shape[1]].copy(), (None if line1 is None else prof[self.shape[1]:].copy())

    def homogenize_lines_dev(self, image_ptr, sigma, line0_ptr, line1_ptr, out_ptr, profiles_ptr=None):
        check(self.lib.gpa_homogenize_lines_dev(self.handle, _ptr(int(image_ptr)), float(sigma), _ptr(int(line0_ptr)),
                                                None if line1_ptr is None else _ptr(int(line1_ptr)), _ptr(int(out_ptr)),
                                                None if profiles_ptr is None else _ptr(int(profiles_ptr))), 'gpa_homogenize_lines_dev')

    @staticmethod
    def _rects(rects):
        """None, one (r0, c0, h, w) or a list of them -> (ctypes int array or None, count)"""
        if rects is None:
            return None, 0
        flat = np.asarray(rects, dtype=np.int64).reshape(-1)
        if flat.size % 4:
            raise ValueError('rects: (r0, c0, h, w) per window')
        return (C.c_int * flat.size)(*[int(v) for v in flat]), flat.size // 4

    def invert_u_dev(self, u_ptr, out_ptr, scale=1.0, iters=35, edge=0, overlap=True, mode='nearest', rects=None):
        """invert_u_overlap / invert_u of scale * u on device pointers, enqueued on the plan's stream (no host sync);
        rects = (r0, c0, h, w) or a list of such windows: only those parts of the output grid are computed.  mode: as in
        invert_u (an unknown one raises NotImplementedError)"""
        code = warp_mode_code(mode)
        arr, n = self._rects(rects)
        check(self.lib.gpa_invert_u_mode_dev(self.handle, _ptr(int(u_ptr)), float(scale), int(iters), int(edge), int(bool(overlap)),
                                             code, arr, n, _ptr(int(out_ptr))), 'gpa_invert_u_mode_dev')

    def undistort_image_dev(self, deformed_ptr, u_ptr, out_ptr, uinv_ptr=None, rects=None, scale=1.0):
        """undistort_image(deformed, scale * u) on device pointers, enqueued on the plan's stream (no host sync); uinv_ptr
        (2 x n0 x n1) receives u_inv = invert_u_overlap(-scale * u); rects = (r0, c0, h, w) or a list: only those windows of the
        outputs are computed.  scale = -1: u is the field as extract_displacement_field returns it (minus the displacement)"""
        arr, n = self._rects(rects)
        check(self.lib.gpa_undistort_image_scaled_dev(self.handle, _ptr(int(deformed_ptr)), _ptr(int(u_ptr)), float(scale), arr, n,
                                                      _ptr(uinv_ptr), _ptr(int(out_ptr))),
              'gpa_undistort_image_dev')

    def phasegradient2J(self, kvecs, grads, weights, nmperpixel, dks=None):
        kvecs = _f64(kvecs).reshape(-1, 2)
        grads = np.ascontiguousarray(grads, dtype=self.rdtype)
        weights = np.ascontiguousarray(weights, dtype=self.rdtype)
        if grads.shape != (len(kvecs),) + self.shape + (2,) or weights.shape != grads.shape[:-1]:
            raise ValueError('grads must be (P,) + plan shape + (2,), weights (P,) + plan shape')
        dks = None if dks is None else _f64(dks).reshape(len(kvecs), 2)
        J = np.empty(self.shape + (2, 2), dtype=self.rdtype)
        check(self.lib.gpa_phasegradient2J(self.handle, _ptr(kvecs), len(kvecs), _ptr(grads), _ptr(weights),
                                           float(nmperpixel), _ptr(dks), _ptr(J)), 'gpa_phasegradient2J')
        return J

    # ---- device-pointer forms of the rows after the path (f-2, f-4): nothing leaves HBM -----------------------------
    def sweep_grad_dev(self, image_ptr, kref, klist, sigma, lockin_ptr, grad_ptr, kidx_ptr=None, grad_mode=0):
        """wfr2_grad_opt of one peak on device pointers: lockin (n0 x n1 complex), grad (n0 x n1 x 2), optional kidx"""
        kref = _f64(kref).reshape(2)
        klist = _f64(klist).reshape(-1, 2)
        check(self.lib.gpa_sweep_grad_dev(self.handle, _ptr(int(image_ptr)), _ptr(kref), _ptr(klist), len(klist), float(sigma),
                                          int(grad_mode), _ptr(int(lockin_ptr)),
                                          _ptr(kidx_ptr), _ptr(int(grad_ptr))),
              'gpa_sweep_grad_dev')

    def lockin_batch_dev(self, image_ptr, kvecs, sigma, out_ptr):
        """lockin_batch on device pointers: image n0 x n1 reals (its mean is NOT subtracted), out len(kvecs) x n0 x n1 complex;
        enqueued on the plan's stream"""
        kvecs = _f64(kvecs).reshape(-1, 2)
        check(self.lib.gpa_lockin_batch_dev(self.handle, _ptr(int(image_ptr)), _ptr(kvecs), len(kvecs), float(sigma),
                                            _ptr(int(out_ptr))), 'gpa_lockin_batch_dev')

    def lockin_weights_dev(self, lockins_ptr, P, weights_ptr):
        """np.abs of P lock-ins on the device"""
        check(self.lib.gpa_lockin_weights_dev(self.handle, _ptr(int(lockins_ptr)), int(P), _ptr(int(weights_ptr))),
              'gpa_lockin_weights_dev')

    def phasegradient2J_dev(self, kvecs, grads_ptr, weights_ptr, nmperpixel, J_ptr, dks=None):
        """phasegradient2J on device pointers: grads (P x n0 x n1 x 2), weights (P x n0 x n1) -> J (n0 x n1 x 2 x 2)"""
        kvecs = _f64(kvecs).reshape(-1, 2)
        dks = None if dks is None else _f64(dks).reshape(len(kvecs), 2)
        check(self.lib.gpa_phasegradient2J_dev(self.handle, _ptr(kvecs), len(kvecs), _ptr(int(grads_ptr)),
                                               _ptr(int(weights_ptr)), float(nmperpixel), _ptr(dks), _ptr(int(J_ptr))),
              'gpa_phasegradient2J_dev')

    def props_from_jac_dev(self, jac_ptr, props_ptr, add_identity=False, refangle=0., refscale=1., diff=False):
        """props_from_Jac on device pointers (n0 x n1 x 2 x 2 -> 4 x n0 x n1), on the plan's stream"""
        check(self.lib.gpa_props_from_jac_dev(self.device, self.code, self.shape[0] * self.shape[1], _ptr(int(jac_ptr)),
                                              int(bool(add_identity)), float(refangle), float(refscale), int(bool(diff)),
                                              _ptr(int(props_ptr)), _ptr(self.stream())), 'gpa_props_from_jac_dev')

    def fit_plane_dev(self, image_ptr, max_iter=200, tol=1e-12):
        coef = (C.c_double * 3)()
        iters = C.c_int(0)
        check(self.lib.gpa_fit_plane_dev(self.handle, _ptr(int(image_ptr)), int(max_iter), float(tol), coef, C.byref(iters)),
              'gpa_fit_plane_dev')
        return np.array(coef[:]), iters.value

    def fit_plane(self, image, max_iter=200, tol=1e-12):
        image = self._img(image)
        coef = (C.c_double * 3)()
        iters = C.c_int(0)
        check(self.lib.gpa_fit_plane(self.handle, _ptr(image), int(max_iter), float(tol), coef, C.byref(iters)),
              'gpa_fit_plane')
        return np.array(coef[:]), iters.value

    def fit_planes_dev(self, images_ptr, P, max_iter=200, tol=1e-12):
        """fit_plane_dev of P contiguous plan-shaped planes on the device, one synchronisation per IRLS round for all of them:
        (coef (P, 3), passes (P,)); plane q gets the bits fit_plane_dev gives for it alone"""
        P = int(P)
        coef = np.empty((P, 3), dtype=np.float64)
        iters = np.zeros(P, dtype=np.int32)
        check(self.lib.gpa_fit_planes_dev(self.handle, _ptr(int(images_ptr)), P, int(max_iter), float(tol), _ptr(coef), _ptr(iters)),
              'gpa_fit_planes_dev')
        return coef, iters

    def lockin_polar_crop_dev(self, lockins_ptr, P, edge, psi_ptr, amp_ptr, amax_ptr, weight_ptr=None):
        """P device lock-ins on the plan's grid -> np.angle / np.abs of the window [edge:-edge, edge:-edge] as compact planes
        (psi, amp: P x m0 x m1 reals), amax (P reals) = amp[p].max() over the window, weight (optional) = sqrt(amp / amax[p]);
        enqueued on the plan's stream"""
        check(self.lib.gpa_lockin_polar_crop_dev(self.handle, _ptr(int(lockins_ptr)), int(P), int(edge), _ptr(int(psi_ptr)),
                                                 _ptr(int(amp_ptr)), _ptr(weight_ptr), _ptr(int(amax_ptr))),
              'gpa_lockin_polar_crop_dev')

    def _iterate_args(self, kvecs, edge, iters, crop_plan):
        """(kvecs (P, 2), P, window shape, crop handle, corr, delta_ks, unwrap_iters) of an iterate_gpa call"""
        kvecs = _f64(kvecs).reshape(-1, 2)
        P, edge, iters = len(kvecs), int(edge), int(iters)
        if iters < 0 or edge < 0 or 2 * edge >= min(self.shape) - 1:
            raise ValueError('iterate_gpa: need iters >= 0 and 0 <= 2 * edge < min(shape) - 1')
        win = (self.shape[0] - 2 * edge, self.shape[1] - 2 * edge)
        handle = None if crop_plan is None else crop_plan.handle
        return (kvecs, P, win, handle, np.zeros((P, 2)), np.zeros((iters, P, 2)), np.zeros((iters + 1, P), dtype=np.int32))

    def iterate_gpa(self, image, kvecs, sigma, edge=5, iters=3, kmax_iter=25, kmax=200, crop_plan=None):
        """iterate_GPA of the reference in one library call (gpa_iterate_gpa).  image: the plan's shape, its mean already
        subtracted; crop_plan: a Plan of the window's shape (n - 2 * edge per axis), the same dtype and device -- edge = 0
        does without.  Returns (prs, w, corr, delta_ks, unwrap_iters): the final unwrapped phases and amplitudes
        (P, m0, m1), the correction (P, 2), what each pass subtracted from it (iters, P, 2) and the unwraps' iteration
        counts (iters + 1, P)."""
        image = self._img(image)
        kvecs, P, win, crop, corr, delta_ks, uit = self._iterate_args(kvecs, edge, iters, crop_plan)
        prs = np.empty((P,) + win, dtype=self.rdtype)
        w = np.empty((P,) + win, dtype=self.rdtype)
        check(self.lib.gpa_iterate_gpa(self.handle, crop, _ptr(image), _ptr(kvecs), P, float(sigma), int(edge), int(iters),
                                       int(kmax_iter), int(kmax), _ptr(prs), _ptr(w), _ptr(corr), _ptr(delta_ks), _ptr(uit)),
              'gpa_iterate_gpa')
        return prs, w, corr, delta_ks, uit

    def iterate_gpa_dev(self, image_ptr, kvecs, sigma, prs_ptr, w_ptr, edge=5, iters=3, kmax_iter=25, kmax=200, crop_plan=None):
        """iterate_gpa on device pointers: image n0 x n1, prs / w P x m0 x m1 of the plan's dtype.  Returns (corr, delta_ks,
        unwrap_iters); the call has finished when it returns"""
        kvecs, P, win, crop, corr, delta_ks, uit = self._iterate_args(kvecs, edge, iters, crop_plan)
        check(self.lib.gpa_iterate_gpa_dev(self.handle, crop, _ptr(int(image_ptr)), _ptr(kvecs), P, float(sigma), int(edge),
                                           int(iters), int(kmax_iter), int(kmax), _ptr(int(prs_ptr)), _ptr(int(w_ptr)),
                                           _ptr(corr), _ptr(delta_ks), _ptr(uit)), 'gpa_iterate_gpa_dev')
        return corr, delta_ks, uit

    def find_peaks(self, image, sigma, dog_sigma, threshold_rel, want_smooth=False, max_out=4096):
        """peak_local_max candidates of the smoothed spectrum: (coords (n, 2) int, values (n,)) sorted like
        skimage (highest first, raster order among equals) [, smooth]."""
        image = self._img(image)
        smooth = np.empty(self.shape, dtype=self.rdtype) if want_smooth else None
        tried_full = False
        while True:
            coords = np.empty((max_out, 2), dtype=np.int32)
            vals = np.empty(max_out, dtype=self.rdtype)
            count = C.c_int(0)
            check(self.lib.gpa_find_peaks(self.handle, _ptr(image), float(sigma), float(dog_sigma), float(threshold_rel),
                                          int(max_out), _ptr(coords), _ptr(vals), C.byref(count), _ptr(smooth)),
                  'gpa_find_peaks')
            if count.value <= max_out or tried_full:
                break
            max_out, tried_full = count.value, True   # (the library caps max_out at its buffer size)
        n = min(count.value, max_out)
        coords, vals = coords[:n], vals[:n]
        order = np.lexsort((coords[:, 1], coords[:, 0], -vals))
        out = (coords[order].astype(np.intp), vals[order])
        return out + (smooth,) if want_smooth else out

    def find_peaks_dev(self, image_ptr, sigma, dog_sigma, threshold_rel, smooth_ptr=None, max_out=4096):
        """find_peaks on a device image (not modified); the candidate list comes back to the host, the smoothed spectrum
        (optional) stays on the device"""
        coords = np.empty((max_out, 2), dtype=np.int32)
        vals = np.empty(max_out, dtype=self.rdtype)
        count = C.c_int(0)
        check(self.lib.gpa_find_peaks_dev(self.handle, _ptr(int(image_ptr)), float(sigma), float(dog_sigma),
                                          float(threshold_rel), int(max_out), _ptr(coords), _ptr(vals), C.byref(count),
                                          _ptr(smooth_ptr)), 'gpa_find_peaks_dev')
        if count.value > max_out:
            # the first max_out candidates in the device's atomic-append order are an arbitrary subset: fetch them all from
            # the smoothed spectrum the plan now holds, as find_peaks retries
            return self.find_peaks_again(threshold_rel, max_out=count.value)
        n = min(count.value, max_out)
        coords, vals = coords[:n], vals[:n]
        order = np.lexsort((coords[:, 1], coords[:, 0], -vals))
        return coords[order].astype(np.intp), vals[order]

    def find_peaks_again(self, threshold_rel, max_out=4096):
        """the candidates of the smoothed spectrum of the LAST find_peaks / find_peaks_dev call at another threshold"""
        tried_full = False
        while True:
            coords = np.empty((max_out, 2), dtype=np.int32)
            vals = np.empty(max_out, dtype=self.rdtype)
            count = C.c_int(0)
            check(self.lib.gpa_find_peaks_again(self.handle, float(threshold_rel), int(max_out), _ptr(coords), _ptr(vals),
                                                C.byref(count)), 'gpa_find_peaks_again')
            if count.value <= max_out or tried_full:
                break
            max_out, tried_full = count.value, True
        n = min(count.value, max_out)
        coords, vals = coords[:n], vals[:n]
        order = np.lexsort((coords[:, 1], coords[:, 0], -vals))
        return coords[order].astype(np.intp), vals[order]

    def per_dft_dev(self, image_ptr, out_ptr):
        """per_dft on device pointers (n0 x n1 reals in, n0 x n1 complex out), enqueued on the plan's stream"""
        check(self.lib.gpa_per_dft_dev(self.handle, _ptr(int(image_ptr)), _ptr(int(out_ptr))), 'gpa_per_dft_dev')

    def gaussian_deconvolve_dev(self, data_ptr, dr, sigma, balance, out_ptr):
        """gaussian_deconvolve of one m0 x m1 device field (this plan: the padded shape); out_ptr may equal data_ptr"""
        check(self.lib.gpa_gaussian_deconvolve_dev(self.handle, _ptr(int(data_ptr)), int(dr), float(sigma), float(balance),
                                                   _ptr(int(out_ptr))), 'gpa_gaussian_deconvolve_dev')

    def gaussian_deconvolve(self, data, dr, sigma, balance):
        """one m0 x m1 field; this plan has the padded shape (m0 + 4 dr, m1 + 4 dr)"""
        data = np.ascontiguousarray(data, dtype=self.rdtype)
        if data.shape != (self.shape[0] - 4 * dr, self.shape[1] - 4 * dr):
            raise ValueError('data shape %s does not match the padded plan %s' % (data.shape, self.shape))
        out = np.empty(data.shape, dtype=self.rdtype)
        check(self.lib.gpa_gaussian_deconvolve(self.handle, _ptr(data), int(dr), float(sigma), float(balance), _ptr(out)),
              'gpa_gaussian_deconvolve')
        return out

    def per_dft(self, image):
        image = self._img(image)
        out = np.empty(self.shape, dtype=self.cdtype)
        check(self.lib.gpa_per_dft(self.handle, _ptr(image), _ptr(out)), 'gpa_per_dft')
        return out

    def per(self, image, inverse_dft=True):
        """moisan2011.per: (p, s) real for inverse_dft=True, their DFTs (p_hat, s_hat) otherwise"""
        image = self._img(image)
        dt = self.rdtype if inverse_dft else self.cdtype
        pc, sc = np.empty(self.shape, dtype=dt), np.empty(self.shape, dtype=dt)
        check(self.lib.gpa_per(self.handle, _ptr(image), 1 if inverse_dft else 0, _ptr(pc), _ptr(sc)), 'gpa_per')
        return pc, sc

    def unwrap_prediff(self, dx, dy, weight=None, kmax=100, eps=1e-9, axes_compat=True):
        n0, n1 = self.shape
        dx = np.ascontiguousarray(dx, dtype=self.rdtype)
        dy = np.ascontiguousarray(dy, dtype=self.rdtype)
        if dx.shape != (n0, n1 - 1) or dy.shape != (n0 - 1, n1):
            raise ValueError('dx/dy shapes %s %s do not match the plan %s' % (dx.shape, dy.shape, self.shape))
        w = None if weight is None else self._img(weight)
        phi = np.empty((n0, n1), dtype=self.rdtype)
        iters = C.c_int(0)
        check(self.lib.gpa_unwrap_prediff(self.handle, _ptr(dx), _ptr(dy), _ptr(w), int(kmax), float(eps),
                                          1 if axes_compat else 0, _ptr(phi), C.byref(iters)), 'gpa_unwrap_prediff')
        return phi, iters.value

    def unwrap(self, psi, weight=None, kmax=100, eps=1e-9, axes_compat=True):
        psi = self._img(psi)
        w = None if weight is None else self._img(weight)
        phi = np.empty(self.shape, dtype=self.rdtype)
        iters = C.c_int(0)
        check(self.lib.gpa_unwrap(self.handle, _ptr(psi), _ptr(w), int(kmax), float(eps), 1 if axes_compat else 0,
                                  _ptr(phi), C.byref(iters)), 'gpa_unwrap')
        return phi, iters.value

    def unwrap_dev(self, psi_ptr, weight_ptr, phi_ptr, kmax=100, eps=1e-9, axes_compat=True):
        """unwrap on device pointers (psi, weight or None, phi: plan-shaped, phi apart from the inputs); returns the iteration
        count, i.e. waits for the solve"""
        iters = C.c_int(0)
        check(self.lib.gpa_unwrap_dev(self.handle, _ptr(int(psi_ptr)), _ptr(weight_ptr), int(kmax), float(eps),
                                      1 if axes_compat else 0, _ptr(int(phi_ptr)), C.byref(iters)), 'gpa_unwrap_dev')
        return iters.value

    def _stack_weight(self, weight, B):
        """(array or None, weight_planes) of a stack call: None, one plan-shaped plane, or B of them"""
        if weight is None:
            return None, 0
        planes = unwrap_stack_weight_planes(np.shape(weight), B, self.shape)
        return np.ascontiguousarray(weight, dtype=self.rdtype), planes

    def _stack_out(self, out, B):
        phi = out if out is not None else np.empty((B,) + tuple(self.shape), self.rdtype)
        if phi.shape != (B,) + tuple(self.shape) or phi.dtype != self.rdtype or not phi.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous (B, n0, n1) array of the plan dtype')
        return phi

    def _unwrap_stack_run(self, planes, weight, kmax, eps, axes_compat, out):
        """planes: (psis,) or (dxs, dys), checked and converted.  The stack in calls of at most UNWRAP_BATCH_MAX problems;
        shapes without a batched unwrap (asked once: gpa_supports_batch) loop over the single call."""
        B = planes[0].shape[0]
        w, _ = self._stack_weight(weight, B)
        phi = self._stack_out(out, B)
        iters = np.zeros(B, dtype=np.int64)
        prediff = len(planes) == 2
        if not self.lib.gpa_supports_batch(self.handle):
            single = self.unwrap_prediff if prediff else self.unwrap
            for b in range(B):
                wb = None if w is None else (w if w.ndim == 2 else w[b])
                phi[b], iters[b] = single(*[a[b] for a in planes], wb, kmax=kmax, eps=eps, axes_compat=axes_compat)
            return phi, iters
        fn = self.lib.gpa_unwrap_prediff_batch if prediff else self.lib.gpa_unwrap_batch
        for c0 in range(0, B, UNWRAP_BATCH_MAX):
            n = min(UNWRAP_BATCH_MAX, B - c0)
            it = (C.c_int * n)()
            own = w is not None and w.ndim == 3     # (B, n0, n1): one plane per map
            wc = None if w is None else (w[c0:c0 + n] if own else w)
            wp = 0 if w is None else (n if own else 1)
            check(fn(self.handle, *[_ptr(a[c0:c0 + n]) for a in planes], n, _ptr(wc), wp, int(kmax), float(eps),
                     1 if axes_compat else 0, _ptr(phi[c0:c0 + n]), it),
                  'gpa_unwrap_prediff_batch' if prediff else 'gpa_unwrap_batch')
            iters[c0:c0 + n] = it[:]
        return phi, iters

    def unwrap_stack(self, psis, weight=None, kmax=100, eps=1e-9, axes_compat=True, out=None):
        """B wrapped phase maps (B, n0, n1) in one device call: (phi (B, n0, n1), iters (B,)).  weight: None, one
        (n0, n1) plane for all maps or (B, n0, n1), one each.  Map b's phi and count are those of unwrap() on it."""
        B = unwrap_stack_shapes(np.shape(psis), None, self.shape)
        psis = np.ascontiguousarray(psis, dtype=self.rdtype)
        return self._unwrap_stack_run((psis,), weight, kmax, eps, axes_compat, out)

    def unwrap_prediff_stack(self, dxs, dys, weight=None, kmax=100, eps=1e-9, axes_compat=True, out=None):
        """the same from pre-differenced gradients: dxs (B, n0, n1 - 1), dys (B, n0 - 1, n1)"""
        B = unwrap_stack_shapes(np.shape(dxs), np.shape(dys), self.shape)
        dxs = np.ascontiguousarray(dxs, dtype=self.rdtype)
        dys = np.ascontiguousarray(dys, dtype=self.rdtype)
        return self._unwrap_stack_run((dxs, dys), weight, kmax, eps, axes_compat, out)

    def unwrap_batch_dev(self, psi_ptr, nb, weight_ptr, weight_planes, phi_ptr, kmax=100, eps=1e-9, axes_compat=True,
                         want_iters=True):
        """device pointers (psi nb x n0 x n1, weight weight_planes x n0 x n1 or None with 0, phi nb x n0 x n1 apart from
        the inputs).  Returns the nb iteration counts, or None without waiting when want_iters is False (pair with
        unwrap_batch_finish)"""
        it = (C.c_int * max(1, int(nb)))() if want_iters else None
        check(self.lib.gpa_unwrap_batch_dev(self.handle, _ptr(psi_ptr), int(nb), _ptr(weight_ptr), int(weight_planes), int(kmax),
                                            float(eps), 1 if axes_compat else 0, _ptr(phi_ptr), it), 'gpa_unwrap_batch_dev')
        return None if it is None else np.array(it[:int(nb)], dtype=np.int64)

    def unwrap_prediff_batch_dev(self, dx_ptr, dy_ptr, nb, weight_ptr, weight_planes, phi_ptr, kmax=100, eps=1e-9,
                                 axes_compat=True, want_iters=True):
        """unwrap_batch_dev from gradients: dx nb x n0 x (n1 - 1), dy nb x (n0 - 1) x n1"""
        it = (C.c_int * max(1, int(nb)))() if want_iters else None
        check(self.lib.gpa_unwrap_prediff_batch_dev(self.handle, _ptr(dx_ptr), _ptr(dy_ptr), int(nb), _ptr(weight_ptr),
                                                    int(weight_planes), int(kmax), float(eps), 1 if axes_compat else 0,
                                                    _ptr(phi_ptr), it), 'gpa_unwrap_prediff_batch_dev')
        return None if it is None else np.array(it[:int(nb)], dtype=np.int64)

    def unwrap_batch_finish(self, nb):
        """waits for the plan's stream; the nb iteration counts of the last unwrap_*batch_dev call"""
        it = (C.c_int * max(1, int(nb)))()
        check(self.lib.gpa_unwrap_batch_finish(self.handle, int(nb), it), 'gpa_unwrap_batch_finish')
        return np.array(it[:int(nb)], dtype=np.int64)

    def unwrap_batch_problem_bytes(self, kmax=100):
        """device bytes of one problem of a stack unwrap (UNWRAP_STACK_BYTES divided by this is the chunk of a call)"""
        return int(self.lib.gpa_unwrap_batch_problem_bytes(self.handle, int(kmax)))

    def extract_displacement_field(self, image, kvecs, klists, sigma, mask_border, kmax=10,
                                   want_lockins=False, want_kidx=False, out=None, want_grads=False, want_weights=False,
                                   grad_mode=0):
        """The fused driver on host arrays: (u, lockins, kidx, iters).  want_grads / want_weights: the same sweep also gives
        the winners' phase gradients (P, n0, n1, 2; stencil `grad_mode` as in sweep) and |lockins| (P, n0, n1) -- the return
        value is then the 6-tuple (u, lockins, kidx, iters, grads, weights), with None for what was not asked for."""
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        if out is not None and (out.shape != (2,) + self.shape or out.dtype != self.rdtype or not out.flags.c_contiguous):
            raise ValueError('out must be a C-contiguous (2,) + plan shape array of the plan dtype')
        one_sweep = bool(want_grads or want_weights)
        if not want_lockins and not want_kidx and not one_sweep and self.shape[0] * self.shape[1] >= 512 * 512:
            return self._extract_host_pipelined(image, kvecs, klists, sigma, mask_border, kmax, out)
        u = out if out is not None else np.empty((2,) + self.shape, dtype=self.rdtype)
        image = self._img(image)
        lock = np.empty((P,) + self.shape, dtype=self.cdtype) if want_lockins else None
        kidx = np.empty((P,) + self.shape, dtype=np.int32) if want_kidx else None
        grads = np.empty((P,) + self.shape + (2,), dtype=self.rdtype) if want_grads else None
        absw = np.empty((P,) + self.shape, dtype=self.rdtype) if want_weights else None
        iters = (C.c_int * 2)()
        self._extract_call('', image, (kvecs, P, klists, K), sigma, mask_border, kmax, u, lock, kidx, grads, absw, grad_mode, iters)
        res = (u, lock, kidx, (iters[0], iters[1]))
        return res + (grads, absw) if one_sweep else res

    def _extract_call(self, form, image, lists, sigma, mask_border, kmax, u, lockins, kidx, grads, absw, grad_mode, iters=None):
        """the one library call of a driver method, gpa_extract_displacement_field<form> -- its _grad variant (which also takes
        grad_mode, grads and absw) if and only if grads or absw is asked for.  lists: what _peak_lists returns; the arrays or
        addresses are host or device ones as `form` takes them; iters: the (C.c_int * 2) of a synchronising form"""
        kvecs, P, klists, K = lists
        name = 'gpa_extract_displacement_field'
        args = [self.handle, _ptr(image), _ptr(kvecs), P, _ptr(klists), K, float(sigma), int(mask_border), int(kmax)]
        outs = [_ptr(u), _ptr(lockins), _ptr(kidx)]
        if grads is not None or absw is not None:
            name += '_grad'
            args.append(int(grad_mode))
            outs += [_ptr(grads), _ptr(absw)]
        if iters is not None:
            outs.append(iters)
        name += form
        check(getattr(self.lib, name)(*args, *outs), name)

    def _extract_host_pipelined(self, image, kvecs, klists, sigma, mask_border, kmax, out):
        """The host-array form of the driver with its host work overlapped.  A 4096^2 f32 call spent 18 of its 29 ms on
        the host: `astype` of the image into a fresh array (8.6 ms) and page-faulting a fresh 128 MB result array
        during the download (8 ms).  Here the image is converted into a staging array kept by the plan (resident
        pages: 4.3 ms), the device work is enqueued asynchronously, the result array is allocated and touched WHILE the
        GPU computes, and the download lands in resident pages (2.4 ms).  (Several host threads for the conversion and
        the first touch were tried and dropped: on the 256-core box the pages end up on other NUMA nodes and the
        copies slow down by more than the threads save.)"""
        image = np.asarray(image)
        if image.shape != self.shape:
            raise ValueError('image shape %s does not match the plan %s' % (image.shape, self.shape))
        npx = self.shape[0] * self.shape[1]
        item = np.dtype(self.rdtype).itemsize
        if getattr(self, '_d_img', None) is None:
            self._d_img, self._d_u = DeviceBuffer(npx * item, self.device), DeviceBuffer(2 * npx * item, self.device)
        if image.dtype == self.rdtype and image.flags.c_contiguous:
            src = image
        else:
            if getattr(self, '_stage', None) is None:
                self._stage = np.empty(self.shape, dtype=self.rdtype)
            src = self._stage
            np.copyto(src, image, casting='unsafe')
        self._d_img.upload(src)
        self.extract_displacement_field_async(self._d_img.ptr, kvecs, klists, sigma, mask_border, kmax, self._d_u.ptr)
        if out is None:
            out = np.empty((2,) + self.shape, dtype=self.rdtype)
            out.fill(0)                    # first touch while the GPU computes
        iters = self.last_iters()          # waits for the device
        self._d_u.download_into(out)
        return out, None, None, iters

    def extract_gradients(self, image, kvecs, klists, sigma, mask_border):
        image = self._img(image)
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        n0, n1 = self.shape
        dudx = np.empty((2, n0, n1 - 1), dtype=self.rdtype)
        dudy = np.empty((2, n0 - 1, n1), dtype=self.rdtype)
        wnorm = np.empty((n0, n1), dtype=self.rdtype)
        check(self.lib.gpa_extract_gradients(self.handle, _ptr(image), _ptr(kvecs), P, _ptr(klists), K,
                                             float(sigma), int(mask_border), _ptr(dudx), _ptr(dudy), _ptr(wnorm)),
              'gpa_extract_gradients')
        return dudx, dudy, wnorm

    # ---- device-pointer entry points (ints from torch.Tensor.data_ptr()) -----
    def mean_dev(self, ptr, count):
        out = C.c_double(0.0)
        check(self.lib.gpa_mean_dev(self.handle, _ptr(int(ptr)), int(count), C.byref(out)), 'gpa_mean_dev')
        return out.value

    def tile_gradients_dev(self, image_ptr, image_pitch, r0, c0, mean, kvecs, klists, sigma, mask_border,
                           interior, dx, dy, wn):
        """interior = (i0, j0, t0, t1); dx, dy = (ptr, pitch, plane), wn = (ptr, pitch); element units."""
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        i0, j0, t0, t1 = (int(v) for v in interior)
        check(self.lib.gpa_tile_gradients_dev(self.handle, _ptr(int(image_ptr)), int(image_pitch), int(r0), int(c0),
                                              float(mean), _ptr(kvecs), P, _ptr(klists), K, float(sigma),
                                              int(mask_border), i0, j0, t0, t1, _ptr(int(dx[0])), int(dx[1]), int(dx[2]),
                                              _ptr(int(dy[0])), int(dy[1]), int(dy[2]), _ptr(int(wn[0])), int(wn[1])),
              'gpa_tile_gradients_dev')

    def tile_sums_dev(self, wins_ptr, win_stride, win_pitch, rects_dev_ptr, ntiles, max_rows, sum_dev_ptr):
        """sum over the interior rectangles (device table of (o0, o1, z0, z1)) of ntiles windows -> one double on the device"""
        check(self.lib.gpa_tile_sums_dev(self.handle, _ptr(int(wins_ptr)), int(win_stride), int(win_pitch),
                                         _ptr(int(rects_dev_ptr)), int(ntiles), int(max_rows), _ptr(int(sum_dev_ptr))),
              'gpa_tile_sums_dev')

    def tile_set_mean_dev(self, sum_dev_ptr, scale):
        check(self.lib.gpa_tile_set_mean_dev(self.handle, _ptr(int(sum_dev_ptr)), float(scale)), 'gpa_tile_set_mean_dev')

    def tile_gradients_meandev_dev(self, image_ptr, image_pitch, r0, c0, kvecs, klists, sigma, mask_border, interior, dx, dy, wn):
        """tile_gradients_dev with the mean of gpa_tile_set_mean_dev; wn = (ptr, pitch, plane): plane != 0 writes the
        weight twice (plane elements apart)"""
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        i0, j0, t0, t1 = (int(v) for v in interior)
        check(self.lib.gpa_tile_gradients_meandev_dev(self.handle, _ptr(int(image_ptr)), int(image_pitch), int(r0), int(c0),
                                                      _ptr(kvecs), P, _ptr(klists), K, float(sigma),
                                                      int(mask_border), i0, j0, t0, t1, _ptr(int(dx[0])), int(dx[1]), int(dx[2]),
                                                      _ptr(int(dy[0])), int(dy[1]), int(dy[2]), _ptr(int(wn[0])), int(wn[1]),
                                                      int(wn[2])),
              'gpa_tile_gradients_meandev_dev')

    def stitch_tiles_dev(self, tiles_ptr, slot_stride, field_stride, tile_pitch, table_dev_ptr, ntiles, t0, t1, dst):
        """dst: list of (device pointer, pitch, rows, cols) per field (<= 6); one launch on the plan's stream"""
        nf = len(dst)
        ptrs = (C.c_void_p * nf)(*[int(d[0]) for d in dst])
        pitch = (C.c_size_t * nf)(*[int(d[1]) for d in dst])
        rows = (C.c_int * nf)(*[int(d[2]) for d in dst])
        cols = (C.c_int * nf)(*[int(d[3]) for d in dst])
        check(self.lib.gpa_stitch_tiles_dev(self.handle, _ptr(int(tiles_ptr)), int(slot_stride), int(field_stride),
                                            int(tile_pitch), _ptr(int(table_dev_ptr)), int(ntiles), int(t0), int(t1), nf,
                                            ptrs, pitch, rows, cols), 'gpa_stitch_tiles_dev')

    def stream(self):
        """the plan's main stream (raw hipStream_t as an int)"""
        return int(self.lib.gpa_plan_stream(self.handle) or 0)

    def wait_stream(self, stream):
        """the plan's stream waits for what has been enqueued on `stream` (raw hipStream_t as an int, 0 = default)"""
        check(self.lib.gpa_plan_wait_stream(self.handle, C.c_void_p(int(stream))), 'gpa_plan_wait_stream')

    def stream_wait(self, stream):
        """`stream` waits for what has been enqueued on the plan's stream"""
        check(self.lib.gpa_stream_wait_plan(self.handle, C.c_void_p(int(stream))), 'gpa_stream_wait_plan')

    def unwrap_prediff_dev(self, dx_ptr, dy_ptr, weight_ptr, phi_ptr, kmax=100, eps=1e-9, axes_compat=True):
        iters = C.c_int(0)
        check(self.lib.gpa_unwrap_prediff_dev(self.handle, _ptr(int(dx_ptr)), _ptr(int(dy_ptr)),
                                              _ptr(weight_ptr), int(kmax), float(eps),
                                              int(bool(axes_compat)), _ptr(int(phi_ptr)), C.byref(iters)),
              'gpa_unwrap_prediff_dev')
        return iters.value

    def unwrap_prediff_enqueue_dev(self, dx_ptr, dy_ptr, weight_ptr, phi_ptr, kmax=100, eps=1e-9, axes_compat=True):
        """the solve of unwrap_prediff_dev put on the plan's stream without waiting for it (unwrap_finish does)"""
        check(self.lib.gpa_unwrap_prediff_enqueue_dev(self.handle, _ptr(int(dx_ptr)), _ptr(int(dy_ptr)),
                                                      _ptr(weight_ptr), int(kmax),
                                                      float(eps), int(bool(axes_compat)), _ptr(int(phi_ptr))),
              'gpa_unwrap_prediff_enqueue_dev')

    def unwrap_finish(self):
        iters = C.c_int(0)
        check(self.lib.gpa_unwrap_finish(self.handle, C.byref(iters)), 'gpa_unwrap_finish')
        return iters.value

    def extract_displacement_field_dev(self, image_ptr, kvecs, klists, sigma, mask_border, kmax, u_ptr,
                                       lockins_ptr=None, kidx_ptr=None, grads_ptr=None, weights_ptr=None, grad_mode=0):
        """device pointers; grads_ptr (P x n0 x n1 x 2) / weights_ptr (P x n0 x n1): the winners' phase gradients and
        |lockins| from the same sweep (gpa_extract_displacement_field_grad_dev); without them the plain driver is called"""
        iters = (C.c_int * 2)()
        self._extract_call('_dev', image_ptr, _peak_lists(kvecs, klists), sigma, mask_border, kmax, u_ptr, lockins_ptr, kidx_ptr,
                           grads_ptr, weights_ptr, grad_mode, iters)
        return iters[0], iters[1]

    def extract_displacement_field_async(self, image_ptr, kvecs, klists, sigma, mask_border, kmax, u_ptr,
                                         lockins_ptr=None, kidx_ptr=None, grads_ptr=None, weights_ptr=None, grad_mode=0):
        """enqueue only; pair with sync() / last_iters()"""
        self._extract_call('_async', image_ptr, _peak_lists(kvecs, klists), sigma, mask_border, kmax, u_ptr, lockins_ptr,
                           kidx_ptr, grads_ptr, weights_ptr, grad_mode)

    def extract_displacement_field_batch_dev(self, images_ptr, nimages, kvecs, klists, sigma, mask_border, kmax, u_ptr,
                                             want_iters=True):
        """a stack of `nimages` images (device pointers: images nimages x n0 x n1, u nimages x 2 x n0 x n1): sweeps
        image after image, the 2 * nimages unwraps in one set of launches.  Returns the (nimages, 2) iteration counts,
        or None without synchronising when want_iters is False (pair with sync())"""
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        it = (C.c_int * (2 * int(nimages)))() if want_iters else None
        check(self.lib.gpa_extract_displacement_field_batch_dev(self.handle, _ptr(images_ptr), int(nimages), _ptr(kvecs), P,
                                                                _ptr(klists), K, float(sigma), int(mask_border),
                                                                int(kmax), _ptr(u_ptr), it),
              'gpa_extract_displacement_field_batch_dev')
        return None if it is None else np.array(it[:], dtype=np.int64).reshape(int(nimages), 2)

    def extract_displacement_field_grad_batch_dev(self, images_ptr, nimages, kvecs, klists, sigma, mask_border, kmax, u_ptr,
                                                  lockins_ptr=None, kidx_ptr=None, grads_ptr=None, weights_ptr=None, grad_mode=0,
                                                  want_iters=True):
        """extract_displacement_field_batch_dev with the optional outputs of extract_displacement_field_dev, one leading frame
        axis each (device pointers): lockins nimages x P x n0 x n1 complex, kidx the same in int32, grads nimages x P x n0 x n1 x 2,
        weights nimages x P x n0 x n1.  With none of them the launches are those of extract_displacement_field_batch_dev."""
        kvecs, P, klists, K = _peak_lists(kvecs, klists)
        it = (C.c_int * (2 * int(nimages)))() if want_iters else None
        check(self.lib.gpa_extract_displacement_field_grad_batch_dev(self.handle, _ptr(images_ptr), int(nimages), _ptr(kvecs), P,
                                                                     _ptr(klists), K, float(sigma), int(mask_border), int(kmax),
                                                                     int(grad_mode), _ptr(u_ptr), _ptr(lockins_ptr), _ptr(kidx_ptr),
                                                                     _ptr(grads_ptr), _ptr(weights_ptr), it),
              'gpa_extract_displacement_field_grad_batch_dev')
        return None if it is None else np.array(it[:], dtype=np.int64).reshape(int(nimages), 2)

    def extract_displacement_field_stack(self, images, kvecs, klists, sigma, mask_border, kmax=10, chunk=None, out=None,
                                         want_lockins=False, want_kidx=False, want_grads=False, want_weights=False, grad_mode=0,
                                         out_lockins=None, out_kidx=None, out_grads=None, out_weights=None):
        """host arrays: images (B, n0, n1) -> u (B, 2, n0, n1) (written into `out` if given) and the (B, 2)
        iteration counts, through extract_displacement_field_batch_dev.  The stack goes through the GPU in chunks of
        `chunk` frames (default: ~16 Mpixel per chunk) on two sets of device buffers: while the GPU works on chunk i a
        host thread uploads chunk i + 1 and another downloads chunk i - 1 (PCIe is full duplex, plain hipMemcpy on the
        default stream does not wait for the plan's non-blocking streams, ctypes releases the GIL).
        want_lockins / want_kidx / want_grads / want_weights (or an out_* buffer to write into): the per-frame outputs of
        extract_displacement_field with a leading frame axis, from the same sweep (extract_displacement_field_grad_batch_dev);
        the return value is then (u, iters, lockins, kidx, grads, weights) with None for what was not asked for.  The default
        chunk shrinks by what a frame adds to u's two reals per pixel, so a chunk's outputs stay near the same budget."""
        from concurrent.futures import ThreadPoolExecutor
        images = np.asarray(images)
        if images.ndim != 3 or images.shape[1:] != tuple(self.shape):
            raise ValueError('images must be (B, %d, %d)' % tuple(self.shape))
        B = images.shape[0]
        npx = int(self.shape[0]) * int(self.shape[1])
        item = np.dtype(self.rdtype).itemsize
        P = len(_peak_lists(kvecs, klists)[0])
        # name -> (asked for, caller's buffer, shape after the frame axis, dtype)
        extras = {'lockins': (want_lockins, out_lockins, (P,) + tuple(self.shape), self.cdtype),
                  'kidx': (want_kidx, out_kidx, (P,) + tuple(self.shape), np.int32),
                  'grads': (want_grads, out_grads, (P,) + tuple(self.shape) + (2,), self.rdtype),
                  'weights': (want_weights, out_weights, (P,) + tuple(self.shape), self.rdtype)}
        extras = {k: v for k, v in extras.items() if v[0] or v[1] is not None}
        if extras:
            return self._extract_stack_outputs(images, kvecs, klists, sigma, mask_border, kmax, chunk, out, extras, grad_mode)
        if chunk is None:
            chunk = max(1, min(B, (16 << 20) // npx))
        chunk = int(max(1, min(chunk, B, 4096)))     # the batched driver takes at most 4096 frames per call
        nchunks = -(-B // chunk)
        # (a plain array: page-locking hundreds of MB costs more than it saves -- 104 ms for 256 MB on the MI355X box,
        #  where hipMemcpy into pageable memory runs at ~50 GB/s anyway; pass out= to reuse a buffer)
        u = out if out is not None else np.empty((B, 2) + tuple(self.shape), self.rdtype)
        if u.shape != (B, 2) + tuple(self.shape) or u.dtype != self.rdtype or not u.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous (B, 2, n0, n1) array of the plan dtype')
        iters = np.zeros((B, 2), dtype=np.int64)
        d_img = [DeviceBuffer(chunk * npx * item, self.device) for _ in range(min(2, nchunks))]
        d_u = [DeviceBuffer(2 * chunk * npx * item, self.device) for _ in range(min(2, nchunks))]
        bounds = [(c * chunk, min(B, (c + 1) * chunk)) for c in range(nchunks)]
        batched = bool(self.lib.gpa_supports_batch(self.handle))   # asked once, not discovered per chunk from an error text

        def upload(c):
            a, b = bounds[c]
            d_img[c % 2].upload(np.ascontiguousarray(images[a:b], dtype=self.rdtype))

        def download(c):
            a, b = bounds[c]
            d_u[c % 2].download_into(u[a:b])

        try:
            with ThreadPoolExecutor(1) as up_pool, ThreadPoolExecutor(1) as dn_pool:
                ups = {0: up_pool.submit(upload, 0)}
                dns = {}
                for c in range(nchunks):
                    ups[c].result()                       # chunk c is on the device
                    if c - 2 in dns:
                        dns.pop(c - 2).result()           # its u buffer has been read out
                    a, b = bounds[c]
                    if batched:
                        self.extract_displacement_field_batch_dev(d_img[c % 2].ptr, b - a, kvecs, klists, sigma, mask_border,
                                                                  kmax, d_u[c % 2].ptr, want_iters=False)
                    else:
                        # shapes without a batched unwrap (sides no fused path covers): the same frames one call each --
                        # the numbers the docstring promises, just without the shared launch chain
                        for f in range(b - a):
                            iters[a + f] = self.extract_displacement_field_dev(d_img[c % 2].ptr + f * npx * item, kvecs, klists, sigma,
                                                                               mask_border, kmax, d_u[c % 2].ptr + 2 * f * npx * item)
                    if c + 1 < nchunks:                    # (its image buffer was last read by chunk c - 1: done, see sync below)
                        ups[c + 1] = up_pool.submit(upload, c + 1)
                    if batched:
                        iters[a:b] = self._batch_iters(b - a)   # synchronises: chunk c is finished
                    dns[c] = dn_pool.submit(download, c)
                for f in dns.values():
                    f.result()
        finally:
            for buf in d_img + d_u:
                buf.free()
        return u, iters

    def _extract_stack_outputs(self, images, kvecs, klists, sigma, mask_border, kmax, chunk, out, extras, grad_mode):
        """extract_displacement_field_stack with optional outputs: the same upload / compute / download pipeline on two sets of
        device buffers, every output of a chunk downloaded by the download thread.  extras: name -> (asked, buffer, shape, dtype)"""
        from concurrent.futures import ThreadPoolExecutor
        B = images.shape[0]
        npx = int(self.shape[0]) * int(self.shape[1])
        item = np.dtype(self.rdtype).itemsize
        shapes = {'u': ((2,) + tuple(self.shape), np.dtype(self.rdtype))}
        host = {'u': out}
        for k, (_, buf, sh, dt) in extras.items():
            shapes[k] = (sh, np.dtype(dt))
            host[k] = buf
        for k, (sh, dt) in shapes.items():
            if host[k] is None:
                host[k] = np.empty((B,) + sh, dt)
            elif host[k].shape != (B,) + sh or host[k].dtype != dt or not host[k].flags.c_contiguous:
                raise ValueError('out%s must be a C-contiguous %s array of dtype %s' % ('' if k == 'u' else '_' + k, (B,) + sh, dt))
        frame_bytes = {k: int(np.prod(sh)) * dt.itemsize for k, (sh, dt) in shapes.items()}
        if chunk is None:   # today's budget: 16 Mpixel of u per chunk
            chunk = max(1, min(B, (16 << 20) * 2 * item // sum(frame_bytes.values())))
        chunk = int(max(1, min(chunk, B, 4096)))
        nchunks = -(-B // chunk)
        iters = np.zeros((B, 2), dtype=np.int64)
        nbuf = min(2, nchunks)
        d_img = [DeviceBuffer(chunk * npx * item, self.device) for _ in range(nbuf)]
        d_out = [{k: DeviceBuffer(chunk * nb, self.device) for k, nb in frame_bytes.items()} for _ in range(nbuf)]
        bounds = [(c * chunk, min(B, (c + 1) * chunk)) for c in range(nchunks)]
        batched = bool(self.lib.gpa_supports_batch(self.handle))

        def upload(c):
            a, b = bounds[c]
            d_img[c % 2].upload(np.ascontiguousarray(images[a:b], dtype=self.rdtype))

        def download(c):
            a, b = bounds[c]
            for k, buf in d_out[c % 2].items():
                buf.download_into(host[k][a:b])

        def ptrs(c, f=0):
            d = d_out[c % 2]
            return [d[k].ptr + f * frame_bytes[k] if k in d else None for k in ('u', 'lockins', 'kidx', 'grads', 'weights')]

        try:
            with ThreadPoolExecutor(1) as up_pool, ThreadPoolExecutor(1) as dn_pool:
                ups = {0: up_pool.submit(upload, 0)}
                dns = {}
                for c in range(nchunks):
                    ups[c].result()                       # chunk c is on the device
                    if c - 2 in dns:
                        dns.pop(c - 2).result()           # its output buffers have been read out
                    a, b = bounds[c]
                    if batched:
                        u_p, l_p, k_p, g_p, w_p = ptrs(c)
                        self.extract_displacement_field_grad_batch_dev(d_img[c % 2].ptr, b - a, kvecs, klists, sigma, mask_border, kmax,
                                                                       u_p, l_p, k_p, g_p, w_p, grad_mode, want_iters=False)
                    else:   # shapes without a batched unwrap: the same frames one call each
                        for f in range(b - a):
                            u_p, l_p, k_p, g_p, w_p = ptrs(c, f)
                            iters[a + f] = self.extract_displacement_field_dev(d_img[c % 2].ptr + f * npx * item, kvecs, klists, sigma,
                                                                               mask_border, kmax, u_p, l_p, k_p, g_p, w_p, grad_mode)
                    if c + 1 < nchunks:
                        ups[c + 1] = up_pool.submit(upload, c + 1)
                    if batched:
                        iters[a:b] = self._batch_iters(b - a)   # synchronises: chunk c is finished
                    dns[c] = dn_pool.submit(download, c)
                for f in dns.values():
                    f.result()
        finally:
            for buf in d_img + [b for d in d_out for b in d.values()]:
                buf.free()
        return (host['u'], iters) + tuple(host.get(k) for k in ('lockins', 'kidx', 'grads', 'weights'))

    def _batch_iters(self, nimages):
        it = (C.c_int * (2 * int(nimages)))()
        check(self.lib.gpa_last_batch_iters(self.handle, int(nimages), it), 'gpa_last_batch_iters')
        return np.array(it[:], dtype=np.int64).reshape(int(nimages), 2)

    def last_iters(self):
        it = (C.c_int * 2)()
        check(self.lib.gpa_last_iters(self.handle, it), 'gpa_last_iters')
        return it[0], it[1]

    def timer_start(self):
        check(self.lib.gpa_timer_start(self.handle), 'gpa_timer_start')

    def timer_stop(self):
        ms = C.c_float(0)
        check(self.lib.gpa_timer_stop(self.handle, C.byref(ms)), 'gpa_timer_stop')
        return ms.value

    def set_profiling(self, on):
        check(self.lib.gpa_set_profiling(self.handle, 1 if on else 0), 'gpa_set_profiling')

    def last_kernel_profile(self):
        """{kernel name: (launches, total ms)} of the last profiled fused-driver call"""
        buf = C.create_string_buffer(1 << 16)
        check(self.lib.gpa_last_kernel_profile(self.handle, buf, len(buf)), 'gpa_last_kernel_profile')
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.rsplit(' ', 2)
            out[name] = (int(calls), float(ms))
        return out

    def last_passb_skips(self):
        """(skipped, visited): the (row, candidate) pairs the shared pass B of the last profiled sweep skipped by its spectral
        bound, and all it visited"""
        sk, vi = C.c_longlong(0), C.c_longlong(0)
        check(self.lib.gpa_last_passb_skips(self.handle, C.byref(sk), C.byref(vi)), 'gpa_last_passb_skips')
        return sk.value, vi.value

    def download_async(self, host_array, dev_ptr, slot):
        """enqueue the D2H copy of host_array.nbytes from dev_ptr into the (page-locked) host_array"""
        check(self.lib.gpa_download_async(self.handle, _ptr(host_array), _ptr(int(dev_ptr)), host_array.nbytes, int(slot)),
              'gpa_download_async')

    def download_wait(self, slot):
        check(self.lib.gpa_download_wait(self.handle, int(slot)), 'gpa_download_wait')

    def last_stage_ms(self):
        ms = (C.c_float * 5)()
        check(self.lib.gpa_last_stage_ms(self.handle, ms), 'gpa_last_stage_ms')
        return [ms[i] for i in range(5)]


class DeviceBuffer:
    """A raw device allocation through the HIP runtime (hipMalloc / hipMemcpy via ctypes) for
    callers of the `_dev` / `_async` entry points that do not want torch for it."""
    _hip = None

    def __init__(self, nbytes, device=0):
        """`device`: the GPU the memory lives on.  hipMalloc / hipMemcpy act on the calling THREAD's current device, so
        every method selects it first (a plan on GPU 1 used from a thread whose current device is 0 -- the default of
        every new thread, e.g. the upload / download workers of the stack call -- would otherwise allocate on GPU 0
        and hand the plan's kernels a pointer they cannot reach)."""
        load()
        if DeviceBuffer._hip is None:
            DeviceBuffer._hip = C.CDLL('libamdhip64.so')   # already mapped as a dependency of libgpa_hip.so
        self.device = int(device)
        self._select()
        p = C.c_void_p()
        rc = self._hip.hipMalloc(C.byref(p), C.c_size_t(int(nbytes)))
        if rc != 0 or not p.value:
            raise GPAError('hipMalloc(%d) on device %d failed (%d)' % (nbytes, self.device, rc))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def _select(self):
        rc = self._hip.hipSetDevice(C.c_int(self.device))
        if rc != 0:
            raise GPAError('hipSetDevice(%d) failed (%d)' % (self.device, rc))

    def upload(self, host):
        host = np.ascontiguousarray(host)
        self._select()
        if self._hip.hipMemcpy(C.c_void_p(self.ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) != 0:
            raise GPAError('hipMemcpy H2D failed')

    def upload_at(self, host, byte_offset):
        """H2D of `host` to ptr + byte_offset (a large buffer filled piece by piece)"""
        host = np.ascontiguousarray(host)
        if byte_offset < 0 or byte_offset + host.nbytes > self.nbytes:
            raise ValueError('upload_at: outside the buffer')
        self._select()
        if self._hip.hipMemcpy(C.c_void_p(self.ptr + int(byte_offset)), host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) != 0:
            raise GPAError('hipMemcpy H2D failed')

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._select()
        if self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), 2) != 0:
            raise GPAError('hipMemcpy D2H failed')
        return out

    def download_into(self, out):
        """copy the first out.nbytes bytes into the (C-contiguous) array `out`"""
        if not out.flags.c_contiguous:
            raise ValueError('destination must be C-contiguous')
        self._select()
        if self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), 2) != 0:
            raise GPAError('hipMemcpy D2H failed')

    def free(self):
        if getattr(self, 'ptr', None):
            self._hip.hipSetDevice(C.c_int(self.device))
            self._hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64):
    """NumPy array in page-locked host memory (hipHostMalloc).  The host-pointer entry points copy
    from / to such arrays at full PCIe rate (about 4x the rate of pageable memory); use it for images
    and pass it as `out=` where offered.  Freed when the array (and every view of it) is collected."""
    import weakref
    load()
    if DeviceBuffer._hip is None:
        DeviceBuffer._hip = C.CDLL('libamdhip64.so')
    hip = DeviceBuffer._hip
    dtype = np.dtype(dtype)
    nbytes = max(int(np.prod(shape)) * dtype.itemsize, 1)
    ptr = C.c_void_p()
    rc = hip.hipHostMalloc(C.byref(ptr), C.c_size_t(nbytes), C.c_uint(0))
    if rc != 0 or not ptr.value:
        raise GPAError('hipHostMalloc(%d) failed (%d)' % (nbytes, rc))
    buf = (C.c_char * nbytes).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, hip.hipHostFree, C.c_void_p(ptr.value))
    return arr


# small plan cache so the drop-in functions do not rebuild tables on every call
_plans = {}


def get_plan(shape, batch, dtype=np.float64, device=0):
    key = (int(shape[0]), int(shape[1]), np.dtype(dtype).name, int(device))
    p = _plans.get(key)
    if p is None or p.max_batch < batch:
        # evicted plans are only dropped from the cache: a caller may still hold one, and
        # Plan.__del__ releases the device memory with the last reference
        if len(_plans) >= 4 and key not in _plans:
            _plans.pop(next(iter(_plans)))
        p = Plan(shape, max(int(batch), 1), dtype, device)
        _plans[key] = p
    return p


def props_from_jac(jac, add_identity=False, refangle=0., refscale=1., diff=False, dtype=np.float64, device=0):
    """Plan-free f-2 entry: jac (..., 2, 2) -> props (4, ...)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64')
    jac = np.ascontiguousarray(jac, dtype=dtype)
    if jac.shape[-2:] != (2, 2):
        raise ValueError('jac must have shape (..., 2, 2)')
    lead = jac.shape[:-2]
    props = np.empty((4,) + lead, dtype=dtype)
    check(load().gpa_props_from_jac(int(device), 0 if dtype == np.float32 else 1, jac.size // 4, _ptr(jac),
                                    int(bool(add_identity)), float(refangle), float(refscale), int(bool(diff)),
                                    _ptr(props)), 'gpa_props_from_jac')
    return props


def _kerelsky_args(x0, a0, max_nfev, retry_cost, dtype):
    """the checked scalar arguments of gpa_kerelsky_fit[_dev]: (dtype code, x0, a0 or None, max_nfev, retry_cost)"""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64')
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    if x0.shape != (4,) or not np.isfinite(x0).all():
        raise ValueError('x0 must be four finite numbers (theta, psi, epsilon, xi)')
    if x0[0] < 0 or x0[2] < 0:
        raise ValueError('x0 must respect the bounds theta >= 0 and epsilon >= 0')
    if a0 is not None:
        a0 = np.ascontiguousarray(a0, dtype=np.float64)
        if a0.shape != (2, 2) or not np.isfinite(a0).all():
            raise ValueError('a0 must be a finite 2 x 2 matrix')
    if int(max_nfev) != max_nfev or int(max_nfev) < 1:
        raise ValueError('max_nfev must be an integer >= 1')
    if np.isnan(retry_cost):
        raise ValueError('retry_cost must not be NaN')
    return GPA_F32 if dtype == np.float32 else GPA_F64, x0, a0, int(max_nfev), float(retry_cost)


def kerelsky_fit(jac, x0, a0=None, max_nfev=50, retry_cost=1e-5, dtype=np.float64, device=0):
    """Plan-free per-pixel Kerelsky fits (gpa_kerelsky_fit): jac (..., 2, 2) -- J when a0 (2 x 2) is given, else A itself -- and
    the start x0 -> (X (..., 4) in the dtype, cost (...) in f64)."""
    code, x0, a0, max_nfev, retry_cost = _kerelsky_args(x0, a0, max_nfev, retry_cost, dtype)
    jac = np.ascontiguousarray(jac, dtype=dtype)
    if jac.shape[-2:] != (2, 2):
        raise ValueError('jac must have shape (..., 2, 2)')
    lead = jac.shape[:-2]
    out = np.empty(lead + (4,), dtype=dtype)
    cost = np.empty(lead, dtype=np.float64)
    check(load().gpa_kerelsky_fit(int(device), code, jac.size // 4, _ptr(jac), None if a0 is None else _ptr(a0), _ptr(x0), max_nfev,
                                  retry_cost, _ptr(out), _ptr(cost)), 'gpa_kerelsky_fit')
    return out, cost


def kerelsky_fit_dev(jac_ptr, npx, x0, out_ptr, a0=None, max_nfev=50, retry_cost=1e-5, cost_ptr=None, dtype=np.float64, device=0,
                     stream=None):
    """gpa_kerelsky_fit_dev: device pointers jac (npx x 2 x 2) and out (npx x 4) in the dtype, cost (npx doubles, optional);
    asynchronous on `stream` (a hipStream_t as an integer; None: the default stream)."""
    code, x0, a0, max_nfev, retry_cost = _kerelsky_args(x0, a0, max_nfev, retry_cost, dtype)
    if int(npx) < 0:
        raise ValueError('npx must be >= 0')
    check(load().gpa_kerelsky_fit_dev(int(device), code, int(npx), _ptr(int(jac_ptr)), None if a0 is None else _ptr(a0), _ptr(x0),
                                      max_nfev, retry_cost, _ptr(int(out_ptr)), None if cost_ptr is None else _ptr(int(cost_ptr)),
                                      None if stream is None else _ptr(int(stream))), 'gpa_kerelsky_fit_dev')


def _real_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64')
    return dtype, GPA_F32 if dtype == np.float32 else GPA_F64


def _spacing(nmperpixel):
    h = float(nmperpixel)
    if not np.isfinite(h) or h == 0.0:
        raise ValueError('nmperpixel must be finite and not zero')
    return h


def _stream(stream):
    return None if stream is None else _ptr(int(stream))


def field_jacobian_shape(shape):
    """(nimg, n0, n1) of a displacement field (2, N, M) or stack (B, 2, N, M); ValueError for anything else"""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[1] != 2 or shape[0] < 1:
        raise ValueError('U must be a displacement field (2, N, M) or a stack (B, 2, N, M), not %s' % (shape,))
    if shape[2] < 2 or shape[3] < 2:
        raise ValueError('every axis of U needs at least two samples for a difference, not %s' % (shape[2:],))
    return shape[0], shape[2], shape[3]


def field_jacobian(u, nmperpixel, add_identity=False, want_J=True, want_props=False, refangle=0., refscale=1., diff=False,
                   dtype=np.float64, device=0):
    """Plan-free gpa_field_jacobian: u (2, N, M) or (B, 2, N, M) -> (J (..., N, M, 2, 2) or None, props (..., 4, N, M) or None),
    J = np.gradient(-u, nmperpixel) per component and axis (+ I with add_identity), props those of I + J."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    nimg, n0, n1 = field_jacobian_shape(np.shape(u))
    if not (want_J or want_props):
        raise ValueError('nothing to compute: neither J nor props is wanted')
    lead = np.shape(u)[:-3]
    u = np.ascontiguousarray(u, dtype=dtype)
    J = np.empty(lead + (n0, n1, 2, 2), dtype=dtype) if want_J else None
    props = np.empty(lead + (4, n0, n1), dtype=dtype) if want_props else None
    check(load().gpa_field_jacobian(int(device), code, nimg, n0, n1, _ptr(u), h, int(bool(add_identity)), _ptr(J), _ptr(props),
                                    float(refangle), float(refscale), int(bool(diff))), 'gpa_field_jacobian')
    return J, props


def field_jacobian_dev(u_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, add_identity=False, refangle=0., refscale=1.,
                       diff=False, dtype=np.float64, device=0, stream=None):
    """gpa_field_jacobian_dev on device pointers: u of `shape` (2, N, M) or (B, 2, N, M), J and props as field_jacobian lays them
    out, at least one of them; asynchronous on `stream` (a hipStream_t as an integer; None: the default stream)."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    nimg, n0, n1 = field_jacobian_shape(shape)
    if J_ptr is None and props_ptr is None:
        raise ValueError('nothing to compute: J_ptr and props_ptr are both None')
    check(load().gpa_field_jacobian_dev(int(device), code, nimg, n0, n1, _ptr(int(u_ptr)), h, int(bool(add_identity)),
                                        None if J_ptr is None else _ptr(int(J_ptr)),
                                        None if props_ptr is None else _ptr(int(props_ptr)), float(refangle), float(refscale),
                                        int(bool(diff)), _stream(stream)), 'gpa_field_jacobian_dev')


def _phases_args(kvecs, phases_shape, weights_shape):
    kvecs = _f64(kvecs)
    if kvecs.ndim != 2 or kvecs.shape[1] != 2 or not 2 <= len(kvecs) <= 8:
        raise ValueError('kvecs must have shape (P, 2) with 2 <= P <= 8, not %s' % (kvecs.shape,))
    if not np.isfinite(kvecs).all():
        raise ValueError('kvecs must be finite')
    phases_shape = tuple(int(v) for v in phases_shape)
    if len(phases_shape) != 3 or phases_shape[0] != len(kvecs):
        raise ValueError('phases must have shape (P, N, M) with one plane per k-vector, not %s' % (phases_shape,))
    if tuple(weights_shape) != phases_shape:
        raise ValueError('weights %s must have the shape of phases %s' % (tuple(weights_shape), phases_shape))
    if phases_shape[1] < 2 or phases_shape[2] < 2:
        raise ValueError('every axis of phases needs at least two samples for a difference, not %s' % (phases_shape[1:],))
    return kvecs


def phases_jacobian(kvecs, phases, weights, nmperpixel, add_identity=False, want_J=True, want_props=False, refangle=0., refscale=1.,
                    diff=False, dtype=np.float64, device=0):
    """Plan-free gpa_phases_jacobian: phases and weights (P, N, M), kvecs (P, 2) -> (J (N, M, 2, 2) or None, props (4, N, M) or
    None)."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    kvecs = _phases_args(kvecs, np.shape(phases), np.shape(weights))
    if not (want_J or want_props):
        raise ValueError('nothing to compute: neither J nor props is wanted')
    phases = np.ascontiguousarray(phases, dtype=dtype)
    weights = np.ascontiguousarray(weights, dtype=dtype)
    P, n0, n1 = phases.shape
    J = np.empty((n0, n1, 2, 2), dtype=dtype) if want_J else None
    props = np.empty((4, n0, n1), dtype=dtype) if want_props else None
    check(load().gpa_phases_jacobian(int(device), code, n0, n1, P, _ptr(kvecs), _ptr(phases), _ptr(weights), h,
                                     int(bool(add_identity)), _ptr(J), _ptr(props), float(refangle), float(refscale),
                                     int(bool(diff))), 'gpa_phases_jacobian')
    return J, props


def phases_jacobian_dev(kvecs, phases_ptr, weights_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, add_identity=False,
                        refangle=0., refscale=1., diff=False, dtype=np.float64, device=0, stream=None):
    """gpa_phases_jacobian_dev on device pointers: phases and weights of `shape` (P, N, M); J and props as phases_jacobian lays
    them out, at least one of them; asynchronous on `stream`."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    kvecs = _phases_args(kvecs, shape, shape)
    if J_ptr is None and props_ptr is None:
        raise ValueError('nothing to compute: J_ptr and props_ptr are both None')
    P, n0, n1 = (int(v) for v in shape)
    check(load().gpa_phases_jacobian_dev(int(device), code, n0, n1, P, _ptr(kvecs), _ptr(int(phases_ptr)), _ptr(int(weights_ptr)),
                                         h, int(bool(add_identity)), None if J_ptr is None else _ptr(int(J_ptr)),
                                         None if props_ptr is None else _ptr(int(props_ptr)), float(refangle), float(refscale),
                                         int(bool(diff)), _stream(stream)), 'gpa_phases_jacobian_dev')


def _gradients_args(kvecs, dks, grads_shape, weights_shape):
    """(kvecs, dks or None, lead, (nimg, n0, n1)) of grads (P, N, M, 2) or a stack (B, P, N, M, 2) with weights to match"""
    kvecs = _f64(kvecs)
    if kvecs.ndim != 2 or kvecs.shape[1] != 2 or not 2 <= len(kvecs) <= 8:
        raise ValueError('kvecs must have shape (P, 2) with 2 <= P <= 8, not %s' % (kvecs.shape,))
    if not np.isfinite(kvecs).all():
        raise ValueError('kvecs must be finite')
    if dks is not None:
        dks = _f64(dks)
        if dks.shape != kvecs.shape or not np.isfinite(dks).all():
            raise ValueError('dks must be finite and have the shape of kvecs %s, not %s' % (kvecs.shape, dks.shape))
    gs = tuple(int(v) for v in grads_shape)
    if len(gs) not in (4, 5) or gs[-1] != 2 or gs[-4] != len(kvecs) or min(gs) < 1:
        raise ValueError('grads must have shape (P, N, M, 2) or (B, P, N, M, 2) with one plane per k-vector, not %s' % (gs,))
    if tuple(int(v) for v in weights_shape) != gs[:-1]:
        raise ValueError('weights %s must have the shape of grads %s without its last axis' % (tuple(weights_shape), gs))
    lead = gs[:-4]
    return kvecs, dks, lead, (lead[0] if lead else 1, gs[-3], gs[-2])


def gradients_jacobian(kvecs, grads, weights, nmperpixel, dks=None, add_identity=False, want_J=True, want_props=False, refangle=0.,
                       refscale=1., diff=False, dtype=np.float64, device=0):
    """Plan-free gpa_gradients_jacobian: phase gradients (P, N, M, 2) and weights (P, N, M) of one frame, or (B, P, N, M, 2) and
    (B, P, N, M) of a stack, kvecs (P, 2), dks None or (P, 2) (iso_ref) -> (J (..., N, M, 2, 2) or None, props (..., 4, N, M) or
    None): the J of Plan.phasegradient2J per frame, the props of props_from_jac(J, add_identity=True)."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    kvecs, dks, lead, (nimg, n0, n1) = _gradients_args(kvecs, dks, np.shape(grads), np.shape(weights))
    if not (want_J or want_props):
        raise ValueError('nothing to compute: neither J nor props is wanted')
    grads = np.ascontiguousarray(grads, dtype=dtype)
    weights = np.ascontiguousarray(weights, dtype=dtype)
    J = np.empty(lead + (n0, n1, 2, 2), dtype=dtype) if want_J else None
    props = np.empty(lead + (4, n0, n1), dtype=dtype) if want_props else None
    check(load().gpa_gradients_jacobian(int(device), code, nimg, n0, n1, len(kvecs), _ptr(kvecs), _ptr(dks), _ptr(grads),
                                        _ptr(weights), h, int(bool(add_identity)), _ptr(J), _ptr(props), float(refangle),
                                        float(refscale), int(bool(diff))), 'gpa_gradients_jacobian')
    return J, props


def gradients_jacobian_dev(kvecs, grads_ptr, weights_ptr, shape, nmperpixel, J_ptr=None, props_ptr=None, dks=None,
                           add_identity=False, refangle=0., refscale=1., diff=False, dtype=np.float64, device=0, stream=None):
    """gpa_gradients_jacobian_dev on device pointers: grads of `shape` (P, N, M, 2) or (B, P, N, M, 2), weights of that shape
    without its last axis; J and props as gradients_jacobian lays them out, at least one of them; asynchronous on `stream`."""
    dtype, code = _real_dtype(dtype)
    h = _spacing(nmperpixel)
    kvecs, dks, _, (nimg, n0, n1) = _gradients_args(kvecs, dks, shape, tuple(shape)[:-1])
    if J_ptr is None and props_ptr is None:
        raise ValueError('nothing to compute: J_ptr and props_ptr are both None')
    check(load().gpa_gradients_jacobian_dev(int(device), code, nimg, n0, n1, len(kvecs), _ptr(kvecs), _ptr(dks),
                                            _ptr(int(grads_ptr)), _ptr(int(weights_ptr)), h, int(bool(add_identity)),
                                            None if J_ptr is None else _ptr(int(J_ptr)),
                                            None if props_ptr is None else _ptr(int(props_ptr)), float(refangle), float(refscale),
                                            int(bool(diff)), _stream(stream)), 'gpa_gradients_jacobian_dev')


def phys_props_from_jac(jac, add_identity=False, refangle=0., refscale=1., diff=False, poisson_ratio=0.16, dtype=np.float64,
                        device=0):
    """Plan-free gpa_phys_props_from_jac: jac (..., 2, 2) -> (angle, aniangle, alpha, epsilon) as (4, ...)."""
    dtype, code = _real_dtype(dtype)
    if not np.isfinite(poisson_ratio):
        raise ValueError('poisson_ratio must be finite')
    if np.shape(jac)[-2:] != (2, 2):
        raise ValueError('jac must have shape (..., 2, 2)')
    jac = np.ascontiguousarray(jac, dtype=dtype)
    props = np.empty((4,) + jac.shape[:-2], dtype=dtype)
    check(load().gpa_phys_props_from_jac(int(device), code, jac.size // 4, _ptr(jac), int(bool(add_identity)), float(refangle),
                                         float(refscale), int(bool(diff)), float(poisson_ratio), _ptr(props)),
          'gpa_phys_props_from_jac')
    return props


@atexit.register
def _close_plans():
    for p in list(_plans.values()):
        try:
            p.close()
        except Exception:
            pass
    _plans.clear()
