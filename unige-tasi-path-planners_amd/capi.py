"""ctypes binding of include/ufm.h (libufm.so).  No CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ALGO_FD, ALGO_SG, ALGO_DFM = 0, 1, 2
LOOP_OK, LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL = 0, -1, -2

# every symbol include/ufm.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "ufm_create", "ufm_destroy", "ufm_reset", "ufm_set_occupancy_threshold",
    "ufm_set_heuristic_multiplier", "ufm_set_map", "ufm_patch_map", "ufm_set_start",
    "ufm_set_goal", "ufm_step", "ufm_set_map_device", "ufm_patch_map_device",
    "ufm_field_dims", "ufm_read_field", "ufm_read_map", "ufm_set_param", "ufm_set_profiling", "ufm_stream",
    "ufm_version", "ufm_tile_edge", "ufm_batch_create", "ufm_batch_destroy", "ufm_batch_size",
    "ufm_batch_set_occupancy_threshold", "ufm_batch_set_map", "ufm_batch_patch_map",
    "ufm_batch_set_start", "ufm_batch_set_goal", "ufm_batch_reset", "ufm_batch_step",
    "ufm_batch_read_field", "ufm_extract_path", "ufm_batch_extract_path", "ufm_read_info", "ufm_read_info_derived",
    "ufm_check_layout", "ufm_batch_check_layout", "ufm_batch_set_param", "ufm_check_info", "ufm_batch_check_info",
    "ufm_batch_create_sharded", "ufm_batch_shards", "ufm_batch_set_heuristic_multiplier", "ufm_batch_set_map_device",
    "ufm_batch_patch_map_device", "ufm_batch_read_map", "ufm_batch_set_profiling", "ufm_batch_stream", "ufm_read_queue",
    "ufm_track_changes", "ufm_read_changes", "ufm_batch_track_changes", "ufm_batch_read_changes",
    "ufm_extract_paths_from", "ufm_batch_extract_paths_from",
    "ufm_set_cspace", "ufm_read_raw_map", "ufm_batch_set_cspace", "ufm_batch_read_raw_map",
    "ufm_track_costs", "ufm_read_cost_census", "ufm_heuristic_multiplier",
    "ufm_batch_track_costs", "ufm_batch_read_cost_census", "ufm_batch_heuristic_multiplier",
    "ufm_set_sensor", "ufm_set_survey", "ufm_set_survey_device", "ufm_reveal", "ufm_read_survey",
    "ufm_batch_set_sensor", "ufm_batch_set_survey", "ufm_batch_set_survey_device", "ufm_batch_reveal", "ufm_batch_read_survey",
    "ufm_gaussian_taps", "ufm_set_image", "ufm_set_image_device", "ufm_batch_set_image", "ufm_batch_set_image_device",
    "ufm_set_layers", "ufm_patch_layer", "ufm_patch_layer_device", "ufm_set_layer", "ufm_set_layer_device",
    "ufm_set_layer_survey", "ufm_set_layer_survey_device", "ufm_read_layer", "ufm_read_layer_survey",
    "ufm_batch_set_layers", "ufm_batch_patch_layer", "ufm_batch_patch_layer_device", "ufm_batch_set_layer", "ufm_batch_set_layer_device",
    "ufm_batch_set_layer_survey", "ufm_batch_set_layer_survey_device", "ufm_batch_read_layer", "ufm_batch_read_layer_survey",
]
MAX_LAYERS = 4     # UFM_MAX_LAYERS


class UfmError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [
        ("u_ms", C.c_float), ("p_ms", C.c_float),
        ("updated", C.c_uint64), ("expanded", C.c_uint64),
        ("tile_visits", C.c_uint64), ("tile_iters", C.c_uint64), ("elem_evals", C.c_uint64),
        ("launches", C.c_uint32), ("raise_launches", C.c_uint32),
        ("kernel_ms", C.c_float),
        ("crit_sweeps", C.c_uint64),
        ("raise_tile_visits", C.c_uint64),
        ("raise_kernel_ms", C.c_float),
        ("queued_lower", C.c_uint32),
        ("queued_raise", C.c_uint32),
        ("timed_launches", C.c_uint32),
        ("timed_raise_launches", C.c_uint32),
        ("graphs_instantiated", C.c_uint32),
        ("region_replans", C.c_uint32),
        ("region_replans_done", C.c_uint32),
        ("resident_launches", C.c_uint32),
        ("resident_kernel_ms", C.c_float),
        ("resident_stops", C.c_uint32),
        ("resident_tile_visits", C.c_uint64),
        ("region_launches", C.c_uint32),
        ("region_timed", C.c_uint32),
        ("region_kernel_ms", C.c_float),
        ("region_tiles", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PathInfo(C.Structure):
    """ufm_path_info (include/ufm.h)"""
    _fields_ = [
        ("n_points", C.c_int32), ("n_costs", C.c_int32),
        ("total_cost", C.c_float), ("total_dist", C.c_float),
        ("steps", C.c_int32), ("e_ms", C.c_float),
    ]


_LIB_PATH = os.path.join(_HERE, "libufm.so")


def library_path():
    return _LIB_PATH


def use_library(path):
    """Bind another build of the same library (tools/: kernel tuning experiments, diagnostic builds).  Explicit, per
    process, before the first planner is created -- the product, the tests and bench.py never call this."""
    global _LIB_PATH
    if _LIB is not None:
        raise UfmError("use_library() after the library has been loaded")
    _LIB_PATH = os.path.abspath(path)


def build_library():
    """hipcc cross-compiles gfx950 without a GPU (seconds)."""
    subprocess.check_call(["make", "-s", "-C", _HERE])


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = library_path()
    if not os.path.exists(so):
        raise UfmError("libufm.so is not built (run `make -C unige-tasi-path-planners_amd` "
                       "or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(so)
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    L.ufm_create.argtypes = [C.POINTER(vp), i, i, i, i]
    L.ufm_destroy.argtypes = [vp]
    L.ufm_reset.argtypes = [vp]
    L.ufm_set_occupancy_threshold.argtypes = [vp, f]
    L.ufm_set_heuristic_multiplier.argtypes = [vp, f]
    L.ufm_set_map.argtypes = [vp, vp, i, i]
    L.ufm_set_map_device.argtypes = [vp, vp, i, i]
    L.ufm_patch_map.argtypes = [vp, vp, i, i, i, i]
    L.ufm_patch_map_device.argtypes = [vp, vp, i, i, i, i]
    L.ufm_set_start.argtypes = [vp, f, f]
    L.ufm_set_goal.argtypes = [vp, f, f]
    L.ufm_step.argtypes = [vp, C.POINTER(Stats)]
    L.ufm_field_dims.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.ufm_read_field.argtypes = [vp, i, i, i, i, vp, vp]
    L.ufm_read_map.argtypes = [vp, vp]
    L.ufm_check_layout.argtypes = [vp, vp, vp]
    L.ufm_batch_check_layout.argtypes = [vp, vp, vp]
    L.ufm_check_info.argtypes = [vp, vp]
    L.ufm_read_queue.argtypes = [vp, i, vp, vp, vp]
    L.ufm_batch_check_info.argtypes = [vp, vp]
    L.ufm_batch_set_param.argtypes = [vp, C.c_char_p, C.c_double]
    L.ufm_set_param.argtypes = [vp, C.c_char_p, C.c_double]
    L.ufm_set_profiling.argtypes = [vp, i]
    L.ufm_stream.argtypes = [vp]
    L.ufm_stream.restype = vp
    L.ufm_version.restype = C.c_char_p
    L.ufm_batch_create.argtypes = [C.POINTER(vp), i, i, i, i, i]
    L.ufm_batch_create_sharded.argtypes = [C.POINTER(vp), i, i, i, i, C.POINTER(i), i]
    L.ufm_batch_shards.argtypes = [vp]
    L.ufm_batch_set_heuristic_multiplier.argtypes = [vp, f]
    L.ufm_batch_set_map_device.argtypes = [vp, i, vp, i, i]
    L.ufm_batch_patch_map_device.argtypes = [vp, i, vp, i, i, i, i]
    L.ufm_batch_read_map.argtypes = [vp, i, vp]
    L.ufm_batch_set_profiling.argtypes = [vp, i]
    L.ufm_batch_stream.argtypes = [vp, i]
    L.ufm_batch_stream.restype = vp
    L.ufm_batch_destroy.argtypes = [vp]
    L.ufm_batch_size.argtypes = [vp]
    L.ufm_batch_set_occupancy_threshold.argtypes = [vp, f]
    L.ufm_batch_set_map.argtypes = [vp, i, vp, i, i]
    L.ufm_batch_patch_map.argtypes = [vp, i, vp, i, i, i, i]
    L.ufm_batch_set_start.argtypes = [vp, i, f, f]
    L.ufm_batch_set_goal.argtypes = [vp, i, f, f]
    L.ufm_batch_reset.argtypes = [vp, i]
    L.ufm_batch_step.argtypes = [vp, C.POINTER(Stats)]
    L.ufm_batch_read_field.argtypes = [vp, i, i, i, i, i, vp, vp]
    L.ufm_read_info.argtypes = [vp, i, i, i, i, vp]
    L.ufm_read_info_derived.argtypes = [vp, i, i, i, i, vp]
    L.ufm_extract_path.argtypes = [vp, i, i, i, vp, i, vp, i, C.POINTER(PathInfo)]
    L.ufm_batch_extract_path.argtypes = [vp, i, i, i, vp, i, vp, i, C.POINTER(PathInfo)]
    L.ufm_extract_paths_from.argtypes = [vp, i, vp, i, i, i, vp, i, vp, i, vp]
    L.ufm_batch_extract_paths_from.argtypes = [vp, i, vp, vp, i, i, i, vp, i, vp, i, vp]
    L.ufm_track_changes.argtypes = [vp, i]
    L.ufm_read_changes.argtypes = [vp, i, vp, vp, vp, vp]
    L.ufm_batch_track_changes.argtypes = [vp, i]
    L.ufm_batch_read_changes.argtypes = [vp, i, i, vp, vp, vp, vp]
    L.ufm_set_cspace.argtypes = [vp, vp, i, i, i, i]
    L.ufm_read_raw_map.argtypes = [vp, vp]
    L.ufm_batch_set_cspace.argtypes = [vp, vp, i, i, i, i]
    L.ufm_batch_read_raw_map.argtypes = [vp, i, vp]
    L.ufm_track_costs.argtypes = [vp, i]
    L.ufm_read_cost_census.argtypes = [vp, vp, C.POINTER(i), C.POINTER(i)]
    L.ufm_heuristic_multiplier.argtypes = [vp, C.POINTER(f)]
    L.ufm_batch_track_costs.argtypes = [vp, i]
    L.ufm_batch_read_cost_census.argtypes = [vp, i, vp, C.POINTER(i), C.POINTER(i)]
    L.ufm_batch_heuristic_multiplier.argtypes = [vp, C.POINTER(f)]
    L.ufm_set_sensor.argtypes = [vp, vp, i, i, i, i]
    L.ufm_set_survey.argtypes = [vp, vp, i, i]
    L.ufm_set_survey_device.argtypes = [vp, vp, i, i]
    L.ufm_reveal.argtypes = [vp, i, i, vp]
    L.ufm_read_survey.argtypes = [vp, vp]
    L.ufm_batch_set_sensor.argtypes = [vp, vp, i, i, i, i]
    L.ufm_batch_set_survey.argtypes = [vp, i, vp, i, i]
    L.ufm_batch_set_survey_device.argtypes = [vp, i, vp, i, i]
    L.ufm_batch_reveal.argtypes = [vp, vp, vp]
    L.ufm_batch_read_survey.argtypes = [vp, i, vp]
    L.ufm_gaussian_taps.argtypes = [i, vp]
    L.ufm_set_image.argtypes = [vp, vp, i, i, vp, i, i]
    L.ufm_set_image_device.argtypes = [vp, vp, i, i, vp, i, i]
    L.ufm_batch_set_image.argtypes = [vp, i, vp, i, i, vp, i, i]
    L.ufm_batch_set_image_device.argtypes = [vp, i, vp, i, i, vp, i, i]
    L.ufm_set_layers.argtypes = [vp, i]
    L.ufm_patch_layer.argtypes = [vp, i, vp, i, i, i, i]
    L.ufm_patch_layer_device.argtypes = [vp, i, vp, i, i, i, i]
    L.ufm_set_layer.argtypes = [vp, i, vp, i, i]
    L.ufm_set_layer_device.argtypes = [vp, i, vp, i, i]
    L.ufm_set_layer_survey.argtypes = [vp, i, vp, i, i]
    L.ufm_set_layer_survey_device.argtypes = [vp, i, vp, i, i]
    L.ufm_read_layer.argtypes = [vp, i, vp]
    L.ufm_read_layer_survey.argtypes = [vp, i, vp]
    L.ufm_batch_set_layers.argtypes = [vp, i]
    L.ufm_batch_patch_layer.argtypes = [vp, i, i, vp, i, i, i, i]
    L.ufm_batch_patch_layer_device.argtypes = [vp, i, i, vp, i, i, i, i]
    L.ufm_batch_set_layer.argtypes = [vp, i, i, vp, i, i]
    L.ufm_batch_set_layer_device.argtypes = [vp, i, i, vp, i, i]
    L.ufm_batch_set_layer_survey.argtypes = [vp, i, i, vp, i, i]
    L.ufm_batch_set_layer_survey_device.argtypes = [vp, i, i, vp, i, i]
    L.ufm_batch_read_layer.argtypes = [vp, i, i, vp]
    L.ufm_batch_read_layer_survey.argtypes = [vp, i, i, vp]
    _LIB = L
    return L


def _chk(rc, what):
    if rc != 0:
        raise UfmError("%s failed with code %d" % (what, rc))


def cspace_disc(diameter):
    """The footprint harness.dilate(img, diameter) dilates by, as ufm_set_cspace takes it: a uint8 matrix of edge 2 * (diameter // 2) + 1
    with the anchor at its centre -- the disc x^2 + y^2 <= r^2, r = diameter // 2 (diameter <= 1: the 1 x 1 mask, "off")."""
    if diameter <= 1:
        return np.ones((1, 1), np.uint8)
    r = diameter // 2
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return ((xx * xx) / max(r * r, 1) + (yy * yy) / max(r * r, 1) <= 1.0).astype(np.uint8)


def _cspace_args(mask, anchor):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    if mask.ndim != 2:
        raise UfmError("a footprint is a matrix")
    ar, ac = (-1, -1) if anchor is None else (int(anchor[0]), int(anchor[1]))
    return mask, mask.shape[1], mask.shape[0], ar, ac


def sensor_disc(radius):
    """The field of view harness.round_patch_update reveals (run_simulator.py:9-28), as ufm_set_sensor takes it: the (2 r + 1)^2 uint8 matrix
    of x^2 + y^2 <= r^2 with the anchor at its centre."""
    r = int(radius)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (xx * xx + yy * yy <= r * r).astype(np.uint8)


def _survey_args(raster, width=None, length=None):
    """(pointer, width, length, on_device, the object to keep alive) of a survey: a host matrix, or a device buffer (anything with .ptr, e.g.
    the tests' DeviceBytes) with its dimensions -- its own .shape = (length, width), or the two keywords"""
    if hasattr(raster, "ptr"):
        if width is None or length is None:
            if not hasattr(raster, "shape"):
                raise UfmError("a device survey needs width and length")
            length, width = raster.shape
        return raster.ptr, int(width), int(length), True, raster
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    if raster.ndim != 2:
        raise UfmError("a survey is a matrix")
    return raster.ctypes.data, raster.shape[1], raster.shape[0], False, raster


def gaussian_taps(ksize):
    """ufm_gaussian_taps: the taps cv2.GaussianBlur(img, (k, k), 0) applies to 8-bit images (uint16 [ksize], their sum 256) -- the C
    definition of harness.gaussian_kernel_fixed; ksize odd, 1 .. 31"""
    ksize = int(ksize)
    taps = np.zeros(max(ksize, 1), np.uint16)
    _chk(load_library().ufm_gaussian_taps(ksize, taps.ctypes.data), "ufm_gaussian_taps")
    return taps


def _image_args(img, taps, ksize, width, length):
    """(pointer, width, length, on_device, taps uint16, the object to keep alive) of a bitmap for set_image: the image as a survey is taken
    (_survey_args); the filter as `taps`, or as the Gaussian of `ksize`, or -- neither given -- {256}, no blur"""
    if taps is not None and ksize is not None:
        raise UfmError("set_image takes taps or ksize, not both")
    if taps is None:
        taps = gaussian_taps(1 if ksize is None else ksize)
    taps = np.ascontiguousarray(taps)
    if taps.ndim != 1 or taps.size == 0 or (taps < 0).any() or (taps > 65535).any():
        raise UfmError("taps are a vector of uint16")
    ptr, width, length, dev, keep = _survey_args(img, width, length)
    return ptr, width, length, dev, taps.astype(np.uint16), keep


def _read_census(call, what):
    """ufm_read_cost_census / ufm_batch_read_cost_census through `call(hist, min, max)`: (hist uint64 [256], min_cost, max_cost)"""
    hist = np.zeros(256, np.uint64)
    mn, mx = C.c_int(0), C.c_int(0)
    _chk(call(hist.ctypes.data, C.byref(mn), C.byref(mx)), what)
    return hist, mn.value, mx.value


def _read_changes(call, what, want_info, cap=None):
    """ufm_read_changes / ufm_batch_read_changes through `call(cap, xy, g, info, total)`: a counting call sizes the buffers (cap None),
    the second call delivers.  Returns (xy int32 [n, 2], g float32 [n], info int32 [n, 2] | None, total); with an explicit cap that is
    too small n = 0 and nothing was committed."""
    total = C.c_int(0)
    if cap is None:
        _chk(call(0, None, None, None, C.addressof(total)), what)
        cap = total.value
        if cap == 0:
            return np.zeros((0, 2), np.int32), np.zeros(0, np.float32), (np.zeros((0, 2), np.int32) if want_info else None), 0
    xy = np.zeros((max(cap, 1), 2), np.int32)
    g = np.zeros(max(cap, 1), np.float32)
    info = np.zeros((max(cap, 1), 2), np.int32) if want_info else None
    _chk(call(cap, xy.ctypes.data, g.ctypes.data, info.ctypes.data if want_info else None, C.addressof(total)), what)
    n = total.value if total.value <= cap else 0
    return xy[:n], g[:n], (info[:n] if want_info else None), total.value


def _paths_from(call, what, starts, max_steps):
    """ufm_extract_paths_from / ufm_batch_extract_paths_from through `call(n, starts, pts, cap_p, costs, cap_c, info)`:
    ([(points, step_costs, total_cost, total_dist)] in the order of `starts`, the PathInfo array)"""
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 2)
    n = len(starts)
    cap_p, cap_c = 3 * max_steps + 1, 2 * max_steps
    pts = np.zeros((max(n, 1), cap_p, 2), np.float32)
    costs = np.zeros((max(n, 1), cap_c), np.float32)
    info = (PathInfo * max(n, 1))()
    _chk(call(n, starts.ctypes.data, pts.ctypes.data, cap_p, costs.ctypes.data, cap_c, C.addressof(info)), what)
    return [(pts[k, :info[k].n_points].copy(), costs[k, :info[k].n_costs].copy(),
             info[k].total_cost, info[k].total_dist) for k in range(n)], info


class Planner:
    """Mirror of the reference planner surface (ReplannerBase.h:39-123):
    reset / set_occupancy_threshold / set_heuristic_multiplier / set_map /
    patch_map / set_start / set_goal / step, public stats u_time, p_time,
    num_nodes_updated, num_nodes_expanded, and a dense field view in place of
    ExpandedMap::get_g / get_rhs."""

    def __init__(self, algo, opt_lvl=0, use_heuristic=False, device=0, follow_info=False):
        self.L = load_library()
        h = C.c_void_p()
        _chk(self.L.ufm_create(C.byref(h), algo, opt_lvl, int(use_heuristic), device), "ufm_create")
        self.h = h
        if follow_info:     # MS-DFM level 1: invalidation along the stored back-pointers (ufm_set_param "dfm_follow_info")
            self.set_param("dfm_follow_info", 1)
        self.algo = algo
        self.stats = Stats()
        self.u_time = 0.0
        self.p_time = 0.0
        self.num_nodes_updated = 0
        self.num_nodes_expanded = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.ufm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _chk(self.L.ufm_reset(self.h), "ufm_reset")

    def set_occupancy_threshold(self, t):
        _chk(self.L.ufm_set_occupancy_threshold(self.h, float(t)), "ufm_set_occupancy_threshold")

    def set_heuristic_multiplier(self, m):
        _chk(self.L.ufm_set_heuristic_multiplier(self.h, float(m)), "ufm_set_heuristic_multiplier")

    def set_map(self, m):
        m = np.ascontiguousarray(m, dtype=np.uint8)
        length, width = m.shape
        _chk(self.L.ufm_set_map(self.h, m.ctypes.data, width, length), "ufm_set_map")

    def set_map_device(self, dev_ptr, width, length):
        _chk(self.L.ufm_set_map_device(self.h, dev_ptr, width, length), "ufm_set_map_device")

    def patch_map(self, patch, x, y):
        patch = np.ascontiguousarray(patch, dtype=np.uint8)
        h, w = patch.shape
        _chk(self.L.ufm_patch_map(self.h, patch.ctypes.data, int(x), int(y), w, h), "ufm_patch_map")

    def patch_map_device(self, dev_ptr, x, y, w, h):
        _chk(self.L.ufm_patch_map_device(self.h, dev_ptr, int(x), int(y), int(w), int(h)), "ufm_patch_map_device")

    def patch_map_host(self, host_ptr, x, y, w, h):
        """ufm_patch_map with the address of a host buffer (a caller that keeps its patches in one array: no numpy view per call)"""
        _chk(self.L.ufm_patch_map(self.h, host_ptr, int(x), int(y), int(w), int(h)), "ufm_patch_map")

    def set_start(self, x, y):
        _chk(self.L.ufm_set_start(self.h, float(x), float(y)), "ufm_set_start")

    def set_goal(self, x, y):
        _chk(self.L.ufm_set_goal(self.h, float(x), float(y)), "ufm_set_goal")

    def set_param(self, name, value):
        _chk(self.L.ufm_set_param(self.h, name.encode(), float(value)), "ufm_set_param")

    def stream_ptr(self):
        """hipStream_t the engine's kernels run on (e.g. for torch.cuda.ExternalStream)"""
        return int(self.L.ufm_stream(self.h) or 0)

    def set_profiling(self, on):
        _chk(self.L.ufm_set_profiling(self.h, int(on)), "ufm_set_profiling")

    def step(self):
        rc = self.L.ufm_step(self.h, C.byref(self.stats))
        if rc in (LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL):
            return rc
        _chk(rc, "ufm_step")
        self.u_time, self.p_time = self.stats.u_ms, self.stats.p_ms
        self.num_nodes_updated = self.stats.updated
        self.num_nodes_expanded = self.stats.expanded
        return rc

    def dims(self):
        a, b = C.c_int(), C.c_int()
        _chk(self.L.ufm_field_dims(self.h, C.byref(a), C.byref(b)), "ufm_field_dims")
        return a.value, b.value

    def read_field(self, x0=0, y0=0, nx=None, ny=None):
        ex, ey = self.dims()
        nx = ex - x0 if nx is None else nx
        ny = ey - y0 if ny is None else ny
        g = np.empty((nx, ny), dtype=np.float32)
        rhs = np.empty((nx, ny), dtype=np.float32)
        _chk(self.L.ufm_read_field(self.h, x0, y0, nx, ny, g.ctypes.data, rhs.ctypes.data), "ufm_read_field")
        return g, rhs

    def g(self):
        return self.read_field()[0]

    def read_info(self, x0=0, y0=0, nx=None, ny=None, derived=False):
        """back-pointers (the reference's INFO of level-1/2 planners): int32 [nx][ny][2] -- the stored ones, or
        (derived=True) those min_rhs<level>() derives from the field alone"""
        ex, ey = self.dims()
        nx = ex - x0 if nx is None else nx
        ny = ey - y0 if ny is None else ny
        out = np.empty((nx, ny, 2), np.int32)
        fn = self.L.ufm_read_info_derived if derived else self.L.ufm_read_info
        _chk(fn(self.h, x0, y0, nx, ny, out.ctypes.data), "ufm_read_info")
        return out

    def extract_path(self, max_steps=20, lookahead=True, allow_indirect=True):
        """LinearInterpolationPathExtractor::extract_path on the device:
        returns (points[n,2], step_costs[m], total_cost, total_dist); the call's info is kept in
        self.path_info."""
        cap_p, cap_c = 3 * max_steps + 1, 2 * max_steps
        pts = np.zeros((cap_p, 2), np.float32)
        costs = np.zeros(cap_c, np.float32)
        self.path_info = PathInfo()
        _chk(self.L.ufm_extract_path(self.h, int(max_steps), int(lookahead), int(allow_indirect),
                                     pts.ctypes.data, cap_p, costs.ctypes.data, cap_c,
                                     C.byref(self.path_info)), "ufm_extract_path")
        pi = self.path_info
        return pts[:pi.n_points].copy(), costs[:pi.n_costs].copy(), pi.total_cost, pi.total_dist

    def extract_paths_from(self, starts, max_steps=20, lookahead=True, allow_indirect=True):
        """position queries (ufm_extract_paths_from): paths from the positions `starts` ([n, 2]) over the field as it stands, in one
        call, without touching the planner's own start.  Returns a list of (points, step_costs, total_cost, total_dist) in the order
        of `starts`; the calls' infos are kept in self.path_infos."""
        out, self.path_infos = _paths_from(
            lambda n, s, *bufs: self.L.ufm_extract_paths_from(self.h, n, s, int(max_steps), int(lookahead), int(allow_indirect), *bufs),
            "ufm_extract_paths_from", starts, max_steps)
        return out

    def read_map(self, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_read_map(self.h, m.ctypes.data), "ufm_read_map")
        return m

    def set_cspace(self, mask, anchor=None):
        """ufm_set_cspace: the vehicle's footprint (uint8 matrix, non-zero = set; anchor (row, col), None: the centre (mh // 2, mw // 2)).
        Before the first set_map; from then on set_map / patch_map take the RAW raster and the engine plans on its dilation."""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _chk(self.L.ufm_set_cspace(self.h, mask.ctypes.data, mw, mh, ar, ac), "ufm_set_cspace")

    def read_raw_map(self, width, length):
        """the raster as the caller gave it, patches applied (read_map: the planning raster, its dilation); only with a footprint set"""
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_read_raw_map(self.h, m.ctypes.data), "ufm_read_raw_map")
        return m

    def track_costs(self, on=True):
        """the cost census (ufm_track_costs): 256 exact counters of the planning raster's values, kept under patches"""
        _chk(self.L.ufm_track_costs(self.h, int(on)), "ufm_track_costs")

    def read_cost_census(self):
        """(hist uint64 [256], min_cost, max_cost) of the planning raster as it stands"""
        return _read_census(lambda *a: self.L.ufm_read_cost_census(self.h, *a), "ufm_read_cost_census")

    def heuristic_multiplier(self):
        """the multiplier the last step used: the caller's, or with set_param("auto_multiplier", 1) the census' minimum"""
        v = C.c_float(0.0)
        _chk(self.L.ufm_heuristic_multiplier(self.h, C.byref(v)), "ufm_heuristic_multiplier")
        return v.value

    def set_sensor(self, mask, anchor=None):
        """ufm_set_sensor: the field of view (uint8 matrix, non-zero = seen; anchor (row, col), None: the centre); sensor_disc(r) is the
        reference simulator's"""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _chk(self.L.ufm_set_sensor(self.h, mask.ctypes.data, mw, mh, ar, ac), "ufm_set_sensor")

    def set_survey(self, raster, width=None, length=None):
        """ufm_set_survey / _device: what the sensor would see, [length][width] like the map -- a host matrix, or a device buffer (.ptr)
        with width and length"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_set_survey_device if dev else self.L.ufm_set_survey
        _chk(fn(self.h, ptr, width, length), "ufm_set_survey")

    def reveal(self, row, col, count=False):
        """ufm_reveal: uncover the field of view around cell (row, col).  count: wait and return the number of cells that changed"""
        n = C.c_uint64(0)
        _chk(self.L.ufm_reveal(self.h, int(row), int(col), C.addressof(n) if count else None), "ufm_reveal")
        return int(n.value) if count else None

    def read_survey(self, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_read_survey(self.h, m.ctypes.data), "ufm_read_survey")
        return m

    def set_image(self, img, taps=None, penalty=0, ksize=None, width=None, length=None):
        """ufm_set_image / _device: the grey-scale bitmap becomes the map (blurred by `taps` -- or gaussian_taps(ksize) --, complemented,
        0 -> 1, + penalty saturating) and its survey (complemented, 0 -> 1) in one launch: harness.simulation_data on the device.  A host
        matrix, or a device buffer (.ptr) with width and length"""
        ptr, width, length, dev, taps, keep = _image_args(img, taps, ksize, width, length)
        fn = self.L.ufm_set_image_device if dev else self.L.ufm_set_image
        _chk(fn(self.h, ptr, width, length, taps.ctypes.data, len(taps), int(penalty)), "ufm_set_image")

    def set_layers(self, n):
        """ufm_set_layers: n rasters per map whose element-wise maximum is the caller's raster (1: off, the default); before the first
        set_map / set_image"""
        _chk(self.L.ufm_set_layers(self.h, int(n)), "ufm_set_layers")

    def patch_layer(self, k, patch, x, y, w=None, h=None):
        """ufm_patch_layer / _device: the bytes into layer k over rows x .., columns y ..; the map takes the maximum over the layers there.
        A host matrix, or a device buffer (.ptr) with w and h"""
        ptr, w, h, dev, keep = _survey_args(patch, w, h)
        fn = self.L.ufm_patch_layer_device if dev else self.L.ufm_patch_layer
        _chk(fn(self.h, int(k), ptr, int(x), int(y), w, h), "ufm_patch_layer")

    def set_layer(self, k, raster, width=None, length=None):
        """ufm_set_layer / _device: layer k wholesale -- a whole-map patch, not a set_map: the field is kept"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_set_layer_device if dev else self.L.ufm_set_layer
        _chk(fn(self.h, int(k), ptr, width, length), "ufm_set_layer")

    def set_layer_survey(self, k, raster, width=None, length=None):
        """ufm_set_layer_survey / _device: what the sensor would see of layer k (k = 0: set_survey)"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_set_layer_survey_device if dev else self.L.ufm_set_layer_survey
        _chk(fn(self.h, int(k), ptr, width, length), "ufm_set_layer_survey")

    def read_layer(self, k, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_read_layer(self.h, int(k), m.ctypes.data), "ufm_read_layer")
        return m

    def read_layer_survey(self, k, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_read_layer_survey(self.h, int(k), m.ctypes.data), "ufm_read_layer_survey")
        return m

    def check_layout(self):
        """(ring entries, cost-window bytes) that differ from the values they copy; (0, 0) when sound"""
        bad = (C.c_uint64 * 2)()
        _chk(self.L.ufm_check_layout(self.h, C.addressof(bad), C.addressof(bad) + 8), "ufm_check_layout")
        return int(bad[0]), int(bad[1])


    def check_info(self):
        """stored back-pointers (level-1/2 planners): (elements with a value, without a back-pointer, whose parent triangle does not
        give the value but a larger one, whose dependence bits are off, whose parent gives a smaller value -- waiting to be
        lowered, beyond the start's key --, unsupported ones at / beyond the start's key: queued invalidations); [1:4] are 0 when sound.
        MS-DFM level 1: the named candidate against the value within 8 ulp (include/ufm.h); level 0 raises UfmError (no Info)"""
        out = (C.c_uint64 * 6)()
        _chk(self.L.ufm_check_info(self.h, C.addressof(out)), "ufm_check_info")
        return tuple(int(v) for v in out)

    def read_queue(self, cap=None):
        """the reference's priority_queue as a caller could observe it between two steps: the elements that are not consistent.
        Returns (xy int32 [n, 2], g float32 [n], rhs float32 [n], total); n = min(total, cap), cap None: all of them"""
        total = C.c_int(0)
        if cap is None:
            _chk(self.L.ufm_read_queue(self.h, 0, None, None, C.addressof(total)), "ufm_read_queue")
            cap = total.value
        xy = np.zeros((max(cap, 1), 2), np.int32)
        gr = np.zeros((max(cap, 1), 2), np.float32)
        _chk(self.L.ufm_read_queue(self.h, cap, xy.ctypes.data, gr.ctypes.data, C.addressof(total)), "ufm_read_queue")
        n = min(total.value, cap)
        return xy[:n], gr[:n, 0].copy(), gr[:n, 1].copy(), total.value

    def track_changes(self, on=True):
        """step deltas (ufm_track_changes): the engine keeps a baseline -- what read_changes last delivered, empty at first"""
        _chk(self.L.ufm_track_changes(self.h, int(on)), "ufm_track_changes")

    def read_changes(self, want_info=False, cap=None):
        """the elements whose value (want_info: or Info pair) differs from the baseline, all or nothing:
        (xy int32 [n, 2], g float32 [n] -- +inf: the element lost its value --, info int32 [n, 2] | None); the baseline advances.
        cap: deliver only if the delta has at most that many records; then returns (xy, g, info, total) -- n = 0 and nothing
        committed if total > cap"""
        out = _read_changes(lambda *a: self.L.ufm_read_changes(self.h, *a), "ufm_read_changes", want_info, cap)
        return out if cap is not None else out[:3]


class BatchPlanner:
    """Batch of independent, equally sized map instances: on one device, or (devices=[...]) spread over several
    in contiguous blocks, one engine per device inside the one handle."""

    def __init__(self, n_maps, algo, opt_lvl=0, use_heuristic=False, device=0, devices=None, follow_info=False):
        self.L = load_library()
        h = C.c_void_p()
        if devices is None:
            _chk(self.L.ufm_batch_create(C.byref(h), n_maps, algo, opt_lvl, int(use_heuristic), device), "ufm_batch_create")
        else:
            arr = (C.c_int * len(devices))(*devices)
            _chk(self.L.ufm_batch_create_sharded(C.byref(h), n_maps, algo, opt_lvl, int(use_heuristic), arr, len(devices)),
                 "ufm_batch_create_sharded")
        self.h = h
        if follow_info:     # as Planner's
            self.set_param("dfm_follow_info", 1)
        self.n = n_maps
        self.algo = algo
        self.stats = Stats()

    def close(self):
        if getattr(self, "h", None):
            self.L.ufm_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_occupancy_threshold(self, t):
        _chk(self.L.ufm_batch_set_occupancy_threshold(self.h, float(t)), "ufm_batch_set_occupancy_threshold")

    def set_map(self, i, m):
        m = np.ascontiguousarray(m, dtype=np.uint8)
        length, width = m.shape
        _chk(self.L.ufm_batch_set_map(self.h, i, m.ctypes.data, width, length), "ufm_batch_set_map")
        self._dims = (length + (0 if self.algo == ALGO_DFM else 1), width + (0 if self.algo == ALGO_DFM else 1))

    def set_map_device(self, i, dev_ptr, width, length):
        _chk(self.L.ufm_batch_set_map_device(self.h, i, dev_ptr, width, length), "ufm_batch_set_map_device")
        self._dims = (length + (0 if self.algo == ALGO_DFM else 1), width + (0 if self.algo == ALGO_DFM else 1))

    def patch_map(self, i, patch, x, y):
        patch = np.ascontiguousarray(patch, dtype=np.uint8)
        h, w = patch.shape
        _chk(self.L.ufm_batch_patch_map(self.h, i, patch.ctypes.data, int(x), int(y), w, h), "ufm_batch_patch_map")

    def patch_map_device(self, i, dev_ptr, x, y, w, h):
        _chk(self.L.ufm_batch_patch_map_device(self.h, i, dev_ptr, int(x), int(y), int(w), int(h)), "ufm_batch_patch_map_device")

    def set_heuristic_multiplier(self, m):
        _chk(self.L.ufm_batch_set_heuristic_multiplier(self.h, float(m)), "ufm_batch_set_heuristic_multiplier")

    def set_profiling(self, on):
        _chk(self.L.ufm_batch_set_profiling(self.h, int(on)), "ufm_batch_set_profiling")

    def stream_ptr(self, shard=0):
        return int(self.L.ufm_batch_stream(self.h, shard) or 0)

    def shards(self):
        return self.L.ufm_batch_shards(self.h)

    def read_map(self, i, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_batch_read_map(self.h, i, m.ctypes.data), "ufm_batch_read_map")
        return m

    def set_cspace(self, mask, anchor=None):
        """as Planner.set_cspace, for every map on every shard"""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _chk(self.L.ufm_batch_set_cspace(self.h, mask.ctypes.data, mw, mh, ar, ac), "ufm_batch_set_cspace")

    def read_raw_map(self, i, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_batch_read_raw_map(self.h, i, m.ctypes.data), "ufm_batch_read_raw_map")
        return m

    def track_costs(self, on=True):
        """as Planner.track_costs, for every map on every shard"""
        _chk(self.L.ufm_batch_track_costs(self.h, int(on)), "ufm_batch_track_costs")

    def read_cost_census(self, i=-1):
        """as Planner.read_cost_census, for map i; -1: all maps of the batch, summed"""
        return _read_census(lambda *a: self.L.ufm_batch_read_cost_census(self.h, int(i), *a), "ufm_batch_read_cost_census")

    def heuristic_multiplier(self):
        v = C.c_float(0.0)
        _chk(self.L.ufm_batch_heuristic_multiplier(self.h, C.byref(v)), "ufm_batch_heuristic_multiplier")
        return v.value

    def set_sensor(self, mask, anchor=None):
        """as Planner.set_sensor, for every map on every shard"""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _chk(self.L.ufm_batch_set_sensor(self.h, mask.ctypes.data, mw, mh, ar, ac), "ufm_batch_set_sensor")

    def set_survey(self, i, raster, width=None, length=None):
        """as Planner.set_survey, for map i"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_batch_set_survey_device if dev else self.L.ufm_batch_set_survey
        _chk(fn(self.h, int(i), ptr, width, length), "ufm_batch_set_survey")

    def reveal(self, centres, count=False):
        """ufm_batch_reveal: one launch per device for all maps; centres [n][2] = (row, col), row < 0 skips the map.  count: wait and
        return the changed cells per map (uint64 [n])"""
        c = np.ascontiguousarray(centres, np.int32).reshape(-1, 2)
        if len(c) != self.n:
            raise UfmError("one centre per map")
        out = np.zeros(self.n, np.uint64)
        _chk(self.L.ufm_batch_reveal(self.h, c.ctypes.data, out.ctypes.data if count else None), "ufm_batch_reveal")
        return out if count else None

    def read_survey(self, i, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_batch_read_survey(self.h, int(i), m.ctypes.data), "ufm_batch_read_survey")
        return m

    def set_image(self, i, img, taps=None, penalty=0, ksize=None, width=None, length=None):
        """as Planner.set_image, for map i"""
        ptr, width, length, dev, taps, keep = _image_args(img, taps, ksize, width, length)
        fn = self.L.ufm_batch_set_image_device if dev else self.L.ufm_batch_set_image
        _chk(fn(self.h, int(i), ptr, width, length, taps.ctypes.data, len(taps), int(penalty)), "ufm_batch_set_image")
        self._dims = (length + (0 if self.algo == ALGO_DFM else 1), width + (0 if self.algo == ALGO_DFM else 1))

    def set_layers(self, n):
        """as Planner.set_layers: one n for every map on every shard"""
        _chk(self.L.ufm_batch_set_layers(self.h, int(n)), "ufm_batch_set_layers")

    def patch_layer(self, i, k, patch, x, y, w=None, h=None):
        """as Planner.patch_layer, for map i"""
        ptr, w, h, dev, keep = _survey_args(patch, w, h)
        fn = self.L.ufm_batch_patch_layer_device if dev else self.L.ufm_batch_patch_layer
        _chk(fn(self.h, int(i), int(k), ptr, int(x), int(y), w, h), "ufm_batch_patch_layer")

    def set_layer(self, i, k, raster, width=None, length=None):
        """as Planner.set_layer, for map i"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_batch_set_layer_device if dev else self.L.ufm_batch_set_layer
        _chk(fn(self.h, int(i), int(k), ptr, width, length), "ufm_batch_set_layer")

    def set_layer_survey(self, i, k, raster, width=None, length=None):
        """as Planner.set_layer_survey, for map i"""
        ptr, width, length, dev, keep = _survey_args(raster, width, length)
        fn = self.L.ufm_batch_set_layer_survey_device if dev else self.L.ufm_batch_set_layer_survey
        _chk(fn(self.h, int(i), int(k), ptr, width, length), "ufm_batch_set_layer_survey")

    def read_layer(self, i, k, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_batch_read_layer(self.h, int(i), int(k), m.ctypes.data), "ufm_batch_read_layer")
        return m

    def read_layer_survey(self, i, k, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _chk(self.L.ufm_batch_read_layer_survey(self.h, int(i), int(k), m.ctypes.data), "ufm_batch_read_layer_survey")
        return m

    def set_start(self, i, x, y):
        _chk(self.L.ufm_batch_set_start(self.h, i, float(x), float(y)), "ufm_batch_set_start")

    def set_goal(self, i, x, y):
        _chk(self.L.ufm_batch_set_goal(self.h, i, float(x), float(y)), "ufm_batch_set_goal")

    def reset(self, i):
        _chk(self.L.ufm_batch_reset(self.h, i), "ufm_batch_reset")

    def step(self):
        rc = self.L.ufm_batch_step(self.h, C.byref(self.stats))
        if rc in (LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL):
            return rc
        _chk(rc, "ufm_batch_step")
        return rc

    def extract_paths(self, max_steps=20, lookahead=True, allow_indirect=True):
        """One launch for all maps: list of (points, step_costs, total_cost, total_dist)."""
        n = self.L.ufm_batch_size(self.h)
        cap_p, cap_c = 3 * max_steps + 1, 2 * max_steps
        pts = np.zeros((n, cap_p, 2), np.float32)
        costs = np.zeros((n, cap_c), np.float32)
        info = (PathInfo * n)()
        _chk(self.L.ufm_batch_extract_path(self.h, int(max_steps), int(lookahead), int(allow_indirect),
                                           pts.ctypes.data, cap_p, costs.ctypes.data, cap_c, info),
             "ufm_batch_extract_path")
        self.path_info = info
        return [(pts[k, :info[k].n_points].copy(), costs[k, :info[k].n_costs].copy(),
                 info[k].total_cost, info[k].total_dist) for k in range(n)]

    def extract_paths_from(self, map_index, starts, max_steps=20, lookahead=True, allow_indirect=True):
        """as Planner.extract_paths_from: start k is a position on map map_index[k] (any order, any number per map)"""
        mi = np.ascontiguousarray(map_index, np.int32).ravel()
        assert len(mi) == len(np.asarray(starts).reshape(-1, 2)), "one map index per start"
        out, self.path_infos = _paths_from(
            lambda n, s, *bufs: self.L.ufm_batch_extract_paths_from(self.h, n, mi.ctypes.data, s, int(max_steps), int(lookahead),
                                                                    int(allow_indirect), *bufs),
            "ufm_batch_extract_paths_from", starts, max_steps)
        return out

    def read_field(self, i):
        nx, ny = self._dims
        g = np.empty((nx, ny), dtype=np.float32)
        _chk(self.L.ufm_batch_read_field(self.h, i, 0, 0, nx, ny, g.ctypes.data, None), "ufm_batch_read_field")
        return g

    def set_param(self, name, value):
        _chk(self.L.ufm_batch_set_param(self.h, name.encode(), float(value)), "ufm_batch_set_param")

    def track_changes(self, on=True):
        """as Planner.track_changes, for every map"""
        _chk(self.L.ufm_batch_track_changes(self.h, int(on)), "ufm_batch_track_changes")

    def read_changes(self, i, want_info=False, cap=None):
        """as Planner.read_changes, for map i"""
        out = _read_changes(lambda *a: self.L.ufm_batch_read_changes(self.h, i, *a), "ufm_batch_read_changes", want_info, cap)
        return out if cap is not None else out[:3]

    def check_info(self):
        """as Planner.check_info, summed over the maps"""
        out = (C.c_uint64 * 6)()
        _chk(self.L.ufm_batch_check_info(self.h, C.addressof(out)), "ufm_batch_check_info")
        return tuple(int(v) for v in out)

    def check_layout(self):
        bad = (C.c_uint64 * 2)()
        _chk(self.L.ufm_batch_check_layout(self.h, C.addressof(bad), C.addressof(bad) + 8), "ufm_batch_check_layout")
        return int(bad[0]), int(bad[1])
