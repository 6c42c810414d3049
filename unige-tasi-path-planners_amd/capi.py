"""ctypes binding of include/ufm.h (libufm.so).  No CPU fallback."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_FN = None     # the bound functions by handle kind, {"p": planner, "b": batch, "f": no handle}: _FN["p"].set_map is ufm_set_map

ALGO_FD, ALGO_SG, ALGO_DFM = 0, 1, 2
LOOP_OK, LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL = 0, -1, -2
MAX_LAYERS = 4     # UFM_MAX_LAYERS


class UfmError(RuntimeError):
    pass


class Stats(C.Structure):
    """ufm_stats (include/ufm.h; tests/test_capi_surface.py holds the two against each other)"""
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


# ufm_score (include/ufm_score.h): the record of one scored path, as score_paths returns it
SCORE_DTYPE = np.dtype([("cost", "<f4"), ("cost_before", "<f4"), ("dist", "<f4"), ("blocked_at", "<f4"),
                        ("blocked_segment", "<i4"), ("pieces", "<i4")])


def _path_arrays(paths):
    """(points float32 [total, 2], offsets int32 [n + 1]) of `paths`: a list of [n_i, 2] arrays, or the pair (points, offsets) itself"""
    if isinstance(paths, tuple) and len(paths) == 2 and np.ndim(paths[1]) == 1 and np.ndim(paths[0]) == 2:
        pts, off = paths
        return np.ascontiguousarray(pts, np.float32).reshape(-1, 2), np.ascontiguousarray(off, np.int32)
    parts = [np.asarray(p, np.float32).reshape(-1, 2) for p in paths]
    off = np.zeros(len(parts) + 1, np.int32)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    pts = np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts, np.float32), off


# The surface, once: (operation, forms, argument types after the handle and the map index).  Forms: "p" ufm_<op>(planner, ...);
# "b" ufm_batch_<op>(batch, ...); "B" ufm_batch_<op>(batch, map index, ...); "f" ufm_<op>(...), no handle.  An operation whose two
# forms take different arguments has a row for each.  SYMBOLS, every argtypes and every restype come from here.
_vp, _f, _i = C.c_void_p, C.c_float, C.c_int
_pi, _pvp = C.POINTER(C.c_int), C.POINTER(C.c_void_p)
_RASTER, _RECT, _MASK, _IMAGE = [_vp, _i, _i], [_vp, _i, _i, _i, _i], [_vp, _i, _i, _i, _i], [_vp, _i, _i, _vp, _i, _i]
_WALK = [_i, _i, _i, _vp, _i, _vp, _i]       # max_steps, lookahead, allow_indirect, points, cap, costs, cap
_OPS = [
    ("version", "f", []), ("tile_edge", "f", []), ("gaussian_taps", "f", [_i, _vp]),
    ("create", "f", [_pvp, _i, _i, _i, _i]), ("batch_create", "f", [_pvp, _i, _i, _i, _i, _i]),
    ("batch_create_sharded", "f", [_pvp, _i, _i, _i, _i, _pi, _i]),
    ("destroy", "pb", []), ("size", "b", []), ("shards", "b", []), ("stream", "p", []), ("stream", "b", [_i]),
    # the whole handle
    ("set_occupancy_threshold", "pb", [_f]), ("set_heuristic_multiplier", "pb", [_f]), ("heuristic_multiplier", "pb", [C.POINTER(_f)]),
    ("set_param", "pb", [C.c_char_p, C.c_double]), ("set_profiling", "pb", [_i]), ("track_costs", "pb", [_i]), ("track_changes", "pb", [_i]),
    ("set_cspace", "pb", _MASK), ("set_sensor", "pb", _MASK), ("set_layers", "pb", [_i]),
    ("step", "pb", [C.POINTER(Stats)]), ("check_layout", "pb", [_vp, _vp]), ("check_info", "pb", [_vp]),
    ("extract_path", "pb", _WALK + [C.POINTER(PathInfo)]),
    ("extract_paths_from", "p", [_i, _vp] + _WALK + [_vp]), ("extract_paths_from", "b", [_i, _vp, _vp] + _WALK + [_vp]),
    ("reveal", "p", [_i, _i, _vp]), ("reveal", "b", [_vp, _vp]),
    # one map
    ("set_map", "pB", _RASTER), ("set_map_device", "pB", _RASTER), ("patch_map", "pB", _RECT), ("patch_map_device", "pB", _RECT),
    ("set_image", "pB", _IMAGE), ("set_image_device", "pB", _IMAGE),
    ("read_map", "pB", [_vp]), ("read_raw_map", "pB", [_vp]), ("read_cost_census", "pB", [_vp, _pi, _pi]),
    ("set_survey", "pB", _RASTER), ("set_survey_device", "pB", _RASTER), ("read_survey", "pB", [_vp]),
    ("patch_layer", "pB", [_i] + _RECT), ("patch_layer_device", "pB", [_i] + _RECT),
    ("set_layer", "pB", [_i] + _RASTER), ("set_layer_device", "pB", [_i] + _RASTER),
    ("set_layer_survey", "pB", [_i] + _RASTER), ("set_layer_survey_device", "pB", [_i] + _RASTER),
    ("read_layer", "pB", [_i, _vp]), ("read_layer_survey", "pB", [_i, _vp]),
    ("reset", "pB", []), ("set_start", "pB", [_f, _f]), ("set_goal", "pB", [_f, _f]),
    ("read_field", "pB", [_i, _i, _i, _i, _vp, _vp]), ("read_changes", "pB", [_i, _vp, _vp, _vp, _vp]),
    # a planner alone
    ("field_dims", "p", [_pi, _pi]), ("read_info", "p", [_i, _i, _i, _i, _vp]), ("read_info_derived", "p", [_i, _i, _i, _i, _vp]),
    ("read_queue", "p", [_i, _vp, _vp, _vp]),
]
_RESTYPE = {"version": C.c_char_p, "stream": _vp}       # everything else returns a code
_FORMS = {"p": ("ufm_", [_vp]), "b": ("ufm_batch_", [_vp]), "B": ("ufm_batch_", [_vp, _i]), "f": ("ufm_", [])}
# every symbol include/ufm.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [_FORMS[form][0] + op for op, forms, _ in _OPS for form in forms]
# Trajectory scoring is a header of its own, include/ufm_score.h, which ufm.h includes (ufm.h's own list of entry points is held to a
# fixed count by tests/test_capi_surface.py): its rows, in the same format, bound by the same loop; SCORE_SYMBOLS is what it declares
# (checked by tests/test_score_surface.py).  A second table is debt: whoever may next change that count folds these rows into _OPS and
# the declarations into ufm.h.
_SCORE_OPS = [
    ("score_paths", "p", [_i, _vp, _vp, _vp]), ("score_paths", "b", [_i, _vp, _vp, _vp, _vp]),
    ("score_paths_device", "pB", [_i, _i, _vp, _vp, _vp]),
]
SCORE_SYMBOLS = [_FORMS[form][0] + op for op, forms, _ in _SCORE_OPS for form in forms]
# The graded footprint, likewise: include/ufm_cspace_graded.h, GRADED_SYMBOLS (checked by tests/test_cspace_graded_surface.py); the
# same debt.
_GRADED_OPS = [("set_cspace_graded", "pb", _MASK), ("cspace_cone", "f", [_i, _i, _i, _vp])]
GRADED_SYMBOLS = [_FORMS[form][0] + op for op, forms, _ in _GRADED_OPS for form in forms]
CSPACE_OUTSIDE, CSPACE_MAX_LEVELS = 255, 16     # UFM_CSPACE_OUTSIDE, UFM_CSPACE_MAX_LEVELS

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
    global _LIB, _FN
    if _LIB is not None:
        return _LIB
    so = library_path()
    if not os.path.exists(so):
        raise UfmError("libufm.so is not built (run `make -C unige-tasi-path-planners_amd` "
                       "or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(so)
    fn = {kind: types.SimpleNamespace() for kind in "pbf"}
    for op, forms, args in _OPS + _SCORE_OPS + _GRADED_OPS:
        for form in forms:
            prefix, head = _FORMS[form]
            func = getattr(L, prefix + op)
            func.argtypes = head + args
            func.restype = _RESTYPE.get(op, C.c_int)
            setattr(fn[form.lower()], op, func)
    _LIB, _FN = L, fn
    return L


def _chk(rc, what):
    if rc != 0:
        raise UfmError("%s failed with code %d" % (what, rc))


def _call(func, *args):
    """a library call that returns a code: UfmError with the entry point's name unless it is 0"""
    rc = func(*args)
    if rc != 0:
        raise UfmError("%s failed with code %d" % (func.__name__, rc))


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


def cspace_cone(inner_d, outer_d, step):
    """ufm_cspace_cone: the cone footprint as ufm_set_cspace_graded takes it -- drop 0 on the disc of diameter inner_d, then `step` more
    per ring of one cell out to the disc of diameter outer_d (at most 254), 255 beyond; a uint8 matrix of edge 2 * (outer_d // 2) + 1
    with the anchor at its centre.  The C definition, called, not restated."""
    r = int(outer_d) // 2
    fits = 0 <= r <= 15                        # (otherwise the call is made without a buffer, for its error)
    drop = np.zeros((2 * r + 1, 2 * r + 1) if fits else (1, 1), np.uint8)
    load_library()
    _call(_FN["f"].cspace_cone, int(inner_d), int(outer_d), int(step), drop.ctypes.data if fits else None)
    return drop


def sensor_disc(radius):
    """The field of view harness.round_patch_update reveals (run_simulator.py:9-28), as ufm_set_sensor takes it: the (2 r + 1)^2 uint8 matrix
    of x^2 + y^2 <= r^2 with the anchor at its centre."""
    r = int(radius)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (xx * xx + yy * yy <= r * r).astype(np.uint8)


def _survey_args(raster, width=None, length=None):
    """("_device" or "", pointer, width, length, the object to keep alive) of a raster: a host matrix, or a device buffer (anything with
    .ptr, e.g. the tests' DeviceBytes) with its dimensions -- its own .shape = (length, width), or the two keywords"""
    if hasattr(raster, "ptr"):
        if width is None or length is None:
            if not hasattr(raster, "shape"):
                raise UfmError("a device survey needs width and length")
            length, width = raster.shape
        return "_device", raster.ptr, int(width), int(length), raster
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    if raster.ndim != 2:
        raise UfmError("a survey is a matrix")
    return "", raster.ctypes.data, raster.shape[1], raster.shape[0], raster


def gaussian_taps(ksize):
    """ufm_gaussian_taps: the taps cv2.GaussianBlur(img, (k, k), 0) applies to 8-bit images (uint16 [ksize], their sum 256) -- the C
    definition of harness.gaussian_kernel_fixed; ksize odd, 1 .. 31"""
    ksize = int(ksize)
    taps = np.zeros(max(ksize, 1), np.uint16)
    load_library()
    _call(_FN["f"].gaussian_taps, ksize, taps.ctypes.data)
    return taps


def _image_taps(taps, ksize):
    """the filter of set_image as uint16: `taps`, or the Gaussian of `ksize`, or -- neither given -- {256}, no blur"""
    if taps is not None and ksize is not None:
        raise UfmError("set_image takes taps or ksize, not both")
    if taps is None:
        taps = gaussian_taps(1 if ksize is None else ksize)
    taps = np.ascontiguousarray(taps)
    if taps.ndim != 1 or taps.size == 0 or (taps < 0).any() or (taps > 65535).any():
        raise UfmError("taps are a vector of uint16")
    return taps.astype(np.uint16)


class _Handle:
    """What Planner and BatchPlanner share: the body of every operation, once.  `at` says where a per-map operation applies -- () for
    a planner, (i,) for map i of a batch -- and goes between the handle and the arguments, as in the C signatures; the classes'
    own methods only supply it.  Operations on the whole handle have one signature and are public here."""
    _kind = None     # "p" / "b": which functions of _FN

    def _open(self, create, *args):
        self.L = load_library()
        self._F = F = _FN[self._kind]
        h = C.c_void_p()
        _call(getattr(_FN["f"], create), C.byref(h), *args)
        self.h = h
        self.stats = Stats()
        # the calls inside a replan loop (step, set_start, patch_map, patch_map_host) are bound here and written out in each class: a
        # shared body would put a second frame and an argument tuple into every call of the loop bench.py times
        self._step, self._stats_ref = F.step, C.byref(self.stats)
        self._set_start, self._patch_map = F.set_start, F.patch_map

    def close(self):
        if getattr(self, "h", None):
            self._F.destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the whole handle ----
    def set_occupancy_threshold(self, t):
        _call(self._F.set_occupancy_threshold, self.h, float(t))

    def set_heuristic_multiplier(self, m):
        _call(self._F.set_heuristic_multiplier, self.h, float(m))

    def heuristic_multiplier(self):
        """the multiplier the last step used: the caller's, or with set_param("auto_multiplier", 1) the census' minimum (a batch: over
        all its maps)"""
        v = C.c_float(0.0)
        _call(self._F.heuristic_multiplier, self.h, C.byref(v))
        return v.value

    def set_param(self, name, value):
        _call(self._F.set_param, self.h, name.encode(), float(value))

    def set_profiling(self, on):
        _call(self._F.set_profiling, self.h, int(on))

    def track_costs(self, on=True):
        """the cost census (ufm_track_costs): 256 exact counters of the planning raster's values, kept under patches; a batch: for
        every map on every shard"""
        _call(self._F.track_costs, self.h, int(on))

    def track_changes(self, on=True):
        """step deltas (ufm_track_changes): the engine keeps a baseline -- what read_changes last delivered, empty at first; a batch:
        for every map"""
        _call(self._F.track_changes, self.h, int(on))

    def set_cspace(self, mask, anchor=None):
        """ufm_set_cspace: the vehicle's footprint (uint8 matrix, non-zero = set; anchor (row, col), None: the centre (mh // 2, mw // 2)).
        Before the first set_map; from then on set_map / patch_map take the RAW raster and the engine plans on its dilation.  A batch:
        for every map on every shard"""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _call(self._F.set_cspace, self.h, mask.ctypes.data, mw, mh, ar, ac)

    def set_cspace_graded(self, drop, anchor=None):
        """ufm_set_cspace_graded: a footprint with a drop per cell (uint8 matrix, 255 = outside; drop[anchor] == 0; at most 16 distinct
        values): planning = max over the footprint of max(raw - drop, 0).  cspace_cone(inner_d, outer_d, step) makes the usual one.
        Before the first set_map, as set_cspace, which it replaces and is replaced by.  A batch: for every map on every shard"""
        drop, mw, mh, ar, ac = _cspace_args(drop, anchor)
        _call(self._F.set_cspace_graded, self.h, drop.ctypes.data, mw, mh, ar, ac)

    def set_sensor(self, mask, anchor=None):
        """ufm_set_sensor: the field of view (uint8 matrix, non-zero = seen; anchor (row, col), None: the centre); sensor_disc(r) is the
        reference simulator's.  A batch: for every map on every shard"""
        mask, mw, mh, ar, ac = _cspace_args(mask, anchor)
        _call(self._F.set_sensor, self.h, mask.ctypes.data, mw, mh, ar, ac)

    def set_layers(self, n):
        """ufm_set_layers: n rasters per map whose element-wise maximum is the caller's raster (1: off, the default); before the first
        set_map / set_image.  A batch: one n for every map on every shard"""
        _call(self._F.set_layers, self.h, int(n))

    def check_layout(self):
        """(ring entries, cost-window bytes) that differ from the values they copy; (0, 0) when sound"""
        bad = (C.c_uint64 * 2)()
        _call(self._F.check_layout, self.h, C.addressof(bad), C.addressof(bad) + 8)
        return int(bad[0]), int(bad[1])

    def check_info(self):
        """stored back-pointers (level-1/2 planners): (elements with a value, without a back-pointer, whose parent triangle does not
        give the value but a larger one, whose dependence bits are off, whose parent gives a smaller value -- waiting to be
        lowered, beyond the start's key --, unsupported ones at / beyond the start's key: queued invalidations); [1:4] are 0 when sound.
        MS-DFM level 1: the named candidate against the value within 8 ulp (include/ufm.h); level 0 raises UfmError (no Info).  A batch:
        summed over the maps"""
        out = (C.c_uint64 * 6)()
        _call(self._F.check_info, self.h, C.addressof(out))
        return tuple(int(v) for v in out)

    def _extract(self, n, max_steps, lookahead, allow_indirect, pre=None):
        """the walks of one call -- extract_path(s): one per map, from its start (pre None); extract_paths_from: `pre` = the C arguments in
        front of the walk's, n starts --: ([(points, step_costs, total_cost, total_dist)], the PathInfo array)"""
        cap_p, cap_c = 3 * max_steps + 1, 2 * max_steps
        pts = np.zeros((max(n, 1), cap_p, 2), np.float32)
        costs = np.zeros((max(n, 1), cap_c), np.float32)
        info = (PathInfo * max(n, 1))()
        func, pre = (self._F.extract_path, ()) if pre is None else (self._F.extract_paths_from, pre)
        _call(func, self.h, *pre, int(max_steps), int(lookahead), int(allow_indirect), pts.ctypes.data, cap_p, costs.ctypes.data, cap_c, info)
        return [(pts[k, :info[k].n_points].copy(), costs[k, :info[k].n_costs].copy(),
                 info[k].total_cost, info[k].total_dist) for k in range(n)], info

    def _score(self, paths, pre=()):
        """score_paths of both classes (ufm_score_paths / ufm_batch_score_paths; `pre`: a batch's map indices): one SCORE_DTYPE record
        per path, in the caller's order"""
        pts, off = _path_arrays(paths)
        n = len(off) - 1
        out = np.zeros(max(n, 1), SCORE_DTYPE)
        keep = np.zeros((1, 2), np.float32) if len(pts) == 0 else pts        # (an address even when no path has a point)
        _call(self._F.score_paths, self.h, n, *pre, off.ctypes.data, keep.ctypes.data, out.ctypes.data)
        return out[:n]

    def _score_device(self, at, n_paths, total_points, dev_offsets, dev_points, dev_out):
        _call(self._F.score_paths_device, self.h, *at, int(n_paths), int(total_points), dev_offsets, dev_points, dev_out)

    # ---- one map: `at` ----
    def _raster_set(self, at, op, raster, width, length, *more):
        """set_map / set_survey / set_layer ...: ufm_<op> or ufm_<op>_device by where the raster lives"""
        dev, ptr, width, length, keep = _survey_args(raster, width, length)
        _call(getattr(self._F, op + dev), self.h, *at, ptr, width, length, *more)
        return width, length

    def _raster_read(self, at, op, width, length):
        m = np.empty((length, width), dtype=np.uint8)
        _call(getattr(self._F, op), self.h, *at, m.ctypes.data)
        return m

    def _new_raster(self, width, length):      # the field's dimensions, for a batch's read_field
        edge = 0 if self.algo == ALGO_DFM else 1
        self._dims = (length + edge, width + edge)

    def _set_map(self, at, m):
        self._new_raster(*self._raster_set(at, "set_map", np.ascontiguousarray(m, dtype=np.uint8), None, None))

    def _set_map_device(self, at, dev_ptr, width, length):
        _call(self._F.set_map_device, self.h, *at, dev_ptr, width, length)
        self._new_raster(width, length)

    def _set_image(self, at, img, taps, penalty, ksize, width, length):
        taps = _image_taps(taps, ksize)
        self._new_raster(*self._raster_set(at, "set_image", img, width, length, taps.ctypes.data, len(taps), int(penalty)))

    def _patch_map_device(self, at, dev_ptr, x, y, w, h):
        _call(self._F.patch_map_device, self.h, *at, dev_ptr, int(x), int(y), int(w), int(h))

    def _patch_layer(self, at, k, patch, x, y, w, h):
        dev, ptr, w, h, keep = _survey_args(patch, w, h)
        _call(getattr(self._F, "patch_layer" + dev), self.h, *at, int(k), ptr, int(x), int(y), w, h)

    def _read_cost_census(self, at):
        hist = np.zeros(256, np.uint64)
        mn, mx = C.c_int(0), C.c_int(0)
        _call(self._F.read_cost_census, self.h, *at, hist.ctypes.data, C.byref(mn), C.byref(mx))
        return hist, mn.value, mx.value

    def _read_field(self, at, x0, y0, nx, ny, want_rhs):
        g = np.empty((nx, ny), dtype=np.float32)
        rhs = np.empty((nx, ny), dtype=np.float32) if want_rhs else None
        _call(self._F.read_field, self.h, *at, x0, y0, nx, ny, g.ctypes.data, rhs.ctypes.data if want_rhs else None)
        return g, rhs

    def _read_changes(self, at, want_info, cap):
        """a counting call sizes the buffers (cap None), the second call delivers: (xy int32 [n, 2], g float32 [n], info int32 [n, 2] |
        None, total); with an explicit cap that is too small n = 0 and nothing was committed.  Without a cap the total is left off."""
        total, func, given = C.c_int(0), self._F.read_changes, cap is not None
        if cap is None:
            _call(func, self.h, *at, 0, None, None, None, C.addressof(total))
            cap = total.value
        xy = np.zeros((max(cap, 1), 2), np.int32)
        g = np.zeros(max(cap, 1), np.float32)
        info = np.zeros((max(cap, 1), 2), np.int32) if want_info else None
        if cap or given:
            _call(func, self.h, *at, cap, xy.ctypes.data, g.ctypes.data, info.ctypes.data if want_info else None, C.addressof(total))
        n = total.value if total.value <= cap else 0
        out = xy[:n], g[:n], (info[:n] if want_info else None), total.value
        return out if given else out[:3]


class Planner(_Handle):
    """Mirror of the reference planner surface (ReplannerBase.h:39-123):
    reset / set_occupancy_threshold / set_heuristic_multiplier / set_map /
    patch_map / set_start / set_goal / step, public stats u_time, p_time,
    num_nodes_updated, num_nodes_expanded, and a dense field view in place of
    ExpandedMap::get_g / get_rhs."""
    _kind = "p"

    def __init__(self, algo, opt_lvl=0, use_heuristic=False, device=0, follow_info=False):
        self._open("create", algo, opt_lvl, int(use_heuristic), device)
        if follow_info:     # MS-DFM level 1: invalidation along the stored back-pointers (ufm_set_param "dfm_follow_info")
            self.set_param("dfm_follow_info", 1)
        self.algo = algo
        self.u_time = 0.0
        self.p_time = 0.0
        self.num_nodes_updated = 0
        self.num_nodes_expanded = 0

    def reset(self):
        _call(self._F.reset, self.h)

    def set_map(self, m):
        self._set_map((), m)

    def set_map_device(self, dev_ptr, width, length):
        self._set_map_device((), dev_ptr, width, length)

    def patch_map(self, patch, x, y):
        patch = np.ascontiguousarray(patch, dtype=np.uint8)
        h, w = patch.shape
        _chk(self._patch_map(self.h, patch.ctypes.data, int(x), int(y), w, h), "ufm_patch_map")

    def patch_map_device(self, dev_ptr, x, y, w, h):
        self._patch_map_device((), dev_ptr, x, y, w, h)

    def patch_map_host(self, host_ptr, x, y, w, h):
        """ufm_patch_map with the address of a host buffer (a caller that keeps its patches in one array: no numpy view per call)"""
        _chk(self._patch_map(self.h, host_ptr, int(x), int(y), int(w), int(h)), "ufm_patch_map")

    def set_start(self, x, y):
        _chk(self._set_start(self.h, float(x), float(y)), "ufm_set_start")

    def set_goal(self, x, y):
        _call(self._F.set_goal, self.h, float(x), float(y))

    def stream_ptr(self):
        """hipStream_t the engine's kernels run on (e.g. for torch.cuda.ExternalStream)"""
        return int(self._F.stream(self.h) or 0)

    def step(self):
        rc = self._step(self.h, self._stats_ref)
        if rc in (LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL):
            return rc
        _chk(rc, "ufm_step")
        self.u_time, self.p_time = self.stats.u_ms, self.stats.p_ms
        self.num_nodes_updated = self.stats.updated
        self.num_nodes_expanded = self.stats.expanded
        return rc

    def dims(self):
        a, b = C.c_int(), C.c_int()
        _call(self._F.field_dims, self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def _window(self, x0, y0, nx, ny):
        ex, ey = self.dims()
        return x0, y0, (ex - x0 if nx is None else nx), (ey - y0 if ny is None else ny)

    def read_field(self, x0=0, y0=0, nx=None, ny=None):
        return self._read_field((), *self._window(x0, y0, nx, ny), True)

    def g(self):
        return self.read_field()[0]

    def read_info(self, x0=0, y0=0, nx=None, ny=None, derived=False):
        """back-pointers (the reference's INFO of level-1/2 planners): int32 [nx][ny][2] -- the stored ones, or
        (derived=True) those min_rhs<level>() derives from the field alone"""
        x0, y0, nx, ny = self._window(x0, y0, nx, ny)
        out = np.empty((nx, ny, 2), np.int32)
        _call(self._F.read_info_derived if derived else self._F.read_info, self.h, x0, y0, nx, ny, out.ctypes.data)
        return out

    def extract_path(self, max_steps=20, lookahead=True, allow_indirect=True):
        """LinearInterpolationPathExtractor::extract_path on the device:
        returns (points[n,2], step_costs[m], total_cost, total_dist); the call's info is kept in
        self.path_info."""
        out, info = self._extract(1, max_steps, lookahead, allow_indirect)
        self.path_info = info[0]
        return out[0]

    def extract_paths_from(self, starts, max_steps=20, lookahead=True, allow_indirect=True):
        """position queries (ufm_extract_paths_from): paths from the positions `starts` ([n, 2]) over the field as it stands, in one
        call, without touching the planner's own start.  Returns a list of (points, step_costs, total_cost, total_dist) in the order
        of `starts`; the calls' infos are kept in self.path_infos."""
        starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 2)
        out, self.path_infos = self._extract(len(starts), max_steps, lookahead, allow_indirect, (len(starts), starts.ctypes.data))
        return out

    def score_paths(self, paths):
        """trajectory scoring (ufm_score_paths): what the caller's polylines cost on the planning raster, and whether they are blocked.
        `paths`: a list of [n_i, 2] arrays of (x, y), or (points [total, 2], offsets [n + 1]).  Returns a structured array
        (SCORE_DTYPE: cost, cost_before, dist, blocked_at, blocked_segment, pieces), one record per path.  Read-only on the planner."""
        return self._score(paths)

    def score_paths_device(self, n_paths, total_points, dev_offsets, dev_points, dev_out):
        """ufm_score_paths_device: offsets (int32 [n_paths + 1]), points (float32 [total_points, 2]) and records (ufm_score [n_paths])
        as device addresses, e.g. tensor.data_ptr(); queued on the engine's stream (stream_ptr()), nothing is waited for"""
        self._score_device((), n_paths, total_points, dev_offsets, dev_points, dev_out)

    def read_map(self, width, length):
        return self._raster_read((), "read_map", width, length)

    def read_raw_map(self, width, length):
        """the raster as the caller gave it, patches applied (read_map: the planning raster, its dilation); only with a footprint set"""
        return self._raster_read((), "read_raw_map", width, length)

    def read_cost_census(self):
        """(hist uint64 [256], min_cost, max_cost) of the planning raster as it stands"""
        return self._read_cost_census(())

    def set_survey(self, raster, width=None, length=None):
        """ufm_set_survey / _device: what the sensor would see, [length][width] like the map -- a host matrix, or a device buffer (.ptr)
        with width and length"""
        self._raster_set((), "set_survey", raster, width, length)

    def reveal(self, row, col, count=False):
        """ufm_reveal: uncover the field of view around cell (row, col).  count: wait and return the number of cells that changed"""
        n = C.c_uint64(0)
        _call(self._F.reveal, self.h, int(row), int(col), C.addressof(n) if count else None)
        return int(n.value) if count else None

    def read_survey(self, width, length):
        return self._raster_read((), "read_survey", width, length)

    def set_image(self, img, taps=None, penalty=0, ksize=None, width=None, length=None):
        """ufm_set_image / _device: the grey-scale bitmap becomes the map (blurred by `taps` -- or gaussian_taps(ksize) --, complemented,
        0 -> 1, + penalty saturating) and its survey (complemented, 0 -> 1) in one launch: harness.simulation_data on the device.  A host
        matrix, or a device buffer (.ptr) with width and length"""
        self._set_image((), img, taps, penalty, ksize, width, length)

    def patch_layer(self, k, patch, x, y, w=None, h=None):
        """ufm_patch_layer / _device: the bytes into layer k over rows x .., columns y ..; the map takes the maximum over the layers there.
        A host matrix, or a device buffer (.ptr) with w and h"""
        self._patch_layer((), k, patch, x, y, w, h)

    def set_layer(self, k, raster, width=None, length=None):
        """ufm_set_layer / _device: layer k wholesale -- a whole-map patch, not a set_map: the field is kept"""
        self._raster_set((int(k),), "set_layer", raster, width, length)

    def set_layer_survey(self, k, raster, width=None, length=None):
        """ufm_set_layer_survey / _device: what the sensor would see of layer k (k = 0: set_survey)"""
        self._raster_set((int(k),), "set_layer_survey", raster, width, length)

    def read_layer(self, k, width, length):
        return self._raster_read((int(k),), "read_layer", width, length)

    def read_layer_survey(self, k, width, length):
        return self._raster_read((int(k),), "read_layer_survey", width, length)

    def read_queue(self, cap=None):
        """the reference's priority_queue as a caller could observe it between two steps: the elements that are not consistent.
        Returns (xy int32 [n, 2], g float32 [n], rhs float32 [n], total); n = min(total, cap), cap None: all of them"""
        total = C.c_int(0)
        if cap is None:
            _call(self._F.read_queue, self.h, 0, None, None, C.addressof(total))
            cap = total.value
        xy = np.zeros((max(cap, 1), 2), np.int32)
        gr = np.zeros((max(cap, 1), 2), np.float32)
        _call(self._F.read_queue, self.h, cap, xy.ctypes.data, gr.ctypes.data, C.addressof(total))
        n = min(total.value, cap)
        return xy[:n], gr[:n, 0].copy(), gr[:n, 1].copy(), total.value

    def read_changes(self, want_info=False, cap=None):
        """the elements whose value (want_info: or Info pair) differs from the baseline, all or nothing:
        (xy int32 [n, 2], g float32 [n] -- +inf: the element lost its value --, info int32 [n, 2] | None); the baseline advances.
        cap: deliver only if the delta has at most that many records; then returns (xy, g, info, total) -- n = 0 and nothing
        committed if total > cap"""
        return self._read_changes((), want_info, cap)


class BatchPlanner(_Handle):
    """Batch of independent, equally sized map instances: on one device, or (devices=[...]) spread over several
    in contiguous blocks, one engine per device inside the one handle.  Every per-map method is Planner's with the
    map index in front."""
    _kind = "b"

    def __init__(self, n_maps, algo, opt_lvl=0, use_heuristic=False, device=0, devices=None, follow_info=False):
        if devices is None:
            self._open("batch_create", n_maps, algo, opt_lvl, int(use_heuristic), device)
        else:
            self._open("batch_create_sharded", n_maps, algo, opt_lvl, int(use_heuristic), (C.c_int * len(devices))(*devices), len(devices))
        if follow_info:     # as Planner's
            self.set_param("dfm_follow_info", 1)
        self.n = n_maps
        self.algo = algo

    def set_map(self, i, m):
        self._set_map((i,), m)

    def set_map_device(self, i, dev_ptr, width, length):
        self._set_map_device((i,), dev_ptr, width, length)

    def patch_map(self, i, patch, x, y):
        patch = np.ascontiguousarray(patch, dtype=np.uint8)
        h, w = patch.shape
        _chk(self._patch_map(self.h, i, patch.ctypes.data, int(x), int(y), w, h), "ufm_batch_patch_map")

    def patch_map_device(self, i, dev_ptr, x, y, w, h):
        self._patch_map_device((i,), dev_ptr, x, y, w, h)

    def stream_ptr(self, shard=0):
        return int(self._F.stream(self.h, shard) or 0)

    def shards(self):
        return self._F.shards(self.h)

    def read_map(self, i, width, length):
        return self._raster_read((i,), "read_map", width, length)

    def read_raw_map(self, i, width, length):
        return self._raster_read((i,), "read_raw_map", width, length)

    def read_cost_census(self, i=-1):
        """as Planner.read_cost_census, for map i; -1: all maps of the batch, summed"""
        return self._read_cost_census((int(i),))

    def set_survey(self, i, raster, width=None, length=None):
        """as Planner.set_survey, for map i"""
        self._raster_set((int(i),), "set_survey", raster, width, length)

    def reveal(self, centres, count=False):
        """ufm_batch_reveal: one launch per device for all maps; centres [n][2] = (row, col), row < 0 skips the map.  count: wait and
        return the changed cells per map (uint64 [n])"""
        c = np.ascontiguousarray(centres, np.int32).reshape(-1, 2)
        if len(c) != self.n:
            raise UfmError("one centre per map")
        out = np.zeros(self.n, np.uint64)
        _call(self._F.reveal, self.h, c.ctypes.data, out.ctypes.data if count else None)
        return out if count else None

    def read_survey(self, i, width, length):
        return self._raster_read((int(i),), "read_survey", width, length)

    def set_image(self, i, img, taps=None, penalty=0, ksize=None, width=None, length=None):
        """as Planner.set_image, for map i"""
        self._set_image((int(i),), img, taps, penalty, ksize, width, length)

    def patch_layer(self, i, k, patch, x, y, w=None, h=None):
        """as Planner.patch_layer, for map i"""
        self._patch_layer((int(i),), k, patch, x, y, w, h)

    def set_layer(self, i, k, raster, width=None, length=None):
        """as Planner.set_layer, for map i"""
        self._raster_set((int(i), int(k)), "set_layer", raster, width, length)

    def set_layer_survey(self, i, k, raster, width=None, length=None):
        """as Planner.set_layer_survey, for map i"""
        self._raster_set((int(i), int(k)), "set_layer_survey", raster, width, length)

    def read_layer(self, i, k, width, length):
        return self._raster_read((int(i), int(k)), "read_layer", width, length)

    def read_layer_survey(self, i, k, width, length):
        return self._raster_read((int(i), int(k)), "read_layer_survey", width, length)

    def set_start(self, i, x, y):
        _chk(self._set_start(self.h, i, float(x), float(y)), "ufm_batch_set_start")

    def set_goal(self, i, x, y):
        _call(self._F.set_goal, self.h, i, float(x), float(y))

    def reset(self, i):
        _call(self._F.reset, self.h, i)

    def step(self):
        rc = self._step(self.h, self._stats_ref)
        if rc not in (LOOP_FAILURE_NO_GRAPH, LOOP_FAILURE_NO_GOAL):
            _chk(rc, "ufm_batch_step")
        return rc

    def extract_paths(self, max_steps=20, lookahead=True, allow_indirect=True):
        """One launch for all maps: list of (points, step_costs, total_cost, total_dist)."""
        out, self.path_info = self._extract(self._F.size(self.h), max_steps, lookahead, allow_indirect)
        return out

    def extract_paths_from(self, map_index, starts, max_steps=20, lookahead=True, allow_indirect=True):
        """as Planner.extract_paths_from: start k is a position on map map_index[k] (any order, any number per map)"""
        mi = np.ascontiguousarray(map_index, np.int32).ravel()
        starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 2)
        assert len(mi) == len(starts), "one map index per start"
        out, self.path_infos = self._extract(len(starts), max_steps, lookahead, allow_indirect, (len(starts), mi.ctypes.data, starts.ctypes.data))
        return out

    def score_paths(self, map_index, paths):
        """as Planner.score_paths: path k lies on map map_index[k] (any order, any number per map)"""
        mi = np.ascontiguousarray(map_index, np.int32).ravel()
        pts, off = _path_arrays(paths)
        if len(mi) != len(off) - 1:
            raise UfmError("one map index per path")
        return self._score((pts, off), (mi.ctypes.data,))

    def score_paths_device(self, i, n_paths, total_points, dev_offsets, dev_points, dev_out):
        """as Planner.score_paths_device: every path on map i, the buffers on that map's device, queued on its shard's stream"""
        self._score_device((int(i),), n_paths, total_points, dev_offsets, dev_points, dev_out)

    def read_field(self, i):
        return self._read_field((i,), 0, 0, *self._dims, False)[0]

    def read_changes(self, i, want_info=False, cap=None):
        """as Planner.read_changes, for map i"""
        return self._read_changes((i,), want_info, cap)
