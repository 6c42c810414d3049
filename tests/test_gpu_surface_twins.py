"""GPU: a planner is a batch of one.  Every operation that exists as ufm_X(planner, ...) and as ufm_batch_X(batch, map, ...) is driven
through a Planner and through map 0 of a BatchPlanner(1, ...) by the same script, and the two must agree: return codes, statistics
(all but the measured times), rasters, fields (bit for bit for FD and SG; MS-DFM's float fixed point is not unique, so within
tolerances.DFM_RTOL), paths and their infos (all but the measured time), the self-checks, the error codes.  The map is 70 wide by 54
long -- non-square, no multiple of the tile, 5 x 4 tiles --, "focused" is 0, so every element is final and comparable.

Four statistics are not a function of the script on either form: tile_visits, tile_iters, elem_evals and resident_tile_visits count
what the asynchronous waves of a launch happened to do (include/ufm.h, note 3).  Measured with this file's core script, 8 runs per form
and planner family (profiles/surface_refactor.txt): a plan of FD visits 47 .. 54 tiles through a Planner and 44 .. 53 through a batch of
one, with 72 048 .. 81 312 and 70 848 .. 82 720 element evaluations; every other field had one value over all 16 runs.  So those four
are held to what both forms do -- work was counted on one exactly when it was on the other -- and every other field to equality."""
import numpy as np
import pytest

import ufm_amd
from helpers import DeviceBytes

pytestmark = pytest.mark.gpu

W, LEN = 70, 54
INVALID = -22
PLANNERS = {"FD": (ufm_amd.ALGO_FD, 1), "SG": (ufm_amd.ALGO_SG, 2), "DFM": (ufm_amd.ALGO_DFM, 1)}
PER_MAP = {"set_map", "set_map_device", "patch_map", "patch_map_device", "set_start", "set_goal", "reset", "read_map", "read_raw_map",
           "read_cost_census", "set_survey", "read_survey", "set_image", "patch_layer", "set_layer", "set_layer_survey", "read_layer",
           "read_layer_survey", "read_changes"}


class MapZero:
    """map 0 of a batch, with a planner's signatures"""

    def __init__(self, b):
        self.b = b

    def __getattr__(self, name):
        f = getattr(self.b, name)
        return (lambda *a, **k: f(0, *a, **k)) if name in PER_MAP else f

    def read_field(self):
        return self.b.read_field(0)

    def reveal(self, row, col, count=False):
        n = self.b.reveal([[row, col]], count=count)
        return int(n[0]) if count else None

    def extract_path(self, **kw):
        out = self.b.extract_paths(**kw)
        return out[0], self.b.path_info[0]

    def extract_paths_from(self, starts, **kw):
        return self.b.extract_paths_from(np.zeros(len(starts), np.int32), starts, **kw), self.b.path_infos


class One:
    """a planner, with the same few return shapes"""

    def __init__(self, p):
        self.p = p

    def __getattr__(self, name):
        return getattr(self.p, name)

    def read_field(self):
        return self.p.read_field()[0]

    def extract_path(self, **kw):
        return self.p.extract_path(**kw), self.p.path_info

    def extract_paths_from(self, starts, **kw):
        return self.p.extract_paths_from(starts, **kw), self.p.path_infos


@pytest.fixture
def twins():
    made = []

    def make(name="FD", heuristic=False):
        algo, lvl = PLANNERS[name]
        pair = (One(ufm_amd.Planner(algo, lvl, heuristic, device=0)), MapZero(ufm_amd.BatchPlanner(1, algo, lvl, heuristic, device=0)))
        made.extend(pair)
        for q in pair:
            q.set_occupancy_threshold(1.0)
            q.set_param("focused", 0)
        return pair
    yield make
    for q in made:
        q.close()


def rasters(seed=5):
    rng = np.random.default_rng(seed)
    cost = ufm_amd.synth.cost_map(seed, W, LEN)
    assert cost.shape == (LEN, W)
    host = rng.integers(1, 255, (9, 7), dtype=np.uint8)
    dev = rng.integers(1, 255, (9, 7), dtype=np.uint8)
    return cost, host, dev, rng


def same(a, b, what):
    """every call through both forms gives the same: arrays bit for bit, tuples item by item"""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (what, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


def both(pair, call, what):
    a, b = call(pair[0]), call(pair[1])
    same(a, b, what)
    return a


SCHEDULED = {"tile_visits", "tile_iters", "elem_evals", "resident_tile_visits"}      # (the module's docstring)


def same_stats(pair, what):
    a, b = pair[0].stats.as_dict(), pair[1].stats.as_dict()
    print(what, {k: (a[k], b[k]) for k in a})
    for k in a:
        if k in SCHEDULED:
            assert (a[k] > 0) == (b[k] > 0), (what, k, a[k], b[k])
        elif not k.endswith("_ms"):     # (the times are measured)
            assert a[k] == b[k], (what, k, a[k], b[k])


def same_infos(a, b, n, what):
    for k in range(n):
        for name, _ in ufm_amd.PathInfo._fields_:
            if name != "e_ms":          # (measured)
                assert getattr(a[k], name) == getattr(b[k], name), (what, k, name)


def same_field(pair, name, what):
    g, h = pair[0].read_field(), pair[1].read_field()
    assert g.shape == h.shape and g.dtype == h.dtype == np.float32, what
    assert np.isfinite(g).any(), what
    if name != "DFM":
        assert np.array_equal(g.view(np.uint32), h.view(np.uint32)), what
        return
    assert np.array_equal(np.isfinite(g), np.isfinite(h)), what
    m = np.isfinite(g)
    err = np.abs(g[m].astype(np.float64) - h[m]) / np.maximum(h[m].astype(np.float64), 1e-30)
    print(what, "MS-DFM worst relative difference", err.max() if err.size else 0.0)
    assert (err <= ufm_amd.tolerances.DFM_RTOL).all(), (what, err.max())


def plan(pair, cost, what="plan"):
    start, goal = ufm_amd.synth.start_goal(W, LEN)
    both(pair, lambda q: q.set_map(cost), "set_map")
    both(pair, lambda q: q.set_start(*start), "set_start")
    both(pair, lambda q: q.set_goal(*goal), "set_goal")
    assert both(pair, lambda q: q.step(), what) == 0
    return start, goal


@pytest.mark.parametrize("name", list(PLANNERS))
def test_core_script(twins, name):
    pair = twins(name)
    cost, host, dev, rng = rasters()
    dbuf = DeviceBytes(dev)
    try:
        def check(what):
            same_stats(pair, what)
            both(pair, lambda q: q.read_map(W, LEN), what + " read_map")
            same_field(pair, name, what + " field")
            both(pair, lambda q: q.check_layout(), what + " check_layout")
            both(pair, lambda q: q.check_info(), what + " check_info")
            if name == "DFM":
                return
            kw = dict(max_steps=40, allow_indirect=name != "SG")
            (pa, ia), (pb, ib) = pair[0].extract_path(**kw), pair[1].extract_path(**kw)
            same(pa, pb, what + " extract_path")
            same_infos([ia], [ib], 1, what + " path_info")
            assert ia.n_points > 1, what
            starts = np.array([[8.0, 8.0], [20.5, 31.25], [3.0, 60.0], [45.75, 12.5], [30.0, 66.0]], np.float32)
            (pa, ia), (pb, ib) = pair[0].extract_paths_from(starts, **kw), pair[1].extract_paths_from(starts, **kw)
            same(pa, pb, what + " extract_paths_from")
            same_infos(ia, ib, len(starts), what + " path_infos")

        plan(pair, cost)
        check("plan")
        both(pair, lambda q: q.patch_map(host, 20, 30), "patch_map")
        both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")          # (a step takes the patches in when the start is new)
        assert both(pair, lambda q: q.step(), "step after the host patch") == 0
        assert pair[0].stats.updated > 0
        check("host patch")
        both(pair, lambda q: q.patch_map_device(dbuf.data_ptr(), 31, 11, 7, 9), "patch_map_device")
        both(pair, lambda q: q.set_start(11.0, 12.75), "set_start")
        assert both(pair, lambda q: q.step(), "step after the device patch") == 0
        assert pair[0].stats.updated > 0
        check("device patch")
        want = cost.copy()
        want[20:29, 30:37] = host
        want[31:40, 11:18] = dev
        assert np.array_equal(pair[0].read_map(W, LEN), want)
        both(pair, lambda q: q.reset(), "reset")
        assert both(pair, lambda q: q.step(), "step after reset") == 0
        check("reset")
    finally:
        dbuf.free()


def test_footprint(twins):
    pair = twins()
    cost, host, dev, rng = rasters(6)
    both(pair, lambda q: q.set_cspace(ufm_amd.cspace_disc(5)), "set_cspace")
    plan(pair, cost)
    both(pair, lambda q: q.patch_map(host, 20, 30), "patch_map")
    both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")
    assert both(pair, lambda q: q.step(), "step") == 0
    raw = both(pair, lambda q: q.read_raw_map(W, LEN), "read_raw_map")
    dil = both(pair, lambda q: q.read_map(W, LEN), "read_map")
    assert np.array_equal(raw[20:29, 30:37], host) and (dil >= raw).all() and (dil != raw).any()
    same_field(pair, "FD", "footprint field")


def test_census_and_auto_multiplier(twins):
    pair = twins(heuristic=True)
    cost, host, dev, rng = rasters(7)
    both(pair, lambda q: q.track_costs(), "track_costs")
    both(pair, lambda q: q.set_param("auto_multiplier", 1), "auto_multiplier")
    plan(pair, cost)
    both(pair, lambda q: q.patch_map(host, 20, 30), "patch_map")
    both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")
    assert both(pair, lambda q: q.step(), "step") == 0
    hist, mn, mx = both(pair, lambda q: q.read_cost_census(), "read_cost_census")
    now = cost.copy()
    now[20:29, 30:37] = host
    assert np.array_equal(hist, np.bincount(now.ravel(), minlength=256).astype(np.uint64)) and (mn, mx) == (int(now.min()), int(now.max()))
    assert both(pair, lambda q: q.heuristic_multiplier(), "heuristic_multiplier") == float(mn)
    same_field(pair, "FD", "census field")


def test_sensor_reveal(twins):
    pair = twins()
    cost, host, dev, rng = rasters(8)
    survey = rng.integers(1, 255, (LEN, W), dtype=np.uint8)
    both(pair, lambda q: q.set_sensor(ufm_amd.sensor_disc(5)), "set_sensor")
    plan(pair, cost)
    both(pair, lambda q: q.set_survey(survey), "set_survey")
    n = both(pair, lambda q: q.reveal(25, 33, count=True), "reveal")
    disc = ufm_amd.sensor_disc(5).astype(bool)
    assert n == int((cost[20:31, 28:39] != survey[20:31, 28:39])[disc].sum()) and n > 0
    assert both(pair, lambda q: q.reveal(2, 68, count=True), "reveal at the corner") > 0
    both(pair, lambda q: q.read_survey(W, LEN), "read_survey")
    both(pair, lambda q: q.read_map(W, LEN), "read_map")
    both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")
    assert both(pair, lambda q: q.step(), "step") == 0
    same_field(pair, "FD", "reveal field")


def test_set_image(twins):
    pair = twins()
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (LEN, W), dtype=np.uint8)
    both(pair, lambda q: q.set_image(img, ksize=5, penalty=15), "set_image")
    data_l, data_h = ufm_amd.harness.simulation_data(img, low_res_penalty=15, filter_size=5)
    assert np.array_equal(both(pair, lambda q: q.read_map(W, LEN), "read_map"), data_l)
    assert np.array_equal(both(pair, lambda q: q.read_survey(W, LEN), "read_survey"), data_h)


def test_layers(twins):
    pair = twins()
    cost, host, dev, rng = rasters(10)
    second = rng.integers(1, 255, (LEN, W), dtype=np.uint8)
    seen = rng.integers(1, 255, (LEN, W), dtype=np.uint8)
    dbuf = DeviceBytes(dev)
    try:
        both(pair, lambda q: q.set_layers(2), "set_layers")
        plan(pair, cost)
        both(pair, lambda q: q.set_layer(1, second), "set_layer")
        both(pair, lambda q: q.patch_layer(1, host, 20, 30), "patch_layer")
        both(pair, lambda q: q.patch_layer(0, dbuf, 31, 11, w=7, h=9), "patch_layer from the device")
        both(pair, lambda q: q.set_layer_survey(1, seen), "set_layer_survey")
        l0 = both(pair, lambda q: q.read_layer(0, W, LEN), "read_layer 0")
        l1 = both(pair, lambda q: q.read_layer(1, W, LEN), "read_layer 1")
        assert np.array_equal(both(pair, lambda q: q.read_layer_survey(1, W, LEN), "read_layer_survey"), seen)
        assert np.array_equal(l1[20:29, 30:37], host) and np.array_equal(l0[31:40, 11:18], dev)
        assert np.array_equal(both(pair, lambda q: q.read_map(W, LEN), "read_map"), np.maximum(l0, l1))
        both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")
        assert both(pair, lambda q: q.step(), "step") == 0
        same_field(pair, "FD", "layers field")
    finally:
        dbuf.free()


def test_step_deltas(twins):
    pair = twins()
    cost, host, dev, rng = rasters(11)
    both(pair, lambda q: q.track_changes(), "track_changes")
    plan(pair, cost)

    def delta(q):
        xy, g, info = q.read_changes()
        order = np.lexsort((xy[:, 1], xy[:, 0]))
        return xy[order], g[order]
    xy, g = both(pair, delta, "read_changes after the plan")
    assert len(xy) > 0
    both(pair, lambda q: q.patch_map(host, 20, 30), "patch_map")
    both(pair, lambda q: q.set_start(9.5, 10.25), "set_start")
    assert both(pair, lambda q: q.step(), "step") == 0
    xy, g = both(pair, delta, "read_changes after the patch")
    assert len(xy) > 0


def test_errors_are_the_same_codes(twins):
    pair = twins()
    p, b = pair[0].p, pair[1].b
    L = p.L
    cost, host, dev, rng = rasters(12)
    ptr = host.ctypes.data
    centre = np.array([[5, 5]], np.int32)
    # before a map: no sensor yet; an unknown knob
    assert L.ufm_reveal(p.h, 5, 5, None) == L.ufm_batch_reveal(b.h, centre.ctypes.data, None) == INVALID
    assert L.ufm_set_param(p.h, b"dag", 1.0) == L.ufm_batch_set_param(b.h, b"dag", 1.0) == INVALID
    both(pair, lambda q: q.set_layers(2), "set_layers")
    plan(pair, cost)
    # a patch that leaves the map (rows 50 .. 58 of 54; columns 65 .. 71 of 70)
    assert L.ufm_patch_map(p.h, ptr, 50, 30, 7, 9) == L.ufm_batch_patch_map(b.h, 0, ptr, 50, 30, 7, 9) == INVALID
    assert L.ufm_patch_map(p.h, ptr, 20, 65, 7, 9) == L.ufm_batch_patch_map(b.h, 0, ptr, 20, 65, 7, 9) == INVALID
    # layer 2 of 2
    assert L.ufm_patch_layer(p.h, 2, ptr, 20, 30, 7, 9) == L.ufm_batch_patch_layer(b.h, 0, 2, ptr, 20, 30, 7, 9) == INVALID
    assert L.ufm_patch_layer(p.h, 1, ptr, 20, 30, 7, 9) == L.ufm_batch_patch_layer(b.h, 0, 1, ptr, 20, 30, 7, 9) == 0
    # properties of the handle, after a map
    assert L.ufm_set_layers(p.h, 3) == L.ufm_batch_set_layers(b.h, 3) == INVALID
    mask = ufm_amd.cspace_disc(5)
    assert L.ufm_set_cspace(p.h, mask.ctypes.data, 5, 5, -1, -1) == L.ufm_batch_set_cspace(b.h, mask.ctypes.data, 5, 5, -1, -1) == INVALID
    # a map the batch does not have
    buf = np.zeros((LEN, W), np.uint8)
    for i in (-1, 1):
        assert L.ufm_batch_set_start(b.h, i, 8.0, 8.0) == INVALID
        assert L.ufm_batch_set_goal(b.h, i, 8.0, 8.0) == INVALID
        assert L.ufm_batch_reset(b.h, i) == INVALID
        assert L.ufm_batch_patch_map(b.h, i, ptr, 20, 30, 7, 9) == INVALID
        assert L.ufm_batch_read_map(b.h, i, buf.ctypes.data) == INVALID
        assert L.ufm_batch_read_field(b.h, i, 0, 0, 1, 1, buf.ctypes.data, None) == INVALID
    assert L.ufm_batch_read_map(b.h, 0, buf.ctypes.data) == L.ufm_read_map(p.h, buf.ctypes.data) == 0
    # where the forms differ on purpose: a planner has no map to skip
    both(pair, lambda q: q.set_sensor(ufm_amd.sensor_disc(5)), "set_sensor")
    both(pair, lambda q: q.set_survey(cost), "set_survey")
    skip = np.array([[-1, 5]], np.int32)
    assert L.ufm_reveal(p.h, -1, 5, None) == INVALID and L.ufm_batch_reveal(b.h, skip.ctypes.data, None) == 0
