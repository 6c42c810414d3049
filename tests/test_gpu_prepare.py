"""-m gpu: map preparation in the engine (ufm_set_image).  The call is defined by equivalence (include/ufm.h): with
(L, H) = harness.simulation_data(image, penalty, ntaps) -- pure integer arithmetic, so there is no tolerance anywhere below -- it leaves
the handle as ufm_set_map(L) followed by ufm_set_survey(H) would.  Held to that: the rasters bit for bit in every mode, the planner's
fields against a planner handed L and H, batches, every rejection, the lifetime of the survey, the planner process fed a bitmap, and
the reference's recorded mission from the bitmap alone."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
from helpers import ALGOS, DFM_RTOL, DeviceBytes, check_parity
from test_cspace_surface import dilate_ref
from test_gpu_sensor import SensesForItself, apply_ref, changes_sorted
from test_reference_mission import check_mission, g_counts, load
from ufm_amd_pkg import capi, harness

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
INVALID = -22
DISC5 = ufm_amd.cspace_disc(5)
SIZES = [(7, 7), (13, 100), (100, 100), (65, 130), (63, 257)]       # (length, width): one tile and several, W a multiple of 4 and not
TAPS = [1, 3, 13, 31]
PENALTIES = [0, 15, 255]
_REF = {}


def bitmap(L, W, kind, seed=5):
    if kind == "random":
        return np.random.default_rng(seed + 1000 * L + W).integers(0, 256, (L, W)).astype(np.uint8)
    return np.full((L, W), 0 if kind == "zeros" else 255, np.uint8)


def reference(L, W, kind, ntaps, penalty):
    """(image, L, H) of the definition, computed once per case and left unchanged"""
    key = (L, W, kind, ntaps, penalty)
    if key not in _REF:
        img = bitmap(L, W, kind)
        lo, hi = harness.simulation_data(img, penalty, ntaps)
        for a in (img, lo, hi):
            a.setflags(write=False)
        _REF[key] = (img, lo, hi)
    return _REF[key]


class Offset:
    """a device pointer `by` bytes into a DeviceBytes buffer"""

    def __init__(self, dev, by):
        self.ptr = dev.data_ptr() + by


def scene(L, W, seed):
    """a bitmap with structure (the complement of a synthetic cost map), and what the definition makes of it with 13 taps and penalty 15"""
    img = np.ascontiguousarray(255 - ufm_amd.synth.cost_map(seed, W, L)).astype(np.uint8)
    lo, hi = harness.simulation_data(img, 15, 13)
    return img, lo, hi


# ---- 1. the rasters, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "cspace", "census", "cspace+census"])
@pytest.mark.parametrize("L,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_rasters(L, W, mode):
    """every tap count that fits, every penalty on the random image and one each on the all-0 and all-255 images, each call replacing the
    map before it: read_survey == H, the caller's raster == L, read_map == L or dilate(L), the census == bincount, the cost windows sound;
    then the same from a device buffer, aligned and one byte off; after a step check_layout() == (0, 0)"""
    cspace, census = "cspace" in mode, "census" in mode
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0)
    if cspace:
        g.set_cspace(DISC5)
    if census:
        g.track_costs()
    n = 0

    def check(what, lo, hi):
        assert np.array_equal(g.read_survey(W, L), hi), "%s: the survey differs from H in %d cells" % (what, int((g.read_survey(W, L) != hi).sum()))
        if cspace:
            raw = g.read_raw_map(W, L)
            assert np.array_equal(raw, lo), "%s: the raw store differs from L in %d cells, first %r" % (what, int((raw != lo).sum()), tuple(np.argwhere(raw != lo)[0]))
        planning, want = g.read_map(W, L), dilate_ref(lo, DISC5) if cspace else lo
        assert np.array_equal(planning, want), "%s: the planning raster differs in %d cells, first %r" % (
            what, int((planning != want).sum()), tuple(np.argwhere(planning != want)[0]))
        if census:
            hist, mn, mx = g.read_cost_census()
            assert np.array_equal(hist, np.bincount(want.ravel(), minlength=256).astype(np.uint64)), what
            assert (mn, mx) == (int(want.min()), int(want.max())), what
        assert g.check_layout()[1] == 0, "%s: cost windows %r" % (what, g.check_layout())

    for ntaps in TAPS:
        if ntaps // 2 >= min(L, W):
            continue
        cases = [("random", p) for p in PENALTIES] + [("zeros", PENALTIES[(L + ntaps) % 3]), ("ones", PENALTIES[(W + ntaps) % 3])]
        for kind, penalty in cases:
            img, lo, hi = reference(L, W, kind, ntaps, penalty)
            what = "%s %dx%d %s, %d taps, penalty %d" % (mode, L, W, kind, ntaps, penalty)
            if n % 2:
                g.set_image(img, taps=capi.gaussian_taps(ntaps), penalty=penalty)
            else:
                g.set_image(img, ksize=ntaps, penalty=penalty)
            check(what, lo, hi)
            n += 1
        # the device form: the whole buffer, and one byte into a buffer (no 32-bit load is aligned then)
        img, lo, hi = reference(L, W, "random", ntaps, 15)
        dev = DeviceBytes(np.concatenate([np.zeros(1, np.uint8), img.ravel()]))
        whole = DeviceBytes(img)
        for buf, name in ((whole, "device"), (Offset(dev, 1), "device + 1")):
            g.set_image(reference(L, W, "zeros", ntaps, 0)[0], ksize=ntaps)                     # (something else in between)
            g.set_image(buf, ksize=ntaps, penalty=15, width=W, length=L)
            whole.overwrite(np.zeros_like(img)) if buf is whole else dev.overwrite(np.zeros(img.size + 1, np.uint8))   # read at the call
            check("%s %dx%d %s, %d taps" % (mode, L, W, name, ntaps), lo, hi)
            n += 1
        dev.free(); whole.free()
    assert n == 7 * sum(t // 2 < min(L, W) for t in TAPS)
    g.set_start(1.0, 1.0); g.set_goal(L - 2.0, W - 2.0)
    assert g.step() == 0 and g.check_layout() == (0, 0)
    g.close()


# ---- 2. equivalence with a planner handed L and H ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
def test_set_image_equals_set_map_and_set_survey(algo):
    """Planner A gets set_image(img), planner B set_map(L) + set_survey(H); a plan and three reveal + replan moves on 96 x 80 with a moving
    start.  After every step, FD and SG: stats.updated / expanded, the whole field, the stored Info and the step deltas, bit for bit;
    MS-DFM (not bit-reproducible): both planners against the oracle fed L and the same patches, within DFM_RTOL.
    Both run with "focused" = 0, every element final after every step, for the reason tests/test_gpu_census.py and tests/test_gpu_sensor.py
    measured: beyond the start's key a focused search leaves whatever its asynchronous waves had reached, and two IDENTICAL planners already
    differ there -- which is no property of how the raster arrived."""
    L, W = 96, 80
    img, lo, hi = scene(L, W, 33)
    mask = ufm_amd.sensor_disc(5)
    start, goal = ufm_amd.synth.start_goal(W, L)
    a, b = ufm_amd.Planner(ALGOS[algo], 1, False), ufm_amd.Planner(ALGOS[algo], 1, False)
    o = orc.OraclePlanner(ALGOS[algo], 1, False)
    for p in (a, b, o):
        p.reset(); p.set_occupancy_threshold(1.0); p.set_heuristic_multiplier(1.0)
    for p in (a, b):
        p.set_param("focused", 0)
        p.track_changes(True)
        p.set_sensor(mask)
    a.set_image(img, ksize=13, penalty=15)
    b.set_map(lo); b.set_survey(hi)
    o.set_map(lo)
    for p in (a, b, o):
        p.set_start(*start); p.set_goal(*goal)
    cur = lo.copy()

    def compare(what):
        assert np.array_equal(a.read_map(W, L), cur) and np.array_equal(b.read_map(W, L), cur), what
        assert np.array_equal(a.read_survey(W, L), hi) and np.array_equal(b.read_survey(W, L), hi), what
        print("%s: updated %d / %d, expanded %d / %d" % (what, a.stats.updated, b.stats.updated, a.stats.expanded, b.stats.expanded))
        if algo == "DFM":
            for p in (a, b):
                check_parity(o, p, what, below_start_key=True, rtol=DFM_RTOL)
            return
        assert (a.stats.updated, a.stats.expanded) == (b.stats.updated, b.stats.expanded), what
        fa, fb = a.read_field()[0], b.read_field()[0]
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), "%s: the fields differ in %d elements" % (what, int((fa.view(np.uint32) != fb.view(np.uint32)).sum()))
        assert np.array_equal(a.read_info(), b.read_info()), "%s: the stored Info differs" % what
        ca, cb = changes_sorted(a), changes_sorted(b)
        assert len(ca[0]) > 0 and all(np.array_equal(x, y) for x, y in zip(ca, cb)), "%s: the step deltas differ (%d, %d records)" % (what, len(ca[0]), len(cb[0]))
        assert a.check_layout() == (0, 0) and a.check_info()[1:4] == (0, 0, 0), what

    assert a.step() == 0 and b.step() == 0 and o.step() == 0
    compare("%s plan" % algo)
    n_changed = 0
    for k in range(1, 4):
        s = (start[0] + 5.0 * k + 0.25, start[1] + 4.0 * k - 0.5)
        row, col = int(round(s[0])), int(round(s[1]))
        Q, x, y, want = apply_ref(cur, hi, mask, None, row, col)
        assert a.reveal(row, col, count=True) == b.reveal(row, col, count=True) == want
        n_changed += want
        o.patch_map(Q, x, y)
        for p in (a, b, o):
            p.set_start(*s)
        assert a.step() == 0 and b.step() == 0 and o.step() == 0
        compare("%s move %d" % (algo, k))
    assert n_changed > 100
    a.close(); b.close()


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_engine", "sharded"])
def test_batch(devices):
    """3 maps from 3 different bitmaps (one of them a device buffer): every map's rasters are the definition's, a bitmap of another size
    is rejected and leaves everything as it was, and a step advances all of them -- each equal to its own oracle below the start's key"""
    n, L, W = 3, 65, 130
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, False, devices=devices)
    b.set_occupancy_threshold(1.0)
    start, goal = ufm_amd.synth.start_goal(W, L)
    scenes = [scene(L, W, 50 + m) for m in range(n)]
    dev = DeviceBytes(scenes[1][0])
    for m, (img, lo, hi) in enumerate(scenes):
        if m == 1:
            b.set_image(m, dev, ksize=13, penalty=15, width=W, length=L)
        else:
            b.set_image(m, img, taps=capi.gaussian_taps(13), penalty=15)
        b.set_start(m, *start); b.set_goal(m, *goal)
    dev.overwrite(np.zeros((L, W), np.uint8))

    def rasters(what):
        for m, (img, lo, hi) in enumerate(scenes):
            assert np.array_equal(b.read_map(m, W, L), lo), "%s: map %d differs from L" % (what, m)
            assert np.array_equal(b.read_survey(m, W, L), hi), "%s: survey %d differs from H" % (what, m)

    rasters("after set_image")
    small = scenes[0][0][:, :W - 2]
    taps = capi.gaussian_taps(13)
    assert b.L.ufm_batch_set_image(b.h, 1, np.ascontiguousarray(small).ctypes.data, W - 2, L, taps.ctypes.data, 13, 15) == INVALID
    assert b.L.ufm_batch_set_image(b.h, 0, scenes[0][0].ctypes.data, L, W, taps.ctypes.data, 13, 15) == INVALID          # transposed
    for i in (-1, n, n + 4):
        assert b.L.ufm_batch_set_image(b.h, i, scenes[0][0].ctypes.data, W, L, taps.ctypes.data, 13, 15) == INVALID
        assert b.L.ufm_batch_set_image_device(b.h, i, dev.data_ptr(), W, L, taps.ctypes.data, 13, 15) == INVALID
    rasters("after the rejected calls")
    assert b.step() == 0
    assert b.check_layout() == (0, 0) and b.check_info()[1:4] == (0, 0, 0)
    for m, (img, lo, hi) in enumerate(scenes):
        o = orc.OraclePlanner(ufm_amd.ALGO_FD, 1, False)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_heuristic_multiplier(1.0)
        o.set_map(lo); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        below = o.trusted_mask(below_start_key=True)
        assert int(below.sum()) > 100
        assert np.array_equal(b.read_field(m)[below], o.g()[below]), "map %d differs from its oracle" % m
    # a second bitmap for one map replaces that map alone
    img2, lo2, hi2 = scene(L, W, 77)
    b.set_image(2, img2, ksize=13, penalty=15)
    scenes[2] = (img2, lo2, hi2)
    rasters("after replacing map 2")
    b.reset(2)
    assert b.step() == 0 and b.check_layout() == (0, 0)
    b.close(); dev.free()


# ---- 4. rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_usable():
    """every rejection of the header, each followed by a valid set_image and a step that gives the oracle's field"""
    L, W = 50, 37
    img, lo, hi = scene(L, W, 21)
    start, goal = (8.0, 8.0), (L - 8.0, W - 8.0)
    o = orc.OraclePlanner(ufm_amd.ALGO_FD, 1, False)
    o.reset(); o.set_occupancy_threshold(1.0); o.set_heuristic_multiplier(1.0)
    o.set_map(lo); o.set_start(*start); o.set_goal(*goal)
    assert o.step() == 0
    below, want = o.trusted_mask(below_start_key=True), o.g()
    assert int(below.sum()) > 100
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_heuristic_multiplier(1.0)
    t13 = capi.gaussian_taps(13)
    t3 = capi.gaussian_taps(3)
    p, t = img.ctypes.data, t13.ctypes.data

    def taps(*v):
        return np.array(v, np.uint16)

    over, short, even, t32 = taps(0, 257, 0), taps(64, 127, 64), taps(128, 128), np.concatenate([taps(128, 128), np.zeros(30, np.uint16)])
    wrap = taps(256, 256, 65280)                  # sums to 256 in 16 bits
    t33 = np.concatenate([taps(256), np.zeros(32, np.uint16)])
    bad = [("NULL image", (None, W, L, t, 13, 15)), ("NULL taps", (p, W, L, None, 13, 15)),
           ("width 0", (p, 0, L, t, 13, 15)), ("length 0", (p, W, 0, t, 13, 15)), ("width < 0", (p, -W, L, t, 13, 15)), ("length < 0", (p, W, -1, t, 13, 15)),
           ("ntaps 0", (p, W, L, t, 0, 15)), ("ntaps even", (p, W, L, even.ctypes.data, 2, 15)), ("ntaps 32", (p, W, L, t32.ctypes.data, 32, 15)),
           ("ntaps 33", (p, W, L, t33.ctypes.data, 33, 15)), ("ntaps < 0", (p, W, L, t, -13, 15)),
           ("a tap > 256", (p, W, L, over.ctypes.data, 3, 15)), ("sum 255", (p, W, L, short.ctypes.data, 3, 15)), ("sum wraps", (p, W, L, wrap.ctypes.data, 3, 15)),
           ("13 taps of a 31-tap sum", (p, W, L, capi.gaussian_taps(31).ctypes.data, 13, 15)),
           ("halo as wide as the map", (p, 6, L, t, 13, 15)), ("halo as long as the map", (p, W, 6, t, 13, 15)), ("31 taps on 37 x 15", (p, W, 15, capi.gaussian_taps(31).ctypes.data, 31, 15)),
           ("penalty -1", (p, W, L, t, 13, -1)), ("penalty 256", (p, W, L, t, 13, 256))]
    assert g.L.ufm_set_image(None, p, W, L, t, 13, 15) == INVALID and g.L.ufm_set_image_device(None, p, W, L, t, 13, 15) == INVALID
    first = True
    for what, args in bad:
        assert g.L.ufm_set_image(g.h, *args) == INVALID, what
        if args[0] is not None:
            assert g.L.ufm_set_image_device(g.h, *args) == INVALID, what + " (device form)"      # (rejected before the pointer is looked at)
        if first:
            assert g.L.ufm_read_map(g.h, np.zeros((L, W), np.uint8).ctypes.data) == INVALID, "a rejected call left a map"
            first = False
        else:
            assert np.array_equal(g.read_map(W, L), lo) and np.array_equal(g.read_survey(W, L), hi), "%s: the rejected call wrote something" % what
        g.set_image(img, taps=t3, penalty=0)                                # (another map in between: the next valid call has work to do)
        g.set_image(img, taps=t13, penalty=15)
        g.reset(); g.set_start(*start); g.set_goal(*goal)
        assert g.step() == 0, what
        assert np.array_equal(g.read_field()[0][below], want[below]), "%s: the field after the next valid call differs from the oracle's" % what
    assert g.check_layout() == (0, 0)
    g.close()


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------------------------
def test_lifetime_of_map_and_survey():
    L, W = 50, 37
    img, lo, hi = scene(L, W, 21)
    img2, lo2, hi2 = scene(L, W, 22)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0)
    g.set_image(img, ksize=13, penalty=15)
    g.set_start(8, 8); g.set_goal(L - 8, W - 8)
    assert g.step() == 0
    assert np.array_equal(g.read_map(W, L), lo) and np.array_equal(g.read_survey(W, L), hi)
    g.set_image(img2, ksize=13, penalty=15)                     # the same dimensions: map AND survey replaced
    assert np.array_equal(g.read_map(W, L), lo2) and np.array_equal(g.read_survey(W, L), hi2)
    g.reset()
    assert g.step() == 0
    other = ufm_amd.synth.cost_map(77, W, L)
    g.set_map(other)                                            # a plain set_map of the same size keeps the survey
    assert np.array_equal(g.read_map(W, L), other) and np.array_equal(g.read_survey(W, L), hi2)
    g.reset()                                                   # ufm_reset leaves both
    assert g.step() == 0
    assert np.array_equal(g.read_map(W, L), other) and np.array_equal(g.read_survey(W, L), hi2)
    # the survey set_image left serves a reveal like one that was handed over
    g.set_sensor(ufm_amd.sensor_disc(5))
    cur = other.copy()
    Q, x, y, want = apply_ref(cur, hi2, ufm_amd.sensor_disc(5), None, 25, 18)
    assert g.reveal(25, 18, count=True) == want and np.array_equal(g.read_map(W, L), cur)
    img3, lo3, hi3 = scene(L - 3, W + 7, 23)                    # a different size drops and re-creates both
    g.set_image(img3, ksize=13, penalty=15)
    assert np.array_equal(g.read_map(W + 7, L - 3), lo3) and np.array_equal(g.read_survey(W + 7, L - 3), hi3)
    g.reset(); g.set_goal(L - 11, W - 1)
    assert g.step() == 0 and g.check_layout() == (0, 0)
    small = ufm_amd.synth.cost_map(78, W, L)
    g.set_map(small)                                            # and a set_map of another size drops the survey, as it always did
    assert g.L.ufm_read_survey(g.h, np.zeros((L, W), np.uint8).ctypes.data) == INVALID
    g.set_image(img, ksize=13, penalty=15)
    assert np.array_equal(g.read_map(W, L), lo) and np.array_equal(g.read_survey(W, L), hi)
    g.close()


# ---- 6. the planner process -------------------------------------------------------------------------------------------------------------
def test_planner_process_prepares(tmp_path, ref_bitmaps):
    """ufm_planner --planner FD --level 1 --image 13 15 --inflate 5 --auto-heuristic --sense 5 under
    run_mission(planner_prepares=True, planner_senses=True) on the noise-trap bitmap cropped to 64 x 64 (as
    test_gpu_sensor.test_planner_process_senses crops it): reaches the goal, and its trace and every path equal, bit for bit, those of
    the same process without --image fed the prepared rasters.  The host hands over a bitmap and positions."""
    cost, _ = ref_bitmaps["noise-trap"]
    img = np.ascontiguousarray((~cost).astype(np.uint8)[28:92, 28:92])
    (sx, sy), (gx, gy) = (56.0, 56.0), (14.0, 14.0)
    exe = os.path.join(PKG, "ufm_planner")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
    common = ["--planner", "FD", "--level", "1", "--inflate", "5", "--auto-heuristic", "--sense", "5"]

    def run(tag, extra, **more):
        replies = []
        trace, finished = harness.run_mission(
            [exe] + extra + common, str(tmp_path / ("in_" + tag)), str(tmp_path / ("out_" + tag)),
            img, (sx, sy), (gx, gy), radius=5, use_heuristic=True, max_moves=100, cspace_diameter=5, low_res_penalty=15, filter_size=13,
            planner_inflates=True, planner_min_cost=True, planner_senses=True,
            on_move=lambda i, pos, top, left, patch, mc, reply: replies.append((pos, top, left, patch.copy(), mc, reply[:4])), **more)
        assert finished, "%s: the planner did not report the goal after %d moves, last position %r" % (tag, len(trace), trace[-1])
        return trace, replies

    fed_trace, fed = run("fed", [])
    own_trace, own = run("own", ["--image", "13", "15"], planner_prepares=True)
    assert own_trace[0] == (sx, sy) and len(own_trace) > 5
    assert own_trace == fed_trace
    assert len(own) == len(fed)
    for k, (x, y) in enumerate(zip(own, fed)):
        assert x[0] == y[0] and x[1:3] == y[1:3] and np.array_equal(x[3], y[3]) and x[4] == y[4], "move %d: the simulator's side differs" % k
        (pa, ca, da, ta), (pb, cb, db, tb) = x[5], y[5]
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), "move %d: the paths differ" % k
        assert (da, ta) == (db, tb), "move %d: path length / cost differ" % k


# ---- 7. the reference's recorded mission from the bitmap alone --------------------------------------------------------------------------
class PreparesForItself(SensesForItself):
    """as SensesForItself, and the raster replay() made on the host is ignored too: the engine is handed the mission's bitmap"""

    def __init__(self, g, pixels, radius):
        SensesForItself.__init__(self, g, None, radius)
        self.pixels = pixels

    def set_map(self, m):
        self.g.set_image(self.pixels, ksize=13, penalty=15)              # run_simulator.py:147-148
        self.g.set_sensor(ufm_amd.sensor_disc(self.radius))


def test_reference_mission_from_the_bitmap_alone():
    """the noise-trap log (tests/test_reference_mission.py) replayed closed-loop by an engine that is handed the 100 x 100 bitmap and
    positions, nothing else: every printed position, path cost and path length, and "nodes updated" in as many steps, as in
    test_gpu_sensor.test_reference_mission_sensing_for_itself"""
    pixels, _, _, _ = load("noise-trap")
    assert pixels.shape == (100, 100)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 0, True)
    w = PreparesForItself(g, pixels, 15)
    n, upd_same, _, _ = check_mission("noise-trap", w, g_counts, False)
    assert (n, upd_same) == (134, 124)
    assert w.reveals == 134
    g.close()
