"""-m gpu: the sensor reveal in the engine (ufm_set_sensor / ufm_set_survey / ufm_reveal).  A reveal is defined by equivalence
(include/ufm.h): with R the mask's bounding rectangle on the centre, clipped to the map, and Q = the survey where the mask covers a cell,
the caller's raster elsewhere, ufm_reveal leaves the handle as ufm_patch_map_device(Q, R) would.  reveal_ref below is that definition
written out in numpy; everything here is held to it: the rasters, the changed count, the census, the planner's fields against a planner
fed (Q, R) from the host and against the CPU oracle fed the same, batches, the planner process, and the reference's recorded mission."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
from helpers import ALGOS, DFM_RTOL, DeviceBytes, check_parity
from test_cspace_surface import dilate_ref
from test_reference_mission import check_mission, g_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
INVALID = -22

ELLIPSE5 = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], np.uint8)   # cv2 MORPH_ELLIPSE (5, 5)
WEDGE = np.array([[1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], np.uint8)      # 3 x 5, anchor (2, 0): a reflected mask would look down and left
BLOCK71 = (np.random.default_rng(71).integers(0, 4, (71, 71)) != 0).astype(np.uint8)  # 71 x 71 > 4096 cells: patch()'s large route
MASKS = {"disc5": (ufm_amd.sensor_disc(5), None), "disc15": (ufm_amd.sensor_disc(15), None), "wedge3x5": (WEDGE, (2, 0)),
         "one": (np.ones((1, 1), np.uint8), None), "block71": (BLOCK71, (10, 60))}
SIZES = [(96, 80), (50, 37)]          # (length, width): tiles are 16 wide -- partial tiles, no multiple of 64


def reveal_ref(cur, survey, mask, anchor, row, col):
    """the definition: (Q, x, y, changed) -- Q dense over R = rows x .. x+h-1, columns y .. y+w-1; `cur` is the caller's raster"""
    mh, mw = mask.shape
    ar, ac = (mh // 2, mw // 2) if anchor is None else anchor
    L, W = cur.shape
    x0, y0 = max(row - ar, 0), max(col - ac, 0)
    x1, y1 = min(row - ar + mh - 1, L - 1), min(col - ac + mw - 1, W - 1)
    Q = cur[x0:x1 + 1, y0:y1 + 1].copy()
    for i in range(x0, x1 + 1):
        for j in range(y0, y1 + 1):
            if mask[i - row + ar, j - col + ac]:          # not reflected: mask cell (a, b) covers (row + a - ar, col + b - ac)
                Q[i - x0, j - y0] = survey[i, j]
    changed = int((Q != cur[x0:x1 + 1, y0:y1 + 1]).sum())
    return np.ascontiguousarray(Q), x0, y0, changed


def apply_ref(cur, survey, mask, anchor, row, col):
    Q, x, y, changed = reveal_ref(cur, survey, mask, anchor, row, col)
    cur[x:x + Q.shape[0], y:y + Q.shape[1]] = Q
    return Q, x, y, changed


def rasters(L, W, seed=21):
    return ufm_amd.synth.cost_map(seed, W, L), ufm_amd.synth.cost_map(seed + 100, W, L, obstacles=False)


def centre_groups(L, W):
    """groups of centres, a step after each: the four corners, the four borders, the interior (the second one leaves the 71 x 71 block
    whole on the larger map), two overlapping reveals between two steps, and one centre twice"""
    return [[(0, 0)], [(0, W - 1)], [(L - 1, 0)], [(L - 1, W - 1)],
            [(0, W // 2)], [(L - 1, W // 3)], [(L // 2, 0)], [(L // 3, W - 1)],
            [(L // 2, W // 2)], [(L // 8, (5 * W) // 6)], [(L // 2 + 3, W // 2 - 4), (L // 2 + 5, W // 2 - 1)], [(L // 4, W // 4), (L // 4, W // 4)]]


# ---- 1. the raster invariant ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "cspace", "census", "cspace+census"])
@pytest.mark.parametrize("L,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_raster_invariant(L, W, mode):
    """after EVERY reveal, for every mask (each replacing the one before, each with a fresh survey): the caller's raster equals the
    reference and `changed` the count; with the 5 x 5 ellipse footprint the raw store equals the reference and read_map == dilate(raw);
    with the census hist == bincount(read_map); after every step check_layout() == (0, 0)"""
    cspace, census = "cspace" in mode, "census" in mode
    raw0, _ = rasters(L, W)
    start, goal = ufm_amd.synth.start_goal(W, L)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0)
    if cspace:
        g.set_cspace(ELLIPSE5)
    if census:
        g.track_costs()
    g.set_map(raw0); g.set_start(*start); g.set_goal(*goal)
    assert g.step() == 0
    cur = raw0.copy()
    n_reveals = n_zero = n_steps = n_large = 0
    groups = centre_groups(L, W)
    for k, (name, (mask, anchor)) in enumerate(MASKS.items()):
        survey = ufm_amd.synth.cost_map(300 + 7 * k + L, W, L, obstacles=False)
        g.set_sensor(mask, anchor)
        g.set_survey(survey)
        assert np.array_equal(g.read_survey(W, L), survey)
        for n, group in enumerate(groups):
            for r, (row, col) in enumerate(group):
                what = "%s %s reveal at (%d, %d)" % (mode, name, row, col)
                Q, x, y, want = apply_ref(cur, survey, mask, anchor, row, col)
                again = n == len(groups) - 1 and r == 1
                counted = again or (n + r) % 3 != 2             # every third one is only queued
                got = g.reveal(row, col, count=counted)
                if counted:
                    assert got == want, "%s: changed %d, the reference %d" % (what, got, want)
                if again:
                    assert want == 0 and got == 0, what       # the same centre again: a patch that changes nothing
                    n_zero += 1
                n_large += Q.size > 4096
                raster = g.read_raw_map(W, L) if cspace else g.read_map(W, L)
                assert np.array_equal(raster, cur), "%s: the raster differs from the reference in %d cells, first %r" % (
                    what, int((raster != cur).sum()), tuple(np.argwhere(raster != cur)[0]))
                planning = g.read_map(W, L)
                if cspace:
                    want_p = dilate_ref(raster, ELLIPSE5)
                    assert np.array_equal(planning, want_p), "%s: planning raster != dilate(raw) in %d cells" % (what, int((planning != want_p).sum()))
                if census:
                    hist, mn, mx = g.read_cost_census()
                    assert np.array_equal(hist, np.bincount(planning.ravel(), minlength=256).astype(np.uint64)), what
                    assert (mn, mx) == (int(planning.min()), int(planning.max())), what
                n_reveals += 1
            g.set_start(start[0] + 2 * (n % 5), start[1] + (n % 4))
            assert g.step() == 0
            assert g.check_layout() == (0, 0), "%s %s after step %d: %r" % (mode, name, n, g.check_layout())
            n_steps += 1
    assert n_reveals == 5 * 14 and n_zero == 5 and n_steps == 5 * 12
    assert (n_large > 0) == (L == 96), "the 71 x 71 block was meant to take the large-patch route on the larger map"
    g.close()


# ---- 2. equivalence with a planner that is fed (Q, R) from the host, and with the oracle fed the same --------------------------------
PLANNERS = {"FD-1": ("FD", 1), "SG-2": ("SG", 2), "DFM-1": ("DFM", 1)}
EQUIV = [(p, h, f) for p in PLANNERS for h in (False, True) for f in (1, 0)]


def changes_sorted(p):
    xy, gv, info = p.read_changes(want_info=True)
    order = np.lexsort((xy[:, 1], xy[:, 0]))
    return xy[order], gv[order].view(np.uint32), info[order]


@pytest.mark.parametrize("name,heur,focused", EQUIV, ids=["%s-%s-%s" % (p, "heur" if h else "plain", "focused" if f else "converged") for p, h, f in EQUIV])
def test_reveal_equals_host_patch(name, heur, focused):
    """Planner A gets reveals, planner B ufm_patch_map of (Q, R) computed on the host, the oracle the same patches: 8 moves with a moving
    start on 96 x 80, disc5.  After every step A and B agree on stats.updated and read_map, A equals the oracle under
    helpers.check_parity's rule (FD / SG bit for bit), and
      "converged" ("focused" = 0: every element final): the WHOLE field bit for bit (MS-DFM: within DFM_RTOL) and the step deltas;
      "focused" (the default): the field bit for bit below the start's key.
    The whole field is compared under "focused" = 0 only, as tests/test_gpu_census.py does and for the reason measured there: beyond the
    start's key a focused search leaves whatever its asynchronous waves had reached, two IDENTICAL host-fed planners already differ there,
    and B's small host patches travel another route than A's (held for the block kernel) -- which is what this comparison is about.
    Measured here (printed per step): with "focused" = 1 A and B differ in 23 .. 51 of 7 857 elements (MS-DFM: 24 .. 57 of 7 680) after the
    first PLAN already, before any reveal or patch, both having been fed the same bytes; with "focused" = 0 in none, at any step.
    stats.region_replans grows for A: a reveal still reaches the block kernel."""
    algo, lvl = PLANNERS[name]
    L, W = 96, 80
    raw0, survey = rasters(L, W, 33)
    mask, anchor = MASKS["disc5"]
    start, goal = ufm_amd.synth.start_goal(W, L)
    a, b = ufm_amd.Planner(ALGOS[algo], lvl, heur), ufm_amd.Planner(ALGOS[algo], lvl, heur)
    o = orc.OraclePlanner(ALGOS[algo], lvl, heur)
    for p in (a, b, o):
        p.reset(); p.set_occupancy_threshold(1.0); p.set_heuristic_multiplier(1.0)
    for p in (a, b):
        p.set_param("focused", focused)
        if not focused:
            p.track_changes(True)
    for p in (a, b, o):
        p.set_map(raw0); p.set_start(*start); p.set_goal(*goal)
    a.set_sensor(mask, anchor); a.set_survey(survey)
    cur = raw0.copy()

    def compare(what):
        assert np.array_equal(a.read_map(W, L), cur) and np.array_equal(b.read_map(W, L), cur), what
        assert a.stats.updated == b.stats.updated, (what, a.stats.updated, b.stats.updated)
        fa, fb = a.read_field()[0], b.read_field()[0]
        whole = int((fa.view(np.uint32) != fb.view(np.uint32)).sum())
        print("%s: the two fields differ in %d of %d elements" % (what, whole, fa.size))
        if focused:
            below = o.trusted_mask(below_start_key=True)
            assert int(below.sum()) > 100, what
            if algo == "DFM":
                assert np.all(np.abs(fa[below].astype(np.float64) - fb[below]) <= DFM_RTOL * fb[below]), what
            else:
                assert np.array_equal(fa[below].view(np.uint32), fb[below].view(np.uint32)), "%s: the fields differ below the start's key in %d elements" % (
                    what, int((fa[below].view(np.uint32) != fb[below].view(np.uint32)).sum()))
        elif algo == "DFM":
            fin = np.isfinite(fb)
            assert np.array_equal(np.isfinite(fa), fin) and np.all(np.abs(fa[fin].astype(np.float64) - fb[fin]) <= DFM_RTOL * fb[fin]), what
        else:
            assert whole == 0, "%s: the fields differ in %d elements" % (what, whole)
            ca, cb = changes_sorted(a), changes_sorted(b)
            assert all(np.array_equal(x, y) for x, y in zip(ca, cb)), "%s: the step deltas differ (%d, %d records)" % (what, len(ca[0]), len(cb[0]))
        n, nbad = check_parity(o, a, what, below_start_key=True)
        assert algo == "DFM" or nbad == 0, what

    assert a.step() == 0 and b.step() == 0 and o.step() == 0
    compare("%s plan" % name)
    regions0 = a.stats.region_replans
    n_changed = 0
    for k in range(1, 9):
        s = (start[0] + 5.0 * k + 0.25, start[1] + 4.0 * k - 0.5)
        row, col = int(round(s[0])), int(round(s[1]))
        Q, x, y, want = apply_ref(cur, survey, mask, anchor, row, col)
        assert a.reveal(row, col, count=True) == want
        n_changed += want
        b.patch_map(Q, x, y)
        o.patch_map(Q, x, y)
        for p in (a, b, o):
            p.set_start(*s)
        assert a.step() == 0 and b.step() == 0 and o.step() == 0
        assert a.stats.updated == o.num_updated, (k, a.stats.updated, o.num_updated)
        compare("%s move %d" % (name, k))
    assert n_changed > 300
    assert a.stats.region_replans > regions0, "reveals no longer reach the block kernel"
    a.close(); b.close()


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defer", [0, 1], ids=["at_the_call", "deferred"])
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_engine", "sharded"])
def test_batch(devices, defer):
    """3 maps, one ufm_batch_reveal per round: three different centres; one map skipped (row < 0: untouched, changed 0); and a second
    reveal of one map before the step -- with "defer_patches" the first one's patch is then still held and points into the slot the second
    launch writes: it must have been applied first.  Every map's raster equals the reference, `changed` holds per map, and after the step
    every map equals its own oracle below the start's key, bit for bit."""
    n = 3
    L, W = SIZES[defer]
    mask, anchor = MASKS["disc5"]
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, False, devices=devices)
    b.set_occupancy_threshold(1.0)
    b.set_param("defer_patches", defer)
    b.set_sensor(mask, anchor)
    start, goal = ufm_amd.synth.start_goal(W, L)
    curs, surveys, oracles = [], [], []
    for m in range(n):
        raw0, survey = rasters(L, W, 40 + m)
        b.set_map(m, raw0); b.set_start(m, *start); b.set_goal(m, *goal)
        b.set_survey(m, survey)
        o = orc.OraclePlanner(ufm_amd.ALGO_FD, 1, False)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_heuristic_multiplier(1.0)
        o.set_map(raw0); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        curs.append(raw0.copy()); surveys.append(survey); oracles.append(o)
    assert b.step() == 0

    def against(what):
        for m, o in enumerate(oracles):
            got = b.read_map(m, W, L)
            assert np.array_equal(got, curs[m]), "%s: raster of map %d differs from the reference in %d cells" % (what, m, int((got != curs[m]).sum()))
            below = o.trusted_mask(below_start_key=True)
            assert int(below.sum()) > 100
            assert np.array_equal(b.read_field(m)[below], o.g()[below]), "%s: map %d differs from its oracle" % (what, m)
        assert b.check_layout() == (0, 0)
        assert b.check_info()[1:4] == (0, 0, 0), b.check_info()

    def one_round(k, centres_list, count):
        """the reveals of one round (each a whole-batch call), then a step; the oracle of a map gets ONE patch per step -- the bounding
        rectangle of what its reveals touched, cut from the raster they leave (its update() seeds from the last patch_map alone)"""
        s = (start[0] + 4.0 * k, start[1] + 3.0 * k)
        boxes = {}
        for centres in centres_list:
            want = np.zeros(n, np.uint64)
            for m, (row, col) in enumerate(centres):
                if row < 0:
                    continue
                Q, x, y, want[m] = apply_ref(curs[m], surveys[m], mask, anchor, row, col)
                x0, y0, x1, y1 = boxes.get(m, (x, y, x + Q.shape[0], y + Q.shape[1]))
                boxes[m] = (min(x0, x), min(y0, y), max(x1, x + Q.shape[0]), max(y1, y + Q.shape[1]))
            got = b.reveal(centres, count=count)
            if count:
                assert np.array_equal(got, want), ("round %d" % k, got, want)
        for m, o in enumerate(oracles):
            if m in boxes:
                x0, y0, x1, y1 = boxes[m]
                o.patch_map(np.ascontiguousarray(curs[m][x0:x1, y0:y1]), x0, y0)
            o.set_start(*s); b.set_start(m, *s)
            assert o.step() == 0
        assert b.step() == 0
        against("round %d" % k)

    one_round(1, [[(14, 12), (0, W - 1), (L - 1, 5)]], True)
    before = b.read_map(1, W, L)
    one_round(2, [[(18, 15), (-1, 0), (20, 9)]], True)
    assert np.array_equal(b.read_map(1, W, L), before), "the skipped map was touched"
    one_round(3, [[(22, 18), (24, 20), (25, 12)], [(24, 20), (-1, -1), (-1, 7)]], False)      # map 0 twice before the step, overlapping
    one_round(4, [[(26, 21), (27, 22), (28, 15)], [(-1, 0), (29, 24), (-1, 0)]], True)
    b.close()


# ---- 4. rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_usable():
    L, W = 50, 37
    raw0, survey = rasters(L, W)
    mask, anchor = MASKS["wedge3x5"]
    n = ufm_amd.capi.C.c_uint64(0)
    cnt = ufm_amd.capi.C.addressof(n)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    lib, h = g.L, g.h
    buf = np.zeros((L, W), np.uint8)
    assert lib.ufm_reveal(h, 3, 3, cnt) == INVALID                                             # nothing set at all
    assert lib.ufm_set_survey(h, survey.ctypes.data, W, L) == INVALID                           # a survey with no map
    assert lib.ufm_read_survey(h, buf.ctypes.data) == INVALID
    g.set_sensor(mask, anchor)                                                                  # (needs no map)
    assert lib.ufm_reveal(h, 3, 3, cnt) == INVALID                                             # a sensor, no map, no survey
    g.reset(); g.set_occupancy_threshold(1.0); g.set_map(raw0); g.set_start(8, 8); g.set_goal(L - 8, W - 8)
    assert lib.ufm_reveal(h, 3, 3, cnt) == INVALID                                             # a sensor and a map, no survey
    assert lib.ufm_read_survey(h, buf.ctypes.data) == INVALID
    assert lib.ufm_set_survey(h, survey.ctypes.data, L, W) == INVALID                           # transposed dimensions
    assert lib.ufm_set_survey(h, survey.ctypes.data, W, L - 1) == INVALID
    assert lib.ufm_set_survey(h, None, W, L) == INVALID
    g.set_survey(survey)
    for bad in ((None, 5, 3, 2, 0), (mask.ctypes.data, 0, 3, 0, 0), (mask.ctypes.data, 5, 0, 0, 0), (mask.ctypes.data, 128, 1, 0, 0),
                (mask.ctypes.data, 1, 128, 0, 0), (mask.ctypes.data, 5, 3, 3, 0), (mask.ctypes.data, 5, 3, 0, 5), (mask.ctypes.data, 5, 3, -1, 0),
                (np.zeros((3, 5), np.uint8).ctypes.data, 5, 3, 2, 0)):
        assert lib.ufm_set_sensor(h, *bad) == INVALID, bad
    for row, col in ((-1, 3), (3, -1), (L, 3), (3, W), (L + 100, W + 100)):
        assert lib.ufm_reveal(h, row, col, cnt) == INVALID, (row, col)
        assert lib.ufm_reveal(h, row, col, None) == INVALID, (row, col)
    assert np.array_equal(g.read_map(W, L), raw0)                                               # nothing was written
    # the handle works: the mask set before the rejected ones is still the mask
    cur = raw0.copy()
    Q, x, y, want = apply_ref(cur, survey, mask, anchor, 20, 10)
    assert g.reveal(20, 10, count=True) == want and want > 0
    assert np.array_equal(g.read_map(W, L), cur)
    assert g.step() == 0 and g.check_layout() == (0, 0)
    g.close()
    # no sensor, but a survey and a map
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.set_map(raw0); g.set_survey(survey)
    assert g.L.ufm_reveal(g.h, 3, 3, cnt) == INVALID
    g.close()
    # batch: an index outside the batch, a centre outside the map in ONE of the maps rejects the whole call
    b = ufm_amd.BatchPlanner(2, ufm_amd.ALGO_FD, 1, False)
    b.set_sensor(mask, anchor)
    for m in range(2):
        b.set_map(m, raw0); b.set_start(m, 8, 8); b.set_goal(m, L - 8, W - 8)
    b.set_survey(0, survey)
    for i in (-1, 2, 7):
        assert b.L.ufm_batch_set_survey(b.h, i, survey.ctypes.data, W, L) == INVALID
        assert b.L.ufm_batch_read_survey(b.h, i, buf.ctypes.data) == INVALID
    assert b.L.ufm_batch_read_survey(b.h, 1, buf.ctypes.data) == INVALID                        # this map has none
    centres = np.array([[5, 5], [6, 6]], np.int32)
    assert b.L.ufm_batch_reveal(b.h, centres.ctypes.data, None) == INVALID                      # map 1 has no survey
    assert b.L.ufm_batch_reveal(b.h, None, None) == INVALID
    b.set_survey(1, survey)
    centres = np.array([[5, 5], [L, 6]], np.int32)
    assert b.L.ufm_batch_reveal(b.h, centres.ctypes.data, None) == INVALID
    assert b.L.ufm_batch_set_sensor(b.h, None, 5, 3, 2, 0) == INVALID
    assert np.array_equal(b.read_map(0, W, L), raw0) and np.array_equal(b.read_map(1, W, L), raw0)
    got = b.reveal([[5, 5], [-1, 0]], count=True)
    cur = raw0.copy()
    Q, x, y, want = apply_ref(cur, survey, mask, anchor, 5, 5)
    assert got[0] == want and got[1] == 0 and np.array_equal(b.read_map(0, W, L), cur) and np.array_equal(b.read_map(1, W, L), raw0)
    assert b.step() == 0
    b.close()


# ---- 5. the survey's lifetime -----------------------------------------------------------------------------------------------------------
def test_survey_lifetime_and_device_form():
    L, W = 50, 37
    raw0, survey = rasters(L, W)
    mask, anchor = MASKS["disc5"]
    n = ufm_amd.capi.C.c_uint64(0)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_map(raw0); g.set_start(8, 8); g.set_goal(L - 8, W - 8)
    g.set_sensor(mask, anchor); g.set_survey(survey)
    assert g.step() == 0
    other = ufm_amd.synth.cost_map(77, W, L)
    g.set_map(other)                                          # the same dimensions: the survey stays
    assert np.array_equal(g.read_survey(W, L), survey)
    cur = other.copy()
    Q, x, y, want = apply_ref(cur, survey, mask, anchor, 25, 18)
    assert g.reveal(25, 18, count=True) == want and np.array_equal(g.read_map(W, L), cur)
    g.reset()                                                 # ufm_reset leaves it alone
    assert g.step() == 0
    assert np.array_equal(g.read_survey(W, L), survey)
    Q, x, y, want = apply_ref(cur, survey, mask, anchor, 30, 20)
    assert g.reveal(30, 20, count=True) == want and np.array_equal(g.read_map(W, L), cur)
    small = ufm_amd.synth.cost_map(78, W - 1, L)
    g.set_map(small)                                          # other dimensions: dropped
    buf = np.zeros((L, W), np.uint8)
    assert g.L.ufm_read_survey(g.h, buf.ctypes.data) == INVALID
    assert g.L.ufm_reveal(g.h, 10, 10, ufm_amd.capi.C.addressof(n)) == INVALID
    assert g.L.ufm_set_survey(g.h, survey.ctypes.data, W, L) == INVALID            # the old survey no longer fits
    assert np.array_equal(g.read_map(W - 1, L), small)
    g.set_goal(L - 8, W - 9)
    assert g.step() == 0
    # the device form against the host form
    dev = DeviceBytes(survey)
    a, b = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False), ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    for p in (a, b):
        p.reset(); p.set_occupancy_threshold(1.0); p.set_map(raw0); p.set_start(8, 8); p.set_goal(L - 8, W - 8); p.set_sensor(mask, anchor)
    a.set_survey(survey)
    b.set_survey(dev, width=W, length=L)
    dev.overwrite(np.zeros_like(survey))                     # copied at the call
    assert np.array_equal(a.read_survey(W, L), survey) and np.array_equal(b.read_survey(W, L), survey)
    cur = raw0.copy()
    Q, x, y, want = apply_ref(cur, survey, mask, anchor, 12, 30)
    assert a.reveal(12, 30, count=True) == b.reveal(12, 30, count=True) == want
    assert np.array_equal(a.read_map(W, L), cur) and np.array_equal(b.read_map(W, L), cur)
    for p in (g, a, b):
        p.close()
    dev.free()


# ---- 6. the planner process ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options,kw", [([], {}), (["--inflate", "5", "--auto-heuristic"], {"cspace_diameter": 5, "planner_inflates": True, "planner_min_cost": True})],
                         ids=["sense", "inflate+auto+sense"])
def test_planner_process_senses(tmp_path, ref_bitmaps, options, kw):
    """ufm_planner --planner FD --level 1 [--inflate 5 --auto-heuristic] --sense 5 under run_mission(planner_senses=True) on the noise-trap
    bitmap cropped to 64 x 64 (as test_gpu_cspace.test_planner_process_inflates crops it): reaches the goal, and its trace and every path
    equal, bit for bit, those of the same process without --sense fed host patches.  In the second form the host touches no raster after
    the start."""
    cost, _ = ref_bitmaps["noise-trap"]
    img = np.ascontiguousarray((~cost).astype(np.uint8)[28:92, 28:92])
    (sx, sy), (gx, gy) = (56.0, 56.0), (14.0, 14.0)
    exe = os.path.join(PKG, "ufm_planner")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", PKG, "apps"])

    def run(tag, extra, **more):
        replies = []
        trace, finished = ufm_amd.harness.run_mission(
            [exe, "--planner", "FD", "--level", "1"] + options + extra, str(tmp_path / ("in_" + tag)), str(tmp_path / ("out_" + tag)),
            img, (sx, sy), (gx, gy), radius=5, use_heuristic=True, max_moves=100,
            on_move=lambda i, pos, top, left, patch, mc, reply: replies.append((pos, top, left, patch.copy(), mc, reply[:4])), **kw, **more)
        assert finished, "%s: the planner did not report the goal after %d moves, last position %r" % (tag, len(trace), trace[-1])
        return trace, replies

    fed_trace, fed = run("fed", [])
    own_trace, own = run("own", ["--sense", "5"], planner_senses=True)
    assert own_trace[0] == (sx, sy) and len(own_trace) > 5
    assert own_trace == fed_trace
    assert len(own) == len(fed)
    for k, (x, y) in enumerate(zip(own, fed)):
        assert x[0] == y[0] and x[1:3] == y[1:3] and np.array_equal(x[3], y[3]) and x[4] == y[4], "move %d: the simulator's side differs" % k
        (pa, ca, da, ta), (pb, cb, db, tb) = x[5], y[5]
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), "move %d: the paths differ" % k
        assert (da, ta) == (db, tb), "move %d: path length / cost differ" % k


# ---- 7. the reference's recorded mission --------------------------------------------------------------------------------------------------
class SensesForItself:
    """the planner surface test_reference_mission.replay drives, sensing for itself: the survey is the simulator's data_h, the radius the
    recorded mission's (15); the patches replay() cuts on the host are dropped, the position it sets is where the field of view opens"""

    def __init__(self, g, survey, radius):
        self.g, self.survey, self.radius, self.reveals, self.due = g, survey, radius, 0, False

    def set_map(self, m):
        self.g.set_map(m)
        self.g.set_sensor(ufm_amd.sensor_disc(self.radius))
        self.g.set_survey(self.survey)

    def patch_map(self, patch, top, left):
        self.due = True                                          # (a move: the next position set is where the robot stands)

    def set_start(self, x, y):
        if self.due:
            self.g.reveal(int(round(x)), int(round(y)))          # run_simulator.py:170
            self.reveals += 1
            self.due = False
        self.g.set_start(x, y)

    def __getattr__(self, name):
        return getattr(self.g, name)


def test_reference_mission_sensing_for_itself():
    """the noise-trap log (tests/test_reference_mission.py) replayed closed-loop by an engine that is handed positions only: every printed
    position, path cost and path length, and "nodes updated" in as many steps, as for the host-fed engine replay"""
    from test_reference_mission import load
    from ufm_amd_pkg import harness
    pixels, _, _, _ = load("noise-trap")
    _, data_h = harness.simulation_data(pixels, low_res_penalty=15, filter_size=13)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 0, True)
    w = SensesForItself(g, data_h, 15)
    n, upd_same, _, _ = check_mission("noise-trap", w, g_counts, False)
    assert (n, upd_same) == (134, 124)
    assert w.reveals == 134
    g.close()
