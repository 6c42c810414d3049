"""-m gpu: the cost census (ufm_track_costs) and the automatic heuristic multiplier ("auto_multiplier").  The census must equal a count
over the planning raster -- np.bincount of ufm_read_map's raster and of a numpy model of it -- after set_map by every route and after
every kind of patch, with and without a footprint; the automatic multiplier must make a planner do exactly what a planner does that
is fed float(int(planning.min())) before every step.  All comparisons are exact: integer counts, and bit-for-bit fields of the
deterministic planners (MS-DFM is held to the oracle instead)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
from helpers import ALGOS, DeviceBytes, check_parity
from test_cspace_surface import dilate_ref
from test_gpu_cspace import ELLIPSE5, Inflated
from test_gpu_path import INDIRECT, close_path
from test_reference_mission import check_mission, g_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
INVALID = -22
ONE = np.ones((1, 1), np.uint8)


def count(raster):
    return np.bincount(np.asarray(raster, np.uint8).ravel(), minlength=256).astype(np.uint64)


def census_is(g, raster, what):
    """the planner's census against a raster: every counter, the range, the sum"""
    hist, mn, mx = g.read_cost_census()
    want = count(raster)
    assert int(hist.sum()) == raster.size, "%s: the counts sum to %d, the map has %d cells" % (what, int(hist.sum()), raster.size)
    bad = np.flatnonzero(hist != want)
    assert bad.size == 0, "%s: %d counters differ, first value %d: %d against %d" % (what, bad.size, bad[0] if bad.size else -1,
                                                                                  hist[bad[0]] if bad.size else 0, want[bad[0]] if bad.size else 0)
    assert (mn, mx) == (int(raster.min()), int(raster.max())), (what, mn, mx, int(raster.min()), int(raster.max()))


def device_copy(arr, offset):
    """the array in HBM, its first byte `offset` bytes behind the start of an allocation: (buffer, pointer)"""
    buf = DeviceBytes(np.concatenate([np.zeros(offset, np.uint8), np.ascontiguousarray(arr, np.uint8).ravel()]))
    return buf, buf.data_ptr() + offset


# ---- 1. build -------------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (23, 17), (50, 41), (300, 257)]      # one tile; odd, no multiple of 4; ...; several workgroups of the build plus a tail


def rasters(L, W):
    rng = np.random.default_rng(L * 1000 + W)
    return {"random": rng.integers(0, 256, (L, W)).astype(np.uint8), "all7": np.full((L, W), 7, np.uint8), "all255": np.full((L, W), 255, np.uint8),
            "binary": (rng.integers(0, 2, (L, W)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("L,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_build(L, W):
    """ufm_set_map and ufm_set_map_device (from pointers 1 and 3 bytes off an allocation) of random, constant and binary rasters: the census
    is np.bincount of the array, min and max the array's own; every new raster rebuilds it"""
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    g.track_costs()
    bufs = []
    for kind, r in rasters(L, W).items():
        g.set_map(r)
        census_is(g, r, "%s host" % kind)
        assert np.array_equal(g.read_map(W, L), r)
        for off in (1, 3):
            r2 = np.ascontiguousarray(r[::-1]) if kind in ("random", "binary") else r       # (another raster: the rebuild is seen)
            buf, ptr = device_copy(r2, off)
            bufs.append(buf)
            g.set_map_device(ptr, W, L)
            census_is(g, r2, "%s device + %d" % (kind, off))
            census_is(g, g.read_map(W, L), "%s device + %d against ufm_read_map" % (kind, off))
    g.close()
    for b in bufs:
        b.free()


def test_build_with_a_footprint_counts_the_planning_raster():
    raw = rasters(50, 41)["random"]
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    g.set_cspace(ELLIPSE5)
    g.track_costs()
    g.set_map(raw)
    census_is(g, dilate_ref(raw, ELLIPSE5), "footprint")
    census_is(g, g.read_map(41, 50), "footprint against ufm_read_map")
    g.close()


# ---- 2. patches -----------------------------------------------------------------------------------------------------------------------
def patch_sequence(mask, algo="FD", lvl=1):
    """a scripted sequence of patches on 96 x 80; after each the census is the count of ufm_read_map's raster and of the numpy model's"""
    L, W = 96, 80
    rng = np.random.default_rng(7 + mask.size)
    raw0 = ufm_amd.synth.cost_map(21, W, L)
    start, goal = ufm_amd.synth.start_goal(W, L)
    model = Inflated(raw0, mask, None)
    g = ufm_amd.Planner(ALGOS[algo], lvl, False)
    g.reset(); g.set_occupancy_threshold(1.0)
    if mask.size > 1:
        g.set_cspace(mask)
    g.track_costs()
    g.set_map(raw0); g.set_start(*start); g.set_goal(*goal)
    bufs, n = [], [0]

    def check(what):
        planning = model.planning()
        census_is(g, planning, what + " [model]")
        got = g.read_map(W, L)
        assert np.array_equal(got, planning), what
        census_is(g, got, what + " [ufm_read_map]")
        n[0] += 1

    def host(top, left, patch, what):
        g.patch_map(patch, top, left)
        model.patch(patch, top, left)
        check(what)

    def device(top, left, patch, off, what):
        buf, ptr = device_copy(patch, off)
        bufs.append(buf)
        g.patch_map_device(ptr, top, left, patch.shape[1], patch.shape[0])
        model.patch(patch, top, left)
        check(what)

    def rnd(h, w):
        return rng.integers(1, 256, (h, w)).astype(np.uint8)         # (costs >= 1: the planner steps on these)

    check("set_map")
    assert g.step() == 0
    for k, (x, y) in enumerate([(40, 33), (0, 0), (L - 1, W - 1)]):
        host(x, y, np.array([[(37 * k + 1) % 256]], np.uint8), "1 x 1 at (%d, %d)" % (x, y))
    before = g.read_cost_census()[0]
    host(30, 20, np.ascontiguousarray(model.raw[30:39, 20:33]), "a patch equal to what is there")
    assert np.array_equal(g.read_cost_census()[0], before)
    for x, y in [(0, 0), (0, W - 6), (L - 5, 0), (L - 5, W - 6)]:
        host(x, y, rnd(5, 6), "corner (%d, %d)" % (x, y))
    host(0, 9, rnd(3, 50), "top border"); host(L - 2, 13, rnd(2, 41), "bottom border")
    host(11, 0, rnd(60, 3), "left border"); host(7, W - 4, rnd(33, 4), "right border")
    g.set_start(start[0] + 1, start[1]); assert g.step() == 0
    host(0, 0, rnd(L, W), "the whole map as one patch")
    host(0, 0, np.full((L, W), 255, np.uint8), "the whole map, constant")
    host(0, 0, ufm_amd.synth.cost_map(22, W, L), "the whole map again")
    host(13, 5, rnd(70, 70), "70 x 70: above 4096 cells")
    host(20, 9, (1 + rng.integers(0, 2, (70, 70)) * 254).astype(np.uint8), "70 x 70, binary")
    g.set_start(start[0] + 2, start[1] + 1); assert g.step() == 0
    for k, (x, y) in enumerate([(40, 30), (44, 35), (38, 33)]):              # three overlapping ones before one step: checked together below
        p = rnd(11, 9)
        g.patch_map(p, x, y); model.patch(p, x, y)
    g.set_start(start[0] + 3, start[1] + 1); assert g.step() == 0
    check("three overlapping patches, one step")
    device(50, 41, rnd(7, 13), 1, "device patch, pointer + 1")
    device(3, 60, rnd(9, 9), 3, "device patch, pointer + 3")
    device(8, 2, rnd(70, 70), 5, "device patch 70 x 70, pointer + 5")
    device(L - 1, 0, rnd(1, W), 15, "device patch, a row, pointer + 15")
    g.set_start(start[0] + 4, start[1] + 2); assert g.step() == 0
    check("after the last step")
    assert g.check_layout() == (0, 0)
    assert n[0] >= 24
    g.close()
    for b in bufs:
        b.free()


@pytest.mark.parametrize("name", ["none", "ellipse5", "disc31"])
def test_patches(name):
    """without a footprint (small host patches then go through the staging copy, not the held route), with the 5 x 5 ellipse and with the
    31 x 31 disc, where the planning raster changes outside the patch (the model: test_cspace_surface.dilate_ref)"""
    patch_sequence({"none": ONE, "ellipse5": ELLIPSE5, "disc31": ufm_amd.cspace_disc(31)}[name])


def test_patches_cell_planner():
    """MS-DFM plans on cells: the same census (it counts the raster, not the elements)"""
    patch_sequence(ONE, "DFM", 1)


# ---- 3. the minimum rises ---------------------------------------------------------------------------------------------------------------
def test_minimum_rises_when_the_cheapest_cell_goes():
    rng = np.random.default_rng(3)
    raw = rng.integers(21, 200, (40, 37)).astype(np.uint8)
    raw[5, 5] = 20
    raw[17, 30] = 3                                     # the single cheapest cell
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, True)
    g.reset(); g.set_occupancy_threshold(1.0)
    g.set_param("auto_multiplier", 1)                   # (turns the census on)
    g.set_heuristic_multiplier(77.0)                    # stored, ignored
    g.set_map(raw); g.set_start(4.0, 4.0); g.set_goal(35.0, 33.0)

    def expect(mn, what):
        assert g.read_cost_census()[1] == mn == int(raw.min()), (what, g.read_cost_census()[1:], int(raw.min()))
        g.set_start(4.0 + expect.k, 4.0); expect.k += 1
        assert g.step() == 0
        assert g.heuristic_multiplier() == float(mn), (what, g.heuristic_multiplier())
        census_is(g, raw, what)
    expect.k = 0

    def put(x, y, v):
        raw[x, y] = v
        g.patch_map(np.array([[v]], np.uint8), x, y)
    expect(3, "as set")
    put(17, 30, 40); expect(20, "the cheapest cell patched to 40")
    put(30, 8, 1); expect(1, "another cell patched to 1")
    put(30, 8, 90); expect(20, "that cell patched back")
    g.set_param("auto_multiplier", 0)
    g.set_start(9.0, 4.0); assert g.step() == 0
    assert g.heuristic_multiplier() == 77.0             # back to the caller's
    g.close()


# ---- 4. automatic == host-fed, bit for bit ------------------------------------------------------------------------------------------------
BLOCKS = {2: ((57, 0), 2), 4: ((57, 0), 30), 5: ((0, 57), 25), 6: ((2, 40), 7), 8: ((2, 40), 50)}     # replan -> ((top, left), value) of a 7 x 7 block


def mission64(floor=8):
    """(raw0, start, goal, [(start, [(top, left, patch)])]): synth's 8 replans on 64 x 64 with every cost raised to >= floor and a 7 x 7
    block of 5 in a corner; five of the eight patches are replaced by 7 x 7 blocks of low values placed and removed so that the minimum
    of the raster -- and, the blocks being wider than the footprint, of its dilation -- falls and rises: 5, 2, 5, floor, 7, floor.
    ONE patch per step: the reference's update() seeds from the last patch_map alone, and so does the oracle that restates it."""
    raw0 = np.maximum(ufm_amd.synth.cost_map(33, 64, 64), floor).astype(np.uint8)
    raw0[0:7, 57:64] = 5
    start, goal = ufm_amd.synth.start_goal(64, 64)
    steps = []
    for k, s, top, left, patch in ufm_amd.synth.replan_script(33, 64, 64, n_patches=8, size=11, stride=5):
        if k in BLOCKS:
            (t, l), v = BLOCKS[k]
            steps.append((s, [(t, l, np.full((7, 7), v, np.uint8))]))
        else:
            steps.append((s, [(top, left, np.maximum(patch, floor).astype(np.uint8))]))
    return raw0, start, goal, steps


def queue_sorted(g):
    xy, qg, qrhs, total = g.read_queue()
    order = np.lexsort((xy[:, 1], xy[:, 0]))
    return xy[order], qg[order].view(np.uint32), qrhs[order].view(np.uint32), total


def auto_against_fed(algo, lvl, mask, focused, params=()):
    raw0, start, goal, steps = mission64()
    model = Inflated(raw0, mask, None)
    fed, auto = ufm_amd.Planner(ALGOS[algo], lvl, True), ufm_amd.Planner(ALGOS[algo], lvl, True)
    for p in (fed, auto):
        p.reset(); p.set_occupancy_threshold(1.0)
        p.set_param("focused", focused)
        for name, v in params:
            p.set_param(name, v)
        if mask.size > 1:
            p.set_cspace(mask)
    auto.set_param("auto_multiplier", 1)
    auto.set_heuristic_multiplier(1000.0)                # ignored
    o = orc.OraclePlanner(ALGOS[algo], lvl, True)        # fed the inflated data and the same minimum: says which elements are below the start's key
    o.reset(); o.set_occupancy_threshold(1.0); o.set_map(model.planning()); o.set_start(*start); o.set_goal(*goal)
    for p in (fed, auto):
        p.set_map(raw0); p.set_start(*start); p.set_goal(*goal)
    mins = []

    def one_step(s, what):
        mn = int(model.planning().min())
        mins.append(mn)
        fed.set_heuristic_multiplier(float(mn)); o.set_heuristic_multiplier(float(mn))
        for p in (fed, auto, o):
            p.set_start(*s)
        assert o.step() == 0 and fed.step() == 0 and auto.step() == 0
        assert auto.heuristic_multiplier() == fed.heuristic_multiplier() == float(mn), (what, auto.heuristic_multiplier(), fed.heuristic_multiplier(), mn)
        assert auto.stats.graphs_instantiated == fed.stats.graphs_instantiated, (what, auto.stats.graphs_instantiated, fed.stats.graphs_instantiated)
        census_is(auto, model.planning(), what)
        if algo == "DFM":                               # MS-DFM is not bit-reproducible: each planner against the oracle
            for p, who in ((auto, "auto"), (fed, "fed")):
                check_parity(o, p, "%s %s" % (what, who), below_start_key=True)
            return
        assert auto.stats.updated == fed.stats.updated, (what, auto.stats.updated, fed.stats.updated)
        kw = dict(max_steps=20, lookahead=True, allow_indirect=INDIRECT[algo])
        pa, pb = auto.extract_path(**kw), fed.extract_path(**kw)
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]) and pa[2:] == pb[2:], "%s: the paths differ" % what
        a, b = auto.read_field()[0].view(np.uint32), fed.read_field()[0].view(np.uint32)
        if focused:                                     # final values only below the start's key: there, bit for bit -- and the oracle's
            below = o.trusted_mask(below_start_key=True)
            assert int(below.sum()) > 100, what
            assert np.array_equal(a[below], b[below]), "%s: the fields differ below the start's key in %d elements" % (what, int((a[below] != b[below]).sum()))
            n_, nbad = check_parity(o, auto, what, below_start_key=True)
            assert nbad == 0, what
            return
        assert np.array_equal(a, b), "%s: the fields differ in %d elements" % (what, int((a != b).sum()))
        assert auto.stats.expanded == fed.stats.expanded, (what, auto.stats.expanded, fed.stats.expanded)
        qa, qb = queue_sorted(auto), queue_sorted(fed)
        assert qa[3] == qb[3] and all(np.array_equal(x, y) for x, y in zip(qa[:3], qb[:3])), "%s: the queue views differ (%d, %d)" % (what, qa[3], qb[3])

    one_step(start, "%s plan" % algo)
    for k, (s, patches) in enumerate(steps, 1):
        for top, left, patch in patches:
            for p in (fed, auto):
                p.patch_map(patch, top, left)
            o.patch_map(*model.patch(patch, top, left))
        one_step(s, "%s replan %d" % (algo, k))
    # the script does what it is for: the minimum changes at least 3 times, falls and rises both
    changes = [b - a for a, b in zip(mins, mins[1:]) if a != b]
    assert len(changes) >= 3 and min(changes) < 0 < max(changes), mins
    made = auto.stats.graphs_instantiated
    fed.close(); auto.close()
    return made


VARIANTS4 = [(a, l, m, f, ()) for a, l in (("FD", 1), ("SG", 2)) for m in ("none", "ellipse5") for f in (0, 1)]
VARIANTS4 += [("FD", 1, "none", 0, (("region", 0),)), ("FD", 1, "none", 1, (("region", 0),)), ("DFM", 1, "none", 1, ()), ("DFM", 1, "ellipse5", 1, ())]


@pytest.mark.parametrize("algo,lvl,mask,focused,params", VARIANTS4,
                         ids=["%s-%d-%s-%s%s" % (a, l, m, "focused" if f else "converged", "-graph" if p else "") for a, l, m, f, p in VARIANTS4])
def test_auto_multiplier_equals_host_fed(algo, lvl, mask, focused, params):
    """Two planners on one 64 x 64 mission with heuristic keys, 8 replans, a moving start, the minimum falling and rising: one fed
    float(int(planning.min())) before every step, one with "auto_multiplier".  After every step: the same ufm_heuristic_multiplier, the same
    number of instantiated graphs, the census exact, the same stats.updated and the same extracted path; and
      "converged" ("focused" = 0, every element final after every step): the WHOLE field bit for bit, stats.expanded and the queue view;
      "focused" (the default): the field bit for bit BELOW THE START'S KEY, where it also equals the oracle's.
    Why the whole field is compared under "focused" = 0 only: beyond the start's key a focused search leaves whatever the asynchronous waves
    had reached (include/ufm.h: FD and SG are bit-reproducible below the start's key), and that is no property of this feature -- measured
    on this mission with two IDENTICAL host-fed planners, census never on: SG-2 differs from its twin in 7 elements of the whole field
    after every step and in the queue view (FD-1: in none); with the census on in one of them FD-1 differs in 7 .. 125 elements beyond the
    key, stats.expanded in 2 of 9 steps, the queue view in all; below the key, and with "focused" = 0 everywhere, nothing ever differed.
    MS-DFM is not bit-reproducible: both planners are held to the oracle (helpers.check_parity).
    With ("region", 0) the replans go through the captured graph, whose multiplier travels in the job record: the changing multiplier
    adds no graph to those the host-fed planner makes."""
    made = auto_against_fed(algo, lvl, {"none": ONE, "ellipse5": ELLIPSE5}[mask], focused, params)
    if params:
        assert made > 0, "the replans of this variant were meant to go through the captured graph"


# ---- 5. the reference's own mission -----------------------------------------------------------------------------------------------------
class IgnoresTheHint:
    """a planner whose set_heuristic_multiplier does nothing: the multiplier is the engine's own"""

    def __init__(self, g):
        self.g, self.used = g, []

    def set_heuristic_multiplier(self, m):
        pass

    def step(self):
        rc = self.g.step()
        self.used.append(self.g.heuristic_multiplier())
        return rc

    def __getattr__(self, name):
        return getattr(self.g, name)


def test_reference_mission_with_the_automatic_multiplier():
    """the noise-trap log (tests/test_reference_mission.py) replayed by a planner that is never told a multiplier: every printed position,
    path cost and path length as in the engine's replay that is told.  The minimum is 56 before the first reveal and 38 from the first
    step on: a census not kept under the first patch would plan with 56."""
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 0, True)
    g.set_param("auto_multiplier", 1)
    w = IgnoresTheHint(g)
    n, upd_same, _, _ = check_mission("noise-trap", w, g_counts, False)
    assert (n, upd_same) == (134, 124)
    assert w.used == [38.0] * 134, sorted(set(w.used))
    g.close()


# ---- 6. batches -------------------------------------------------------------------------------------------------------------------------
def run_batch(devices):
    n, L, W = 3, 64, 64
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, True, devices=devices)
    b.set_occupancy_threshold(1.0)
    b.set_param("defer_patches", 1)                      # without effect while the census is on
    b.set_param("auto_multiplier", 1)
    b.set_heuristic_multiplier(500.0)                    # ignored
    start, goal = ufm_amd.synth.start_goal(W, L)
    rs = []
    for m in range(n):
        r = np.maximum(ufm_amd.synth.cost_map(40 + m, W, L), 30 + 5 * m).astype(np.uint8)
        if m == 2:
            r[60, 3] = 9                                 # the batch's cheapest cell: on the last map (the second shard of a sharded handle)
        rs.append(r)
        b.set_map(m, r); b.set_start(m, *start); b.set_goal(m, *goal)
    used, expanded = [], []

    def check(what):
        total = np.zeros(256, np.uint64)
        for m in range(n):
            hist, mn, mx = b.read_cost_census(m)
            assert np.array_equal(hist, count(rs[m])) and (mn, mx) == (int(rs[m].min()), int(rs[m].max())), (what, m)
            assert np.array_equal(b.read_map(m, W, L), rs[m]), (what, m)
            total += hist
        hist, mn, mx = b.read_cost_census(-1)
        assert np.array_equal(hist, total) and int(hist.sum()) == n * L * W, what
        assert (mn, mx) == (min(int(r.min()) for r in rs), max(int(r.max()) for r in rs)), what
        return mn
    mn = check("set_map")
    assert b.step() == 0
    assert b.heuristic_multiplier() == float(mn) == 9.0
    used.append(b.heuristic_multiplier()); expanded.append(int(b.stats.expanded))
    bufs = [DeviceBytes(np.zeros((13, 13), np.uint8)) for _ in range(n)]
    for k in range(1, 5):
        s = (start[0] + 5 * k, start[1] + 4 * k)
        for m in range(n):
            h, w = 7 + 2 * m, 13 - 3 * m + (k % 2)
            top, left = int(s[0]) - 4 + m, int(s[1]) - 3 - m
            patch = (40 + (ufm_amd.synth.h64((40 + m) ^ k, *np.meshgrid(np.arange(top, top + h), np.arange(left, left + w), indexing="ij")) % np.uint64(200))).astype(np.uint8)
            if k == 2 and m == 0:
                patch[0, 0] = 4                          # the minimum moves to the first map ...
            bufs[m].overwrite(patch)
            b.patch_map_device(m, bufs[m].data_ptr(), top, left, w, h); b.set_start(m, *s)
            bufs[m].overwrite(np.zeros_like(patch))      # (a deferred patch would now apply zeros, and the counts would show them)
            rs[m][top:top + h, left:left + w] = patch
        if k == 3:                                       # ... and rises when both cheap cells have gone: host patches, one per round
            b.patch_map(2, np.array([[60]], np.uint8), 60, 3); rs[2][60, 3] = 60
        if k == 4:
            b.patch_map(0, np.array([[80]], np.uint8), 14, 13); rs[0][14, 13] = 80
        mn = check("round %d" % k)
        assert b.step() == 0
        assert b.heuristic_multiplier() == float(mn), (k, b.heuristic_multiplier(), mn)
        used.append(b.heuristic_multiplier()); expanded.append(int(b.stats.expanded))
        check("after step %d" % k)
        assert b.check_layout() == (0, 0)
    assert b.L.ufm_batch_read_cost_census(b.h, 3, None, None, None) == INVALID and b.L.ufm_batch_read_cost_census(b.h, -2, None, None, None) == INVALID
    b.close()
    for d in bufs:
        d.free()
    return used, expanded


def test_batch_one_engine_and_sharded():
    """3 maps on one engine and on a sharded handle [0, 0] (maps 0, 1 | 2): per-map census, i = -1 the sum, the automatic multiplier the
    minimum over ALL maps -- the cheapest cell sits on the last map first, then on the first -- and the same on both handles;
    "defer_patches" = 1 is without effect: device patches whose buffers are overwritten right after the call are counted exactly"""
    one, sharded = run_batch(None), run_batch([0, 0])
    assert one[0] == sharded[0] == [9.0, 9.0, 4.0, 4.0, 30.0], (one[0], sharded[0])
    print("expanded per round, one engine %r, sharded %r" % (one[1], sharded[1]))


# ---- 7. off is off ------------------------------------------------------------------------------------------------------------------------
def test_off_is_off_and_on_mid_mission():
    """a planner that never turns the census on answers UFM_ERR_INVALID and keeps the held route for its host patches (the block kernel
    applies them: what the census declines); turning it on with a held patch pending counts the raster with that patch applied; off
    frees it, on again rebuilds from the raster as it stands"""
    raw = ufm_amd.synth.cost_map(33, 64, 64)
    start, goal = ufm_amd.synth.start_goal(64, 64)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_map(raw); g.set_start(*start); g.set_goal(*goal)
    mn, mx = ufm_amd.capi.C.c_int(0), ufm_amd.capi.C.c_int(0)
    hist = np.zeros(256, np.uint64)

    def read_rc():
        return g.L.ufm_read_cost_census(g.h, hist.ctypes.data, ufm_amd.capi.C.byref(mn), ufm_amd.capi.C.byref(mx))
    assert g.step() == 0
    script = list(ufm_amd.synth.replan_script(33, 64, 64, n_patches=4, size=11, stride=5))
    for k, s, top, left, patch in script[:2]:
        g.patch_map(patch, top, left); raw[top:top + 11, left:left + 11] = patch
        g.set_start(*s)
        assert read_rc() == INVALID
        assert g.step() == 0
    assert g.stats.region_replans > 0 and read_rc() == INVALID
    assert g.heuristic_multiplier() == 1.0
    k, s, top, left, patch = script[2]
    g.patch_map(patch, top, left); raw[top:top + 11, left:left + 11] = patch      # held: not yet in the raster
    g.track_costs()
    census_is(g, raw, "turned on with a held patch pending")
    assert np.array_equal(g.read_map(64, 64), raw)
    g.set_start(*s); assert g.step() == 0
    census_is(g, raw, "after the step")
    g.track_costs(False)
    assert read_rc() == INVALID
    k, s, top, left, patch = script[3]
    g.patch_map(patch, top, left); raw[top:top + 11, left:left + 11] = patch      # while off: nothing counts it
    g.set_start(*s); assert g.step() == 0
    g.track_costs()
    census_is(g, raw, "on again")
    g.reset()                                                                      # ufm_reset leaves the census alone
    assert g.step() == 0
    census_is(g, raw, "after ufm_reset")
    g.set_param("auto_multiplier", 1)
    assert g.L.ufm_track_costs(g.h, 0) == INVALID                                  # not while the multiplier depends on it
    g.set_param("auto_multiplier", 0)
    g.track_costs(False)
    g.close()


# ---- 8. the planner process -----------------------------------------------------------------------------------------------------------------
def test_planner_process_inflates_and_finds_its_multiplier(tmp_path, ref_bitmaps):
    """ufm_planner --inflate 5 --auto-heuristic (the build with heuristic keys) fed by harness.run_mission(planner_inflates=True,
    planner_min_cost=True) -- raw data and a placeholder hint, nothing dilated on the simulator's side -- on the noise-trap bitmap cropped to
    64 x 64, as test_gpu_cspace.test_planner_process_inflates: reaches the goal, and at every move its path is the one of the oracle fed the
    inflated map and the inflated map's true minimum, within that test's bound (test_gpu_path.close_path)"""
    cost, _ = ref_bitmaps["noise-trap"]
    img = np.ascontiguousarray((~cost).astype(np.uint8)[28:92, 28:92])
    (sx, sy), (gx, gy) = (56.0, 56.0), (14.0, 14.0)
    exe = os.path.join(PKG, "ufm_planner")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
    disc = ufm_amd.cspace_disc(5)
    o = orc.OraclePlanner(orc.ALGO_FD, 1, True)
    state = {"moves": 0, "inf": None, "mins": []}

    def on_map(raw, min_cost):
        state["inf"] = Inflated(raw, disc, None)
        planning = state["inf"].planning()
        assert min_cost == int(raw.min())                # the placeholder
        state["mins"].append(int(planning.min()))
        o.reset(); o.set_occupancy_threshold(1); o.set_heuristic_multiplier(float(int(planning.min())))
        o.set_map(planning); o.set_start(sx, sy); o.set_goal(gx, gy)

    def on_move(i, pos, top, left, patch, min_cost, reply):
        path, costs, dist, total, times = reply
        o.patch_map(*state["inf"].patch(patch, top, left))
        true_min = int(state["inf"].planning().min())
        state["mins"].append(true_min)
        o.set_heuristic_multiplier(float(true_min)); o.set_start(*pos)
        assert o.step() == 0
        ref = o.extract_path(max_steps=20, allow_indirect=True)
        close_path((path, costs, total, dist), ref, "mission move %d at %r" % (i, pos))
        state["moves"] += 1

    trace, finished = ufm_amd.harness.run_mission(
        [exe, "--planner", "FD", "--level", "1", "--inflate", "5", "--auto-heuristic"], str(tmp_path / "pipe_1"), str(tmp_path / "pipe_2"),
        img, (sx, sy), (gx, gy), radius=5, cspace_diameter=5, use_heuristic=True, on_map=on_map, on_move=on_move, max_moves=100,
        planner_inflates=True, planner_min_cost=True)
    assert trace[0] == (sx, sy) and state["moves"] == len(trace)
    assert finished, "the planner did not report the goal after %d moves, last position %r" % (len(trace), trace[-1])
