"""-m gpu: position queries -- ufm_extract_paths_from / ufm_batch_extract_paths_from, paths from many positions of one field in a
single call.  Every walk is held bit for bit to the oracle's extractor run on the device's own field from that position (the
directed inputs of tests/path_cases.py, so the comparison inherits their census of traversal cases), and to what the parent's way
-- ufm_set_start + ufm_extract_path, start by start -- returns; the call is held to leave the planner alone (field, queue, own
path, the graphs of the next step, parity with the oracle over a mission), and to its launch shapes (1..65 starts, a chunk
boundary at 65 536), capacities, rejections and the batch / sharded forms."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as orc
import path_cases as pc
import ufm_amd
from helpers import ALGOS, check_parity
from test_gpu_path import same_path

pytestmark = pytest.mark.gpu

CANARY = np.float32(-7777.0)
INFO_DTYPE = np.dtype([("n_points", "<i4"), ("n_costs", "<i4"), ("total_cost", "<f4"), ("total_dist", "<f4"), ("steps", "<i4"), ("e_ms", "<f4")])


def thr_uchar(thr):
    return int(np.float32(thr) * np.float32(255.0))     # Graph.cpp:18-20


class Planned:
    """a directed map planned on the device with `focused = 0` from path_cases.plan_start: every position reads a final field"""

    def __init__(self, algo, name, cost, thr, jobs):
        self.algo, self.name, self.cost, self.tu, self.jobs = algo, name, cost, thr_uchar(thr), jobs
        g = ufm_amd.Planner(pc.ALGOS[algo], 0)
        g.reset()
        g.set_param("focused", 0)
        g.set_occupancy_threshold(thr)
        g.set_map(cost)
        g.set_start(*pc.plan_start(cost))
        g.set_goal(*pc.GOAL)
        assert g.step() == 0
        self.g = g
        self.field = g.read_field()[1]

    def starts(self, lookahead):
        return [s for s, la in self.jobs if la == lookahead]

    def oracle(self, start, max_steps=pc.MAX_STEPS, lookahead=True):
        """(path, moves made) of the oracle's extractor on the device's field"""
        ref = orc.extract_path_field(self.field, self.algo == "DFM", self.cost, self.tu, start, pc.GOAL, max_steps=max_steps,
                                     lookahead=lookahead, allow_indirect=pc.INDIRECT[self.algo])
        return ref, len(orc.path_move_log())


@pytest.fixture(scope="module")
def planned():
    """(algo, k) -> the k-th map of every third of pc.extraction_plan(algo), planned once for the whole module"""
    made = {}

    def get(algo, k=0):
        if (algo, k) not in made:
            made[(algo, k)] = Planned(algo, *pc.extraction_plan(algo)[::3][k])
        return made[(algo, k)]
    yield get
    for p in made.values():
        p.g.close()


def raw_call(g, starts, max_steps, lookahead, indirect, cap_p, cap_c, pad=0):
    """ufm_extract_paths_from with canary-filled buffers of `pad` more records than the call is told of:
    (rc, pts [n + pad, cap_p, 2], costs [n + pad, cap_c], info records [n + pad])"""
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 2)
    n = len(starts)
    pts = np.full((n + pad, cap_p, 2), CANARY, np.float32)
    costs = np.full((n + pad, cap_c), CANARY, np.float32)
    info = np.zeros(n + pad, INFO_DTYPE)
    info["n_points"] = info["steps"] = -5
    rc = g.L.ufm_extract_paths_from(g.h, n, starts.ctypes.data, max_steps, int(lookahead), int(indirect),
                                    pts.ctypes.data if cap_p else None, cap_p, costs.ctypes.data if cap_c else None, cap_c, info.ctypes.data)
    return rc, pts, costs, info


def untouched(pts, costs, info):
    return bool((pts == CANARY).all() and (costs == CANARY).all() and (info["n_points"] == -5).all() and (info["steps"] == -5).all())


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
def test_paths_from_equal_the_oracle_on_the_device_field(planned, algo):
    """every third directed map, all of a map's starts of one lookahead value in ONE call: each path bit-equal to the oracle's
    extractor from that start on the device's field, as many moves as the oracle made"""
    walks = 0
    for k in range(4):
        p = planned(algo, k)
        for la in (True, False):
            starts = p.starts(la)
            paths = p.g.extract_paths_from(starts, max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=pc.INDIRECT[algo])
            assert len(paths) == len(starts)
            for j, s in enumerate(starts):
                what = "%s %s start %r lookahead %d" % (algo, p.name, s, la)
                ref, moves = p.oracle(s, lookahead=la)
                same_path(paths[j], ref, what)
                assert p.g.path_infos[j].steps == moves, "%s: %d moves, the oracle made %d" % (what, p.g.path_infos[j].steps, moves)
                assert p.g.path_infos[j].e_ms == p.g.path_infos[0].e_ms > 0
            walks += len(starts)
    assert walks > 1400, walks


# -------------------------------------------------------------------------------------------------------- 2. equal to the old way
@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
def test_paths_from_equal_set_start_and_extract_path(planned, algo):
    p = planned(algo)
    starts = p.starts(True)[:40]
    kw = dict(max_steps=pc.MAX_STEPS, lookahead=True, allow_indirect=pc.INDIRECT[algo])
    paths = p.g.extract_paths_from(starts, **kw)
    infos = [(i.n_points, i.n_costs, i.steps) for i in p.g.path_infos]
    for j, s in enumerate(starts):
        p.g.set_start(*s)
        one = p.g.extract_path(**kw)
        what = "%s %s start %r" % (algo, p.name, s)
        assert np.array_equal(paths[j][0], one[0]) and np.array_equal(paths[j][1], one[1]), what
        assert paths[j][2] == one[2] and paths[j][3] == one[3], what
        assert infos[j] == (p.g.path_info.n_points, p.g.path_info.n_costs, p.g.path_info.steps), what
    p.g.set_start(*pc.plan_start(p.cost))


# ------------------------------------------------------------------------------------------------------------ 3. no side effects
def queue_total(g):
    total = C.c_int(-1)
    assert g.L.ufm_read_queue(g.h, 0, None, None, C.addressof(total)) == 0
    return total.value


def query_and_check_untouched(g, starts, what, has_start=True):
    kw = dict(max_steps=20, lookahead=True, allow_indirect=True)
    field, queue = g.read_field()[0], queue_total(g)
    own = g.extract_path(**kw) if has_start else None
    paths = g.extract_paths_from(starts, **kw)
    assert len(paths) == len(starts)
    assert np.array_equal(g.read_field()[0], field), "%s: the query changed the field" % what
    assert queue_total(g) == queue, "%s: the query changed the queue" % what
    if has_start:
        same_path(g.extract_path(**kw), own, "%s: the planner's own path after the query" % what)
    return paths


def test_a_query_leaves_the_mission_alone():
    """Field D* level 1 with heuristic keys, focused (the default): a plan and three replans, 64 position queries before the first
    step (once without a start, once with one) and between every two steps -- after a step, before the next patch arrives: a patch
    that is being held is applied by a query as by ufm_extract_path (include/ufm.h), which is not what this test is about.  The
    planner stays in step with an oracle that is never queried and instantiates no more graphs than a twin that is never queried."""
    size, seed = 256, 21
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    starts = pc.starts_for(cost, 9)[::7][:64]
    assert len(starts) == 64
    o = orc.OraclePlanner(ALGOS["FD"], 1, True)
    g, twin = ufm_amd.Planner(ALGOS["FD"], 1, True), ufm_amd.Planner(ALGOS["FD"], 1, True)
    for p in (o, g, twin):
        p.reset()
        p.set_occupancy_threshold(1.0)
        p.set_heuristic_multiplier(1.0)
        p.set_map(cost)
        p.set_goal(*goal)
    query_and_check_untouched(g, starts, "map and goal, no start yet", has_start=False)
    for p in (o, g, twin):
        p.set_start(*start)
    query_and_check_untouched(g, starts, "before the first step")
    for p in (o, g, twin):
        assert p.step() == 0
    check_parity(o, g, "plan", below_start_key=True)
    cur = cost.copy()
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=3, size=15):
        paths = query_and_check_untouched(g, starts, "before replan %d" % k)
        field = g.read_field()[1]
        for j in (0, 31, 63):      # (what the query returns is the oracle's walk over the field it read, focused or not)
            ref = orc.extract_path_field(field, False, cur, 255, starts[j], goal, max_steps=20)
            same_path(paths[j], ref, "before replan %d, start %r" % (k, starts[j]))
        cur[top:top + patch.shape[0], left:left + patch.shape[1]] = patch
        for p in (o, g, twin):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
        assert g.stats.graphs_instantiated <= twin.stats.graphs_instantiated, (k, g.stats.graphs_instantiated, twin.stats.graphs_instantiated)
        n, nbad = check_parity(o, g, "replan %d" % k, below_start_key=True)
        assert nbad == 0
    query_and_check_untouched(g, starts, "after the last replan")
    g.close()
    twin.close()


# ------------------------------------------------------------------------------------------------------------ 4. launch shapes
def test_small_calls_equal_the_entries_of_one_large_call(planned):
    p = planned("FD")
    starts = p.starts(True)[:200]
    kw = dict(max_steps=pc.MAX_STEPS, lookahead=True, allow_indirect=True)
    large = p.g.extract_paths_from(starts, **kw)
    steps = [i.steps for i in p.g.path_infos]
    for n in (1, 2, 3, 4, 5, 63, 64, 65):
        small = p.g.extract_paths_from(starts[:n], **kw)
        assert len(small) == n
        for j in range(n):
            same_path(small[j], large[j], "n_starts %d, entry %d" % (n, j))
            assert p.g.path_infos[j].steps == steps[j]


# ----------------------------------------------------------------------------------------------------------- 5. chunk boundary
def test_totals_across_the_chunk_boundary(planned):
    """65 537 starts, totals only: one more than a launch takes.  The directed list repeated: every record equals the record of the
    same start in the first repetition, and the first, the last of the first chunk and the first of the second equal the oracle"""
    p = planned("FD")
    base = np.asarray(p.starts(True), np.float32)
    n = 65537
    reps = -(-n // len(base))
    starts = np.ascontiguousarray(np.tile(base, (reps, 1))[:n])
    rc, _, _, info = raw_call(p.g, starts, 2, True, True, 0, 0)
    assert rc == 0
    first = info[:len(base)]
    for f in ("n_points", "n_costs", "total_cost", "total_dist", "steps"):
        assert np.array_equal(info[f], np.tile(first[f], reps)[:n]), f
    assert (info["e_ms"] == info["e_ms"][0]).all() and info["e_ms"][0] > 0
    assert (first["n_points"] > 1).any() and (first["total_cost"] > 0).any()
    for j in (0, 65535, 65536):
        ref, moves = p.oracle(tuple(float(v) for v in starts[j]), max_steps=2)
        got = info[j]
        assert (got["n_points"], got["n_costs"], got["steps"]) == (len(ref[0]), len(ref[1]), moves), j
        assert got["total_cost"] == np.float32(ref[2]) and got["total_dist"] == np.float32(ref[3]), j


# --------------------------------------------------------------------------------------------------------------- 6. capacities
def test_capacities_around_a_three_point_move_between_two_neighbours(planned):
    """a start whose path holds a three-point / two-cost move, as the middle of three starts: capacities ending before, inside and
    behind that move -- counts stay full, the stored prefixes are the full paths', nothing is written beyond a path's capacity
    or its count: not into the rest of its record, not into the next start's, not behind the last"""
    done, by_name = 0, {}
    try:
        for algo, name, start, la in pc.found_inputs():
            if algo != "FD" or done >= 2:
                continue
            if name not in by_name:
                by_name[name] = Planned("FD", name, *pc.map_by_name(name), [])
            p = by_name[name]
            ref, _ = p.oracle(start, lookahead=la)
            moves = orc.path_move_log()
            three = [i for i, mv in enumerate(moves) if mv[0] == 3]
            if not three:
                continue
            ip, ic = 1 + int(moves[:three[0], 0].sum()), int(moves[:three[0], 1].sum())
            assert moves[three[0]][1] == 2
            trio = [(3.0, 4.5), start, (20.25, 7.0)]
            full = p.g.extract_paths_from(trio, max_steps=pc.MAX_STEPS, lookahead=la)
            steps = [i.steps for i in p.g.path_infos]
            same_path(full[1], ref, "capacity: full path of the middle start")
            for cap_p, cap_c in [(ip + d, ic + e) for d in (0, 1, 2, 3) for e in (0, 1, 2)]:
                rc, pts, costs, info = raw_call(p.g, trio, pc.MAX_STEPS, la, True, cap_p, cap_c, pad=2)
                assert rc == 0
                what = "cap_pts %d cap_costs %d (three-point move at point %d, cost %d)" % (cap_p, cap_c, ip, ic)
                for j in range(3):
                    fp, fc, tc, td = full[j]
                    assert (info[j]["n_points"], info[j]["n_costs"], info[j]["steps"]) == (len(fp), len(fc), steps[j]), what
                    assert info[j]["total_cost"] == tc and info[j]["total_dist"] == td, what
                    kp, kc = min(cap_p, len(fp)), min(cap_c, len(fc))
                    assert np.array_equal(pts[j, :kp], fp[:kp]) and np.array_equal(costs[j, :kc], fc[:kc]), what + ", start %d" % j
                    assert (pts[j, kp:] == CANARY).all() and (costs[j, kc:] == CANARY).all(), what + ", start %d: written beyond its path" % j
                assert untouched(pts[3:], costs[3:], info[3:]), what + ": written behind the last start's record"
            done += 1
    finally:
        for p in by_name.values():
            p.g.close()
    assert done >= 2, "no found input of Field D* holds a three-point move any more (tests/golden/search_path_cases.py)"


# --------------------------------------------------------------------------------------------------------------- 7. rejections
def test_rejections_write_nothing(planned):
    p = planned("FD")
    length, width = p.cost.shape
    good = [(3.0, 4.5), (10.0, 10.0), (20.25, 7.0)]
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 5.0), (5.0, nan), (inf, 5.0), (5.0, inf), (-inf, 5.0), (-0.5, 5.0), (5.0, -0.5), (length + 0.5, 5.0), (5.0, width + 0.5)):
        rc, pts, costs, info = raw_call(p.g, [good[0], bad, good[2]], pc.MAX_STEPS, True, True, 19, 12)
        assert rc == -22 and untouched(pts, costs, info), bad
    rc, pts, costs, info = raw_call(p.g, [good[0], (float(length), float(width)), (0.0, 0.0)], pc.MAX_STEPS, True, True, 19, 12)
    assert rc == 0 and (info["n_points"] >= 0).all(), "the far corner and the origin are positions of the map"
    # n_starts = 0; a capacity without its buffer; max_steps = 0; no info
    pts = np.full((3, 19, 2), CANARY, np.float32)
    costs = np.full((3, 12), CANARY, np.float32)
    info = np.zeros(3, INFO_DTYPE)
    info["n_points"] = info["steps"] = -5
    s = np.asarray(good, np.float32)
    L, h = p.g.L, p.g.h
    assert L.ufm_extract_paths_from(h, 0, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, -1, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, None, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 6, 1, 1, None, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, None, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 6, 1, 1, pts.ctypes.data, -1, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 0, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, None) == -22
    assert untouched(pts, costs, info)
    # totals only: no buffers at all
    assert L.ufm_extract_paths_from(h, 3, s.ctypes.data, 6, 1, 1, None, 0, None, 0, info.ctypes.data) == 0
    full = p.g.extract_paths_from(good, max_steps=6)
    for j in range(3):
        assert (info[j]["n_points"], info[j]["n_costs"]) == (len(full[j][0]), len(full[j][1]))
        assert info[j]["total_cost"] == full[j][2] and info[j]["total_dist"] == full[j][3]
    # a planner without a goal, and one without a map
    g = ufm_amd.Planner(ALGOS["FD"], 0)
    rc, pts, costs, info = raw_call(g, good, 6, True, True, 19, 12)
    assert rc == -22 and untouched(pts, costs, info), "no map"
    g.set_map(p.cost)
    g.set_start(5.0, 5.0)
    rc, pts, costs, info = raw_call(g, good, 6, True, True, 19, 12)
    assert rc == -22 and untouched(pts, costs, info), "no goal"
    g.close()
    # a map index outside the batch; a map of the batch without a goal
    b = ufm_amd.BatchPlanner(2, ALGOS["FD"], 0)
    for m in range(2):
        b.set_map(m, p.cost)
    b.set_goal(0, *pc.GOAL)
    for maps in ([0, 2, 0], [0, -1, 0], [0, 1, 0]):
        mi = np.asarray(maps, np.int32)
        pts[:], costs[:] = CANARY, CANARY
        info["n_points"] = info["steps"] = -5
        rc = b.L.ufm_batch_extract_paths_from(b.h, 3, mi.ctypes.data, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data)
        assert rc == -22 and untouched(pts, costs, info), maps
    assert b.L.ufm_batch_extract_paths_from(b.h, 3, None, s.ctypes.data, 6, 1, 1, pts.ctypes.data, 19, costs.ctypes.data, 12, info.ctypes.data) == -22
    mi = np.zeros(3, np.int32)
    assert b.L.ufm_batch_extract_paths_from(b.h, 3, mi.ctypes.data, s.ctypes.data, 6, 1, 1, None, 0, None, 0, info.ctypes.data) == 0
    b.close()


# -------------------------------------------------------------------------------------------------------------------- 8. batch
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_batch_jobs_on_hashed_maps(devices):
    """MS-DFM level 1, four different directed maps in one batch (and in a handle of two engines on the one device, two maps each),
    200 walks with a hashed map index each -- unsorted, so a sharded handle has to scatter its results back -- every one equal
    to the oracle's on that map's device field"""
    names = ["bimodal-a", "sparse-a", "stripes-a", "checker-a"]
    maps = [pc.map_by_name(n) for n in names]
    assert all(c.shape == (48, 48) and thr == 1.0 for c, thr in maps)
    b = ufm_amd.BatchPlanner(4, ALGOS["DFM"], 1, devices=devices)
    assert b.shards() == (2 if devices else 1)
    b.set_param("focused", 0)
    b.set_occupancy_threshold(1.0)
    for m, (cost, _) in enumerate(maps):
        b.set_map(m, cost)
        b.set_start(m, *pc.plan_start(cost))
        b.set_goal(m, *pc.GOAL)
    assert b.step() == 0
    fields = [b.read_field(m) for m in range(4)]
    h = ufm_amd.synth.h64
    pool = pc.starts_for(maps[0][0], 7100)
    idx = [int(h(77, k, 0)) % 4 for k in range(200)]
    starts = [pool[int(h(77, k, 1)) % len(pool)] for k in range(200)]
    assert len(set(idx)) == 4 and idx != sorted(idx)
    for la in (True, False):
        paths = b.extract_paths_from(idx, starts, max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=True)
        assert len(paths) == 200
        for k in range(200):
            ref = orc.extract_path_field(fields[idx[k]], True, maps[idx[k]][0], 255, starts[k], pc.GOAL, max_steps=pc.MAX_STEPS,
                                         lookahead=la, allow_indirect=True)
            what = "job %d on map %d (%s) from %r lookahead %d" % (k, idx[k], names[idx[k]], starts[k], la)
            same_path(paths[k], ref, what)
            assert b.path_infos[k].steps == len(orc.path_move_log()), what
    b.close()
