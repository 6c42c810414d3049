"""-m gpu: trajectory scoring -- ufm_score_paths and its three siblings, k_score_paths -- against the float64 restatement of
tests/score_reference.py, under the bound of ufm_amd.tolerances.SCORE_FP64_CHAIN.  The inputs are those of tests/score_cases.py, which
tests/test_score_surface.py has already run through the same walk on the CPU: the directed and the hostile paths on every map and
threshold, the random set.  Beyond the values: the launch shapes (paths around 64 segments, a chunk boundary at 65 536 paths) with a
fixed path's record bit-identical wherever it stands, the raster that is in force (footprint, held patch, threshold), a mission
that must not notice the scoring calls, the batch and sharded forms with their rejections, the device form on torch tensors, the
extractor's own moves as paths (the project's yardstick for the charging rule), and the staging buffers under growth."""
import math

import numpy as np
import pytest

import oracle_py as orc
import path_cases as pc
import score_cases as sc
import score_reference as sr
import ufm_amd
from ufm_amd_pkg import capi

pytestmark = pytest.mark.gpu

CHAIN = ufm_amd.tolerances.SCORE_FP64_CHAIN
MAPS = sc.maps()
SENTINEL = -12345
FD = ufm_amd.ALGO_FD


def scorer(cost, thr, configure=None):
    """a planner with a raster and nothing else: no start, no goal, no step"""
    p = ufm_amd.Planner(FD, 0)
    p.reset()
    p.set_occupancy_threshold(thr)
    if configure:
        configure(p)
    p.set_map(cost)
    return p


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_all(rec, paths, cost, tu, what, refs=None):
    """every record against the reference; returns (worst deviations in units of the bound, the references)"""
    refs = refs or [sr.score_path(p, cost, tu) for p in paths]
    worst = [0.0, 0.0]
    assert len(rec) == len(paths)
    for k, (r, ref) in enumerate(zip(rec, refs)):
        if ref["doubtful"]:
            continue
        u = sc.check_record(r, ref, CHAIN, "%s, path %d" % (what, k))
        worst = [max(a, b) for a, b in zip(worst, u + [0.0])]
    return worst, refs


# --------------------------------------------------------------------------------------------------------- 1. directed geometry
@pytest.mark.parametrize("case", range(len(MAPS)), ids=[m[0] for m in MAPS])
def test_directed_paths(case):
    name, cost, thr, tu = MAPS[case]
    cases = sc.directed(cost, tu)
    p = scorer(cost, thr)
    rec = p.score_paths([pts for _, pts in cases])
    p.close()
    for (what, pts), r in zip(cases, rec):
        sc.check_record(r, sr.score_path(pts, cost, tu), CHAIN, "%s: %s" % (name, what))


# ----------------------------------------------------------------------------------------- 2. leaving, entering, hostile coordinates
@pytest.mark.parametrize("case", range(len(MAPS)), ids=[m[0] for m in MAPS])
def test_hostile_paths(case):
    """the inputs the CPU driver has walked to their end (tests/test_score_surface.py): every call returns, every record is the
    defined one"""
    name, cost, thr, tu = MAPS[case]
    cases = sc.hostile(cost, tu)
    p = scorer(cost, thr)
    rec = p.score_paths([pts for _, pts in cases])
    p.close()
    for (what, pts), r in zip(cases, rec):
        sc.check_record(r, sr.score_path(pts, cost, tu), CHAIN, "%s: %s" % (name, what))
        if not np.isfinite(pts).all() or what.startswith(("leaves", "enters", "outside", "from the border")):
            assert r["blocked_segment"] >= 0 and r["cost"] == np.inf, (name, what, r)


# ------------------------------------------------------------------------------------------------------ 3. wave and chunk edges
def zigzag(cost, tu, nseg, seed):
    """nseg segments back and forth inside the longest free run of a row: free, with several pieces each"""
    ri, rj, rn = sc._free_run(cost, tu, True)
    assert rn >= 4
    rng = np.random.default_rng(seed)
    pts = np.empty((nseg + 1, 2))
    pts[:, 0] = ri + rng.uniform(0.05, 0.95, nseg + 1)
    pts[0::2, 1] = rj + rng.uniform(0.05, 0.9, len(pts[0::2]))
    pts[1::2, 1] = rj + rn - rng.uniform(0.05, 0.9, len(pts[1::2]))
    return pts.astype(np.float32)


def test_paths_around_the_wave_width():
    """1, 63, 64, 65 and 200 segments, free (every lane block adds to the sums) and with the one blocked segment in the first, the
    second and the fourth block of 64"""
    name, cost, thr, tu = MAPS[0]
    wall = sc._scan(cost, lambda i, j: sc._free(cost, tu, i, j) and j + 1 < cost.shape[1] and not sc._free(cost, tu, i, j + 1))
    paths = [zigzag(cost, tu, n, 40 + n) for n in (1, 63, 64, 65, 200)]
    for at in (10, 64, 70, 199):
        q = zigzag(cost, tu, 200, 300 + at)
        q[at] = (wall[0] + 0.5, wall[1] + 0.5)
        q[at + 1] = (wall[0] + 0.5, wall[1] + 1.5)       # segment `at` steps into an obstacle
        paths.append(q)
    p = scorer(cost, thr)
    rec = p.score_paths(paths)
    worst, refs = check_all(rec, paths, cost, tu, "wave width")
    assert [r["blocked_segment"] for r in refs[:5]] == [-1] * 5 and [r["segments"] for r in refs[:5]] == [1, 63, 64, 65, 200]
    assert refs[4]["pieces"] >= 800
    blocked = [r["blocked_segment"] for r in refs[5:]]
    assert all(0 <= b <= at for b, at in zip(blocked, (10, 64, 70, 199))) and blocked[3] >= 128, blocked
    # a long path's record does not depend on its neighbours either
    alone = p.score_paths([paths[4]])
    mixed = p.score_paths(paths[5:] + [paths[4]] + paths[:3])
    assert same_bytes(alone[0:1], rec[4:5]) and same_bytes(mixed[4:5], rec[4:5])
    p.close()


def test_chunk_boundary_and_bit_identity():
    """65 537 two-point paths in one call -- one more than a launch takes; one fixed path alone, first, last of the first chunk and
    in the second chunk: the same 24 bytes every time.  A sample of the others against the reference."""
    name, cost, thr, tu = MAPS[0]
    L, W = cost.shape
    n = 65537
    rng = np.random.default_rng(5)
    pts = rng.uniform([-1.0, -1.0], [L + 1.0, W + 1.0], (n, 2, 2)).astype(np.float32)
    ri, rj, rn = sc._free_run(cost, tu, True)
    fixed = np.array([(ri + 0.3, rj + 0.2), (ri + 0.7, rj + rn - 0.3)], np.float32)
    for k in (0, 65535, 65536):
        pts[k] = fixed
    off = (2 * np.arange(n + 1)).astype(np.int32)
    p = scorer(cost, thr)
    rec = p.score_paths((pts.reshape(-1, 2), off))
    alone = p.score_paths([fixed])
    p.close()
    assert len(rec) == n
    ref = sr.score_path(fixed, cost, tu)
    assert ref["blocked_segment"] == -1 and ref["pieces"] >= 4
    sc.check_record(alone[0], ref, CHAIN, "the fixed path")
    for k in (0, 65535, 65536):
        assert same_bytes(rec[k:k + 1], alone), k
    sample = list(range(1, n, 997)) + [65534, 65535, 65536]
    check_all(rec[sample], [pts[k] for k in sample], cost, tu, "sample of the 65 537")


# ------------------------------------------------------------------------------------------------------------ 4. raster in force
def test_the_planning_raster_is_scored():
    name, cost, thr, tu = MAPS[0]
    L, W = cost.shape
    paths = [pts for _, pts in sc.directed(cost, tu)]
    # a footprint: the dilated raster, not the caller's
    p = scorer(cost, thr, lambda q: q.set_cspace(ufm_amd.cspace_disc(5)))
    planning, raw = p.read_map(W, L), p.read_raw_map(W, L)
    assert np.array_equal(raw, cost) and (planning != raw).any()
    rec = p.score_paths(paths)
    check_all(rec, paths, planning, tu, "footprint: the planning raster")
    ri, rj, rn = sc._free_run(cost, tu, True)
    chosen = np.array([(ri + 0.5, rj + 0.125), (ri + 0.5, rj + rn - 0.125)], np.float32)
    on_raw, on_planning = sr.score_path(chosen, raw, tu), sr.score_path(chosen, planning, tu)
    assert on_raw["blocked_segment"] == -1 and (on_planning["blocked_segment"], on_planning["cost_before"]) != (-1, on_raw["cost_before"])
    got = p.score_paths([chosen])[0]
    sc.check_record(got, on_planning, CHAIN, "footprint: the chosen path")
    assert (int(got["blocked_segment"]), float(got["cost_before"])) != (-1, float(np.float32(on_raw["cost_before"])))
    p.close()
    # a small host patch that no step has consumed is seen
    p = scorer(cost, thr)
    p.set_start(float(ri), float(rj))
    p.set_goal(*pc.GOAL)
    assert p.step() == 0
    before = p.score_paths([chosen])[0]
    sc.check_record(before, on_raw, CHAIN, "before the patch")
    patch = np.full((1, 2), 255, np.uint8)
    p.patch_map(patch, ri, rj + 1)
    now = cost.copy()
    now[ri, rj + 1:rj + 3] = 255
    after = p.score_paths([chosen])[0]
    sc.check_record(after, sr.score_path(chosen, now, tu), CHAIN, "after the held patch")
    assert after["blocked_segment"] == 0 and after["pieces"] == 1
    assert np.array_equal(p.read_map(W, L), now)
    # the threshold: a cell of value >= 153 is an obstacle at 0.6
    cell = sc._scan(now, lambda i, j: 153 <= int(now[i, j]) < 255)
    inside = np.array([(cell[0] + 0.25, cell[1] + 0.25), (cell[0] + 0.75, cell[1] + 0.75)], np.float32)
    assert p.score_paths([inside])[0]["blocked_segment"] == -1
    p.set_occupancy_threshold(0.6)
    got = p.score_paths([inside])[0]
    assert got["blocked_segment"] == 0 and got["cost"] == np.inf and got["pieces"] == 0
    check_all(p.score_paths(paths), paths, now, sc.thr_uchar(0.6), "threshold 0.6")
    p.close()


# ------------------------------------------------------------------------------------------------------------------ 5. read-only
SCHEDULED = {"tile_visits", "tile_iters", "elem_evals", "resident_tile_visits"}      # (tests/test_gpu_surface_twins.py)


def test_scoring_leaves_the_mission_alone():
    """plan and three replans of Field D* level 1 on two handles; one of them scores paths between every two calls of the mission,
    the twin never does: fields, queue views, the steps' statistics (all but the measured times and the four counts of what the
    asynchronous waves happened to do), extracted paths and step deltas are the same"""
    W_, L_ = 96, 80
    cost = ufm_amd.synth.cost_map(3, W_, L_)
    rng = np.random.default_rng(17)
    paths = [rng.uniform([0.0, 0.0], [float(L_), float(W_)], (int(rng.integers(2, 20)), 2)).astype(np.float32) for _ in range(40)]
    g, twin = ufm_amd.Planner(FD, 1, False), ufm_amd.Planner(FD, 1, False)
    now = cost.copy()

    def score():
        check_all(g.score_paths(paths), paths, now, 255, "between two calls of the mission")

    def everyone(call, then_score=True):
        call(g)
        call(twin)
        if then_score:
            score()

    def compare(what):
        a, b = g.stats.as_dict(), twin.stats.as_dict()
        for k in a:
            if k in SCHEDULED:
                assert (a[k] > 0) == (b[k] > 0), (what, k, a[k], b[k])
            elif not k.endswith("_ms"):
                assert a[k] == b[k], (what, k, a[k], b[k])
        score()
        fa, fb = g.read_field(), twin.read_field()
        assert same_bytes(fa[0], fb[0]) and same_bytes(fa[1], fb[1]), what
        score()
        qa, qb = g.read_queue(), twin.read_queue()
        assert qa[3] == qb[3], what
        for x, y in zip(qa[:3], qb[:3]):
            oa, ob = np.lexsort((qa[0][:, 1], qa[0][:, 0])), np.lexsort((qb[0][:, 1], qb[0][:, 0]))
            assert same_bytes(x[oa], y[ob]), what
        score()
        pa, pb = g.extract_path(max_steps=40), twin.extract_path(max_steps=40)
        assert same_bytes(pa[0], pb[0]) and same_bytes(pa[1], pb[1]) and pa[2:] == pb[2:] and len(pa[0]) > 1, what
        score()
        ca, cb = g.read_changes(), twin.read_changes()
        oa, ob = np.lexsort((ca[0][:, 1], ca[0][:, 0])), np.lexsort((cb[0][:, 1], cb[0][:, 0]))
        assert same_bytes(ca[0][oa], cb[0][ob]) and same_bytes(ca[1][oa], cb[1][ob]) and len(ca[0]) > 0, what
        score()

    everyone(lambda q: (q.reset(), q.set_occupancy_threshold(1.0), q.set_param("focused", 0), q.track_changes(True)), then_score=False)
    everyone(lambda q: q.set_map(cost))
    everyone(lambda q: q.set_start(6.0, 5.0))
    everyone(lambda q: q.set_goal(float(L_ - 7), float(W_ - 6)))
    everyone(lambda q: q.step())
    compare("plan")
    for k in range(3):
        patch = rng.integers(1, 255, (9, 7)).astype(np.uint8)
        x, y = 20 + 11 * k, 30 + 9 * k
        now[x:x + 9, y:y + 7] = patch
        everyone(lambda q: q.patch_map(patch, x, y))
        everyone(lambda q: q.set_start(7.0 + k, 6.5 + k))
        everyone(lambda q: q.step())
        compare("replan %d" % k)
    g.close()
    twin.close()


# ------------------------------------------------------------------------------------------------- 6. batch and sharded handle
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_batch_scores_by_map_index(devices):
    """three different maps in one batch (and in a handle of two engines on the one device), 120 paths with a scrambled map index
    each, maps named repeatedly: every record is the reference's on that map, in the caller's order"""
    L, W = 37, 43
    costs = [pc.make_map("speckle", s, L, W)[0] for s in (900, 910, 911)]
    b = ufm_amd.BatchPlanner(3, FD, 0, devices=devices)
    assert b.shards() == (2 if devices else 1)
    b.set_occupancy_threshold(1.0)
    for m, c in enumerate(costs):
        b.set_map(m, c)
    pool = [p for c in costs for _, p in sc.directed(c, 255)] + sc.random_paths(costs[0], 60, 7)
    h = ufm_amd.synth.h64
    idx = [int(h(91, k, 0)) % 3 for k in range(120)]
    paths = [pool[int(h(91, k, 1)) % len(pool)] for k in range(120)]
    assert len(set(idx)) == 3 and idx != sorted(idx)
    rec = b.score_paths(idx, paths)
    assert len(rec) == 120
    for k in range(120):
        ref = sr.score_path(paths[k], costs[idx[k]], 255)
        if not ref["doubtful"]:
            sc.check_record(rec[k], ref, CHAIN, "path %d on map %d" % (k, idx[k]))
    # the same paths, map by map, through a planner: the same bytes
    for m, c in enumerate(costs):
        mine = [k for k in range(120) if idx[k] == m]
        p = scorer(c, 1.0)
        one = p.score_paths([paths[k] for k in mine])
        p.close()
        assert same_bytes(one, rec[mine]), m
    b.close()


def raw_score(h, maps, off, pts, n=None):
    """ufm_score_paths / ufm_batch_score_paths with a sentinel-filled output: (rc, records)"""
    off = np.ascontiguousarray(off, np.int32)
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(off) - 1 if n is None else n
    out = np.zeros(max(len(off) - 1, 1), capi.SCORE_DTYPE)
    out["pieces"] = out["blocked_segment"] = SENTINEL
    if maps is None:
        rc = h.L.ufm_score_paths(h.h, n, off.ctypes.data, pts.ctypes.data, out.ctypes.data)
    else:
        mi = np.ascontiguousarray(maps, np.int32)
        rc = h.L.ufm_batch_score_paths(h.h, n, mi.ctypes.data, off.ctypes.data, pts.ctypes.data, out.ctypes.data)
    return rc, out


def untouched(out):
    return bool((out["pieces"] == SENTINEL).all() and (out["blocked_segment"] == SENTINEL).all() and (out["cost"] == 0).all())


def test_planner_and_batch_of_one_give_the_same_bytes_and_rejections_write_nothing():
    name, cost, thr, tu = MAPS[0]
    paths = [p for _, p in sc.directed(cost, tu)] + [p for _, p in sc.hostile(cost, tu)]
    pts, off = sc.pack(paths)
    p = scorer(cost, thr)
    b = ufm_amd.BatchPlanner(1, FD, 0)
    b.set_occupancy_threshold(thr)
    b.set_map(0, cost)
    assert same_bytes(p.score_paths(paths), b.score_paths(np.zeros(len(paths), np.int32), paths))
    rc, out = raw_score(p, None, off, pts)
    assert rc == 0 and same_bytes(out, p.score_paths((pts, off)))
    # n_paths < 1, offsets that do not start at 0, decreasing offsets, NULL buffers
    assert raw_score(p, None, off, pts, n=0)[0] == -22 and raw_score(p, None, off, pts, n=-3)[0] == -22
    for bad in (off + 1, np.array([0, 4, 2, 6], np.int32)):
        rc, out = raw_score(p, None, bad, pts)
        assert rc == -22 and untouched(out)
    out = np.zeros(3, capi.SCORE_DTYPE)
    assert p.L.ufm_score_paths(p.h, 3, None, pts.ctypes.data, out.ctypes.data) == -22
    assert p.L.ufm_score_paths(p.h, 3, off.ctypes.data, None, out.ctypes.data) == -22
    assert p.L.ufm_score_paths(p.h, 3, off.ctypes.data, pts.ctypes.data, None) == -22
    assert p.L.ufm_score_paths_device(p.h, 0, 4, off.ctypes.data, pts.ctypes.data, out.ctypes.data) == -22
    assert p.L.ufm_score_paths_device(p.h, 3, -1, off.ctypes.data, pts.ctypes.data, out.ctypes.data) == -22
    assert p.L.ufm_score_paths_device(p.h, 3, 4, None, pts.ctypes.data, out.ctypes.data) == -22
    p.close()
    b.close()
    # a planner without a map
    g = ufm_amd.Planner(FD, 0)
    rc, out = raw_score(g, None, off, pts)
    assert rc == -22 and untouched(out)
    g.close()
    # a map index outside the batch, a map of the batch without a raster, no map indices
    b = ufm_amd.BatchPlanner(2, FD, 0)
    b.set_map(0, cost)
    three = off[:4]
    for maps in ([0, 2, 0], [0, -1, 0], [0, 1, 0]):
        rc, out = raw_score(b, maps, three, pts)
        assert rc == -22 and untouched(out), maps
    out = np.zeros(3, capi.SCORE_DTYPE)
    assert b.L.ufm_batch_score_paths(b.h, 3, None, three.ctypes.data, pts.ctypes.data, out.ctypes.data) == -22
    assert b.L.ufm_batch_score_paths_device(b.h, 1, 3, 4, three.ctypes.data, pts.ctypes.data, out.ctypes.data) == -22      # (map 1 has no raster)
    assert b.L.ufm_batch_score_paths_device(b.h, 2, 3, 4, three.ctypes.data, pts.ctypes.data, out.ctypes.data) == -22
    rc, out = raw_score(b, [0, 0, 0], three, pts)
    assert rc == 0 and not untouched(out)
    b.close()


# ----------------------------------------------------------------------------------------------------------------- 7. device form
def test_device_form_on_device_buffers():
    """offsets, points and records in HBM (helpers.DeviceBytes, the buffers of the ufm_patch_map_device tests): the checks of
    tests/score_device_checks.py in this process"""
    import score_device_checks
    score_device_checks.run_checks(score_device_checks.device_bytes_runner)


def test_device_form_on_torch_tensors():
    """the same checks with torch tensors on the GPU, in a process of their own that imports torch FIRST: torch brings its own HIP
    runtime, and a process that has already opened the GPU through another copy of it -- as this one has -- gets no device from
    torch.  That process is what this test is about: a consumer whose rollouts are tensors starts the same way."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle"), here] +
                                                      [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.join(here, "score_device_checks.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "device form checks passed (torch tensors)" in r.stdout


# ---------------------------------------------------------------------------------------------- 8. the extractor's own way points
MOVE_PLAN = pc.extraction_plan("FD")


@pytest.mark.parametrize("case", range(len(MOVE_PLAN)), ids=[m[0] for m in MOVE_PLAN])
def test_moves_of_the_extractor_cost_what_the_extractor_charged(case):
    """Field D* with indirect traversals on one directed map of tests/path_cases.py -- all ten of them, each with every start of its
    plan, extracted with that start's own lookahead flag: every real move of every extraction, scored as a path of its own, costs
    what the move's step costs add up to, within path_cases.move_bound"""
    name, cost, thr, jobs = MOVE_PLAN[case]
    tu = sc.thr_uchar(thr)
    g = ufm_amd.Planner(FD, 0)
    g.reset()
    g.set_param("focused", 0)
    g.set_occupancy_threshold(thr)
    g.set_map(cost)
    g.set_start(*pc.plan_start(cost))
    g.set_goal(*pc.GOAL)
    assert g.step() == 0
    field = g.read_field()[1]
    moves_as_paths, charged, extractions = [], [], 0
    for la in (True, False):
        starts = [s for s, l in jobs if l == la]
        assert starts, (name, la)
        walks = g.extract_paths_from(starts, max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=True)
        for start, (pts, costs, _, _) in zip(starts, walks):
            orc.extract_path_field(field, False, cost, tu, start, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=True)
            moves = orc.path_move_log()
            extractions += 1
            if len(pts) == 0:
                continue
            assert int(moves[:, 0].sum()) == len(pts) - 1 and int(moves[:, 1].sum()) == len(costs), (name, start, la)
            ip = ic = 0
            for mv in moves:
                ns, nc = int(mv[0]), int(mv[1])
                if ns == 0:
                    continue
                moves_as_paths.append(pts[ip:ip + ns + 1])
                charged.append(float(np.asarray(costs[ic:ic + nc], np.float64).sum()))
                ip += ns
                ic += nc
    assert extractions == len(jobs)
    rec = g.score_paths(moves_as_paths)
    g.close()
    worst = 0.0
    for k, (mv, want, r) in enumerate(zip(moves_as_paths, charged, rec)):
        ref = sr.score_path(mv, cost, tu)
        assert r["blocked_segment"] == -1, (name, k, mv.tolist(), r)
        bound = pc.move_bound(len(mv) - 1, float(np.abs(mv).max()), ref["cmax"], want)
        dev = abs(float(r["cost"]) - want)
        assert dev <= bound, (name, k, mv.tolist(), float(r["cost"]), want, dev, bound)
        worst = max(worst, dev / bound)
    print("moves of the extractor scored as paths, %s (%d x %d): %d extractions, %d real moves, worst deviation %.4f of move_bound" % (
        name, cost.shape[0], cost.shape[1], extractions, len(moves_as_paths), worst))
    assert len(moves_as_paths) > 500


# ------------------------------------------------------------------------------------------------------------------------ 9. random
def test_random_paths():
    name, cost, thr, tu = MAPS[0]
    paths = sc.random_paths(cost)
    refs = [sr.score_path(p, cost, tu) for p in paths]
    doubtful = sum(r["doubtful"] for r in refs)
    assert len(paths) == 2000 and doubtful <= 20
    p = scorer(cost, thr)
    rec = p.score_paths(paths)
    p.close()
    worst, _ = check_all(rec, paths, cost, tu, "random", refs)
    print("random set on the device: %d doubtful; worst deviation in units of the bound: cost %.4f, dist %.4f" % (doubtful, worst[0], worst[1]))


# -------------------------------------------------------------------------------------------------------------------- 10. resources
def test_staging_grows_under_use():
    """a 3-path call and the 65 537-path call in turn -- the staging buffers are freed and made anew while the handle is in use --
    answer like a fresh handle that makes only the large call; then the handles are destroyed"""
    name, cost, thr, tu = MAPS[0]
    L, W = cost.shape
    n = 65537
    rng = np.random.default_rng(6)
    pts = rng.uniform([0.0, 0.0], [float(L), float(W)], (n, 2, 2)).astype(np.float32).reshape(-1, 2)
    off = (2 * np.arange(n + 1)).astype(np.int32)
    small = [p for _, p in sc.directed(cost, tu)[:3]]
    a, b = scorer(cost, thr), scorer(cost, thr)
    s1 = a.score_paths(small)
    l1 = a.score_paths((pts, off))
    s2 = a.score_paths(small)
    l2 = a.score_paths((pts, off))
    fresh = b.score_paths((pts, off))
    assert same_bytes(s1, s2) and same_bytes(l1, l2) and same_bytes(l1, fresh)
    check_all(s1, small, cost, tu, "the small call")
    a.close()
    b.close()
