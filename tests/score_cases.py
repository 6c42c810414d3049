"""Inputs of the trajectory-scoring tests, shared by tests/test_score_surface.py (the header's walk on the CPU) and
tests/test_gpu_score.py (the kernel): the maps -- path_cases.make_map's bimodal noise with obstacle speckle, 37 x 43, 16 x 16, 1 x 40
and 3 x 2 cells, at the occupancy thresholds 1.0 and 0.6 --, the directed paths, the hostile ones and the seeded random set.

Directed paths that need a particular neighbourhood (a grid line with the cheaper cell on its left, a vertex between two obstacles
...) are FOUND in the map by a scan in a fixed order, not painted into it: the raster stays the generator's."""
import math

import numpy as np

import path_cases as pc
import score_reference as sr

SIZES = [(37, 43), (16, 16), (1, 40), (3, 2)]           # (length, width) in cells
THRESHOLDS = [1.0, 0.6]
RANDOM_SEED = 20240611      # chosen on the CPU: the reference alone finds 0 of the 2 000 paths doubtful (the cap is 1 %)
N_RANDOM = 2000


def thr_uchar(thr):
    return int(np.float32(thr) * np.float32(255.0))     # Graph.cpp:18-20


def maps():
    """[(name, cost uint8 [length][width], thr, thr_uchar)]"""
    out = []
    for k, (length, width) in enumerate(SIZES):
        cost, _ = pc.make_map("speckle", 900 + k, length, width)
        for thr in THRESHOLDS:
            out.append(("%dx%d@%.1f" % (length, width, thr), cost, thr, thr_uchar(thr)))
    return out


def _free(cost, tu, i, j):
    return 0 <= i < cost.shape[0] and 0 <= j < cost.shape[1] and int(cost[i, j]) < tu


def _scan(cost, pred):
    """the first (i, j), row-major, with pred(i, j); None if there is none"""
    for i in range(cost.shape[0]):
        for j in range(cost.shape[1]):
            if pred(i, j):
                return i, j
    return None


def _free_run(cost, tu, along_rows):
    """the longest run of chargeable cells in one row (along_rows) or one column: (i, j of its first cell, its length)"""
    best = (0, 0, 0)
    length, width = cost.shape
    for a in range(length if along_rows else width):
        run = 0
        for b in range(width if along_rows else length):
            i, j = (a, b) if along_rows else (b, a)
            run = run + 1 if _free(cost, tu, i, j) else 0
            if run > best[2]:
                best = ((i, j - run + 1, run) if along_rows else (i - run + 1, j, run))
    return best


def directed(cost, tu):
    """[(name, points)] on one map; what a name promises is asserted by tests/test_score_surface.py through the reference"""
    L, W = cost.shape
    f = lambda i, j: _free(cost, tu, i, j)
    out = []
    add = lambda name, pts: out.append((name, np.asarray(pts, np.float32).reshape(-1, 2)))
    c = _scan(cost, f)
    if c is None:
        c = (0, 0)
    i, j = c
    add("inside one cell", [(i + 0.25, j + 0.25), (i + 0.75, j + 0.5)])
    add("zero-length segment", [(i + 0.5, j + 0.5), (i + 0.5, j + 0.5)])
    add("zero-length segment in the middle", [(i + 0.25, j + 0.25), (i + 0.5, j + 0.5), (i + 0.5, j + 0.5), (i + 0.75, j + 0.25)])
    add("one point", [(i + 0.5, j + 0.5)])
    add("empty", np.zeros((0, 2)))
    # axis-aligned across many cells: the whole map, and the longest free runs
    add("row, end to end", [(min(L - 0.5, 5.5), 0.0), (min(L - 0.5, 5.5), float(W))])
    add("column, end to end", [(0.0, min(W - 0.5, 7.5)), (float(L), min(W - 0.5, 7.5))])
    ri, rj, rn = _free_run(cost, tu, True)
    add("free run along a row", [(ri + 0.5, rj + 0.125), (ri + 0.5, rj + rn - 0.125)])
    add("free run along a row, backwards", [(ri + 0.25, rj + rn - 0.25), (ri + 0.25, rj + 0.25)])
    ci, cj, cn = _free_run(cost, tu, False)
    add("free run along a column", [(ci + 0.125, cj + 0.5), (ci + cn - 0.125, cj + 0.5)])
    # shallow and steep crossings
    add("shallow", [(min(L, 3.3), min(W, 2.1)), (min(L, 4.1), W * 0.7)])
    add("steep", [(min(L, 2.2), min(W, 7.6)), (L * 0.8, min(W, 8.3))])
    add("shallow in the free run", [(ri + 0.2, rj + 0.1), (ri + 0.8, rj + rn - 0.1)])
    add("steep in the free run", [(ci + 0.1, cj + 0.3), (ci + cn - 0.1, cj + 0.7)])
    add("diagonal of the map", [(0.0, 0.0), (float(L), float(W))])
    # segments ON interior grid lines x = k (cells (k - 1, j) and (k, j)) and y = k (cells (i, k - 1), (i, k))
    pairs = {
        "cheaper before": lambda a, b: f(*a) and f(*b) and cost[a] < cost[b],
        "cheaper behind": lambda a, b: f(*a) and f(*b) and cost[a] > cost[b],
        "obstacle before": lambda a, b: not f(*a) and f(*b),
        "obstacle behind": lambda a, b: f(*a) and not f(*b),
        "both obstacles": lambda a, b: not f(*a) and not f(*b),
    }
    for what, pred in pairs.items():
        hit = _scan(cost, lambda i, j: i >= 1 and pred((i - 1, j), (i, j)))
        if hit:
            add("on a line x = k, " + what, [(float(hit[0]), hit[1] + 0.25), (float(hit[0]), hit[1] + 0.75)])
        hit = _scan(cost, lambda i, j: j >= 1 and pred((i, j - 1), (i, j)))
        if hit:
            add("on a line y = k, " + what, [(hit[0] + 0.75, float(hit[1])), (hit[0] + 0.25, float(hit[1]))])
    if L > 1:
        add("along a whole interior line x = 1", [(1.0, 0.0), (1.0, float(W))])
    if W > 1:
        add("along a whole interior line y = 1", [(float(L), 1.0), (0.0, 1.0)])
    # the four borders
    add("border x = 0", [(0.0, 0.25), (0.0, W - 0.25)])
    add("border x = L", [(float(L), W - 0.25), (float(L), 0.25)])
    add("border y = 0", [(0.25, 0.0), (L - 0.25, 0.0)])
    add("border y = W", [(L - 0.25, float(W)), (0.25, float(W))])
    # exact diagonals through vertices
    hit = _scan(cost, lambda i, j: f(i, j) and f(i + 1, j + 1) and i + 1 < L and j + 1 < W and not f(i, j + 1) and not f(i + 1, j))
    if hit:
        add("diagonal between two obstacles", [(float(hit[0]), float(hit[1])), (hit[0] + 2.0, hit[1] + 2.0)])
        add("diagonal between two obstacles, backwards", [(hit[0] + 2.0, hit[1] + 2.0), (float(hit[0]), float(hit[1]))])
    hit = _scan(cost, lambda i, j: f(i, j) and i + 2 < L and j + 2 < W and not f(i + 1, j + 1) and f(i + 2, j + 2))
    if hit:
        add("diagonal through an obstacle", [(float(hit[0]), float(hit[1])), (hit[0] + 3.0, hit[1] + 3.0)])
    hit = _scan(cost, lambda i, j: f(i, j) and i + 1 < L and j >= 1 and f(i + 1, j - 1) and not f(i, j - 1) and not f(i + 1, j))
    if hit:
        add("anti-diagonal between two obstacles", [(float(hit[0]), hit[1] + 1.0), (hit[0] + 2.0, hit[1] - 1.0)])
    # blocked in the first, a middle and the last segment: a walk inside a free cell that steps into the obstacle beside it
    wall = _scan(cost, lambda i, j: f(i, j) and j + 1 < W and not f(i, j + 1))
    if wall:
        a, b, c = (wall[0] + 0.25, wall[1] + 0.25), (wall[0] + 0.75, wall[1] + 0.25), (wall[0] + 0.75, wall[1] + 0.75)
        d = (wall[0] + 0.5, wall[1] + 1.5)
        add("blocked in the first segment", [a, d, a, b])
        add("blocked in a middle segment", [a, b, c, d, c, b])
        add("blocked in the last segment", [a, b, c, d])
    return out


NAN, INF, BIG = float("nan"), float("inf"), 1e30
FLT_MAX = float(np.finfo(np.float32).max)


def hostile(cost, tu):
    """paths that leave or enter the map, and coordinates no caller should send: [(name, points)]"""
    L, W = cost.shape
    c = _scan(cost, lambda i, j: _free(cost, tu, i, j)) or (0, 0)
    mid = (c[0] + 0.5, c[1] + 0.5)
    out = []
    add = lambda name, pts: out.append((name, np.asarray(pts, np.float32).reshape(-1, 2)))
    add("leaves through x = L", [mid, (L + 3.0, mid[1] + 0.25)])
    add("leaves through y = 0", [mid, (mid[0] + 0.25, -2.5)])
    add("leaves through a corner", [mid, (-1.0 - mid[0], -1.0 - mid[1])])
    add("enters from outside", [(-1.5, mid[1]), mid])
    add("outside all the way", [(-1.5, -1.0), (L + 2.0, -1.0)])
    add("from the border outwards", [(0.0, mid[1]), (-2.0, mid[1])])
    add("inside, then out and back", [mid, (mid[0], -1.0), mid])
    for name, v in (("nan", NAN), ("+inf", INF), ("-inf", -INF), ("1e30", BIG), ("-1e30", -BIG), ("FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX)):
        add("to x = " + name, [mid, (v, mid[1])])
        add("to y = " + name, [mid, (mid[0], v)])
        add("to both = " + name, [mid, (v, v)])
        add("from x = " + name, [(v, mid[1]), mid])
        add("from both = %s to the opposite" % name, [(v, v), (-v, -v)])
        add("good, %s, good" % name, [mid, (mid[0] + 0.125, mid[1] + 0.125), (v, mid[1]), mid, (mid[0] + 0.125, mid[1])])
    add("denormal steps", [(1e-45, 1e-45), (0.0, 0.0), (2e-45, 1e-45)])
    add("minus zero", [(-0.0, -0.0), (min(L, 0.5), min(W, 0.5))])
    return out


def random_paths(cost, n=N_RANDOM, seed=RANDOM_SEED):
    """n seeded paths of 2 .. 40 points with coordinates in [-2, length + 2] x [-2, width + 2]: a quarter each with steps of about 0.3,
    1 and 3 cells (long walks inside the map) and with independent uniform points (long segments)"""
    L, W = cost.shape
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-2.0, -2.0]), np.array([L + 2.0, W + 2.0])
    out = []
    for k in range(n):
        npts = int(rng.integers(2, 41))
        kind = k % 4
        if kind == 3:
            pts = rng.uniform(lo, hi, (npts, 2))
        else:
            step = (0.3, 1.0, 3.0)[kind]
            start = rng.uniform([0.0, 0.0], [float(L), float(W)])
            pts = np.clip(start + np.cumsum(rng.normal(0.0, step, (npts, 2)), axis=0), lo, hi)
            pts[0] = start
        out.append(pts.astype(np.float32))
    return out


def pack(paths):
    """(points float32 [total, 2], offsets int32 [n + 1])"""
    off = np.zeros(len(paths) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in paths])
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in paths]) if paths else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts, np.float32), off


def check_record(rec, ref, chain, what):
    """one record (a mapping with ufm_score's members) against the reference's, within the bound of tolerances.SCORE_FP64_CHAIN;
    returns the deviations in units of their bounds (cost_before, dist)"""
    assert not ref["doubtful"], what
    assert int(rec["blocked_segment"]) == ref["blocked_segment"], (what, rec, ref)
    assert int(rec["pieces"]) == ref["pieces"], (what, rec, ref)
    blocked = ref["blocked_segment"] >= 0
    assert (float(rec["cost"]) == math.inf) == blocked, (what, rec, ref)
    bound = sr.score_bound(ref["cost_before"], ref["pieces"], ref["cmax"], ref["mcoord"], chain)
    dev = abs(float(rec["cost_before"]) - ref["cost_before"])
    assert dev <= bound, (what, "cost_before", float(rec["cost_before"]), ref["cost_before"], dev, bound)
    if not blocked:
        assert float(rec["cost"]) == float(rec["cost_before"]), (what, rec)
        assert float(rec["blocked_at"]) == 0.0, (what, rec)
    else:
        assert abs(float(rec["blocked_at"]) - ref["blocked_at"]) <= 4 * 2.0 ** -24, (what, "blocked_at", float(rec["blocked_at"]), ref["blocked_at"])
    units = [dev / bound if bound else 0.0]
    if ref["dist"] <= FLT_MAX:
        nseg = max(ref.get("segments", 0), 1)
        dbound = sr.dist_bound(ref["dist"], nseg, ref["mcoord"], chain)
        ddev = abs(float(rec["dist"]) - ref["dist"])
        assert ddev <= dbound, (what, "dist", float(rec["dist"]), ref["dist"], ddev, dbound)
        units.append(ddev / dbound if dbound else 0.0)
    else:
        assert float(rec["dist"]) == math.inf, (what, rec)
    return units

