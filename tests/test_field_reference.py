"""The oracle's fields against the float64 operators of tests/field_reference.py (CPU only).

Every other field test holds the engine to oracle/ufm_oracle.c, a restatement written next to the engine from the same reading of the
reference.  Here the oracle itself is held to a criterion that needs no second planner: each value G(s) of its trusted set is, to a
fraction of an ulp, what the operator -- restated from the geometry, in float64 -- makes of the neighbours of s in the same field.  The
criterion is local, so it does not grow with the map, and a misread edge, stencil pair or case formula moves it by thousands of ulp.

MAPS: field_reference.recipe_map(SEED, ...) at 37 x 43 (three ragged tiles each way), 16 x 16, 17 x 17, 1 x 40 and 3 x 2, thresholds 1.0
and 0.6, every (algorithm, level) the oracle has; levels 1 and 2 also after each of four random patches with a moved start.

BOUNDS (ufm_amd.tolerances.NODE_LOCAL_ULP / DFM_LOCAL_ULP): twice the worst residual of the ORACLE over all of the above, rounded up
to a whole ulp; test_bounds_are_the_measurement recomputes them.  Measured: node planners 0.919 ulp, MS-DFM 1.423 ulp (1.131 on the fresh plans).  The comparison
window (field_reference) was needed by no element.

SEEDS tried for the census floors (every deciding Field D* case the first minimum of >= 5 trusted elements in float64, and the only case
at the minimum of at least one, over this file's Field D* maps): 1 .. 8 all meet them over the file (rarest: II with c > b, 6 .. 19; A with c > b, 21 .. 44); at 37 x 43 and threshold 1.0
alone seeds 6, 7 do not (II with c > b: 2, 3).  SEED = 5: 14 and 31 over the file, 7 and 17 on the one map.

TYPE III decides nothing, on any map: test_type_iii_never_decides."""
import functools
import math

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
import field_reference as fr

SEED = 5
SIZES = [(37, 43), (16, 16), (17, 17), (1, 40), (3, 2)]
THRESHOLDS = [1.0, 0.6]
PLANNERS = [("FD", 0), ("FD", 1), ("SG", 0), ("SG", 1), ("SG", 2), ("DFM", 0), ("DFM", 1)]
ALGOS = {"FD": fr.FD, "SG": fr.SG, "DFM": fr.DFM}
NODE_BOUND = ufm_amd.tolerances.NODE_LOCAL_ULP
DFM_BOUND = ufm_amd.tolerances.DFM_LOCAL_ULP
CENSUS_FLOOR = 5


def bound_for(algo):
    return DFM_BOUND if algo == "DFM" else NODE_BOUND


def planner(algo, lvl, cost, thr, start, goal):
    o = orc.OraclePlanner(ALGOS[algo], lvl, False)
    o.reset(); o.set_occupancy_threshold(thr); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
    assert o.step() == 0
    return o


def patches(seed, cost, thr, n=4):
    """random rectangular patches that add and remove obstacles, each with a start moved to a random free cell
    (as tests/test_gpu_parity.py::test_random_small_maps_with_obstacles_and_patches) -> [(patch, top, left, start, raster after it)]"""
    rng = np.random.default_rng(1000 + seed)
    length, width = cost.shape
    cur, out = cost.copy(), []
    for _ in range(n):
        ph, pw = int(rng.integers(1, min(length, 20) + 1)), int(rng.integers(1, min(width, 20) + 1))
        top, left = int(rng.integers(0, length - ph + 1)), int(rng.integers(0, width - pw + 1))
        patch = rng.integers(1, 255, (ph, pw), dtype=np.uint8)
        patch[rng.random((ph, pw)) < 0.15] = 255
        cur[top:top + ph, left:left + pw] = patch
        free = np.argwhere(cur < fr.threshold_byte(thr))
        a = free[rng.integers(len(free))] if len(free) else np.array([0, 0])
        out.append((patch, top, left, (float(a[0]), float(a[1])), cur.copy()))
    return out


@functools.lru_cache(maxsize=None)
def fields(algo, lvl, size, thr):
    """the oracle's fields on one map: after the plan and, levels 1 and 2, after each of four replans -> [(what, raster, G, trusted mask)],
    computed once and shared (nobody writes into them)"""
    cost, start, goal = fr.recipe_map(SEED, *size)
    o = planner(algo, lvl, cost, thr, start, goal)
    out = [("plan", cost, o.g(), o.trusted_mask(below_start_key=True))]
    if lvl:
        for k, (patch, top, left, s, cur) in enumerate(patches(SEED, cost, thr)):
            o.patch_map(patch, top, left); o.set_start(*s)
            assert o.step() == 0
            out.append(("replan %d" % k, cur, o.g(), o.trusted_mask(below_start_key=True)))
    return out


def goal_of(size):
    return (size[0] - 1, size[1] - 1)


CASES = [(a, l, s, t) for a, l in PLANNERS for s in SIZES for t in THRESHOLDS]
IDS = ["%s-%d-%dx%d-thr%.1f" % (a, l, s[0], s[1], t) for a, l, s, t in CASES]


@pytest.mark.parametrize("algo,lvl,size,thr", CASES, ids=IDS)
def test_oracle_field_is_a_fixed_point(algo, lvl, size, thr):
    """every trusted value below the start's key, after the plan and after every replan, is the float64 operator's of its neighbours"""
    for what, cost, g, mask in fields(algo, lvl, size, thr):
        assert mask.any() or what != "plan", what      # (a patch may wall the goal in: nothing is trusted then)
        ck = fr.check(g, fr.rhs64(ALGOS[algo], cost, thr, g, goal_of(size)), bound_for(algo), mask)
        print("%s: worst %.3f ulp over %d, %d through the window" % (what, ck.worst, ck.n, ck.windowed))
        assert ck.off == 0, "%s: %d of %d trusted elements off their operator, worst %.1f ulp, first %r" % (what, ck.off, ck.n, ck.worst, ck.where)
        assert ck.share <= fr.WINDOW_SHARE, "%s: %d of %d elements lean on the comparison window" % (what, ck.windowed, ck.n)


def test_bounds_are_the_measurement():
    """the two constants are twice the oracle's worst residual over this file's maps, rounded up to a whole ulp -- measured here, on the
    oracle against float64, never on the engine"""
    worst = {"node": 0.0, "DFM": 0.0}
    for algo, lvl, size, thr in CASES:
        for what, cost, g, mask in fields(algo, lvl, size, thr):
            r = fr.residual_ulp(g, fr.rhs64(ALGOS[algo], cost, thr, g, goal_of(size)))[mask]
            k = "DFM" if algo == "DFM" else "node"
            worst[k] = max(worst[k], float(r.max()) if r.size else 0.0)
    print("worst residual of the oracle: node planners %.3f ulp, MS-DFM %.3f ulp" % (worst["node"], worst["DFM"]))
    assert NODE_BOUND == math.ceil(2 * worst["node"]) and DFM_BOUND == math.ceil(2 * worst["DFM"]), worst


def test_census():
    """every case of both node operators is evaluated by the oracle, and every case that can decide a value is the float64 minimum's on at
    least CENSUS_FLOOR trusted elements of this file's maps; MS-DFM: both stencils win in both forms"""
    orc.case_counts_reset()
    cost, start, goal = fr.recipe_map(SEED, 37, 43)
    for algo in ("FD", "SG"):
        planner(algo, 0, cost, 1.0, start, goal)
    evaluated, won = orc.case_counts()
    print("oracle, 37 x 43: evaluated %r\nwon %r" % (evaluated, won))
    assert all(evaluated[c] > 0 for c in orc.CASES), evaluated
    first, alone, dfm = np.zeros(11, int), np.zeros(11, int), np.zeros(4, int)
    for algo, lvl, size, thr in CASES:
        if lvl:
            continue
        (what, cost, g, mask), = fields(algo, lvl, size, thr)
        cen = fr.census(fr.rhs64(ALGOS[algo], cost, thr, g, goal_of(size)), mask)
        if algo == "DFM":
            dfm += [cen[k] for k in range(4)]
        else:
            first += [cen[k][0] for k in range(11)]; alone += [cen[k][1] for k in range(11)]
    print("float64 winners: %r\nalone: %r\nMS-DFM: %r" % (dict(zip(fr.CASE_NAMES, first)), dict(zip(fr.CASE_NAMES, alone)), dict(zip(fr.DFM_CASE_NAMES, dfm))))
    for k in fr.FD_CASES + fr.SG_CASES:
        if k not in fr.FD_CANNOT_DECIDE:
            assert first[k] >= CENSUS_FLOOR and alone[k] >= 1, (fr.CASE_NAMES[k], first[k], alone[k])
    assert (dfm >= CENSUS_FLOOR).all(), dfm


def test_type_iii_never_decides():
    """Field D*'s Type III (either clause) is never the only case at a minimum.  Its value g1 + b walks the edge s-p1 inside the cheaper cell
    b.  The triangle on the other side of that edge has the same p1 and c' = b < b' = c, so it takes the c <= b chain: B gives g1 + b, the
    same path; II gives g1 + sqrt(b^2 - f'^2) < g1 + b; A is taken only when f' sqrt 2 >= b and gives g2' + b sqrt 2 <= g1 + b / sqrt 2.
    So no field can tell Type III from its absence.  The oracle agrees: without the f^2 clause (ablation 1), and with a Type III that
    pays c instead of b (ablation 8), its fields are bit for bit the same."""
    L = orc.lib()
    for size in SIZES:
        for thr in THRESHOLDS:
            (what, cost, g, mask), = fields("FD", 0, size, thr)
            r = fr.rhs64(fr.FD, cost, thr, g, goal_of(size))
            for k in fr.FD_CANNOT_DECIDE:
                assert not (r.tied[mask] == (1 << k)).any(), (size, thr, fr.CASE_NAMES[k])
            assert not (r.tied[mask] == ((1 << fr.FD_III) | (1 << fr.FD_III_SQ))).any()
            for ablation in (1, 8):
                try:
                    L.orc_set_fd_ablation(ablation)
                    cost_, start, goal = fr.recipe_map(SEED, *size)
                    o = planner("FD", 0, cost_, thr, start, goal)
                finally:
                    L.orc_set_fd_ablation(0)
                assert np.array_equal(o.g(), g) and np.array_equal(o.trusted_mask(below_start_key=True), mask), (size, thr, ablation)


# ---- the checker catches real errors: each of these must FAIL the criterion of test_oracle_field_is_a_fixed_point ----

@pytest.mark.parametrize("ablation", [2, 4], ids=["no-type-I", "no-c>b-chain"])
def test_checker_catches_a_wrong_case_chain(ablation):
    """the oracle without Type I / without the c > b chain plans a field that is a fixed point of ITS operator, not of the geometry's"""
    cost, start, goal = fr.recipe_map(SEED, 37, 43)
    L = orc.lib()
    try:
        L.orc_set_fd_ablation(ablation)
        o = planner("FD", 0, cost, 1.0, start, goal)
    finally:
        L.orc_set_fd_ablation(0)
    g, mask = o.g(), o.trusted_mask(below_start_key=True)
    ck = fr.check(g, fr.rhs64(fr.FD, cost, 1.0, g, (36, 42)), NODE_BOUND, mask)
    print("ablation %d: %d of %d off, worst %.3g ulp" % (ablation, ck.off, ck.n, ck.worst))
    assert ck.off >= 10 and ck.worst > 100


@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
@pytest.mark.parametrize("ulps", [1, -1], ids=["raised", "lowered"])
def test_checker_catches_one_element(algo, ulps):
    """one trusted element moved by the bound + 2 ulp is reported, and it is the first offender"""
    (what, cost, g, mask), = fields(algo, 0, (37, 43), 1.0)
    bound = bound_for(algo)
    x, y = np.argwhere(mask & (g > 0))[len(np.argwhere(mask & (g > 0))) // 2]
    bad = g.copy()
    bad[x, y] = (bad[x:x + 1, y].view(np.int32) + ulps * (bound + 2)).view(np.float32)[0]
    mask = mask & np.isfinite(g)
    one = np.zeros_like(mask); one[x, y] = True
    ck = fr.check(bad, fr.rhs64(ALGOS[algo], cost, 1.0, bad, (36, 42)), bound, one)
    assert ck.off == 1 and ck.where == (x, y) and bound + 1 <= ck.worst <= bound + 3, ck
    assert fr.check(bad, fr.rhs64(ALGOS[algo], cost, 1.0, bad, (36, 42)), bound, mask).off >= 1


def test_checker_catches_a_missing_stencil():
    """MS-DFM's field iterated by this module WITHOUT the diagonal stencil is a fixed point of that operator and not of MS-DFM's"""
    cost, _, _ = fr.recipe_map(SEED, 37, 43)
    g = fr.fixed_point_dfm(cost, 1.0, (36, 42), diagonal=False)
    mask = np.isfinite(g)
    ck = fr.check(g, fr.rhs64(fr.DFM, cost, 1.0, g, (36, 42)), DFM_BOUND, mask)
    print("orthogonal stencil only: %d of %d off, worst %.3g ulp" % (ck.off, ck.n, ck.worst))
    assert ck.off >= 100
    assert fr.check(g, fr.rhs64(fr.DFM, cost, 1.0, g, (36, 42), diagonal=False), DFM_BOUND, mask).off == 0
    # ... while the iteration with both stencils is one, and agrees with the oracle's field within the parity bound
    g = fr.fixed_point_dfm(cost, 1.0, (36, 42))
    assert fr.check(g, fr.rhs64(fr.DFM, cost, 1.0, g, (36, 42)), DFM_BOUND).off == 0
    (what, _, og, omask), = fields("DFM", 0, (37, 43), 1.0)
    assert np.allclose(g[omask], og[omask], rtol=ufm_amd.tolerances.DFM_RTOL, atol=0)


# ---- geometric soundness: every case is the cost of a real path ----

@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("algo", ["FD", "SG"])
def test_rhs_is_never_below_the_cheapest_path(algo, thr):
    """the float64 operator's RHS against the brute-force minimum over (distance walked along the edge, crossing point), on every seventh
    node of the 37 x 43 field: never below it by more than the lattice's resolution (derived at field_reference.GRID_RESOLUTION).  How far
    ABOVE it the RHS lies is printed, not asserted: no bound has been derived for the reference's `f^2 <= sqrt(c^2 - b^2)` clause, which
    may take Type III where Type II or I would be cheaper (the minimum over the eight triangles then comes from the triangle across the
    edge).  Measured, FD and SG at both thresholds, 204 .. 237 nodes each: below by 7.3e-8 relative at most, above by 1.8e-16 at most
    -- on no node by more than 1e-6: the chains are the geometric minimum."""
    (what, cost, g, mask), = fields(algo, 0, (37, 43), thr)
    nodes = np.argwhere(np.ones_like(mask))[::7]
    assert len(nodes) >= 200
    rhs = fr.rhs64(ALGOS[algo], cost, thr, g, (36, 42)).value[nodes[:, 0], nodes[:, 1]]
    geo = fr.geometric_min(ALGOS[algo], cost, thr, g, nodes, goal=(36, 42))
    assert np.array_equal(np.isinf(rhs), np.isinf(geo))
    fin = np.isfinite(rhs) & (rhs > 0)
    rel = (rhs[fin] - geo[fin]) / geo[fin]
    print("%s thr %.1f: %d nodes, RHS below the lattice minimum by at most %.3g, above by at most %.3g; above by > 1e-6 on %.1f %%" % (
        algo, thr, int(fin.sum()), max(0.0, -rel.min()), max(0.0, rel.max()), 100.0 * (rel > 1e-6).mean()))
    assert fin.sum() >= 100
    assert (rhs[fin] >= geo[fin] * (1.0 - fr.GRID_RESOLUTION)).all(), "RHS below the cheapest path by %.3g relative" % -rel.min()
