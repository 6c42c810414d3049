"""-m gpu: the engine's fields against the float64 operators of tests/field_reference.py -- a reference that shares nothing with the oracle.

The criterion is local: each value G(s) the device holds is, within a few ulp, what the operator makes of the neighbours of s in the
device's own field.  With "focused" = 0 every element is final, so EVERY element is checked, with no oracle mask: finite values against
the operator, +inf elements against an operator that gives +inf (no neighbour offers them a value), the goal 0, RHS == G.  That covers
what the parity tests leave out -- the elements beyond the oracle's trusted set, the ones a replan's invalidation left behind, the
unreached ones -- and it holds MS-DFM to ulps where its parity bound (a relative 1e-6 / 2e-6 of a non-unique fixed point) leaves 10 to
30 ulp of slack at every element.

BOUNDS.  FD / SG: tolerances.NODE_LOCAL_ULP, the oracle's own measured residual doubled (tests/test_field_reference.py) -- their fields
are bit-equal to the oracle's.  MS-DFM: tolerances.DFM_LOCAL_ULP plus the 8 ulp the engine documents for values its lowering leaves off
their operator (include/ufm.h at ufm_check_info, csrc/ufm_control.h at k_check_bp): a number of the project's, not one measured on the
code under test.  The worst residual each MS-DFM test saw goes to the margins table (helpers.note_margin, in ulp / 2^23 and bound / 2^23).
The comparison window may excuse at most field_reference.WINDOW_SHARE of a test's elements."""
import numpy as np
import pytest

import ufm_amd
import field_reference as fr
from helpers import ALGOS, make_pair, note_margin
from test_gpu_replan_tail import workload

pytestmark = pytest.mark.gpu

SEED = 5
SIZES = [(37, 43), (17, 17), (1, 40)]
THRESHOLDS = [1.0, 0.6]
PLANNERS = [("FD", 0), ("FD", 1), ("SG", 0), ("SG", 1), ("SG", 2), ("DFM", 0), ("DFM", 1)]
ENGINE_DFM_SLACK_ULP = 8                      # include/ufm.h, ufm_check_info
NODE_BOUND = ufm_amd.tolerances.NODE_LOCAL_ULP
DFM_BOUND = ufm_amd.tolerances.DFM_LOCAL_ULP + ENGINE_DFM_SLACK_ULP
CENSUS_FLOOR = 5


def bound_for(algo):
    return DFM_BOUND if algo == "DFM" else NODE_BOUND


def device_planner(algo, lvl, cost, start, goal, thr=1.0, heuristic=False, **params):
    g = ufm_amd.Planner(ALGOS[algo], lvl, heuristic)
    g.reset(); g.set_occupancy_threshold(thr); g.set_heuristic_multiplier(1.0)
    for name, v in params.items():
        g.set_param(name, v)
    g.set_map(cost); g.set_start(*start); g.set_goal(*goal)
    return g


def free_cell(rng, cur, thr=1.0):
    """a random traversable cell of the raster, as a start position"""
    free = np.argwhere(cur < fr.threshold_byte(thr))
    a = free[rng.integers(len(free))]
    return float(a[0]), float(a[1])


def goal_elem(goal):
    return (int(round(goal[0])), int(round(goal[1])))


def check_elements(algo, cost, thr, g, rhs, goal, what, mask=None, tally=None):
    """the local criterion on the device's field `g` (RHS view `rhs`); mask None: every element, unreached ones and the goal included.
    -> (field_reference.Check, the float64 operator's result); tally: [elements, needed the window] summed over a test"""
    assert np.array_equal(g, rhs), "%s: RHS != G on %d elements" % (what, int((g != rhs).sum()))
    gx, gy = goal_elem(goal)
    r = fr.rhs64(ALGOS[algo], cost, thr, g, (gx, gy))
    bound = bound_for(algo)
    if mask is None:
        assert g[gx, gy] == 0.0, "%s: the goal holds %r" % (what, float(g[gx, gy]))
        unreached = np.isinf(g)
        assert np.isinf(r.value[unreached]).all(), "%s: %d elements hold no value although their neighbours give them one, first %r" % (
            what, int(np.isfinite(r.value[unreached]).sum()), tuple(np.argwhere(unreached & np.isfinite(r.value))[0]))
    ck = fr.check(g, r, bound, mask)
    print("%s: worst %.3f ulp over %d elements (%d finite), %d through the window" % (
        what, ck.worst, ck.n, int(np.isfinite(g[mask] if mask is not None else g).sum()), ck.windowed))
    if algo == "DFM":
        note_margin(what, ck.worst * 2.0 ** -23, int(np.ceil(ck.worst)) if np.isfinite(ck.worst) else 0, bound * 2.0 ** -23, ck.off, ck.n)
    assert ck.off == 0, "%s: %d of %d elements off their operator by more than %d ulp, worst %.1f, first %r" % (
        what, ck.off, ck.n, bound, ck.worst, ck.where)
    if tally is not None:
        tally[0] += ck.n; tally[1] += ck.windowed
    return ck, r


def window_share_ok(tally, what):
    assert tally[1] <= fr.WINDOW_SHARE * tally[0], "%s: %d of %d elements lean on the comparison window" % (what, tally[1], tally[0])


@pytest.mark.parametrize("owned", [1, 0], ids=["resident", "launch-chain"])
@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=["%s-%d" % p for p in PLANNERS])
def test_whole_field(algo, lvl, owned):
    """fresh plans with "focused" = 0 on the 37 x 43, 17 x 17 and 1 x 40 maps at thresholds 1.0 and 0.6, through the resident kernel and through
    the launch chain: every element against the float64 operator on the device's own field, and the census floors of
    tests/test_field_reference.py on the float64 winners of these fields"""
    tally, worst_fresh = [0, 0], 0.0
    first, alone, dfm = np.zeros(11, int), np.zeros(11, int), np.zeros(4, int)
    for size in SIZES:
        for thr in THRESHOLDS:
            cost, start, goal = fr.recipe_map(SEED, *size)
            p = device_planner(algo, lvl, cost, start, goal, thr, focused=0, owned=owned)
            assert p.step() == 0
            assert p.stats.resident_launches == (1 if owned else 0)
            g, rhs = p.read_field()
            ck, r = check_elements(algo, cost, thr, g, rhs, goal, "%dx%d thr %.1f" % (size + (thr,)), tally=tally)
            worst_fresh = max(worst_fresh, ck.worst)
            cen = fr.census(r)
            if algo == "DFM":
                dfm += [cen[k] for k in range(4)]
            else:
                first += [cen[k][0] for k in range(11)]; alone += [cen[k][1] for k in range(11)]
                for k in fr.FD_CANNOT_DECIDE:
                    assert cen[k][1] == 0
            p.close()
    window_share_ok(tally, "fresh plans")
    print("%s-%d: worst residual of the fresh plans %.3f ulp; winners %r alone %r MS-DFM %r" % (algo, lvl, worst_fresh, first.tolist(), alone.tolist(), dfm.tolist()))
    if algo == "DFM":
        assert (dfm >= CENSUS_FLOOR).all(), dict(zip(fr.DFM_CASE_NAMES, dfm))
    else:
        for k in (fr.FD_CASES if algo == "FD" else fr.SG_CASES):
            if k not in fr.FD_CANNOT_DECIDE:
                assert first[k] >= CENSUS_FLOOR and alone[k] >= 1, (fr.CASE_NAMES[k], first[k], alone[k])


REPLANS = [("FD", 1, 160, {}), ("SG", 2, 160, {}), ("DFM", 1, 192, {"dfm_follow_info": 0}), ("DFM", 1, 192, {"dfm_follow_info": 1})]


@pytest.mark.parametrize("region", [1, 0], ids=["block-kernel", "launch-chain"])
@pytest.mark.parametrize("algo,lvl,size,params", REPLANS, ids=["FD-1", "SG-2", "DFM-1", "DFM-1-follow"])
def test_replans_whole_field(algo, lvl, size, params, region):
    """the workload of tests/test_gpu_replan_tail.py (12 patches of 31 x 31, five cells apart, with a moving start) with "focused" = 0, through
    the block kernel and through the launch chain: the whole field after the plan and after every step -- the elements the invalidation left
    behind and the ones it cut off from the goal included"""
    cost, start, goal, script = workload(size)
    p = device_planner(algo, lvl, cost, start, goal, focused=0, region=region, **params)
    assert p.step() == 0
    cur, tally = cost.copy(), [0, 0]
    check_elements(algo, cur, 1.0, *p.read_field(), goal, "plan", tally=tally)
    r0 = p.stats.region_replans
    for k, s, top, left, patch in script:
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
        cur[top:top + patch.shape[0], left:left + patch.shape[1]] = patch
        check_elements(algo, cur, 1.0, *p.read_field(), goal, "replan %d" % k, tally=tally)
    window_share_ok(tally, "replans")
    assert p.stats.region_replans - r0 == (len(script) if region else 0)      # every step went through the block kernel / none did
    assert np.array_equal(p.read_map(size, size), cur)
    p.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)], ids=["FD-1", "SG-2", "DFM-1"])
def test_focused_below_the_start_key(algo, lvl):
    """the default, focused search on the 37 x 43 map: the elements the oracle trusts below the start's key"""
    cost, start, goal = fr.recipe_map(SEED, 37, 43)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    mask = o.trusted_mask(below_start_key=True)
    assert mask.sum() > 1000
    tally = [0, 0]
    check_elements(algo, cost, 1.0, *g.read_field(), goal, "focused", mask=mask, tally=tally)
    window_share_ok(tally, "focused")
    g.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 1)], ids=["FD-1", "SG-1"])
def test_heuristic_keys(algo, lvl):
    """heuristic keys (multiplier 1 = the map's cheapest cell): the corridor the oracle trusts below the start's key"""
    cost, start, goal = fr.recipe_map(SEED, 37, 43)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, heuristic=True, hm=1.0)
    assert o.step() == 0 and g.step() == 0
    mask = o.trusted_mask(below_start_key=True)
    assert mask.sum() > 100
    tally = [0, 0]
    check_elements(algo, cost, 1.0, *g.read_field(), goal, "heuristic keys", mask=mask, tally=tally)
    window_share_ok(tally, "heuristic keys")
    g.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)], ids=["FD-1", "SG-2", "DFM-1"])
def test_batch_of_two_maps(algo, lvl):
    """two 37 x 43 maps (seeds 5 and 6) in one BatchPlanner with "focused" = 0, a plan and two rounds of patches: every element of both fields"""
    b = ufm_amd.BatchPlanner(2, ALGOS[algo], lvl)
    b.set_occupancy_threshold(1.0)
    b.set_param("focused", 0)
    maps = []
    for m, seed in enumerate((SEED, SEED + 1)):
        cost, start, goal = fr.recipe_map(seed, 37, 43)
        b.set_map(m, cost); b.set_start(m, *start); b.set_goal(m, *goal)
        maps.append([cost.copy(), goal, np.random.default_rng(seed)])
    assert b.step() == 0
    tally = [0, 0]
    for rnd in range(3):
        for m, (cur, goal, rng) in enumerate(maps):
            g = b.read_field(m)
            check_elements(algo, cur, 1.0, g, g, goal, "map %d round %d" % (m, rnd), tally=tally)
            top, left = int(rng.integers(0, 37 - 9)), int(rng.integers(0, 43 - 11))
            patch = rng.integers(1, 255, (9, 11), dtype=np.uint8)
            patch[rng.random((9, 11)) < 0.15] = 255
            cur[top:top + 9, left:left + 11] = patch
            b.patch_map(m, patch, top, left); b.set_start(m, *free_cell(rng, cur))
        assert b.step() == 0
    for m, (cur, goal, rng) in enumerate(maps):
        g = b.read_field(m)
        check_elements(algo, cur, 1.0, g, g, goal, "map %d at the end" % m, tally=tally)
    window_share_ok(tally, "batch")
    assert b.check_layout() == (0, 0)
    b.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 1), ("SG", 2)], ids=["FD-1", "SG-1", "SG-2"])
def test_stored_parents(algo, lvl):
    """ufm_check_info's claim in arithmetic that is not the engine's: for every element that holds a value, the triangle its stored
    back-pointer names -- the node b and b's counter-clockwise neighbour -- gives that value in float64, within the bound; after a plan and
    after each of four random patches ("focused" = 0: every element final)"""
    cost, start, goal = fr.recipe_map(SEED, 37, 43)
    p = device_planner(algo, lvl, cost, start, goal, focused=0)
    assert p.step() == 0
    rng = np.random.default_rng(SEED)
    cur, checked, windowed = cost.copy(), 0, 0
    for k in range(5):
        g, _ = p.read_field()
        info = p.read_info()[..., 0]
        has = np.isfinite(g)
        has[goal_elem(goal)] = False
        assert (info[has] >= 0).all(), "step %d: %d elements with a value and no back-pointer" % (k, int((info[has] < 0).sum()))
        x, y = np.nonzero(has)
        bx, by = info[has] // g.shape[1], info[has] % g.shape[1]
        assert (np.maximum(np.abs(bx - x), np.abs(by - y)) == 1).all(), "step %d: a back-pointer names a node that is no neighbour" % k
        v, lo, hi, case = fr.via64(ALGOS[algo], cur, 1.0, g, x, y, bx, by)
        own = np.full(g.shape, np.inf)
        lo_f, hi_f = own.copy(), own.copy()
        own[has], lo_f[has], hi_f[has] = v, lo, hi
        ck = fr.check(g, fr.Rhs(own, lo_f, hi_f, None, None, None, None), NODE_BOUND, has)
        print("step %d: %d parents, worst %.3f ulp, %d through the window" % (k, ck.n, ck.worst, ck.windowed))
        assert ck.off == 0, "step %d: the stored parent of %d of %d elements does not give their value, worst %.1f ulp, first %r" % (
            k, ck.off, ck.n, ck.worst, ck.where)
        checked += ck.n; windowed += ck.windowed
        if k < 4:
            ph, pw = int(rng.integers(3, 20)), int(rng.integers(3, 20))
            top, left = int(rng.integers(0, 37 - ph + 1)), int(rng.integers(0, 43 - pw + 1))
            patch = rng.integers(1, 255, (ph, pw), dtype=np.uint8)
            patch[rng.random((ph, pw)) < 0.15] = 255
            cur[top:top + ph, left:left + pw] = patch
            p.patch_map(patch, top, left); p.set_start(*free_cell(rng, cur))
            assert p.step() == 0
    window_share_ok([checked, windowed], "stored parents")
    assert checked > 5000
    p.close()
