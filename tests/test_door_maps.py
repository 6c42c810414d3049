"""The premises of tests/test_gpu_doors.py, held on the oracle alone (CPU only).

The door maps (tests/door_maps.py) exist to make a replan a structural event: a door closes and most of the field rises or goes to +inf, a
door opens and most of it falls -- more elements than the block replan kernel holds, so that the wave leaves the block through its
border.  Whether the recipe does that is measured here on the oracle, never on the engine: the oracle is stepped through the scenario and

  * its trusted values are, after the plan and after every step, the float64 operator's of their neighbours on the current raster
    (the bounds and the window share of tests/test_field_reference.py, unchanged);
  * steps 1 - 3 each change more elements than the block holds; after step 2 more than half the field is +inf and the start's key is
    +inf; after step 4 the field is the plan's again, bit for bit;
  * the local criterion notices what the GPU tests are there to find: a field the replan did not touch, ONE element the invalidation
    missed (left at its old, lower value), one cut-off element left finite.

MEASURED (oracle; FD-1 and SG-2 give the same counts on this map): elements changed by steps 1 .. 8 -- 160 x 160, block 9 216: 19 409,
14 347, 18 737, 672, 744, 5 949, 4 044, 17 181; MS-DFM 192 x 192, block 16 384: 21 823, 19 778, 26 502, 4 957, 123, 9 137, 4 225, 17 393.
+inf after step 2: 19 803 of 25 921 / 28 224 of 36 864.  Worst residual 0.651 ulp (node planners) and 1.084 ulp (MS-DFM); no element
needed the comparison window."""
import functools

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
import field_reference as fr
import door_maps as dm
from helpers import ALGOS
from test_gpu_field_reference import check_elements

PLANNERS = [("FD", 1), ("SG", 2), ("DFM", 1)]
IDS = ["FD-1", "SG-2", "DFM-1"]
NODE_BOUND = ufm_amd.tolerances.NODE_LOCAL_ULP
DFM_BOUND = ufm_amd.tolerances.DFM_LOCAL_ULP


def bound_for(algo):
    return DFM_BOUND if algo == "DFM" else NODE_BOUND


def goal_elem(goal):
    return (int(round(goal[0])), int(round(goal[1])))


@functools.lru_cache(maxsize=None)
def fields(algo, lvl):
    """the oracle stepped through the scenario -> [(what, raster, G, trusted mask below the start's key, the start's key)], the plan
    first; computed once and shared (nobody writes into them)"""
    size = dm.SIZES[algo]
    cost, start, goal = dm.comb(dm.SEED, size)
    o = orc.OraclePlanner(ALGOS[algo], lvl, False)
    o.reset(); o.set_occupancy_threshold(dm.THRESHOLD); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
    assert o.step() == 0
    cur = cost.copy()
    out = [("plan", cost, o.g(), o.trusted_mask(below_start_key=True), o.start_key())]
    for name, patch, top, left, s in dm.scenario(size):
        o.patch_map(patch, top, left); o.set_start(*s)
        assert o.step() == 0
        dm.apply(cur, patch, top, left)
        out.append((name, cur.copy(), o.g(), o.trusted_mask(below_start_key=True), o.start_key()))
    for rec in out:
        for a in rec[1:4]:
            a.setflags(write=False)
    return out


def changed(algo, lvl, k):
    """elements whose value scenario step k (0-based) changed"""
    f = fields(algo, lvl)
    return int((f[k + 1][2].view(np.int32) != f[k][2].view(np.int32)).sum())


def test_the_recipe():
    """the map is what door_maps says: three walls of three columns, two doors of seven rows each, free cells everywhere else; every
    patch of the scenario is 9 x 5, changes the raster, and step 4 gives comb()'s raster back"""
    for size in (160, 192):
        cost, start, goal = dm.comb(dm.SEED, size)
        lethal = cost == 255
        cols = np.flatnonzero(lethal.any(axis=0))
        assert cols.tolist() == [w + k for w in dm.walls(size) for k in range(dm.WALL_W)]
        for w in dm.walls(size):
            rows = np.flatnonzero(~lethal[:, w])
            assert rows.tolist() == [r + k for r in dm.door_rows(size) for k in range(dm.DOOR_H)]
            assert (lethal[:, w] == lethal[:, w + 1]).all() and (lethal[:, w] == lethal[:, w + 2]).all()
        assert start == (8.0, 8.0) and goal == (size - 8.0, size - 8.0)
        cur = cost.copy()
        for k, (name, patch, top, left, s) in enumerate(dm.scenario(size) + dm.filler(size)):
            assert patch.shape == (dm.PATCH_H, dm.PATCH_W)
            before = cur.copy()
            dm.apply(cur, patch, top, left)
            assert (cur != before).any(), name
            assert cur[int(s[0]), int(s[1])] < 255
            if k == dm.RESTORED:
                assert np.array_equal(cur, cost)
        assert dm.scenario(size)[dm.WALLED_OFF][4] == (30.0, 8.0)


@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=IDS)
def test_oracle_fields(algo, lvl):
    """after the plan and after every step the oracle's trusted values lie within NODE_LOCAL_ULP / DFM_LOCAL_ULP of the float64 operator on
    the current raster, and the comparison window excuses at most WINDOW_SHARE of them"""
    goal = goal_elem(dm.comb(dm.SEED, dm.SIZES[algo])[2])
    n = windowed = 0
    for what, cost, g, mask, skey in fields(algo, lvl):
        assert mask.sum() > 1000, what
        ck = fr.check(g, fr.rhs64(ALGOS[algo], cost, dm.THRESHOLD, g, goal), bound_for(algo), mask)
        print("%s: worst %.3f ulp over %d, %d through the window" % (what, ck.worst, ck.n, ck.windowed))
        assert ck.off == 0, "%s: %d of %d trusted elements off their operator, worst %.1f ulp, first %r" % (what, ck.off, ck.n, ck.worst, ck.where)
        assert ck.share <= fr.WINDOW_SHARE, "%s: %d of %d elements lean on the comparison window" % (what, ck.windowed, ck.n)
        n += ck.n; windowed += ck.windowed
    assert windowed <= fr.WINDOW_SHARE * n


@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=IDS)
def test_conditions(algo, lvl):
    """what makes these replans structural, on the oracle: the wave of steps 1 - 3 cannot fit the block; step 2 cuts the start off;
    step 4 restores the plan's field"""
    f = fields(algo, lvl)
    counts = [changed(algo, lvl, k) for k in range(len(dm.STEPS))]
    print("%s-%d: changed per step %r, the block holds %d" % (algo, lvl, counts, dm.BLOCK[algo]))
    for k in dm.LARGE:
        assert counts[k] > dm.BLOCK[algo], "%s changes %d elements, the block holds %d" % (dm.STEPS[k][0], counts[k], dm.BLOCK[algo])
    what, cost, g, mask, skey = f[dm.CUT_OFF + 1]
    assert np.isinf(g).sum() > g.size // 2, "%s: %d of %d elements are +inf" % (what, int(np.isinf(g).sum()), g.size)
    assert np.isinf(skey), what
    # ... everything with a wall between it and the goal is +inf, everything beyond the goal-side wall that is no wall keeps a value
    wall = dm.walls(g.shape[0] - (algo != "DFM"))[dm.GOAL_SIDE]
    assert np.isinf(g[:, :wall]).all() and np.isfinite(g[:, wall + dm.WALL_W + 1:]).all()
    assert np.isinf(f[dm.WALLED_OFF + 1][4]), f[dm.WALLED_OFF + 1][0]
    plan, back = f[0], f[dm.RESTORED + 1]
    assert np.array_equal(plan[1], back[1])
    assert np.array_equal(plan[3], back[3]), "the trusted set after step 4 is not the plan's"
    if algo == "DFM":
        assert np.array_equal(np.isfinite(plan[2]), np.isfinite(back[2]))
        m = np.isfinite(plan[2])
        assert np.allclose(back[2][m], plan[2][m], rtol=ufm_amd.tolerances.DFM_RTOL, atol=0)
    else:
        assert dm.same_bits(plan[2][plan[3]], back[2][back[3]])
    # the start's key is finite wherever the start has a way to the goal
    for k, (what, cost, g, mask, skey) in enumerate(f):
        assert np.isinf(skey) == (k - 1 in (dm.CUT_OFF, dm.WALLED_OFF)), what


# ---- the checker notices what the GPU tests are for ----

def door_reach(shape, patch_at, reach=2):
    """the elements within `reach` of a door patch's rectangle"""
    top, left = patch_at
    m = np.zeros(shape, bool)
    m[max(top - reach, 0):top + dm.PATCH_H + reach + 1, max(left - reach, 0):left + dm.PATCH_W + reach + 1] = True
    return m


@pytest.mark.parametrize("k", [0, 1], ids=["step-1", "step-2"])
@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=IDS)
def test_checker_catches_a_field_no_replan_touched(algo, lvl, k):
    """the field of the step before, held against the raster after a door closed.  It is wrong at thousands of elements -- every element
    the step changes, more than the block holds.  The criterion is local: it reports the stale field where an element's operator reads a
    cell of the door, at the door's rim and nowhere else.  (Which is why the GPU tests check EVERY element after every step: of a field
    left wholly stale only some dozens of elements say so.)"""
    f = fields(algo, lvl)
    stale, (what, cost, g, mask, skey) = f[k][2], f[k + 1]
    goal = goal_elem(dm.comb(dm.SEED, dm.SIZES[algo])[2])
    wrong = int((stale.view(np.int32) != g.view(np.int32)).sum())
    assert wrong > dm.BLOCK[algo] and wrong >= 2000
    every = np.isfinite(stale)
    ck = fr.check(stale, fr.rhs64(ALGOS[algo], cost, dm.THRESHOLD, stale, goal), bound_for(algo), every)
    res = fr.residual_ulp(stale, fr.rhs64(ALGOS[algo], cost, dm.THRESHOLD, stale, goal))
    off = every & ~(res <= bound_for(algo))
    print("%s: the stale field is wrong at %d elements; the criterion reports %d, worst %.3g ulp" % (what, wrong, ck.off, ck.worst))
    assert ck.off >= dm.DOOR_H and ck.worst > 1000
    name, patch, top, left, s = dm.scenario(dm.SIZES[algo])[k]
    assert not (off & ~door_reach(stale.shape, (top, left))).any()


@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=IDS)
def test_checker_catches_one_missed_descendant(algo, lvl):
    """the correct field after step 1 with ONE element upstream of the closed door put back to the value it had before -- lower: what an
    invalidation leaves that misses a descendant.  The element is reported, and through the whole-field check as well."""
    f = fields(algo, lvl)
    old, (what, cost, g, mask, skey) = f[0][2], f[1]
    goal = goal_elem(dm.comb(dm.SEED, dm.SIZES[algo])[2])
    size = dm.SIZES[algo]
    rose = mask & f[0][3] & (old < g)
    rose[:, dm.walls(size)[dm.START_SIDE]:] = False          # far upstream: on the start's side of all three walls
    assert rose.sum() > 1000
    x, y = (int(v) for v in np.argwhere(rose)[len(np.argwhere(rose)) // 2])
    bad = g.copy()
    bad[x, y] = old[x, y]
    r = fr.rhs64(ALGOS[algo], cost, dm.THRESHOLD, bad, goal)
    one = np.zeros(g.shape, bool); one[x, y] = True
    ck = fr.check(bad, r, bound_for(algo), one)
    print("%s: element %r at its old value %r instead of %r: %.3g ulp off" % (what, (x, y), float(old[x, y]), float(g[x, y]), ck.worst))
    assert ck.off == 1 and ck.where == (x, y) and ck.worst > bound_for(algo)
    assert fr.check(bad, r, bound_for(algo), mask).off >= 1
    assert fr.check(g, fr.rhs64(ALGOS[algo], cost, dm.THRESHOLD, g, goal), bound_for(algo), mask).off == 0


@pytest.mark.parametrize("algo,lvl", PLANNERS, ids=IDS)
def test_checker_catches_one_element_left_finite(algo, lvl):
    """after step 2 the start's key is +inf: the oracle empties its queue, every element is final and the whole field passes
    check_elements -- unreached elements, the goal and all.  With one cut-off element left at its old value the check's "+inf where the
    operator gives +inf" assertion reports the neighbours that element would give a value to"""
    f = fields(algo, lvl)
    old, (what, cost, g, mask, skey) = f[1][2], f[dm.CUT_OFF + 1]
    goal = dm.comb(dm.SEED, dm.SIZES[algo])[2]
    check_elements(algo, cost, dm.THRESHOLD, g, g, goal, what)
    cut = np.isinf(g) & np.isfinite(old)
    cut[:, dm.walls(dm.SIZES[algo])[dm.MIDDLE]:] = False
    cut[:, :dm.walls(dm.SIZES[algo])[dm.START_SIDE] + dm.WALL_W + 2] = False         # between the start-side wall and the middle one
    cut[:5] = False; cut[-5:] = False
    x, y = np.argwhere(cut)[len(np.argwhere(cut)) // 2]
    bad = g.copy()
    bad[x, y] = old[x, y]
    with pytest.raises(AssertionError, match="hold no value although their neighbours give them one"):
        check_elements(algo, cost, dm.THRESHOLD, bad, bad, goal, what + ", one element left finite")
