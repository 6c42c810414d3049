"""-m gpu: the block replan kernel (k_replan_region, ufm_region.h) comes in three forms -- no heuristic term and no diagnostics / heuristic
term / everything -- of which the host picks one per launch (Engine::submit_block).  The form may not change a field: the cases below run the
kernel on the smallest maps on which it has an interior block and a clipped one (160 x 160 for FD level 1 and SG level 2, 192 x 192 for
MS-DFM level 1 following its stored bytes; 31 x 31 patches, at most 12 replans) against the oracle stepped alike, and the forms against each
other -- with the bursts that matter to a kernel that tells early which bursts are futile: patches with nothing finite in reach, the goal's
patch with +inf all around it, clipped blocks, a batch.  FD / SG: bit for bit below the start's key; MS-DFM: dfm_close at its bound."""
import functools

import numpy as np
import pytest

import ufm_amd
import oracle_py as orc
from helpers import ALGOS, make_pair, check_parity, dfm_close
from test_gpu_replan_tail import CASES, IDS, PATCH, workload, corner_script, pair

pytestmark = pytest.mark.gpu

NODE_CASES, NODE_IDS = CASES[:2], IDS[:2]


def check(algo, o, g, what):
    """the field against the oracle on what a planner honouring end_condition must have finalised, the byte self-check"""
    if algo == "DFM":
        m = o.trusted_mask(below_start_key=True)
        assert int(m.sum()) > 0, what
        assert dfm_close(g.read_field()[0][m], o.g()[m], what=what), "%s: differs from the oracle" % what
        assert g.check_layout() == (0, 0), what
    else:
        n, nbad = check_parity(o, g, what, below_start_key=True)
        assert nbad == 0, "%s: %d of %d trusted elements differ from the oracle" % (what, nbad, n)
    ci = g.check_info()
    assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)


def both_step(o, g, patch, top, left, s, hm=None):
    for p in (o, g):
        p.patch_map(patch, top, left)
        if hm is not None:
            p.set_heuristic_multiplier(hm)
        p.set_start(*s)
        assert p.step() == 0


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_back_to_back(algo, lvl, size):
    """12 replans, every one through the block kernel, then the field against the oracle"""
    o, g, goal = pair(algo, lvl, size)
    _, _, _, script = workload(size)
    r0 = g.stats.region_replans
    for k, s, top, left, patch in script:
        both_step(o, g, patch, top, left, s)
    assert g.stats.region_replans - r0 == len(script)
    check(algo, o, g, "%s after 12 replans" % algo)
    g.close()


def run_script(algo, lvl, size, region_debug, region_band=None):
    """the scripted replans on the device alone: the whole field and, per step, what a caller can count"""
    cost, start, goal, script = workload(size)
    g = ufm_amd.Planner(ALGOS[algo], lvl, False, follow_info=(algo == "DFM"))
    g.reset(); g.set_occupancy_threshold(1.0); g.set_heuristic_multiplier(1.0)
    g.set_map(cost); g.set_start(*start); g.set_goal(*goal)
    g.set_param("region_debug", region_debug)
    if region_band is not None:
        g.set_param("region_band", region_band)
    assert g.step() == 0
    r0, d0, counts = g.stats.region_replans, g.stats.region_replans_done, []
    for k, s, top, left, patch in script:
        g.patch_map(patch, top, left); g.set_start(*s)
        assert g.step() == 0
        counts.append((g.stats.region_replans_done - d0, g.num_nodes_updated, g.num_nodes_expanded))
    assert g.stats.region_replans - r0 == len(script)
    field = g.read_field()[0].copy()
    g.close()
    return field, counts


@functools.lru_cache(maxsize=None)
def finalised(algo, lvl, size):
    """what the oracle, stepped through the script, calls final below the start's key after the last step"""
    cost, start, goal, script = workload(size)
    o = orc.OraclePlanner(ALGOS[algo], lvl, False)
    o.reset(); o.set_occupancy_threshold(1.0); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
    assert o.step() == 0
    for k, s, top, left, patch in script:
        o.patch_map(patch, top, left); o.set_start(*s)
        assert o.step() == 0
    m = o.trusted_mask(below_start_key=True)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def lean_and_full(algo, lvl, size, region_band=None):
    """the same script through the lean form (region_debug 0) and through the full one (region_debug 2: diagnostics on, all gates as they are)"""
    return run_script(algo, lvl, size, 0, region_band), run_script(algo, lvl, size, 2, region_band)


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_lean_against_full(algo, lvl, size):
    """FD / SG: the whole field bit for bit -- beyond the start's key too --, and per step the same count of steps the block kernel finished,
    the same num_nodes_updated and num_nodes_expanded.  MS-DFM (its float fixed point is not unique, two runs of ONE form differ in the last
    places and with them the count of changed elements; its fields are compared where they are final, in the test below): the same
    num_nodes_updated.

    What this guards: beyond the start's key a result is applied or held back by the ordering band of the lowering sub-rounds, and the band
    must not depend on how the waves interleave -- the diagnostics' atomics and time stamps change that interleaving.  It once did: the key
    at which the next band starts was collected over all bursts of a sub-round, stale evaluations included (with the single-form kernel,
    region_debug 0 against 2: SG-2, 4 of 25 921 elements after replan 7, num_nodes_expanded 1347 against 1348; with the forms FD-1 up to 4
    elements between two runs of ONE form).  It is now taken from every patch's last burst (RegionShared::pkey)."""
    (lean, c_lean), (full, c_full) = lean_and_full(algo, lvl, size)
    if algo != "DFM":
        ndiff = int((lean.view(np.int32) != full.view(np.int32)).sum())
        print("%s: %d of %d elements differ between the lean and the full form; counts per step %r against %r" % (algo, ndiff, lean.size, c_lean, c_full))
        assert ndiff == 0, "%d elements differ between the lean and the full form" % ndiff
        assert c_lean == c_full
    else:
        assert [c[1] for c in c_lean] == [c[1] for c in c_full]


@pytest.mark.parametrize("algo,lvl,size", NODE_CASES, ids=NODE_IDS)
def test_lean_against_full_unordered(algo, lvl, size):
    """the whole-field comparison with the lowering sub-rounds unordered ("region_band" 0: one bound per sub-round, nothing that moves with the
    interleaving of the waves): the forms give the same field bit for bit, beyond the start's key too, and the same three counts per step"""
    (lean, c_lean), (full, c_full) = lean_and_full(algo, lvl, size, 0.0)
    assert np.array_equal(lean.view(np.int32), full.view(np.int32)), "%d elements differ between the lean and the full form" % int(
        (lean.view(np.int32) != full.view(np.int32)).sum())
    assert c_lean == c_full


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_lean_against_full_below_the_start_key(algo, lvl, size):
    """what the engine promises -- the elements final below the start's key -- is the same in the lean and in the full form: FD / SG bit for
    bit, MS-DFM within its bound; the block kernel finished the same steps and counted the same num_nodes_updated"""
    (lean, c_lean), (full, c_full) = lean_and_full(algo, lvl, size)
    m = finalised(algo, lvl, size)
    assert int(m.sum()) > 1000
    if algo != "DFM":
        assert np.array_equal(lean[m].view(np.int32), full[m].view(np.int32))
    else:
        assert dfm_close(lean[m], full[m], what="lean against full")
    assert [c[:2] for c in c_lean] == [c[:2] for c in c_full]


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_heuristic_form(algo, lvl, size):
    """heuristic keys with the multiplier at the map's smallest cost (the reference harness's choice): the form with the heuristic term"""
    cost, start, goal, script = workload(size)
    hm = float(cost.min())
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, heuristic=True, hm=hm)
    if algo == "DFM":
        g.set_param("dfm_follow_info", 1)
    assert o.step() == 0 and g.step() == 0
    r0 = g.stats.region_replans
    for k, s, top, left, patch in script:
        both_step(o, g, patch, top, left, s, hm=hm)
        if k % 4 == 0:
            check(algo, o, g, "%s heuristic replan %d" % (algo, k))
    assert g.stats.region_replans - r0 == len(script)
    g.close()


@pytest.mark.parametrize("algo,lvl,size", NODE_CASES, ids=NODE_IDS)
def test_heuristic_keys_with_multiplier_zero(algo, lvl, size):
    """a planner built with heuristic keys whose multiplier is 0 has no heuristic term: the host gives it the lean form (the form follows
    the multiplier, not how the planner was built), and its field is the one of the planner built without heuristic keys -- bit for bit on
    what that planner's oracle calls final below the start's key -- and its own oracle's"""
    cost, start, goal, script = workload(size)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, heuristic=True, hm=0.0)
    ou, gu = make_pair(ALGOS[algo], lvl, cost, start, goal)
    for p in (o, g, ou, gu):
        assert p.step() == 0
    r0 = g.stats.region_replans
    for k, s, top, left, patch in script[:6]:
        both_step(o, g, patch, top, left, s, hm=0.0)
        both_step(ou, gu, patch, top, left, s)
    assert g.stats.region_replans - r0 == 6
    check(algo, o, g, "%s multiplier 0" % algo)
    m = ou.trusted_mask(below_start_key=True)
    assert int(m.sum()) > 1000
    assert np.array_equal(g.read_field()[0][m], gu.read_field()[0][m])
    g.close(); gu.close()


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_nothing_finite_around(algo, lvl, size):
    """a ring of obstacles walls the start in: what the invalidation takes away inside stays +inf, the lowering bursts there find nothing
    finite in reach and leave at once.  The next patch opens the ring: the patches that left early are swept when a finite neighbour arrives."""
    cost, _, goal, _ = workload(size)
    start = (72.0, 75.0)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    if algo == "DFM":
        g.set_param("dfm_follow_info", 1)
    assert o.step() == 0 and g.step() == 0
    top, left = 57, 60
    open_ = np.clip(cost[top:top + PATCH, left:left + PATCH], 1, 200)     # (no obstacle block of the map inside the ring)
    wall = open_.copy(); wall[:2, :] = wall[-2:, :] = 255; wall[:, :2] = wall[:, -2:] = 255
    r0 = g.stats.region_replans
    both_step(o, g, wall, top, left, start)
    assert not np.isfinite(o.start_key())
    gg, og = g.read_field()[0], o.g()
    assert np.isinf(gg[top + 3:top + PATCH - 3, left + 3:left + PATCH - 3]).all() and np.isinf(og[top + 3:top + PATCH - 3, left + 3:left + PATCH - 3]).all()
    check(algo, o, g, "%s walled in" % algo)
    both_step(o, g, open_, top, left, start)
    assert np.isfinite(o.start_key())
    assert np.isfinite(g.read_field()[0][top + 3:top + PATCH - 3, left + 3:left + PATCH - 3]).all()
    check(algo, o, g, "%s opened again" % algo)
    assert g.stats.region_replans - r0 == 2
    g.close()


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_goal_inside_the_block(algo, lvl, size):
    """start and patch next to the goal, the patch's costs at their highest: the invalidation takes away everything around the goal, whose
    patch is then swept with +inf all around it -- RHS(goal) = 0 must survive and the field be rebuilt from it"""
    cost, _, goal, _ = workload(size)
    gx, gy = int(goal[0]), int(goal[1])
    start = (float(gx - 14), float(gy - 12))
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    if algo == "DFM":
        g.set_param("dfm_follow_info", 1)
    assert o.step() == 0 and g.step() == 0
    top = left = size - PATCH
    r0 = g.stats.region_replans
    for i, fill in enumerate((200, 3)):
        both_step(o, g, np.full((PATCH, PATCH), fill, np.uint8), top, left, start)
        assert g.read_field()[0][gx, gy] == 0.0 and o.g()[gx, gy] == 0.0
        check(algo, o, g, "%s patch %d over the goal" % (algo, i))
    assert g.stats.region_replans - r0 == 2
    g.close()


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_clipped_blocks(algo, lvl, size):
    """the patches in three corners of the map in turn: every block is clipped on two sides"""
    o, g, goal = pair(algo, lvl, size)
    r0 = g.stats.region_replans
    for k, s, top, left, patch in corner_script(size):
        both_step(o, g, patch, top, left, s)
        check(algo, o, g, "%s corner patch %d" % (algo, k))
    assert g.stats.region_replans - r0 == 6
    g.close()


@pytest.mark.parametrize("algo,lvl,follow", [("FD", 1, False), ("SG", 2, False), ("DFM", 1, False), ("DFM", 1, True)], ids=["FD-1", "SG-2", "DFM-1", "DFM-1-info"])
def test_batch_round(algo, lvl, follow):
    """one round of a batch of two maps, a patch per map: one launch, a workgroup per map -- for all four operator ids of the kernel"""
    n, size = 2, 192 if algo == "DFM" else 160
    b = ufm_amd.BatchPlanner(n, ALGOS[algo], lvl, follow_info=follow)
    b.set_occupancy_threshold(1.0)
    oracles = []
    for m in range(n):
        cost, start, goal, script = workload(size, 1000 + m)
        b.set_map(m, cost); b.set_start(m, *start); b.set_goal(m, *goal)
        o = orc.OraclePlanner(ALGOS[algo], lvl, False)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        oracles.append((o, script[0]))
    assert b.step() == 0
    r0 = b.stats.region_replans
    for m, (o, (k, s, top, left, patch)) in enumerate(oracles):
        b.patch_map(m, patch, top, left); b.set_start(m, *s)
        o.patch_map(patch, top, left); o.set_start(*s)
        assert o.step() == 0
    assert b.step() == 0
    assert b.stats.region_replans - r0 == n
    if algo != "DFM" or follow:         # (MS-DFM's bytes are promised where its invalidation follows them)
        ci = b.check_info()
        assert ci[1:4] == (0, 0, 0), "back-pointer self-check %r" % (ci,)
    for m, (o, _) in enumerate(oracles):
        mask = o.trusted_mask(below_start_key=True)
        assert int(mask.sum()) > 1000
        got, want = b.read_field(m)[mask], o.g()[mask]
        if algo == "DFM":
            assert dfm_close(got, want, what="batch"), "map %d differs from its oracle" % m
        else:
            assert np.array_equal(got, want), "map %d: %d elements differ from its oracle" % (m, int((got != want).sum()))
    assert b.check_layout() == (0, 0)
    b.close()
