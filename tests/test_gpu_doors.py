"""-m gpu: replans that are structural events -- a door closes and most of the field rises or goes to +inf, a door opens and most of it
falls -- on the maps of tests/door_maps.py (160 x 160 for FD level 1 and SG level 2, 192 x 192 for MS-DFM level 1; tests/test_door_maps.py
holds the premises on the oracle).  The patch is a 9 x 5 door, so a single planner holds it and gives it to the block replan kernel; the
wave it starts changes two to three times as many elements as the block holds and leaves it through its border: the invalidation along
stored back-pointers, the write-back of a frame the block did not finish, continue_block / the adaptive rounds behind the tail, the blind
batches of the graph route, the early exits of bursts with nothing finite in reach and their later wake-up all run in one step.

THE JUDGE is the local criterion of tests/test_gpu_field_reference.py (check_elements: every value against the float64 operator on the
device's own field, "focused" = 0 so that EVERY element is final and checked).  The operators are causal, so a field that passes at every
element is the field; a value left too low upstream of a closed door -- what an invalidation leaves that misses a descendant -- is off
at that element by millions of ulp (tests/test_door_maps.py).  On top of it: parity with the oracle stepped alike (focused, FD / SG bit for
bit), the path extractor across the doors, a batch, the step deltas.

KNOWN TO FAIL, not every time: MS-DFM level 1 with "dfm_follow_info" = 0 in the focused tests (2, 3), at step 6 -- the start walled off
while invalidations beyond the bound its old key gave are still held back.  ufm_step returns UFM_ERR_NOT_CONVERGED: Engine::converge's
lowering phase, unbounded once the start has no value, walks into values that wait for their invalidation, and they climb by a cell's cost
per sweep until the launch cap (28 672 launches, 0.7 s; afterwards 7 680 elements above 1e5 where the field's largest value is 24 094;
seen in the first run of test_focused_against_the_oracle[DFM-1]; test_paths_across_the_doors[DFM-1] passed its three runs).  The defect is the
engine's and is open (profiles/door_replans.txt, section 3); the cases stay so that it stays visible.  With "focused" = 0 (test 1) and
with "dfm_follow_info" = 1 the same steps pass.

BOUNDS: none of this file's own.  tolerances.NODE_LOCAL_ULP; tolerances.DFM_LOCAL_ULP + the 8 ulp of include/ufm.h at ufm_check_info;
field_reference.WINDOW_SHARE; bit equality for FD / SG; DFM_RTOL through helpers.dfm_close / check_parity."""
import functools

import numpy as np
import pytest

import ufm_amd
import oracle_py as orc
import door_maps as dm
from helpers import ALGOS, make_pair, check_parity, dfm_close
from test_gpu_field_reference import check_elements, window_share_ok, device_planner
from test_gpu_path import INDIRECT, same_path, close_path, oracle_on_device_field
from test_gpu_changes import Mirror

pytestmark = pytest.mark.gpu

PLANNERS = {"FD-1": ("FD", 1, {}), "SG-2": ("SG", 2, {}), "DFM-1": ("DFM", 1, {"dfm_follow_info": 0}), "DFM-1-follow": ("DFM", 1, {"dfm_follow_info": 1})}
# the block kernel; the launch chain as a captured graph, as a fused chain, as separate launches
VARIANTS = ({}, {"region": 0}, {"region": 0, "graph": 0}, {"region": 0, "graph": 0, "fuse_control": 0})
VARIANT_IDS = ["block-kernel", "graph", "fused-chain", "separate-launches"]
MAX_STEPS = 1000


def has_bytes(name):
    """the planners whose stored back-pointers the engine promises (ufm_check_info): FD / SG, and MS-DFM where its invalidation follows them"""
    return name != "DFM-1"


# ---------------------------------------------------------------------------------------------------- 1. whole field, every route
@functools.lru_cache(maxsize=None)
def whole_fields(name, variant):
    """the scenario with "focused" = 0 through one route, everything checked after the plan and after every step -> the fields, the plan's
    first (computed once per planner and route, shared by the comparison between the routes; nobody writes into them)"""
    algo, lvl, params = PLANNERS[name]
    size = dm.SIZES[algo]
    cost, start, goal = dm.comb(dm.SEED, size)
    p = device_planner(algo, lvl, cost, start, goal, dm.THRESHOLD, focused=0, **params, **VARIANTS[variant])
    cur, tally, out = cost.copy(), [0, 0], []

    def everything(what):
        g, rhs = p.read_field()
        ck, _ = check_elements(algo, cur, dm.THRESHOLD, g, rhs, goal, what, tally=tally)
        assert np.array_equal(p.read_map(size, size), cur), what + ": the device's raster is not the host's"
        assert p.check_layout() == (0, 0), "%s: layout self-check %r" % (what, p.check_layout())
        if has_bytes(name):
            ci = p.check_info()
            assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)
        g.setflags(write=False)
        out.append(g)
        return ck

    assert p.step() == 0
    everything("%s %s plan" % (name, VARIANT_IDS[variant]))
    for k, (step, patch, top, left, s) in enumerate(dm.scenario(size)):
        r0, d0 = p.stats.region_replans, p.stats.region_replans_done
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
        dm.apply(cur, patch, top, left)
        runs, done, launches = p.stats.region_replans - r0, p.stats.region_replans_done - d0, p.stats.region_launches
        ck = everything("%s %s step %s" % (name, VARIANT_IDS[variant], step))
        changed = int((out[-1].view(np.int32) != out[-2].view(np.int32)).sum())
        print("PROFILE %s | %s | %s | changed %d of %d, the block holds %d | region_replans +%d, region_replans_done +%d | worst %.3f ulp, %d through the window" % (
            name, VARIANT_IDS[variant], step, changed, out[-1].size, dm.BLOCK[algo], runs, done, ck.worst, ck.windowed))
        # the route, pinned by the statistics
        if variant == 0:
            assert (runs, launches) == (1, 1), "%s: the step did not go to the block kernel (region_replans +%d)" % (step, runs)
            if k in dm.LARGE:
                assert changed > dm.BLOCK[algo], "%s changed %d elements, the block holds %d" % (step, changed, dm.BLOCK[algo])
                assert done == 0, "%s: the block kernel reports a replan of %d elements finished inside a block of %d" % (step, changed, dm.BLOCK[algo])
        else:
            assert (runs, done, launches) == (0, 0, 0), "%s: a block-kernel launch with \"region\" = 0" % step
    window_share_ok(tally, "%s %s" % (name, VARIANT_IDS[variant]))
    # what the scenario is there for, on the device's own field
    cut = out[dm.CUT_OFF + 1]
    assert np.isinf(cut).sum() > cut.size // 2
    plan, back = out[0], out[dm.RESTORED + 1]
    if algo != "DFM":
        assert dm.same_bits(plan, back), "%d elements differ from the plan's after step 4" % int((plan.view(np.int32) != back.view(np.int32)).sum())
    else:
        fin = np.isfinite(plan)
        assert np.array_equal(fin, np.isfinite(back))
        assert dfm_close(back[fin], plan[fin], what=name + " after step 4 against the plan")
    p.close()
    return tuple(out)


@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("name", list(PLANNERS))
def test_whole_field(name, variant):
    """ "focused" = 0, the scenario through the block kernel and through the three forms of the launch chain.  After the plan and after every
    step: every element against the float64 operator (unreached ones, the goal and RHS == G included), the device's raster against the
    host's, the layout self-check, the byte self-check; the window share over the scenario.  The route by the statistics: in the default
    variant every step is a block-kernel replan, and steps 1 - 3 -- whose wave cannot fit the block -- are NOT finished by it alone; with
    "region" = 0 the block kernel is never launched.  After step 2 more than half the field is +inf; after step 4 the field is the plan's
    (FD / SG bit for bit)."""
    whole_fields(name, variant)


@pytest.mark.parametrize("name", list(PLANNERS))
def test_routes_agree(name):
    """the fields of the four routes at every step: FD / SG bit for bit, whole fields; MS-DFM the same finite set and dfm_close"""
    algo = PLANNERS[name][0]
    runs = [whole_fields(name, v) for v in range(len(VARIANTS))]
    for v in range(1, len(VARIANTS)):
        for k, (a, b) in enumerate(zip(runs[0], runs[v])):
            what = "%s step %d, %s against %s" % (name, k, VARIANT_IDS[v], VARIANT_IDS[0])
            if algo != "DFM":
                assert dm.same_bits(a, b), "%s: %d elements differ" % (what, int((a.view(np.int32) != b.view(np.int32)).sum()))
            else:
                fin = np.isfinite(a)
                assert np.array_equal(fin, np.isfinite(b)), "%s: %d elements hold a value in one field only" % (what, int((fin != np.isfinite(b)).sum()))
                assert dfm_close(b[fin], a[fin], what=what), what


# ---------------------------------------------------------------------------------------------------- 2. focused, against the oracle
def stepped_pair(name, heuristic=False):
    algo, lvl, params = PLANNERS[name]
    size = dm.SIZES[algo]
    cost, start, goal = dm.comb(dm.SEED, size)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, dm.THRESHOLD, heuristic=heuristic, hm=float(cost.min()) if heuristic else 1.0)
    for k, v in params.items():
        g.set_param(k, v)
    assert o.step() == 0 and g.step() == 0
    return algo, size, cost, goal, o, g


def parity(name, algo, o, g, what):
    n, nbad = check_parity(o, g, what, below_start_key=True)
    if algo != "DFM":
        assert nbad == 0, "%s: %d of %d trusted elements differ from the oracle" % (what, nbad, n)
    elif has_bytes(name):
        ci = g.check_info()
        assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)


@pytest.mark.parametrize("name", list(PLANNERS))
def test_focused_against_the_oracle(name):
    """default parameters, the oracle stepped alike: check_parity below the start's key after the plan and after every step -- FD / SG bit
    for bit --, the steps that leave the start's key at +inf (2 and 6: the whole field is final then) included"""
    algo, size, cost, goal, o, g = stepped_pair(name)
    parity(name, algo, o, g, name + " plan")
    r0 = g.stats.region_replans
    for k, (step, patch, top, left, s) in enumerate(dm.scenario(size)):
        for p in (o, g):
            p.patch_map(patch, top, left); p.set_start(*s)
            assert p.step() == 0
        assert np.isinf(o.start_key()) == (k in (dm.CUT_OFF, dm.WALLED_OFF)), step
        parity(name, algo, o, g, "%s step %s" % (name, step))
    assert g.stats.region_replans - r0 == len(dm.STEPS)
    g.close()


@pytest.mark.parametrize("name", ["FD-1", "SG-2"])
def test_heuristic_keys_against_the_oracle(name):
    """the same with heuristic keys, the multiplier at the raster's smallest cost (it follows the raster: the cheap door lowers it)"""
    algo, size, cost, goal, o, g = stepped_pair(name, heuristic=True)
    parity(name, algo, o, g, name + " heuristic plan")
    cur = cost.copy()
    for step, patch, top, left, s in dm.scenario(size):
        dm.apply(cur, patch, top, left)
        for p in (o, g):
            p.patch_map(patch, top, left); p.set_heuristic_multiplier(float(cur.min())); p.set_start(*s)
            assert p.step() == 0
        parity(name, algo, o, g, "%s heuristic step %s" % (name, step))
    g.close()


# ---------------------------------------------------------------------------------------------------- 3. paths across the doors
@pytest.mark.parametrize("name", list(PLANNERS))
def test_paths_across_the_doors(name):
    """default parameters.  After steps 1, 3, 5 and 7 -- the start has a way to the goal, through another door than before --
    extract_path(max_steps = 1000) is bit for bit the oracle's extractor on the device's field and close_path to the oracle's own path.
    After steps 2 and 6 the start is cut off: the walk is what the oracle's extractor returns on that field, and ONE extract_paths_from
    call walks from positions on both sides of every wall, cut-off ones included, each against the oracle's extractor from there."""
    algo, size, cost, goal, o, g = stepped_pair(name)
    kw = dict(max_steps=MAX_STEPS, lookahead=True, allow_indirect=INDIRECT[algo])
    cur = cost.copy()
    probes = dm.probe_positions(size)
    for k, (step, patch, top, left, s) in enumerate(dm.scenario(size)):
        dm.apply(cur, patch, top, left)
        for p in (o, g):
            p.patch_map(patch, top, left); p.set_start(*s)
            assert p.step() == 0
        what = "%s step %s" % (name, step)
        dev = g.extract_path(**kw)
        same_path(dev, oracle_on_device_field(g, algo, cur, 255, s, goal, **kw), what + " [device field]")
        if k in (dm.CUT_OFF, dm.WALLED_OFF):
            assert np.isinf(o.start_key()), what
            assert tuple(dev[0][-1]) != tuple(goal), what + ": a path from a start that is cut off"
            field = g.read_field()[1]
            paths = g.extract_paths_from(probes, **kw)
            assert len(paths) == len(probes)
            reached = 0
            for pos, path in zip(probes, paths):
                ref = orc.extract_path_field(field, algo == "DFM", cur, 255, (float(pos[0]), float(pos[1])), goal, **kw)
                same_path(path, ref, "%s from %r" % (what, tuple(pos)))
                reached += tuple(path[0][-1]) == tuple(goal)
            print("%s: %d of %d positions reach the goal" % (what, reached, len(probes)))
            if algo != "DFM":       # (MS-DFM with this extractor may oscillate short of the goal)
                assert 0 < reached < len(probes), what
        elif k in (0, 2, 4, 6):
            assert np.isfinite(o.start_key()), what
            close_path(dev, o.extract_path(**kw), what)
            if algo != "DFM":
                assert tuple(dev[0][-1]) == tuple(goal), what + ": the path does not reach the goal"
    g.close()


# ---------------------------------------------------------------------------------------------------- 4. a batch
@pytest.mark.parametrize("name", ["FD-1", "DFM-1-follow"])
def test_batch_of_two(name):
    """BatchPlanner(2), "focused" = 0.  Map 0 runs the scenario, map 1 runs it two rounds later (door_maps.filler keeps the map that has
    no scenario step busy), so that one map closes a door while the other opens one in the same launch.  Every element of both maps
    after every round; every round is one block-kernel launch with a workgroup per map."""
    algo, lvl, params = PLANNERS[name]
    size = dm.SIZES[algo]
    cost, start, goal = dm.comb(dm.SEED, size)
    b = ufm_amd.BatchPlanner(2, ALGOS[algo], lvl, follow_info=bool(params.get("dfm_follow_info")))
    b.set_occupancy_threshold(dm.THRESHOLD)
    b.set_param("focused", 0)
    for m in range(2):
        b.set_map(m, cost); b.set_start(m, *start); b.set_goal(m, *goal)
    assert b.step() == 0
    scripts = [dm.scenario(size) + dm.filler(size), dm.filler(size) + dm.scenario(size)]
    curs, tally = [cost.copy(), cost.copy()], [0, 0]
    closes_while_opens = 0
    for rnd in range(len(scripts[0])):
        r0 = b.stats.region_replans
        names = []
        for m in range(2):
            step, patch, top, left, s = scripts[m][rnd]
            b.patch_map(m, patch, top, left); b.set_start(m, *s)
            dm.apply(curs[m], patch, top, left)
            names.append(step)
        closes_while_opens += ("close" in names[0] and "open" in names[1]) or ("open" in names[0] and "close" in names[1])
        assert b.step() == 0
        assert b.stats.region_replans - r0 == 2, "round %d (%s | %s): region_replans +%d" % (rnd, names[0], names[1], b.stats.region_replans - r0)
        for m in range(2):
            g = b.read_field(m)
            check_elements(algo, curs[m], dm.THRESHOLD, g, g, goal, "%s map %d round %d (%s)" % (name, m, rnd, names[m]), tally=tally)
            assert np.array_equal(b.read_map(m, size, size), curs[m])
        ci = b.check_info()
        assert ci[1:4] == (0, 0, 0), "round %d: back-pointer self-check %r" % (rnd, ci)
    assert closes_while_opens >= 2
    window_share_ok(tally, name + " batch")
    assert b.check_layout() == (0, 0)
    b.close()


# ---------------------------------------------------------------------------------------------------- 5. step deltas at this scale
@pytest.mark.parametrize("name", ["FD-1", "DFM-1-follow"])
def test_step_deltas(name):
    """track_changes, default parameters.  After the plan and after every step: a read with room for all records but one delivers nothing
    and commits nothing; the full read, applied to a host mirror, makes the mirror the field bit for bit and its Info read_info's.  The
    values step 2 takes away -- more than the block holds -- arrive as +inf."""
    algo, lvl, params = PLANNERS[name]
    size = dm.SIZES[algo]
    cost, start, goal = dm.comb(dm.SEED, size)
    p = device_planner(algo, lvl, cost, start, goal, dm.THRESHOLD, **params)
    p.track_changes(True)
    m = Mirror(p.dims(), True)
    assert p.step() == 0
    for k, (step, patch, top, left, s) in enumerate([("plan", None, 0, 0, start)] + dm.scenario(size)):
        if patch is not None:
            p.patch_map(patch, top, left); p.set_start(*s)
            assert p.step() == 0
        what = "%s %s" % (name, step)
        total = p.read_changes(want_info=True, cap=0)[3]
        assert total > 1, what
        xy, g, info, t2 = p.read_changes(want_info=True, cap=total - 1)
        assert t2 == total and len(g) == 0, what
        before = m.g.copy()
        xy, g, info, t3 = p.read_changes(want_info=True, cap=total)
        assert t3 == total and len(g) == total, what
        m.apply(xy, g, info, what)
        m.check(p, what)
        assert p.read_changes(want_info=True, cap=0)[3] == 0, what
        removed = int((np.isfinite(before) & np.isinf(m.g)).sum())      # (the mirror is the field: these are the values the step took away)
        assert int(np.isinf(g).sum()) >= removed, what
        print("%s: %d records, %d of them removals" % (what, total, removed))
        if k - 1 == dm.CUT_OFF:
            assert removed > dm.BLOCK[algo], "%s: %d removals, the block holds %d" % (what, removed, dm.BLOCK[algo])
    p.close()
