"""-m gpu: HIP engine (through the C ABI) vs the CPU oracle."""
import numpy as np
import pytest

import ufm_amd
import oracle_py as orc
from helpers import ALGOS, DFM_RTOL, DeviceBytes, check_parity, dfm_close, make_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
@pytest.mark.parametrize("bitmap", ["noise-trap", "square", "wall-a", "wall-b"])
def test_first_plan_reference_bitmaps(ref_bitmaps, algo, bitmap):
    cost, (fx, fy, tx, ty) = ref_bitmaps[bitmap]
    o, g = make_pair(ALGOS[algo], 0, cost, (fx, fy), (tx, ty))
    assert o.step() == 0
    assert g.step() == 0
    n, nbad = check_parity(o, g, "%s/%s" % (algo, bitmap))
    if algo != "DFM":   # DFM: tolerance (check_parity), its float fixed point is not unique
        assert nbad == 0, "%d of %d trusted elements not bit-equal" % (nbad, n)
    g.close()


@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
@pytest.mark.parametrize("size", [(64, 64), (200, 136), (256, 256)])
def test_first_plan_synthetic(algo, size):
    width, length = size
    cost = ufm_amd.synth.cost_map(1234, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    o, g = make_pair(ALGOS[algo], 0, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    n, nbad = check_parity(o, g, "%s/%dx%d" % (algo, width, length))
    if algo != "DFM":
        assert nbad == 0, "%d of %d trusted elements not bit-equal" % (nbad, n)
    # the engine counts every element it finalised; the oracle's expansions are a subset
    assert g.num_nodes_expanded >= n
    g.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 0), ("FD", 1), ("SG", 0), ("SG", 2), ("DFM", 0), ("DFM", 1)])
def test_replans_synthetic(algo, lvl):
    width = length = 192
    seed = 7
    cost = ufm_amd.synth.cost_map(seed, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    check_parity(o, g, "%s first plan" % algo)
    total_bad = 0
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, width, length, n_patches=25):
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
        assert o.step() == 0 and g.step() == 0
        assert g.num_nodes_updated == o.num_updated, (k, g.num_nodes_updated, o.num_updated)
        n, nbad = check_parity(o, g, "%s replan %d" % (algo, k))
        total_bad += nbad
    # FD / SG: bit-equal.  DFM: the upwind quadratic is not monotone at the ulp level, its
    # float fixed point is not unique (the oracle's own DFM-0 and DFM-1 differ in the last
    # bits on this map, see tests/test_oracle.py), so DFM is held to helpers.DFM_RTOL, which check_parity enforces.
    if algo != "DFM":
        assert total_bad == 0
    # the device raster followed the patches
    assert np.array_equal(g.read_map(width, length)[:40, :40], _patched(cost, seed, width, length, 25)[:40, :40])
    g.close()


def _patched(cost, seed, width, length, n):
    c = cost.copy()
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, width, length, n_patches=n):
        c[top:top + patch.shape[0], left:left + patch.shape[1]] = patch
    return c


def test_full_field_is_fixed_point_after_replans():
    """Size-independent property: after any sequence of patches the converged
    field equals the field of a fresh plan on the patched map (bitwise)."""
    width = length = 320
    seed = 99
    cost = ufm_amd.synth.cost_map(seed, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    g.set_param("focused", 0)          # converge the whole field every step
    g.set_occupancy_threshold(1)
    g.set_map(cost)
    g.set_start(*start)
    g.set_goal(*goal)
    assert g.step() == 0
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, width, length, n_patches=12):
        g.patch_map(patch, top, left)
        g.set_start(*s)
        assert g.step() == 0
    inc = g.g()
    f = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    f.set_param("focused", 0)
    f.set_occupancy_threshold(1)
    f.set_map(_patched(cost, seed, width, length, 12))
    f.set_start(*start)
    f.set_goal(*goal)
    assert f.step() == 0
    fresh = f.g()
    assert np.array_equal(inc, fresh)
    g.close(); f.close()


@pytest.mark.parametrize("algo", ["FD", "SG", "DFM"])
def test_focused_and_full_field_agree_below_the_start_key(algo):
    """The default (focused) engine stops at the start's key like the reference's end_condition;
    every element whose value is below that key must equal the fully converged field."""
    width = length = 256
    seed = 21
    cost = ufm_amd.synth.cost_map(seed, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    ps = []
    for focused in (1, 0):
        p = ufm_amd.Planner(ALGOS[algo], 0)
        p.set_param("focused", focused)
        p.set_occupancy_threshold(1)
        p.set_map(cost)
        p.set_start(*start)
        p.set_goal(*goal)
        assert p.step() == 0
        ps.append(p)
    work = [0, 0]
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, width, length, n_patches=30):
        for i, p in enumerate(ps):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
            work[i] += p.stats.tile_visits
        gf, gu = ps[0].g(), ps[1].g()
        sx, sy = int(s[0]), int(s[1])
        key = gu[sx, sy] if algo == "DFM" else max(gu[sx, sy], gu[sx + 1, sy], gu[sx, sy + 1], gu[sx + 1, sy + 1])
        m = gu < key
        assert m.sum() > 100
        if algo == "DFM":   # tolerance: the float fixed point of the DFM quadratic is not unique
            assert dfm_close(gf[m], gu[m])
        else:
            assert np.array_equal(gf[m], gu[m]), "replan %d: %d differ" % (k, int((gf[m] != gu[m]).sum()))
    assert work[0] < work[1]          # focusing must save work
    for p in ps:
        p.close()


def test_result_independent_of_scheduler_knobs():
    """Band width, sweep cap, grid size, batch submission and hand-out mode are scheduling knobs only
    (full-field mode: bitwise)."""
    width, length = 224, 160
    cost = ufm_amd.synth.cost_map(4, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    fields = []
    for scale, cap, grid, extra in [(1.0, 128, 512, {}), (0.25, 128, 512, {}), (1e9, 128, 64, {}), (2.0, 3, 7, {}),
                                    (1.5, 32, 64, {"pipeline_batches": 0}),            # host waits for every batch of launches
                                    (1.5, 32, 64, {"delta_scale_long": 3.0, "batch": 2}),   # other band for long queues, short batches
                                    (1.5, 32, 16, {"dynamic": 0}),                     # fused triage only
                                    (1.5, 32, 64, {"owned": 0}),                       # the plan through the launch chain, not the resident kernel
                                    (1.5, 32, 64, {"owned_band": 0.5}),                # resident kernel: narrow band, ...
                                    (1.5, 32, 64, {"owned_waves": 8}),                 # ... 8 waves per tile visit (two visits per CU, 512 owners), ...
                                    (1.5, 5, 64, {"owned_band": 1e9, "owned_flags": 1}),   # ... no band, no tile taken ahead, a low sweep cap,
                                    (1.5, 32, 64, {"owned_limit_ms": 0.02})]:          # ... and one that runs into its time limit and hands back
        p = ufm_amd.Planner(ufm_amd.ALGO_SG, 0)
        p.set_param("focused", 0); p.set_param("delta_scale", scale); p.set_param("max_iters", cap); p.set_param("grid", grid)
        for name, val in extra.items():
            p.set_param(name, val)
        p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
        assert p.step() == 0
        for k, s, top, left, patch in ufm_amd.synth.replan_script(4, width, length, n_patches=5):
            p.patch_map(patch, top, left); p.set_start(*s)
            assert p.step() == 0
        fields.append(p.g())
        p.close()
    for f in fields[1:]:
        assert np.array_equal(fields[0], f)


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)])
def test_resident_plan_kernel(algo, lvl):
    """The plan's lowering phase as one resident launch (k_relax<., LOWER, false, 1 | 2>): against the oracle below the start's
    key; it reports itself in the statistics; cut short by its time limit it hands the queue back to the launch chain, which
    finishes the plan with the same result."""
    size = 600
    cost = ufm_amd.synth.cost_map(11, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    st = g.stats
    assert st.resident_launches == 1 and st.resident_stops == 0
    assert 0 < st.resident_tile_visits <= st.tile_visits
    check_parity(o, g, "%s-%d resident" % (algo, lvl))
    g.close()
    p = ufm_amd.Planner(ALGOS[algo], lvl)
    p.set_param("owned_waves", 8)                                       # the other form: 8 waves per visit, 512 workgroups
    p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
    assert p.step() == 0
    assert p.stats.resident_launches == 1 and p.stats.resident_stops == 0
    check_parity(o, p, "%s-%d resident, 8 waves" % (algo, lvl))
    p.close()
    p = ufm_amd.Planner(ALGOS[algo], lvl)
    p.set_param("owned_limit_ms", 0.05)
    p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
    assert p.step() == 0
    st = p.stats
    assert st.resident_launches == 1 and st.resident_stops > 0          # every workgroup left on the limit ...
    assert st.launches > 1 and st.resident_tile_visits < st.tile_visits  # ... and the launch chain did the rest
    check_parity(o, p, "%s-%d resident, handed back" % (algo, lvl))
    p.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)])
def test_resident_scheduler_variants(algo, lvl):
    """The resident kernel's scheduler in its variants -- idle workgroups helping out or not, border values handed out during a visit
    or only at its end, activations taken in during a visit or not (owned_flags), both wave counts, a narrow and a wide band, no tile
    taken ahead -- only decides who visits which tile when: focused, every variant equals the oracle below the start's key; unfocused,
    the whole FD / SG field is the same bit for bit in all of them (DFM: within its bound)."""
    size = 520
    cost = ufm_amd.synth.cost_map(23, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    variants = [dict(), dict(owned_flags=32), dict(owned_flags=2), dict(owned_flags=16), dict(owned_flags=34), dict(owned_flags=4), dict(owned_flags=8),
                dict(owned_flags=1), dict(owned_waves=8), dict(owned_waves=8, owned_flags=32), dict(owned_band=1.0), dict(owned_band=1e9)]
    o, g0 = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert o.step() == 0
    g0.close()
    ref = None
    for full in (0, 1):
        for v in variants:
            p = ufm_amd.Planner(ALGOS[algo], lvl)
            p.set_param("focused", 0 if full else 1)
            for name, val in v.items():
                p.set_param(name, val)
            p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
            assert p.step() == 0
            assert p.stats.resident_launches == 1 and p.stats.resident_stops == 0, v
            assert p.check_layout() == (0, 0), v
            if not full:
                check_parity(o, p, "%s-%d resident %r" % (algo, lvl, v))
            else:
                f = p.g()
                if ref is None:
                    ref = f
                elif algo != "DFM":
                    assert np.array_equal(f, ref), v
                else:
                    fin = np.isfinite(ref)
                    assert np.array_equal(fin, np.isfinite(f)), v
                    assert dfm_close(f[fin], ref[fin]), v
            p.close()


def test_edge_cases():
    # tiny maps, maps smaller than a tile, non-multiple-of-tile sizes, goal in a corner, start == goal
    for (w, l) in [(1, 1), (3, 2), (33, 31), (64, 65)]:
        cost = np.full((l, w), 7, dtype=np.uint8)
        for algo in ("FD", "SG", "DFM"):
            o, g = make_pair(ALGOS[algo], 0, cost, (0.0, 0.0), (float(l - 1), float(w - 1)))
            assert o.step() == 0 and g.step() == 0
            check_parity(o, g, "%s %dx%d" % (algo, w, l))
            g.close()
    # a wall that separates start and goal: everything behind it stays +inf on both sides
    cost = np.full((40, 40), 5, dtype=np.uint8)
    cost[:, 20] = 255
    o, g = make_pair(ALGOS["FD"], 0, cost, (5.0, 5.0), (30.0, 30.0))
    assert o.step() == 0 and g.step() == 0
    gg = g.g()
    assert np.isinf(gg[:, :20]).all() and np.isfinite(gg[:, 22:]).all()
    # return codes of step() without a map / without a goal (ReplannerBase.h:44-45)
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 0)
    assert p.step() == ufm_amd.LOOP_FAILURE_NO_GRAPH
    p.set_map(cost)
    assert p.step() == ufm_amd.LOOP_FAILURE_NO_GOAL
    p.close(); g.close()


def test_occupancy_threshold_semantics():
    # Graph.cpp:18-20,267: byte >= int(thr*255) is an obstacle; default 254
    cost = np.full((48, 48), 10, dtype=np.uint8)
    cost[10:20, 10:20] = 254
    for thr in (None, 1.0, 0.5):
        o = __import__("oracle_py").OraclePlanner(0, 0, False)
        g = ufm_amd.Planner(0, 0)
        for p in (o, g):
            p.reset()
            if thr is not None:
                p.set_occupancy_threshold(thr)
            p.set_map(cost); p.set_start(2.0, 2.0); p.set_goal(40.0, 40.0)
            assert p.step() == 0
        n, nbad = check_parity(o, g, "thr %s" % thr)
        assert nbad == 0
        g.close()


def test_batch_of_independent_maps():
    n, size = 5, 128
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_DFM, 0)
    b.set_occupancy_threshold(1)
    import oracle_py as orc
    oracles = []
    for i in range(n):
        cost = ufm_amd.synth.cost_map(1000 + i, size, size)
        start, goal = ufm_amd.synth.start_goal(size, size)
        b.set_map(i, cost); b.set_start(i, *start); b.set_goal(i, *goal)
        o = orc.OraclePlanner(orc.ALGO_DFM, 0, False)
        o.reset(); o.set_occupancy_threshold(1); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        oracles.append(o)
    assert b.step() == 0
    for i, o in enumerate(oracles):
        m = o.trusted_mask(below_start_key=True)   # what a planner honouring end_condition must have finalised
        a, ref = b.read_field(i)[m], o.g()[m]
        assert m.sum() > 10000
        assert dfm_close(a, ref)
    # patch two of the maps, leave the others alone
    for i in (1, 3):
        patch = np.full((9, 9), 3 + i, dtype=np.uint8)
        b.patch_map(i, patch, 60, 60); b.set_start(i, 8.0, 8.0)
        oracles[i].patch_map(patch, 60, 60); oracles[i].set_start(8.0, 8.0)
        assert oracles[i].step() == 0
    assert b.step() == 0
    for i, o in enumerate(oracles):
        m = o.trusted_mask(below_start_key=True)
        a, ref = b.read_field(i)[m], o.g()[m]
        assert dfm_close(a, ref), (i, int(m.sum()))
    assert b.check_layout() == (0, 0)
    b.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)])
def test_heuristic_keys(algo, lvl):
    """Planners built with heuristic keys (the reference's default, no -DNO_HEURISTIC): the engine
    prunes tiles whose admissible key bound is not below the start's key.  Everything the reference
    guarantees final AND a planner honouring end_condition must have finalised (key < start key)
    has to match; the heuristic multiplier is the map's minimum cost as in the reference harness."""
    width = length = 224
    seed = 31
    cost = ufm_amd.synth.cost_map(seed, width, length)
    hm = float(cost.min())
    # start in the interior so that the heuristic actually prunes part of the map
    start, goal = (60.0, 70.0), (float(length - 8), float(width - 8))
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, heuristic=True, hm=hm)
    assert o.step() == 0 and g.step() == 0
    n, nbad = check_parity(o, g, "%s heuristic first plan" % algo, below_start_key=True)
    assert n > 1000
    if algo != "DFM":
        assert nbad == 0
    reached = np.isfinite(g.g()).sum()
    assert reached < 0.98 * g.g().size        # the search was focused: part of the map never got relaxed
    sx, sy = start
    for k in range(1, 13):
        top, left = int(sx) - 15 + 3 * k, int(sy) - 15 + 2 * k
        patch = (1 + (ufm_amd.synth.h64(seed ^ k, *np.meshgrid(np.arange(top, top + 31), np.arange(left, left + 31), indexing="ij")) % np.uint64(200))).astype(np.uint8)
        s = (sx + 3 * k, sy + 2 * k)
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_heuristic_multiplier(hm)
            p.set_start(*s)
        assert o.step() == 0 and g.step() == 0
        n, nbad = check_parity(o, g, "%s heuristic replan %d" % (algo, k), below_start_key=True)
        if algo != "DFM":
            assert nbad == 0, (k, nbad, n)
    g.close()


@pytest.mark.parametrize("algo,size,seed", [("FD", 1024, 1000), ("SG", 1024, 1000), ("DFM", 1024, 1000), ("DFM", 2048, 1000),
                                            ("SG", 2048, 1234)])
def test_first_plan_large(algo, size, seed):
    """Larger maps (the oracle still finishes in seconds): FD / SG bit-equal (SG at 2048^2 with seed 1234 is
    BASELINE config 2); DFM within helpers.DFM_RTOL -- including the 2048^2 map on which the level-0 form of the
    DFM operator never settles (the reference's own DFMPlanner<0> does not terminate there either)."""
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS[algo], 1 if algo != "SG" else 2, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    assert g.stats.launches < 4000
    n, nbad = check_parity(o, g, "%s/%d" % (algo, size))
    assert n > 0.9 * size * size
    if algo != "DFM":
        assert nbad == 0
    g.close()


@pytest.mark.parametrize("algo,lvl,size,seed", [("FD", 0, 2048, 3), ("SG", 0, 2048, 3), ("SG", 1, 2048, 3), ("SG", 2, 4096, 7)])
def test_first_plan_large_other_levels(algo, lvl, size, seed):
    """the optimisation levels test_first_plan_large does not run, at 2048^2, and the shifted-grid planner at the headline size:
    bit-equal to the oracle's planner of that level below the start's key (the levels differ in bookkeeping, not in the field)"""
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    n, nbad = check_parity(o, g, "%s-%d/%d" % (algo, lvl, size), below_start_key=True)
    assert n > 0.9 * size * size and nbad == 0
    g.close()


@pytest.mark.parametrize("seed", [1000, 1003])
def test_dfm_level0_at_1024(seed):
    """MS-DFM level 0 (DFMPlanner<0>, min_rhs<0>: the better cell of each opposite pair, one quadratic per stencil) against the
    oracle's level-0 planner at the largest size of the config-4 maps where that one terminates (1024^2: one map's worth of
    expansions; at 2048^2 seed 1000 it does not), plan and five replans, under the one DFM bound
    (helpers.DFM_RTOL).  The engine serves a level-0 planner with the level-1 operator (the smallest of the eight
    per-neighbour candidates): same fixed point in exact arithmetic, and in fp32 CLOSER to the reference's level-0 field than
    iterating min_rhs<0> itself with the creep cut-offs that needs (24 maps 256^2..1024^2: <= 1.03e-6 against <= 2.45e-6;
    seed 1003 is the map on which the level-0 operator broke the bound)."""
    size = 1024
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS["DFM"], 0, cost, start, goal)
    assert o.step() == 0 and g.step() == 0
    assert g.stats.launches < 4000
    n, nbad = check_parity(o, g, "DFM-0/%d seed %d" % (size, seed), below_start_key=True)
    assert n > 0.9 * size * size
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=5):
        for p in (o, g):
            p.patch_map(patch, top, left); p.set_start(*s)
            assert p.step() == 0
        check_parity(o, g, "DFM-0/%d seed %d replan %d" % (size, seed, k), below_start_key=True)
    g.close()


def test_patches_accumulate_until_the_next_step():
    """Several patch_map calls before one step() (overlapping, one of them a no-op) are all
    propagated -- a superset of the reference, which keeps only the last patch's change list
    (Graph.cpp:37).  Checked against a fresh plan on the patched raster, full-field mode, bitwise."""
    width = length = 200
    cost = ufm_amd.synth.cost_map(77, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    g = ufm_amd.Planner(ufm_amd.ALGO_SG, 2)
    g.set_param("focused", 0)
    g.set_occupancy_threshold(1); g.set_map(cost); g.set_start(*start); g.set_goal(*goal)
    assert g.step() == 0
    cur = cost.copy()
    rng = np.random.default_rng(5)
    patches = [(40, 50, rng.integers(1, 200, (20, 30), dtype=np.uint8)),
               (50, 60, rng.integers(150, 255, (25, 25), dtype=np.uint8)),      # overlaps the first, raises costs
               (120, 30, None)]                                                  # a no-op patch (current bytes)
    for (x, y, pt) in patches:
        if pt is None:
            pt = cur[x:x + 10, y:y + 10].copy()
        g.patch_map(pt, x, y)
        cur[x:x + pt.shape[0], y:y + pt.shape[1]] = pt
    g.set_start(*start)
    assert g.step() == 0
    assert g.num_nodes_updated > 0
    f = ufm_amd.Planner(ufm_amd.ALGO_SG, 2)
    f.set_param("focused", 0)
    f.set_occupancy_threshold(1); f.set_map(cur); f.set_start(*start); f.set_goal(*goal)
    assert f.step() == 0
    assert np.array_equal(g.g(), f.g())
    assert np.array_equal(g.read_map(width, length), cur)
    # a step without set_start does not propagate a pending patch (ReplannerBase.h:56) ...
    g.patch_map(np.full((5, 5), 9, np.uint8), 10, 10)
    before = g.g()
    assert g.step() == 0
    assert np.array_equal(before, g.g()) and g.num_nodes_expanded == 0
    # ... the next one with set_start does
    g.set_start(*start)
    assert g.step() == 0
    assert g.num_nodes_updated > 0
    g.close(); f.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("DFM", 1)])
def test_replan_submission_variants_agree(algo, lvl):
    """A replan runs in the block-resident kernel (one workgroup, both phases in LDS) and falls back to the
    launch chain -- one captured graph of fused control kernels whose result the host picks up from
    host-coherent memory.  Each of the mechanisms can be switched off; fields
    (focused mode, below the start key: against the oracle; full field: bitwise between variants in
    full-field mode), num_nodes_updated and num_nodes_expanded must not depend on them.  Includes a
    step with 6 pending patches (more than the fused kernel takes) and one with a 70x70 patch
    (larger than the single-workgroup patch kernel takes).  The statistics of every step pin the route it took: the resident kernel plans,
    the default variant replans in the block kernel except on those two steps, a variant without the block kernel never does, and
    graphs are instantiated exactly where the fused chain may be replayed as one."""
    width = length = 208
    seed = 31
    cost = ufm_amd.synth.cost_map(seed, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    script = list(ufm_amd.synth.replan_script(seed, width, length, n_patches=12))
    rng = np.random.default_rng(3)
    big = rng.integers(1, 200, (70, 70), dtype=np.uint8)
    # default: the block-resident kernel (region); region=0: the launch chain in its submission forms
    variants = [dict(), dict(region_tiles=3, region_band=0), dict(region=0), dict(owned=0), dict(region=0, graph=0), dict(region=0, graph=0, fuse_control=0),
                dict(region=0, graph=0, fuse_control=0, spin_wait=0), dict(region=0, spin_wait=0)]
    results = []
    for full in (1, 0):
        results.clear()
        for v in variants:
            p = ufm_amd.Planner(ALGOS[algo], lvl)
            p.set_param("focused", 0 if full else 1)
            for name, val in v.items():
                p.set_param(name, val)
            p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
            assert p.step() == 0
            assert p.stats.resident_launches == (0 if v.get("owned") == 0 else 1), v
            log = []
            for k, s, top, left, patch in script:
                if k == 5:        # six rectangles before one step
                    for j in range(5):
                        p.patch_map(patch[: 8 + j, : 9 + j].copy(), min(top + 3 * j, length - 40), min(left + 5 * j, width - 40))
                if k == 8:        # a patch of 70 x 70 cells
                    p.patch_map(big, 60, 70)
                p.patch_map(patch, top, left)
                p.set_start(*s)
                assert p.step() == 0
                log.append((p.num_nodes_updated, p.num_nodes_expanded if (full and algo != "DFM") else 0))
                if not v:                     # default: a single small patch goes through the block kernel, six or a 70 x 70 one cannot
                    assert p.stats.region_launches == (0 if k in (5, 8) else 1), k
                elif v.get("region") == 0:
                    assert p.stats.region_launches == 0, (v, k)
            if v.get("region") == 0:          # only a fused chain is captured: graph on, and spin_wait on (without it nothing is fused)
                graphed = v.get("graph", 1) != 0 and v.get("spin_wait", 1) != 0
                assert (p.stats.graphs_instantiated > 0) == graphed and (graphed or p.stats.graphs_instantiated == 0), v
            results.append((p.g(), log, p.read_map(width, length)))
            p.close()
        for g, log, m in results[1:]:
            assert log == results[0][1]
            assert np.array_equal(m, results[0][2])
            if full and algo != "DFM":
                assert np.array_equal(g, results[0][0])
            elif full:   # DFM's float fixed point depends on the relaxation order at the ulp level
                r0 = results[0][0]
                fin = np.isfinite(r0)
                assert np.array_equal(fin, np.isfinite(g))
                assert dfm_close(g[fin], r0[fin])
    # focused mode (the last loop): against the oracle, below the start's key
    o = __import__("oracle_py").OraclePlanner(ALGOS[algo], lvl, False)
    o.reset(); o.set_occupancy_threshold(1); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
    assert o.step() == 0
    for k, s, top, left, patch in script:
        if k == 5:
            for j in range(5):
                o.patch_map(patch[: 8 + j, : 9 + j].copy(), min(top + 3 * j, length - 40), min(left + 5 * j, width - 40))
                o.set_start(*s); o.step()      # the reference keeps only the last patch's change list: step per patch
        if k == 8:
            o.patch_map(big, 60, 70); o.set_start(*s); o.step()
        o.patch_map(patch, top, left)
        o.set_start(*s)
        assert o.step() == 0
    mask = o.trusted_mask(below_start_key=True)
    og = o.g()
    for g, log, m in results:
        a, b = g[mask], og[mask]
        if algo == "DFM":
            assert dfm_close(a, b)
        else:
            assert np.array_equal(a, b)


def test_headline_size_4096_against_oracle_and_properties():
    """BASELINE.json's headline configuration (Field D* level 1, 4096x4096, seed 7): the full plan and ALL 100
    replans of the episode bench.py times are compared with the oracle bit for bit on the set a planner
    honouring end_condition must have finalised (after the plan, after each of the first 4 replans, then after
    every 8th and after the last one; num_nodes_updated after every one), plus size-independent properties
    (idempotence, goal value, a second engine in full-field mode agrees below the start's key)."""
    size, seed = 4096, 7
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS["FD"], 1, cost, start, goal)
    u = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    u.set_param("focused", 0)
    u.set_occupancy_threshold(1); u.set_map(cost); u.set_start(*start); u.set_goal(*goal)
    assert o.step() == 0 and g.step() == 0 and u.step() == 0
    n, nbad = check_parity(o, g, "FD-1 4096 plan", below_start_key=True)
    assert n > 16_000_000 and nbad == 0
    assert g.g()[int(goal[0]), int(goal[1])] == 0.0
    script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=100))
    for i, (k, s, top, left, patch) in enumerate(script):
        for p in (o, g) + ((u,) if i < 4 else ()):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
        assert g.num_nodes_updated == o.num_updated, (k, g.num_nodes_updated, o.num_updated)
        if i < 4 or i % 8 == 7 or i == len(script) - 1:
            n, nbad = check_parity(o, g, "FD-1 4096 replan %d" % k, below_start_key=True)
            assert nbad == 0
        if i < 4:
            gf, gu = g.g(), u.g()
            key = max(gu[int(s[0]) + a, int(s[1]) + b] for a in (0, 1) for b in (0, 1))
            m = gu < key
            assert np.array_equal(gf[m], gu[m])
    # idempotence: nothing pending, nothing changes
    before = g.g()
    g.set_start(*s)
    assert g.step() == 0
    assert g.num_nodes_expanded == 0 and np.array_equal(before, g.g())
    g.close(); u.close()


def test_config5_8192_heuristic_keys_moving_start_properties():
    """BASELINE.json config 5 (Field D* 8192x8192, moving start, heuristic keys re-ordered per move;
    this GPU's replica).  The oracle needs minutes at this size, so the check is by properties: a
    focused engine with heuristic keys equals a full-field engine on every node whose key lies below
    the start's key, after the plan and after each move; the goal stays 0; an idle step changes
    nothing."""
    size, seed = 8192, 42
    cost = ufm_amd.synth.cost_map(seed, size, size)
    hm = float(cost.min())
    start, goal = ufm_amd.synth.start_goal(size, size)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, True)
    u = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    u.set_param("focused", 0)
    for p in (g, u):
        p.set_occupancy_threshold(1); p.set_heuristic_multiplier(hm); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
        assert p.step() == 0
    xs = np.arange(size + 1, dtype=np.float32)

    def agree(s):
        gf, gu = g.g(), u.g()
        assert gf[int(goal[0]), int(goal[1])] == 0.0
        sx, sy = int(round(s[0])), int(round(s[1]))
        dist = np.hypot(xs[:, None] - np.float32(s[0]), xs[None, :] - np.float32(s[1])).astype(np.float32)
        corners = [(sx + a, sy + b) for a in (0, 1) for b in (0, 1)]
        key = max(gu[c] + np.float32(hm) * dist[c] for c in corners)
        m = (gu + np.float32(hm) * dist) < key
        assert int(m.sum()) > 1000
        assert np.array_equal(gf[m], gu[m]), "focused/heuristic engine differs from the full field below the start's key"
        return int(m.sum())

    n0 = agree(start)
    assert n0 < (size + 1) ** 2            # the heuristic did leave part of the map alone
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=3):
        for p in (g, u):
            p.patch_map(patch, top, left)
            p.set_heuristic_multiplier(hm)
            p.set_start(*s)
            assert p.step() == 0
        agree(s)
    before = g.g()
    g.set_start(*s)
    assert g.step() == 0 and g.num_nodes_expanded == 0
    assert np.array_equal(before, g.g())
    g.close(); u.close()


def test_config5_8192_heuristic_keys_moving_start_against_the_oracle():
    """BASELINE.json config 5 against the oracle: Field D* level 1, 8192x8192, seed 42, heuristic keys (hm = the map's
    smallest cost), the start moving with the patch script.  Plan + 8 replans.  After the plan and after the last replan
    the WHOLE field is compared with the oracle on the set it guarantees final below the start's key -- bit for bit (FD),
    layout and back-pointer self-checks included (check_parity); after every replan in between, the 1537 x 1537 nodes
    around the start (a replan changes a few thousand nodes next to its patch; the whole-field mask of 67 M elements
    costs the host more than the nine steps cost the oracle)."""
    size, seed = 8192, 42
    cost = ufm_amd.synth.cost_map(seed, size, size)
    hm = float(cost.min())
    start, goal = ufm_amd.synth.start_goal(size, size)
    o, g = make_pair(ALGOS["FD"], 1, cost, start, goal, heuristic=True, hm=hm)
    assert o.step() == 0 and g.step() == 0
    n, nbad = check_parity(o, g, "config 5 plan", below_start_key=True)
    assert nbad == 0 and n > 1_000_000
    script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=8))
    for k, s, top, left, patch in script:
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_heuristic_multiplier(hm)
            p.set_start(*s)
            assert p.step() == 0
        assert g.num_nodes_updated == o.num_updated
        x0, y0 = max(0, int(s[0]) - 768), max(0, int(s[1]) - 768)
        x1, y1 = min(size + 1, x0 + 1537), min(size + 1, y0 + 1537)
        mask = o.trusted_mask(below_start_key=True, window=(x0, x1, y0, y1))
        assert int(mask.sum()) > 10_000
        got = g.read_field(x0, y0, x1 - x0, y1 - y0)[0]
        assert np.array_equal(got[mask], o.g()[x0:x1, y0:y1][mask]), "config 5 replan %d: field differs from the oracle around the start" % k
        assert g.check_layout() == (0, 0) and g.check_info()[1:4] == (0, 0, 0)
    n, nbad = check_parity(o, g, "config 5 after %d replans" % len(script), below_start_key=True)
    assert nbad == 0 and n > 1_000_000
    g.close()


def test_batch_with_heuristic_keys_and_a_new_multiplier_every_round():
    """A batch whose heuristic multiplier changes with every replan round (what the reference's harness does per
    planner, Tests/Planners/DFM/main.cpp:111-112): every map's workgroup of the block kernel reads the per-step scalars
    (the multiplier in start_bound / tile_heuristic) -- they are in device memory before the launch, not stored by one of
    the workgroups during it.  Every map against its own oracle after every round, bit for bit."""
    n, width, length = 5, 208, 176
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, True)
    b.set_occupancy_threshold(1.0)
    b.set_heuristic_multiplier(1.0)
    start, goal = (50.0, 40.0), (float(length - 8), float(width - 8))
    oracles, costs = [], []
    for m in range(n):
        c = ufm_amd.synth.cost_map(300 + m, width, length)
        costs.append(c)
        b.set_map(m, c); b.set_start(m, *start); b.set_goal(m, *goal)
        o = orc.OraclePlanner(orc.ALGO_FD, 1, True)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_heuristic_multiplier(1.0); o.set_map(c); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        oracles.append(o)
    assert b.step() == 0

    def against(what):
        for m, o in enumerate(oracles):
            mask = o.trusted_mask(below_start_key=True)
            assert int(mask.sum()) > 100
            assert np.array_equal(b.read_field(m)[mask], o.g()[mask]), "%s: map %d differs from its oracle" % (what, m)
        assert b.check_layout() == (0, 0)
        assert b.check_info()[1:4] == (0, 0, 0), b.check_info()
    against("plan")
    regions0 = b.stats.region_replans
    for k in range(1, 13):
        hm = 1.0 - 0.03 * (k % 5)
        b.set_heuristic_multiplier(hm)
        s = (start[0] + 3 * k, start[1] + 2 * k)
        for m, o in enumerate(oracles):
            top, left = int(s[0]) - 15 + (m % 3), int(s[1]) - 15 + (m % 2)
            patch = (1 + (ufm_amd.synth.h64((300 + m) ^ k, *np.meshgrid(np.arange(top, top + 31), np.arange(left, left + 31), indexing="ij")) % np.uint64(200))).astype(np.uint8)
            b.patch_map(m, patch, top, left); b.set_start(m, *s)
            o.patch_map(patch, top, left); o.set_heuristic_multiplier(hm); o.set_start(*s)
            assert o.step() == 0
        assert b.step() == 0
        against("round %d hm %.2f" % (k, hm))
    assert b.stats.region_replans > regions0      # the rounds did go through the block kernel (one workgroup per map)
    b.close()


def test_config4_batch_of_8_maps_2048_dfm():
    """BASELINE.json config 4, one GPU's share: 8 independent 2048x2048 MS-DFM maps (seeds 1000..1007) in one
    batch, every map with its own 100-patch stream -- the episode `bench.py --algo DFM --size 2048 --batch 8` times.
    ALL eight maps against their oracles on the set the reference guarantees final below the start's key
    (helpers.DFM_RTOL): after the plan, after every 10th replan round and after the last; all 100 rounds are stepped
    (the oracles in lockstep).  Every map reaches its start, one launch extracts all eight paths."""
    n, size, rounds = 8, 2048, 100
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_DFM, 1)
    b.set_occupancy_threshold(1.0)
    start, goal = ufm_amd.synth.start_goal(size, size)
    oracles, scripts = [], []
    for m in range(n):
        c = ufm_amd.synth.cost_map(1000 + m, size, size)
        b.set_map(m, c); b.set_start(m, *start); b.set_goal(m, *goal)
        o = orc.OraclePlanner(orc.ALGO_DFM, 1, False)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_map(c); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        oracles.append(o)
        scripts.append(list(ufm_amd.synth.replan_script(1000 + m, size, size, n_patches=rounds)))
    assert b.step() == 0

    def against_oracle(what, least):
        worst = 0.0
        for m, o in enumerate(oracles):
            mask = o.trusted_mask(below_start_key=True)
            assert int(mask.sum()) > least
            a, ref = b.read_field(m)[mask], o.g()[mask]
            err = np.abs(a.astype(np.float64) - ref)
            assert dfm_close(a, ref), "%s map %d: max rel %.3g" % (what, m, float((err / ref.clip(1)).max()))
            worst = max(worst, float((err / ref.clip(1)).max()))
        return worst
    against_oracle("plan", 3_000_000)
    for k in range(n):
        assert np.isfinite(b.read_field(k)[int(start[0]), int(start[1])])
    paths = b.extract_paths(max_steps=20)
    assert len(paths) == n and all(len(pt[0]) >= 2 and pt[2] > 0 for pt in paths)
    worst = 0.0
    for i in range(rounds):
        for m in range(n):
            k, s, top, left, patch = scripts[m][i]
            b.patch_map(m, patch, top, left); b.set_start(m, *s)
            oracles[m].patch_map(patch, top, left); oracles[m].set_start(*s)
            assert oracles[m].step() == 0
        assert b.step() == 0
        if (i + 1) % 10 == 0:
            worst = max(worst, against_oracle("round %d" % (i + 1), 2_000_000))
    assert b.check_layout() == (0, 0)
    print("config 4: 8 maps x 100 rounds, largest relative deviation from the oracle %.3g" % worst)
    b.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 1), ("SG", 2), ("DFM", 1)])
def test_back_pointer_view(algo, lvl):
    """ufm_read_info: the reference's INFO (back-pointers of the level-1/2 planners).  Three views of it, after a plan and
    some replans: the engine's STORED ones (one byte per element, written with every value; the invalidation follows them),
    the ones the engine DERIVES from the field alone, and the oracle's min_rhs<level> evaluated on the very same field
    (loaded into the oracle).  Derived == oracle element by element.  Stored: every element the step finalised has one,
    and the candidate it names reproduces the element's value bit for bit (orc_cost_via); it names the same neighbour as
    the derived view except where two candidates tie.  A level-0 planner has no Info."""
    width, length = 120, 88
    cost = ufm_amd.synth.cost_map(17, width, length)
    start, goal = ufm_amd.synth.start_goal(width, length)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    assert g.step() == 0 and o.step() == 0
    for k, s, top, left, patch in ufm_amd.synth.replan_script(17, width, length, n_patches=3, size=15):
        g.patch_map(patch, top, left); o.patch_map(patch, top, left)
        g.set_start(*s); o.set_start(*s)
        assert g.step() == 0 and o.step() == 0
    final = o.trusted_mask(below_start_key=True)      # what the planners guarantee final
    field = g.g()
    o.load_g(field)                       # same raster (patched above), same field
    ref = o.info_field()
    got = g.read_info(derived=True)
    assert got.shape == ref.shape
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, "%d of %d elements differ, first %r: engine %r oracle %r" % (
        len(bad), got.shape[0] * got.shape[1], tuple(bad[0]), got[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    # the view says something: most reached elements have a back-pointer
    assert (got[..., 0] >= 0).sum() > 0.8 * np.isfinite(field).sum()
    # ---- the stored back-pointers ----
    sto = g.read_info()
    gx, gy = int(round(goal[0])), int(round(goal[1]))
    check = final & np.isfinite(field)
    check[gx, gy] = False                 # the goal has none
    assert (sto[..., 0][check] >= 0).all(), "%d finalised elements without a stored back-pointer" % int((sto[..., 0][check] < 0).sum())
    same = (sto == got).all(axis=2)
    # Ties are structural (along a grid edge both triangles over that edge cost g1 + min(c, b)): round 3 kept the lowest code among tied candidates and
    # the two views parted on 7-8 % of the nodes.  Round 4: the tied candidate the reference's min_rhs<1>() keeps -- the last in neighbors_8 order -- so
    # for the level-1 node planners stored == derived, element by element.  (SG level 2 derives its back-pointer from another candidate structure,
    # ShiftedGridPlanner_impl.h:280-303; MS-DFM keeps the lowest code: there the two views may still part at ties.)
    if (algo, lvl) in (("FD", 1), ("SG", 1)):
        assert same[check].all(), "stored and derived back-pointers differ on %d of %d finalised elements, first %r" % (
            int((~same[check]).sum()), int(check.sum()), tuple(np.argwhere(check & ~same)[0]))
    else:
        assert same[check].mean() > 0.8, "stored and derived back-pointers agree on only %.3f of the finalised elements" % same[check].mean()
    ey = field.shape[1]
    n_tie = 0
    for x, y in np.argwhere(check):       # the named candidate reproduces the value (all of them; the ties are the interesting ones)
        b0, b1 = int(sto[x, y, 0]), int(sto[x, y, 1])
        if ALGOS[algo] == 2:              # DFM: one of the eight level-1 candidates leaves this pair and gives this value
            ok = False
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    if (dx or dy) and 0 <= x + dx < field.shape[0] and 0 <= y + dy < ey:
                        c, a0, a1 = o.cost_via(x, y, x + dx, y + dy)
                        ok = ok or (a0 == b0 and a1 == b1 and abs(c - float(field[x, y])) <= DFM_RTOL * float(field[x, y]))
            assert ok, "DFM cell (%d, %d): no level-1 candidate leaves the stored pair (%d, %d) with value %r" % (x, y, b0, b1, float(field[x, y]))
        else:
            c, a0, _a1 = o.cost_via(x, y, b0 // ey, b0 % ey)
            assert a0 == b0 and c == float(field[x, y]), "node (%d, %d): stored parent %d gives %r, the field holds %r" % (x, y, b0, c, float(field[x, y]))
        n_tie += 0 if same[x, y] else 1
    print("%s-%d: %d finalised elements, stored == derived on all but %d (ties)" % (algo, lvl, int(check.sum()), n_tie))
    # a window equals the same part of the whole
    win = g.read_info(10, 20, 30, 40, derived=True)
    assert np.array_equal(win, got[10:40, 20:60])
    assert np.array_equal(g.read_info(10, 20, 30, 40), sto[10:40, 20:60])
    z = ufm_amd.Planner(ALGOS[algo], 0)
    z.set_occupancy_threshold(1); z.set_map(cost); z.set_start(*start); z.set_goal(*goal)
    assert z.step() == 0
    with pytest.raises(ufm_amd.UfmError):
        z.read_info()
    z.close(); g.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)])
def test_random_small_maps_with_obstacles_and_patches(algo, lvl):
    """Seeded random cases at awkward sizes: white-noise costs (no smoothness at all), 15 % obstacle
    cells, random start / goal, random rectangular patches that add and remove obstacles, thresholds
    below 1.  Every step is compared with the oracle (and the extracted path on the same field)."""
    rng = np.random.default_rng(20260 + lvl)
    n_cases = 14
    for case in range(n_cases):
        width, length = int(rng.integers(2, 70)), int(rng.integers(2, 70))
        cost = rng.integers(1, 255, (length, width), dtype=np.uint8)
        cost[rng.random((length, width)) < 0.15] = 255
        thr = float(rng.choice([1.0, 1.0, 0.9, 0.6]))
        free = np.argwhere(cost < int(thr * 255))
        if len(free) < 2:
            continue
        a, b = free[rng.integers(len(free))], free[rng.integers(len(free))]
        start, goal = (float(a[0]), float(a[1])), (float(b[0]), float(b[1]))
        heur = bool(case % 3 == 0) and algo != "DFM"
        o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, thr=thr, heuristic=heur, hm=1.0)
        what = "%s case %d (%dx%d thr %.1f heur %d)" % (algo, case, width, length, thr, heur)
        assert o.step() == 0 and g.step() == 0
        check_parity(o, g, what, below_start_key=True)
        cur = cost.copy()
        for k in range(4):
            ph, pw = int(rng.integers(1, min(length, 20) + 1)), int(rng.integers(1, min(width, 20) + 1))
            top, left = int(rng.integers(0, length - ph + 1)), int(rng.integers(0, width - pw + 1))
            patch = rng.integers(1, 255, (ph, pw), dtype=np.uint8)
            patch[rng.random((ph, pw)) < 0.15] = 255
            cur[top:top + ph, left:left + pw] = patch
            free = np.argwhere(cur < int(thr * 255))
            a = free[rng.integers(len(free))] if len(free) else np.array([0, 0])
            s = (float(a[0]), float(a[1]))
            for p in (o, g):
                p.patch_map(patch, top, left)
                p.set_start(*s)
                assert p.step() == 0
            assert g.num_nodes_updated == o.num_updated, what
            check_parity(o, g, what + " patch %d" % k, below_start_key=True)
            dev = g.extract_path(max_steps=30, allow_indirect=(algo != "SG"))
            ref = orc.extract_path_field(g.read_field()[1], algo == "DFM", cur, int(thr * 255), s, goal,
                                         max_steps=30, allow_indirect=(algo != "SG"))
            assert np.array_equal(dev[0], ref[0]) and np.array_equal(dev[1], ref[1]) and dev[2] == ref[2], what
        assert np.array_equal(g.read_map(width, length), cur)
        g.close()


@pytest.mark.parametrize("algo,lvl", [("FD", 1), ("SG", 2), ("DFM", 1)])
def test_patches_on_tile_corners_keep_the_layout_copies_sound(algo, lvl):
    """The engine keeps per-tile copies of cost bytes (a cell on a tile edge belongs to up to four windows)
    and of neighbours' border values.  Single-cell and 2x2 patches on and around tile corners, map corners
    included, must leave every copy equal to its original (ufm_check_layout, asserted inside check_parity)
    and the field equal to the oracle's."""
    width, length = 83, 70          # not multiples of the tile edge
    rng = np.random.default_rng(7)
    cost = rng.integers(1, 60, (length, width), dtype=np.uint8)
    o, g = make_pair(ALGOS[algo], lvl, cost, (3.0, 4.0), (float(length - 3), float(width - 4)))
    assert o.step() == 0 and g.step() == 0
    check_parity(o, g, "%s plan" % algo)
    spots = [(0, 0), (15, 15), (16, 16), (15, 16), (31, 32), (32, 31), (47, 48), (63, 64), (length - 1, width - 1),
             (length - 2, 15), (16, width - 2), (48, 79)]
    cur = cost.copy()
    for k, (x, y) in enumerate(spots):
        h, w = (1, 1) if k % 2 == 0 else (min(2, length - x), min(2, width - y))
        patch = np.full((h, w), 200 if k % 3 else 2, dtype=np.uint8)
        cur[x:x + h, y:y + w] = patch
        for p in (o, g):
            p.patch_map(patch, x, y)
            p.set_start(3.0 + (k % 3), 4.0)
            assert p.step() == 0
        n, nbad = check_parity(o, g, "%s patch at (%d,%d)" % (algo, x, y), below_start_key=True)
        if algo != "DFM":
            assert nbad == 0
    assert np.array_equal(g.read_map(width, length), cur)
    g.close()


def test_heuristic_multiplier_per_move_does_not_re_instantiate_graphs():
    """The reference harness sends a new min_cost with every move (Tests/Planners/DFM/main.cpp:111-112 ->
    set_heuristic_multiplier).  The multiplier (like the occupancy threshold) reaches the kernels through device
    memory, not through the captured graphs' frozen arguments: a replan with a new multiplier replays an existing
    graph.  Fields are checked against the oracle, which gets the same multipliers."""
    width = length = 224
    seed = 31
    cost = ufm_amd.synth.cost_map(seed, width, length)
    start, goal = (60.0, 70.0), (float(length - 8), float(width - 8))
    o, g = make_pair(ALGOS["FD"], 1, cost, start, goal, heuristic=True, hm=1.0)
    assert o.step() == 0 and g.step() == 0
    counts = []
    sx, sy = start
    for k in range(1, 25):
        top, left = int(sx) - 15 + 3 * k, int(sy) - 15 + 2 * k
        patch = (1 + (ufm_amd.synth.h64(seed ^ k, *np.meshgrid(np.arange(top, top + 31), np.arange(left, left + 31), indexing="ij")) % np.uint64(200))).astype(np.uint8)
        hm = 1.0 - 0.02 * (k % 7)            # a different multiplier every move
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_heuristic_multiplier(hm)
            p.set_start(sx + 3 * k, sy + 2 * k)
            assert p.step() == 0
        n, nbad = check_parity(o, g, "hm %.2f replan %d" % (hm, k), below_start_key=True)
        assert nbad == 0
        counts.append(g.stats.graphs_instantiated)
    # graphs are keyed by the launch counts of a submission (what recent replans needed) and by nothing else: far
    # fewer graphs than replans, although every one of the 24 replans came with a new multiplier
    assert counts[-1] <= 10, counts
    g.close()


def test_absurd_map_size_fails_cleanly_and_the_handle_survives():
    """hipMalloc failure half way through alloc(): a negative code, nothing aborts, nothing leaks into the next
    set_map (which works), destroy is clean."""
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    L = g.L
    dummy = np.zeros(16, np.uint8)
    rc = L.ufm_set_map(g.h, dummy.ctypes.data, 400000, 400000)      # 160 G cells: 640 GB for G alone
    assert rc < 0 and rc != ufm_amd.LOOP_FAILURE_NO_GRAPH
    assert g.step() == ufm_amd.LOOP_FAILURE_NO_GRAPH               # still no map
    cost = ufm_amd.synth.cost_map(3, 96, 96)
    g.set_occupancy_threshold(1); g.set_map(cost); g.set_start(8.0, 8.0); g.set_goal(88.0, 88.0)
    assert g.step() == 0 and np.isfinite(g.g()[8, 8])
    g.close()


@pytest.mark.parametrize("defer", [0, 1])
def test_batch_device_inputs_and_sharded_handle(defer):
    """ufm_batch_set_map_device / ufm_batch_patch_map_device (HBM pointers, e.g. a buffer an RCCL broadcast
    filled) and ufm_batch_create_sharded (here: two engines on the one device of the box, devices = [0, 0]; on a
    node each shard gets its own GPU and ufm_batch_step advances them side by side) give the fields of a
    one-engine batch fed from host memory, bit for bit (FD, full-field mode).
    defer = 0 (the default): a patch is read at the call, stream-ordered -- its buffer is overwritten here before the step.
    defer = 1 (opt-in "defer_patches": one apply launch per round; the buffers stay untouched until the step has returned)."""
    n, size = 4, 160
    costs = [ufm_amd.synth.cost_map(50 + i, size, size) for i in range(n)]
    start, goal = ufm_amd.synth.start_goal(size, size)
    scripts = [list(ufm_amd.synth.replan_script(50 + i, size, size, n_patches=3)) for i in range(n)]
    a = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1)
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, devices=[0, 0])
    assert b.shards() == 2 and a.shards() == 1
    d_costs = [DeviceBytes(c) for c in costs]
    for p in (a, b):
        p.set_param("focused", 0); p.set_occupancy_threshold(1)
    b.set_param("defer_patches", defer)
    for i in range(n):
        a.set_map(i, costs[i]); b.set_map_device(i, d_costs[i].data_ptr(), size, size)
        for p in (a, b):
            p.set_start(i, *start); p.set_goal(i, *goal)
    assert a.step() == 0 and b.step() == 0
    assert b.stats.expanded == a.stats.expanded
    for r in range(3):
        keep = []
        for i in range(n):
            k, s, top, left, patch = scripts[i][r]
            dp = DeviceBytes(patch); keep.append(dp)
            a.patch_map(i, patch, top, left); b.patch_map_device(i, dp.data_ptr(), top, left, 31, 31)
            if r == 1 and i == 0:      # a second patch of the same map that overlaps the first (device patches are held back until
                p2 = np.ascontiguousarray(patch[::-1, ::-1][:20, :17])      # the step: their order must survive that)
                dp2 = DeviceBytes(p2); keep.append(dp2)
                a.patch_map(i, p2, top + 5, left + 7); b.patch_map_device(i, dp2.data_ptr(), top + 5, left + 7, 17, 20)
            for p in (a, b):
                p.set_start(i, *s)
        if not defer:                  # the ABI's lifetime: the call has read (queued the read of) the buffer -- what happens to it afterwards is the caller's business
            for dp in keep:
                dp.overwrite(np.full(dp.nbytes, 77, np.uint8))
        if r == 2:                     # a read of the raster between patch and step sees the patch
            assert np.array_equal(a.read_map(1, size, size), b.read_map(1, size, size))
        assert a.step() == 0 and b.step() == 0
        assert b.stats.updated == a.stats.updated
        for i in range(n):
            assert np.array_equal(a.read_field(i), b.read_field(i)), (r, i)
            assert np.array_equal(a.read_map(i, size, size), b.read_map(i, size, size))
    assert b.check_layout() == (0, 0)
    pa, pb = a.extract_paths(max_steps=10), b.extract_paths(max_steps=10)
    for x, y in zip(pa, pb):
        assert np.array_equal(x[0], y[0]) and x[2] == y[2]
    a.close(); b.close()
    for d in d_costs:
        d.free()
