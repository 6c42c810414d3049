"""-m gpu: MS-DFM level 1's stored back-pointer bytes -- the self-check of them (ufm_check_info) and the invalidation that follows them
(ufm_set_param "dfm_follow_info", opt-in), against the CPU oracle."""
import numpy as np
import pytest

import ufm_amd
import oracle_py as orc
from helpers import DFM_RTOL, dfm_close, ulp_diff

pytestmark = pytest.mark.gpu

DFM = ufm_amd.ALGO_DFM
SLACK_ULP = 8          # what the MS-DFM invalidation and ufm_check_info allow between a value and its candidate


def make_dfm_pair(size, seed, heuristic=False, follow=False, region=1, focused=1):
    cost = ufm_amd.synth.cost_map(seed, size, size)
    start, goal = ufm_amd.synth.start_goal(size, size)
    o = orc.OraclePlanner(DFM, 1, heuristic)
    g = ufm_amd.Planner(DFM, 1, heuristic, follow_info=follow)
    g.set_param("region", region)
    g.set_param("focused", focused)
    for p in (o, g):
        p.reset()
        p.set_occupancy_threshold(1.0)
        p.set_heuristic_multiplier(1.0)
        p.set_map(cost)
        p.set_start(*start)
        p.set_goal(*goal)
    return o, g, cost, start, goal


def valued_elements(field, goal):
    gx, gy = int(round(goal[0])), int(round(goal[1]))
    return int(np.isfinite(field).sum()) - (1 if np.isfinite(field[gx, gy]) else 0)


def check_bytes(g, goal, what):
    ci = g.check_info()
    assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)
    assert ci[0] == valued_elements(g.g(), goal), "%s: %d elements checked, the field holds %d values" % (what, ci[0], valued_elements(g.g(), goal))


def queue_below_start_key(o, g):
    """the elements the queue view holds below the start's key (with the MS-DFM slack check_parity uses)"""
    xy, qg, qrhs, total = g.read_queue()
    skey = o.start_key()
    if not total or not np.isfinite(skey):
        return 0
    k = np.minimum(qg, qrhs)
    if o.use_heuristic:
        sx, sy = o._start_xy()
        k = (k + np.float32(o.hm) * np.hypot(np.float32(sx) - xy[:, 0].astype(np.float32),
                                            np.float32(sy) - xy[:, 1].astype(np.float32)).astype(np.float32)).astype(np.float32)
    return int((k < skey - DFM_RTOL * skey).sum())


def against_oracle(o, g, goal, what):
    mask = o.trusted_mask(below_start_key=True)
    assert int(mask.sum()) > 1000, what
    assert dfm_close(g.g()[mask], o.g()[mask], what=what), "%s: field differs from the oracle beyond DFM_RTOL" % what
    assert g.check_layout() == (0, 0), what
    check_bytes(g, goal, what)
    assert queue_below_start_key(o, g) == 0, "%s: elements wait below the start's key" % what


@pytest.mark.parametrize("size", [512, 1024])
def test_check_info_dfm_level1(size):
    """ufm_check_info on MS-DFM level 1 (the default invalidation): after the plan and after each of 20 replans every element with a value
    has a byte, the candidate it names gives the value within 8 ulp and, below the start's key, its dependence bits leave out no cell it
    leans on beyond that.  A level-0 planner has no bytes: UfmError."""
    seed = 7
    o, g, cost, start, goal = make_dfm_pair(size, seed)
    assert g.step() == 0
    check_bytes(g, goal, "plan")
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=20):
        g.patch_map(patch, top, left)
        g.set_start(*s)
        assert g.step() == 0
        check_bytes(g, goal, "replan %d" % k)
    g.close()
    z = ufm_amd.Planner(DFM, 0)
    z.set_occupancy_threshold(1); z.set_map(cost); z.set_start(*start); z.set_goal(*goal)
    assert z.step() == 0
    with pytest.raises(ufm_amd.UfmError):
        z.check_info()
    z.close()


def test_follow_info_knob():
    """"dfm_follow_info": accepted on MS-DFM level 1 and (without effect) on the node planners; refused on MS-DFM level 0, single and batch"""
    for algo, lvl in ((DFM, 1), (ufm_amd.ALGO_FD, 0), (ufm_amd.ALGO_FD, 1), (ufm_amd.ALGO_SG, 1), (ufm_amd.ALGO_SG, 2)):
        p = ufm_amd.Planner(algo, lvl)
        p.set_param("dfm_follow_info", 1)
        p.set_param("dfm_follow_info", 0)
        p.close()
    z = ufm_amd.Planner(DFM, 0)
    with pytest.raises(ufm_amd.UfmError):
        z.set_param("dfm_follow_info", 1)
    z.set_param("dfm_follow_info", 0)
    z.close()
    b = ufm_amd.BatchPlanner(2, DFM, 1)
    b.set_param("dfm_follow_info", 1)
    b.close()
    b = ufm_amd.BatchPlanner(2, DFM, 0)
    with pytest.raises(ufm_amd.UfmError):
        b.set_param("dfm_follow_info", 1)
    b.close()


@pytest.mark.parametrize("heuristic", [False, True])
@pytest.mark.parametrize("region", [1, 0])
def test_follow_info_parity(region, heuristic):
    """The knob on, 1024^2, a plan and 50 replans, each against the oracle: field within DFM_RTOL on what the oracle guarantees final, layout
    and byte self-checks, nothing queued below the start's key.  region 1: the block kernel's dead test (plus the seeded patches' own
    candidate); region 0: the launch chain's evaluation of the element's own candidate, alone."""
    size, seed = 1024, 21
    o, g, cost, start, goal = make_dfm_pair(size, seed, heuristic=heuristic, follow=True, region=region)
    assert o.step() == 0 and g.step() == 0
    against_oracle(o, g, goal, "plan")
    raise_visits, regions0 = 0, g.stats.region_replans
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=50):
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
        raise_visits += g.stats.raise_tile_visits
        against_oracle(o, g, goal, "replan %d" % k)
    if region:
        assert g.stats.region_replans > regions0       # the replans went through the block kernel
    else:
        assert g.stats.region_replans == regions0 and raise_visits > 0      # ... through the launch chain's invalidation
    g.close()


def test_follow_info_changes_the_invalidation():
    """The knob is not just accepted: the launch chain's invalidation (region 0) takes other values away with it -- also the ones whose named
    cell went while another candidate still gives them (the reference's level-1 rule), and not the ones whose other candidates moved.  Same
    map, same script, the default run twice: the invalidation tile visits with the knob on differ from the default's by well more than the
    default's own spread from run to run."""
    size, seed = 512, 21
    visits = []
    for follow in (0, 1, 0):
        o, g, cost, start, goal = make_dfm_pair(size, seed, follow=bool(follow), region=0)
        assert g.step() == 0
        n = 0
        for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=40):
            g.patch_map(patch, top, left)
            g.set_start(*s)
            assert g.step() == 0
            n += g.stats.raise_tile_visits
        check_bytes(g, goal, "follow %d" % follow)
        g.close()
        visits.append(n)
    off1, on, off2 = visits
    print("invalidation tile visits, knob off / on / off: %d / %d / %d" % (off1, on, off2))
    assert off1 > 0 and abs(on - off1) > 3 * max(abs(off2 - off1), 4)


def test_follow_info_batch():
    """The knob on a batch: 8 x 1024^2 (seeds 1000..1007), 30 rounds, every map against its oracle every 10 rounds, the byte self-check
    after every round, paths from every start.  And a handle of two engines on the one device (ufm_batch_create_sharded)."""
    n, size, rounds = 8, 1024, 30
    start, goal = ufm_amd.synth.start_goal(size, size)
    costs = [ufm_amd.synth.cost_map(1000 + i, size, size) for i in range(n)]
    scripts = [list(ufm_amd.synth.replan_script(1000 + i, size, size, n_patches=rounds)) for i in range(n)]

    def run(b, n_maps, n_rounds, check_every):
        oracles = []
        b.set_occupancy_threshold(1.0)
        for i in range(n_maps):
            b.set_map(i, costs[i]); b.set_start(i, *start); b.set_goal(i, *goal)
            o = orc.OraclePlanner(DFM, 1, False)
            o.reset(); o.set_occupancy_threshold(1.0); o.set_map(costs[i]); o.set_start(*start); o.set_goal(*goal)
            assert o.step() == 0
            oracles.append(o)
        assert b.step() == 0
        for r in range(n_rounds):
            for i, o in enumerate(oracles):
                k, s, top, left, patch = scripts[i][r]
                b.patch_map(i, patch, top, left); b.set_start(i, *s)
                o.patch_map(patch, top, left); o.set_start(*s)
                assert o.step() == 0
            assert b.step() == 0
            ci = b.check_info()
            assert ci[1:4] == (0, 0, 0), "round %d: back-pointer self-check %r" % (r, ci)
            if (r + 1) % check_every == 0 or r == n_rounds - 1:
                for i, o in enumerate(oracles):
                    mask = o.trusted_mask(below_start_key=True)
                    assert int(mask.sum()) > 1000
                    assert dfm_close(b.read_field(i)[mask], o.g()[mask], what="batch"), "round %d: map %d differs from its oracle" % (r, i)
                assert b.check_layout() == (0, 0)
        for i, (pts, step_costs, total_cost, _dist) in enumerate(b.extract_paths(max_steps=20)):
            s = scripts[i][n_rounds - 1][1]
            assert len(pts) > 1 and np.isfinite(total_cost), "map %d: no path" % i
            assert tuple(pts[0]) == (np.float32(s[0]), np.float32(s[1])), "map %d: the path starts at %r, not at the start %r" % (i, tuple(pts[0]), s)

    b = ufm_amd.BatchPlanner(n, DFM, 1, follow_info=True)
    run(b, n, rounds, 10)
    assert b.stats.region_replans > 0
    b.close()
    b = ufm_amd.BatchPlanner(4, DFM, 1, devices=[0, 0], follow_info=True)
    assert b.shards() == 2
    run(b, 4, 10, 5)
    b.close()


def test_stored_dfm_parents_are_real():
    """A converged 256^2 field after a few replans (the knob on), loaded into the oracle: for every element with a value, one of its eight
    neighbours carries the level-1 candidate (orc_cost_via, min_rhs_decreased_neighbor) that leaves exactly the pair of cells ufm_read_info
    reports from the stored byte -- the axis neighbour and the perpendicular cell bit 5 names -- and gives the element's value within 8 ulp."""
    size, seed = 256, 5
    o, g, cost, start, goal = make_dfm_pair(size, seed, follow=True, focused=0)
    assert g.step() == 0 and o.step() == 0
    for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=4, size=21):
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
    check_bytes(g, goal, "after the replans")
    field = g.g()
    o.load_g(field)
    sto = g.read_info()
    gx, gy = int(round(goal[0])), int(round(goal[1]))
    check = np.isfinite(field)
    check[gx, gy] = False
    assert check.sum() > 0.9 * size * size
    n_pair = 0
    for x, y in np.argwhere(check):
        b0, b1 = int(sto[x, y, 0]), int(sto[x, y, 1])
        assert b0 >= 0, "cell (%d, %d) has a value and no stored parent" % (x, y)
        gv = np.float32(field[x, y])
        ok = False
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if (dx or dy) and 0 <= x + dx < size and 0 <= y + dy < size:
                    c, a0, a1 = o.cost_via(x, y, x + dx, y + dy)
                    if a0 == b0 and a1 == b1 and np.isfinite(c):
                        ok = ok or int(ulp_diff(np.array([c], np.float32), np.array([gv]))[0]) <= SLACK_ULP
        assert ok, "cell (%d, %d): no level-1 candidate leaves the stored pair (%d, %d) with value %r within %d ulp" % (
            x, y, b0, b1, float(gv), SLACK_ULP)
        n_pair += 1 if b1 >= 0 else 0
    assert n_pair > 0.5 * check.sum()      # most values come from the quadratic case: the perpendicular cell is part of the pair
    g.close()
