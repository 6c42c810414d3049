"""-m gpu: k_extract_path case by case.  The directed inputs of tests/path_cases.py, planned by the engine itself (full field:
`focused = 0`), extracted on the device from every start and held

* bit for bit to the oracle's extractor run on the device's own field (way points, step costs, totals), through the single handle
  and -- the same map with many starts as one batch -- through one launch of ufm_batch_extract_path;
* to the census of those very oracle runs: the floors of path_cases.census_shortfalls(), so that the equality above is known to have
  covered every reachable case, orientation, ring slot and special branch;
* to the float64 reference of the operation (path_cases.polyline_reference), under the same derived bound as the oracle's extractor
  (tests/test_path_cases.py).

Plus the buffers' capacities around the three-point / two-cost move and the walk that gets stuck after a real move."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as orc
import path_cases as pc
import ufm_amd
from test_gpu_path import same_path

pytestmark = pytest.mark.gpu


def device_planner(algo, cost, thr, lvl=0):
    g = ufm_amd.Planner(pc.ALGOS[algo], lvl)
    g.reset()
    g.set_param("focused", 0)       # every start reads a final field
    g.set_occupancy_threshold(thr)
    g.set_map(cost)
    g.set_start(*pc.plan_start(cost))
    g.set_goal(*pc.GOAL)
    assert g.step() == 0
    return g


def thr_uchar(thr):
    return int(np.float32(thr) * np.float32(255.0))     # Graph.cpp:18-20


@pytest.fixture(scope="module")
def survey():
    """every directed extraction on the device, once, next to the oracle's extractor on the device's field"""
    out = {"census": {}, "worst": {}, "differing": [], "violations": [], "extractions": 0, "field_differs": {}}
    for algo in ("FD", "SG", "DFM"):
        total = {}
        for name, cost, thr, jobs in pc.extraction_plan(algo):
            g = device_planner(algo, cost, thr)
            field = g.read_field()[1]
            tu = thr_uchar(thr)
            ofield, otu = pc.oracle_field(algo, cost, thr)
            assert otu == tu
            out["field_differs"][(algo, name)] = int((field != ofield).sum())
            orc.path_census_reset()
            for start, la in jobs:
                kw = dict(max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=pc.INDIRECT[algo])
                g.set_start(*start)
                dev = g.extract_path(**kw)
                ref = orc.extract_path_field(field, algo == "DFM", cost, tu, start, pc.GOAL, **kw)
                moves = orc.path_move_log()
                out["extractions"] += 1
                what = "%s %s start %r lookahead %d" % (algo, name, start, la)
                try:
                    same_path(dev, ref, what)
                    assert g.path_info.steps == len(moves), "%s: %d moves, the oracle made %d" % (what, g.path_info.steps, len(moves))
                except AssertionError as e:
                    out["differing"].append(str(e))
                    continue
                if len(dev[0]) == 0:
                    continue
                try:
                    for k, t, dev_, bound in pc.polyline_reference(dev, moves, cost, tu, pc.INDIRECT[algo]):
                        key = (orc.PC_KINDS[k], orc.PC_TYPES[t])
                        if key not in out["worst"] or dev_ / bound > out["worst"][key][0] / out["worst"][key][1]:
                            out["worst"][key] = (dev_, bound)
                except AssertionError as e:
                    out["violations"].append("%s: %s" % (what, e))
            pc.add_census(total, orc.path_census())
            g.close()
        out["census"][algo] = total
    return out


def test_directed_paths_equal_the_oracle_on_the_device_field(survey):
    assert survey["extractions"] > 5000
    assert not survey["differing"], "%d of %d extractions differ from the oracle's extractor, first: %s" % (
        len(survey["differing"]), survey["extractions"], survey["differing"][0])


def test_census_of_the_device_field_runs_meets_the_floors(survey):
    """FD / SG fields are bit-equal to the oracle's in full-field mode, so their census is the CPU test's; MS-DFM fields are only
    close (2e-6), a case may tip: half the floor"""
    c = survey["census"]
    both = pc.add_census(pc.add_census({}, c["FD"]), c["DFM"])
    print("\n%d extractions; field elements that differ from the oracle's: %r\n%s" % (
        survey["extractions"], {k: v for k, v in survey["field_differs"].items() if v}, pc.census_table(both, c["SG"], survey["worst"])))
    for algo, scale in (("FD", 1.0), ("DFM", 0.5)):
        bad = pc.census_shortfalls(c[algo], c["SG"], scale, stuck=(algo == "DFM"))
        assert not bad, "%s + SG on the device's fields: the directed inputs miss %s" % (algo, "; ".join(bad))
    for algo in c:
        for o in orc.PC_ORIENT:
            assert c[algo]["chosen"][("opposite", "B", o)] == 0


def test_device_paths_against_the_float64_reference(survey):
    assert len(survey["worst"]) == 14
    assert not survey["violations"], "%d extractions off the float64 reference, first: %s" % (len(survey["violations"]), survey["violations"][0])


@pytest.mark.parametrize("algo", ["FD", "DFM"])
def test_directed_paths_one_batch_launch(algo):
    """the same map in every slot of a batch, a different start per slot: one launch of ufm_batch_extract_path per 16 starts, each
    path equal to the oracle's extractor on that slot's field"""
    n = 16
    for name, cost, thr, jobs in pc.extraction_plan(algo)[::3]:
        b = ufm_amd.BatchPlanner(n, pc.ALGOS[algo], 1)
        b.set_param("focused", 0)
        b.set_occupancy_threshold(thr)
        for m in range(n):
            b.set_map(m, cost)
            b.set_start(m, *pc.plan_start(cost))
            b.set_goal(m, *pc.GOAL)
        assert b.step() == 0
        fields = [b.read_field(m) for m in range(n)]
        tu = thr_uchar(thr)
        for la in (True, False):
            starts = [s for s, l in jobs if l == la]
            for k in range(0, len(starts), n):
                chunk = (starts[k:k + n] + starts[:n])[:n]
                for m, s in enumerate(chunk):
                    b.set_start(m, *s)
                kw = dict(max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=pc.INDIRECT[algo])
                paths = b.extract_paths(**kw)
                for m, s in enumerate(chunk):
                    ref = orc.extract_path_field(fields[m], algo == "DFM", cost, tu, s, pc.GOAL, **kw)
                    same_path(paths[m], ref, "%s %s batch slot %d start %r lookahead %d" % (algo, name, m, s, la))
        b.close()


CANARY = np.float32(-7777.0)


def test_capacity_around_the_three_point_move():
    """cap_pts ending before the first, the second, the third point of a three-point move and behind it, cap_costs before, inside and
    behind its two step costs: counted, not stored, nothing written beyond the capacity"""
    done = 0
    for algo, name, start, la in pc.found_inputs():
        if algo != "FD" or done >= 4:
            continue
        cost, thr = pc.map_by_name(name)
        g = device_planner(algo, cost, thr)
        g.set_start(*start)
        full = g.extract_path(max_steps=pc.MAX_STEPS, lookahead=la)
        ref = orc.extract_path_field(g.read_field()[1], False, cost, thr_uchar(thr), start, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la)
        moves = orc.path_move_log()
        same_path(full, ref, "capacity: full path")
        three = [i for i, mv in enumerate(moves) if mv[0] == 3]
        if not three:
            g.close()
            continue
        ip, ic = 1 + int(moves[:three[0], 0].sum()), int(moves[:three[0], 1].sum())
        assert moves[three[0]][1] == 2
        for cap_p, cap_c in [(ip + d, ic + e) for d in (0, 1, 2, 3) for e in (0, 1, 2)]:
            pts = np.full((cap_p + 8, 2), CANARY, np.float32)
            costs = np.full(cap_c + 8, CANARY, np.float32)
            info = ufm_amd.capi.PathInfo()
            rc = g.L.ufm_extract_path(g.h, pc.MAX_STEPS, int(la), 1, pts.ctypes.data, cap_p, costs.ctypes.data, cap_c, C.byref(info))
            assert rc == 0
            what = "cap_pts %d cap_costs %d (three-point move at point %d, cost %d)" % (cap_p, cap_c, ip, ic)
            assert info.n_points == len(full[0]) and info.n_costs == len(full[1]), what
            assert info.total_cost == full[2] and info.total_dist == full[3] and info.steps == len(moves), what
            assert np.array_equal(pts[:cap_p], full[0][:cap_p]) and np.array_equal(costs[:cap_c], full[1][:cap_c]), what
            assert (pts[cap_p:] == CANARY).all() and (costs[cap_c:] == CANARY).all(), what + ": written beyond the capacity"
        done += 1
        g.close()
    assert done >= 2, "no found input of Field D* holds a three-point move any more (tests/golden/search_path_cases.py)"


def test_stuck_after_a_move_repeats_the_step_cost():
    """a walk that stays put after k >= 1 real moves: the reference adds the previous move's step cost again with every further step
    (its step_cost is left untouched) -- the kernel's loop-carried step_cost does the same: totals equal the oracle's"""
    done = 0
    for algo, name, start, la in pc.found_inputs():
        cost, thr = pc.map_by_name(name)
        g = None
        try:
            tu = thr_uchar(thr)
            g = device_planner(algo, cost, thr)
            g.set_start(*start)
            kw = dict(max_steps=pc.MAX_STEPS, lookahead=la, allow_indirect=pc.INDIRECT[algo])
            dev = g.extract_path(**kw)
            ref = orc.extract_path_field(g.read_field()[1], algo == "DFM", cost, tu, start, pc.GOAL, **kw)
            moves = orc.path_move_log()
            stuck = [i for i, mv in enumerate(moves) if mv[0] == 0 and i > 0 and moves[:i, 0].sum() > 0]
            if not stuck:
                continue
            same_path(dev, ref, "stuck walk %s %s %r" % (algo, name, start))
            assert g.path_info.steps == pc.MAX_STEPS == len(moves)
            assert len(dev[0]) == 1 + int(moves[:, 0].sum())
            if float(dev[1][-1]) > 0:
                assert dev[2] > float(np.sum(dev[1], dtype=np.float64)) * (1 + 1e-6), "the step cost was not added again"
            done += 1
        finally:
            if g is not None:
                g.close()
    assert done >= 5, "only %d found inputs get stuck after a move on the device's fields" % done
