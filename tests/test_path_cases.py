"""The path extractor's case tables, case by case, on the CPU: the oracle's extractor (oracle/ufm_path_oracle.c) over the directed
inputs of tests/path_cases.py, counted by its census and held to a float64 reference of the operation itself.

tests/test_gpu_path_cases.py runs the same inputs on the device; this file shows that the inputs reach every case (so that the
bit-for-bit comparison there covers every case and is not merely assumed to) and that the closed forms the oracle and the kernel
share describe the way points they return.

Measured on the oracle (every directed extraction of FD, SG and DFM: 12 744 extractions, 76 139 moves; `pytest -s` prints the table
with every run) -- won as indirect (FD + DFM) h / v and direct (SG) h / v, and the worst |sum of a move's step costs - float64 cost of
its way points| per case with the bound path_cases.move_bound() derives for that very move:

    case             won, indirect h / v    won, direct h / v    worst deviation (its bound)
    corner I         650 / 723              -                    1.68e-07 (6.29e-06)
    corner II        1862 / 1830            1472 / 1479          5.40e-06 (1.99e-05)
    corner III       5103 / 5216            -                    0        (2.49e-04)
    corner A         3161 / 3124            1711 / 1520          1.38e-05 (2.93e-04)
    corner B         7837 / 7097            5126 / 4885          0        (3.42e-04)
    contiguous I     106 / 89               -                    1.40e-05 (3.58e-04)
    contiguous II    934 / 880              780 / 752            3.70e-04 (1.04e-03)
    contiguous III   898 / 636              -                    1.91e-06 (2.96e-04)
    contiguous A     1068 / 1093            642 / 744            5.21e-07 (6.34e-06)
    contiguous B     815 / 1055             1171 / 1097          1.91e-06 (1.18e-04)
    opposite I       53 / 46                -                    3.34e-06 (2.39e-04)
    opposite II      669 / 697              642 / 658            5.48e-06 (2.48e-05)
    opposite III     505 / 514              -                    1.39e-05 (3.01e-04)
    opposite A       855 / 870              644 / 698            5.21e-07 (6.93e-06)
    opposite B       never chosen, never won
    ring slots       vertex 8182 6944 4058 10215 6600 9395 5477 1925; x fractional 2705 1957 1542 1260 1526 907;
                     y fractional 2658 1053 1424 1571 2315 693
    lookahead rejected the would-be winner 78 (any candidate 94), tie-break 42 773, stuck after a real move 150 (all on MS-DFM fields)

(shown per case: the move that used the largest share of its own bound).  No case of the oracle exceeds its derived bound; the
largest share used is 36 % (contiguous II).  Opposite I and, on MS-DFM fields, contiguous I reach their floors through the found inputs
of tests/golden/path_cases_found.json; without them the generators give opposite I 10 / 2.  Field D* and SG walks never got stuck
after a real move in the search (path_cases.census_shortfalls), MS-DFM walks do.

Mutants of the oracle (scratch copies, not committed), all 12 744 extractions: opposite I's v with p + 2 for p + 1 -- 94 extractions
fail the float64 test; contiguous I's x with b / c for b / CATH(c, b) -- 127 (way point misplaced); contiguous III charged c for b --
1441; opposite III's x without the factor p -- 743; vertex ring slots 4 and 5 swapped -- 7153 paths differ from the unmutated oracle's.
"""
import numpy as np
import pytest

import oracle_py as orc
import path_cases as pc


@pytest.fixture(scope="module")
def survey():
    """every directed extraction on the oracle's fields, once: census per planner, float64 deviations, violations"""
    out = {"census": {}, "worst": {}, "violations": [], "extractions": 0, "paths": {}}
    for algo in ("FD", "SG", "DFM"):
        total = {}
        for name, cost, thr, jobs in pc.extraction_plan(algo):
            rhs, tu = pc.oracle_field(algo, cost, thr)
            orc.path_census_reset()
            for start, la in jobs:
                path = orc.extract_path_field(rhs, algo == "DFM", cost, tu, start, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la,
                                              allow_indirect=pc.INDIRECT[algo])
                moves = orc.path_move_log()
                out["extractions"] += 1
                if len(path[0]) == 0:       # "no valid path": the start lies where the field has no value
                    continue
                try:
                    for k, t, dev, bound in pc.polyline_reference(path, moves, cost, tu, pc.INDIRECT[algo]):
                        key = (orc.PC_KINDS[k], orc.PC_TYPES[t])
                        if key not in out["worst"] or dev / bound > out["worst"][key][0] / out["worst"][key][1]:
                            out["worst"][key] = (dev, bound)
                except AssertionError as e:
                    out["violations"].append("%s %s start %r lookahead %d: %s" % (algo, name, start, la, e))
            pc.add_census(total, orc.path_census())
        out["census"][algo] = total
    return out


def test_census_meets_the_floors(survey):
    """the directed inputs make every reachable case win, in both orientations, through every ring slot, and take the extractor's
    special branches -- on the oracle alone, for Field D* and for MS-DFM fields each (SG supplies the direct-only cases)"""
    c = survey["census"]
    both = pc.add_census(pc.add_census({}, c["FD"]), c["DFM"])
    print("\n%d extractions\n%s" % (survey["extractions"], pc.census_table(both, c["SG"], survey["worst"])))
    for algo in ("FD", "DFM"):
        print("%s alone: opposite I won h / v %d / %d, lookahead rejected the winner %d, tie-break %d, stuck after a move %d" % (
            algo, c[algo]["won"][("opposite", "I", "h")], c[algo]["won"][("opposite", "I", "v")],
            c[algo]["la_rejected_winner"] + c["SG"]["la_rejected_winner"], c[algo]["tie_break"] + c["SG"]["tie_break"],
            c[algo]["stuck_after_move"] + c["SG"]["stuck_after_move"]))
        bad = pc.census_shortfalls(c[algo], c["SG"], stuck=(algo == "DFM"))
        assert not bad, "%s + SG: the directed inputs miss %s" % (algo, "; ".join(bad))


def test_opposite_B_is_never_offered(survey):
    """the reference's tables hold an opposite-edge Type B (InterpolatedTraversal.cpp:454-476) that its selection code never offers
    (:580-656, :735-778): 14 of the 15 case functions are reachable"""
    for algo, c in survey["census"].items():
        for o in orc.PC_ORIENT:
            assert c["chosen"][("opposite", "B", o)] == 0 and c["won"][("opposite", "B", o)] == 0, algo
    # ... and with direct traversals only II, A and B exist
    for (k, t, o), n in survey["census"]["SG"]["chosen"].items():
        assert n == 0 or t in ("II", "A", "B"), (k, t, o, n)


def test_oracle_extractor_against_the_float64_reference(survey):
    """every move of every directed extraction: the step costs the extractor reports are what walking its way points over the raster
    costs, within what fp32 does to the way points (path_cases.move_bound); total_dist is their length; total_cost their sum"""
    assert survey["extractions"] > 5000 and len(survey["worst"]) == 14
    assert not survey["violations"], "%d extractions off the float64 reference, first: %s" % (len(survey["violations"]), survey["violations"][0])


def test_the_float64_reference_is_not_blind():
    """a step cost off by 1e-4 of itself, a way point off by 1e-3 of a cell, a cost charged to the dearer side of a grid line: each is seen"""
    name, cost, thr = pc.directed_maps()[0]
    rhs, tu = pc.oracle_field("FD", cost, thr)
    seen = {"cost": 0, "point": 0, "side": 0}
    for start, la in pc.extraction_plan("FD")[0][3][:120]:
        pts, costs, tc, td = orc.extract_path_field(rhs, False, cost, tu, start, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la)
        moves = orc.path_move_log()
        if len(pts) < 2:
            continue
        pc.polyline_reference((pts, costs, tc, td), moves, cost, tu, True)
        wrong = costs.copy()
        wrong[0] *= np.float32(1.0001)
        with pytest.raises(AssertionError):
            pc.polyline_reference((pts, wrong, tc, td), moves, cost, tu, True)
        seen["cost"] += 1
        frac = pts[1] != np.floor(pts[1])
        if frac.any() and moves[0][0] == 1:         # a way point inside a cell side: slide it along the side
            bent = pts.copy()
            bent[1][frac] += np.float32(1e-3)
            with pytest.raises(AssertionError):
                pc.polyline_reference((bent, costs, tc, td), moves, cost, tu, True)
            seen["point"] += 1
        length, lo, hi, line = pc.segment_reference(pts[0], pts[1], cost, tu)
        if line and hi > lo and moves[0][0] == 1:
            dear = costs.copy()
            dear[0] = np.float32(length * hi)
            with pytest.raises(AssertionError):
                pc.polyline_reference((pts, dear, tc, td), moves, cost, tu, True)
            seen["side"] += 1
    assert min(seen.values()) >= 5, seen


def test_census_is_counters_only():
    """the same extraction with and without a census reset in between returns the same bits (the counters are never read back)"""
    name, cost, thr = pc.directed_maps()[1]
    rhs, tu = pc.oracle_field("DFM", cost, thr)
    jobs = pc.extraction_plan("DFM")[1][3][:40]
    first = [orc.extract_path_field(rhs, True, cost, tu, s, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la) for s, la in jobs]
    for (s, la), a in zip(jobs, first):
        orc.path_census_reset()
        b = orc.extract_path_field(rhs, True, cost, tu, s, pc.GOAL, max_steps=pc.MAX_STEPS, lookahead=la)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
