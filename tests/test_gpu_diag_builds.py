"""-m gpu: the two diagnostic builds of the engine (csrc/ufm_diag.h: -DUFM_TIMING -> libufm_timing.so, -DUFM_SWEEPSTAT -> libufm_sstat.so; the
libraries the tools under tools/ load) against the product.  The same kernels with their recording hooks filled in: they must compute the product's
field bit for bit -- FD fields are bit-equal whatever the schedule -- in the resident form (case A) and in the launch chain with the cursor hand-out
(case B), and what they record about a plan must agree with the engine's own statistics where the code guarantees it:
  timing build      g_tdiag[3] (visits timed: thread 0, once per lowering visit that reaches the end of the loop body) == stats.tile_visits
                    (thread 4, same place; a plan from scratch has no invalidation visits); case A: the per-tile visit counts sum to
                    stats.resident_tile_visits, idle workgroups looked at least once, visits were recorded; every reader returns
  sweep statistics  16 * g_sstat[0] == stats.elem_evals (a sweep is 16 node evaluations: s_stat[2] += 16 * s_misc[2]); the sweeps that changed
                    nothing and the bursts are each at most the sweeps
tests/diag_probe.py measures (a process per library: a process binds one build) and prints; the assertions are here."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")


def _probe(lib):
    assert os.path.exists(os.path.join(PKG, lib)), "make -C unige-tasi-path-planners_amd (or __graft_entry__.build()) builds " + lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "diag_probe.py"), os.path.join(PKG, lib)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    print(lib + "\n" + out.stdout)
    return [l.split() for l in out.stdout.strip().splitlines()]


@pytest.fixture(scope="module")
def runs():
    return {lib: _probe(lib) for lib in ("libufm.so", "libufm_timing.so", "libufm_sstat.so")}


def _relations(lines):
    """the counter pairs a probe printed: {(case, what): (kind, values)}, each asserted as it is collected"""
    found = {}
    for l in lines:
        if l[0] in ("eq", "le", "gt0"):
            vals = [int(v) for v in l[3:]]
            found[(l[1], l[2])] = (l[0], vals)
            ok = {"eq": lambda v: v[0] == v[1], "le": lambda v: v[0] <= v[1], "gt0": lambda v: v[0] > 0}[l[0]](vals)
            assert ok, " ".join(l)
    return found


def test_fields_of_the_diagnostic_builds_equal_the_products(runs):
    fields = {lib: [l for l in lines if l[0] == "field"] for lib, lines in runs.items()}
    assert [l[1] for l in fields["libufm.so"]] == ["A", "B"]
    assert fields["libufm_timing.so"] == fields["libufm.so"] and fields["libufm_sstat.so"] == fields["libufm.so"], fields
    for lib, lines in runs.items():
        checks = [l for l in lines if l[0] == "checks"]
        assert len(checks) == 2 and all(" ".join(l[2:]) == "layout (0, 0) info (0, 0, 0)" for l in checks), (lib, checks)
        assert set(_relations(lines)) >= {("A", "resident_launches"), ("B", "resident_launches")}, lib


def test_version_strings_name_the_diagnostic_builds(runs):
    v = {lib: " ".join(lines[0][1:]) for lib, lines in runs.items()}
    assert "timing build" in v["libufm_timing.so"] and "sweep-statistics build" in v["libufm_sstat.so"]
    assert "build" not in v["libufm.so"] and v["libufm.so"].startswith("ufm-gfx950"), v


def test_timing_records_agree_with_the_statistics(runs):
    rel = _relations(runs["libufm_timing.so"])
    assert set(rel) == {("A", "resident_launches"), ("B", "resident_launches"),
                        ("A", "tdiag[3]:visits_timed=tile_visits"), ("B", "tdiag[3]:visits_timed=tile_visits"),
                        ("A", "sum(tiles[3]):visits=resident_tile_visits"), ("A", "sdiag[0]:looks"), ("A", "visits_recorded")}, sorted(rel)
    assert all(rel[k][1][0] > 0 for k in rel if k[1].startswith("tdiag")), rel        # (something was timed)
    readers = [l for l in runs["libufm_timing.so"] if l[0] == "readers"]
    assert [l[1] for l in readers] == ["A", "B"]
    for l in readers:                                 # plog and trace return a count, wtrace a code
        assert int(l[3]) >= 0 and int(l[5]) >= 0 and int(l[7]) == 0, l


def test_sweep_statistics_agree_with_the_statistics(runs):
    rel = _relations(runs["libufm_sstat.so"])
    assert set(rel) == {(c, w) for c in "AB" for w in ("resident_launches", "16*sstat[0]:sweeps=elem_evals", "sstat[1]:quiet_sweeps<=sstat[0]:sweeps",
                                                       "sstat[3]:bursts<=sstat[0]:sweeps")}, sorted(rel)
    assert all(rel[(c, "16*sstat[0]:sweeps=elem_evals")][1][0] > 0 for c in "AB"), rel
