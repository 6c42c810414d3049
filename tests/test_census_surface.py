"""CPU: the surface of the cost census (ufm_track_costs, include/ufm.h) -- the symbols, the answers to NULL handles, the index
arithmetic of csrc/ufm_census_rect.h run lane by lane under sanitizers (tests/cpp/census_driver.cpp), the mirror's new members, the
harness' planner_min_cost mode and the planner process' --auto-heuristic."""
import os
import subprocess

import numpy as np
import pytest

import ufm_amd
from ufm_amd_pkg import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
CSRC = os.path.join(PKG, "csrc")
NEW = ["ufm_track_costs", "ufm_read_cost_census", "ufm_heuristic_multiplier",
       "ufm_batch_track_costs", "ufm_batch_read_cost_census", "ufm_batch_heuristic_multiplier"]
INVALID = -22


def test_symbols_exported():
    assert set(NEW) <= set(capi.SYMBOLS)
    lib = ufm_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for cls in (ufm_amd.Planner, ufm_amd.BatchPlanner):
        for member in ("track_costs", "read_cost_census", "heuristic_multiplier"):
            assert hasattr(cls, member), (cls, member)


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    hist = np.zeros(256, np.uint64)
    mn, mx, used = capi.C.c_int(0), capi.C.c_int(0), capi.C.c_float(0)
    assert lib.ufm_track_costs(None, 1) == INVALID
    assert lib.ufm_read_cost_census(None, hist.ctypes.data, capi.C.byref(mn), capi.C.byref(mx)) == INVALID
    assert lib.ufm_heuristic_multiplier(None, capi.C.byref(used)) == INVALID
    assert lib.ufm_batch_track_costs(None, 1) == INVALID
    assert lib.ufm_batch_read_cost_census(None, 0, hist.ctypes.data, capi.C.byref(mn), capi.C.byref(mx)) == INVALID
    assert lib.ufm_batch_read_cost_census(None, -1, None, None, None) == INVALID
    assert lib.ufm_batch_heuristic_multiplier(None, capi.C.byref(used)) == INVALID
    assert lib.ufm_set_param(None, b"auto_multiplier", 1.0) == INVALID


def test_off_state_is_invalid_where_a_planner_can_be_made():
    """tracking off, and on without a map: UFM_ERR_INVALID (on a machine without a GPU no planner can be created: nothing to ask)"""
    try:
        p = ufm_amd.Planner(ufm_amd.ALGO_FD, 0)
    except ufm_amd.UfmError:
        return
    try:
        mn, mx = capi.C.c_int(0), capi.C.c_int(0)
        assert p.L.ufm_read_cost_census(p.h, None, capi.C.byref(mn), capi.C.byref(mx)) == INVALID       # off
        p.track_costs()
        assert p.L.ufm_read_cost_census(p.h, None, capi.C.byref(mn), capi.C.byref(mx)) == INVALID       # on, no map
        assert p.heuristic_multiplier() == 1.0
    finally:
        p.close()


def test_census_driver(tmp_path):
    """every lane of every workgroup of k_census_build / k_census_patch as csrc/ufm_census_rect.h places it, under AddressSanitizer and
    UBSan: W = 1 .. 70, base addresses misaligned by 0 .. 15, rectangles at every border -- each cell read exactly once, counts equal to a
    brute-force count"""
    exe = str(tmp_path / "census_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "census_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    builds = 70 * 4 * 16 + 70 * 16 + 3
    patches = 70 * 11 + 3
    assert out.strip() == "%d cases, 0 bad" % (builds + patches)


@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]], ids=["heuristic", "no_heuristic"])
def test_mirror_members_type_check(define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "include")] + define + [os.path.join(ROOT, "tests", "cpp", "census_surface_driver.cpp")])


def test_planner_process_accepts_auto_heuristic(tmp_path):
    for name in ("ufm_planner", "ufm_planner_no_heur"):
        exe = os.path.join(PKG, name)
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--auto-heuristic" in r.stderr
        # the option is consumed by the parser: with it and no pipes the arguments are still "too few" (usage, exit code 1), and with it
        # and two pipes that do not exist the process gets as far as opening them (exit code 3) -- it is not taken for a positional
        r = subprocess.run([exe, "--auto-heuristic"], capture_output=True, text=True)
        assert r.returncode == 1 and "Usage" in r.stderr
        r = subprocess.run([exe, "--inflate", "5", "--auto-heuristic", str(tmp_path / "no_such_in"), str(tmp_path / "no_such_out")],
                           capture_output=True, text=True)
        assert r.returncode == 3 and "cannot open" in r.stderr


def test_harness_never_dilates_when_the_planner_does_both(monkeypatch):
    """run_mission(planner_inflates=True, planner_min_cost=True) against a stand-in for the pipes: raw map, raw patches, the raw minimum as
    the placeholder hint -- and harness.dilate is never called.  With planner_min_cost alone the inflated data still goes out."""
    h = ufm_amd.harness
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (24, 20)).astype(np.uint8)

    class FakePipes:
        def __init__(self, *a, **k):
            self.sent, self.replies = [], [("b", (0,)), ("b", (1,)), ("fff", (12.0, 9.0, 0.0)), ("b", (3,)), ("i", (0,)), ("0f", ()), ("0f", ()),
                                           ("ff", (0.0, 0.0)), ("fff", (0.0, 0.0, 0.0)), ("b", (2,))]

        def send(self, fmt, *v): self.sent.append((fmt, v))
        def send_bytes(self, b): self.sent.append(("bytes", b))
        def flush(self): pass
        def close(self): pass

        def recv(self, fmt):
            want, v = self.replies.pop(0)
            assert want == fmt, (want, fmt)
            return v

    class FakeProc:
        def __init__(self, *a, **k): pass
        def poll(self): return 0
        def wait(self, timeout=None): return 0
        def kill(self): pass

    made, calls = [], []
    real_dilate = h.dilate
    monkeypatch.setattr(h, "Pipes", lambda *a, **k: made.append(FakePipes()) or made[-1])
    monkeypatch.setattr(h.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(h.os, "mkfifo", lambda p: None)
    monkeypatch.setattr(h.os.path, "exists", lambda p: True)
    monkeypatch.setattr(h, "dilate", lambda *a, **k: calls.append(a[1]) or real_dilate(*a, **k))
    data_l, data_h = h.simulation_data(img, 10)
    after, (top, left), rng_ = h.round_patch_update(data_l, data_h, (9, 12), 5)

    def run(**kw):
        del calls[:]
        trace, finished = h.run_mission(["x"], "a", "b", img, (12.0, 9.0), (2.0, 2.0), radius=5, cspace_diameter=5, use_heuristic=True, **kw)
        assert finished and trace == [(12.0, 9.0)]
        blobs = [v for f, v in made[-1].sent if f == "bytes"]
        ints = [v for f, v in made[-1].sent if f == "i"]
        return blobs, ints, list(calls)

    blobs, ints, dilated = run(planner_inflates=True, planner_min_cost=True)
    assert dilated == [], "harness.dilate was called %d times" % len(dilated)
    assert blobs[0] == data_l.tobytes() and blobs[1] == np.ascontiguousarray(after[rng_[0], rng_[1]]).tobytes()
    assert ints == [(int(data_l.min()),), (int(after.min()),)]
    blobs, ints, dilated = run(planner_min_cost=True)
    assert dilated == [5, 5]
    assert blobs[0] == real_dilate(data_l, 5).tobytes() and ints[0] == (int(data_l.min()),)
    blobs, ints, dilated = run(planner_inflates=True)                    # as before the keyword existed
    assert dilated == [5, 5] and blobs[0] == data_l.tobytes()
    assert ints == [(int(real_dilate(data_l, 5).min()),), (int(real_dilate(after, 5).min()),)]
