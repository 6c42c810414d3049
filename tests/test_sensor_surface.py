"""CPU: the surface of the sensor reveal (ufm_set_sensor / ufm_set_survey / ufm_reveal, include/ufm.h) -- the symbols, the answers to NULL
handles, sensor_disc against the disc the harness reveals, the index arithmetic of csrc/ufm_sensor_rect.h run lane by lane under
sanitizers (tests/cpp/sensor_driver.cpp), the mirror's new members, the planner process' --sense and the harness' planner_senses mode
against a stub planner process over real FIFOs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ufm_amd
from ufm_amd_pkg import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
CSRC = os.path.join(PKG, "csrc")
NEW = ["ufm_set_sensor", "ufm_set_survey", "ufm_set_survey_device", "ufm_reveal", "ufm_read_survey",
       "ufm_batch_set_sensor", "ufm_batch_set_survey", "ufm_batch_set_survey_device", "ufm_batch_reveal", "ufm_batch_read_survey"]
INVALID = -22


def test_symbols_exported():
    assert set(NEW) <= set(capi.SYMBOLS)
    lib = ufm_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for cls in (ufm_amd.Planner, ufm_amd.BatchPlanner):
        for member in ("set_sensor", "set_survey", "reveal", "read_survey"):
            assert hasattr(cls, member), (cls, member)
    assert capi.sensor_disc is ufm_amd.sensor_disc


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    one = np.ones((1, 1), np.uint8)
    raster = np.ones((4, 4), np.uint8)
    n = capi.C.c_uint64(0)
    centres = np.zeros((1, 2), np.int32)
    assert lib.ufm_set_sensor(None, one.ctypes.data, 1, 1, -1, -1) == INVALID
    assert lib.ufm_set_survey(None, raster.ctypes.data, 4, 4) == INVALID
    assert lib.ufm_set_survey_device(None, raster.ctypes.data, 4, 4) == INVALID
    assert lib.ufm_reveal(None, 0, 0, capi.C.addressof(n)) == INVALID
    assert lib.ufm_reveal(None, 0, 0, None) == INVALID
    assert lib.ufm_read_survey(None, raster.ctypes.data) == INVALID
    assert lib.ufm_batch_set_sensor(None, one.ctypes.data, 1, 1, -1, -1) == INVALID
    assert lib.ufm_batch_set_survey(None, 0, raster.ctypes.data, 4, 4) == INVALID
    assert lib.ufm_batch_set_survey_device(None, 0, raster.ctypes.data, 4, 4) == INVALID
    assert lib.ufm_batch_reveal(None, centres.ctypes.data, None) == INVALID
    assert lib.ufm_batch_read_survey(None, 0, raster.ctypes.data) == INVALID


def test_sensor_disc_is_the_disc_the_harness_reveals():
    """revealing a ones raster into a zero raster leaves exactly the field of view: sensor_disc(5), anchored at its centre"""
    zeros, ones = np.zeros((31, 29), np.uint8), np.ones((31, 29), np.uint8)
    for radius in (0, 1, 5, 15):
        d = capi.sensor_disc(radius)
        assert d.dtype == np.uint8 and d.shape == (2 * radius + 1, 2 * radius + 1) and d[radius, radius] == 1
        row, col = 15, 14
        if radius > 13:
            continue                     # (does not fit this raster whole; the clipped cases are the driver's)
        out, (top, left), rng = ufm_amd.harness.round_patch_update(zeros, ones, (col, row), radius)
        assert (top, left) == (row - radius, col - radius)
        assert np.array_equal(out[rng[0], rng[1]], d)
        assert out.sum() == d.sum()
    # clipped at a corner: the harness' rectangle is the mask's bounding rectangle clipped on all four sides
    out, (top, left), rng = ufm_amd.harness.round_patch_update(zeros, ones, (27, 2), 5)
    d = capi.sensor_disc(5)
    assert (top, left) == (0, 22) and np.array_equal(out[rng[0], rng[1]], d[3:, :7])


def test_sensor_driver(tmp_path):
    """every lane of every workgroup of k_reveal as csrc/ufm_sensor_rect.h places it, under AddressSanitizer and UBSan: maps W, L = 1 .. 40,
    masks 1 x 1, 3 x 5 with anchor (2, 0), the 11 x 11 disc and 71 x 71, centres at every corner, border and inside -- each cell of R
    written exactly once, nothing outside, Q and the changed count equal to a brute-force loop"""
    exe = str(tmp_path / "sensor_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "sensor_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "%d cases, 0 bad" % (40 * 40 * 4 * 16)


@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]], ids=["heuristic", "no_heuristic"])
def test_mirror_members_type_check(define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "include")] + define + [os.path.join(ROOT, "tests", "cpp", "sense_driver.cpp")])


def test_planner_process_accepts_sense(tmp_path):
    for name in ("ufm_planner", "ufm_planner_no_heur"):
        exe = os.path.join(PKG, name)
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--sense" in r.stderr
        r = subprocess.run([exe, "--sense", "5"], capture_output=True, text=True)          # the option and its value are consumed: too few arguments
        assert r.returncode == 1 and "Usage" in r.stderr
        r = subprocess.run([exe, "--inflate", "5", "--auto-heuristic", "--sense", "5", str(tmp_path / "no_such_in"), str(tmp_path / "no_such_out")],
                           capture_output=True, text=True)
        assert r.returncode == 3 and "cannot open" in r.stderr


# a planner process that plans nothing: it speaks the planner's side of the wire protocol (apps/ufm_planner.cpp) over the two FIFOs, reports
# the positions it is given and writes down every byte the simulator's side sent
STUB = r'''
import json, struct, sys
senses, dump, fin, fout = sys.argv[1] == "1", sys.argv[2], sys.argv[3], sys.argv[4]
positions = [(12.0, 9.0), (14.5, 3.5), (2.0, 17.0)]
i = open(fin, "rb"); o = open(fout, "wb")
def get(fmt):
    n = struct.calcsize("<" + fmt); b = i.read(n); assert len(b) == n; return struct.unpack("<" + fmt, b)
def put(fmt, *v):
    o.write(struct.pack("<" + fmt, *v))
rec = {"moves": []}
put("b", 0); o.flush()
assert get("b") == (0,)
w, h = get("ii")
rec["size"] = [w, h]
rec["map"] = i.read(w * h).hex()
rec["survey"] = i.read(w * h).hex() if senses else None
rec["start_goal"] = list(get("ffffB"))
rec["min_cost"] = get("i")[0]
for x, y in positions:
    put("b", 1); put("fff", x, y, 0.0); o.flush()
    assert get("b") == (1,)
    top, left, ph, pw = get("iiii")
    body = i.read(ph * pw)
    assert len(body) == ph * pw
    rec["moves"].append({"header": [top, left, ph, pw], "bytes": body.hex(), "min_cost": get("i")[0]})
    put("b", 3); put("i", 0); put("ff", 0.0, 0.0); put("fff", 0.0, 0.0, 0.0); o.flush()
put("b", 2); o.flush()
assert get("b") == (2,)
json.dump(rec, open(dump, "w"))
'''


def _stub_mission(tmp_path, tag, img, **kw):
    stub = tmp_path / "stub_planner.py"
    stub.write_text(STUB)
    dump = tmp_path / ("dump_%s.json" % tag)
    moves = []
    trace, finished = ufm_amd.harness.run_mission(
        [sys.executable, str(stub), "1" if kw.get("planner_senses") else "0", str(dump)],
        str(tmp_path / ("to_%s" % tag)), str(tmp_path / ("from_%s" % tag)), img, (12.0, 9.0), (2.0, 2.0), radius=5, use_heuristic=True,
        on_move=lambda k, pos, top, left, patch, mc, reply: moves.append((pos, top, left, patch.copy(), mc)), **kw)
    assert finished and trace == [(12.0, 9.0), (14.5, 3.5), (2.0, 17.0)]
    return json.load(open(dump)), moves


def test_harness_planner_senses_over_fifos(tmp_path):
    """run_mission(planner_senses=True): the survey goes out once, directly after the map, and every patch message is a header with
    h = w = 0 and no bytes; on_move still reports the patch the reference would have sent.  The default mode is byte for byte what it was."""
    h = ufm_amd.harness
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (24, 20)).astype(np.uint8)
    data_l, data_h = h.simulation_data(img, 10)
    # what the simulator's side holds after each of the stub's three positions (round half to even: 14.5 -> 14, 3.5 -> 4)
    want, cur = [], data_l
    for row, col in ((12, 9), (14, 4), (2, 17)):
        cur, (top, left), r = h.round_patch_update(cur, data_h, (col, row), 5)
        want.append((top, left, np.ascontiguousarray(cur[r[0], r[1]]), int(cur.min())))

    plain, moves_plain = _stub_mission(tmp_path, "plain", img)
    assert plain["size"] == [20, 24] and plain["map"] == data_l.tobytes().hex() and plain["survey"] is None
    assert plain["min_cost"] == int(data_l.min())
    for got, (top, left, patch, mc) in zip(plain["moves"], want):
        assert got["header"] == [top, left, patch.shape[0], patch.shape[1]] and got["bytes"] == patch.tobytes().hex() and got["min_cost"] == mc

    senses, moves_senses = _stub_mission(tmp_path, "senses", img, planner_senses=True)
    assert senses["size"] == [20, 24] and senses["map"] == data_l.tobytes().hex()
    assert senses["survey"] == data_h.tobytes().hex()
    assert senses["start_goal"] == plain["start_goal"] and senses["min_cost"] == plain["min_cost"]
    for got, (top, left, patch, mc) in zip(senses["moves"], want):
        assert got["header"] == [top, left, 0, 0] and got["bytes"] == "" and got["min_cost"] == mc
    # on_move: the same report in both modes
    assert len(moves_plain) == len(moves_senses) == 3
    for a, b, (top, left, patch, mc) in zip(moves_plain, moves_senses, want):
        assert a[0] == b[0] and a[1:3] == b[1:3] == (top, left) and a[4] == b[4] == mc
        assert np.array_equal(a[3], patch) and np.array_equal(b[3], patch)
