"""CPU: the surface of map preparation (ufm_gaussian_taps / ufm_set_image, include/ufm.h) -- the symbols, the answers to NULL handles,
capi.gaussian_taps against harness.gaussian_kernel_fixed, the arithmetic of csrc/ufm_prepare_rect.h run workgroup by workgroup and lane by
lane under sanitizers (tests/cpp/prepare_driver.cpp), the mirror's new member, the planner process' --image and the harness'
planner_prepares mode against a stub planner process over real FIFOs."""
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
NEW = ["ufm_gaussian_taps", "ufm_set_image", "ufm_set_image_device", "ufm_batch_set_image", "ufm_batch_set_image_device"]
INVALID = -22


def test_symbols_exported():
    assert set(NEW) <= set(capi.SYMBOLS)
    lib = ufm_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for cls in (ufm_amd.Planner, ufm_amd.BatchPlanner):
        assert hasattr(cls, "set_image"), cls
    assert callable(capi.gaussian_taps)
    mirror = open(os.path.join(PKG, "include", "ReplannerBase.h")).read()
    assert "void set_image(" in mirror and "ufm_set_image(handle_" in mirror


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    img = np.ones((4, 4), np.uint8)
    taps = np.array([256], np.uint16)
    assert lib.ufm_set_image(None, img.ctypes.data, 4, 4, taps.ctypes.data, 1, 0) == INVALID
    assert lib.ufm_set_image_device(None, img.ctypes.data, 4, 4, taps.ctypes.data, 1, 0) == INVALID
    assert lib.ufm_batch_set_image(None, 0, img.ctypes.data, 4, 4, taps.ctypes.data, 1, 0) == INVALID
    assert lib.ufm_batch_set_image_device(None, 0, img.ctypes.data, 4, 4, taps.ctypes.data, 1, 0) == INVALID
    assert lib.ufm_gaussian_taps(13, None) == INVALID


def test_gaussian_taps_are_the_harness():
    """the one C definition against its numpy restatement, every size there is; k = 13 is the recorded mission's kernel"""
    for k in range(1, 32, 2):
        got, want = capi.gaussian_taps(k), ufm_amd.harness.gaussian_kernel_fixed(k)
        assert got.dtype == np.uint16 and got.shape == (k,)
        assert np.array_equal(got.astype(np.int64), want), (k, got, want)
        assert int(got.sum()) == 256 and int(want.min()) >= 0, k
    assert capi.gaussian_taps(13).tolist() == [1, 5, 10, 19, 30, 41, 44, 41, 30, 19, 10, 5, 1]
    assert capi.gaussian_taps(1).tolist() == [256] and capi.gaussian_taps(3).tolist() == [64, 128, 64]
    for bad in (0, 2, 12, 32, 33, -1, -3):
        with pytest.raises(ufm_amd.UfmError):
            capi.gaussian_taps(bad)


def test_prepare_driver(tmp_path):
    """every lane of every workgroup of k_prepare as csrc/ufm_prepare_rect.h runs it, under AddressSanitizer and UBSan: maps W, L = 1 .. 40
    plus 63 x 257 and 130 x 65 both ways round and 68 x 132; 1, 3, 13 and 31 taps wherever ntaps / 2 < min(W, L); penalties 0, 15, 255;
    random, all-0 and all-255 images; aligned and misaligned rasters -- every output cell written exactly once and nothing beyond the
    rasters, every staged source index inside the image, no row sum beyond 16 bits, L and H equal to a brute-force double loop"""
    exe = str(tmp_path / "prepare_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "prepare_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    # maps that take n taps: (40 - n // 2)^2 of the 40 x 40, plus the five large ones; 5 launches each; 2 lane footprints
    maps = sum((40 - n // 2) ** 2 + 5 for n in (1, 3, 13, 31))
    assert out.strip() == "%d cases, 0 bad" % (5 * maps + 2)


@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]], ids=["heuristic", "no_heuristic"])
def test_mirror_members_type_check(define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "include")] + define + [os.path.join(ROOT, "tests", "cpp", "image_driver.cpp")])


def test_planner_process_accepts_image(tmp_path):
    for name in ("ufm_planner", "ufm_planner_no_heur"):
        exe = os.path.join(PKG, name)
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--image K P" in r.stderr
        r = subprocess.run([exe, "--image", "13", "15"], capture_output=True, text=True)      # the option and both values are consumed: too few arguments
        assert r.returncode == 1 and "Usage" in r.stderr
        r = subprocess.run([exe, "--image", "13", "15", "--inflate", "5", "--auto-heuristic", "--sense", "5", str(tmp_path / "no_such_in"),
                            str(tmp_path / "no_such_out")], capture_output=True, text=True)
        assert r.returncode == 3 and "cannot open" in r.stderr


# a planner process that plans nothing: it speaks the planner's side of the wire protocol (apps/ufm_planner.cpp) over the two FIFOs, reports
# the positions it is given and writes down every byte the simulator's side sent.  argv[1]: "1" if a survey message follows the map.
STUB = r'''
import json, struct, sys
survey, dump, fin, fout = sys.argv[1] == "1", sys.argv[2], sys.argv[3], sys.argv[4]
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
rec["survey"] = i.read(w * h).hex() if survey else None
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


def _stub_mission(tmp_path, tag, img, survey_message, **kw):
    stub = tmp_path / "stub_planner.py"
    stub.write_text(STUB)
    dump = tmp_path / ("dump_%s.json" % tag)
    moves, maps = [], []
    trace, finished = ufm_amd.harness.run_mission(
        [sys.executable, str(stub), "1" if survey_message else "0", str(dump)],
        str(tmp_path / ("to_%s" % tag)), str(tmp_path / ("from_%s" % tag)), img, (12.0, 9.0), (2.0, 2.0), radius=5, use_heuristic=True,
        on_map=lambda m, mc: maps.append((m.copy(), mc)),
        on_move=lambda k, pos, top, left, patch, mc, reply: moves.append((pos, top, left, patch.copy(), mc)), **kw)
    assert finished and trace == [(12.0, 9.0), (14.5, 3.5), (2.0, 17.0)]
    return json.load(open(dump)), moves, maps


def test_harness_planner_prepares_over_fifos(tmp_path):
    """run_mission(planner_prepares=True): where the map raster would go the BITMAP goes out, framed the same way, and with planner_senses no
    survey message follows it; min_cost, the patch messages and what on_map / on_move report are those of the mode without it.
    filter_size reaches simulation_data; the default (3, no planner_prepares) is byte for byte what it was."""
    h = ufm_amd.harness
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (24, 20)).astype(np.uint8)
    for fs, pen in ((3, 10), (13, 15)):
        data_l, data_h = h.simulation_data(img, pen, fs)
        want, cur = [], data_l
        for row, col in ((12, 9), (14, 4), (2, 17)):
            cur, (top, left), r = h.round_patch_update(cur, data_h, (col, row), 5)
            want.append((top, left, np.ascontiguousarray(cur[r[0], r[1]]), int(cur.min())))
        kw = {} if fs == 3 else {"filter_size": fs}
        tag = "k%d_" % fs
        plain, moves_plain, maps_plain = _stub_mission(tmp_path, tag + "plain", img, False, low_res_penalty=pen, **kw)
        assert plain["size"] == [20, 24] and plain["map"] == data_l.tobytes().hex() and plain["min_cost"] == int(data_l.min())

        # the planner prepares, the host still cuts the patches
        prep, moves_prep, maps_prep = _stub_mission(tmp_path, tag + "prep", img, False, low_res_penalty=pen, planner_prepares=True, **kw)
        assert prep["size"] == [20, 24] and prep["map"] == img.tobytes().hex() and prep["survey"] is None
        assert prep["start_goal"] == plain["start_goal"] and prep["min_cost"] == plain["min_cost"]
        assert prep["moves"] == plain["moves"]
        for got, (top, left, patch, mc) in zip(prep["moves"], want):
            assert got["header"] == [top, left, patch.shape[0], patch.shape[1]] and got["bytes"] == patch.tobytes().hex() and got["min_cost"] == mc

        # the planner prepares and senses: the bitmap and positions, nothing else
        both, moves_both, maps_both = _stub_mission(tmp_path, tag + "both", img, False, low_res_penalty=pen, planner_prepares=True, planner_senses=True, **kw)
        assert both["map"] == img.tobytes().hex() and both["survey"] is None and both["min_cost"] == plain["min_cost"]
        for got, (top, left, patch, mc) in zip(both["moves"], want):
            assert got["header"] == [top, left, 0, 0] and got["bytes"] == "" and got["min_cost"] == mc
        # planner_senses alone still sends the survey
        senses, _, _ = _stub_mission(tmp_path, tag + "senses", img, True, low_res_penalty=pen, planner_senses=True, **kw)
        assert senses["map"] == data_l.tobytes().hex() and senses["survey"] == data_h.tobytes().hex()

        # on_map / on_move: the same report in every mode
        for maps in (maps_plain, maps_prep, maps_both):
            assert len(maps) == 1 and np.array_equal(maps[0][0], data_l) and maps[0][1] == int(data_l.min())
        for moves in (moves_plain, moves_prep, moves_both):
            assert len(moves) == 3
            for a, (top, left, patch, mc) in zip(moves, want):
                assert a[1:3] == (top, left) and a[4] == mc and np.array_equal(a[3], patch)
    # the planner makes the raw map: a footprint is then the planner's too
    with pytest.raises(ValueError):
        h.run_mission(["true"], str(tmp_path / "x_in"), str(tmp_path / "x_out"), img, (12.0, 9.0), (2.0, 2.0), cspace_diameter=5, planner_prepares=True)
