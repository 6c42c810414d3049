"""CPU: the surface of the cost layers (ufm_set_layers / ufm_patch_layer / ufm_set_layer / ufm_set_layer_survey, include/ufm.h) -- the
symbols, the answers to NULL handles, the validation and index arithmetic of csrc/ufm_layers_rect.h run lane by lane under sanitizers
(tests/cpp/layers_driver.cpp, a stand-alone program), the mirror's new members, the planner process' --layers and the harness'
layers / planner_layers modes against a stub planner process over real FIFOs."""
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
SINGLE = ["ufm_set_layers", "ufm_patch_layer", "ufm_patch_layer_device", "ufm_set_layer", "ufm_set_layer_device",
          "ufm_set_layer_survey", "ufm_set_layer_survey_device", "ufm_read_layer", "ufm_read_layer_survey"]
NEW = SINGLE + [s.replace("ufm_", "ufm_batch_", 1) for s in SINGLE]
INVALID = -22


def test_symbols_exported():
    assert len(NEW) == 18 and set(NEW) <= set(capi.SYMBOLS)
    lib = ufm_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for cls in (ufm_amd.Planner, ufm_amd.BatchPlanner):
        for member in ("set_layers", "set_layer", "patch_layer", "set_layer_survey", "read_layer", "read_layer_survey"):
            assert hasattr(cls, member), (cls, member)
    assert capi.MAX_LAYERS == 4
    header = open(os.path.join(ROOT, "include", "ufm.h")).read()
    assert "#define UFM_MAX_LAYERS 4" in header


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    raster = np.ones((4, 4), np.uint8)
    p = raster.ctypes.data
    assert lib.ufm_set_layers(None, 2) == INVALID
    assert lib.ufm_patch_layer(None, 0, p, 0, 0, 4, 4) == INVALID
    assert lib.ufm_patch_layer_device(None, 0, p, 0, 0, 4, 4) == INVALID
    assert lib.ufm_set_layer(None, 0, p, 4, 4) == INVALID
    assert lib.ufm_set_layer_device(None, 0, p, 4, 4) == INVALID
    assert lib.ufm_set_layer_survey(None, 0, p, 4, 4) == INVALID
    assert lib.ufm_set_layer_survey(None, 1, p, 4, 4) == INVALID
    assert lib.ufm_set_layer_survey_device(None, 1, p, 4, 4) == INVALID
    assert lib.ufm_read_layer(None, 0, p) == INVALID
    assert lib.ufm_read_layer_survey(None, 0, p) == INVALID
    assert lib.ufm_batch_set_layers(None, 2) == INVALID
    assert lib.ufm_batch_patch_layer(None, 0, 0, p, 0, 0, 4, 4) == INVALID
    assert lib.ufm_batch_patch_layer_device(None, 0, 0, p, 0, 0, 4, 4) == INVALID
    assert lib.ufm_batch_set_layer(None, 0, 0, p, 4, 4) == INVALID
    assert lib.ufm_batch_set_layer_device(None, 0, 0, p, 4, 4) == INVALID
    assert lib.ufm_batch_set_layer_survey(None, 0, 0, p, 4, 4) == INVALID
    assert lib.ufm_batch_set_layer_survey_device(None, 0, 1, p, 4, 4) == INVALID
    assert lib.ufm_batch_read_layer(None, 0, 0, p) == INVALID
    assert lib.ufm_batch_read_layer_survey(None, 0, 0, p) == INVALID


def test_layers_driver(tmp_path):
    """every lane of every workgroup of k_layer_compose, k_layer_compose_all and k_reveal_layers as csrc/ufm_layers_rect.h places them,
    under AddressSanitizer and UBSan, in a stand-alone program: maps W, L = 1 .. 40, n = 2 and 4, ten rectangles (corners, borders,
    inside, the whole map), the vector split at all 16 base alignments, masks 1 x 1, 3 x 5 with anchor (2, 0), the 11 x 11 disc and
    71 x 71 at 16 centres -- every output element written exactly once, nothing outside, the layer stores, the composed patch, Q and
    the changed count equal to a brute-force loop"""
    exe = str(tmp_path / "layers_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "layers_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    per_map = 10 + 1 + 4 * 16
    assert out.strip() == "%d cases, 0 bad" % (40 * 40 * 2 * per_map + 16 * 71 * 2 + 16 + 1)


@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]], ids=["heuristic", "no_heuristic"])
def test_mirror_members_type_check(define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "include")] + define + [os.path.join(ROOT, "tests", "cpp", "layers_mirror_driver.cpp")])


def test_planner_process_accepts_layers(tmp_path):
    for name in ("ufm_planner", "ufm_planner_no_heur"):
        exe = os.path.join(PKG, name)
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--layers" in r.stderr
        r = subprocess.run([exe, "--sense", "5", "--layers", "2"], capture_output=True, text=True)    # the option and its value are consumed
        assert r.returncode == 1 and "Usage" in r.stderr
        r = subprocess.run([exe, "--layers", "2", "a", "b"], capture_output=True, text=True)           # needs --sense
        assert r.returncode == 1 and "--sense" in r.stderr
        r = subprocess.run([exe, "--sense", "5", "--layers", "5", "a", "b"], capture_output=True, text=True)
        assert r.returncode == 1 and "--layers" in r.stderr
        r = subprocess.run([exe, "--inflate", "5", "--auto-heuristic", "--sense", "5", "--layers", "3", str(tmp_path / "no_such_in"), str(tmp_path / "no_such_out")],
                           capture_output=True, text=True)
        assert r.returncode == 3 and "cannot open" in r.stderr


# a planner process that plans nothing: it speaks the planner's side of the wire protocol (apps/ufm_planner.cpp, --sense / --layers N) over
# the two FIFOs, reports the positions it is given and writes down every byte the simulator's side sent
STUB = r'''
import json, struct, sys
senses, nlayers, dump, fin, fout = sys.argv[1] == "1", int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
positions = [(12.0, 9.0), (14.5, 3.5), (2.0, 17.0), (13.0, 10.0)]
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
rec["layer_surveys"] = [i.read(w * h).hex() for k in range(1, nlayers)]
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
POSITIONS = [(12.0, 9.0), (14.5, 3.5), (2.0, 17.0), (13.0, 10.0)]
CELLS = ((12, 9), (14, 4), (2, 17), (13, 10))       # round half to even: 14.5 -> 14, 3.5 -> 4


def _stub_mission(tmp_path, tag, img, senses, nlayers, **kw):
    stub = tmp_path / "stub_planner.py"
    stub.write_text(STUB)
    dump = tmp_path / ("dump_%s.json" % tag)
    moves = []
    trace, finished = ufm_amd.harness.run_mission(
        [sys.executable, str(stub), "1" if senses else "0", str(nlayers), str(dump)],
        str(tmp_path / ("to_%s" % tag)), str(tmp_path / ("from_%s" % tag)), img, (12.0, 9.0), (2.0, 2.0), radius=5, use_heuristic=True,
        on_move=lambda k, pos, top, left, patch, mc, reply: moves.append((pos, top, left, patch.copy(), mc)), **kw)
    assert finished and trace == POSITIONS
    return json.load(open(dump)), moves


def _run_test_py(data_l, data_h, extra_h, diameter):
    """Tests/run_test.py:102,136-147 restated: the known rasters, the same disc uncovered in each, np.maximum, the dilation, the patch"""
    h = ufm_amd.harness
    known = [np.zeros_like(a) for a in extra_h]
    out = []
    for row, col in CELLS:
        data_l, (top, left), r = h.round_patch_update(data_l, data_h, (col, row), 5)
        known = [h.round_patch_update(k, a, (col, row), 5)[0] for k, a in zip(known, extra_h)]
        raw = data_l
        for k in known:
            raw = np.maximum(raw, k)
        cspace = h.dilate(raw, diameter)
        out.append((top, left, np.ascontiguousarray(cspace[r[0], r[1]]), int(cspace.min()), np.ascontiguousarray(raw[r[0], r[1]])))
    return out


@pytest.mark.parametrize("diameter", [1, 5])
def test_harness_composes_layers_on_the_host(tmp_path, diameter):
    """run_mission(layers=[...], planner_layers=False): every patch on the wire is the dilated maximum of the known rasters over the
    disc's rectangle, exactly as a numpy restatement of Tests/run_test.py:136-140 gives it; the first map is data_l alone (the extra
    layers start at zero); without layers the call is byte for byte what it was"""
    h = ufm_amd.harness
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (24, 20)).astype(np.uint8)
    extra = [rng.integers(1, 256, (24, 20)).astype(np.uint8), (rng.integers(0, 4, (24, 20)) == 0).astype(np.uint8) * 250]
    data_l, data_h = h.simulation_data(img, 10)
    want = _run_test_py(data_l, data_h, extra, diameter)
    got, moves = _stub_mission(tmp_path, "host%d" % diameter, img, False, 1, layers=extra, cspace_diameter=diameter)
    assert got["size"] == [20, 24] and got["map"] == h.dilate(data_l, diameter).tobytes().hex() and got["survey"] is None and got["layer_surveys"] == []
    assert got["min_cost"] == int(h.dilate(data_l, diameter).min())
    n_above = 0
    for g, (top, left, patch, mc, raw) in zip(got["moves"], want):
        assert g["header"] == [top, left, patch.shape[0], patch.shape[1]] and g["bytes"] == patch.tobytes().hex() and g["min_cost"] == mc
        n_above += int((raw > data_l[top:top + raw.shape[0], left:left + raw.shape[1]]).sum())
    assert n_above > 50, "the extra layers never showed in a patch"
    for a, (top, left, patch, mc, raw) in zip(moves, want):
        assert a[1:3] == (top, left) and np.array_equal(a[3], patch) and a[4] == mc
    plain, _ = _stub_mission(tmp_path, "plain%d" % diameter, img, False, 1, cspace_diameter=diameter)
    none, _ = _stub_mission(tmp_path, "none%d" % diameter, img, False, 1, cspace_diameter=diameter, layers=[])
    assert plain == none
    for g, (top, left, patch, mc, raw) in zip(plain["moves"], _run_test_py(data_l, data_h, [], diameter)):
        assert g["header"] == [top, left, patch.shape[0], patch.shape[1]] and g["bytes"] == patch.tobytes().hex() and g["min_cost"] == mc


def test_harness_planner_layers_over_fifos(tmp_path):
    """run_mission(planner_senses=True, planner_layers=True): the extra high-resolution rasters go out once, behind the survey, in
    order; every patch message is a header with h = w = 0 and no bytes; on_move still reports the composed patch the reference would
    have sent.  planner_layers without planner_senses is refused."""
    h = ufm_amd.harness
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (24, 20)).astype(np.uint8)
    extra = [rng.integers(1, 256, (24, 20)).astype(np.uint8), rng.integers(1, 256, (24, 20)).astype(np.uint8)]
    data_l, data_h = h.simulation_data(img, 10)
    want = _run_test_py(data_l, data_h, extra, 1)
    got, moves = _stub_mission(tmp_path, "own", img, True, 3, layers=extra, planner_senses=True, planner_layers=True)
    assert got["size"] == [20, 24] and got["map"] == data_l.tobytes().hex() and got["survey"] == data_h.tobytes().hex()
    assert got["layer_surveys"] == [a.tobytes().hex() for a in extra]
    assert got["min_cost"] == int(data_l.min())
    for g, a, (top, left, patch, mc, raw) in zip(got["moves"], moves, want):
        assert g["header"] == [top, left, 0, 0] and g["bytes"] == "" and g["min_cost"] == mc
        assert a[1:3] == (top, left) and np.array_equal(a[3], patch) and a[4] == mc
    with pytest.raises(ValueError):
        h.run_mission(["true"], str(tmp_path / "x"), str(tmp_path / "y"), img, (1.0, 1.0), (2.0, 2.0), layers=extra, planner_layers=True)
    with pytest.raises(ValueError):
        h.run_mission(["true"], str(tmp_path / "x"), str(tmp_path / "y"), img, (1.0, 1.0), (2.0, 2.0), layers=[extra[0][:5]])
