"""CPU: the surface of the graded footprint (ufm_set_cspace_graded, include/ufm_cspace_graded.h) -- the symbols, the NULL-handle answers,
the host-side arithmetic of csrc/ufm_cspace_graded_rect.h through tests/cpp/graded_driver.cpp, the kernel's body run on the host
(tests/cpp/graded_kernel_driver.cpp), the cone of ufm_cspace_cone against matrices written out by hand, and the harness' dilate_graded.
The expected lines of the driver were worked out by hand from the definition
    planning[i][j] = max { max(raw[i + a - ar][j + b - ac] - drop[a][b], 0) : drop[a][b] != 255 }
and the format of a level (bit b of row word a: drop[a][b] equals the level's drop; levels ascending by drop), not read off the code."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ufm_amd
from ufm_amd_pkg import capi
from test_cspace_surface import dilate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
CSRC = os.path.join(PKG, "csrc")
NAMES = ["ufm_set_cspace_graded", "ufm_batch_set_cspace_graded", "ufm_cspace_cone"]
O = 255


def dilate_graded_ref(raw, drop, anchor=None):
    """the definition, shift, subtract and max in int32: cells outside the map are ignored"""
    drop = np.asarray(drop)
    mh, mw = drop.shape
    ar, ac = (mh // 2, mw // 2) if anchor is None else anchor
    L, W = raw.shape
    out = np.zeros((L, W), np.int32)
    for a in range(mh):
        for b in range(mw):
            if drop[a, b] != 255:
                di, dj = a - ar, b - ac                     # out[i][j] takes raw[i + di][j + dj] - drop[a][b], not below 0
                i0, i1, j0, j1 = max(0, -di), min(L, L - di), max(0, -dj), min(W, W - dj)
                if i0 < i1 and j0 < j1:
                    out[i0:i1, j0:j1] = np.maximum(out[i0:i1, j0:j1], raw[i0 + di:i1 + di, j0 + dj:j1 + dj].astype(np.int32) - int(drop[a, b]))
    return out.astype(np.uint8)


# the footprints of the device tests (tests/test_gpu_cspace_graded.py), written out
CONE5 = np.array([[O, O, 80, O, O], [O, 80, 40, 80, O], [80, 40, 0, 40, 80], [O, 80, 40, 80, O], [O, O, 80, O, O]], np.uint8)   # cone (1, 5, 40)
ELL_GRADED = (np.array([[60, O, O, O, O], [30, O, O, O, O], [0, 25, 50, 75, 100]], np.uint8), (2, 0))
NON_MONOTONE = np.array([[50, 0, 50], [20, 0, 20], [0, O, 10]], np.uint8)


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ufm_[a-z_0-9]+)\s*\(", txt)))


def test_symbols_exported():
    """the three calls are declared in include/ufm_cspace_graded.h, which include/ufm.h includes, are the binding's GRADED_SYMBOLS, and
    are exported by the library; the Python and C++ surfaces have their callers"""
    assert _declared("ufm_cspace_graded.h") == sorted(capi.GRADED_SYMBOLS) == sorted(NAMES)
    assert not set(NAMES) & set(capi.SYMBOLS)
    assert re.search(r'^#include "ufm_cspace_graded\.h"$', open(os.path.join(ROOT, "include", "ufm.h")).read(), flags=re.M)
    lib = ufm_amd.load_library()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes and fn.restype is ctypes.c_int, name
    for cls in (ufm_amd.Planner, ufm_amd.BatchPlanner):
        assert callable(getattr(cls, "set_cspace_graded"))
    assert ufm_amd.Planner.set_cspace_graded is ufm_amd.BatchPlanner.set_cspace_graded      # one body
    assert callable(ufm_amd.cspace_cone) and callable(ufm_amd.harness.dilate_graded)
    assert "ufm_set_cspace_graded(handle_" in open(os.path.join(PKG, "include", "ReplannerBase.h")).read()
    header = open(os.path.join(ROOT, "include", "ufm_cspace_graded.h")).read()
    assert re.search(r"#define\s+UFM_CSPACE_OUTSIDE\s+255\b", header) and re.search(r"#define\s+UFM_CSPACE_MAX_LEVELS\s+16\b", header)
    assert (capi.CSPACE_OUTSIDE, capi.CSPACE_MAX_LEVELS) == (255, 16)


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    drop = np.zeros((3, 3), np.uint8)
    assert lib.ufm_set_cspace_graded(None, drop.ctypes.data, 3, 3, -1, -1) == -22
    assert lib.ufm_batch_set_cspace_graded(None, drop.ctypes.data, 3, 3, -1, -1) == -22


def test_headers_are_plain_c(tmp_path):
    """a C99 program that includes ufm.h alone calls the three entry points and links; the new header included alone, and first, compiles"""
    src = tmp_path / "graded.c"
    src.write_text('#include "ufm.h"\n#include <stdio.h>\nint main(void) {\n  uint8_t drop[25] = {0};\n'
                   '  if (ufm_set_cspace_graded(NULL, drop, 5, 5, -1, -1) != UFM_ERR_INVALID) return 1;\n'
                   '  if (ufm_batch_set_cspace_graded(NULL, drop, 5, 5, -1, -1) != UFM_ERR_INVALID) return 2;\n'
                   '  if (ufm_cspace_cone(1, 5, 40, drop) != UFM_OK) return 3;\n'
                   '  printf("%d %d %d %d %d\\n", drop[12], drop[11], drop[10], drop[0], UFM_CSPACE_OUTSIDE + UFM_CSPACE_MAX_LEVELS);\n  return 0;\n}\n')
    exe = tmp_path / "graded"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + PKG, "-lufm", "-Wl,-rpath," + PKG])
    assert subprocess.check_output([str(exe)], text=True).split() == ["0", "40", "80", "255", "271"]
    alone = tmp_path / "alone.c"
    alone.write_text('#include "ufm_cspace_graded.h"\n#include "ufm.h"\nint main(void) { ufm_stats t; ufm_score s; (void)t; (void)s; return UFM_CSPACE_OUTSIDE - 255; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(alone)])


R31 = ",".join(["7fffffff"] * 31)
RAMP = " ".join("d%d=%x" % (k, 1 << k) for k in range(16))
EXPECTED = """\
graded anchor_drop_nonzero: ok=0
graded levels_17: ok=0
graded levels_16: ok=1 on=1 anchor=0,0 levels=16 support=ffff union=1 disjoint=1 %s
graded levels_16_and_outside: ok=1 on=1 anchor=0,0 levels=16 support=ffff union=1 disjoint=1 %s
graded size_0: ok=0
graded size_0_rows: ok=0
graded size_32: ok=0
graded size_31: ok=1 on=1 anchor=15,15 levels=1 support=%s union=1 disjoint=1 d0=%s
graded anchor_outside: ok=0
graded anchor_negative: ok=0
graded anchor_is_outside_cell: ok=0
graded null_drop: ok=0
graded one_by_one: ok=1 on=0 anchor=0,0 levels=1 support=1 union=1 disjoint=1 d0=1
graded ell_flat: ok=1 on=1 anchor=2,0 levels=1 support=1,1,1f union=1 disjoint=1 d0=1,1,1f
flat ell_flat: ok=1 same=1 on=1
flat block_4x4: ok=1 same=1 on=1
flat one_by_one: ok=1 same=1 on=0
graded cone_5x5_two_rings: ok=1 on=1 anchor=2,2 levels=3 support=4,e,1f,e,4 union=1 disjoint=1 d0=0,0,4,0,0 d40=0,4,a,4,0 d80=4,a,11,a,4
graded non_monotone: ok=1 on=1 anchor=1,1 levels=4 support=7,7,5 union=1 disjoint=1 d0=2,2,1 d10=0,0,4 d20=0,5,0 d50=5,0,0
graded ell_graded: ok=1 on=1 anchor=2,0 levels=7 support=1,1,1f union=1 disjoint=1 d0=0,0,1 d25=0,0,2 d30=0,1,0 d50=0,0,4 d60=1,0,0 d75=0,0,8 d100=0,0,10
""" % (RAMP, RAMP, R31, R31)


def test_graded_driver(tmp_path):
    exe = str(tmp_path / "graded_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "graded_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.splitlines() == EXPECTED.splitlines()


def test_kernel_body_on_the_host(tmp_path):
    """tests/cpp/graded_kernel_driver.cpp: k_cspace_dilate_graded's body as plain C++, every thread of every workgroup, under sanitizers,
    against a brute-force loop over the definition -- 160 whole maps and 160 grown rectangles with pitches of their own, widths with and
    without the dword staging path, footprints up to 31 x 31, every level count 1 .. 16"""
    exe = str(tmp_path / "graded_kernel_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-attributes", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "graded_kernel_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "320 cases, 0 bad, level counts seen ffff"


def test_flat_kernel_header_is_untouched():
    """the graded kernel is a header of its own behind ufm_cspace.h; the engine picks between the two kernels in Engine::cspace_dilate
    and nowhere else"""
    flat = open(os.path.join(CSRC, "ufm_cspace.h")).read()
    assert "graded" not in flat and "k_cspace_dilate(CspaceJob J)" in flat
    launches = {}
    for f in sorted(os.listdir(CSRC)):
        txt = open(os.path.join(CSRC, f)).read()
        for k in ("k_cspace_dilate<<<", "k_cspace_dilate_graded<<<"):
            if k in txt:
                launches.setdefault(k, []).append((f, txt.count(k)))
    assert launches == {"k_cspace_dilate<<<": [("ufm_map_host.h", 1)], "k_cspace_dilate_graded<<<": [("ufm_map_host.h", 1)]}
    rect = open(os.path.join(CSRC, "ufm_cspace_graded_rect.h")).read()
    assert "hip" not in rect.lower().replace("without hip", "")


# ---- ufm_cspace_cone: matrices written out by hand from the definition --------------------------------------------------------------
# (5, 9, 30): r_in = 2, r_out = 4.  d2 <= 4: 0; d2 <= 9: 30 (k = 1); d2 <= 16: 60 (k = 2); beyond: 255.  Row dy, column dx, d2 = dx^2 + dy^2:
CONE_5_9_30 = np.array([
    [O,  O,  O,  O,  60, O,  O,  O,  O],      # dy = -4: d2 = 32 25 20 17 16 17 20 25 32
    [O,  O,  60, 60, 30, 60, 60, O,  O],      # dy = -3:      25 18 13 10  9 10 13 18 25
    [O,  60, 30, 30, 0,  30, 30, 60, O],      # dy = -2:      20 13  8  5  4  5  8 13 20
    [O,  60, 30, 0,  0,  0,  30, 60, O],      # dy = -1:      17 10  5  2  1  2  5 10 17
    [60, 30, 0,  0,  0,  0,  0,  30, 60],     # dy =  0:      16  9  4  1  0  1  4  9 16
    [O,  60, 30, 0,  0,  0,  30, 60, O],
    [O,  60, 30, 30, 0,  30, 30, 60, O],
    [O,  O,  60, 60, 30, 60, 60, O,  O],
    [O,  O,  O,  O,  60, O,  O,  O,  O]], np.uint8)


def test_cone_by_hand():
    assert np.array_equal(ufm_amd.cspace_cone(1, 5, 40), CONE5)
    assert np.array_equal(ufm_amd.cspace_cone(5, 9, 30), CONE_5_9_30)
    # (3, 31, 17): r_in = 1, r_out = 15; along the axis at distance t: t <= 1: 0, else ring k = t - 1, drop min(254, 17 k) -- 17 * 14 = 238 is
    # the last below the cap -- and on the diagonal at (t, t), d2 = 2 t^2: k = ceil(sqrt(2) t) - 1 while 2 t^2 <= 225, i.e. t <= 10
    c = ufm_amd.cspace_cone(3, 31, 17)
    assert c.shape == (31, 31) and c.dtype == np.uint8
    axis = [0, 0] + [17 * k for k in range(1, 15)]
    assert axis[-1] == 238 and c[15, 15:].tolist() == axis and c[15:, 15].tolist() == axis and c[15, 15::-1].tolist() == axis
    #        t:  0  1  2   3   4   5    6    7    8    9    10    11
    # 2 t^2:     0  2  8   18  32  50   72   98   128  162  200   242
    # k:         -  1  2   4   5   7    8    9    11   12   14    outside  (k + 1 = ceil(sqrt(2 t^2)): 2, 3, 5, 6, 8, 9, 10, 12, 13, 15)
    assert [int(c[15 + t, 15 + t]) for t in range(12)] == [0, 17, 34, 68, 85, 119, 136, 153, 187, 204, 238, 255]
    # the last row, dy = 15: d2 = 225 + dx^2, inside for dx = 0 only, ring 14; the one before, dy = 14: d2 = 196 + dx^2 <= 225 for |dx| <= 5,
    # ring 13 at dx = 0 (196 = 14^2), ring 14 beside it
    assert c[30].tolist() == [255] * 15 + [238] + [255] * 15
    assert c[29].tolist() == [255] * 10 + [238] * 5 + [221] + [238] * 5 + [255] * 10
    assert np.array_equal(c, c.T) and np.array_equal(c, c[::-1]) and np.array_equal(c, c[:, ::-1])
    # step 100 on the same rings: 100, 200, then the cap
    assert ufm_amd.cspace_cone(3, 31, 100)[15, 15:].tolist() == [0, 0, 100, 200] + [254] * 12
    assert sorted(set(c.ravel().tolist())) == [17 * k for k in range(15)] + [255]       # 15 levels and outside
    # the binding returns the bytes the C function writes
    lib = ufm_amd.load_library()
    raw = np.full((31, 31), 7, np.uint8)
    assert lib.ufm_cspace_cone(3, 31, 17, raw.ctypes.data) == 0 and np.array_equal(raw, c)
    buf = np.zeros((31, 31), np.uint8)
    for bad in ((0, 5, 40), (7, 5, 40), (1, 33, 40), (1, 32, 8), (1, 5, 0), (1, 5, 255), (-3, 5, 40)):
        assert lib.ufm_cspace_cone(*bad, buf.ctypes.data) == -22, bad
        with pytest.raises(ufm_amd.UfmError):
            ufm_amd.cspace_cone(*bad)
    assert lib.ufm_cspace_cone(1, 5, 40, None) == -22
    assert not buf.any()
    assert lib.ufm_cspace_cone(1, 31, 8, buf.ctypes.data) == 0 and lib.ufm_cspace_cone(31, 31, 254, buf.ctypes.data) == 0     # 15 rings; a flat disc
    assert set(buf.ravel().tolist()) == {0, 255}
    assert np.array_equal(ufm_amd.cspace_cone(1, 1, 9), [[0]])


def test_cone_clips_at_254():
    """(3, 31, 17) does not reach the cap on its own rings -- the last is 14 * 17 = 238 --, so the clip is pinned where it bites: with the
    step 20 ring 13 is 254, not 260, and with 19 ring 14 is 254, not 266"""
    assert ufm_amd.cspace_cone(3, 31, 20)[15, 15:].tolist() == [0, 0] + [20 * k for k in range(1, 13)] + [254, 254]
    assert ufm_amd.cspace_cone(3, 31, 19)[15, 15:].tolist() == [0, 0] + [19 * k for k in range(1, 14)] + [254]


def test_harness_dilate_graded():
    """harness.dilate_graded == the shift-subtract-max reference; with all-zero drops it is the flat dilation of the same support"""
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 256, (37, 29)).astype(np.uint8)
    h = ufm_amd.harness
    for drop, anchor in ((CONE5, None), ELL_GRADED, (NON_MONOTONE, None), (CONE_5_9_30, None), (ufm_amd.cspace_cone(3, 31, 17), None)):
        got = h.dilate_graded(raw, drop, anchor)
        assert got.dtype == np.uint8 and np.array_equal(got, dilate_graded_ref(raw, drop, anchor))
        flat = np.where(drop != 255, 0, 255).astype(np.uint8)
        assert np.array_equal(h.dilate_graded(raw, flat, anchor), dilate_ref(raw, drop != 255, anchor))
        assert np.array_equal(dilate_graded_ref(raw, flat, anchor), dilate_ref(raw, drop != 255, anchor))
        assert (got >= raw).all() and (got <= dilate_ref(raw, drop != 255, anchor)).all()
    # one obstacle: the footprint reflected about its anchor appears around it
    one = np.zeros((9, 9), np.uint8)
    one[4, 4] = 200
    assert np.array_equal(h.dilate_graded(one, CONE5)[2:7, 2:7], np.where(CONE5 == 255, 0, 200 - CONE5.astype(int)))
    got = h.dilate_graded(one, *ELL_GRADED)
    assert got[4, 4] == 200 and got[4, 0] == 100 and got[6, 4] == 140 and got[5, 4] == 170 and got[3, 4] == 0 and got[4, 5] == 0
    # for discs the harness' flat dilation and the graded one with zero drops agree (one footprint: cspace_disc)
    for d in (3, 5, 9):
        assert np.array_equal(h.dilate_graded(raw, np.where(ufm_amd.cspace_disc(d), 0, 255)), h.dilate(raw, d))


def test_harness_margin_on_the_wire(monkeypatch):
    """run_mission(margin=(9, 30)) against a stand-in for the pipes: by default the bytes on the wire are dilate_graded(data_l, cone) and
    its patches; with planner_inflates=True they are data_l and its raw patches, and min_cost still comes from the inflated map"""
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

    made = []
    monkeypatch.setattr(h, "Pipes", lambda *a, **k: made.append(FakePipes()) or made[-1])
    monkeypatch.setattr(h.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(h.os, "mkfifo", lambda p: None)
    monkeypatch.setattr(h.os.path, "exists", lambda p: True)
    cone = ufm_amd.cspace_cone(5, 9, 30)
    data_l, data_h = h.simulation_data(img, 10)
    after, (top, left), rng_ = h.round_patch_update(data_l, data_h, (9, 12), 5)
    for kw, first, second in (({}, dilate_graded_ref(data_l, cone), dilate_graded_ref(after, cone)), ({"planner_inflates": True}, data_l, after)):
        trace, finished = h.run_mission(["x"], "a", "b", img, (12.0, 9.0), (2.0, 2.0), radius=5, cspace_diameter=5, margin=(9, 30), **kw)
        assert finished and trace == [(12.0, 9.0)]
        blobs = [v for f, v in made[-1].sent if f == "bytes"]
        ints = [v for f, v in made[-1].sent if f == "i"]
        assert blobs[0] == first.tobytes()
        assert blobs[1] == np.ascontiguousarray(second[rng_[0], rng_[1]]).tobytes()
        assert ints[0] == (int(dilate_graded_ref(data_l, cone).min()),)
    assert made[0].sent != made[1].sent
