"""CPU: the surface of the C-space inflation (ufm_set_cspace, include/ufm.h) -- the symbols, the NULL-handle answers, the host-side
arithmetic of csrc/ufm_cspace_rect.h through tests/cpp/cspace_driver.cpp, the kernel's body run on the host
(tests/cpp/cspace_kernel_driver.cpp), the harness' raw mode, and the footprint of harness.dilate as data.
The expected lines of the driver were worked out by hand from the definition
    planning[i][j] = max { raw[i + a - ar][j + b - ac] : mask[a][b] != 0 }
(a raw change at row c reaches the outputs c - a + ar: the mask reflected about its anchor), not read off the code."""
import ctypes
import os
import subprocess

import numpy as np

import ufm_amd
from ufm_amd_pkg import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unige-tasi-path-planners_amd", "csrc")
NEW = ["ufm_set_cspace", "ufm_read_raw_map", "ufm_batch_set_cspace", "ufm_batch_read_raw_map"]


def dilate_ref(raw, mask, anchor=None):
    """the definition, shift and max: cells outside the map are ignored"""
    mask = np.asarray(mask)
    mh, mw = mask.shape
    ar, ac = (mh // 2, mw // 2) if anchor is None else anchor
    L, W = raw.shape
    out = np.zeros_like(raw)
    for a in range(mh):
        for b in range(mw):
            if mask[a, b]:
                di, dj = a - ar, b - ac                     # out[i][j] takes raw[i + di][j + dj]
                i0, i1, j0, j1 = max(0, -di), min(L, L - di), max(0, -dj), min(W, W - dj)
                if i0 < i1 and j0 < j1:
                    out[i0:i1, j0:j1] = np.maximum(out[i0:i1, j0:j1], raw[i0 + di:i1 + di, j0 + dj:j1 + dj])
    return out


def test_symbols_exported():
    assert set(NEW) <= set(capi.SYMBOLS)
    lib = ufm_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    assert hasattr(ufm_amd, "cspace_disc") and hasattr(ufm_amd.Planner, "set_cspace") and hasattr(ufm_amd.Planner, "read_raw_map")
    assert hasattr(ufm_amd.BatchPlanner, "set_cspace") and hasattr(ufm_amd.BatchPlanner, "read_raw_map")


def test_null_handles_are_invalid():
    lib = ufm_amd.load_library()
    mask = np.ones((3, 3), np.uint8)
    buf = np.zeros(16, np.uint8)
    assert lib.ufm_set_cspace(None, mask.ctypes.data, 3, 3, -1, -1) == -22
    assert lib.ufm_read_raw_map(None, buf.ctypes.data) == -22
    assert lib.ufm_batch_set_cspace(None, mask.ctypes.data, 3, 3, -1, -1) == -22
    assert lib.ufm_batch_read_raw_map(None, 0, buf.ctypes.data) == -22


EXPECTED = """\
grow ell_anchor_bottom_left: m=0 x=20 y=6 w=8 h=8
grow ell_anchor_top_left: m=0 x=18 y=6 w=8 h=8
grow cross_inside: m=2 x=19 y=9 w=6 h=8
grow even_4x4_anchor_2_2: m=0 x=19 y=9 w=4 h=4
grow top_border: m=0 x=0 y=8 w=8 h=8
grow bottom_border: m=0 x=40 y=8 w=8 h=8
grow left_border: m=0 x=18 y=0 w=6 h=10
grow right_border: m=0 x=18 y=34 w=6 h=10
grow corner: m=0 x=45 y=37 w=3 h=3
grow corner_ell: m=0 x=0 y=0 w=1 h=3
grow mask_31_on_20x12: m=0 x=0 y=0 w=12 h=20
mask ell_corner: ok=1 on=1 anchor=2,0 rows=1,1,1f
mask ell_default_anchor_clear: ok=0
mask one_by_one: ok=1 on=0 anchor=0,0 rows=1
mask cross_default_anchor: ok=1 on=1 anchor=1,1 rows=2,7,2
mask even_4x4: ok=1 on=1 anchor=2,2 rows=f,f,f,f
mask size_0: ok=0
mask size_0_rows: ok=0
mask size_32: ok=0
mask size_31: ok=1 on=1 anchor=15,15 rows=%s
mask anchor_outside: ok=0
mask anchor_negative: ok=0
mask anchor_cell_clear: ok=0
mask all_zero: ok=0
mask null_mask: ok=0
""" % ",".join(["7fffffff"] * 31)


def test_cspace_driver(tmp_path):
    exe = str(tmp_path / "cspace_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "cspace_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.splitlines() == EXPECTED.splitlines()


def test_kernel_body_on_the_host(tmp_path):
    """tests/cpp/cspace_kernel_driver.cpp: k_cspace_dilate's body as plain C++, every thread of every workgroup, under sanitizers, against
    a brute-force dilation -- whole maps and grown rectangles, widths with and without the dword staging path, masks up to 31 x 31"""
    exe = str(tmp_path / "cspace_kernel_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-attributes", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "cspace_kernel_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "320 cases, 0 bad"


def test_grow_rect_is_where_the_dilation_can_change():
    """the driver's grown rectangles against the numpy reference: changing raw cells inside the patch rectangle changes the dilation
    nowhere outside the grown rectangle, and somewhere on each of its four edges"""
    ell = np.array([[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.uint8)
    raw = np.zeros((48, 40), np.uint8)
    hit = raw.copy()
    hit[20:26, 10:14] = 200                                     # the patch {x=20, y=10, w=4, h=6}
    for anchor, (x, y, w, h) in (((2, 0), (20, 6, 8, 8)), ((0, 0), (18, 6, 8, 8))):
        ch = dilate_ref(hit, ell, anchor) != dilate_ref(raw, ell, anchor)
        rows, cols = np.where(ch.any(axis=1))[0], np.where(ch.any(axis=0))[0]
        assert (rows.min(), rows.max(), cols.min(), cols.max()) == (x, x + h - 1, y, y + w - 1)


def test_disc_is_the_harness_footprint():
    """cspace_disc(d) with the reference dilation == harness.dilate(., d), d = 1 .. 9: one definition"""
    rng = np.random.default_rng(5)
    raw = rng.integers(1, 256, (37, 29)).astype(np.uint8)
    for d in range(1, 10):
        m = ufm_amd.cspace_disc(d)
        assert m.dtype == np.uint8 and m.shape == ((1, 1) if d <= 1 else (2 * (d // 2) + 1,) * 2)
        assert m[m.shape[0] // 2, m.shape[1] // 2] == 1
        assert np.array_equal(dilate_ref(raw, m), ufm_amd.harness.dilate(raw, d)), d
    assert np.array_equal(ufm_amd.cspace_disc(3), [[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def test_harness_sends_raw_only_when_asked(monkeypatch):
    """run_mission against a stand-in for the pipes: by default the bytes on the wire are dilate(data_l) and its patches, as before the
    keyword existed; with planner_inflates=True they are data_l and its raw patches, and min_cost still comes from the inflated map"""
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
    data_l, data_h = h.simulation_data(img, 10)
    after, (top, left), rng_ = h.round_patch_update(data_l, data_h, (9, 12), 5)
    for kw, first, second in (({}, h.dilate(data_l, 5), h.dilate(after, 5)), ({"planner_inflates": True}, data_l, after)):
        trace, finished = h.run_mission(["x"], "a", "b", img, (12.0, 9.0), (2.0, 2.0), radius=5, cspace_diameter=5, **kw)
        assert finished and trace == [(12.0, 9.0)]
        blobs = [v for f, v in made[-1].sent if f == "bytes"]
        ints = [v for f, v in made[-1].sent if f == "i"]
        assert blobs[0] == first.tobytes()
        assert blobs[1] == np.ascontiguousarray(second[rng_[0], rng_[1]]).tobytes()
        assert ints[0] == (int(h.dilate(data_l, 5).min()),)           # the heuristic hint: from the inflated map either way
    assert made[0].sent != made[1].sent
