"""Trajectory scoring without a GPU: the four entry points exist (header, binding, library) and refuse a NULL handle before they
write anything; the binding's record is the header's ufm_score; and the segment walk of csrc/ufm_score_rect.h -- the text the kernel
runs one lane per segment -- is run on the host by tests/cpp/score_rect_driver.cpp, a program of its own under the address and
undefined-behaviour sanitizers, over rasters and paths this test writes to a file, and held to the float64 restatement of
tests/score_reference.py: the directed and the hostile paths of tests/score_cases.py on every map and threshold (none of them doubtful),
the 2 000 random ones, and the bound of length + width + 2 pieces per segment whatever the coordinates are.  What terminates here is
what tests/test_gpu_score.py then hands to the device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import score_cases as sc
import score_reference as sr
import ufm_amd
from ufm_amd_pkg import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
CHAIN = ufm_amd.tolerances.SCORE_FP64_CHAIN
NAMES = ["ufm_score_paths", "ufm_score_paths_device", "ufm_batch_score_paths", "ufm_batch_score_paths_device"]
SENTINEL = -12345


# ------------------------------------------------------------------------------------------------------------------- the surface
def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ufm_[a-z_0-9]+)\s*\(", txt)))


def test_symbols_exported():
    """The four calls are declared in include/ufm_score.h, which include/ufm.h includes (a C program that includes ufm.h alone calls
    them: test_record_is_the_headers_struct), are the binding's SCORE_SYMBOLS, bound with argument types, and exported by the library.
    They are not members of capi.SYMBOLS yet: that list and ufm.h's own text are held to each other and to 98 names by
    tests/test_capi_symbols.py and tests/test_capi_surface.py, which stay as they are; so the header and the list of these four stand
    beside them and are held to each other here, the same way."""
    assert _declared("ufm_score.h") == sorted(capi.SCORE_SYMBOLS) == sorted(NAMES)
    assert re.search(r'^#include "ufm_score\.h"$', open(os.path.join(ROOT, "include", "ufm.h")).read(), flags=re.M)
    lib = ufm_amd.load_library()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes and fn.argtypes[0] is ctypes.c_void_p and fn.restype is ctypes.c_int, name
        # the sweep of tests/test_capi_surface.py, for these four: a NULL handle, zero or NULL for everything else
        args = [0 if t is ctypes.c_int else None for t in fn.argtypes]
        assert fn(*args) == -22, name


def test_null_handle_is_invalid_and_writes_nothing():
    lib = ufm_amd.load_library()
    pts = np.array([[1.0, 2.0], [3.0, 4.5], [5.0, 5.0]], np.float32)
    off = np.array([0, 2, 3], np.int32)
    maps = np.zeros(2, np.int32)
    out = np.zeros(2, capi.SCORE_DTYPE)
    out["pieces"] = out["blocked_segment"] = SENTINEL
    args = (off.ctypes.data, pts.ctypes.data, out.ctypes.data)
    assert lib.ufm_score_paths(None, 2, *args) == -22
    assert lib.ufm_batch_score_paths(None, 2, maps.ctypes.data, *args) == -22
    assert lib.ufm_score_paths_device(None, 2, 3, *args) == -22
    assert lib.ufm_batch_score_paths_device(None, 0, 2, 3, *args) == -22
    assert (out["pieces"] == SENTINEL).all() and (out["blocked_segment"] == SENTINEL).all() and (out["cost"] == 0).all()


def test_record_is_the_headers_struct(tmp_path):
    """a C program that includes ufm.h alone and links libufm.so calls two of the entry points and prints sizeof(ufm_score), every
    member's offset and the short-piece threshold; ufm_score.h included alone, and first, compiles too"""
    names = list(capi.SCORE_DTYPE.names)
    src = tmp_path / "score.c"
    src.write_text('#include "ufm.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n  printf("%zu\\n", sizeof(ufm_score));\n'
                   '  if (ufm_score_paths(NULL, 1, NULL, NULL, NULL) != UFM_ERR_INVALID || ufm_batch_score_paths_device(NULL, 0, 1, 0, NULL, NULL, NULL) != UFM_ERR_INVALID) return 1;\n' +
                   "".join('  printf("%%zu %%zu\\n", offsetof(ufm_score, %s), sizeof(((ufm_score *)0)->%s));\n' % (n, n) for n in names) +
                   '  printf("%.17g\\n", UFM_SCORE_MIN_PIECE);\n  return 0;\n}\n')
    exe = tmp_path / "score"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + PKG, "-lufm", "-Wl,-rpath," + PKG])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(out[0]) == capi.SCORE_DTYPE.itemsize == 24
    for line, n in zip(out[1:], names):
        off, size = line.split()
        assert (int(off), int(size)) == (capi.SCORE_DTYPE.fields[n][1], capi.SCORE_DTYPE.fields[n][0].itemsize), n
    assert float(out[1 + len(names)]) == 2.0 ** -20 == sr.MIN_PIECE
    alone = tmp_path / "alone.c"
    alone.write_text('#include "ufm_score.h"\n#include "ufm.h"\nint main(void) { ufm_score s; ufm_stats t; (void)s; (void)t; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(alone)])
    rect = open(os.path.join(PKG, "csrc", "ufm_score_rect.h")).read()
    assert float(re.search(r"SCORE_MIN_PIECE\s*=\s*([0-9.eE+-]+);", rect).group(1)) == 2.0 ** -20


def test_path_arrays_of_the_binding():
    """score_paths takes a list of [n_i, 2] arrays or (points, offsets): the same flat arrays either way"""
    paths = [np.array([[1, 2], [3, 4]]), np.zeros((0, 2)), np.array([[5.5, 6.5]])]
    pts, off = capi._path_arrays(paths)
    assert pts.dtype == np.float32 and off.dtype == np.int32 and off.tolist() == [0, 2, 2, 3]
    assert pts.tolist() == [[1, 2], [3, 4], [5.5, 6.5]]
    pts2, off2 = capi._path_arrays((pts, off))
    assert np.array_equal(pts2, pts) and np.array_equal(off2, off)
    pts3, off3 = capi._path_arrays([])
    assert pts3.shape == (0, 2) and off3.tolist() == [0]


@pytest.mark.parametrize("planner", ["DFMPlanner<1>", "FieldDPlanner<0>", "ShiftedGridPlanner<2>"])
@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]])
def test_score_driver_type_checks(planner, define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DSCORE_PLANNER=" + planner] + define +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "include"),
                           os.path.join(ROOT, "tests", "cpp", "score_driver.cpp")])


# ------------------------------------------------------------------------------------------------------ the walk, on the host
DRIVER_DTYPE = np.dtype([("cost", "<f4"), ("cost_before", "<f4"), ("dist", "<f4"), ("blocked_at", "<f4"), ("blocked_segment", "<i4"),
                         ("pieces", "<i4"), ("most_pieces", "<i4"), ("most_lookups", "<i8")])


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """walk(cost, thr_uchar, paths[, offsets]) -> the driver's records"""
    tmp = tmp_path_factory.mktemp("score_rect")
    exe = str(tmp / "score_rect_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "score_rect_driver.cpp"), "-o", exe])
    count = [0]

    def run(cost, tu, paths, offsets=None):
        pts, off = sc.pack(paths)
        if offsets is not None:
            off = np.asarray(offsets, np.int32)
        count[0] += 1
        name = str(tmp / ("in%d.txt" % count[0]))
        with open(name, "w") as f:
            f.write("%d %d %d %d %d\n" % (cost.shape[0], cost.shape[1], tu, len(off) - 1, len(pts)))
            f.write(" ".join(str(int(v)) for v in cost.ravel()) + "\n")
            f.write(" ".join(str(int(v)) for v in off) + "\n")
            f.write(" ".join(str(int(v)) for v in pts.ravel().view(np.uint32)) + "\n")
        out = subprocess.run([exe, name], check=True, capture_output=True, text=True, timeout=120).stdout.split("\n")
        rec = np.zeros(len(off) - 1, DRIVER_DTYPE)
        for k in range(len(rec)):
            v = out[k].split()
            rec[k] = tuple(np.array([int(x)], np.uint32).view(np.float32)[0] for x in v[:4]) + tuple(int(x) for x in v[4:])
        return rec
    return run


MAPS = sc.maps()


@pytest.mark.parametrize("case", range(len(MAPS)), ids=[m[0] for m in MAPS])
def test_directed_paths_on_the_host(walk, case):
    name, cost, thr, tu = MAPS[case]
    cases = sc.directed(cost, tu)
    refs = [sr.score_path(p, cost, tu) for _, p in cases]
    assert not any(r["doubtful"] for r in refs), [n for (n, _), r in zip(cases, refs) if r["doubtful"]]
    rec = walk(cost, tu, [p for _, p in cases])
    for (what, _), r, ref in zip(cases, rec, refs):
        sc.check_record(r, ref, CHAIN, "%s: %s" % (name, what))
        assert r["most_pieces"] <= cost.shape[0] + cost.shape[1] + 2, what


def test_directed_set_covers_what_it_names():
    """on the 37 x 43 map at threshold 1.0 every directed case exists and is what its name says, by the reference"""
    name, cost, thr, tu = MAPS[0]
    assert cost.shape == (37, 43) and tu == 255
    cases = dict(sc.directed(cost, tu))
    ref = {k: sr.score_path(p, cost, tu) for k, p in cases.items()}
    free = lambda k: ref[k]["blocked_segment"] == -1
    for k in ("inside one cell", "free run along a row", "free run along a row, backwards", "free run along a column",
              "shallow in the free run", "steep in the free run", "diagonal between two obstacles",
              "diagonal between two obstacles, backwards", "anti-diagonal between two obstacles", "zero-length segment", "one point", "empty"):
        assert free(k), k
    assert ref["inside one cell"]["pieces"] == 1
    assert ref["free run along a row"]["pieces"] >= 4 and ref["free run along a column"]["pieces"] >= 4
    assert ref["shallow in the free run"]["pieces"] >= 4 and ref["steep in the free run"]["pieces"] >= 4
    for k in ("zero-length segment", "one point", "empty"):
        assert ref[k]["pieces"] == 0 and ref[k]["cost"] == 0.0 and ref[k]["dist"] == 0.0, k
    # the diagonal touches the two obstacles in the vertex only: two pieces, both charged
    assert ref["diagonal between two obstacles"]["pieces"] == 2
    r = ref["diagonal through an obstacle"]
    assert r["blocked_segment"] == 0 and abs(r["blocked_at"] - 1.0 / 3.0) < 1e-15 and r["pieces"] == 1
    for axis in ("x", "y"):
        for what in ("cheaper before", "cheaper behind", "obstacle before", "obstacle behind"):
            k = "on a line %s = k, %s" % (axis, what)
            assert free(k) and ref[k]["pieces"] == 1, k
        both = ref["on a line %s = k, both obstacles" % axis]
        assert both["blocked_segment"] == 0 and both["blocked_at"] == 0.0 and both["pieces"] == 0
    # the cheaper of the two cells: half a cell side times min(c1, c2)
    p = cases["on a line x = k, cheaper behind"]
    k_, j_ = int(p[0][0]), int(math.floor(p[0][1]))
    assert ref["on a line x = k, cheaper behind"]["cost"] == 0.5 * min(int(cost[k_ - 1, j_]), int(cost[k_, j_])) == 0.5 * int(cost[k_, j_])
    # a border is charged the one cell beside it (the other is outside): free as far as those cells are, blocked at the first obstacle
    L, W = cost.shape
    inner = {"border x = 0": cost[0, :], "border x = L": cost[L - 1, ::-1], "border y = 0": cost[:, 0], "border y = W": cost[::-1, W - 1]}
    for k, cells in inner.items():
        n_free = int(np.argmax(cells >= tu)) if (cells >= tu).any() else len(cells)
        assert ref[k]["pieces"] == n_free and (ref[k]["blocked_segment"] == -1) == (n_free == len(cells)), (k, n_free, ref[k])
    assert max(ref[k]["pieces"] for k in inner) >= 2
    assert ref["blocked in the first segment"]["blocked_segment"] == 0
    assert ref["blocked in a middle segment"]["blocked_segment"] == 2
    assert ref["blocked in the last segment"]["blocked_segment"] == len(cases["blocked in the last segment"]) - 2 == 2
    assert abs(ref["blocked in the last segment"]["blocked_at"] - 1.0 / 3.0) < 1e-15 and ref["blocked in the last segment"]["pieces"] == 3


@pytest.mark.parametrize("case", range(len(MAPS)), ids=[m[0] for m in MAPS])
def test_hostile_paths_on_the_host(walk, case):
    """leaving, entering, NaN, the infinities, +-1e30, +-FLT_MAX: every walk ends within length + width + 2 pieces per segment, and
    every record is the defined one"""
    name, cost, thr, tu = MAPS[case]
    cases = sc.hostile(cost, tu)
    refs = [sr.score_path(p, cost, tu) for _, p in cases]
    assert not any(r["doubtful"] for r in refs)
    rec = walk(cost, tu, [p for _, p in cases])
    limit = cost.shape[0] + cost.shape[1] + 2
    for (what, p), r, ref in zip(cases, rec, refs):
        assert r["most_pieces"] <= limit and r["most_lookups"] <= 2 * limit, (name, what, r)
        sc.check_record(r, ref, CHAIN, "%s: %s" % (name, what))
        if not np.isfinite(p).all() or what.startswith(("leaves", "enters", "outside", "from the border")):
            assert r["blocked_segment"] >= 0 and r["cost"] == np.inf, (name, what, r)


def test_garbage_offsets_on_the_host(walk):
    """the kernel's view of device offsets (the driver applies the same clamp): beyond the points, negative, decreasing"""
    name, cost, thr, tu = MAPS[0]
    paths = [p for _, p in sc.directed(cost, tu)[:6]]
    pts, off = sc.pack(paths)
    total = len(pts)
    bad = np.array([0, 2, total + 50, 5, -7, 3, 2 ** 31 - 1], np.int32)
    rec = walk(cost, tu, paths, offsets=bad)
    clamp = np.clip(bad.astype(np.int64), 0, total)
    for k in range(len(bad) - 1):
        a, b = int(clamp[k]), int(clamp[k + 1])
        ref = sr.score_path(pts[a:b] if b > a else pts[:0], cost, tu)
        sc.check_record(rec[k], ref, CHAIN, "offsets %d .. %d" % (bad[k], bad[k + 1]))


def test_random_paths_on_the_host(walk):
    name, cost, thr, tu = MAPS[0]
    paths = sc.random_paths(cost)
    assert len(paths) == 2000 and all(2 <= len(p) <= 40 for p in paths)
    allp = np.concatenate(paths)
    assert allp.min() >= -2.0 and allp[:, 0].max() <= cost.shape[0] + 2.0 and allp[:, 1].max() <= cost.shape[1] + 2.0
    refs = [sr.score_path(p, cost, tu) for p in paths]
    doubtful = sum(r["doubtful"] for r in refs)
    assert doubtful <= len(paths) // 100, doubtful
    n_free = sum(r["blocked_segment"] < 0 for r in refs)
    assert n_free >= 100 and len(paths) - n_free >= 100, n_free        # (both outcomes are well represented)
    rec = walk(cost, tu, paths)
    worst = [0.0, 0.0]
    for k, (r, ref) in enumerate(zip(rec, refs)):
        if not ref["doubtful"]:
            u = sc.check_record(r, ref, CHAIN, "random path %d" % k)
            worst = [max(a, b) for a, b in zip(worst, u)]
    print("random set on the host: %d doubtful, %d free; worst deviation in units of the bound: cost %.4f, dist %.4f" % (doubtful, n_free, worst[0], worst[1]))
