"""Map preparation in the engine (ufm_set_image) against the route it replaces, on one GPU.  A measurement tool, not part of the product.
A seeded synth bitmap (the complement of synth.cost_map), 13 Gaussian taps, penalty 15; per configuration the two sides alternate inside
one process, one warm-up and REPEATS timed repeats each; medians with min - max.
  "host":      the parent commit's route -- harness.simulation_data in numpy, then ufm_set_map + ufm_set_survey of the two rasters it
               made (two rasters of the map's size over PCIe); the numpy part is also reported on its own;
  "set_image": ufm_set_image of the bitmap (one raster over PCIe, both made by k_prepare).
(a) wall time of the two sides for a single planner; (b) k_prepare's own time, from HIP events on the dispatch (ufm_set_profiling), and
what that is in bytes per second over 1 x read + 2 x written rasters; (c) both for a batch of maps.  Both sides must leave the same rasters.
usage: prepare_probe.py [--size N] [--batch M] [--batch-size N] [--repeats R] [--out FILE]   (default FILE: profiles/prepare_probe.txt)"""
import argparse
import ctypes as C
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import ufm_amd
from ufm_amd_pkg import capi, harness

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--batch-size", type=int, default=2048)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_probe.txt"))
args = ap.parse_args()
seed, ksize, penalty = 7, 13, 15
taps = capi.gaussian_taps(ksize)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(a, unit="ms"):
    a = np.asarray(a, np.float64)
    return "median %.3f %s (min %.3f, max %.3f, %d repeats)" % (np.median(a), unit, a.min(), a.max(), len(a))


def bitmap(size, m=0):
    return np.ascontiguousarray(255 - ufm_amd.synth.cost_map(seed + 10 * m, size, size)).astype(np.uint8)


lib = ufm_amd.load_library()
lib.ufm_debug_prepare_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.ufm_debug_batch_prepare_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
say("prepare_probe: seed %d, %d taps, penalty %d, %s" % (seed, ksize, penalty, lib.ufm_version().decode()))


def single(size):
    img = bitmap(size)
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    p.reset(); p.set_occupancy_threshold(1)
    p.L.ufm_set_profiling(p.h, 1)
    res = {"numpy": [], "host": [], "set_image": [], "kernel": []}
    ms = C.c_float(0)
    for r in range(args.repeats + 1):
        t0 = time.perf_counter()
        lo, hi = harness.simulation_data(img, penalty, ksize)
        t1 = time.perf_counter()
        p.set_map(lo); p.set_survey(hi)
        t2 = time.perf_counter()
        if r == 0:
            want = (p.read_map(size, size), p.read_survey(size, size))
        t3 = time.perf_counter()
        p.set_image(img, taps=taps, penalty=penalty)
        t4 = time.perf_counter()
        assert lib.ufm_debug_prepare_ms(p.h, C.byref(ms)) == 0
        if r == 0:
            got = (p.read_map(size, size), p.read_survey(size, size))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the sides leave different rasters"
        else:
            res["numpy"].append((t1 - t0) * 1e3); res["host"].append((t2 - t0) * 1e3); res["set_image"].append((t4 - t3) * 1e3); res["kernel"].append(ms.value)
    p.close()
    return res


def batch(n, size):
    imgs = [bitmap(size, m) for m in range(n)]
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, False)
    b.set_occupancy_threshold(1)
    b.L.ufm_batch_set_profiling(b.h, 1)
    res = {"numpy": [], "host": [], "set_image": [], "kernel": []}
    ms = C.c_float(0)
    for r in range(args.repeats + 1):
        t_np = 0.0
        t0 = time.perf_counter()
        for m in range(n):
            ta = time.perf_counter()
            lo, hi = harness.simulation_data(imgs[m], penalty, ksize)
            t_np += time.perf_counter() - ta
            b.set_map(m, lo); b.set_survey(m, hi)
        t2 = time.perf_counter()
        if r == 0:
            want = [(b.read_map(m, size, size), b.read_survey(m, size, size)) for m in range(n)]
        t3 = time.perf_counter()
        k_ms = 0.0
        for m in range(n):
            b.set_image(m, imgs[m], taps=taps, penalty=penalty)
        t4 = time.perf_counter()
        if r == 0:
            for m in range(n):
                assert np.array_equal(b.read_map(m, size, size), want[m][0]) and np.array_equal(b.read_survey(m, size, size), want[m][1]), "the sides leave different rasters"
        else:
            for m in range(n):              # (one more round, untimed by the wall clock: the events of each map's own launch)
                b.set_image(m, imgs[m], taps=taps, penalty=penalty)
                assert lib.ufm_debug_batch_prepare_ms(b.h, m, C.byref(ms)) == 0
                k_ms += ms.value
            res["numpy"].append(t_np * 1e3); res["host"].append((t2 - t0) * 1e3); res["set_image"].append((t4 - t3) * 1e3); res["kernel"].append(k_ms)
    b.close()
    return res


def report(title, res, cells):
    say(title)
    say("    host: simulation_data + set_map + set_survey:  %s" % spread(res["host"]))
    say("    ... of which simulation_data (numpy):          %s" % spread(res["numpy"]))
    say("    set_image:                                     %s" % spread(res["set_image"]))
    say("    set_image against the host route: %.1f x (medians); against set_map + set_survey alone: %.2f x" % (
        np.median(res["host"]) / np.median(res["set_image"]), (np.median(res["host"]) - np.median(res["numpy"])) / np.median(res["set_image"])))
    k = np.asarray(res["kernel"], np.float64)
    say("    k_prepare, HIP events on the dispatch:         %s" % spread(k))
    gbs = 3.0 * cells / (k * 1e-3) / 1e9
    say("    ... over 1 x read + 2 x written rasters (%d bytes): median %.1f GB/s (min %.1f, max %.1f)" % (3 * cells, np.median(gbs), gbs.min(), gbs.max()))


report("(a, b) single planner, %d^2:" % args.size, single(args.size), args.size * args.size)
report("(c) batch of %d maps, %d^2 each, one call and one launch per map:" % (args.batch, args.batch_size), batch(args.batch, args.batch_size),
       args.batch * args.batch_size * args.batch_size)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
