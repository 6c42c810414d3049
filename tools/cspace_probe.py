"""C-space inflation in the engine (ufm_set_cspace) against inflation on the host, on one GPU.  One warm-up and REPEATS timed repeats of
every figure, the two sides of a comparison alternating inside one process; medians (and the spread) are reported.
(a) ufm_set_map of a 4096^2 raster with and without a 15 x 15 disc: wall time of the call, which ends in a stream synchronise
    (what the footprint adds: the copy into the raw store's place is the same copy, plus one k_cspace_dilate over the whole map).
(b) the headline replan loop (FD-1, 4096^2, seed 7, 100 replans with a moving start) with a 5 x 5 footprint and RAW 11 x 11 host patches,
    against the same loop WITHOUT a footprint -- the code path of a build without the feature: off changes no route -- fed 15 x 15 patches
    inflated on the host with numpy from a host copy of the raw raster (the window around the patch only, shift and max); the host
    inflation is timed inside the loop and also reported on its own.  Both sides must end with the same planning raster and path.
usage: cspace_probe.py [--size N] [--replans K] [--repeats R] [--out FILE]   (default FILE: profiles/cspace_probe.txt)"""
import argparse
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import ufm_amd

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--replans", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cspace_probe.txt"))
args = ap.parse_args()
assert args.repeats >= 5, "at least 5 repeats"
size, seed = args.size, 7
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def dilate(raw, mask):
    """shift and max from the definition (include/ufm.h), anchor at the centre, cells outside ignored"""
    mh, mw = mask.shape
    ar, ac = mh // 2, mw // 2
    L, W = raw.shape
    out = np.zeros_like(raw)
    for a in range(mh):
        for b in range(mw):
            if mask[a, b]:
                di, dj = a - ar, b - ac
                i0, i1, j0, j1 = max(0, -di), min(L, L - di), max(0, -dj), min(W, W - dj)
                if i0 < i1 and j0 < j1:
                    np.maximum(out[i0:i1, j0:j1], raw[i0 + di:i1 + di, j0 + dj:j1 + dj], out=out[i0:i1, j0:j1])
    return out


def spread(a):
    a = np.asarray(a, np.float64)
    return "median %.3f ms (min %.3f, max %.3f, %d repeats)" % (np.median(a), a.min(), a.max(), len(a))


raw0 = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=args.replans, size=11))
say("cspace_probe: %d^2, seed %d, %s" % (size, seed, ufm_amd.load_library().ufm_version().decode()))

# ---- (a) set_map with and without a 15 x 15 disc
disc15 = ufm_amd.cspace_disc(15)
t_off, t_on = [], []
for r in range(args.repeats + 1):
    for mask, acc in ((None, t_off), (disc15, t_on)):
        p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
        p.set_occupancy_threshold(1)
        if mask is not None:
            p.set_cspace(mask)
        p.set_map(raw0)                       # the first call allocates the engine's arrays: not what is compared
        t = time.perf_counter(); p.set_map(raw0); dt = (time.perf_counter() - t) * 1e3
        if r:
            acc.append(dt)
        if mask is not None and r == 0:
            assert np.array_equal(p.read_map(size, size), dilate(raw0, disc15)), "planning raster != dilate(raw)"
        p.close()
say("(a) ufm_set_map of a %d^2 raster, second call on a handle (nothing allocated), wall incl. its stream synchronise:" % size)
say("    no footprint:          %s" % spread(t_off))
say("    15 x 15 disc (%d cells): %s" % (int(disc15.sum()), spread(t_on)))
say("    -> the footprint adds %.3f ms (medians): one dilation of the whole map on the device" % (np.median(t_on) - np.median(t_off)))
t = time.perf_counter(); dilate(raw0, disc15); say("    for scale: the same dilation with numpy on the host: %.0f ms" % ((time.perf_counter() - t) * 1e3))

# ---- (b) the replan loop: engine-inflated raw patches against host-inflated patches on a planner without a footprint
disc5 = ufm_amd.cspace_disc(5)
planning0 = dilate(raw0, disc5)


def planner(mask, first_map):
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    p.reset(); p.set_occupancy_threshold(1)
    if mask is not None:
        p.set_cspace(mask)
    p.set_map(first_map); p.set_start(*start); p.set_goal(*goal)
    assert p.step() == 0
    return p


def loop_engine():
    p = planner(disc5, raw0)
    t = time.perf_counter()
    for k, s, top, left, patch in script:
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
    dt = (time.perf_counter() - t) * 1e3
    return p, dt, 0.0, p.stats.region_replans


def loop_host():
    p = planner(None, planning0)
    raw = raw0.copy()
    host = 0.0
    t = time.perf_counter()
    for k, s, top, left, patch in script:
        th = time.perf_counter()
        h, w = patch.shape
        raw[top:top + h, left:left + w] = patch
        x0, y0, x1, y1 = max(top - 2, 0), max(left - 2, 0), min(top + h + 2, size), min(left + w + 2, size)      # the grown rectangle
        wx0, wy0, wx1, wy1 = max(x0 - 2, 0), max(y0 - 2, 0), min(x1 + 2, size), min(y1 + 2, size)                # ... and what it reads
        big = np.ascontiguousarray(dilate(raw[wx0:wx1, wy0:wy1], disc5)[x0 - wx0:x1 - wx0, y0 - wy0:y1 - wy0])
        host += time.perf_counter() - th
        p.patch_map(big, x0, y0); p.set_start(*s)
        assert p.step() == 0
    dt = (time.perf_counter() - t) * 1e3
    return p, dt, host * 1e3, p.stats.region_replans


res = {"engine": [], "host": []}
hostpart, regions = [], {}
for r in range(args.repeats + 1):
    out = {}
    for name, fn in (("engine", loop_engine), ("host", loop_host)):
        p, dt, hp, reg = fn()
        out[name] = (p.read_map(size, size), p.extract_path(max_steps=200))
        p.close()
        regions[name] = reg
        if r:
            res[name].append(dt)
            if name == "host":
                hostpart.append(hp)
    if r == 0:      # the two sides computed the same thing
        assert np.array_equal(out["engine"][0], out["host"][0]), "the two planning rasters differ"
        assert np.array_equal(out["engine"][1][0], out["host"][1][0]) and out["engine"][1][2] == out["host"][1][2], "the two paths differ"
n = args.replans
say("(b) FD-1, %d replans with a moving start, 5 x 5 footprint (%d cells), raw 11 x 11 host patches; wall of the loop patch_map + set_start + step:" % (n, int(disc5.sum())))
say("    engine inflates (ufm_set_cspace, raw patches):                     %s = %.1f us per replan; %d of %d replans through the block kernel" % (
    spread(res["engine"]), 1e3 * np.median(res["engine"]) / n, regions["engine"], n))
say("    host inflates (numpy, window around the patch) + no footprint:     %s = %.1f us per replan; %d of %d through the block kernel" % (
    spread(res["host"]), 1e3 * np.median(res["host"]) / n, regions["host"], n))
say("      of which the host inflation itself:                              %s = %.1f us per replan" % (spread(hostpart), 1e3 * np.median(hostpart) / n))
say("      -> without it (the parent's path alone, pre-inflated patches):   median %.3f ms = %.1f us per replan" % (
    np.median(res["host"]) - np.median(hostpart), 1e3 * (np.median(res["host"]) - np.median(hostpart)) / n))
say("    comparison: engine-inflated / (host inflation + parent's path) = %.3f (medians); same planning raster and path on both sides" % (
    np.median(res["engine"]) / np.median(res["host"])))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
