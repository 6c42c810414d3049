"""The graded footprint (ufm_set_cspace_graded, k_cspace_dilate_graded) against the flat one (ufm_set_cspace, k_cspace_dilate) at EQUAL
SUPPORT, on one GPU: the 31-cell disc flat -- the yardstick, the parent's kernel unchanged --, the same cells with 4 levels of drop, and
with 16.  HIP events on the engine's stream around the call (torch.cuda.Event on an ExternalStream); WARMUP untimed and REPEATS timed
repeats of every figure, the footprints alternating inside one process; medians and the spread are reported.
(a) ufm_set_map_device of a SIZE^2 raster, second and later calls on a handle (nothing allocated): the device-to-device copy into the raw
    store, ONE dilation of the whole map, the cost windows and the mean cost.  A planner without a footprint gives the part that is not
    the dilation.
(b) ufm_patch_map_device of a 20 x 20 raw patch: the raw store, the dilation of the grown 50 x 50 rectangle, the patch kernels.
Each graded planner's planning raster is checked against the numpy definition on a window around the last patch.
usage: cspace_graded_probe.py [--size N] [--repeats R] [--warmup W] [--out FILE]   (default FILE: profiles/cspace_graded_probe.txt)"""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ufm_amd

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cspace_graded_probe.txt"))
args = ap.parse_args()
assert args.repeats >= 5 and args.warmup >= 1, "at least 5 repeats and one warm-up"
size, seed = args.size, 7
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(a):
    a = np.asarray(a, np.float64)
    return "median %.1f us (min %.1f, max %.1f, %d repeats)" % (np.median(a), a.min(), a.max(), len(a))


disc = ufm_amd.cspace_disc(31)
ring = ufm_amd.cspace_cone(1, 31, 1)                       # the ring index 0 .. 15 of every cell of the disc of radius 15
assert ((ring != 255) | (disc == 0)).all()
graded16 = np.where(disc != 0, ring * 10, 255).astype(np.uint8)
graded4 = np.where(disc != 0, (ring // 4) * 40, 255).astype(np.uint8)
for g, n in ((graded4, 4), (graded16, 16)):
    assert np.array_equal(g != 255, disc != 0) and len(set(g.ravel().tolist()) - {255}) == n
FOOT = [("no footprint", None, None), ("flat 31-disc (k_cspace_dilate)", "flat", disc), ("graded, 4 levels", "graded", graded4),
        ("graded, 16 levels", "graded", graded16)]

raw0 = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
say("cspace_graded_probe: %d^2, seed %d, support %d cells of 31 x 31, %s" % (size, seed, int((disc != 0).sum()), ufm_amd.load_library().ufm_version().decode()))
dev_map = torch.from_numpy(raw0).cuda()             # (device buffers are torch tensors: plain pointers for the *_device calls)
planners = []
for name, kind, fp in FOOT:
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    p.reset(); p.set_occupancy_threshold(1)
    if kind == "flat":
        p.set_cspace(fp)
    elif kind == "graded":
        p.set_cspace_graded(fp)
    p.set_map_device(dev_map.data_ptr(), size, size)        # the first call allocates the engine's arrays: not what is compared
    planners.append((name, kind, fp, p, torch.cuda.ExternalStream(p.stream_ptr())))


def timed(st, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


# ---- (a) the whole map
t_map = {name: [] for name, *_ in FOOT}
for r in range(args.warmup + args.repeats):
    for name, kind, fp, p, st in planners:
        dt = timed(st, lambda: p.set_map_device(dev_map.data_ptr(), size, size))
        if r >= args.warmup:
            t_map[name].append(dt)
say("(a) ufm_set_map_device of a %d^2 raster, events on the engine's stream around the call:" % size)
base = np.median(t_map["no footprint"])
flat = np.median(t_map[FOOT[1][0]]) - base
for name, *_ in FOOT:
    extra = np.median(t_map[name]) - base
    say("    %-32s %s%s" % (name + ":", spread(t_map[name]), "" if name == "no footprint" else
                            "; over no footprint: %.1f us = %.2f x the flat kernel's" % (extra, extra / flat)))

# ---- (b) a 20 x 20 raw patch
for name, kind, fp, p, st in planners:
    p.set_start(*start); p.set_goal(*goal)
    assert p.step() == 0
rng = np.random.default_rng(seed)
t_patch = {name: [] for name, *_ in FOOT}
raw = raw0.copy()
bufs = []
for r in range(args.warmup + args.repeats):
    top, left = 40 + 9 * r, 36 + 11 * r
    patch = rng.integers(1, 255, (20, 20)).astype(np.uint8)
    raw[top:top + 20, left:left + 20] = patch
    bufs.append(torch.from_numpy(patch).cuda())
    for name, kind, fp, p, st in planners:
        dt = timed(st, lambda: p.patch_map_device(bufs[-1].data_ptr(), top, left, 20, 20))
        if r >= args.warmup:
            t_patch[name].append(dt)
        p.set_start(start[0] + r, start[1] + r)
        assert p.step() == 0                                # (outside the timed window: the patch is consumed, nothing piles up)
say("(b) ufm_patch_map_device of a 20 x 20 raw patch (grown to 50 x 50 with a footprint), events around the call:")
base = np.median(t_patch["no footprint"])
for name, *_ in FOOT:
    say("    %-32s %s%s" % (name + ":", spread(t_patch[name]), "" if name == "no footprint" else
                            "; %.2f x the flat footprint's" % (np.median(t_patch[name]) / np.median(t_patch[FOOT[1][0]]))))
# the rasters are the definition's, on the window the last patch can reach (and what that window reads)
x0, y0, x1, y1 = max(top - 15, 0), max(left - 15, 0), min(top + 35, size), min(left + 35, size)
wx0, wy0, wx1, wy1 = max(x0 - 15, 0), max(y0 - 15, 0), min(x1 + 15, size), min(y1 + 15, size)
for name, kind, fp, p, st in planners:
    got = p.read_map(size, size)[x0:x1, y0:y1]
    drop = None if kind is None else (np.where(fp != 0, 0, 255).astype(np.uint8) if kind == "flat" else fp)
    want = raw[x0:x1, y0:y1] if drop is None else ufm_amd.harness.dilate_graded(raw[wx0:wx1, wy0:wy1], drop)[x0 - wx0:x1 - wx0, y0 - wy0:y1 - wy0]
    assert np.array_equal(got, want), "%s: the planning raster around the last patch is not the definition's" % name
    p.close()
say("    every planning raster equals the numpy definition on the %d x %d window around the last patch" % (x1 - x0, y1 - y0))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
