"""The sensor reveal (ufm_set_sensor / ufm_set_survey / ufm_reveal) against the route it replaces, host patches, on one GPU: FD-1 on a
4096^2 map, a disc of radius 15 as the field of view, 100 moves along the diagonal.  A measurement tool, not part of the product.
Per configuration the two sides alternate inside one process, one warm-up and REPEATS timed repeats each; medians with min - max.
  "host":   the parent commit's route -- the host keeps the raster, copies the survey's disc into it, cuts the bounding rectangle
            (numpy, on the rectangle only) and hands it over with ufm_patch_map; timed twice: with that host work inside the loop (what a
            simulator pays), and with the patches cut beforehand (the engine's share alone);
  "reveal": ufm_reveal with the position, nothing else.
Every loop is patch / reveal + set_start + step per move; a step is synchronous, so the wall time of the loop is device time plus the
host's.  Both sides must end with the same planning raster and the same path.
(1) a single planner, no footprint, no census; (2) a single planner with the 5 x 5 footprint (--inflate 5) and the census on
("auto_multiplier", heuristic keys); (3) a batch of 8 maps, per round 8 host patches against one ufm_batch_reveal.
usage: reveal_probe.py [--size N] [--moves K] [--repeats R] [--batch M] [--out FILE]   (default FILE: profiles/reveal_probe.txt)"""
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
ap.add_argument("--moves", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--radius", type=int, default=15)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reveal_probe.txt"))
args = ap.parse_args()
size, seed, n, radius = args.size, 7, args.moves, args.radius
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(a):
    a = np.asarray(a, np.float64)
    return "median %.3f ms (min %.3f, max %.3f, %d repeats)" % (np.median(a), a.min(), a.max(), len(a))


disc = ufm_amd.sensor_disc(radius)
start, goal = ufm_amd.synth.start_goal(size, size)
moves = [s for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=n, size=11)]
centres = [(int(round(s[0])), int(round(s[1]))) for s in moves]
say("reveal_probe: %d^2, seed %d, radius %d (%d of %d cells seen), %d moves, %s" % (
    size, seed, radius, int(disc.sum()), disc.size, n, ufm_amd.load_library().ufm_version().decode()))


def host_patch(cur, survey, row, col):
    """round_patch_update on the rectangle alone: the disc copied into the host's raster, the clipped bounding rectangle cut"""
    L, W = cur.shape
    x0, y0, x1, y1 = max(row - radius, 0), max(col - radius, 0), min(row + radius + 1, L), min(col + radius + 1, W)
    sub = disc[x0 - (row - radius):x1 - (row - radius), y0 - (col - radius):y1 - (col - radius)].astype(bool)
    np.copyto(cur[x0:x1, y0:y1], survey[x0:x1, y0:y1], where=sub)
    return np.ascontiguousarray(cur[x0:x1, y0:y1]), x0, y0


def maps(m):
    return ufm_amd.synth.cost_map(seed + 10 * m, size, size), ufm_amd.synth.cost_map(seed + 10 * m + 5, size, size, obstacles=False)


def single(side, inflate, raw0, survey, precut):
    heur = inflate
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, heur)
    p.reset(); p.set_occupancy_threshold(1); p.set_heuristic_multiplier(1.0)
    if inflate:
        p.set_cspace(ufm_amd.cspace_disc(5))
        p.set_param("auto_multiplier", 1)
    p.set_map(raw0); p.set_start(*start); p.set_goal(*goal)
    if side == "reveal":
        p.set_sensor(disc); p.set_survey(survey)
    assert p.step() == 0
    cur = raw0.copy()
    t = time.perf_counter()
    for i, s in enumerate(moves):
        if side == "reveal":
            p.reveal(*centres[i])
        elif precut is not None:
            p.patch_map(*precut[i])
        else:
            p.patch_map(*host_patch(cur, survey, *centres[i]))
        p.set_start(*s)
        assert p.step() == 0
    return p, (time.perf_counter() - t) * 1e3


def batch(side, rasters, precut):
    m = len(rasters)
    b = ufm_amd.BatchPlanner(m, ufm_amd.ALGO_FD, 1, False)
    b.set_occupancy_threshold(1)
    for i, (raw0, survey) in enumerate(rasters):
        b.set_map(i, raw0); b.set_start(i, *start); b.set_goal(i, *goal)
    if side == "reveal":
        b.set_sensor(disc)
        for i, (raw0, survey) in enumerate(rasters):
            b.set_survey(i, survey)
    assert b.step() == 0
    curs = [r[0].copy() for r in rasters]
    t = time.perf_counter()
    for k, s in enumerate(moves):
        if side == "reveal":
            b.reveal([centres[k]] * m)
        else:
            for i in range(m):
                b.patch_map(i, *(precut[i][k] if precut is not None else host_patch(curs[i], rasters[i][1], *centres[k])))
        for i in range(m):
            b.set_start(i, *s)
        assert b.step() == 0
    return b, (time.perf_counter() - t) * 1e3


def precut_of(raw0, survey):
    cur = raw0.copy()
    return [host_patch(cur, survey, *c) for c in centres]


def compare(title, run, check):
    sides = [("host, cutting in the loop", "host", False), ("host, patches cut beforehand", "host", True), ("reveal", "reveal", False)]
    res = {name: [] for name, _, _ in sides}
    for r in range(args.repeats + 1):
        outs = []
        for name, side, pre in sides:
            h, dt = run(side, pre)
            if r == 0:
                outs.append(check(h))
            h.close()
            if r:
                res[name].append(dt)
        if r == 0:
            for o in outs[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(o, outs[0])), "the sides end differently"
    say(title)
    for name, _, _ in sides:
        say("    %-30s %s = %.1f us per move" % (name + ":", spread(res[name]), 1e3 * np.median(res[name]) / n))
    med = {k: np.median(v) for k, v in res.items()}
    say("    reveal against host patches cut in the loop: %+.1f us per move; against patches cut beforehand: %+.1f us per move (medians)" % (
        1e3 * (med["reveal"] - med["host, cutting in the loop"]) / n, 1e3 * (med["reveal"] - med["host, patches cut beforehand"]) / n))


raw0, survey = maps(0)
pre0 = precut_of(raw0, survey)
single_check = lambda p: (p.read_map(size, size), p.extract_path(max_steps=200)[0])
compare("(1) single planner, no footprint, no census (small host patches are held for the block kernel: no patch kernel at all on that side):",
        lambda side, pre: single(side, False, raw0, survey, pre0 if pre else None), single_check)
compare("(2) single planner, 5 x 5 footprint and census (\"auto_multiplier\", heuristic keys): raw store, re-dilation and census correction on both sides:",
        lambda side, pre: single(side, True, raw0, survey, pre0 if pre else None), single_check)
rasters = [maps(m) for m in range(args.batch)]
pres = [precut_of(*r) for r in rasters]
compare("(3) batch of %d maps: %d host patches per round against one ufm_batch_reveal:" % (args.batch, args.batch),
        lambda side, pre: batch(side, rasters, pres if pre else None),
        lambda b: tuple(b.read_map(i, size, size) for i in range(args.batch)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
