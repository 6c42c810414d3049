"""The cost census (ufm_track_costs) and the automatic heuristic multiplier ("auto_multiplier"), on one GPU.  One warm-up and REPEATS
timed repeats of every figure, the sides of a comparison alternating inside one process; medians with min - max are reported.
(a) ufm_set_map of a 4096^2 raster with the census off and on, for three rasters: uniform random bytes, a constant one, a binary one
    (wall time of the call, which ends in a stream synchronise: what the census adds is one k_census_build over the map; the constant
    and binary rasters are the ones its aggregation in front of the LDS atomics exists for).
(b) the headline replan loop with heuristic keys (FD-1, 4096^2, seed 7, 100 replans with a moving start), a 5 x 5 footprint and RAW
    11 x 11 host patches, four ways:
      1 "fed":      the multiplier set by the host before every step (census off) -- the parent commit's loop.  The minima are worked out
                    before the timed loop; what it costs a host to GET them the way the harness does today, a dilation and a minimum of
                    the whole map per move, is timed separately on a few moves and reported per move;
      2 "auto":     "auto_multiplier" (census on, the step waits for the published minimum);
      3 "floor":    census off, one constant multiplier;
      4 "counted":  census on, the multiplier fed as in 1 -- against 2: what waiting for the published minimum costs.
    All four must end with the same planning raster and path.
(c) the same loop without a footprint, census off and on (multiplier fed): the price of the held route the census declines.
usage: census_probe.py [--size N] [--replans K] [--repeats R] [--out FILE]   (default FILE: profiles/census_probe.txt)"""
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
ap.add_argument("--host-moves", type=int, default=3, help="moves on which the host's whole-map dilation + minimum is timed")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_probe.txt"))
args = ap.parse_args()
assert args.repeats >= 5, "at least 5 repeats"
size, seed, n = args.size, 7, args.replans
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(a):
    a = np.asarray(a, np.float64)
    return "median %.3f ms (min %.3f, max %.3f, %d repeats)" % (np.median(a), a.min(), a.max(), len(a))


raw0 = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=n, size=11))
say("census_probe: %d^2, seed %d, %s" % (size, seed, ufm_amd.load_library().ufm_version().decode()))

# ---- (a) set_map with the census off and on
rng = np.random.default_rng(seed)
kinds = [("uniform random bytes", rng.integers(0, 256, (size, size)).astype(np.uint8)),
         ("constant (all 7)", np.full((size, size), 7, np.uint8)),
         ("binary {1, 255}", (1 + 254 * (rng.integers(0, 4, (size, size)) == 0)).astype(np.uint8))]
say("(a) ufm_set_map of a %d^2 raster, second call on a handle (nothing allocated), wall incl. its stream synchronise:" % size)
for name, r in kinds:
    t_off, t_on = [], []
    for k in range(args.repeats + 1):
        for on, acc in ((False, t_off), (True, t_on)):
            p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
            p.set_occupancy_threshold(1)
            if on:
                p.track_costs()
            p.set_map(r)
            t = time.perf_counter(); p.set_map(r); dt = (time.perf_counter() - t) * 1e3
            if k:
                acc.append(dt)
            elif on:
                hist, mn, mx = p.read_cost_census()
                assert np.array_equal(hist, np.bincount(r.ravel(), minlength=256).astype(np.uint64)) and (mn, mx) == (int(r.min()), int(r.max()))
            p.close()
    say("    %-22s census off: %s" % (name + ",", spread(t_off)))
    say("    %-22s census on:  %s  -> the census adds %.3f ms (medians)" % ("", spread(t_on), np.median(t_on) - np.median(t_off)))

# ---- (b), (c) the replan loop
disc5 = ufm_amd.cspace_disc(5)


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


def minima(mask):
    """the planning raster's minimum before the plan and before every replan: the raster kept on the host, outside any timed loop, the
    window a patch can change dilated anew; the harness' own way, the whole map dilated per move, is timed on the first moves"""
    raw = raw0.copy()
    r = 0 if mask is None else mask.shape[0] // 2
    t = time.perf_counter()
    planning = raw.copy() if mask is None else dilate(raw, mask)
    out, whole = [int(planning.min())], [(time.perf_counter() - t) * 1e3]
    for i, (k, s, top, left, patch) in enumerate(script):
        h, w = patch.shape
        raw[top:top + h, left:left + w] = patch
        if mask is not None and i < args.host_moves:
            t = time.perf_counter(); full = dilate(raw, mask); mn = int(full.min()); whole.append((time.perf_counter() - t) * 1e3)
        x0, y0, x1, y1 = max(top - r, 0), max(left - r, 0), min(top + h + r, size), min(left + w + r, size)
        wx0, wy0, wx1, wy1 = max(x0 - r, 0), max(y0 - r, 0), min(x1 + r, size), min(y1 + r, size)
        win = raw[wx0:wx1, wy0:wy1] if mask is None else dilate(raw[wx0:wx1, wy0:wy1], mask)
        planning[x0:x1, y0:y1] = win[x0 - wx0:x1 - wx0, y0 - wy0:y1 - wy0]
        if mask is not None and i < args.host_moves:
            assert np.array_equal(full, planning) and mn == int(planning.min())
        out.append(int(planning.min()))
    return out, whole[1:], planning


def loop(mask, mins, census, auto, fed):
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, True)
    p.reset(); p.set_occupancy_threshold(1)
    if mask is not None:
        p.set_cspace(mask)
    if census:
        p.track_costs()
    if auto:
        p.set_param("auto_multiplier", 1)
    p.set_heuristic_multiplier(float(mins[0]))
    p.set_map(raw0); p.set_start(*start); p.set_goal(*goal)
    assert p.step() == 0
    t = time.perf_counter()
    for i, (k, s, top, left, patch) in enumerate(script):
        p.patch_map(patch, top, left)
        if fed:
            p.set_heuristic_multiplier(float(mins[i + 1]))
        p.set_start(*s)
        assert p.step() == 0
    dt = (time.perf_counter() - t) * 1e3
    return p, dt


def compare(mask, sides, mins, planning):
    res = {name: [] for name, _ in sides}
    info = {}
    for r in range(args.repeats + 1):
        out = {}
        for name, kw in sides:
            p, dt = loop(mask, mins, **kw)
            if r == 0:
                out[name] = (p.read_map(size, size), p.extract_path(max_steps=200))
                if kw["census"]:
                    hist, mn, mx = p.read_cost_census()
                    assert np.array_equal(hist, np.bincount(planning.ravel(), minlength=256).astype(np.uint64)) and mn == mins[-1]
                if kw["auto"]:
                    assert p.heuristic_multiplier() == float(mins[-1])
            info[name] = (p.stats.region_replans, p.stats.graphs_instantiated)
            p.close()
            if r:
                res[name].append(dt)
        if r == 0:
            first = sides[0][0]
            assert np.array_equal(out[first][0], planning), "the planning raster is not the host's"
            for name, _ in sides[1:]:
                assert np.array_equal(out[name][0], out[first][0]), "the planning rasters differ"
                assert np.array_equal(out[name][1][0], out[first][1][0]) and out[name][1][2] == out[first][1][2], "the paths differ"
    return res, info


mins5, whole, planning5 = minima(disc5)
say("(b) FD-1 with heuristic keys, %d replans with a moving start, 5 x 5 footprint (%d cells), raw 11 x 11 host patches; wall of the loop" % (n, int(disc5.sum())))
say("    patch_map [+ set_heuristic_multiplier] + set_start + step; the planning raster's minimum over the mission: %s" % sorted(set(mins5)))
sides = [("fed", dict(census=False, auto=False, fed=True)), ("auto", dict(census=True, auto=True, fed=False)),
         ("floor", dict(census=False, auto=False, fed=False)), ("counted", dict(census=True, auto=False, fed=True))]
res, info = compare(disc5, sides, mins5, planning5)
label = {"fed": "1 multiplier fed by the host, census off (the parent's loop):", "auto": "2 \"auto_multiplier\" (census on):",
         "floor": "3 census off, constant multiplier (the floor):", "counted": "4 census on, multiplier fed (no wait for the minimum):"}
for name, _ in sides:
    say("    %-62s %s = %.1f us per replan; %d of %d replans through the block kernel, %d graphs" % (
        label[name], spread(res[name]), 1e3 * np.median(res[name]) / n, info[name][0], n, info[name][1]))
say("      what side 1 leaves out -- getting the minimum the harness' way, a numpy dilation + minimum of the whole map per move: %s" % (
    ("median %.0f ms per move (%d moves timed)" % (np.median(whole), len(whole))) if whole else "not measured"))
m = {k: np.median(v) for k, v in res.items()}
say("    automatic against host-fed: %+.3f ms per %d replans (medians; the repeats of the two sides spread over %.3f and %.3f ms)" % (
    m["auto"] - m["fed"], n, max(res["fed"]) - min(res["fed"]), max(res["auto"]) - min(res["auto"])))
say("    over the floor: automatic %+.1f us per replan, host-fed %+.1f us per replan; the wait for the published minimum (2 against 4): %+.1f us per replan" % (
    1e3 * (m["auto"] - m["floor"]) / n, 1e3 * (m["fed"] - m["floor"]) / n, 1e3 * (m["auto"] - m["counted"]) / n))

mins1, _, planning1 = minima(None)
sides = [("off", dict(census=False, auto=False, fed=True)), ("on", dict(census=True, auto=False, fed=True))]
res, info = compare(None, sides, mins1, planning1)
say("(c) the same loop without a footprint (small host patches: held for the block kernel while the census is off, staged and applied at the call while it is on):")
for name, _ in sides:
    say("    census %-4s %s = %.1f us per replan; %d of %d replans through the block kernel" % (
        name + ":", spread(res[name]), 1e3 * np.median(res[name]) / n, info[name][0], n))
say("    -> the declined held route and the census kernels cost %+.1f us per replan (medians)" % (1e3 * (np.median(res["on"]) - np.median(res["off"])) / n))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
