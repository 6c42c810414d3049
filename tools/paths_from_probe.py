"""Position queries against the loop they replace: Field D* level 1, 2048^2 (seed 7), `focused = 0`, 1 024 hashed start positions
(vertices and points on cell edges at k/16), max_steps 20.  Wall time, host clock around calls that end in a stream synchronise, of
  (a) ONE ufm_extract_paths_from call with room for every way point and step cost,
  (b) the same call in its totals-only form (no buffers),
  (c) the loop ufm_set_start + ufm_extract_path, start by start: a launch, a synchronise and a copy per path,
each 5 times after one warm-up round, alternating; medians, the ratio (c) / (a), and that (a) and (c) returned the same bits.
usage: paths_from_probe.py [out.txt] [size] [n_starts]   (default out: profiles/paths_from_probe.txt)"""
import ctypes as C
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import ufm_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paths_from_probe.txt")
size = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
seed, max_steps, rounds = 7, 20, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


cost = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
h = ufm_amd.synth.h64
starts = np.zeros((n, 2), np.float32)
for k in range(n):
    x, y = int(h(seed, k, 1)) % size, int(h(seed, k, 2)) % size
    frac = (1 + int(h(seed, k, 3)) % 15) / 16.0
    kind = int(h(seed, k, 4)) % 3          # a vertex, a point on an edge along x, one on an edge along y
    starts[k] = (x + (frac if kind == 1 else 0.0), y + (frac if kind == 2 else 0.0))

p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
p.reset()
p.set_param("focused", 0)
p.set_occupancy_threshold(1.0)
p.set_map(cost)
p.set_start(*start)
p.set_goal(*goal)
assert p.step() == 0
L, hd = p.L, p.h
cap_p, cap_c = 3 * max_steps + 1, 2 * max_steps
pts = np.zeros((n, cap_p, 2), np.float32)
costs = np.zeros((n, cap_c), np.float32)
info = (ufm_amd.capi.PathInfo * n)()
pts1 = np.zeros((n, cap_p, 2), np.float32)
costs1 = np.zeros((n, cap_c), np.float32)
info1 = (ufm_amd.capi.PathInfo * n)()


def one_call():
    assert L.ufm_extract_paths_from(hd, n, starts.ctypes.data, max_steps, 1, 1, pts.ctypes.data, cap_p, costs.ctypes.data, cap_c, C.addressof(info)) == 0


def totals_only():
    assert L.ufm_extract_paths_from(hd, n, starts.ctypes.data, max_steps, 1, 1, None, 0, None, 0, C.addressof(info)) == 0


def loop():
    sz = C.sizeof(ufm_amd.capi.PathInfo)
    for k in range(n):
        assert L.ufm_set_start(hd, float(starts[k, 0]), float(starts[k, 1])) == 0
        assert L.ufm_extract_path(hd, max_steps, 1, 1, pts1[k].ctypes.data, cap_p, costs1[k].ctypes.data, cap_c, C.addressof(info1) + k * sz) == 0


forms = (("one call, all way points", one_call), ("one call, totals only", totals_only), ("set_start + extract_path loop", loop))
times = {name: [] for name, _ in forms}
for r in range(rounds + 1):
    for name, fn in forms:
        t0 = time.perf_counter()
        fn()
        if r:
            times[name].append((time.perf_counter() - t0) * 1e3)
one_call()
same = all((info[k].n_points, info[k].n_costs, info[k].steps, info[k].total_cost, info[k].total_dist) ==
           (info1[k].n_points, info1[k].n_costs, info1[k].steps, info1[k].total_cost, info1[k].total_dist) and
           np.array_equal(pts[k, :info[k].n_points], pts1[k, :info1[k].n_points]) and
           np.array_equal(costs[k, :info[k].n_costs], costs1[k, :info1[k].n_costs]) for k in range(n))
found = sum(1 for k in range(n) if info[k].n_points > 1)
moves = sum(info[k].steps for k in range(n))
say("%s: FD-1 %dx%d seed %d, focused 0, %d starts, max_steps %d; %d starts have a path, %d moves in all" % (
    L.ufm_version().decode(), size, size, seed, n, max_steps, found, moves))
med = {}
for name, _ in forms:
    med[name] = float(np.median(times[name]))
    say("%-32s median %9.3f ms  (%s)" % (name, med[name], " ".join("%.3f" % t for t in times[name])))
say("per path: %.2f us in one call, %.2f us in the loop; loop / one call = %.1f, loop / totals only = %.1f" % (
    1e3 * med[forms[0][0]] / n, 1e3 * med[forms[2][0]] / n, med[forms[2][0]] / med[forms[0][0]], med[forms[2][0]] / med[forms[1][0]]))
say("one call and the loop returned the same bits: %s" % same)
p.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
