"""Step deltas on the headline workload (FD-1, 4096^2, seed 7, plan + 100 replans) with tracking on: per step the delta's size, the
scan kernel's time (HIP events inside the engine, profiling on), the wall time of read_changes, and beside it the wall time of the
other way to the same information -- ufm_read_field of the whole field plus ufm_read_info.  The scan moves 8 B per element (value +
baseline) + 2 B with the byte planes; HBM figure as DESIGN.md section 7: 8 TB/s.  For scale the same probe times k_gather_field, the
repository's own streaming kernel (4 B read + 4 B written per element), with events around ufm_read_field's launch on the engine's stream.
usage: delta_probe.py [size] [algo] [replans]   -> profiles/delta_scan.txt (size 4096, FD) or stdout only"""
import ctypes as C
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import ufm_amd

size = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
algo = sys.argv[2] if len(sys.argv) > 2 else "FD"
n_rep = int(sys.argv[3]) if len(sys.argv) > 3 else 100
A = {"FD": ufm_amd.ALGO_FD, "SG": ufm_amd.ALGO_SG, "DFM": ufm_amd.ALGO_DFM}[algo]
HBM = 8e12
seed = 7
cost = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=n_rep))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scan_ms(p):
    v = C.c_float(0)
    p.L.ufm_debug_delta_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    assert p.L.ufm_debug_delta_ms(p.h, C.byref(v)) == 0
    return v.value


def stats(a):
    a = np.asarray(a, np.float64)
    return "median %.3f, p10 %.3f, p90 %.3f, max %.3f" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90), a.max())


p = ufm_amd.Planner(A, 2 if algo == "SG" else 1)
p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
p.track_changes(True)
p.set_profiling(True)
ex, ey = p.dims()
tile = p.L.ufm_tile_edge()
padded = ((ex + tile - 1) // tile) * ((ey + tile - 1) // tile) * tile * tile
scan_bytes = padded * 10
floor_ms = scan_bytes / HBM * 1e3
assert p.step() == 0
t = time.perf_counter(); xy, g, info = p.read_changes(want_info=True); t_first = time.perf_counter() - t
say("%s-1 %d^2 seed %d: plan, then %d replans; field %d x %d, %d elements with padding, scan traffic %.1f MB = %.4f ms at 8 TB/s" % (
    algo, size, seed, n_rep, ex, ey, padded, scan_bytes / 1e6, floor_ms))
say("first read after the plan (baseline empty: the whole state): %d records, %.1f ms wall (counting call + delivering call, record buffer grown)" % (len(g), t_first * 1e3))
mirror = np.full((ex, ey), np.inf, np.float32); mirror[xy[:, 0], xy[:, 1]] = g
n_rec, k_ms, w_delta, w_full, w_step = [], [], [], [], []
for i, (k, s, top, left, patch) in enumerate(script):
    p.patch_map(patch, top, left); p.set_start(*s)
    t = time.perf_counter(); assert p.step() == 0; w_step.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter(); xy, g, info, total = p.read_changes(want_info=True, cap=1 << 16); w_delta.append((time.perf_counter() - t) * 1e3)
    assert total <= 1 << 16
    k_ms.append(scan_ms(p)); n_rec.append(total)
    mirror[xy[:, 0], xy[:, 1]] = g
    t = time.perf_counter(); field = p.read_field()[0]; stored = p.read_info(); w_full.append((time.perf_counter() - t) * 1e3)
    assert np.array_equal(mirror.view(np.uint32), field.view(np.uint32))
w = 10      # warm-up replans left out of the figures
say("per replan, replans %d..%d (the first %d are warm-up), ms:" % (w + 1, n_rep, w))
say("  delta size (records):            median %d, min %d, max %d" % (np.median(n_rec[w:]), min(n_rec[w:]), max(n_rec[w:])))
say("  scan kernel (HIP events):        %s" % stats(k_ms[w:]))
say("    -> %.1f %% of 8 TB/s for its %.1f MB (median)" % (100 * floor_ms / np.median(k_ms[w:]), scan_bytes / 1e6))
say("  read_changes wall (one call, cap 65536, Info included): %s" % stats(w_delta[w:]))
say("  ufm_read_field + ufm_read_info of the whole field, wall: %s" % stats(w_full[w:]))
say("    -> read_changes is %.0f x faster (medians)" % (np.median(w_full[w:]) / np.median(w_delta[w:])))
say("  the replan itself (ufm_step wall, profiling on): %s" % stats(w_step[w:]))
# the repository's own streaming kernel for scale: k_gather_field over the whole field (4 B read, 4 B written per element)
try:
    import torch
    st = torch.cuda.ExternalStream(p.stream_ptr())
    out = np.empty((ex, ey), np.float32)
    gm = []
    for r in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        assert p.L.ufm_read_field(p.h, 0, 0, ex, ey, out.ctypes.data, None) == 0      # gather kernel + D2H copy; the events bracket both
        e1.record(st); e1.synchronize()
        gm.append(e0.elapsed_time(e1))
    say("for scale: ufm_read_field's device side (k_gather_field + the copy to the host, %d MB), events on the engine's stream: %s" % (ex * ey * 4 // 1000000, stats(gm[2:])))
except Exception as e:      # the probe's own figures do not depend on it
    say("for scale: (k_gather_field not timed: %r)" % (e,))
p.close()
if size == 4096 and algo == "FD" and n_rep == 100:
    with open(os.path.join(ROOT, "profiles", "delta_scan.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
