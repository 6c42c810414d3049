"""Trajectory scoring at the size of a sampling controller's cycle (not part of the product): Field D* level 0 handle with a footprint
(cspace_disc(5)) on a 4096^2 map (seed 7), 65 536 rollouts of 32 points each, steps of about one cell with a slowly turning heading,
starts hashed over the map.  Per call, HIP events on the engine's stream (torch.cuda.Event on an ExternalStream) and the host clock
around calls that end in a synchronise, of
  (a) ufm_score_paths_device: offsets, points and records are torch tensors on the GPU -- events around the queued kernel,
  (b) ufm_score_paths: the same rollouts from host memory -- staging, two copies up, the kernel, one copy down, a synchronise,
  (c) one ufm_read_map of the same map: what a caller pays to pull the planning raster back before it can score anything itself,
each 20 times after 3 warm-up rounds, alternating; medians and extremes, and that (a) and (b) returned the same bytes.  One wavefront
per path is the shape measured; nothing else was tried.
usage: score_probe.py [out.txt] [size] [n_paths] [n_points]   (default out: profiles/score_probe.txt)"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ufm_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_probe.txt")
size = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
npts = int(sys.argv[4]) if len(sys.argv) > 4 else 32
seed, warm, rounds = 7, 3, 20
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


cost = ufm_amd.synth.cost_map(seed, size, size)
rng = np.random.default_rng(seed)
heading = rng.uniform(0.0, 2.0 * np.pi, (n, 1)) + np.cumsum(rng.normal(0.0, 0.15, (n, npts)), axis=1)
steps = np.stack([np.cos(heading), np.sin(heading)], axis=2)
steps[:, 0, :] = 0.0
pts = np.clip(rng.uniform(40.0, size - 40.0, (n, 1, 2)) + np.cumsum(steps, axis=1), 0.0, float(size)).astype(np.float32).reshape(-1, 2)
off = (npts * np.arange(n + 1)).astype(np.int32)

p = ufm_amd.Planner(ufm_amd.ALGO_FD, 0)
p.reset()
p.set_occupancy_threshold(1.0)
p.set_cspace(ufm_amd.cspace_disc(5))
p.set_map(cost)
dev = torch.device("cuda", 0)
stream = torch.cuda.ExternalStream(p.stream_ptr(), device=dev)
d_pts, d_off = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
d_out = torch.zeros((n, 6), dtype=torch.int32, device=dev)
host_out = np.zeros(n, ufm_amd.capi.SCORE_DTYPE)
raster = np.empty((size, size), np.uint8)
torch.cuda.synchronize()
L, hd = p.L, p.h


def device_form():
    assert L.ufm_score_paths_device(hd, n, len(pts), d_off.data_ptr(), d_pts.data_ptr(), d_out.data_ptr()) == 0


def host_form():
    assert L.ufm_score_paths(hd, n, off.ctypes.data, pts.ctypes.data, host_out.ctypes.data) == 0


def read_map():
    assert L.ufm_read_map(hd, raster.ctypes.data) == 0


forms = (("score_paths_device", device_form), ("score_paths (host)", host_form), ("read_map", read_map))
ev_ms = {name: [] for name, _ in forms}
wall_ms = {name: [] for name, _ in forms}
for r in range(warm + rounds):
    for name, fn in forms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        if r >= warm:
            ev_ms[name].append(e0.elapsed_time(e1))
            wall_ms[name].append((t1 - t0) * 1e3)
torch.cuda.synchronize()
got = d_out.cpu().numpy().view(ufm_amd.capi.SCORE_DTYPE).reshape(-1)
same = np.array_equal(got.view(np.uint8), host_out.view(np.uint8))
free = int((host_out["blocked_segment"] < 0).sum())
say("%s: %dx%d seed %d, footprint disc(5), %d rollouts x %d points (%.1f MB of points); %d free, %d blocked, %d pieces charged in all" % (
    L.ufm_version().decode(), size, size, seed, n, npts, pts.nbytes / 1e6, free, n - free, int(host_out["pieces"].astype(np.int64).sum())))
say("%d rounds after %d warm-up rounds, the three forms alternating; ms per call: median (min .. max)" % (rounds, warm))
for name, _ in forms:
    e, w = np.array(ev_ms[name]), np.array(wall_ms[name])
    say("%-22s events %9.3f (%.3f .. %.3f)   host clock %9.3f (%.3f .. %.3f)" % (name, np.median(e), e.min(), e.max(), np.median(w), w.min(), w.max()))
say("per rollout, device form: %.2f ns" % (1e6 * float(np.median(ev_ms["score_paths_device"])) / n))
say("device form and host form returned the same bytes: %s" % same)
p.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
