"""Cost layers in the engine (ufm_set_layers / ufm_set_layer / ufm_reveal with n > 1) on one GPU: what the layer kernels cost.  A
measurement tool, not part of the product.  FD-1 on a 4096^2 map, profiling on.
(a) the reveal: a disc of radius 15 as the field of view, 100 moves along the diagonal, n = 1, 2, 4 layers, every layer with a survey.
    Per move the device time of everything the reveal call queues -- the counter's memset, k_reveal (n = 1: the parent commit's kernel,
    unchanged) or k_reveal_layers (n > 1), the patch kernel behind it -- between two events on the engine's stream, and for n > 1
    k_reveal_layers' own duration from the events on its dispatch.
(b) the whole-raster compose: ufm_set_layer_device of a 4096^2 raster, n = 2 and 4 -- k_layer_compose_all's own duration from the events
    on its dispatch, against a device-to-device hipMemcpyAsync of (n + 1) * L * W bytes on the same machine (n rasters read, one written).
usage: layers_probe.py [--size N] [--moves K] [--repeats R] [--out FILE]   (default FILE: profiles/layers_probe.txt)"""
import argparse
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ufm_amd

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--moves", type=int, default=100)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--radius", type=int, default=15)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_probe.txt"))
args = ap.parse_args()
size, seed, n_moves, radius = args.size, 7, args.moves, args.radius
lines = []


class DeviceBytes:
    """a raster in HBM (a torch tensor), as the *_device entry points take it: .ptr"""

    def __init__(self, arr):
        self.t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr()

    def free(self):
        self.t = None


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(a, unit="us"):
    a = np.asarray(a, np.float64)
    return "median %.1f %s (min %.1f, max %.1f, %d samples)" % (np.median(a), unit, a.min(), a.max(), len(a))


lib = ufm_amd.load_library()
lib.ufm_debug_layers_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
disc = ufm_amd.sensor_disc(radius)
start, goal = ufm_amd.synth.start_goal(size, size)
moves = [s for k, s, top, left, patch in ufm_amd.synth.replan_script(seed, size, size, n_patches=n_moves, size=11)]
centres = [(int(round(s[0])), int(round(s[1]))) for s in moves]
raw0 = ufm_amd.synth.cost_map(seed, size, size)
surveys = [ufm_amd.synth.cost_map(seed + 5 + 10 * k, size, size, obstacles=False) for k in range(4)]
say("layers_probe: %d^2, seed %d, radius %d (%d of %d cells seen), %d moves, %s" % (
    size, seed, radius, int(disc.sum()), disc.size, n_moves, lib.ufm_version().decode()))


def planner(n):
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    p.reset(); p.set_occupancy_threshold(1)
    if n > 1:
        p.set_layers(n)
    p.set_profiling(True)
    p.set_map(raw0); p.set_start(*start); p.set_goal(*goal)
    return p


# ---- (a) the reveal ----
say("(a) reveal, disc of radius %d, per move: device time of what the call queues (events on the engine's stream around it)" % radius)
ms = C.c_float(0)
for n in (1, 2, 4):
    p = planner(n)
    p.set_sensor(disc)
    for k in range(n):
        p.set_layer_survey(k, surveys[k])
    assert p.step() == 0
    st = torch.cuda.ExternalStream(p.stream_ptr())
    call, kern, changed = [], [], 0
    for i, s in enumerate(moves):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        p.reveal(*centres[i])
        e1.record(st)
        e1.synchronize()
        if i:                                    # (the first move warms up: buffers grow, code is loaded)
            call.append(e0.elapsed_time(e1) * 1e3)
            if n > 1:
                assert lib.ufm_debug_layers_ms(p.h, C.byref(ms)) == 0
                kern.append(ms.value * 1e3)
        p.set_start(*s)
        assert p.step() == 0
    say("    n = %d: the whole call on the stream, %s: %s" % (n, "memset + k_reveal + patch kernel" if n == 1 else "memset + k_reveal_layers + patch kernel", spread(call)))
    if n > 1:
        say("           k_reveal_layers alone, events on the dispatch: %s" % spread(kern))
    p.close()

# ---- (b) the whole-raster compose ----
say("(b) ufm_set_layer_device of a %d^2 raster: k_layer_compose_all, events on the dispatch, against hipMemcpyAsync device-to-device" % size)
hip = C.CDLL("libamdhip64.so")
cells = size * size
for n in (2, 4):
    p = planner(n)
    devs = [DeviceBytes(surveys[k]) for k in range(n)]
    for k in range(1, n):
        p.set_layer(k, devs[k], width=size, length=size)
    kern = []
    for r in range(args.repeats + 1):
        k = 1 + r % (n - 1)
        p.set_layer(k, devs[(k + r) % n], width=size, length=size)
        assert lib.ufm_debug_layers_ms(p.h, C.byref(ms)) == 0
        if r:
            kern.append(ms.value * 1e3)
    want = np.maximum.reduce([p.read_layer(k, size, size) for k in range(n)])
    assert np.array_equal(p.read_map(size, size), want), "the map is not the maximum of the layers"
    p.close()
    for d in devs:
        d.free()
    nbytes = (n + 1) * cells
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    copy = []
    for r in range(args.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        e1.record()
        e1.synchronize()
        if r:
            copy.append(e0.elapsed_time(e1) * 1e3)
    kern, copy = np.asarray(kern), np.asarray(copy)
    say("    n = %d: k_layer_compose_all, %d bytes read + %d written: %s = %.0f GB/s" % (n, n * cells, cells, spread(kern), nbytes / (np.median(kern) * 1e-6) / 1e9))
    say("           hipMemcpyAsync device-to-device of %d bytes (that many moved: read once, written once): %s = %.0f GB/s moved" % (
        nbytes, spread(copy), 2 * nbytes / (np.median(copy) * 1e-6) / 1e9))
    say("           kernel / copy: %.2f (medians)" % (np.median(kern) / np.median(copy)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
