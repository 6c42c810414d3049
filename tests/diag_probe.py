"""Helper of tests/test_gpu_diag_builds.py (run as a process of its own: a process binds one build of the library): an FD-1 plan and three
replans of a 256 x 256 map on the library given as argv[1] -- the product or one of the diagnostic builds (csrc/ufm_diag.h) -- in the resident
form (case A: early hand-off and in-visit refresh run) and in the launch chain with the cursor hand-out (case B: owned = 0, grid = 8, so that a
front of three tiles is long enough for k_triage and k_relax<DYN>).  Full-field mode: every element is final, the field is one deterministic array.
Prints, per case, `field` (the SHA-1 of the field after the plan and after the replans) and, on a diagnostic build, what its records say about the
plan step next to the engine's own statistics: `eq what a b`, `le what a b`, `gt0 what a` -- the test asserts them, this file only measures."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import ufm_amd  # noqa: E402

ufm_amd.use_library(sys.argv[1])
L = ufm_amd.load_library()
print("version", L.ufm_version().decode())
timing, sstat = hasattr(L, "ufm_debug_tdiag"), hasattr(L, "ufm_debug_sstat")
for name in ("tdiag", "sdiag", "sstat", "tiles", "visits", "plog", "trace"):
    if hasattr(L, "ufm_debug_" + name):
        getattr(L, "ufm_debug_" + name).argtypes = [C.c_void_p, C.c_int]
if timing:
    L.ufm_debug_wtrace.argtypes = [C.c_void_p, C.c_void_p]

size, seed = 256, 5
T = L.ufm_tile_edge()
NT = ((size + 1 + T - 1) // T) ** 2           # 17 x 17 tiles of nodes
cost = ufm_amd.synth.cost_map(seed, size, size)
start, goal = ufm_amd.synth.start_goal(size, size)
script = list(ufm_amd.synth.replan_script(seed, size, size, n_patches=3))


def sha(p):
    return hashlib.sha1(np.ascontiguousarray(p.g()).tobytes()).hexdigest()


for case, params in (("A", {"owned_waves": 16}), ("B", {"owned": 0, "grid": 8})):
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    p.set_param("focused", 0)
    for k, v in params.items():
        p.set_param(k, v)
    p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*goal)
    if timing:
        assert L.ufm_debug_tdiag(None, 1) == 0 and L.ufm_debug_sdiag(None, 1) == 0
    if sstat:
        assert L.ufm_debug_sstat(None, 1) == 0
    assert p.step() == 0
    st = p.stats
    print("eq %s resident_launches %d %d" % (case, st.resident_launches, 1 if case == "A" else 0))
    if timing:
        td = (C.c_ulonglong * 64)(); assert L.ufm_debug_tdiag(td, 0) == 0
        print("eq %s tdiag[3]:visits_timed=tile_visits %d %d" % (case, td[3], st.tile_visits))
        if case == "A":
            tiles = np.zeros((5, NT), np.uint32); assert L.ufm_debug_tiles(tiles.ctypes.data, NT) == NT
            print("eq A sum(tiles[3]):visits=resident_tile_visits %d %d" % (int(tiles[3].astype(np.int64).sum()), st.resident_tile_visits))
            sd = (C.c_ulonglong * 16)(); assert L.ufm_debug_sdiag(sd, 0) == 0
            print("gt0 A sdiag[0]:looks %d" % sd[0])
            vis = np.zeros((1 << 16, 5), np.uint32)
            print("gt0 A visits_recorded %d" % L.ufm_debug_visits(vis.ctypes.data, 1 << 16))
        plog = np.zeros((1 << 14, 4), np.uint32); trace = np.zeros(4 * 16384, np.uint64)
        wt = np.zeros(16 * 256 * 2, np.uint64); nw = np.zeros(16, np.uint32)
        n_plog, n_trace = L.ufm_debug_plog(plog.ctypes.data, 1 << 14), L.ufm_debug_trace(trace.ctypes.data, 16384)
        rc = L.ufm_debug_wtrace(wt.ctypes.data, nw.ctypes.data)
        print("readers %s plog %d trace %d wtrace %d" % (case, n_plog, n_trace, rc))
    if sstat:
        ss = (C.c_ulonglong * 32)(); assert L.ufm_debug_sstat(ss, 0) == 0
        print("eq %s 16*sstat[0]:sweeps=elem_evals %d %d" % (case, 16 * ss[0], st.elem_evals))
        print("le %s sstat[1]:quiet_sweeps<=sstat[0]:sweeps %d %d" % (case, ss[1], ss[0]))
        print("le %s sstat[3]:bursts<=sstat[0]:sweeps %d %d" % (case, ss[3], ss[0]))
    h = sha(p)
    for k, s, top, left, patch in script:
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
    h2 = sha(p)
    lay, info = p.check_layout(), p.check_info()[1:4]
    print("checks %s layout %s info %s" % (case, tuple(int(x) for x in lay), tuple(int(x) for x in info)))
    print("field %s plan %s replans %s" % (case, h, h2))
    p.close()
