"""The checks of the device form of trajectory scoring (ufm_score_paths_device / ufm_batch_score_paths_device), over a `runner` that
says where the three buffers live: helpers.DeviceBytes in the test process (tests/test_gpu_score.py), torch tensors when this file is
run as a program -- `python tests/score_device_checks.py`, a process of its own that imports torch before anything opens the GPU.

run_checks(): the device form returns the bytes of the host form for the directed, the hostile and 100 random paths; offsets beyond
the points, negative and decreasing give the records the kernel's clamp defines; the batch form scores all its paths on the one map
it names."""
import ctypes as C
import sys

import numpy as np

SENTINEL = -12345


def device_bytes_runner(form, n_paths, offsets, pts):
    """buffers from hipMalloc, filled by synchronous copies; the device is waited for before the records are copied back"""
    from helpers import DeviceBytes
    import ufm_amd
    d_pts, d_off = DeviceBytes(pts), DeviceBytes(np.ascontiguousarray(offsets, np.int32))
    d_out = DeviceBytes(np.full((n_paths, 6), SENTINEL, np.int32))
    form(n_paths, len(pts), d_off.data_ptr(), d_pts.data_ptr(), d_out.data_ptr())
    out = np.zeros(n_paths, ufm_amd.capi.SCORE_DTYPE)
    hip = DeviceBytes._hip
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), d_out.ptr, C.c_size_t(out.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    for b in (d_pts, d_off, d_out):
        b.free()
    return out


def torch_runner(form, n_paths, offsets, pts):
    """torch tensors on the GPU; torch's work is waited for before the call (the engine's stream is not torch's), the device after it"""
    import torch
    import ufm_amd
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(pts).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(dev)
    d_out = torch.full((n_paths, 6), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    form(n_paths, len(pts), d_off.data_ptr(), d_pts.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(ufm_amd.capi.SCORE_DTYPE).reshape(-1)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_checks(runner):
    import path_cases as pc
    import score_cases as sc
    import score_reference as sr
    import ufm_amd
    name, cost, thr, tu = sc.maps()[0]
    paths = [p for _, p in sc.directed(cost, tu)] + [p for _, p in sc.hostile(cost, tu)] + sc.random_paths(cost, 100, 3)
    pts, off = sc.pack(paths)
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 0)
    p.reset()
    p.set_occupancy_threshold(thr)
    p.set_map(cost)
    host = p.score_paths((pts, off))
    got = runner(p.score_paths_device, len(paths), off, pts)
    assert same_bytes(got, host), "the device form differs from the host form"
    total = len(pts)
    bad = np.array([0, 2, total + 50, 5, -7, 3, 2 ** 31 - 1, 9], np.int32)
    got = runner(p.score_paths_device, len(bad) - 1, bad, pts)
    clamp = np.clip(bad.astype(np.int64), 0, total)
    for k in range(len(bad) - 1):
        a, c = int(clamp[k]), int(clamp[k + 1])
        want = p.score_paths([pts[a:c] if c > a else pts[:0]])
        assert same_bytes(got[k:k + 1], want), (k, int(bad[k]), int(bad[k + 1]), got[k], want)
    p.close()
    # the batch form scores all its paths on one map
    other = pc.make_map("speckle", 910, *cost.shape)[0]
    b = ufm_amd.BatchPlanner(2, ufm_amd.ALGO_FD, 0)
    b.set_occupancy_threshold(thr)
    b.set_map(0, cost)
    b.set_map(1, other)
    got = runner(lambda *a: b.score_paths_device(1, *a), len(paths), off, pts)
    assert same_bytes(got, b.score_paths(np.ones(len(paths), np.int32), (pts, off))), "map 1 of the batch"
    assert not same_bytes(got, host)
    chain = ufm_amd.tolerances.SCORE_FP64_CHAIN
    for k, path in enumerate(paths):
        ref = sr.score_path(path, other, tu)
        if not ref["doubtful"]:
            sc.check_record(got[k], ref, chain, "device form, map 1 of a batch, path %d" % k)
    b.close()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "torch sees no GPU"
    torch.zeros(1, device="cuda")          # (torch's runtime is the process's)
    run_checks(torch_runner)
    print("device form checks passed (torch tensors)")
    sys.exit(0)
