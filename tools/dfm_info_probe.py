"""MS-DFM level 1, replans with the invalidation along the stored back-pointer bytes ("dfm_follow_info" 1) against the default one (0).

BASELINE config 4, one GPU's share: a batch of 8 x 2048^2 maps (seeds 1000..1007), a plan, then 100 replan rounds of the synth scripts
(every map its own patch per round), once per mode with the same scripts.  Per mode: the 100 rounds' wall time (a run without event
timing), region_kernel_ms of the sampled block-kernel launches (a second run with profiling on), region_replans_done / region_replans,
raise_tile_visits of the rounds that fell back to the launch chain, and the largest relative deviation of the final fields from the
other mode's.

    python tools/dfm_info_probe.py [--rounds 100] [--size 2048] [--maps 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ufm_amd  # noqa: E402


def run(follow, costs, scripts, start, goal, rounds, profile):
    n = len(costs)
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_DFM, 1)
    b.set_param("dfm_follow_info", follow)
    b.set_occupancy_threshold(1)
    b.set_param("defer_patches", 1)       # (as bench.py's batch runs)
    b.set_profiling(profile)
    for i in range(n):
        b.set_map(i, costs[i]); b.set_start(i, *start); b.set_goal(i, *goal)
    assert b.step() == 0
    reg0, done0 = b.stats.region_replans, b.stats.region_replans_done
    wall, kms, fell_back, raise_visits = 0.0, [], 0, 0
    prev = (reg0, done0)
    for r in range(rounds):
        for i in range(n):
            _k, s, top, left, patch = scripts[i][r]
            b.patch_map(i, patch, top, left); b.set_start(i, *s)
        t0 = time.perf_counter()
        assert b.step() == 0
        wall += time.perf_counter() - t0
        st = b.stats
        if profile and st.region_timed:
            kms.append(float(st.region_kernel_ms))
        # (region_replans / _done are cumulative: a round the block kernel did not finish for every map went on in the launch chain)
        if st.region_replans - prev[0] != st.region_replans_done - prev[1] or st.raise_tile_visits:
            fell_back += 1
            raise_visits += int(st.raise_tile_visits)
        prev = (st.region_replans, st.region_replans_done)
    out = {"follow_info": follow, "rounds": rounds, "wall_ms": wall * 1e3,
           "region_replans": int(b.stats.region_replans - reg0), "region_replans_done": int(b.stats.region_replans_done - done0),
           "rounds_with_launch_chain": fell_back, "raise_tile_visits_launch_chain": raise_visits}
    if profile:
        out.update({"region_kernel_ms_mean": float(np.mean(kms)) if kms else None, "region_kernel_ms_median": float(np.median(kms)) if kms else None,
                    "region_timed": len(kms)})
    fields = [b.read_field(i) for i in range(n)]
    check = b.check_info()
    out["check_info"] = list(check)
    b.close()
    return out, fields


def start_key(f, s):
    """the start's key of a field (no heuristic): the largest finite value of the cells around the start"""
    x0, y0 = int(np.floor(s[0])), int(np.floor(s[1]))
    v = f[max(x0 - 1, 0):x0 + 2, max(y0 - 1, 0):y0 + 2]
    v = v[np.isfinite(v)]
    return float(v.max()) if v.size else np.inf


def deviation(fa, fb, s):
    """largest relative deviation over the cells below the start's key in both fields (what a focused search has finalised), over all
    cells finite in both, and how many cells are finite in one field only"""
    worst_key, worst_all, only = 0.0, 0.0, 0
    for a, c in zip(fa, fb):
        both = np.isfinite(a) & np.isfinite(c)
        only += int((np.isfinite(a) != np.isfinite(c)).sum())
        if both.any():
            d = np.abs(a.astype(np.float64) - c) / np.maximum(c.astype(np.float64), 1e-30)
            worst_all = max(worst_all, float(d[both].max()))
            key = min(start_key(a, s), start_key(c, s))
            below = both & (a < key) & (c < key)
            if below.any():
                worst_key = max(worst_key, float(d[below].max()))
    return worst_key, worst_all, only


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--maps", type=int, default=8)
    args = ap.parse_args()
    size, n = args.size, args.maps
    start, goal = ufm_amd.synth.start_goal(size, size)
    costs = [ufm_amd.synth.cost_map(1000 + i, size, size) for i in range(n)]
    scripts = [list(ufm_amd.synth.replan_script(1000 + i, size, size, n_patches=args.rounds)) for i in range(n)]
    res, fields = {}, {}
    for follow in (0, 1):
        timed, fields[follow] = run(follow, costs, scripts, start, goal, args.rounds, profile=False)
        prof, _ = run(follow, costs, scripts, start, goal, args.rounds, profile=True)
        timed.update({k: v for k, v in prof.items() if k.startswith("region_kernel") or k == "region_timed"})
        res[follow] = timed
    last_start = scripts[0][args.rounds - 1][1]
    for follow in (0, 1):
        worst_key, worst_all, only = deviation(fields[follow], fields[1 - follow], last_start)
        res[follow]["max_rel_dev_vs_other_mode_below_start_key"] = worst_key
        res[follow]["max_rel_dev_vs_other_mode_all_finite"] = worst_all
        res[follow]["finite_in_one_mode_only"] = only
        print(json.dumps(res[follow]))


if __name__ == "__main__":
    main()
