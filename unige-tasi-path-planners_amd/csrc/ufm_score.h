// ufm_score.h -- trajectory scoring on the device (a piece of ufm_engine.hip, behind ufm_path.h; gfx950 only): what the caller's
// polylines cost on the planning raster, and whether they are blocked (ufm_score_paths, include/ufm_score.h).
//
// One wavefront per path, one path per workgroup, as k_extract_path has one per walk: the paths share nothing.  The lanes stride over
// the path's segments, 64 at a time; each lane walks its segment through score_segment() (ufm_score_rect.h: the arithmetic, in fp64,
// the same text the CPU driver runs) and reads the raster through PathField / raster_cost() -- one dependent byte load per piece, from
// L2 / MALL for any map that has been planned on.  The segments' results are then added in SEGMENT-INDEX order: every lane fetches the
// result of lane 0, 1, 2 ... of the block of 64 in turn (wave-uniform source lane: v_readlane_b32, two per double) and runs score_add_segment() on
// it, so all lanes hold the same sums and the order depends on nothing but the path -- no atomics, no tree whose shape could depend on
// the launch.  Blocks of 64 follow each other in index order too.  Behind a blocked segment only the lengths are still computed.
// The kernel only reads: the raster, the offsets, the points; it writes the records.
#pragma once
#include "ufm_score_rect.h"

// lane j's value of v in every lane, j wave-uniform: a v_readlane_b32 per half (no trip through the LDS crossbar, as __shfl would make)
__device__ __forceinline__ double lane_f64(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// Path i of the launch: points offsets[i] .. offsets[i + 1] - 1 of pts ([total_points][2]) on map maps[i] (maps == nullptr: on `map`).
// The offsets are the caller's and may be anything: both are clamped to [0, total_points] and a decreasing pair is an empty path, so no
// read leaves pts.  (maps, where given, comes from the host, which has checked it.)
__global__ __launch_bounds__(64) void k_score_paths(PathField F0, size_t cstride, const int32_t *offsets, const int32_t *maps, int map,
                                                    const float *pts, int total_points, ufm_score *out) {
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    PathField F = F0;
    F.cost += (size_t)(maps ? maps[i] : map) * cstride;
    const int p0 = min(max(offsets[i], 0), total_points), p1 = min(max(offsets[i + 1], 0), total_points);
    const int nseg = p1 - p0 > 1 ? p1 - p0 - 1 : 0;
    const float *p = pts + 2 * (size_t)p0;
    auto cost = [&](int cx, int cy) { return raster_cost(F, cx, cy); };
    PathScore acc;
    for (int base = 0; base < nseg; base = nseg - base > 64 ? base + 64 : nseg) {      // (never beyond nseg: no overflow however long the path)
        SegScore r{0.0, 0.0, 0.0, 0, 0};
        if (lane < nseg - base) {
            const size_t s = (size_t)base + lane;
            const float ax = p[2 * s], ay = p[2 * s + 1], bx = p[2 * s + 2], by = p[2 * s + 3];
            if (acc.blocked_segment >= 0) r.dist = score_segment_dist(ax, ay, bx, by);
            else r = score_segment(ax, ay, bx, by, F.L, F.W, cost);
        }
        const int cnt = min(64, nseg - base);      // wave-uniform: every lane takes part in every fetch
        for (int j = 0; j < cnt; ++j) {
            SegScore q;
            q.cost = lane_f64(r.cost, j); q.dist = lane_f64(r.dist, j); q.t = lane_f64(r.t, j);
            q.pieces = __builtin_amdgcn_readlane(r.pieces, j); q.blocked = __builtin_amdgcn_readlane(r.blocked, j);
            score_add_segment(acc, base + j, q);
        }
    }
    if (lane == 0) {      // fp64 -> fp32 once
        ufm_score o;
        score_narrow(acc, o);
        out[i] = o;
    }
}
