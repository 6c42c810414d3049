// ufm_census.h -- the cost census on the device (ufm_track_costs): per map 256 counters, hist[v] = cells of the PLANNING raster with
// value v, built by one pass over the raster and kept exact under patches at a cost proportional to the patch; its smallest non-empty
// bin is the reference's min_cost, the heuristic multiplier ("auto_multiplier").  ufm_census_rect.h has the index arithmetic and its
// host driver; DESIGN.md section 4.11.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

#include "ufm_census_rect.h"

constexpr int CENSUS_WAVES = CENSUS_THREADS / 64;

struct CensusBuildJob { const uint8_t *cost; size_t n; uint32_t *hist; };          // one map's raster, n = L * W bytes, and its counters
struct CensusPatchJob {
    const uint8_t *cost;     // the map's raster as it stands: the old bytes
    const uint8_t *patch;    // dense [h][w], any alignment: the new bytes
    uint32_t *hist;
    int W, x, y, w, h;
};

// One byte per lane into the wave's private LDS histogram: wh[b] += amount for every lane that is `on`.  Rasters here are often almost
// constant (a binary bitmap, a flat prior), and 64 lanes adding to one LDS word serialise -- so up to ROUNDS times the first lane that is
// still on names its byte, every lane holding the same one is counted by a ballot and that lane adds the count in one atomic; whoever is
// left after that adds for itself.  EVERY lane of the wave must call.  Returns how many lanes were left to add for themselves.
// (`amount` may be (uint32_t)-1: the counters are exact modulo 2^32, and the sums they end at lie inside the range.)
template <int ROUNDS>
__device__ __forceinline__ int census_wave_add(uint32_t *wh, uint32_t b, bool on, uint32_t amount) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned long long m = __ballot(on);
        if (!m) return 0;                                   // (wave-uniform)
        const int lead = __ffsll((long long)m) - 1;
        const uint32_t bl = __shfl(b, lead);
        const unsigned long long same = __ballot(on && b == bl);
        if (lane == lead) atomicAdd(&wh[bl], amount * (uint32_t)__popcll(same));
        on = on && b != bl;
    }
    if (on) atomicAdd(&wh[b], amount);
    return __popcll(__ballot(on));
}

__device__ __forceinline__ void census_clear(uint32_t *lh) {
    for (int i = threadIdx.x; i < CENSUS_WAVES * CENSUS_BINS; i += CENSUS_THREADS) lh[i] = 0;
    __syncthreads();
}
// the workgroup's four histograms into the map's counters: one global atomic per bin that is not empty
__device__ __forceinline__ void census_flush(const uint32_t *lh, uint32_t *hist) {
    __syncthreads();
    for (int v = threadIdx.x; v < CENSUS_BINS; v += CENSUS_THREADS) {
        uint32_t s = 0;
        for (int k = 0; k < CENSUS_WAVES; ++k) s += lh[k * CENSUS_BINS + v];
        if (s) atomicAdd(&hist[v], s);
    }
}

// The histogram of one raster, added to J.hist (the host has cleared it).  16-byte loads from the first aligned address on, the up to 15
// bytes in front and behind by the first wave of workgroup 0.  A vector whose 16 bytes are one value in every lane of the wave -- the
// constant stretches -- costs one ballot and one LDS atomic for 1024 cells; otherwise byte 0 is added with two aggregation rounds, and
// whether those took most of the wave decides if the other 15 bytes are aggregated too (few distinct values) or added lane by lane
// (noise, where a ballot per distinct value would cost more than the conflicts it saves).
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_build(CensusBuildJob J) {
    __shared__ uint32_t lh[CENSUS_WAVES * CENSUS_BINS];
    census_clear(lh);
    uint32_t *wh = lh + (threadIdx.x >> 6) * CENSUS_BINS;
    const CensusSplit s = census_split(reinterpret_cast<uintptr_t>(J.cost), J.n);
    const size_t G = (size_t)gridDim.x * CENSUS_THREADS, g = (size_t)blockIdx.x * CENSUS_THREADS + threadIdx.x;
    const size_t iters = census_iters(s, G);
    for (size_t it = 0; it < iters; ++it) {
        const size_t v = census_lane_vec(it, g, G);
        const bool on = v < s.nvec;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (on) q = *reinterpret_cast<const uint4 *>(J.cost + census_vec_offset(s, v));
        const uint32_t b0 = q.x & 255u, splat = b0 * 0x01010101u;
        const bool flat = q.x == splat && q.y == splat && q.z == splat && q.w == splat;
        if (__all(flat || !on)) { census_wave_add<2>(wh, b0, on, (uint32_t)CENSUS_VEC); continue; }
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
        const bool few = census_wave_add<2>(wh, b0, on, 1u) <= 16;
        if (few) {
#pragma unroll
            for (int k = 1; k < CENSUS_VEC; ++k) census_wave_add<2>(wh, (w4[k >> 2] >> (8 * (k & 3))) & 255u, on, 1u);
        } else if (on) {
#pragma unroll
            for (int k = 1; k < CENSUS_VEC; ++k) atomicAdd(&wh[(w4[k >> 2] >> (8 * (k & 3))) & 255u], 1u);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const bool on = threadIdx.x < s.head + s.tail;
        const uint32_t b = on ? J.cost[census_edge_offset(s, threadIdx.x)] : 0u;
        census_wave_add<2>(wh, b, on, 1u);
    }
    census_flush(lh, J.hist);
}

// A patch that Engine::patch is about to apply, in front of it on the stream: for every cell whose byte changes, hist[old]-- and
// hist[new]++.  One workgroup up to 4096 cells; above that a grid of them, each aggregating in LDS like the build.  The patch is read
// byte by byte (a batch hands over pointer + offset into a receive buffer: any alignment), and so are the short rows of the rectangle.
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_patch(CensusPatchJob J) {
    __shared__ uint32_t lh[CENSUS_WAVES * CENSUS_BINS];
    census_clear(lh);
    uint32_t *wh = lh + (threadIdx.x >> 6) * CENSUS_BINS;
    const int n = J.w * J.h;
    const int iters = census_patch_iters(n, (int)gridDim.x);
    for (int it = 0; it < iters; ++it) {
        const int e = census_patch_elem(it, (int)gridDim.x, (int)blockIdx.x, (int)threadIdx.x);
        uint32_t ov = 0u, nv = 0u;
        if (e < n) { ov = J.cost[census_rect_cell(e, J.x, J.y, J.w, J.W)]; nv = J.patch[e]; }
        const bool ch = e < n && ov != nv;
        census_wave_add<2>(wh, ov, ch, 0xFFFFFFFFu);
        census_wave_add<2>(wh, nv, ch, 1u);
    }
    census_flush(lh, J.hist);
}

// The smallest and largest value present in any map of the engine -- cv2.minMaxLoc of the reference's simulator, obstacles included --
// into host-coherent pinned memory, then the sequence word the host waits for (Engine::wait_flag, like the step's counters).
// No map yet: (256, -1).
__global__ __launch_bounds__(CENSUS_BINS) void k_census_publish(const uint32_t *hist, int nmaps, int *out, unsigned int *flag, unsigned int seq) {
    __shared__ int s_min, s_max;
    if (threadIdx.x == 0) { s_min = CENSUS_BINS; s_max = -1; }
    __syncthreads();
    bool any = false;
    for (int m = 0; m < nmaps; ++m) any = any || hist[(size_t)m * CENSUS_BINS + threadIdx.x] != 0u;
    if (any) { atomicMin(&s_min, (int)threadIdx.x); atomicMax(&s_max, (int)threadIdx.x); }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = s_min; out[1] = s_max;
        __threadfence_system();
        __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
