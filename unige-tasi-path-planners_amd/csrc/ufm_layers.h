// ufm_layers.h -- cost layers on the device (ufm_set_layers / ufm_patch_layer / ufm_set_layer / ufm_reveal with n > 1): a map's raster is
// the element-wise maximum of n rasters that lie in HBM next to it (the reference's simulator keeps two, slope and rocks, and plans on
// dilate(np.maximum(data_l, rock_aboundance_l)), Tests/run_test.py:102,136-140).  Every kernel here makes a DENSE composed patch that the
// host hands to Engine::patch_raw() / patch() as the caller's device patch would be handed; none of them touches the planning raster.
// ufm_layers_rect.h has the validation and the index arithmetic; DESIGN.md section 4.14.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

#include "ufm_layers_rect.h"

// the rectangle of a patch to layer k of one map
struct LayerComposeJob {
    uint8_t *layer[LAYERS_MAX];     // this map's rasters, layer[0 .. n-1]
    const uint8_t *patch;           // [h][w], dense
    uint8_t *out;                   // [h][w], dense: the maximum over the layers after the store
    int n, k, W, x, y, w, h;
};
// Lane e stores the patch byte into layer k and writes the maximum over the n layers.  One cell per lane, consecutive lanes along a row:
// byte accesses, 64 adjacent ones per wave instruction wherever a row of the rectangle is that long.  A lane reads and writes only its
// own cell of every store.
__global__ __launch_bounds__(LAYERS_THREADS) void k_layer_compose(LayerComposeJob J) {
    const int e = layers_lane_elem((int)blockIdx.x, (int)threadIdx.x);
    if (e >= J.w * J.h) return;
    const size_t at = layers_rect_cell(e, J.x, J.y, J.w, J.W);
    const uint8_t b = J.patch[e];
    uint32_t mx = b;
    uint8_t *dst = J.layer[0];                    // (selected, not indexed: the pointers stay in registers)
#pragma unroll
    for (int l = 0; l < LAYERS_MAX; ++l) {
        if (l == J.k) dst = J.layer[l];
        else if (l < J.n) mx = max(mx, (uint32_t)J.layer[l][at]);
    }
    dst[at] = b;
    J.out[e] = (uint8_t)mx;
}

// the whole raster of one map: out = max over the n layers as they stand (the host has copied the new raster into its layer before)
struct LayerComposeAllJob {
    const uint8_t *layer[LAYERS_MAX];
    uint8_t *out;                   // [L][W]; the same address modulo 16 as every layer
    size_t cells;
    int n;
};
__device__ __forceinline__ uint4 layers_max16(uint4 a, uint4 b) {
    return make_uint4(layers_max4(a.x, b.x), layers_max4(a.y, b.y), layers_max4(a.z, b.z), layers_max4(a.w, b.w));
}
// 16 bytes per lane from the first aligned address on, consecutive lanes consecutive vectors; the up to 15 bytes in front and behind by
// the first wave of workgroup 0.  n reads and one write per byte, nothing else: the kernel runs at the speed of the memory.
__global__ __launch_bounds__(LAYERS_THREADS) void k_layer_compose_all(LayerComposeAllJob J) {
    const LayersSplit s = layers_split(reinterpret_cast<uintptr_t>(J.out), J.cells);
    const size_t G = (size_t)gridDim.x * LAYERS_THREADS, g = (size_t)blockIdx.x * LAYERS_THREADS + threadIdx.x;
    const size_t iters = layers_iters(s, G);
    for (size_t it = 0; it < iters; ++it) {
        const size_t v = layers_lane_vec(it, g, G);
        if (v >= s.nvec) break;
        const size_t off = layers_vec_offset(s, v);
        uint4 q = *reinterpret_cast<const uint4 *>(J.layer[0] + off);
#pragma unroll
        for (int l = 1; l < LAYERS_MAX; ++l)
            if (l < J.n) q = layers_max16(q, *reinterpret_cast<const uint4 *>(J.layer[l] + off));
        *reinterpret_cast<uint4 *>(J.out + off) = q;
    }
    if (blockIdx.x == 0 && threadIdx.x < s.head + s.tail) {
        const size_t off = layers_edge_offset(s, threadIdx.x);
        uint32_t mx = J.layer[0][off];
#pragma unroll
        for (int l = 1; l < LAYERS_MAX; ++l)
            if (l < J.n) mx = max(mx, (uint32_t)J.layer[l][off]);
        J.out[off] = (uint8_t)mx;
    }
}

// One launch for all layers of all maps of an engine: blockIdx.y is the map, blockIdx.x a run of 256 elements of that map's Q.
struct RevealLayersJob {
    const uint8_t *mask;                 // [mh][mw], device bytes
    uint8_t *layers;                     // the store: layer k of map m at layers_slot(k, m, nmaps, lstride)
    const uint8_t *survey[LAYERS_MAX];   // layer k's surveys, [nmaps][L][W] at cstride, or null
    const uint8_t *cur;                  // the composed raster as it stands: the raw store with a footprint, the planning raster without
    uint8_t *slots;                      // the engine's patch buffer: map m's dense Q at m * slot_stride
    unsigned int *count;                 // [nmaps]: cells of R whose composed byte changes (the host has cleared it)
    const int32_t *centres;              // [nmaps][3] = (row, col, which layers of this map have a survey: bit k), host-coherent pinned
    size_t cstride, lstride, slot_stride;
    int n, nmaps, L, W, mh, mw, ar, ac;
};
// k_reveal with the layer loop: per lane one mask byte; for every layer with a survey the layer byte and the survey byte, the new layer
// byte stored where the mask covers the cell; the maximum folded over all layers is Q's byte, counted against the composed raster.  A
// lane reads and writes only its own cell of every store.  Every lane of a wave that has work reaches the ballot.
__global__ __launch_bounds__(SENSOR_THREADS) void k_reveal_layers(RevealLayersJob J) {
    const int m = blockIdx.y;
    const int row = J.centres[3 * m], col = J.centres[3 * m + 1];
    if (row < 0) return;                                                  // (uniform: the whole workgroup)
    const int have = J.centres[3 * m + 2];
    const SensorRect r = sensor_place(row, col, J.mh, J.mw, J.ar, J.ac, J.L, J.W);
    const int n = r.w * r.h;
    if (sensor_lane_elem((int)blockIdx.x, 0) >= n) return;                // (uniform: a workgroup beyond the clipped R)
    const int e = sensor_lane_elem((int)blockIdx.x, (int)threadIdx.x);
    bool ch = false;
    if (e < n) {
        const SensorCell c = sensor_cell(r, e, J.W, J.mw);
        const bool seen = J.mask[c.mask] != 0;
        uint32_t q = 0;
#pragma unroll
        for (int l = 0; l < LAYERS_MAX; ++l) {
            if (l >= J.n) continue;
            uint8_t *lay = J.layers + layers_slot(l, m, J.nmaps, J.lstride) + c.cell;
            uint32_t v = *lay;
            if (seen && ((have >> l) & 1)) {
                const uint32_t sv = J.survey[l][(size_t)m * J.cstride + c.cell];
                if (sv != v) *lay = (uint8_t)sv;
                v = sv;
            }
            q = max(q, v);
        }
        J.slots[(size_t)m * J.slot_stride + e] = (uint8_t)q;
        ch = q != J.cur[(size_t)m * J.cstride + c.cell];
    }
    const unsigned long long b = __ballot(ch);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&J.count[m], (unsigned int)__popcll(b));
}
