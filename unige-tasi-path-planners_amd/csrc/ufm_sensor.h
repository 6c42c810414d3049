// ufm_sensor.h -- the sensor reveal on the device (ufm_set_sensor / ufm_set_survey / ufm_reveal): the survey raster -- what the sensor
// would see -- lies in HBM next to the map, and a move uncovers its field of view there instead of arriving as a host patch
// (the reference's round_patch_update, Simulator/simulator/run_simulator.py:9-28,177, Tests/run_test.py:143).  ufm_sensor_rect.h has the
// definition and the index arithmetic; DESIGN.md section 4.12.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

#include "ufm_sensor_rect.h"

// One launch for all maps of an engine: blockIdx.y is the map, blockIdx.x a run of 256 elements of that map's Q.
struct RevealJob {
    const uint8_t *mask;       // [mh][mw], device bytes
    const uint8_t *survey;     // [nmaps][L][W]
    const uint8_t *cur;        // the caller's raster as it stands: the raw store with a footprint, the planning raster without; [nmaps][L][W]
    uint8_t *slots;            // the engine's patch buffer: map m's dense Q at m * slot_stride
    unsigned int *count;       // [nmaps]: cells of R whose byte changes (the host has cleared it)
    const int32_t *centres;    // [nmaps][2] = (row, col), host-coherent pinned; row < 0: this map is skipped
    size_t cstride, slot_stride;
    int L, W, mh, mw, ar, ac;
};

// Q over R, and how many of its cells differ from the raster.  A lane makes one element: consecutive lanes read consecutive bytes of a
// row of the raster, the survey and the mask and write consecutive bytes of the slot (rows of R are at most 127 bytes at any alignment:
// byte accesses, 64 adjacent ones per wave instruction).  The work is R's, whatever the map's size.  The count: one ballot per wave,
// one atomic per wave that saw a change.  Every lane of a wave that has work reaches the ballot.
__global__ __launch_bounds__(SENSOR_THREADS) void k_reveal(RevealJob J) {
    const int m = blockIdx.y;
    const int row = J.centres[2 * m], col = J.centres[2 * m + 1];
    if (row < 0) return;                                                  // (uniform: the whole workgroup)
    const SensorRect r = sensor_place(row, col, J.mh, J.mw, J.ar, J.ac, J.L, J.W);
    const int n = r.w * r.h;
    if (sensor_lane_elem((int)blockIdx.x, 0) >= n) return;                // (uniform: a workgroup beyond the clipped R)
    const int e = sensor_lane_elem((int)blockIdx.x, (int)threadIdx.x);
    bool ch = false;
    if (e < n) {
        const SensorCell c = sensor_cell(r, e, J.W, J.mw);
        const size_t at = (size_t)m * J.cstride + c.cell;
        const uint8_t old = J.cur[at];
        const uint8_t q = J.mask[c.mask] ? J.survey[at] : old;
        J.slots[(size_t)m * J.slot_stride + e] = q;
        ch = q != old;
    }
    const unsigned long long b = __ballot(ch);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&J.count[m], (unsigned int)__popcll(b));
}
