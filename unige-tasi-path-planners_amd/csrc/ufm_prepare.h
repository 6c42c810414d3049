// ufm_prepare.h -- map preparation on the device (ufm_set_image): from the grey-scale bitmap both rasters a mission starts with, the
// blurred, penalised low-resolution costs (the map) and the complemented high-resolution costs (the survey), in one launch that reads
// the bitmap once (the reference's simulation_data, Simulator/simulator/run_simulator.py:106-113,148, Tests/run_test.py:101).
// ufm_prepare_rect.h has the definition, the index arithmetic and the passes as one lane runs them; DESIGN.md section 4.13.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

#include "ufm_prepare_rect.h"

struct PrepareJob {
    const uint8_t *src;        // the bitmap [L][W]; aliases neither output
    uint8_t *out_l;            // the map's slot of the raw store (a footprint is set) or of the planning raster
    uint8_t *out_h;            // the map's slot of the survey
    int W, L, penalty;
    int wide_in, wide_out;     // W a multiple of 4 and the pointers 4-byte aligned: 32-bit loads / stores
    PrepTaps taps;             // 31 x uint16_t and their number, in the kernel argument
};

// One workgroup, one 32 x 64 tile of both outputs.  The taps go to LDS as 32-bit words (a broadcast read per use).  The tile and its halo of ntaps / 2 source bytes go to LDS (reflect-101 at the map's
// borders; consecutive lanes read consecutive dwords of a row); the horizontal pass leaves 16-bit row sums in LDS, four per lane at a
// time from a sliding window of bytes; the vertical pass reads four adjacent columns of them per lane and tap (one 64-bit LDS read),
// finishes in registers and stores one dword of L and one of H -- H from the staged centre, so the bitmap is read from HBM once.  No
// sliding column in the vertical pass: a lane makes two rows, 16 apart.
__global__ __launch_bounds__(PREP_THREADS) void k_prepare(PrepareJob J) {
    __shared__ uint32_t stage[PREP_STAGE_WORDS];
    __shared__ alignas(8) uint16_t mid[PREP_MID_ELEMS];
    __shared__ uint32_t w[PREP_MAX_TAPS + 1];
    const int t = (int)threadIdx.x, ntaps = J.taps.n;
    const PrepTile tl = prep_tile((int)blockIdx.x, (int)blockIdx.y, ntaps);
    prep_taps_lane(t, J.taps, w);
    prep_stage_lane(t, tl, J.src, J.W, J.L, J.wide_in != 0, stage);
    __syncthreads();
    prep_hpass_lane(t, tl, w, ntaps, stage, mid);
    __syncthreads();
    prep_vpass_lane(t, tl, w, ntaps, J.penalty, stage, mid, J.out_l, J.out_h, J.W, J.L, J.wide_out != 0);
}
