// ufm_engine.hip -- MI355X (gfx950) cost-propagation engine behind include/ufm.h.
//
// What it replaces: the priority-queue driven G/RHS wavefront of the reference
// replanners -- ReplannerBase::step (ProjectToolkit/include/ReplannerBase.h:43-75)
// with FieldDPlanner / ShiftedGridPlanner / DFMPlanner init/update/plan
// (FieldDStar/FieldDPlanner_impl.h:15-163, ShiftedGridFastMarching/
// ShiftedGridPlanner_impl.h:9-231, DynamicFastMarching/DynamicFastMarching_impl.h:6-132).
//
// How: the serial D*-Lite expansion order is replaced by a block Fast Iterative Method ordered
// like fast marching at tile granularity.  The field G lives densely in HBM; the domain is cut
// into UFM_TILE x UFM_TILE-element tiles (16 by default); per-tile priorities (the smallest value
// that entered a tile since its last visit) drive launches of k_relax, which releases the tiles of
// the current band, stages each (+1 halo) in LDS, sweeps it to its local fixed point with
// asynchronous waves (one 4x4-node patch per wave, four lanes per node), writes it back and queues
// the neighbours whose halo changed.  The fixed point G = F(G) is unique (costs >= 1), so it equals
// the reference's consistent field.  Map patches (cost increases) are handled by an invalidation
// ("raise") phase -- an element whose value is no longer supported by its neighbours is reset to
// +inf, transitively -- followed by the usual lowering phase; both stop at the start's key like the
// reference's end_condition and keep the rest queued across steps.  DESIGN.md has the full story.
//
// Arithmetic contract (bit parity with oracle/ufm_oracle.c): IEEE fp32, one
// rounding per operation (-ffp-contract=off), correctly rounded sqrt.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <thread>
#include <vector>

#include "../../include/ufm.h"

namespace {

#include "ufm_defs.h"
#include "ufm_ops.h"
#include "ufm_relax.h"
#include "ufm_control.h"

#include "ufm_region.h"
#include "ufm_cspace.h"
#include "ufm_census.h"
#include "ufm_sensor.h"
#include "ufm_prepare.h"
#include "ufm_layers.h"

#include "ufm_host.h"
#include "ufm_map_host.h"
#include "ufm_delta.h"

}  // namespace

// ---- debug readers of the diagnostic builds (UFM_SWEEPSTAT, UFM_TIMING: csrc/ufm_defs.h) --------------
extern "C" {

#ifdef UFM_SWEEPSTAT
int ufm_debug_sstat(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sstat), sizeof(unsigned long long) * 32) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[32] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sstat), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
#endif
#ifdef UFM_TIMING
int ufm_debug_trace(unsigned long long *out, int cap) {     // returns the number of records copied (4 words each)
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_ntrace), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > 16384) n = 16384;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), sizeof(unsigned long long) * 4 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    const unsigned int z = 0;
    hipMemcpyToSymbol(HIP_SYMBOL(g_ntrace), &z, sizeof(z));
    return (int)n;
}
int ufm_debug_visits(unsigned int *out, int cap) {   // out[cap][5]; returns the number of visits recorded
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_nvis), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > VIS_DIAG_MAX) n = VIS_DIAG_MAX;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vis), sizeof(unsigned int) * 5 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    return (int)n;
}
int ufm_debug_plog(unsigned int *out, int cap) {     // out[cap][4]
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_nplog), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > PLOG_MAX) n = PLOG_MAX;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plog), sizeof(unsigned int) * 4 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    return (int)n;
}
int ufm_debug_sdiag(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sdiag), sizeof(unsigned long long) * 16) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sdiag), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
int ufm_debug_tiles(unsigned int *out, int n) {     // out[5][n]
    if (n > TILE_DIAG_MAX) n = TILE_DIAG_MAX;
    for (int r = 0; r < 5; ++r)
        if (hipMemcpyFromSymbol(out + (size_t)r * n, HIP_SYMBOL(g_tile), sizeof(unsigned int) * n, sizeof(unsigned int) * (size_t)r * TILE_DIAG_MAX) != hipSuccess) return UFM_ERR_HIP_BASE;
    return n;
}
int ufm_debug_wtrace(unsigned long long *out, unsigned int *counts) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wtrace), sizeof(unsigned long long) * 16 * 256 * 2) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_nw), sizeof(unsigned int) * 16) != hipSuccess) return UFM_ERR_HIP_BASE;
    unsigned int z[16] = {};
    hipMemcpyToSymbol(HIP_SYMBOL(g_nw), z, sizeof(z));
    return UFM_OK;
}
int ufm_debug_tdiag(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tdiag), sizeof(unsigned long long) * 64) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[64] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_tdiag), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
#endif

}  // extern "C"

// ---- C ABI ---------------------------------------------------------------------------
#include "ufm_capi.h"
