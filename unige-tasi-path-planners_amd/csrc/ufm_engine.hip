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

// ---- C ABI ---------------------------------------------------------------------------
struct ufm_planner { Engine *e; };
struct ufm_batch { std::vector<Engine *> shards; int n_maps = 0, per = 1; };

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
int ufm_debug_lmax(ufm_t *p, int32_t *out, int n) {      // diagnostics array of the device (not part of include/ufm.h)
    if (!p || !p->e->allocated || n > LMAX) return UFM_ERR_INVALID;
    hipStreamSynchronize(p->e->stream);
    return hipMemcpy(out, p->e->P.lmax, sizeof(int) * n, hipMemcpyDeviceToHost) == hipSuccess ? UFM_OK : UFM_ERR_HIP_BASE;
}
int ufm_tile_edge(void) { return T; }
#ifdef UFM_STRICT_FENCES
const char *ufm_version(void) { return "ufm-gfx950 0.1 (block-FIM, strict-fence checking build)"; }
#else
const char *ufm_version(void) { return T == 32 ? "ufm-gfx950 0.1 (block-FIM, tile 32)" : "ufm-gfx950 0.1 (block-FIM, tile 16)"; }
#endif

int ufm_create(ufm_t **out, int algo, int opt_lvl, int use_heuristic, int device_id) {
    if (!out) return UFM_ERR_INVALID;
    Engine *e = nullptr;
    int rc = engine_create(&e, 1, algo, opt_lvl, use_heuristic, device_id);
    if (rc != UFM_OK) return rc;
    *out = new ufm_planner{e};
    return UFM_OK;
}
int ufm_destroy(ufm_t *p) {
    if (!p) return UFM_ERR_INVALID;
    int rc = engine_destroy(p->e);
    delete p;
    return rc;
}
int ufm_reset(ufm_t *p) { if (!p) return UFM_ERR_INVALID; p->e->maps[0].initialize_search = true; return UFM_OK; }
int ufm_set_occupancy_threshold(ufm_t *p, float thr) {
    if (!p) return UFM_ERR_INVALID;
    p->e->thr_uchar = (int)(thr * 255.0f);   // Graph.cpp:18-20
    return UFM_OK;
}
int ufm_set_heuristic_multiplier(ufm_t *p, float mult) { if (!p) return UFM_ERR_INVALID; p->e->heuristic_multiplier = mult; return UFM_OK; }
int ufm_set_map(ufm_t *p, const uint8_t *host_map, int width, int length) { return p ? engine_set_map(p->e, 0, host_map, false, width, length) : UFM_ERR_INVALID; }
int ufm_set_map_device(ufm_t *p, const uint8_t *dev_map, int width, int length) { return p ? engine_set_map(p->e, 0, dev_map, true, width, length) : UFM_ERR_INVALID; }
int ufm_patch_map(ufm_t *p, const uint8_t *host_patch, int x, int y, int w, int h) { return p ? engine_patch(p->e, 0, host_patch, false, x, y, w, h) : UFM_ERR_INVALID; }
int ufm_patch_map_device(ufm_t *p, const uint8_t *dev_patch, int x, int y, int w, int h) { return p ? engine_patch(p->e, 0, dev_patch, true, x, y, w, h) : UFM_ERR_INVALID; }
int ufm_set_start(ufm_t *p, float x, float y) {
    if (!p) return UFM_ERR_INVALID;
    MapState &ms = p->e->maps[0];
    ms.start_x = x; ms.start_y = y; ms.new_start = true; ms.start_set = true;   // ReplannerBase.h:94-97
    return UFM_OK;
}
int ufm_set_goal(ufm_t *p, float x, float y) { return p ? engine_set_goal(p->e, 0, x, y) : UFM_ERR_INVALID; }
int ufm_step(ufm_t *p, ufm_stats *stats) {
    if (!p) return UFM_ERR_INVALID;
    if (hipSetDevice(p->e->device) != hipSuccess) return UFM_ERR_HIP_BASE;
    return p->e->step(stats);
}
int ufm_field_dims(const ufm_t *p, int *nx, int *ny) {
    if (!p || !p->e->allocated) return UFM_ERR_INVALID;
    if (nx) *nx = p->e->P.EX;
    if (ny) *ny = p->e->P.EY;
    return UFM_OK;
}
int ufm_read_field(ufm_t *p, int x0, int y0, int nx, int ny, float *g, float *rhs) { return p ? engine_read_field(p->e, 0, x0, y0, nx, ny, g, rhs) : UFM_ERR_INVALID; }
static int engine_check_layout(Engine *e, uint64_t *bad_ring, uint64_t *bad_cost) {
    if (!e || !e->allocated) return UFM_ERR_INVALID;
    for (const MapState &ms : e->maps) if (!ms.have_map) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    unsigned long long *d_acc = reinterpret_cast<unsigned long long *>(e->d_scratch);
    HIPCHK(hipMemsetAsync(d_acc, 0, 2 * sizeof(unsigned long long), e->stream));
    k_check_layout<<<1024, 256, 0, e->stream>>>(e->P, d_acc);
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, d_acc, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (bad_ring) *bad_ring = h[0];
    if (bad_cost) *bad_cost = h[1];
    return UFM_OK;
}
int ufm_check_layout(ufm_t *p, uint64_t *bad_ring, uint64_t *bad_cost) { return p ? engine_check_layout(p->e, bad_ring, bad_cost) : UFM_ERR_INVALID; }
static int engine_check_info(Engine *e, uint64_t out[6]) {
    if (!e || !e->allocated || !out) return UFM_ERR_INVALID;
    if (e->algo == UFM_ALGO_DFM && e->opt_lvl == 0) return UFM_ERR_INVALID;       // (MS-DFM level 0: its map has no Info, there are no bytes)
    for (const MapState &ms : e->maps) if (!ms.have_map) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    unsigned long long *d_acc = reinterpret_cast<unsigned long long *>(e->d_scratch);
    HIPCHK(hipMemsetAsync(d_acc, 0, 6 * sizeof(unsigned long long), e->stream));
    with_lower_op(e->algo, [&](auto a) { k_check_bp<a()><<<1024, 256, 0, e->stream>>>(e->P, d_acc); });
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, d_acc, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 6; ++i) out[i] = h[i];
    return UFM_OK;
}
int ufm_check_info(ufm_t *p, uint64_t out[6]) { return p ? engine_check_info(p->e, out) : UFM_ERR_INVALID; }
int ufm_batch_check_info(ufm_batch_t *b, uint64_t out[6]) {
    if (!b || !out) return UFM_ERR_INVALID;
    uint64_t acc[6] = {0, 0, 0, 0, 0, 0};
    for (Engine *e : b->shards) {
        uint64_t o[6];
        const int rc = engine_check_info(e, o);
        if (rc != UFM_OK) return rc;
        for (int i = 0; i < 6; ++i) acc[i] += o[i];
    }
    for (int i = 0; i < 6; ++i) out[i] = acc[i];
    return UFM_OK;
}
int ufm_batch_check_layout(ufm_batch_t *b, uint64_t *bad_ring, uint64_t *bad_cost) {
    if (!b) return UFM_ERR_INVALID;
    uint64_t r = 0, c = 0;
    for (Engine *e : b->shards) {
        uint64_t a = 0, d = 0;
        const int rc = engine_check_layout(e, &a, &d);
        if (rc != UFM_OK) return rc;
        r += a; c += d;
    }
    if (bad_ring) *bad_ring = r;
    if (bad_cost) *bad_cost = c;
    return UFM_OK;
}
int ufm_read_map(ufm_t *p, uint8_t *host_map) { return p ? engine_read_map(p->e, 0, host_map) : UFM_ERR_INVALID; }
int ufm_set_cspace(ufm_t *p, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) { return p ? engine_set_cspace(p->e, mask, mw, mh, anchor_row, anchor_col) : UFM_ERR_INVALID; }
int ufm_read_raw_map(ufm_t *p, uint8_t *host_map) { return p ? engine_read_raw_map(p->e, 0, host_map) : UFM_ERR_INVALID; }
static int engine_set_param(Engine *e, const char *name, double value) {
    if (!e || !name) return UFM_ERR_INVALID;
    if (!std::strcmp(name, "delta")) e->delta_abs = (float)value;
    else if (!std::strcmp(name, "delta_scale")) { e->delta_scale = e->delta_scale_long = (float)value; e->delta_abs = -1.0f; }
    else if (!std::strcmp(name, "delta_scale_long")) { e->delta_scale_long = (float)value; e->delta_abs = -1.0f; }
    else if (!std::strcmp(name, "max_iters")) e->max_iters = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "batch")) e->batch_fixed = value < 0 ? 0 : (value > 1024 ? 1024 : (int)value);
    else if (!std::strcmp(name, "pipeline_batches")) e->pipeline_batches = value != 0;
    else if (!std::strcmp(name, "grid")) e->grid_relax = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "small_grid")) e->small_grid = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "dyn_grid")) e->dyn_grid = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "spin_wait")) e->spin_wait = value != 0;
    else if (!std::strcmp(name, "fuse_control")) e->fuse_control = value != 0;
    else if (!std::strcmp(name, "graph")) e->use_graph = value != 0;
    else if (!std::strcmp(name, "region")) e->use_region = value != 0;
    else if (!std::strcmp(name, "owned")) e->use_owned = value != 0;
    else if (!std::strcmp(name, "owned_limit_ms")) e->owned_limit_ms = (float)value;
    else if (!std::strcmp(name, "owned_band")) e->owned_band = (float)value;
    else if (!std::strcmp(name, "owned_flags")) e->owned_flags = (int)value;
    else if (!std::strcmp(name, "owned_waves")) e->owned_waves = (int)value;
    else if (!std::strcmp(name, "defer_patches")) { if (e->allocated) { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; } e->defer_patches = value != 0; }
    else if (!std::strcmp(name, "auto_multiplier")) {         // the census' minimum as the heuristic multiplier; 1 turns the census on
        if (value != 0.0) { const int rc = engine_track_costs(e, 1); if (rc != UFM_OK) return rc; }
        e->auto_multiplier = value != 0.0;
    }
    else if (!std::strcmp(name, "region_debug")) e->region_debug = (int)value;
    else if (!std::strcmp(name, "region_band")) e->region_band = (float)value;
    else if (!std::strcmp(name, "region_ahead")) e->region_ahead = (int)value;
    else if (!std::strcmp(name, "region_tiles")) e->region_tiles = value < 3 ? 3 : (value > RTMAX ? RTMAX : (int)value);
    else if (!std::strcmp(name, "cont_raise")) e->cont_raise = value < 0 ? 0 : (int)value;
    else if (!std::strcmp(name, "cont_lower")) e->cont_lower = value < 0 ? 0 : (int)value;
    else if (!std::strcmp(name, "region_sweeps")) e->region_sweeps = value < 16 ? 16 : (int)value;
    else if (!std::strcmp(name, "batch_margin")) e->batch_margin = (int)value;
    else if (!std::strcmp(name, "raise_margin")) e->raise_margin = (float)value;
    else if (!std::strcmp(name, "tail_grid")) e->tail_grid = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "profile_stride")) e->profile_stride = value < 1 ? 1 : (int)value;
    else if (!std::strcmp(name, "focused")) e->focused = value != 0.0;
    else if (!std::strcmp(name, "start_cell_floor")) e->start_cell_floor = value != 0.0;
    else if (!std::strcmp(name, "lazy_patches")) { if (e->allocated) { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; } e->lazy_patches = value != 0; }
    else if (!std::strcmp(name, "dynamic")) e->dynamic_mode = value != 0.0;
    else if (!std::strcmp(name, "dfm_follow_info")) {         // MS-DFM level 1: invalidation along the stored bytes (no effect on FD / SG, which always do)
        if (value != 0.0 && e->algo == UFM_ALGO_DFM && e->opt_lvl == 0) return UFM_ERR_INVALID;
        e->dfm_follow_info = value != 0.0 && e->algo == UFM_ALGO_DFM;
    }
    else return UFM_ERR_INVALID;
    return UFM_OK;
}
int ufm_set_param(ufm_t *p, const char *name, double value) { return p ? engine_set_param(p->e, name, value) : UFM_ERR_INVALID; }
int ufm_batch_set_param(ufm_batch_t *b, const char *name, double value) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_param(e, name, value); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
// the census of the engines' maps `first` .. `first + count - 1` (numbered through the shards, `per` to a shard), summed
static int census_sum(Engine *const *shards, int per, int first, int count, uint64_t hist[256], int *min_cost, int *max_cost) {
    uint64_t acc[CENSUS_BINS] = {};
    for (int i = first; i < first + count; ++i) {
        uint32_t h[CENSUS_BINS];
        const int rc = engine_read_census(shards[i / per], i % per, h);
        if (rc != UFM_OK) return rc;
        for (int v = 0; v < CENSUS_BINS; ++v) acc[v] += h[v];
    }
    int mn = CENSUS_BINS, mx = -1;
    for (int v = 0; v < CENSUS_BINS; ++v) if (acc[v]) { mn = std::min(mn, v); mx = v; }
    if (hist) std::memcpy(hist, acc, sizeof(acc));
    if (min_cost) *min_cost = mn;
    if (max_cost) *max_cost = mx;
    return UFM_OK;
}
int ufm_track_costs(ufm_t *p, int enable) { return p ? engine_track_costs(p->e, enable) : UFM_ERR_INVALID; }
int ufm_read_cost_census(ufm_t *p, uint64_t hist[256], int *min_cost, int *max_cost) { return p ? census_sum(&p->e, 1, 0, 1, hist, min_cost, max_cost) : UFM_ERR_INVALID; }
int ufm_heuristic_multiplier(ufm_t *p, float *used) { if (!p || !used) return UFM_ERR_INVALID; *used = p->e->last_multiplier; return UFM_OK; }
int ufm_set_sensor(ufm_t *p, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) { return p ? engine_set_sensor(p->e, mask, mw, mh, anchor_row, anchor_col) : UFM_ERR_INVALID; }
int ufm_set_survey(ufm_t *p, const uint8_t *host_survey, int width, int length) { return p ? engine_set_layer_survey(p->e, 0, 0, host_survey, false, width, length) : UFM_ERR_INVALID; }
int ufm_set_survey_device(ufm_t *p, const uint8_t *dev_survey, int width, int length) { return p ? engine_set_layer_survey(p->e, 0, 0, dev_survey, true, width, length) : UFM_ERR_INVALID; }
int ufm_read_survey(ufm_t *p, uint8_t *host_survey) { return p ? engine_read_layer_survey(p->e, 0, 0, host_survey, false) : UFM_ERR_INVALID; }
int ufm_reveal(ufm_t *p, int row, int col, uint64_t *changed) {
    if (!p) return UFM_ERR_INVALID;
    const int32_t c[2] = {row, col};
    if (row < 0) return UFM_ERR_INVALID;        // (a single planner has no map to skip)
    HIPCHK(hipSetDevice(p->e->device));
    { int rc = p->e->reveal(c); if (rc != UFM_OK) return rc; }
    return changed ? p->e->reveal_counts(c, changed) : UFM_OK;
}
int ufm_gaussian_taps(int ksize, uint16_t *taps) { return prep_gaussian_taps(ksize, taps) ? UFM_OK : UFM_ERR_INVALID; }
int ufm_set_image(ufm_t *p, const uint8_t *host_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    return p ? engine_set_image(p->e, 0, host_image, false, width, length, taps, ntaps, penalty) : UFM_ERR_INVALID;
}
int ufm_set_image_device(ufm_t *p, const uint8_t *dev_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    return p ? engine_set_image(p->e, 0, dev_image, true, width, length, taps, ntaps, penalty) : UFM_ERR_INVALID;
}
int ufm_set_layers(ufm_t *p, int n) { return p ? engine_set_layers(p->e, n) : UFM_ERR_INVALID; }
int ufm_patch_layer(ufm_t *p, int k, const uint8_t *host_patch, int x, int y, int w, int h) { return p ? engine_patch_layer(p->e, 0, k, host_patch, false, x, y, w, h) : UFM_ERR_INVALID; }
int ufm_patch_layer_device(ufm_t *p, int k, const uint8_t *dev_patch, int x, int y, int w, int h) { return p ? engine_patch_layer(p->e, 0, k, dev_patch, true, x, y, w, h) : UFM_ERR_INVALID; }
int ufm_set_layer(ufm_t *p, int k, const uint8_t *host_raster, int width, int length) { return p ? engine_set_layer(p->e, 0, k, host_raster, false, width, length) : UFM_ERR_INVALID; }
int ufm_set_layer_device(ufm_t *p, int k, const uint8_t *dev_raster, int width, int length) { return p ? engine_set_layer(p->e, 0, k, dev_raster, true, width, length) : UFM_ERR_INVALID; }
int ufm_set_layer_survey(ufm_t *p, int k, const uint8_t *host_survey, int width, int length) { return p ? engine_set_layer_survey(p->e, 0, k, host_survey, false, width, length) : UFM_ERR_INVALID; }
int ufm_set_layer_survey_device(ufm_t *p, int k, const uint8_t *dev_survey, int width, int length) { return p ? engine_set_layer_survey(p->e, 0, k, dev_survey, true, width, length) : UFM_ERR_INVALID; }
int ufm_read_layer(ufm_t *p, int k, uint8_t *host_raster) { return p ? engine_read_layer(p->e, 0, k, host_raster) : UFM_ERR_INVALID; }
int ufm_read_layer_survey(ufm_t *p, int k, uint8_t *host_survey) { return p ? engine_read_layer_survey(p->e, 0, k, host_survey) : UFM_ERR_INVALID; }
// profiling: duration of the last layer kernel (k_layer_compose / k_layer_compose_all / k_reveal_layers), taken from the dispatch while
// ufm_set_profiling is on (tools/layers_probe.py; not part of include/ufm.h)
int ufm_debug_layers_ms(ufm_t *p, float *ms) {
    if (!p || !ms || !p->e->lay_timed) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(p->e->device));
    HIPCHK(hipStreamSynchronize(p->e->stream));
    HIPCHK(hipEventElapsedTime(ms, p->e->lay_ev[0], p->e->lay_ev[1]));
    return UFM_OK;
}
int ufm_set_profiling(ufm_t *p, int enable) { if (!p) return UFM_ERR_INVALID; p->e->profiling = enable != 0; return UFM_OK; }
void *ufm_stream(ufm_t *p) { return p ? (void *)p->e->stream : nullptr; }

// A batch is one engine per device; map i lives in shard i / per (contiguous blocks of maps).
static int batch_locate(const ufm_batch *b, int i, Engine **e, int *local) {
    if (!b || i < 0 || i >= b->n_maps) return UFM_ERR_INVALID;
    const int s = i / b->per;
    *e = b->shards[s];
    *local = i - s * b->per;
    return UFM_OK;
}
int ufm_batch_create_sharded(ufm_batch_t **out, int n_maps, int algo, int opt_lvl, int use_heuristic, const int *devices, int n_devices) {
    if (!out || !devices || n_devices < 1 || n_maps < n_devices) return UFM_ERR_INVALID;
    ufm_batch *b = new (std::nothrow) ufm_batch();
    if (!b) return UFM_ERR_NOMEM;
    b->n_maps = n_maps;
    b->per = (n_maps + n_devices - 1) / n_devices;
    for (int s = 0; s * b->per < n_maps; ++s) {
        Engine *e = nullptr;
        const int cnt = std::min(b->per, n_maps - s * b->per);
        const int rc = engine_create(&e, cnt, algo, opt_lvl, use_heuristic, devices[s]);
        if (rc != UFM_OK) { ufm_batch_destroy(b); return rc; }
        b->shards.push_back(e);
    }
    *out = b;
    return UFM_OK;
}
int ufm_batch_create(ufm_batch_t **out, int n_maps, int algo, int opt_lvl, int use_heuristic, int device_id) {
    return ufm_batch_create_sharded(out, n_maps, algo, opt_lvl, use_heuristic, &device_id, 1);
}
int ufm_batch_destroy(ufm_batch_t *b) {
    if (!b) return UFM_ERR_INVALID;
    int rc = UFM_OK;
    for (Engine *e : b->shards) { const int r = engine_destroy(e); if (rc == UFM_OK) rc = r; }
    delete b;
    return rc;
}
int ufm_batch_size(const ufm_batch_t *b) { return b ? b->n_maps : UFM_ERR_INVALID; }
int ufm_batch_shards(const ufm_batch_t *b) { return b ? (int)b->shards.size() : UFM_ERR_INVALID; }
int ufm_batch_set_occupancy_threshold(ufm_batch_t *b, float thr) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->thr_uchar = (int)(thr * 255.0f);
    return UFM_OK;
}
int ufm_batch_set_heuristic_multiplier(ufm_batch_t *b, float mult) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->heuristic_multiplier = mult;
    return UFM_OK;
}
int ufm_batch_track_costs(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_track_costs(e, enable); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_batch_read_cost_census(ufm_batch_t *b, int i, uint64_t hist[256], int *min_cost, int *max_cost) {
    if (!b || b->shards.empty() || i < -1 || i >= b->n_maps) return UFM_ERR_INVALID;
    return i < 0 ? census_sum(b->shards.data(), b->per, 0, b->n_maps, hist, min_cost, max_cost)
                 : census_sum(b->shards.data(), b->per, i, 1, hist, min_cost, max_cost);
}
int ufm_batch_heuristic_multiplier(ufm_batch_t *b, float *used) {
    if (!b || b->shards.empty() || !used) return UFM_ERR_INVALID;
    *used = b->shards[0]->last_multiplier;
    return UFM_OK;
}
#define UFM_BATCH_MAP(b, i) Engine *e = nullptr; int li = 0; { const int rc_ = batch_locate(b, i, &e, &li); if (rc_ != UFM_OK) return rc_; }
int ufm_batch_set_map(ufm_batch_t *b, int i, const uint8_t *host_map, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_map(e, li, host_map, false, width, length); }
int ufm_batch_set_map_device(ufm_batch_t *b, int i, const uint8_t *dev_map, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_map(e, li, dev_map, true, width, length); }
int ufm_batch_patch_map(ufm_batch_t *b, int i, const uint8_t *host_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch(e, li, host_patch, false, x, y, w, h); }
int ufm_batch_patch_map_device(ufm_batch_t *b, int i, const uint8_t *dev_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch(e, li, dev_patch, true, x, y, w, h); }
int ufm_batch_set_start(ufm_batch_t *b, int i, float x, float y) {
    UFM_BATCH_MAP(b, i);
    MapState &ms = e->maps[li];
    ms.start_x = x; ms.start_y = y; ms.new_start = true; ms.start_set = true;
    return UFM_OK;
}
int ufm_batch_set_goal(ufm_batch_t *b, int i, float x, float y) { UFM_BATCH_MAP(b, i); return engine_set_goal(e, li, x, y); }
int ufm_batch_reset(ufm_batch_t *b, int i) {
    UFM_BATCH_MAP(b, i);
    e->maps[li].initialize_search = true;
    return UFM_OK;
}
// One step of every map.  Shards on different devices advance side by side, one host thread each (a step is
// synchronous: its host thread spins on the device's published counters); the statistics are summed, the times
// are those of the slowest shard.
int ufm_batch_step(ufm_batch_t *b, ufm_stats *stats) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    const size_t n = b->shards.size();
    std::vector<ufm_stats> st(n);
    std::vector<int> rcs(n, UFM_OK);
    // "auto_multiplier": one multiplier for the whole batch, the smallest cost over all maps of all shards -- admissible for every map, and
    // the same however the maps are spread (a shard with a map still missing fails its step below)
    float auto_mult = 0.0f;
    const float *auto_ptr = nullptr;
    if (n > 1 && b->shards[0]->auto_multiplier && b->shards[0]->heur) {
        int mn = CENSUS_BINS;
        for (Engine *e : b->shards) {
            int a = 0, c = 0;
            if (hipSetDevice(e->device) != hipSuccess) return UFM_ERR_HIP_BASE;
            const int rc = e->census_minmax(&a, &c);
            if (rc != UFM_OK) return rc;
            mn = std::min(mn, a);
        }
        auto_mult = (float)mn; auto_ptr = &auto_mult;
    }
    auto run = [&](size_t s) {
        if (hipSetDevice(b->shards[s]->device) != hipSuccess) { rcs[s] = UFM_ERR_HIP_BASE; return; }
        rcs[s] = b->shards[s]->step(&st[s], auto_ptr);
    };
    if (n == 1) run(0);
    else {
        std::vector<std::thread> th;
        for (size_t s = 1; s < n; ++s) th.emplace_back(run, s);
        run(0);
        for (auto &t : th) t.join();
    }
    for (size_t s = 0; s < n; ++s) if (rcs[s] != UFM_OK) return rcs[s];
    if (stats) {
        ufm_stats a = st[0];
        for (size_t s = 1; s < n; ++s) {
            const ufm_stats &c = st[s];
            a.u_ms = std::max(a.u_ms, c.u_ms); a.p_ms = std::max(a.p_ms, c.p_ms);
            a.updated += c.updated; a.expanded += c.expanded; a.tile_visits += c.tile_visits; a.tile_iters += c.tile_iters;
            a.elem_evals += c.elem_evals; a.launches += c.launches; a.raise_launches += c.raise_launches; a.kernel_ms += c.kernel_ms;
            a.crit_sweeps += c.crit_sweeps; a.raise_tile_visits += c.raise_tile_visits; a.raise_kernel_ms += c.raise_kernel_ms;
            a.queued_lower += c.queued_lower; a.queued_raise += c.queued_raise; a.timed_launches += c.timed_launches;
            a.timed_raise_launches += c.timed_raise_launches; a.graphs_instantiated += c.graphs_instantiated;
            a.region_replans += c.region_replans; a.region_replans_done += c.region_replans_done;
            a.resident_launches += c.resident_launches; a.resident_kernel_ms += c.resident_kernel_ms;
            a.resident_stops += c.resident_stops; a.resident_tile_visits += c.resident_tile_visits;
            a.region_launches += c.region_launches; a.region_timed += c.region_timed; a.region_kernel_ms += c.region_kernel_ms; a.region_tiles += c.region_tiles;
        }
        *stats = a;
    }
    return UFM_OK;
}
int ufm_batch_read_field(ufm_batch_t *b, int i, int x0, int y0, int nx, int ny, float *g, float *rhs) { UFM_BATCH_MAP(b, i); return engine_read_field(e, li, x0, y0, nx, ny, g, rhs); }
int ufm_batch_read_map(ufm_batch_t *b, int i, uint8_t *host_map) { UFM_BATCH_MAP(b, i); return engine_read_map(e, li, host_map); }
int ufm_batch_read_raw_map(ufm_batch_t *b, int i, uint8_t *host_map) { UFM_BATCH_MAP(b, i); return engine_read_raw_map(e, li, host_map); }
int ufm_batch_set_cspace(ufm_batch_t *b, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;   // (all shards or none)
    for (Engine *e : b->shards) { const int rc = engine_set_cspace(e, mask, mw, mh, anchor_row, anchor_col); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_batch_set_sensor(ufm_batch_t *b, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) {
    if (!b || b->shards.empty() || !sensor_valid(mask, mw, mh, anchor_row, anchor_col)) return UFM_ERR_INVALID;   // (all shards or none)
    for (Engine *e : b->shards) { const int rc = engine_set_sensor(e, mask, mw, mh, anchor_row, anchor_col); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_batch_set_survey(ufm_batch_t *b, int i, const uint8_t *host_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, 0, host_survey, false, width, length); }
int ufm_batch_set_survey_device(ufm_batch_t *b, int i, const uint8_t *dev_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, 0, dev_survey, true, width, length); }
int ufm_batch_set_image(ufm_batch_t *b, int i, const uint8_t *host_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    UFM_BATCH_MAP(b, i);
    return engine_set_image(e, li, host_image, false, width, length, taps, ntaps, penalty);
}
int ufm_batch_set_image_device(ufm_batch_t *b, int i, const uint8_t *dev_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    UFM_BATCH_MAP(b, i);
    return engine_set_image(e, li, dev_image, true, width, length, taps, ntaps, penalty);
}
int ufm_batch_read_survey(ufm_batch_t *b, int i, uint8_t *host_survey) { UFM_BATCH_MAP(b, i); return engine_read_layer_survey(e, li, 0, host_survey, false); }
int ufm_batch_set_layers(ufm_batch_t *b, int n) {
    if (!b || b->shards.empty() || !layers_count_ok(n)) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;   // (all shards or none)
    for (Engine *e : b->shards) { const int rc = engine_set_layers(e, n); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_batch_patch_layer(ufm_batch_t *b, int i, int k, const uint8_t *host_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch_layer(e, li, k, host_patch, false, x, y, w, h); }
int ufm_batch_patch_layer_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch_layer(e, li, k, dev_patch, true, x, y, w, h); }
int ufm_batch_set_layer(ufm_batch_t *b, int i, int k, const uint8_t *host_raster, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer(e, li, k, host_raster, false, width, length); }
int ufm_batch_set_layer_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_raster, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer(e, li, k, dev_raster, true, width, length); }
int ufm_batch_set_layer_survey(ufm_batch_t *b, int i, int k, const uint8_t *host_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, k, host_survey, false, width, length); }
int ufm_batch_set_layer_survey_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, k, dev_survey, true, width, length); }
int ufm_batch_read_layer(ufm_batch_t *b, int i, int k, uint8_t *host_raster) { UFM_BATCH_MAP(b, i); return engine_read_layer(e, li, k, host_raster); }
int ufm_batch_read_layer_survey(ufm_batch_t *b, int i, int k, uint8_t *host_survey) { UFM_BATCH_MAP(b, i); return engine_read_layer_survey(e, li, k, host_survey); }
// The maps grouped by the device that owns them (contiguous blocks: a shard's centres are a slice of the caller's array): every shard is
// checked before any of them launches; then one k_reveal per shard, queued side by side, and only then the counts are waited for.
int ufm_batch_reveal(ufm_batch_t *b, const int32_t *centres, uint64_t *changed) {
    if (!b || b->shards.empty() || !centres) return UFM_ERR_INVALID;
    for (size_t s = 0; s < b->shards.size(); ++s) {
        const int rc = b->shards[s]->reveal_check(centres + 2 * s * (size_t)b->per);
        if (rc != UFM_OK) return rc;
    }
    for (size_t s = 0; s < b->shards.size(); ++s) {
        HIPCHK(hipSetDevice(b->shards[s]->device));
        const int rc = b->shards[s]->reveal(centres + 2 * s * (size_t)b->per);
        if (rc != UFM_OK) return rc;
    }
    if (!changed) return UFM_OK;
    for (size_t s = 0; s < b->shards.size(); ++s) {
        HIPCHK(hipSetDevice(b->shards[s]->device));
        const int rc = b->shards[s]->reveal_counts(centres + 2 * s * (size_t)b->per, changed + s * (size_t)b->per);
        if (rc != UFM_OK) return rc;
    }
    return UFM_OK;
}
int ufm_batch_set_profiling(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->profiling = enable != 0;
    return UFM_OK;
}
void *ufm_batch_stream(ufm_batch_t *b, int shard) { return (b && shard >= 0 && shard < (int)b->shards.size()) ? (void *)b->shards[shard]->stream : nullptr; }

int ufm_read_info(ufm_t *p, int x0, int y0, int nx, int ny, int32_t *info) { return p ? engine_read_info(p->e, 0, x0, y0, nx, ny, info, false) : UFM_ERR_INVALID; }
int ufm_read_info_derived(ufm_t *p, int x0, int y0, int nx, int ny, int32_t *info) { return p ? engine_read_info(p->e, 0, x0, y0, nx, ny, info, true) : UFM_ERR_INVALID; }
int ufm_read_queue(ufm_t *p, int cap, int32_t *xy, float *g_rhs, int *total) { return p ? engine_read_queue(p->e, 0, cap, xy, g_rhs, total) : UFM_ERR_INVALID; }
int ufm_track_changes(ufm_t *p, int enable) { return p ? engine_track_changes(p->e, enable) : UFM_ERR_INVALID; }
int ufm_read_changes(ufm_t *p, int cap, int32_t *xy, float *g, int32_t *info, int *total) { return p ? engine_read_changes(p->e, 0, cap, xy, g, info, total) : UFM_ERR_INVALID; }
int ufm_batch_track_changes(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_track_changes(e, enable); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_batch_read_changes(ufm_batch_t *b, int i, int cap, int32_t *xy, float *g, int32_t *info, int *total) { UFM_BATCH_MAP(b, i); return engine_read_changes(e, li, cap, xy, g, info, total); }
// profiling: duration of the last scan kernel of ufm_read_changes (tools/delta_probe.py; not part of include/ufm.h)
int ufm_debug_delta_ms(ufm_t *p, float *ms) { if (!p || !ms) return UFM_ERR_INVALID; *ms = p->e->trk_scan_ms; return UFM_OK; }
// profiling: duration of the last k_prepare of ufm_set_image / of map i's ufm_batch_set_image, taken from the dispatch while
// ufm_set_profiling is on (tools/prepare_probe.py; not part of include/ufm.h)
int ufm_debug_prepare_ms(ufm_t *p, float *ms) { if (!p || !ms) return UFM_ERR_INVALID; *ms = p->e->prep_ms; return UFM_OK; }
int ufm_debug_batch_prepare_ms(ufm_batch_t *b, int i, float *ms) { UFM_BATCH_MAP(b, i); if (!ms) return UFM_ERR_INVALID; *ms = e->prep_ms; return UFM_OK; }
int ufm_extract_path(ufm_t *p, int max_steps, int lookahead, int allow_indirect,
                     float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    return p ? engine_extract_path(p->e, max_steps, lookahead, allow_indirect, path_xy, cap_points, step_costs, cap_costs, info) : UFM_ERR_INVALID;
}
int ufm_batch_extract_path(ufm_batch_t *b, int max_steps, int lookahead, int allow_indirect,
                           float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (!b) return UFM_ERR_INVALID;
    int first = 0;                      // shard by shard (one launch each), outputs in map order
    for (Engine *e : b->shards) {
        const int rc = engine_extract_path(e, max_steps, lookahead, allow_indirect,
                                           path_xy ? path_xy + (size_t)first * cap_points * 2 : nullptr, cap_points,
                                           step_costs ? step_costs + (size_t)first * cap_costs : nullptr, cap_costs, info ? info + first : nullptr);
        if (rc != UFM_OK) return rc;
        first += e->nmaps;
    }
    return UFM_OK;
}
int ufm_extract_paths_from(ufm_t *p, int n_starts, const float *starts_xy, int max_steps, int lookahead, int allow_indirect,
                           float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    return p ? paths_from(&p->e, 1, 1, n_starts, nullptr, starts_xy, max_steps, lookahead, allow_indirect, path_xy, cap_points, step_costs, cap_costs, info)
             : UFM_ERR_INVALID;
}
int ufm_batch_extract_paths_from(ufm_batch_t *b, int n_starts, const int32_t *map_index, const float *starts_xy, int max_steps, int lookahead,
                                 int allow_indirect, float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (!b || b->shards.empty() || !map_index) return UFM_ERR_INVALID;
    return paths_from(b->shards.data(), b->per, b->n_maps, n_starts, map_index, starts_xy, max_steps, lookahead, allow_indirect,
                      path_xy, cap_points, step_costs, cap_costs, info);
}

}  // extern "C"
