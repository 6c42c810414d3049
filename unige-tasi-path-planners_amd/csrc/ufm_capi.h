// ufm_capi.h -- the C ABI of include/ufm.h over the engine (a piece of ufm_engine.hip: included there last, outside its anonymous namespace).
//
// One handle shape.  A batch is one engine per device ("shard"); map i lives in shard i / per (contiguous blocks of maps).  A planner IS a
// batch of one map on one shard -- nothing in the engine asks for more than nmaps == 1 -- so every ufm_X with a batch twin is a one-line
// forward to ufm_batch_X with map 0, and the batch form is the only one with a body.  Calls that exist for a planner alone
// (ufm_field_dims, ufm_read_info*, ufm_read_queue, ufm_debug_*) use shard 0, map 0 of the same handle.  Where the two forms differ
// (DESIGN.md section 2.1): ufm_reveal refuses row < 0, which a batch reads as "skip this map"; ufm_extract_paths_from takes no map
// indices, which ufm_batch_extract_paths_from requires; likewise ufm_score_paths and ufm_batch_score_paths.
#pragma once

struct ufm_batch { std::vector<Engine *> shards; int n_maps = 0, per = 1; };
struct ufm_planner : ufm_batch {};

static int batch_locate(const ufm_batch *b, int i, Engine **e, int *local) {
    if (!b || i < 0 || i >= b->n_maps) return UFM_ERR_INVALID;
    const int s = i / b->per;
    *e = b->shards[s];
    *local = i - s * b->per;
    return UFM_OK;
}
#define UFM_BATCH_MAP(b, i) Engine *e = nullptr; int li = 0; { const int rc_ = batch_locate(b, i, &e, &li); if (rc_ != UFM_OK) return rc_; }
// the engines of a new handle; on failure those made so far stay in b for batch_release
static int batch_fill(ufm_batch *b, int n_maps, int algo, int opt_lvl, int use_heuristic, const int *devices, int n_devices) {
    b->n_maps = n_maps;
    b->per = (n_maps + n_devices - 1) / n_devices;
    for (int s = 0; s * b->per < n_maps; ++s) {
        Engine *e = nullptr;
        const int rc = engine_create(&e, std::min(b->per, n_maps - s * b->per), algo, opt_lvl, use_heuristic, devices[s]);
        if (rc != UFM_OK) return rc;
        b->shards.push_back(e);
    }
    return UFM_OK;
}
static int batch_release(ufm_batch *b) {
    int rc = UFM_OK;
    for (Engine *e : b->shards) { const int r = engine_destroy(e); if (rc == UFM_OK) rc = r; }
    b->shards.clear();
    return rc;
}

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
    *bad_ring = h[0];
    *bad_cost = h[1];
    return UFM_OK;
}
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
// the four knobs that need the engine, then the table (ufm_knobs.h)
static int engine_set_param(Engine *e, const char *name, double value) {
    if (!e || !name) return UFM_ERR_INVALID;
    const bool defer = !std::strcmp(name, "defer_patches");
    if (defer || !std::strcmp(name, "lazy_patches")) {        // what is being held or deferred under the old setting is applied first
        if (e->allocated) { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
        (defer ? e->defer_patches : e->lazy_patches) = value != 0;
    } else if (!std::strcmp(name, "auto_multiplier")) {       // the census' minimum as the heuristic multiplier; 1 turns the census on
        if (value != 0.0) { const int rc = engine_track_costs(e, 1); if (rc != UFM_OK) return rc; }
        e->auto_multiplier = value != 0.0;
    } else if (!std::strcmp(name, "dfm_follow_info")) {       // MS-DFM level 1: invalidation along the stored bytes (no effect on FD / SG, which always do)
        if (value != 0.0 && e->algo == UFM_ALGO_DFM && e->opt_lvl == 0) return UFM_ERR_INVALID;
        e->dfm_follow_info = value != 0.0 && e->algo == UFM_ALGO_DFM;
    } else if (!knob_set(*e, name, value, RTMAX)) return UFM_ERR_INVALID;
    return UFM_OK;
}
// the census of the maps `first` .. `first + count - 1` of the batch, summed
static int census_sum(const ufm_batch *b, int first, int count, uint64_t hist[256], int *min_cost, int *max_cost) {
    uint64_t acc[CENSUS_BINS] = {};
    for (int i = first; i < first + count; ++i) {
        uint32_t h[CENSUS_BINS];
        const int rc = engine_read_census(b->shards[i / b->per], i % b->per, h);
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
// How the shards' statistics become the batch's: one row per field of ufm_stats -- counts are summed, the times the host measures are
// those of the slowest shard.  tests/test_capi_surface.py holds the rows against the fields include/ufm.h declares: a field without a
// row fails there.
#define UFM_STATS_MERGE(SUM, MAX) \
    MAX(u_ms) MAX(p_ms) SUM(updated) SUM(expanded) SUM(tile_visits) SUM(tile_iters) SUM(elem_evals) SUM(launches) SUM(raise_launches) \
    SUM(kernel_ms) SUM(crit_sweeps) SUM(raise_tile_visits) SUM(raise_kernel_ms) SUM(queued_lower) SUM(queued_raise) SUM(timed_launches) \
    SUM(timed_raise_launches) SUM(graphs_instantiated) SUM(region_replans) SUM(region_replans_done) SUM(resident_launches) \
    SUM(resident_kernel_ms) SUM(resident_stops) SUM(resident_tile_visits) SUM(region_launches) SUM(region_timed) SUM(region_kernel_ms) \
    SUM(region_tiles)
static void stats_merge(ufm_stats &a, const ufm_stats &c) {
#define UFM_STATS_SUM(f) a.f += c.f;
#define UFM_STATS_MAX(f) a.f = std::max(a.f, c.f);
    UFM_STATS_MERGE(UFM_STATS_SUM, UFM_STATS_MAX)
#undef UFM_STATS_SUM
#undef UFM_STATS_MAX
}

extern "C" {

int ufm_tile_edge(void) { return T; }
#ifdef UFM_STRICT_FENCES
const char *ufm_version(void) { return "ufm-gfx950 0.1 (block-FIM, strict-fence checking build)"; }
#elif defined(UFM_TIMING)
const char *ufm_version(void) { return "ufm-gfx950 0.1 (block-FIM, timing build)"; }
#elif defined(UFM_SWEEPSTAT)
const char *ufm_version(void) { return "ufm-gfx950 0.1 (block-FIM, sweep-statistics build)"; }
#else
const char *ufm_version(void) { return T == 32 ? "ufm-gfx950 0.1 (block-FIM, tile 32)" : "ufm-gfx950 0.1 (block-FIM, tile 16)"; }
#endif
int ufm_gaussian_taps(int ksize, uint16_t *taps) { return prep_gaussian_taps(ksize, taps) ? UFM_OK : UFM_ERR_INVALID; }

// ---- the handles ----
int ufm_batch_create_sharded(ufm_batch_t **out, int n_maps, int algo, int opt_lvl, int use_heuristic, const int *devices, int n_devices) {
    if (!out || !devices || n_devices < 1 || n_maps < n_devices) return UFM_ERR_INVALID;
    ufm_batch *b = new (std::nothrow) ufm_batch();
    if (!b) return UFM_ERR_NOMEM;
    const int rc = batch_fill(b, n_maps, algo, opt_lvl, use_heuristic, devices, n_devices);
    if (rc != UFM_OK) { ufm_batch_destroy(b); return rc; }
    *out = b;
    return UFM_OK;
}
int ufm_batch_create(ufm_batch_t **out, int n_maps, int algo, int opt_lvl, int use_heuristic, int device_id) {
    return ufm_batch_create_sharded(out, n_maps, algo, opt_lvl, use_heuristic, &device_id, 1);
}
int ufm_create(ufm_t **out, int algo, int opt_lvl, int use_heuristic, int device_id) {
    if (!out) return UFM_ERR_INVALID;
    ufm_planner *p = new (std::nothrow) ufm_planner();
    if (!p) return UFM_ERR_NOMEM;
    const int rc = batch_fill(p, 1, algo, opt_lvl, use_heuristic, &device_id, 1);
    if (rc != UFM_OK) { ufm_destroy(p); return rc; }
    *out = p;
    return UFM_OK;
}
int ufm_batch_destroy(ufm_batch_t *b) { if (!b) return UFM_ERR_INVALID; const int rc = batch_release(b); delete b; return rc; }
int ufm_destroy(ufm_t *p) { if (!p) return UFM_ERR_INVALID; const int rc = batch_release(p); delete p; return rc; }
int ufm_batch_size(const ufm_batch_t *b) { return b ? b->n_maps : UFM_ERR_INVALID; }
int ufm_batch_shards(const ufm_batch_t *b) { return b ? (int)b->shards.size() : UFM_ERR_INVALID; }
void *ufm_batch_stream(ufm_batch_t *b, int shard) { return (b && shard >= 0 && shard < (int)b->shards.size()) ? (void *)b->shards[shard]->stream : nullptr; }
void *ufm_stream(ufm_t *p) { return ufm_batch_stream(p, 0); }

// ---- settings of the whole handle: every shard ----
int ufm_batch_set_occupancy_threshold(ufm_batch_t *b, float thr) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->thr_uchar = (int)(thr * 255.0f);   // Graph.cpp:18-20
    return UFM_OK;
}
int ufm_set_occupancy_threshold(ufm_t *p, float thr) { return ufm_batch_set_occupancy_threshold(p, thr); }
int ufm_batch_set_heuristic_multiplier(ufm_batch_t *b, float mult) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->heuristic_multiplier = mult;
    return UFM_OK;
}
int ufm_set_heuristic_multiplier(ufm_t *p, float mult) { return ufm_batch_set_heuristic_multiplier(p, mult); }
int ufm_batch_heuristic_multiplier(ufm_batch_t *b, float *used) {
    if (!b || b->shards.empty() || !used) return UFM_ERR_INVALID;
    *used = b->shards[0]->last_multiplier;
    return UFM_OK;
}
int ufm_heuristic_multiplier(ufm_t *p, float *used) { return ufm_batch_heuristic_multiplier(p, used); }
int ufm_batch_set_param(ufm_batch_t *b, const char *name, double value) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_param(e, name, value); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_set_param(ufm_t *p, const char *name, double value) { return ufm_batch_set_param(p, name, value); }
int ufm_batch_set_profiling(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) e->profiling = enable != 0;
    return UFM_OK;
}
int ufm_set_profiling(ufm_t *p, int enable) { return ufm_batch_set_profiling(p, enable); }
int ufm_batch_track_costs(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_track_costs(e, enable); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_track_costs(ufm_t *p, int enable) { return ufm_batch_track_costs(p, enable); }
int ufm_batch_track_changes(ufm_batch_t *b, int enable) {
    if (!b) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_track_changes(e, enable); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_track_changes(ufm_t *p, int enable) { return ufm_batch_track_changes(p, enable); }
// footprint, sensor, layer count: all shards or none, so what one shard could refuse is checked on all of them first
int ufm_batch_set_cspace(ufm_batch_t *b, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_cspace(e, mask, mw, mh, anchor_row, anchor_col); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_set_cspace(ufm_t *p, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) { return ufm_batch_set_cspace(p, mask, mw, mh, anchor_row, anchor_col); }
// (include/ufm_cspace_graded.h)
int ufm_batch_set_cspace_graded(ufm_batch_t *b, const uint8_t *drop, int mw, int mh, int anchor_row, int anchor_col) {
    if (!b || b->shards.empty() || !cspace_graded_valid(drop, mw, mh, anchor_row, anchor_col)) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_cspace_graded(e, drop, mw, mh, anchor_row, anchor_col); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_set_cspace_graded(ufm_t *p, const uint8_t *drop, int mw, int mh, int anchor_row, int anchor_col) { return ufm_batch_set_cspace_graded(p, drop, mw, mh, anchor_row, anchor_col); }
int ufm_cspace_cone(int inner_d, int outer_d, int step, uint8_t *drop) { return cspace_cone(inner_d, outer_d, step, drop) ? UFM_OK : UFM_ERR_INVALID; }
int ufm_batch_set_sensor(ufm_batch_t *b, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) {
    if (!b || b->shards.empty() || !sensor_valid(mask, mw, mh, anchor_row, anchor_col)) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_sensor(e, mask, mw, mh, anchor_row, anchor_col); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_set_sensor(ufm_t *p, const uint8_t *mask, int mw, int mh, int anchor_row, int anchor_col) { return ufm_batch_set_sensor(p, mask, mw, mh, anchor_row, anchor_col); }
int ufm_batch_set_layers(ufm_batch_t *b, int n) {
    if (!b || b->shards.empty() || !layers_count_ok(n)) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    for (Engine *e : b->shards) { const int rc = engine_set_layers(e, n); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
int ufm_set_layers(ufm_t *p, int n) { return ufm_batch_set_layers(p, n); }

// ---- one map: the raster, its layers and surveys ----
int ufm_batch_set_map(ufm_batch_t *b, int i, const uint8_t *host_map, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_map(e, li, host_map, false, width, length); }
int ufm_set_map(ufm_t *p, const uint8_t *host_map, int width, int length) { return ufm_batch_set_map(p, 0, host_map, width, length); }
int ufm_batch_set_map_device(ufm_batch_t *b, int i, const uint8_t *dev_map, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_map(e, li, dev_map, true, width, length); }
int ufm_set_map_device(ufm_t *p, const uint8_t *dev_map, int width, int length) { return ufm_batch_set_map_device(p, 0, dev_map, width, length); }
int ufm_batch_patch_map(ufm_batch_t *b, int i, const uint8_t *host_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch(e, li, host_patch, false, x, y, w, h); }
int ufm_patch_map(ufm_t *p, const uint8_t *host_patch, int x, int y, int w, int h) { return ufm_batch_patch_map(p, 0, host_patch, x, y, w, h); }
int ufm_batch_patch_map_device(ufm_batch_t *b, int i, const uint8_t *dev_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch(e, li, dev_patch, true, x, y, w, h); }
int ufm_patch_map_device(ufm_t *p, const uint8_t *dev_patch, int x, int y, int w, int h) { return ufm_batch_patch_map_device(p, 0, dev_patch, x, y, w, h); }
int ufm_batch_set_image(ufm_batch_t *b, int i, const uint8_t *host_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    UFM_BATCH_MAP(b, i);
    return engine_set_image(e, li, host_image, false, width, length, taps, ntaps, penalty);
}
int ufm_set_image(ufm_t *p, const uint8_t *host_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    return ufm_batch_set_image(p, 0, host_image, width, length, taps, ntaps, penalty);
}
int ufm_batch_set_image_device(ufm_batch_t *b, int i, const uint8_t *dev_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    UFM_BATCH_MAP(b, i);
    return engine_set_image(e, li, dev_image, true, width, length, taps, ntaps, penalty);
}
int ufm_set_image_device(ufm_t *p, const uint8_t *dev_image, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    return ufm_batch_set_image_device(p, 0, dev_image, width, length, taps, ntaps, penalty);
}
int ufm_batch_read_map(ufm_batch_t *b, int i, uint8_t *host_map) { UFM_BATCH_MAP(b, i); return engine_read_map(e, li, host_map); }
int ufm_read_map(ufm_t *p, uint8_t *host_map) { return ufm_batch_read_map(p, 0, host_map); }
int ufm_batch_read_raw_map(ufm_batch_t *b, int i, uint8_t *host_map) { UFM_BATCH_MAP(b, i); return engine_read_raw_map(e, li, host_map); }
int ufm_read_raw_map(ufm_t *p, uint8_t *host_map) { return ufm_batch_read_raw_map(p, 0, host_map); }
int ufm_batch_read_cost_census(ufm_batch_t *b, int i, uint64_t hist[256], int *min_cost, int *max_cost) {      // i == -1: all maps, summed
    if (!b || b->shards.empty() || i < -1 || i >= b->n_maps) return UFM_ERR_INVALID;
    return i < 0 ? census_sum(b, 0, b->n_maps, hist, min_cost, max_cost) : census_sum(b, i, 1, hist, min_cost, max_cost);
}
int ufm_read_cost_census(ufm_t *p, uint64_t hist[256], int *min_cost, int *max_cost) { return ufm_batch_read_cost_census(p, 0, hist, min_cost, max_cost); }
int ufm_batch_set_survey(ufm_batch_t *b, int i, const uint8_t *host_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, 0, host_survey, false, width, length); }
int ufm_set_survey(ufm_t *p, const uint8_t *host_survey, int width, int length) { return ufm_batch_set_survey(p, 0, host_survey, width, length); }
int ufm_batch_set_survey_device(ufm_batch_t *b, int i, const uint8_t *dev_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, 0, dev_survey, true, width, length); }
int ufm_set_survey_device(ufm_t *p, const uint8_t *dev_survey, int width, int length) { return ufm_batch_set_survey_device(p, 0, dev_survey, width, length); }
int ufm_batch_read_survey(ufm_batch_t *b, int i, uint8_t *host_survey) { UFM_BATCH_MAP(b, i); return engine_read_layer_survey(e, li, 0, host_survey, false); }
int ufm_read_survey(ufm_t *p, uint8_t *host_survey) { return ufm_batch_read_survey(p, 0, host_survey); }
int ufm_batch_patch_layer(ufm_batch_t *b, int i, int k, const uint8_t *host_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch_layer(e, li, k, host_patch, false, x, y, w, h); }
int ufm_patch_layer(ufm_t *p, int k, const uint8_t *host_patch, int x, int y, int w, int h) { return ufm_batch_patch_layer(p, 0, k, host_patch, x, y, w, h); }
int ufm_batch_patch_layer_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_patch, int x, int y, int w, int h) { UFM_BATCH_MAP(b, i); return engine_patch_layer(e, li, k, dev_patch, true, x, y, w, h); }
int ufm_patch_layer_device(ufm_t *p, int k, const uint8_t *dev_patch, int x, int y, int w, int h) { return ufm_batch_patch_layer_device(p, 0, k, dev_patch, x, y, w, h); }
int ufm_batch_set_layer(ufm_batch_t *b, int i, int k, const uint8_t *host_raster, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer(e, li, k, host_raster, false, width, length); }
int ufm_set_layer(ufm_t *p, int k, const uint8_t *host_raster, int width, int length) { return ufm_batch_set_layer(p, 0, k, host_raster, width, length); }
int ufm_batch_set_layer_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_raster, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer(e, li, k, dev_raster, true, width, length); }
int ufm_set_layer_device(ufm_t *p, int k, const uint8_t *dev_raster, int width, int length) { return ufm_batch_set_layer_device(p, 0, k, dev_raster, width, length); }
int ufm_batch_set_layer_survey(ufm_batch_t *b, int i, int k, const uint8_t *host_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, k, host_survey, false, width, length); }
int ufm_set_layer_survey(ufm_t *p, int k, const uint8_t *host_survey, int width, int length) { return ufm_batch_set_layer_survey(p, 0, k, host_survey, width, length); }
int ufm_batch_set_layer_survey_device(ufm_batch_t *b, int i, int k, const uint8_t *dev_survey, int width, int length) { UFM_BATCH_MAP(b, i); return engine_set_layer_survey(e, li, k, dev_survey, true, width, length); }
int ufm_set_layer_survey_device(ufm_t *p, int k, const uint8_t *dev_survey, int width, int length) { return ufm_batch_set_layer_survey_device(p, 0, k, dev_survey, width, length); }
int ufm_batch_read_layer(ufm_batch_t *b, int i, int k, uint8_t *host_raster) { UFM_BATCH_MAP(b, i); return engine_read_layer(e, li, k, host_raster); }
int ufm_read_layer(ufm_t *p, int k, uint8_t *host_raster) { return ufm_batch_read_layer(p, 0, k, host_raster); }
int ufm_batch_read_layer_survey(ufm_batch_t *b, int i, int k, uint8_t *host_survey) { UFM_BATCH_MAP(b, i); return engine_read_layer_survey(e, li, k, host_survey); }
int ufm_read_layer_survey(ufm_t *p, int k, uint8_t *host_survey) { return ufm_batch_read_layer_survey(p, 0, k, host_survey); }
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
int ufm_reveal(ufm_t *p, int row, int col, uint64_t *changed) {
    const int32_t c[2] = {row, col};
    return row < 0 ? UFM_ERR_INVALID : ufm_batch_reveal(p, c, changed);        // (a single planner has no map to skip)
}

// ---- one map: start, goal, step, the field ----
int ufm_batch_reset(ufm_batch_t *b, int i) { UFM_BATCH_MAP(b, i); e->maps[li].initialize_search = true; return UFM_OK; }
int ufm_reset(ufm_t *p) { return ufm_batch_reset(p, 0); }
int ufm_batch_set_start(ufm_batch_t *b, int i, float x, float y) {
    UFM_BATCH_MAP(b, i);
    MapState &ms = e->maps[li];
    ms.start_x = x; ms.start_y = y; ms.new_start = true; ms.start_set = true;   // ReplannerBase.h:94-97
    return UFM_OK;
}
int ufm_set_start(ufm_t *p, float x, float y) { return ufm_batch_set_start(p, 0, x, y); }
int ufm_batch_set_goal(ufm_batch_t *b, int i, float x, float y) { UFM_BATCH_MAP(b, i); return engine_set_goal(e, li, x, y); }
int ufm_set_goal(ufm_t *p, float x, float y) { return ufm_batch_set_goal(p, 0, x, y); }
// One step of every map.  One shard -- every planner -- steps on the caller's thread, straight into the caller's statistics: nothing is
// allocated.  Shards on different devices advance side by side, one host thread each (a step is synchronous: its host thread spins on
// the device's published counters); their statistics are merged by the table above.
int ufm_batch_step(ufm_batch_t *b, ufm_stats *stats) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    const size_t n = b->shards.size();
    if (n == 1) {
        if (hipSetDevice(b->shards[0]->device) != hipSuccess) return UFM_ERR_HIP_BASE;
        return b->shards[0]->step(stats);
    }
    std::vector<ufm_stats> st(n);
    std::vector<int> rcs(n, UFM_OK);
    // "auto_multiplier": one multiplier for the whole batch, the smallest cost over all maps of all shards -- admissible for every map, and
    // the same however the maps are spread (a shard with a map still missing fails its step below)
    float auto_mult = 0.0f;
    const float *auto_ptr = nullptr;
    if (b->shards[0]->auto_multiplier && b->shards[0]->heur) {
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
    std::vector<std::thread> th;
    for (size_t s = 1; s < n; ++s) th.emplace_back(run, s);
    run(0);
    for (auto &t : th) t.join();
    for (size_t s = 0; s < n; ++s) if (rcs[s] != UFM_OK) return rcs[s];
    if (stats) {
        *stats = st[0];
        for (size_t s = 1; s < n; ++s) stats_merge(*stats, st[s]);
    }
    return UFM_OK;
}
int ufm_step(ufm_t *p, ufm_stats *stats) { return ufm_batch_step(p, stats); }
int ufm_batch_read_field(ufm_batch_t *b, int i, int x0, int y0, int nx, int ny, float *g, float *rhs) { UFM_BATCH_MAP(b, i); return engine_read_field(e, li, x0, y0, nx, ny, g, rhs); }
int ufm_read_field(ufm_t *p, int x0, int y0, int nx, int ny, float *g, float *rhs) { return ufm_batch_read_field(p, 0, x0, y0, nx, ny, g, rhs); }
int ufm_batch_read_changes(ufm_batch_t *b, int i, int cap, int32_t *xy, float *g, int32_t *info, int *total) { UFM_BATCH_MAP(b, i); return engine_read_changes(e, li, cap, xy, g, info, total); }
int ufm_read_changes(ufm_t *p, int cap, int32_t *xy, float *g, int32_t *info, int *total) { return ufm_batch_read_changes(p, 0, cap, xy, g, info, total); }
int ufm_batch_check_layout(ufm_batch_t *b, uint64_t *bad_ring, uint64_t *bad_cost) {      // summed over the shards
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
int ufm_check_layout(ufm_t *p, uint64_t *bad_ring, uint64_t *bad_cost) { return ufm_batch_check_layout(p, bad_ring, bad_cost); }
int ufm_batch_check_info(ufm_batch_t *b, uint64_t out[6]) {      // summed over the shards
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
int ufm_check_info(ufm_t *p, uint64_t out[6]) { return ufm_batch_check_info(p, out); }
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
int ufm_extract_path(ufm_t *p, int max_steps, int lookahead, int allow_indirect,
                     float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    return ufm_batch_extract_path(p, max_steps, lookahead, allow_indirect, path_xy, cap_points, step_costs, cap_costs, info);
}
// position queries: start k lies on map map_index[k]; a planner has one map and passes no indices
static int batch_paths_from(ufm_batch *b, int n_starts, const int32_t *map_index, const float *starts_xy, int max_steps, int lookahead,
                            int allow_indirect, float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    return paths_from(b->shards.data(), b->per, b->n_maps, n_starts, map_index, starts_xy, max_steps, lookahead, allow_indirect,
                      path_xy, cap_points, step_costs, cap_costs, info);
}
int ufm_batch_extract_paths_from(ufm_batch_t *b, int n_starts, const int32_t *map_index, const float *starts_xy, int max_steps, int lookahead,
                                 int allow_indirect, float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (!map_index) return UFM_ERR_INVALID;
    return batch_paths_from(b, n_starts, map_index, starts_xy, max_steps, lookahead, allow_indirect, path_xy, cap_points, step_costs, cap_costs, info);
}
int ufm_extract_paths_from(ufm_t *p, int n_starts, const float *starts_xy, int max_steps, int lookahead, int allow_indirect,
                           float *path_xy, int cap_points, float *step_costs, int cap_costs, ufm_path_info *info) {
    return batch_paths_from(p, n_starts, nullptr, starts_xy, max_steps, lookahead, allow_indirect, path_xy, cap_points, step_costs, cap_costs, info);
}
// trajectory scoring: path k lies on map map_index[k]; a planner has one map and passes no indices
static int batch_score_paths(ufm_batch *b, int n_paths, const int32_t *map_index, const int32_t *offsets, const float *points_xy, ufm_score *out) {
    if (!b || b->shards.empty()) return UFM_ERR_INVALID;
    return score_paths(b->shards.data(), b->per, b->n_maps, n_paths, map_index, offsets, points_xy, out);
}
int ufm_batch_score_paths(ufm_batch_t *b, int n_paths, const int32_t *map_index, const int32_t *offsets, const float *points_xy, ufm_score *out) {
    if (!map_index) return UFM_ERR_INVALID;
    return batch_score_paths(b, n_paths, map_index, offsets, points_xy, out);
}
int ufm_score_paths(ufm_t *p, int n_paths, const int32_t *offsets, const float *points_xy, ufm_score *out) {
    return batch_score_paths(p, n_paths, nullptr, offsets, points_xy, out);
}
int ufm_batch_score_paths_device(ufm_batch_t *b, int i, int n_paths, int total_points, const int32_t *dev_offsets, const float *dev_points_xy, ufm_score *dev_out) {
    UFM_BATCH_MAP(b, i);
    return engine_score_device(e, li, n_paths, total_points, dev_offsets, dev_points_xy, dev_out);
}
int ufm_score_paths_device(ufm_t *p, int n_paths, int total_points, const int32_t *dev_offsets, const float *dev_points_xy, ufm_score *dev_out) {
    return ufm_batch_score_paths_device(p, 0, n_paths, total_points, dev_offsets, dev_points_xy, dev_out);
}

// ---- a planner alone: shard 0, map 0 ----
#define UFM_PLANNER_ENGINE(p) if (!(p)) return UFM_ERR_INVALID; Engine *e = (p)->shards[0];
int ufm_field_dims(const ufm_t *p, int *nx, int *ny) {
    UFM_PLANNER_ENGINE(p);
    if (!e->allocated) return UFM_ERR_INVALID;
    if (nx) *nx = e->P.EX;
    if (ny) *ny = e->P.EY;
    return UFM_OK;
}
int ufm_read_info(ufm_t *p, int x0, int y0, int nx, int ny, int32_t *info) { UFM_PLANNER_ENGINE(p); return engine_read_info(e, 0, x0, y0, nx, ny, info, false); }
int ufm_read_info_derived(ufm_t *p, int x0, int y0, int nx, int ny, int32_t *info) { UFM_PLANNER_ENGINE(p); return engine_read_info(e, 0, x0, y0, nx, ny, info, true); }
int ufm_read_queue(ufm_t *p, int cap, int32_t *xy, float *g_rhs, int *total) { UFM_PLANNER_ENGINE(p); return engine_read_queue(e, 0, cap, xy, g_rhs, total); }
int ufm_debug_lmax(ufm_t *p, int32_t *out, int n) {      // diagnostics array of the device (not part of include/ufm.h)
    UFM_PLANNER_ENGINE(p);
    if (!e->allocated || n > LMAX) return UFM_ERR_INVALID;
    hipStreamSynchronize(e->stream);
    return hipMemcpy(out, e->P.lmax, sizeof(int) * n, hipMemcpyDeviceToHost) == hipSuccess ? UFM_OK : UFM_ERR_HIP_BASE;
}
// profiling: duration of the last layer kernel (k_layer_compose / k_layer_compose_all / k_reveal_layers), taken from the dispatch while
// ufm_set_profiling is on (tools/layers_probe.py; not part of include/ufm.h)
int ufm_debug_layers_ms(ufm_t *p, float *ms) {
    UFM_PLANNER_ENGINE(p);
    if (!ms || !e->lay_timed) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventElapsedTime(ms, e->lay_ev[0], e->lay_ev[1]));
    return UFM_OK;
}
// profiling: duration of the last scan kernel of ufm_read_changes (tools/delta_probe.py; not part of include/ufm.h)
int ufm_debug_delta_ms(ufm_t *p, float *ms) { UFM_PLANNER_ENGINE(p); if (!ms) return UFM_ERR_INVALID; *ms = e->trk_scan_ms; return UFM_OK; }
// profiling: duration of the last k_prepare of ufm_set_image / of map i's ufm_batch_set_image, taken from the dispatch while
// ufm_set_profiling is on (tools/prepare_probe.py; not part of include/ufm.h)
int ufm_debug_batch_prepare_ms(ufm_batch_t *b, int i, float *ms) { UFM_BATCH_MAP(b, i); if (!ms) return UFM_ERR_INVALID; *ms = e->prep_ms; return UFM_OK; }
int ufm_debug_prepare_ms(ufm_t *p, float *ms) { return ufm_debug_batch_prepare_ms(p, 0, ms); }

}  // extern "C"
