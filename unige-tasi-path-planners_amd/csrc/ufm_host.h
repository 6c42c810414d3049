// ufm_host.h -- the host side of planning: Engine (its members, allocation, launch chain, resident phase, replan submission,
// ReplannerBase::step), creation and destruction, the goal, field reads, path extraction, queue and back-pointer reads.  Keeping the
// raster -- patches, footprint, census, surveys and reveals, layers, images -- is ufm_map_host.h; the step code uses flush_deferred(),
// lazy, h_lazy and pending of it.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

// ---- host side -------------------------------------------------------------------
#define HIPCHK(expr)                                                      \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) return UFM_ERR_HIP_BASE - (int)_e;          \
    } while (0)

#include "ufm_route.h"
#include "ufm_patch_route.h"
#include "ufm_path.h"
#include "ufm_score.h"

static_assert(RJOBS <= ROUTE_MAX_JOBS && RTMAX >= 3, "ufm_route.h places at most ROUTE_MAX_JOBS blocks");
constexpr RouteConfig ROUTE_CONFIG{T, RTMAX, RJOBS, ROUTE_MAX_RECTS, 65 * 65};

// ---- which kernel forms exist ----------------------------------------------------
// The operator id as a compile-time constant, handed to a generic lambda.  Two selectors, because the instantiated forms differ: lowering,
// finalisation and the checks know FD, SG and MS-DFM; invalidation (k_relax<., MODE_RAISE, .>, k_replan_region) also MS-DFM along the stored bytes.
template <int V> using IntC = std::integral_constant<int, V>;
template <class F> void with_lower_op(int algo, F &&f) {
    if (algo == UFM_ALGO_FD) f(IntC<UFM_ALGO_FD>{});
    else if (algo == UFM_ALGO_SG) f(IntC<UFM_ALGO_SG>{});
    else f(IntC<ALGO_DFM1>{});
}
template <class F> void with_raise_op(int algo, bool follow_info, F &&f) {
    if (algo == UFM_ALGO_DFM && follow_info) f(IntC<ALGO_DFM1_INFO>{});
    else with_lower_op(algo, f);
}
template <class F> void with_elements(int algo, F &&f) {     // the patch kernels' <NODES>: FD / SG plan on nodes, MS-DFM on cells
    if (algo == UFM_ALGO_DFM) f(std::false_type{}); else f(std::true_type{});
}
// one launch; with both events given they are attached to the dispatch itself (start / stop time stamps of the kernel, what rocprofv3
// reports too), not recorded around it as separate packets
template <class... KA, class... A>
void launch(void (*k)(KA...), dim3 g, dim3 b, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const A &...a) {
    if (e0 && e1) hipExtLaunchKernelGGL(k, g, b, 0, s, e0, e1, 0, static_cast<KA>(a)...);
    else k<<<g, b, 0, s>>>(static_cast<KA>(a)...);
}

// ---- what the engine owns (ufm_resources.h), over HIP.  One error mapping for every allocation, event and wait of the owners: out of
// memory is UFM_ERR_NOMEM, anything else UFM_ERR_HIP_BASE - e, and the runtime's sticky error is cleared either way.
using ResStream = hipStream_t;
using ResEvent = hipEvent_t;
#include "ufm_resources.h"
static_assert(UFM_OK == 0, "the owners report success as 0");
int res_code(hipError_t e) {
    if (e == hipSuccess) return UFM_OK;
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? UFM_ERR_NOMEM : UFM_ERR_HIP_BASE - (int)e;
}
int res_dev_alloc(void **p, size_t bytes) { *p = nullptr; return res_code(hipMalloc(p, bytes ? bytes : 1)); }
void res_dev_free(void *p) { (void)hipFree(p); }
int res_pin_alloc(void **p, size_t bytes, Pin kind) {
    *p = nullptr;
    return res_code(hipHostMalloc(p, bytes, kind == Pin::Default ? hipHostMallocDefault : kind == Pin::Mapped ? hipHostMallocMapped : hipHostMallocMapped | hipHostMallocCoherent));
}
void res_pin_free(void *p) { (void)hipHostFree(p); }
int res_event_create(hipEvent_t *e) { *e = nullptr; return res_code(hipEventCreate(e)); }
void res_event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
int res_stream_sync(hipStream_t s) { return res_code(hipStreamSynchronize(s)); }
using ScratchBytes = GrowArray<uint8_t, 4096>;   // the map side's scratch: bytes, never fewer than 4096 once there are any
struct StreamOwner {                             // the engine's stream: its first member, so the last thing it gives back
    hipStream_t s = nullptr;
    StreamOwner() = default;
    StreamOwner(const StreamOwner &) = delete;
    ~StreamOwner() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

#include "ufm_knobs.h"

struct Engine : Knobs {     // the tuning members -- what ufm_set_param sets -- are Knobs' (ufm_knobs.h)
    StreamOwner stream;              // declared first, destroyed last: behind every buffer and event below
    ~Engine() {                      // the members give back what they own, in reverse order; first nothing may be running or hold their pointers
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        drop_graphs();
    }
    int algo = 0, opt_lvl = 0, heur = 0, device = 0, nmaps = 1;
    float heuristic_multiplier = 1.0f;
    int thr_uchar = 254;             // Graph.h:34
    DevDyn dyn_dev{-1.0f, -1, -1, 0};  // what *P.dyn holds (as far as the host knows)
    uint32_t graphs_made = 0;        // replan graphs instantiated so far (ufm_stats::graphs_instantiated)
    int W = 0, L = 0;
    DevParams P{};
    DevTable bufs;                   // owns what P's pointers and d_scratch point to (buffer_rows(), alloc(), release())
    bool allocated = false;
    Published<DevCounters> h_ctr;    // k_publish writes it, the host spins on h_ctr.flag(): the sequence number of the last published copy
    Published<DevCounters> h_pipe_ctr[2];   // run_phase keeps one batch of launches in flight ahead of the one whose
                                            // counters it is looking at: two more published copies, used alternately
    unsigned int pub_seq = 0;
    uint32_t owned_launches = 0;
    EventSet<2> own_ev;
    EventSet<2> reg_ev;              // profiling: around the block kernel of a replan
    bool own_timed = false;
    uint32_t region_runs = 0, region_done = 0;   // replans submitted to the block kernel / completed by it alone
    uint32_t region_cont = 0, region_cont_done = 0;   // ... continued by one blind submission of the launch chain / completed by that
    PinArray<ReplanJob> h_job;       // host-coherent pinned: per-replan inputs of the graph's first node
    struct GraphSig { DevParams P; float band, delta; int max_iters, grid, follow; };
    GraphSig graph_sig{};
    std::vector<std::pair<int, hipGraphExec_t>> graphs;   // key nr * 256 + nl
    void relax(int mode, bool dyn, dim3 g, int k_arg, float delta, float rbound, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
    float band_delta(float scale) const { return delta_abs >= 0.0f ? delta_abs : scale * T * mean_cost; }   // the ordering band
    void finalize_bp(int only_if_done) {   // the back-pointers of the tiles the step touched (k_finalize_bp); MS-DFM level 0 has none (its map has no Info)
        if (algo == UFM_ALGO_DFM && opt_lvl < 1) return;
        with_lower_op(algo, [&](auto a) { k_finalize_bp<a()><<<2048, 256, 0, stream>>>(P, only_if_done); });
    }
    int replan_graph(int nr, int nl, float band, hipGraphExec_t *out);
    void drop_graphs() { for (auto &g : graphs) hipGraphExecDestroy(g.second); graphs.clear(); }
    struct StepScratch {             // pinned: 2 accumulators + 12 * nmaps ints, one allocation carved once (engine_create)
        PinArray<unsigned long long> acc;      // [2]: engine_set_map's cost sum and count; it owns the whole allocation
        int *consume = nullptr, *init = nullptr, *init_tiles = nullptr;   // [nmaps] each: plan_step's answer per map; the goal tiles of the initialising maps, dense
        int *goals = nullptr;                  // [2 * nmaps]
        unsigned int *num_updated = nullptr;   // [nmaps]
        int *start_el = nullptr;               // [4 * nmaps]
        float *start_pos = nullptr;            // [2 * nmaps]
        int carve(int n) {
            { int rc = acc.alloc(2 + 6 * (size_t)n); if (rc != UFM_OK) return rc; }    // (12 ints are 6 of its elements)
            consume = reinterpret_cast<int *>(acc + 2); init = consume + n; init_tiles = init + n; goals = init_tiles + n;
            num_updated = reinterpret_cast<unsigned int *>(goals + 2 * n); start_el = goals + 3 * n;
            start_pos = reinterpret_cast<float *>(start_el + 4 * n);
            return UFM_OK;
        }
    } scratch;
    int *d_scratch = nullptr;
    GrowArray<float> d_field;        // ufm_read_field: the requested window, dense
    GrowArray<int32_t> d_info;       // ufm_read_info: back-pointers of the requested window
    GrowArray<PathJob> d_jobs;       // path extraction: the walks of one launch, with the pinned twin
    GrowArray<float> d_path;         // ... and the per-job output records, with the pinned twin
    struct ScoreStage {              // trajectory scoring, the host forms: one launch's paths and records, each with its pinned twin
        GrowArray<int32_t> idx;      // [cnt + 1] offsets into pts, then [cnt] map indices
        GrowArray<float> pts;        // the points of the launch's paths, dense
        GrowArray<ufm_score> out;    // [cnt]
    } score;
    std::vector<MapState> maps;
    std::vector<PatchRect> pending;
    int iter[2] = {0, 0};            // index k of the next relax launch of each queue (never reset: the queues persist)
    PinArray<float> h_bnd;           // pinned [nmaps]
    int last_active = 1;             // queue length at the last host check: long queues go through k_triage
    float mean_cost = 1.0f;
    bool profiling = false;
    EventSet<4> chain_ev;            // profiling: around the two blind batches of a replan's launch chain
    std::vector<EventSet<1>> batch_ev;    // ... and the sampled launches of run_phase's batches, batch_ev_slot events per batch in flight
    int batch_ev_slot = 64;
    hipEvent_t batch_event(int slot, int i) const { return batch_ev[(size_t)slot * batch_ev_slot + i][0]; }
    ufm_stats last{};

    std::vector<DevRow> buffer_rows();
    int alloc(int width, int length);
    void release();
    void launch_relax(int mode, float rbound, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
    int fetch_counters();
    int wait_published();
    int wait_flag(const unsigned int *flag, unsigned int seq);
    int win_raise[6] = {8, 8, 8, 8, 8, 8}, win_lower[6] = {8, 8, 8, 8, 8, 8}, win_pos = 0;   // launches recent replans needed
    int run_phase(int mode, float rbound, uint32_t *launches, float *kernel_ms, uint32_t *timed);
    int owned_phase();
    void own_layout(int ys) {            // the owner pattern: 16 x (1 << ys) tiles per block, one word per block and map for each owner
        P.own_ys = ys; P.own_nw = 16 << ys;
        P.own_sx = (P.TX + 15) / 16; P.own_sy = (P.TY + (1 << ys) - 1) >> ys;
        P.own_slots = nmaps * P.own_sx * P.own_sy;
    }
    size_t own_words() const {           // words of the queue array: enough for either pattern
        const size_t sx = (size_t)(P.TX + 15) / 16;
        return (size_t)nmaps * sx * std::max<size_t>(256 * (size_t)((P.TY + 15) / 16), 512 * (size_t)((P.TY + 31) / 32));
    }
    int reset_queues();
    int read_bounds(float *bmax);
    // a step (ReplannerBase::step) and its parts, in the order they run; StepRun is what they share
    struct StepRun {
        StepPlan plan;
        ufm_stats st;
        DevDyn dyn_now;
        bool dyn_pending;
        ReplanBegin rb;              // single map: the step bookkeeping and the consumed rectangles of the fused forms
        float band;                  // margin of the invalidation bound above the start's current key (the key may rise through the patch)
        int nr, nl;                  // blind batch sizes of a replan
        int n_init_tiles;
        uint64_t updated;
        bool fast_done, skip_raise;  // skip_raise: the block kernel has left nothing to invalidate below its bound (only lowering work beyond the block)
        std::chrono::steady_clock::time_point t0, t_seed;
        double u_acc, p_acc;
    };
    RouteSwitches route_switches() const {
        return RouteSwitches{fuse_control, spin_wait, use_region, use_graph, algo != UFM_ALGO_DFM, region_tiles, region_ahead, P.TX, P.TY, nmaps};
    }
    int step(ufm_stats *out, const float *auto_mult = nullptr);
    void flush_dyn(StepRun &r);
    int begin_step(StepRun &r);
    void start_elements();
    StepBegin step_begin_of(int m, int consume, int clear_lmax) const;
    int replan(StepRun &r);
    int submit_block(StepRun &r);
    int continue_block(StepRun &r);
    int submit_graph(StepRun &r);
    int submit_chain(StepRun &r);
    int fused_end(float band);
    int seed_only(StepRun &r);
    int converge(StepRun &r);
    void copy_counters(ufm_stats &st) const;

    // ---- the map side: keeping the raster (ufm_map_host.h has the functions).  Of all this the step code above uses flush_deferred(),
    // lazy, h_lazy and pending.  Every patch -- the caller's host or device bytes, a reveal's slot, a layer patch -- goes through
    // route_patch(), which acts on what plan_patch (ufm_patch_route.h) says: held, deferred or applied.
    PatchSwitches patch_switches(int m) const;
    PatchPlan patch_plan(PatchSource source, bool host_bytes, int k, const PatchRect &r) const;
    int patch_room(const PatchPlan &p);
    int route_patch(PatchSource source, bool host_bytes, int k, const uint8_t *bytes, const PatchRect &r);
    int stage_host_patch(const uint8_t *src, size_t n);
    ScratchBytes d_patch;            // staging for host patches, with its pinned twin
    ScratchBytes d_pmask;            // changed-cell mask of the patch being applied
    int ensure_pmask(size_t need);
    void patch_small(int m, const uint8_t *src, int x, int y, int w, int h) {
        with_elements(algo, [&](auto nodes) { k_patch_small<nodes()><<<1, 1024, 0, stream>>>(P, m, src, d_pmask.dev, x, y, w, h); });
    }
    // Deferred -- OPT-IN (ufm_batch_set_param "defer_patches", 1; round 4: it was the default, which silently extended the lifetime the ABI
    // asks of a patch buffer): small patches handed to a batch as device pointers are held back until something needs them applied (the
    // next step, a read of the raster, a path extraction) and applied by ONE launch -- the caller then keeps each buffer valid and unchanged
    // until that call has returned.  Off: every patch is applied at the call, stream-ordered, like a single planner's.
    struct DeferredPatch { int m, x, y, w, h; const uint8_t *ptr; };
    std::vector<DeferredPatch> deferred;
    int flush_deferred();            // everything that is being held or deferred, applied
    int flush_deferred_only();
    // Held -- a small patch of a SINGLE planner handed over from HOST memory (ufm_patch_map) is not uploaded and applied at the call: its
    // bytes are copied into a slot of host-coherent pinned memory (the caller's buffer is free again when the call returns, as before) and
    // the replan's block kernel reads them from there and does Graph::update + the seeding itself (RegionJob::psrc) -- no staging copy, no
    // stream synchronisation, no patch kernel in front of the replan.  Whatever else needs the raster first (a read of the map, a path
    // extraction, another kind of patch, a step that does not go through the block kernel) applies the held patches the ordinary way:
    // flush_lazy().
    static constexpr int LAZY_SLOTS = 4;                  // = the most rectangles a block-kernel job takes
    struct LazyPatch { int m, x, y, w, h, slot; };
    std::vector<LazyPatch> lazy;
    PinArray<uint8_t> h_lazy;        // LAZY_SLOTS x 4096 bytes, pinned + mapped
    int lazy_next = 0;               // slot after the last one handed out
    bool lazy_dirty[LAZY_SLOTS] = {false, false, false, false};   // a kernel queued on the stream may still read the slot
    int hold_host_patch(const PatchRect &r, const uint8_t *host_patch);
    int flush_lazy();
    // C-space inflation (ufm_set_cspace; ufm_cspace.h).  Off -- the default, and a 1 x 1 mask -- nothing below exists
    // or runs.  On: d_raw holds the caller's raster per map, P.cost its dilation by the footprint; a raw patch goes to d_raw, the rectangle
    // of P.cost it can change is dilated into d_cs_patch and that one is applied as an ordinary patch.
    CspaceMask cs;
    CspaceLevels csl;                // ufm_set_cspace_graded (ufm_cspace_graded.h, section 4.16): cs is then the support; n <= 1: a flat footprint
    DevArray<uint8_t> d_raw;        // [nmaps][L][W]; dropped with the rasters (release())
    ScratchBytes d_cs_patch;           // the dilated grown rectangle of the patch being applied, dense
    void cspace_dilate(int m, uint8_t *out, int pitch, const PatchRect &r);
    // Cost census (ufm_track_costs; ufm_census.h).  Off -- the default -- nothing below exists or runs.  On: d_census
    // holds, per map, how many cells of P.cost have each value, exactly, between any two calls: built after the raster is final
    // (engine_new_raster), corrected in front of every patch kernel.  After every build or patch the smallest and largest value present
    // are published to h_cen; "auto_multiplier" makes a step take that minimum as its heuristic multiplier.
    bool census_on = false;
    DevArray<uint32_t> d_census;     // [nmaps][256]
    struct CensusRange { int v[2]; };
    Published<CensusRange> h_cen;    // {min, max} over the engine's maps, and the sequence number of that copy
    unsigned int cen_seq = 0;
    float last_multiplier = 1.0f;    // what the last step used (ufm_heuristic_multiplier)
    void census_build(int m);
    void census_patch(int m, const uint8_t *dev_patch, int x, int y, int w, int h);
    void census_publish() { k_census_publish<<<1, CENSUS_BINS, 0, stream>>>(d_census, nmaps, h_cen->v, h_cen.flag(), ++cen_seq); }
    int census_minmax(int *mn, int *mx);
    void census_free() { d_census.reset(); h_cen.reset(); census_on = auto_multiplier = false; }
    // Sensor reveal (ufm_set_sensor / ufm_set_survey / ufm_reveal; ufm_sensor.h).  No sensor and no survey -- the
    // default -- nothing below exists or runs.  d_lsurvey[k] holds what the sensor would see of layer k, per map (one layer: k = 0, the
    // map); a reveal makes the dense patch Q of every map's field of view in ONE launch (k_reveal, k_reveal_layers with more than one
    // layer) into that map's slot of d_reveal and hands the slot to route_patch().  A deferred patch may point into d_reveal: reveal()
    // applies what is held before the kernel writes the slots again.
    SensorShape sensor;
    DevArray<uint8_t> d_sensor;      // the mask's bytes, room for SENSOR_MAX^2
    DevArray<uint8_t> d_lsurvey[LAYERS_MAX];     // [nmaps][L][W] each; dropped with the rasters (release())
    std::vector<uint8_t> have_lsurvey[LAYERS_MAX];   // [nmaps] each
    int survey_alloc(int k);
    ScratchBytes d_reveal;           // [nmaps] slots of sensor_slot_stride() bytes
    DevArray<unsigned int> d_reveal_cnt;     // [nmaps]: changed cells of the last reveal
    PinArray<int32_t> h_centres;     // [3 * nmaps], pinned + mapped: the centres as the reveal kernel reads them ([nmaps][2], with layers [nmaps][3])
    bool reveal_busy = false;        // a reveal kernel that is only queued may still read h_centres
    int reveal_check(const int32_t *centres) const;
    int reveal(const int32_t *centres);
    int reveal_counts(const int32_t *centres, uint64_t *changed);
    // Map preparation (ufm_set_image; ufm_prepare.h).  Never called -- the default -- nothing below exists.  k_prepare
    // must not read what it writes: a host bitmap, or a device bitmap that overlaps the rasters, goes through this buffer, which is the
    // engine's and reused by every map, not kept per map.
    ScratchBytes d_image;
    EventSet<2> prep_ev;             // profiling: on the k_prepare dispatch itself
    float prep_ms = 0.0f;            // ... its duration (tools/prepare_probe.py)
    // Cost layers (ufm_set_layers / ufm_patch_layer / ufm_set_layer; ufm_layers.h).  n_layers == 1 -- the default --
    // nothing below exists or runs.  With more, d_layers holds n rasters per map and the caller's raster (d_raw with a footprint, P.cost
    // without) is their element-wise maximum between any two calls: a layer patch is stored, composed over its rectangle into the dense
    // d_lcomp and that one goes on as the caller's device patch would.  A reveal uncovers every layer that has a survey.
    int n_layers = 1;
    DevArray<uint8_t> d_layers;      // [n_layers][nmaps] rasters at lstride bytes; dropped with the rasters (release())
    size_t lstride = 0;
    ScratchBytes d_lcomp;            // the dense composed patch of the layer call being applied
    EventSet<2> lay_ev;              // profiling: on the dispatch of the last layer kernel
    bool lay_timed = false;
    uint8_t *layer_ptr(int k, int m) const { return d_layers + layers_slot(k, m, nmaps, lstride); }
    int layer_surveys(int m) const {             // bit k: layer k of map m has a survey
        int have = 0;
        for (int k = 0; k < n_layers; ++k) if (d_lsurvey[k] && (size_t)m < have_lsurvey[k].size() && have_lsurvey[k][m]) have |= 1 << k;
        return have;
    }
    int layer_events(hipEvent_t *e0, hipEvent_t *e1);
    int compose_layer(int k, const uint8_t *dev_patch, const PatchRect &r);
    // step deltas (ufm_track_changes / ufm_read_changes, ufm_delta.h): nothing below exists unless a caller turned tracking on
    bool track = false;
    DevArray<float> trk_g;           // the baseline: the field as the caller was last told, in the layout of P.G (same gstride)
    DevArray<uint8_t> trk_key;       // ... and (level 1/2) the key of every element's Info pair (info_from_byte, ufm_path.h)
    GrowArray<uint8_t> trk_rec;      // record buffer of the scan (DeltaRecords): 256 bytes and 21 for each of ...
    size_t trk_cap() const { return trk_rec.cap ? (trk_rec.cap - 256) / 21 : 0; }   // ... this many records
    EventSet<2> trk_ev;
    float trk_scan_ms = 0.0f;        // profiling: duration of the last scan kernel
    int track_alloc();
    int track_reset(int m);
    int track_records(size_t cap) { return trk_rec.reserve(stream, 256 + (cap + 63) / 64 * 64 * 21); }   // at least `cap` records
    void track_free() {
        if (trk_g || trk_rec.dev) hipStreamSynchronize(stream);
        trk_g.reset(); trk_key.reset(); trk_rec.release();
    }
};

void Engine::release() {
    if (!allocated) return;
    if (stream) hipStreamSynchronize(stream);
    track_free();
    drop_graphs();                       // captured kernel arguments hold these pointers
    deferred.clear();
    std::memset(&graph_sig, 0, sizeof(graph_sig));
    bufs.release();
    d_raw.reset();
    d_layers.reset();                    // (the layers: rasters of these dimensions too)
    for (int k = 0; k < LAYERS_MAX; ++k) {   // (a survey belongs to rasters of these dimensions)
        d_lsurvey[k].reset();
        std::fill(have_lsurvey[k].begin(), have_lsurvey[k].end(), (uint8_t)0);
    }
    P = DevParams{};                     // every pointer null again: a failed alloc() can be released, and released twice
    allocated = false;
}

// Every array DevParams points to, and d_scratch: one row each -- the field, its bytes, its first contents.  alloc() allocates and
// fills from this table, release() frees what it got from it; the queue state (*: reset_queues()) is written there.
std::vector<DevRow> Engine::buffer_rows() {
    const size_t NT = (size_t)P.NT, n = (size_t)nmaps, gbytes = P.gstride * n * sizeof(float), I = sizeof(int);
    return {
        dev_row(P.G, gbytes, Fill::Inf),
        dev_row(P.Gprev, gbytes, Fill::Inf),
        dev_row(P.bp, P.gstride * n, Fill::BpNone),
        dev_row(P.ring, NT * RING * sizeof(float), Fill::Inf),
        dev_row(P.cost, P.cstride * n),
        dev_row(P.costT, NT * CTS),
        dev_row(P.goal, I * 2 * n, Fill::Ones),
        // (the lists: a slot that was never written must still read as a tile id -- an in-launch reader may look at a slot its writer has claimed
        //  but not yet stored, see the end check of k_replan_region)
        dev_row(P.cand, I * 6 * NT, Fill::Zero),
        dev_row(P.ready, I * NT, Fill::Zero),
        dev_row(P.hint, I * NT, Fill::Zero),
        dev_row(P.rank, I * NT, Fill::Zero),
        dev_row(P.park, I * 4 * NT, Fill::Zero),
        dev_row(P.pflag, I * 2 * NT),                                  // *
        dev_row(P.pprio, I * 2 * NT),                                  // *
        dev_row(P.queued, I * 4 * NT),                                 // *
        dev_row(P.prio, sizeof(unsigned long long) * 4 * NT),          // *
        dev_row(P.start, I * 4 * n, Fill::Ones),
        dev_row(P.bnd, sizeof(float) * n),
        dev_row(P.dyn, sizeof(DevDyn)),                                // (k_set_dyn, alloc())
        dev_row(P.spos, sizeof(float) * 2 * n, Fill::Zero),
        dev_row(P.touched, I * NT, Fill::Zero),
        dev_row(P.fresh, NT, Fill::Zero),
        dev_row(P.tlist, I * NT, Fill::Zero),
        dev_row(P.sflag, I * NT, Fill::Zero),
        dev_row(P.slist, I * NT, Fill::Zero),
        dev_row(P.slist2, I * NT, Fill::Zero),
        dev_row(P.mark, P.mstride * n, Fill::Zero),
        dev_row(P.num_updated, sizeof(unsigned int) * n, Fill::Zero),
        dev_row(P.consume, I * n),
        dev_row(P.lmax, I * LMAX),
        dev_row(P.own_prio, I * own_words()),                          // *
        dev_row(P.own_lock, I * own_words()),                          // *
        dev_row(P.own_min, I * OWN_NW),                                // *
        dev_row(P.ctr, sizeof(DevCounters), Fill::Zero),               // (and *: its head)
        dev_row(d_scratch, I * (4 * n + 16)),
    };
}

int Engine::alloc(int width, int length) {
    release();
    W = width; L = length;
    const bool nodes = algo != UFM_ALGO_DFM;
    P.W = W; P.L = L;
    P.EX = nodes ? L + 1 : L;
    P.EY = nodes ? W + 1 : W;
    P.TX = (P.EX + T - 1) / T;
    P.TY = (P.EY + T - 1) / T;
    // tile ids are ints; the element count of a map must fit one as well (start elements, marks)
    if ((long long)P.TX * P.TY * nmaps > (long long)INT32_MAX / 4 || (long long)P.EX * P.EY > INT32_MAX) return UFM_ERR_NOMEM;
    P.NTm = P.TX * P.TY;
    P.nmaps = nmaps;
    P.NT = P.NTm * nmaps;
    P.cells = nodes ? 0 : 1;
    P.gstride = (size_t)P.NTm * TT;
    P.cstride = (size_t)L * W;
    P.mstride = (size_t)P.EX * P.EY;
    own_layout(4);
    allocated = true;                    // from here on release() has something to free, also after a failure half way
    const std::vector<DevRow> rows = buffer_rows();
    const int rc = [&]() -> int {
        { int ra = bufs.alloc(rows); if (ra != UFM_OK) return ra; }
        if (cs.on) { int ra = d_raw.alloc(P.cstride * nmaps); if (ra != UFM_OK) return ra; }
        if (n_layers > 1) {
            lstride = layers_stride(P.cstride);
            { int ra = d_layers.alloc(lstride * nmaps * n_layers); if (ra != UFM_OK) return ra; }
            HIPCHK(hipMemsetAsync(d_layers, 0, lstride * nmaps * n_layers, stream));
        }
        for (const DevRow &r : rows) {
            if (r.fill == Fill::Inf) k_fill<<<1024, 256, 0, stream>>>(static_cast<float *>(*r.field), r.bytes / sizeof(float), INFINITY);
            else if (r.fill != Fill::None) HIPCHK(hipMemsetAsync(*r.field, r.fill == Fill::Zero ? 0 : (r.fill == Fill::Ones ? 0xFF : BP_NONE), r.bytes, stream));
        }
        { int rq = reset_queues(); if (rq != UFM_OK) return rq; }     // (behind the table's fills: it writes into the zeroed counter block)
        dyn_dev = DevDyn{heur ? heuristic_multiplier : 0.0f, thr_uchar, focused ? 1 : 0, 0};
        k_set_dyn<<<1, 1, 0, stream>>>(P.dyn, dyn_dev);
        HIPCHK(hipGetLastError());
        return track ? track_alloc() : UFM_OK;
    }();
    if (rc != UFM_OK) { release(); return rc; }
    pending.clear();
    for (auto &ms : maps) { ms.have_map = false; ms.initialize_search = true; }
    return UFM_OK;
}

// drop every queued tile (full re-initialisation: nothing of the old search survives)
int Engine::reset_queues() {
    HIPCHK(hipMemsetAsync(P.queued, 0, sizeof(int) * 4 * P.NT, stream));
    HIPCHK(hipMemsetAsync(P.prio, 0xFF, sizeof(unsigned long long) * 4 * P.NT, stream));   // tag of no launch, larger than any key
    HIPCHK(hipMemsetAsync(P.pflag, 0, sizeof(int) * 2 * P.NT, stream));
    k_fill<<<64, 256, 0, stream>>>(reinterpret_cast<float *>(P.pprio), (size_t)2 * P.NT, INFINITY);
    k_fill<<<64, 256, 0, stream>>>(reinterpret_cast<float *>(P.own_prio), own_words(), INFINITY);   // (+inf = INFBITS: empty)
    HIPCHK(hipMemsetAsync(P.own_lock, 0, sizeof(int) * own_words(), stream));
    k_fill<<<2, 256, 0, stream>>>(reinterpret_cast<float *>(P.own_min), (size_t)OWN_NW, INFINITY);
    // the queue state at the head of DevCounters: cnt, rel, lmin, npark, nready, rcursor, nshort, last_work, fin_blocks
    static_assert(offsetof(DevCounters, cnt) == 0, "queue state leads the counter block");
    HIPCHK(hipMemsetAsync(P.ctr, 0, offsetof(DevCounters, kbase), stream));
    k_fill<<<1, 64, 0, stream>>>(reinterpret_cast<float *>(&P.ctr->lmin[0][0]), (size_t)6, INFINITY);
    last_active = 1;
    iter[0] = iter[1] = 0;
    return UFM_OK;
}
// largest start key over the maps (+inf if some map's start is not reached yet)
int Engine::read_bounds(float *bmax) {
    k_start_bound<<<(nmaps + 63) / 64, 64, 0, stream>>>(P);
    HIPCHK(hipMemcpyAsync(h_bnd, P.bnd, sizeof(float) * nmaps, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float b = 0.0f;
    for (int m = 0; m < nmaps; ++m) b = std::fmax(b, h_bnd[m]);
    *bmax = b;
    return UFM_OK;
}

// Counters to the host.  A D2H copy + hipStreamSynchronize costs ~40 us of wake-up latency per
// host round trip (measured: copy done at 289 us, host running again at 327 us); a replan has one
// round trip, a plan one per batch of launches.  Instead the last kernel of a submission writes
// the counters into host-coherent pinned memory, fences, and bumps a sequence number the host
// spins on (the reference's driver owns its core anyway, main.cpp:36-47).
__global__ void k_publish(const DevCounters *src, DevCounters *dst, unsigned int *flag, unsigned int seq) {
    const int *s = reinterpret_cast<const int *>(src);
    int *d = reinterpret_cast<int *>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(DevCounters) / sizeof(int)); i += blockDim.x) d[i] = s[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int Engine::fetch_counters() {
    if (!spin_wait) {
        HIPCHK(hipMemcpyAsync(h_ctr, P.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return UFM_OK;
    }
    ++pub_seq;
    k_publish<<<1, 64, 0, stream>>>(P.ctr, h_ctr, h_ctr.flag(), pub_seq);
    HIPCHK(hipGetLastError());
    return wait_published();
}
// spin until the device has published copy number pub_seq
int Engine::wait_published() { return wait_flag(h_ctr.flag(), pub_seq); }
int Engine::wait_flag(const unsigned int *flag, unsigned int seq) {
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::milliseconds(200);
    for (unsigned int spins = 1;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return UFM_OK;
        __builtin_ia32_pause();
        if ((spins & 0xFFF) != 0) continue;
        // a faulted kernel never publishes: every 200 ms ask the runtime whether the stream is still alive
        const auto now = std::chrono::steady_clock::now();
        if (now < next_query) continue;
        next_query = now + std::chrono::milliseconds(200);
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return UFM_ERR_HIP_BASE - (int)q;
        break;                          // the stream has drained: the flag is there by now, or it never will be
    }
    return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq ? UFM_OK : UFM_ERR_HIP_BASE;
}

// one relax launch: the operator by the planner, the mode, and whether the queue was triaged by k_triage (dyn) or is triaged in the launch (fused)
void Engine::relax(int mode, bool dyn, dim3 g, int k_arg, float delta, float rbound, hipEvent_t e0, hipEvent_t e1) {
    auto go = [&](auto a, auto m) {
        if (dyn) launch(k_relax<a(), m(), true>, g, dim3(NTHR), stream, e0, e1, P, k_arg, delta, rbound, max_iters);
        else launch(k_relax<a(), m(), false>, g, dim3(NTHR), stream, e0, e1, P, k_arg, delta, rbound, max_iters);
    };
    if (mode == MODE_LOWER) with_lower_op(algo, [&](auto a) { go(a, IntC<MODE_LOWER>{}); });
    else with_raise_op(algo, dfm_follow_info, [&](auto a) { go(a, IntC<MODE_RAISE>{}); });
}
// The whole replan submission -- begin, nr invalidation launches, transition, nl lowering
// launches, end -- captured once per (nr, nl) and replayed: the host enqueues one graph instead of
// ~20 kernels (2.9 us of host time each, measured; the kernels of a replan are that short).  The
// graph is static: launch indices are offsets to a base the first node takes, with the rest of
// the per-replan inputs, from host-coherent memory (h_job).
int Engine::replan_graph(int nr, int nl, float band, hipGraphExec_t *out) {
    GraphSig sig{};
    sig.P = P; sig.band = band; sig.delta = band_delta(delta_scale);
    sig.max_iters = max_iters; sig.grid = grid_relax * 4096 + tail_grid; sig.follow = dfm_follow_info ? 1 : 0;
    if (std::memcmp(&sig, &graph_sig, sizeof(GraphSig)) != 0) { drop_graphs(); std::memcpy(&graph_sig, &sig, sizeof(GraphSig)); }
    const int key = nr * 256 + nl;
    for (auto &g : graphs) if (g.first == key) { *out = g.second; return UFM_OK; }
    if (graphs.size() >= 64) drop_graphs();
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    k_replan_begin_job<<<1, 1024, 0, stream>>>(P, h_job);
    // a phase starts with its largest launches; what is left after a few of them fits a small
    // grid, which starts -- and, when the queue has run dry, ends -- sooner (an empty 512-workgroup
    // launch lasts 4.6 us)
    auto grid_of = [&](int i) { return i < 2 ? grid_relax : (i < 4 ? std::max(tail_grid, grid_relax / 2) : tail_grid); };
    for (int i = 0; i < nr; ++i) relax(MODE_RAISE, false, dim3(std::min(grid_relax, grid_of(i))), -1 - i, INFINITY, -1.0f);
    k_raise_to_lower<<<1, 1024, 0, stream>>>(P, -1);
    for (int i = 0; i < nl; ++i) relax(MODE_LOWER, false, dim3(std::min(grid_relax, grid_of(i))), -1 - i, band_delta(delta_scale), INFINITY);
    k_replan_end<<<64, T * T, 0, stream>>>(P, -1 - nr, -1 - nl, band, h_ctr, h_ctr.flag(), 0u);
    finalize_bp(1);     // (behind the publication: the host does not wait for it, the next step's kernels do)
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamEndCapture(stream, &g));
    hipGraphExec_t ge = nullptr;
    const hipError_t err = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    HIPCHK(err);
    graphs.emplace_back(key, ge);
    ++graphs_made;
    *out = ge;
    return UFM_OK;
}

// the next launch of a queue; e0 / e1 (profiling): events attached to the relax kernel's dispatch
void Engine::launch_relax(int mode, float rbound, hipEvent_t e0, hipEvent_t e1) {
    dim3 g(grid_relax);
    const int q = (mode == MODE_LOWER) ? Q_LOWER : Q_RAISE;
    // long queue: vectorised triage + balanced hand-out of the released tiles; short queue: fused
    const bool dyn = dynamic_mode && last_active > grid_relax / 4;
    // invalidation is order-free; lowering releases tiles in bands of `delta`
    const float delta = (mode == MODE_RAISE) ? INFINITY : band_delta(dyn ? delta_scale_long : delta_scale);
    // a short queue (replans: a handful of tiles per launch) does not need the whole chip: a small
    // grid starts, and when there is nothing left to do ends, sooner
    if (!dyn && last_active <= small_grid / 2 && small_grid < grid_relax) g = dim3(small_grid);
    if (dyn) g = dim3(std::min(grid_relax, dyn_grid));   // one resident workgroup per CU
    if (dyn) {
        if (mode == MODE_LOWER) k_triage<MODE_LOWER><<<64, 256, 0, stream>>>(P, iter[q], delta, rbound);
        else k_triage<MODE_RAISE><<<64, 256, 0, stream>>>(P, iter[q], delta, rbound);
    }
    relax(mode, dyn, g, iter[q], delta, rbound, e0, e1);
    ++iter[q];
}

// A whole lowering phase in one launch: the resident kernel (k_relax<., LOWER, false, 1 | 2>) between the two kernels that
// move the queue into and out of its per-owner words.  What it leaves behind is an ordinary (short or empty) list
// for launch iter + 1, which run_phase() then finds.
int Engine::owned_phase() {
    const int k = iter[Q_LOWER];
    // the ordering band in tile crossings.  Round 2: 4 (a workgroup that finds nothing inside the band idles, so wider paid).  With the idle
    // workgroups' looks made cheap (round 3) the optimum moved down -- 4096^2 FD 14.7 / 14.2 / 14.2 / 14.2 / 14.6 ms for 1.5 / 2 / 2.5 / 3 / 4 with 230 k ... 350 k
    // visits, 8192^2 36.7 / 35.8 / 35.5 / 36.0 / 37.4, SG 2048^2 5.85 / 5.4 / 5.3 / 5.4 / 5.7; MS-DFM 2048^2 12.0 / 11.8 / 11.4 / 11.7 (2 ... 4); the 8-map
    // MS-DFM batch, bound by the number of visits: 34.0 / 34.3 / 34.9 / 35.8 (2 ... 4)
    const float band_auto = nmaps > 1 ? 2.0f : (algo == UFM_ALGO_DFM ? 3.0f : 2.5f);
    const float delta = band_delta(owned_band >= 0.0f ? owned_band : band_auto);
    const double limit_ms = owned_limit_ms >= 0.0f ? (double)owned_limit_ms : 200.0 + (double)P.NT / 250.0;   // (4096^2: 0.46 s; its plan takes 17 ms)
    P.own_limit = (unsigned long long)(limit_ms * 1e5);   // 100 MHz ticks
    P.own_flags = owned_flags;
    // (measured with the helping workgroups in place: FD 4096^2 15.9-16.3 ms with 8 waves against 16.5-16.8 with 16, 2048^2 7.25 against 6.44,
    //  SG 2048^2 7.08 against 6.55, 1024^2 3.40 against 2.84; MS-DFM, whose visits are longer and which has no early hand-off, 2048^2 13.1 against 15.0)
    const bool half = T == 16 && (owned_waves == 8 || (owned_waves == 0 && (nmaps > 1 || P.NTm > (algo == UFM_ALGO_DFM ? 12000 : 50000))));
    own_layout(half ? 5 : 4);
    k_own_import<<<64, 256, 0, stream>>>(P, k);
    // 16 waves per tile visit, one visit per CU -- or 8 and two: a visit is then ~17 % longer and a CU makes 1.7 x as many.  That pays
    // where there are always more tiles to visit than workgroups (several maps, or a front as long as that of an 8192^2 map); a single
    // 4096^2 plan is bound by the chain of dependent visits along the front's way, not by their number
    const dim3 g(P.own_nw), b(half ? NTHR / 2 : NTHR);
    own_timed = false;
    if (profiling) {
        { int rc = own_ev.ensure(); if (rc != UFM_OK) return rc; }
        own_timed = true;
    }
    hipEvent_t e0 = own_timed ? own_ev[0] : nullptr, e1 = own_timed ? own_ev[1] : nullptr;
    with_lower_op(algo, [&](auto a) {
#if UFM_TILE == 16
        if (half) launch(k_relax<a(), MODE_LOWER, false, 2>, g, b, stream, e0, e1, P, k, delta, INFINITY, max_iters);
        else
#endif      // (32 x 32 tiles: the 16-wave form only -- the skewed 8-wave patch map is written for 4 x 4 patches per tile)
        launch(k_relax<a(), MODE_LOWER, false, 1>, g, b, stream, e0, e1, P, k, delta, INFINITY, max_iters);
    });
    k_own_export<<<256, 256, 0, stream>>>(P, k + 1);
    HIPCHK(hipGetLastError());
    ++iter[Q_LOWER];
    last_active = 1;
    ++owned_launches;
    return UFM_OK;
}

// Launch relax kernels until the active list runs dry.  The list lengths live on
// the device; the host peeks at them once per batch of launches (an empty launch
// costs a few microseconds, a host round trip more).
// A phase also ends when a launch released nothing: everything still queued lies beyond the bound
// (the start's key) and stays queued for a later step.
// The host does not wait for a batch before it submits the next one: while it reads the counters batch
// b published, batch b+1 is already running (a host round trip -- publish, PCIe, decision, first
// dispatch -- left the GPU idle for ~15 us, 68 times per 4096^2 plan).  The price: when batch b turns
// out to have drained the queue, batch b+1 consists of launches that find nothing to do (a few us each).
int Engine::run_phase(int mode, float rbound, uint32_t *launches, float *kernel_ms, uint32_t *timed) {
    const int q = (mode == MODE_LOWER) ? Q_LOWER : Q_RAISE;
    const long cap = 64L * (P.TX + P.TY) * T + 4096;   // generous bound on sweeps
    // pipelined: batch b + 1 is submitted before the counters batch b published are looked at; otherwise the host waits for every batch
    const bool pipelined = spin_wait && pipeline_batches && h_pipe_ctr[0];
    batch_ev_slot = 2 * std::max(32, batch_fixed);     // events per batch: two per launch (adaptive batches: <= 32 launches)
    while (profiling && batch_ev.size() < (size_t)((pipelined ? 2 : 1) * batch_ev_slot)) { EventSet<1> a; int rc = a.ensure(); if (rc != UFM_OK) return rc; batch_ev.push_back(std::move(a)); }
    struct Batch { unsigned int seq; int slot, ns, iter_after; };
    auto counters = [&](const Batch &b) -> const DevCounters * { return pipelined ? h_pipe_ctr[b.slot] : h_ctr; };
    long total = 0;
    auto submit = [&](int n, int slot, Batch *b) -> int {     // one batch with its sampled events (the event packets cost ~4 us each)
        int ns = 0;
        for (int k = 0; k < n; ++k) {
            const bool timed_k = profiling && ((total + k) % profile_stride == 0);
            launch_relax(mode, rbound, timed_k ? batch_event(slot, 2 * ns) : nullptr, timed_k ? batch_event(slot, 2 * ns + 1) : nullptr);
            if (timed_k) ++ns;
        }
        if (pipelined) k_publish<<<1, 64, 0, stream>>>(P.ctr, h_pipe_ctr[slot], h_pipe_ctr[slot].flag(), ++pub_seq);
        HIPCHK(hipGetLastError());
        *b = {pub_seq, slot, ns, iter[q]};
        *launches += (uint32_t)n;
        total += n;
        return UFM_OK;
    };
    auto collect = [&](const Batch &b) -> int {               // wait for the batch's counters, add its timed launches
        int rc = pipelined ? wait_flag(h_pipe_ctr[b.slot].flag(), b.seq) : fetch_counters();
        if (rc != UFM_OK) return rc;
        for (int k = 0; k < b.ns; ++k) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, batch_event(b.slot, 2 * k), batch_event(b.slot, 2 * k + 1)));
            *kernel_ms += ms;
        }
        *timed += (uint32_t)b.ns;
        return UFM_OK;
    };
    Batch prev{}, cur{};
    int batch = batch_fixed > 0 ? batch_fixed : 4;
    for (bool first = true;; first = false) {
        { int rc = submit(batch, pipelined ? (prev.slot ^ (first ? 0 : 1)) : 0, &cur); if (rc != UFM_OK) return rc; }
        if (pipelined && first) { prev = cur; continue; }
        const Batch &look = pipelined ? prev : cur;           // the batch whose counters decide
        { int rc = collect(look); if (rc != UFM_OK) return rc; }
        const int active = counters(look)->cnt[q][look.iter_after % 3];
        const bool done = active == 0 || counters(look)->rel[q][(look.iter_after + 2) % 3] == 0;   // drained / nothing released: the rest lies beyond the bound
        last_active = active;
        if (done || total > cap) {
            if (pipelined) {                                  // the batch submitted meanwhile found nothing to do
                int rc = collect(cur);
                if (rc != UFM_OK) return rc;
                last_active = counters(cur)->cnt[q][cur.iter_after % 3];
            }
            return done ? UFM_OK : UFM_ERR_NOT_CONVERGED;
        }
        batch = batch_fixed > 0 ? batch_fixed : (active > 512 ? 32 : (active > 256 ? 16 : (active > 32 ? 8 : 4)));
        prev = cur;
    }
}

// ---- a step: ReplannerBase::step (ReplannerBase.h:43-75) --------------------------------------------------------------------
// plan_step (ufm_route.h) says what the step is and which route a replan takes; the parts below act on that, in the order they are written.

// heuristic multiplier / threshold / focused flag live in device memory (DevDyn); a changed value reaches the
// device with the first kernel of the step: through the job record of the block kernel or of the graph, or here by k_set_dyn
void Engine::flush_dyn(StepRun &r) {
    if (!r.dyn_pending) return;
    k_set_dyn<<<1, 1, 0, stream>>>(P.dyn, r.dyn_now);
    dyn_dev = r.dyn_now; r.dyn_pending = false;
}

// start elements: the 4 corners of the start cell (FD impl:9-13, Cell.cpp:48-60) / the start cell (DFM)
void Engine::start_elements() {
    for (int m = 0; m < nmaps; ++m) {
        const MapState &ms = maps[m];
        int *st_el = scratch.start_el + 4 * m;
        float *sp = scratch.start_pos + 2 * m;
        for (int i = 0; i < 4; ++i) st_el[i] = -1;
        sp[0] = sp[1] = 0.0f;
        if (!ms.start_set) continue;
        const int cx = (int)(start_cell_floor ? std::floor(ms.start_x) : std::roundf(ms.start_x)), cy = (int)(start_cell_floor ? std::floor(ms.start_y) : std::roundf(ms.start_y));
        // keys measure from start_pos_ (FD/SG, Position::distance) or from start_cell_ (DFM, Cell::distance)
        sp[0] = (algo == UFM_ALGO_DFM) ? (float)cx : ms.start_x;
        sp[1] = (algo == UFM_ALGO_DFM) ? (float)cy : ms.start_y;
        const int ncorner = (algo == UFM_ALGO_DFM) ? 1 : 4;
        for (int i = 0; i < ncorner; ++i) {
            const int ex = cx + (i & 1), ey = cy + (i >> 1);
            if (ex >= 0 && ey >= 0 && ex < P.EX && ey < P.EY) st_el[i] = ex * P.EY + ey;
        }
    }
}
StepBegin Engine::step_begin_of(int m, int consume, int clear_lmax) const {
    StepBegin sb{};
    for (int i = 0; i < 4; ++i) sb.start[i] = scratch.start_el[4 * m + i];
    sb.consume = consume; sb.clear_lmax = clear_lmax;
    sb.sx = scratch.start_pos[2 * m]; sb.sy = scratch.start_pos[2 * m + 1];
    return sb;
}

// Everything in front of the step's submission: the held patches, the batch's counters, the initialising maps' fills and goals, the
// start elements, and the consumed rectangles -- their marks cleared, or handed to the fused forms in r.rb
int Engine::begin_step(StepRun &r) {
    const StepPlan &pl = r.plan;
    const bool single = (nmaps == 1);
    // held host patches: the replan's block kernel applies them itself if this step goes that way; otherwise now, the ordinary way
    if (!pl.held_in_kernel) { int rc = flush_deferred(); if (rc != UFM_OK) return rc; }   // (and a batch's deferred device patches: one launch)
    if (!single) {
        HIPCHK(hipMemsetAsync(&P.ctr->tcount, 0, sizeof(int), stream));
        HIPCHK(hipMemsetAsync(&P.ctr->expanded, 0, 4 * sizeof(unsigned long long), stream));
        HIPCHK(hipMemsetAsync(&P.ctr->raise_visits, 0, sizeof(unsigned long long), stream));
        if (profiling) HIPCHK(hipMemsetAsync(P.lmax, 0, sizeof(int) * LMAX, stream));
    }
    // a full re-initialisation drops whatever the old search left queued
    if (pl.n_init == nmaps) { int rc = reset_queues(); if (rc != UFM_OK) return rc; }
    for (int m = 0; m < nmaps; ++m) {
        MapState &ms = maps[m];
        if (!scratch.init[m]) { if (scratch.consume[m]) ms.new_start = false; continue; }
        scratch.goals[2 * m] = ms.goal_elem_valid ? ms.goal_ex : -1;
        scratch.goals[2 * m + 1] = ms.goal_elem_valid ? ms.goal_ey : -1;
        k_fill<<<1024, 256, 0, stream>>>(P.G + (size_t)m * P.gstride, P.gstride, INFINITY);
        HIPCHK(hipMemsetAsync(P.bp + (size_t)m * P.gstride, BP_NONE, P.gstride, stream));
        k_fill<<<256, 256, 0, stream>>>(P.ring + (size_t)m * P.NTm * RING, (size_t)P.NTm * RING, INFINITY);
        // (a goal outside the map: nothing reachable, the field stays +inf -- the map initialises, the list does not get a tile)
        if (ms.goal_elem_valid) scratch.init_tiles[r.n_init_tiles++] = m * P.NTm + (ms.goal_ex / T) * P.TY + (ms.goal_ey / T);
    }
    // (goal array upload is per map to keep untouched maps' goals)
    for (int m = 0; m < nmaps; ++m)
        if (scratch.init[m]) HIPCHK(hipMemcpyAsync(P.goal + 2 * m, scratch.goals + 2 * m, 2 * sizeof(int), hipMemcpyHostToDevice, stream));
    start_elements();
    if (single) {
        r.rb.sb = step_begin_of(0, scratch.consume[0], profiling ? 1 : 0);
        if (!pl.fused) k_step_begin<<<1, 256, 0, stream>>>(P, r.rb.sb);
    } else {
        HIPCHK(hipMemcpyAsync(P.start, scratch.start_el, sizeof(int) * 4 * nmaps, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(P.spos, scratch.start_pos, sizeof(float) * 2 * nmaps, hipMemcpyHostToDevice, stream));
    }
    if (pl.n_upd > 0 || pl.n_init > 0) {
        if (!single) HIPCHK(hipMemcpyAsync(P.consume, scratch.consume, sizeof(int) * nmaps, hipMemcpyHostToDevice, stream));
        // consume the pending patch rectangles of the participating maps, keep the others
        size_t kept = 0;
        for (const PatchRect &p : pending) {
            if (!scratch.consume[p.m]) { pending[kept++] = p; continue; }
            const int cnt = (p.h + 1) * (p.w + 1);
            if (pl.fused) put_rect(r.rb.rect[r.rb.nrect++], p);
            else k_clear_marks<<<(cnt + 255) / 256, 256, 0, stream>>>(P, p.m, p.x, p.y, p.w, p.h);
        }
        pending.resize(kept);
    }
    return UFM_OK;
}

// the device-side end check of a fused submission (k_replan_end publishes the counters), the back-pointers behind it
int Engine::fused_end(float band) {
    ++pub_seq;
    k_replan_end<<<64, T * T, 0, stream>>>(P, iter[Q_RAISE], iter[Q_LOWER], band, h_ctr, h_ctr.flag(), pub_seq);
    finalize_bp(1);     // (behind the publication: the host does not wait for it, the next step's kernels do)
    HIPCHK(hipGetLastError());
    return wait_published();
}

// Route::BlockSingle / BlockBatch: one workgroup per job runs both phases in LDS on the block plan_step placed (ufm_region.h)
int Engine::submit_block(StepRun &r) {
    const StepPlan &pl = r.plan;
    const bool batch = pl.route == Route::BlockBatch;
    RegionJobs rjs{};
    rjs.n = pl.njobs;
    const unsigned int seq = ++pub_seq;
    for (int i = 0; i < pl.njobs; ++i) {
        const RouteJob &pj = pl.job[i];
        RegionJob &j = rjs.j[i];
        if (batch) {       // (the host has done the step bookkeeping of a batch: k_step_begin's part is the job's alone)
            j.rb.sb = step_begin_of(pj.map, 1, 0);
            j.rb.nrect = pj.nrect;
            std::memcpy(j.rb.rect, pj.rect, sizeof(pj.rect));
        } else {
            j.rb = r.rb;
        }
        j.rb.k_raise = iter[Q_RAISE]; j.rb.band = r.band;
        j.tx0 = pj.tx0; j.ntx = pj.ntx; j.ty0 = pj.ty0; j.nty = pj.nty;
        j.dyn = r.dyn_now; j.k_lower = iter[Q_LOWER]; j.max_sweeps = region_sweeps; j.debug = region_debug;
        j.slack = 255.0f * SQRT2F + 1.0f;     // the largest cost of one move (a diagonal through the most expensive cell)
        j.delta = region_band > 0.0f ? region_band * 4.0f * mean_cost : INFINITY;
        j.map = pj.map; j.batch = batch ? 1 : 0; j.seq = seq;
    }
    if (pl.held_in_kernel) {                        // the held host patches are the last rectangles: the kernel applies them
        const int first = r.rb.nrect - (int)lazy.size();
        for (size_t i = 0; i < lazy.size(); ++i) rjs.j[0].psrc[first + (int)i] = h_lazy + (size_t)lazy[i].slot * 4096;
        lazy.clear();                               // (the kernel has read them when this step returns: the slots are free again then)
    }
    if (batch) {   // the counters the maps' workgroups add to
        HIPCHK(hipMemsetAsync(&P.ctr->rbound, 0, offsetof(DevCounters, done_fail) + sizeof(int) - offsetof(DevCounters, rbound), stream));
        k_fill<<<1, 64, 0, stream>>>(reinterpret_cast<float *>(&P.ctr->qmin[Q_RAISE]), (size_t)1, INFINITY);
    }
    // the per-step scalars: a single map's workgroup stores the job's copy itself (it is the only reader before the next launch); a batch's
    // workgroups read *P.dyn side by side (start_bound, tile_heuristic), so there it is in place before the launch
    if (batch) flush_dyn(r);
    else { dyn_dev = r.dyn_now; r.dyn_pending = false; }
    const bool reg_timed = profiling && (region_runs & 7u) == 0u;     // a sample: the event packets cost a few microseconds each
    if (reg_timed) { int rc = reg_ev.ensure(); if (rc != UFM_OK) return rc; }
    // the kernel's form (ufm_region.h, RF_*): the diagnostics bring everything with them; otherwise the heuristic term only where the keys have one
    const int form = region_debug ? (RF_HEUR | RF_DEBUG) : (r.dyn_now.hm != 0.0f ? RF_HEUR : 0);
    with_raise_op(algo, dfm_follow_info, [&](auto a) {
        auto go = [&](auto f) {
            launch(k_replan_region<a(), f()>, dim3(rjs.n), dim3(NTHR), stream, reg_timed ? reg_ev[0] : nullptr, reg_timed ? reg_ev[1] : nullptr, P, rjs, h_ctr, h_ctr.flag());
        };
        if (form == 0) go(IntC<0>{});
        else if (form == RF_HEUR) go(IntC<RF_HEUR>{});
        else go(IntC<(RF_HEUR | RF_DEBUG)>{});
    });
    HIPCHK(hipGetLastError());
    last_active = 1;
    { int rc = wait_published(); if (rc != UFM_OK) return rc; }
    ufm_stats &st = r.st;
    st.region_launches = 1u;
    for (int i = 0; i < rjs.n; ++i) st.region_tiles += (uint32_t)(rjs.j[i].ntx * rjs.j[i].nty);
    if (reg_timed) {      // (the kernel has published its result: its stop event follows within microseconds -- spin, do not sleep)
        hipError_t q;
        while ((q = hipEventQuery(reg_ev[1])) == hipErrorNotReady) __builtin_ia32_pause();
        HIPCHK(q);
        HIPCHK(hipEventElapsedTime(&st.region_kernel_ms, reg_ev[0], reg_ev[1]));
        st.region_timed = 1u;
    }
    region_runs += (uint32_t)rjs.n;
    if (h_ctr->done) region_done += (uint32_t)rjs.n;
    else if (focused) {
        // (its end check has the smallest invalidation priority of the map -- of any map of a batch --, queued or parked: at or
        //  beyond the bound -- a batch: the largest of the maps' bounds -- means the launch chain's invalidation phase, two batches
        //  of launches and two host round trips, would release nothing)
        float qm;
        std::memcpy(&qm, &h_ctr->qmin[Q_RAISE], sizeof(float));
        r.skip_raise = !(qm < h_ctr->rbound);
    }
    return UFM_OK;
}

// The block kernel has left work beyond its block (3 of the headline's 100 replans; a round of a batch as soon as ONE of its maps
// has): the launch chain takes over from the queues -- first as ONE blind submission ending in the device-side end check, like
// the fused chain (a few launches that may find nothing to do are cheaper than the adaptive loop's host round trips:
// that loop cost a batch round of config 4 ~0.6 ms), and only if that was not enough through converge().
int Engine::continue_block(StepRun &r) {
    // (one invalidation launch even when the block kernel saw nothing to invalidate below its bound: the end check reads what the
    //  last launch of each phase released)
    const int nr2 = r.skip_raise ? 1 : std::max(1, cont_raise), nl2 = cont_lower;
    last_active = 1;
    k_unpark<<<1, 1024, 0, stream>>>(P, Q_RAISE, iter[Q_RAISE], -1.0f);       // (-1: the bound the block kernel left in the counters)
    for (int i = 0; i < nr2; ++i) launch_relax(MODE_RAISE, -1.0f);
    k_raise_to_lower<<<1, 1024, 0, stream>>>(P, iter[Q_LOWER]);
    for (int i = 0; i < nl2; ++i) launch_relax(MODE_LOWER, INFINITY);
    { int rc = fused_end(r.band); if (rc != UFM_OK) return rc; }
    r.fast_done = h_ctr->done != 0;
    r.st.raise_launches += (uint32_t)nr2;
    r.st.launches += (uint32_t)(nr2 + nl2);
    r.skip_raise = false;
    ++region_cont; if (r.fast_done) ++region_cont_done;
    return UFM_OK;
}

// Route::Graph: the fused chain, captured once per (nr, nl) and replayed; its inputs go through the job record
int Engine::submit_graph(StepRun &r) {
    r.rb.k_raise = iter[Q_RAISE]; r.rb.band = r.band;
    hipGraphExec_t ge = nullptr;
    { int rc = replan_graph(r.nr, r.nl, r.band, &ge); if (rc != UFM_OK) return rc; }
    h_job->rb = r.rb; h_job->k_lower = iter[Q_LOWER]; h_job->seq = ++pub_seq;
    h_job->dyn = r.dyn_now; dyn_dev = r.dyn_now; r.dyn_pending = false;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    HIPCHK(hipGraphLaunch(ge, stream));
    iter[Q_RAISE] += r.nr; iter[Q_LOWER] += r.nl;
    last_active = 1;
    return wait_published();
}

// Route::FusedChain / Separate: seeds -> invalidation bound -> a blind batch of invalidation launches -> re-lower what they touched ->
// a blind batch of lowering launches -> device-side check -> finalise if the check says "done"; the control steps fused or one by one
int Engine::submit_chain(StepRun &r) {
    const bool fused = r.plan.fused;
    flush_dyn(r);
    if (fused) {
        r.rb.k_raise = iter[Q_RAISE]; r.rb.band = r.band;
        k_replan_begin<<<1, 1024, 0, stream>>>(P, r.rb);
    } else {
        k_seeds_to_active<<<1, 1024, 0, stream>>>(P, Q_RAISE, iter[Q_RAISE]);
        k_prepare_bound<<<1, 64, 0, stream>>>(P, r.band);
        k_unpark<<<1, 1024, 0, stream>>>(P, Q_RAISE, iter[Q_RAISE], -1.0f);
    }
    const EventSet<4> &e = chain_ev;
    if (profiling) {
        { int rc = chain_ev.ensure(); if (rc != UFM_OK) return rc; }
        HIPCHK(hipEventRecord(e[0], stream));
    }
    last_active = 1;             // replans touch a handful of tiles: fused triage
    for (int i = 0; i < r.nr; ++i) launch_relax(MODE_RAISE, -1.0f);
    if (profiling) HIPCHK(hipEventRecord(e[1], stream));
    if (fused) {
        k_raise_to_lower<<<1, 1024, 0, stream>>>(P, iter[Q_LOWER]);
    } else {
        k_touched_to_active<<<64, 256, 0, stream>>>(P, Q_LOWER, iter[Q_LOWER]);
        k_unpark<<<1, 1024, 0, stream>>>(P, Q_LOWER, iter[Q_LOWER], INFINITY);
    }
    if (profiling) HIPCHK(hipEventRecord(e[2], stream));
    for (int i = 0; i < r.nl; ++i) launch_relax(MODE_LOWER, INFINITY);
    if (profiling) HIPCHK(hipEventRecord(e[3], stream));
    if (fused) {
        int rc = fused_end(r.band);
        if (rc != UFM_OK) return rc;
    } else {
        k_check<<<1, 1024, 0, stream>>>(P, iter[Q_RAISE], iter[Q_LOWER], r.band);
        finalize_bp(1);
        k_finalize<<<2048, 256, 0, stream>>>(P, 1);
        HIPCHK(hipGetLastError());
        int rc = fetch_counters();
        if (rc != UFM_OK) return rc;
    }
    if (profiling) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e[0], e[1])); r.st.kernel_ms += ms; r.st.raise_kernel_ms += ms;
        HIPCHK(hipEventElapsedTime(&ms, e[2], e[3])); r.st.kernel_ms += ms;
    }
    return UFM_OK;
}

// A replan: one submission, one host round trip, by the route plan_step chose.  (An empty launch costs a few microseconds; a host
// round trip costs more.)  If that was not enough, converge() takes over.
int Engine::replan(StepRun &r) {
    const Route route = r.plan.route;
    const bool block = route == Route::BlockSingle || route == Route::BlockBatch;
    const int k0_raise = iter[Q_RAISE], k0_lower = iter[Q_LOWER];
    { int rc = block ? submit_block(r) : (route == Route::Graph ? submit_graph(r) : submit_chain(r)); if (rc != UFM_OK) return rc; }
    r.updated += h_ctr->updated;
    r.fast_done = h_ctr->done != 0;
    ufm_stats &st = r.st;
    if (block) {
        st.launches += 1u;
        return (!r.fast_done && spin_wait && cont_lower > 0) ? continue_block(r) : UFM_OK;
    }
    st.raise_launches += (uint32_t)r.nr;
    st.launches += (uint32_t)(r.nr + r.nl);
    // (launches replayed from the graph are not event-timed: HIP cannot read events recorded by graph nodes)
    if (profiling && route != Route::Graph) { st.timed_launches += (uint32_t)(r.nr + r.nl); st.timed_raise_launches += (uint32_t)r.nr; }
    // launches the batches actually needed (for the next steps' batch sizes); a batch that was
    // too short costs a host round trip and the adaptive loop, so err on the long side after one
    const int need_r = std::max(0, h_ctr->last_work[Q_RAISE] - k0_raise + 1);
    const int need_l = std::max(0, h_ctr->last_work[Q_LOWER] - k0_lower + 1);
    win_raise[win_pos] = r.fast_done ? need_r : r.nr + 2;
    win_lower[win_pos] = r.fast_done ? need_l : r.nl + 2;
    win_pos = (win_pos + 1) % 6;
    return UFM_OK;
}

// Route::SeedsOnly: the seeds of initialising maps go to the queue, converge() plans
int Engine::seed_only(StepRun &r) {
    flush_dyn(r);
    // num_nodes_updated (FD impl:138, DFM impl:109) of the participating maps
    HIPCHK(hipMemcpyAsync(scratch.num_updated, P.num_updated, sizeof(unsigned int) * nmaps, hipMemcpyDeviceToHost, stream));
    // patches enter an existing field through the invalidation queue, a fresh one directly
    const int sq = (r.plan.n_upd > 0) ? Q_RAISE : Q_LOWER;
    k_seeds_to_active<<<1, 1024, 0, stream>>>(P, sq, iter[sq]);
    HIPCHK(hipStreamSynchronize(stream));
    for (int m = 0; m < nmaps; ++m) {
        if (!scratch.consume[m]) continue;
        if (!scratch.init[m]) r.updated += scratch.num_updated[m];
        HIPCHK(hipMemsetAsync(P.num_updated + m, 0, sizeof(unsigned int), stream));
    }
    return UFM_OK;
}

// The adaptive rounds.  Invalidate, then lower, both only as far as the start's key (the reference's end_condition).  The
// invalidation bound must reach the key the start ends up with, which is only known afterwards: start from the current key plus
// one ordering band and repeat while invalidations below the new key are still queued.
int Engine::converge(StepRun &r) {
    const StepPlan &pl = r.plan;
    ufm_stats &st = r.st;
    const bool do_raise = pl.have_seeds && pl.n_upd > 0;
    flush_dyn(r);
    float rbound = INFINITY;
    if (focused && do_raise) {
        if (h_ctr->rbound > 0.0f && pl.n_init == 0 && pl.n_upd > 0) {
            rbound = h_ctr->rbound;      // continue from the replan's (possibly enlarged) bound
        } else {
            float b0 = 0.0f;
            int rc = read_bounds(&b0);
            if (rc != UFM_OK) return rc;
            rbound = b0 + r.band;
        }
    }
    for (int round = 0; round < 64; ++round) {
        const auto ta = std::chrono::steady_clock::now();
        if (do_raise && !(r.skip_raise && round == 0)) {
            uint32_t rl = 0, rt = 0;
            float rk = 0.0f;
            k_unpark<<<1, 1024, 0, stream>>>(P, Q_RAISE, iter[Q_RAISE], rbound);
            int rc = run_phase(MODE_RAISE, rbound, &rl, &rk, &rt);
            if (rc != UFM_OK) return rc;
            st.kernel_ms += rk; st.raise_kernel_ms += rk;
            st.timed_launches += rt; st.timed_raise_launches += rt;
            st.raise_launches += rl;
            st.launches += rl;
            // everything invalidation touched must be re-lowered
            k_touched_to_active<<<64, 256, 0, stream>>>(P, Q_LOWER, iter[Q_LOWER]);
        }
        const auto tb = std::chrono::steady_clock::now();
        uint32_t ll = 0;
        k_unpark<<<1, 1024, 0, stream>>>(P, Q_LOWER, iter[Q_LOWER], INFINITY);
        int owned_left = -1;
        if (use_owned && pl.n_init > 0 && round == 0 && dyn_grid >= 256) {
            int rc = owned_phase();
            if (rc != UFM_OK) return rc;
            st.launches += 1u;
            st.resident_launches += 1u;
            // what it handed back (nothing, unless it ran into its time limit): no need to send launches after an empty list
            rc = fetch_counters();
            if (rc != UFM_OK) return rc;
            owned_left = h_ctr->cnt[Q_LOWER][iter[Q_LOWER] % 3];
        }
        int rc = owned_left == 0 ? UFM_OK : run_phase(MODE_LOWER, INFINITY, &ll, &st.kernel_ms, &st.timed_launches);
        if (rc != UFM_OK) return rc;
        st.launches += ll;
        bool again = false;
        if (focused && do_raise) {
            float bnew = 0.0f;
            rc = read_bounds(&bnew);
            if (rc != UFM_OK) return rc;
            k_queue_min<<<1, 1024, 0, stream>>>(P, Q_RAISE, iter[Q_RAISE]);
            rc = fetch_counters();
            if (rc != UFM_OK) return rc;
            float qm;
            std::memcpy(&qm, &h_ctr->qmin[Q_RAISE], sizeof(float));
            if (qm < bnew) { again = true; rbound = std::fmax(bnew, rbound) + r.band; }
        }
        const auto tc = std::chrono::steady_clock::now();
        r.u_acc += std::chrono::duration<double, std::milli>(tb - ta).count();
        r.p_acc += std::chrono::duration<double, std::milli>(tc - tb).count();
        if (!again) break;
    }
    const auto td = std::chrono::steady_clock::now();
    finalize_bp(0);
    k_finalize<<<2048, 256, 0, stream>>>(P, 0);
    { int rc = fetch_counters(); if (rc != UFM_OK) return rc; }
    copy_counters(st);
    if (st.resident_launches) {
        st.resident_tile_visits = h_ctr->own_vis1 - h_ctr->own_vis0;
        st.resident_stops = (uint32_t)h_ctr->own_stops;
        if (own_timed) HIPCHK(hipEventElapsedTime(&st.resident_kernel_ms, own_ev[0], own_ev[1]));
    }
    if (profiling) {   // diagnostics: sum over launches of the slowest tile's sweep count
        std::vector<int> lm(LMAX);
        HIPCHK(hipMemcpy(lm.data(), P.lmax, sizeof(int) * LMAX, hipMemcpyDeviceToHost));
        for (int v : lm) st.crit_sweeps += (uint64_t)v;
    }
    r.p_acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td).count();
    return UFM_OK;
}

void Engine::copy_counters(ufm_stats &st) const {   // the published counter block into the step's statistics
    st.expanded = h_ctr->expanded;
    st.tile_visits = h_ctr->tile_visits;
    st.tile_iters = h_ctr->tile_iters;
    st.elem_evals = h_ctr->elem_evals;
    st.raise_tile_visits = h_ctr->raise_visits;
}

int Engine::step(ufm_stats *out, const float *auto_mult) {
    // ReplannerBase.h:44-45
    for (int m = 0; m < nmaps; ++m) if (!maps[m].have_map) return UFM_LOOP_FAILURE_NO_GRAPH;
    for (int m = 0; m < nmaps; ++m) if (!maps[m].goal_set) return UFM_LOOP_FAILURE_NO_GOAL;
    StepRun r{};
    r.t0 = std::chrono::steady_clock::now();
    // blind batch sizes of a replan: what the recent replans needed, plus one
    r.nr = r.nl = 1;
    for (int i = 0; i < 6; ++i) { r.nr = std::max(r.nr, win_raise[i] + batch_margin); r.nl = std::max(r.nl, win_lower[i] + batch_margin); }
    r.plan = plan_step(ROUTE_CONFIG, route_switches(), maps.data(), pending.data(), (int)pending.size(), (int)lazy.size(), r.nr, r.nl,
                       scratch.consume, scratch.init);
    const StepPlan &pl = r.plan;
    // "auto_multiplier": the smallest cost of the planning rasters as they stand (a batch: ufm_batch_step hands in the minimum over all shards)
    // instead of the caller's; it reaches the device like any new multiplier, through the job record or k_set_dyn
    float mult = heuristic_multiplier;
    if (auto_multiplier && heur) {
        if (auto_mult) mult = *auto_mult;
        else { int mn = 0, mx = 0; const int rc = census_minmax(&mn, &mx); if (rc != UFM_OK) return rc; mult = (float)mn; }
    }
    last_multiplier = mult;
    r.dyn_now = DevDyn{heur ? mult : 0.0f, thr_uchar, focused ? 1 : 0, 0};
    r.dyn_pending = std::memcmp(&r.dyn_now, &dyn_dev, sizeof(DevDyn)) != 0;
    r.band = raise_margin * band_delta(delta_scale);
    { int rc = begin_step(r); if (rc != UFM_OK) return rc; }
    r.t_seed = std::chrono::steady_clock::now();
    if (pl.route == Route::SeedsOnly) { int rc = seed_only(r); if (rc != UFM_OK) return rc; }
    else if (pl.route != Route::None) { int rc = replan(r); if (rc != UFM_OK) return rc; }
    if (r.n_init_tiles > 0) {        // the goal tiles of the initialising maps: where their plans start
        HIPCHK(hipMemcpyAsync(d_scratch, scratch.init_tiles, sizeof(int) * r.n_init_tiles, hipMemcpyHostToDevice, stream));
        k_activate_list<<<1, 64, 0, stream>>>(P, Q_LOWER, iter[Q_LOWER], d_scratch, r.n_init_tiles);
    }
    // ReplannerBase.h:65-69: plan() only if something was (re)initialised or updated
    const bool do_plan = (pl.n_init > 0 || r.updated > 0 || (pl.have_seeds && pl.n_upd > 0)) && !r.fast_done;
    r.u_acc = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r.t0).count();
    if (do_plan) {
        int rc = converge(r);
        if (rc != UFM_OK) return rc;
    } else if (r.fast_done) {
        copy_counters(r.st);
        const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r.t_seed).count();
        r.u_acc += 0.5 * dt;   // invalidation and lowering ran in one submission: split evenly
        r.p_acc += 0.5 * dt;
    } else {
        HIPCHK(hipStreamSynchronize(stream));
    }
    for (int m = 0; m < nmaps; ++m) maps[m].new_goal = maps[m].initialize_search = false;
    ufm_stats &st = r.st;
    st.updated = r.updated;
    st.queued_lower = (uint32_t)(h_ctr->cnt[Q_LOWER][iter[Q_LOWER] % 3] + h_ctr->npark[Q_LOWER]);   // parked beyond the start's key
    st.queued_raise = (uint32_t)(h_ctr->cnt[Q_RAISE][iter[Q_RAISE] % 3] + h_ctr->npark[Q_RAISE]);
    st.graphs_instantiated = graphs_made;
    st.region_replans = region_runs; st.region_replans_done = region_done;
    reveal_busy = false;        // (the step has waited for kernels queued behind any reveal)
    st.u_ms = (float)r.u_acc;   // seeding + invalidation (the reference's update())
    st.p_ms = (float)r.p_acc;   // propagation + finalisation (the reference's plan())
    last = st;
    if (out) *out = st;
    return UFM_OK;
}

int engine_create(Engine **out, int n_maps, int algo, int opt_lvl, int use_heuristic, int device_id) {
    if (!out || n_maps < 1 || algo < 0 || algo > 2 || opt_lvl < 0 || opt_lvl > 2) return UFM_ERR_INVALID;
    if (algo != UFM_ALGO_SG && opt_lvl > 1) return UFM_ERR_INVALID;   // only ShiftedGridPlanner has level 2
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<Engine> e(new (std::nothrow) Engine());   // every early return below frees what has been made so far
    if (!e) return UFM_ERR_NOMEM;
    e->algo = algo; e->opt_lvl = opt_lvl; e->heur = use_heuristic; e->device = device_id; e->nmaps = n_maps;
    // scheduling defaults per planner family (tools/sweep.py, 4096^2): DFM's two-stencil operator needs about
    // twice the sweeps per tile; a wider band and an earlier re-queue suit it better (plan 60 -> 52 ms)
    // -- for a single map; a batch is throughput-bound and keeps the less redundant setting (8 x 2048^2: 484 vs 476 M cells/s)
    if (algo == UFM_ALGO_DFM && n_maps == 1) { e->delta_scale = e->delta_scale_long = 2.5f; e->max_iters = 16; }
    if (algo == UFM_ALGO_DFM) { e->cont_lower = 0; e->region_tiles = 8; e->region_ahead = 3; }   // (config 4: the 8 x 8 block finishes 78 % of the rounds alone, 6 x 6: 71 %)
    e->maps.resize(n_maps);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    e->grid_relax = prop.multiProcessorCount * 2;
    e->dyn_grid = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&e->stream.s, hipStreamNonBlocking));
    for (Published<DevCounters> *pub : {&e->h_ctr, &e->h_pipe_ctr[0], &e->h_pipe_ctr[1]}) { int rc = pub->alloc(); if (rc != UFM_OK) return rc; }
    { int rc = e->h_job.alloc(1, Pin::Coherent); if (rc != UFM_OK) return rc; }
    std::memset(e->h_job, 0, sizeof(ReplanJob));
    {   // The first graph a process captures and instantiates costs ~8 ms of one-time set-up inside the
        // runtime; pay it here, not in the first replan (a planner is created outside any timed step).
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            k_fill<<<1, 64, 0, e->stream>>>(reinterpret_cast<float *>(e->h_job.p), 0, 0.0f);
            if (hipStreamEndCapture(e->stream, &g) == hipSuccess && g) {
                if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess && ge) {
                    (void)hipGraphLaunch(ge, e->stream);
                    (void)hipStreamSynchronize(e->stream);
                    (void)hipGraphExecDestroy(ge);
                }
                (void)hipGraphDestroy(g);
            }
        }
        (void)hipGetLastError();
    }
    { int rc = e->scratch.carve(n_maps); if (rc != UFM_OK) return rc; }
    { int rc = e->h_bnd.alloc(n_maps); if (rc != UFM_OK) return rc; }
    *out = e.release();
    return UFM_OK;
}

int engine_destroy(Engine *e) {     // ~Engine waits for the stream and drops the graphs; the members' order does the rest
    if (!e) return UFM_ERR_INVALID;
    delete e;
    return UFM_OK;
}

int engine_set_goal(Engine *e, int m, float x, float y) {
    if (!e || m < 0 || m >= e->nmaps) return UFM_ERR_INVALID;
    MapState &ms = e->maps[m];
    // Node(Position)/Cell(Position) round (Node.cpp:14-17, Cell.cpp:20-21); ReplannerBase.h:99-108
    const int ex = (int)std::roundf(x), ey = (int)std::roundf(y);
    ms.new_goal = !ms.goal_set ? true : (ex != ms.goal_ex || ey != ms.goal_ey);
    ms.goal_x = x; ms.goal_y = y; ms.goal_ex = ex; ms.goal_ey = ey;
    ms.goal_set = true;
    ms.goal_elem_valid = e->allocated && ex >= 0 && ey >= 0 && ex < e->P.EX && ey < e->P.EY;
    return UFM_OK;
}

int engine_read_field(Engine *e, int m, int x0, int y0, int nx, int ny, float *g, float *rhs) {
    if (!e || m < 0 || m >= e->nmaps || !e->allocated) return UFM_ERR_INVALID;
    if (x0 < 0 || y0 < 0 || nx <= 0 || ny <= 0 || x0 + nx > e->P.EX || y0 + ny > e->P.EY) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    float *dst = g ? g : rhs;
    if (!dst) return UFM_OK;
    // the field is tile-major on the device: gather the window into a dense buffer, then one copy
    const size_t n = (size_t)nx * ny;
    { int rc = e->d_field.reserve(e->stream, n); if (rc != UFM_OK) return rc; }
    k_gather_field<<<(unsigned)std::min<size_t>((n + 255) / 256, 65535), 256, 0, e->stream>>>(e->P, m, x0, y0, nx, ny, e->d_field);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, e->d_field, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // at the fixed point RHS(s) = F(G)(s) = G(s) for every element (goal: 0 = 0)
    if (g && rhs) std::memcpy(rhs, g, (size_t)nx * ny * sizeof(float));
    return UFM_OK;
}

// Path extraction: n walks over this engine's maps, one wavefront each (k_extract_path).  Walk k starts at (q[k].sx, q[k].sy) on map
// q[k].m, ends at that map's goal and is delivered as record q[k].slot of the caller's arrays -- path_xy: [..][cap_pts][2],
// step_costs: [..][cap_costs], info: [..] (e_ms is the caller's to fill).  The caller has checked the arguments; patches that are being
// held are applied first (the walk reads the raster).  Launches of at most PATH_CHUNK_JOBS walks, and of at most PATH_CHUNK_FLOATS of
// output, so that the device and the pinned buffer stay bounded whatever n and max_steps are.
struct PathQuery { int m; float sx, sy; size_t slot; };
// map m's field and raster as the kernels of ufm_path.h and ufm_delta.h read them (FD: all five cost cases; SG: B / II / A)
static PathField path_field(const Engine *e, int m) {
    PathField F{};
    F.G = e->P.G + (size_t)m * e->P.gstride; F.cost = e->P.cost + (size_t)m * e->P.cstride;
    F.EX = e->P.EX; F.EY = e->P.EY; F.L = e->P.L; F.W = e->P.W; F.TY = e->P.TY; F.thr = e->thr_uchar;
    F.cells = (e->algo == UFM_ALGO_DFM); F.indirect = (e->algo == UFM_ALGO_FD);
    return F;
}
constexpr size_t PATH_CHUNK_JOBS = 65536, PATH_CHUNK_FLOATS = (size_t)16 << 20;

int engine_walk(Engine *e, const PathQuery *q, size_t n, int max_steps, int lookahead, int allow_indirect,
                float *path_xy, int cap_pts, float *step_costs, int cap_costs, ufm_path_info *info) {
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    // the device keeps what the caller has room for, at most what max_steps moves can produce
    const int dev_pts = std::min(cap_pts, 3 * max_steps + 1), dev_cst = std::min(cap_costs, 2 * max_steps);
    const size_t ostride = PATH_HDR + 2 * (size_t)dev_pts + dev_cst;
    const size_t chunk = std::min(n, std::min(PATH_CHUNK_JOBS, std::max<size_t>(PATH_CHUNK_FLOATS / ostride, 1)));
    { int rc = e->d_path.reserve(e->stream, ostride * chunk, true, true); if (rc != UFM_OK) return rc; }
    { int rc = e->d_jobs.reserve(e->stream, chunk, true, true); if (rc != UFM_OK) return rc; }
    PathJob *h_jobs = e->d_jobs.pinned;
    const float *h_path = e->d_path.pinned;
    PathField F = path_field(e, 0);     // (the walks' jobs name their maps)
    F.indirect = allow_indirect != 0;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = std::min(chunk, n - first);
        for (size_t k = 0; k < cnt; ++k) {      // (the pinned buffers are free again: every chunk ends with a wait for the stream)
            const PathQuery &w = q[first + k];
            h_jobs[k] = PathJob{w.sx, w.sy, e->maps[w.m].goal_x, e->maps[w.m].goal_y, w.m};
        }
        HIPCHK(hipMemcpyAsync(e->d_jobs, h_jobs, sizeof(PathJob) * cnt, hipMemcpyHostToDevice, e->stream));
        k_extract_path<<<(unsigned)cnt, 64, 0, e->stream>>>(F, e->P.gstride, e->P.cstride, e->d_jobs, e->d_path, ostride,
                                                            dev_pts, dev_cst, lookahead != 0, max_steps);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(e->d_path.pinned, e->d_path, ostride * cnt * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (size_t k = 0; k < cnt; ++k) {
            const float *o = h_path + ostride * k;
            const size_t slot = q[first + k].slot;
            ufm_path_info &pi = info[slot];
            std::memcpy(&pi.n_points, &o[0], 4);
            std::memcpy(&pi.n_costs, &o[1], 4);
            pi.total_cost = o[2];
            pi.total_dist = o[3];
            std::memcpy(&pi.steps, &o[4], 4);
            const int np = std::min(pi.n_points, dev_pts), nc = std::min(pi.n_costs, dev_cst);
            if (np > 0) std::memcpy(path_xy + slot * cap_pts * 2, o + PATH_HDR, sizeof(float) * 2 * np);
            if (nc > 0) std::memcpy(step_costs + slot * cap_costs, o + PATH_HDR + 2 * (size_t)dev_pts, sizeof(float) * nc);
        }
    }
    return UFM_OK;
}

// what every extraction asks of its buffers
static bool path_buffers_ok(int max_steps, const float *path_xy, int cap_pts, const float *step_costs, int cap_costs, const ufm_path_info *info) {
    return info && max_steps >= 1 && cap_pts >= 0 && cap_costs >= 0 && !(cap_pts > 0 && !path_xy) && !(cap_costs > 0 && !step_costs);
}

// Every map of the engine from its own start (Graph::start_pos_): the walks "one per map, in map order".
// path_xy: [nmaps][cap_pts][2], step_costs: [nmaps][cap_costs], info: [nmaps].
int engine_extract_path(Engine *e, int max_steps, int lookahead, int allow_indirect,
                        float *path_xy, int cap_pts, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (!e || !e->allocated || !path_buffers_ok(max_steps, path_xy, cap_pts, step_costs, cap_costs, info)) return UFM_ERR_INVALID;
    for (const MapState &ms : e->maps) if (!ms.have_map || !ms.start_set || !ms.goal_set) return UFM_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<PathQuery> q((size_t)e->nmaps);
    for (int m = 0; m < e->nmaps; ++m) q[m] = PathQuery{m, e->maps[m].start_x, e->maps[m].start_y, (size_t)m};
    { int rc = engine_walk(e, q.data(), q.size(), max_steps, lookahead, allow_indirect, path_xy, cap_pts, step_costs, cap_costs, info); if (rc != UFM_OK) return rc; }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int m = 0; m < e->nmaps; ++m) info[m].e_ms = ms;
    return UFM_OK;
}

// Walks from the caller's positions, on the fields as they stand (ufm_extract_paths_from / ufm_batch_extract_paths_from): walk k
// starts at starts_xy[k] on map map_index[k] (nullptr: map 0) of the handle, whose map i lives in shards[i / per].  Everything is
// checked before anything is launched or written; nothing of a planner's state is touched (start, new_start, queues: a query, not a
// set_start).  One launch sequence per shard, results in the caller's order.
int paths_from(Engine *const *shards, int per, int n_maps, int n_starts, const int32_t *map_index, const float *starts_xy,
               int max_steps, int lookahead, int allow_indirect, float *path_xy, int cap_pts, float *step_costs, int cap_costs, ufm_path_info *info) {
    if (n_starts < 1 || !starts_xy || !path_buffers_ok(max_steps, path_xy, cap_pts, step_costs, cap_costs, info)) return UFM_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    const int n_shards = (n_maps + per - 1) / per;
    std::vector<std::vector<PathQuery>> q((size_t)n_shards);
    for (int k = 0; k < n_starts; ++k) {
        const int i = map_index ? map_index[k] : 0;
        if (i < 0 || i >= n_maps) return UFM_ERR_INVALID;
        const Engine *e = shards[i / per];
        const int m = i % per;
        if (!e->allocated || !e->maps[m].have_map || !e->maps[m].goal_set) return UFM_ERR_INVALID;
        const float x = starts_xy[2 * (size_t)k], y = starts_xy[2 * (size_t)k + 1];
        if (!(x >= 0.0f && x <= (float)e->L && y >= 0.0f && y <= (float)e->W)) return UFM_ERR_INVALID;     // (a NaN fails every comparison)
        q[i / per].push_back(PathQuery{m, x, y, (size_t)k});
    }
    for (int s = 0; s < n_shards; ++s) {
        if (q[s].empty()) continue;
        const int rc = engine_walk(shards[s], q[s].data(), q[s].size(), max_steps, lookahead, allow_indirect, path_xy, cap_pts, step_costs, cap_costs, info);
        if (rc != UFM_OK) return rc;
    }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < n_starts; ++k) info[k].e_ms = ms;
    return UFM_OK;
}

// Trajectory scoring (ufm_score_paths ...; k_score_paths, ufm_score.h): n of the caller's paths on this engine's maps, one wavefront
// each.  Path q[j].k of the caller's arrays -- points offsets[k] .. offsets[k + 1] - 1 of points_xy -- lies on map q[j].m and its record
// goes to out[k].  The caller has checked the arguments; patches that are being held are applied first (the walk reads the raster).
// Launches of at most SCORE_CHUNK_PATHS paths, each staged dense through the pinned twins and followed by a wait for the stream.
struct ScoreQuery { int m; size_t k; };
constexpr size_t SCORE_CHUNK_PATHS = 65536;
int engine_score(Engine *e, const ScoreQuery *q, size_t n, const int32_t *offsets, const float *points_xy, ufm_score *out) {
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    const PathField F = path_field(e, 0);     // (the paths name their maps)
    Engine::ScoreStage &st = e->score;
    for (size_t first = 0; first < n; first += SCORE_CHUNK_PATHS) {
        const size_t cnt = std::min(SCORE_CHUNK_PATHS, n - first);
        size_t npts = 0;
        for (size_t j = 0; j < cnt; ++j) { const size_t k = q[first + j].k; npts += (size_t)(offsets[k + 1] - offsets[k]); }
        if (npts > (size_t)INT_MAX) return UFM_ERR_INVALID;
        // (the pinned twins are free: every chunk ends with a wait for the stream)
        { int rc = st.idx.reserve(e->stream, 2 * cnt + 1, true, true); if (rc != UFM_OK) return rc; }
        { int rc = st.pts.reserve(e->stream, 2 * std::max<size_t>(npts, 1), true, true); if (rc != UFM_OK) return rc; }
        { int rc = st.out.reserve(e->stream, cnt, true, true); if (rc != UFM_OK) return rc; }
        int32_t *h_off = st.idx.pinned, *h_map = h_off + cnt + 1;
        size_t at = 0;
        for (size_t j = 0; j < cnt; ++j) {
            const size_t k = q[first + j].k, np = (size_t)(offsets[k + 1] - offsets[k]);
            h_off[j] = (int32_t)at;
            h_map[j] = q[first + j].m;
            if (np) std::memcpy(st.pts.pinned + 2 * at, points_xy + 2 * (size_t)offsets[k], sizeof(float) * 2 * np);
            at += np;
        }
        h_off[cnt] = (int32_t)at;
        HIPCHK(hipMemcpyAsync(st.idx, st.idx.pinned, sizeof(int32_t) * (2 * cnt + 1), hipMemcpyHostToDevice, e->stream));
        if (npts) HIPCHK(hipMemcpyAsync(st.pts, st.pts.pinned, sizeof(float) * 2 * npts, hipMemcpyHostToDevice, e->stream));
        k_score_paths<<<(unsigned)cnt, 64, 0, e->stream>>>(F, e->P.cstride, st.idx, st.idx + cnt + 1, 0, st.pts, (int)npts, st.out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st.out.pinned, st.out, sizeof(ufm_score) * cnt, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (size_t j = 0; j < cnt; ++j) out[q[first + j].k] = st.out.pinned[j];
    }
    return UFM_OK;
}

// The host forms (ufm_score_paths / ufm_batch_score_paths): path k lies on map map_index[k] (nullptr: map 0) of the handle, whose map i
// lives in shards[i / per].  Everything is checked before anything is launched or written; one launch sequence per shard, records in
// the caller's order.
int score_paths(Engine *const *shards, int per, int n_maps, int n_paths, const int32_t *map_index, const int32_t *offsets,
                const float *points_xy, ufm_score *out) {
    if (n_paths < 1 || !offsets || !points_xy || !out || offsets[0] != 0) return UFM_ERR_INVALID;
    const int n_shards = (n_maps + per - 1) / per;
    std::vector<std::vector<ScoreQuery>> q((size_t)n_shards);
    for (int k = 0; k < n_paths; ++k) {
        const int i = map_index ? map_index[k] : 0;
        if (i < 0 || i >= n_maps || offsets[k + 1] < offsets[k]) return UFM_ERR_INVALID;
        const Engine *e = shards[i / per];
        if (!e->allocated || !e->maps[i % per].have_map) return UFM_ERR_INVALID;
        q[i / per].push_back(ScoreQuery{i % per, (size_t)k});
    }
    for (int s = 0; s < n_shards; ++s) {
        if (q[s].empty()) continue;
        const int rc = engine_score(shards[s], q[s].data(), q[s].size(), offsets, points_xy, out);
        if (rc != UFM_OK) return rc;
    }
    return UFM_OK;
}

// The device form: every path on map m, offsets, points and records in this device's memory; queued on the engine's stream, nothing
// copied, nothing waited for (flush_deferred() itself only queues, unless a held patch has to be staged).
int engine_score_device(Engine *e, int m, int n_paths, int total_points, const int32_t *dev_offsets, const float *dev_points_xy, ufm_score *dev_out) {
    if (!e || !e->allocated || m < 0 || m >= e->nmaps || !e->maps[m].have_map) return UFM_ERR_INVALID;
    if (n_paths < 1 || total_points < 0 || !dev_offsets || !dev_points_xy || !dev_out) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    k_score_paths<<<(unsigned)n_paths, 64, 0, e->stream>>>(path_field(e, 0), e->P.cstride, dev_offsets, nullptr, m, dev_points_xy, total_points, dev_out);
    HIPCHK(hipGetLastError());
    return UFM_OK;
}

// The elements the reference would hold in its priority queue after the step: G != RHS (k_queue_scan, ufm_path.h).
int engine_read_queue(Engine *e, int m, int cap, int32_t *xy, float *g_rhs, int *total) {
    if (!e || m < 0 || m >= e->nmaps || !e->allocated || !total || cap < 0 || (cap > 0 && (!xy || !g_rhs))) return UFM_ERR_INVALID;
    if (!e->maps[m].goal_set) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }   // (the derived RHS / the stored bytes' view read the raster)
    const size_t words = (size_t)std::max(cap, 1) * 4 + 1;          // [cap][2] int32, [cap][2] float, the count
    { int rc = e->d_info.reserve(e->stream, words); if (rc != UFM_OK) return rc; }
    int32_t *d_xy = e->d_info;
    float *d_gr = reinterpret_cast<float *>(e->d_info + (size_t)std::max(cap, 1) * 2);
    unsigned int *d_cnt = reinterpret_cast<unsigned int *>(e->d_info + (size_t)std::max(cap, 1) * 4);
    const PathField F = path_field(e, m);
    const MapState &ms = e->maps[m];
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned int), e->stream));
    const size_t n = (size_t)e->P.EX * e->P.EY;
    k_queue_scan<<<(unsigned)std::min<size_t>((n + 255) / 256, 4096), 256, 0, e->stream>>>(F, e->opt_lvl, ms.goal_ex, ms.goal_ey, cap, d_xy, d_gr, d_cnt);
    hipError_t err = hipGetLastError();
    unsigned int cnt = 0;
    if (err == hipSuccess) err = hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIPCHK(err);
    *total = (int)cnt;
    const size_t k = std::min<size_t>(cnt, (size_t)cap);
    if (k) {
        HIPCHK(hipMemcpyAsync(xy, d_xy, k * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(g_rhs, d_gr, k * 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return UFM_OK;
}

// Back-pointers of a window of elements: the stored codes in the reference's format (k_info_stored), or derived from the field alone
// (k_info, the checker), ufm_path.h.
int engine_read_info(Engine *e, int m, int x0, int y0, int nx, int ny, int32_t *info, bool derived) {
    if (!e || m < 0 || m >= e->nmaps || !e->allocated || !info) return UFM_ERR_INVALID;
    if (e->opt_lvl == 0) return UFM_ERR_INVALID;            // level 0: the map has no Info member (void)
    if (x0 < 0 || y0 < 0 || nx <= 0 || ny <= 0 || x0 + nx > e->P.EX || y0 + ny > e->P.EY) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }   // (the derived RHS / the stored bytes' view read the raster)
    const size_t n = (size_t)nx * ny;
    { int rc = e->d_info.reserve(e->stream, n * 2); if (rc != UFM_OK) return rc; }     // (kept between calls: a consumer asks window after window)
    int32_t *d_out = e->d_info;
    const PathField F = path_field(e, m);
    if (derived) k_info<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(F, e->opt_lvl, x0, y0, nx, ny, d_out);
    else k_info_stored<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(F, e->P.bp + (size_t)m * e->P.gstride, x0, y0, nx, ny, d_out);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(info, d_out, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIPCHK(err);
    return UFM_OK;
}

