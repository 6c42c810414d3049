// ufm_knobs.h -- the engine's tuning members and the one table that names them: what ufm_set_param / ufm_batch_set_param can set.
// Engine derives from Knobs (ufm_host.h), so the engine reads them as its own members; Knobs owns nothing.  Four names need more than
// a member write -- "defer_patches", "lazy_patches", "auto_multiplier", "dfm_follow_info" -- and are handled by engine_set_param
// (ufm_capi.h) in front of the table; their members live here with the rest.  Plain C++17 without HIP: tests/cpp/knobs_driver.cpp
// compiles this header alone.  DESIGN.md section 2.1 lists the knobs from this table.
#pragma once
#include <cmath>
#include <cstring>

struct Knobs {
    bool pipeline_batches = true;
    bool spin_wait = true;           // false: hipMemcpyAsync + hipStreamSynchronize instead
    bool fuse_control = true;        // replans: fused control kernels (k_replan_begin / _raise_to_lower / _end)
    bool use_graph = true;           // replans: the whole submission replayed as one captured hipGraph
    bool use_owned = true;           // plans: the lowering phase as ONE resident launch (k_relax<.,LOWER,false,1|2>) instead of a launch per band step
    float owned_limit_ms = -1.0f;    // ... which hands back to the launch chain after this long, whatever happens (< 0: by the size of the job,
                                     //     ~15 x what a plan of that many tiles takes: a device shared with another long-running kernel)
    float owned_band = -1.0f;        // ... ordering band in tile crossings (< 0: by the job -- 2.5 for a single map of a node planner, 3 for MS-DFM, 2 for a batch: owned_phase())
    int owned_flags = 0;             // resident kernel, diagnostics and variants.  1: no tile taken ahead; 2: no early hand-off (FD / SG); 4: early hand-off once per patch and visit;
                                     // 8: early hand-off waits for its stores inside the sweep loop; 16: no in-visit halo refresh; 32: idle workgroups do not help out;
                                     // 64: a workgroup does not follow the front (the neighbour it has just queued); 128: ... follows it beyond the ordering band too
    int owned_waves = 0;             // waves per tile visit of the resident kernel: 16 (256 workgroups), 8 (512), 0 = by the size of the job
    bool dfm_follow_info = false;    // MS-DFM level 1: the invalidation follows the stored back-pointer bytes (k_relax / k_replan_region<ALGO_DFM1_INFO>)
    bool use_region = true;          // replans: one workgroup runs both phases in LDS on the block around the patch (ufm_region.h);
                                     // the launch chain only takes over when work is left outside the block
    int region_ahead = 2;            // block placement: tiles kept between the patches' centre and the block's goal-side edge
    int region_tiles = 6;            // block edge in tiles (<= RTMAX; measured on the headline replans: 10 -> 6 tiles: 20.0 -> 18.6 ms per 100, same completion rate)
    int region_sweeps = 4096;        // sweep budget per wave and phase
    int region_debug = 0;
    float region_band = 1.5f;        // ordering band of the block's lowering sub-rounds, in patch crossings at the mean cost (0: unordered)
    int cont_raise = 4, cont_lower = 8;          // launches of that submission per phase (0: straight to the adaptive loop -- MS-DFM, whose leftovers are
                                                 // chains of 20-40 band steps, mostly invalidation: measured, config 4, 903 us per such round either way;
                                                 // sending the leftover lowering through the resident kernel instead: 1 111 us)
    int batch_margin = 1;            // replans: launches per phase = most that the last 6 replans needed + this
    float raise_margin = 0.25f;      // invalidation bound = start key + this many ordering bands (a miss costs a second round)
    int tail_grid = 96;              // replan graph: workgroups of the later launches of a phase (few tiles left)
    bool focused = true;             // stop at the start's key like the reference (end_condition)
    bool start_cell_floor = false;   // start_cell_ = the cell that contains the start position (floor) instead of Cell(Position)'s roundf (Cell.cpp:20-21): what the
                                     // revision of the reference that wrote its two recorded mission logs did (tests/test_reference_mission.py; oracle: ORC_REV_LOG)
    bool dynamic_mode = true;        // long queues: k_triage + cursor hand-out
    int grid_relax = 512;
    int dyn_grid = 256;              // workgroups of a cursor hand-out launch: the number of CUs
    int small_grid = 1 << 30;        // workgroups of a relax launch over a short queue (measured: no gain, off)
    int max_iters = 32;              // sweep cap per tile visit (x4 patch sweeps per wave): a tile that needs more is
                                     // re-queued instead of holding the whole launch (measured optimum on 4096^2)
    float delta_abs = -1.0f;         // ordering band; < 0: delta_scale * T * mean traversable cost
    float delta_scale = 1.5f;
    float delta_scale_long = 2.0f;   // ... for long queues (the plans' cursor hand-out launches): a wider band, fewer band steps
                                     // (tools/sweep.py on the final scheduler: plan 24.2 ms at 1.5, 23.6 at 2.0, 23.9 at 2.5;
                                     //  the replans' short launches are best at 1.5)
    int batch_fixed = 0;
    int profile_stride = 4;          // profiling: every n-th launch of a plan is bracketed by events
    bool defer_patches = false;      // small device patches of a batch wait for the next flush (Engine::deferred has the contract)
    bool lazy_patches = true;        // small host patches of a single planner are held for the block kernel (Engine::lazy)
    bool auto_multiplier = false;    // a step takes the census' minimum as its heuristic multiplier
};

// One row per name: the member it sets, which also says how the double is converted -- bool: value != 0; int: (int)value after the clamp
// lo .. hi, applied to the double; float: (float)value, never clamped.
constexpr double KNOB_NONE = HUGE_VAL;       // no clamp on that side
constexpr double KNOB_RTMAX = -HUGE_VAL;     // (as an upper clamp) the engine's RTMAX, which knob_set is given -- as RouteConfig is
struct KnobRow {
    const char *name;
    bool Knobs::*b = nullptr;
    int Knobs::*i = nullptr;
    float Knobs::*f = nullptr;
    double lo = -KNOB_NONE, hi = KNOB_NONE;
    constexpr KnobRow(const char *n, bool Knobs::*m) : name(n), b(m) {}
    constexpr KnobRow(const char *n, int Knobs::*m, double l = -KNOB_NONE, double h = KNOB_NONE) : name(n), i(m), lo(l), hi(h) {}
    constexpr KnobRow(const char *n, float Knobs::*m) : name(n), f(m) {}
};
constexpr KnobRow KNOB_TABLE[] = {
    {"delta", &Knobs::delta_abs},
    {"delta_scale", &Knobs::delta_scale},                  // (and delta_scale_long, and delta_abs back to "by the scale": knob_set)
    {"delta_scale_long", &Knobs::delta_scale_long},        // (and delta_abs back to "by the scale")
    {"max_iters", &Knobs::max_iters, 1},
    {"batch", &Knobs::batch_fixed, 0, 1024},
    {"pipeline_batches", &Knobs::pipeline_batches},
    {"grid", &Knobs::grid_relax, 1},
    {"small_grid", &Knobs::small_grid, 1},
    {"dyn_grid", &Knobs::dyn_grid, 1},
    {"spin_wait", &Knobs::spin_wait},
    {"fuse_control", &Knobs::fuse_control},
    {"graph", &Knobs::use_graph},
    {"region", &Knobs::use_region},
    {"owned", &Knobs::use_owned},
    {"owned_limit_ms", &Knobs::owned_limit_ms},
    {"owned_band", &Knobs::owned_band},
    {"owned_flags", &Knobs::owned_flags},
    {"owned_waves", &Knobs::owned_waves},
    {"region_debug", &Knobs::region_debug},
    {"region_band", &Knobs::region_band},
    {"region_ahead", &Knobs::region_ahead},
    {"region_tiles", &Knobs::region_tiles, 3, KNOB_RTMAX},
    {"cont_raise", &Knobs::cont_raise, 0},
    {"cont_lower", &Knobs::cont_lower, 0},
    {"region_sweeps", &Knobs::region_sweeps, 16},
    {"batch_margin", &Knobs::batch_margin},
    {"raise_margin", &Knobs::raise_margin},
    {"tail_grid", &Knobs::tail_grid, 1},
    {"profile_stride", &Knobs::profile_stride, 1},
    {"focused", &Knobs::focused},
    {"start_cell_floor", &Knobs::start_cell_floor},
    {"dynamic", &Knobs::dynamic_mode},
};

// sets the knob `name`; false: no row has that name
inline bool knob_set(Knobs &k, const char *name, double value, int rtmax) {
    if (!name) return false;
    for (const KnobRow &r : KNOB_TABLE) {
        if (std::strcmp(name, r.name)) continue;
        if (r.b) k.*r.b = value != 0;
        else if (r.f) k.*r.f = (float)value;
        else {
            const double hi = r.hi == KNOB_RTMAX ? (double)rtmax : r.hi;
            k.*r.i = value < r.lo ? (int)r.lo : (value > hi ? (int)hi : (int)value);
        }
        if (r.f == &Knobs::delta_scale) k.delta_scale_long = k.delta_scale;
        if (r.f == &Knobs::delta_scale || r.f == &Knobs::delta_scale_long) k.delta_abs = -1.0f;
        return true;
    }
    return false;
}
