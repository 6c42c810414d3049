// ufm_patch_route.h -- where a patch of the cost raster goes, decided once per patch (Engine::route_patch of ufm_map_host.h acts on the
// result): held for the replan's block kernel, deferred to the next flush, or applied now -- and then through which stages, behind which
// flushes, with how much scratch.  Plain C++17 without HIP: tests/cpp/patch_route_driver.cpp compiles this header alone.  The engine's
// constants come in through PatchRouteConfig.  DESIGN.md section 5.1 has the table.
#pragma once
#include <algorithm>
#include <cstddef>

#include "ufm_cspace_rect.h"
#include "ufm_route.h"

struct PatchRouteConfig {
    int multi;            // PATCH_MULTI: patches one deferred launch takes
    int small_cells;      // a patch of at most this many cells goes through k_patch_small, and may be deferred (4096)
    int hold_edge;        // a held host patch is at most this wide and high (64)
    int hold_slots;       // ... and there are this many pinned slots for them (4 = the rectangles a block-kernel job takes)
};

enum class PatchSource {
    Host,                 // the caller's host bytes (ufm_patch_map)
    Device,               // the caller's device pointer (ufm_patch_map_device)
    RevealSlot,           // a map's slot of the reveal buffer, made by k_reveal / k_reveal_layers
    Layer                 // a patch of layer k (ufm_patch_layer*, ufm_set_layer*): the engine composes the map's patch from it
};

struct PatchSwitches {
    bool footprint;       // ufm_set_cspace: the planning raster is the dilation of the raw store ...
    int mh, mw, ar, ac;   // ... by this mask
    bool census;          // ufm_track_costs
    int n_layers, nmaps;
    bool defer_patches, lazy_patches, use_region, fuse_control, spin_wait;
    int L, W;
    bool have_raster;     // map r.m (if there is such a map) has a raster
};
struct PatchQueue {
    int n_pending;        // rectangles waiting for a step
    int n_held;           // host patches held for the block kernel
    int n_deferred;       // device patches deferred
    bool deferred_same_map;   // ... one of them for map r.m
};
struct PatchRequest {
    PatchSource source;
    bool host_bytes;      // Layer: the bytes are in host memory (Host: always, Device / RevealSlot: never)
    int k;                // Layer: which one
    int sensor_mh, sensor_mw;   // RevealSlot: the sensor mask, which sizes the scratch of every map's slot alike
    PatchRect r;
};

enum class PatchWay { Invalid, Hold, Defer, Apply };
struct PatchPlan {
    PatchWay way;
    bool flush_held, flush_deferred;    // what is being held / deferred goes to the raster first (false also: there is nothing)
    // the stages of a patch that is not held, in the order they run; `small` / `census` only of one that is applied
    bool stage;           // host bytes through the staging buffer
    bool compose;         // into layer k, the maximum over the layers into the dense composed patch
    bool raw;             // into the raw store, the grown rectangle dilated into the scratch patch
    bool census;          // the census corrected in front of the kernel that overwrites the bytes
    bool small;           // k_patch_small; false: k_patch_apply + k_patch_seed
    PatchRect applied;    // the rectangle that reaches the planning raster: with a footprint the grown and clipped one
    size_t lcomp_bytes, cs_bytes, pmask_bytes;   // scratch: the composed patch, the dilated patch, the changed-cell mask
};

// the changed-cell mask: room for the masks of `multi` small patches (one deferred launch), or of one large patch
inline size_t patch_mask_bytes(const PatchRouteConfig &c, size_t cells) { return std::max((size_t)c.multi * (size_t)c.small_cells, cells); }

inline PatchPlan plan_patch(const PatchRouteConfig &c, const PatchSwitches &s, const PatchQueue &q, const PatchRequest &rq) {
    PatchPlan p{};
    const PatchRect &r = rq.r;
    const bool layer_call = rq.source == PatchSource::Layer;
    if (r.m < 0 || r.m >= s.nmaps || !s.have_raster) return p;
    if (r.x < 0 || r.y < 0 || r.w <= 0 || r.h <= 0 || r.x + r.h > s.L || r.y + r.w > s.W) return p;   // Graph.cpp:38-41
    if (layer_call && !(s.n_layers > 1 && rq.k >= 0 && rq.k < s.n_layers)) return p;
    const bool host = rq.source == PatchSource::Host || (layer_call && rq.host_bytes);
    p.applied = r;
    // held: the block kernel applies the bytes as they are, in order, behind the other held ones -- so no footprint (raw bytes), no
    // census (counters), no layers (one layer's bytes), and nothing else pending in between
    if (rq.source == PatchSource::Host && s.n_layers == 1 && !s.footprint && !s.census && s.lazy_patches && s.nmaps == 1 && s.use_region &&
        s.fuse_control && s.spin_wait && r.w <= c.hold_edge && r.h <= c.hold_edge && q.n_held < c.hold_slots && q.n_pending == q.n_held) {
        p.way = PatchWay::Hold;
        return p;
    }
    p.stage = host;
    p.compose = s.n_layers > 1 && rq.source != PatchSource::RevealSlot;   // (with layers a map patch is a patch of layer 0; a reveal composes itself)
    p.raw = s.footprint;
    if (s.footprint) p.applied = grow_rect(r, s.mh, s.mw, s.ar, s.ac, s.L, s.W);
    const size_t cells = (size_t)p.applied.w * (size_t)p.applied.h;
    // deferred: a pointer that stays valid (not the staging buffer, not the composed patch), bytes that are the planning raster's
    const bool defer = (rq.source == PatchSource::Device || rq.source == PatchSource::RevealSlot) && !s.footprint && s.defer_patches &&
                       !s.census && s.n_layers == 1 && s.nmaps > 1 && cells <= (size_t)c.small_cells;
    p.flush_held = q.n_held > 0;
    if (defer) {
        p.way = PatchWay::Defer;      // (one per map at a time: two patches of one map may overlap, and then their order counts)
        p.flush_deferred = q.n_deferred > 0 && (q.n_deferred >= c.multi || q.deferred_same_map);
    } else {
        p.way = PatchWay::Apply;
        p.flush_deferred = q.n_deferred > 0;
        p.census = s.census;
        p.small = cells <= (size_t)c.small_cells;
    }
    // a reveal: one size for every map's slot, the largest rectangle a slot can become -- not this map's clipped one
    size_t most = cells;
    if (rq.source == PatchSource::RevealSlot)
        most = s.footprint ? (size_t)(rq.sensor_mw + s.mw - 1) * (size_t)(rq.sensor_mh + s.mh - 1) : (size_t)rq.sensor_mw * (size_t)rq.sensor_mh;
    p.lcomp_bytes = p.compose ? (size_t)r.w * (size_t)r.h : 0;
    p.cs_bytes = s.footprint ? most : 0;
    p.pmask_bytes = patch_mask_bytes(c, most);
    return p;
}
