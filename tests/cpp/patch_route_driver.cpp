// patch_route_driver.cpp -- prints what plan_patch (csrc/ufm_patch_route.h) decides for a table of cases: the way of a patch, what is
// flushed in front of it, its stages, the rectangle that reaches the planning raster and the scratch it needs.  Stand-alone: it includes
// that header only.  tests/test_patch_route.py builds it with sanitizers, runs it and compares the lines with what the engine's patch
// functions did before the decision was split out of them.
#include <cstdio>
#include <string>
#include <vector>

#include "ufm_patch_route.h"

namespace {

const PatchRouteConfig CFG{16, 4096, 64, 4};     // 16 patches per deferred launch, small: <= 4096 cells, held: <= 64 x 64 in 4 slots

struct Case {
    std::string name;
    PatchSwitches s;
    PatchQueue q;
    PatchRequest rq;
};

// a planner (or a batch) on 208 x 208 cells, every switch at its default
PatchSwitches planner(int nmaps = 1, int edge = 208) {
    return PatchSwitches{false, 1, 1, 0, 0, false, 1, nmaps, false, true, true, true, true, edge, edge, true};
}
PatchSwitches with_footprint(PatchSwitches s, int edge) { s.footprint = true; s.mh = s.mw = edge; s.ar = s.ac = edge / 2; return s; }
PatchSwitches deferring(int nmaps = 4) { PatchSwitches s = planner(nmaps); s.defer_patches = true; return s; }
const PatchQueue EMPTY{0, 0, 0, false};
PatchRequest from(PatchSource src, PatchRect r) { return PatchRequest{src, false, 0, 0, 0, r}; }
PatchRequest host(PatchRect r) { return from(PatchSource::Host, r); }
PatchRequest device(PatchRect r) { return from(PatchSource::Device, r); }
PatchRequest slot(PatchRect r) { PatchRequest q = from(PatchSource::RevealSlot, r); q.sensor_mh = q.sensor_mw = 7; return q; }
PatchRequest layer(int k, PatchRect r) { PatchRequest q = from(PatchSource::Layer, r); q.k = k; return q; }

void run(const Case &c) {
    const PatchPlan p = plan_patch(CFG, c.s, c.q, c.rq);
    std::printf("%s: ", c.name.c_str());
    if (p.way == PatchWay::Invalid) { std::printf("invalid\n"); return; }
    std::printf("%s first=%s stages=", p.way == PatchWay::Hold ? "hold" : (p.way == PatchWay::Defer ? "defer" : "apply"),
                p.flush_held ? (p.flush_deferred ? "held+deferred" : "held") : (p.flush_deferred ? "deferred" : "-"));
    std::string st;
    if (p.stage) st += "stage+";
    if (p.compose) st += "compose+";
    if (p.raw) st += "raw+";
    if (p.census) st += "census+";
    if (p.way == PatchWay::Apply) st += p.small ? "small" : "large";
    if (!st.empty() && st.back() == '+') st.pop_back();
    if (st.empty()) st = "-";
    std::printf("%s rect=%d,%d,%d,%d scratch=%zu/%zu/%zu\n", st.c_str(), p.applied.x, p.applied.y, p.applied.w, p.applied.h,
                p.lcomp_bytes, p.cs_bytes, p.pmask_bytes);
}

}  // namespace

int main() {
    const PatchRect mid{0, 96, 96, 31, 31}, tiny{0, 100, 100, 8, 8};
    std::vector<Case> cases;
    auto add = [&](const char *name, PatchSwitches s, PatchQueue q, PatchRequest rq) { cases.push_back(Case{name, s, q, rq}); };
    // ---- host patches of a single planner
    add("host_31", planner(), EMPTY, host(mid));
    { PatchSwitches s = planner(); s.use_region = false; add("host_31_region_off", s, EMPTY, host(mid)); }
    { PatchSwitches s = planner(); s.spin_wait = false; add("host_31_spin_wait_off", s, EMPTY, host(mid)); }
    { PatchSwitches s = planner(); s.lazy_patches = false; add("host_31_lazy_off", s, EMPTY, host(mid)); }
    add("host_65x20", planner(), EMPTY, host({0, 96, 96, 65, 20}));
    add("host_64_three_held", planner(), PatchQueue{3, 3, 0, false}, host({0, 96, 96, 64, 64}));
    add("host_64_four_held", planner(), PatchQueue{4, 4, 0, false}, host({0, 96, 96, 64, 64}));
    add("host_small_behind_one_not_held", planner(), PatchQueue{1, 0, 0, false}, host(tiny));
    { PatchSwitches s = planner(); s.census = true; add("host_small_census", s, EMPTY, host(tiny)); }
    // ---- a 5 x 5 footprint, anchor (2, 2)
    add("footprint_interior", with_footprint(planner(), 5), EMPTY, host(tiny));
    add("footprint_corner", with_footprint(planner(), 5), EMPTY, host({0, 0, 0, 8, 8}));
    // ---- the large form, the mask
    add("device_70", planner(), EMPTY, device({0, 60, 70, 70, 70}));
    add("device_300", planner(1, 512), EMPTY, device({0, 100, 100, 300, 300}));
    // ---- a batch of 4 with defer_patches on
    add("batch_device_31", deferring(), EMPTY, device({1, 96, 96, 31, 31}));
    add("batch_same_map_deferred", deferring(), PatchQueue{1, 0, 1, true}, device({1, 96, 96, 31, 31}));
    add("batch_other_map_deferred", deferring(), PatchQueue{1, 0, 1, false}, device({1, 96, 96, 31, 31}));
    add("batch_16_deferred", deferring(32), PatchQueue{16, 0, 16, false}, device({20, 96, 96, 31, 31}));
    { PatchSwitches s = deferring(); s.census = true; add("batch_census", s, EMPTY, device({1, 96, 96, 31, 31})); }
    add("batch_host", deferring(), PatchQueue{2, 0, 2, false}, host({1, 96, 96, 31, 31}));
    add("batch_64x65", deferring(), EMPTY, device({1, 96, 96, 64, 65}));
    add("batch_footprint", with_footprint(deferring(), 5), EMPTY, device({1, 96, 96, 31, 31}));
    add("batch_reveal_slot", deferring(), EMPTY, slot({1, 50, 50, 7, 7}));
    { PatchSwitches s = deferring(); s.n_layers = 2; add("batch_reveal_slot_two_layers", s, EMPTY, slot({1, 50, 50, 7, 7})); }
    add("batch_defer_off", planner(4), EMPTY, device({1, 96, 96, 31, 31}));
    // ---- a reveal's scratch: the 7 x 7 sensor at cell (0, 0), clipped to 4 x 4, with a 3 x 3 footprint
    add("reveal_slot_footprint_corner", with_footprint(planner(), 3), EMPTY, slot({0, 0, 0, 4, 4}));
    // ---- two layers
    { PatchSwitches s = planner(); s.n_layers = 2; add("layers_host_map_patch", s, EMPTY, host(mid)); }
    { PatchSwitches s = with_footprint(planner(), 5); s.n_layers = 2; add("layers_layer1_footprint", s, EMPTY, layer(1, mid)); }
    { PatchSwitches s = planner(); s.n_layers = 2; PatchRequest q = layer(1, mid); q.host_bytes = true; add("layers_layer1_host_bytes", s, EMPTY, q); }
    // ---- invalid
    add("invalid_w_0", planner(), EMPTY, host({0, 96, 96, 0, 31}));
    add("invalid_x_h_beyond_L", planner(), EMPTY, host({0, 200, 96, 8, 10}));
    add("invalid_y_w_beyond_W", planner(), EMPTY, device({0, 96, 200, 10, 8}));
    add("invalid_map_index", planner(), EMPTY, host({1, 96, 96, 8, 8}));
    { PatchSwitches s = planner(); s.have_raster = false; add("invalid_no_raster", s, EMPTY, device(tiny)); }
    { PatchSwitches s = planner(); s.n_layers = 2; add("invalid_layer_2_of_2", s, EMPTY, layer(2, mid)); }
    add("invalid_layer_call_one_layer", planner(), EMPTY, layer(0, mid));
    for (const Case &c : cases) run(c);
    return 0;
}
