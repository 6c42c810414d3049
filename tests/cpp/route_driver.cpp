// route_driver.cpp -- prints what plan_step (csrc/ufm_route.h) decides for a table of cases: the kind of step, the route of a replan and
// the placed blocks.  Stand-alone: it includes that header only.  tests/test_route.py builds it with sanitizers, runs it and compares
// the lines with what the engine's step() did before the decision was split out of it.
#include <cstdio>
#include <string>
#include <vector>

#include "ufm_route.h"

namespace {

const RouteConfig CFG{16, 8, 8, 4, 65 * 65};     // 16 x 16 tiles, blocks of <= 8 x 8 tiles, 8 jobs, 4 rectangles of <= 65 x 65 elements

struct Case {
    std::string name;
    RouteSwitches s;
    std::vector<MapState> maps;
    std::vector<PatchRect> pending;
    int n_held = 0, nr = 9, nl = 9;
};

// a planner on 208 x 208 cells; FD / SG: 209 x 209 nodes, 14 x 14 tiles; MS-DFM: 208 x 208 cells, 13 x 13 tiles, and its own block defaults
RouteSwitches fd(int nmaps = 1) { return RouteSwitches{true, true, true, true, true, 6, 2, 14, 14, nmaps}; }
RouteSwitches dfm(int nmaps = 1) { return RouteSwitches{true, true, true, true, false, 8, 3, 13, 13, nmaps}; }

MapState replanning(int gx = 200, int gy = 200) {       // has planned before, has a new start
    MapState m;
    m.initialize_search = false; m.goal_set = true; m.have_map = true; m.start_set = true; m.new_start = true;
    m.goal_ex = gx; m.goal_ey = gy; m.goal_x = (float)gx; m.goal_y = (float)gy; m.goal_elem_valid = true;
    return m;
}
MapState initialising() { MapState m = replanning(); m.initialize_search = true; return m; }
MapState idle() { MapState m = replanning(); m.new_start = false; return m; }

const char *name_of(Route r) {
    switch (r) {
        case Route::None: return "none";
        case Route::SeedsOnly: return "seeds_only";
        case Route::BlockSingle: return "block_single";
        case Route::BlockBatch: return "block_batch";
        case Route::Graph: return "graph";
        case Route::FusedChain: return "fused_chain";
        case Route::Separate: return "separate";
    }
    return "?";
}

void run(const Case &c) {
    std::vector<int> consume(c.maps.size(), -1), init(c.maps.size(), -1);
    const StepPlan p = plan_step(CFG, c.s, c.maps.data(), c.pending.data(), (int)c.pending.size(), c.n_held, c.nr, c.nl, consume.data(), init.data());
    std::printf("%s: %s init=%d upd=%d consumed=%d kept=%d fused=%d held_in_kernel=%d consume=", c.name.c_str(), name_of(p.route), p.n_init, p.n_upd,
                p.n_consumed, (int)c.pending.size() - p.n_consumed, (int)p.fused, (int)p.held_in_kernel);
    for (int v : consume) std::printf("%d", v);
    std::printf(" jobs=");
    for (int i = 0; i < p.njobs; ++i) {
        const RouteJob &j = p.job[i];
        std::printf("%s%d/%d:%d+%d,%d+%d", i ? ";" : "", j.map, j.nrect, j.tx0, j.ntx, j.ty0, j.nty);
    }
    std::printf("\n");
}

const std::vector<PatchRect> FOUR = {{0, 96, 96, 8, 8}, {0, 100, 104, 8, 8}, {0, 110, 90, 8, 8}, {0, 104, 110, 8, 8}};
std::vector<PatchRect> on_map(std::vector<PatchRect> v, int m) { for (auto &r : v) r.m = m; return v; }
std::vector<PatchRect> join(std::vector<PatchRect> a, const std::vector<PatchRect> &b) { a.insert(a.end(), b.begin(), b.end()); return a; }

}  // namespace

int main() {
    const PatchRect mid{0, 96, 96, 31, 31}, apart_a{0, 16, 16, 8, 8}, apart_b{0, 160, 160, 8, 8};
    std::vector<Case> cases;
    auto add = [&](const char *name, RouteSwitches s, std::vector<MapState> maps, std::vector<PatchRect> pending) -> Case & {
        cases.push_back(Case{name, s, std::move(maps), std::move(pending)});
        return cases.back();
    };
    // ---- a single FD planner
    add("one_patch", fd(), {replanning()}, {mid});
    add("one_patch_goal_other_side", fd(), {replanning(5, 5)}, {mid});
    add("one_patch_at_border", fd(), {replanning()}, {{0, 170, 0, 31, 31}});
    add("four_small", fd(), {replanning()}, FOUR);
    add("five_small", fd(), {replanning()}, join(FOUR, {{0, 98, 98, 8, 8}}));
    add("patch_70", fd(), {replanning()}, {{0, 60, 70, 70, 70}});
    add("two_apart", fd(), {replanning()}, {apart_a, apart_b});
    { RouteSwitches s = fd(); s.use_region = false; add("region_off", s, {replanning()}, {mid}); }
    { RouteSwitches s = fd(); s.use_region = false; add("region_off_nr_250", s, {replanning()}, {mid}).nr = 250; }
    { RouteSwitches s = fd(); s.use_region = false; add("region_off_nl_250", s, {replanning()}, {mid}).nl = 250; }
    { RouteSwitches s = fd(); s.use_region = false; s.use_graph = false; add("region_off_graph_off", s, {replanning()}, {mid}); }
    { RouteSwitches s = fd(); s.fuse_control = false; add("fuse_control_off", s, {replanning()}, {mid}); }
    { RouteSwitches s = fd(); s.spin_wait = false; add("spin_wait_off", s, {replanning()}, {mid}); }
    { RouteSwitches s = fd(); s.region_tiles = 3; add("region_tiles_3_inside", s, {replanning()}, {mid}); }
    { RouteSwitches s = fd(); s.region_tiles = 3; add("region_tiles_3_starts_a_tile_before", s, {replanning()}, {{0, 88, 88, 31, 31}}); }
    add("initialising_with_patch", fd(), {initialising()}, {mid});
    add("initialising", fd(), {initialising()}, {});
    { MapState m = replanning(); m.new_goal = true; add("new_goal_with_patch", fd(), {m}, {mid}); }
    add("new_start_only", fd(), {replanning()}, {});
    add("patch_without_new_start", fd(), {idle()}, {mid});
    add("held_block", fd(), {replanning()}, {mid}).n_held = 1;
    add("held_two_apart", fd(), {replanning()}, {apart_a, apart_b}).n_held = 2;
    add("held_initialising", fd(), {initialising()}, {mid}).n_held = 1;
    // ---- MS-DFM: 8 x 8 block, 3 tiles ahead, cells (a rectangle of h cells ends at x + h - 1)
    add("dfm_one_patch", dfm(), {replanning()}, {mid});
    add("dfm_goal_other_side", dfm(), {replanning(5, 5)}, {mid});
    add("dfm_cells_end_on_the_block_edge", dfm(), {replanning()}, {apart_a, {0, 120, 120, 8, 8}});
    { RouteSwitches s = fd(); s.region_tiles = 8; s.region_ahead = 3; add("fd_nodes_same_rectangles_end_beyond", s, {replanning()}, {apart_a, {0, 120, 120, 8, 8}}); }
    // ---- a batch of 3 maps
    const std::vector<PatchRect> two1 = {{1, 32, 32, 8, 8}, {1, 48, 40, 8, 8}};
    add("batch_1_2_4", fd(3), {replanning(), replanning(), replanning()}, join(join({{0, 96, 96, 8, 8}}, two1), on_map(FOUR, 2)));
    add("batch_map1_idle", fd(3), {replanning(), idle(), replanning()}, join(join({{0, 96, 96, 8, 8}}, two1), on_map(FOUR, 2)));
    add("batch_five_on_one_map", fd(3), {replanning(), replanning(), replanning()},
        join(join({{0, 96, 96, 8, 8}}, two1), join(on_map(FOUR, 2), {{2, 98, 98, 8, 8}})));
    add("batch_consuming_map_without_patch", fd(3), {replanning(), replanning(), replanning()}, join({{0, 96, 96, 8, 8}}, on_map(FOUR, 2)));
    { RouteSwitches s = fd(3); s.spin_wait = false; add("batch_spin_wait_off", s, {replanning(), replanning(), replanning()}, join(join({{0, 96, 96, 8, 8}}, two1), on_map(FOUR, 2))); }
    { RouteSwitches s = fd(3); s.use_region = false; add("batch_region_off", s, {replanning(), replanning(), replanning()}, join(join({{0, 96, 96, 8, 8}}, two1), on_map(FOUR, 2))); }
    {
        std::vector<MapState> nine(9, replanning());
        std::vector<PatchRect> each;
        for (int m = 0; m < 9; ++m) each.push_back({m, 96, 96, 8, 8});
        add("batch_of_9", fd(9), nine, each);
        nine.pop_back(); each.pop_back();
        add("batch_of_8", fd(8), nine, each);
    }
    add("batch_none_consuming", fd(3), {idle(), idle(), idle()}, join({{0, 96, 96, 8, 8}}, two1));
    add("batch_one_initialising", fd(3), {replanning(), initialising(), replanning()}, join({{0, 96, 96, 8, 8}}, two1));
    for (const Case &c : cases) run(c);
    return 0;
}
