// ufm_route.h -- what a step is and which way it goes to the device, decided once per step (Engine::step acts on the result).
// Plain C++17 without HIP: tests/cpp/route_driver.cpp compiles this header alone.  The engine's constants come in through RouteConfig.
#pragma once
#include <algorithm>
#include <climits>

struct PatchRect { int m, x, y, w, h; };

struct MapState {
    bool initialize_search = true;   // ReplannerBase.h:149
    bool goal_set = false;           // :150
    bool new_goal = false;           // :151
    bool new_start = false;          // :152
    bool have_map = false;           // !initialize_graph :148
    bool start_set = false;
    float start_x = 0, start_y = 0, goal_x = 0, goal_y = 0;
    int goal_ex = 0, goal_ey = 0;    // Node()/Cell() of the goal
    bool goal_elem_valid = false;
};

// the kernels' argument layout of a rectangle: {map, x, y, w, h}
inline void put_rect(int *q, const PatchRect &r) { q[0] = r.m; q[1] = r.x; q[2] = r.y; q[3] = r.w; q[4] = r.h; }

struct RouteConfig {
    int tile;             // T
    int rtmax;            // RTMAX: largest block edge in tiles
    int rjobs;            // RJOBS: jobs of one block-kernel launch
    int max_rects;        // rectangles a block-kernel job / a fused replan takes (4)
    int max_rect_elems;   // ... each of at most this many elements (65 x 65)
};
struct RouteSwitches {
    bool fuse_control, spin_wait, use_region, use_graph;
    bool nodes;           // FD / SG: node planners; MS-DFM: cells
    int region_tiles, region_ahead;
    int TX, TY, nmaps;
};

enum class Route {
    None,            // nothing to propagate from: no seeds (a plain initialisation still plans)
    SeedsOnly,       // initialising maps with pending patches: the seeds go to the queue, the adaptive rounds plan
    BlockSingle,     // replan, one map: k_replan_region on the block around the patches (it applies held host patches itself)
    BlockBatch,      // replan, a batch: one block-kernel job per consuming map
    Graph,           // replan: the fused submission replayed as one captured graph
    FusedChain,      // replan: k_replan_begin / k_raise_to_lower / k_replan_end around blind batches of launches
    Separate         // replan: the control steps as separate launches
};
constexpr int ROUTE_MAX_JOBS = 8, ROUTE_MAX_RECTS = 4;
struct RouteJob { int map, nrect; int rect[ROUTE_MAX_RECTS][5]; int tx0, ntx, ty0, nty; };
struct StepPlan {
    Route route;
    int n_init, n_upd;        // maps that (re)initialise / that propagate pending patches
    int n_consumed;           // pending rectangles this step consumes (the others are kept)
    bool have_seeds, fused;
    bool held_in_kernel;      // held host patches are applied inside the block kernel (otherwise before the step)
    int njobs;                // block-kernel routes: the placed blocks
    RouteJob job[ROUTE_MAX_JOBS];
};

// the block of the replan kernel around a set of consumed rectangles {map, x, y, w, h}: its goal-side edge `region_ahead` tiles beyond the
// rectangles' centre, the rest of its extent behind it -- where the elements that lean on the patched cells are; false if they do not fit into one block
inline bool region_fits(const RouteConfig &c, const RouteSwitches &s, const MapState &ms, const int (*rects)[5], int nrect,
                        int *tx0, int *ntx, int *ty0, int *nty) {
    if (nrect <= 0) return false;
    const int T = c.tile;
    int ex0 = INT_MAX, ex1 = -1, ey0 = INT_MAX, ey1 = -1;
    for (int r = 0; r < nrect; ++r) {
        const int *qr = rects[r];
        ex0 = std::min(ex0, qr[1]); ex1 = std::max(ex1, qr[1] + qr[4] - (s.nodes ? 0 : 1));
        ey0 = std::min(ey0, qr[2]); ey1 = std::max(ey1, qr[2] + qr[3] - (s.nodes ? 0 : 1));
    }
    auto place = [&](int e0, int e1, int goal_e, int ntiles_map, int *t0, int *nt) {
        *nt = std::min(std::min(s.region_tiles, c.rtmax), ntiles_map);
        const int tc = ((e0 + e1) / 2) / T;
        int lo = (goal_e >= (e0 + e1) / 2) ? tc + s.region_ahead - *nt + 1 : tc - s.region_ahead;
        lo = std::max(0, std::min(lo, ntiles_map - *nt));
        *t0 = lo;
        return e0 / T >= lo && e1 / T <= lo + *nt - 1;      // every consumed rectangle inside the block
    };
    const bool okx = place(ex0, ex1, ms.goal_ex, s.TX, tx0, ntx);
    const bool oky = place(ey0, ey1, ms.goal_ey, s.TY, ty0, nty);
    return okx && oky;
}

// What the step is (ReplannerBase.h:48-59) and, for a replan, its route.  consume[nmaps] / init[nmaps] are filled per map; nothing else
// is written, nothing is enqueued.  n_held: host patches being held (the last rectangles of `pending`); nr / nl: the blind batch sizes.
inline StepPlan plan_step(const RouteConfig &c, const RouteSwitches &s, const MapState *maps, const PatchRect *pending, int npending,
                          int n_held, int nr, int nl, int *consume, int *init) {
    StepPlan p{};
    for (int m = 0; m < s.nmaps; ++m) {
        init[m] = (maps[m].initialize_search || maps[m].new_goal) ? 1 : 0;
        consume[m] = (init[m] || maps[m].new_start) ? 1 : 0;
        if (init[m]) ++p.n_init; else if (consume[m]) ++p.n_upd;
    }
    const bool single = s.nmaps == 1;
    auto small = [&](const PatchRect &r) { return (r.w + 1) * (r.h + 1) <= c.max_rect_elems; };
    // replan of a single map with a few small pending patches: the control steps run fused
    p.fused = single && s.fuse_control && s.spin_wait && p.n_init == 0 && p.n_upd > 0 && npending > 0 && npending <= c.max_rects;
    for (int i = 0; i < npending && p.fused; ++i) p.fused = consume[pending[i].m] && small(pending[i]);
    for (int i = 0; i < npending; ++i) if (consume[pending[i].m]) ++p.n_consumed;
    p.have_seeds = p.n_consumed > 0;
    if (!p.have_seeds) { p.route = Route::None; return p; }
    if (!(p.n_init == 0 && p.n_upd > 0)) { p.route = Route::SeedsOnly; return p; }
    // the rectangles map m consumes, as one job; false: more or larger ones than a job takes
    auto collect = [&](RouteJob &j, int m) {
        j = RouteJob{};
        j.map = m;
        for (int i = 0; i < npending; ++i) {
            const PatchRect &r = pending[i];
            if (r.m != m || !consume[m]) continue;
            if (j.nrect >= c.max_rects || !small(r)) return false;
            put_rect(j.rect[j.nrect++], r);
        }
        return true;
    };
    auto fits = [&](RouteJob &j) { return region_fits(c, s, maps[j.map], j.rect, j.nrect, &j.tx0, &j.ntx, &j.ty0, &j.nty); };
    bool regioned = false;
    if (p.fused && s.use_region) {                       // one map, a few small patches
        p.njobs = 1;
        regioned = collect(p.job[0], 0) && fits(p.job[0]);
    } else if (!single && s.use_region && s.spin_wait && s.nmaps <= c.rjobs && s.nmaps <= ROUTE_MAX_JOBS) {
        // a batch: one job per consuming map, every one of them with 1..4 small rectangles of its own
        bool ok = true;
        for (int m = 0; m < s.nmaps && ok; ++m) {
            if (!consume[m]) continue;
            RouteJob &j = p.job[p.njobs++];
            ok = collect(j, m) && fits(j);
        }
        regioned = ok && p.njobs > 0;
    }
    if (regioned) p.route = single ? Route::BlockSingle : Route::BlockBatch;
    else if (p.fused && s.use_graph && nr < 250 && nl < 250) p.route = Route::Graph;
    else p.route = p.fused ? Route::FusedChain : Route::Separate;
    if (!regioned) p.njobs = 0;
    p.held_in_kernel = n_held > 0 && p.route == Route::BlockSingle;
    return p;
}
