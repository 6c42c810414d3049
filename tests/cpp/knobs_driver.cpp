// knobs_driver.cpp -- sets knobs by name through knob_set (csrc/ufm_knobs.h) and prints which members of Knobs changed, to what.
// Stand-alone: it includes that header only, and lists the members itself -- not through the header's table.  Arguments: RTMAX, then
// triples name value base; base A starts from every bool false, every int -777, every float -777.5, base B from true, 777, 777.5, so
// that any write shows.  One line per triple: "<name> <value>: ok|unknown <member>=<value> ...".
// "defaults" alone: the members of a fresh Knobs (against either base, so each shows at least once).  tests/test_knobs.py builds it with
// sanitizers and compares the lines with what the engine's strcmp chain did before the table replaced it.
#include <cstdio>
#include <cstdlib>

#include "ufm_knobs.h"

namespace {

#define KNOB_MEMBERS(B, I, F) \
    B(pipeline_batches) B(spin_wait) B(fuse_control) B(use_graph) B(use_owned) F(owned_limit_ms) F(owned_band) I(owned_flags) I(owned_waves) \
    B(dfm_follow_info) B(use_region) I(region_ahead) I(region_tiles) I(region_sweeps) I(region_debug) F(region_band) I(cont_raise) \
    I(cont_lower) I(batch_margin) F(raise_margin) I(tail_grid) B(focused) B(start_cell_floor) B(dynamic_mode) I(grid_relax) I(dyn_grid) \
    I(small_grid) I(max_iters) F(delta_abs) F(delta_scale) F(delta_scale_long) I(batch_fixed) I(profile_stride) B(defer_patches) \
    B(lazy_patches) B(auto_multiplier)

Knobs base(bool b) {
    Knobs k;
#define SET_B(m) k.m = b;
#define SET_I(m) k.m = b ? 777 : -777;
#define SET_F(m) k.m = b ? 777.5f : -777.5f;
    KNOB_MEMBERS(SET_B, SET_I, SET_F)
    return k;
}

void print_changes(const Knobs &was, const Knobs &is) {
#define SHOW_B(m) if (was.m != is.m) std::printf(" " #m "=%d", is.m ? 1 : 0);
#define SHOW_I(m) if (was.m != is.m) std::printf(" " #m "=%d", is.m);
#define SHOW_F(m) if (was.m != is.m) std::printf(" " #m "=%g", (double)is.m);
    KNOB_MEMBERS(SHOW_B, SHOW_I, SHOW_F)
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && argv[1][0] == 'd') {        // "defaults": every member of a fresh Knobs
        print_changes(base(false), Knobs{});
        print_changes(base(true), Knobs{});
        std::printf("\n");
        return 0;
    }
    if (argc < 2 || (argc - 2) % 3) return 2;
    const int rtmax = std::atoi(argv[1]);
    for (int a = 2; a < argc; a += 3) {
        const Knobs was = base(argv[a + 2][0] == 'B');
        Knobs k = was;
        const bool ok = knob_set(k, argv[a], std::atof(argv[a + 1]), rtmax);
        std::printf("%s %s: %s", argv[a], argv[a + 1], ok ? "ok" : "unknown");
        print_changes(was, k);
        std::printf("\n");
    }
    Knobs k;
    return knob_set(k, nullptr, 1.0, rtmax) ? 3 : 0;       // no name: unknown
}
