// cspace_driver.cpp -- prints what the host side of the C-space inflation (csrc/ufm_cspace_rect.h) computes for a table of cases: the
// rectangle of the planning raster a raw patch can change (grow_rect), the validation of a footprint and its row bit-words.
// Stand-alone: it includes that header only.  tests/test_cspace_surface.py builds it with sanitizers, runs it and compares the lines
// with values worked out by hand from the definition in include/ufm.h.
#include <cstdio>
#include <vector>

#include "ufm_cspace_rect.h"

namespace {

void grow(const char *name, PatchRect r, int mh, int mw, int ar, int ac, int L, int W) {
    const PatchRect g = grow_rect(r, mh, mw, ar, ac, L, W);
    std::printf("grow %s: m=%d x=%d y=%d w=%d h=%d\n", name, g.m, g.x, g.y, g.w, g.h);
}

void valid(const char *name, const std::vector<uint8_t> &mask, int mw, int mh, int ar, int ac) {
    CspaceMask c;
    const bool ok = cspace_pack(mask.empty() ? nullptr : mask.data(), mw, mh, ar, ac, &c);
    std::printf("mask %s: ok=%d", name, (int)ok);
    if (ok) {
        std::printf(" on=%d anchor=%d,%d rows=", (int)c.on, c.ar, c.ac);
        for (int a = 0; a < c.mh; ++a) std::printf("%s%x", a ? "," : "", c.rows[a]);
    }
    std::printf("\n");
}

}  // namespace

int main() {
    // the 3 x 5 L: a column of three with a foot of five, 10000 / 10000 / 11111
    const std::vector<uint8_t> ell = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1};
    // ---- grow_rect on a 48 x 40 map (L = 48 rows, W = 40 columns); PatchRect is {m, x = row, y = column, w, h}
    grow("ell_anchor_bottom_left", {0, 20, 10, 4, 6}, 3, 5, 2, 0, 48, 40);
    grow("ell_anchor_top_left", {0, 20, 10, 4, 6}, 3, 5, 0, 0, 48, 40);
    grow("cross_inside", {2, 20, 10, 4, 6}, 3, 3, 1, 1, 48, 40);
    grow("even_4x4_anchor_2_2", {0, 20, 10, 1, 1}, 4, 4, 2, 2, 48, 40);
    grow("top_border", {0, 0, 10, 4, 6}, 5, 5, 2, 2, 48, 40);
    grow("bottom_border", {0, 42, 10, 4, 6}, 5, 5, 2, 2, 48, 40);
    grow("left_border", {0, 20, 0, 4, 6}, 5, 5, 2, 2, 48, 40);
    grow("right_border", {0, 20, 36, 4, 6}, 5, 5, 2, 2, 48, 40);
    grow("corner", {0, 47, 39, 1, 1}, 5, 5, 2, 2, 48, 40);
    grow("corner_ell", {0, 0, 0, 1, 1}, 3, 5, 2, 0, 48, 40);
    grow("mask_31_on_20x12", {0, 5, 5, 2, 2}, 31, 31, 15, 15, 20, 12);
    // ---- validation and packing
    valid("ell_corner", ell, 5, 3, 2, 0);
    valid("ell_default_anchor_clear", ell, 5, 3, -1, -1);
    valid("one_by_one", {1}, 1, 1, -1, -1);
    valid("cross_default_anchor", {0, 1, 0, 1, 1, 1, 0, 1, 0}, 3, 3, -1, -1);
    valid("even_4x4", std::vector<uint8_t>(16, 7), 4, 4, 2, 2);
    valid("size_0", {1}, 0, 1, 0, 0);
    valid("size_0_rows", {1}, 1, 0, 0, 0);
    valid("size_32", std::vector<uint8_t>(32 * 32, 1), 32, 32, 16, 16);
    valid("size_31", std::vector<uint8_t>(31 * 31, 1), 31, 31, -1, -1);
    valid("anchor_outside", {0, 1, 0, 1, 1, 1, 0, 1, 0}, 3, 3, 3, 1);
    valid("anchor_negative", {0, 1, 0, 1, 1, 1, 0, 1, 0}, 3, 3, -1, 1);
    valid("anchor_cell_clear", {0, 1, 0, 1, 1, 1, 0, 1, 0}, 3, 3, 0, 0);
    valid("all_zero", std::vector<uint8_t>(9, 0), 3, 3, -1, -1);
    valid("null_mask", {}, 3, 3, -1, -1);
    return 0;
}
