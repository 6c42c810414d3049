// graded_driver.cpp -- prints what the host side of the graded footprint (csrc/ufm_cspace_graded_rect.h) computes for a table of cases:
// the validation of a footprint, its support in the flat mask's format, and its levels -- drop and row bit-words, sorted by drop.
// Stand-alone: it includes that header only (which brings ufm_cspace_rect.h).  tests/test_cspace_graded_surface.py builds it with
// sanitizers, runs it and compares the lines with values worked out by hand from the definition in include/ufm_cspace_graded.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ufm_cspace_graded_rect.h"

namespace {

void rows(const uint32_t *r, int mh) {
    for (int a = 0; a < mh; ++a) std::printf("%s%x", a ? "," : "", r[a]);
}

void graded(const char *name, const std::vector<uint8_t> &drop, int mw, int mh, int ar, int ac) {
    CspaceMask c;
    CspaceLevels s;
    const bool ok = cspace_graded_pack(drop.empty() ? nullptr : drop.data(), mw, mh, ar, ac, &c, &s);
    std::printf("graded %s: ok=%d", name, (int)ok);
    if (ok) {
        // the union of the levels is the support, over all 31 row words, and no cell is in two levels
        bool uni = true, disjoint = true;
        for (int a = 0; a < CSPACE_MAX; ++a) {
            uint32_t u = 0;
            for (int l = 0; l < s.n; ++l) { disjoint = disjoint && !(u & s.rows[l][a]); u |= s.rows[l][a]; }
            uni = uni && u == c.rows[a];
        }
        std::printf(" on=%d anchor=%d,%d levels=%d support=", (int)c.on, c.ar, c.ac, s.n);
        rows(c.rows, c.mh);
        std::printf(" union=%d disjoint=%d", (int)uni, (int)disjoint);
        for (int l = 0; l < s.n; ++l) { std::printf(" d%d=", (int)s.drop[l]); rows(s.rows[l], c.mh); }
    }
    std::printf("\n");
}

// drops in {0, 255}: one level, and everything cspace_pack makes of the mask drop != 255
void flat(const char *name, const std::vector<uint8_t> &drop, int mw, int mh, int ar, int ac) {
    std::vector<uint8_t> mask(drop.size());
    for (size_t e = 0; e < drop.size(); ++e) mask[e] = drop[e] != 255;
    CspaceMask c, f;
    CspaceLevels s;
    const bool ok = cspace_graded_pack(drop.data(), mw, mh, ar, ac, &c, &s) && cspace_pack(mask.data(), mw, mh, ar, ac, &f);
    const bool same = ok && s.n == 1 && s.drop[0] == 0 && c.mw == f.mw && c.mh == f.mh && c.ar == f.ar && c.ac == f.ac && c.on == f.on &&
                      !std::memcmp(c.rows, f.rows, sizeof(f.rows)) && !std::memcmp(s.rows[0], f.rows, sizeof(f.rows));
    std::printf("flat %s: ok=%d same=%d on=%d\n", name, (int)ok, (int)same, (int)c.on);
}

}  // namespace

int main() {
    const uint8_t O = 255;
    std::vector<uint8_t> ramp17(17), ramp16(16);
    for (int b = 0; b < 17; ++b) ramp17[b] = (uint8_t)b;
    for (int b = 0; b < 16; ++b) ramp16[b] = (uint8_t)b;
    graded("anchor_drop_nonzero", {0, 0, 0, 0, 10, 0, 0, 0, 0}, 3, 3, -1, -1);
    graded("levels_17", ramp17, 17, 1, 0, 0);
    graded("levels_16", ramp16, 16, 1, 0, 0);
    graded("levels_16_and_outside", {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, O, O}, 18, 1, 0, 0);
    graded("size_0", {0}, 0, 1, 0, 0);
    graded("size_0_rows", {0}, 1, 0, 0, 0);
    graded("size_32", std::vector<uint8_t>(32 * 32, 0), 32, 32, 16, 16);
    graded("size_31", std::vector<uint8_t>(31 * 31, 0), 31, 31, -1, -1);
    graded("anchor_outside", std::vector<uint8_t>(9, 0), 3, 3, 3, 1);
    graded("anchor_negative", std::vector<uint8_t>(9, 0), 3, 3, -1, 1);
    graded("anchor_is_outside_cell", {0, 0, 0, 0, O, 0, 0, 0, 0}, 3, 3, -1, -1);
    graded("null_drop", {}, 3, 3, -1, -1);
    graded("one_by_one", {0}, 1, 1, -1, -1);
    // the 3 x 5 L of the flat tests as drops in {0, 255}, anchor in its corner; and the full 4 x 4 block
    const std::vector<uint8_t> ell = {0, O, O, O, O, 0, O, O, O, O, 0, 0, 0, 0, 0};
    graded("ell_flat", ell, 5, 3, 2, 0);
    flat("ell_flat", ell, 5, 3, 2, 0);
    flat("block_4x4", std::vector<uint8_t>(16, 0), 4, 4, 2, 2);
    flat("one_by_one", {0}, 1, 1, -1, -1);
    // the cone of inner diameter 1, outer 5, step 40: 0 at the centre, 40 at distance 1, 80 up to distance 2
    graded("cone_5x5_two_rings", {O, O,  80, O,  O,
                                  O, 80, 40, 80, O,
                                  80, 40, 0, 40, 80,
                                  O, 80, 40, 80, O,
                                  O, O,  80, O,  O}, 5, 5, -1, -1);
    // not monotone: full cost straight up and at the lower left corner, less at the sides, a hole below
    graded("non_monotone", {50, 0, 50,
                            20, 0, 20,
                            0,  O, 10}, 3, 3, -1, -1);
    // the L with a drop per cell, anchor in its corner
    graded("ell_graded", {60, O,  O,  O,  O,
                          30, O,  O,  O,  O,
                          0,  25, 50, 75, 100}, 5, 3, 2, 0);
    return 0;
}
