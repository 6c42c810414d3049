// ufm_cspace_graded_rect.h -- the graded footprint of ufm_set_cspace_graded as the host handles it: validation, the grouping of its cells
// by drop value into the levels the dilation kernel takes, and the cone of ufm_cspace_cone.  Plain C++17 without HIP:
// tests/cpp/graded_driver.cpp compiles this header alone (with ufm_cspace_rect.h, whose CspaceMask and grow_rect it keeps using).
//
// One definition (include/ufm_cspace_graded.h): drop[mh][mw] row-major, 255 = not a cell of the footprint, anchor (ar, ac);
//     planning[i][j] = max { max(raw[i + a - ar][j + b - ac] - drop[a][b], 0) : drop[a][b] != 255, the raw index inside the map }
// Grouped by level -- the cells that share one drop d_l --:  max over l of max(m_l - d_l, 0), m_l the plain maximum of raw over the
// cells of level l.  Exact: x -> max(x - d, 0) is monotone, so it commutes with the maximum over a level's cells, and with no cell of
// a level inside the map m_l = 0 gives 0, the identity of the outer maximum.
#pragma once
#include <cstdint>

#include "ufm_cspace_rect.h"

constexpr int CSPACE_OUTSIDE = 255;       // UFM_CSPACE_OUTSIDE
constexpr int CSPACE_MAX_LEVELS = 16;     // UFM_CSPACE_MAX_LEVELS

struct CspaceLevels {
    int n = 0;                                              // 0 or 1: flat -- the support alone says everything, k_cspace_dilate runs
    uint8_t drop[CSPACE_MAX_LEVELS] = {};                   // ascending: drop[0] == 0, the level that holds the anchor
    uint32_t rows[CSPACE_MAX_LEVELS][CSPACE_MAX] = {};      // bit b of rows[l][a]: drop[a][b] == drop[l]; their union is CspaceMask::rows
};

// drop non-NULL, 1 <= mw, mh <= 31, the anchor inside the matrix with drop 0 (so planning >= raw), at most 16 distinct values below 255
inline bool cspace_graded_valid(const uint8_t *drop, int mw, int mh, int ar, int ac) {
    if (!drop || mw < 1 || mh < 1 || mw > CSPACE_MAX || mh > CSPACE_MAX) return false;
    cspace_default_anchor(mw, mh, &ar, &ac);
    if (ar < 0 || ac < 0 || ar >= mh || ac >= mw) return false;
    if (drop[ar * mw + ac] != 0) return false;
    bool seen[CSPACE_OUTSIDE] = {};
    int n = 0;
    for (int e = 0; e < mw * mh; ++e)
        if (drop[e] != CSPACE_OUTSIDE && !seen[drop[e]]) { seen[drop[e]] = true; ++n; }
    return n <= CSPACE_MAX_LEVELS;
}

// false: not a valid footprint, *support and *levels untouched.  The support -- every cell with a drop below 255 -- in the flat mask's
// format (what cspace_pack makes of the mask drop != 255), the levels sorted by drop.
inline bool cspace_graded_pack(const uint8_t *drop, int mw, int mh, int ar, int ac, CspaceMask *support, CspaceLevels *levels) {
    if (!cspace_graded_valid(drop, mw, mh, ar, ac)) return false;
    cspace_default_anchor(mw, mh, &ar, &ac);
    CspaceMask c;
    c.mw = mw; c.mh = mh; c.ar = ar; c.ac = ac;
    for (int a = 0; a < CSPACE_MAX; ++a) c.rows[a] = 0;
    int level_of[CSPACE_OUTSIDE];
    for (int v = 0; v < CSPACE_OUTSIDE; ++v) level_of[v] = -1;
    for (int e = 0; e < mw * mh; ++e) if (drop[e] != CSPACE_OUTSIDE) level_of[drop[e]] = 0;
    CspaceLevels s;
    for (int v = 0; v < CSPACE_OUTSIDE; ++v)
        if (level_of[v] == 0) { level_of[v] = s.n; s.drop[s.n++] = (uint8_t)v; }
    for (int a = 0; a < mh; ++a)
        for (int b = 0; b < mw; ++b) {
            const int v = drop[a * mw + b];
            if (v == CSPACE_OUTSIDE) continue;
            c.rows[a] |= 1u << b;
            s.rows[level_of[v]][a] |= 1u << b;
        }
    c.on = !(mw == 1 && mh == 1);
    *support = c;
    *levels = s;
    return true;
}

// ufm_cspace_cone: r_in = inner_d / 2, r_out = outer_d / 2, n = 2 r_out + 1; at offset (dx, dy) from the centre, d2 = dx^2 + dy^2:
// d2 <= r_in^2: 0; d2 <= r_out^2: min(254, step * k), k the smallest integer >= 1 with d2 <= (r_in + k)^2; beyond: 255.  Integers throughout.
inline bool cspace_cone(int inner_d, int outer_d, int step, uint8_t *drop) {
    if (!drop || inner_d < 1 || inner_d > outer_d || step < 1 || step > 254) return false;
    const int r_in = inner_d / 2, r_out = outer_d / 2, n = 2 * r_out + 1;
    if (r_out > CSPACE_MAX / 2 || r_out - r_in > CSPACE_MAX_LEVELS - 1) return false;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const int d2 = (a - r_out) * (a - r_out) + (b - r_out) * (b - r_out);
            int v = CSPACE_OUTSIDE;
            if (d2 <= r_in * r_in) v = 0;
            else if (d2 <= r_out * r_out) {
                int k = 1;
                while (d2 > (r_in + k) * (r_in + k)) ++k;
                v = step * k > 254 ? 254 : step * k;
            }
            drop[a * n + b] = (uint8_t)v;
        }
    return true;
}
