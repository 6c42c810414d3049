// ufm_cspace_rect.h -- the footprint of ufm_set_cspace as the host handles it: validation, the row bit-words the dilation kernel takes,
// and the rectangle of the planning raster a raw patch can change.  Plain C++17 without HIP: tests/cpp/cspace_driver.cpp compiles this
// header alone (with ufm_route.h for PatchRect).
//
// One definition (include/ufm.h): mask[mh][mw] row-major, non-zero = set, anchor (ar, ac);
//     planning[i][j] = max { raw[i + a - ar][j + b - ac] : mask[a][b] != 0, the raw index inside the map }
#pragma once
#include <cstdint>

#include "ufm_route.h"

constexpr int CSPACE_MAX = 31;       // largest footprint edge: a row of the mask is one 32-bit word

struct CspaceMask {
    int mw = 1, mh = 1, ar = 0, ac = 0;
    uint32_t rows[CSPACE_MAX] = {1u};   // bit b of rows[a]: mask[a][b] is set
    bool on = false;                    // false: 1 x 1, planning raster == raw raster, nothing of the feature runs
};

// The anchor an (-1, -1) stands for: the centre as OpenCV's getStructuringElement / dilate place it.
inline void cspace_default_anchor(int mw, int mh, int *ar, int *ac) {
    if (*ar == -1 && *ac == -1) { *ar = mh / 2; *ac = mw / 2; }
}

// 1 <= mw, mh <= 31, the anchor inside the mask, the anchor cell set (so the max is never empty and planning >= raw)
inline bool cspace_valid(const uint8_t *mask, int mw, int mh, int ar, int ac) {
    if (!mask || mw < 1 || mh < 1 || mw > CSPACE_MAX || mh > CSPACE_MAX) return false;
    cspace_default_anchor(mw, mh, &ar, &ac);
    if (ar < 0 || ac < 0 || ar >= mh || ac >= mw) return false;
    return mask[ar * mw + ac] != 0;
}

// false: not a valid footprint, *out untouched
inline bool cspace_pack(const uint8_t *mask, int mw, int mh, int ar, int ac, CspaceMask *out) {
    if (!cspace_valid(mask, mw, mh, ar, ac)) return false;
    cspace_default_anchor(mw, mh, &ar, &ac);
    CspaceMask c;
    c.mw = mw; c.mh = mh; c.ar = ar; c.ac = ac;
    for (int a = 0; a < CSPACE_MAX; ++a) c.rows[a] = 0;
    for (int a = 0; a < mh; ++a)
        for (int b = 0; b < mw; ++b)
            if (mask[a * mw + b]) c.rows[a] |= 1u << b;
    c.on = !(mw == 1 && mh == 1);
    *out = c;
    return true;
}

// The cells of the planning raster that read a raw cell of r (rows r.x .. r.x+r.h-1, columns r.y .. r.y+r.w-1 of an L x W map): a raw
// change at row c reaches the outputs c - a + ar, a = 0 .. mh-1 -- the extent of the mask REFLECTED about its anchor --, clipped to the map.
inline PatchRect grow_rect(const PatchRect &r, int mh, int mw, int ar, int ac, int L, int W) {
    const int x0 = r.x - (mh - 1 - ar) < 0 ? 0 : r.x - (mh - 1 - ar);
    const int y0 = r.y - (mw - 1 - ac) < 0 ? 0 : r.y - (mw - 1 - ac);
    const int x1 = r.x + r.h - 1 + ar > L - 1 ? L - 1 : r.x + r.h - 1 + ar;
    const int y1 = r.y + r.w - 1 + ac > W - 1 ? W - 1 : r.y + r.w - 1 + ac;
    return PatchRect{r.m, x0, y0, y1 - y0 + 1, x1 - x0 + 1};
}
