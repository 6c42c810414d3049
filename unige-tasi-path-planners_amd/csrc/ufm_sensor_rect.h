// ufm_sensor_rect.h -- the sensor reveal (ufm_set_sensor / ufm_reveal) as far as it is index arithmetic: validating a field-of-view mask,
// placing its bounding rectangle R on a centre cell and clipping it to the map, which element of the dense patch Q a lane of k_reveal
// makes and which cells of the raster and of the mask that element stands for, where a map's slot lies in the engine's patch buffer and
// how many workgroups a launch takes.  Plain C++17, with or without HIP: k_reveal (ufm_sensor.h) calls these functions and
// tests/cpp/sensor_driver.cpp runs them lane by lane on the host against a brute-force loop.
//
// One definition (include/ufm.h): mask[mh][mw] row-major, non-zero = seen, anchor (ar, ac), NOT reflected --
//     mask cell (a, b) covers map cell (row + a - ar, col + b - ac) of a reveal at (row, col);
//     Q[i][j] = survey[i][j] where the mask covers (i, j), the caller's raster as it stands elsewhere, over R.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define SENSOR_HD __host__ __device__
#else
#define SENSOR_HD
#endif

constexpr int SENSOR_MAX = 127;         // largest mask edge
constexpr int SENSOR_THREADS = 256;     // per workgroup: four waves, one element of Q per lane

struct SensorShape {
    int mw = 0, mh = 0, ar = 0, ac = 0;
    bool set = false;                   // false: no sensor, nothing of the feature exists or runs
};

// The anchor an (-1, -1) stands for: the centre, as ufm_set_cspace places it.
inline void sensor_default_anchor(int mw, int mh, int *ar, int *ac) {
    if (*ar == -1 && *ac == -1) { *ar = mh / 2; *ac = mw / 2; }
}

// 1 <= mw, mh <= 127, the anchor inside the mask, at least one cell set (the anchor cell need not be)
inline bool sensor_valid(const uint8_t *mask, int mw, int mh, int ar, int ac) {
    if (!mask || mw < 1 || mh < 1 || mw > SENSOR_MAX || mh > SENSOR_MAX) return false;
    sensor_default_anchor(mw, mh, &ar, &ac);
    if (ar < 0 || ac < 0 || ar >= mh || ac >= mw) return false;
    for (int k = 0; k < mw * mh; ++k) if (mask[k]) return true;
    return false;
}
// false: not a valid mask, *out untouched
inline bool sensor_pack(const uint8_t *mask, int mw, int mh, int ar, int ac, SensorShape *out) {
    if (!sensor_valid(mask, mw, mh, ar, ac)) return false;
    sensor_default_anchor(mw, mh, &ar, &ac);
    SensorShape s;
    s.mw = mw; s.mh = mh; s.ar = ar; s.ac = ac; s.set = true;
    *out = s;
    return true;
}

// a centre a reveal accepts: a cell of the L x W map
SENSOR_HD inline bool sensor_centre_ok(int row, int col, int L, int W) { return row >= 0 && col >= 0 && row < L && col < W; }

// R: rows x .. x+h-1, columns y .. y+w-1 (the order of Graph::update and ufm_patch_map: x, y, w, h), and the mask cell (a0, b0) that
// lies on its first cell -- (0, 0) unless the top or the left border cut the mask.  With the centre inside the map and the anchor inside
// the mask R holds the centre cell: w, h >= 1.
struct SensorRect { int x, y, w, h, a0, b0; };
SENSOR_HD inline SensorRect sensor_place(int row, int col, int mh, int mw, int ar, int ac, int L, int W) {
    const int x0 = row - ar, y0 = col - ac;                   // where mask cell (0, 0) falls
    const int x1 = x0 + mh - 1 > L - 1 ? L - 1 : x0 + mh - 1, y1 = y0 + mw - 1 > W - 1 ? W - 1 : y0 + mw - 1;
    SensorRect r;
    r.x = x0 < 0 ? 0 : x0; r.y = y0 < 0 ? 0 : y0;
    r.w = y1 - r.y + 1; r.h = x1 - r.x + 1;
    r.a0 = r.x - x0; r.b0 = r.y - y0;
    return r;
}

// Element e of the dense Q [h][w]: row i, column j of R -- consecutive lanes walk along a row --, the index of its cell in a raster of
// width W and of its cell in the mask.
struct SensorCell { size_t cell; int mask; };
SENSOR_HD inline SensorCell sensor_cell(const SensorRect &r, int e, int W, int mw) {
    const int i = e / r.w, j = e - i * r.w;
    SensorCell c;
    c.cell = (size_t)(r.x + i) * (size_t)W + (size_t)(r.y + j);
    c.mask = (r.a0 + i) * mw + (r.b0 + j);
    return c;
}

// The launch: workgroup (bx, m) makes elements bx * 256 .. + 255 of map m's Q; the grid's x extent covers the unclipped mask, a clipped
// R leaves its last workgroups without work.  Map m's Q lies at byte m * sensor_slot_stride() of the engine's patch buffer.
SENSOR_HD inline int sensor_lane_elem(int bx, int t) { return bx * SENSOR_THREADS + t; }
inline unsigned sensor_grid_x(int mw, int mh) { return (unsigned)((mw * mh + SENSOR_THREADS - 1) / SENSOR_THREADS); }
SENSOR_HD inline size_t sensor_slot_stride(int mw, int mh) { return ((size_t)mw * (size_t)mh + 15) & ~(size_t)15; }
