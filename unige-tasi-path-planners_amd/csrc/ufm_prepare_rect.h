// ufm_prepare_rect.h -- map preparation (ufm_set_image, ufm_gaussian_taps) as far as it is integer and index arithmetic: validating and
// packing the taps, the reflect-101 index, the launch's grid and a workgroup's tile, which staged elements a lane of k_prepare loads and
// from which source cells, the two passes of the separable filter as one lane runs them, and the finishing arithmetic of one L and one
// H element.  Plain C++17, with or without HIP: k_prepare (ufm_prepare.h) is these lane functions with a barrier between the passes,
// engine_set_image validates with them, and tests/cpp/prepare_driver.cpp runs them workgroup by workgroup, lane by lane on the host
// against a brute-force double loop.
//
// One definition (include/ufm.h): H = ~image, 0 -> 1;  L = min(max(~((taps (x) taps) * image, reflect-101, one rounding (v + 2^15) >> 16), 1)
// + penalty, 255) -- harness.simulation_data(image, penalty, ntaps) when the taps are the Gaussian's.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define PREP_HD __host__ __device__
#else
#define PREP_HD
#endif

constexpr int PREP_MAX_TAPS = 31;       // taps of one axis: odd, 1 .. 31
constexpr int PREP_THREADS = 256;       // per workgroup: four waves
constexpr int PREP_TW = 64;             // a workgroup's output tile: 64 columns (16 lanes x 4 bytes: one dword store per lane and row) ...
constexpr int PREP_TH = 32;             // ... by 32 rows, two per lane
constexpr int PREP_MAX_R = PREP_MAX_TAPS / 2;
constexpr int PREP_MAX_HX = (PREP_MAX_R + 3) & ~3;                          // the column halo, rounded up to whole dwords
constexpr int PREP_STAGE_WORDS = (PREP_TW + 2 * PREP_MAX_HX) / 4 * (PREP_TH + 2 * PREP_MAX_R);   // staged source bytes, as dwords: 5 952 B
constexpr int PREP_MID_ELEMS = PREP_TW * (PREP_TH + 2 * PREP_MAX_R);        // row sums, 16 bits each: 7 936 B

// the taps as they travel in the kernel argument
struct PrepTaps {
    uint16_t t[PREP_MAX_TAPS];
    uint16_t n;
};

// ntaps odd, 1 .. 31, every tap <= 256, their sum exactly 256 (so a row sum is at most 255 * 256 and fits 16 bits)
inline bool prep_taps_valid(const uint16_t *taps, int ntaps) {
    if (!taps || ntaps < 1 || ntaps > PREP_MAX_TAPS || !(ntaps & 1)) return false;
    unsigned sum = 0;
    for (int i = 0; i < ntaps; ++i) {
        if (taps[i] > 256) return false;
        sum += taps[i];
    }
    return sum == 256;
}
// everything ufm_set_image checks but the handle: a single reflection must suffice -- ntaps / 2 < min(width, length)
inline bool prep_args_valid(const uint16_t *taps, int ntaps, int width, int length, int penalty) {
    if (width <= 0 || length <= 0 || penalty < 0 || penalty > 255 || !prep_taps_valid(taps, ntaps)) return false;
    return ntaps / 2 < (width < length ? width : length);
}
// false: not valid taps, *out untouched
inline bool prep_pack(const uint16_t *taps, int ntaps, PrepTaps *out) {
    if (!prep_taps_valid(taps, ntaps)) return false;
    PrepTaps k{};
    for (int i = 0; i < ntaps; ++i) k.t[i] = taps[i];
    k.n = (uint16_t)ntaps;
    *out = k;
    return true;
}

// ufm_gaussian_taps: what cv2.GaussianBlur(img, (k, k), 0) applies to 8-bit images, as harness.gaussian_kernel_fixed restates it -- the
// fixed table for k <= 7, else sigma = 0.3 ((k - 1) / 2 - 1) + 0.8; x 256, rounded half to even with the rounding error carried to the
// next tap, the centre taking what is left of 256.  (The normalising sum is taken in numpy's order: eight partial sums for eight taps
// or more, so that a coefficient on a rounding boundary falls the same way.)
inline bool prep_gaussian_taps(int ksize, uint16_t *taps) {
    if (!taps || ksize < 1 || ksize > PREP_MAX_TAPS || !(ksize & 1)) return false;
    static const double small[4][7] = {{1.0}, {0.25, 0.5, 0.25}, {0.0625, 0.25, 0.375, 0.25, 0.0625},
                                       {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125}};
    double k[PREP_MAX_TAPS];
    if (ksize <= 7) {
        for (int i = 0; i < ksize; ++i) k[i] = small[ksize / 2][i];
    } else {
        const double sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8, scale = -0.5 / (sigma * sigma);
        for (int i = 0; i < ksize; ++i) {
            const double x = i - (ksize - 1) * 0.5;
            k[i] = std::exp(scale * x * x);
        }
        double r[8], sum;
        for (int j = 0; j < 8; ++j) r[j] = k[j];
        int i = 8;
        for (; i + 8 <= ksize; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += k[i + j];
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < ksize; ++i) sum += k[i];
        for (int j = 0; j < ksize; ++j) k[j] /= sum;
    }
    double err = 0.0;
    int acc = 0;
    for (int i = 0; i < ksize / 2; ++i) {
        const double adj = k[i] * 256 + err;
        const double v = std::nearbyint(adj);
        err = adj - v;
        taps[i] = taps[ksize - 1 - i] = (uint16_t)(int)v;
        acc += (int)v;
    }
    taps[ksize / 2] = (uint16_t)(256 - 2 * acc);
    return true;
}

// reflect-101 (numpy.pad(mode="reflect")): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; one reflection, right for -n < i < 2 n - 1
PREP_HD inline int prep_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}
// The source index of a staged element.  A tile on the far border stages rows and columns beyond the reach of any output it makes
// (beyond n - 1 + ntaps / 2); those are never read back, and their index is clamped so that every load stays inside the image.
PREP_HD inline int prep_src_index(int i, int n) {
    i = prep_reflect(i, n);
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

// The launch: workgroup (bx, by) makes rows by * 32 .. + 31, columns bx * 64 .. + 63 of both outputs of one map.
inline unsigned prep_grid_x(int W) { return (unsigned)((W + PREP_TW - 1) / PREP_TW); }
inline unsigned prep_grid_y(int L) { return (unsigned)((L + PREP_TH - 1) / PREP_TH); }

// A workgroup's tile and what it stages: rows row0 - r .. row0 + 31 + r, columns col0 - hx .. col0 + 63 + hx, hx = r rounded up to 4 --
// so that a staged dword starts at a column that is a multiple of 4.  pitch: bytes per staged row.
struct PrepTile { int row0, col0, r, hx, pitch, srows; };
PREP_HD inline PrepTile prep_tile(int bx, int by, int ntaps) {
    PrepTile tl;
    tl.row0 = by * PREP_TH; tl.col0 = bx * PREP_TW;
    tl.r = ntaps / 2; tl.hx = (tl.r + 3) & ~3;
    tl.pitch = PREP_TW + 2 * tl.hx; tl.srows = PREP_TH + 2 * tl.r;
    return tl;
}

// Staged element u of a tile -- a dword, four columns of one staged row; consecutive u walk along a row --: the source row (reflected)
// and the column of its first byte, which may lie outside [0, W); byte b then comes from column prep_src_index(col + b, W).
struct PrepUnit { int row, col; };
PREP_HD inline int prep_stage_units(const PrepTile &tl) { return tl.srows * (tl.pitch >> 2); }
PREP_HD inline PrepUnit prep_stage_unit(const PrepTile &tl, int u, int L) {
    const int wpr = tl.pitch >> 2, s = u / wpr, w = u - s * wpr;
    PrepUnit un;
    un.row = prep_src_index(tl.row0 - tl.r + s, L);
    un.col = tl.col0 - tl.hx + 4 * w;
    return un;
}

PREP_HD inline uint32_t prep_load4(const uint8_t *p) {      // p is 4-byte aligned
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
}
PREP_HD inline void prep_store4(uint8_t *p, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4); }
PREP_HD inline uint64_t prep_load8(const uint16_t *p) {     // four row sums; p is 8-byte aligned
    uint64_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
    return v;
}
PREP_HD inline void prep_store8(uint16_t *p, uint64_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 8), &v, 8); }

// Lane t stages elements t, t + 256, ... .  wide_in (W a multiple of 4 and the image 4-byte aligned): an element inside the image is one
// 32-bit load; elsewhere four byte loads at reflected columns.
PREP_HD inline void prep_stage_lane(int t, const PrepTile &tl, const uint8_t *src, int W, int L, bool wide_in, uint32_t *stage) {
    const int n = prep_stage_units(tl);
    for (int u = t; u < n; u += PREP_THREADS) {
        const PrepUnit un = prep_stage_unit(tl, u, L);
        const uint8_t *row = src + (size_t)un.row * (size_t)W;
        uint32_t v;
        if (wide_in && un.col >= 0 && un.col + 3 < W) {
            v = prep_load4(row + un.col);
        } else {
            v = 0;
            for (int b = 0; b < 4; ++b) v |= (uint32_t)row[prep_src_index(un.col + b, W)] << (8 * b);
        }
        stage[u] = v;
    }
}

// one element of the horizontal pass: at most 255 * 256 = 65 280
PREP_HD inline uint32_t prep_row_sum(const uint8_t *p, const PrepTaps &k) {
    uint32_t a = 0;
    for (int i = 0; i < k.n; ++i) a += (uint32_t)k.t[i] * p[i];
    return a;
}
// The taps as the passes read them: 32-bit words in LDS, written once per workgroup by its first 31 lanes (a lane reads ITS tap from the
// kernel argument).  A pass then takes tap i with one LDS read at an address all lanes share -- a broadcast, no bank conflict -- instead of
// a scalar load by index from the kernel argument in every iteration, or 31 scalar registers if the loops were unrolled (tried: 106 SGPRs,
// 36 of them spilled).
PREP_HD inline void prep_taps_lane(int t, const PrepTaps &k, uint32_t *w) {
    if (t < PREP_MAX_TAPS) w[t] = t < k.n ? k.t[t] : 0u;
}

// Lane t makes groups t, t + 256, ... of the intermediate [srows][64], a group being four adjacent row sums of one staged row: a window
// of three bytes slides along the row, so every tap costs ONE LDS byte read for four sums, and the group is one 64-bit LDS write.
PREP_HD inline void prep_hpass_lane(int t, const PrepTile &tl, const uint32_t *w, int ntaps, const uint32_t *stage, uint16_t *mid) {
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
    const int n = tl.srows * (PREP_TW / 4);
    for (int e = t; e < n; e += PREP_THREADS) {
        const int s = e / (PREP_TW / 4), c = 4 * (e - s * (PREP_TW / 4));
        const uint8_t *p = sb + s * tl.pitch + tl.hx - tl.r + c;
        uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, b0 = p[0], b1 = p[1], b2 = p[2];
        for (int i = 0; i < ntaps; ++i) {
            const uint32_t b3 = p[i + 3], wi = w[i];
            v0 += wi * b0; v1 += wi * b1; v2 += wi * b2; v3 += wi * b3;
            b0 = b1; b1 = b2; b2 = b3;
        }
        prep_store8(mid + s * PREP_TW + c, (uint64_t)(v0 | (v1 << 16)) | ((uint64_t)(v2 | (v3 << 16)) << 32));
    }
}

// the finishing arithmetic: v is the exact double sum (<= 255 * 65 536), px the source byte
PREP_HD inline uint8_t prep_finish_l(uint32_t v, int penalty) {
    uint32_t c = 255u - ((v + 32768u) >> 16);
    if (c == 0) c = 1;
    c += (uint32_t)penalty;
    return (uint8_t)(c > 255u ? 255u : c);
}
PREP_HD inline uint8_t prep_finish_h(uint8_t px) {
    const uint8_t c = (uint8_t)(255 - px);
    return c ? c : (uint8_t)1;
}

// Lane t makes four adjacent columns (t & 15) of rows (t >> 4) and (t >> 4) + 16 of the tile: the column sums from the intermediate (one
// 64-bit LDS read per tap), H
// from the staged centre.  wide_out (W a multiple of 4 and both outputs 4-byte aligned): one 32-bit store per output and row;
// otherwise byte stores, which also end at the map's last column.
PREP_HD inline void prep_vpass_lane(int t, const PrepTile &tl, const uint32_t *w, int ntaps, int penalty, const uint32_t *stage, const uint16_t *mid,
                                    uint8_t *out_l, uint8_t *out_h, int W, int L, bool wide_out) {
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
    const int g = 4 * (t & 15), col = tl.col0 + g;
    if (col >= W) return;
    for (int y = t >> 4; y < PREP_TH; y += PREP_THREADS / 16) {
        const int row = tl.row0 + y;
        if (row >= L) return;
        uint32_t v[4] = {0, 0, 0, 0};
        for (int i = 0; i < ntaps; ++i) {
            const uint64_t q = prep_load8(mid + (y + i) * PREP_TW + g);
            const uint32_t wi = w[i];
            for (int b = 0; b < 4; ++b) v[b] += wi * (uint32_t)((q >> (16 * b)) & 0xFFFFu);
        }
        const uint8_t *centre = sb + (y + tl.r) * tl.pitch + tl.hx + g;
        uint32_t lw = 0, hw = 0;
        for (int b = 0; b < 4; ++b) {
            lw |= (uint32_t)prep_finish_l(v[b], penalty) << (8 * b);
            hw |= (uint32_t)prep_finish_h(centre[b]) << (8 * b);
        }
        const size_t at = (size_t)row * (size_t)W + (size_t)col;
        if (wide_out) {
            prep_store4(out_l + at, lw);
            prep_store4(out_h + at, hw);
        } else {
            for (int b = 0; b < 4 && col + b < W; ++b) {
                out_l[at + b] = (uint8_t)(lw >> (8 * b));
                out_h[at + b] = (uint8_t)(hw >> (8 * b));
            }
        }
    }
}

// may [a, a + na) and [b, b + nb) share a byte?
inline bool prep_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
inline bool prep_aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }
