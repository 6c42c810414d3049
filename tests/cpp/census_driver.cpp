// census_driver.cpp -- the index arithmetic of the cost census (csrc/ufm_census_rect.h), run lane by lane on the host the way
// k_census_build and k_census_patch run it: every workgroup, every thread, every round.  Each read is made through the pointer the
// kernel would use -- a 16-byte vector only at an address that is a multiple of 16, the edge bytes and the patch byte by byte -- on heap
// blocks of exactly the raster's and the patch's size, so tests/test_census_surface.py, which builds this with AddressSanitizer / UBSan,
// ends the run on any byte outside them.  Checked: every cell is read exactly once, and the counts equal a brute-force count.
// Rasters of every width 1 .. 70 at base addresses misaligned by 0 .. 15; rectangles at every corner and border, 1 x 1, the whole map,
// and one above the one-workgroup limit.  Stand-alone: that header only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ufm_census_rect.h"

static int bad = 0, cases = 0;
static void fail(const char *what, int a, int b, int c) { if (++bad <= 10) std::printf("%s (%d, %d, %d)\n", what, a, b, c); }

static uint8_t *block16(size_t n) {           // 16-byte aligned, exactly n bytes (n >= 1)
    void *p = nullptr;
    if (posix_memalign(&p, 16, n) != 0) std::abort();
    return static_cast<uint8_t *>(p);
}

// one build of a raster of n bytes at `cost`, on `grid` workgroups
static void build(const uint8_t *cost, size_t n, unsigned grid, int W, int mis) {
    std::vector<int> reads(n, 0);
    std::vector<uint32_t> hist(CENSUS_BINS, 0), want(CENSUS_BINS, 0);
    for (size_t i = 0; i < n; ++i) ++want[cost[i]];
    const CensusSplit s = census_split(reinterpret_cast<uintptr_t>(cost), n);
    if (s.head + s.tail > 30 || s.head + s.tail + CENSUS_VEC * s.nvec != n) fail("split", W, mis, (int)n);
    const size_t G = (size_t)grid * CENSUS_THREADS, iters = census_iters(s, G);
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned t = 0; t < (unsigned)CENSUS_THREADS; ++t) {
            const size_t g = (size_t)b * CENSUS_THREADS + t;
            for (size_t it = 0; it < iters; ++it) {
                const size_t v = census_lane_vec(it, g, G);
                if (v >= s.nvec) continue;
                const uint8_t *q = cost + census_vec_offset(s, v);
                if (reinterpret_cast<uintptr_t>(q) % CENSUS_VEC) { fail("misaligned vector", W, mis, (int)v); continue; }
                uint8_t vec[CENSUS_VEC];
                std::memcpy(vec, q, CENSUS_VEC);                  // (the wide load: all 16 bytes must lie inside the block)
                for (int k = 0; k < CENSUS_VEC; ++k) { ++hist[vec[k]]; ++reads[(q - cost) + k]; }
            }
            if (b == 0 && t < 64 && t < s.head + s.tail) {
                const size_t off = census_edge_offset(s, t);
                ++hist[cost[off]]; ++reads[off];
            }
        }
    for (size_t i = 0; i < n; ++i) if (reads[i] != 1) { fail("cell not read exactly once", W, mis, (int)i); break; }
    if (hist != want) fail("histogram", W, mis, (int)grid);
    ++cases;
}

// one patch [h][w] at (x, y) of an L x W raster, read from an address misaligned by `mis`, on `grid` workgroups
static void patch(std::vector<uint8_t> &raster, int L, int W, int x, int y, int w, int h, int mis, int grid) {
    const int n = w * h;
    uint8_t *blk = block16((size_t)n + mis);
    uint8_t *p = blk + mis;
    for (int e = 0; e < n; ++e) p[e] = (uint8_t)(rand() % 5 == 0 ? raster[census_rect_cell(e, x, y, w, W)] : rand() & 255);   // some cells keep their value
    uint8_t *cost = block16((size_t)L * W);
    std::memcpy(cost, raster.data(), (size_t)L * W);
    std::vector<long> hist(CENSUS_BINS, 0), want(CENSUS_BINS, 0);
    for (int i = 0; i < L * W; ++i) { ++hist[cost[i]]; ++want[cost[i]]; }
    std::vector<int> seen(n, 0);
    const int iters = census_patch_iters(n, grid);
    for (int b = 0; b < grid; ++b)
        for (int t = 0; t < CENSUS_THREADS; ++t)
            for (int it = 0; it < iters; ++it) {
                const int e = census_patch_elem(it, grid, b, t);
                if (e >= n) continue;
                const size_t c = census_rect_cell(e, x, y, w, W);
                const int ci = (int)(c / W), cj = (int)(c % W);
                if (ci != x + e / w || cj != y + e % w || ci >= L) fail("cell of element", e, ci, cj);
                const uint8_t ov = cost[c], nv = p[e];
                ++seen[e];
                if (ov != nv) { --hist[ov]; ++hist[nv]; }
            }
    for (int e = 0; e < n; ++e) if (seen[e] != 1) { fail("element not seen exactly once", e, w, h); break; }
    for (int i = 0; i < h; ++i) for (int j = 0; j < w; ++j) {       // Graph::update, and the count of what it leaves
        uint8_t &c = raster[(size_t)(x + i) * W + y + j];
        --want[c]; c = p[i * w + j]; ++want[c];
    }
    if (hist != want) fail("patched histogram", x, y, w * 1000 + h);
    long sum = 0;
    for (long v : hist) { sum += v; if (v < 0) fail("negative count", x, y, w); }
    if (sum != (long)L * W) fail("sum of counts", x, y, (int)sum);
    std::free(blk); std::free(cost);
    ++cases;
}

int main() {
    srand(3);
    // ---- builds ----
    for (int W = 1; W <= 70; ++W)
        for (int L : {1, 2, 3, 37})
            for (int mis = 0; mis < 16; ++mis) {
                const size_t n = (size_t)L * W;
                uint8_t *blk = block16(n + mis);
                uint8_t *cost = blk + mis;
                for (size_t i = 0; i < n; ++i) cost[i] = (W % 3 == 0) ? (uint8_t)(rand() & 1 ? 255 : 0) : (uint8_t)(rand() & 255);
                const size_t nvec = census_split(reinterpret_cast<uintptr_t>(cost), n).nvec;
                build(cost, n, census_build_grid(nvec), W, mis);
                if (L == 37) build(cost, n, 1, W, mis);       // (one workgroup of 256 lanes over up to 161 vectors; below: several rounds)
                std::free(blk);
            }
    {   // several rounds per lane, several workgroups, a grid that does not divide the work
        const size_t n = 300 * 257 + 5;
        uint8_t *blk = block16(n + 3);
        for (size_t i = 0; i < n; ++i) blk[3 + i] = (uint8_t)(rand() & 255);
        for (unsigned grid : {1u, 3u, census_build_grid(n / 16)}) build(blk + 3, n, grid, 257, 3);
        std::free(blk);
    }
    // ---- patches ----
    for (int W = 1; W <= 70; ++W) {
        const int L = 9 + W % 4;
        std::vector<uint8_t> raster((size_t)L * W);
        for (auto &v : raster) v = (uint8_t)(rand() & 255);
        const int w2 = W < 3 ? 1 : 3, h2 = 2;
        const int rects[][4] = {   // x, y, w, h
            {0, 0, w2, h2}, {0, W - w2, w2, h2}, {L - h2, 0, w2, h2}, {L - h2, W - w2, w2, h2},            // the four corners
            {0, W / 3, W - W / 3, 1}, {L - 1, 0, W, 1}, {1, 0, 1, L - 2}, {2, W - 1, 1, L - 3},            // the four borders
            {L / 2, W / 2, 1, 1}, {0, 0, W, L}, {1, W > 2 ? 1 : 0, W > 2 ? W - 2 : 1, L - 2}};             // 1 x 1, the whole map, the interior
        for (const auto &r : rects) patch(raster, L, W, r[0], r[1], r[2], r[3], (W + r[0]) & 15, (int)census_patch_grid(r[2] * r[3]));
    }
    {   // above the one-workgroup limit: 80 x 70 cells whole, 70 x 70 inside, on their own grids and on one that leaves a remainder
        const int L = 90, W = 75;
        std::vector<uint8_t> raster((size_t)L * W);
        for (auto &v : raster) v = (uint8_t)(rand() & 255);
        if (census_patch_grid(70 * 70) < 2 || census_patch_grid(CENSUS_SMALL) != 1) fail("patch grid", 0, 0, 0);
        patch(raster, L, W, 0, 0, W, L, 5, (int)census_patch_grid(L * W));
        patch(raster, L, W, 11, 3, 70, 70, 1, (int)census_patch_grid(70 * 70));
        patch(raster, L, W, 20, 5, 70, 70, 15, 3);
    }
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
