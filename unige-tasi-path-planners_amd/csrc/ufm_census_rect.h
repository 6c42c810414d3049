// ufm_census_rect.h -- the cost census (ufm_track_costs) as far as it is index arithmetic: which bytes of a raster a lane of
// k_census_build reads -- the alignment head, the 16-byte vectors, the tail -- and which cell of the raster an element of a dense patch
// stands for.  Plain C++17, with or without HIP: the kernels of ufm_census.h call these functions and tests/cpp/census_driver.cpp runs
// them lane by lane on the host against a brute-force count (every byte read exactly once, nothing outside the raster).
//
// One definition (include/ufm.h): hist[v] = number of cells of a map's PLANNING raster whose value is v, v = 0 .. 255.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define CENSUS_HD __host__ __device__
#else
#define CENSUS_HD
#endif

constexpr int CENSUS_BINS = 256;
constexpr int CENSUS_VEC = 16;          // bytes per wide load
constexpr int CENSUS_THREADS = 256;     // per workgroup: four waves, a private histogram each
constexpr int CENSUS_SMALL = 4096;      // a patch of at most this many cells: one workgroup

// A raster of n bytes at address addr: `head` bytes up to the first 16-byte boundary (all of it if it ends before), nvec aligned
// vectors, `tail` bytes behind the last one.  head + tail <= 30.
struct CensusSplit { uint32_t head; size_t nvec; uint32_t tail; };
CENSUS_HD inline CensusSplit census_split(uintptr_t addr, size_t n) {
    size_t head = (CENSUS_VEC - (addr & (CENSUS_VEC - 1))) & (CENSUS_VEC - 1);
    if (head > n) head = n;
    const size_t nvec = (n - head) / CENSUS_VEC;
    return CensusSplit{(uint32_t)head, nvec, (uint32_t)(n - head - nvec * CENSUS_VEC)};
}
// Thread g of G (all workgroups) makes census_iters() rounds; in round `it` it reads vector census_lane_vec() if that is < nvec, at byte
// offset census_vec_offset().  (The trip count is the same for every lane: the waves aggregate with ballots.)
CENSUS_HD inline size_t census_iters(const CensusSplit &s, size_t G) { return (s.nvec + G - 1) / G; }
CENSUS_HD inline size_t census_lane_vec(size_t it, size_t g, size_t G) { return it * G + g; }
CENSUS_HD inline size_t census_vec_offset(const CensusSplit &s, size_t v) { return s.head + (size_t)CENSUS_VEC * v; }
// The head and tail bytes, numbered q = 0 .. head + tail - 1, are read one per lane by the first wave of workgroup 0.
CENSUS_HD inline size_t census_edge_offset(const CensusSplit &s, uint32_t q) {
    return q < s.head ? (size_t)q : (size_t)s.head + (size_t)CENSUS_VEC * s.nvec + (q - s.head);
}
// workgroups of a build: four vectors per thread and round, at most 1024 of them
inline unsigned census_build_grid(size_t nvec) {
    const size_t per = (size_t)CENSUS_THREADS * 4;
    const size_t g = (nvec + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

// Element e of a dense patch [h][w] whose first element lies at cell (x, y) of a raster of width W: the raster index of its cell
// (rows x .. x+h-1, columns y .. y+w-1, as Graph::update places it).
CENSUS_HD inline size_t census_rect_cell(int e, int x, int y, int w, int W) {
    const int i = e / w, j = e - i * w;
    return (size_t)(x + i) * (size_t)W + (size_t)(y + j);
}
// workgroups of a patch: one up to CENSUS_SMALL cells, then one per 1024 cells, at most 256; every workgroup makes
// census_patch_iters() rounds, thread t of workgroup b looking at element (round * grid + b) * CENSUS_THREADS + t
inline unsigned census_patch_grid(int n) {
    if (n <= CENSUS_SMALL) return 1u;
    const int g = (n + 1023) / 1024;
    return (unsigned)(g > 256 ? 256 : g);
}
CENSUS_HD inline int census_patch_iters(int n, int grid) { return (n + grid * CENSUS_THREADS - 1) / (grid * CENSUS_THREADS); }
CENSUS_HD inline int census_patch_elem(int it, int grid, int block, int t) { return (it * grid + block) * CENSUS_THREADS + t; }
