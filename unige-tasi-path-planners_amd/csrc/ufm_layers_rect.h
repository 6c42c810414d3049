// ufm_layers_rect.h -- cost layers (ufm_set_layers / ufm_patch_layer / ufm_set_layer / ufm_reveal with n > 1) as far as they are
// validation and index arithmetic: which layer indices and rectangles a call accepts, where layer k of map m lies in the engine's store,
// which cell and which element of the dense composed patch a lane of k_layer_compose makes, how k_layer_compose_all cuts a whole raster
// into an unaligned head, 16-byte vectors and a tail, how the byte-wise maximum of four packed bytes is formed, and how many workgroups
// a launch takes.  The rectangle of a reveal is the sensor's: sensor_place / sensor_cell of ufm_sensor_rect.h.  Plain C++17, with or
// without HIP: the kernels of ufm_layers.h call these functions and tests/cpp/layers_driver.cpp runs them lane by lane on the host
// against a brute-force loop.
//
// One definition (include/ufm.h): a handle has n layers, 1 <= n <= 4; with n > 1 the caller's raster == max_k layer[k], cell for cell.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ufm_sensor_rect.h"

#ifdef __HIPCC__
#define LAYERS_HD __host__ __device__
#else
#define LAYERS_HD
#endif

constexpr int LAYERS_MAX = 4;           // = UFM_MAX_LAYERS
constexpr int LAYERS_VEC = 16;          // bytes per wide access
constexpr int LAYERS_THREADS = 256;     // per workgroup: four waves, one cell (or one vector) per lane

LAYERS_HD inline bool layers_count_ok(int n) { return n >= 1 && n <= LAYERS_MAX; }
// a layer call: only with more than one layer, k one of them
LAYERS_HD inline bool layers_index_ok(int k, int n) { return n > 1 && n <= LAYERS_MAX && k >= 0 && k < n; }
// rows x .. x+h-1, columns y .. y+w-1 inside the L x W map (Graph.cpp:38-41 as Engine::patch applies it)
LAYERS_HD inline bool layers_rect_ok(int x, int y, int w, int h, int L, int W) {
    return x >= 0 && y >= 0 && w > 0 && h > 0 && x <= L - h && y <= W - w;
}
LAYERS_HD inline bool layers_rect_is_map(int x, int y, int w, int h, int L, int W) { return x == 0 && y == 0 && w == W && h == L; }

// The store: layer k of map m is a raster of `cells` bytes at byte layers_slot() of one allocation; the stride is a multiple of 16, so
// with the allocation's own alignment every raster starts on a 16-byte boundary and all of them share one vector split.
LAYERS_HD inline size_t layers_stride(size_t cells) { return (cells + (LAYERS_VEC - 1)) & ~(size_t)(LAYERS_VEC - 1); }
LAYERS_HD inline size_t layers_slot(int k, int m, int nmaps, size_t stride) { return ((size_t)k * (size_t)nmaps + (size_t)m) * stride; }

// ---- the rectangle form (k_layer_compose): element e of the dense patch [h][w] -- consecutive lanes walk along a row -- and its cell
LAYERS_HD inline size_t layers_rect_cell(int e, int x, int y, int w, int W) {
    const int i = e / w, j = e - i * w;
    return (size_t)(x + i) * (size_t)W + (size_t)(y + j);
}
LAYERS_HD inline int layers_lane_elem(int bx, int t) { return bx * LAYERS_THREADS + t; }
inline unsigned layers_rect_grid(int n) { return (unsigned)((n + LAYERS_THREADS - 1) / LAYERS_THREADS); }

// ---- the whole-raster form (k_layer_compose_all): n bytes at address addr are `head` bytes up to the first 16-byte boundary (all of
// them if the raster ends before), nvec aligned vectors and `tail` bytes behind the last one; head + tail <= 30.  Every raster of a
// launch -- the layers and the dense output -- has the same address modulo 16 (layers_same_phase), so one split serves them all.
struct LayersSplit { uint32_t head; size_t nvec; uint32_t tail; };
LAYERS_HD inline LayersSplit layers_split(uintptr_t addr, size_t n) {
    size_t head = (LAYERS_VEC - (addr & (LAYERS_VEC - 1))) & (LAYERS_VEC - 1);
    if (head > n) head = n;
    const size_t nvec = (n - head) / LAYERS_VEC;
    return LayersSplit{(uint32_t)head, nvec, (uint32_t)(n - head - nvec * LAYERS_VEC)};
}
LAYERS_HD inline bool layers_same_phase(uintptr_t a, uintptr_t b) { return ((a ^ b) & (LAYERS_VEC - 1)) == 0; }
// Thread g of G (all workgroups) makes layers_iters() rounds; in round `it` it makes vector layers_lane_vec() if that is < nvec, at
// byte offset layers_vec_offset().
LAYERS_HD inline size_t layers_iters(const LayersSplit &s, size_t G) { return (s.nvec + G - 1) / G; }
LAYERS_HD inline size_t layers_lane_vec(size_t it, size_t g, size_t G) { return it * G + g; }
LAYERS_HD inline size_t layers_vec_offset(const LayersSplit &s, size_t v) { return s.head + (size_t)LAYERS_VEC * v; }
// the head and tail bytes, numbered q = 0 .. head + tail - 1: one per lane of the first wave of workgroup 0
LAYERS_HD inline size_t layers_edge_offset(const LayersSplit &s, uint32_t q) {
    return q < s.head ? (size_t)q : (size_t)s.head + (size_t)LAYERS_VEC * s.nvec + (q - s.head);
}
// workgroups of the whole-raster form: one vector per thread and round, at most 4096 of them (16 per CU of a 256-CU device)
inline unsigned layers_all_grid(size_t nvec) {
    const size_t g = (nvec + LAYERS_THREADS - 1) / LAYERS_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// max of four packed unsigned bytes, byte by byte, without a carry between them: bit 7 of t says whether a's low seven bits are >= b's,
// the top bits decide where they differ
LAYERS_HD inline uint32_t layers_max4(uint32_t a, uint32_t b) {
    const uint32_t H = 0x80808080u;
    const uint32_t t = (a | H) - (b & ~H);
    const uint32_t ge = ((a & ~b) | (~(a ^ b) & t)) & H;      // bit 7 of every byte: a >= b
    const uint32_t m = (ge >> 7) * 0xFFu;
    return (a & m) | (b & ~m);
}
