// layers_driver.cpp -- the validation and index arithmetic of the cost layers (csrc/ufm_layers_rect.h), run lane by lane on the host the
// way k_layer_compose, k_layer_compose_all and k_reveal_layers run it: every workgroup of every launch, every thread.  Each read and
// write is made at the index the kernel would use, on heap blocks of exactly the rasters', the patch's, the mask's and the slot's size,
// so tests/test_layers_surface.py, which builds this with AddressSanitizer / UBSan, ends the run on any byte outside them.  Checked:
// every element of a dense output is written exactly once and nothing beyond it, and the layer stores, the composed patch, Q and the
// changed count equal a brute-force loop over the whole map.  Maps W, L = 1 .. 40; n = 2 and 4; rectangles at every corner, on every
// border, inside, and the whole map; raster base addresses at all 16 byte alignments for the vector split; masks 1 x 1, 3 x 5 with anchor
// (2, 0), the 11 x 11 disc, 71 x 71.  Stand-alone: that header (and ufm_sensor_rect.h, which it includes) only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ufm_layers_rect.h"

static int bad = 0, cases = 0;
static void fail(const char *what, int a, int b, int c) { if (++bad <= 10) std::printf("%s (%d, %d, %d)\n", what, a, b, c); }

static uint8_t *block(size_t n) {
    uint8_t *p = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    if (!p) std::abort();
    return p;
}
// (a generator of the driver's own: the rasters of the largest case are 16 MiB each)
static uint32_t rng_state = 2463534242u;
static inline uint32_t rnd32() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static inline int rand_() { return (int)(rnd32() >> 1); }
static inline uint8_t rnd() { return (uint8_t)(rnd32() >> 11); }

// the store of one map: n rasters of exactly `cells` bytes each
struct Store {
    int n; size_t cells; uint8_t *layer[LAYERS_MAX];
    Store(int n_, size_t cells_) : n(n_), cells(cells_) {
        for (int k = 0; k < LAYERS_MAX; ++k) layer[k] = nullptr;
        for (int k = 0; k < n; ++k) { layer[k] = block(cells); for (size_t i = 0; i < cells; ++i) layer[k][i] = rand_() % 3 ? rnd() : 0; }
    }
    ~Store() { for (int k = 0; k < n; ++k) std::free(layer[k]); }
    uint8_t max_at(size_t i) const { uint8_t m = 0; for (int k = 0; k < n; ++k) if (layer[k][i] > m) m = layer[k][i]; return m; }
};

// ---- k_layer_compose: a patch of w x h at (x, y) into layer k of an L x W map
static void compose_rect(int n, int k, int L, int W, int x, int y, int w, int h) {
    if (!layers_index_ok(k, n) || !layers_rect_ok(x, y, w, h, L, W)) { fail("rejected", L, W, x * 1000 + y); return; }
    const size_t cells = (size_t)L * W;
    Store st(n, cells);
    const int ne = w * h;
    uint8_t *patch = block((size_t)ne), *out = block((size_t)ne);
    for (int e = 0; e < ne; ++e) patch[e] = rand_() % 4 ? rnd() : 0;
    std::memset(out, 0xA5, (size_t)ne);
    // brute force: the stores after the call, the dense maximum
    std::vector<std::vector<uint8_t>> want(n);
    for (int l = 0; l < n; ++l) want[l].assign(st.layer[l], st.layer[l] + cells);
    for (int i = 0; i < h; ++i) for (int j = 0; j < w; ++j) want[k][(size_t)(x + i) * W + (y + j)] = patch[(size_t)i * w + j];
    std::vector<uint8_t> want_out((size_t)ne);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            uint8_t m = 0;
            for (int l = 0; l < n; ++l) if (want[l][(size_t)(x + i) * W + (y + j)] > m) m = want[l][(size_t)(x + i) * W + (y + j)];
            want_out[(size_t)i * w + j] = m;
        }
    // the launch
    std::vector<int> writes((size_t)ne, 0), stores(cells, 0);
    const unsigned grid = layers_rect_grid(ne);
    if ((size_t)grid * LAYERS_THREADS < (size_t)ne) fail("grid too small", (int)grid, ne, 0);
    for (unsigned b = 0; b < grid; ++b)
        for (int t = 0; t < LAYERS_THREADS; ++t) {
            const int e = layers_lane_elem((int)b, t);
            if (e >= ne) continue;
            const size_t at = layers_rect_cell(e, x, y, w, W);
            const uint8_t v = patch[e];
            uint32_t mx = v;
            uint8_t *dst = st.layer[0];
            for (int l = 0; l < LAYERS_MAX; ++l) {
                if (l == k) dst = st.layer[l];
                else if (l < n) { const uint32_t o = st.layer[l][at]; if (o > mx) mx = o; }
            }
            dst[at] = v; ++stores[at];
            out[e] = (uint8_t)mx; ++writes[(size_t)e];
        }
    for (int e = 0; e < ne; ++e) if (writes[(size_t)e] != 1) { fail("element not written exactly once", e, w, h); break; }
    for (size_t i = 0; i < cells; ++i) {
        const int r = (int)(i / (size_t)W), c = (int)(i % (size_t)W);
        const bool in = r >= x && r < x + h && c >= y && c < y + w;
        if (stores[i] != (in ? 1 : 0)) { fail("layer cell stored other than once inside / never outside", r, c, k); break; }
    }
    for (int l = 0; l < n; ++l) if (std::memcmp(st.layer[l], want[l].data(), cells) != 0) fail("layer store", l, L, W);
    if (std::memcmp(out, want_out.data(), (size_t)ne) != 0) fail("composed patch", L, W, x * 1000 + y);
    std::free(patch); std::free(out);
    ++cases;
}

// ---- k_layer_compose_all: a whole raster of `cells` bytes, every raster at address = `phase` modulo 16
static void compose_all(int n, size_t cells, int phase) {
    // (aligned_alloc + phase: blocks that end exactly behind the raster, so the sanitizer sees the first byte too far)
    uint8_t *base[LAYERS_MAX + 1];
    uint8_t *ras[LAYERS_MAX + 1];
    const size_t room = ((size_t)phase + cells + 15) & ~(size_t)15;
    for (int l = 0; l <= n; ++l) {
        base[l] = static_cast<uint8_t *>(std::aligned_alloc(16, room ? room : 16));
        if (!base[l]) std::abort();
        std::memset(base[l], 0x5A, room ? room : 16);
        ras[l] = base[l] + phase;
    }
    for (int l = 0; l < n; ++l) for (size_t i = 0; i < cells; ++i) ras[l][i] = rand_() % 3 ? rnd() : (uint8_t)(rand_() % 2 ? 0 : 255);
    uint8_t *out = ras[n];
    for (int l = 0; l < n; ++l) if (!layers_same_phase(reinterpret_cast<uintptr_t>(ras[l]), reinterpret_cast<uintptr_t>(out))) fail("phase", l, phase, 0);
    const LayersSplit s = layers_split(reinterpret_cast<uintptr_t>(out), cells);
    if ((size_t)s.head + s.nvec * LAYERS_VEC + s.tail != cells || s.head > 15 || s.tail > 15) fail("split", (int)s.head, (int)s.nvec, (int)s.tail);
    if (s.nvec && ((reinterpret_cast<uintptr_t>(out) + s.head) & 15)) fail("vectors not aligned", phase, (int)cells, 0);
    std::vector<int> writes(cells, 0);
    const unsigned grid = layers_all_grid(s.nvec);
    const size_t G = (size_t)grid * LAYERS_THREADS, iters = layers_iters(s, G);
    for (unsigned b = 0; b < grid; ++b)
        for (int t = 0; t < LAYERS_THREADS; ++t) {
            const size_t g = (size_t)b * LAYERS_THREADS + (size_t)t;
            for (size_t it = 0; it < iters; ++it) {
                const size_t v = layers_lane_vec(it, g, G);
                if (v >= s.nvec) break;
                const size_t off = layers_vec_offset(s, v);
                uint32_t q[4];
                std::memcpy(q, ras[0] + off, 16);
                for (int l = 1; l < LAYERS_MAX; ++l)
                    if (l < n) {
                        uint32_t o[4];
                        std::memcpy(o, ras[l] + off, 16);
                        for (int c = 0; c < 4; ++c) q[c] = layers_max4(q[c], o[c]);
                    }
                std::memcpy(out + off, q, 16);
                for (int c = 0; c < 16; ++c) ++writes[off + (size_t)c];
            }
            if (b == 0 && (uint32_t)t < s.head + s.tail) {
                const size_t off = layers_edge_offset(s, (uint32_t)t);
                uint32_t mx = ras[0][off];
                for (int l = 1; l < LAYERS_MAX; ++l) if (l < n && ras[l][off] > mx) mx = ras[l][off];
                out[off] = (uint8_t)mx; ++writes[off];
            }
        }
    if (s.head + s.tail > 64) fail("edge bytes beyond one wave", (int)s.head, (int)s.tail, 0);
    for (size_t i = 0; i < cells; ++i) if (writes[i] != 1) { fail("byte not written exactly once", (int)i, (int)cells, phase); break; }
    for (size_t i = 0; i < cells; ++i) {
        uint8_t m = 0;
        for (int l = 0; l < n; ++l) if (ras[l][i] > m) m = ras[l][i];
        if (out[i] != m) { fail("composed raster", (int)i, (int)cells, phase); break; }
    }
    for (int i = 0; i < phase; ++i) if (base[n][i] != 0x5A) fail("byte in front of the raster written", i, phase, 0);
    for (size_t i = (size_t)phase + cells; i < room; ++i) if (base[n][i] != 0x5A) { fail("byte behind the raster written", (int)i, phase, 0); break; }
    for (int l = 0; l <= n; ++l) std::free(base[l]);
    ++cases;
}

// ---- k_reveal_layers: one reveal at (row, col) of an L x W map with n layers, `have` = which of them have a survey
struct Mask { int mw, mh, ar, ac; std::vector<uint8_t> bytes; };
static void reveal(const Mask &mk, int n, int have, int L, int W, int row, int col) {
    SensorShape s;
    if (!sensor_pack(mk.bytes.data(), mk.mw, mk.mh, mk.ar, mk.ac, &s) || !sensor_centre_ok(row, col, L, W)) { fail("rejected", L, W, row); return; }
    const size_t cells = (size_t)L * W, stride = sensor_slot_stride(s.mw, s.mh);
    Store st(n, cells);
    uint8_t *survey[LAYERS_MAX] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < n; ++k)
        if ((have >> k) & 1) { survey[k] = block(cells); for (size_t i = 0; i < cells; ++i) survey[k][i] = rand_() % 3 == 0 ? st.layer[k][i] : rnd(); }
    uint8_t *cur = block(cells), *mask = block((size_t)s.mw * s.mh), *slot = block(stride);
    for (size_t i = 0; i < cells; ++i) cur[i] = st.max_at(i);           // the invariant as the call finds it
    std::memcpy(mask, mk.bytes.data(), (size_t)s.mw * s.mh);
    std::memset(slot, 0xA5, stride);
    const SensorRect r = sensor_place(row, col, s.mh, s.mw, s.ar, s.ac, L, W);
    // brute force over the whole map
    std::vector<std::vector<uint8_t>> want(n);
    for (int l = 0; l < n; ++l) want[l].assign(st.layer[l], st.layer[l] + cells);
    std::vector<uint8_t> want_q((size_t)r.w * r.h);
    unsigned want_changed = 0;
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < W; ++j) {
            const int a = i - row + s.ar, b = j - col + s.ac;
            const bool in_mask = a >= 0 && b >= 0 && a < s.mh && b < s.mw;
            const bool in_r = i >= r.x && i < r.x + r.h && j >= r.y && j < r.y + r.w;
            if (in_mask != in_r) fail("R is not the mask's extent", i, j, row * 1000 + col);
            if (!in_r) continue;
            const size_t at = (size_t)i * W + j;
            uint8_t q = 0;
            for (int l = 0; l < n; ++l) {
                if (survey[l] && mk.bytes[(size_t)a * s.mw + b]) want[l][at] = survey[l][at];
                if (want[l][at] > q) q = want[l][at];
            }
            want_q[(size_t)(i - r.x) * r.w + (j - r.y)] = q;
            want_changed += q != cur[at];
        }
    // the launch
    const int ne = r.w * r.h;
    std::vector<int> writes(stride, 0);
    unsigned changed = 0;
    const unsigned grid = sensor_grid_x(s.mw, s.mh);
    if ((size_t)grid * SENSOR_THREADS < (size_t)ne) fail("grid too small", (int)grid, ne, 0);
    for (unsigned b = 0; b < grid; ++b) {
        if (sensor_lane_elem((int)b, 0) >= ne) continue;
        for (int t = 0; t < SENSOR_THREADS; ++t) {
            const int e = sensor_lane_elem((int)b, t);
            if (e >= ne) continue;
            const SensorCell c = sensor_cell(r, e, W, s.mw);
            const bool seen = mask[c.mask] != 0;
            uint32_t q = 0;
            for (int l = 0; l < LAYERS_MAX; ++l) {
                if (l >= n) continue;
                uint8_t *lay = st.layer[l] + c.cell;          // (the kernel: the store + layers_slot(l, m, nmaps, stride) + cell)
                uint32_t v = *lay;
                if (seen && ((have >> l) & 1)) { const uint32_t sv = survey[l][c.cell]; if (sv != v) *lay = (uint8_t)sv; v = sv; }
                if (v > q) q = v;
            }
            slot[e] = (uint8_t)q; ++writes[(size_t)e];
            changed += q != cur[c.cell];
        }
    }
    for (int e = 0; e < ne; ++e) if (writes[(size_t)e] != 1) { fail("cell of R not written exactly once", e, r.w, r.h); break; }
    for (size_t e = (size_t)ne; e < stride; ++e) if (slot[e] != 0xA5) { fail("byte beyond R written", (int)e, ne, 0); break; }
    if (std::memcmp(slot, want_q.data(), (size_t)ne) != 0) fail("Q", L, W, row * 1000 + col);
    if (changed != want_changed) fail("changed", (int)changed, (int)want_changed, row * 1000 + col);
    for (int l = 0; l < n; ++l) if (std::memcmp(st.layer[l], want[l].data(), cells) != 0) fail("layer store after the reveal", l, L, W);
    for (int k = 0; k < n; ++k) std::free(survey[k]);
    std::free(cur); std::free(mask); std::free(slot);
    ++cases;
}

int main() {
    // validation
    if (layers_count_ok(0) || layers_count_ok(5) || !layers_count_ok(1) || !layers_count_ok(4)) fail("layer count", 0, 0, 0);
    if (layers_index_ok(0, 1) || layers_index_ok(-1, 2) || layers_index_ok(2, 2) || layers_index_ok(4, 5) || !layers_index_ok(0, 2) || !layers_index_ok(3, 4)) fail("layer index", 0, 0, 0);
    if (layers_rect_ok(-1, 0, 1, 1, 4, 4) || layers_rect_ok(0, -1, 1, 1, 4, 4) || layers_rect_ok(0, 0, 0, 1, 4, 4) || layers_rect_ok(0, 0, 1, 0, 4, 4) ||
        layers_rect_ok(3, 0, 1, 2, 4, 4) || layers_rect_ok(0, 3, 2, 1, 4, 4) || layers_rect_ok(0, 0, 2147483647, 2, 4, 4) || layers_rect_ok(2147483647, 0, 1, 1, 4, 4) ||
        !layers_rect_ok(0, 0, 4, 4, 4, 4) || !layers_rect_ok(3, 3, 1, 1, 4, 4)) fail("rectangle check", 0, 0, 0);
    if (!layers_rect_is_map(0, 0, 5, 4, 4, 5) || layers_rect_is_map(0, 0, 4, 4, 4, 5) || layers_rect_is_map(1, 0, 5, 3, 4, 5)) fail("whole map", 0, 0, 0);
    if (layers_stride(1) != 16 || layers_stride(16) != 16 || layers_stride(17) != 32 || layers_slot(2, 1, 3, 32) != (size_t)7 * 32) fail("store", 0, 0, 0);
    for (int i = 0; i < 200000; ++i) {          // the packed byte maximum against four plain ones
        const uint32_t a = ((uint32_t)rand_() << 16) ^ (uint32_t)rand_() ^ (i % 5 == 0 ? 0x80FF0080u : 0u), b = ((uint32_t)rand_() << 16) ^ (uint32_t)rand_() ^ (i % 7 == 0 ? a : 0u);
        uint32_t want = 0;
        for (int c = 0; c < 4; ++c) { const uint32_t x = (a >> (8 * c)) & 255u, y = (b >> (8 * c)) & 255u; want |= (x > y ? x : y) << (8 * c); }
        if (layers_max4(a, b) != want) { fail("layers_max4", (int)a, (int)b, 0); break; }
    }
    std::vector<Mask> masks;
    masks.push_back({1, 1, -1, -1, {1}});
    masks.push_back({5, 3, 2, 0, {1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0}});
    {
        Mask d{11, 11, -1, -1, std::vector<uint8_t>(121)};
        for (int a = 0; a < 11; ++a) for (int b = 0; b < 11; ++b) d.bytes[a * 11 + b] = (a - 5) * (a - 5) + (b - 5) * (b - 5) <= 25;
        masks.push_back(d);
    }
    {
        Mask big{71, 71, 10, 60, std::vector<uint8_t>(71 * 71)};
        for (auto &v : big.bytes) v = (uint8_t)(rand_() % 4 != 0);
        masks.push_back(big);
    }
    const int ns[2] = {2, 4};
    for (int W = 1; W <= 40; ++W)
        for (int L = 1; L <= 40; ++L)
            for (int n : ns) {
                // rectangles: the four corners, the four borders, inside, the whole map (each clipped to what the map has room for)
                const int w = W < 3 ? 1 : (W + 2) / 3, h = L < 3 ? 1 : (L + 2) / 3;
                const int rect[10][4] = {{0, 0, w, h}, {0, W - w, w, h}, {L - h, 0, w, h}, {L - h, W - w, w, h},
                                         {0, (W - w) / 2, w, h}, {L - h, (W - w) / 2, w, h}, {(L - h) / 2, 0, w, h}, {(L - h) / 2, W - w, w, h},
                                         {(L - h) / 2, (W - w) / 2, w, h}, {0, 0, W, L}};
                for (int q = 0; q < 10; ++q) compose_rect(n, (q + W + L) % n, L, W, rect[q][0], rect[q][1], rect[q][2], rect[q][3]);
                // the vector split: the base address at one of the 16 alignments per map, all 16 over the sizes
                compose_all(n, (size_t)L * W, (W + 3 * L + n) & 15);
                // reveals: the four corners, the four borders, the interior; every layer surveyed, or one of them not
                const int rows[] = {0, L - 1, L / 2, L / 3}, cols[] = {0, W - 1, W / 2, (2 * W) / 3};
                const int have = (W + L) % 2 ? (1 << n) - 1 : ((1 << n) - 1) & ~(1 << ((W + L / 2) % n));
                for (const Mask &mk : masks)
                    for (int row : rows)
                        for (int col : cols) reveal(mk, n, have, L, W, row, col);
            }
    // every alignment against every remainder of the length, and sizes beyond one round of the grid
    for (int phase = 0; phase < 16; ++phase)
        for (size_t cells = 0; cells <= 70; ++cells) { compose_all(2, cells, phase); compose_all(4, cells, phase); }
    for (int phase = 0; phase < 16; ++phase) compose_all(3, (size_t)262144 + 16 * 5 + 7 + (size_t)phase, phase);
    compose_all(2, (size_t)4096 * LAYERS_THREADS * LAYERS_VEC + 16 * 3 + 5, 9);      // more vectors than the largest grid has threads: a second round
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
