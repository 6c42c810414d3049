// sensor_driver.cpp -- the index arithmetic of the sensor reveal (csrc/ufm_sensor_rect.h), run lane by lane on the host the way k_reveal
// runs it: every workgroup of the launch, every thread.  Each read and write is made at the index the kernel would use, on heap blocks of
// exactly the raster's, the survey's, the mask's and the slot's size, so tests/test_sensor_surface.py, which builds this with
// AddressSanitizer / UBSan, ends the run on any byte outside them.  Checked: every cell of R is written exactly once and nothing beyond
// R's w * h bytes of the slot is touched, R is the mask's bounding rectangle clipped to the map, and Q and the changed count equal a
// brute-force loop over the whole map.  Maps W, L = 1 .. 40; masks 1 x 1, 3 x 5 with anchor (2, 0), the 11 x 11 disc, 71 x 71; centres
// at every corner, on every border and in the interior.  Stand-alone: that header only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ufm_sensor_rect.h"

static int bad = 0, cases = 0;
static void fail(const char *what, int a, int b, int c) { if (++bad <= 10) std::printf("%s (%d, %d, %d)\n", what, a, b, c); }

struct Mask { int mw, mh, ar, ac; std::vector<uint8_t> bytes; };

static uint8_t *block(size_t n) {
    uint8_t *p = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    if (!p) std::abort();
    return p;
}

// one reveal at (row, col) of an L x W map
static void reveal(const Mask &mk, int L, int W, int row, int col) {
    SensorShape s;
    if (!sensor_pack(mk.bytes.data(), mk.mw, mk.mh, mk.ar, mk.ac, &s) || !sensor_centre_ok(row, col, L, W)) { fail("rejected", L, W, row); return; }
    const size_t cells = (size_t)L * W, stride = sensor_slot_stride(s.mw, s.mh);
    uint8_t *cur = block(cells), *survey = block(cells), *mask = block((size_t)s.mw * s.mh), *slot = block(stride);
    for (size_t i = 0; i < cells; ++i) { cur[i] = (uint8_t)(rand() & 255); survey[i] = (uint8_t)(rand() % 3 == 0 ? cur[i] : rand() & 255); }   // some cells already agree
    std::memcpy(mask, mk.bytes.data(), (size_t)s.mw * s.mh);
    std::memset(slot, 0xA5, stride);
    // brute force over the whole map: which cells the mask covers, and R as their clipped bounding rectangle's definition gives it
    const int x0 = row - s.ar, y0 = col - s.ac;
    int bx0 = x0 < 0 ? 0 : x0, by0 = y0 < 0 ? 0 : y0, bx1 = x0 + s.mh - 1, by1 = y0 + s.mw - 1;
    if (bx1 > L - 1) bx1 = L - 1;
    if (by1 > W - 1) by1 = W - 1;
    const SensorRect r = sensor_place(row, col, s.mh, s.mw, s.ar, s.ac, L, W);
    if (r.x != bx0 || r.y != by0 || r.h != bx1 - bx0 + 1 || r.w != by1 - by0 + 1 || r.w < 1 || r.h < 1) fail("rectangle", L, W, row * 1000 + col);
    if (row < r.x || row >= r.x + r.h || col < r.y || col >= r.y + r.w) fail("centre outside R", L, W, row * 1000 + col);
    std::vector<uint8_t> want((size_t)r.w * r.h);
    unsigned want_changed = 0;
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < W; ++j) {
            const int a = i - row + s.ar, b = j - col + s.ac;        // the mask cell on (i, j), not reflected
            const bool in_mask = a >= 0 && b >= 0 && a < s.mh && b < s.mw;
            const bool in_r = i >= r.x && i < r.x + r.h && j >= r.y && j < r.y + r.w;
            if (in_mask != in_r) fail("R is not the mask's extent", i, j, row * 1000 + col);
            if (!in_r) continue;
            const uint8_t q = mk.bytes[(size_t)a * s.mw + b] ? survey[(size_t)i * W + j] : cur[(size_t)i * W + j];
            want[(size_t)(i - r.x) * r.w + (j - r.y)] = q;
            want_changed += q != cur[(size_t)i * W + j];
        }
    // the launch
    const int n = r.w * r.h;
    std::vector<int> writes(stride, 0);
    unsigned changed = 0;
    const unsigned grid = sensor_grid_x(s.mw, s.mh);
    if ((size_t)grid * SENSOR_THREADS < (size_t)n) fail("grid too small", (int)grid, n, 0);
    for (unsigned b = 0; b < grid; ++b) {
        if (sensor_lane_elem((int)b, 0) >= n) continue;
        for (int t = 0; t < SENSOR_THREADS; ++t) {
            const int e = sensor_lane_elem((int)b, t);
            if (e >= n) continue;
            const SensorCell c = sensor_cell(r, e, W, s.mw);
            const uint8_t old = cur[c.cell];
            const uint8_t q = mask[c.mask] ? survey[c.cell] : old;
            slot[e] = q;
            ++writes[e];
            changed += q != old;
        }
    }
    for (int e = 0; e < n; ++e) if (writes[e] != 1) { fail("cell of R not written exactly once", e, r.w, r.h); break; }
    for (size_t e = n; e < stride; ++e) if (slot[e] != 0xA5) { fail("byte beyond R written", (int)e, n, 0); break; }
    if (std::memcmp(slot, want.data(), (size_t)n) != 0) fail("Q", L, W, row * 1000 + col);
    if (changed != want_changed) fail("changed", (int)changed, (int)want_changed, row * 1000 + col);
    std::free(cur); std::free(survey); std::free(mask); std::free(slot);
    ++cases;
}

int main() {
    srand(5);
    std::vector<Mask> masks;
    masks.push_back({1, 1, -1, -1, {1}});
    masks.push_back({5, 3, 2, 0, {1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0}});        // 3 rows x 5 columns, anchor in the bottom left corner (not set)
    {
        Mask d{11, 11, -1, -1, std::vector<uint8_t>(121)};
        for (int a = 0; a < 11; ++a) for (int b = 0; b < 11; ++b) d.bytes[a * 11 + b] = (a - 5) * (a - 5) + (b - 5) * (b - 5) <= 25;
        masks.push_back(d);
    }
    {
        Mask big{71, 71, 10, 60, std::vector<uint8_t>(71 * 71)};
        for (auto &v : big.bytes) v = (uint8_t)(rand() % 4 != 0);
        masks.push_back(big);
    }
    // rejected masks
    {
        SensorShape s;
        const uint8_t one[1] = {1}, none[4] = {0, 0, 0, 0};
        std::vector<uint8_t> wide(128, 1);
        if (sensor_pack(nullptr, 1, 1, -1, -1, &s) || sensor_pack(one, 0, 1, -1, -1, &s) || sensor_pack(wide.data(), 128, 1, -1, -1, &s) ||
            sensor_pack(wide.data(), 1, 128, -1, -1, &s) || sensor_pack(none, 2, 2, -1, -1, &s) || sensor_pack(one, 1, 1, 1, 0, &s) ||
            sensor_pack(one, 1, 1, 0, -1, &s) || s.set) fail("a bad mask was accepted", 0, 0, 0);
        if (!sensor_pack(wide.data(), 127, 1, 0, 126, &s) || !s.set || s.ac != 126) fail("a good mask was rejected", 0, 0, 0);
        if (sensor_centre_ok(-1, 0, 4, 4) || sensor_centre_ok(0, 4, 4, 4) || sensor_centre_ok(4, 0, 4, 4) || !sensor_centre_ok(3, 3, 4, 4)) fail("centre check", 0, 0, 0);
        if (sensor_slot_stride(127, 127) < 127 * 127 || sensor_slot_stride(1, 1) != 16) fail("slot stride", 0, 0, 0);
    }
    for (int W = 1; W <= 40; ++W)
        for (int L = 1; L <= 40; ++L) {
            const int rows[] = {0, L - 1, L / 2, L / 3}, cols[] = {0, W - 1, W / 2, (2 * W) / 3};
            for (const Mask &mk : masks)
                for (int row : rows)
                    for (int col : cols) reveal(mk, L, W, row, col);     // the four corners, the four borders, the interior
        }
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
