// prepare_driver.cpp -- map preparation (csrc/ufm_prepare_rect.h) run on the host the way k_prepare runs it: every workgroup of the
// launch, every lane, the lane functions in the kernel's order with the barriers' meaning kept (all lanes finish one before any
// starts the next).  The image, both outputs and the two LDS arrays are heap blocks of exactly their size, so
// tests/test_prepare_surface.py, which builds this with AddressSanitizer / UBSan, ends the run on any byte outside them.  Checked: every
// cell of L and of H is written exactly once (counted from the lanes' cells, and lane_footprint() shows that a lane writes those cells and
// no others), the guard bytes around both rasters stay, every staged source index lies inside the image, no row sum exceeds 16 bits,
// and L and H equal a brute-force double loop with numpy.pad(mode="reflect") borders.
// Maps W, L = 1 .. 40 plus 63 x 257 and 130 x 65, both ways round; 1, 3, 13 and 31 taps wherever ntaps / 2 < min(W, L); penalties 0, 15,
// 255; random, all-0 and all-255 images; the aligned (32-bit) and the byte forms.  Stand-alone: that header only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ufm_prepare_rect.h"

static long bad = 0, cases = 0;
static void fail(const char *what, int a, int b, int c) { if (++bad <= 10) std::printf("%s (%d, %d, %d)\n", what, a, b, c); }

static uint8_t *block(size_t n) {
    uint8_t *p = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    if (!p) std::abort();
    return p;
}

static int reflect101(int i, int n) {        // the definition, by walking
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// the blurred image by the definition: a double loop over the cells, the whole 2-D kernel on each
static std::vector<uint8_t> blur_ref(const std::vector<uint8_t> &img, int L, int W, const uint16_t *taps, int ntaps) {
    std::vector<uint8_t> out((size_t)L * W);
    const int r = ntaps / 2;
    std::vector<int> rows(L + 2 * r), cols(W + 2 * r);          // the padded image's rows and columns
    for (int i = 0; i < L + 2 * r; ++i) rows[i] = reflect101(i - r, L);
    for (int j = 0; j < W + 2 * r; ++j) cols[j] = reflect101(j - r, W);
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < W; ++j) {
            uint64_t v = 0;
            for (int a = 0; a < ntaps; ++a) {
                const uint8_t *row = img.data() + (size_t)rows[i + a] * W;
                uint64_t h = 0;
                for (int b = 0; b < ntaps; ++b) h += (uint64_t)taps[b] * row[cols[j + b]];
                v += taps[a] * h;
            }
            const uint64_t q = (v + 32768) >> 16;
            out[(size_t)i * W + j] = (uint8_t)(q > 255 ? 255 : q);
        }
    return out;
}

// one launch over an L x W image whose blur is `blurred`.  misalign: the image and the outputs start one byte off a 4-byte boundary, so
// the byte forms run whatever W is.
static void prepare(int L, int W, int ntaps, int penalty, const std::vector<uint8_t> &image, const std::vector<uint8_t> &blurred, bool misalign) {
    uint16_t taps[PREP_MAX_TAPS];
    PrepTaps k;
    if (!prep_gaussian_taps(ntaps, taps) || !prep_args_valid(taps, ntaps, W, L, penalty) || !prep_pack(taps, ntaps, &k)) { fail("rejected", L, W, ntaps); return; }
    const size_t cells = (size_t)L * W, off = misalign ? 1 : 0;
    uint8_t *img_block = block(cells + off), *img = img_block + off;
    const size_t guard = 8;
    uint8_t *l_block = block(cells + off + guard), *h_block = block(cells + off + guard), *out_l = l_block + off, *out_h = h_block + off;
    std::memcpy(img, image.data(), cells);
    std::memset(l_block, 0xA5, cells + off + guard);
    std::memset(h_block, 0xA5, cells + off + guard);
    const bool wide_in = W % 4 == 0 && prep_aligned4(img), wide_out = W % 4 == 0 && prep_aligned4(out_l) && prep_aligned4(out_h);
    // brute force
    std::vector<uint8_t> want_l(cells), want_h(cells);
    for (size_t i = 0; i < cells; ++i) {
        int lo = 255 - blurred[i];
        if (lo == 0) lo = 1;
        lo += penalty;
        want_l[i] = (uint8_t)(lo > 255 ? 255 : lo);
        const int hi = 255 - img[i];
        want_h[i] = (uint8_t)(hi ? hi : 1);
    }
    // the launch
    std::vector<int> writes(cells, 0);
    uint32_t *stage = reinterpret_cast<uint32_t *>(block(sizeof(uint32_t) * PREP_STAGE_WORDS));
    uint16_t *mid = reinterpret_cast<uint16_t *>(block(sizeof(uint16_t) * PREP_MID_ELEMS));
    uint32_t *w = reinterpret_cast<uint32_t *>(block(sizeof(uint32_t) * (PREP_MAX_TAPS + 1)));
    const unsigned gx = prep_grid_x(W), gy = prep_grid_y(L);
    if ((size_t)gx * PREP_TW < (size_t)W || (size_t)gy * PREP_TH < (size_t)L) fail("grid too small", (int)gx, (int)gy, 0);
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned bx = 0; bx < gx; ++bx) {
            const PrepTile tl = prep_tile((int)bx, (int)by, k.n);
            if (prep_stage_units(tl) > PREP_STAGE_WORDS || tl.srows * PREP_TW > PREP_MID_ELEMS) fail("LDS too small", tl.srows, tl.pitch, 0);
            for (int u = 0; u < prep_stage_units(tl); ++u) {
                const PrepUnit un = prep_stage_unit(tl, u, L);
                if (un.row < 0 || un.row >= L) fail("staged row outside the image", un.row, L, u);
                for (int b = 0; b < 4; ++b) {
                    const int c = prep_src_index(un.col + b, W);
                    if (c < 0 || c >= W) fail("staged column outside the image", c, W, u);
                    // within reach of an output the index is the reflection's
                    if (un.col + b >= -tl.r && un.col + b <= W - 1 + tl.r && c != reflect101(un.col + b, W)) fail("reflect-101", un.col + b, W, c);
                }
            }
            std::memset(stage, 0xEE, sizeof(uint32_t) * PREP_STAGE_WORDS);
            std::memset(mid, 0xEE, sizeof(uint16_t) * PREP_MID_ELEMS);
            std::memset(w, 0xEE, sizeof(uint32_t) * (PREP_MAX_TAPS + 1));
            for (int t = 0; t < PREP_THREADS; ++t) { prep_taps_lane(t, k, w); prep_stage_lane(t, tl, img, W, L, wide_in, stage); }
            for (int t = 0; t < PREP_THREADS; ++t) prep_hpass_lane(t, tl, w, k.n, stage, mid);
            for (int e = 0; e < tl.srows * PREP_TW; ++e) {
                const int s = e / PREP_TW, c = e % PREP_TW;
                const uint32_t sum = prep_row_sum(reinterpret_cast<const uint8_t *>(stage) + s * tl.pitch + tl.hx - tl.r + c, k);
                if (sum > 65535u || sum != mid[e]) { fail("row sum does not fit 16 bits", e, (int)sum, mid[e]); break; }
            }
            // the cells that are a lane's to write (lane_footprint(): it writes those and no others)
            for (int t = 0; t < PREP_THREADS; ++t) {
                const int col = tl.col0 + 4 * (t & 15);
                for (int y = t >> 4; y < PREP_TH; y += PREP_THREADS / 16)
                    for (int b = 0; b < 4; ++b)
                        if (tl.row0 + y < L && col + b < W) ++writes[(size_t)(tl.row0 + y) * W + col + b];
                prep_vpass_lane(t, tl, w, k.n, penalty, stage, mid, out_l, out_h, W, L, wide_out);
            }
        }
    for (size_t i = 0; i < cells; ++i) if (writes[i] != 1) { fail("cell not written exactly once", (int)i, W, writes[i]); break; }
    for (size_t i = 0; i < off; ++i) if (l_block[i] != 0xA5 || h_block[i] != 0xA5) fail("byte in front of a raster written", (int)i, 0, 0);
    for (size_t i = cells; i < cells + guard; ++i) if (out_l[i] != 0xA5 || out_h[i] != 0xA5) { fail("byte beyond a raster written", (int)i, 0, 0); break; }
    if (std::memcmp(out_l, want_l.data(), cells) != 0) fail("L", L, W, ntaps * 1000 + penalty);
    if (std::memcmp(out_h, want_h.data(), cells) != 0) fail("H", L, W, ntaps * 1000 + penalty);
    std::free(stage); std::free(mid); std::free(w); std::free(img_block); std::free(l_block); std::free(h_block);
    ++cases;
}

// a lane alone: only its own cells change (so the exactly-once count above, taken from the tiles' layout, is the lanes' own)
static void lane_footprint(int L, int W, int ntaps) {
    uint16_t taps[PREP_MAX_TAPS];
    PrepTaps k;
    if (!prep_gaussian_taps(ntaps, taps) || !prep_pack(taps, ntaps, &k)) { fail("taps", ntaps, 0, 0); return; }
    const size_t cells = (size_t)L * W;
    std::vector<uint8_t> img(cells), out_l(cells), out_h(cells);
    for (auto &v : img) v = (uint8_t)(rand() & 255);
    std::vector<uint32_t> stage(PREP_STAGE_WORDS);
    std::vector<uint16_t> mid(PREP_MID_ELEMS);
    std::vector<uint32_t> w(PREP_MAX_TAPS + 1);
    const bool wide = W % 4 == 0 && prep_aligned4(img.data()) && prep_aligned4(out_l.data()) && prep_aligned4(out_h.data());
    for (unsigned by = 0; by < prep_grid_y(L); ++by)
        for (unsigned bx = 0; bx < prep_grid_x(W); ++bx) {
            const PrepTile tl = prep_tile((int)bx, (int)by, k.n);
            for (int t = 0; t < PREP_THREADS; ++t) { prep_taps_lane(t, k, w.data()); prep_stage_lane(t, tl, img.data(), W, L, wide, stage.data()); }
            for (int t = 0; t < PREP_THREADS; ++t) prep_hpass_lane(t, tl, w.data(), k.n, stage.data(), mid.data());
            for (int t = 0; t < PREP_THREADS; ++t) {
                // 0 is no value of L or of H: a cell that holds anything else afterwards was written
                std::fill(out_l.begin(), out_l.end(), (uint8_t)0);
                std::fill(out_h.begin(), out_h.end(), (uint8_t)0);
                prep_vpass_lane(t, tl, w.data(), k.n, 0, stage.data(), mid.data(), out_l.data(), out_h.data(), W, L, wide);
                const int col = tl.col0 + 4 * (t & 15);
                for (int i = 0; i < L; ++i)
                    for (int j = 0; j < W; ++j) {
                        const int y = i - tl.row0;
                        const bool own = j >= col && j < col + 4 && y >= 0 && y < PREP_TH && (y & 15) == (t >> 4);
                        const bool wrote_l = out_l[(size_t)i * W + j] != 0, wrote_h = out_h[(size_t)i * W + j] != 0;
                        if (wrote_l != own || wrote_h != own) { fail("a lane's cells", t, i, j); return; }
                    }
            }
        }
    ++cases;
}

int main() {
    srand(7);
    {   // taps: what is accepted and what is not
        uint16_t t13[13], t31[32];
        const uint16_t want13[13] = {1, 5, 10, 19, 30, 41, 44, 41, 30, 19, 10, 5, 1};
        if (!prep_gaussian_taps(13, t13) || std::memcmp(t13, want13, sizeof(want13)) != 0) fail("13 taps", 0, 0, 0);
        if (prep_gaussian_taps(0, t31) || prep_gaussian_taps(2, t31) || prep_gaussian_taps(33, t31) || prep_gaussian_taps(13, nullptr)) fail("bad ksize accepted", 0, 0, 0);
        for (int ks = 1; ks <= 31; ks += 2) if (!prep_gaussian_taps(ks, t31) || !prep_taps_valid(t31, ks)) fail("gaussian taps invalid", ks, 0, 0);
        const uint16_t one[1] = {256}, low[1] = {255}, big[3] = {0, 257, 0}, even[2] = {128, 128}, wrap[3] = {256, 256, 65280};
        PrepTaps k{};
        if (!prep_taps_valid(one, 1) || prep_taps_valid(low, 1) || prep_taps_valid(big, 3) || prep_taps_valid(even, 2) || prep_taps_valid(wrap, 3) ||
            prep_taps_valid(nullptr, 1) || prep_taps_valid(one, 0) || prep_pack(low, 1, &k) || k.n != 0) fail("taps validation", 0, 0, 0);
        if (prep_args_valid(t13, 13, 6, 40, 0) || prep_args_valid(t13, 13, 40, 6, 0) || !prep_args_valid(t13, 13, 7, 7, 255) || prep_args_valid(t13, 13, 7, 7, 256) ||
            prep_args_valid(t13, 13, 7, 7, -1) || prep_args_valid(one, 1, 0, 1, 0) || !prep_args_valid(one, 1, 1, 1, 0)) fail("argument validation", 0, 0, 0);
        if (prep_reflect(-3, 7) != 3 || prep_reflect(8, 7) != 4 || prep_reflect(6, 7) != 6 || prep_src_index(40, 7) != 0 || prep_src_index(-9, 3) != 0) fail("reflect", 0, 0, 0);
        int a = 0;
        if (!prep_overlap(&a, 4, &a, 1) || prep_overlap(&a, 0, &a + 1, 4) || prep_overlap(&a, 4, &a + 1, 4)) fail("overlap", 0, 0, 0);
    }
    const int ntaps[] = {1, 3, 13, 31}, penalties[] = {0, 15, 255};
    auto sweep = [&](int L, int W) {
        for (int n : ntaps) {
            if (n / 2 >= (W < L ? W : L)) continue;
            uint16_t taps[PREP_MAX_TAPS];
            prep_gaussian_taps(n, taps);
            for (int kind = 0; kind < 3; ++kind) {          // random, all 0, all 255
                std::vector<uint8_t> img((size_t)L * W);
                for (auto &v : img) v = kind == 0 ? (uint8_t)(rand() & 255) : kind == 1 ? 0 : 255;
                const std::vector<uint8_t> blurred = blur_ref(img, L, W, taps, n);
                // (the penalty enters the finishing arithmetic only: all three on the random image, one each on the constant ones)
                for (int p : penalties)
                    if (kind == 0 || p == penalties[(L + W + kind) % 3]) prepare(L, W, n, p, img, blurred, (L + W + p + kind) % 2 == 1);
            }
        }
    };
    for (int W = 1; W <= 40; ++W)
        for (int L = 1; L <= 40; ++L) sweep(L, W);
    sweep(63, 257);
    sweep(257, 63);
    sweep(65, 130);
    sweep(130, 65);
    sweep(68, 132);          // (a multiple of 4 beyond one tile: the 32-bit forms across tile borders)
    lane_footprint(40, 70, 13);
    lane_footprint(33, 68, 3);
    std::printf("%ld cases, %ld bad\n", cases, bad);
    return bad != 0;
}
