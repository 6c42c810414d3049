// region_rect_driver.cpp -- csrc/ufm_region_rect.h, the block replan kernel's index arithmetic, walked on the host for every block shape
// ntx, nty = 1 .. RTMAX against brute-force statements of what each rule means.  Stand-alone: tests/test_region_surface.py compiles it
// with -fsanitize=address,undefined (for UFM_TILE 16 and 32), runs it and checks the counts it prints.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "ufm_region_rect.h"

static long bad = 0;
#define CHECK(c) do { if (!(c)) { if (++bad <= 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

static bool in_block(int pr, int pc, int nprow, int npcol) { return pr >= 0 && pc >= 0 && pr < nprow && pc < npcol; }

int main() {
    long shapes = 0, patches = 0, bits = 0, targets = 0, frame_tiles = 0, frame_elems = 0, units = 0;
    for (int ntx = 1; ntx <= RTMAX; ++ntx)
        for (int nty = 1; nty <= RTMAX; ++nty) {
            ++shapes;
            const int nprow = ntx * TP, npcol = nty * TP, nwords = region_nwords(nprow, npcol);
            CHECK(nwords >= 1 && nwords <= RWW);
            // every patch: a (wave, word, bit) of its own, below nwords, and the way back
            std::set<std::tuple<int, int, int>> seen;
            for (int pr = 0; pr < nprow; ++pr)
                for (int pc = 0; pc < npcol; ++pc) {
                    ++patches;
                    const RegionWakeBit b = region_wake_bit(pr, pc);
                    CHECK(b.wave >= 0 && b.wave < 16 && b.word >= 0 && b.word < nwords && b.bit != 0 && ((unsigned)b.bit & ((unsigned)b.bit - 1u)) == 0u);
                    CHECK(b.wave == region_patch_wave(pr, pc));
                    CHECK(seen.insert(std::make_tuple(b.wave, b.word, b.bit)).second);
                    const int idx = region_patch_idx(pr, pc);
                    CHECK(b.word == idx >> 5 && (unsigned)b.bit == 1u << (idx & 31));
                    CHECK(region_bit_row(b.wave, idx) == pr && region_bit_col(b.wave, idx) == pc);
                    // the nine wake targets through the per-lane constants against the neighbour computed directly
                    for (int lane = 0; lane < 64; ++lane) {
                        const RegionWakeTarget t = region_wake_target(b.wave, lane);
                        const bool ok = region_wake_target_ok(t, pr, pc, nprow, npcol);
                        if (lane >= 9) { CHECK(!t.lane && !ok); continue; }
                        ++targets;
                        const int dr = lane / 3 - 1, dc = lane % 3 - 1, npr = pr + dr, npc = pc + dc;
                        CHECK(t.lane && t.dr == dr && t.dc == dc);
                        CHECK(ok == in_block(npr, npc, nprow, npcol));
                        if (!ok) continue;
                        CHECK(t.wave == region_patch_wave(npr, npc) && idx + t.di == region_patch_idx(npr, npc));
                        const RegionWakeBit nb = region_wake_bit(npr, npc);
                        CHECK(nb.word == (idx + t.di) >> 5 && (unsigned)nb.bit == 1u << ((idx + t.di) & 31));
                    }
                }
            // every bit of a word below nwords: rejected by the kernel's range test, or a patch of the block that maps to this very bit
            for (int w = 0; w < 16; ++w)
                for (int idx = 0; idx < nwords * 32; ++idx) {
                    ++bits;
                    const int pr = region_bit_row(w, idx), pc = region_bit_col(w, idx);
                    CHECK(pr >= 0 && pc >= 0);
                    if (pr >= nprow || pc >= npcol) continue;
                    CHECK(region_patch_wave(pr, pc) == w && region_patch_idx(pr, pc) == idx);
                }
            // the frame: tiles (ntx, nty) and elements (rnx, rny) alike -- a bijection onto the ring, inverted by region_frame_index
            const int rnx = ntx * REGION_T, rny = nty * REGION_T;
            for (int pass = 0; pass < 2; ++pass) {
                const int na = pass ? rnx : ntx, nb = pass ? rny : nty, n = region_frame_count(na, nb);
                CHECK(n == (na + 2) * (nb + 2) - na * nb);
                if (!pass) CHECK(n <= RFRAME);
                std::set<std::pair<int, int>> ring;
                std::set<int> offs;
                for (int i = 0; i < n; ++i) {
                    (pass ? frame_elems : frame_tiles) += 1;
                    const RegionFramePos f = region_frame_at(i, na, nb);
                    CHECK(f.a >= -1 && f.a <= na && f.b >= -1 && f.b <= nb && (f.a == -1 || f.a == na || f.b == -1 || f.b == nb));
                    CHECK(ring.insert(std::make_pair(f.a, f.b)).second);
                    CHECK(region_frame_index(f.a, f.b, na, nb) == i);
                    if (pass) {
                        const int o = region_field_offset(f.a, f.b);
                        CHECK(o == (f.a + 1) * RP + f.b + 1 && o >= 0 && o < (RN + 2) * RP);
                        CHECK(offs.insert(o).second);
                    }
                }
                CHECK((int)ring.size() == n);
            }
            // the write-back's units over every tile of the block
            std::vector<int> hit((size_t)ntx * nty * REGION_UPT, 0);
            for (int u = 0; u < ntx * nty * REGION_UPT; ++u) {
                ++units;
                int k, part;
                region_unit(u, k, part);
                CHECK(k >= 0 && k < ntx * nty && part >= 0 && part < REGION_UPT && k * REGION_UPT + part == u);
                if (k >= 0 && k < ntx * nty && part >= 0 && part < REGION_UPT) ++hit[(size_t)k * REGION_UPT + part];
            }
            for (int h : hit) CHECK(h == 1);
        }
    // wake_sel: lane 4 * nd + q is selected for direction (dr, dc) exactly if node (nd >> 2, nd & 3) has one of its eight neighbours, or itself, in
    // the 4 x 4 patch at (dr, dc) -- the centre: every node
    long sel = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const unsigned long long m = region_wake_sel(lane);
        if (lane >= 9) { CHECK(m == 0ull); continue; }
        ++sel;
        const int dr = lane / 3 - 1, dc = lane % 3 - 1;
        for (int l = 0; l < 64; ++l) {
            const int nd = l >> 2, r = nd >> 2, c = nd & 3;
            bool borders = false;
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b) {
                    const int rr = r + a - 4 * dr, cc = c + b - 4 * dc;       // the neighbour's position in the patch at (dr, dc)
                    if (rr >= 0 && rr < 4 && cc >= 0 && cc < 4) borders = true;
                }
            CHECK(((m >> l) & 1ull) == (borders ? 1ull : 0ull));
        }
    }
    // the divisions by multiplication, on every point of their domains
    long nty_pts = 0, pw_pts = 0, ew_pts = 0;
    for (int nty = 1; nty <= RTMAX; ++nty) {
        const int magic = region_nty_magic(nty);
        for (int tl = 0; tl < RTMAX * RTMAX; ++tl) { ++nty_pts; CHECK(region_tile_row(tl, magic) == tl / nty); }
    }
    for (int pw = 1; pw <= REGION_HELD_EDGE; ++pw) {            // the cells of a held patch
        const unsigned magic = region_dense_magic(pw);
        for (int e = 0; e < pw * REGION_HELD_EDGE; ++e) { ++pw_pts; CHECK(region_dense_row(e, magic) == e / pw); }
    }
    for (int ew = 1; ew <= REGION_HELD_EDGE + 1; ++ew) {        // the elements its cells touch
        const unsigned magic = region_dense_magic(ew);
        for (int e = 0; e < ew * (REGION_HELD_EDGE + 1); ++e) { ++ew_pts; CHECK(region_dense_row(e, magic) == e / ew); }
    }
    // the seeding's range: the patches that hold an element of the rectangle inside the block, by brute force (rows and columns alike)
    long seeds = 0;
    for (int cells = 0; cells < 2; ++cells)
        for (int nt = 1; nt <= RTMAX; ++nt) {
            const int rn = nt * REGION_T, r0 = 3 * REGION_T;
            for (int x = 0; x < rn; ++x)
                for (int h = 1; h <= REGION_HELD_EDGE + 1 && x + h <= rn; ++h) {
                    ++seeds;
                    const int qr[5] = {0, r0 + x, r0 + x, h, h};
                    const RegionPatchRange s = region_seed_range(qr, cells != 0, r0, r0, rn, rn);
                    int lo = 1 << 30, hi = -1;
                    for (int e = x; e <= x + h - (cells ? 1 : 0); ++e) if (e >= 0 && e < rn) { lo = e / 4 < lo ? e / 4 : lo; hi = e / 4 > hi ? e / 4 : hi; }
                    CHECK(s.p0 == lo && s.p1 == hi && s.c0 == lo && s.c1 == hi);
                }
        }
    std::printf("tile %d shapes %ld patches %ld bits %ld targets %ld sel %ld frame_tiles %ld frame_elems %ld units %ld nty_magic %ld pw_magic %ld ew_magic %ld seeds %ld bad %ld\n",
                REGION_T, shapes, patches, bits, targets, sel, frame_tiles, frame_elems, units, nty_pts, pw_pts, ew_pts, seeds, bad);
    return bad ? 1 : 0;
}
