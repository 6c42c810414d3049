// ufm_region_rect.h -- the block replan kernel (k_replan_region, ufm_region.h) as far as it is index arithmetic: the block's geometry in LDS,
// which wave and which bit of its wake words a 4 x 4 patch is and back, the per-lane constants of a burst's nine wake targets, the tiles
// and elements of the frame around the block, the three divisions the kernel does by multiplication, the patches a consumed rectangle
// seeds, the (tile, part) a unit of the write-back stands for.  Plain C++17, with or without HIP: ufm_region.h calls these functions and
// tests/cpp/region_rect_driver.cpp walks them on the host for every block shape, under sanitizers, against brute-force statements.
//
// The tile edge comes in as UFM_TILE, as in ufm_defs.h (16 by default; the engine still compiles with 32, and the driver is built and run for both).
#pragma once

#ifdef __HIPCC__
#define REGION_HD __host__ __device__ __attribute__((always_inline))   // (inlined before anything else looks at the kernel: the text the compiler optimises is the text written in place)
#else
#define REGION_HD
#endif

#ifndef UFM_TILE
#define UFM_TILE 16
#endif
constexpr int REGION_T = UFM_TILE;              // tile edge (= T of ufm_defs.h)
constexpr int RTMAX = 128 / REGION_T;     // block edge in tiles (8 for 16 x 16 tiles: field 71 KB + cost bytes 17 KB + back-pointer codes 16 KB of the CU's 160 KB LDS)
constexpr int RN = RTMAX * REGION_T;      // ... in elements (160)
constexpr int RP = RN + 8;                // LDS pitch of the block's field: rows 4 apart on distinct banks (168 = 5*32 + 8)
constexpr int RCP = RN + 4;               // pitch of the cost bytes
constexpr int RBP = RN;                   // pitch of the back-pointer codes
constexpr int TP = REGION_T / 4;          // 4x4-element patches per tile side
constexpr int RPW = RTMAX * TP / 4;       // patches per wave per side: patch (pr, pc) belongs to wave ((pr & 3) << 2 | (pc & 3))
constexpr int RWW = (RPW * RPW + 31) / 32;   // wake words per wave
constexpr int RFRAME = 4 * RTMAX + 4;     // tiles around the block
constexpr int REGION_UPT = REGION_T * REGION_T / 64;   // units (64 consecutive elements = one wave) per tile
// The largest patch that comes with a job (RegionJob::psrc: a host patch held for the kernel) is REGION_HELD_EDGE cells wide and high:
// plan_patch (ufm_patch_route.h) holds a patch only if r.w <= hold_edge && r.h <= hold_edge, and PATCH_ROUTE_CONFIG (ufm_map_host.h)
// sets hold_edge to this constant; its pinned slot and the kernel's change mask have REGION_HELD_EDGE^2 bytes.  (The rectangles a job
// merely CONSUMES -- applied before the launch -- are bounded by ROUTE_CONFIG's (w + 1) * (h + 1) <= 65 * 65 and by the block they must lie
// in, not by this edge; nothing of theirs is divided by multiplication.)
constexpr int REGION_HELD_EDGE = 64;

// the element (lx, ly) of the block, lx in -1 .. RN, ly in -1 .. RN (the frame included), in the LDS field of (RN + 2) x RP floats
REGION_HD inline int region_field_offset(int lx, int ly) { return (lx + 1) * RP + ly + 1; }

// ---- patch <-> wake bit.  Patch (pr, pc) of the block belongs to wave ((pr & 3) << 2) | (pc & 3) and is bit idx = (pr >> 2) * RPW + (pc >> 2) of
// that wave's words: word idx >> 5, bit idx & 31.
struct RegionWakeBit { int wave, word, bit; };          // (bit: the mask, 1 << (idx & 31))
REGION_HD inline int region_patch_wave(int pr, int pc) { return ((pr & 3) << 2) | (pc & 3); }
REGION_HD inline int region_patch_idx(int pr, int pc) { return (pr >> 2) * RPW + (pc >> 2); }
REGION_HD inline RegionWakeBit region_wake_bit(int pr, int pc) {
    const int ni = region_patch_idx(pr, pc);
    return RegionWakeBit{region_patch_wave(pr, pc), ni >> 5, 1 << (ni & 31)};
}
// ... and back: bit idx of wave w.  Not every (w, idx) is a patch of the block: the caller rejects pr >= nprow || pc >= npcol.
REGION_HD inline int region_bit_row(int w, int idx) { return (idx / RPW) * 4 + (w >> 2); }
REGION_HD inline int region_bit_col(int w, int idx) { return (idx % RPW) * 4 + (w & 3); }
// words of a wave that can hold a bit at all in a block of nprow x npcol patches (a block smaller than RTMAX x RTMAX leaves the upper ones empty)
REGION_HD inline int region_nwords(int nprow, int npcol) {
    const int n = (((nprow + 3) / 4 - 1) * RPW + (npcol + 3) / 4 + 31) / 32;
    return RWW < n ? RWW : n;
}
// A burst's wake targets: lane 0 .. 8 = the 3 x 3 patches around the burst's own (lane 4: itself), direction (dr, dc) = (lane / 3 - 1, lane % 3 - 1).
// A wave's patches all have (pr & 3, pc & 3) = (w >> 2, w & 3), so the neighbour's wave and the distance `di` of its bit index from the
// patch's own do not depend on the patch: per burst only the position and the range test are left.  Lanes 9 .. 63: no target.
struct RegionWakeTarget { bool lane; int dr, dc, wave, di; };
REGION_HD inline RegionWakeTarget region_wake_target(int w, int lane) {
    const bool wt_lane = lane < 9;
    const int wt_dr = wt_lane ? lane / 3 - 1 : 0, wt_dc = wt_lane ? lane % 3 - 1 : 0;
    const int wt_ar = (w >> 2) + wt_dr, wt_ac = (w & 3) + wt_dc;                       // -1 .. 4
    return RegionWakeTarget{wt_lane, wt_dr, wt_dc, ((wt_ar & 3) << 2) | (wt_ac & 3), (wt_ar >> 2) * RPW + (wt_ac >> 2)};
}
// the target of patch (pr, pc) lies inside the block
REGION_HD inline bool region_wake_target_ok(const RegionWakeTarget &t, int pr, int pc, int nprow, int npcol) {
    const int npr = pr + t.dr, npc = pc + t.dc;
    return t.lane & ((unsigned)npr < (unsigned)nprow) & ((unsigned)npc < (unsigned)npcol);
}
// Lane 4 * nd + q of a burst works on node (nd >> 2, nd & 3) of the 4 x 4 patch.  The mask of the lanes whose node borders direction
// (dr, dc) of wake-target lane 0 .. 8 (the centre: all of them), 0 for the other lanes: a change wakes a neighbour only if it is next to it.
REGION_HD inline unsigned long long region_wake_sel(int lane) {
    unsigned long long wake_sel = 0ull;
    if (lane < 9) {
        const int dr = lane / 3 - 1, dc = lane % 3 - 1;
        wake_sel = ~0ull;
        if (dr < 0) wake_sel &= 0x000000000000FFFFull; else if (dr > 0) wake_sel &= 0xFFFF000000000000ull;
        if (dc < 0) wake_sel &= 0x000F000F000F000Full; else if (dc > 0) wake_sel &= 0xF000F000F000F000ull;
    }
    return wake_sel;
}

// ---- the frame: the ring one wide around a block of na x nb, positions (a, b) with a in -1 .. na, b in -1 .. nb and one of them outside 0 .. n - 1.
// The tiles around the block (na, nb = ntx, nty) and the elements around its field (rnx, rny) are enumerated alike: the top row with its two
// corners, the bottom row with its two, the left column, the right column.
REGION_HD constexpr int region_frame_count(int na, int nb) { return 2 * (nb + 2) + 2 * na; }
struct RegionFramePos { int a, b; };
REGION_HD inline RegionFramePos region_frame_at(int i, int na, int nb) {
    if (i < nb + 2) return RegionFramePos{-1, i - 1};
    if (i < 2 * (nb + 2)) return RegionFramePos{na, i - (nb + 2) - 1};
    if (i < 2 * (nb + 2) + na) return RegionFramePos{i - 2 * (nb + 2), -1};
    return RegionFramePos{i - 2 * (nb + 2) - na, nb};
}
REGION_HD inline int region_frame_index(int a, int b, int na, int nb) {
    if (a < 0) return b + 1;                                  // top row: 0 .. nb+1
    if (a >= na) return (nb + 2) + b + 1;                     // bottom row
    if (b < 0) return 2 * (nb + 2) + a;                       // left column
    return 2 * (nb + 2) + na + a;                             // right column
}
static_assert(region_frame_count(RTMAX, RTMAX) == RFRAME, "the largest block's frame");

// ---- divisions by multiplication (a division is ~25 instructions; these run once per iteration and thread of the staging and write-back loops)
// Tile index tl of a block with nty columns -> its row tl / nty.  Domain: 0 <= tl < RTMAX * RTMAX, 1 <= nty <= RTMAX.
static_assert(RTMAX * RTMAX <= 256 && RTMAX <= 8, "region_tile_row: exact for tl < 256, nty <= 8");
REGION_HD inline int region_nty_magic(int nty) { return (65536 + nty - 1) / nty; }
REGION_HD inline int region_tile_row(int tl, int nty_magic) { return (tl * nty_magic) >> 16; }
// Element e of a dense array of rows `w` long -> its row e / w: the cells of a held patch (w = pw, its width) and the elements its cells
// touch (w = ew: pw, or pw + 1 for the node planners).  Domain: 1 <= w <= REGION_HELD_EDGE + 1, 0 <= e < w * (REGION_HELD_EDGE + 1) --
// which holds the cells (pw <= REGION_HELD_EDGE, e < pw * ph <= pw * REGION_HELD_EDGE) and the elements (e < (pw + 1) * (ph + 1)).
// (The product e * magic stays below 2^32 there: at most (REGION_HELD_EDGE + 1) * (2^20 + w).)
static_assert((unsigned long long)(REGION_HELD_EDGE + 1) * ((1ull << 20) + REGION_HELD_EDGE + 1) < (1ull << 32), "region_dense_row: 32-bit product");
REGION_HD inline unsigned region_dense_magic(int w) { return ((1u << 20) + (unsigned)w - 1u) / (unsigned)w; }
REGION_HD inline int region_dense_row(int e, unsigned magic) { return (int)(((unsigned)e * magic) >> 20); }

// ---- the seeding: the patches that hold an element of a consumed rectangle {map, x, y, w, h} (cells x .. x+h-1, y .. y+w-1; `cells`: the
// elements are the cells, MS-DFM -- otherwise the nodes, one more each way), clipped to the block at (rx0, ry0) of rnx x rny elements:
// rows p0 .. p1, columns c0 .. c1
struct RegionPatchRange { int p0, p1, c0, c1; };
REGION_HD inline RegionPatchRange region_seed_range(const int *qr, bool cells, int rx0, int ry0, int rnx, int rny) {
    const int ex0 = qr[1] - rx0, ex1 = qr[1] + qr[4] - (cells ? 1 : 0) - rx0, ey0 = qr[2] - ry0, ey1 = qr[2] + qr[3] - (cells ? 1 : 0) - ry0;
    return RegionPatchRange{(ex0 > 0 ? ex0 : 0) / 4, (ex1 < rnx - 1 ? ex1 : rnx - 1) / 4, (ey0 > 0 ? ey0 : 0) / 4, (ey1 < rny - 1 ? ey1 : rny - 1) / 4};
}

// ---- the write-back: unit u (64 consecutive elements, one wave's) -> entry k of the list of tiles and which part of that tile
REGION_HD inline void region_unit(int u, int &k, int &part) { k = u / REGION_UPT; part = u - k * REGION_UPT; }
