// graded_kernel_driver.cpp -- the body of k_cspace_dilate_graded (csrc/ufm_cspace_graded.h) compiled as plain C++ and run thread by
// thread on the host, in the manner of cspace_kernel_driver.cpp: threadIdx / blockIdx are variables, __shared__ is a static array, and a
// workgroup runs in two passes split at the kernel's one barrier (pass 0 returns there; pass 1 stages again -- the same values -- and
// goes on).  Random maps, footprints of 1 .. 16 levels, anchors, rectangles and output pitches against a brute-force loop over the
// definition; tests/test_cspace_graded_surface.py builds it with AddressSanitizer / UBSan, so an index outside the raw raster, the
// output or the LDS array, or a misaligned dword access, ends the run.  It also checks grow_rect for graded footprints: a raw change
// inside a patch moves no cell of the dilation outside the grown rectangle.  Stand-alone: that header and what it includes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>
using std::min; using std::max;
struct D3 { unsigned x, y, z; };
static D3 threadIdx, blockIdx, blockDim = {256, 1, 1};
static int g_phase;
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define __syncthreads() if (g_phase == 0) return
#include "ufm_cspace_graded.h"

static void run(const CspaceGradedJob &J) {
    for (unsigned by = 0; by < (unsigned)(J.h + CS_TR - 1) / CS_TR; ++by)
        for (unsigned bx = 0; bx < (unsigned)(J.w + CS_TC - 1) / CS_TC; ++bx) {
            blockIdx = {bx, by, 0};
            for (g_phase = 0; g_phase < 2; ++g_phase)
                for (unsigned t = 0; t < 256; ++t) { threadIdx = {t, 0, 0}; k_cspace_dilate_graded(J); }
        }
}
// the definition, cell by cell
static void ref(const std::vector<uint8_t> &raw, int L, int W, const uint8_t *drop, int mh, int mw, int ar, int ac, std::vector<uint8_t> &out) {
    out.assign((size_t)L * W, 0);
    for (int i = 0; i < L; ++i) for (int j = 0; j < W; ++j) {
        int m = 0;
        for (int a = 0; a < mh; ++a) for (int b = 0; b < mw; ++b) if (drop[a * mw + b] != 255) {
            int r = i + a - ar, c = j + b - ac;
            if (r >= 0 && r < L && c >= 0 && c < W) m = max(m, max((int)raw[(size_t)r * W + c] - (int)drop[a * mw + b], 0));
        }
        out[(size_t)i * W + j] = (uint8_t)m;
    }
}
static CspaceGradedJob job(const CspaceMask &cm, const CspaceLevels &cl) {
    CspaceGradedJob J{};
    J.mh = cm.mh; J.mw = cm.mw; J.ar = cm.ar; J.ac = cm.ac; J.nl = cl.n;
    for (int l = 0; l < cl.n; ++l) { J.drop[l] = cl.drop[l]; for (int a = 0; a < CSPACE_MAX; ++a) J.rows[l][a] = cl.rows[l][a]; }
    return J;
}
int main() {
    srand(2);
    int bad = 0, cases = 0, level_counts = 0;
    for (int it = 0; it < 160; ++it) {
        int L = 1 + rand() % 100, W = 1 + rand() % 150;
        if (it % 3 == 0) W = (W + 3) & ~3;
        int mh = 1 + rand() % 31, mw = 1 + rand() % 31;
        if (it % 2) { mh = 1 + rand() % 6; mw = 1 + rand() % 6; }
        if (it == 1) { mh = mw = 1; }
        if (it == 2) { mh = mw = 31; }
        // 1 .. 16 levels: a palette of distinct drops with 0 first (the anchor's), every 16th case all 16 of them
        const int want_levels = it % 16 == 0 ? 16 : 1 + rand() % 16;
        int pal[16] = {0};
        for (int l = 1; l < want_levels; ++l) {
            bool fresh;
            do { pal[l] = 1 + rand() % 254; fresh = true; for (int k = 0; k < l; ++k) fresh = fresh && pal[k] != pal[l]; } while (!fresh);
        }
        std::vector<uint8_t> drop((size_t)mh * mw);
        for (auto &v : drop) v = rand() % 3 == 0 ? (uint8_t)pal[rand() % want_levels] : 255;
        int ar = rand() % mh, ac = rand() % mw;
        drop[ar * mw + ac] = 0;
        CspaceMask cm;
        CspaceLevels cl;
        if (!cspace_graded_pack(drop.data(), mw, mh, ar, ac, &cm, &cl)) { printf("pack failed\n"); return 1; }
        if (cl.n < 1 || cl.n > want_levels) { printf("level count\n"); return 1; }
        level_counts |= 1 << (cl.n - 1);
        // raw in a heap buffer of exactly L*W bytes (ASan catches overreads); aligned by malloc
        std::vector<uint8_t> raw((size_t)L * W);
        for (auto &v : raw) v = rand() & 255;
        std::vector<uint8_t> want;
        ref(raw, L, W, drop.data(), mh, mw, ar, ac, want);
        // whole map
        {
            uint8_t *out = (uint8_t *)malloc((size_t)L * W);
            memset(out, 0xEE, (size_t)L * W);
            CspaceGradedJob J = job(cm, cl); J.raw = raw.data(); J.out = out; J.L = L; J.W = W; J.x0 = 0; J.y0 = 0; J.h = L; J.w = W; J.pitch = W;
            run(J);
            if (memcmp(out, want.data(), (size_t)L * W)) { ++bad; printf("whole map mismatch L=%d W=%d m=%dx%d a=%d,%d levels=%d\n", L, W, mh, mw, ar, ac, cl.n); }
            free(out); ++cases;
        }
        // a rectangle, grown from a random patch, written with a pitch of its own: the bytes between the rows stay as they were
        {
            int h = 1 + rand() % min(L, 40), w = 1 + rand() % min(W, 40), x = rand() % (L - h + 1), y = rand() % (W - w + 1);
            PatchRect g = grow_rect(PatchRect{0, x, y, w, h}, mh, mw, ar, ac, L, W);
            const int pitch = g.w + rand() % 4;
            uint8_t *out = (uint8_t *)malloc((size_t)pitch * g.h);
            memset(out, 0xEE, (size_t)pitch * g.h);
            CspaceGradedJob J = job(cm, cl); J.raw = raw.data(); J.out = out; J.L = L; J.W = W; J.x0 = g.x; J.y0 = g.y; J.h = g.h; J.w = g.w; J.pitch = pitch;
            run(J);
            for (int i = 0; i < g.h; ++i) for (int j = 0; j < pitch; ++j)
                if (out[(size_t)i * pitch + j] != (j < g.w ? want[(size_t)(g.x + i) * W + g.y + j] : 0xEE)) { ++bad; printf("rect mismatch\n"); i = g.h; break; }
            // and: changing raw inside the patch changes nothing outside the grown rectangle
            std::vector<uint8_t> raw2 = raw, want2;
            for (int i = 0; i < h; ++i) for (int j = 0; j < w; ++j) raw2[(size_t)(x + i) * W + y + j] = rand() & 255;
            ref(raw2, L, W, drop.data(), mh, mw, ar, ac, want2);
            for (int i = 0; i < L; ++i) for (int j = 0; j < W; ++j)
                if (want2[(size_t)i * W + j] != want[(size_t)i * W + j] && !(i >= g.x && i < g.x + g.h && j >= g.y && j < g.y + g.w)) { ++bad; printf("change outside grown rect\n"); i = L; break; }
            free(out); ++cases;
        }
    }
    printf("%d cases, %d bad, level counts seen %x\n", cases, bad, level_counts);
    return bad != 0;
}
