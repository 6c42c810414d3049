// The walk of csrc/ufm_score_rect.h on the host: the text k_score_paths runs one lane per segment, here one segment after the other, under
// the sanitizers (tests/test_score_surface.py builds and runs it; it is never loaded into python).
// Input, a text file: "L W thr n_paths total_points", the raster's L * W bytes, the n_paths + 1 offsets, then the points as the BIT
// PATTERNS of their fp32 coordinates (2 * total_points unsigned integers: NaN and the infinities pass unharmed).
// Output, one line per path: the bit patterns of cost, cost_before, dist and blocked_at, then blocked_segment, pieces, the most pieces
// any one segment of the path was charged and the most raster look-ups any one segment made.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ufm_score_rect.h"

struct Record { float cost, cost_before, dist, blocked_at; int32_t blocked_segment, pieces; };

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int L = 0, W = 0, thr = 0, n_paths = 0, total = 0;
    if (std::fscanf(f, "%d %d %d %d %d", &L, &W, &thr, &n_paths, &total) != 5 || L < 1 || W < 1 || n_paths < 0 || total < 0) return 3;
    std::vector<uint8_t> raster((size_t)L * W);
    for (uint8_t &b : raster) { unsigned v; if (std::fscanf(f, "%u", &v) != 1 || v > 255) return 3; b = (uint8_t)v; }
    std::vector<int> off((size_t)n_paths + 1);
    for (int &o : off) if (std::fscanf(f, "%d", &o) != 1) return 3;
    std::vector<float> pts(2 * (size_t)total);
    for (float &p : pts) { unsigned u; if (std::fscanf(f, "%u", &u) != 1) return 3; const uint32_t v = u; std::memcpy(&p, &v, 4); }
    std::fclose(f);

    long lookups = 0;
    auto cost = [&](int cx, int cy) -> float {       // raster_cost() of csrc/ufm_path.h
        ++lookups;
        if (cx < 0 || cy < 0 || cx >= L || cy >= W) return INFINITY;
        const int v = raster[(size_t)cx * W + cy];
        return v >= thr ? INFINITY : (float)v;
    };
    for (int i = 0; i < n_paths; ++i) {
        // the kernel's view of the offsets: clamped, a decreasing pair an empty path
        const int p0 = std::min(std::max(off[i], 0), total), p1 = std::min(std::max(off[i + 1], 0), total);
        const int nseg = p1 - p0 > 1 ? p1 - p0 - 1 : 0;
        const float *p = pts.data() + 2 * (size_t)p0;
        PathScore acc;
        int most_pieces = 0;
        long most_lookups = 0;
        for (int s = 0; s < nseg; ++s) {
            SegScore r{0.0, 0.0, 0.0, 0, 0};
            lookups = 0;
            if (acc.blocked_segment >= 0) r.dist = score_segment_dist(p[2 * s], p[2 * s + 1], p[2 * s + 2], p[2 * s + 3]);
            else r = score_segment(p[2 * s], p[2 * s + 1], p[2 * s + 2], p[2 * s + 3], L, W, cost);
            most_pieces = std::max(most_pieces, r.pieces);
            most_lookups = std::max(most_lookups, lookups);
            score_add_segment(acc, s, r);
        }
        Record o;
        score_narrow(acc, o);
        std::printf("%u %u %u %u %d %d %d %ld\n", bits(o.cost), bits(o.cost_before), bits(o.dist), bits(o.blocked_at), o.blocked_segment,
                    o.pieces, most_pieces, most_lookups);
    }
    return 0;
}
