// ufm_score_rect.h -- trajectory scoring (ufm_score_paths, include/ufm_score.h) as far as it is arithmetic: the walk
// of ONE straight segment over the raster -- where the grid lines cut it, which stretches count as pieces, which cell a piece is
// charged, where the walk is blocked -- and how the segments' results become the path's record.  Plain C++17, with or without HIP:
// k_score_paths (ufm_score.h) calls these functions one lane per segment, tests/cpp/score_rect_driver.cpp runs the same text on the
// host, under sanitizers, over a raster in a file.
//
// Coordinates are the reference's: x the row in 0 .. L, y the column in 0 .. W; cell (i, j) is [i, i + 1] x [j, j + 1].  The end points
// arrive as fp32 and everything from there on is fp64 (all fp32 values are fp64 values; the squares of the differences stay far below
// DBL_MAX).  The raster comes in as a callable cost(cx, cy) -> float: the byte of an inside cell below the occupancy threshold, +inf for
// anything else (raster_cost() of ufm_path.h) -- "+inf" is "cannot be charged".
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define SCORE_HD __host__ __device__
#else
#define SCORE_HD
#endif

// a stretch between two cuts shorter than this (cell sides) is no piece: neither charged nor able to block (UFM_SCORE_MIN_PIECE, 2^-20)
constexpr double SCORE_MIN_PIECE = 9.5367431640625e-07;

struct SegScore {
    double cost;      // sum of length x cost over the pieces charged, in walking order: all of them, or those before the blocked one
    double dist;      // length of the segment; 0 with a non-finite end point
    double t;         // blocked: the parameter in [0, 1] where the piece that cannot be charged begins
    int pieces;       // pieces charged
    int blocked;
};

// the length alone (what is left to do for the segments behind a blocked one)
SCORE_HD inline double score_segment_dist(float fax, float fay, float fbx, float fby) {
    const double ax = fax, ay = fay, bx = fbx, by = fby;
    if (!(std::isfinite(ax) && std::isfinite(ay) && std::isfinite(bx) && std::isfinite(by))) return 0.0;
    const double dx = bx - ax, dy = by - ay;
    return std::sqrt(dx * dx + dy * dy);
}

// The walk of the segment a -> b over a raster of L x W cells.
// BOUND: the loop below runs at most L + W + 2 times, whatever the end points are.  A walk begins inside [0, L] x [0, W] (anything else
// is blocked at t = 0 before the loop) and every turn of the loop but the last moves on to the next cut, a crossing with a line x = k or
// y = j in walking order.  While the walk is inside, those are lines 1 .. L-1 and 1 .. W-1 and, once, a border line: at most
// (L - 1) + (W - 1) + 1 cuts.  The stretch behind a border line has its midpoint outside the raster, cannot be charged and ends the
// walk.  That is L + W turns at the most; the counter allows two more and, should it ever run out, the walk is blocked where it
// stands -- no input makes it longer.
template <class Cost>
SCORE_HD inline SegScore score_segment(float fax, float fay, float fbx, float fby, int L, int W, Cost cost) {
    SegScore r{0.0, 0.0, 0.0, 0, 0};
    const double ax = fax, ay = fay, bx = fbx, by = fby;
    if (!(std::isfinite(ax) && std::isfinite(ay) && std::isfinite(bx) && std::isfinite(by))) { r.blocked = 1; return r; }
    const double dx = bx - ax, dy = by - ay;
    r.dist = std::sqrt(dx * dx + dy * dy);
    if (!(ax >= 0.0 && ax <= (double)L && ay >= 0.0 && ay <= (double)W)) { r.blocked = 1; return r; }
    if (dx == 0.0 && dy == 0.0) return r;
    // the next line each axis crosses, and the parameter of that crossing (beyond 1: none on this segment)
    const double NONE = 2.0;
    int kx = dx > 0.0 ? (int)std::floor(ax) + 1 : (int)std::ceil(ax) - 1;
    int ky = dy > 0.0 ? (int)std::floor(ay) + 1 : (int)std::ceil(ay) - 1;
    const int sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1;
    double tx = dx != 0.0 ? ((double)kx - ax) / dx : NONE;
    double ty = dy != 0.0 ? ((double)ky - ay) / dy : NONE;
    // a segment ON a grid line runs between two cells: every piece is charged the cheaper one that can be charged
    const bool on_x = dx == 0.0 && ax == std::floor(ax), on_y = dy == 0.0 && ay == std::floor(ay);
    double t0 = 0.0;
    for (int turn = 0; turn < L + W + 2; ++turn) {
        const double tn = std::fmin(std::fmin(tx, ty), 1.0);
        const double len = (tn - t0) * r.dist;
        if (len >= SCORE_MIN_PIECE) {
            const double tm = 0.5 * (t0 + tn), mx = ax + tm * dx, my = ay + tm * dy;
            // (a midpoint is never more than one cell outside the raster; anything else -- there is none -- would be "outside" too)
            const int cx = (mx >= -1.0 && mx <= (double)L + 1.0) ? (int)std::floor(mx) : -1;
            const int cy = (my >= -1.0 && my <= (double)W + 1.0) ? (int)std::floor(my) : -1;
            float c;
            if (on_x) c = std::fmin(cost((int)ax - 1, cy), cost((int)ax, cy));
            else if (on_y) c = std::fmin(cost(cx, (int)ay - 1), cost(cx, (int)ay));
            else c = cost(cx, cy);
            if (!(c < INFINITY)) { r.blocked = 1; r.t = t0; return r; }
            r.cost += len * (double)c;
            ++r.pieces;
        }
        if (tn >= 1.0) return r;
        if (tx <= tn) { kx += sx; tx = ((double)kx - ax) / dx; }
        if (ty <= tn) { ky += sy; ty = ((double)ky - ay) / dy; }
        t0 = tn;
    }
    r.blocked = 1; r.t = t0;      // (the bound above: not reached)
    return r;
}

// The path's record while its segments are added in index order: the sums stop at the first blocked segment, the length goes on.
struct PathScore {
    double cost = 0.0, dist = 0.0, t = 0.0;
    int blocked_segment = -1, pieces = 0;
};
SCORE_HD inline void score_add_segment(PathScore &p, int index, const SegScore &s) {
    p.dist += s.dist;
    if (p.blocked_segment >= 0) return;
    p.cost += s.cost;
    p.pieces += s.pieces;
    if (s.blocked) { p.blocked_segment = index; p.t = s.t; }
}
// fp64 -> fp32, once, into a record with ufm_score's members (include/ufm_score.h)
template <class Record>
SCORE_HD inline void score_narrow(const PathScore &p, Record &o) {
    o.cost = p.blocked_segment >= 0 ? INFINITY : (float)p.cost;
    o.cost_before = (float)p.cost;
    o.dist = (float)p.dist;
    o.blocked_at = (float)p.t;
    o.blocked_segment = p.blocked_segment;
    o.pieces = p.pieces;
}
