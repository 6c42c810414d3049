"""A float64 restatement of trajectory scoring (include/ufm_score.h), from the geometry alone: nothing of the engine is
imported, and the segment is not walked as csrc/ufm_score_rect.h walks it -- here ALL crossings of a segment with the grid lines are
collected first, sorted, and the stretches between neighbours examined in order; midpoints are the means of the stretch's two end
points; the sums are math.fsum's.  Cell costs follow path_cases._cell_cost: outside the raster or at / above the threshold is +inf.

score_path() also says whether a path is DOUBTFUL: some stretch it examined has a length in [2^-21, 2^-19], so close to the short-piece
threshold 2^-20 that two float64 evaluations of the same geometry may fall on different sides of it.  LIMITATION: the flag looks at
piece lengths only.  A segment that is almost parallel to a grid line without lying on it can keep a LONG piece within rounding
distance of that line, and the floor() of that piece's midpoint may then fall on either side between two float64 evaluations; such a
path is not flagged and would be held to exact `pieces` and `blocked_segment`.  No input of tests/score_cases.py is built that way;
a new input that is must be excluded by hand.  score_bound() is the bound of
ufm_amd.tolerances.SCORE_FP64_CHAIN."""
import math

import numpy as np

from path_cases import _cell_cost, ulp32

MIN_PIECE = 2.0 ** -20
DOUBT_LO, DOUBT_HI = 2.0 ** -21, 2.0 ** -19


def _cuts(a, d, hi):
    """parameters t in (0, 1) where a + t d crosses an integer line k, for the lines -1 .. hi + 1 (beyond them the walk is over)"""
    if d == 0.0:
        return []
    b = a + d
    lo_k = max(math.floor(min(a, b)), -1)
    hi_k = min(math.ceil(max(a, b)), hi + 1)
    out = []
    for k in range(int(lo_k), int(hi_k) + 1):
        t = (k - a) / d
        if 0.0 < t < 1.0:
            out.append(t)
    return out


def score_segment(a, b, cost, thr_uchar):
    """(cost of the pieces charged, length, pieces charged, blocked, t of the blocked piece, doubtful, dearest cell charged)"""
    length_cells, width_cells = cost.shape
    ax, ay, bx, by = (float(v) for v in (a[0], a[1], b[0], b[1]))
    if not all(math.isfinite(v) for v in (ax, ay, bx, by)):
        return 0.0, 0.0, 0, True, 0.0, False, 0.0
    dx, dy = bx - ax, by - ay
    dist = math.hypot(dx, dy)
    if not (0.0 <= ax <= length_cells and 0.0 <= ay <= width_cells):
        return 0.0, dist, 0, True, 0.0, False, 0.0
    if dist == 0.0:
        return 0.0, 0.0, 0, False, 0.0, False, 0.0
    ts = sorted(set([0.0, 1.0] + _cuts(ax, dx, length_cells) + _cuts(ay, dy, width_cells)))
    on_x = dx == 0.0 and ax == math.floor(ax)
    on_y = dy == 0.0 and ay == math.floor(ay)
    charges, pieces, doubtful, cmax = [], 0, False, 0.0
    for t0, t1 in zip(ts[:-1], ts[1:]):
        length = (t1 - t0) * dist
        if DOUBT_LO <= length <= DOUBT_HI:
            doubtful = True
        if length < MIN_PIECE:
            continue
        mx = 0.5 * ((ax + t0 * dx) + (ax + t1 * dx))
        my = 0.5 * ((ay + t0 * dy) + (ay + t1 * dy))
        if on_x:
            c = min(_cell_cost(cost, thr_uchar, int(ax) - 1, math.floor(my)), _cell_cost(cost, thr_uchar, int(ax), math.floor(my)))
        elif on_y:
            c = min(_cell_cost(cost, thr_uchar, math.floor(mx), int(ay) - 1), _cell_cost(cost, thr_uchar, math.floor(mx), int(ay)))
        else:
            c = _cell_cost(cost, thr_uchar, math.floor(mx), math.floor(my))
        if c == math.inf:
            return math.fsum(charges), dist, pieces, True, t0, doubtful, cmax
        charges.append(length * c)
        cmax = max(cmax, c)
        pieces += 1
    return math.fsum(charges), dist, pieces, False, 0.0, doubtful, cmax


def score_path(points, cost, thr_uchar):
    """the record of one polyline ([n, 2], any n >= 0) as a dict: cost (inf when blocked), cost_before, dist, blocked_at,
    blocked_segment (-1: free), pieces -- and doubtful, cmax (the dearest cell charged), mcoord (the largest finite |coordinate|),
    segments"""
    pts = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    costs, dists = [], []
    pieces, blocked_segment, blocked_at, doubtful, cmax = 0, -1, 0.0, False, 0.0
    for s in range(len(pts) - 1):
        if blocked_segment >= 0:
            a, b = pts[s], pts[s + 1]
            dists.append(math.hypot(b[0] - a[0], b[1] - a[1]) if np.isfinite(a).all() and np.isfinite(b).all() else 0.0)
            continue
        c, d, n, blocked, t, doubt, cm = score_segment(pts[s], pts[s + 1], cost, thr_uchar)
        costs.append(c)
        dists.append(d)
        pieces += n
        doubtful = doubtful or doubt
        cmax = max(cmax, cm)
        if blocked:
            blocked_segment, blocked_at = s, t
    total = math.fsum(costs)
    finite = np.abs(pts[np.isfinite(pts)])
    return {"cost": math.inf if blocked_segment >= 0 else total, "cost_before": total, "dist": math.fsum(dists),
            "blocked_at": blocked_at, "blocked_segment": blocked_segment, "pieces": pieces, "doubtful": doubtful, "cmax": cmax,
            "mcoord": float(finite.max()) if finite.size else 0.0, "segments": max(len(pts) - 1, 0)}


def score_bound(ref_value, pieces, cmax, mcoord, chain):
    """0.5 ulp32(ref) + pieces * Cmax * K * 2^-53 * max(M, 1) (ufm_amd.tolerances.SCORE_FP64_CHAIN is K)"""
    return 0.5 * ulp32(ref_value) + pieces * cmax * chain * 2.0 ** -53 * max(mcoord, 1.0)


def dist_bound(ref_value, segments, mcoord, chain):
    """the same form for the length: one "piece" per segment, charged 1"""
    return 0.5 * ulp32(ref_value) + segments * chain * 2.0 ** -53 * max(mcoord, 1.0)
