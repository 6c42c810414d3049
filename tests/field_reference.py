"""The three update operators as float64 functions of a whole field, written from their geometry: the checker of the local criterion
"every value G(s) is what the operator makes of the neighbours of s in the same field".

Nothing here is taken from oracle/*.c or from the engine's csrc/: the formulas are the planar geometry the reference's sources describe
(FieldDPlanner_impl.h / ShiftedGridPlanner_impl.h: compute_optimal_cost and fill_traversal_costs, InterpolatedTraversal.cpp: the Corner
costs, DynamicFastMarching_impl.h: min_rhs and compute_optimal_cost), evaluated in float64 with numpy over all elements at once.

NODE PLANNERS (Field D*, Shifted Grid).  Axes as the reference's: x runs along the raster's rows (length), y along its columns (width);
cell (i, j) is the unit square between the nodes (i, j) and (i + 1, j + 1).  Node s = (x, y) touches the four cells (x - 1 + dx, y - 1 + dy),
dx, dy in {0, 1}.  Each such cell c carries two triangles (s, p1, p2): p2 the cell's node diagonally opposite s, p1 one of the two nodes of
the cell next to s (along x, or along y).  A path leaves s, may first walk a distance t along the edge s-p1 inside the cell b on the OTHER
side of that edge (Field D* only, worth it only where b is cheaper than c), then crosses c in a straight line to the point at distance u
from p1 on the edge p1-p2, where the field is interpolated linearly:
    cost(t, u) = t * b + c * hypot(1 - t, u) + g1 + (g2 - g1) * u            0 <= t, u <= 1
The case chains pick the minimiser in closed form, with f = g1 - g2 (what walking the far edge from p1 to p2 gains):
    B    t = 0, u = 0: straight to p1                       g1 + c
    A    t = 0, u = 1: straight to p2                       g2 + c * sqrt 2
    II   t = 0, 0 < u < 1 where c u / hypot(1, u) = f       g1 + sqrt(c^2 - f^2)
    I    0 < t < 1, u = 1 where c (1-t) / hypot(1-t, 1) = b g2 + b + sqrt(c^2 - b^2)
    III  t = 1: along the edge to p1                        g1 + b
A cell's cost is its byte as a number, +inf at or above int(threshold * 255) (computed in float32, as the reference's Graph does) and
outside the map.  RHS(s) = the minimum over the eight triangles; RHS(goal) = 0.

MS-DFM.  Cell s with cost tau: the orthogonal stencil q(min(N, S), min(E, W), tau), the diagonal one q(min(NE, SW), min(NW, SE),
tau * sqrt 2), q(a, b, th) = (a + b + sqrt(2 th^2 - (a - b)^2)) / 2 where th > |a - b| -- the root of (T - a)^2 + (T - b)^2 = th^2 above
both -- and min(a, b) + th otherwise; RHS = the smaller of the two stencils.

COMPARISON WINDOW.  The chains decide by comparisons the planners make in float32.  Where the two sides of a comparison lie within
WINDOW_REL of each other, float32 may fall the other way, so the result carries the interval [lo, hi] spanned by the value and by the
chain with that one comparison inverted.  All but one of the comparisons sit where both branches agree (the cases are continuous there);
Field D*'s `f^2 <= sqrt(c^2 - b^2)` is a real discontinuity.  A checker that leans on the window hides failures: check() reports the
share of elements that needed it and every test holds that share to WINDOW_SHARE."""
import collections

import numpy as np

FD, SG, DFM = 0, 1, 2
WINDOW_REL = 1e-6
WINDOW_SHARE = 0.005
SQRT2 = np.sqrt(2.0)

# case numbers, in the order of oracle_py.CASES so that the two censuses read alike
FD_III, FD_III_SQ, FD_II_CGB, FD_I, FD_A_CGB, FD_B, FD_II, FD_A, SG_B, SG_II, SG_A = range(11)
CASE_NAMES = ("FD III (f <= 0)", "FD III (f^2 <= sqrt(c^2 - b^2))", "FD II (c > b)", "FD I", "FD A (c > b)", "FD B", "FD II (c <= b)",
              "FD A (c <= b)", "SG B", "SG II", "SG A")
FD_CASES, SG_CASES = tuple(range(0, 8)), tuple(range(8, 11))
FD_CANNOT_DECIDE = (FD_III, FD_III_SQ)          # see test_field_reference.test_type_iii_never_decides
DEP_P1, DEP_P2, DEP_BOTH = 1, 2, 3
_DEP = np.array([DEP_P1, DEP_P1, DEP_BOTH, DEP_P2, DEP_P2, DEP_P1, DEP_BOTH, DEP_P2, DEP_P1, DEP_BOTH, DEP_P2], np.int8)
# MS-DFM: case = 2 * stencil + form
ORTHO, DIAG = 0, 1
QUADRATIC, ONE_SIDED = 0, 1
DFM_CASE_NAMES = ("orthogonal quadratic", "orthogonal one-sided", "diagonal quadratic", "diagonal one-sided")

# the eight neighbours of a node in the order in which each one's counter-clockwise neighbour is the next (Graph::ccw_neighbor's tables)
RING = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))

Rhs = collections.namedtuple("Rhs", "value lo hi case dep stencil tied")
Rhs.__doc__ = """value: float64 RHS per element; [lo, hi]: the comparison window's interval around it (== value almost everywhere); case: the
winning triangle's / stencil's case; dep: node planners, what the winning case reads (DEP_*); stencil: MS-DFM, ORTHO / DIAG; tied: node
planners, bit mask of the cases whose triangles attain the minimum (equal float64 values)"""


def threshold_byte(thr):
    """Graph::set_occupancy_threshold: the float32 product, truncated"""
    return int(np.float32(thr) * np.float32(255.0))


def cell_costs(cost, thr):
    """the raster as float64 traversal costs, with a border of +inf cells: cell (i, j) is at [i + 1, j + 1]"""
    cost = np.asarray(cost)
    c = np.where(cost >= threshold_byte(thr), np.inf, cost.astype(np.float64))
    return np.pad(c, 1, constant_values=np.inf)


def _near(a, b):
    """the two sides of a comparison are close enough for float32 to decide it the other way"""
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= WINDOW_REL * np.maximum(np.abs(a), np.abs(b))


def _cath(h, k):
    """the other leg of a right triangle; nan -> only ever taken in a branch the comparisons exclude"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.maximum(h * h - k * k, 0.0))


class _Chain:
    """comparisons of a case chain, numbered in the order they are made; `flip` inverts one of them where its sides are near"""

    def __init__(self, flip):
        self.flip, self.k, self.used = flip, 0, False

    def __call__(self, result, lhs, rhs):
        k, self.k = self.k, self.k + 1
        if k != self.flip:
            return result
        near = _near(lhs, rhs)
        self.used = bool(near.any())
        return result ^ near


def _fd_chain(g1, g2, c, b, flip=None):
    """Field D*: (value, case) of a triangle"""
    cmp = _Chain(flip)
    with np.errstate(invalid="ignore", over="ignore"):
        f = g1 - g2                                   # +-inf where one of the two is; nan (both inf) is masked by the caller
        leg_b, leg_f = _cath(c, b), _cath(c, np.minimum(np.abs(f), c))
        cheaper_edge = cmp(c > b, c, b)
        down = cmp(f <= 0, f, np.zeros_like(f))
        iii_sq = cmp(f * f <= leg_b, f * f, leg_b)
        ii_a = cmp(f <= b, f, b) & cmp(c > f * SQRT2, c, f * SQRT2)
        i_ok = cmp(f > b, f, b) & cmp(c > b * SQRT2, c, b * SQRT2)
        ii_b = cmp(f * SQRT2 < c, f * SQRT2, c)
        v_b, v_a, v_ii = g1 + c, g2 + c * SQRT2, g1 + leg_f
        v_iii, v_i = g1 + b, g2 + b + leg_b
        case = np.where(cheaper_edge,
                        np.where(down, FD_III, np.where(iii_sq, FD_III_SQ, np.where(ii_a, FD_II_CGB, np.where(i_ok, FD_I, FD_A_CGB)))),
                        np.where(down, FD_B, np.where(ii_b, FD_II, FD_A)))
        value = np.choose(case, [v_iii, v_iii, v_ii, v_i, v_a, v_b, v_ii, v_a])
    return value, case, cmp.used or flip is None


def _sg_chain(g1, g2, c, b, flip=None):
    """Shifted Grid: no walk along the edge, b is not read"""
    cmp = _Chain(flip)
    with np.errstate(invalid="ignore", over="ignore"):
        f = g1 - g2
        down = cmp(f <= 0, f, np.zeros_like(f))
        inner = cmp(f * SQRT2 <= c, f * SQRT2, c)
        case = np.where(down, SG_B, np.where(inner, SG_II, SG_A))
        value = np.choose(case - SG_B, [g1 + c, g1 + _cath(c, np.minimum(np.abs(f), c)), g2 + c * SQRT2])
    return value, case, cmp.used or flip is None


_N_CMP = {FD: 8, SG: 2}


def triangle64(algo, g1, g2, c, b):
    """one triangle per array element: (value, lo, hi, case); +inf where both nodes are unreached or the cell cannot be crossed"""
    chain = _fd_chain if algo == FD else _sg_chain
    g1, g2, c, b = (np.asarray(a, np.float64) for a in (g1, g2, c, b))
    dead = (np.isinf(g1) & np.isinf(g2)) | np.isinf(c)
    value, case, _ = chain(g1, g2, c, b, None)
    value = np.where(dead, np.inf, value)
    lo, hi = value.copy(), value.copy()
    for k in range(_N_CMP[algo]):
        v, _, used = chain(g1, g2, c, b, k)
        if used:
            v = np.where(dead | np.isnan(v), value, v)
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return value, lo, hi, np.where(dead, -1, case)


def _at(padded, x, y):
    """padded[x + 1, y + 1] with everything beyond the one-element border reading as the border (+inf)"""
    return padded[np.clip(x + 1, 0, padded.shape[0] - 1), np.clip(y + 1, 0, padded.shape[1] - 1)]


def triangles_of(x, y, a, d):
    """the triangle of node (x, y) with the neighbours at offsets a and d (one beside the node, one diagonal, in either order; arrays):
    (p1, p2, cell c, cell b) as index arrays.  c is the cell holding all three nodes; b lies across the edge s-p1 from it."""
    a, d = (np.asarray(a[0]), np.asarray(a[1])), (np.asarray(d[0]), np.asarray(d[1]))
    a_diag = (a[0] != 0) & (a[1] != 0)
    p1 = (np.where(a_diag, d[0], a[0]), np.where(a_diag, d[1], a[1]))
    p2 = (np.where(a_diag, a[0], d[0]), np.where(a_diag, a[1], d[1]))
    cx, cy = x + np.minimum(p2[0], 0), y + np.minimum(p2[1], 0)
    along_x = p1[0] != 0                            # the edge s-p1 runs along x: the cell across it has the other y
    bx = np.where(along_x, cx, x + np.minimum(-p2[0], 0))
    by = np.where(along_x, y + np.minimum(-p2[1], 0), cy)
    return (x + p1[0], y + p1[1]), (x + p2[0], y + p2[1]), (cx, cy), (bx, by)


def via64(algo, cost, thr, field, x, y, bx, by):
    """nodes (x, y) through the triangle a stored back-pointer names: the node (bx, by) and its counter-clockwise neighbour.
    (value, lo, hi, case) per node."""
    gp, cp = np.pad(np.asarray(field, np.float64), 1, constant_values=np.inf), cell_costs(cost, thr)
    off = np.array(RING)
    slot = np.argmax((off[None, :, 0] == (bx - x)[:, None]) & (off[None, :, 1] == (by - y)[:, None]), axis=1)
    nxt = off[(slot + 1) % 8]
    p1, p2, c, b = triangles_of(x, y, (bx - x, by - y), (nxt[:, 0], nxt[:, 1]))
    return triangle64(algo, _at(gp, *p1), _at(gp, *p2), _at(cp, *c), _at(cp, *b))


def _node_rhs64(algo, cost, thr, field, goal):
    field = np.asarray(field, np.float64)
    nx, ny = field.shape
    assert (nx - 1, ny - 1) == np.asarray(cost).shape, "a node field is one larger than its raster each way"
    gp, cp = np.pad(field, 1, constant_values=np.inf), cell_costs(cost, thr)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    vals, los, his, cases = [], [], [], []
    for k in range(8):                              # the edge (RING[k], RING[k + 1]): every cell twice, once per node beside s
        p1, p2, c, b = triangles_of(x, y, (np.full_like(x, RING[k][0]), np.full_like(x, RING[k][1])),
                                    (np.full_like(x, RING[(k + 1) % 8][0]), np.full_like(x, RING[(k + 1) % 8][1])))
        v, lo, hi, case = triangle64(algo, _at(gp, *p1), _at(gp, *p2), _at(cp, *c), _at(cp, *b))
        vals.append(v); los.append(lo); his.append(hi); cases.append(case)
    vals, cases = np.stack(vals), np.stack(cases)
    value, win = vals.min(axis=0), vals.argmin(axis=0)
    case = np.take_along_axis(cases, win[None], 0)[0]
    tied = np.zeros(value.shape, np.int32)
    for k in range(8):
        tied |= np.where((vals[k] == value) & (cases[k] >= 0), 1 << np.maximum(cases[k], 0), 0).astype(np.int32)
    lo, hi = np.stack(los).min(axis=0), np.stack(his).min(axis=0)
    dep = np.where(case >= 0, _DEP[np.maximum(case, 0)], 0).astype(np.int8)
    if goal is not None:
        gx, gy = goal
        value[gx, gy] = lo[gx, gy] = hi[gx, gy] = 0.0
        case[gx, gy], dep[gx, gy], tied[gx, gy] = -1, 0, 0
    return Rhs(value, lo, hi, case, dep, None, tied)


def _q(a, b, th, flip):
    """one stencil: (value, form)"""
    with np.errstate(invalid="ignore", over="ignore"):
        lo, d = np.minimum(a, b), np.abs(a - b)
        d = np.where(np.isnan(d), np.inf, d)        # both unreached
        quad = th > d
        if flip:
            quad = quad ^ _near(th, d)
        root = (a + b + np.sqrt(np.maximum(2.0 * th * th - d * d, 0.0))) * 0.5
        value = np.where(quad, root, lo + th)
    return np.where(np.isnan(value), np.inf, value), np.where(quad, QUADRATIC, ONE_SIDED)


def _dfm_rhs64(cost, thr, field, goal, diagonal=True):
    field = np.asarray(field, np.float64)
    assert field.shape == np.asarray(cost).shape, "a cell field has its raster's shape"
    gp = np.pad(field, 1, constant_values=np.inf)
    tau = cell_costs(cost, thr)[1:-1, 1:-1]
    nx, ny = field.shape

    def nb(dx, dy):
        return gp[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny]

    pairs = [(np.minimum(nb(-1, 0), nb(1, 0)), np.minimum(nb(0, -1), nb(0, 1)), tau),
             (np.minimum(nb(-1, 1), nb(1, -1)), np.minimum(nb(-1, -1), nb(1, 1)), tau * SQRT2)]
    out = []
    for flip in (False, True):
        (vo, fo), (vd, fd) = (_q(a, b, th, flip) for a, b, th in pairs)
        if not diagonal:
            vd = np.full_like(vd, np.inf)
        out.append((vo, fo, vd, fd))
    vo, fo, vd, fd = out[0]
    stencil = np.where(vd < vo, DIAG, ORTHO)
    value = np.minimum(vo, vd)
    alt = np.minimum(out[1][0], out[1][2])
    # the stencils' own comparison (diagonal < orthogonal) picks the smaller value: either way the minimum
    lo, hi = np.minimum(value, alt), np.maximum(value, alt)
    case = 2 * stencil + np.where(stencil == DIAG, fd, fo)
    dead = np.isinf(tau) | np.isinf(value)
    value, lo, hi = (np.where(dead, np.inf, a) for a in (value, lo, hi))
    case = np.where(dead, -1, case)
    if goal is not None:
        gx, gy = goal
        value[gx, gy] = lo[gx, gy] = hi[gx, gy] = 0.0
        case[gx, gy] = -1
    return Rhs(value, lo, hi, case, None, np.where(case >= 0, stencil, -1), None)


def rhs64(algo, cost, thr, field, goal, diagonal=True):
    """The operator applied to every element of `field` (node planners: [length + 1][width + 1], MS-DFM: [length][width]) on the raster `cost`
    with occupancy threshold `thr`; goal = the goal element's (x, y) or None.  -> Rhs.  diagonal = False: MS-DFM without its diagonal
    stencil, for the test that shows the checker catching a wrong operator."""
    if algo == DFM:
        return _dfm_rhs64(cost, thr, field, goal, diagonal)
    return _node_rhs64(algo, cost, thr, field, goal)


def residual_ulp(field, rhs, window=True):
    """distance of every element of the float32 `field` from the operator's value (from its window interval), in units in the last place
    of the element; 0 where both are +inf, +inf where only one is"""
    field = np.asarray(field, np.float32)
    f64 = field.astype(np.float64)
    lo, hi = (rhs.lo, rhs.hi) if window else (rhs.value, rhs.value)
    with np.errstate(invalid="ignore"):
        dist = np.maximum(np.maximum(lo - f64, f64 - hi), 0.0)
        ulp = np.spacing(np.where(np.isfinite(field), np.maximum(np.abs(field), np.float32(1e-30)), np.float32(1))).astype(np.float64)
        res = dist / ulp
    both_inf = np.isinf(f64) & np.isinf(rhs.value) & (f64 > 0)
    return np.where(both_inf, 0.0, np.where(np.isnan(res), np.inf, res))


Check = collections.namedtuple("Check", "worst n off windowed share where")


def check(field, rhs, bound, mask=None):
    """the local criterion over the elements of `mask` (default: all): worst residual, how many were checked, how many lie off by more than
    `bound` ulp, how many are within it only through the comparison window (and their share), and the first offender's index"""
    mask = np.ones(np.shape(field), bool) if mask is None else mask
    strict, windowed = residual_ulp(field, rhs, window=False), residual_ulp(field, rhs, window=True)
    off = mask & ~(windowed <= bound)
    needed = mask & (windowed <= bound) & ~(strict <= bound)
    n = int(mask.sum())
    worst = float(windowed[mask].max()) if n else 0.0
    return Check(worst, n, int(off.sum()), int(needed.sum()), needed.sum() / max(n, 1), tuple(np.argwhere(off)[0]) if off.any() else None)


def fixed_point_dfm(cost, thr, goal, diagonal=True, sweeps=10000):
    """MS-DFM's field by this module's own operator: Jacobi iteration of rhs64 in float32 storage from the goal until nothing moves"""
    g = np.full(np.asarray(cost).shape, np.inf, np.float32)
    g[goal] = 0.0
    for _ in range(sweeps):
        new = np.minimum(g, rhs64(DFM, cost, thr, g, goal, diagonal=diagonal).value.astype(np.float32))
        if np.array_equal(new, g):
            return g
        g = new
    raise RuntimeError("no fixed point after %d sweeps" % sweeps)


def census(rhs, mask=None):
    """how often each case wins over the elements of `mask`.  Node planners: {case: (wins, decides)} -- wins: the minimum's first triangle has
    this case; decides: every triangle that attains the minimum has it.  MS-DFM: {case: wins}."""
    mask = np.ones(rhs.value.shape, bool) if mask is None else mask
    mask = mask & (rhs.case >= 0)
    if rhs.tied is None:
        return {k: int((rhs.case[mask] == k).sum()) for k in range(4)}
    return {k: (int((rhs.case[mask] == k).sum()), int((rhs.tied[mask] == (1 << k)).sum())) for k in range(11)}


GRID = 401
GRID_RESOLUTION = (1.0 / (GRID - 1)) ** 2 / 8.0
"""How far the brute-force minimum can lie ABOVE the true one, relative.  cost(t, u) is convex -- a linear function plus c times a
Euclidean norm -- and its minimum over the unit square lies on the square's border: inside, a zero gradient needs (b / c)^2 + (f / c)^2
= 1, and then the cost is constant along the ray towards p1, border included.  The border lines are grid lines.  Along u = 0 the cost is
linear in t: the minimiser is a corner, a grid point.  Along t = 0 and along u = 1 the straight leg is at least 1 long, so the second
derivative of c * hypot along the line is at most c, the nearest grid point is within h / 2 of the minimiser, where the derivative along
the line is zero or points out of the square: the grid point's cost exceeds the minimum by at most c (h / 2)^2 / 2 = c h^2 / 8, and the
minimum itself is at least c.  (t = 1 is the single path along the edge to p1.)"""


def geometric_min(algo, cost, thr, field, nodes, goal=None):
    """Node planners, CPU only: for each node of `nodes` ([n][2]) the cheapest path by brute force -- over the eight triangles and a
    GRID x GRID lattice of (distance walked along the edge s-p1, crossing point on p1-p2); Shifted Grid does not walk the edge."""
    gp, cp = np.pad(np.asarray(field, np.float64), 1, constant_values=np.inf), cell_costs(cost, thr)
    nodes = np.asarray(nodes)
    x, y = nodes[:, 0], nodes[:, 1]
    t = np.linspace(0.0, 1.0, GRID)[None, :, None]
    u = np.linspace(0.0, 1.0, GRID)[None, None, :]
    leg = np.hypot(1.0 - t, u)
    best = np.full(len(nodes), np.inf)
    for k in range(8):
        p1, p2, c, b = triangles_of(x, y, (np.full_like(x, RING[k][0]), np.full_like(x, RING[k][1])),
                                    (np.full_like(x, RING[(k + 1) % 8][0]), np.full_like(x, RING[(k + 1) % 8][1])))
        g1, g2, c, b = _at(gp, *p1), _at(gp, *p2), _at(cp, *c), _at(cp, *b)
        for i in np.flatnonzero(np.isfinite(c) & (np.isfinite(g1) | np.isfinite(g2))):
            walk = t * b[i] if (algo == FD and np.isfinite(b[i])) else np.where(t == 0, 0.0, np.inf)
            if np.isinf(g2[i]):
                far = np.where(u == 0, g1[i], np.inf)            # an unreached end: only the other end of the far edge has a value
            elif np.isinf(g1[i]):
                far = np.where(u == 1, g2[i], np.inf)
            else:
                far = g1[i] + (g2[i] - g1[i]) * u
            best[i] = min(best[i], float((walk + c[i] * leg + far).min()))
    if goal is not None:
        best[(x == goal[0]) & (y == goal[1])] = 0.0
    return best


def recipe_map(seed, length, width):
    """the fixture recipe of the field tests: white-noise costs 1 .. 254, 15 % lethal cells, cheap free corners for the start (0, 0) and the goal
    (length - 1, width - 1) -> (cost raster, start, goal)"""
    rng = np.random.default_rng(seed)
    cost = rng.integers(1, 255, (length, width), dtype=np.uint8)
    cost[rng.random((length, width)) < 0.15] = 255
    cost[0:2, 0:2] = 5
    cost[max(length - 2, 0):, max(width - 2, 0):] = 5
    return cost, (0.0, 0.0), (float(length - 1), float(width - 1))
