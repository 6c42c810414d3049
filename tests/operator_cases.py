"""Constructed inputs for the device update operators of csrc/ufm_ops.h, one function at a time (numpy only, seeded; shared by
tests/test_operator_cases.py on the CPU and tests/test_gpu_operators.py on the device).

A converged field only ever offers an operator the inputs fixed points produce.  The families here place inputs where the operators'
case chains turn, for every pair of cost bytes, and where their arithmetic has an edge:

  S  square roots      arguments of sqrt_rn                                             square_roots()
  T  single triangles  (g1, g2, c, b) of one triangle, around every boundary of its chain      triangles()
  Q  neighbourhoods    one 3 x 3 block of elements and the cells around its centre       node_quads(), dfm_quads()

Q cases -- and T cases, as one triangle in an otherwise unreached block -- are tiled into ONE field with stride 3 (tile_node, tile_dfm):
the centres' neighbourhoods do not overlap, so a single load of that field into the oracle and a single float64 evaluation
(field_reference.rhs64) serve all cases.  Cell costs are floats here, +inf for a lethal cell; tile_* turns them into bytes (255 = lethal at
threshold 1.0)."""
import collections

import numpy as np

import field_reference as fr

SEED = 20
INF = np.float32(np.inf)
SQRT2F = np.float32(1.41421356237309504880168872420969807856967187537694)
COSTS = np.concatenate([np.arange(1, 255, dtype=np.float32), [INF]])      # every traversable byte and the lethal cell
N8 = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))      # Graph::neighbors_8: top, top-left, left, ... , top-right
BP_CODE_TO_N8 = (1, 2, 0, 7, 4, 3, 5, 6)            # csrc/ufm_ops.h above bp_ref: code (q << 1) | h -> index in neighbors_8


def _step_ulp(x, k):
    """float32 x (positive, finite or +inf) moved by k units in the last place; +inf stays"""
    x = np.asarray(x, np.float32)
    bits = x.view(np.int32) + np.where(np.isfinite(x), k, 0).astype(np.int32)
    return bits.view(np.float32)


# ---- S ---------------------------------------------------------------------------------------------------------------------------
SQRT_BINADES = tuple(range(-1, 18))


def square_roots(seed=SEED):
    """S.  sqrt_rn's arguments.  Its three call sites and what they can pass where the result is used (cost bytes 1 .. 254):
      c^2 - b^2      with c > b (TriFD::set; set2 clamps the rest to 0): 3 (2^2 - 1^2) .. 254^2 - 1 = 64515
      c^2 - f^2      used where c > f sqrt 2, so at least c^2 / 2:        0.5 .. 254^2 = 64516
      2 th^2 - d^2   used where th > d, th = tau or tau sqrt 2:           above th^2 = 1 .. 4 * 254^2 = 258064
    -> [0.5, 258064]: the binades 2^-1 .. 2^17 (SQRT_BINADES).  Where the result is NOT used the argument may be negative, NaN, 0 (set2's
    clamp) or +inf (a lethal cell): no value is promised there, and none is asserted; EDGE records what 0 and +inf give.

    dense: every float32 in [1, 4).  Scaling the argument by 4 scales the root by 2, both exactly, so correct rounding on two adjacent
    binades carries to every normal binade -- as long as the routine does nothing that depends on the exponent; that is what `binades`
    watches: for each binade of the range its two ends with 64 neighbours on either side, 4096 seeded values, and every exact square
    (m^2 * 4^k, 2048 <= m < 4096: the roots that are floats, where a wrong neighbour choice cannot hide behind a tie)."""
    rng = np.random.default_rng(seed)
    dense = np.arange(0x3F800000, 0x40800000, dtype=np.uint32).view(np.float32)
    parts = []
    for e in SQRT_BINADES:
        lo, hi = np.float32(2.0 ** e), np.float32(2.0 ** (e + 1))
        for end in (lo, hi):
            parts.append(_step_ulp(np.full(129, end, np.float32), np.arange(-64, 65)))
        parts.append((lo + (hi - lo) * rng.random(4096)).astype(np.float32))
    m = np.arange(2048, 4096, dtype=np.float64) ** 2
    sq = (m[None, :] * 4.0 ** np.arange(-12, -1)[:, None]).ravel()
    sq = sq[(sq >= 2.0 ** SQRT_BINADES[0]) & (sq < 2.0 ** (SQRT_BINADES[-1] + 1))]
    assert np.array_equal(sq.astype(np.float32).astype(np.float64), sq)
    parts.append(sq.astype(np.float32))
    return {"dense": dense, "binades": np.concatenate(parts), "squares": sq.astype(np.float32), "edge": np.array([0.0, np.inf], np.float32)}


# ---- T ---------------------------------------------------------------------------------------------------------------------------
BOUNDARIES = ("f = 0", "f = b", "f sqrt 2 = c", "f^2 = CATH(c, b)", "f = c", "f = b sqrt 2")
UNREACHED = len(BOUNDARIES)          # the `boundary` number of the cases with g1, g2 or both at +inf
OFFSETS = (-2, -1, 0, 1, 2)
MAGNITUDES = (1.0, 1e3, 1e6)

Triangles = collections.namedtuple("Triangles", "g1 g2 c b boundary offset exists pair slot")


def boundary_f(c, b):
    """float64 [6][n]: the f = g1 - g2 at which a comparison of the chains turns for the cell costs (c, b), in the order of BOUNDARIES:
    0 (B / III against the rest), b (II against I), c / sqrt 2 (II against A), sqrt(CATH(c, b)) (Field D*'s `f^2 <= CATH(c, b)`), c (where
    c^2 - f^2 changes sign: the square root's argument, used or not), b sqrt 2 (the f at which Type I's own condition c > b sqrt 2 and
    Type II's c > f sqrt 2 meet).  nan where the pair has no such boundary (a lethal cell, CATH with c <= b)."""
    c, b = np.asarray(c, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        out = np.stack([np.zeros_like(c), b, c / fr.SQRT2, np.sqrt(np.sqrt(c * c - b * b)), c, b * fr.SQRT2])
    return np.where(np.isfinite(out), out, np.nan)


def triangles(seed=SEED):
    """T.  One triangle per case.  Every pair (c, b) of COSTS^2 (65 025 pairs) meets every boundary of its chain that exists for it once
    (BOUNDARIES), with g1 placed OFFSETS units in the last place of g1 from g2 + boundary -- the offset, g2's magnitude (MAGNITUDES, times
    1 .. 2) and the ring slot the triangle takes in its block drawn per case from the seeded generator, so every offset occurs at every
    boundary and at every magnitude thousands of times (counted by tests/test_operator_cases.py).  Where a pair lacks a boundary the case
    keeps a drawn f in [0, 300) (`exists` False).  One more case per pair has g1, g2 or both at +inf (boundary == UNREACHED, `offset` = which).
    7 x 65 025 = 455 175 cases, the same for Field D* and Shifted Grid (which does not read b)."""
    rng = np.random.default_rng(seed)
    c, b = (a.ravel() for a in np.meshgrid(COSTS, COSTS, indexing="ij"))
    npairs = len(c)
    fb = boundary_f(c, b)
    exists = np.isfinite(fb)
    f = np.where(exists, fb, rng.uniform(0.0, 300.0, fb.shape))
    off = rng.integers(OFFSETS[0], OFFSETS[-1] + 1, fb.shape)
    g2 = (np.array(MAGNITUDES)[rng.integers(0, len(MAGNITUDES), fb.shape)] * (1.0 + rng.random(fb.shape))).astype(np.float32)
    g1 = _step_ulp((g2.astype(np.float64) + f).astype(np.float32), off)
    which = rng.integers(0, 3, npairs)                     # 0: g1 unreached, 1: g2, 2: both
    u1 = (np.array(MAGNITUDES)[rng.integers(0, 3, npairs)] * (1.0 + rng.random(npairs))).astype(np.float32)
    u2 = (u1.astype(np.float64) + rng.uniform(-100.0, 100.0, npairs)).clip(0.0).astype(np.float32)
    u1, u2 = np.where(which != 1, INF, u1), np.where(which != 0, INF, u2)
    n_b = len(BOUNDARIES)
    t = Triangles(g1=np.concatenate([g1.ravel(), u1]).astype(np.float32), g2=np.concatenate([g2.ravel(), u2]).astype(np.float32),
                  c=np.tile(c, n_b + 1), b=np.tile(b, n_b + 1),
                  boundary=np.concatenate([np.repeat(np.arange(n_b), npairs), np.full(npairs, UNREACHED)]),
                  offset=np.concatenate([off.ravel(), which]), exists=np.concatenate([exists.ravel(), np.ones(npairs, bool)]),
                  pair=np.tile(np.arange(npairs), n_b + 1), slot=rng.integers(0, 8, (n_b + 1) * npairs))
    return t


def triangle_blocks(t):
    """the cases of T as neighbourhoods: the triangle (centre, RING[slot], RING[slot + 1]) of a 3 x 3 block of nodes holds g1 at its node
    beside the centre and g2 at its diagonal one, every other node is unreached; the cell inside the triangle costs c, the one across the
    edge centre-p1 costs b, the other two 7.  -> (g9 [n][9], costs [n][4] as [dx][dy], via [n][2]: the offset of RING[slot], the
    back-pointer whose triangle this is)"""
    n = len(t.g1)
    ring = np.array(fr.RING)
    a, d = ring[t.slot], ring[(t.slot + 1) % 8]
    one = np.ones(n, np.int64)
    p1, p2, cc, cb = fr.triangles_of(one, one, (a[:, 0], a[:, 1]), (d[:, 0], d[:, 1]))
    g9 = np.full((n, 9), INF, np.float32)
    idx = np.arange(n)
    g9[idx, p1[0] * 3 + p1[1]] = t.g1
    g9[idx, p2[0] * 3 + p2[1]] = t.g2
    costs = np.full((n, 4), np.float32(7.0), np.float32)
    costs[idx, cc[0] * 2 + cc[1]] = t.c
    costs[idx, cb[0] * 2 + cb[1]] = t.b
    return g9, costs, a


def triangle_dep64(algo, g1, g2, c, b):
    """the float64 chain's dep (field_reference.DEP_*; 0: no value) and `firm`: no comparison of the chain is near enough for float32 to
    take another case (inverting it, where its sides lie within field_reference.WINDOW_REL, leaves the case as it is)"""
    chain = fr._fd_chain if algo == fr.FD else fr._sg_chain
    g1, g2, c, b = (np.asarray(a, np.float64) for a in (g1, g2, c, b))
    dead = (np.isinf(g1) & np.isinf(g2)) | np.isinf(c)
    _, case, _ = chain(g1, g2, c, b, None)
    firm = ~dead
    for k in range(fr._N_CMP[algo]):
        _, alt, used = chain(g1, g2, c, b, k)
        if used:
            firm &= alt == case
    return np.where(dead, 0, fr._DEP[case]), firm


# ---- Q, node planners ------------------------------------------------------------------------------------------------------------
Quads = collections.namedtuple("Quads", "g9 costs family")
NODE_FAMILIES = ("random wide", "random narrow", "boundary triangles", "ties", "obstacles")
DFM_FAMILIES = ("random wide", "random narrow", "boundary th = d", "ties", "obstacles")
WIDE, NARROW, BOUNDARY, TIES, OBSTACLES = range(5)
TIE_PAIRS = tuple((i, j) for i in range(8) for j in range(i + 1, 8))


def _random_costs(rng, shape, lethal):
    c = rng.integers(1, 255, shape).astype(np.float32)
    c[rng.random(shape) < lethal] = INF
    return c


def _random_g(rng, n, narrow, unreached):
    if narrow:
        g = (rng.uniform(0.0, 1000.0, (n, 1)) + rng.uniform(0.0, 3.0, (n, 9))).astype(np.float32)
    else:
        g = rng.uniform(0.0, 300.0, (n, 9)).astype(np.float32)
    g[rng.random((n, 9)) < unreached] = INF
    return g


def _stack(parts):
    return Quads(np.concatenate([p[0] for p in parts]).astype(np.float32), np.concatenate([p[1] for p in parts]).astype(np.float32),
                 np.concatenate([np.full(len(p[0]), k) for k, p in enumerate(parts)]))


def node_quads(t, seed=SEED, n_random=20000, per_pair=100, n_obstacles=5000, boundary_stride=13):
    """Q for Field D* and Shifted Grid: per case the 3 x 3 nodes around a centre (row-major) and its four cells ([dx][dy]).
      random wide      g in [0, 300), 10 % unreached, costs 1 .. 254 with 10 % lethal: every triangle of the eight competes
      random narrow    g within 3 of each other on top of 0 .. 1000: the interpolating cases, the last bits of large values
      boundary         every boundary_stride-th case of T as a block (triangle_blocks): one triangle decides, at its chain's turns
      ties             uniform costs and symmetric g: for every pair of the eight triangles (TIE_PAIRS, ring slots) per_pair cases in which
                       both triangles hold the same g at their nodes beside the centre and the same g at their diagonal nodes -- the two
                       evaluate the same expression and tie exactly; and per_pair cases with all eight alike.  What wins is the tie rule's.
      obstacles        half the nodes unreached and half the cells lethal; every node unreached; every cell lethal; both"""
    rng = np.random.default_rng(seed + 1)
    wide = (_random_g(rng, n_random, False, 0.10), _random_costs(rng, (n_random, 4), 0.10))
    narrow = (_random_g(rng, n_random, True, 0.10), _random_costs(rng, (n_random, 4), 0.10))
    sub = Triangles(*(a[::boundary_stride] for a in t))
    bg9, bcosts, _ = triangle_blocks(sub)
    pairs = np.array(TIE_PAIRS + ((-1, -1),))
    k12 = np.repeat(pairs, per_pair, axis=0)
    n = len(k12)
    c = rng.integers(1, 255, n).astype(np.float32)
    a = rng.uniform(0.0, 500.0, n).astype(np.float32)
    d = (a.astype(np.float64) + rng.uniform(-1.5, 1.5, n) * c).clip(0.0).astype(np.float32)
    ring = np.array(fr.RING)
    tg9 = np.full((n, 9), INF, np.float32)
    idx = np.arange(n)
    for col in range(2):
        for k in range(8):
            use = (k12[:, col] == k) | (k12[:, col] < 0)
            for node in (ring[k], ring[(k + 1) % 8]):
                at = (1 + node[0]) * 3 + 1 + node[1]
                tg9[idx[use], at] = (d if node[0] != 0 and node[1] != 0 else a)[use]
    ties = (tg9, np.repeat(c[:, None], 4, axis=1))
    og9, ocosts = _random_g(rng, n_obstacles, False, 0.5), _random_costs(rng, (n_obstacles, 4), 0.5)
    og9[-24:-16] = INF
    ocosts[-16:-8] = INF
    og9[-8:] = INF; ocosts[-8:] = INF
    return _stack([wide, narrow, (bg9, bcosts), ties, (og9, ocosts)])


def tile_node(g9, costs):
    """the cases as one node field: case k's block at nodes (3i .. 3i + 2, 3j .. 3j + 2), (i, j) = divmod(k, side), its four cells at
    (3i + dx, 3j + dy); every other cell costs 1 and touches no centre.  -> (raster uint8 [3 side][3 side], field float32 one larger each way,
    centres int32 [n][2])"""
    n = len(g9)
    side = int(np.ceil(np.sqrt(n)))
    blocks = np.full((side * side, 3, 3), INF, np.float32)
    blocks[:n] = g9.reshape(n, 3, 3)
    field = np.full((3 * side + 1, 3 * side + 1), INF, np.float32)
    field[:-1, :-1] = blocks.reshape(side, side, 3, 3).transpose(0, 2, 1, 3).reshape(3 * side, 3 * side)
    cells = np.ones((side * side, 3, 3), np.uint8)
    cells[:n, :2, :2] = np.where(np.isinf(costs), 255, costs).astype(np.uint8).reshape(n, 2, 2)
    raster = np.ascontiguousarray(cells.reshape(side, side, 3, 3).transpose(0, 2, 1, 3).reshape(3 * side, 3 * side))
    k = np.arange(n)
    return raster, field, np.stack([3 * (k // side) + 1, 3 * (k % side) + 1], axis=1).astype(np.int32)


# ---- Q, MS-DFM -------------------------------------------------------------------------------------------------------------------
def dfm_quads(seed=SEED, n_random=10000, per_pair=60, n_obstacles=3000):
    """Q for MS-DFM: per case the 3 x 3 cells around a centre and the centre's cost tau in costs[:, 0].
      random wide / narrow   as for the node planners, tau 1 .. 254
      boundary th = d        for every tau, each of the eight neighbours a and each OFFSET: a's perpendicular pair holds p and +inf, with
                             |a - p| placed that many units in the last place of the larger from th (tau, or tau sqrt 2 on the diagonals) --
                             where q_dfm turns from the quadratic to min + th; all other cells unreached; both signs of a - p
      ties                   symmetric g: for every pair of the eight neighbours per_pair cases with the same g at both and one common g
                             at all other cells, and per_pair cases with all orthogonal cells alike and all diagonal cells alike
      obstacles              half the cells unreached; every cell unreached; a lethal centre; both"""
    rng = np.random.default_rng(seed + 2)

    def taus(n, lethal=0.0):
        c = np.ones((n, 4), np.float32)
        c[:, 0] = _random_costs(rng, n, lethal)
        return c

    wide = (_random_g(rng, n_random, False, 0.10), taus(n_random))
    narrow = (_random_g(rng, n_random, True, 0.10), taus(n_random))
    # boundary: tau x neighbour x offset x sign
    tau, nb, off, sign = (a.ravel() for a in np.meshgrid(np.arange(1, 255), np.arange(8), np.array(OFFSETS), np.array([0, 1]), indexing="ij"))
    n = len(tau)
    dxy = np.array(N8)[nb]
    diag = (dxy[:, 0] != 0) & (dxy[:, 1] != 0)
    th = np.where(diag, np.float32(tau) * SQRT2F, np.float32(tau)).astype(np.float32)
    lo = (np.array(MAGNITUDES)[rng.integers(0, 3, n)] * (1.0 + rng.random(n))).astype(np.float32)
    hi = _step_ulp((lo.astype(np.float64) + th).astype(np.float32), off)
    a_val, p_val = np.where(sign == 0, hi, lo), np.where(sign == 0, lo, hi)
    # one cell of the perpendicular pair, either one: the other axis for an orthogonal neighbour, the other diagonal for a diagonal one
    perp = np.where(diag[:, None], np.stack([dxy[:, 0], -dxy[:, 1]], axis=1), np.stack([dxy[:, 1], dxy[:, 0]], axis=1))
    perp = perp * np.where(rng.random(n) < 0.5, 1, -1)[:, None]
    bg9 = np.full((n, 9), INF, np.float32)
    idx = np.arange(n)
    bg9[idx, (1 + dxy[:, 0]) * 3 + 1 + dxy[:, 1]] = a_val
    bg9[idx, (1 + perp[:, 0]) * 3 + 1 + perp[:, 1]] = p_val
    bc = np.ones((n, 4), np.float32)
    bc[:, 0] = tau
    # ties
    pairs = np.array(TIE_PAIRS + ((-1, -1),))
    k12 = np.repeat(pairs, per_pair, axis=0)
    n = len(k12)
    a = rng.uniform(0.0, 500.0, n).astype(np.float32)
    rest = (a.astype(np.float64) + rng.uniform(-100.0, 300.0, n)).clip(0.0).astype(np.float32)
    tg9 = np.empty((n, 9), np.float32)
    n8 = np.array(N8)
    for k in range(8):
        at = (1 + n8[k, 0]) * 3 + 1 + n8[k, 1]
        is_diag = n8[k, 0] != 0 and n8[k, 1] != 0
        tg9[:, at] = np.where(k12[:, 0] < 0, rest if is_diag else a, np.where((k12[:, 0] == k) | (k12[:, 1] == k), a, rest))
    tg9[:, 4] = a
    tc = taus(n)
    og9, oc = _random_g(rng, n_obstacles, False, 0.5), taus(n_obstacles, 0.1)
    og9[-24:-16] = INF
    oc[-16:-8, 0] = INF
    og9[-8:] = INF; oc[-8:, 0] = INF
    return _stack([wide, narrow, (bg9, bc), (tg9, tc), (og9, oc)])


def tile_dfm(g9, costs):
    """the cases as one cell field: case k's block at cells (3i .. 3i + 2, 3j .. 3j + 2), the centre costs tau, every other cell 1.
    -> (raster uint8, field float32, centres int32 [n][2])"""
    n = len(g9)
    side = int(np.ceil(np.sqrt(n)))
    blocks = np.full((side * side, 3, 3), INF, np.float32)
    blocks[:n] = g9.reshape(n, 3, 3)
    field = np.ascontiguousarray(blocks.reshape(side, side, 3, 3).transpose(0, 2, 1, 3).reshape(3 * side, 3 * side))
    cells = np.ones((side * side, 3, 3), np.uint8)
    cells[:n, 1, 1] = np.where(np.isinf(costs[:, 0]), 255, costs[:, 0]).astype(np.uint8)
    raster = np.ascontiguousarray(cells.reshape(side, side, 3, 3).transpose(0, 2, 1, 3).reshape(3 * side, 3 * side))
    k = np.arange(n)
    return raster, field, np.stack([3 * (k // side) + 1, 3 * (k % side) + 1], axis=1).astype(np.int32)


def dfm_candidates(g9, costs):
    """the inputs of MS-DFM's eight per-neighbour candidates (DynamicFastMarching_impl.h:270-313), in N8 order: (a, p, th) float32 [n][8] --
    the neighbour's value, the smaller value of its perpendicular pair, tau times the stencil's step (1, or sqrt 2 in float32)"""
    g = g9.reshape(-1, 3, 3)
    a, p, th = (np.empty((len(g9), 8), np.float32) for _ in range(3))
    for k, (dx, dy) in enumerate(N8):
        a[:, k] = g[:, 1 + dx, 1 + dy]
        if dx * dy == 0:
            pair = ((0, -1), (0, 1)) if dx != 0 else ((-1, 0), (1, 0))
        else:
            pair = ((-1, -1), (1, 1)) if dx != dy else ((1, -1), (-1, 1))
        p[:, k] = np.minimum(g[:, 1 + pair[0][0], 1 + pair[0][1]], g[:, 1 + pair[1][0], 1 + pair[1][1]])
        th[:, k] = costs[:, 0] * (SQRT2F if dx * dy != 0 else np.float32(1.0))
    return a, p, th


def node_bp_neighbour(byte):
    """the offset (dx, dy) of the neighbour a node planner's back-pointer byte names ((code << 2) | dep; csrc/ufm_ops.h above bp_ref)"""
    return np.array(N8)[np.array(BP_CODE_TO_N8)[(np.asarray(byte) >> 2) & 7]]


def dfm_bp_cells(byte):
    """MS-DFM's byte (pp << 5) | (code << 2) | dep, code = (q << 1) | side: the offsets of the axis neighbour and of the perpendicular cell it
    names (QuadConsts<ALGO_DFM1>::load_at: axis q = 0 along x, 1 along y, 2 (+1, -1), 3 (+1, +1); the perpendicular pair 0: y, 1: x, 2: (+1, +1),
    3: (+1, -1); side / pp 0: minus, 1: plus)"""
    byte = np.asarray(byte)
    q, side, pp = (byte >> 3) & 3, (byte >> 2) & 1, (byte >> 5) & 1
    so = np.array([(1, 0), (0, 1), (1, -1), (1, 1)])[q]
    po = np.array([(0, 1), (1, 0), (1, 1), (1, -1)])[q]
    return so * np.where(side == 1, 1, -1)[:, None], po * np.where(pp == 1, 1, -1)[:, None]
