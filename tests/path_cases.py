"""Directed inputs for the path extractor, a float64 reference of what an extraction must return, and the census floors.

Three things the tests of the extractor share (tests/test_path_cases.py on the CPU, tests/test_gpu_path_cases.py on the device):

* `directed_maps()` / `starts_for()`: seed-exact (ufm_amd.synth's hash) high-contrast rasters -- bimodal white noise, one-cell-wide
  cheap stripes in expensive ground, checkerboards, obstacle speckle, an occupancy threshold below 1 -- small enough that the oracle plans
  them in milliseconds, and per map a list of start positions: vertices, and points on cell edges at offsets k/16 (exact in fp32), the
  map borders included (rings with missing nodes).  Every map carries a 3 x 3 block of obstacles in its far corner and is planned FROM
  the middle of that block: none of the start elements ever gets a value, so the reference's end condition never holds, the queue
  drains and the oracle's field is final everywhere -- what `focused = 0` gives on the engine.  Each start then reads a final field.
  `found_inputs()` adds the (map, start) pairs tests/golden/search_path_cases.py found for what no generator produces often enough.

* `polyline_reference()`: the cost and the length of walking the returned way points over the raster, in float64, from nothing but the
  way points, the raster and the threshold -- no case table, no closed form.

* `FLOORS` / `census_shortfalls()`: how often each case, ring slot and special branch must have been taken for a comparison over the
  directed inputs to count as covering it.
"""
import json
import math
import os

import numpy as np

import oracle_py as orc
import ufm_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ALGOS = {"FD": 0, "SG": 1, "DFM": 2}
MAX_STEPS = 6
GOAL = (9.0, 11.0)


# ---------------------------------------------------------------------------------------------------------------- maps
def _u(seed, shape, mod):
    """hashed integers in [0, mod) per cell"""
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return (ufm_amd.synth.h64(seed, i, j) % np.uint64(mod)).astype(np.int64)


def _bimodal(seed, shape, hi=(60, 253), p_cheap_256=128):
    cheap = 1 + _u(seed ^ 0x11, shape, 5)
    dear = hi[0] + _u(seed ^ 0x22, shape, hi[1] - hi[0] + 1)
    return np.where(_u(seed ^ 0x33, shape, 256) < p_cheap_256, cheap, dear)


def make_map(kind, seed, length, width):
    """uint8 [length][width] and the occupancy threshold to plan it with"""
    shape = (length, width)
    thr = 1.0
    if kind == "bimodal":
        m = _bimodal(seed, shape)
    elif kind == "bimodal-sparse":          # few cheap cells: long detours along cell sides
        m = _bimodal(seed, shape, p_cheap_256=70)
    elif kind == "stripes":                 # one-cell-wide cheap stripes (period 3 / 4) in expensive ground
        m = 200 + _u(seed ^ 0x44, shape, 54)
        cheap = 1 + _u(seed ^ 0x55, shape, 5)
        i, j = np.meshgrid(np.arange(length), np.arange(width), indexing="ij")
        s = ((i % 3) == 1) | ((j % 4) == 2)
        m = np.where(s, cheap, m)
    elif kind == "checkerboard":
        i, j = np.meshgrid(np.arange(length), np.arange(width), indexing="ij")
        m = np.where((i + j) % 2 == 0, 1 + _u(seed ^ 0x66, shape, 5), 60 + _u(seed ^ 0x77, shape, 194))
    elif kind == "speckle":                 # bimodal with one cell in eight an obstacle
        m = _bimodal(seed, shape)
        m = np.where(_u(seed ^ 0x88, shape, 8) == 0, 255, m)
    elif kind == "low-threshold":           # threshold 0.5 -> every cost >= 127 is an obstacle
        m = _bimodal(seed, shape, hi=(60, 140))
        thr = 0.5
    else:
        raise ValueError(kind)
    m = m.astype(np.uint8)
    gx, gy = int(GOAL[0]), int(GOAL[1])
    m[gx - 1:gx + 1, gy - 1:gy + 1] = np.minimum(m[gx - 1:gx + 1, gy - 1:gy + 1], 5)     # the goal is reachable
    m[length - 3:, width - 3:] = 255                                                        # the block the plan starts from
    return np.ascontiguousarray(m), thr


def plan_start(cost):
    """the middle of the obstacle block: a start no planner ever reaches (see the module docstring)"""
    return float(cost.shape[0] - 2), float(cost.shape[1] - 2)


# (name, kind, seed, length, width)
MAP_SPECS = [
    ("bimodal-a", "bimodal", 101, 48, 48),
    ("bimodal-b", "bimodal", 102, 40, 56),
    ("bimodal-c", "bimodal", 103, 56, 40),
    ("sparse-a", "bimodal-sparse", 111, 48, 48),
    ("sparse-b", "bimodal-sparse", 112, 44, 52),
    ("stripes-a", "stripes", 121, 48, 48),
    ("checker-a", "checkerboard", 131, 48, 48),
    ("speckle-a", "speckle", 141, 48, 48),
    ("speckle-b", "speckle", 142, 40, 56),
    ("lowthr-a", "low-threshold", 151, 48, 48),
]


def directed_maps():
    """[(name, cost, thr)]"""
    return [(name,) + make_map(kind, seed, length, width) for name, kind, seed, length, width in MAP_SPECS]


def map_by_name(name):
    for n, kind, seed, length, width in MAP_SPECS:
        if n == name:
            return make_map(kind, seed, length, width)
    raise KeyError(name)


def starts_for(cost, seed, n_vertices=60, n_edges=300):
    """start positions (x, y): every vertex of the four borders' neighbourhood on a coarse lattice, hashed vertices, and hashed points
    on cell edges at k/16, k = 1..15 -- a third of them on or next to a border"""
    length, width = cost.shape
    out = []
    for x in (0, 1, length - 1, length):
        for y in range(0, width + 1, 7):
            out.append((float(x), float(y)))
    for y in (0, 1, width - 1, width):
        for x in range(3, length + 1, 7):
            out.append((float(x), float(y)))
    h = ufm_amd.synth.h64
    for k in range(n_vertices):
        out.append((float(int(h(seed, k, 1)) % (length + 1)), float(int(h(seed, k, 2)) % (width + 1))))
    for k in range(n_edges):
        frac = (1 + int(h(seed, k, 3)) % 15) / 16.0
        border = int(h(seed, k, 4)) % 3 == 0
        if int(h(seed, k, 5)) % 2:          # x fractional: a point on an edge that runs along x
            x = int(h(seed, k, 6)) % length
            y = (0, 1, width - 1, width)[int(h(seed, k, 7)) % 4] if border else int(h(seed, k, 7)) % (width + 1)
            if border and int(h(seed, k, 8)) % 2:
                x = (0, length - 1)[int(h(seed, k, 9)) % 2]
            out.append((x + frac, float(y)))
        else:
            y = int(h(seed, k, 6)) % width
            x = (0, 1, length - 1, length)[int(h(seed, k, 7)) % 4] if border else int(h(seed, k, 7)) % (length + 1)
            if border and int(h(seed, k, 8)) % 2:
                y = (0, width - 1)[int(h(seed, k, 9)) % 2]
            out.append((float(x), y + frac))
    return out


# what each planner's extractions are run with: FD and DFM with indirect traversals, SG with direct ones only (the reference's drivers)
INDIRECT = {"FD": True, "SG": False, "DFM": True}


def found_inputs():
    """[(algo, map name, (x, y), lookahead)] found by tests/golden/search_path_cases.py (opposite I, stuck after a move, ...)"""
    with open(os.path.join(HERE, "golden", "path_cases_found.json")) as f:
        return [(r["algo"], r["map"], (float(r["x"]), float(r["y"])), bool(r["lookahead"])) for r in json.load(f)["inputs"]]


def extraction_plan(algo):
    """every directed extraction of one planner: [(map name, cost, thr, [(start, lookahead), ...])]"""
    found = {}
    for a, name, start, la in found_inputs():
        if a == algo:
            found.setdefault(name, []).append((start, la))
    plan = []
    for k, (name, cost, thr) in enumerate(directed_maps()):
        jobs = [(s, bool((i + k) % 4)) for i, s in enumerate(starts_for(cost, 7000 + k))]      # one start in four without lookahead
        jobs += found.get(name, [])
        plan.append((name, cost, thr, jobs))
    return plan


def oracle_field(algo, cost, thr):
    """the oracle's final field of a map (RHS, dense) and its uchar threshold"""
    o = orc.OraclePlanner(ALGOS[algo], 0, False)
    o.reset()
    o.set_occupancy_threshold(thr)
    o.set_map(cost)
    o.set_start(*plan_start(cost))
    o.set_goal(*GOAL)
    assert o.step() == 0
    assert o.queue_size == 0, "the plan from inside the obstacle block must drain the queue"
    return o.rhs(), o.threshold_uchar()


# ------------------------------------------------------------------------------------------------- the float64 reference
def _cell_cost(cost, thr_uchar, cx, cy):
    if cx < 0 or cy < 0 or cx >= cost.shape[0] or cy >= cost.shape[1]:
        return math.inf
    v = int(cost[cx, cy])
    return math.inf if v >= thr_uchar else float(v)


def segment_reference(a, b, cost, thr_uchar):
    """(length, cheaper cost, dearer cost, on a grid line) of the straight segment a -> b (float64 pairs): the cost of the cell that
    holds its midpoint; a segment that lies on a grid line runs between two cells and may be charged either -- both are returned
    (a cell that is outside the raster or an obstacle cannot be charged: then both are the other one)."""
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    length = math.hypot(bx - ax, by - ay)
    mx, my = 0.5 * (ax + bx), 0.5 * (ay + by)
    if ax == bx and ax == math.floor(ax):
        c1, c2 = _cell_cost(cost, thr_uchar, int(ax) - 1, math.floor(my)), _cell_cost(cost, thr_uchar, int(ax), math.floor(my))
        line = True
    elif ay == by and ay == math.floor(ay):
        c1, c2 = _cell_cost(cost, thr_uchar, math.floor(mx), int(ay) - 1), _cell_cost(cost, thr_uchar, math.floor(mx), int(ay))
        line = True
    else:
        c1 = c2 = _cell_cost(cost, thr_uchar, math.floor(mx), math.floor(my))
        line = False
    lo, hi = min(c1, c2), max(c1, c2)
    if hi == math.inf:
        hi = lo
    return length, lo, hi, line


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


SLIDE = 2.0 ** -6           # how far polyline_reference() slides a way point to see that it sits at the minimum
EPS32 = 2.0 ** -24          # half an ulp of 1: the relative error of one correctly rounded fp32 operation
CLOSED_FORM_ROUNDINGS = 8   # the longest chain from the parameters to a step cost: 1 + p, * b, / CATH, 1 - (x); 1 - x, hypot, * c; the sum


def move_bound(n_segments, max_coord, max_cell_cost, step_cost):
    """How far the fp32 step costs of ONE move may lie from the float64 cost of its way points.

    The step costs are closed forms of the traversal's parameters (x, y, v, p, q); the way points are those parameters laid along a
    cell side, p0 + d * x with d = +-1, and rounded to fp32 at the magnitude M of the coordinate: each end point of a segment is off
    the closed form's point by at most ulp(M) / 2, along the side it lies on, so a segment's length by at most ulp(M), charged at no
    more than the dearest cell C the move touches: n_segments * ulp(M) * C.  The closed form itself is a chain of at most
    CLOSED_FORM_ROUNDINGS correctly rounded fp32 operations (the divisions, square roots and hypotf of the extractor are correctly
    rounded; CATH's squares of two uchar costs and their difference are exact) on lengths that never exceed the longest leg,
    hypot(1, 2): each contributes at most 2^-24 * sqrt(5) * C.  Errors IN the parameters do not enter: way points and step costs
    are made from the same rounded x, and the split point v of the three-point move sits at the minimum of the two legs' total
    length, where an error of v is of second order.  Last, the two step costs are added here in float64 and by the extractor in
    fp32: 2^-24 of their sum."""
    return (max_cell_cost * (n_segments * ulp32(max(max_coord, 1.0)) + CLOSED_FORM_ROUNDINGS * EPS32 * math.sqrt(5.0))
            + EPS32 * abs(step_cost))


def dist_bound(n_segments, total):
    """total_dist against the float64 length of the same fp32 way points: per segment the two coordinate differences, the
    hypotf and the running sum are rounded -- four roundings of at most 2^-24 * max(leg, running total) each"""
    return n_segments * 4 * EPS32 * max(math.sqrt(5.0), abs(total))


def polyline_reference(path, moves, cost, thr_uchar, indirect):
    """Hold one extraction -- (points, step_costs, total_cost, total_dist) -- to the raster.  `moves` says how the flat lists split
    into moves (rows of orc.path_move_log(): way points, step costs, kind, type, ...): a three-point move carries two step costs, so
    costs can only be compared per move.  Which cell a segment ON a grid line is charged: with indirect traversals always the cheaper
    one -- the extractor walks along a side only through Type III / I (conditions c > b ...: charged b, the cheaper) or B with
    c <= b (charged c); the same side seen from the other triangle swaps b and c and gives the same cell.  With direct traversals
    only, B charges the cell c of whichever triangle offered the move; the cheaper side's triangle always offers something at least
    as cheap, but when that something is a Type II the lookahead may reject it, so either cell is accepted.
    Returns a list of records (kind, type, deviation, bound) per real move; raises AssertionError on a violation."""
    pts, costs, total_cost, total_dist = path
    pts64 = np.asarray(pts, np.float64)
    costs64 = np.asarray(costs, np.float64)
    assert len(pts64) >= 1
    assert int(moves[:, 0].sum()) == len(pts64) - 1 and int(moves[:, 1].sum()) == len(costs64), "the move log does not describe this path"
    out = []
    ip, ic = 0, 0
    length_sum, cost_sum, last_step, nseg_total = 0.0, 0.0, 0.0, 0
    for mv in moves:
        ns, nc, kind, typ = int(mv[0]), int(mv[1]), int(mv[2]), int(mv[3])
        if ns == 0:
            cost_sum += last_step        # the reference adds the untouched step_cost of the previous move again
            continue
        lo_sum = hi_sum = 0.0
        cmax, mcoord = 0.0, 0.0
        for s in range(ns):
            a, b = pts64[ip + s], pts64[ip + s + 1]
            length, lo, hi, line = segment_reference(a, b, cost, thr_uchar)
            assert length == 0.0 or lo < math.inf, "segment %r -> %r crosses an obstacle or leaves the raster" % (tuple(a), tuple(b))
            if length > 0.0:
                lo_sum += length * lo
                hi_sum += length * (lo if indirect else hi)
                cmax = max(cmax, hi)
            length_sum += length
            mcoord = max(mcoord, abs(a).max(), abs(b).max())
        got = float(costs64[ic:ic + nc].sum())
        bound = move_bound(ns, mcoord, cmax, got)
        dev = min(abs(got - lo_sum), abs(got - hi_sum))
        out.append((kind, typ, dev, bound))
        assert dev <= bound, "move %d (%s %s, %d way points) from %r: step costs %r sum to %.9g, the way points cost %.9g%s; off by %.3g, bound %.3g" % (
            len(out) - 1, orc.PC_KINDS[kind], orc.PC_TYPES[typ], ns, tuple(pts64[ip]), list(costs64[ic:ic + nc]), got, lo_sum,
            "" if hi_sum == lo_sum else " (or %.9g)" % hi_sum, dev, bound)
        # A way point in the middle of a move (Types I and III over an edge: in along a cell side at the cheaper cell's cost, out
        # through the dearer cell) sits where the move is cheapest -- Snell's law, which the closed forms x = 1 - b / CATH(c, b) etc.
        # solve.  Slid along its side by +-SLIDE, the move must not get cheaper by more than the bound: a consistent but misplaced
        # way point (step costs that match the way points, both from a wrong x) shows up here and nowhere above.
        for s in range(ns - 1):
            w = pts64[ip + s + 1]
            for axis in (0, 1):
                if w[axis] == math.floor(w[axis]):
                    continue
                for d in (-SLIDE, SLIDE):
                    if math.floor(w[axis] + d) != math.floor(w[axis]) or w[axis] + d == math.floor(w[axis] + d):
                        continue        # would leave the cell side
                    moved = pts64[ip:ip + ns + 1].copy()
                    moved[s + 1][axis] += d
                    alt = sum(l * c for l, c, _, _ in (segment_reference(moved[i], moved[i + 1], cost, thr_uchar) for i in range(ns)) if l > 0.0)
                    assert alt >= lo_sum - 2 * bound, "move %d (%s %s) from %r: way point %r is misplaced, %+g along its side costs %.9g instead of %.9g" % (
                        len(out) - 1, orc.PC_KINDS[kind], orc.PC_TYPES[typ], tuple(pts64[ip]), tuple(w), d, alt, lo_sum)
        last_step = float(np.float32(costs64[ic:ic + nc].astype(np.float32).sum(dtype=np.float32))) if nc else 0.0
        cost_sum += last_step
        nseg_total += ns
        ip += ns
        ic += nc
    assert abs(total_dist - length_sum) <= dist_bound(nseg_total, length_sum), "total_dist %.9g, the way points measure %.9g" % (total_dist, length_sum)
    assert abs(total_cost - cost_sum) <= len(moves) * EPS32 * max(abs(cost_sum), 1.0), "total_cost %.9g, the step costs add up to %.9g" % (total_cost, cost_sum)
    return out


# ------------------------------------------------------------------------------------------------------------ the census
REACHABLE_INDIRECT = [(k, t) for k in orc.PC_KINDS for t in orc.PC_TYPES if (k, t) != ("opposite", "B")]
REACHABLE_DIRECT = [(k, t) for k in orc.PC_KINDS for t in ("II", "A", "B") if (k, t) != ("opposite", "B")]
FLOOR, FLOOR_OPPOSITE_I, FLOOR_STUCK = 25, 8, 5


def add_census(total, c):
    """accumulate a census dict (orc.path_census()) into `total`"""
    if not total:
        total.update({"chosen": dict(c["chosen"]), "won": dict(c["won"]), "ring": {k: list(v) for k, v in c["ring"].items()},
                      **{k: c[k] for k in c if k not in ("chosen", "won", "ring")}})
        return total
    for k in c["chosen"]:
        total["chosen"][k] += c["chosen"][k]
        total["won"][k] += c["won"][k]
    for k, v in c["ring"].items():
        total["ring"][k] = [a + b for a, b in zip(total["ring"][k], v)]
    for k in c:
        if k not in ("chosen", "won", "ring"):
            total[k] += c[k]
    return total


def census_shortfalls(indirect, direct, scale=1.0, stuck=True):
    """The floors (conditions, not measurements) against the census of the extractions with indirect traversals (FD, DFM) and of those
    with direct ones only (SG); `scale` 0.5 for a census on fields that are only close to the oracle's (MS-DFM on the device).
    `stuck` False leaves the stuck-after-a-move floor out: on node fields (FD, SG) no walk of the search
    (tests/golden/search_path_cases.py: every vertex and every point k/16 of every cell edge of all directed maps, two moves, with and
    without lookahead) stays put after a real move; on MS-DFM's node averages they do, and that is where the branch is covered.
    Returns the list of unmet floors as text (empty: all met)."""
    need = lambda n: int(math.ceil(n * scale))
    bad = []
    for k, t in REACHABLE_INDIRECT:
        for o in orc.PC_ORIENT:
            n = need(FLOOR_OPPOSITE_I if (k, t) == ("opposite", "I") else FLOOR)
            if indirect["won"][(k, t, o)] < n:
                bad.append("indirect: %s %s / %s won %d < %d" % (k, t, o, indirect["won"][(k, t, o)], n))
    for k, t in REACHABLE_DIRECT:
        n = sum(direct["won"][(k, t, o)] for o in orc.PC_ORIENT)
        if n < need(FLOOR):
            bad.append("direct: %s %s won %d < %d" % (k, t, n, need(FLOOR)))
    for ring, slots in indirect["ring"].items():
        for s, n in enumerate(slots):
            n += direct["ring"][ring][s]
            if n < need(FLOOR):
                bad.append("ring %s slot %d won %d < %d" % (ring, s, n, need(FLOOR)))
    for what, floor in (("la_rejected_winner", FLOOR), ("tie_break", FLOOR), ("stuck_after_move", FLOOR_STUCK)):
        if what == "stuck_after_move" and not stuck:
            continue
        n = indirect[what] + direct[what]
        if n < need(floor):
            bad.append("%s %d < %d" % (what, n, need(floor)))
    return bad


def census_table(indirect, direct, worst=None):
    """the census as text: won (chosen) per case, horizontal / vertical, indirect | direct; `worst`: {(kind, type): (deviation, bound)}"""
    lines = ["%-16s %-26s %-26s %s" % ("case", "indirect won(chosen) h / v", "direct won(chosen) h / v", "worst |cost - float64| (bound)" if worst else "")]
    for k in orc.PC_KINDS:
        for t in orc.PC_TYPES:
            cell = lambda c: " / ".join("%d(%d)" % (c["won"][(k, t, o)], c["chosen"][(k, t, o)]) for o in orc.PC_ORIENT)
            w = ""
            if worst and (k, t) in worst:
                w = "%.3g (%.3g)" % worst[(k, t)]
            lines.append("%-16s %-26s %-26s %s" % (k + " " + t, cell(indirect), cell(direct), w))
    for ring in ("vertex", "xfrac", "yfrac"):
        lines.append("ring %-11s %s" % (ring, " ".join(str(a + b) for a, b in zip(indirect["ring"][ring], direct["ring"][ring]))))
    for what in ("moves", "la_rejected_any", "la_rejected_winner", "tie_break", "stuck_after_move"):
        lines.append("%-16s %d" % (what, indirect[what] + direct[what]))
    return "\n".join(lines)
