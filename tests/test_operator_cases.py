"""CPU: the constructed operator cases of tests/operator_cases.py -- that they cover what they claim, and the ORACLE on them against the
float64 operators of tests/field_reference.py.  tests/test_gpu_operators.py then holds the device functions of csrc/ufm_ops.h to the
oracle on the same cases, bit for bit, and to float64 within the bounds measured here.

The references are computed once per process (functools.lru_cache) and are not modified by any test.

SEED.  operator_cases.SEED = 20 is the committed seed.  Seeds 20, 21 and 22 were tried and behave alike; 20 is simply the first.  On each
the oracle needed the comparison window on no case of Q and of Shifted Grid's T, and on 660 / 618 / 685 of Field D*'s 455 175 triangles
(0.15 %), all of them at the boundary `f^2 = CATH(c, b)` -- the chain's one real discontinuity, where a case placed on the turn to the last
bit is decided by the rounding of f * f.  Worst residuals, node planners / MS-DFM: 1.493 / 1.830, 1.300 / 1.896, 1.357 / 1.974 ulp: the
same bounds (3 and 4) on all three."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import ufm_amd
from ufm_amd_pkg import capi
import field_reference as fr
import operator_cases as oc
import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(ufm_amd.library_path())
PROBE = os.path.join(PKG, "libufm_ops_probe.so")
PROBE_SYMBOLS = ["ufm_probe_qdfm", "ufm_probe_quad", "ufm_probe_quad_min", "ufm_probe_sqrt", "ufm_probe_tri"]
NODE_BOUND = ufm_amd.tolerances.NODE_OPERATOR_ULP
DFM_BOUND = ufm_amd.tolerances.DFM_OPERATOR_ULP
NODE = {"FD": (orc.ALGO_FD, fr.FD), "SG": (orc.ALGO_SG, fr.SG)}
ABLATIONS = (1, 2, 4, 8)          # oracle/ufm_oracle.h, orc_set_fd_ablation: without the f^2 <= CATH(c, b) clause; without Type I; without the c > b chain; Type III pays c
# Floors of the ablation counts on T, from the generator's construction, not from a run: 32 131 pairs have finite c > b.  Each of them meets
# f = 0 (offsets <= 0, three in five: f <= 0 -> Type III pays b, ablation 8 pays c > b) and f^2 = CATH(c, b) (offsets <= 0: the clause
# ablation 1 removes holds; without it the chain goes on to II, I or A); of those with c > b sqrt 2 (more than 20 000) each meets f = c and
# f = b sqrt 2 > b, where Type I decides (ablation 2); ablation 4 removes all of these.  A fifth of the smallest of these counts:
ABLATION_FLOOR = 4000
CENSUS_FLOOR = 50                 # each case wins on at least this many cases of Q ...
DECIDES_FLOOR = 10                # ... and is the only case at the minimum on at least this many


@functools.lru_cache(None)
def t_cases():
    return oc.triangles()


@functools.lru_cache(None)
def node_q():
    return oc.node_quads(t_cases())


@functools.lru_cache(None)
def dfm_q():
    return oc.dfm_quads()


def loaded_oracle(algo, raster, field):
    o = orc.OraclePlanner(algo, 1, False)
    o.reset(); o.set_occupancy_threshold(1.0); o.set_map(raster)
    o.load_g(field)
    return o


@functools.lru_cache(None)
def t_tiled():
    g9, costs, via = oc.triangle_blocks(t_cases())
    raster, field, xy = oc.tile_node(g9, costs)
    return raster, field, xy, (xy + via).astype(np.int32)


@functools.lru_cache(None)
def t_oracle(name, ablation=0):
    """orc_cost_via on every case of T (float32 [n]), under an ablation of Field D*'s chain if asked"""
    raster, field, xy, via = t_tiled()
    o = loaded_oracle(NODE[name][0], raster, field)
    L = orc.lib()
    try:
        L.orc_set_fd_ablation(ablation)
        v, b = o.cost_via_n(xy, via)
    finally:
        L.orc_set_fd_ablation(0)
    assert ablation or (b[:, 0] == via[:, 0] * field.shape[1] + via[:, 1]).all()
    v.setflags(write=False)
    return v


@functools.lru_cache(None)
def t_float64(name):
    """field_reference.triangle64 on T -> (Rhs with value, lo, hi, case; dep, firm of operator_cases.triangle_dep64)"""
    t = t_cases()
    v, lo, hi, case = fr.triangle64(NODE[name][1], t.g1, t.g2, t.c, t.b)
    dep, firm = oc.triangle_dep64(NODE[name][1], t.g1, t.g2, t.c, t.b)
    return fr.Rhs(v, lo, hi, case, None, None, None), dep, firm


@functools.lru_cache(None)
def node_q_tiled():
    q = node_q()
    return oc.tile_node(q.g9, q.costs)


@functools.lru_cache(None)
def node_q_oracle(name):
    """orc_min_rhs_info at every centre of Q: (values, offset of the neighbour b0 names [n][2])"""
    raster, field, xy = node_q_tiled()
    o = loaded_oracle(NODE[name][0], raster, field)
    v, b = o.min_rhs_info_n(xy)
    off = np.stack([b[:, 0] // field.shape[1], b[:, 0] % field.shape[1]], axis=1) - xy
    v.setflags(write=False)
    return v, off


@functools.lru_cache(None)
def node_q_candidates(name):
    """orc_cost_via through each of the eight neighbours (N8 order) at every centre of Q: float32 [n][8]"""
    raster, field, xy = node_q_tiled()
    o = loaded_oracle(NODE[name][0], raster, field)
    return np.stack([o.cost_via_n(xy, xy + np.array(d, np.int32))[0] for d in oc.N8], axis=1)


@functools.lru_cache(None)
def node_q_float64(name):
    raster, field, xy = node_q_tiled()
    r = fr.rhs64(NODE[name][1], raster, 1.0, field, None)
    return fr.Rhs(*(None if a is None else a[xy[:, 0], xy[:, 1]] for a in r))


@functools.lru_cache(None)
def dfm_q_tiled():
    q = dfm_q()
    return oc.tile_dfm(q.g9, q.costs)


@functools.lru_cache(None)
def dfm_q_oracle():
    """MS-DFM on Q: (the eight orc_cost_via candidates float32 [n][8] in N8 order, their minimum, orc_min_rhs_info)"""
    raster, field, xy = dfm_q_tiled()
    o = loaded_oracle(orc.ALGO_DFM, raster, field)
    cand = np.stack([o.cost_via_n(xy, xy + np.array(d, np.int32))[0] for d in oc.N8], axis=1)
    return cand, cand.min(axis=1), o.min_rhs_info_n(xy)[0]


@functools.lru_cache(None)
def dfm_q_candidate_cells():
    """the pair of cells each of the eight candidates leaves (orc_cost_via's b0, b1): int32 [n][8][2], linear indices in the tiled field"""
    raster, field, xy = dfm_q_tiled()
    o = loaded_oracle(orc.ALGO_DFM, raster, field)
    return np.stack([o.cost_via_n(xy, xy + np.array(d, np.int32))[1] for d in oc.N8], axis=1)


def dfm_q_neighbour_index():
    """linear index of each centre's eight neighbours in the tiled field: [n][8]"""
    raster, field, xy = dfm_q_tiled()
    nb = xy[:, None, :] + np.array(oc.N8, np.int32)[None]
    return nb[..., 0] * field.shape[1] + nb[..., 1]


@functools.lru_cache(None)
def dfm_q_float64():
    raster, field, xy = dfm_q_tiled()
    r = fr.rhs64(fr.DFM, raster, 1.0, field, None)
    return fr.Rhs(*(None if a is None else a[xy[:, 0], xy[:, 1]] for a in r))


def families(what):
    """(name, mask) of every family a bound is measured and asserted on, for "FD" / "SG" / "DFM": T by boundary, Q by sub-family"""
    if what == "DFM":
        return [("Q " + n, dfm_q().family == k) for k, n in enumerate(oc.DFM_FAMILIES)]
    return [("Q " + n, node_q().family == k) for k, n in enumerate(oc.NODE_FAMILIES)]


def oracle_residuals(what):
    """[(family, Check of the oracle's values against float64 at `bound`)] for "FD" / "SG" / "DFM", T first"""
    bound = DFM_BOUND if what == "DFM" else NODE_BOUND
    out = []
    if what != "DFM":
        r, _, _ = t_float64(what)
        v = t_oracle(what)
        for k, n in enumerate(oc.BOUNDARIES + ("unreached",)):
            out.append(("T " + n, fr.check(v, r, bound, t_cases().boundary == k)))
        v, r = node_q_oracle(what)[0], node_q_float64(what)
    else:
        v, r = dfm_q_oracle()[1], dfm_q_float64()
    for n, mask in families(what):
        out.append((n, fr.check(v, r, bound, mask)))
    return out


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_square_root_cases_cover_their_range():
    s = oc.square_roots()
    assert len(s["dense"]) == 1 << 24 and s["dense"][0] == 1.0 and s["dense"][-1] == np.nextafter(np.float32(4), np.float32(0))
    assert (np.diff(s["dense"].view(np.int32)) == 1).all()
    b = s["binades"]
    assert np.isfinite(b).all() and (b > 0).all() and b.min() >= 2.0 ** -126          # normal numbers only
    expo = np.floor(np.log2(b.astype(np.float64))).astype(int)
    for e in oc.SQRT_BINADES:
        assert (expo == e).sum() >= 4096 + 2 * 64, e
        for end in (2.0 ** e, float(np.nextafter(np.float32(2.0 ** (e + 1)), np.float32(0)))):
            assert (b == np.float32(end)).any(), (e, end)
    # the engine's range, from the call sites (docstring of square_roots)
    assert 2.0 ** oc.SQRT_BINADES[0] <= 0.5 and 4 * 254 ** 2 < 2.0 ** (oc.SQRT_BINADES[-1] + 1)
    root = np.sqrt(s["squares"].astype(np.float64))
    assert len(root) > 10000 and np.array_equal(root.astype(np.float32).astype(np.float64), root)


def test_triangle_cases_cover_every_pair_boundary_and_offset():
    t = t_cases()
    npairs = len(oc.COSTS) ** 2
    assert len(t.g1) == 7 * npairs
    fb = oc.boundary_f(t.c[:npairs], t.b[:npairs])
    for k, name in enumerate(oc.BOUNDARIES + ("unreached",)):
        m = t.boundary == k
        assert np.array_equal(np.sort(t.pair[m]), np.arange(npairs)), name            # every pair, once
        if k == oc.UNREACHED:
            assert set(t.offset[m]) == {0, 1, 2}
            assert (np.isinf(t.g1[m]) | np.isinf(t.g2[m])).all()
            continue
        assert np.array_equal(t.exists[m], np.isfinite(fb[k])), name                   # ... wherever the pair has that boundary
        ex = m & t.exists
        for off in oc.OFFSETS:
            for mag in oc.MAGNITUDES:
                hit = ex & (t.offset == off) & (t.g2 >= mag) & (t.g2 < 2 * mag)
                assert hit.sum() >= 500, (name, off, mag, int(hit.sum()))
        # the case sits where it claims: g1 within |offset| + 1 units in its last place of g2 + boundary
        want = t.g2[ex].astype(np.float64) + fb[k][t.pair[ex]]
        fin = np.isfinite(want)
        err = np.abs(t.g1[ex][fin].astype(np.float64) - want[fin]) / np.spacing(t.g1[ex][fin]).astype(np.float64)
        assert (err <= np.abs(t.offset[ex][fin]) + 1).all(), name
    for s in range(8):
        assert (t.slot == s).sum() > 40000


def test_every_case_wins_on_the_neighbourhoods():
    """field_reference.census over Q: each of the eleven node cases and of the four MS-DFM cases wins, and -- where DESIGN.md section 6 says
    a case can decide a value at all (not Field D*'s Type III) -- is the only case at the minimum (DECIDES_FLOOR)"""
    for name, cases_ in (("FD", fr.FD_CASES), ("SG", fr.SG_CASES)):
        cen = fr.census(node_q_float64(name))
        print(name, {fr.CASE_NAMES[k]: cen[k] for k in cases_})
        for k in cases_:
            assert cen[k][0] >= CENSUS_FLOOR, (fr.CASE_NAMES[k], cen[k])
            if k not in fr.FD_CANNOT_DECIDE:
                assert cen[k][1] >= DECIDES_FLOOR, (fr.CASE_NAMES[k], cen[k])
    cen = fr.census(dfm_q_float64())
    print("DFM", dict(zip(fr.DFM_CASE_NAMES, (cen[k] for k in range(4)))))
    assert all(cen[k] >= CENSUS_FLOOR for k in range(4)), cen


def test_tie_cases_tie_in_every_pair_of_positions():
    """the oracle's eight candidates on the tie family: two or more attain the minimum exactly, and every pair of the eight triangles
    (node planners) does so together somewhere; MS-DFM: every pair of neighbours on the same stencil"""
    for name in ("FD", "SG"):
        cand = node_q_candidates(name)[node_q().family == oc.TIES]
        at_min = (cand == cand.min(axis=1, keepdims=True)) & np.isfinite(cand)
        assert (at_min.sum(axis=1) >= 2).mean() > 0.9, name
        for i, j in oc.TIE_PAIRS:
            assert (at_min[:, i] & at_min[:, j]).sum() >= 10, (name, i, j)
    cand = dfm_q_oracle()[0][dfm_q().family == oc.TIES]
    at_min = (cand == cand.min(axis=1, keepdims=True)) & np.isfinite(cand)
    assert (at_min.sum(axis=1) >= 2).mean() > 0.5
    for i, j in oc.TIE_PAIRS:
        if (i % 2) == (j % 2):          # N8 alternates orthogonal / diagonal neighbours: the same stencil
            assert (at_min[:, i] & at_min[:, j]).sum() >= 10, (i, j)


def test_obstacle_cases_hold_the_dead_ends():
    q = node_q()
    m = q.family == oc.OBSTACLES
    allg, allc = np.isinf(q.g9[m]).all(axis=1), np.isinf(q.costs[m]).all(axis=1)
    assert (allg & ~allc).sum() >= 8 and (allc & ~allg).sum() >= 8 and (allg & allc).sum() >= 8
    for name in ("FD", "SG"):
        assert np.isinf(node_q_oracle(name)[0][m][allg | allc]).all()
    q = dfm_q()
    m = q.family == oc.OBSTACLES
    allg, dead = np.isinf(np.delete(q.g9[m], 4, axis=1)).all(axis=1), np.isinf(q.costs[m][:, 0])
    assert (allg & ~dead).sum() >= 8 and (dead & ~allg).sum() >= 8 and (allg & dead).sum() >= 8
    assert np.isinf(dfm_q_oracle()[1][m][allg | dead]).all()


# ---- the oracle against float64 ----------------------------------------------------------------------------------------------------
def report(what):
    rows = oracle_residuals(what)
    for n, ck in rows:
        print("%-3s %-22s %7d cases, worst %.3f ulp, %d through the window (%.3f %%)" % (what, n, ck.n, ck.worst, ck.windowed, 100 * ck.share))
    return rows


def window_shares(rows):
    """{family: (cases that needed the comparison window, cases)} -- T as one family (the families are S, T and Q): its boundary
    `f^2 = CATH(c, b)` is Field D*'s one real discontinuity, and a case placed on it to the last bit is decided by the rounding of f * f
    (about one in a hundred of that boundary's cases differ between float32 and float64); every sub-family of Q on its own"""
    out = {}
    for n, ck in rows:
        k = "T" if n.startswith("T ") else n
        a, b = out.get(k, (0, 0))
        out[k] = (a + ck.windowed, b + ck.n)
    return out


def test_oracle_is_the_float64_operator_on_every_family():
    for what in ("FD", "SG", "DFM"):
        rows = report(what)
        for n, ck in rows:
            assert ck.n > 0 and ck.off == 0, "%s %s: %d of %d off by more than the bound, worst %.2f ulp, first %r" % (what, n, ck.off, ck.n, ck.worst, ck.where)
        for n, (windowed, cases_) in window_shares(rows).items():
            print("%-3s %-22s window share %d of %d" % (what, n, windowed, cases_))
            assert windowed <= fr.WINDOW_SHARE * cases_, "%s %s: %d of %d lean on the comparison window" % (what, n, windowed, cases_)


def test_operator_bounds_are_the_measurement():
    """tolerances.NODE_OPERATOR_ULP / DFM_OPERATOR_ULP: twice the oracle's worst residual over the committed cases, rounded up to a whole
    ulp, and no less than the field bounds NODE_LOCAL_ULP / DFM_LOCAL_ULP -- measured on the oracle, never on the device"""
    worst = {"node": 0.0, "DFM": 0.0}
    for what in ("FD", "SG", "DFM"):
        k = "DFM" if what == "DFM" else "node"
        worst[k] = max([worst[k]] + [ck.worst for _, ck in oracle_residuals(what)])
    print("worst residual of the oracle on the operator cases: node planners %.3f ulp, MS-DFM %.3f ulp" % (worst["node"], worst["DFM"]))
    assert NODE_BOUND == max(ufm_amd.tolerances.NODE_LOCAL_ULP, math.ceil(2 * worst["node"])), worst
    assert DFM_BOUND == max(ufm_amd.tolerances.DFM_LOCAL_ULP, math.ceil(2 * worst["DFM"])), worst


def test_dfm_eight_candidates_against_the_stencil_minimum():
    """The minimum of the eight level-1 candidates (orc_cost_via) against min_rhs<0>'s "best cell of each pair, one quadratic per stencil"
    (orc_min_rhs_info).  Bit-equal on the random, tie and obstacle families.  On the boundary family th = d they part, as csrc/ufm_defs.h
    says of ALGO_DFM1: the float quadratic is not monotone -- the candidate built on the UNREACHED cell of an axis is the one-sided
    p + th, and at the turn the quadratic of (a, p) rounds one unit above it.  Never more than one unit, never the other way."""
    cand, low, info = dfm_q_oracle()
    fam = dfm_q().family
    differ = low != info
    print("eight candidates != stencil minimum on %d cases, by family %r" % (differ.sum(), np.bincount(fam[differ], minlength=5).tolist()))
    assert not differ[fam != oc.BOUNDARY].any()
    assert (low[differ] < info[differ]).all()
    assert (info[differ].view(np.int32) - low[differ].view(np.int32) == 1).all()


def ablation_differences(name="FD"):
    """{ablation: cases of T on which orc_cost_via under it differs from the operator's value}"""
    v = t_oracle(name)
    return {a: v.view(np.int32) != t_oracle(name, a).view(np.int32) for a in ABLATIONS}


def test_type_iii_shows_at_the_triangle():
    """No field can pin Field D*'s Type III: the ablations 1 and 8 leave every field as it is.  A single triangle's
    own value they cannot leave alone -- nor can 2 and 4.  These are the wrong values the device test must reject."""
    diff = ablation_differences()
    t = t_cases()
    for a, d in diff.items():
        print("ablation %d: %d of %d triangles differ; by boundary %r" % (a, d.sum(), len(d), np.bincount(t.boundary[d], minlength=7).tolist()))
        assert d.sum() >= ABLATION_FLOOR, (a, int(d.sum()))
    # what differs under 1 and 8 are Type III triangles of the float64 chain, or cases at its turn
    r, _, firm = t_float64("FD")
    for a in (1, 8):
        assert np.isin(r.case[diff[a] & firm], (fr.FD_III, fr.FD_III_SQ)).all()


# ---- build ---------------------------------------------------------------------------------------------------------------------------
def test_probe_builds_and_exports_its_entry_points():
    """`make libufm_ops_probe.so` is up to date or builds, and the library defines the ufm_probe_* functions and no other function of its own
    (what the toolchain adds -- HIP's registration symbols -- starts with an underscore)"""
    subprocess.check_call(["make", "-s", "-C", PKG, "libufm_ops_probe.so"])
    out = subprocess.check_output(["nm", "-D", "--defined-only", PROBE], text=True)
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split() and not line.split()[-1].startswith("_"))
    assert names == PROBE_SYMBOLS, names
    lib = ctypes.CDLL(PROBE)
    assert all(hasattr(lib, n) for n in PROBE_SYMBOLS)
    assert not any(hasattr(lib, n) for n in capi.SYMBOLS)
