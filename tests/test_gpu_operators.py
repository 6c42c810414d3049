"""-m gpu: the device functions of csrc/ufm_ops.h, one at a time, through the probe library (tests/hip/ops_probe.hip) on the constructed cases
of tests/operator_cases.py.

Device against oracle: bit for bit, no tolerance -- sqrt_rn against the correctly rounded float32 root, every triangle and every MS-DFM
candidate against orc_cost_via, every neighbourhood against orc_min_rhs_info (MS-DFM: against the smallest of its eight orc_cost_via
candidates, the operator both texts state).  Device against float64 (tests/field_reference.py): within tolerances.NODE_OPERATOR_ULP /
DFM_OPERATOR_ULP, which tests/test_operator_cases.py measures on the oracle.  The references come from that module, computed once per process.

What a field cannot show and these do: Field D*'s Type III clause at the level of one triangle (the oracle's values under its ablations
are REJECTED here, on a counted number of cases); TriFD::set against TriFD::set2; the tie rule on exact ties; sqrt_rn on its whole domain.

Each test makes one to three launches and stops at the first entry point that returns a HIP error."""
import ctypes
import functools

import numpy as np
import pytest

import field_reference as fr
import operator_cases as oc
import test_operator_cases as ref

pytestmark = pytest.mark.gpu

FD, SG, DFM1 = 0, 1, 3            # include/ufm.h: UFM_ALGO_FD, UFM_ALGO_SG; csrc/ufm_defs.h: ALGO_DFM1
ALGO = {"FD": FD, "SG": SG}
PITCHES = (3, 0)                  # 3, and 0 = the kernels' own LDS pitch GP


@functools.lru_cache(None)
def probe():
    lib = ctypes.CDLL(ref.PROBE)
    vp, i, n = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.ufm_probe_sqrt.argtypes = [vp, vp, n]
    lib.ufm_probe_tri.argtypes = [i, vp, vp, vp, vp, n, vp, vp, vp, vp]
    lib.ufm_probe_qdfm.argtypes = [vp, vp, vp, n, vp, vp]
    lib.ufm_probe_quad.argtypes = [i, i, vp, vp, n, vp, vp, vp, vp]
    lib.ufm_probe_quad_min.argtypes = [vp, vp, n, vp, vp]
    return lib


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def run(name, *args):
    rc = getattr(probe(), name)(*(a.ctypes.data if isinstance(a, np.ndarray) else a for a in args))
    assert rc == 0, "%s returned HIP error %d" % (name, rc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b, what):
    ne = bits(a) != bits(b)
    assert not ne.any(), "%s: %d of %d differ, first at %d: %r against %r" % (
        what, int(ne.sum()), ne.size, int(np.argmax(ne)), float(np.ravel(a)[np.argmax(ne)]), float(np.ravel(b)[np.argmax(ne)]))


def device_sqrt(x):
    x = f32(x)
    y = np.empty_like(x)
    run("ufm_probe_sqrt", x, y, len(x))
    return y


def test_sqrt_rn_is_the_correctly_rounded_root():
    """sqrt_rn == the float32 square root, bit for bit: on every float32 of [1, 4) and on every binade of the engine's arguments
    (operator_cases.square_roots); what 0 and +inf give is printed and only held not to be NaN"""
    s = oc.square_roots()
    for key in ("dense", "binades"):
        same(device_sqrt(s[key]), np.sqrt(s[key]), "sqrt_rn, " + key)
    edge = device_sqrt(s["edge"])
    print("sqrt_rn(0) = %r, sqrt_rn(+inf) = %r" % (float(edge[0]), float(edge[1])))
    assert not np.isnan(edge).any()


def device_triangles(name):
    t = ref.t_cases()
    n = len(t.g1)
    v = [np.empty(n, np.float32) for _ in range(3)]
    dep = np.empty(n, np.int32)
    run("ufm_probe_tri", ALGO[name], f32(t.g1), f32(t.g2), f32(t.c), f32(t.b), n, v[0], v[1], v[2], dep)
    return v, dep


@pytest.mark.parametrize("name", ["FD", "SG"])
def test_triangles(name):
    """T, one launch: tri_fd with the constants of TriFD::set, of set2's first and of set2's second slot (tri_sg for Shifted Grid) all equal
    orc_cost_via bit for bit; dep_fd / dep_sg is the float64 chain's dep wherever no comparison of that chain is near its turn.  Field D*:
    the oracle's values under each of its ablations -- Type III without its f^2 clause (1), paying c (8), no Type I (2), no c > b chain (4) --
    do NOT pass the same comparison, on exactly the cases the CPU test counted"""
    (v_set, v_set2v, v_set2h), dep = device_triangles(name)
    want = ref.t_oracle(name)
    same(v_set, want, name + ", constants of TriFD::set")
    same(v_set2v, v_set, name + ", TriFD::set2 (first slot) against set")
    same(v_set2h, v_set, name + ", TriFD::set2 (second slot) against set")
    _, dep64, firm = ref.t_float64(name)
    assert firm.sum() > 100000
    wrong = firm & (dep != dep64)
    assert not wrong.any(), "%s: dep differs from the float64 chain's on %d of %d firm cases, first %d" % (name, wrong.sum(), firm.sum(), np.argmax(wrong))
    if name == "FD":
        for a, differs in ref.ablation_differences().items():
            rejected = bits(v_set) != bits(ref.t_oracle("FD", a))
            print("ablation %d: the device rejects %d triangles" % (a, rejected.sum()))
            assert rejected.sum() >= ref.ABLATION_FLOOR and np.array_equal(rejected, differs), a


def test_q_dfm_candidates():
    """q_dfm on the inputs of each of the eight candidates of every MS-DFM case of Q == orc_cost_via through that neighbour, bit for bit;
    dep_dfm: both inputs exactly where the oracle's candidate leaves a pair of cells, else the smaller one"""
    q = ref.dfm_q()
    a, p, th = (f32(x.ravel()) for x in oc.dfm_candidates(q.g9, q.costs))
    v, dep = np.empty(len(a), np.float32), np.empty(len(a), np.int32)
    run("ufm_probe_qdfm", a, p, th, len(a), v, dep)
    cand, b = ref.dfm_q_oracle()[0], ref.dfm_q_candidate_cells()
    same(v.reshape(cand.shape), cand, "q_dfm against orc_cost_via")
    live = np.isfinite(cand) & np.isfinite(q.costs[:, :1])
    dep, nb = dep.reshape(cand.shape), ref.dfm_q_neighbour_index()
    pair = b[..., 1] >= 0
    assert ((dep == 3) == pair)[live].all(), "dep_dfm: the quadratic case"
    one = live & ~pair
    assert ((dep == 1) == (b[..., 0] == nb))[one].all() and np.isin(dep[one], (1, 2)).all(), "dep_dfm: the one-sided case"


def device_quads(algo, q, pitch):
    n = len(q.g9)
    rhs, rhs_w, via = (np.empty(n, np.float32) for _ in range(3))
    byte = np.empty(n, np.int32)
    run("ufm_probe_quad", algo, pitch, f32(q.g9), f32(q.costs), n, rhs, rhs_w, byte, via)
    return rhs, rhs_w, byte, via


def float64_bound(what, values, r, q, bound):
    """the device's values of the random and obstacle families against float64, with the window share capped"""
    for fam in (oc.WIDE, oc.NARROW, oc.OBSTACLES):
        ck = fr.check(values, r, bound, q.family == fam)
        print("%s family %d: worst %.3f ulp over %d, %d through the window" % (what, fam, ck.worst, ck.n, ck.windowed))
        assert ck.off == 0, "%s family %d: %d of %d off float64 by more than %d ulp, worst %.2f" % (what, fam, ck.off, ck.n, bound, ck.worst)
        assert ck.share <= fr.WINDOW_SHARE, (what, fam, ck.windowed, ck.n)


@pytest.mark.parametrize("name", ["FD", "SG"])
def test_quads(name):
    """Q, node planners, one launch per LDS pitch: quad_min(eval_quad) == quad_min(eval_quad_w) == the value through the chosen byte
    (eval_quad_bp) == orc_min_rhs_info, bit for bit, and the byte names the neighbour min_rhs<1> names -- the tie family first, under its own
    name.  A node without any finite candidate gives +inf; its byte is NOT BP_NONE: as k_finalize_bp chooses the winner (le.r == the
    quad's minimum) every lane of an all-+inf quad wins, and the byte names the last neighbour of neighbors_8 -- as min_rhs<1>'s
    `if (rhs == cost) bptr = ...` does on +inf == +inf, so the oracle's b0 is held there too.  (BP_NONE is what the engine stores for the
    goal and for elements no step has finalised.)"""
    q = ref.node_q()
    want, off = ref.node_q_oracle(name)
    out = [device_quads(ALGO[name], q, pitch) for pitch in PITCHES]
    for k in range(4):
        assert np.array_equal(out[0][k].view(np.int32), out[1][k].view(np.int32)), "%s: pitch 3 and the kernels' pitch differ in output %d" % (name, k)
    rhs, rhs_w, byte, via = out[0]
    assert ((byte >= 0) & (byte < 32)).all()
    named = oc.node_bp_neighbour(byte)
    ties = q.family == oc.TIES
    for mask, what in ((ties, "TIE RULE"), (~ties, "values")):
        same(rhs[mask], want[mask], "%s, %s: quad_min(eval_quad) against orc_min_rhs_info" % (name, what))
        same(rhs_w[mask], rhs[mask], "%s, %s: eval_quad_w against eval_quad" % (name, what))
        same(via[mask], rhs[mask], "%s, %s: the value through the chosen byte" % (name, what))
        wrong = mask & (named != off).any(axis=1)
        assert not wrong.any(), "%s, %s: the byte names another neighbour than min_rhs<1> on %d of %d cases, first %d: %r against %r" % (
            name, what, wrong.sum(), mask.sum(), np.argmax(wrong), named[np.argmax(wrong)].tolist(), off[np.argmax(wrong)].tolist())
    dead = np.isinf(q.g9).all(axis=1) | np.isinf(q.costs).all(axis=1)
    assert dead.sum() >= 24 and np.isposinf(rhs[dead]).all() and np.isposinf(via[dead]).all()
    float64_bound(name, rhs, ref.node_q_float64(name), q, ref.NODE_BOUND)


def test_quads_dfm():
    """Q, MS-DFM: rhs == rhs_w == via == the smallest of the eight orc_cost_via candidates, bit for bit -- the first hard pin on the MS-DFM
    operator: same inputs, so no evaluation order to hide behind --; the byte's axis neighbour names a candidate that attains it and its
    perpendicular cell holds the smaller value of that candidate's pair"""
    q = ref.dfm_q()
    cand, want, _ = ref.dfm_q_oracle()
    out = [device_quads(DFM1, q, pitch) for pitch in PITCHES]
    for k in range(4):
        assert np.array_equal(out[0][k].view(np.int32), out[1][k].view(np.int32)), "MS-DFM: pitch 3 and the kernels' pitch differ in output %d" % k
    rhs, rhs_w, byte, via = out[0]
    assert ((byte >= 0) & (byte < 64)).all()
    ties = q.family == oc.TIES
    axis, perp = oc.dfm_bp_cells(byte)
    k = np.argmax((np.array(oc.N8)[None] == axis[:, None]).all(axis=2), axis=1)
    idx = np.arange(len(k))
    _, p, _ = oc.dfm_candidates(q.g9, q.costs)
    for mask, what in ((ties, "TIE RULE"), (~ties, "values")):
        same(rhs[mask], want[mask], "MS-DFM, %s: quad_min(eval_quad) against the eight candidates' minimum" % what)
        same(rhs_w[mask], rhs[mask], "MS-DFM, %s: eval_quad_w against eval_quad" % what)
        same(via[mask], rhs[mask], "MS-DFM, %s: the value through the chosen byte" % what)
        same(cand[idx, k][mask], rhs[mask], "MS-DFM, %s: the candidate the byte's axis neighbour names" % what)
        got = q.g9[idx, (1 + perp[:, 0]) * 3 + 1 + perp[:, 1]]
        same(got[mask], p[idx, k][mask], "MS-DFM, %s: the byte's perpendicular cell against the smaller of the pair" % what)
    dead = np.isinf(np.delete(q.g9, 4, axis=1)).all(axis=1) | np.isinf(q.costs[:, 0])
    assert dead.sum() >= 24 and np.isposinf(rhs[dead]).all() and np.isposinf(via[dead]).all()
    float64_bound("MS-DFM", rhs, ref.dfm_q_float64(), q, ref.DFM_BOUND)


def test_quad_min():
    """quad_min / quad_min_int on full waves and a ragged tail: every lane holds its quad's minimum -- quads of distinct values, of equal
    values, with +inf in one to four lanes"""
    rng = np.random.default_rng(oc.SEED)
    n = 64 * 67 + 8                                           # 67 waves and two quads of a 68th
    v = rng.uniform(0.0, 1e6, (n // 4, 4)).astype(np.float32)
    v[100:200] = v[100:200, :1]                               # all four equal
    v[200:300, 1:3] = v[200:300, :1]                          # three equal
    for lanes in range(1, 5):
        rows = slice(300 + 100 * lanes, 400 + 100 * lanes)
        v[rows] = np.where(rng.permuted(np.tile(np.arange(4) < lanes, (100, 1)), axis=1), np.float32(np.inf), v[rows])
    vi = rng.integers(0, 0x400, (n // 4, 4)).astype(np.int32)
    vi[100:200] = 0x3FF
    vi[200:300] = vi[200:300, :1]
    out, outi = np.empty(n, np.float32), np.empty(n, np.int32)
    run("ufm_probe_quad_min", f32(v.ravel()), np.ascontiguousarray(vi.ravel()), n, out, outi)
    same(out, np.repeat(v.min(axis=1), 4), "quad_min")
    assert np.array_equal(outi, np.repeat(vi.min(axis=1), 4)), "quad_min_int"
