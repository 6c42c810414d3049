"""-m gpu: the block replan kernel publishes its result BEFORE it renews the back-pointer bytes (k_replan_region's tail, ufm_region.h): the
host leaves step() while the kernel still writes DevParams::bp.  Everything that reads those bytes is ordered behind the kernel on the
engine's stream -- these tests put each such reader directly behind a step, on the smallest maps on which the block kernel runs with an
interior block and with a clipped one: 160 x 160 for FD level 1 and SG level 2 (10 x 10 tiles, block 6 x 6), 192 x 192 for MS-DFM level 1
following its stored bytes (block 8 x 8).  31 x 31 patches five cells apart: consecutive blocks overlap almost entirely, so the next
kernel's staging reads the bytes the tail has just written.

Stored against derived back-pointers (ufm_read_info / ufm_read_info_derived): compared where the engine promises the two views to be one --
FD level 1, on the elements the step finalised (test_gpu_parity.test_back_pointer_view: SG level 2 derives its view from another candidate
structure, MS-DFM keeps the lowest code among tied candidates, and beyond the start's key a byte may name a parent that has moved on).
There the comparison is asserted, element by element; for SG level 2 and MS-DFM level 1 the share of agreeing finalised elements is held to
TIE_BOUND.  The count over the whole window is printed as well.  For every planner the byte self-check (ufm_check_info: the candidate a
byte names gives the element's value) runs over all elements, as a kernel of its own directly behind the tail."""
import functools

import numpy as np
import pytest

import ufm_amd
import oracle_py as orc
from helpers import ALGOS, make_pair, check_parity, dfm_close

pytestmark = pytest.mark.gpu

SEED = 7
PATCH, STRIDE = 31, 5
CASES = [("FD", 1, 160), ("SG", 2, 160), ("DFM", 1, 192)]
IDS = ["FD-1", "SG-2", "DFM-1"]
# SG level 2 and MS-DFM level 1: the share of the finalised elements on which the stored and the derived view must name the same parent.
# The two views part only where candidates tie (test_gpu_parity.test_back_pointer_view holds them to the same bound); a tail that had not
# run, or had run half, behind a replan leaves the bytes of the ~1 500 elements the replan changed as they were -- on these maps a
# tenth of the finalised elements of the window, which the self-check then reports one by one.
TIE_BOUND = 0.8


@functools.lru_cache(maxsize=None)
def workload(size, seed=SEED):
    """(cost map, start, goal, 12 scripted patches), computed once per size and seed and shared (nobody writes into them)"""
    cost = ufm_amd.synth.cost_map(seed, size, size)
    cost.setflags(write=False)
    start, goal = ufm_amd.synth.start_goal(size, size)
    script = tuple(ufm_amd.synth.replan_script(seed, size, size, n_patches=12, size=PATCH, stride=STRIDE))
    return cost, start, goal, script


def corner_script(size):
    """the scripted patches' bytes and starts, the patches themselves in three corners of the map in turn: every block is clipped on two sides"""
    _, _, _, script = workload(size)
    corners = [(0, 0), (size - PATCH, size - PATCH), (0, size - PATCH)]
    return tuple((k, s) + corners[i % 3] + (patch,) for i, (k, s, top, left, patch) in enumerate(script[:6]))


def pair(algo, lvl, size, **params):
    cost, start, goal, _ = workload(size)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal)
    if algo == "DFM":
        g.set_param("dfm_follow_info", 1)
    for name, v in params.items():
        g.set_param(name, v)
    assert o.step() == 0 and g.step() == 0
    return o, g, goal


def window(size, top, left, reach):
    """the patch and `reach` cells around it, clipped to the field: the block lies inside"""
    x0, y0 = max(0, top - reach), max(0, left - reach)
    return x0, y0, min(size, top + PATCH + reach) - x0, min(size, left + PATCH + reach) - y0


def bytes_at_once(g, x0, y0, nx, ny):
    """the two views of the back-pointers over a window, the stored one first: the first reader of DevParams::bp behind the step"""
    sto = g.read_info(x0, y0, nx, ny)
    return sto, g.read_info(x0, y0, nx, ny, derived=True)


def compare_views(algo, o, g, goal, sto, der, x0, y0, what):
    same = (sto == der).all(axis=2)
    field = g.read_field(x0, y0, *sto.shape[:2])[0]
    check = o.trusted_mask(below_start_key=True)[x0:x0 + sto.shape[0], y0:y0 + sto.shape[1]] & np.isfinite(field)
    gx, gy = int(round(goal[0])) - x0, int(round(goal[1])) - y0
    if 0 <= gx < check.shape[0] and 0 <= gy < check.shape[1]:
        check[gx, gy] = False
    print("%s: stored != derived on %d of %d elements of the window, on %d of %d finalised ones" % (
        what, int((~same).sum()), same.size, int((~same[check]).sum()), int(check.sum())))
    assert (sto[..., 0][check] >= 0).all(), "%s: %d finalised elements without a stored back-pointer" % (what, int((sto[..., 0][check] < 0).sum()))
    if algo == "FD":
        assert same[check].all(), "%s: stored and derived back-pointers differ on %d of %d finalised elements, first %r" % (
            what, int((~same[check]).sum()), int(check.sum()), tuple(np.argwhere(check & ~same)[0]))
    else:
        assert same[check].mean() > TIE_BOUND, "%s: stored and derived back-pointers agree on only %.3f of the %d finalised elements" % (
            what, same[check].mean(), int(check.sum()))


def check_all(algo, o, g, goal, what):
    n, nbad = check_parity(o, g, what, below_start_key=True)
    if algo != "DFM":
        assert nbad == 0, "%s: %d of %d trusted elements differ from the oracle" % (what, nbad, n)
    ci = g.check_info()
    assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)
    sto, der = bytes_at_once(g, 0, 0, None, None)
    compare_views(algo, o, g, goal, sto, der, 0, 0, what)


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_back_to_back(algo, lvl, size):
    """12 replans with nothing read between them (each kernel stages what the previous one's tail wrote), then everything: the field against the
    oracle stepped alike (FD / SG bit for bit below the start's key), the byte self-check, stored against derived back-pointers over the map"""
    o, g, goal = pair(algo, lvl, size)
    _, _, _, script = workload(size)
    r0, d0 = g.stats.region_replans, g.stats.region_replans_done
    for k, s, top, left, patch in script:
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
    print("block route: %d of %d steps, %d finished there" % (g.stats.region_replans - r0, len(script), g.stats.region_replans_done - d0))
    assert g.stats.region_replans - r0 == len(script)          # every step went through the block kernel ...
    assert g.stats.region_replans_done - d0 > 0                # ... and it finished steps alone: nothing but its tail wrote their bytes
    check_all(algo, o, g, goal, "after 12 replans")
    g.close()


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_read_at_once(algo, lvl, size):
    """after every step the stored bytes of the block's surroundings are read first thing (k_info_stored directly behind the tail) and compared
    with the derived view of the same field; the byte self-check over the map behind it"""
    o, g, goal = pair(algo, lvl, size)
    _, _, _, script = workload(size)
    r0 = g.stats.region_replans
    for k, s, top, left, patch in script:
        o.patch_map(patch, top, left); o.set_start(*s)
        assert o.step() == 0
        g.patch_map(patch, top, left); g.set_start(*s)
        assert g.step() == 0
        x0, y0, nx, ny = window(size, top, left, 8 * 16)
        sto, der = bytes_at_once(g, x0, y0, nx, ny)
        compare_views(algo, o, g, goal, sto, der, x0, y0, "replan %d" % k)
        ci = g.check_info()
        assert ci[1:4] == (0, 0, 0), "replan %d: back-pointer self-check %r" % (k, ci)
    assert g.stats.region_replans - r0 == len(script)
    check_all(algo, o, g, goal, "after 12 replans")
    g.close()


@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_not_done(algo, lvl, size):
    """a sweep budget of 16 per wave and phase: the block kernel gives up and the launch chain's invalidation follows the stored bytes
    directly behind the tail (continue_block / the adaptive rounds).  Everything checked after each of 6 replans."""
    o, g, goal = pair(algo, lvl, size, region_sweeps=16)
    _, _, _, script = workload(size)
    r0, d0 = g.stats.region_replans, g.stats.region_replans_done
    for k, s, top, left, patch in script[:6]:
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
        check_all(algo, o, g, goal, "replan %d" % k)
    runs, done = g.stats.region_replans - r0, g.stats.region_replans_done - d0
    print("block route: %d of 6 steps, %d finished there" % (runs, done))
    assert runs == 6 and done < runs                           # the block kernel ran every step and left at least one to the launch chain
    g.close()


@pytest.mark.parametrize("tiles", [0, 3], ids=["default-block", "3x3-block"])
@pytest.mark.parametrize("algo,lvl,size", CASES, ids=IDS)
def test_clipped_and_small_block(algo, lvl, size, tiles):
    """patches in the corners of the map (the block clipped on two sides), with the default block and with the smallest (region_tiles = 3)"""
    # (region_ahead 2: a block of three tiles then starts at the tile of the patch's centre, and the map's edge pushes it over the whole patch)
    o, g, goal = pair(algo, lvl, size, **({"region_tiles": tiles, "region_ahead": 2} if tiles else {}))
    r0 = g.stats.region_replans
    for k, s, top, left, patch in corner_script(size):
        for p in (o, g):
            p.patch_map(patch, top, left)
            p.set_start(*s)
            assert p.step() == 0
        x0, y0, nx, ny = window(size, top, left, 8 * 16)
        sto, der = bytes_at_once(g, x0, y0, nx, ny)
        compare_views(algo, o, g, goal, sto, der, x0, y0, "corner patch %d" % k)
        check_all(algo, o, g, goal, "corner patch %d" % k)
    assert g.stats.region_replans - r0 == 6                    # a 31 x 31 patch in a corner fits a block of 3 x 3 tiles put against the map's edge
    g.close()


def test_batch():
    """two maps of MS-DFM level 1 following its stored bytes, 192 x 192, a patch per map and round, 6 rounds: one launch, one workgroup per map,
    the one that is not the last runs its tail without publishing.  Fields against the oracles (dfm_close at its bound), the byte self-check
    through the batch entry point, after every round."""
    n, size, rounds = 2, 192, 6
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_DFM, 1, follow_info=True)
    b.set_occupancy_threshold(1.0)
    oracles, scripts = [], []
    for m in range(n):
        cost, start, goal, script = workload(size, 1000 + m)
        b.set_map(m, cost); b.set_start(m, *start); b.set_goal(m, *goal)
        o = orc.OraclePlanner(orc.ALGO_DFM, 1, False)
        o.reset(); o.set_occupancy_threshold(1.0); o.set_map(cost); o.set_start(*start); o.set_goal(*goal)
        assert o.step() == 0
        oracles.append(o); scripts.append(script)
    assert b.step() == 0
    r0 = b.stats.region_replans
    for r in range(rounds):
        for m, o in enumerate(oracles):
            k, s, top, left, patch = scripts[m][r]
            b.patch_map(m, patch, top, left); b.set_start(m, *s)
            o.patch_map(patch, top, left); o.set_start(*s)
            assert o.step() == 0
        assert b.step() == 0
        ci = b.check_info()
        assert ci[1:4] == (0, 0, 0), "round %d: back-pointer self-check %r" % (r, ci)
        for m, o in enumerate(oracles):
            mask = o.trusted_mask(below_start_key=True)
            assert int(mask.sum()) > 1000
            assert dfm_close(b.read_field(m)[mask], o.g()[mask], what="batch"), "round %d: map %d differs from its oracle" % (r, m)
    assert b.check_layout() == (0, 0)
    assert b.stats.region_replans - r0 == n * rounds           # every round was one block-kernel launch with a workgroup per map
    b.close()
