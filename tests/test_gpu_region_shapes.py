"""-m gpu: the block replan kernel on blocks the map clips and on blocks that are not square -- where the tile-row division by
multiplication, the count of wake words a wave looks at and the frame's "outside the map" branches decide (csrc/ufm_region_rect.h;
tests/test_region_surface.py walks the same rules on the CPU).

Maps: 40 x 40 cells -- the block is the whole map, every tile of its frame lies outside -- and 40 x 100 cells -- ntx != nty.  Costs from
synth.cost_map.  Five 5 x 5 host patches, one replan each: the four corners and the middle.  The placed block is read from
ufm_stats.region_tiles, and every step must be ONE block-kernel launch.

After every step: FD level 1 and SG level 2 with "focused" = 0 -- the field bit for bit the field of the same script with "region" = 0
(the launch chain); MS-DFM level 1 ("focused" = 0, with and without "dfm_follow_info") and FD level 1 focused with heuristic keys --
against the oracle stepped alike, as tests/test_gpu_doors.py does (check_parity below the start's key: FD bit for bit, MS-DFM within
tolerances.DFM_RTOL / FIELD_RTOL); the layout self-check; ufm_check_info clean where the planner promises its bytes.

BOUNDS: none of this file's own."""
import functools

import numpy as np
import pytest

import ufm_amd
from helpers import ALGOS, make_pair, check_parity
from test_gpu_field_reference import device_planner

pytestmark = pytest.mark.gpu

TILE = 16                                  # the library's tile edge (UFM_TILE)
SEED = 11
MAPS = {"40x40": (40, 40), "40x100": (40, 100)}       # (length = rows, width = columns) in cells
PLANNERS = {"FD-1": ("FD", 1, {}), "SG-2": ("SG", 2, {}), "DFM-1": ("DFM", 1, {"dfm_follow_info": 0}), "DFM-1-follow": ("DFM", 1, {"dfm_follow_info": 1})}


@functools.lru_cache(maxsize=None)
def workload(shape):
    """(cost map, start, goal, the five steps (patch, top, left, start)), computed once per map and shared (nobody writes into them)"""
    length, width = MAPS[shape]
    cost = ufm_amd.synth.cost_map(SEED, width, length)
    cost.setflags(write=False)
    start, goal = ufm_amd.synth.start_goal(width, length)
    rng = np.random.default_rng(SEED)
    places = [(0, 0), (0, width - 5), (length - 5, 0), (length - 5, width - 5), (length // 2 - 2, width // 2 - 2)]
    steps = []
    for k, (top, left) in enumerate(places):
        patch = rng.integers(1, 201, (5, 5)).astype(np.uint8)
        patch[patch == cost[top:top + 5, left:left + 5]] += 1          # every cell of the patch changes
        patch.setflags(write=False)
        steps.append((patch, top, left, (start[0] + k + 1, start[1] + k + 1)))
    return cost, start, goal, tuple(steps)


def expected_block(p, algo):
    """tiles of the block Engine::step places: the knob's default edge (6; MS-DFM 8), clipped to the map"""
    ex, ey = p.dims()
    edge = 8 if algo == "DFM" else 6
    return min(edge, -(-ex // TILE)), min(edge, -(-ey // TILE))


def went_through_the_block(p, algo, shape, what):
    ntx, nty = expected_block(p, algo)
    st = p.stats
    print("%s: region_launches %d, region_tiles %d (block %d x %d)" % (what, st.region_launches, st.region_tiles, ntx, nty))
    assert st.region_launches == 1, "%s: the step did not go through the block kernel" % what
    assert st.region_tiles == ntx * nty, "%s: a block of %d tiles, expected %d x %d" % (what, st.region_tiles, ntx, nty)
    if shape == "40x40":
        assert (ntx, nty) == (3, 3)          # the whole map
    else:
        assert ntx == 3 and nty in (6, 7) and ntx != nty


def info_clean(p, name, what):
    if name != "DFM-1":                      # (without "dfm_follow_info" MS-DFM promises no bytes: test_gpu_doors.has_bytes)
        ci = p.check_info()
        assert ci[1:4] == (0, 0, 0), "%s: back-pointer self-check %r" % (what, ci)


@functools.lru_cache(maxsize=None)
def chain_fields(name, shape):
    """the script with "focused" = 0 and "region" = 0: the fields after every step"""
    algo, lvl, params = PLANNERS[name]
    cost, start, goal, steps = workload(shape)
    p = device_planner(algo, lvl, cost, start, goal, focused=0, region=0, **params)
    assert p.step() == 0
    out = []
    for patch, top, left, s in steps:
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
        assert p.stats.region_launches == 0
        g = p.read_field()[0]
        g.setflags(write=False)
        out.append(g)
    p.close()
    return tuple(out)


@pytest.mark.parametrize("shape", list(MAPS))
@pytest.mark.parametrize("name", ["FD-1", "SG-2"])
def test_unfocused_nodes_equal_the_launch_chain(name, shape):
    algo, lvl, params = PLANNERS[name]
    cost, start, goal, steps = workload(shape)
    ref = chain_fields(name, shape)
    p = device_planner(algo, lvl, cost, start, goal, focused=0, **params)
    assert p.step() == 0
    for k, (patch, top, left, s) in enumerate(steps):
        what = "%s %s step %d" % (name, shape, k)
        p.patch_map(patch, top, left); p.set_start(*s)
        assert p.step() == 0
        went_through_the_block(p, algo, shape, what)
        g = p.read_field()[0]
        differ = int((g.view(np.int32) != ref[k].view(np.int32)).sum())
        assert differ == 0, "%s: %d elements differ from the launch chain's field" % (what, differ)
        assert p.check_layout() == (0, 0), "%s: layout self-check %r" % (what, p.check_layout())
        info_clean(p, name, what)
    p.close()


def against_the_oracle(name, shape, heuristic, **params):
    algo, lvl, more = PLANNERS[name]
    cost, start, goal, steps = workload(shape)
    o, g = make_pair(ALGOS[algo], lvl, cost, start, goal, heuristic=heuristic, hm=float(cost.min()) if heuristic else 1.0)
    for k, v in dict(more, **params).items():
        g.set_param(k, v)
    assert o.step() == 0 and g.step() == 0
    cur = cost.copy()
    for k, (patch, top, left, s) in enumerate(steps):
        what = "%s %s%s step %d" % (name, shape, " heuristic" if heuristic else "", k)
        cur[top:top + 5, left:left + 5] = patch
        for p in (o, g):
            p.patch_map(patch, top, left)
            if heuristic:
                p.set_heuristic_multiplier(float(cur.min()))
            p.set_start(*s)
            assert p.step() == 0
        went_through_the_block(g, algo, shape, what)
        n, nbad = check_parity(o, g, what, below_start_key=True)      # (the layout self-check is in there)
        if algo != "DFM":
            assert nbad == 0, "%s: %d of %d trusted elements differ from the oracle" % (what, nbad, n)
        info_clean(g, name, what)
    g.close()


@pytest.mark.parametrize("shape", list(MAPS))
@pytest.mark.parametrize("name", ["DFM-1", "DFM-1-follow"])
def test_unfocused_cells_against_the_oracle(name, shape):
    against_the_oracle(name, shape, False, focused=0)


@pytest.mark.parametrize("shape", list(MAPS))
def test_focused_heuristic_keys_against_the_oracle(shape):
    against_the_oracle("FD-1", shape, True)
