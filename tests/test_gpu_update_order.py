"""-m gpu: the order of mixed raster updates through every route a patch can take (Engine::route_patch, csrc/ufm_map_host.h, acting
on plan_patch of csrc/ufm_patch_route.h).  One sequence per handle -- a small host patch (held for the block kernel where the handle
allows it), a device patch over it, a reveal over both, another small host patch, a 66 x 40 host patch (too large to be held: staged),
a reveal at a corner -- on overlapping rectangles, so that any two updates applied in the wrong order, or one dropped, leave a wrong
byte.  The same sequence is replayed in numpy (Model of test_gpu_layers: the element-wise maximum over the layers, reveal_ref per
layer; dilate_ref for the footprint) and the rasters must be equal byte for byte, the census equal to np.bincount of the planning
raster; then one step, and ufm_check_layout finds no bad ring entry and no bad cost window.  Integer equality throughout: no tolerance."""
import numpy as np
import pytest

import ufm_amd
from helpers import DeviceBytes
from test_cspace_surface import dilate_ref
from test_gpu_layers import Model

pytestmark = pytest.mark.gpu

L, W = 70, 45                            # (length, width): partial 16 x 16 tiles both ways, more than one tile
FOOTPRINT = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 1]], np.uint8)     # 3 x 3, not symmetric: a reflected or transposed mask shows
SENSOR = np.ones((7, 7), np.uint8)
SENSOR[0, 0] = SENSOR[6, 5] = SENSOR[3, 3] = 0
MODES = ["plain", "cspace", "census", "cspace+census", "layers", "layers+cspace"]

_RASTERS = {}


def raster(seed, obstacles=False):
    if (seed, obstacles) not in _RASTERS:
        r = ufm_amd.synth.cost_map(seed, W, L, obstacles=obstacles)
        r.setflags(write=False)
        _RASTERS[(seed, obstacles)] = r
    return _RASTERS[(seed, obstacles)]


def patch_bytes(seed, h, w):
    return np.random.default_rng(seed).integers(1, 255, (h, w)).astype(np.uint8)


def check(what, read_map, read_raw_map, read_census, model, cspace, census):
    want = model.composed()
    if cspace:
        got = read_raw_map()
        assert np.array_equal(got, want), "%s: the raw raster differs from the replay in %d cells, first %r" % (
            what, int((got != want).sum()), tuple(np.argwhere(got != want)[0]))
        want = dilate_ref(want, FOOTPRINT)
    planning = read_map()
    assert np.array_equal(planning, want), "%s: the planning raster differs from the replay in %d cells, first %r" % (
        what, int((planning != want).sum()), tuple(np.argwhere(planning != want)[0]))
    if census:
        hist = read_census()[0]
        assert np.array_equal(hist, np.bincount(planning.ravel(), minlength=256).astype(np.uint64)), what


@pytest.mark.parametrize("mode", MODES)
def test_single_planner(mode):
    """FD level 1, 70 x 45 cells; with two layers the device patch goes to layer 1 and both layers have surveys"""
    cspace, census, n = "cspace" in mode, "census" in mode, 2 if "layers" in mode else 1
    start, goal = ufm_amd.synth.start_goal(W, L)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    g.reset(); g.set_occupancy_threshold(1.0)
    if n > 1:
        g.set_layers(n)
    if cspace:
        g.set_cspace(FOOTPRINT)
    if census:
        g.track_costs()
    g.set_map(raster(31, True)); g.set_start(*start); g.set_goal(*goal)
    g.set_sensor(SENSOR)
    model = Model(raster(31, True), n)
    for k in range(n):
        g.set_layer_survey(k, raster(131 + k)); model.surveys[k] = raster(131 + k)
    assert g.step() == 0
    held = []
    # 1. a small host patch
    a = patch_bytes(1, 7, 9)
    g.patch_map(a, 20, 10); model.patch_layer(0, a, 20, 10)
    # 2. a device patch over it
    b = patch_bytes(2, 10, 12)
    held.append(DeviceBytes(b))
    if n > 1:
        g.patch_layer(1, held[-1], 24, 13, w=12, h=10); model.patch_layer(1, b, 24, 13)
    else:
        g.patch_map_device(held[-1].data_ptr(), 24, 13, 12, 10); model.patch_layer(0, b, 24, 13)
    # 3. a reveal over both
    g.reveal(27, 16); model.reveal(SENSOR, None, 27, 16)
    # 4. another small host patch, over all three
    c = patch_bytes(4, 8, 6)
    g.patch_map(c, 25, 12); model.patch_layer(0, c, 25, 12)
    # 5. 66 x 40 from the host: rows 2 .. 67, columns 3 .. 42
    d = patch_bytes(5, 66, 40)
    g.patch_map(d, 2, 3); model.patch_layer(0, d, 2, 3)
    # 6. a reveal at a corner, clipped to 4 x 4
    g.reveal(0, 0); model.reveal(SENSOR, None, 0, 0)
    check(mode, lambda: g.read_map(W, L), lambda: g.read_raw_map(W, L), g.read_cost_census, model, cspace, census)
    for k in range(n if n > 1 else 0):
        assert np.array_equal(g.read_layer(k, W, L), model.layers[k]), "layer %d" % k
    g.set_start(start[0] + 2, start[1] + 1)
    assert g.step() == 0
    assert g.check_layout() == (0, 0)
    check(mode + ", after the step", lambda: g.read_map(W, L), lambda: g.read_raw_map(W, L), g.read_cost_census, model, cspace, census)
    g.close()


@pytest.mark.parametrize("mode", ["plain", "cspace+census"])
@pytest.mark.parametrize("defer", [0, 1], ids=["at_the_call", "deferred"])
def test_batch(defer, mode):
    """3 maps of 70 x 45: a host patch and then two device patches to map 0 in a row, all overlapping -- with "defer_patches" the second
    one meets the first still deferred and has it applied first --, a device patch to map 1 beside them, a reveal that skips map 1,
    a small host patch to map 2, the 66 x 40 host patch to map 1, a reveal of every map at a corner"""
    cspace, census = "cspace" in mode, "census" in mode
    start, goal = ufm_amd.synth.start_goal(W, L)
    b = ufm_amd.BatchPlanner(3, ufm_amd.ALGO_FD, 1, False)
    b.set_occupancy_threshold(1.0)
    b.set_param("defer_patches", defer)
    if cspace:
        b.set_cspace(FOOTPRINT)
    if census:
        b.track_costs()
    b.set_sensor(SENSOR)
    models = []
    for m in range(3):
        b.set_map(m, raster(41 + m, True)); b.set_start(m, *start); b.set_goal(m, *goal)
        b.set_survey(m, raster(141 + m))
        models.append(Model(raster(41 + m, True), 1)); models[m].surveys[0] = raster(141 + m)
    assert b.step() == 0
    held = []

    def host(m, seed, x, y, h, w):
        p = patch_bytes(seed, h, w)
        b.patch_map(m, p, x, y); models[m].patch_layer(0, p, x, y)

    def device(m, seed, x, y, h, w):
        p = patch_bytes(seed, h, w)
        held.append(DeviceBytes(p))
        b.patch_map_device(m, held[-1].data_ptr(), x, y, w, h); models[m].patch_layer(0, p, x, y)

    def reveal(centres):
        b.reveal(centres)
        for m, (row, col) in enumerate(centres):
            if row >= 0:
                models[m].reveal(SENSOR, None, row, col)

    host(0, 11, 20, 10, 7, 9)
    device(0, 12, 24, 13, 10, 12)
    device(0, 13, 22, 15, 9, 8)              # map 0 again: the clash
    device(1, 14, 30, 20, 11, 7)
    before = models[1].composed().copy()
    reveal([(27, 16), (-1, 0), (L - 1, W - 1)])
    assert np.array_equal(models[1].composed(), before)
    host(2, 15, L - 6, W - 8, 6, 8)          # over map 2's reveal
    host(1, 16, 2, 3, 66, 40)                # over map 1's device patch
    device(2, 17, L - 9, W - 12, 8, 10)
    reveal([(0, 0), (0, W - 1), (L - 1, 0)])
    for m in range(3):
        check("%s, map %d" % (mode, m), lambda: b.read_map(m, W, L), lambda: b.read_raw_map(m, W, L), lambda: b.read_cost_census(m),
              models[m], cspace, census)
    for m in range(3):
        b.set_start(m, start[0] + 2, start[1] + 1)
    assert b.step() == 0
    assert b.check_layout() == (0, 0)
    for m in range(3):
        check("%s, map %d after the step" % (mode, m), lambda: b.read_map(m, W, L), lambda: b.read_raw_map(m, W, L),
              lambda: b.read_cost_census(m), models[m], cspace, census)
    b.close()
