"""-m gpu: the engine's buffers under use (csrc/ufm_resources.h owns them; tests/test_resources.py is the leak check, on the CPU).

Growth: a handle that makes a call first small, then large -- so that the buffer behind the call is freed and made anew while the
handle is in use -- must answer the large call exactly like a fresh handle that makes only the large one.  Fields are compared whole
and bit for bit, so the planners run with "focused" 0: the converged field of Field D* is the unique fixed point, whatever the history
(with the end condition on, what lies beyond the start's key depends on how far each handle happened to get).  The scratch buffers
of the map side never hold fewer than 4096 bytes, and a 40 x 40 host patch is still small enough to be held for the block kernel:
the pairs with 40 x 40 patches and a radius-9 sensor therefore stay inside the first allocation, and each is followed by a third call
(a 70 x 70 patch, a radius-40 sensor) that does outgrow it, against a third, fresh handle.

Size changes: one handle with every optional feature on goes through three map sizes; what each feature promises is checked after
every one of them.  Create / use / destroy, 30 times in one process, with profiling on so that every event set exists: the same field
every time."""
import numpy as np
import pytest

import ufm_amd

pytestmark = pytest.mark.gpu

W, L = 96, 80                                    # width, length: rasters are [L][W]
COST = ufm_amd.synth.cost_map(3, W, L)
SURVEY = ufm_amd.synth.cost_map(13, W, L)
START, GOAL = (6.0, 5.0), (float(L - 7), float(W - 6))
ONES5 = np.ones((5, 5), np.uint8)


def planner(configure=None):
    """a Field D* level-1 planner that has planned COST, unfocused; configure(p) runs before the map is set"""
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    p.reset(); p.set_occupancy_threshold(1.0); p.set_param("focused", 0)
    if configure:
        configure(p)
    p.set_map(COST); p.set_start(*START); p.set_goal(*GOAL)
    assert p.step() == 0
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_raster_and_field(a, b, what, width=W, length=L):
    """the planning rasters are equal; one step of each later (it consumes what is pending) so are the whole fields"""
    assert np.array_equal(a.read_map(width, length), b.read_map(width, length)), what
    for p in (a, b):
        p.set_start(*START)
        assert p.step() == 0
    assert np.array_equal(bits(a.g()), bits(b.g())), what
    assert a.check_layout() == (0, 0) and b.check_layout() == (0, 0), what


def sorted_queue(q):
    xy, g, rhs, total = q
    order = np.lexsort((xy[:, 1], xy[:, 0]))
    return xy[order], bits(g[order]), bits(rhs[order]), total


def test_reads_grow_their_buffers():
    """read_field, read_info, read_queue, extract_paths_from: small, then large.  A patch that no step has consumed leaves elements
    whose value the new raster does not support: the queue view is not empty, and it is the same on both handles."""
    a, b = planner(), planner()
    for p in (a, b):
        p.patch_map(np.full((9, 9), 250, np.uint8), 36, 44)
    starts = np.random.default_rng(1).uniform([0.0, 0.0], [float(L), float(W)], (70, 2)).astype(np.float32)
    a.read_field(3, 4, 1, 1)
    a.read_info(3, 4, 2, 2)
    assert len(a.read_queue(cap=1)[0]) == 1
    a.extract_paths_from(starts[:1], max_steps=40)
    fa, fb = [(p.read_field()[0], p.read_info(), sorted_queue(p.read_queue()), p.extract_paths_from(starts, max_steps=40)) for p in (a, b)]
    assert np.array_equal(bits(fa[0]), bits(fb[0]))
    assert np.array_equal(fa[1], fb[1])
    assert fa[2][3] == fb[2][3] > 1                                           # the total: more than the first call's single record
    for x, y in zip(fa[2][:3], fb[2][:3]):
        assert np.array_equal(x, y)
    assert len(fa[3]) == len(fb[3]) == 70
    for (pa, ca, ta, da), (pb, cb, tb, db) in zip(fa[3], fb[3]):
        assert np.array_equal(bits(pa), bits(pb)) and np.array_equal(bits(ca), bits(cb)) and (ta, da) == (tb, db)
    a.close(); b.close()


# edge, first row, first column: each rectangle inside the next, so that the last patch alone decides the raster
NESTED = [(3, 38, 46), (40, 20, 28), (70, 5, 13)]
PATCH_CASES = {
    "host_patch": (None, lambda p, patch, x, y: p.patch_map(patch, x, y)),                         # the staging buffer
    "host_patch_footprint": (lambda p: p.set_cspace(ONES5), lambda p, patch, x, y: p.patch_map(patch, x, y)),    # ... and the dilated patch
    "layer_patch": (lambda p: p.set_layers(2), lambda p, patch, x, y: p.patch_layer(1, patch, x, y)),            # ... and the composed patch
}


@pytest.mark.parametrize("case", list(PATCH_CASES))
def test_patches_grow_their_buffers(case):
    configure, apply = PATCH_CASES[case]
    rng = np.random.default_rng(7)
    patches = [(rng.integers(1, 201, (e, e)).astype(np.uint8), x, y) for e, x, y in NESTED]
    a, b, c = planner(configure), planner(configure), planner(configure)
    apply(a, *patches[0]); apply(a, *patches[1])
    apply(b, *patches[1])
    same_raster_and_field(a, b, case + ": 3 x 3, then 40 x 40")
    apply(a, *patches[2])
    apply(c, *patches[2])
    same_raster_and_field(a, c, case + ": then 70 x 70")
    for p in (a, b, c):
        p.close()


def test_reveal_slots_grow_with_the_sensor():
    def configure(p):
        p.set_sensor(ufm_amd.sensor_disc(2))
    a, b, c = planner(configure), planner(lambda p: p.set_sensor(ufm_amd.sensor_disc(9))), planner(lambda p: p.set_sensor(ufm_amd.sensor_disc(40)))
    for p in (a, b, c):
        p.set_survey(SURVEY)
    a.reveal(40, 48)
    a.set_sensor(ufm_amd.sensor_disc(9)); a.reveal(40, 48)
    b.reveal(40, 48)
    same_raster_and_field(a, b, "radius 2, then 9")
    a.set_sensor(ufm_amd.sensor_disc(40)); a.reveal(40, 48)
    c.reveal(40, 48)
    same_raster_and_field(a, c, "then radius 40")
    for p in (a, b, c):
        p.close()


def test_image_staging_grows():
    rng = np.random.default_rng(9)
    small, large = rng.integers(0, 256, (47, 33)).astype(np.uint8), rng.integers(0, 256, (136, 200)).astype(np.uint8)
    a, b = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False), ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    for p in (a, b):
        p.reset(); p.set_occupancy_threshold(1.0); p.set_param("focused", 0)
    a.set_image(small, ksize=5, penalty=15)
    for p in (a, b):
        p.set_image(large, ksize=5, penalty=15)
        p.set_goal(129.0, 194.0)
    assert np.array_equal(a.read_survey(200, 136), b.read_survey(200, 136))
    same_raster_and_field(a, b, "33 x 47, then 200 x 136", 200, 136)
    a.close(); b.close()


def dilate5(raw):
    """grey dilation by the full 5 x 5 footprint, anchor at its centre; beyond the map there is nothing"""
    pad = np.pad(raw, 2)
    out = np.zeros_like(raw)
    for i in range(5):
        for j in range(5):
            out = np.maximum(out, pad[i:i + raw.shape[0], j:j + raw.shape[1]])
    return out


def test_every_feature_across_a_change_of_size():
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
    p.reset(); p.set_occupancy_threshold(1.0)
    p.set_cspace(ONES5); p.track_costs(True); p.set_sensor(ufm_amd.sensor_disc(2)); p.set_layers(2); p.track_changes(True)
    for width, length, seed in [(96, 80, 3), (200, 136, 4), (33, 47, 5)]:
        what = "%d x %d" % (width, length)
        cost = ufm_amd.synth.cost_map(seed, width, length)
        p.set_map(cost)
        p.set_survey(ufm_amd.synth.cost_map(seed + 10, width, length))
        p.set_start(6.0, 5.0); p.set_goal(float(length - 7), float(width - 6))
        patch = np.full((9, 9), 200, np.uint8)
        p.patch_layer(1, patch, length // 2 - 4, width // 2 - 4)
        assert p.reveal(length // 3, width // 3, count=True) > 0, what
        assert p.step() == 0
        layers = [p.read_layer(k, width, length) for k in (0, 1)]
        want1 = np.zeros((length, width), np.uint8)
        want1[length // 2 - 4:length // 2 + 5, width // 2 - 4:width // 2 + 5] = patch
        assert np.array_equal(layers[1], want1), what
        raw = np.maximum(layers[0], layers[1])
        assert np.array_equal(p.read_raw_map(width, length), raw), what
        planning = p.read_map(width, length)
        assert np.array_equal(planning, dilate5(raw)), what
        hist, lo, hi = p.read_cost_census()
        assert np.array_equal(hist, np.bincount(planning.ravel(), minlength=256).astype(np.uint64)), what
        assert (lo, hi) == (int(planning.min()), int(planning.max())), what
        field = p.g()
        mirror = np.full(field.shape, np.inf, np.float32)            # (a new raster: the caller's view starts empty again)
        xy, g, _ = p.read_changes()
        mirror[xy[:, 0], xy[:, 1]] = g
        assert np.array_equal(bits(mirror), bits(field)), what
        assert p.check_layout() == (0, 0), what
    p.close()


def test_create_use_destroy_thirty_times():
    """every feature and profiling on: the event sets of the plan (resident kernel, launch batches), of the block kernel, of the launch
    chain, of the layer kernels, of the delta scan and of k_prepare all get created -- and destroyed with the handle"""
    rng = np.random.default_rng(11)
    image = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    patches = [rng.integers(1, 201, (9, 9)).astype(np.uint8) for _ in range(3)]
    first = None
    for cycle in range(30):
        p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, False)
        p.reset(); p.set_occupancy_threshold(1.0); p.set_param("focused", 0); p.set_profiling(1)
        p.set_cspace(ONES5); p.track_costs(True); p.set_sensor(ufm_amd.sensor_disc(2)); p.set_layers(2); p.track_changes(True)
        p.set_image(image, ksize=5, penalty=15)
        p.set_start(6.0, 5.0); p.set_goal(57.0, 58.0)
        assert p.step() == 0 and p.stats.resident_launches == 1
        p.patch_map(patches[0], 20, 20); p.reveal(40, 40); p.set_start(6.0, 5.0)
        assert p.step() == 0 and p.stats.region_launches == 1, cycle          # through the block kernel
        p.set_param("region", 0)
        p.patch_map(patches[1], 30, 24); p.set_start(6.0, 5.0)
        assert p.step() == 0 and p.stats.region_launches == 0, cycle          # the captured graph
        p.set_param("graph", 0)
        p.patch_map(patches[2], 26, 34); p.set_start(6.0, 5.0)
        assert p.step() == 0                                                  # the launch chain, with its events
        p.read_changes()
        field = bits(p.g())
        p.close()
        if first is None:
            first = field
        assert np.array_equal(field, first), cycle
