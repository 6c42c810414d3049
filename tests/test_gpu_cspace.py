"""-m gpu: C-space inflation in the engine (ufm_set_cspace).  A planner with a footprint is fed RAW rasters and patches and must
(1) keep `planning raster == dilate(raw raster)` bit for bit, (2) plan exactly as a planner -- here the CPU oracle -- that is fed the
consistently inflated data: dilate(raw) first, then per patch the grown rectangle cut from dilate(raw as it stands).
The dilation reference is test_cspace_surface.dilate_ref, a shift-and-max written from the definition in include/ufm.h."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import ufm_amd
from helpers import ALGOS, DeviceBytes, check_parity
from test_cspace_surface import dilate_ref
from test_gpu_changes import Mirror
from test_gpu_path import INDIRECT, close_path, close_path_while_final, same_path

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
ELLIPSE5 = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], np.uint8)   # cv2 MORPH_ELLIPSE (5, 5)
BLOCK4 = np.ones((4, 4), np.uint8)
ELL = np.array([[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.uint8)
MASKS = {"cross3": (CROSS, None), "ellipse5": (ELLIPSE5, None), "block4": (BLOCK4, (2, 2)), "ell3x5": (ELL, (2, 0))}


def grown(mask, anchor, top, left, h, w, L, W):
    """the grown rectangle (include/ufm.h): rows [top - (mh-1-ar), top+h-1 + ar], columns alike, clipped -> (top', left', h', w')"""
    mh, mw = mask.shape
    ar, ac = (mh // 2, mw // 2) if anchor is None else anchor
    x0, y0 = max(top - (mh - 1 - ar), 0), max(left - (mw - 1 - ac), 0)
    x1, y1 = min(top + h - 1 + ar, L - 1), min(left + w - 1 + ac, W - 1)
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


class Inflated:
    """a host copy of the raw raster, and the oracle's feed derived from it"""

    def __init__(self, raw, mask, anchor):
        self.raw, self.mask, self.anchor = raw.copy(), mask, anchor

    def planning(self):
        return dilate_ref(self.raw, self.mask, self.anchor)

    def patch(self, patch, top, left):
        """apply a raw patch; returns (grown patch of the planning raster, top', left')"""
        h, w = patch.shape
        self.raw[top:top + h, left:left + w] = patch
        x0, y0, gh, gw = grown(self.mask, self.anchor, top, left, h, w, *self.raw.shape)
        return np.ascontiguousarray(self.planning()[x0:x0 + gh, y0:y0 + gw]), x0, y0


def make_planner(algo, lvl, heur, raw, start, goal, mask=None, anchor=None):
    g = ufm_amd.Planner(algo, lvl, heur)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_heuristic_multiplier(1.0)
    if mask is not None:
        g.set_cspace(mask, anchor)
    g.set_map(raw); g.set_start(*start); g.set_goal(*goal)
    return g


def make_oracle(algo, lvl, heur, planning, start, goal):
    o = orc.OraclePlanner(algo, lvl, heur)
    o.reset(); o.set_occupancy_threshold(1.0); o.set_heuristic_multiplier(1.0)
    o.set_map(planning); o.set_start(*start); o.set_goal(*goal)
    return o


def raster_invariant(g, inf, what):
    L, W = inf.raw.shape
    raw = g.read_raw_map(W, L)
    assert np.array_equal(raw, inf.raw), "%s: the raw store differs from the host's raw copy in %d cells" % (what, int((raw != inf.raw).sum()))
    got, want = g.read_map(W, L), dilate_ref(raw, inf.mask, inf.anchor)
    assert np.array_equal(got, want), "%s: planning raster != dilate(raw) in %d cells, first %r" % (
        what, int((got != want).sum()), tuple(np.argwhere(got != want)[0]))


def random_patch(rng, L, W, hmax=20, wmax=20):
    h, w = int(rng.integers(1, hmax + 1)), int(rng.integers(1, wmax + 1))
    return int(rng.integers(0, L - h + 1)), int(rng.integers(0, W - w + 1)), rng.integers(1, 255, (h, w)).astype(np.uint8)


def invariant_mission(mask, anchor, L, W, extra=()):
    """set_map, then raw patches -- random ones, overlapping ones, one on every border and at a corner, several between two steps, one
    that lowers a cell under neighbours that keep the max -- with the raster invariant after every patch and the layout check after every step"""
    rng = np.random.default_rng(L * 1000 + W + mask.size)
    raw0 = ufm_amd.synth.cost_map(21, W, L)
    start, goal = ufm_amd.synth.start_goal(W, L)
    inf = Inflated(raw0, mask, anchor)
    g = make_planner(ufm_amd.ALGO_FD, 1, False, raw0, start, goal, mask, anchor)
    raster_invariant(g, inf, "set_map")
    assert g.step() == 0 and g.check_layout() == (0, 0)
    groups = [[random_patch(rng, L, W)] for _ in range(4)]
    t, l, p = random_patch(rng, L, W)
    groups.append([(t, l, p), (min(t + 2, L - p.shape[0]), min(l + 3, W - p.shape[1]), (255 - p).clip(1, 254).astype(np.uint8))])   # overlapping, one step
    groups.append([(0, 7, rng.integers(1, 255, (3, 9)).astype(np.uint8)),                    # top border
                   (L - 4, 11, rng.integers(1, 255, (4, 6)).astype(np.uint8)),               # bottom border
                   (17, 0, rng.integers(1, 255, (7, 2)).astype(np.uint8))])                  # left border: three between two steps
    groups.append([(9, W - 5, rng.integers(1, 255, (11, 5)).astype(np.uint8))])              # right border
    groups.append([(L - 1, W - 1, np.array([[254]], np.uint8))])                             # a corner, 1 x 1
    groups.append([(0, 0, rng.integers(1, 255, (20, 20)).astype(np.uint8))])                 # the other corner, the largest
    groups.append([(20, 16, np.full((7, 7), 254, np.uint8))])                                # a plateau ...
    groups += [[q] for q in extra]
    k = 0
    for n, group in enumerate(groups):
        for top, left, patch in group:
            g.patch_map(patch, top, left)
            inf.patch(patch, top, left)
            raster_invariant(g, inf, "patch %d at (%d, %d) %r" % (k, top, left, patch.shape))
            k += 1
        s = (start[0] + 2 * (n % 5), start[1] + (n % 4))
        g.set_start(*s)
        assert g.step() == 0
        assert g.check_layout() == (0, 0), "after step %d: %r" % (n, g.check_layout())
    # ... whose centre is lowered: every window that holds it holds a neighbour on the plateau, the planning raster keeps its value
    before = inf.planning()
    g.patch_map(np.array([[1]], np.uint8), 23, 19)
    inf.patch(np.array([[1]], np.uint8), 23, 19)
    assert np.array_equal(inf.planning(), before)
    raster_invariant(g, inf, "lowered under a neighbour")
    g.set_start(start[0] + 1, start[1] + 1)
    assert g.step() == 0
    assert g.stats.updated == 0, "a raw change that leaves the planning raster alone seeded %d elements" % g.stats.updated
    assert g.check_layout() == (0, 0)
    assert k + 1 >= 12
    g.close()


@pytest.mark.parametrize("name", list(MASKS))
def test_raster_invariant(name):
    """48 x 40: no multiple of the dilation tile (16 x 64) nor of the engine's, and not square"""
    mask, anchor = MASKS[name]
    invariant_mission(mask, anchor, 48, 40)


def test_raster_invariant_31_disc():
    """a 31 x 31 disc on 96 x 80: the apron is wider than a tile, every patch grows by 30 cells, and the 36 x 36 one grows to 66 x 66 --
    above the block kernel's 65 x 65 elements and the one-workgroup patch kernel's 4096 cells: the ordinary large-patch route"""
    rng = np.random.default_rng(31)
    invariant_mission(ufm_amd.cspace_disc(31), None, 96, 80, extra=[(30, 22, rng.integers(1, 255, (36, 36)).astype(np.uint8))])


def test_raster_invariant_odd_width_byte_loads():
    """a width that is no multiple of 4: the staging takes its byte path, the stores are mostly unaligned"""
    invariant_mission(ELLIPSE5, None, 50, 41)


PLANNERS = {"FD-1h": ("FD", 1, True), "SG-2": ("SG", 2, False), "DFM-1": ("DFM", 1, False)}
# FD-1h three ways: host patches (held patches are declined: they go through the staging copy), device-pointer patches and rasters,
# and the launch chain instead of the block kernel ("region" = 0) -- each against the same oracle, so all three give the same fields
VARIANTS = [("FD-1h", "host"), ("FD-1h", "device"), ("FD-1h", "chain"), ("SG-2", "host"), ("DFM-1", "host")]


def script64(seed, n=8, size=11):
    return list(ufm_amd.synth.replan_script(seed, 64, 64, n_patches=n, size=size, stride=5))


@pytest.mark.parametrize("name,variant", VARIANTS, ids=["%s-%s" % v for v in VARIANTS])
def test_planner_equivalence(name, variant):
    """a planner with the 5 x 5 ellipse fed raw data == the oracle fed the inflated data: 8 replans with a moving start on 64 x 64; the
    field under helpers.check_parity's rule (FD / SG bit for bit below the start's key, MS-DFM within DFM_RTOL), ufm_stats.updated, the
    raster invariant, and the extracted path as test_gpu_path.py compares it"""
    algo, lvl, heur = PLANNERS[name]
    raw0 = ufm_amd.synth.cost_map(33, 64, 64)
    start, goal = ufm_amd.synth.start_goal(64, 64)
    inf = Inflated(raw0, ELLIPSE5, None)
    bufs = []
    g = ufm_amd.Planner(ALGOS[algo], lvl, heur)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_heuristic_multiplier(1.0)
    if variant == "chain":
        g.set_param("region", 0)
    g.set_cspace(ELLIPSE5)
    if variant == "device":
        bufs.append(DeviceBytes(raw0))
        g.set_map_device(bufs[-1].data_ptr(), 64, 64)
    else:
        g.set_map(raw0)
    g.set_start(*start); g.set_goal(*goal)
    o = make_oracle(ALGOS[algo], lvl, heur, inf.planning(), start, goal)
    assert o.step() == 0 and g.step() == 0
    n, nbad = check_parity(o, g, name + " plan", below_start_key=True)
    assert algo == "DFM" or nbad == 0
    raster_invariant(g, inf, name + " plan")
    regions0 = g.stats.region_replans
    for k, s, top, left, patch in script64(33):
        if variant == "device":
            bufs.append(DeviceBytes(patch))
            g.patch_map_device(bufs[-1].data_ptr(), top, left, patch.shape[1], patch.shape[0])
        else:
            g.patch_map(patch, top, left)
        o.patch_map(*inf.patch(patch, top, left))
        for p in (o, g):
            p.set_start(*s)
        assert o.step() == 0 and g.step() == 0
        what = "%s %s replan %d" % (name, variant, k)
        n, nbad = check_parity(o, g, what, below_start_key=True)
        assert algo == "DFM" or nbad == 0, what
        assert g.stats.updated == o.num_updated, (what, g.stats.updated, o.num_updated)
        raster_invariant(g, inf, what)
        kw = dict(max_steps=20, lookahead=True, allow_indirect=INDIRECT[algo])
        dev = g.extract_path(**kw)
        same_path(dev, orc.extract_path_field(g.read_field()[1], algo == "DFM", inf.planning(), 255, s, goal, **kw), what + " [device field]")
        ref = o.extract_path(**kw)
        if algo == "DFM":
            close_path_while_final(dev, ref, o, what)
        else:
            close_path(dev, ref, what)
    if variant == "chain":
        assert g.stats.region_replans == regions0
    elif algo == "FD":
        assert g.stats.region_replans > regions0, "engine-inflated small patches no longer reach the block kernel"
    g.close()
    for d in bufs:
        d.free()


def converged_run(variant):
    """the FD-1h mission of test_planner_equivalence with "focused" = 0 -- every element final after every step, so the whole field is
    comparable, not only the part below the start's key; returns per step (field, planning raster, raw raster)"""
    raw0 = ufm_amd.synth.cost_map(33, 64, 64)
    start, goal = ufm_amd.synth.start_goal(64, 64)
    bufs = []
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1, True)
    g.reset(); g.set_occupancy_threshold(1.0); g.set_heuristic_multiplier(1.0)
    g.set_param("focused", 0)
    if variant == "chain":
        g.set_param("region", 0)
    g.set_cspace(ELLIPSE5)
    if variant == "device":
        bufs.append(DeviceBytes(raw0))
        g.set_map_device(bufs[-1].data_ptr(), 64, 64)
    else:
        g.set_map(raw0)
    g.set_start(*start); g.set_goal(*goal)
    assert g.step() == 0
    out = [(g.read_field()[0], g.read_map(64, 64), g.read_raw_map(64, 64))]
    for k, s, top, left, patch in script64(33):
        if variant == "device":
            bufs.append(DeviceBytes(patch))
            g.patch_map_device(bufs[-1].data_ptr(), top, left, patch.shape[1], patch.shape[0])
        else:
            g.patch_map(patch, top, left)
        g.set_start(*s)
        assert g.step() == 0
        out.append((g.read_field()[0], g.read_map(64, 64), g.read_raw_map(64, 64)))
    regions = g.stats.region_replans
    g.close()
    for d in bufs:
        d.free()
    return out, regions


def test_fd_variants_agree_bit_for_bit():
    """host patches, device-pointer patches and the launch chain ("region" = 0), compared with each other directly: the same whole field,
    planning raster and raw raster after the plan and after every replan"""
    host, regions = converged_run("host")
    assert regions > 0
    for variant in ("device", "chain"):
        other, regions = converged_run(variant)
        assert (regions == 0) == (variant == "chain")
        for k, (a, b) in enumerate(zip(host, other)):
            assert np.isfinite(a[0]).sum() > 3000
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "host against %s: fields differ after step %d in %d elements" % (
                variant, k, int((a[0].view(np.uint32) != b[0].view(np.uint32)).sum()))
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "host against %s: rasters differ after step %d" % (variant, k)


def run_fd(mask, n=8):
    """the FD mission above without heuristic keys, fed as it is (a planner without a footprint plans on what it is given); returns
    (the values of the oracle's trusted set per step, rasters per step, the planner's last statistics)"""
    raw0 = ufm_amd.synth.cost_map(33, 64, 64)
    start, goal = ufm_amd.synth.start_goal(64, 64)
    g = make_planner(ufm_amd.ALGO_FD, 1, False, raw0, start, goal, mask)
    o = make_oracle(ufm_amd.ALGO_FD, 1, False, raw0, start, goal)
    assert o.step() == 0 and g.step() == 0
    fields, rasters = [g.read_field()[0][o.trusted_mask(below_start_key=True)]], [g.read_map(64, 64)]
    for k, s, top, left, patch in script64(33, n):
        for p in (o, g):
            p.patch_map(patch, top, left); p.set_start(*s)
        assert o.step() == 0 and g.step() == 0
        fields.append(g.read_field()[0][o.trusted_mask(below_start_key=True)]); rasters.append(g.read_map(64, 64))
    stats = g.stats.as_dict()
    g.close()
    return fields, rasters, stats


def test_one_by_one_mask_is_off_and_set_cspace_comes_first():
    none = run_fd(None)
    one = run_fd(np.ones((1, 1), np.uint8))
    for k, (fa, fb) in enumerate(zip(none[0], one[0])):
        assert len(fa) > 100 and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), "no footprint against the 1 x 1 mask: fields differ after step %d" % k
    for k, (ra, rb) in enumerate(zip(none[1], one[1])):
        assert np.array_equal(ra, rb), "no footprint against the 1 x 1 mask: rasters differ after step %d" % k
    assert none[2]["region_replans"] == one[2]["region_replans"] > 0      # the same route: held host patches, the block kernel
    raw0 = ufm_amd.synth.cost_map(33, 64, 64)
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    g.set_cspace(np.ones((1, 1), np.uint8))
    buf = np.zeros((64, 64), np.uint8)
    assert g.L.ufm_read_raw_map(g.h, buf.ctypes.data) == -22          # no map, and off
    g.set_map(raw0)
    assert g.L.ufm_read_raw_map(g.h, buf.ctypes.data) == -22          # off: there is no raw store
    assert g.L.ufm_set_cspace(g.h, CROSS.ctypes.data, 3, 3, -1, -1) == -22      # after ufm_set_map
    assert np.array_equal(g.read_map(64, 64), raw0)
    g.close()
    g = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    bad = np.zeros((3, 3), np.uint8)
    assert g.L.ufm_set_cspace(g.h, bad.ctypes.data, 3, 3, -1, -1) == -22        # anchor cell clear
    assert g.L.ufm_set_cspace(g.h, CROSS.ctypes.data, 3, 3, 3, 0) == -22        # anchor outside
    assert g.L.ufm_set_cspace(g.h, CROSS.ctypes.data, 32, 1, 0, 0) == -22
    assert g.L.ufm_set_cspace(g.h, None, 3, 3, -1, -1) == -22
    g.set_cspace(CROSS)                                                          # a rejected call leaves the handle usable
    g.set_map(raw0)
    assert np.array_equal(g.read_map(64, 64), dilate_ref(raw0, CROSS)) and np.array_equal(g.read_raw_map(64, 64), raw0)
    g.close()


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_engine", "sharded"])
def test_batch(devices):
    """3 maps with "defer_patches" on and a footprint: a different raw device-pointer patch per map per round (read at the call: each buffer
    is overwritten as soon as the device has run what the call queued), 4 rounds; the raster invariant and parity with its own oracle per map"""
    n, L, W = 3, 64, 64
    b = ufm_amd.BatchPlanner(n, ufm_amd.ALGO_FD, 1, False, devices=devices)
    b.set_occupancy_threshold(1.0)
    b.set_param("defer_patches", 1)
    b.set_cspace(ELLIPSE5)
    start, goal = ufm_amd.synth.start_goal(W, L)
    infs, oracles = [], []
    for m in range(n):
        raw0 = ufm_amd.synth.cost_map(40 + m, W, L)
        infs.append(Inflated(raw0, ELLIPSE5, None))
        b.set_map(m, raw0); b.set_start(m, *start); b.set_goal(m, *goal)
        o = make_oracle(ufm_amd.ALGO_FD, 1, False, infs[m].planning(), start, goal)
        assert o.step() == 0
        oracles.append(o)
    assert b.step() == 0

    def against(what):
        for m, o in enumerate(oracles):
            raw = b.read_raw_map(m, W, L)
            assert np.array_equal(raw, infs[m].raw), "%s: raw store of map %d" % (what, m)
            assert np.array_equal(b.read_map(m, W, L), dilate_ref(raw, ELLIPSE5)), "%s: planning raster of map %d != dilate(raw)" % (what, m)
            mask = o.trusted_mask(below_start_key=True)
            assert int(mask.sum()) > 100
            assert np.array_equal(b.read_field(m)[mask], o.g()[mask]), "%s: map %d differs from its oracle" % (what, m)
        assert b.check_layout() == (0, 0)
        assert b.check_info()[1:4] == (0, 0, 0), b.check_info()
    against("plan")
    bufs = [DeviceBytes(np.zeros((13, 13), np.uint8)) for _ in range(n)]
    for k in range(1, 5):
        s = (start[0] + 5 * k, start[1] + 4 * k)
        for m, o in enumerate(oracles):
            h, w = 7 + 2 * m, 13 - 3 * m + (k % 2)
            top, left = int(s[0]) - 4 + m, int(s[1]) - 3 - m
            patch = (1 + (ufm_amd.synth.h64((40 + m) ^ k, *np.meshgrid(np.arange(top, top + h), np.arange(left, left + w), indexing="ij")) % np.uint64(200))).astype(np.uint8)
            bufs[m].overwrite(patch)
            b.patch_map_device(m, bufs[m].data_ptr(), top, left, w, h); b.set_start(m, *s)
            bufs[m].overwrite(np.zeros_like(patch))            # (a deferred patch would now apply zeros)
            o.patch_map(*infs[m].patch(patch, top, left)); o.set_start(*s)
            assert o.step() == 0
        assert b.step() == 0
        against("round %d" % k)
    b.close()
    for d in bufs:
        d.free()


def test_step_deltas_follow_the_planning_raster():
    """ufm_track_changes with a footprint: a host mirror built from ufm_read_changes alone equals the field after the plan and each replan"""
    raw0 = ufm_amd.synth.cost_map(33, 64, 64)
    start, goal = ufm_amd.synth.start_goal(64, 64)
    g = make_planner(ufm_amd.ALGO_FD, 1, False, raw0, start, goal, ELLIPSE5)
    g.track_changes(True)
    m = Mirror(g.dims(), True)
    assert g.step() == 0
    m.apply(*g.read_changes(want_info=True), what="plan")
    m.check(g, "plan")
    for k, s, top, left, patch in script64(33):
        g.patch_map(patch, top, left); g.set_start(*s)
        assert g.step() == 0
        xy, gv, info = g.read_changes(want_info=True)
        changed = m.apply(xy, gv, info, "replan %d" % k)
        m.check(g, "replan %d" % k)
        assert changed == int(g.stats.expanded), (k, changed, int(g.stats.expanded))
    g.close()


def test_planner_process_inflates(tmp_path, ref_bitmaps):
    """ufm_planner --inflate 5 fed raw data by harness.run_mission(planner_inflates=True), on the noise-trap bitmap cropped to 64 x 64:
    reaches the goal, and at every step its path is the one of the oracle fed the consistently inflated map, within the bound of
    tests/test_harness_mission.py (test_gpu_path.close_path)"""
    cost, _ = ref_bitmaps["noise-trap"]
    img = np.ascontiguousarray((~cost).astype(np.uint8)[28:92, 28:92])
    (sx, sy), (gx, gy) = (56.0, 56.0), (14.0, 14.0)       # (the CPU oracle alone walks this mission in 12 moves)
    exe = os.path.join(PKG, "ufm_planner_no_heur")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", PKG, "apps"])
    disc = ufm_amd.cspace_disc(5)
    o = orc.OraclePlanner(orc.ALGO_FD, 1, False)
    state = {"moves": 0, "inf": None}

    def on_map(raw, min_cost):
        state["inf"] = Inflated(raw, disc, None)
        planning = state["inf"].planning()
        assert np.array_equal(planning, ufm_amd.harness.dilate(raw, 5)) and min_cost == int(planning.min())
        o.reset(); o.set_occupancy_threshold(1); o.set_heuristic_multiplier(min_cost)
        o.set_map(planning); o.set_start(sx, sy); o.set_goal(gx, gy)

    def on_move(i, pos, top, left, patch, min_cost, reply):
        path, costs, dist, total, times = reply
        o.patch_map(*state["inf"].patch(patch, top, left))
        o.set_heuristic_multiplier(min_cost); o.set_start(*pos)
        assert o.step() == 0
        ref = o.extract_path(max_steps=20, allow_indirect=True)
        close_path((path, costs, total, dist), ref, "mission move %d at %r" % (i, pos))
        state["moves"] += 1

    trace, finished = ufm_amd.harness.run_mission(
        [exe, "--planner", "FD", "--level", "1", "--inflate", "5"], str(tmp_path / "pipe_1"), str(tmp_path / "pipe_2"),
        img, (sx, sy), (gx, gy), radius=5, cspace_diameter=5, on_map=on_map, on_move=on_move, max_moves=100, planner_inflates=True)
    assert trace[0] == (sx, sy) and state["moves"] == len(trace)
    assert finished, "the planner did not report the goal after %d moves, last position %r" % (len(trace), trace[-1])
