"""The list of goal tiles a step hands to k_activate_list holds one entry per initialising map whose goal lies inside the map, densely: a
map whose goal lies outside initialises too (its field stays +inf) but contributes no tile, wherever it stands in the batch."""
import functools

import numpy as np
import pytest

import ufm_amd

pytestmark = pytest.mark.gpu

SIZE = 48
GOAL_OUTSIDE = (500.0, 500.0)


def inputs():
    cost = ufm_amd.synth.cost_map(7, SIZE, SIZE)
    start, goal = ufm_amd.synth.start_goal(SIZE, SIZE)
    return cost, start, goal


@functools.lru_cache(maxsize=None)
def single_field(goal_inside):
    """the full field of a single FD level-1 planner, and its layout check"""
    cost, start, goal = inputs()
    p = ufm_amd.Planner(ufm_amd.ALGO_FD, 1)
    p.set_param("focused", 0)
    p.set_occupancy_threshold(1); p.set_map(cost); p.set_start(*start); p.set_goal(*(goal if goal_inside else GOAL_OUTSIDE))
    rc = p.step()
    g, layout = p.g(), p.check_layout()
    p.close()
    g.setflags(write=False)
    return rc, g, layout


def batch_fields(valid):
    """a batch of two maps on the same inputs; valid[i]: map i's goal lies inside the map"""
    cost, start, goal = inputs()
    b = ufm_amd.BatchPlanner(2, ufm_amd.ALGO_FD, 1)
    b.set_param("focused", 0)
    b.set_occupancy_threshold(1)
    for i in range(2):
        b.set_map(i, cost); b.set_start(i, *start); b.set_goal(i, *(goal if valid[i] else GOAL_OUTSIDE))
    assert b.step() == 0
    fields = [b.read_field(i) for i in range(2)]
    assert b.check_layout() == (0, 0)
    b.close()
    return fields


def test_single_planner_with_goal_outside_the_map():
    rc, g, layout = single_field(False)
    assert rc == 0
    assert np.isposinf(g).all()
    assert layout == (0, 0)


def check_batch(valid):
    rc, ref, layout = single_field(True)
    assert rc == 0 and layout == (0, 0) and np.isfinite(ref).any()
    fields = batch_fields(valid)
    for i in range(2):
        if valid[i]:
            assert np.array_equal(fields[i].view(np.uint32), ref.view(np.uint32)), "map %d differs from a single planner's field" % i
        else:
            assert np.isposinf(fields[i]).all(), "map %d: goal outside the map, the field must stay +inf" % i


def test_batch_valid_goal_then_goal_outside():
    check_batch((True, False))


def test_batch_goal_outside_then_valid_goal():
    check_batch((False, True))
