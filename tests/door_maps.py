"""Maps on which a replan is a structural event: three walls with two doors each between the start and the goal, and a scenario that closes
and opens the doors.  Plain numpy (the raster's free cells are ufm_amd.synth.cost_map's, which is numpy too); shared by
tests/test_door_maps.py (CPU: the premises, on the oracle alone) and tests/test_gpu_doors.py (the engine).

THE MAP, comb(seed, size).  synth.cost_map(seed, size, size, obstacles=False) as the free cells; walls of WALL_W = 3 columns of 255 over
all rows at the columns size // 4 (the start's side), size // 2 and 3 * size // 4 (the goal's side); in every wall two doors DOOR_H = 7
rows high that keep the free cells' bytes: door A at rows 16 .. 22, door B at rows size - 24 .. size - 18.  Start (8, 8), goal
(size - 8, size - 8), occupancy threshold 1.0.  x runs along the rows, y along the columns, as everywhere in the project: a wall
separates small y from large y, a path from the start crosses all three.

A DOOR PATCH is the 9 x 5 rectangle at (row - 1, wall - 1): the door, the wall's row above and below it and a column of free cells on
either side.  closed: its three middle columns 255; open: the map's bytes as comb() made them; cheap: the door's 7 x 3 cells 1.  45
cells: a host patch that a single planner holds and its block kernel applies (Route::BlockSingle).

THE SCENARIO, scenario(size): see STEPS.  With both doors of one wall closed nothing on the start's side of it has a path to the goal: the
replan takes every value there away.  Opening one door gives them all back."""
import functools

import numpy as np

import ufm_amd

SEED = 7
THRESHOLD = 1.0
WALL_W, DOOR_H = 3, 7
PATCH_H, PATCH_W = DOOR_H + 2, WALL_W + 2
SIZES = {"FD": 160, "SG": 160, "DFM": 192}        # the smallest maps on which the block kernel has an interior block (6 x 6 / 8 x 8 tiles)
BLOCK = {"FD": 96 * 96, "SG": 96 * 96, "DFM": 128 * 128}      # elements the block holds

START_SIDE, MIDDLE, GOAL_SIDE = 0, 1, 2
DOOR_A, DOOR_B = 0, 1
# (name, wall, door, state, start or None: the start stays where it is)
STEPS = (
    ("1 close B of the goal-side wall", GOAL_SIDE, DOOR_B, "closed", None),
    ("2 close A of the goal-side wall: cut off", GOAL_SIDE, DOOR_A, "closed", None),
    ("3 open B of the goal-side wall", GOAL_SIDE, DOOR_B, "open", None),
    ("4 open A of the goal-side wall", GOAL_SIDE, DOOR_A, "open", None),
    ("5 close A of the start-side wall", START_SIDE, DOOR_A, "closed", (30.0, 8.0)),
    ("6 close B of the start-side wall: start walled off", START_SIDE, DOOR_B, "closed", (30.0, 8.0)),
    ("7 open A of the start-side wall", START_SIDE, DOOR_A, "open", (100.0, 20.0)),
    ("8 cheap B of the goal-side wall", GOAL_SIDE, DOOR_B, "cheap", None),
)
LARGE = (0, 1, 2)          # indices into STEPS of the replans that change more elements than the block holds
CUT_OFF = 1                # ... after which the start's key is +inf
RESTORED = 3               # ... after which the raster is comb()'s again
WALLED_OFF = 5


def walls(size):
    return (size // 4, size // 2, 3 * size // 4)


def door_rows(size):
    return (16, size - 24)


@functools.lru_cache(maxsize=None)
def comb(seed=SEED, size=160):
    """-> (cost raster, read-only; start; goal)"""
    cost = ufm_amd.synth.cost_map(seed, size, size, obstacles=False)
    free = cost.copy()
    for w in walls(size):
        cost[:, w:w + WALL_W] = 255
        for r in door_rows(size):
            cost[r:r + DOOR_H, w:w + WALL_W] = free[r:r + DOOR_H, w:w + WALL_W]
    assert (free < 255).all()
    cost.setflags(write=False)
    start, goal = ufm_amd.synth.start_goal(size, size)
    return cost, start, goal


def door_patch(size, wall, door, state, seed=SEED):
    """-> (patch uint8 [9][5], top, left)"""
    base = comb(seed, size)[0]
    top, left = door_rows(size)[door] - 1, walls(size)[wall] - 1
    patch = base[top:top + PATCH_H, left:left + PATCH_W].copy()
    if state == "closed":
        patch[:, 1:1 + WALL_W] = 255
    elif state == "cheap":
        patch[1:1 + DOOR_H, 1:1 + WALL_W] = 1
    else:
        assert state == "open", state
    return patch, top, left


def scenario(size, seed=SEED):
    """-> [(name, patch, top, left, start)]: STEPS as patches; the start of every step is given, moved or not (a step needs a set_start)"""
    start = comb(seed, size)[1]
    out = []
    for name, wall, door, state, s in STEPS:
        start = s if s is not None else start
        out.append((name,) + door_patch(size, wall, door, state, seed) + (start,))
    return out


def filler(size, seed=SEED):
    """two steps on the middle wall, which the scenario leaves alone -- its door A cheap, then as it was: what a map of a batch does while
    another map's scenario runs ahead of it or behind it"""
    start = comb(seed, size)[1]
    return [("middle A %s" % state,) + door_patch(size, MIDDLE, DOOR_A, state, seed) + (start,) for state in ("cheap", "open")]


def same_bits(a, b):
    """two float32 fields are equal bit for bit"""
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def apply(cur, patch, top, left):
    cur[top:top + patch.shape[0], left:left + patch.shape[1]] = patch


def side_of(size, y):
    """how many walls lie between column y and column 0"""
    return sum(1 for w in walls(size) if y >= w + WALL_W)


def probe_positions(size):
    """positions on both sides of every wall, near both doors and far from them: [n][2]"""
    w = walls(size)
    a, b = door_rows(size)
    ys = [w[0] - 6, w[0] + WALL_W + 5, w[1] - 6, w[1] + WALL_W + 5, w[2] - 6, w[2] + WALL_W + 5]
    return np.array([(float(x), float(y)) for y in ys for x in (a + 3, size // 2, b + 3)], np.float32)
