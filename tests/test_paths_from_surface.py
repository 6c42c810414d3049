"""Position queries without a GPU: both entry points reject a NULL handle before they write anything (the symbols exist), and a
driver that asks the mirror's extractor for paths from a list of positions type-checks for one planner of each family."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ufm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")
CANARY = np.float32(-7777.0)


def test_null_handle_is_invalid_and_writes_nothing():
    lib = ufm_amd.load_library()
    starts = np.array([[1.0, 2.0], [3.0, 4.5]], np.float32)
    maps = np.zeros(2, np.int32)
    pts = np.full((2, 7, 2), CANARY, np.float32)
    costs = np.full((2, 4), CANARY, np.float32)
    info = (ufm_amd.capi.PathInfo * 2)()
    for k in range(2):
        info[k].n_points = info[k].steps = -5
    assert lib.ufm_extract_paths_from(None, 2, starts.ctypes.data, 2, 1, 1, pts.ctypes.data, 7, costs.ctypes.data, 4,
                                      ctypes.addressof(info)) == -22
    assert lib.ufm_batch_extract_paths_from(None, 2, maps.ctypes.data, starts.ctypes.data, 2, 1, 1, pts.ctypes.data, 7,
                                            costs.ctypes.data, 4, ctypes.addressof(info)) == -22
    assert (pts == CANARY).all() and (costs == CANARY).all()
    assert all(info[k].n_points == -5 and info[k].steps == -5 for k in range(2))


@pytest.mark.parametrize("planner", ["DFMPlanner<1>", "FieldDPlanner<0>", "ShiftedGridPlanner<2>"])
@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]])
def test_query_driver_type_checks(planner, define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DPATHS_FROM_PLANNER=" + planner] + define +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "include"),
                           os.path.join(ROOT, "tests", "cpp", "paths_from_driver.cpp")])
