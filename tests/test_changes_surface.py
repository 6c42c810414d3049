"""Step deltas without a GPU: the C ABI rejects a NULL handle (the symbols exist), and a driver that follows the deltas through the
mirror -- map.follow_changes(true), then size(), then the iteration over map.buckets -- type-checks for one planner of each family."""
import ctypes
import os
import subprocess

import pytest

import ufm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unige-tasi-path-planners_amd")


def test_null_handle_is_invalid():
    lib = ufm_amd.load_library()
    total = ctypes.c_int(-1)
    assert lib.ufm_track_changes(None, 1) == -22
    assert lib.ufm_read_changes(None, 0, None, None, None, ctypes.addressof(total)) == -22
    assert lib.ufm_batch_track_changes(None, 1) == -22
    assert lib.ufm_batch_read_changes(None, 0, 0, None, None, None, ctypes.addressof(total)) == -22
    assert total.value == -1


@pytest.mark.parametrize("planner", ["DFMPlanner<1>", "FieldDPlanner<0>", "ShiftedGridPlanner<2>"])
@pytest.mark.parametrize("define", [[], ["-DNO_HEURISTIC"]])
def test_following_driver_type_checks(planner, define):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFOLLOW_PLANNER=" + planner] + define +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "include"),
                           os.path.join(ROOT, "tests", "cpp", "follow_driver.cpp")])
