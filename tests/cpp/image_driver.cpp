// What the mirror adds for map preparation (ReplannerBase::set_image), used the way a driver would: in place of set_map, next to the calls
// of the reference's surface, for a node planner and a cell planner, with and without heuristic keys.
// Type-checked against the mirrored headers (tests/test_prepare_surface.py, g++ -fsyntax-only), with and without -DNO_HEURISTIC.
#include <cstdint>
#include <memory>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"

template <typename Planner>
static long drive() {
  const int32_t width = 64, height = 48;
  std::shared_ptr<uint8_t> bitmap(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  uint16_t taps[31];
  const int t = ufm_gaussian_taps(13, taps);
  Position start, goal;
  start.x = 2; start.y = 2; goal.x = 40; goal.y = 60;
  Planner planner{};
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_image(bitmap, width, height, taps, 13, 15);     // the map and its survey: no set_map, no set_survey
  const uint8_t one[1] = {1};
  planner.set_sensor(one, 1, 1);
  planner.set_start(start);
  planner.set_goal(goal);
  const int r0 = planner.reveal(2, 2);
  const int rc = planner.step();
  const uint16_t none[1] = {256};
  const int r1 = ufm_set_image(planner.native_handle(), bitmap.get(), width, height, none, 1, 0);
  const int r2 = ufm_set_image_device(planner.native_handle(), nullptr, width, height, none, 1, 0);
  return (long)t + r0 + rc + r1 + r2 + planner.last_error;
}

int main() { return (int)(drive<FieldDPlanner<1>>() + drive<ShiftedGridPlanner<2>>() + drive<DFMPlanner<1>>() + drive<FieldDPlanner<0>>()); }
