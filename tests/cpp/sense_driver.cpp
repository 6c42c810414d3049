// What the mirror adds for the sensor reveal (ReplannerBase::set_sensor / set_survey / reveal), used the way a driver would: next to the
// calls of the reference's surface, for a node planner and a cell planner, with and without heuristic keys.
// Type-checked against the mirrored headers (tests/test_sensor_surface.py, g++ -fsyntax-only), with and without -DNO_HEURISTIC.
#include <cstdint>
#include <memory>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"

template <typename Planner>
static long drive() {
  const int32_t width = 64, height = 64;
  std::shared_ptr<uint8_t> data(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> survey(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  const uint8_t wedge[3 * 5] = {1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0};
  Position start, goal;
  start.x = 2; start.y = 2; goal.x = 60; goal.y = 60;
  Planner planner{};
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_sensor(wedge, 5, 3, 2, 0);     // the field of view may come before the map
  planner.set_map(data, width, height);
  planner.set_survey(survey, width, height);
  planner.set_start(start);
  planner.set_goal(goal);
  uint64_t changed = 0;
  const int r0 = planner.reveal(2, 2);                 // queued
  const int r1 = planner.reveal(3, 2, &changed);       // waited for, counted
  const int rc = planner.step();
  planner.set_sensor(wedge, 5, 3);                     // replaced between two calls, anchor at the centre
  const int r2 = ufm_reveal(planner.native_handle(), 4, 4, nullptr);
  uint8_t back[64 * 64];
  const int r3 = ufm_read_survey(planner.native_handle(), back);
  return (long)r0 + r1 + rc + r2 + r3 + (long)changed + back[0] + planner.last_error;
}

int main() { return (int)(drive<FieldDPlanner<1>>() + drive<ShiftedGridPlanner<2>>() + drive<DFMPlanner<1>>() + drive<FieldDPlanner<0>>()); }
