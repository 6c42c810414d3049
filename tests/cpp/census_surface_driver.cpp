// What the mirror adds for the cost census (ReplannerBase::track_costs / min_cost / cost_census / set_auto_heuristic), used the way a
// driver would: next to the calls of the reference's surface, for a node planner and a cell planner, with and without heuristic keys.
// Type-checked against the mirrored headers (tests/test_census_surface.py, g++ -fsyntax-only), with and without -DNO_HEURISTIC.
#include <cstdint>
#include <memory>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"

template <typename Planner>
static long drive() {
  const int32_t width = 64, height = 64;
  std::shared_ptr<uint8_t> data(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> patch(new uint8_t[4 * 4](), std::default_delete<uint8_t[]>());
  Position start, goal;
  start.x = 2; start.y = 2; goal.x = 60; goal.y = 60;
  Planner planner{};
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_auto_heuristic(true);          // (turns the census on)
  planner.set_heuristic_multiplier(7);       // stored, ignored
  planner.set_map(data, width, height);
  planner.set_start(start);
  planner.set_goal(goal);
  planner.patch_map(patch, 8, 8, 4, 4);
  const int rc = planner.step();
  uint64_t hist[256];
  int lo = 0, hi = 0;
  const int rd = planner.cost_census(hist, &lo, &hi);
  const int mn = planner.min_cost();
  float used = 0;
  const int ru = ufm_heuristic_multiplier(planner.native_handle(), &used);
  planner.set_auto_heuristic(false);
  planner.track_costs(false);
  planner.track_costs();
  return (long)rc + rd + mn + lo + hi + ru + (long)used + (long)hist[0] + planner.last_error;
}

int main() { return (int)(drive<FieldDPlanner<1>>() + drive<ShiftedGridPlanner<2>>() + drive<DFMPlanner<1>>() + drive<FieldDPlanner<0>>()); }
