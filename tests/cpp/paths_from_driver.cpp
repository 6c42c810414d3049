// A planner process that answers "what would the path be from there" for a list of positions while its own mission goes on:
// LinearInterpolationPathExtractor::extract_paths_from (one call of ufm_extract_paths_from) between two steps, the extractor's own
// path_ / cost_ and the planner's start left alone.  Type-checked by tests/test_paths_from_surface.py for one planner of each
// family: -DPATHS_FROM_PLANNER='DFMPlanner<1>' etc.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"
#include "LinearInterpolationPathExtractor.h"

#ifndef PATHS_FROM_PLANNER
#define PATHS_FROM_PLANNER FieldDPlanner<1>
#endif

int main() {
  typedef PATHS_FROM_PLANNER Planner;
  const int w = 64, h = 48;
  std::shared_ptr<uint8_t> data(new uint8_t[w * h], std::default_delete<uint8_t[]>());
  for (int i = 0; i < w * h; ++i) data.get()[i] = 1 + i % 7;
  Planner planner{};
  LinearInterpolationPathExtractor<typename Planner::Map::ElemType, typename Planner::Base::Info>
      extractor(planner.get_expanded_map(), planner.get_grid());
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_map(data, w, h);
  planner.set_start(Position(4, 4));
  planner.set_goal(Position(h - 4, w - 4));
  if (planner.step() != LOOP_OK) return 3;
  extractor.extract_path();
  const size_t own = extractor.path_.size();

  std::vector<Position> from;
  for (int k = 0; k < 5; ++k) from.emplace_back(6.0f + 3 * k, 8.5f + 2 * k);
  extractor.max_steps = 12;
  const auto answers = extractor.extract_paths_from(from);
  if (extractor.last_error != UFM_OK || answers.size() != from.size()) return 4;
  double sum = 0;
  for (const auto &a : answers) {
    for (const Position &pose : a.path_) sum += pose.x + pose.y;
    for (const float step_cost : a.cost_) sum += step_cost;
    sum += a.total_cost + a.total_dist;
  }
  std::printf("%zu queries, own path %zu points (still %zu), checksum %.9g\n", answers.size(), own, extractor.path_.size(), sum);
  return extractor.path_.size() == own ? 0 : 5;
}
