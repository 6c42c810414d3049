// A local planner next to the global one: it scores a fan of candidate arcs on the raster the planner plans on --
// LinearInterpolationPathExtractor::score_paths (one call of ufm_score_paths) between two steps -- and keeps the cheapest free one; the
// extractor's own path_ / cost_ and the planner's start are left alone.  Type-checked by tests/test_score_surface.py for one planner of
// each family: -DSCORE_PLANNER='DFMPlanner<1>' etc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"
#include "LinearInterpolationPathExtractor.h"

#ifndef SCORE_PLANNER
#define SCORE_PLANNER FieldDPlanner<1>
#endif

int main() {
  typedef SCORE_PLANNER Planner;
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

  std::vector<std::vector<Position>> arcs;
  for (int k = -3; k <= 3; ++k) {          // seven arcs of twelve points from the start, curving left to right
    std::vector<Position> arc;
    float x = 4, y = 4, heading = 0.8f;
    for (int i = 0; i < 12; ++i) {
      arc.emplace_back(x, y);
      heading += 0.05f * k;
      x += std::cos(heading);
      y += std::sin(heading);
    }
    arcs.push_back(arc);
  }
  const std::vector<ufm_score> scores = extractor.score_paths(arcs);
  if (extractor.last_error != UFM_OK || scores.size() != arcs.size()) return 4;
  int best = -1;
  for (size_t k = 0; k < scores.size(); ++k)
    if (scores[k].blocked_segment < 0 && (best < 0 || scores[k].cost < scores[best].cost)) best = static_cast<int>(k);
  std::printf("%zu arcs, best %d (cost %.9g over %.9g cells, %d pieces), own path %zu points (still %zu)\n", scores.size(), best,
              best < 0 ? 0.0 : scores[best].cost, best < 0 ? 0.0 : scores[best].dist, best < 0 ? 0 : scores[best].pieces, own,
              extractor.path_.size());
  return extractor.path_.size() == own ? 0 : 5;
}
