// Everything a planner process of the reference (Tests/Planners/{FDSTAR,SGDFM,DFM}/main.cpp) touches of the planner surface, in one
// translation unit per planner: the planner class with its OPT_LVL, the path extractor built on the planner's map and grid, the
// configuration calls, a patch and a step, the extractor's outputs and timers, the planners' public timers, the `tof` dump over the
// map's buckets with the element type of that planner, and the distance check on the next way point.  Type-checked against the
// mirrored headers (tests/test_cpp_surface.py, g++ -fsyntax-only) with and without -DNO_HEURISTIC.
//
// -DSURFACE_FDSTAR / -DSURFACE_SGDFM / -DSURFACE_DFM selects the planner.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <tuple>

#if defined(SURFACE_FDSTAR)
#include "FieldDPlanner.h"
#define SURFACE_LVL 1
typedef FieldDPlanner<SURFACE_LVL> Planner;
typedef Node DumpElem;
static const bool kIndirect = true;
#elif defined(SURFACE_SGDFM)
#include "ShiftedGridPlanner.h"
#define SURFACE_LVL 2
typedef ShiftedGridPlanner<SURFACE_LVL> Planner;
typedef Node DumpElem;
static const bool kIndirect = false;
#elif defined(SURFACE_DFM)
#include "DynamicFastMarching.h"
#define SURFACE_LVL 1
typedef DFMPlanner<SURFACE_LVL> Planner;
typedef Cell DumpElem;
static const bool kIndirect = true;
#else
#error "define SURFACE_FDSTAR, SURFACE_SGDFM or SURFACE_DFM"
#endif
#include "Graph.h"
#include "LinearInterpolationPathExtractor.h"

int main() {
  const int32_t width = 64, height = 64, top = 8, left = 8, hint = 1;
  std::shared_ptr<uint8_t> data(new uint8_t[width * height], std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> patch(new uint8_t[4 * 4], std::default_delete<uint8_t[]>());
  Position next_point, prev_point, goal;
  next_point.x = 2; next_point.y = 2; goal.x = 60; goal.y = 60;

  Planner planner{};
  LinearInterpolationPathExtractor<typename Planner::Map::ElemType, typename Planner::Base::Info>
      extractor(planner.get_expanded_map(), planner.get_grid());
  extractor.allow_indirect_traversals = kIndirect;
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_heuristic_multiplier(hint);
  planner.set_map(data, width, height);
  planner.set_start(next_point);
  planner.set_goal(goal);

  planner.patch_map(patch, top, left, 4, 4);
  planner.set_heuristic_multiplier(hint);
  planner.step();
  extractor.extract_path();
  float out[6] = {(float)extractor.path_.size(), extractor.total_dist, extractor.total_cost, planner.u_time, planner.p_time, extractor.e_time};
  for (const auto &pose : extractor.path_) out[0] += pose.x + pose.y;
  for (const auto &step_cost : extractor.cost_) out[1] += step_cost;

  long long expanded_size = (long long)planner.map.size();
  for (auto b : planner.map.buckets)
    for (auto &expanded : b) {
      const DumpElem &exp = expanded.first;
      float g = std::get<0>(expanded.second);
      float rhs = std::get<1>(expanded.second);
      out[2] += exp.x + exp.y + g + rhs;
    }

  prev_point = next_point;
  for (unsigned int i = 1; i < extractor.path_.size(); i++) {
    next_point = {extractor.path_[i].x, extractor.path_[i].y};
    out[3] += extractor.cost_[i - 1];
    if (Cell(next_point).distance(Cell(prev_point)) > 5) break;
  }
  planner.set_start(next_point);
  std::printf("%lld %g %g %g %g %g %g\n", expanded_size, out[0], out[1], out[2], out[3], out[4], out[5]);
  return 0;
}
