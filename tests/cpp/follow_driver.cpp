// A driver that follows the steps' deltas on the host (ExpandedMap::follow_changes) -- the `tof` dump of the reference's planner
// processes (Tests/Planners/*/main.cpp:139-156) without a read of the whole field per step.  Type-checked by
// tests/test_changes_surface.py for one planner of each family: -DFOLLOW_PLANNER='DFMPlanner<1>' etc.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <tuple>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"

#ifndef FOLLOW_PLANNER
#define FOLLOW_PLANNER DFMPlanner<1>
#endif

int main() {
  typedef FOLLOW_PLANNER Planner;
  typedef typename Planner::Map::ElemType Elem;
  const int w = 64, h = 48;
  std::shared_ptr<uint8_t> data(new uint8_t[w * h], std::default_delete<uint8_t[]>());
  for (int i = 0; i < w * h; ++i) data.get()[i] = 1 + i % 7;
  Planner planner{};
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_map(data, w, h);
  if (planner.map.follow_changes(true) != UFM_OK) return 2;
  planner.set_start(Position(4, 4));
  planner.set_goal(Position(h - 4, w - 4));
  if (planner.step() != LOOP_OK) return 3;
  const size_t n = planner.map.size();
  size_t iterated = 0;
  double sum = 0;
  for (const auto &bucket : planner.map.buckets)
    for (const auto &kv : bucket) {
      const Elem &el = kv.first;
      sum += std::get<0>(kv.second) + std::get<1>(kv.second) + 0 * (el.x + el.y);
      ++iterated;
    }
  const float at_start = planner.get_expanded_map().get_g(Elem(4, 4));
  std::printf("size %zu iterated %zu sum %.9g following %d g_start %.9g consistent %d\n", n, iterated, sum, (int)planner.map.following(), at_start,
              (int)planner.map.consistent(Elem(4, 4)));
  return planner.map.follow_changes(false) == UFM_OK && n == iterated ? 0 : 4;
}
