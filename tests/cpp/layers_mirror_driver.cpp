// What the mirror adds for the cost layers (ReplannerBase::set_layers / patch_layer / set_layer / set_layer_survey / read_layer /
// read_layer_survey), used the way a driver would: next to the calls of the reference's surface, for a node planner and a cell planner,
// with and without heuristic keys.
// Type-checked against the mirrored headers (tests/test_layers_surface.py, g++ -fsyntax-only), with and without -DNO_HEURISTIC.
#include <cstdint>
#include <memory>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "ShiftedGridPlanner.h"

static_assert(UFM_MAX_LAYERS == 4, "the header's layer limit");

template <typename Planner>
static long drive() {
  const int32_t width = 64, height = 64;
  std::shared_ptr<uint8_t> slope(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> rocks(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> slope_h(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> rocks_h(new uint8_t[width * height](), std::default_delete<uint8_t[]>());
  std::shared_ptr<uint8_t> block(new uint8_t[4 * 3](), std::default_delete<uint8_t[]>());
  const uint8_t one[1] = {1};
  Position start, goal;
  start.x = 2; start.y = 2; goal.x = 60; goal.y = 60;
  Planner planner{};
  planner.reset();
  planner.set_occupancy_threshold(1);
  const int r0 = planner.set_layers(2);                                  // before the first map
  planner.set_sensor(one, 1, 1);
  planner.set_map(slope, width, height);                                 // layer 0; layer 1 starts at zero
  const int r1 = planner.set_layer(1, rocks, width, height);             // a whole-map patch
  const int r2 = planner.set_layer_survey(0, slope_h, width, height);    // = set_survey
  const int r3 = planner.set_layer_survey(1, rocks_h, width, height);
  planner.set_start(start);
  planner.set_goal(goal);
  const int r4 = planner.patch_layer(1, block, 10, 12, 4, 3);
  uint64_t changed = 0;
  const int r5 = planner.reveal(3, 2, &changed);                         // both layers in one launch
  const int rc = planner.step();
  uint8_t back[64 * 64];
  const int r6 = planner.read_layer(1, back);
  const int r7 = planner.read_layer_survey(1, back);
  const int r8 = ufm_patch_layer_device(planner.native_handle(), 0, nullptr, 0, 0, 1, 1);   // (rejected: a NULL buffer)
  return (long)r0 + r1 + r2 + r3 + r4 + r5 + rc + r6 + r7 + r8 + (long)changed + back[0] + planner.last_error;
}

int main() { return (int)(drive<FieldDPlanner<1>>() + drive<ShiftedGridPlanner<2>>() + drive<DFMPlanner<1>>() + drive<FieldDPlanner<0>>()); }
