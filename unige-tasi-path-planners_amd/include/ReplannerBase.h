// ReplannerBase.h -- the planner driver surface of the reference
// (ProjectToolkit/include/ReplannerBase.h:29-163) on top of the MI355X engine (libufm.so).
//
// Same template signature, typedefs, public data members and methods, so a driver written for
// the reference (Tests/Planners/*/main.cpp) compiles against it: reset(), step(),
// set_occupancy_threshold(), set_heuristic_multiplier(), set_map(), patch_map(), set_start(),
// set_goal(), get_expanded_map(), get_grid(); u_time / p_time, num_nodes_updated /
// num_nodes_expanded, grid, map, priority_queue -- the last as a read view (PriorityQueue.h: size / empty /
// top_key / top_value / ordered iteration over the elements that are not consistent, derived from the field;
// the engine has no heap, its tile queues live on the device).  What is not here: enqueue_if_inconsistent()
// and the queue's mutators -- nothing outside the device decides what is relaxed next.
// step() returns LOOP_OK / LOOP_FAILURE_NO_GRAPH / LOOP_FAILURE_NO_GOAL like the reference; a
// device error is returned as the negative ufm code and kept in last_error.
#ifndef UFM_REPLANNER_BASE_H
#define UFM_REPLANNER_BASE_H

#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "ExpandedMap.h"
#include "Graph.h"
#include "GridTypes.h"
#include "PriorityQueue.h"
#include "ufm.h"

#define LOOP_OK 0
#define LOOP_FAILURE_NO_GRAPH -1
#define LOOP_FAILURE_NO_GOAL -2

template <typename Derived, typename MapElem_, typename MapInfo_, typename QueueKey_>
class ReplannerBase {
 public:
  typedef QueueKey_ Key;
  typedef MapElem_ Elem;
  typedef MapInfo_ Info;
  typedef ExpandedMap<MapElem_, MapInfo_> Map;
  typedef PriorityQueue<QueueKey_, MapElem_> Queue;
  float u_time = 0, p_time = 0;

  void reset() { initialize_search = true; check(ufm_reset(handle_)); map.invalidate(); priority_queue.invalidate(); }

  int step() {
    if (initialize_graph) return LOOP_FAILURE_NO_GRAPH;
    if (!goal_set) return LOOP_FAILURE_NO_GOAL;
    ufm_stats st{};
    const int rc = ufm_step(handle_, &st);
    map.invalidate();
    priority_queue.invalidate();
    if (rc != UFM_OK) { last_error = rc; return rc; }
    if (map.following()) {        // opt-in (map.follow_changes): the host copy takes the step's delta
      const int rd = map.apply_changes();
      if (rd != UFM_OK) { last_error = rd; return rd; }
    }
    if (auto_heuristic_) check(ufm_heuristic_multiplier(handle_, &used_multiplier_));   // the queue view's keys use what the step used
    u_time = st.u_ms; p_time = st.p_ms;
    num_nodes_updated = st.updated; num_nodes_expanded = st.expanded;
    stats = st;
    new_goal = initialize_search = new_start = false;
    return LOOP_OK;
  }

  void set_occupancy_threshold(float threshold) { grid.set_occupancy_threshold(threshold); check(ufm_set_occupancy_threshold(handle_, threshold)); }
  void set_heuristic_multiplier(float mult) { heuristic_multiplier = mult; check(ufm_set_heuristic_multiplier(handle_, mult)); }

  /** C-space inflation on the device (ufm_set_cspace; no reference counterpart: the reference's simulator dilates on the host): the
   *  vehicle's footprint mask[mh][mw] with its anchor (-1, -1: the centre), before the first set_map.  set_map / patch_map then take the
   *  RAW raster; `grid` keeps holding that raw raster, the engine plans (and the extractor walks) on its dilation. */
  void set_cspace(const uint8_t *mask, int mw, int mh, int anchor_row = -1, int anchor_col = -1) {
    check(ufm_set_cspace(handle_, mask, mw, mh, anchor_row, anchor_col));
  }
  /** The same with a drop per cell (ufm_set_cspace_graded, include/ufm_cspace_graded.h): drop[mh][mw], 255 = outside, drop[anchor] == 0. */
  void set_cspace_graded(const uint8_t *drop, int mw, int mh, int anchor_row = -1, int anchor_col = -1) {
    check(ufm_set_cspace_graded(handle_, drop, mw, mh, anchor_row, anchor_col));
  }
  /** Sensor reveal on the device (ufm_set_sensor / ufm_set_survey / ufm_reveal; no reference counterpart: the reference's simulator keeps
   *  the high-resolution raster and ships the revealed rectangle every move, run_simulator.py:9-28,177): the field of view mask[mh][mw]
   *  with its anchor (-1, -1: the centre), the survey raster -- what the sensor would see, of the map's size, after set_map --, and
   *  reveal(row, col), which uncovers the field of view around that cell as a patch_map of those bytes would; changed (optional) gets the
   *  number of cells that changed and makes the call wait.  `grid` keeps the raster the host handed over: it does not follow reveals. */
  void set_sensor(const uint8_t *mask, int mw, int mh, int anchor_row = -1, int anchor_col = -1) {
    check(ufm_set_sensor(handle_, mask, mw, mh, anchor_row, anchor_col));
  }
  void set_survey(const std::shared_ptr<uint8_t> &survey, int w, int h) { check(ufm_set_survey(handle_, survey.get(), w, h)); }
  int reveal(int row, int col, uint64_t *changed = nullptr) {
    const int rc = ufm_reveal(handle_, row, col, changed);
    if (rc != UFM_OK) last_error = rc;
    return rc;
  }
  /** Cost layers on the device (ufm_set_layers / ufm_patch_layer / ufm_set_layer / ufm_set_layer_survey; no reference counterpart: the
   *  reference's simulator keeps slope and rocks on the host and ships np.maximum of them, Tests/run_test.py:102,136-140): n rasters per
   *  map whose element-wise maximum is the raster the planner sees, set before the first set_map -- which feeds layer 0, as patch_map
   *  does.  patch_layer / set_layer store into layer k and patch the map with the maximum; with a survey per layer reveal() uncovers
   *  every layer at once.  `grid` keeps what set_map / patch_map were handed: it follows neither the other layers nor reveals. */
  int set_layers(int n) { return noted(ufm_set_layers(handle_, n)); }
  int patch_layer(int k, const std::shared_ptr<uint8_t> &patch, int x, int y, int w, int h) { return noted(ufm_patch_layer(handle_, k, patch.get(), x, y, w, h)); }
  int set_layer(int k, const std::shared_ptr<uint8_t> &raster, int w, int h) { return noted(ufm_set_layer(handle_, k, raster.get(), w, h)); }
  int set_layer_survey(int k, const std::shared_ptr<uint8_t> &survey, int w, int h) { return noted(ufm_set_layer_survey(handle_, k, survey.get(), w, h)); }
  int read_layer(int k, uint8_t *out) { return noted(ufm_read_layer(handle_, k, out)); }
  int read_layer_survey(int k, uint8_t *out) { return noted(ufm_read_layer_survey(handle_, k, out)); }
  /** Cost census (ufm_track_costs; no reference counterpart: the reference's simulator takes cv2.minMaxLoc of the map it inflated itself,
   *  run_simulator.py:152,183): exact counts of the PLANNING raster's values, kept under patches.  min_cost(): the smallest value present,
   *  -1 if the census is off or no map is set; cost_census(): all 256 counters, returns the ufm code. */
  void track_costs(bool on = true) { check(ufm_track_costs(handle_, on ? 1 : 0)); }
  int min_cost() {
    int mn = -1;
    const int rc = ufm_read_cost_census(handle_, nullptr, &mn, nullptr);
    if (rc != UFM_OK) { last_error = rc; return -1; }
    return mn;
  }
  int cost_census(uint64_t hist[256], int *min_cost = nullptr, int *max_cost = nullptr) {
    const int rc = ufm_read_cost_census(handle_, hist, min_cost, max_cost);
    if (rc != UFM_OK) last_error = rc;
    return rc;
  }
  /** step() takes min_cost() of the planning raster as it stands as the heuristic multiplier, as the reference's drivers do with the
   *  simulator's hint (DFM/main.cpp:111-112); set_heuristic_multiplier is stored and ignored meanwhile.  Turns the census on. */
  void set_auto_heuristic(bool on = true) {
    check(ufm_set_param(handle_, "auto_multiplier", on ? 1.0 : 0.0));
    auto_heuristic_ = on;
    used_multiplier_ = heuristic_multiplier;
  }
  void set_map(const std::shared_ptr<uint8_t> &new_map, int w, int h) {
    grid.init(new_map, w, h);
    check(ufm_set_map(handle_, new_map.get(), w, h));
    int nx = 0, ny = 0;
    check(ufm_field_dims(handle_, &nx, &ny));
    map.set_dims(nx, ny);
    initialize_graph = false;
  }
  /** Map preparation on the device (ufm_set_image; no reference counterpart: the reference's simulator blurs, complements and penalises the
   *  bitmap on the host, run_simulator.py:106-113,148): in place of set_map, the grey-scale bitmap with the taps of one axis
   *  (ufm_gaussian_taps) and the penalty; the engine makes the map and its survey from it, so no set_survey follows.  `grid` then holds
   *  the BITMAP the host handed over -- its size, start and goal are right, its bytes are not costs. */
  void set_image(const std::shared_ptr<uint8_t> &image, int w, int h, const uint16_t *taps, int ntaps, int penalty) {
    grid.init(image, w, h);
    check(ufm_set_image(handle_, image.get(), w, h, taps, ntaps, penalty));
    int nx = 0, ny = 0;
    check(ufm_field_dims(handle_, &nx, &ny));
    map.set_dims(nx, ny);
    initialize_graph = false;
  }
  void patch_map(const std::shared_ptr<uint8_t> &patch, int x, int y, int w, int h) {
    grid.update(patch, x, y, w, h);
    check(ufm_patch_map(handle_, patch.get(), x, y, w, h));
  }
  void set_start(const Position &pos) { grid.set_start(pos); new_start = true; check(ufm_set_start(handle_, pos.x, pos.y)); }
  void set_goal(const Position &point) {
    if constexpr (std::is_same<MapElem_, Node>::value) new_goal = grid.goal_node_ != Node(point);
    else new_goal = grid.goal_cell_ != Cell(point);
    grid.set_goal(point);
    goal_set = true;
    check(ufm_set_goal(handle_, point.x, point.y));
  }

  const Map &get_expanded_map() { return map; }
  const Graph &get_grid() { return grid; }

  /** engine knobs without a reference counterpart (ufm_set_param) */
  void set_engine_param(const char *name, double v) { check(ufm_set_param(handle_, name, v)); }
  ufm_t *native_handle() { return handle_; }

  unsigned long num_nodes_updated = 0;
  unsigned long num_nodes_expanded = 0;
  float heuristic_multiplier = 1;
  bool initialize_graph = true;
  bool initialize_search = true;
  bool goal_set = false;
  bool new_goal = false;
  bool new_start = false;
  int last_error = 0;
  ufm_stats stats{};

  Queue priority_queue;
  Graph grid;
  Map map;

 protected:
  ReplannerBase(int algo, int opt_lvl, bool use_heuristic, int device = 0) {
    const int rc = ufm_create(&handle_, algo, opt_lvl, use_heuristic ? 1 : 0, device);
    if (rc != UFM_OK) throw std::runtime_error("ufm_create failed with code " + std::to_string(rc) + " (no MI355X / libufm.so?)");
    map.attach(handle_);
    priority_queue.attach(handle_, [this](const MapElem_ &s, float cost_so_far) { return calculate_key(s, cost_so_far); });
  }

  /** FieldDPlanner_impl.h:177-186, ShiftedGridPlanner_impl.h (same), DynamicFastMarching_impl.h:146-155 */
  Key calculate_key(const MapElem_ &s, float cost_so_far) const {
    if constexpr (std::is_same<Key, float>::value) {
      (void)s;
      return cost_so_far;
    } else {
      float dist;
      if constexpr (std::is_same<MapElem_, Node>::value) dist = s.distance(grid.start_pos_);
      else dist = grid.start_cell_.distance(s);
      return {cost_so_far + (auto_heuristic_ ? used_multiplier_ : heuristic_multiplier) * dist, cost_so_far};
    }
  }
  ~ReplannerBase() { if (handle_) ufm_destroy(handle_); }
  ReplannerBase(const ReplannerBase &) = delete;
  ReplannerBase &operator=(const ReplannerBase &) = delete;

 private:
  void check(int rc) { if (rc != UFM_OK) last_error = rc; }
  int noted(int rc) { check(rc); return rc; }
  ufm_t *handle_ = nullptr;
  bool auto_heuristic_ = false;
  float used_multiplier_ = 1;
};

namespace ufm_detail {
#ifdef NO_HEURISTIC
using key_type = float;
constexpr bool kHeuristic = false;
#else
using key_type = std::pair<float, float>;
constexpr bool kHeuristic = true;
#endif
}  // namespace ufm_detail

#endif  // UFM_REPLANNER_BASE_H
