// LinearInterpolationPathExtractor.h -- the reference's path extractor
// (PathExtraction/LinearInterpolationPathExtractor.h:8-40) on the MI355X engine.
//
// Same template signature, constructor and public members (path_, cost_, total_cost, total_dist,
// lookahead, max_steps, e_time, allow_indirect_traversals, extract_path()), so the reference
// drivers' use of it (Tests/Planners/FDSTAR/main.cpp:78-82,116-136,158-160) compiles unchanged.
// extract_path() is one call of ufm_extract_path: the walk over the RHS field, its lookahead and
// the traversal case tables run on the device (one wavefront), the field stays in HBM; start and
// goal are the positions last given to the planner (Graph::start_pos_, goal_pos_).
#ifndef UFM_LINEAR_INTERPOLATION_PATH_EXTRACTOR_H
#define UFM_LINEAR_INTERPOLATION_PATH_EXTRACTOR_H
#include <iostream>
#include <vector>

#include "ExpandedMap.h"
#include "Graph.h"
#include "InterpolatedTraversal.h"
#include "ufm.h"

template <typename E, typename T>
class LinearInterpolationPathExtractor {
 public:
  LinearInterpolationPathExtractor(const ExpandedMap<E, T> &map, const Graph &grid) : map(map), grid(grid) {}

  void extract_path() {
    path_.clear();
    cost_.clear();
    total_cost = 0;
    total_dist = 0;
    e_time = 0;
    const int cap_p = 3 * max_steps + 1, cap_c = 2 * max_steps;
    std::vector<float> xy(2 * static_cast<size_t>(cap_p)), sc(static_cast<size_t>(cap_c));
    ufm_path_info info{};
    last_error = ufm_extract_path(map.native_handle(), max_steps, lookahead ? 1 : 0, allow_indirect_traversals ? 1 : 0,
                                  xy.data(), cap_p, sc.data(), cap_c, &info);
    if (last_error != UFM_OK) return;
    total_cost = info.total_cost;
    total_dist = info.total_dist;
    e_time = info.e_ms;
    if (info.n_points == 0) {                       // impl:49-51
      std::cerr << "[Extraction] No valid path exists" << std::endl;
      return;
    }
    path_.reserve(info.n_points);
    for (int i = 0; i < info.n_points; ++i) path_.emplace_back(xy[2 * i], xy[2 * i + 1]);
    cost_.assign(sc.begin(), sc.begin() + info.n_costs);
  }

  // Not in the reference: paths from many positions of the field as it stands, in one call of ufm_extract_paths_from (one
  // wavefront per position).  A query: the planner's start and this object's path_ / cost_ / totals stay as they are.  One
  // record per position, in their order, each what extract_path() would leave had the planner started there (an empty path_:
  // no valid path exists); empty, with last_error set, when the call fails.
  struct PathFrom {
    std::vector<Position> path_;
    std::vector<float> cost_;
    float total_cost = 0;
    float total_dist = 0;
  };
  std::vector<PathFrom> extract_paths_from(const std::vector<Position> &starts) {
    std::vector<PathFrom> out;
    const size_t n = starts.size(), cap_p = 3 * static_cast<size_t>(max_steps) + 1, cap_c = 2 * static_cast<size_t>(max_steps);
    std::vector<float> from(2 * n), xy(2 * cap_p * n), sc(cap_c * n);
    for (size_t k = 0; k < n; ++k) { from[2 * k] = starts[k].x; from[2 * k + 1] = starts[k].y; }
    std::vector<ufm_path_info> info(n);
    last_error = ufm_extract_paths_from(map.native_handle(), static_cast<int>(n), from.data(), max_steps, lookahead ? 1 : 0,
                                        allow_indirect_traversals ? 1 : 0, xy.data(), static_cast<int>(cap_p), sc.data(),
                                        static_cast<int>(cap_c), info.data());
    if (last_error != UFM_OK) return out;
    out.resize(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].total_cost = info[k].total_cost;
      out[k].total_dist = info[k].total_dist;
      const float *p = xy.data() + 2 * cap_p * k;
      for (int i = 0; i < info[k].n_points; ++i) out[k].path_.emplace_back(p[2 * i], p[2 * i + 1]);
      out[k].cost_.assign(sc.begin() + cap_c * k, sc.begin() + cap_c * k + info[k].n_costs);
    }
    return out;
  }

  // Not in the reference: what the CALLER's polylines cost on the raster the planner plans on, and whether they are blocked, in one
  // call of ufm_score_paths (one wavefront per path).  A query, as extract_paths_from(): nothing of the planner or of this object
  // changes.  One record per path, in their order (include/ufm_score.h); empty, with last_error set, when the call
  // fails -- an empty list of paths included.
  std::vector<ufm_score> score_paths(const std::vector<std::vector<Position>> &paths) {
    std::vector<ufm_score> out;
    std::vector<int32_t> offsets(paths.size() + 1, 0);
    std::vector<float> xy;
    for (size_t k = 0; k < paths.size(); ++k) {
      for (const Position &pose : paths[k]) { xy.push_back(pose.x); xy.push_back(pose.y); }
      offsets[k + 1] = static_cast<int32_t>(xy.size() / 2);
    }
    if (xy.empty()) xy.resize(2);      // (an address even when no path has a point)
    std::vector<ufm_score> records(paths.size());
    last_error = ufm_score_paths(map.native_handle(), static_cast<int>(paths.size()), offsets.data(), xy.data(), records.data());
    if (last_error == UFM_OK) out.swap(records);
    return out;
  }

  std::vector<Position> path_{};
  std::vector<float> cost_{};
  float total_cost = 0;
  float total_dist = 0;
  bool lookahead = true;
  int max_steps = 20;
  float e_time = 0;
  bool allow_indirect_traversals = true;
  int last_error = 0;       // ufm code of the last call (not in the reference)

 private:
  const ExpandedMap<E, T> &map;
  const Graph &grid;
};
#endif
