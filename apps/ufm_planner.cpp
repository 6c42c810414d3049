// ufm_planner -- planner process for the reference's simulator / test harness.
//
// Speaks the wire protocol of the reference drivers (Tests/Planners/{FDSTAR,SGDFM,DFM}/main.cpp
// <-> Simulator/simulator/run_simulator.py:38-103, Tests/run_test.py:85-177)
// over two named FIFOs, so that run_test.py / run_simulator.py drive the MI355X engine instead of
// the CPU planners: point the `planners` table of run_test.py (:12-20) at this executable (or at a
// symlink named like the reference's binaries, e.g. dfm_planner_1, field_d_planner_1_no_heur --
// the planner and its level are then taken from the name).
//
// Built on the mirror of the reference's planner surface (unige-tasi-path-planners_amd/include),
// i.e. on exactly the classes and members the reference drivers use: PlannerT<LVL>,
// LinearInterpolationPathExtractor, reset / set_* / patch_map / step / extract_path, u_time,
// p_time, e_time, map.size(), map.buckets.
//
//   ufm_planner [--planner FD|SG|DFM] [--level K] [--max-moves N] [--verify-follow] [--inflate D] [--margin OUTER STEP] [--auto-heuristic] [--sense R] [--image K P] [--layers N] <fifo_in> <fifo_out>
//        start, goal and the `tof` flag arrive in-band after the map (DFM/main.cpp:62-67)
//   ufm_planner [...] <mapfile> <from_x> <from_y> <to_x> <to_y> <cspace> <fifo_in> <fifo_out> <gui> <tof> <outpath>
//        the 11-argument form of FDSTAR/main.cpp:16-31 and SGDFM/main.cpp
// --inflate D: the map and the patches on the wire are RAW and the engine plans on their dilation by the disc of diameter D
// (ufm_set_cspace; x^2 + y^2 <= (D / 2)^2 on a (2 (D / 2) + 1)-cell square, the footprint of the Python harness' dilate) -- the simulator
// then need not inflate anything.  The positional <cspace> stays as inert as it is in the reference drivers.
// --margin OUTER STEP: a soft margin around the disc of --inflate D (without --inflate: D = 1): the footprint is the cone
// ufm_cspace_cone(D, OUTER, STEP) -- the disc at full cost, then STEP less per cell of distance out to the diameter OUTER
// (ufm_set_cspace_graded, include/ufm_cspace_graded.h).  The wire carries RAW data as with --inflate.
// --auto-heuristic: the heuristic multiplier is the smallest cost of the planning raster as the engine holds it (the cost census,
// ufm_track_costs + "auto_multiplier"); the wire's min_cost is read, as the protocol demands, and not used -- with --inflate the simulator
// then need not know the inflated map at all.
// --sense R: the planner senses for itself (ufm_set_sensor / ufm_set_survey / ufm_reveal).  The survey raster -- the simulator's
// high-resolution data, of the map's size -- arrives ONCE, directly after the map raster; every move's patch message then has h = w = 0
// and no bytes, and before each step the planner uncovers the disc x^2 + y^2 <= R^2 around the cell it has just reported: each
// coordinate AS SENT (the cell planners' display shift included) rounded half-to-even, as Python's round does at Tests/run_test.py:143.
// Composes with --inflate and --auto-heuristic: the simulator then touches no raster after the start.
// --image K P: the planner prepares the map itself (ufm_set_image).  Where the map raster would arrive the wire carries the grey-scale
// BITMAP, framed the same way (width, height, bytes, then min_cost as always); the planner blurs it with ufm_gaussian_taps(K), K odd,
// 1 .. 31, complements it and adds the saturating penalty P, 0 .. 255 -- the simulator's simulation_data (run_simulator.py:106-113,148) --
// and the same launch leaves the complemented bitmap as the survey: with --sense R no separate survey message is sent.  Composes with
// --inflate and --auto-heuristic: the simulator then hands over a bitmap and positions, nothing else.
// --layers N: the map is the maximum of N cost layers the engine keeps (ufm_set_layers), N = 2 .. 4; needs --sense.  Layer 0 is the map as
// it arrives (or as --image makes it) with its survey; behind the map message and the survey message (the latter absent with --image)
// N - 1 more rasters of width x height bytes follow on the wire: the surveys of layers 1 .. N - 1, whose known layers start at zero
// (rock_aboundance_l = np.zeros(...), Tests/run_test.py:102).  Every move then uncovers the disc in all N layers with one reveal.
// Composes with --inflate, --auto-heuristic and --image.
// With `tof` the expanded-element dump after every step is kept up to date from the steps' deltas (ExpandedMap::follow_changes), not
// read back whole; --verify-follow also builds it the old way every step -- a read of the whole field through a second view of the
// same planner -- and ends the run (exit code 3) if the two differ in any element, value, Info or order.
// Keys with the heuristic term unless compiled with -DNO_HEURISTIC (binary ufm_planner_no_heur),
// as for the reference's *_no_heur targets.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "DynamicFastMarching.h"
#include "FieldDPlanner.h"
#include "Graph.h"
#include "LinearInterpolationPathExtractor.h"
#include "ShiftedGridPlanner.h"

namespace {

// raw little-endian structs over a byte stream (both ends run on the same host)
class Wire {
 public:
  Wire(const char *in_path, const char *out_path) {
    // open order as in the reference drivers: read end first, then the write end
    in_ = std::fopen(in_path, "rb");
    if (!in_) throw std::runtime_error(std::string("cannot open ") + in_path);
    out_ = std::fopen(out_path, "wb");
    if (!out_) throw std::runtime_error(std::string("cannot open ") + out_path);
  }
  ~Wire() {
    if (out_) std::fclose(out_);
    if (in_) std::fclose(in_);
  }
  template <typename T> void put(const T &v) { if (std::fwrite(&v, sizeof(T), 1, out_) != 1) throw std::runtime_error("peer closed the pipe (write)"); }
  void put_bytes(const void *p, size_t n) { if (n && std::fwrite(p, 1, n, out_) != n) throw std::runtime_error("peer closed the pipe (write)"); }
  void flush() { std::fflush(out_); }
  template <typename T> T get() { T v; get_bytes(&v, sizeof(T)); return v; }
  void get_bytes(void *p, size_t n) { if (n && std::fread(p, 1, n, in_) != n) throw std::runtime_error("peer closed the pipe (read)"); }
  void expect(int8_t code) { while (get<int8_t>() != code) {} }      // "wait for <code>"

 private:
  FILE *in_ = nullptr, *out_ = nullptr;
};

struct Options {
  std::string planner = "DFM";
  int level = 1;
  long max_moves = -1;
  bool inband = true;        // start / goal / tof follow the map on the wire
  float from_x = 0, from_y = 0, to_x = 0, to_y = 0;
  bool tof = false;
  bool verify_follow = false;
  int inflate = 0;           // --inflate D: footprint diameter (<= 1: off)
  int margin_outer = 0;      // --margin OUTER STEP: the cone around that disc out to the diameter OUTER (0: off) ...
  int margin_step = 0;       // ... losing STEP per cell
  bool auto_heuristic = false;   // --auto-heuristic: the multiplier follows the engine's planning raster
  int sense = -1;            // --sense R: radius of the field of view the planner uncovers itself (< 0: off)
  int image = 0;             // --image K P: the wire carries the bitmap, blurred here with K Gaussian taps (0: off) ...
  int image_penalty = 0;     // ... and P added, saturating
  int layers = 1;            // --layers N: cost layers of the engine; the surveys of layers 1 .. N - 1 follow the survey on the wire
  std::string fifo_in, fifo_out;
};

std::shared_ptr<uint8_t> byte_block(size_t n) { return std::shared_ptr<uint8_t>(new uint8_t[n], std::default_delete<uint8_t[]>()); }

template <typename Planner>
int serve(Options opt, bool cell_planner, bool indirect) {
  typedef typename Planner::Map::ElemType Elem;
  Wire io(opt.fifo_in.c_str(), opt.fifo_out.c_str());

  // 1. handshake, 2. map (+ start / goal / tof in-band) + heuristic hint
  io.put<int8_t>(0); io.flush();
  io.expect(0);
  int32_t width = io.get<int32_t>(), height = io.get<int32_t>();
  std::printf("[PLANNER]   Size: [%d, %d]\n", width, height);
  if (width <= 0 || height <= 0) throw std::runtime_error("bad map size");
  auto data = byte_block((size_t)width * height);
  io.get_bytes(data.get(), (size_t)width * height);
  std::shared_ptr<uint8_t> survey;
  if (opt.sense >= 0 && !opt.image) {
    survey = byte_block((size_t)width * height);
    io.get_bytes(survey.get(), (size_t)width * height);
  }
  std::vector<std::shared_ptr<uint8_t>> layer_surveys;
  for (int k = 1; k < opt.layers; ++k) {
    layer_surveys.push_back(byte_block((size_t)width * height));
    io.get_bytes(layer_surveys.back().get(), (size_t)width * height);
  }
  if (opt.inband) {
    opt.from_x = io.get<float>(); opt.from_y = io.get<float>();
    opt.to_x = io.get<float>(); opt.to_y = io.get<float>();
    opt.tof = io.get<uint8_t>() != 0;
  }
  int32_t min_cost = io.get<int32_t>();

  Position next_point(opt.from_x, opt.from_y), goal(opt.to_x, opt.to_y);
  float next_step_cost = 0;

  Planner planner{};
  LinearInterpolationPathExtractor<Elem, typename Planner::Base::Info> extractor(planner.get_expanded_map(), planner.get_grid());
  extractor.allow_indirect_traversals = indirect;
  planner.reset();
  planner.set_occupancy_threshold(1);
  planner.set_heuristic_multiplier((float)min_cost);
  if (opt.auto_heuristic) planner.set_auto_heuristic(true);
  if (opt.margin_outer > 0) {
    std::vector<uint8_t> cone((size_t)31 * 31);
    if (ufm_cspace_cone(std::max(opt.inflate, 1), opt.margin_outer, opt.margin_step, cone.data()) != UFM_OK)
      throw std::runtime_error("--margin: D <= OUTER <= 31, at most 15 rings, STEP is 1 .. 254");
    const int n = 2 * (opt.margin_outer / 2) + 1;
    planner.set_cspace_graded(cone.data(), n, n);
  } else if (opt.inflate > 1) {
    const int r = opt.inflate / 2, n = 2 * r + 1;
    if (n > 31) throw std::runtime_error("--inflate: the footprint is at most 31 cells wide");
    std::vector<uint8_t> disc((size_t)n * n);
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        disc[(size_t)a * n + b] = (double)((b - r) * (b - r)) / (double)(r * r) + (double)((a - r) * (a - r)) / (double)(r * r) <= 1.0;
    planner.set_cspace(disc.data(), n, n);
  }
  if (opt.layers > 1 && planner.set_layers(opt.layers) != UFM_OK) throw std::runtime_error("--layers: N is 1 .. " + std::to_string(UFM_MAX_LAYERS));
  if (opt.image) {
    uint16_t taps[31];
    if (ufm_gaussian_taps(opt.image, taps) != UFM_OK) throw std::runtime_error("--image: K is odd, 1 .. 31");
    planner.set_image(data, width, height, taps, opt.image, opt.image_penalty);
    if (planner.last_error != UFM_OK) throw std::runtime_error("set_image failed with " + std::to_string(planner.last_error));
  } else {
    planner.set_map(data, width, height);
  }
  // --sense: the disc of harness.round_patch_update / run_simulator.py:9-28.  A position on the map's far border rounds to a cell one
  // beyond the last (nodes run 0 .. length): the simulator's disc then hangs over the border, here the anchor moves by that one cell.
  std::vector<uint8_t> fov;
  int fov_n = 0, fov_ar = -1, fov_ac = -1;
  auto sense_at = [&](float sent_x, float sent_y) {
    const int r = opt.sense;
    int row = (int)std::nearbyint(sent_x), col = (int)std::nearbyint(sent_y);
    const int crow = std::min(std::max(row, 0), height - 1), ccol = std::min(std::max(col, 0), width - 1);
    const int ar = r + crow - row, ac = r + ccol - col;
    if (ar < 0 || ac < 0 || ar >= fov_n || ac >= fov_n) return;        // (the whole disc lies outside the map: nothing is seen)
    if (ar != fov_ar || ac != fov_ac) { planner.set_sensor(fov.data(), fov_n, fov_n, ar, ac); fov_ar = ar; fov_ac = ac; }
    if (planner.reveal(crow, ccol) != UFM_OK) throw std::runtime_error("reveal failed with " + std::to_string(planner.last_error));
  };
  if (opt.sense >= 0) {
    const int r = opt.sense;
    fov_n = 2 * r + 1;
    if (fov_n > 127) throw std::runtime_error("--sense: the field of view is at most 127 cells wide");
    fov.resize((size_t)fov_n * fov_n);
    for (int a = 0; a < fov_n; ++a)
      for (int b = 0; b < fov_n; ++b) fov[(size_t)a * fov_n + b] = (a - r) * (a - r) + (b - r) * (b - r) <= r * r;
    if (!opt.image) planner.set_survey(survey, width, height);        // (--image: set_image has left the survey)
    if (planner.last_error != UFM_OK) throw std::runtime_error("set_survey failed with " + std::to_string(planner.last_error));
    for (int k = 1; k < opt.layers; ++k)
      if (planner.set_layer_survey(k, layer_surveys[(size_t)k - 1], width, height) != UFM_OK)
        throw std::runtime_error("set_layer_survey failed with " + std::to_string(planner.last_error));
  }
  // the dump after every step: follow the steps' deltas on the host instead of reading the whole field back each time
  if (opt.tof && planner.map.follow_changes(true) != UFM_OK) throw std::runtime_error("follow_changes failed");
  planner.set_start(next_point);
  planner.set_goal(goal);

  // 3. one round per robot move
  for (long move = 0; opt.max_moves < 0 || move < opt.max_moves; ++move) {
    std::printf("[PLANNER]   New position: [%g, %g]\n", next_point.x, next_point.y);
    const float shift = cell_planner ? 0.5f : 0.0f;        // cell centres, for the simulator's display
    io.put<int8_t>(1);
    io.put<float>(next_point.x + shift); io.put<float>(next_point.y + shift);
    io.put<float>(next_step_cost);
    io.flush();

    io.expect(1);
    const int32_t top = io.get<int32_t>(), left = io.get<int32_t>(), ph = io.get<int32_t>(), pw = io.get<int32_t>();
    std::printf("[PLANNER]   New patch: position [%d, %d], shape [%d, %d]\n", top, left, pw, ph);
    if (pw < 0 || ph < 0) throw std::runtime_error("bad patch shape");
    auto patch = byte_block((size_t)pw * ph + 1);
    io.get_bytes(patch.get(), (size_t)pw * ph);
    if (pw > 0 && ph > 0) planner.patch_map(patch, top, left, pw, ph);
    if (opt.sense >= 0) sense_at(next_point.x + shift, next_point.y + shift);
    min_cost = io.get<int32_t>();
    if (!opt.auto_heuristic) planner.set_heuristic_multiplier((float)min_cost);

    const int rc = planner.step();
    if (rc != LOOP_OK) throw std::runtime_error("step() returned " + std::to_string(rc));
    extractor.extract_path();
    if (extractor.last_error != UFM_OK) throw std::runtime_error("extract_path failed with " + std::to_string(extractor.last_error));

    io.put<int8_t>(3);
    io.put<int32_t>((int32_t)extractor.path_.size());
    for (const Position &p : extractor.path_) { io.put<float>(p.x); io.put<float>(p.y); }
    for (float c : extractor.cost_) io.put<float>(c);
    io.put<float>(extractor.total_dist); io.put<float>(extractor.total_cost);
    io.put<float>(planner.u_time); io.put<float>(planner.p_time); io.put<float>(extractor.e_time);
    io.flush();

    if (opt.tof) {          // every element that holds a value, as (x, y, g, rhs)
      io.put<int8_t>(4);
      const size_t held = planner.map.size();
      if (opt.verify_follow) {
        typename Planner::Map whole;
        int nx = 0, ny = 0;
        whole.attach(planner.native_handle());
        if (ufm_field_dims(planner.native_handle(), &nx, &ny) != UFM_OK) throw std::runtime_error("ufm_field_dims failed");
        whole.set_dims(nx, ny);
        if (whole.size() != held || !(whole.buckets == planner.map.buckets)) throw std::runtime_error("the followed map differs from a read of the whole field");
      }
      io.put<int64_t>((int64_t)held);
      for (const auto &bucket : planner.map.buckets) {
        for (const auto &kv : bucket) {
          const Elem &el = kv.first;
          io.put<int32_t>(el.x); io.put<int32_t>(el.y);
          io.put<float>(std::get<0>(kv.second)); io.put<float>(std::get<1>(kv.second));
        }
        io.flush();
      }
    }

    // follow the extracted path until more than 5 cells away from where we stand
    const Position here = next_point;
    for (size_t i = 1; i < extractor.path_.size(); ++i) {
      next_point = extractor.path_[i];
      if (i - 1 < extractor.cost_.size()) next_step_cost = extractor.cost_[i - 1];
      if (Cell(next_point).distance(Cell(here)) > 5) break;
    }
    if (next_point == goal) break;
    planner.set_start(next_point);
  }

  // 4. end of run
  io.put<int8_t>(2); io.flush();
  io.expect(2);
  return 0;
}

void usage(const char *argv0) {
  std::fprintf(stderr,
               "Usage:\n\t%s [--planner FD|SG|DFM] [--level K] [--max-moves N] [--verify-follow] [--inflate D] [--margin OUTER STEP] [--auto-heuristic] [--sense R] [--image K P] [--layers N] <fifo_in> <fifo_out>\n"
               "\t%s [...] <mapfile> <from_x> <from_y> <to_x> <to_y> <cspace> <fifo_in> <fifo_out> <gui> <tof> <outpath>\n",
               argv0, argv0);
}

// planner and level from a reference-style binary name: field_d_planner_1[_no_heur],
// shifted_grid_planner_2, dfm_planner_0 (CMakeLists.txt:30-59)
void from_program_name(const std::string &argv0, Options &opt) {
  const size_t slash = argv0.find_last_of('/');
  const std::string base = slash == std::string::npos ? argv0 : argv0.substr(slash + 1);
  if (base.find("field_d") != std::string::npos) opt.planner = "FD";
  else if (base.find("shifted_grid") != std::string::npos) opt.planner = "SG";
  else if (base.find("dfm") != std::string::npos) opt.planner = "DFM";
  else return;
  const size_t k = base.find("planner_");
  if (k != std::string::npos && k + 8 < base.size() && base[k + 8] >= '0' && base[k + 8] <= '2') opt.level = base[k + 8] - '0';
}

}  // namespace

int main(int argc, char **argv) {
  Options opt;
  from_program_name(argv[0], opt);
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--planner" && i + 1 < argc) opt.planner = argv[++i];
    else if (a == "--level" && i + 1 < argc) opt.level = std::atoi(argv[++i]);
    else if (a == "--max-moves" && i + 1 < argc) opt.max_moves = std::atol(argv[++i]);
    else if (a == "--verify-follow") opt.verify_follow = true;
    else if (a == "--inflate" && i + 1 < argc) opt.inflate = std::atoi(argv[++i]);
    else if (a == "--margin" && i + 2 < argc) { opt.margin_outer = std::atoi(argv[++i]); opt.margin_step = std::atoi(argv[++i]); }
    else if (a == "--auto-heuristic") opt.auto_heuristic = true;
    else if (a == "--sense" && i + 1 < argc) opt.sense = std::atoi(argv[++i]);
    else if (a == "--image" && i + 2 < argc) { opt.image = std::atoi(argv[++i]); opt.image_penalty = std::atoi(argv[++i]); }
    else if (a == "--layers" && i + 1 < argc) opt.layers = std::atoi(argv[++i]);
    else if (a == "-h" || a == "--help") { usage(argv[0]); return 0; }
    else pos.push_back(a);
  }
  if (opt.layers != 1 && (opt.sense < 0 || opt.layers < 1 || opt.layers > UFM_MAX_LAYERS)) {
    std::fprintf(stderr, "--layers N needs --sense R, N = 1 .. %d\n", UFM_MAX_LAYERS);
    usage(argv[0]);
    return 1;
  }
  try {
    if (pos.size() == 2) {
      opt.fifo_in = pos[0]; opt.fifo_out = pos[1];
    } else if (pos.size() >= 11) {
      opt.inband = false;
      opt.from_x = std::stof(pos[1]); opt.from_y = std::stof(pos[2]);
      opt.to_x = std::stof(pos[3]); opt.to_y = std::stof(pos[4]);
      opt.fifo_in = pos[6]; opt.fifo_out = pos[7];
      opt.tof = std::stoi(pos[9]) != 0;
    } else {
      usage(argv[0]);
      return 1;
    }
    const std::string &p = opt.planner;
    const int k = opt.level;
    // extractor settings as in the reference drivers: FDSTAR/main.cpp:82, SGDFM/main.cpp:97, DFM/main.cpp:80
    if (p == "FD" && k == 0) return serve<FieldDPlanner<0>>(opt, false, true);
    if (p == "FD" && k == 1) return serve<FieldDPlanner<1>>(opt, false, true);
    if (p == "SG" && k == 0) return serve<ShiftedGridPlanner<0>>(opt, false, false);
    if (p == "SG" && k == 1) return serve<ShiftedGridPlanner<1>>(opt, false, false);
    if (p == "SG" && k == 2) return serve<ShiftedGridPlanner<2>>(opt, false, false);
    if (p == "DFM" && k == 0) return serve<DFMPlanner<0>>(opt, true, true);
    if (p == "DFM" && k == 1) return serve<DFMPlanner<1>>(opt, true, true);
    std::fprintf(stderr, "unknown planner %s level %d\n", p.c_str(), k);
    return 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "[PLANNER]   error: %s\n", e.what());
    return 3;
  }
}
