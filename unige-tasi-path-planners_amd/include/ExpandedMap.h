// ExpandedMap.h -- read view of the search state with the reference's ExpandedMap interface
// (ProjectToolkit/include/ExpandedMap.h:25-73, impl/ExpandedMap_impl.h).
//
// The reference stores (g, rhs[, info]) per expanded element in hash maps.  Here the field lives
// densely in HBM; this view pages it to the host lazily in 64x64 blocks (ufm_read_field) the
// first time a block is read after a step(), so a consumer that walks a path (the reference's
// LinearInterpolationPathExtractor reads get_interp_rhs / get_rhs along ~20 steps) moves a few
// tens of KB, not the whole field.  Out-of-range and unreached elements read +inf, as in the
// reference (impl:54-85).  The engine is at a fixed point of the update operator after every
// step, so RHS == G for every element it finalised.
//
// OPT-IN, follow_changes(true): for a consumer that follows the state over a mission (the `tof` dump after every step, a GUI, a second
// planner layer).  The view then keeps a dense host copy of the values (and of the Info pairs of a level-1/2 planner) and
// ReplannerBase::step() brings it up to date from the step's delta (ufm_read_changes): every member reads the host copy, size() is a
// counter kept from the deltas, `buckets` is built from the copy -- no device traffic beyond the elements a step changed.
#ifndef UFM_EXPANDED_MAP_H
#define UFM_EXPANDED_MAP_H

#include <cmath>
#include <cstdint>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "GridTypes.h"
#include "Macros.h"
#include "ufm.h"

template <typename ElemType_, typename InfoType_>
class ExpandedMap {
 public:
  using ElemType = ElemType_;
  using InfoType = InfoType_;
  // (g, rhs) for the level-0 planners, (g, rhs, info) for the others -- as the reference's
  // ExpandedMap.h:27-29, so that std::get<2>(element.second) of a driver compiles
  using value_ = typename std::conditional<std::is_void<InfoType_>::value, std::tuple<float, float>,
                                           std::tuple<float, float, typename std::conditional<std::is_void<InfoType_>::value, int, InfoType_>::type>>::type;
  using bucket_ = std::vector<std::pair<const ElemType_, value_>>;

  /** Filled by size(): every element that holds a finite value, as (elem, (g, rhs[, info])) pairs in
   * one bucket per 256x256 block -- what the reference's `for (auto b : map.buckets)` dump iterates.
   * info (level-1/2 planners): the engine's stored back-pointer(s), ufm_read_info. */
  std::vector<bucket_> buckets;

  ExpandedMap() = default;

  float get_g(const ElemType &s) const { return value(s.x, s.y); }
  float get_rhs(const ElemType &s) const { return value(s.x, s.y); }
  std::pair<float, float> get_g_rhs(const ElemType &s) const { const float v = value(s.x, s.y); return {v, v}; }
  bool consistent(const ElemType &s) const { const auto gr = get_g_rhs(s); return gr.first == gr.second; }

  /** impl:87-101: node planners return RHS(node); the cell planner averages the four cells
   * around the node. */
  float get_interp_rhs(const Node &s) const {
    if constexpr (std::is_same<ElemType, Cell>::value) {
      const Cell p(static_cast<int>(std::floor(s.x - 0.5)), static_cast<int>(std::floor(s.y - 0.5)));
      return (get_rhs(p.bottom_cell()) + get_rhs(p) + get_rhs(p.bottom_right_cell()) + get_rhs(p.right_cell())) * 0.25f;
    } else {
      return get_rhs(s);
    }
  }

  /** impl:113-118.  Materialises `buckets` (reads the whole field once). */
  size_t size() const {
    auto *self = const_cast<ExpandedMap *>(this);
    if (follow_) { self->buckets_from_copy(); return count_; }
    self->buckets.clear();
    if (!handle_) return 0;
    std::vector<float> g(static_cast<size_t>(nx_) * ny_);
    if (ufm_read_field(handle_, 0, 0, nx_, ny_, g.data(), nullptr) != UFM_OK) return 0;
    const int bx = (nx_ >> 8) + 1, by = (ny_ >> 8) + 1;
    self->buckets.resize(static_cast<size_t>(bx) * by);
    std::vector<int32_t> info;
    if constexpr (!std::is_void<InfoType_>::value) {
      info.resize(static_cast<size_t>(nx_) * ny_ * 2);
      if (ufm_read_info(handle_, 0, 0, nx_, ny_, info.data()) != UFM_OK) return 0;
    }
    size_t n = 0;
    for (int x = 0; x < nx_; ++x)
      for (int y = 0; y < ny_; ++y) {
        const size_t e = static_cast<size_t>(x) * ny_ + y;
        const float v = g[e];
        if (v < INFINITY) {
          auto &bucket = self->buckets[static_cast<size_t>(x >> 8) * by + (y >> 8)];
          if constexpr (std::is_void<InfoType_>::value) bucket.emplace_back(ElemType(x, y), value_(v, v));
          else bucket.emplace_back(ElemType(x, y), value_(v, v, make_info(info[2 * e], info[2 * e + 1])));
          ++n;
        }
      }
    return n;
  }

  // ---- wiring (used by ReplannerBase) ----
  void attach(ufm_t *h) { handle_ = h; }
  ufm_t *native_handle() const { return handle_; }
  void set_dims(int nx, int ny) { nx_ = nx; ny_ = ny; invalidate(); if (follow_) empty_copy(); }   // (ufm_set_map has emptied the engine's baseline too)

  // ---- following the step deltas ----
  /** Turns the engine's change tracking on / off (ufm_track_changes) and with it the host copy; returns the engine's code.  Turned on
   * after steps have run, the copy is filled at once (the baseline starts empty, so the first delta is the whole state). */
  int follow_changes(bool on) {
    if (!handle_) return UFM_ERR_INVALID;
    const int rc = ufm_track_changes(handle_, on ? 1 : 0);
    if (rc != UFM_OK) return rc;
    follow_ = on;
    invalidate();
    buckets.clear();
    host_g_.clear(); host_info_.clear(); count_ = 0;
    if (!on) return UFM_OK;
    empty_copy();
    return nx_ > 0 ? apply_changes() : UFM_OK;
  }
  bool following() const { return follow_; }
  /** Reads the delta since the last call and applies it to the host copy (ReplannerBase::step() calls this); the record buffers grow
   * once when the delta does not fit them -- a delta is delivered whole or not at all. */
  int apply_changes() {
    if (!follow_ || !handle_) return UFM_OK;
    constexpr bool kInfo = !std::is_void<InfoType_>::value;
    if (dg_.empty()) { dg_.resize(1 << 16); dxy_.resize(2 << 16); if (kInfo) dinfo_.resize(2 << 16); }
    int total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      const int rc = ufm_read_changes(handle_, static_cast<int>(dg_.size()), dxy_.data(), dg_.data(), kInfo ? dinfo_.data() : nullptr, &total);
      if (rc != UFM_OK) return rc;
      if (static_cast<size_t>(total) <= dg_.size()) break;
      if (attempt) return UFM_ERR_INVALID;          // (cannot happen: nothing steps between the two calls)
      dg_.resize(total); dxy_.resize(2 * static_cast<size_t>(total)); if (kInfo) dinfo_.resize(2 * static_cast<size_t>(total));
    }
    for (int i = 0; i < total; ++i) {
      const size_t e = static_cast<size_t>(dxy_[2 * i]) * ny_ + dxy_[2 * i + 1];
      const bool had = host_g_[e] < INFINITY, has = dg_[i] < INFINITY;
      if (had && !has) --count_;
      else if (!had && has) ++count_;
      host_g_[e] = dg_[i];
      if (kInfo) { host_info_[2 * e] = dinfo_[2 * i]; host_info_[2 * e + 1] = dinfo_[2 * i + 1]; }
    }
    if (total) buckets_stale_ = true;
    return UFM_OK;
  }
  void invalidate() const { cache_.clear(); }
  void clear() noexcept { invalidate(); buckets.clear(); buckets_stale_ = true; }

 private:
  // linear element index -> Node / Cell (negative: "none", default-constructed like the reference's Node{} / Cell{})
  ElemType elem_of(int32_t idx) const { return idx >= 0 ? ElemType(idx / ny_, idx % ny_) : ElemType(); }
  template <typename U = InfoType_>
  typename std::conditional<std::is_void<U>::value, int, U>::type make_info(int32_t a, int32_t b) const {
    if constexpr (std::is_same<U, ElemType>::value) { (void)b; return elem_of(a); }
    else if constexpr (std::is_same<U, std::pair<ElemType, ElemType>>::value) return {elem_of(a), elem_of(b)};
    else { (void)a; (void)b; return 0; }
  }
  void empty_copy() {          // the reference's empty ExpandedMap
    host_g_.assign(static_cast<size_t>(nx_) * ny_, INFINITY);
    if (!std::is_void<InfoType_>::value) host_info_.assign(static_cast<size_t>(nx_) * ny_ * 2, -1);
    count_ = 0;
    buckets.clear();
    buckets_stale_ = true;
  }
  void buckets_from_copy() {   // same buckets, same order within a bucket, as size() builds from a read of the whole field
    if (!buckets_stale_) return;
    buckets.clear();
    const int bx = (nx_ >> 8) + 1, by = (ny_ >> 8) + 1;
    buckets.resize(static_cast<size_t>(bx) * by);
    for (int x = 0; x < nx_; ++x)
      for (int y = 0; y < ny_; ++y) {
        const size_t e = static_cast<size_t>(x) * ny_ + y;
        const float v = host_g_[e];
        if (!(v < INFINITY)) continue;
        auto &bucket = buckets[static_cast<size_t>(x >> 8) * by + (y >> 8)];
        if constexpr (std::is_void<InfoType_>::value) bucket.emplace_back(ElemType(x, y), value_(v, v));
        else bucket.emplace_back(ElemType(x, y), value_(v, v, make_info(host_info_[2 * e], host_info_[2 * e + 1])));
      }
    buckets_stale_ = false;
  }
  static constexpr int kBlock = 64;
  float value(int x, int y) const {
    if (!handle_ || x < 0 || y < 0 || x >= nx_ || y >= ny_) return INFINITY;
    if (follow_) return host_g_[static_cast<size_t>(x) * ny_ + y];
    const int bx = x / kBlock, by = y / kBlock;
    const uint64_t key = (static_cast<uint64_t>(bx) << 32) | static_cast<uint32_t>(by);
    auto it = cache_.find(key);
    if (it == cache_.end()) {
      const int x0 = bx * kBlock, y0 = by * kBlock;
      const int w = std::min(kBlock, nx_ - x0), h = std::min(kBlock, ny_ - y0);
      std::vector<float> blk(static_cast<size_t>(kBlock) * kBlock, INFINITY);
      std::vector<float> tmp(static_cast<size_t>(w) * h);
      if (ufm_read_field(handle_, x0, y0, w, h, tmp.data(), nullptr) == UFM_OK)
        for (int i = 0; i < w; ++i)
          for (int j = 0; j < h; ++j) blk[static_cast<size_t>(i) * kBlock + j] = tmp[static_cast<size_t>(i) * h + j];
      it = cache_.emplace(key, std::move(blk)).first;
    }
    return it->second[static_cast<size_t>(x - bx * kBlock) * kBlock + (y - by * kBlock)];
  }
  ufm_t *handle_ = nullptr;
  int nx_ = 0, ny_ = 0;
  mutable std::unordered_map<uint64_t, std::vector<float>> cache_;
  bool follow_ = false;
  std::vector<float> host_g_;          // following: the field as of the last delta, row-major [nx_][ny_]
  std::vector<int32_t> host_info_;     // ... and the Info pairs (ufm_read_info's format)
  size_t count_ = 0;                   // ... elements that hold a value
  bool buckets_stale_ = true;
  std::vector<int32_t> dxy_, dinfo_;   // record buffers of apply_changes
  std::vector<float> dg_;
};

#endif  // UFM_EXPANDED_MAP_H
