// The dense map's regions and tiles on the host (include/loamx.h: loamx_densemap_region_* / tile_* / file_merge / page): the window
// arithmetic, the tile of a voxel, the names of the tile files, the buckets of a page-out and the merge of two sets of records.  No HIP
// in here: densemap_region.hip includes it, and tests/densemap_tiles_driver.cpp drives it on a CPU under the sanitizers.  Built on
// densemap_file.hpp: a tile file is an 'LXDM' file like any other, and the merge is the one loamx_densemap_merge defines — words added
// per key modulo 2^64 (miss: 2^32), header statistics summed.  Every function answers with a message, empty when all is well, that
// names the offending field.
#pragma once
#include "densemap_file.hpp"

#include <algorithm>
#include <array>
#include <cerrno>
#include <cstdlib>
#include <map>

namespace loamx {

constexpr int32_t DMT_IMAX = (1 << 20) - 1;        // a voxel index lies in [-DMT_IMAX, DMT_IMAX]
constexpr uint32_t DMT_MAX_TILE = 1u << 20;        // tile_voxels lies in [1, DMT_MAX_TILE]
constexpr uint32_t DMT_INSIDE = 0u, DMT_OUTSIDE = 1u;

// the layout of loamx_densemap_region (include/loamx.h)
struct DmRegion {
  int32_t lo[3], hi[3];
  uint32_t side, reserved;
};

inline int64_t dmt_clamp(int64_t v) { return v < -(int64_t)DMT_IMAX ? -(int64_t)DMT_IMAX : (v > (int64_t)DMT_IMAX ? (int64_t)DMT_IMAX : v); }
inline int64_t dmt_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a < 0)) ? 1 : 0); }   // (b > 0)

inline void dmt_region_default(DmRegion& r) {
  for (int a = 0; a < 3; a++) { r.lo[a] = -DMT_IMAX; r.hi[a] = DMT_IMAX; }
  r.side = DMT_INSIDE;
  r.reserved = 0u;
}

inline std::string dmt_region_check(const DmRegion& r) {
  static const char* ax[3] = {"0", "1", "2"};
  for (int a = 0; a < 3; a++) {
    if (r.lo[a] < -DMT_IMAX || r.lo[a] > DMT_IMAX) return std::string("lo[") + ax[a] + "]: outside +-(2^20 - 1)";
    if (r.hi[a] < -DMT_IMAX || r.hi[a] > DMT_IMAX) return std::string("hi[") + ax[a] + "]: outside +-(2^20 - 1)";
    if (r.lo[a] > r.hi[a]) return std::string("lo[") + ax[a] + "] > hi[" + ax[a] + "]";
  }
  if (r.side > 1u) return "side: must be 0 (inside) or 1 (outside)";
  if (r.reserved != 0u) return "reserved: must be 0";
  return "";
}

// floor(v / leaf) in double, clamped to the index range (v and leaf finite, leaf > 0)
inline int32_t dmt_index_of(double v, double leaf) {
  const double q = std::floor(v / leaf);
  return (int32_t)(q < -(double)DMT_IMAX ? -(double)DMT_IMAX : (q > (double)DMT_IMAX ? (double)DMT_IMAX : q));
}

inline std::string dmt_region_about(float leaf, const float centre[3], const float half[3], DmRegion& r) {
  if (!(leaf > 0.f) || !std::isfinite(leaf)) return "leaf: must be finite and > 0";
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(centre[a])) return "centre: must be finite";
    if (!(half[a] >= 0.f) || !std::isfinite(half[a])) return "half: must be finite and >= 0";
  }
  for (int a = 0; a < 3; a++) {
    r.lo[a] = dmt_index_of((double)centre[a] - (double)half[a], (double)leaf);
    r.hi[a] = dmt_index_of((double)centre[a] + (double)half[a], (double)leaf);
  }
  r.side = DMT_INSIDE;
  r.reserved = 0u;
  return "";
}

inline std::string dmt_check_tile_voxels(uint32_t T) {
  return (T >= 1u && T <= DMT_MAX_TILE) ? "" : "tile_voxels: must be in [1, 2^20]";
}

inline std::string dmt_tile_of(const int32_t idx[3], uint32_t T, int32_t tile[3]) {
  const std::string e = dmt_check_tile_voxels(T);
  if (!e.empty()) return e;
  for (int a = 0; a < 3; a++) tile[a] = (int32_t)dmt_floor_div((int64_t)idx[a], (int64_t)T);
  return "";
}

// the voxels of a tile as a window; a tile that holds no index of the key range is refused
inline std::string dmt_tile_region(const int32_t tile[3], uint32_t T, DmRegion& r) {
  const std::string e = dmt_check_tile_voxels(T);
  if (!e.empty()) return e;
  for (int a = 0; a < 3; a++) {
    const int64_t lo = (int64_t)tile[a] * (int64_t)T, hi = lo + (int64_t)T - 1;
    if (lo > (int64_t)DMT_IMAX || hi < -(int64_t)DMT_IMAX) return "tile: outside the key range";
    r.lo[a] = (int32_t)dmt_clamp(lo);
    r.hi[a] = (int32_t)dmt_clamp(hi);
  }
  r.side = DMT_INSIDE;
  r.reserved = 0u;
  return "";
}

inline std::string dmt_tile_name(const int32_t tile[3]) {
  return "tile_" + std::to_string(tile[0]) + "_" + std::to_string(tile[1]) + "_" + std::to_string(tile[2]) + ".lxdm";
}

// the inverse of dmt_tile_name: true when `name` is exactly the name of `tile`
inline bool dmt_parse_tile_name(const std::string& name, int32_t tile[3]) {
  if (name.compare(0, 5, "tile_") != 0) return false;
  const char* p = name.c_str() + 5;
  for (int a = 0; a < 3; a++) {
    char* end = nullptr;
    errno = 0;
    const long long v = strtoll(p, &end, 10);
    if (end == p || errno || v < -(1ll << 31) || v >= (1ll << 31)) return false;
    tile[a] = (int32_t)v;
    if (a < 2) {
      if (*end != '_') return false;
      p = end + 1;
    } else {
      p = end;
    }
  }
  return std::string(p) == ".lxdm" && dmt_tile_name(tile) == name;
}

// the voxel indices of a key (densemap.hpp, dm_key)
inline void dmt_key_indices(uint64_t k, int32_t ia[3]) {
  for (int a = 0; a < 3; a++) ia[a] = (int32_t)((k >> (21 * a)) & ((1ull << 21) - 1ull)) - (1 << 20);
}

// the header of a file of records taken out of a map (include/loamx.h, loamx_densemap_save_region): `like` gives flags, leaf and the
// carving configuration; offered is the sum of n; the drop counts and the carve statistics are 0
inline DmFileHeader dmt_region_header(const DmFileHeader& like, const std::vector<uint64_t>& keys, const std::vector<uint64_t>& vals) {
  DmFileHeader h;
  h.flags = like.flags;
  h.leaf = like.leaf;
  h.count = keys.size();
  for (size_t i = 0; i < keys.size(); i++) h.offered += vals[4 * i];
  if (like.flags & DMF_CARVING) {
    h.carve_max_range = like.carve_max_range;
    h.ray_stride = like.ray_stride; h.end_margin = like.end_margin; h.max_steps = like.max_steps;
  }
  return h;
}

inline std::string dmt_write(const char* path, const DmFile& f) {
  return dmf_write(path, f.h, f.keys.data(), f.vals.data(), (f.h.flags & DMF_CARVING) ? f.miss.data() : nullptr,
                   (f.h.flags & DMF_MOMENTS) ? f.mom.data() : nullptr);
}

// out = a + b as loamx_densemap_merge adds (both validated: ascending keys); leaf, flags and the carving configuration are a's.
// Refused: a differing bit of the leaf, differing flags, more than 2^30 voxels
inline std::string dmt_merge(const DmFile& a, const DmFile& b, DmFile& out) {
  if (memcmp(&a.h.leaf, &b.h.leaf, sizeof(float)) != 0) return "leaf: the two files differ";
  if (a.h.flags != b.h.flags) return "flags: the two files differ";
  const bool aux = (a.h.flags & DMF_CARVING) != 0, mom = (a.h.flags & DMF_MOMENTS) != 0;
  const size_t na = a.keys.size(), nb = b.keys.size();
  out.h = a.h;
  out.h.offered += b.h.offered; out.h.dropped_range += b.h.dropped_range; out.h.dropped_key += b.h.dropped_key;
  for (int k = 0; k < 6; k++) out.h.carve_stats[k] += b.h.carve_stats[k];
  out.keys.clear(); out.vals.clear(); out.miss.clear(); out.mom.clear();
  out.keys.reserve(na + nb);
  out.vals.reserve(4 * (na + nb));
  size_t i = 0, j = 0;
  while (i < na || j < nb) {
    const bool ta = i < na && (j >= nb || a.keys[i] <= b.keys[j]), tb = j < nb && (i >= na || b.keys[j] <= a.keys[i]);
    out.keys.push_back(ta ? a.keys[i] : b.keys[j]);
    for (int w = 0; w < 4; w++) out.vals.push_back((ta ? a.vals[4 * i + w] : 0ull) + (tb ? b.vals[4 * j + w] : 0ull));
    if (aux) out.miss.push_back((ta ? a.miss[i] : 0u) + (tb ? b.miss[j] : 0u));
    if (mom)
      for (int w = 0; w < DMF_MOM_WORDS; w++)
        out.mom.push_back((ta ? a.mom[DMF_MOM_WORDS * i + w] : 0ull) + (tb ? b.mom[DMF_MOM_WORDS * j + w] : 0ull));
    i += ta ? 1 : 0;
    j += tb ? 1 : 0;
  }
  out.h.count = out.keys.size();
  if (out.h.count > DMF_MAX_COUNT) return "count: more than 2^30 voxels";
  return "";
}

// include/loamx.h, loamx_densemap_file_merge: both files read with the deep check, merged, written under a temporary name and renamed
inline std::string dmt_file_merge(const char* path_a, const char* path_b, const char* path_out) {
  DmFile a, b, out;
  std::string e = dmf_read(path_a, true, a);
  if (!e.empty()) return std::string(path_a) + ": " + e;
  e = dmf_read(path_b, true, b);
  if (!e.empty()) return std::string(path_b) + ": " + e;
  e = dmt_merge(a, b, out);
  if (!e.empty()) return e;
  return dmt_write(path_out, out);
}

struct DmTileLess {
  bool operator()(const std::array<int32_t, 3>& x, const std::array<int32_t, 3>& y) const {
    return x[2] != y[2] ? x[2] < y[2] : (x[1] != y[1] ? x[1] < y[1] : x[0] < y[0]);
  }
};
typedef std::map<std::array<int32_t, 3>, DmFile, DmTileLess> DmTileBuckets;

// the records of src (ascending keys) by the tile of their voxel, each bucket in ascending key order under the header rule of
// dmt_region_header
inline std::string dmt_bucket(const DmFile& src, uint32_t T, DmTileBuckets& out) {
  const std::string e = dmt_check_tile_voxels(T);
  if (!e.empty()) return e;
  const bool aux = (src.h.flags & DMF_CARVING) != 0, mom = (src.h.flags & DMF_MOMENTS) != 0;
  out.clear();
  for (size_t i = 0; i < src.keys.size(); i++) {
    int32_t ia[3], t[3];
    dmt_key_indices(src.keys[i], ia);
    (void)dmt_tile_of(ia, T, t);
    DmFile& f = out[{t[0], t[1], t[2]}];
    f.keys.push_back(src.keys[i]);
    f.vals.insert(f.vals.end(), &src.vals[4 * i], &src.vals[4 * i] + 4);
    if (aux) f.miss.push_back(src.miss[i]);
    if (mom) f.mom.insert(f.mom.end(), &src.mom[DMF_MOM_WORDS * i], &src.mom[DMF_MOM_WORDS * i] + DMF_MOM_WORDS);
  }
  for (auto& kv : out) kv.second.h = dmt_region_header(src.h, kv.second.keys, kv.second.vals);
  return "";
}

}  // namespace loamx
