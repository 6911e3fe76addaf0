// Place recognition (include/loamx.h, loamx_place_*): scan-context descriptors of sweeps in HBM and the exhaustive search over them.
// An entry is R x S f32 cells (the maximum height per ring x sector cell, ring-major; 0 = empty) and R f32 ring-key words.  Heights are
// positive, so their bit patterns order like unsigned integers: the cells are built with integer atomicMax and do not depend on the
// order of the points.
// PlaceDB, the handle's class: declarations and members only.  Each member is defined in the file of its feature (place.hip; the views
// described from a dense map in place_views.hip); the C entry points of a feature are in the same file and reach it through h->d.
#pragma once
#include "common.h"
#include "cloud_stage.hpp"
#include "pinned_copy.hpp"
#include <vector>

namespace loamx {

constexpr int PL_MAX_RINGS = 64;
constexpr int PL_MAX_SECTORS = 128;
constexpr int PL_MAX_CANDIDATES = 256;                 // K of the ring-key pre-selection
constexpr uint32_t PL_CHUNK = 2048;                    // keys per workgroup of a selection pass
constexpr uint32_t PL_DESCRIBE_SPAN = 1024;            // points per workgroup of k_pl_describe (one flush of the LDS grid per span)
constexpr unsigned long long PL_NO_KEY = ~0ull;
constexpr uint32_t PL_FILE_MAGIC = 0x4c50584cu;        // 'LXPL'
constexpr uint32_t PL_FILE_VERSION = 1u;

// boundary directions of the sectors, (cos, sin)(2 pi k / S) evaluated in double and rounded once (host only)
inline void place_sector_table(int S, float* table) {
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int k = 0; k < S; k++) {
    const double t = two_pi * (double)k / (double)S;
    table[2 * k] = (float)cos(t);
    table[2 * k + 1] = (float)sin(t);
  }
}

// what a descriptor kernel needs: the origin (k_pl_describe; the kernels of place_views.hip take theirs from a table) and the
// database's constants
struct PlParams {
  float ox, oy, oz;
  float min2, max2, hoff, ring_scale;
  int R, S;
};

// The cell of the point (px, py, pz) described about (ox, oy, oz) (include/loamx.h: the use rule, the ring and the sector rule), and
// its height in h; -1 when the point is not used.  tab: the S boundary directions, in LDS.  Shared by k_pl_describe and the kernels
// of place_views.hip: one body, one order of the f32 operations
__device__ inline int pl_cell_of(const PlParams& P, const float2* tab, float px, float py, float pz, float ox, float oy, float oz, float& h) {
  if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return -1;
  const float a = pz - oz, b = px - ox;
  const float r2 = a * a + b * b;
  h = (py - oy) + P.hoff;
  if (!(r2 >= P.min2 && r2 < P.max2 && h > 0.f)) return -1;
  int ring = (int)(sqrtf(r2) * P.ring_scale);
  ring = ring < P.R - 1 ? ring : P.R - 1;
  // the sector rule itself, at every boundary (S <= 128 broadcast reads of LDS per point): the smallest k with cross(k) >= 0 > cross(k + 1)
  const float first = tab[0].x * b - tab[0].y * a;
  float c0 = first;
  int sec = -1;
  for (int k = 0; k < P.S; k++) {
    float c1 = first;
    if (k + 1 < P.S) { const float2 t = tab[k + 1]; c1 = t.x * b - t.y * a; }
    if (sec < 0 && c0 >= 0.f && c1 < 0.f) sec = k;
    c0 = c1;
  }
  return sec >= 0 ? ring * P.S + sec : -1;
}

class DenseMap;   // densemap_map.hpp

class PlaceDB {
 public:
  // ---- place.hip: the entries, adds from clouds, the search, files
  explicit PlaceDB(const loamx_place_config& c);
  ~PlaceDB();
  loamx_place_config cfg;
  const int R, S;
  const size_t RS;

  uint32_t size() const { return n_; }
  // a cloud from the host about a finite origin as a source on own_, up through the database's stager
  DenseSource host_source(const loamx_cloud* c, const float origin[3]);
  // enqueued on the source's stream, behind every add so far: own_ for a cloud from the host, the stream that wrote a registered cloud
  // (kept: a non-finite origin from the host is refused in host_source, before the database is found full; a source's only here, after)
  int add(const DenseSource& s, uint32_t* id);
  int query_entry(uint32_t id, loamx_place_match* out, uint32_t n_results, uint32_t* n_found);
  int query_cloud(const loamx_cloud* c, const float origin[3], uint32_t exclude_recent, loamx_place_match* out, uint32_t n_results,
                  uint32_t* n_found);
  void get_descriptor(uint32_t id, float* desc, float* key);
  void reset();
  void save(const char* path);
  void load(const char* path);
  uint64_t growths = 0;

  // ---- place_views.hip: include/loamx.h, loamx_place_add_views: n checked origins (and, in CAST mode, n_rays checked offsets) under a
  // checked configuration and a checked rule or none, described from the map on the map's own stream.  Blocks
  int add_views(DenseMap& dm, const float* origins, uint32_t n, const float* offsets, uint32_t n_rays, const loamx_place_view_config& c,
                const loamx_densemap_static_rule* rule, uint32_t* first_id, uint64_t stats[6]);

 private:
  hipStream_t own_ = nullptr;      // host-fed adds, queries, exports
  bool added_ = false;             // ev_last_ has been recorded: on own_, behind every add enqueued so far (add())
  hipEvent_t ev_last_ = nullptr, ev_done_ = nullptr;
  float* desc_ = nullptr;          // cap_ x R*S
  float* keys_ = nullptr;          // cap_ x R
  uint32_t cap_ = 0, n_ = 0;
  PlParams P_{};
  size_t lds_describe_ = 0, lds_distance_ = 0;
  DevBuf<float2> d_table_;
  DevBuf<float> q_desc_, q_key_, dist_, rkd_;
  DevBuf<uint32_t> shift_, cand_;
  DevBuf<unsigned long long> dkey_, part_;
  PinBuf<loamx_place_match> h_res_;
  DmCloudStage stage_;             // add()'s and query_cloud()'s clouds from the host
  std::vector<void*> graveyard_;   // arrays replaced by a growth: freed at the next point where the host waits anyway
  // views (place_views.hip): the origins and the offsets, four floats each, on their way up and on the device; the qualifying voxels
  // of VOXELS mode; the five ray counts and the voxel cursor.  Allocated by the first add_views, grow to the largest call
  PinBuf<float4> h_view_in_;
  DevBuf<float4> d_view_in_, d_view_vox_;
  DevBuf<unsigned long long> view_ctr_;
  PinLanding<unsigned long long> h_view_ctr_;

  static void check_origin(const float o[3]) {
    LX_REQUIRE(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]), "origin must be finite");
  }
  void alloc_entries(uint32_t cap, float*& d, float*& k);
  void free_graveyard();
  bool full() const { return cfg.max_entries && n_ + 1u > cfg.max_entries; }
  // room for `want` entries (a power of two above cap_): a device-to-device copy of the n_ entries on st, the old arrays freed later
  void grow_to(uint32_t want, hipStream_t st);
  // the adds enqueued on st are the last: the order is handed on to own_ at once (see add())
  void hand_on(hipStream_t st);
  // st runs behind every add enqueued so far (on whichever stream)
  void order_behind(hipStream_t st) {
    if (added_ && st != own_) LX_HIP(hipStreamWaitEvent(st, ev_last_, 0));
  }
  void wait_adds();
  void describe(const float4* pts, uint32_t n, const float origin[3], float* cells, float* key, hipStream_t st);
  // on own_, which the caller has ordered behind every add
  int search(const float* Q, const float* rq, uint32_t q, uint32_t exclude_recent, loamx_place_match* out, uint32_t n_results, uint32_t* n_found);
};

}  // namespace loamx

struct loamx_place {
  loamx::PlaceDB d;
  explicit loamx_place(const loamx_place_config& c) : d(c) {}
};
