// The dense map's handle (include/loamx.h, loamx_densemap): DenseMap, declarations and members only.  Each member is defined in the
// file of its feature, named beside it; the C entry points of a feature are in the same file and reach the map through h->d.
#pragma once
#include "densemap.hpp"
#include "densemap_history.hpp"
#include "densemap_route_core.hpp"
#include <functional>
#include <type_traits>

namespace loamx {

struct DmFilter;   // densemap_dev.hpp
struct DmCarve;
struct DmCtrAdd;   // densemap_merge.hip
struct DmWindow;
struct DmFileHeader;   // densemap_file.hpp
struct DmSurfelList;   // densemap_freeze.hip

// two runtime booleans as the two std::bool_constant arguments of f: the kernels' feature switches are template parameters
template <class F> static void dm_dispatch2(bool a, bool b, F&& f) {
  if (a) { if (b) f(std::true_type(), std::true_type()); else f(std::true_type(), std::false_type()); }
  else { if (b) f(std::false_type(), std::true_type()); else f(std::false_type(), std::false_type()); }
}

class DenseMap {
 public:
  // ---- densemap.hip: the table, its counters, adds, growth and admission
  explicit DenseMap(const loamx_densemap_config& c);
  ~DenseMap();
  loamx_densemap_config cfg;
  // a checked cloud from the host about origin (NULL: zeros) as a source on own_, up through `via`, a stager of this handle
  DenseSource host_source(DmCloudStage& via, const loamx_cloud* c, const float origin[3]);
  DmCloudStage stage;   // the staging block of the adds; the ray casts' ends go up through it too
  int add(const DenseSource& s);
  // [voxels, slots, offered, added, dropped by range, dropped by key]
  void stats(uint64_t out[6]);
  // the occupied slots on the host: keys, values, (carving) miss words and (on request, moments) the nine moment words, and idx =
  // their ascending key order
  struct Snapshot {
    std::vector<unsigned long long> k, v, mom;
    std::vector<uint32_t> miss, idx;
  };
  void snapshot(Snapshot& S, bool want_mom = false);
  // the same download for any table of the map's format that holds `occ` voxels and that nothing enqueued on another stream still
  // writes (the map's own behind read_counters; a coarse level of densemap_pyramid.hip behind its cascade)
  void snapshot_of(const DmTable& T, uint64_t occ, Snapshot& S, bool want_mom);
  // the voxels of a snapshot in ascending key order, without those a rule (NULL: none) calls dynamic: f(j, ia) with j the voxel's
  // place in S.k (4 * j in S.v, 9 * j in S.mom) and ia its indices
  template <class F> static void for_each_voxel(const Snapshot& S, const loamx_densemap_static_rule* rule, F&& f) {
    for (size_t r = 0; r < S.idx.size(); r++) {
      const size_t j = S.idx[r];
      if (rule && dm_dynamic(*rule, S.v[4 * j], S.miss[j])) continue;
      long long ia[3];
      dm_key_indices(S.k[j], ia);
      f(j, ia);
    }
  }
  bool moments() const { return tab_.mom != nullptr; }
  bool carving() const { return tab_.aux != nullptr; }
  // both: allowed while nothing has been offered since creation / reset; the handle is unchanged when refused
  void enable_moments();
  void enable_carving(const loamx_densemap_carve_config& c);
  // [rays traced, not traced by stride, by range, by steps or origin key, cells visited, misses recorded]
  void carve_stats(uint64_t out[6]);
  // the dynamic voxels leave the table: a rehash with the rule as predicate into a fresh table of the same size
  uint64_t prune(const loamx_densemap_static_rule& rule);
  void reset();
  hipStream_t own_stream() const { return own_; }
  bool combine = true;   // (bench A/B: the in-wave combining of equal keys)
  uint64_t rehashes = 0;

  // ---- densemap_export.hip: the voxels on the host.  records: axes 0: LOAM frame, 1: sensor axes, ascending key order; with a rule,
  // without the voxels it calls dynamic.  misses, moment_words, surfels: in the order of records()
  // (W: only the voxels the window selects)
  void records(std::vector<float4>& out, int axes, const loamx_densemap_static_rule* rule = nullptr, const DmWindow* W = nullptr);
  void misses(std::vector<uint32_t>& out);
  void moment_words(std::vector<unsigned long long>& out);
  void surfels(std::vector<loamx_surfel>& out, int axes, const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule);
  // the snapshot the alignment reads (densemap_align.hip): the voxels that have a surfel and that the rule does not call dynamic, each
  // under its key of the table, with the six f32 of its record as surfels() gives them in axes 0.  Replaces an earlier snapshot
  uint64_t freeze(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule);
  DmFrozen frozen;

  // ---- densemap_pyramid.hip: coarser levels of the map and of the snapshot (include/loamx.h, loamx_densemap_coarsen ...
  // loamx_densemap_align_pyramid).  `frozen` is level 0; coarse[l - 1] is level l, a snapshot of the same format whose leaf is
  // level_leaf(l).  freeze, reset and destroy drop the coarse levels; align_level is the level every alignment form reads
  static constexpr uint32_t COARSE_LEVELS = LOAMX_PYRAMID_MAX_LEVELS - 1;
  DmFrozen coarse[COARSE_LEVELS];
  uint32_t align_level = 0;
  // the voxels of level `level` in 1..COARSE_LEVELS on the host (S.k, S.v, S.mom, S.idx); needs moments; a checked rule or none
  void coarsen(uint32_t level, const loamx_densemap_static_rule* rule, Snapshot& S);
  void freeze_pyramid(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule,
                      const loamx_densemap_pyramid_config& pc, uint64_t* n_surfels);
  void drop_coarse();   // the coarse levels go and the selection returns to level 0
  uint32_t frozen_levels() const;
  DmFrozen& level(uint32_t l) { return l ? coarse[l - 1] : frozen; }
  float level_leaf(uint32_t l) const { return cfg.leaf * (float)(1u << l); }   // (one f32 multiply by a power of two)

  // ---- densemap_freeze.hip: snapshots whose surfels are computed on the device (include/loamx.h, loamx_densemap_freeze_device ...).
  // freeze_device / freeze_pyramid_device: the entries of freeze / freeze_pyramid, from the tables where they lie.  freeze_history:
  // level 0 from the window [first_call, first_call + n_calls) of the log, call k of the window under corrections[12 * k ..] (NULL:
  // identities); the map is only read.  history_source: the points of a logged call where they lie, every add waited for
  uint64_t freeze_device(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule);
  void freeze_pyramid_device(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule,
                             const loamx_densemap_pyramid_config& pc, uint64_t* n_surfels);
  int freeze_history(uint64_t first_call, uint64_t n_calls, const double* corrections, const loamx_densemap_surfel_config& sc,
                     uint64_t* n_surfels);
  void history_source(uint64_t call, DenseSource& s);

  // ---- densemap_merge.hip: include/loamx.h, loamx_densemap_save / merge / merge_file and, with `loading`, load
  uint32_t flags() const;   // the features of the handle as the file's flags
  void save(const char* path);
  int merge(DenseMap& src);
  int merge_file(const char* path, bool loading);

  // ---- densemap_region.hip: include/loamx.h, loamx_densemap_count_region ... page.  A checked window each
  // the compaction behind snapshot_of and select: the occupied slots of T (W: of those, the ones the window selects) in slot order
  // on own_ (the block counts scanned through scan_), brought to the host and ordered by key.  Without W, occ is T's count and one wait serves; with W the block counts are
  // scanned and the total and the sum of n waited for first (counts, when given: voxels, points), and only the selected records
  // cross.  S NULL (with W): the counts alone
  void compact_of(const DmTable& T, const DmWindow* W, uint64_t occ, Snapshot* S, bool want_mom, uint64_t counts[2]);
  // waits for the adds; the voxels the window selects as a snapshot (S NULL: only counted)
  void select(const DmWindow& W, Snapshot* S, bool want_mom, uint64_t counts[2]);
  void save_region(const DmWindow& W, const char* path);
  // the selected voxels leave the table (path: into a file first; NULL: discarded); removed: voxels, points
  void evict(const DmWindow& W, const char* path, uint64_t removed[2]);
  int page(const char* dir, uint32_t tile_voxels, const uint32_t radius[3], const float centre[3], uint64_t stats[6]);

  // ---- densemap_raycast.hip: include/loamx.h, loamx_densemap_raycast and its from_* forms: the rays from s.origin to the points of s
  int raycast(const DenseSource& s, const loamx_densemap_raycast_config& c, const loamx_densemap_static_rule* rule, loamx_ray_hit* out,
              uint64_t capacity, uint64_t counts[5]);

  // ---- place_views.hip: what a reader of the table outside the map is handed, as DmCaster::enqueue is: the table, the counters (a
  // probe overflow goes to word 3), inv, the leaf, the voxel count and the map's own stream, every add waited for and the counters
  // read (read_counters).  Read-only: valid until the next call that changes the map
  struct TableView {
    const DmTable* tab;
    unsigned long long* ctr;
    float inv;
    double leaf;
    uint64_t voxels;
    hipStream_t stream;
  };
  TableView table_view();

  // ---- densemap_rebuild.hip: the sweep log and its replay (include/loamx.h, loamx_densemap_enable_history ... rebuild)
  void enable_history(const loamx_densemap_history_config& c);
  bool history() const { return history_; }
  void history_size(uint64_t* calls, uint64_t* points) const { *calls = hist_.calls.size(); *points = hist_.points; }
  int history_download(uint64_t call, loamx_cloud* out, float origin[3]);
  int rebuild(const double* corrections, uint64_t n_calls);
  void rebuild_stats(uint64_t out[4]) const { for (int k = 0; k < 4; k++) out[k] = rebuild_stats_[k]; }

  // ---- densemap_grid.hip, densemap_route.hip, densemap_segment.hip: checked configurations, a checked rule or none; the table is
  // only read, and the outputs are written last, all or none
  void grid(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, loamx_grid_cell* out);
  void route(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
             const uint32_t* goals_xz, uint32_t n_goals, loamx_grid_cell* out_cells, loamx_route_cell* out_field, uint64_t stats[6]);
  void route_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc, const uint32_t* goals_xz,
                   uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]);
  DmRoute& router() { return route_; }
  // what the 2-D and the 3-D route calls share, r being route_ or route3_.  route_on: r.run on own_, then `between` (what else
  // has to succeed before anything is written), then the field and the stats out, each where wanted
  template <class K, class Between = void (*)()>
  void route_on(DmRouteT<K>& r, const typename K::Cell* d_in, uint32_t nx, uint32_t ny, uint32_t nz, const typename K::Config& rc,
                const uint32_t* goals, uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6], Between between = [] {}) {
    uint64_t s[6];
    const loamx_route_cell* field = r.run(d_in, nx, ny, nz, rc, goals, n_goals, out_field != nullptr, s, own_);
    between();
    if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * nx * ny * nz);
    if (stats) memcpy(stats, s, sizeof(s));
  }
  // include/loamx.h, loamx_densemap_route_trace and loamx_densemap_route3_trace: checked starts over the field that stands in r
  template <class K> void route_trace_on(DmRouteT<K>& r, const uint32_t* starts, uint32_t n_starts, uint32_t* out, uint32_t capacity,
                                         uint32_t* lengths) {
    LX_REQUIRE(r.has_field(), std::string("the handle has no field yet (") + K::FIELD_FROM + ")");
    LX_HIP(hipSetDevice(cfg.device));
    r.trace(starts, n_starts, out, capacity, lengths, own_);
  }
  // ---- densemap_frontier.hip: include/loamx.h, loamx_densemap_frontiers and loamx_densemap_frontiers_cells; checked configurations.
  // LOAMX_E_CAPACITY: only *n_frontiers is written
  int frontiers(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
                const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out, uint64_t capacity,
                uint64_t* n_frontiers, uint64_t stats[6]);
  int frontiers_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc,
                      const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out,
                      uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]);
  // ---- densemap_dist.hip: include/loamx.h, loamx_densemap_dist and loamx_densemap_dist_query; a checked configuration, a checked
  // rule or none.  The field stays in dist_ until the next dist, reset or destroy
  void dist(const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, uint16_t* out_d2, uint32_t* out_near,
            uint64_t stats[4]);
  int dist_query(const loamx_cloud* points, uint32_t min_d2, loamx_dist_sample* out, uint64_t capacity, uint64_t stats[5]);
  bool has_dist() const { return dist_.has_field(); }
  const loamx_densemap_dist_config& dist_config() const { return dist_.config(); }   // of the field that stands
  // ---- densemap_route3.hip: include/loamx.h, loamx_densemap_route3 ...; checked configurations, a checked rule or none.  route3
  // replaces the distance field in dist_ as dist() does and routes on it; route3_last routes on the one that stands (the caller has
  // seen to it that there is one of at most 2^22 cells); route3_cells leaves dist_ alone.  The field stays in route3_ until the
  // next of the three, reset or destroy; the outputs are written last, all or none
  void route3(const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, const loamx_route3_config& rc,
              const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]);
  void route3_last(const loamx_route3_config& rc, const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field,
                   uint64_t stats[6]);
  void route3_cells(const uint16_t* d2, uint32_t nx, uint32_t ny, uint32_t nz, const loamx_route3_config& rc, const uint32_t* goals_xyz,
                    uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]);
  DmRoute3& router3() { return route3_; }
  // ---- densemap_mesh.hip: include/loamx.h, loamx_densemap_tsdf_* and loamx_densemap_mesh; checked configurations.  The field
  // stays in tsdf_ until the next tsdf_begin, reset or destroy; everything runs on own_
  void tsdf_begin(const loamx_densemap_tsdf_config& c);
  int tsdf_add(const DenseSource& s);
  int tsdf_add_history(uint64_t first_call, uint64_t n_calls, const double* corrections);
  void tsdf_download(uint32_t* out_w, int64_t* out_d, uint64_t stats[8]);
  int mesh(const loamx_densemap_mesh_config& c, float* verts, uint64_t cap_v, uint32_t* tris, uint64_t cap_t, uint64_t* n_verts,
           uint64_t* n_tris, uint64_t stats[6]);
  DmCloudStage& tsdf_stage() { return tsdf_.cloud; }
  int segment(const loamx_densemap_segment_config& c, const loamx_densemap_static_rule& rule, uint32_t* labels, uint64_t label_capacity,
              uint64_t* n_voxels, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[6]);
  // ---- densemap_segment_cloud.hip: include/loamx.h, loamx_densemap_segment_cloud and its from_* forms: the objects of the cloud of
  // s (a host cloud comes up through cloud_stage()); a checked configuration, a checked rule or none
  int segment_cloud(const DenseSource& s, const loamx_densemap_segment_cloud_config& c, const loamx_densemap_static_rule* rule,
                    uint32_t* labels, uint64_t label_capacity, uint64_t* n_points, loamx_segment* segs, uint64_t seg_capacity,
                    uint64_t* n_segs, uint64_t stats[13]);
  DmCloudStage& cloud_stage() { return cseg_.cloud; }

 private:
  // the table and its counters
  DmTable tab_;   // (aux NULL: carving is off; mom NULL: moments are off)
  float inv_ = 10.f;
  DevBuf<unsigned long long> ctr_;
  PinLanding<unsigned long long> h_ctr_, h_snap_;
  DmScan scan_;       // the one scan state of the handle: compact_of, seg_ and fr_ scan through it, each on own_
  DmOccupancy occ_;   // the bound of the occupancy that growth and admission are decided on (densemap_growth.hpp)
  uint64_t offered_ = 0, drop_range_ = 0, drop_key_ = 0;
  std::vector<void*> graveyard_;   // tables replaced by a rehash: freed at the next point where the host waits anyway
  // adds
  hipStream_t own_ = nullptr;      // host-fed adds, rehash of those, exports
  hipStream_t last_st_ = nullptr;  // the stream of the last enqueued add (ev_last_ recorded behind it)
  hipEvent_t ev_last_ = nullptr, ev_snap_ = nullptr;
  // carving
  loamx_densemap_carve_config carve_ = {0.f, 1u, 1u, 4096u};
  uint32_t seq_ = 0;          // sequence number of the last add call (stamp values; 0 = never stamped)
  uint64_t carve_ctr_[6] = {0, 0, 0, 0, 0, 0};
  // the sweep log (densemap_history.hpp): off unless enabled; hist_ then admits everything and log_ stays NULL
  bool history_ = false;
  DmHistory hist_;
  float4* log_ = nullptr;
  PinBuf<DmReplayCall> h_calls_;
  DevBuf<DmReplayCall> d_calls_;
  PinLanding<unsigned long long> h_rb_;
  PinLanding<float4> h_sweep_;   // history_download's landing
  uint64_t rebuild_stats_[4] = {0, 0, 0, 0};
  // the features that only read the table, each with its own buffers, allocated by its first call
  DmCaster caster_;   // densemap_raycast.hip
  DmGrid grid_;       // densemap_grid.hip
  DmDist dist_;       // densemap_dist.hip
  DmTsdf tsdf_;       // densemap_mesh.hip
  DmRoute route_;     // densemap_route.hip
  DmRoute3 route3_;   // densemap_route3.hip (routes on dist_'s d2 plane, or on an upload of its own)
  DmFrontier fr_;     // densemap_frontier.hip (routes towards the start through route_)
  DmSegment seg_;     // densemap_segment.hip
  DmSegCloud cseg_;   // densemap_segment_cloud.hip (labels its scratch table through seg_)

  // ---- densemap.hip
  DmFilter filter_for(const float origin[3]) const;   // the insert's filter about an origin
  DmCarve carve_args(uint32_t seq) const;             // the ray kernel's arguments for the call with that stamp
  void replace_table(DmTable& nt);   // nt becomes the map's table; the one it replaces goes to the graveyard
  template <int DROP> void launch_rehash(hipStream_t st, const DmTable& nt, const loamx_densemap_static_rule& rule, const DmWindow& W);
  template <bool STAMP> void launch_insert(hipStream_t st, const float4* pts, uint32_t n, const DmFilter& F, uint32_t seq);
  void clear(hipStream_t st);        // the table and the counters (the one place that zeroes both)
  void free_graveyard();
  void order_behind(hipStream_t st);   // st runs behind every add enqueued so far (on whichever stream)
  void wait_adds();
  void read_counters();   // exact counters, after every add
  void poll_snapshot();   // the occupancy snapshot that has landed, if any
  bool admit(uint32_t n);
  void grow_for(uint64_t n, hipStream_t st);
  void enqueue_add(const float4* pts, uint32_t n, const float origin[3], hipStream_t st);
  // ---- densemap_merge.hip
  void merge_records(const unsigned long long* skeys, const unsigned long long* svals, uint32_t sn, uint64_t s_occ, const uint32_t* smiss,
                     uint32_t miss_stride, const unsigned long long* smom, const DmCtrAdd& add, uint64_t s_offered);
  // ---- densemap_region.hip
  void region_header(DmFileHeader& H) const;   // flags, leaf and the carving configuration of the handle; every statistic 0
  // ---- densemap_frontier.hip: the tail of the two forms, behind a wait_adds(): the nx * nz records d_cells written by work on own_
  int frontiers_on(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc,
                   const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out, uint64_t capacity,
                   uint64_t* n_frontiers, uint64_t stats[6]);
  // ---- densemap_pyramid.hip: the levels 1 .. top, each from the one below (level 1 from the map's table, which is only read, without
  // the voxels the rule calls dynamic); out[l - first] = the voxels of level l for l = first .. top.  Waits for the adds; blocks
  void cascade(uint32_t top, const loamx_densemap_static_rule* rule, uint32_t first, std::vector<Snapshot>& out);
  // the same cascade with each level handed to f where it stands on the device: f(l, the level's table, its voxels) for l = 1 .. top,
  // everything that wrote the table waited for; the table goes when the level above it has been built
  void cascade_each(uint32_t top, const loamx_densemap_static_rule* rule, const std::function<void(uint32_t, const DmTable&, uint64_t)>& f);
  // ---- densemap_freeze.hip
  void surfel_list(const DmTable& T, uint64_t occ, double leaf, const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule,
                   float max_curvature, DmSurfelList& L);
  // ---- densemap_rebuild.hip
  void log_reserve(uint64_t n, hipStream_t st);
  void launch_replay(const DmTable& nt, unsigned long long* nctr);
  void launch_replay_range(const DmTable& nt, unsigned long long* nctr, const DmReplayCall* d_calls, uint32_t n_calls, uint64_t first,
                           uint64_t points);
};

}  // namespace loamx

struct loamx_densemap {
  loamx::DenseMap d;
  explicit loamx_densemap(const loamx_densemap_config& c) : d(c) {}
};

namespace loamx {

// ---- what the C entry points of more than one file share

// *cfg, or what its default function fills in
template <class C> C or_default(const C* cfg, void (*default_fn)(C*)) {
  C c;
  if (cfg) c = *cfg; else default_fn(&c);
  return c;
}
// the rule of a call, checked (NULL: the default rule)
inline loamx_densemap_static_rule checked_rule(const loamx_densemap_static_rule* rule) {
  const loamx_densemap_static_rule r = or_default(rule, loamx_densemap_static_rule_default);
  LX_REQUIRE(r.den != 0u, "the rule's den must not be 0");
  return r;
}
#define LX_REQUIRE_CARVING(h) LX_REQUIRE((h)->d.carving(), "carving is not enabled")
// the optional rule of a ray cast, a grid or a route, checked where it lies: NULL is every voxel; a rule needs carving.  (The exports'
// helper of this name with a third argument, densemap_export.hip, hands a checked copy on and has a message of its own)
inline void checked_optional_rule(loamx_densemap* h, const loamx_densemap_static_rule* rule) {
  if (!rule) return;
  LX_REQUIRE(rule->den != 0u, "the rule's den must not be 0");
  LX_REQUIRE(h->d.carving(), "a rule needs carving, which is not enabled");
}
// densemap_route.hip and densemap_route3.hip: the bodies of loamx_densemap_route_trace / loamx_densemap_route3_trace and of the
// bench / test hooks loamx_densemap_route_set_batch / loamx_densemap_route3_set_batch (rounds per look, 1..64); `router` is
// &DenseMap::router or &DenseMap::router3
template <class K, class R>
int dm_route_trace_entry(loamx_densemap* h, R& (DenseMap::*router)(), const uint32_t* starts, uint32_t n_starts, uint32_t* out,
                         uint32_t capacity, uint32_t* lengths) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    dm_route_check_tuples<K>(starts, n_starts, "starts");
    LX_REQUIRE(out || !capacity, std::string("out_") + K::AXES + " is NULL");
    LX_REQUIRE(lengths, "lengths is NULL");
    h->d.route_trace_on<K>((h->d.*router)(), starts, n_starts, out, capacity, lengths);
    return LOAMX_OK;
  });
}
template <class R> int dm_route_set_batch_entry(loamx_densemap* h, R& (DenseMap::*router)(), uint32_t batch) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(batch >= 1u && batch <= 64u, "batch must be in [1, 64]");
    (h->d.*router)().batch = batch;
    return LOAMX_OK;
  });
}
// densemap_export.hip, shared with densemap_pyramid.hip: the surfel of a voxel from its words (include/loamx.h), the surfel settings
// of a call, checked (NULL: the defaults), and the optional rule of a surfel call (NULL stays NULL: every voxel; a rule is checked
// into `r` and needs carving)
#define LX_REQUIRE_MOMENTS(h) LX_REQUIRE((h)->d.moments(), "moments are not enabled")
void dm_surfel(double leaf, const long long ia[3], const unsigned long long* v4, const unsigned long long* m9,
               const loamx_densemap_surfel_config& c, int axes, loamx_surfel& out);
loamx_densemap_surfel_config checked_surfel_config(const loamx_densemap_surfel_config* cfg);
const loamx_densemap_static_rule* checked_optional_rule(loamx_densemap* h, const loamx_densemap_static_rule* rule,
                                                        loamx_densemap_static_rule& r);

}  // namespace loamx
