// Dense global map (densemap.hpp, include/loamx.h loamx_densemap_*): registered sweeps accumulated into a voxel hash table in HBM.
// This file is the core: the table's own kernels, the adds, growth, admission and the counters.  The handle's class is declared in
// densemap_map.hpp; every feature has a file of its own that holds its kernels, its members of the class and its C entry points:
//
//   densemap_dev.hpp      the device helpers that kernels of more than one file share (filter, claim, wave counters, the voxel walk)
//   densemap.hip          insert, carve, rehash; create / add / stats / prune / reset / enable_carving / enable_moments
//   densemap_export.hip   the voxels on the host: records, misses, moment words, surfels, PCD files, and freeze
//   densemap_merge.hip    save, load, merge of two maps and of a file (densemap_file.hpp)
//   densemap_raycast.hip  first hits of rays through the table (DmCaster)
//   densemap_rebuild.hip  the sweep log and its replay under corrected poses (densemap_history.hpp)
//   densemap_align.hip    alignment of sweeps against the frozen surfel snapshot (DmFrozen)
//   densemap_pyramid.hip  coarser levels of the table and of the snapshot, and the coarse-to-fine alignment over them
//   densemap_grid.hip     a window of the table projected to a 2-D navigation grid (DmGrid)
//   densemap_route.hip    cost-to-go field and routes over that grid (DmRoute: the engine of densemap_route_core.hpp, densemap_route_schedule.hpp)
//   densemap_route3.hip   cost-to-go field and routes in 3-D over the distance field (DmRoute3: the same engine, the same schedule)
//   densemap_segment.hip  connected components of the voxels (DmSegment)
//   densemap_segment_cloud.hip  the objects of a cloud that is not in the map, tested against the table (DmSegCloud)
//   densemap_region.hip   the compaction (of every voxel, or of a window's), region exports, evict, tile files and paging
//
// One insert kernel per add: range filter, voxel key, a combine of equal keys inside the wave, the open-addressing insert and the
// accumulation, in one pass over the cloud.  The host keeps an upper bound of the occupancy (last known count + points enqueued since)
// and enqueues a rehash into a table twice the size before that bound could pass half the slots — no wait for the device.  The known
// count is refreshed by a kernel store into pinned memory (pinned_copy.hpp), read once an event shows it has landed.
//
// Carving (loamx_densemap_enable_carving): two more 32-bit words per slot, miss and stamp.  The insert stamps the voxels of its call; a
// second kernel behind it walks each sweep ray from the origin towards its point through the voxel grid and counts a miss in every
// voxel of the table it crosses that the same call did not hit.  The walk only looks keys up: it never claims a slot.
//
// Moments (loamx_densemap_enable_moments): nine more 64-bit words per slot in an array of their own, the sums of the products of the
// offsets and of the fixed-point vectors from the origin.  The insert adds them with the voxel's other sums; the surfel of a voxel
// (covariance, normal, curvature) is computed on the host at export.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include <algorithm>

namespace loamx {

// one point per thread.  vals: 4 words per slot (n, Sx, Sy, Sz).  COMBINE: equal keys of a wave are summed in LDS first, and one lane
// per distinct key touches the table (the sweep is in firing order: neighbouring lanes share voxels).  STAMP (carving): that lane also
// stores the call's sequence number into the slot's stamp word (every writer of a call stores the same value).  MOMENTS: the nine sums
// of mom ride along.  Their combine runs in 64-bit LDS words, one atomic per word and lane: six for the products (64 x 2^40 does not
// fit 32 bits) and three that carry w_a * 2^26 + q_a, the signed viewpoint term above the offset (|64 x 2^30 x 2^26| < 2^63, and the
// low field, a sum of non-negative terms below 2^26, never borrows from the high one).  9 x 64 x 8 B per wave, 18 KiB per block: eight
// blocks of 256 threads still fit a CU's LDS, and the 32-bit accumulators are not allocated in that instantiation.  Word-major layout:
// the lanes of one instruction go to consecutive 8-byte words unless they share a leader
template <bool COMBINE, bool STAMP, bool MOMENTS>
__global__ __launch_bounds__(256) void k_dm_insert(const float4* __restrict__ pts, uint32_t n, DmFilter F, unsigned long long* __restrict__ keys,
                                                   unsigned long long* __restrict__ vals, uint32_t mask, uint32_t shift,
                                                   unsigned long long* __restrict__ ctr, uint32_t* __restrict__ aux, uint32_t seq,
                                                   unsigned long long* __restrict__ mom) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
#define DM_INSERT_HAS_POINT i < n
#define DM_INSERT_POINT pts[i]
#include "dm_insert_body.inc"
#undef DM_INSERT_HAS_POINT
#undef DM_INSERT_POINT
}

// Free-space update behind an insert: one ray per lane.  A block owns 256 * stride consecutive points: every lane first counts the
// added points of that span that the stride leaves out (coalesced), then lane t walks the ray of point base + t * stride.  Rays of a
// wave differ in length, so the wave runs as long as its longest ray; each step is one dependent random probe of the key array, and
// the rays of the other waves on the CU are what hides that latency.  Every loop is bounded by an integer: the span, n_steps <=
// max_steps, mask + 1 probes.
__global__ __launch_bounds__(256) void k_dm_carve(const float4* __restrict__ pts, uint32_t n, DmFilter F, DmCarve R,
                                                  const unsigned long long* keys, uint32_t* aux, uint32_t mask, uint32_t shift,
                                                  unsigned long long* __restrict__ ctr) {
#define DM_CARVE_POINT(j) pts[j]
#include "dm_carve_body.inc"
#undef DM_CARVE_POINT
}

// every occupied slot of the old table into the new one (keys are unique: claim the first empty slot of the probe sequence).  AUX: the
// slot's miss and stamp words travel with it.  DROP: what stays behind — DM_DROP_RULE (with AUX) the voxels the rule calls dynamic,
// DM_DROP_WINDOW those the window selects (densemap_region.hip, evict); the survivors are then counted into ctr[0] (zeroed before the
// launch).  MOM: the slot's nine moment words travel with it
template <bool AUX, int DROP, bool MOM>
__global__ __launch_bounds__(256) void k_dm_rehash(const unsigned long long* __restrict__ okeys, const unsigned long long* __restrict__ ovals,
                                                   uint32_t on, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ vals,
                                                   uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                   const uint32_t* __restrict__ oaux, uint32_t* __restrict__ aux, loamx_densemap_static_rule rule,
                                                   const unsigned long long* __restrict__ omom, unsigned long long* __restrict__ mom, DmWindow W) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < on ? okeys[i] : DM_EMPTY;
  bool live = key != DM_EMPTY;
  if (DROP == DM_DROP_RULE && live) live = !dm_dynamic(rule, ovals[4ull * i], oaux[2ull * i]);
  if (DROP == DM_DROP_WINDOW && live) live = !dm_in_window(key, W);
  uint32_t slot = 0;
  bool won = false;
  if (live) {
    if (dm_find_or_claim(keys, mask, shift, key, slot, won)) {
      const ulonglong2* s = (const ulonglong2*)(ovals + 4ull * i);
      ulonglong2* d = (ulonglong2*)(vals + 4ull * slot);
      d[0] = s[0];
      d[1] = s[1];
      if (AUX) *(uint2*)(aux + 2ull * slot) = *(const uint2*)(oaux + 2ull * i);
      if (MOM) {
        const unsigned long long* ms = omom + (unsigned long long)DM_MOM_WORDS * i;
        unsigned long long* md = mom + (unsigned long long)DM_MOM_WORDS * slot;
#pragma unroll
        for (int k = 0; k < DM_MOM_WORDS; k++) md[k] = ms[k];
      }
    } else {
      ctr[3] = 1ull;
    }
  }
  if (DROP != DM_DROP_NONE) dm_wave_count(&ctr[0], won);
}

DenseMap::DenseMap(const loamx_densemap_config& c) : cfg(c) {
  select_device(cfg.device);
  LX_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
  LX_HIP(hipEventCreateWithFlags(&ev_last_, hipEventDisableTiming));
  LX_HIP(hipEventCreateWithFlags(&ev_snap_, hipEventDisableTiming));
  ctr_.reserve(DM_CTR_WORDS);
  h_ctr_.reserve(DM_CTR_WORDS);
  h_snap_.reserve(1);   // (must not move while a snapshot is in flight)
  inv_ = 1.0f / cfg.leaf;
  tab_.alloc(cfg.initial_slots, false, false);
  clear(own_);
  LX_HIP(hipStreamSynchronize(own_));
}
DenseMap::~DenseMap() {
  (void)hipSetDevice(cfg.device);
  if (last_st_) (void)hipEventSynchronize(ev_last_);
  (void)hipStreamSynchronize(own_);
  free_graveyard();
  (void)hipFree(log_);
  DmTable().swap(tab_);
  (void)hipEventDestroy(ev_last_);
  (void)hipEventDestroy(ev_snap_);
  (void)hipStreamDestroy(own_);
}

DenseSource DenseMap::host_source(DmCloudStage& via, const loamx_cloud* c, const float origin[3]) {
  check_cloud(c, false);
  LX_HIP(hipSetDevice(cfg.device));
  return via.source(c, origin, own_, cfg.device);
}

// enqueued on the source's stream, behind every add so far: own_ for a cloud from the host, the stream that wrote a registered cloud
int DenseMap::add(const DenseSource& s) {
  LX_REQUIRE(s.device == cfg.device, "the dense map and its source live on different devices");
  if (!s.has_cloud) return LOAMX_SKIPPED;
  LX_HIP(hipSetDevice(cfg.device));
  if (!admit(s.n) || !hist_.admits(s.n)) return LOAMX_E_CAPACITY;
  // (kept from the host form, which no test pins: an empty cloud from the host returns before it is staged and enqueues nothing, not
  // even the event of the last add; an empty registered cloud goes on and moves that event to its stream)
  if (!s.n && s.stream == own_) return LOAMX_OK;
  order_behind(s.stream);
  enqueue_add(s.points(), s.n, s.origin, s.stream);
  return LOAMX_OK;
}

void DenseMap::stats(uint64_t out[6]) {
  read_counters();
  out[0] = occ_.occ; out[1] = tab_.slots; out[2] = offered_;
  out[3] = offered_ - drop_range_ - drop_key_; out[4] = drop_range_; out[5] = drop_key_;
}

void DenseMap::snapshot(Snapshot& S, bool want_mom) {
  read_counters();
  snapshot_of(tab_, occ_.occ, S, want_mom);
}

void DenseMap::snapshot_of(const DmTable& T, uint64_t occ, Snapshot& S, bool want_mom) { compact_of(T, nullptr, occ, &S, want_mom, nullptr); }

void DenseMap::enable_moments() {
  read_counters();
  LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "moments can only be enabled on an empty map (a fresh handle, or right after reset)");
  if (!tab_.mom) {   // (no new table: the empty one that stands gets the array, zeroed like the rest of it)
    tab_.add_mom();
    tab_.clear_mom(own_);
    LX_HIP(hipStreamSynchronize(own_));
  }
}

void DenseMap::enable_carving(const loamx_densemap_carve_config& c) {
  read_counters();
  LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "carving can only be enabled on an empty map (a fresh handle, or right after reset)");
  if (!tab_.aux) {   // (as in enable_moments)
    tab_.add_aux();
    tab_.clear_aux(own_);
    LX_HIP(hipStreamSynchronize(own_));
  }
  carve_ = c;
}

void DenseMap::carve_stats(uint64_t out[6]) {
  read_counters();
  for (int k = 0; k < 6; k++) out[k] = carve_ctr_[k];
}

uint64_t DenseMap::prune(const loamx_densemap_static_rule& rule) {
  read_counters();
  const uint64_t before = occ_.occ;
  DmTable nt;
  nt.alloc(tab_.slots, true, tab_.mom != nullptr);   // (aux whatever the map has: the callers require carving)
  nt.clear(own_);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long), own_));   // (the occupancy: recounted by the kernel)
  launch_rehash<DM_DROP_RULE>(own_, nt, rule, DmWindow());
  LX_HIP(hipGetLastError());
  replace_table(nt);
  read_counters();
  return before - occ_.occ;
}

void DenseMap::reset() {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  clear(own_);
  LX_HIP(hipStreamSynchronize(own_));
  frozen.drop();
  drop_coarse();
  dist_.drop();
  route3_.drop();
  tsdf_.drop();
  occ_.reset();
  offered_ = drop_range_ = drop_key_ = 0;
  for (uint64_t& c : carve_ctr_) c = 0;
  seq_ = 0;
  hist_.clear();
}

DmFilter DenseMap::filter_for(const float origin[3]) const {
  DmFilter F;
  F.inv = inv_;
  F.min2 = cfg.min_range * cfg.min_range;
  F.max2 = cfg.max_range * cfg.max_range;
  F.use_max = cfg.max_range > 0.f ? 1 : 0;
  F.ox = origin[0]; F.oy = origin[1]; F.oz = origin[2];
  return F;
}
DmCarve DenseMap::carve_args(uint32_t seq) const {
  DmCarve R;
  R.max2 = carve_.max_range * carve_.max_range;
  R.use_max = carve_.max_range > 0.f ? 1 : 0;
  R.stride = carve_.ray_stride; R.end_margin = carve_.end_margin; R.max_steps = carve_.max_steps; R.seq = seq;
  return R;
}

void DenseMap::replace_table(DmTable& nt) {
  tab_.swap(nt);
  nt.retire(graveyard_);
}
// the current table into nt on st, under the map's features; DROP: DM_DROP_RULE (carving is on) the rule's dynamic voxels stay
// behind, DM_DROP_WINDOW those the window selects
template <int DROP> void DenseMap::launch_rehash(hipStream_t st, const DmTable& nt, const loamx_densemap_static_rule& rule, const DmWindow& W) {
  const DmTable& T = tab_;
  dm_dispatch2(T.aux != nullptr, T.mom != nullptr, [&](auto A, auto M) {
    constexpr bool AUX = decltype(A)::value, MOM = decltype(M)::value;
    if constexpr (AUX || DROP != DM_DROP_RULE)
      hipLaunchKernelGGL((k_dm_rehash<AUX, DROP, MOM>), dim3((T.slots + 255) / 256), dim3(256), 0, st, T.keys, T.vals, T.slots, nt.keys, nt.vals,
                         nt.mask(), nt.shift(), ctr_.p, T.aux, nt.aux, rule, T.mom, nt.mom, W);
  });
}
template void DenseMap::launch_rehash<DM_DROP_WINDOW>(hipStream_t, const DmTable&, const loamx_densemap_static_rule&, const DmWindow&);   // (densemap_region.hip)
// the insert of one add; the combine by the bench hook, the moment words when the map has them
template <bool STAMP> void DenseMap::launch_insert(hipStream_t st, const float4* pts, uint32_t n, const DmFilter& F, uint32_t seq) {
  const DmTable& T = tab_;
  dm_dispatch2(combine, T.mom != nullptr, [&](auto C, auto M) {
    hipLaunchKernelGGL((k_dm_insert<decltype(C)::value, STAMP, decltype(M)::value>), dim3((n + 255) / 256), dim3(256), 0, st, pts, n, F, T.keys,
                       T.vals, T.mask(), T.shift(), ctr_.p, T.aux, seq, T.mom);
  });
}
void DenseMap::clear(hipStream_t st) {
  tab_.clear(st);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long) * DM_CTR_WORDS, st));
}
void DenseMap::free_graveyard() {
  for (void* p : graveyard_) (void)hipFree(p);
  graveyard_.clear();
}
void DenseMap::order_behind(hipStream_t st) {
  if (last_st_ && last_st_ != st) LX_HIP(hipStreamWaitEvent(st, ev_last_, 0));
}
void DenseMap::wait_adds() {
  if (last_st_) LX_HIP(hipEventSynchronize(ev_last_));
  stage.settle();
  occ_.snapshot_abandoned();
  free_graveyard();
}
void DenseMap::read_counters() {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const unsigned long long* c = h_ctr_.fetch(ctr_.p, DM_CTR_WORDS, own_);
  LX_HIP(hipStreamSynchronize(own_));
  LX_REQUIRE(c[3] == 0ull, "dense map: hash table overflow");
  occ_.exact(c[0]);
  drop_range_ = c[1]; drop_key_ = c[2];
  for (int k = 0; k < 6; k++) carve_ctr_[k] = c[4 + k];
}
void DenseMap::poll_snapshot() {
  if (!occ_.snap_pending) return;
  const hipError_t e = hipEventQuery(ev_snap_);
  if (e == hipErrorNotReady) return;
  LX_HIP(e);
  occ_.snapshot_landed(*h_snap_.data());
}
// capacity rule (include/loamx.h): decided before anything is enqueued; the exact count is waited for only near the cap
bool DenseMap::admit(uint32_t n) {
  poll_snapshot();
  if (occ_.admits_by_bound(n, cfg.max_voxels)) return true;
  read_counters();
  return occ_.admits_exact(n, cfg.max_voxels);
}
// growth: keep the load at most one half even if every one of n records, and every point enqueued since the last count, made a voxel
// of its own.  The rehash into the larger table is enqueued on st; the host does not wait
void DenseMap::grow_for(uint64_t n, hipStream_t st) {
  const uint64_t want = occ_.slots_wanted(tab_.slots, n);
  LX_REQUIRE(want <= (1ull << 31), "dense map: more voxels than the table can index");
  if (want != tab_.slots) {
    DmTable nt;
    nt.alloc(want, tab_.aux != nullptr, tab_.mom != nullptr);
    nt.clear(st);
    launch_rehash<DM_DROP_NONE>(st, nt, loamx_densemap_static_rule{0u, 0u, 0u}, DmWindow());
    replace_table(nt);
    rehashes++;
  }
}
void DenseMap::enqueue_add(const float4* pts, uint32_t n, const float origin[3], hipStream_t st) {
  if (history_ && n) log_reserve(n, st);   // (a failed allocation leaves map and log as they were)
  grow_for(n, st);
  if (n) {
    const DmFilter F = filter_for(origin);
    if (!tab_.aux) {
      launch_insert<false>(st, pts, n, F, 0u);
    } else {
      // carving: the insert stamps its voxels with the call's sequence number, and the rays are traced behind it
      seq_++;
      launch_insert<true>(st, pts, n, F, seq_);
      const DmCarve R = carve_args(seq_);
      const uint64_t span = 256ull * R.stride;
      hipLaunchKernelGGL(k_dm_carve, dim3((uint32_t)((n + span - 1) / span)), dim3(256), 0, st, pts, n, F, R, tab_.keys, tab_.aux, tab_.mask(),
                         tab_.shift(), ctr_.p);
    }
  }
  LX_HIP(hipGetLastError());
  if (history_ && n) {   // the whole cloud as offered, behind whatever wrote it
    LX_HIP(hipMemcpyAsync(log_ + hist_.points, pts, DMH_POINT_BYTES * n, hipMemcpyDeviceToDevice, st));
    hist_.append(n, origin);
  }
  offered_ += n;
  if (occ_.enqueued(n)) {   // the occupancy snapshot behind this add
    h_snap_.fetch(ctr_.p, 1, st);
    LX_HIP(hipEventRecord(ev_snap_, st));
  }
  LX_HIP(hipEventRecord(ev_last_, st));
  last_st_ = st;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_default_config(loamx_densemap_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->leaf = 0.1f;
  cfg->min_range = 0.f;
  cfg->max_range = 0.f;
  cfg->max_voxels = 0;
  cfg->initial_slots = 1u << 20;
  cfg->device = 0;
}

loamx_densemap* loamx_densemap_create(const loamx_densemap_config* cfg) {
  loamx_densemap* h = nullptr;
  guard([&]() {
    const loamx_densemap_config c = or_default(cfg, loamx_densemap_default_config);
    LX_REQUIRE(c.leaf > 0.f && std::isfinite(c.leaf), "leaf must be positive");
    LX_REQUIRE(c.min_range >= 0.f && c.max_range >= 0.f && std::isfinite(c.min_range) && std::isfinite(c.max_range), "ranges must be >= 0");
    LX_REQUIRE(c.max_range == 0.f || c.max_range >= c.min_range, "max_range must be 0 or >= min_range");
    LX_REQUIRE(c.initial_slots >= 1024u && c.initial_slots <= (1u << 30) && (c.initial_slots & (c.initial_slots - 1u)) == 0u,
               "initial_slots must be a power of two in [1024, 2^30]");
    h = new loamx_densemap(c);
    return LOAMX_OK;
  });
  return h;
}
void loamx_densemap_destroy(loamx_densemap* h) { delete h; }

int loamx_densemap_reset(loamx_densemap* h) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->d.reset(); return LOAMX_OK; });
}
int loamx_densemap_add(loamx_densemap* h, const loamx_cloud* points, const float origin[3]) {
  return guard([&]() {
    LX_REQUIRE(h && points && origin, "NULL argument");
    return h->d.add(h->d.host_source(h->d.stage, points, origin));
  });
}
int loamx_densemap_add_from_map(loamx_densemap* h, loamx_map* m) {
  return guard([&]() {
    LX_REQUIRE(h && m, "NULL argument");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.add(s);
  });
}
int loamx_densemap_add_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot) {
  return guard([&]() {
    LX_REQUIRE(h && p, "NULL argument");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.add(s);
  });
}
int loamx_densemap_get_stats(loamx_densemap* h, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h && stats, "NULL argument");
    h->d.stats(stats);
    return LOAMX_OK;
  });
}

void loamx_densemap_carve_default_config(loamx_densemap_carve_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 0.f;
  cfg->ray_stride = 1u;
  cfg->end_margin = 1u;
  cfg->max_steps = 4096u;
}
void loamx_densemap_static_rule_default(loamx_densemap_static_rule* rule) {
  if (!rule) return;
  rule->min_misses = 3u;
  rule->num = 1u;
  rule->den = 1u;
}
int loamx_densemap_rule_is_dynamic(const loamx_densemap_static_rule* rule, uint64_t n, uint32_t miss) {
  return guard([&]() {
    LX_REQUIRE(rule, "NULL argument");
    LX_REQUIRE(rule->den != 0u, "the rule's den must not be 0");
    return dm_dynamic(*rule, n, miss) ? 1 : 0;
  });
}
int loamx_densemap_enable_carving(loamx_densemap* h, const loamx_densemap_carve_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_carve_config c = or_default(cfg, loamx_densemap_carve_default_config);
    LX_REQUIRE(c.max_range >= 0.f && std::isfinite(c.max_range), "max_range must be >= 0");
    LX_REQUIRE(c.ray_stride >= 1u, "ray_stride must be >= 1");
    LX_REQUIRE(c.max_steps >= 1u && c.max_steps <= 65536u, "max_steps must be in [1, 65536]");
    h->d.enable_carving(c);
    return LOAMX_OK;
  });
}
int loamx_densemap_get_carve_stats(loamx_densemap* h, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h && stats, "NULL argument");
    LX_REQUIRE_CARVING(h);
    h->d.carve_stats(stats);
    return LOAMX_OK;
  });
}
int loamx_densemap_prune(loamx_densemap* h, const loamx_densemap_static_rule* rule, uint64_t* removed) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_static_rule r = checked_rule(rule);
    LX_REQUIRE_CARVING(h);
    LX_HIP(hipSetDevice(h->d.cfg.device));
    const uint64_t gone = h->d.prune(r);
    if (removed) *removed = gone;
    return LOAMX_OK;
  });
}
int loamx_densemap_enable_moments(loamx_densemap* h) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    h->d.enable_moments();
    return LOAMX_OK;
  });
}

// bench / test hooks (not in include/loamx.h): the in-wave combining of equal keys on or off, and the number of rehashes so far
int loamx_densemap_set_combine(loamx_densemap* h, int on) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->d.combine = on != 0; return LOAMX_OK; });
}
uint64_t loamx_densemap_rehashes(loamx_densemap* h) { return h ? h->d.rehashes : 0; }

}  // extern "C"
