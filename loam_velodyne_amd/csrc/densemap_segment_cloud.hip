// Objects of a sweep that is not in the map (densemap.hpp DmSegCloud, include/loamx.h loamx_densemap_segment_cloud and what goes with
// it): the points of a cloud that `add` would admit are tested against the live table (is a mapped voxel within `margin` cells?), the
// ones that pass go into a scratch table of the map's own format, the five segment kernels of densemap_segment.hip label that table,
// and every point gets the rank of its voxel's component.
//
// Two kernels of its own, one point per thread, 256 threads per block, around DmSegment::run:
//   k_dm_cseg_insert  admission by dm_added (the insert's own expressions); for NEW / KNOWN up to 1, 27 or 125 dm_find probes of the
//                     live table, the point's own cell first, left on the first mapped cell (a found key costs one read of its n and,
//                     with a rule, of its miss word); a neighbour cell outside |i| < 2^20 does not exist and is not looked up, as in
//                     k_dm_seg_link.  The entered points then run dm_insert_body.inc as k_dm_insert does (equal keys combined in the
//                     wave, one claim and four adds per distinct key) into the scratch table; the point's key (EMPTY: not entered) is
//                     kept per point for the labels.  The live table is only read: every add was waited for, nothing writes it.
//   k_dm_cseg_labels  per entered point: dm_find of its key in the scratch table, the flattened parent of that slot, the compact id of
//                     the root (DmSegment's own arrays, as run left them).  The host maps ids to ranks while it copies out.
//
// ctr: [0] voxels of the scratch table, [1] dropped by range, [2] dropped by the key rule, [3] a probe bound was reached in either
// table (never, while the load rules hold: LOAMX_E_INTERNAL), [4] admitted but rejected by the map test, [5] entered.  Counters are
// summed per wave.  No spin-wait, no grid barrier; the scratch table's words are touched by atomics only while the insert runs.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include <algorithm>

namespace loamx {

constexpr int DM_CSEG_CTR = 6;

struct DmCsegArgs {
  uint32_t which, margin, map_min_points;
  int use_rule;
  loamx_densemap_static_rule rule;
};

// 1: the cell is mapped; 0: it is not; -1: the probe bound was reached
__device__ inline int dm_cseg_mapped(const DmCsegArgs& A, const unsigned long long* __restrict__ mkeys, const unsigned long long* __restrict__ mvals,
                                     const uint32_t* __restrict__ maux, uint32_t mmask, uint32_t mshift, int cx, int cy, int cz) {
  uint32_t slot = 0u;
  const int f = dm_find(mkeys, mmask, mshift, dm_key(cx, cy, cz), slot);
  if (f <= 0) return f;
  const unsigned long long cnt = mvals[4ull * slot];
  return cnt >= A.map_min_points && !(A.use_rule && dm_dynamic(A.rule, cnt, maux[2ull * slot])) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dm_cseg_insert(const float4* __restrict__ pts, uint32_t n, DmFilter F, DmCsegArgs A,
                                                        const unsigned long long* __restrict__ mkeys, const unsigned long long* __restrict__ mvals,
                                                        const uint32_t* __restrict__ maux, uint32_t mmask, uint32_t mshift,
                                                        unsigned long long* __restrict__ keys, unsigned long long* __restrict__ vals,
                                                        uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                        unsigned long long* __restrict__ pkey) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
  bool out_range = false, out_key = false, rejected = false, enter = false, overflow = false;
  if (i < n) {
    pt = pts[i];
    float d2;
    if (!dm_added(pt, F, d2)) {
      out_range = !(d2 >= F.min2 && (!F.use_max || d2 <= F.max2));
      out_key = !out_range;
    } else if (A.which == LOAMX_CLOUD_ALL) {
      enter = true;
    } else {
      const int cx = (int)floorf(pt.x * F.inv), cy = (int)floorf(pt.y * F.inv), cz = (int)floorf(pt.z * F.inv);   // (|c| < 2^20)
      const int m = (int)A.margin, side = 2 * m + 1, lim = (1 << DM_QBITS) - 1;
      int near = dm_cseg_mapped(A, mkeys, mvals, maux, mmask, mshift, cx, cy, cz);
      for (int o = 0; o < side * side * side && near == 0; o++) {
        const int dx = o % side - m, dy = (o / side) % side - m, dz = o / (side * side) - m;
        if (dx == 0 && dy == 0 && dz == 0) continue;
        const int nx = cx + dx, ny = cy + dy, nz = cz + dz;
        if (nx < -lim || nx > lim || ny < -lim || ny > lim || nz < -lim || nz > lim) continue;   // no such voxel: not looked up
        near = dm_cseg_mapped(A, mkeys, mvals, maux, mmask, mshift, nx, ny, nz);
      }
      if (near < 0) overflow = true;
      else enter = (near == 1) == (A.which == LOAMX_CLOUD_KNOWN);
      rejected = !enter;
    }
  }
  dm_wave_count(&ctr[1], out_range);
  dm_wave_count(&ctr[2], out_key);
  dm_wave_count(&ctr[4], rejected);
  dm_wave_count(&ctr[5], enter);
  if (overflow) ctr[3] = 1ull;
  // the insert of the entered points, as k_dm_insert<true, false, false> does it (its range filter and key rule pass again: counted above)
  constexpr bool COMBINE = true, STAMP = false, MOMENTS = false;
  uint32_t* const aux = nullptr;
  unsigned long long* const mom = nullptr;
  const uint32_t seq = 0u;
  (void)aux; (void)mom; (void)seq; (void)wid;
#define DM_INSERT_HAS_POINT enter
#define DM_INSERT_POINT pt
#include "dm_insert_body.inc"
#undef DM_INSERT_HAS_POINT
#undef DM_INSERT_POINT
  if (i < n) pkey[i] = key;   // (EMPTY: the point did not enter)
}

// ids[i]: the compact id of the component of point i's voxel, NONE when the point did not enter or its voxel is not selected.  parent
// (flattened) and rootid: DmSegment's arrays over the scratch table's slots
__global__ __launch_bounds__(256) void k_dm_cseg_labels(const unsigned long long* __restrict__ pkey, uint32_t n, const unsigned long long* __restrict__ keys,
                                                        uint32_t mask, uint32_t shift, const uint32_t* __restrict__ parent,
                                                        const uint32_t* __restrict__ rootid, uint32_t n_roots, uint32_t* __restrict__ ids,
                                                        unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t id = LOAMX_SEGMENT_NONE;
  const unsigned long long key = pkey[i];
  if (key != DM_EMPTY) {
    uint32_t slot = 0u;
    const int f = dm_find(keys, mask, shift, key, slot);
    if (f < 0) ctr[3] = 1ull;
    if (f > 0) {
      const uint32_t r = parent[slot];
      if (r != LOAMX_SEGMENT_NONE) id = rootid[r];
      if (id != LOAMX_SEGMENT_NONE && id >= n_roots) id = LOAMX_SEGMENT_NONE;   // (cannot happen: every root got an id below n_roots)
    }
  }
  ids[i] = id;
}

void DmSegCloud::insert(const DmTable& M, const DmFilter& F, const loamx_densemap_segment_cloud_config& c, const loamx_densemap_static_rule* rule,
                        const float4* pts, uint32_t n, hipStream_t st, uint64_t counts[5]) {
  LX_REQUIRE(n <= (1u << 30), "points: more than 2^30 points in one cloud");   // (the scratch table indexes 2^31 slots)
  const uint32_t need = std::max<uint32_t>(1024u, 1u << log2u(2ull * n));   // a load of at most one half: the insert's rule, no growth
  if (need > cap_slots_) {   // (every earlier call has returned: nothing reads the table that goes)
    DmTable().swap(tab_);
    cap_slots_ = 0;
    tab_.alloc(need, false, false);
    cap_slots_ = need;
  }
  tab_.slots = need;   // (the front of the allocation: the kernels of this call see a table of this size)
  pkey_.reserve(n);
  ctr_.reserve(DM_CSEG_CTR);
  tab_.clear(st);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long) * DM_CSEG_CTR, st));
  DmCsegArgs A;
  A.which = c.which; A.margin = c.margin; A.map_min_points = c.map_min_points;
  A.use_rule = rule ? 1 : 0;
  A.rule = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
  hipLaunchKernelGGL(k_dm_cseg_insert, dim3((n + 255u) / 256u), dim3(256), 0, st, pts, n, F, A, M.keys, M.vals, M.aux, M.mask(), M.shift(),
                     tab_.keys, tab_.vals, tab_.mask(), tab_.shift(), ctr_.p, pkey_.p);
  LX_HIP(hipGetLastError());
  const unsigned long long* h = h_ctr_.fetch(ctr_.p, DM_CSEG_CTR, st);
  LX_HIP(hipStreamSynchronize(st));
  if (h[3] != 0ull) throw Error(LOAMX_E_INTERNAL, "segment_cloud: a probe bound was reached in a hash table");
  counts[0] = h[1]; counts[1] = h[2]; counts[2] = h[4]; counts[3] = h[5]; counts[4] = h[0];
}

const uint32_t* DmSegCloud::ids(const DmSegment& seg, uint32_t n_roots, uint32_t n, hipStream_t st) {
  ids_.reserve(n);
  hipLaunchKernelGGL(k_dm_cseg_labels, dim3((n + 255u) / 256u), dim3(256), 0, st, pkey_.p, n, tab_.keys, tab_.mask(), tab_.shift(), seg.parent(),
                     seg.rootid(), n_roots, ids_.p, ctr_.p);
  LX_HIP(hipGetLastError());
  const uint32_t* out = h_ids_.fetch(ids_.p, n, st);
  const unsigned long long* h = h_ctr_.fetch(ctr_.p, DM_CSEG_CTR, st);
  LX_HIP(hipStreamSynchronize(st));
  if (h[3] != 0ull) throw Error(LOAMX_E_INTERNAL, "segment_cloud: a probe bound was reached in the scratch table");
  return out;
}

void dm_segment_cloud_check(const loamx_densemap_segment_cloud_config& c) {
  LX_REQUIRE(c.which <= LOAMX_CLOUD_KNOWN, "which must be LOAMX_CLOUD_ALL, _NEW or _KNOWN");
  LX_REQUIRE(c.margin <= 2u, "margin must be 0, 1 or 2");
  LX_REQUIRE(c.map_min_points >= 1u, "map_min_points must be >= 1");
  loamx_densemap_segment_config s;
  s.which = LOAMX_SEGMENT_ALL;
  s.connectivity = c.connectivity; s.min_points = c.min_points; s.min_voxels = c.min_voxels;
  for (int a = 0; a < 3; a++) { s.lo[a] = c.lo[a]; s.hi[a] = c.hi[a]; }
  dm_segment_check(s);
}

// include/loamx.h, loamx_densemap_segment_cloud: the cloud of src where it lies, own_ behind the stream that wrote it (a cloud from the
// host comes up through the feature's own staging block, on own_; an empty one is not staged), every add waited for; a checked configuration and rule.  The outputs are written last, all or none;
// LOAMX_E_CAPACITY: only the two counts
int DenseMap::segment_cloud(const DenseSource& src, const loamx_densemap_segment_cloud_config& c, const loamx_densemap_static_rule* rule,
                            uint32_t* labels, uint64_t label_capacity, uint64_t* n_points, loamx_segment* segs, uint64_t seg_capacity,
                            uint64_t* n_segs, uint64_t stats[13]) {
  LX_REQUIRE(src.device == cfg.device, "the dense map and its source live on different devices");
  if (!src.has_cloud) return LOAMX_SKIPPED;
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  if (src.n) dm_stream_behind(own_, src.stream);
  const float4* pts = src.n ? src.points() : nullptr;
  const uint32_t n = src.n;
  uint64_t s[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<loamx_segment> sg;
  std::vector<uint32_t> none, rank;
  const uint32_t* ids = nullptr;
  if (n) {
    uint64_t cnt[5];
    cseg_.insert(tab_, filter_for(src.origin), c, rule, pts, n, own_, cnt);
    s[0] = n;
    for (int k = 0; k < 5; k++) s[1 + k] = cnt[k];
    if (s[1] + s[2] + s[3] + s[4] != s[0]) throw Error(LOAMX_E_INTERNAL, "segment_cloud: the counters do not add up to the cloud's count");
    if (s[5]) {
      loamx_densemap_segment_config sc;
      sc.which = LOAMX_SEGMENT_ALL;
      sc.connectivity = c.connectivity; sc.min_points = c.min_points; sc.min_voxels = c.min_voxels;
      for (int a = 0; a < 3; a++) { sc.lo[a] = c.lo[a]; sc.hi[a] = c.hi[a]; }
      uint64_t ss[6];
      seg_.run(cseg_.table(), sc, loamx_densemap_static_rule{0u, 0u, 0u}, s[5], false, none, sg, ss, scan_, own_, &rank);
      s[6] = ss[0]; s[7] = ss[1]; s[8] = ss[2]; s[9] = ss[3]; s[10] = ss[4]; s[12] = ss[5];
      for (const loamx_segment& g : sg) s[11] += g.points;   // (a voxel's n counts the entered points in it)
      if (labels && label_capacity >= n && !(segs && seg_capacity < sg.size())) ids = cseg_.ids(seg_, (uint32_t)rank.size(), n, own_);
    }
  }
  *n_points = n;
  *n_segs = sg.size();
  if ((labels && label_capacity < n) || (segs && seg_capacity < sg.size())) return LOAMX_E_CAPACITY;
  if (labels) {
    uint64_t labelled = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t id = ids ? ids[i] : LOAMX_SEGMENT_NONE;
      labels[i] = id == LOAMX_SEGMENT_NONE ? LOAMX_SEGMENT_NONE : rank[id];
      labelled += labels[i] != LOAMX_SEGMENT_NONE;
    }
    if (labelled != s[11]) throw Error(LOAMX_E_INTERNAL, "segment_cloud: the labels disagree with the components' point counts");
  }
  if (segs && !sg.empty()) memcpy(segs, sg.data(), sizeof(loamx_segment) * sg.size());
  memcpy(stats, s, sizeof(s));
  return LOAMX_OK;
}

// what the three forms check alike: the outputs that must be there, the configuration (cfg NULL: the defaults) and the rule (NULL
// stays NULL: every voxel)
static loamx_densemap_segment_cloud_config checked_segment_cloud(loamx_densemap* h, const loamx_densemap_segment_cloud_config* cfg,
                                                                 const loamx_densemap_static_rule* rule, const uint64_t* n_points,
                                                                 const uint64_t* n_segs, const uint64_t* stats) {
  LX_REQUIRE(n_points, "n_points is NULL");
  LX_REQUIRE(n_segs, "n_segs is NULL");
  LX_REQUIRE(stats, "stats is NULL");
  const loamx_densemap_segment_cloud_config c = or_default(cfg, loamx_densemap_segment_cloud_default_config);
  dm_segment_cloud_check(c);
  checked_optional_rule(h, rule);
  return c;
}

// the overlap of [alo, ahi] grown by gap with [blo, bhi], in cells (0: none)
static uint64_t box_overlap(int32_t alo, int32_t ahi, int32_t blo, int32_t bhi, int64_t gap) {
  const int64_t lo = std::max<int64_t>((int64_t)alo - gap, blo), hi = std::min<int64_t>((int64_t)ahi + gap, bhi);
  return hi >= lo ? (uint64_t)(hi - lo + 1) : 0ull;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_segment_cloud_default_config(loamx_densemap_segment_cloud_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->which = LOAMX_CLOUD_NEW;
  cfg->margin = 1u;
  cfg->map_min_points = 1u;
  cfg->connectivity = 26u;
  cfg->min_points = 1u;
  cfg->min_voxels = 1u;
  for (int a = 0; a < 3; a++) { cfg->lo[a] = -((1 << DM_QBITS) - 1); cfg->hi[a] = (1 << DM_QBITS) - 1; }
}

int loamx_densemap_segment_cloud_check(const loamx_densemap_segment_cloud_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_segment_cloud_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_densemap_segment_cloud(loamx_densemap* h, const loamx_cloud* points, const float origin[3], const loamx_densemap_segment_cloud_config* cfg,
                                 const loamx_densemap_static_rule* rule, uint32_t* labels, uint64_t label_capacity, uint64_t* n_points,
                                 loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[13]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(points, "points is NULL");
    LX_REQUIRE(origin, "origin is NULL");
    const loamx_densemap_segment_cloud_config c = checked_segment_cloud(h, cfg, rule, n_points, n_segs, stats);
    return h->d.segment_cloud(h->d.host_source(h->d.cloud_stage(), points, origin), c, rule, labels, label_capacity, n_points, segs, seg_capacity, n_segs, stats);
  });
}

int loamx_densemap_segment_cloud_from_map(loamx_densemap* h, loamx_map* m, const loamx_densemap_segment_cloud_config* cfg,
                                          const loamx_densemap_static_rule* rule, uint32_t* labels, uint64_t label_capacity, uint64_t* n_points,
                                          loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[13]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(m, "m is NULL");
    const loamx_densemap_segment_cloud_config c = checked_segment_cloud(h, cfg, rule, n_points, n_segs, stats);
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.segment_cloud(s, c, rule, labels, label_capacity, n_points, segs, seg_capacity, n_segs, stats);
  });
}

int loamx_densemap_segment_cloud_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const loamx_densemap_segment_cloud_config* cfg,
                                               const loamx_densemap_static_rule* rule, uint32_t* labels, uint64_t label_capacity,
                                               uint64_t* n_points, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs,
                                               uint64_t stats[13]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(p, "p is NULL");
    const loamx_densemap_segment_cloud_config c = checked_segment_cloud(h, cfg, rule, n_points, n_segs, stats);
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.segment_cloud(s, c, rule, labels, label_capacity, n_points, segs, seg_capacity, n_segs, stats);
  });
}

// host only.  Each overlap is at most 2^21 - 1 cells, so the product of two fits 64 bits and the product of three 128
int loamx_segments_match(const loamx_segment* prev, uint64_t n_prev, const loamx_segment* cur, uint64_t n_cur, uint32_t gap,
                         uint32_t* prev_of_cur) {
  return guard([&]() {
    LX_REQUIRE(prev || n_prev == 0, "prev is NULL");
    LX_REQUIRE(cur || n_cur == 0, "cur is NULL");
    LX_REQUIRE(prev_of_cur || n_cur == 0, "prev_of_cur is NULL");
    LX_REQUIRE(gap <= 1024u, "gap must be in [0, 1024]");
    LX_REQUIRE(n_prev < 0xffffffffull, "n_prev must be below 2^32 - 1");
    for (uint64_t j = 0; j < n_cur; j++) {
      uint32_t best = LOAMX_SEGMENT_NONE;
      unsigned __int128 best_v = 0;
      for (uint64_t i = 0; i < n_prev; i++) {
        unsigned __int128 v = 1;
        for (int a = 0; a < 3; a++) v *= box_overlap(prev[i].lo[a], prev[i].hi[a], cur[j].lo[a], cur[j].hi[a], (int64_t)gap);
        if (v == 0) continue;
        if (best == LOAMX_SEGMENT_NONE || v > best_v || (v == best_v && prev[i].min_key < prev[best].min_key)) { best = (uint32_t)i; best_v = v; }
      }
      prev_of_cur[j] = best;
    }
    return LOAMX_OK;
  });
}

}  // extern "C"
