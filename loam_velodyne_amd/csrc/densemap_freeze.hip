// Dense map, snapshots built on the device (include/loamx.h: loamx_densemap_freeze_device, loamx_densemap_freeze_pyramid_device,
// loamx_densemap_freeze_history, loamx_densemap_download_frozen).
//
// loamx_densemap_freeze downloads every voxel's thirteen words, computes the surfels on the host and uploads them.  Here the surfels
// are computed where the words lie: k_dm_surfels, one thread per slot of a table of the map's format, runs the host's own arithmetic
// (densemap_surfel.hpp: one text for both sides, every operation correctly rounded, so the six f32 of an entry have the host's bytes)
// and compacts the voxels that have a surfel into two device arrays through one counter, one atomic per wave.  Eight bytes come back
// (the count); k_dm_freeze_insert (densemap_align.hip) builds the snapshot's table from the arrays.  The kernel is a pass over
// 8 + 32 + 72 (+ 8 with a rule) bytes per slot, of which a free slot reads the first 8; the arithmetic of an occupied slot (a handful
// of Jacobi sweeps in f64) hides behind the loads of the other waves.  No scratch (the matrices are scalars, densemap_surfel.hpp).
//
// The same kernel serves the live table (freeze_device), the level tables of the cascade where densemap_pyramid.hip leaves them
// (freeze_pyramid_device), and a scratch table into which a window of the sweep log is replayed by k_dm_rebuild
// (freeze_history): a snapshot of the sweeps j - w .. j + w alone, which is what a revisit is aligned against when a loop is closed
// keyframe to keyframe.  The live map, its counters, its log and its carve words are only read.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include "densemap_surfel.hpp"

namespace loamx {

// One thread per slot i < slots.  An occupied slot that the rule (RULE: the table has aux) does not call dynamic computes its surfel at
// `leaf`; one that has a surfel whose curvature max_curvature (0: no limit) does not drop takes the next index of the output, which
// holds `cap` entries (the table's occupancy: never reached; checked all the same), and stores its key and its six f32 there.
// count[0]: entries taken
template <bool RULE>
__global__ __launch_bounds__(256) void k_dm_surfels(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                    const unsigned long long* __restrict__ mom, const uint32_t* __restrict__ aux, uint32_t slots,
                                                    loamx_densemap_static_rule rule, loamx_densemap_surfel_config sc, double leaf,
                                                    float max_curvature, unsigned long long* __restrict__ out_keys, float* __restrict__ out_rec,
                                                    unsigned long long cap, unsigned long long* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < slots ? keys[i] : DM_EMPTY;
  bool live = key != DM_EMPTY;
  float six[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const ulonglong2* s = (const ulonglong2*)(vals + 4ull * i);
    const ulonglong2 lo = s[0], hi = s[1];
    if (RULE) live = !dm_dynamic(rule, lo.x, aux[2ull * i]);
    if (live) {
      unsigned long long m9[DM_MOM_WORDS];
      const unsigned long long* ms = mom + (unsigned long long)DM_MOM_WORDS * i;
#pragma unroll
      for (int k = 0; k < DM_MOM_WORDS; k++) m9[k] = ms[k];
      const long long km = (1ll << DM_KBITS) - 1ll, half = 1ll << DM_QBITS;
      float curvature;
      live = dm_surfel_hd(leaf, ((long long)key & km) - half, ((long long)(key >> DM_KBITS) & km) - half,
                          ((long long)(key >> (2 * DM_KBITS)) & km) - half, lo.x, lo.y, hi.x, hi.y, m9, sc, six, curvature);
      if (max_curvature > 0.f && curvature > max_curvature) live = false;
    }
  }
  // the wave's entries take consecutive indices behind one atomic of its first live lane
  const unsigned long long m = __ballot(live);
  if (!m) return;
  const int lane = (int)(threadIdx.x & 63u), leader = __builtin_ctzll(m);
  unsigned long long base = 0ull;
  if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
  base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), leader, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)base, leader, 64);
  if (!live) return;
  const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
  if (at >= cap) return;
  out_keys[at] = key;
  float* r = out_rec + 6ull * at;
#pragma unroll
  for (int k = 0; k < 6; k++) r[k] = six[k];
}

// the entries of one snapshot on the device: keys[n], rec[6 * n], in no particular order
struct DmSurfelList {
  DevBuf<unsigned long long> keys, count;
  DevBuf<float> rec;
  uint64_t n = 0;
};

// the entries of the table T (`occ` voxels; nothing enqueued on another stream still writes it) under checked settings, a checked rule
// or none, on own_.  Blocks until the count is back
void DenseMap::surfel_list(const DmTable& T, uint64_t occ, double leaf, const loamx_densemap_surfel_config& sc,
                           const loamx_densemap_static_rule* rule, float max_curvature, DmSurfelList& L) {
  L.n = 0;
  if (!occ) return;
  L.keys.reserve(occ);
  L.rec.reserve(6 * occ);
  L.count.reserve(1);
  LX_HIP(hipMemsetAsync(L.count.p, 0, sizeof(unsigned long long), own_));
  const dim3 grid((T.slots + 255u) / 256u), block(256);
  if (rule)
    hipLaunchKernelGGL(k_dm_surfels<true>, grid, block, 0, own_, T.keys, T.vals, T.mom, T.aux, T.slots, *rule, sc, leaf, max_curvature, L.keys.p,
                       L.rec.p, (unsigned long long)occ, L.count.p);
  else
    hipLaunchKernelGGL(k_dm_surfels<false>, grid, block, 0, own_, T.keys, T.vals, T.mom, (const uint32_t*)nullptr, T.slots,
                       loamx_densemap_static_rule{0u, 0u, 1u}, sc, leaf, max_curvature, L.keys.p, L.rec.p, (unsigned long long)occ, L.count.p);
  LX_HIP(hipGetLastError());
  unsigned long long n = 0ull;
  LX_HIP(hipMemcpyAsync(&n, L.count.p, sizeof(n), hipMemcpyDeviceToHost, own_));
  LX_HIP(hipStreamSynchronize(own_));
  if (n > occ) throw Error(LOAMX_E_INTERNAL, "dense map: more surfels than voxels");
  L.n = n;
}

uint64_t DenseMap::freeze_device(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule) {
  read_counters();   // (waits for the adds; the occupancy is exact)
  DmSurfelList L;
  surfel_list(tab_, occ_.occ, (double)cfg.leaf, sc, rule, 0.f, L);
  frozen.build_device(L.keys.p, L.rec.p, L.n, own_);
  drop_coarse();
  return frozen.size();
}

void DenseMap::freeze_pyramid_device(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule,
                                     const loamx_densemap_pyramid_config& pc, uint64_t* n_surfels) {
  // the coarse levels' entries first, each from its table where the cascade leaves it, so that a failure of the cascade leaves the
  // snapshots that stand
  DmSurfelList lv[COARSE_LEVELS];
  const uint32_t top = pc.levels - 1u;
  if (top)
    cascade_each(top, rule, [&](uint32_t l, const DmTable& T, uint64_t occ) {
      surfel_list(T, occ, (double)level_leaf(l), sc, nullptr, pc.max_curvature, lv[l - 1u]);
    });
  const uint64_t n0 = freeze_device(sc, rule);
  if (n_surfels) n_surfels[0] = n0;
  for (uint32_t k = 0; k < top; k++) {
    coarse[k].build_device(lv[k].keys.p, lv[k].rec.p, lv[k].n, own_);
    if (n_surfels) n_surfels[k + 1] = coarse[k].size();
  }
}

// The window [first_call, first_call + n_calls) of the log replayed into a scratch table of the map's format with moment words, no
// carve words and counters of its own, sized as a rebuild sizes its attempts; level 0 from that table's surfels.  Nothing of the
// handle but the snapshot changes
int DenseMap::freeze_history(uint64_t first_call, uint64_t n_calls, const double* corrections, const loamx_densemap_surfel_config& sc,
                             uint64_t* n_surfels) {
  LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
  LX_REQUIRE(n_calls != 0, "n_calls must be at least 1");
  LX_REQUIRE(first_call < hist_.calls.size() && n_calls <= hist_.calls.size() - first_call,
             "first_call + n_calls reaches beyond the log (loamx_densemap_history_size)");
  std::vector<DmReplayCall> calls(n_calls);
  for (uint64_t k = 0; k < n_calls; k++)
    LX_REQUIRE(dm_replay_call(hist_.calls[first_call + k], corrections ? corrections + 12 * k : nullptr, calls[k]),
               "corrections: the correction of call " + std::to_string(k) + " of the window has an entry that is not finite");
  const DmHistoryCall &c0 = hist_.calls[first_call], &c1 = hist_.calls[first_call + n_calls - 1];
  const uint64_t first = c0.first, points = c1.first + c1.count - c0.first;
  LX_REQUIRE((points + 255) / 256 < (1ull << 31), "the window holds more points than one launch covers");
  read_counters();   // (waits for the adds: the log's points are in place)
  DevBuf<unsigned long long> nctr;
  DevBuf<DmReplayCall> d_calls;
  nctr.reserve(DM_CTR_WORDS + 1);
  d_calls.reserve(n_calls);
  LX_HIP(hipMemcpyAsync(d_calls.p, calls.data(), sizeof(DmReplayCall) * n_calls, hipMemcpyHostToDevice, own_));
  unsigned long long w[DM_CTR_WORDS + 1];
  DmTable nt;
  // (the window's voxels are at most its points and, without corrections, at most the map's: a guess, doubled while too small)
  for (uint64_t slots = dm_slots_for(1024, std::min<uint64_t>(points, std::max<uint64_t>(occ_.occ, 1)));; slots *= 2) {
    LX_REQUIRE(slots <= DM_MAX_SLOTS, "dense map: the window has more voxels than a table can index");
    DmTable().swap(nt);   // (a failed attempt's table: the host waited for it)
    nt.alloc(slots, false, true);
    nt.clear(own_);
    LX_HIP(hipMemsetAsync(nctr.p, 0, sizeof(unsigned long long) * (DM_CTR_WORDS + 1), own_));
    launch_replay_range(nt, nctr.p, d_calls.p, (uint32_t)n_calls, first, points);
    LX_HIP(hipGetLastError());
    LX_HIP(hipMemcpyAsync(w, nctr.p, sizeof(w), hipMemcpyDeviceToHost, own_));
    LX_HIP(hipStreamSynchronize(own_));
    if (!dm_rebuild_attempt_failed(slots, w[0], w[DM_CTR_WORDS], w[3])) break;
    if (cfg.max_voxels && slots / 2 >= cfg.max_voxels) return LOAMX_E_CAPACITY;   // (as a rebuild: more voxels than the handle admits)
  }
  if (cfg.max_voxels && w[0] > cfg.max_voxels) return LOAMX_E_CAPACITY;
  DmSurfelList L;
  surfel_list(nt, w[0], (double)cfg.leaf, sc, nullptr, 0.f, L);
  frozen.build_device(L.keys.p, L.rec.p, L.n, own_);
  drop_coarse();
  if (n_surfels) *n_surfels = frozen.size();
  return LOAMX_OK;
}

void DenseMap::history_source(uint64_t call, DenseSource& s) {
  LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
  LX_REQUIRE(call < hist_.calls.size(), "call is beyond the log");
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();   // (the log's points are in place, whichever stream appended them)
  const DmHistoryCall& c = hist_.calls[call];
  s.pts = log_ + c.first;
  s.n = c.count;
  s.stream = own_;
  s.device = cfg.device;
  for (int a = 0; a < 3; a++) s.origin[a] = c.origin[a];
  s.has_cloud = true;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

int loamx_densemap_freeze_device(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                 uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    const uint64_t n = h->d.freeze_device(c, checked_optional_rule(h, rule, r));
    if (n_surfels) *n_surfels = n;
    return LOAMX_OK;
  });
}

int loamx_densemap_freeze_pyramid_device(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                         const loamx_densemap_pyramid_config* pyramid, uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    const loamx_densemap_pyramid_config pc = or_default(pyramid, loamx_densemap_pyramid_default_config);
    LX_REQUIRE(pc.levels >= 1u && pc.levels <= LOAMX_PYRAMID_MAX_LEVELS, "levels must be in [1, LOAMX_PYRAMID_MAX_LEVELS]");
    LX_REQUIRE(pc.max_curvature >= 0.f, "max_curvature must be >= 0 (0: no limit)");   // (NaN too)
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    h->d.freeze_pyramid_device(c, checked_optional_rule(h, rule, r), pc, n_surfels);
    return LOAMX_OK;
  });
}

int loamx_densemap_freeze_history(loamx_densemap* h, uint64_t first_call, uint64_t n_calls, const double* corrections,
                                  const loamx_densemap_surfel_config* cfg, uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    LX_REQUIRE_MOMENTS(h);
    LX_HIP(hipSetDevice(h->d.cfg.device));
    return h->d.freeze_history(first_call, n_calls, corrections, c, n_surfels);
  });
}

int loamx_densemap_download_frozen(loamx_densemap* h, uint32_t level, uint64_t* keys, float* rec, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && ((keys && rec) || !capacity), "NULL argument");
    LX_REQUIRE(level < h->d.frozen_levels(), "level must be a level that stands (loamx_densemap_frozen_levels)");
    const DmFrozen& F = h->d.level(level);
    *n = F.size();
    if (*n > capacity) return (int)LOAMX_E_CAPACITY;
    LX_HIP(hipSetDevice(h->d.cfg.device));
    std::vector<unsigned long long> k;
    std::vector<float> r;
    F.download(k, r, h->d.own_stream());
    if (!k.empty()) {
      memcpy(keys, k.data(), sizeof(unsigned long long) * k.size());
      memcpy(rec, r.data(), sizeof(float) * r.size());
    }
    return (int)LOAMX_OK;
  });
}

}  // extern "C"
