// Dense map, history and rebuild (include/loamx.h: loamx_densemap_enable_history ... loamx_densemap_rebuild; densemap_history.hpp):
// every add also appends its cloud to a log in HBM, and a rebuild replays that log, each call under a rigid correction, into a fresh
// table with the insert's and the carve kernel's own bodies (dm_insert_body.inc, dm_carve_body.inc); the table that stands is replaced
// only when the replay has succeeded.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"

namespace loamx {

// Replay (include/loamx.h, loamx_densemap_rebuild): k_dm_insert and k_dm_carve (densemap.hip) over the sweep log, each point transformed in registers by
// the correction of its call.  calls: one DmReplayCall per logged call, first points ascending.  A replay goes into a fresh table
// whose size is a guess: before any probe a block reads the running occupancy, and once that has passed one half of the slots it sets
// small[0] and returns (the whole block, before the body's barriers), so a table that is too small costs bounded work and no probe
// loop ever runs in a full table for longer than its mask + 1 steps.  A replay that succeeds never took that exit in any block: the
// occupancy only grows

// true for the whole block when the table is too small; says so in small[0]
__device__ inline bool dm_replay_too_small(const unsigned long long* ctr, uint32_t mask, unsigned long long* small) {
  const unsigned long long occ = __hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!__syncthreads_or(occ > ((unsigned long long)mask + 1ull) / 2ull ? 1 : 0)) return false;
  if (threadIdx.x == 0) small[0] = 1ull;
  return true;
}
// point idx of the log under the record of its call
__device__ inline float4 dm_replay_point(const float4* __restrict__ log, unsigned long long idx, const DmReplayCall& c) {
  float4 p = log[idx];
  dm_replayed(c, p.x, p.y, p.z);
  return p;
}

// the insert of the n points from `first` on, which belong to the calls [call_lo, call_hi): one launch for the whole log when no
// word depends on the order of the calls (carving off: equal keys combine inside a wave across call boundaries, each point with the
// range filter about its own call's corrected origin), one launch per call otherwise (STAMP: the stamp is the call's index + 1).
// F0: the map's filter; its origin is not read
template <bool COMBINE, bool STAMP, bool MOMENTS>
__global__ __launch_bounds__(256) void k_dm_rebuild(const float4* __restrict__ log, unsigned long long first, unsigned long long n,
                                                    const DmReplayCall* __restrict__ calls, uint32_t call_lo, uint32_t call_hi, DmFilter F0,
                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ vals,
                                                    uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                    uint32_t* __restrict__ aux, unsigned long long* __restrict__ mom,
                                                    unsigned long long* __restrict__ small) {
  if (dm_replay_too_small(ctr, mask, small)) return;
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  DmFilter F = F0;
  float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t seq = 0u;
  if (i < n) {
    // the last call that starts at or before the point (call_lo does: the launch starts inside it)
    const unsigned long long idx = first + i;
    uint32_t lo = call_lo, hi = call_hi;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (calls[mid].first <= idx) lo = mid; else hi = mid;
    }
    const DmReplayCall& c = calls[lo];
    pt = dm_replay_point(log, idx, c);
    F.ox = c.o[0]; F.oy = c.o[1]; F.oz = c.o[2];
    seq = lo + 1u;
  }
#define DM_INSERT_HAS_POINT i < n
#define DM_INSERT_POINT pt
#include "dm_insert_body.inc"
#undef DM_INSERT_HAS_POINT
#undef DM_INSERT_POINT
}

// the rays of one call behind its insert: k_dm_carve over the n points of *call in the log, from its corrected origin
__global__ __launch_bounds__(256) void k_dm_rebuild_carve(const float4* __restrict__ log, const DmReplayCall* __restrict__ call, uint32_t n,
                                                          DmFilter F0, DmCarve R, const unsigned long long* keys, uint32_t* aux, uint32_t mask,
                                                          uint32_t shift, unsigned long long* __restrict__ ctr,
                                                          unsigned long long* __restrict__ small) {
  if (dm_replay_too_small(ctr, mask, small)) return;
  const DmReplayCall c = *call;
  DmFilter F = F0;
  F.ox = c.o[0]; F.oy = c.o[1]; F.oz = c.o[2];
#define DM_CARVE_POINT(j) dm_replay_point(log, c.first + (j), c)
#include "dm_carve_body.inc"
#undef DM_CARVE_POINT
}

// allowed while nothing has been offered; the handle is unchanged when refused
void DenseMap::enable_history(const loamx_densemap_history_config& c) {
  read_counters();
  LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "history can only be enabled on an empty map (a fresh handle, or right after reset)");
  DmHistory h;
  LX_REQUIRE(h.configure(c.max_bytes, c.initial_points), "initial_points must be >= 1, and max_bytes 0 or at least one point (16 bytes)");
  float4* nb = nullptr;
  LX_HIP(hipMalloc((void**)&nb, DMH_POINT_BYTES * h.capacity));
  (void)hipFree(log_);   // (enabled before: the log is empty and every add was waited for)
  log_ = nb;
  hist_ = h;
  history_ = true;
}

// the logged bytes of one call and its origin
int DenseMap::history_download(uint64_t call, loamx_cloud* out, float origin[3]) {
  LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
  LX_REQUIRE(call < hist_.calls.size(), "call is beyond the log");
  check_cloud(out, false);
  const DmHistoryCall c = hist_.calls[call];
  if (c.count > out->count) { out->count = c.count; return LOAMX_E_CAPACITY; }
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const float4* pts = h_sweep_.fetch(log_ + c.first, c.count, own_);
  LX_HIP(hipStreamSynchronize(own_));
  for (int a = 0; a < 3; a++) origin[a] = c.origin[a];
  return unpack_cloud(pts, c.count, out);
}

// room for n more points in the log: a block of the doubled capacity, the logged points copied over on st, the old block to the
// graveyard (earlier work may still read it)
void DenseMap::log_reserve(uint64_t n, hipStream_t st) {
  const uint64_t want = hist_.capacity_for(n);
  if (want == hist_.capacity) return;
  float4* nb = nullptr;
  LX_HIP(hipMalloc((void**)&nb, DMH_POINT_BYTES * want));
  if (hist_.points) {
    const hipError_t e = hipMemcpyAsync(nb, log_, DMH_POINT_BYTES * hist_.points, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { (void)hipFree(nb); LX_HIP(e); }
  }
  graveyard_.push_back(log_);
  log_ = nb;
  hist_.capacity = want;
}

// one attempt of a rebuild: the log under the records of d_calls_ into nt with the counter words nctr ([DM_CTR_WORDS]: too small),
// enqueued on own_ without a host wait
void DenseMap::launch_replay(const DmTable& nt, unsigned long long* nctr) {
  const uint32_t n_calls = (uint32_t)hist_.calls.size();
  const float no_origin[3] = {0.f, 0.f, 0.f};   // (each point is filtered about its own call's origin)
  const DmFilter F = filter_for(no_origin);
  unsigned long long* small = nctr + DM_CTR_WORDS;
  dm_dispatch2(combine, nt.mom != nullptr, [&](auto C, auto M) {
    constexpr bool CB = decltype(C)::value, MM = decltype(M)::value;
    if (!nt.aux) {
      const uint64_t n = hist_.points;
      hipLaunchKernelGGL((k_dm_rebuild<CB, false, MM>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, own_, log_, 0ull, n, d_calls_.p, 0u,
                         n_calls, F, nt.keys, nt.vals, nt.mask(), nt.shift(), nctr, nt.aux, nt.mom, small);
      rebuild_stats_[2]++;
      return;
    }
    for (uint32_t k = 0; k < n_calls; k++) {
      const DmHistoryCall& c = hist_.calls[k];
      const DmCarve R = carve_args(k + 1u);
      const uint64_t span = 256ull * R.stride;
      hipLaunchKernelGGL((k_dm_rebuild<CB, true, MM>), dim3((c.count + 255u) / 256u), dim3(256), 0, own_, log_, c.first,
                         (unsigned long long)c.count, d_calls_.p, k, k + 1u, F, nt.keys, nt.vals, nt.mask(), nt.shift(), nctr, nt.aux, nt.mom, small);
      hipLaunchKernelGGL(k_dm_rebuild_carve, dim3((uint32_t)((c.count + span - 1) / span)), dim3(256), 0, own_, log_, d_calls_.p + k, c.count, F,
                         R, nt.keys, nt.aux, nt.mask(), nt.shift(), nctr, small);
      rebuild_stats_[2] += 2;
    }
  });
  rebuild_stats_[3] += hist_.points;
}

// the replay of a window of the log (densemap_freeze.hip, freeze_history): the `points` points from `first` on, which belong to the
// n_calls records at d_calls, into the table nt (moment words, no carve words: one launch, no word depends on the order of the calls)
// with the counter words nctr ([DM_CTR_WORDS]: too small), enqueued on own_ without a host wait.  The rebuild's statistics stay
void DenseMap::launch_replay_range(const DmTable& nt, unsigned long long* nctr, const DmReplayCall* d_calls, uint32_t n_calls, uint64_t first,
                                   uint64_t points) {
  const float no_origin[3] = {0.f, 0.f, 0.f};   // (each point is filtered about its own call's origin)
  const DmFilter F = filter_for(no_origin);
  dm_dispatch2(combine, nt.mom != nullptr, [&](auto C, auto M) {
    hipLaunchKernelGGL((k_dm_rebuild<decltype(C)::value, false, decltype(M)::value>), dim3((uint32_t)((points + 255) / 256)), dim3(256), 0, own_,
                       log_, (unsigned long long)first, (unsigned long long)points, d_calls, 0u, n_calls, F, nt.keys, nt.vals, nt.mask(),
                       nt.shift(), nctr, (uint32_t*)nullptr, nt.mom, nctr + DM_CTR_WORDS);
  });
}

// Everything is built beside the handle (table, counter words) and swapped in at the end: a refusal or a failure on the way leaves
// the handle as it was
int DenseMap::rebuild(const double* corrections, uint64_t n_calls) {
  LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
  LX_REQUIRE(n_calls == hist_.calls.size(), "n_calls differs from the number of logged calls (loamx_densemap_history_size)");
  LX_REQUIRE((hist_.points + 255) / 256 < (1ull << 31), "the log holds more points than one launch covers");
  h_calls_.reserve(n_calls + 1);
  for (uint64_t k = 0; k < n_calls; k++)
    LX_REQUIRE(dm_replay_call(hist_.calls[k], corrections ? corrections + 12 * k : nullptr, h_calls_.p[k]),
               "corrections: the correction of call " + std::to_string(k) + " has an entry that is not finite");
  read_counters();   // (waits for the adds; the occupancy is exact)
  const uint64_t before = occ_.occ;
  const bool aux = tab_.aux != nullptr, mom = tab_.mom != nullptr;
  DevBuf<unsigned long long> nctr;
  nctr.reserve(DM_CTR_WORDS + 1);
  h_rb_.reserve(DM_CTR_WORDS + 1);
  d_calls_.reserve(n_calls + 1);
  if (n_calls) LX_HIP(hipMemcpyAsync(d_calls_.p, h_calls_.p, sizeof(DmReplayCall) * n_calls, hipMemcpyHostToDevice, own_));
  const unsigned long long* w = nullptr;   // the attempt's counter words, and [DM_CTR_WORDS]: too small
  DmTable nt;
  for (uint64_t slots = dm_rebuild_first_slots(cfg.initial_slots, before);; slots *= 2) {
    LX_REQUIRE(slots <= DM_MAX_SLOTS, "dense map: the rebuilt map has more voxels than the table can index");
    DmTable().swap(nt);   // (a failed attempt's table: the host waited for it)
    nt.alloc(slots, aux, mom);
    nt.clear(own_);
    LX_HIP(hipMemsetAsync(nctr.p, 0, sizeof(unsigned long long) * (DM_CTR_WORDS + 1), own_));
    rebuild_stats_[1]++;
    if (hist_.points) launch_replay(nt, nctr.p);
    LX_HIP(hipGetLastError());
    w = h_rb_.fetch(nctr.p, DM_CTR_WORDS + 1, own_);
    LX_HIP(hipStreamSynchronize(own_));
    if (!dm_rebuild_attempt_failed(slots, w[0], w[DM_CTR_WORDS], w[3])) break;
    if (cfg.max_voxels && slots / 2 >= cfg.max_voxels) return LOAMX_E_CAPACITY;   // (more voxels than half the slots)
  }
  if (cfg.max_voxels && w[0] > cfg.max_voxels) return LOAMX_E_CAPACITY;
  replace_table(nt);
  std::swap(ctr_.p, nctr.p);
  std::swap(ctr_.cap, nctr.cap);
  free_graveyard();   // (the host has waited: nothing reads the old table any more)
  occ_.reset();
  occ_.exact(w[0]);
  offered_ = hist_.points;
  drop_range_ = w[1]; drop_key_ = w[2];
  for (int k = 0; k < 6; k++) carve_ctr_[k] = w[4 + k];
  seq_ = aux ? (uint32_t)n_calls : 0u;
  rebuild_stats_[0]++;
  return LOAMX_OK;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_history_default_config(loamx_densemap_history_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_bytes = 0;
  cfg->initial_points = 1ull << 20;
}
int loamx_densemap_enable_history(loamx_densemap* h, const loamx_densemap_history_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    h->d.enable_history(or_default(cfg, loamx_densemap_history_default_config));
    return LOAMX_OK;
  });
}
int loamx_densemap_history_size(loamx_densemap* h, uint64_t* calls, uint64_t* points) {
  return guard([&]() {
    LX_REQUIRE(h && calls && points, "NULL argument");
    LX_REQUIRE(h->d.history(), "history is not enabled (loamx_densemap_enable_history)");
    h->d.history_size(calls, points);
    return LOAMX_OK;
  });
}
int loamx_densemap_history_download(loamx_densemap* h, uint64_t call, loamx_cloud* out, float origin[3]) {
  return guard([&]() {
    LX_REQUIRE(h && out && origin, "NULL argument");
    return h->d.history_download(call, out, origin);
  });
}
int loamx_densemap_correct(const double correction[12], const float* xyz_in, float* xyz_out, uint64_t n) {
  return guard([&]() {
    LX_REQUIRE(correction, "correction is NULL");
    LX_REQUIRE((xyz_in && xyz_out) || !n, "xyz_in or xyz_out is NULL");
    DmCorrection c;
    LX_REQUIRE(dm_correction_from(correction, c), "correction has an entry that is not finite");
    if (c.identity) {
      if (n && xyz_out != xyz_in) memmove(xyz_out, xyz_in, sizeof(float) * 3 * n);
      return LOAMX_OK;
    }
    for (uint64_t i = 0; i < n; i++) {
      float o[3];
      dm_correct(c.m, xyz_in[3 * i], xyz_in[3 * i + 1], xyz_in[3 * i + 2], o);
      xyz_out[3 * i] = o[0]; xyz_out[3 * i + 1] = o[1]; xyz_out[3 * i + 2] = o[2];
    }
    return LOAMX_OK;
  });
}
int loamx_densemap_rebuild(loamx_densemap* h, const double* corrections, uint64_t n_calls) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_HIP(hipSetDevice(h->d.cfg.device));
    return h->d.rebuild(corrections, n_calls);
  });
}
int loamx_densemap_get_rebuild_stats(loamx_densemap* h, uint64_t stats[4]) {
  return guard([&]() {
    LX_REQUIRE(h && stats, "NULL argument");
    h->d.rebuild_stats(stats);
    return LOAMX_OK;
  });
}

}  // extern "C"
