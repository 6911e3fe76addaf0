// The dense map's sweep log and rebuild rule (densemap_rebuild.hip, and densemap.hip for the adds; include/loamx.h, loamx_densemap_enable_history / loamx_densemap_rebuild).
// Standard library only: tests/test_densemap_history_cpu.py drives it on a CPU; the two inline functions that the kernels share are
// marked for the device only under hipcc.
//
// The log is one block of float4 in HBM that the adds append to; the host keeps its capacity, its fill and one record per logged call.
// A rebuild replays the log under one rigid correction per call into a fresh table: this header turns the host's 12 doubles into the
// record the kernels read, applies a correction to a point (the one definition: host helper, kernels and the model of
// tests/densemap_rebuild_model.py agree with it to the bit) and decides which table sizes are tried.
#pragma once
#include "densemap_growth.hpp"
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define DMH_HD __host__ __device__
#else
#define DMH_HD
#endif

namespace loamx {

constexpr uint64_t DMH_POINT_BYTES = 16;   // x, y, z, w as f32

// one logged call: where its cloud starts in the log, its points, its origin as given
struct DmHistoryCall {
  uint64_t first;
  uint32_t count;
  float origin[3];
};

struct DmHistory {
  uint64_t max_points = 0;   // max_bytes / 16; 0: no cap
  uint64_t capacity = 0;     // points the block on the device holds
  uint64_t points = 0;       // points logged
  std::vector<DmHistoryCall> calls;

  // the state at enabling.  false: max_bytes is set and holds no point, or initial_points is 0
  bool configure(uint64_t max_bytes, uint64_t initial_points) {
    if (!initial_points || (max_bytes && max_bytes < DMH_POINT_BYTES)) return false;
    max_points = max_bytes / DMH_POINT_BYTES;
    capacity = max_points && initial_points > max_points ? max_points : initial_points;
    points = 0;
    calls.clear();
    return true;
  }
  // the cap rule, decided before anything is enqueued: the log may hold exactly max_points
  bool admits(uint64_t n) const { return !max_points || (n <= max_points && points <= max_points - n); }
  // the capacity the block needs before an admitted call of n points is appended: doubled until it fits, never beyond the cap
  uint64_t capacity_for(uint64_t n) const {
    uint64_t c = capacity;
    while (c < points + n && c < (1ull << 62)) c *= 2;   // (2^62 points: beyond any memory; keeps the doubling from wrapping)
    return max_points && c > max_points ? max_points : c;
  }
  // a call of n points was appended at `points`; an empty call is not logged
  void append(uint32_t n, const float origin[3]) {
    if (!n) return;
    calls.push_back(DmHistoryCall{points, n, {origin[0], origin[1], origin[2]}});
    points += n;
  }
  // reset: the log is empty, the block stays
  void clear() { points = 0; calls.clear(); }
};

// x -> R x + t in f32 without a fused multiply-add (the callers are built without contraction), m = R | t row-major 3x4
DMH_HD inline void dm_correct(const float m[12], float x, float y, float z, float out[3]) {
  out[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  out[1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  out[2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// a correction as the replay reads it: rounded to f32 once; identity: the 12 rounded entries compare equal to the identity's
struct DmCorrection {
  float m[12];
  uint32_t identity;
};
// false: an entry is not finite (out is not written).  c NULL: the identity
inline bool dm_correction_from(const double* c, DmCorrection& out) {
  static const float I[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  DmCorrection r;
  r.identity = 1u;
  for (int k = 0; k < 12; k++) {
    if (c && !std::isfinite(c[k])) return false;
    r.m[k] = c ? (float)c[k] : I[k];
    if (!(r.m[k] == I[k])) r.identity = 0u;
  }
  out = r;
  return true;
}

// the per-call record of the replay in device memory: the call's first point, its correction and its corrected origin
struct DmReplayCall {
  uint64_t first;
  float m[12];
  float o[3];
  uint32_t identity;
};
static_assert(sizeof(DmReplayCall) == 72, "8-byte aligned, no padding");
// false: the correction (NULL: the identity) has a non-finite entry
inline bool dm_replay_call(const DmHistoryCall& h, const double* c, DmReplayCall& out) {
  DmCorrection C;
  if (!dm_correction_from(c, C)) return false;
  out.first = h.first;
  for (int k = 0; k < 12; k++) out.m[k] = C.m[k];
  out.identity = C.identity;
  if (C.identity) { out.o[0] = h.origin[0]; out.o[1] = h.origin[1]; out.o[2] = h.origin[2]; }   // (the logged bytes, no arithmetic)
  else dm_correct(C.m, h.origin[0], h.origin[1], h.origin[2], out.o);
  return true;
}
// a logged point under its call's record; w is untouched
DMH_HD inline void dm_replayed(const DmReplayCall& c, float& x, float& y, float& z) {
  if (c.identity) return;
  float o[3];
  dm_correct(c.m, x, y, z, o);
  x = o[0]; y = o[1]; z = o[2];
}

// Table sizes of a rebuild.  The first table is the smallest that holds the voxels the map has now; the kernels stop inserting once
// the occupancy passes one half and say so.  All three signs of a failed attempt mean "more voxels than half the slots", so the
// sizes tried depend on the map's words alone; a failed attempt is repeated with twice the slots (the caller refuses beyond 2^31)
constexpr uint64_t DM_MAX_SLOTS = 1ull << 31;
inline uint64_t dm_rebuild_first_slots(uint64_t initial_slots, uint64_t voxels_now) { return dm_slots_for(initial_slots, voxels_now); }
inline bool dm_rebuild_attempt_failed(uint64_t slots, uint64_t occupancy, uint64_t too_small, uint64_t overflow) {
  return occupancy > slots / 2 || too_small != 0 || overflow != 0;
}

}  // namespace loamx
