// Dense global map (densemap.hpp, include/loamx.h loamx_densemap_*): registered sweeps accumulated into a voxel hash table in HBM.
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
//
// Freeze (loamx_densemap_freeze): the surfels of that export, computed once, go into a second table on the device that the alignment
// of densemap_align.hip reads; the table above never learns of it.
//
// History (loamx_densemap_enable_history, densemap_history.hpp): every add also appends its cloud to a log in HBM, and
// loamx_densemap_rebuild replays that log, each call under a rigid correction, into a fresh table with the insert's and the carve
// kernel's own bodies (dm_insert_body.inc, dm_carve_body.inc); the table that stands is replaced only when the replay has succeeded.
//
// Navigation grid (loamx_densemap_grid, densemap_grid.hip): a window of the table projected to 2-D cells by kernels of their own that
// only read it; the handle owns their planes.
//
// Routing (loamx_densemap_route ..., densemap_route.hip): the cost-to-go field of that grid towards goal cells, on the records where
// the grid's kernels leave them, and routes traced over it; planes of their own, allocated by the first route call.
#include "densemap.hpp"
#include "densemap_file.hpp"
#include "densemap_history.hpp"
#include "host_math.h"
#include "pinned_copy.hpp"
#include "scan.hpp"
#include <algorithm>
#include <numeric>
#include <type_traits>

namespace loamx {

struct DmFilter {
  float inv, min2, max2;
  int use_max;
  float ox, oy, oz;
};

// counters: [0] occupied slots, [1] dropped by range, [2] dropped outside the key range, [3] probe overflow (never set while the host's
// load rule holds: a guard against hanging the device, reported by the next reading call); carving: [4] rays traced, not traced by
// [5] stride, [6] range, [7] step count or origin key, [8] cells visited, [9] misses recorded
constexpr int DM_CTR_WORDS = 10;

// what the ray kernel needs beyond the insert's filter (include/loamx.h, loamx_densemap_carve_config)
struct DmCarve {
  float max2;
  int use_max;
  uint32_t stride, end_margin, max_steps, seq;
};
// aux: 2 words per slot beside the table, [2 * slot] miss, [2 * slot + 1] stamp
// mom: DM_MOM_WORDS per slot beside the table, [9 * slot + k]: Mxx, Myy, Mzz, Mxy, Mxz, Myz, Vx, Vy, Vz (include/loamx.h)
constexpr int DM_VBITS = 26;   // the combine packs a lane's w_a above its q_a: 64 lanes' q sum stays below 2^26

// the slot of `key` (claimed when absent); won: this call claimed it.  false: the table is full (cannot happen at a load <= 1/2)
__device__ inline bool dm_find_or_claim(unsigned long long* __restrict__ keys, uint32_t mask, uint32_t shift, unsigned long long key,
                                        uint32_t& slot, bool& won) {
  uint32_t h = (uint32_t)dm_hash(key, shift);
  won = false;
  for (uint32_t probe = 0; probe <= mask; probe++) {
    // (a stale EMPTY from another XCD's L2 only costs the CAS below: a slot's key is written once, by the CAS that claims it)
    unsigned long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == DM_EMPTY) {
      cur = atomicCAS(&keys[h], DM_EMPTY, key);
      if (cur == DM_EMPTY) { won = true; slot = h; return true; }
    }
    if (cur == key) { slot = h; return true; }
    h = (h + 1u) & mask;
  }
  return false;
}

// wave-aggregated add of this lane's `c` to a 64-bit counter
__device__ inline void dm_wave_count(unsigned long long* ctr, bool c) {
  const unsigned long long m = __ballot(c);
  if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(ctr, (unsigned long long)__popcll(m));
}
// the same for a count per lane (the wave's sum must fit 32 bits)
__device__ inline void dm_wave_sum(unsigned long long* ctr, uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  if (v && (threadIdx.x & 63) == 0) atomicAdd(ctr, (unsigned long long)v);
}

// the key rule of a point: its cell's indices stay inside the key (a NaN or an infinite component fails it too)
__device__ inline bool dm_in_key_range(const float4 p, float inv) {
  return fabsf(floorf(p.x * inv)) < DM_IMAX && fabsf(floorf(p.y * inv)) < DM_IMAX && fabsf(floorf(p.z * inv)) < DM_IMAX;
}

// true when the insert adds p (its range filter and key rule, the same expressions); d2 as the insert computes it
__device__ inline bool dm_added(const float4 p, const DmFilter& F, float& d2) {
  const float dx = p.x - F.ox, dy = p.y - F.oy, dz = p.z - F.oz;
  d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 >= F.min2 && (!F.use_max || d2 <= F.max2))) return false;
  return dm_in_key_range(p, F.inv);
}

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

// One axis of the voxel walk (include/loamx.h): the origin's and the point's cell, the cells between them, and the ray parameter at
// which the walk next leaves its cell along this axis.  Voxel units, f32, no fused multiply-add (the file is built without contraction).
struct DmAxis {
  int c, s;
  uint32_t rem;
  float tmax, tdelta;
};
__device__ inline bool dm_axis_setup(float o, float p, float inv, DmAxis& A) {
  const float so = o * inv, sp = p * inv;
  const float fo = floorf(so);
  A.c = 0; A.s = 0; A.rem = 0u; A.tmax = 0.f; A.tdelta = 0.f;
  if (!(fabsf(fo) < DM_IMAX)) return false;   // the origin's cell fails the key rule (NaN too)
  const int c0 = (int)fo, c1 = (int)floorf(sp);   // (the point was added: |c1| < 2^20)
  A.c = c0;
  A.s = c1 > c0 ? 1 : (c1 < c0 ? -1 : 0);
  A.rem = (uint32_t)(c1 > c0 ? c1 - c0 : c0 - c1);
  if (A.rem) {
    const float d = sp - so;   // (not 0: the floors differ)
    const float b = (float)(c0 + (A.s > 0 ? 1 : 0));
    A.tmax = (b - so) / d;
    A.tdelta = 1.0f / fabsf(d);
  }
  return true;
}
__device__ inline void dm_axis_step(DmAxis& A) {
  A.c += A.s;
  A.rem -= 1u;
  A.tmax = A.tmax + A.tdelta;
}

// (Both ray kernels write out the three dm_axis_setup calls and the n_steps sum.  A function around them — a struct of the three axes
// with a setup member, or a free function over three DmAxis in any of four shapes — inlines to the same instructions in another order
// in both kernels, so the one-object comparison with the kernels as they stood no longer holds; the walk's step and the key are shared.)
// one step of the walk: the axis with the smallest tmax among those with cells left moves, ties to the lower axis.  The caller has
// cells left on some axis
__device__ inline void dm_walk_step(DmAxis& X, DmAxis& Y, DmAxis& Z) {
  int ax = -1;
  float tb = 0.f;
  if (X.rem) { ax = 0; tb = X.tmax; }
  if (Y.rem && (ax < 0 || Y.tmax < tb)) { ax = 1; tb = Y.tmax; }
  if (Z.rem && (ax < 0 || Z.tmax < tb)) { ax = 2; tb = Z.tmax; }
  if (ax == 0) dm_axis_step(X);
  else if (ax == 1) dm_axis_step(Y);
  else dm_axis_step(Z);
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

// Replay (include/loamx.h, loamx_densemap_rebuild): the two kernels above over the sweep log, each point transformed in registers by
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

// what a ray cast needs (include/loamx.h, loamx_densemap_raycast): the origin, the checked configuration and, with use_rule, the rule
struct DmCast {
  float inv, ox, oy, oz;
  double leaf;
  uint32_t max_steps, skip_steps, min_points;
  int use_rule;
  loamx_densemap_static_rule rule;
};

// First hit along a ray (include/loamx.h, loamx_densemap_raycast): one ray per lane, from the origin to pts[i], the walk of k_dm_carve
// with the end cell included.  The table is only read: a cell costs one dm_find, a found key one read of its n (and, with a rule, of
// its miss word); the position, in double as the export computes it, and the range are computed once, for the hit, and the record
// leaves as one 40-byte store per lane.  A wave runs as long as its longest ray and stops probing for the lanes that have hit: the
// rays of a sweep or of a range image are neighbours in direction, so the lanes of a wave hit after similar step counts, and the
// other waves of the CU hide the latency of the dependent probes as they do for the carve kernel.  Every loop is bounded by an
// integer: n_steps <= max_steps <= 65536, mask + 1 probes.  rc: [0] not traced, [1] miss, [2] hit, [3] hit in the end cell,
// [4] cells looked up; ctr[3]: the probe-overflow flag of the map's counters
__global__ __launch_bounds__(256) void k_dm_raycast(const float4* __restrict__ pts, uint32_t n, DmCast C, const unsigned long long* keys,
                                                    const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                    uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                    unsigned long long* __restrict__ rc, loamx_ray_hit* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  loamx_ray_hit r;
  r.key = 0ull;
  r.x = r.y = r.z = r.range = 0.f;
  r.n = r.miss = r.steps = 0u;
  r.status = 0u;
  uint32_t looked = 0u;
  bool overflow = false;
  if (i < n) {
    const float4 p = pts[i];
    if (dm_in_key_range(p, C.inv)) {   // (the end's cell)
      DmAxis X, Y, Z;
      const bool okx = dm_axis_setup(C.ox, p.x, C.inv, X), oky = dm_axis_setup(C.oy, p.y, C.inv, Y), okz = dm_axis_setup(C.oz, p.z, C.inv, Z);
      const uint32_t n_steps = X.rem + Y.rem + Z.rem;   // (each < 2^21)
      if (okx && oky && okz && n_steps <= C.max_steps) {
        r.status = 1u;
        // cells k = skip_steps .. n_steps are looked up; cell k is the cell after k steps
        if (C.skip_steps <= n_steps) {
          for (uint32_t k = 0; k <= n_steps; k++) {
            if (k >= C.skip_steps) {
              const unsigned long long key = dm_key(X.c, Y.c, Z.c);
              uint32_t slot = 0u;
              const int f = dm_find(keys, mask, shift, key, slot);
              looked++;
              if (f < 0) overflow = true;
              if (f > 0) {
                const unsigned long long* v = vals + 4ull * slot;
                const unsigned long long cnt = v[0];
                if (cnt >= C.min_points && !(C.use_rule && dm_dynamic(C.rule, cnt, aux[2ull * slot]))) {
                  const double den = (double)cnt * 1048576.0;
                  r.key = key;
                  r.x = (float)(((double)X.c + (double)v[1] / den) * C.leaf);
                  r.y = (float)(((double)Y.c + (double)v[2] / den) * C.leaf);
                  r.z = (float)(((double)Z.c + (double)v[3] / den) * C.leaf);
                  const float dx = p.x - C.ox, dy = p.y - C.oy, dz = p.z - C.oz;
                  const float ex = r.x - C.ox, ey = r.y - C.oy, ez = r.z - C.oz;
                  const float l2 = (dx * dx + dy * dy) + dz * dz;
                  r.range = l2 == 0.f ? 0.f : ((dx * ex + dy * ey) + dz * ez) / sqrtf(l2);
                  r.n = cnt > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt;
                  r.miss = aux ? aux[2ull * slot] : 0u;
                  r.steps = k;
                  r.status = k < n_steps ? 2u : 3u;
                  break;
                }
              }
            }
            if (k == n_steps) break;
            dm_walk_step(X, Y, Z);   // (k < n_steps: some axis has cells left)
          }
        }
        if (r.status == 1u) r.steps = looked;
      }
    }
    if (out) out[i] = r;
  }
  if (overflow) ctr[3] = 1ull;
  dm_wave_count(&rc[0], i < n && r.status == 0u);
  dm_wave_count(&rc[1], r.status == 1u);
  dm_wave_count(&rc[2], r.status == 2u);
  dm_wave_count(&rc[3], r.status == 3u);
  dm_wave_sum(&rc[4], looked);
}

// every occupied slot of the old table into the new one (keys are unique: claim the first empty slot of the probe sequence).  AUX: the
// slot's miss and stamp words travel with it.  PRUNE (with AUX): the voxels the rule calls dynamic stay behind, and the survivors are
// counted into ctr[0] (zeroed before the launch).  MOM: the slot's nine moment words travel with it
template <bool AUX, bool PRUNE, bool MOM>
__global__ __launch_bounds__(256) void k_dm_rehash(const unsigned long long* __restrict__ okeys, const unsigned long long* __restrict__ ovals,
                                                   uint32_t on, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ vals,
                                                   uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                   const uint32_t* __restrict__ oaux, uint32_t* __restrict__ aux, loamx_densemap_static_rule rule,
                                                   const unsigned long long* __restrict__ omom, unsigned long long* __restrict__ mom) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < on ? okeys[i] : DM_EMPTY;
  bool live = key != DM_EMPTY;
  if (PRUNE && live) live = !dm_dynamic(rule, ovals[4ull * i], oaux[2ull * i]);
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
  if (PRUNE) dm_wave_count(&ctr[0], won);
}

// the statistics a merge adds to dst's counters: [0] dropped by range, [1] dropped outside the key range, [2..8) the six of carving
struct DmCtrAdd {
  unsigned long long v[8];
};

// Merge (include/loamx.h, loamx_densemap_merge / merge_file): every record of a source is added into the live table, its voxel claimed
// when absent.  The source is another map's table (sn slots, the DM_EMPTY ones skipped, miss at smiss[2 * i]: miss_stride 2) or the
// compact arrays of a file (sn records, miss_stride 1).  AUX: the miss word is added too, the stamp of dst stays (0 in a fresh slot: the
// words beside a free slot are zero).  MOM: the nine moment words.
// Only the key claim is atomic.  The keys of one source are unique, so within the launch one thread at most holds a given slot of
// dst, and nothing else writes dst meanwhile: the launch runs on dst's stream behind its adds, and the host waits for it before it
// returns.  The up to 14 value words are therefore plain loads, integer adds and plain stores (16 bytes at a time for n, Sx, Sy, Sz;
// the 72-byte moment rows are only 8-byte aligned) instead of 14 atomics that each make a trip to the memory side; a slot the CAS
// has just claimed reads as the zeros that the memset of an earlier launch left there.  Integer adds modulo 2^64 (miss: 2^32); no floating point anywhere.
// ctr[0] counts the slots claimed, as the insert does; ctr[3] reports a probe loop that ran out.  The first thread also adds the
// source's statistics to dst's counters
template <bool AUX, bool MOM>
__global__ __launch_bounds__(256) void k_dm_merge(const unsigned long long* __restrict__ skeys, const unsigned long long* __restrict__ svals,
                                                  uint32_t sn, const uint32_t* __restrict__ smiss, uint32_t miss_stride,
                                                  const unsigned long long* __restrict__ smom, unsigned long long* __restrict__ keys,
                                                  unsigned long long* __restrict__ vals, uint32_t mask, uint32_t shift,
                                                  unsigned long long* __restrict__ ctr, uint32_t* __restrict__ aux,
                                                  unsigned long long* __restrict__ mom, DmCtrAdd add) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < sn ? skeys[i] : DM_EMPTY;
  const bool live = key != DM_EMPTY;
  uint32_t slot = 0;
  bool won = false, ok = true;
  if (live) ok = dm_find_or_claim(keys, mask, shift, key, slot, won);
  dm_wave_count(&ctr[0], won);
  if (live && !ok) ctr[3] = 1ull;
  if (live && ok) {
    const ulonglong2* s = (const ulonglong2*)(svals + 4ull * i);
    ulonglong2* d = (ulonglong2*)(vals + 4ull * slot);
    const ulonglong2 s0 = s[0], s1 = s[1];
    ulonglong2 d0 = d[0], d1 = d[1];
    d0.x += s0.x; d0.y += s0.y; d1.x += s1.x; d1.y += s1.y;
    d[0] = d0;
    d[1] = d1;
    if (AUX) aux[2ull * slot] += smiss[(unsigned long long)miss_stride * i];
    if (MOM) {
      const unsigned long long* ms = smom + (unsigned long long)DM_MOM_WORDS * i;
      unsigned long long* md = mom + (unsigned long long)DM_MOM_WORDS * slot;
#pragma unroll
      for (int k = 0; k < DM_MOM_WORDS; k++) md[k] += ms[k];
    }
  }
  if (i == 0) {
    if (add.v[0]) atomicAdd(&ctr[1], add.v[0]);
    if (add.v[1]) atomicAdd(&ctr[2], add.v[1]);
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (add.v[2 + k]) atomicAdd(&ctr[4 + k], add.v[2 + k]);
  }
}

// compaction of the occupied slots in slot order: occupied slots per 256-slot block (ballot), then (behind an exclusive scan of those
// counts) each block writes its keys and values at its offset
__global__ __launch_bounds__(256) void k_dm_count(const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t* __restrict__ blk) {
  __shared__ uint32_t wc[4];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long m = __ballot(i < slots && keys[i] != DM_EMPTY);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// (AUX: the slot's miss word too; MOM: its nine moment words)
template <bool AUX, bool MOM>
__global__ __launch_bounds__(256) void k_dm_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                    uint32_t slots, const uint32_t* __restrict__ blk_off, unsigned long long* __restrict__ okeys,
                                                    unsigned long long* __restrict__ ovals, const uint32_t* __restrict__ aux,
                                                    uint32_t* __restrict__ omiss, const unsigned long long* __restrict__ mom,
                                                    unsigned long long* __restrict__ omom) {
  __shared__ uint32_t wc[4];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  const bool occ = i < slots && keys[i] != DM_EMPTY;
  const unsigned long long m = __ballot(occ);
  if (lane == 0) wc[wid] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!occ) return;
  uint32_t pos = blk_off[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wid; w++) pos += wc[w];
  okeys[pos] = keys[i];
  const ulonglong2* s = (const ulonglong2*)(vals + 4ull * i);
  ulonglong2* d = (ulonglong2*)(ovals + 4ull * pos);
  d[0] = s[0];
  d[1] = s[1];
  if (AUX) omiss[pos] = aux[2ull * i];
  if (MOM) {
    const unsigned long long* ms = mom + (unsigned long long)DM_MOM_WORDS * i;
    unsigned long long* md = omom + (unsigned long long)DM_MOM_WORDS * pos;
#pragma unroll
    for (int k = 0; k < DM_MOM_WORDS; k++) md[k] = ms[k];
  }
}

// the exported position of a voxel (include/loamx.h): its indices and its words n, Sx, Sy, Sz; f64 arithmetic, one f32 rounding
static void dm_position(double leaf, const long long ia[3], const unsigned long long* v4, float out[3]) {
  const double cnt = (double)v4[0], qs = (double)(1u << DM_QBITS);
  for (int a = 0; a < 3; a++) out[a] = (float)(((double)ia[a] + (double)v4[1 + a] / (cnt * qs)) * leaf);
}

// the surfel of a voxel (include/loamx.h): the scatter n*M_ab - S_a*S_b as an exact integer, the rest in double
static void dm_surfel(double leaf, const long long ia[3], const unsigned long long* v4, const unsigned long long* m9,
                      const loamx_densemap_surfel_config& c, int axes, loamx_surfel& out) {
  typedef __int128 i128;
  float p[3];
  dm_position(leaf, ia, v4, p);
  double nrm[3] = {0.0, 0.0, 0.0}, curv = 0.0;
  const unsigned long long n = v4[0];
  static const int A[6] = {0, 1, 2, 0, 0, 1}, B[6] = {0, 1, 2, 1, 2, 2};   // Mxx, Myy, Mzz, Mxy, Mxz, Myz
  i128 N[6];
  for (int k = 0; k < 6; k++) N[k] = (i128)n * (i128)m9[k] - (i128)v4[1 + A[k]] * (i128)v4[1 + B[k]];
  if (n >= c.min_points && N[0] + N[1] + N[2] > 0) {
    const double nn = (double)n * (double)n;
    double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, w[3], v[3][3];
    for (int k = 0; k < 6; k++) a[A[k]][B[k]] = a[B[k]][A[k]] = (double)N[k] / nn;
    jacobi_eig3(a, w, v);
    if (w[1] >= (double)c.min_planar_ratio * w[2]) {
      const double e[3] = {v[0][0], v[1][0], v[2][0]};
      const double dot = (e[0] * (double)(long long)m9[6] + e[1] * (double)(long long)m9[7]) + e[2] * (double)(long long)m9[8];
      bool flip = dot > 0.0;
      if (dot == 0.0) {
        const double first = e[0] != 0.0 ? e[0] : (e[1] != 0.0 ? e[1] : e[2]);
        flip = first < 0.0;
      }
      for (int k = 0; k < 3; k++) nrm[k] = (flip ? -e[k] : e[k]) + 0.0;   // (+ 0.0: no negative zero in the output)
      curv = w[0] / ((w[0] + w[1]) + w[2]);
    }
  }
  const int o[3] = {axes == 1 ? 2 : 0, axes == 1 ? 0 : 1, axes == 1 ? 1 : 2};   // (sensor axes: x_s = z, y_s = x, z_s = y)
  out.x = p[o[0]]; out.y = p[o[1]]; out.z = p[o[2]];
  out.intensity = (float)(double)n;
  out.normal_x = (float)nrm[o[0]]; out.normal_y = (float)nrm[o[1]]; out.normal_z = (float)nrm[o[2]];
  out.curvature = (float)curv;
}

// two runtime booleans as the two std::bool_constant arguments of f: the kernels' feature switches are template parameters
template <class F> static void dm_dispatch2(bool a, bool b, F&& f) {
  if (a) { if (b) f(std::true_type(), std::true_type()); else f(std::true_type(), std::false_type()); }
  else { if (b) f(std::false_type(), std::true_type()); else f(std::false_type(), std::false_type()); }
}

class DenseMap {
 public:
  explicit DenseMap(const loamx_densemap_config& c) : cfg(c) {
    select_device(cfg.device);
    LX_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    LX_HIP(hipEventCreateWithFlags(&ev_last_, hipEventDisableTiming));
    LX_HIP(hipEventCreateWithFlags(&ev_snap_, hipEventDisableTiming));
    LX_HIP(hipEventCreateWithFlags(&ev_staged_, hipEventDisableTiming));
    ctr_.reserve(DM_CTR_WORDS);
    h_ctr_.reserve(2 * DM_CTR_WORDS);
    h_snap_.reserve(2);
    inv_ = 1.0f / cfg.leaf;
    tab_.alloc(cfg.initial_slots, false, false);
    clear(own_);
    LX_HIP(hipStreamSynchronize(own_));
  }
  ~DenseMap() {
    (void)hipSetDevice(cfg.device);
    if (last_st_) (void)hipEventSynchronize(ev_last_);
    (void)hipStreamSynchronize(own_);
    free_graveyard();
    (void)hipFree(log_);
    DmTable().swap(tab_);
    (void)hipEventDestroy(ev_last_);
    (void)hipEventDestroy(ev_snap_);
    (void)hipEventDestroy(ev_staged_);
    (void)hipStreamDestroy(own_);
  }
  loamx_densemap_config cfg;

  int add_host(const loamx_cloud* c, const float origin[3]) {
    check_cloud(c, false);
    LX_HIP(hipSetDevice(cfg.device));
    const uint32_t n = c->count;
    if (!admit(n) || !hist_.admits(n)) return LOAMX_E_CAPACITY;
    if (!n) return LOAMX_OK;
    if (staged_pending_) { LX_HIP(hipEventSynchronize(ev_staged_)); staged_pending_ = false; }   // (the staging block is still being read)
    h_stage_.reserve(n);
    pack_cloud(c, h_stage_.p);
    d_stage_.reserve(n);
    order_behind(own_);
    fetch_from_pinned(d_stage_.p, h_stage_.p, n, own_);
    LX_HIP(hipEventRecord(ev_staged_, own_));
    staged_pending_ = true;
    enqueue_add(d_stage_.p, n, origin, own_);
    return LOAMX_OK;
  }

  int add_device(const DenseSource& s) {
    LX_REQUIRE(s.device == cfg.device, "the dense map and its source live on different devices");
    if (!s.has_cloud) return LOAMX_SKIPPED;
    LX_HIP(hipSetDevice(cfg.device));
    if (!admit(s.n) || !hist_.admits(s.n)) return LOAMX_E_CAPACITY;
    order_behind(s.stream);
    enqueue_add(s.pts, s.n, s.origin, s.stream);
    return LOAMX_OK;
  }

  // [voxels, slots, offered, added, dropped by range, dropped by key]
  void stats(uint64_t out[6]) {
    read_counters();
    out[0] = occ_.occ; out[1] = tab_.slots; out[2] = offered_;
    out[3] = offered_ - drop_range_ - drop_key_; out[4] = drop_range_; out[5] = drop_key_;
  }

  // the occupied slots on the host: keys, values, (carving) miss words and (on request, moments) the nine moment words, and idx =
  // their ascending key order
  struct Snapshot {
    std::vector<unsigned long long> k, v, mom;
    std::vector<uint32_t> miss, idx;
  };
  void snapshot(Snapshot& S, bool want_mom = false) {
    read_counters();
    const DmTable& T = tab_;
    const uint64_t occ = occ_.occ;
    const uint32_t nblk = (T.slots + 255) / 256;
    DevBuf<uint32_t> blk, scratch, omiss;
    DevBuf<unsigned long long> tiles, okeys, ovals, omom;
    blk.reserve((size_t)nblk + 1);
    scratch.reserve(2);
    tiles.reserve(SCAN_SCRATCH_WORDS / 2);
    okeys.reserve(occ + 1);
    ovals.reserve(4 * (occ + 1));
    if (T.aux) omiss.reserve(occ + 1);
    if (want_mom) omom.reserve(DM_MOM_WORDS * (occ + 1));
    LX_HIP(hipMemsetAsync(tiles.p, 0, sizeof(unsigned long long) * (SCAN_SCRATCH_WORDS / 2), own_));
    hipLaunchKernelGGL(k_dm_count, dim3(nblk), dim3(256), 0, own_, T.keys, T.slots, blk.p);
    exclusive_scan_u32_n(blk.p, blk.p, (uint32_t*)tiles.p, scratch.p, nblk, own_);
    dm_dispatch2(T.aux != nullptr, want_mom, [&](auto A, auto M) {   // (an array that is off is not read: omiss.p, omom.p are NULL then)
      hipLaunchKernelGGL((k_dm_compact<decltype(A)::value, decltype(M)::value>), dim3(nblk), dim3(256), 0, own_, T.keys, T.vals, T.slots, blk.p,
                         okeys.p, ovals.p, T.aux, omiss.p, T.mom, omom.p);
    });
    LX_HIP(hipGetLastError());
    S.k.resize(occ);
    S.v.resize(4 * (size_t)occ);
    S.miss.assign(T.aux ? occ : 0, 0u);
    S.mom.resize(want_mom ? DM_MOM_WORDS * (size_t)occ : 0);
    uint32_t total = 0;
    LX_HIP(hipMemcpyAsync(&total, blk.p + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, own_));
    if (occ) {
      LX_HIP(hipMemcpyAsync(S.k.data(), okeys.p, sizeof(unsigned long long) * occ, hipMemcpyDeviceToHost, own_));
      LX_HIP(hipMemcpyAsync(S.v.data(), ovals.p, sizeof(unsigned long long) * 4 * occ, hipMemcpyDeviceToHost, own_));
      if (T.aux) LX_HIP(hipMemcpyAsync(S.miss.data(), omiss.p, sizeof(uint32_t) * occ, hipMemcpyDeviceToHost, own_));
      if (want_mom)
        LX_HIP(hipMemcpyAsync(S.mom.data(), omom.p, sizeof(unsigned long long) * DM_MOM_WORDS * occ, hipMemcpyDeviceToHost, own_));
    }
    LX_HIP(hipStreamSynchronize(own_));
    scan_check_errors();
    LX_REQUIRE(total == occ, "dense map: the compaction disagrees with the occupancy count");
    S.idx.resize(occ);
    std::iota(S.idx.begin(), S.idx.end(), 0u);
    std::sort(S.idx.begin(), S.idx.end(), [&](uint32_t a, uint32_t b) { return S.k[a] < S.k[b]; });
  }
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

  // the voxels as records (axes 0: LOAM frame, 1: sensor axes), ascending key order; with a rule, without the voxels it calls dynamic
  void records(std::vector<float4>& out, int axes, const loamx_densemap_static_rule* rule = nullptr) {
    Snapshot S;
    snapshot(S);
    out.clear();
    out.reserve(S.idx.size());
    const double leaf = (double)cfg.leaf;
    for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
      const double cnt = (double)S.v[4 * j];
      float v[3];
      dm_position(leaf, ia, &S.v[4 * j], v);
      out.push_back(axes == 1 ? make_float4(v[2], v[0], v[1], (float)cnt) : make_float4(v[0], v[1], v[2], (float)cnt));
    });
  }

  bool moments() const { return tab_.mom != nullptr; }

  // allowed while nothing has been offered since creation / reset; the handle is unchanged when refused
  void enable_moments() {
    read_counters();
    LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "moments can only be enabled on an empty map (a fresh handle, or right after reset)");
    if (!tab_.mom) {   // (no new table: the empty one that stands gets the array, zeroed like the rest of it)
      tab_.add_mom();
      tab_.clear_mom(own_);
      LX_HIP(hipStreamSynchronize(own_));
    }
  }

  // the nine moment words per voxel in the order of records()
  void moment_words(std::vector<unsigned long long>& out) {
    Snapshot S;
    snapshot(S, true);
    out.clear();
    out.reserve(DM_MOM_WORDS * S.idx.size());
    for_each_voxel(S, nullptr, [&](size_t j, const long long*) { out.insert(out.end(), &S.mom[DM_MOM_WORDS * j], &S.mom[DM_MOM_WORDS * j] + DM_MOM_WORDS); });
  }

  // the voxels as surfels in the order of records(); with a rule, without the voxels it calls dynamic
  void surfels(std::vector<loamx_surfel>& out, int axes, const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule) {
    Snapshot S;
    snapshot(S, true);
    out.clear();
    out.reserve(S.idx.size());
    const double leaf = (double)cfg.leaf;
    for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
      loamx_surfel s;
      dm_surfel(leaf, ia, &S.v[4 * j], &S.mom[DM_MOM_WORDS * j], sc, axes, s);
      out.push_back(s);
    });
  }

  // the snapshot the alignment reads (densemap_align.hip): the voxels that have a surfel and that the rule does not call dynamic, each
  // under its key of the table, with the six f32 of its record as surfels() gives them in axes 0.  Replaces an earlier snapshot
  uint64_t freeze(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule) {
    Snapshot S;
    snapshot(S, true);
    std::vector<unsigned long long> keys;
    std::vector<float> rec;
    const double leaf = (double)cfg.leaf;
    for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
      loamx_surfel s;
      dm_surfel(leaf, ia, &S.v[4 * j], &S.mom[DM_MOM_WORDS * j], sc, 0, s);
      if (s.normal_x == 0.f && s.normal_y == 0.f && s.normal_z == 0.f) return;
      keys.push_back(S.k[j]);
      const float six[6] = {s.x, s.y, s.z, s.normal_x, s.normal_y, s.normal_z};
      rec.insert(rec.end(), six, six + 6);
    });
    frozen.build(keys.data(), rec.data(), keys.size(), own_);
    return frozen.size();
  }
  DmFrozen frozen;
  hipStream_t own_stream() const { return own_; }

  // the miss word per voxel in the order of records()
  void misses(std::vector<uint32_t>& out) {
    Snapshot S;
    snapshot(S);
    out.clear();
    out.reserve(S.idx.size());
    for_each_voxel(S, nullptr, [&](size_t j, const long long*) { out.push_back(S.miss[j]); });
  }

  bool carving() const { return tab_.aux != nullptr; }

  // allowed while nothing has been offered since creation / reset; the handle is unchanged when refused
  void enable_carving(const loamx_densemap_carve_config& c) {
    read_counters();
    LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "carving can only be enabled on an empty map (a fresh handle, or right after reset)");
    if (!tab_.aux) {   // (as in enable_moments)
      tab_.add_aux();
      tab_.clear_aux(own_);
      LX_HIP(hipStreamSynchronize(own_));
    }
    carve_ = c;
  }

  // [rays traced, not traced by stride, by range, by steps or origin key, cells visited, misses recorded]
  void carve_stats(uint64_t out[6]) {
    read_counters();
    for (int k = 0; k < 6; k++) out[k] = carve_ctr_[k];
  }

  // the dynamic voxels leave the table: a rehash with the rule as predicate into a fresh table of the same size
  uint64_t prune(const loamx_densemap_static_rule& rule) {
    read_counters();
    const uint64_t before = occ_.occ;
    DmTable nt;
    nt.alloc(tab_.slots, true, tab_.mom != nullptr);   // (aux whatever the map has: the callers require carving)
    nt.clear(own_);
    LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long), own_));   // (the occupancy: recounted by the kernel)
    launch_rehash<true>(own_, nt, rule);
    LX_HIP(hipGetLastError());
    replace_table(nt);
    read_counters();
    return before - occ_.occ;
  }

  void reset() {
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    clear(own_);
    LX_HIP(hipStreamSynchronize(own_));
    frozen.drop();
    occ_.reset();
    offered_ = drop_range_ = drop_key_ = 0;
    for (uint64_t& c : carve_ctr_) c = 0;
    seq_ = 0;
    hist_.clear();
  }

  // the features of the handle as the file's flags
  uint32_t flags() const { return (tab_.aux ? DMF_CARVING : 0u) | (tab_.mom ? DMF_MOMENTS : 0u); }

  // include/loamx.h, loamx_densemap_save: the records of snapshot() in ascending key order, with the statistics
  void save(const char* path) {
    Snapshot S;
    const bool aux = carving(), mom = moments();
    snapshot(S, mom);
    const size_t n = S.idx.size();
    DmFileHeader H;
    H.flags = flags();
    H.leaf = cfg.leaf;
    H.count = n;
    H.offered = offered_; H.dropped_range = drop_range_; H.dropped_key = drop_key_;
    if (aux) {
      for (int k = 0; k < 6; k++) H.carve_stats[k] = carve_ctr_[k];
      H.carve_max_range = carve_.max_range;
      H.ray_stride = carve_.ray_stride; H.end_margin = carve_.end_margin; H.max_steps = carve_.max_steps;
    }
    std::vector<uint64_t> k, v, m;
    std::vector<uint32_t> ms;
    k.reserve(n);
    v.reserve(4 * n);
    for_each_voxel(S, nullptr, [&](size_t j, const long long*) {
      k.push_back(S.k[j]);
      v.insert(v.end(), &S.v[4 * j], &S.v[4 * j] + 4);
      if (aux) ms.push_back(S.miss[j]);
      if (mom) m.insert(m.end(), &S.mom[DM_MOM_WORDS * j], &S.mom[DM_MOM_WORDS * j] + DM_MOM_WORDS);
    });
    const std::string e = dmf_write(path, H, k.data(), v.data(), aux ? ms.data() : nullptr, mom ? m.data() : nullptr);
    LX_REQUIRE(e.empty(), e);
  }

  // include/loamx.h, loamx_densemap_merge
  int merge(DenseMap& src) {
    LX_REQUIRE(&src != this, "a dense map cannot be merged into itself");
    LX_REQUIRE(!history_, "the destination keeps a sweep log (loamx_densemap_enable_history): a merged map has no sweeps behind it to rebuild from");
    LX_REQUIRE(src.cfg.device == cfg.device, "the two dense maps live on different devices");
    LX_REQUIRE(memcmp(&src.cfg.leaf, &cfg.leaf, sizeof(float)) == 0, "the two dense maps differ in their leaf");
    LX_REQUIRE(src.flags() == flags(), "the two dense maps do not have the same features enabled (carving, moments)");
    src.read_counters();
    read_counters();
    if (!occ_.admits_exact(src.occ_.occ, cfg.max_voxels)) return LOAMX_E_CAPACITY;
    DmCtrAdd add;
    add.v[0] = src.drop_range_; add.v[1] = src.drop_key_;
    for (int k = 0; k < 6; k++) add.v[2 + k] = src.carve_ctr_[k];
    merge_records(src.tab_.keys, src.tab_.vals, src.tab_.slots, src.occ_.occ, src.tab_.aux, 2u, src.tab_.mom, add, src.offered_);
    return LOAMX_OK;
  }

  // include/loamx.h, loamx_densemap_merge_file, and with `loading` loamx_densemap_load.  The file is validated on the host before the
  // device is touched; every refusal comes before the first change of the handle
  int merge_file(const char* path, bool loading) {
    LX_REQUIRE(!history_, "the dense map keeps a sweep log (loamx_densemap_enable_history): a map from a file has no sweeps behind it to rebuild from");
    DmFile F;
    const std::string e = dmf_read(path, true, F);
    LX_REQUIRE(e.empty(), std::string(path) + ": " + e);
    LX_REQUIRE(memcmp(&F.h.leaf, &cfg.leaf, sizeof(float)) == 0, "the file's leaf differs from the dense map's");
    const uint64_t n = F.h.count;
    read_counters();
    if (loading) {
      LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "a file can only be loaded into an empty map (a fresh handle, or right after reset)");
      LX_REQUIRE((flags() & ~F.h.flags) == 0u, "the dense map has a feature enabled (carving, moments) that the file lacks");
      if (!occ_.admits_exact(n, cfg.max_voxels)) return LOAMX_E_CAPACITY;   // (occ is 0)
      if (F.h.flags & DMF_CARVING) {
        const loamx_densemap_carve_config c = {F.h.carve_max_range, F.h.ray_stride, F.h.end_margin, F.h.max_steps};
        enable_carving(c);
      }
      if (F.h.flags & DMF_MOMENTS) enable_moments();
      // the smallest table the file's voxels fit at a load of one half (a handle reset after it grew holds a larger one)
      const uint64_t target = dm_slots_for(cfg.initial_slots, n);
      if (tab_.slots > target) {
        // (not the sequence of the other replacements, and kept: the host waits for own_ before the old table retires, and the new
        // one is cleared together with the counters once it is the map's)
        DmTable nt;
        nt.alloc(target, tab_.aux != nullptr, tab_.mom != nullptr);
        LX_HIP(hipStreamSynchronize(own_));
        replace_table(nt);
        clear(own_);
      }
    } else {
      LX_REQUIRE(F.h.flags == flags(), "the file and the dense map do not have the same features (carving, moments)");
      if (!occ_.admits_exact(n, cfg.max_voxels)) return LOAMX_E_CAPACITY;
    }
    // one pinned block, one copy: values (first: the kernel reads them 16 bytes at a time), moment words, keys, then the 32-bit miss words
    const size_t nn = (size_t)n, w_mom = moments() ? DM_MOM_WORDS * nn : 0, w_miss = carving() ? (nn + 1) / 2 : 0;
    const size_t o_mom = 4 * nn, o_keys = o_mom + w_mom, o_miss = o_keys + nn, words = o_miss + w_miss;
    PinBuf<unsigned long long> h_up;
    DevBuf<unsigned long long> d_up;
    h_up.reserve(words + 1);
    d_up.reserve(words + 1);
    if (nn) {
      for (size_t i = 0; i < 4 * nn; i++) h_up.p[i] = F.vals[i];
      for (size_t i = 0; i < w_mom; i++) h_up.p[o_mom + i] = F.mom[i];
      for (size_t i = 0; i < nn; i++) h_up.p[o_keys + i] = F.keys[i];
      if (carving()) {
        h_up.p[words - 1] = 0ull;
        memcpy(h_up.p + o_miss, F.miss.data(), sizeof(uint32_t) * nn);
      }
      LX_HIP(hipMemcpyAsync(d_up.p, h_up.p, sizeof(unsigned long long) * words, hipMemcpyHostToDevice, own_));
    }
    DmCtrAdd add;
    add.v[0] = F.h.dropped_range; add.v[1] = F.h.dropped_key;
    for (int k = 0; k < 6; k++) add.v[2 + k] = F.h.carve_stats[k];
    const unsigned long long* d = d_up.p;
    merge_records(d + o_keys, d, (uint32_t)n, n, (const uint32_t*)(d + o_miss), 1u, d + o_mom, add, F.h.offered);
    return LOAMX_OK;
  }

  // include/loamx.h, loamx_densemap_raycast: the ends go up through the staging block of the adds (free once they are waited for)
  int raycast_host(const loamx_cloud* ends, const float origin[3], const loamx_densemap_raycast_config& c,
                   const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
    check_cloud(ends, false);
    const uint32_t n = ends->count;
    if (out && capacity < n) throw Error(LOAMX_E_CAPACITY, "capacity is smaller than the cloud's count");
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    if (n) {
      h_stage_.reserve(n);
      pack_cloud(ends, h_stage_.p);
      d_stage_.reserve(n);
      fetch_from_pinned(d_stage_.p, h_stage_.p, n, own_);
    }
    cast(d_stage_.p, n, origin, c, rule, out, counts);
    return LOAMX_OK;
  }

  // the raycast_from_* forms: the registered cloud where it lies, own_ behind the stream that wrote it
  int raycast_device(const DenseSource& s, const loamx_densemap_raycast_config& c, const loamx_densemap_static_rule* rule,
                     loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
    LX_REQUIRE(s.device == cfg.device, "the dense map and its source live on different devices");
    if (!s.has_cloud) return LOAMX_SKIPPED;
    if (out && capacity < s.n) throw Error(LOAMX_E_CAPACITY, "capacity is smaller than the cloud's count");
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    if (s.n) dm_stream_behind(own_, s.stream);
    cast(s.pts, s.n, s.origin, c, rule, out, counts);
    return LOAMX_OK;
  }

  // include/loamx.h, loamx_densemap_enable_history: allowed while nothing has been offered; the handle is unchanged when refused
  void enable_history(const loamx_densemap_history_config& c) {
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
  bool history() const { return history_; }
  void history_size(uint64_t* calls, uint64_t* points) const { *calls = hist_.calls.size(); *points = hist_.points; }

  // the logged bytes of one call and its origin
  int history_download(uint64_t call, loamx_cloud* out, float origin[3]) {
    LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
    LX_REQUIRE(call < hist_.calls.size(), "call is beyond the log");
    check_cloud(out, false);
    const DmHistoryCall c = hist_.calls[call];
    if (c.count > out->count) { out->count = c.count; return LOAMX_E_CAPACITY; }
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    h_stage_.reserve(c.count);   // (free: the adds were waited for)
    store_to_pinned_u32((uint32_t*)h_stage_.p, (const uint32_t*)(log_ + c.first), 4 * (size_t)c.count, own_);
    LX_HIP(hipStreamSynchronize(own_));
    for (int a = 0; a < 3; a++) origin[a] = c.origin[a];
    return unpack_cloud(h_stage_.p, c.count, out);
  }

  // include/loamx.h, loamx_densemap_rebuild.  Everything is built beside the handle (table, counter words) and swapped in at the end:
  // a refusal or a failure on the way leaves the handle as it was
  int rebuild(const double* corrections, uint64_t n_calls) {
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
    h_rb_.reserve(2 * (DM_CTR_WORDS + 1));
    d_calls_.reserve(n_calls + 1);
    if (n_calls) LX_HIP(hipMemcpyAsync(d_calls_.p, h_calls_.p, sizeof(DmReplayCall) * n_calls, hipMemcpyHostToDevice, own_));
    const unsigned long long* w = (const unsigned long long*)h_rb_.p;
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
      store_to_pinned_u32(h_rb_.p, (const uint32_t*)nctr.p, 2 * (DM_CTR_WORDS + 1), own_);
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
  void rebuild_stats(uint64_t out[4]) const { for (int k = 0; k < 4; k++) out[k] = rebuild_stats_[k]; }

  // include/loamx.h, loamx_densemap_grid: a checked configuration, a checked rule or none; the table is only read
  void grid(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, loamx_grid_cell* out) {
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    const loamx_grid_cell* cells = grid_.run(tab_, c, rule, (double)cfg.leaf, own_);
    memcpy(out, cells, sizeof(loamx_grid_cell) * (size_t)c.nx * c.nz);
  }

  // include/loamx.h, loamx_densemap_route: checked configurations, a checked rule or none; the grid's kernels as grid() runs them,
  // the route on their records where they lie; the outputs are written last, all or none
  void route(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
             const uint32_t* goals_xz, uint32_t n_goals, loamx_grid_cell* out_cells, loamx_route_cell* out_field, uint64_t stats[6]) {
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    const size_t n = (size_t)c.nx * c.nz;
    const loamx_grid_cell* d_cells = grid_.enqueue(tab_, c, rule, (double)cfg.leaf, own_);
    uint64_t s[6];
    const loamx_route_cell* field = route_.run(d_cells, c.nx, c.nz, rc, goals_xz, n_goals, out_field != nullptr, s, own_);
    const loamx_grid_cell* cells = out_cells ? grid_.fetch(d_cells, n, own_) : nullptr;
    if (out_cells) memcpy(out_cells, cells, sizeof(loamx_grid_cell) * n);
    if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * n);
    if (stats) memcpy(stats, s, sizeof(s));
  }
  // loamx_densemap_route_cells: the same on the caller's records (every cls checked), in a buffer of the route's own
  void route_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc, const uint32_t* goals_xz,
                   uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    const size_t n = (size_t)nx * nz;
    uint64_t s[6];
    const loamx_route_cell* field = route_.run(route_.upload(cells, n, own_), nx, nz, rc, goals_xz, n_goals, out_field != nullptr, s, own_);
    if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * n);
    if (stats) memcpy(stats, s, sizeof(s));
  }
  void route_trace(const uint32_t* starts_xz, uint32_t n_starts, uint32_t* out_xz, uint32_t capacity, uint32_t* lengths) {
    LX_REQUIRE(route_.has_field(), "the handle has no field yet (loamx_densemap_route, loamx_densemap_route_cells)");
    LX_HIP(hipSetDevice(cfg.device));
    route_.trace(starts_xz, n_starts, out_xz, capacity, lengths, own_);
  }
  DmRoute& router() { return route_; }

  // include/loamx.h, loamx_densemap_segment: a checked configuration and rule; the table is only read.  The outputs are written last,
  // all or none (LOAMX_E_CAPACITY: only the two counts)
  int segment(const loamx_densemap_segment_config& c, const loamx_densemap_static_rule& rule, uint32_t* labels, uint64_t label_capacity,
              uint64_t* n_voxels, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[6]) {
    read_counters();   // (waits for every add; the exact voxel count)
    const uint64_t occ = occ_.occ;
    std::vector<uint32_t> lab;
    std::vector<loamx_segment> sg;
    uint64_t s[6] = {0, 0, 0, 0, 0, 0};
    if (occ) segmenter().run(tab_, c, rule, occ, labels != nullptr, lab, sg, s, own_);
    *n_voxels = occ;
    *n_segs = sg.size();
    if ((labels && label_capacity < occ) || (segs && seg_capacity < sg.size())) return LOAMX_E_CAPACITY;
    if (labels && occ) memcpy(labels, lab.data(), sizeof(uint32_t) * occ);
    if (segs && !sg.empty()) memcpy(segs, sg.data(), sizeof(loamx_segment) * sg.size());
    memcpy(stats, s, sizeof(s));
    return LOAMX_OK;
  }
  DmSegment& segmenter() { return seg_; }

  bool combine = true;   // (bench A/B: the in-wave combining of equal keys)
  uint64_t rehashes = 0;

 private:
  hipStream_t own_ = nullptr;      // host-fed adds, rehash of those, exports
  hipStream_t last_st_ = nullptr;  // the stream of the last enqueued add (ev_last_ recorded behind it)
  hipEvent_t ev_last_ = nullptr, ev_snap_ = nullptr, ev_staged_ = nullptr;
  bool staged_pending_ = false;
  DmTable tab_;   // (aux NULL: carving is off; mom NULL: moments are off)
  loamx_densemap_carve_config carve_ = {0.f, 1u, 1u, 4096u};
  uint32_t seq_ = 0;          // sequence number of the last add call (stamp values; 0 = never stamped)
  uint64_t carve_ctr_[6] = {0, 0, 0, 0, 0, 0};
  float inv_ = 10.f;
  DevBuf<unsigned long long> ctr_;
  PinBuf<uint32_t> h_ctr_, h_snap_;
  PinBuf<float4> h_stage_;
  DevBuf<float4> d_stage_;
  // ray casts (allocated by the first cast): the five count words, the records on the device and their pinned landing blocks
  DevBuf<unsigned long long> rc_;
  DevBuf<loamx_ray_hit> d_hits_;
  PinBuf<uint32_t> h_rc_, h_hits_;
  std::vector<void*> graveyard_;   // tables replaced by a rehash: freed at the next point where the host waits anyway
  DmOccupancy occ_;   // the bound of the occupancy that growth and admission are decided on (densemap_growth.hpp)
  uint64_t offered_ = 0, drop_range_ = 0, drop_key_ = 0;
  // the sweep log (densemap_history.hpp): off unless enabled; hist_ then admits everything and log_ stays NULL
  bool history_ = false;
  DmHistory hist_;
  float4* log_ = nullptr;
  PinBuf<DmReplayCall> h_calls_;
  DevBuf<DmReplayCall> d_calls_;
  PinBuf<uint32_t> h_rb_;
  uint64_t rebuild_stats_[4] = {0, 0, 0, 0};
  DmGrid grid_;   // the navigation grid's planes (densemap_grid.hip): allocated by the first grid
  DmRoute route_;   // the route's planes and field (densemap_route.hip): allocated by the first route
  DmSegment seg_;   // the components' work arrays (densemap_segment.hip): allocated by the first segment call

  // room for n more points in the log: a block of the doubled capacity, the logged points copied over on st, the old block to the
  // graveyard (earlier work may still read it)
  void log_reserve(uint64_t n, hipStream_t st) {
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
  void launch_replay(const DmTable& nt, unsigned long long* nctr) {
    const uint32_t n_calls = (uint32_t)hist_.calls.size();
    DmFilter F;
    F.inv = inv_;
    F.min2 = cfg.min_range * cfg.min_range;
    F.max2 = cfg.max_range * cfg.max_range;
    F.use_max = cfg.max_range > 0.f ? 1 : 0;
    F.ox = F.oy = F.oz = 0.f;
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
      DmCarve R;
      R.max2 = carve_.max_range * carve_.max_range;
      R.use_max = carve_.max_range > 0.f ? 1 : 0;
      R.stride = carve_.ray_stride; R.end_margin = carve_.end_margin; R.max_steps = carve_.max_steps;
      const uint64_t span = 256ull * R.stride;
      for (uint32_t k = 0; k < n_calls; k++) {
        const DmHistoryCall& c = hist_.calls[k];
        R.seq = k + 1u;
        hipLaunchKernelGGL((k_dm_rebuild<CB, true, MM>), dim3((c.count + 255u) / 256u), dim3(256), 0, own_, log_, c.first,
                           (unsigned long long)c.count, d_calls_.p, k, k + 1u, F, nt.keys, nt.vals, nt.mask(), nt.shift(), nctr, nt.aux, nt.mom, small);
        hipLaunchKernelGGL(k_dm_rebuild_carve, dim3((uint32_t)((c.count + span - 1) / span)), dim3(256), 0, own_, log_, d_calls_.p + k, c.count, F,
                           R, nt.keys, nt.aux, nt.mask(), nt.shift(), nctr, small);
        rebuild_stats_[2] += 2;
      }
    });
    rebuild_stats_[3] += hist_.points;
  }

  // nt becomes the map's table; the one it replaces goes to the graveyard
  void replace_table(DmTable& nt) {
    tab_.swap(nt);
    nt.retire(graveyard_);
  }
  // the current table into nt on st, under the map's features; PRUNE (carving is on): the rule's dynamic voxels stay behind
  template <bool PRUNE> void launch_rehash(hipStream_t st, const DmTable& nt, const loamx_densemap_static_rule& rule) {
    const DmTable& T = tab_;
    dm_dispatch2(T.aux != nullptr, T.mom != nullptr, [&](auto A, auto M) {
      constexpr bool AUX = decltype(A)::value, MOM = decltype(M)::value;
      if constexpr (AUX || !PRUNE)
        hipLaunchKernelGGL((k_dm_rehash<AUX, PRUNE, MOM>), dim3((T.slots + 255) / 256), dim3(256), 0, st, T.keys, T.vals, T.slots, nt.keys, nt.vals,
                           nt.mask(), nt.shift(), ctr_.p, T.aux, nt.aux, rule, T.mom, nt.mom);
    });
  }
  // the insert of one add; the combine by the bench hook, the moment words when the map has them
  template <bool STAMP> void launch_insert(hipStream_t st, const float4* pts, uint32_t n, const DmFilter& F, uint32_t seq) {
    const DmTable& T = tab_;
    dm_dispatch2(combine, T.mom != nullptr, [&](auto C, auto M) {
      hipLaunchKernelGGL((k_dm_insert<decltype(C)::value, STAMP, decltype(M)::value>), dim3((n + 255) / 256), dim3(256), 0, st, pts, n, F, T.keys,
                         T.vals, T.mask(), T.shift(), ctr_.p, T.aux, seq, T.mom);
    });
  }
  // the table and the counters (the one place that zeroes both)
  void clear(hipStream_t st) {
    tab_.clear(st);
    LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long) * DM_CTR_WORDS, st));
  }
  void free_graveyard() {
    for (void* p : graveyard_) (void)hipFree(p);
    graveyard_.clear();
  }
  // st runs behind every add enqueued so far (on whichever stream)
  void order_behind(hipStream_t st) {
    if (last_st_ && last_st_ != st) LX_HIP(hipStreamWaitEvent(st, ev_last_, 0));
  }
  void wait_adds() {
    if (last_st_) LX_HIP(hipEventSynchronize(ev_last_));
    if (staged_pending_) { LX_HIP(hipEventSynchronize(ev_staged_)); staged_pending_ = false; }
    occ_.snapshot_abandoned();
    free_graveyard();
  }
  // exact counters, after every add
  void read_counters() {
    LX_HIP(hipSetDevice(cfg.device));
    wait_adds();
    store_to_pinned_u32(h_ctr_.p, (const uint32_t*)ctr_.p, 2 * DM_CTR_WORDS, own_);
    LX_HIP(hipStreamSynchronize(own_));
    const unsigned long long* c = (const unsigned long long*)h_ctr_.p;
    LX_REQUIRE(c[3] == 0ull, "dense map: hash table overflow");
    occ_.exact(c[0]);
    drop_range_ = c[1]; drop_key_ = c[2];
    for (int k = 0; k < 6; k++) carve_ctr_[k] = c[4 + k];
  }
  // the occupancy snapshot that has landed, if any
  void poll_snapshot() {
    if (!occ_.snap_pending) return;
    const hipError_t e = hipEventQuery(ev_snap_);
    if (e == hipErrorNotReady) return;
    LX_HIP(e);
    occ_.snapshot_landed(h_snap_.p[0] | ((uint64_t)h_snap_.p[1] << 32));
  }
  // capacity rule (include/loamx.h): decided before anything is enqueued; the exact count is waited for only near the cap
  bool admit(uint32_t n) {
    poll_snapshot();
    if (occ_.admits_by_bound(n, cfg.max_voxels)) return true;
    read_counters();
    return occ_.admits_exact(n, cfg.max_voxels);
  }
  // growth: keep the load at most one half even if every one of n records, and every point enqueued since the last count, made a voxel
  // of its own.  The rehash into the larger table is enqueued on st; the host does not wait
  void grow_for(uint64_t n, hipStream_t st) {
    const uint64_t want = occ_.slots_wanted(tab_.slots, n);
    LX_REQUIRE(want <= (1ull << 31), "dense map: more voxels than the table can index");
    if (want != tab_.slots) {
      DmTable nt;
      nt.alloc(want, tab_.aux != nullptr, tab_.mom != nullptr);
      nt.clear(st);
      launch_rehash<false>(st, nt, loamx_densemap_static_rule{0u, 0u, 0u});
      replace_table(nt);
      rehashes++;
    }
  }
  // the tail of merge / merge_file, behind a read_counters() (every add waited for, occ_ exact): sn source slots or records holding
  // s_occ voxels go into the table on own_; returns when the table holds the result
  void merge_records(const unsigned long long* skeys, const unsigned long long* svals, uint32_t sn, uint64_t s_occ, const uint32_t* smiss,
                     uint32_t miss_stride, const unsigned long long* smom, const DmCtrAdd& add, uint64_t s_offered) {
    grow_for(s_occ, own_);
    const dim3 grid(sn ? (sn + 255u) / 256u : 1u), block(256);   // (one block at least: its first thread adds the statistics)
    const DmTable& T = tab_;
    dm_dispatch2(T.aux != nullptr, T.mom != nullptr, [&](auto A, auto M) {
      hipLaunchKernelGGL((k_dm_merge<decltype(A)::value, decltype(M)::value>), grid, block, 0, own_, skeys, svals, sn, smiss, miss_stride, smom, T.keys,
                         T.vals, T.mask(), T.shift(), ctr_.p, T.aux, T.mom, add);
    });
    LX_HIP(hipGetLastError());
    offered_ += s_offered;
    LX_HIP(hipStreamSynchronize(own_));   // (the rehash of a growth still read the table that read_counters is about to free)
    read_counters();
  }
  // the tail of the ray casts, behind a wait_adds(): n rays from origin to pts (readable on own_) against the live table; returns
  // when the counts and, with out, the n records are back.  read_counters() is the wait: it also reports a probe overflow
  void cast(const float4* pts, uint32_t n, const float origin[3], const loamx_densemap_raycast_config& c,
            const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t counts[5]) {
    for (int k = 0; k < 5; k++) counts[k] = 0;
    if (!n) return;
    constexpr size_t HIT_WORDS = sizeof(loamx_ray_hit) / sizeof(uint32_t);
    rc_.reserve(5);
    h_rc_.reserve(10);
    if (out) {
      d_hits_.reserve(n);
      h_hits_.reserve(HIT_WORDS * n);
    }
    DmCast C;
    C.inv = inv_;
    C.ox = origin[0]; C.oy = origin[1]; C.oz = origin[2];
    C.leaf = (double)cfg.leaf;
    C.max_steps = c.max_steps; C.skip_steps = c.skip_steps; C.min_points = c.min_points;
    C.use_rule = rule ? 1 : 0;
    C.rule = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
    LX_HIP(hipMemsetAsync(rc_.p, 0, sizeof(unsigned long long) * 5, own_));
    hipLaunchKernelGGL(k_dm_raycast, dim3((n + 255u) / 256u), dim3(256), 0, own_, pts, n, C, tab_.keys, tab_.vals, tab_.aux, tab_.mask(),
                       tab_.shift(), ctr_.p, rc_.p, out ? d_hits_.p : nullptr);
    LX_HIP(hipGetLastError());
    store_to_pinned_u32(h_rc_.p, (const uint32_t*)rc_.p, 10, own_);
    if (out) store_to_pinned_u32(h_hits_.p, (const uint32_t*)d_hits_.p, HIT_WORDS * n, own_);
    read_counters();
    const unsigned long long* w = (const unsigned long long*)h_rc_.p;
    for (int k = 0; k < 5; k++) counts[k] = w[k];
    if (out) memcpy(out, h_hits_.p, sizeof(loamx_ray_hit) * n);
  }
  void enqueue_add(const float4* pts, uint32_t n, const float origin[3], hipStream_t st) {
    if (history_ && n) log_reserve(n, st);   // (a failed allocation leaves map and log as they were)
    grow_for(n, st);
    if (n) {
      DmFilter F;
      F.inv = inv_;
      F.min2 = cfg.min_range * cfg.min_range;
      F.max2 = cfg.max_range * cfg.max_range;
      F.use_max = cfg.max_range > 0.f ? 1 : 0;
      F.ox = origin[0]; F.oy = origin[1]; F.oz = origin[2];
      if (!tab_.aux) {
        launch_insert<false>(st, pts, n, F, 0u);
      } else {
        // carving: the insert stamps its voxels with the call's sequence number, and the rays are traced behind it
        seq_++;
        launch_insert<true>(st, pts, n, F, seq_);
        DmCarve R;
        R.max2 = carve_.max_range * carve_.max_range;
        R.use_max = carve_.max_range > 0.f ? 1 : 0;
        R.stride = carve_.ray_stride; R.end_margin = carve_.end_margin; R.max_steps = carve_.max_steps; R.seq = seq_;
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
      store_to_pinned_u32(h_snap_.p, (const uint32_t*)ctr_.p, 2, st);
      LX_HIP(hipEventRecord(ev_snap_, st));
    }
    LX_HIP(hipEventRecord(ev_last_, st));
    last_st_ = st;
  }
};

static void write_pcd_records(const char* path, const float4* rec, size_t n) {
  FILE* f = fopen(path, "wb");
  LX_REQUIRE(f, std::string("cannot open ") + path + " for writing");
  const int hl = fprintf(f,
                         "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
                         "COUNT 1 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n", n, n);
  const bool ok = hl > 0 && (n == 0 || fwrite(rec, sizeof(float4), n, f) == n);
  const bool closed = fclose(f) == 0;
  LX_REQUIRE(ok && closed, std::string("write to ") + path + " failed");
}

static void write_pcd_surfels(const char* path, const loamx_surfel* rec, size_t n) {
  FILE* f = fopen(path, "wb");
  LX_REQUIRE(f, std::string("cannot open ") + path + " for writing");
  const int hl = fprintf(f,
                         "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity normal_x normal_y normal_z curvature\n"
                         "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
                         "POINTS %zu\nDATA binary\n", n, n);
  const bool ok = hl > 0 && (n == 0 || fwrite(rec, sizeof(loamx_surfel), n, f) == n);
  const bool closed = fclose(f) == 0;
  LX_REQUIRE(ok && closed, std::string("write to ") + path + " failed");
}

}  // namespace loamx

using namespace loamx;

struct loamx_densemap {
  DenseMap d;
  explicit loamx_densemap(const loamx_densemap_config& c) : d(c) {}
};

static void checked_axes(int axes) { LX_REQUIRE(axes == 0 || axes == 1, "axes must be 0 (LOAM frame) or 1 (sensor axes)"); }

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
    loamx_densemap_config c;
    if (cfg) c = *cfg; else loamx_densemap_default_config(&c);
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
    return h->d.add_host(points, origin);
  });
}
int loamx_densemap_add_from_map(loamx_densemap* h, loamx_map* m) {
  return guard([&]() {
    LX_REQUIRE(h && m, "NULL argument");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.add_device(s);
  });
}
int loamx_densemap_add_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot) {
  return guard([&]() {
    LX_REQUIRE(h && p, "NULL argument");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.add_device(s);
  });
}
int loamx_densemap_get_stats(loamx_densemap* h, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h && stats, "NULL argument");
    h->d.stats(stats);
    return LOAMX_OK;
  });
}
int loamx_densemap_download(loamx_densemap* h, loamx_cloud* out, int axes) {
  return guard([&]() {
    LX_REQUIRE(h && out, "NULL argument");
    checked_axes(axes);
    check_cloud(out, false);
    std::vector<float4> rec;
    h->d.records(rec, axes);
    if (rec.size() > out->count) { out->count = (uint32_t)rec.size(); return LOAMX_E_CAPACITY; }
    return unpack_cloud(rec.data(), (uint32_t)rec.size(), out);
  });
}
int loamx_densemap_save_pcd(loamx_densemap* h, const char* path, int axes) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    checked_axes(axes);
    std::vector<float4> rec;
    h->d.records(rec, axes);
    write_pcd_records(path, rec.data(), rec.size());
    return LOAMX_OK;
  });
}
int loamx_write_pcd(const char* path, const loamx_cloud* c, int axes) {
  return guard([&]() {
    LX_REQUIRE(path && c, "NULL argument");
    checked_axes(axes);
    check_cloud(c, false);
    std::vector<float4> rec(c->count);
    pack_cloud(c, rec.data());
    if (axes == 1)
      for (float4& r : rec) r = make_float4(r.z, r.x, r.y, r.w);
    write_pcd_records(path, rec.data(), rec.size());
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

// the rule of a call, checked (NULL: the default rule)
static loamx_densemap_static_rule checked_rule(const loamx_densemap_static_rule* rule) {
  loamx_densemap_static_rule r;
  if (rule) r = *rule; else loamx_densemap_static_rule_default(&r);
  LX_REQUIRE(r.den != 0u, "the rule's den must not be 0");
  return r;
}
#define LX_REQUIRE_CARVING(h) LX_REQUIRE((h)->d.carving(), "carving is not enabled")
// the optional rule of a call: NULL stays NULL (every voxel); a rule is checked into `r` and needs carving
static const loamx_densemap_static_rule* checked_optional_rule(loamx_densemap* h, const loamx_densemap_static_rule* rule,
                                                               loamx_densemap_static_rule& r) {
  if (!rule) return nullptr;
  r = checked_rule(rule);
  LX_REQUIRE_CARVING(h);
  return &r;
}

int loamx_densemap_enable_carving(loamx_densemap* h, const loamx_densemap_carve_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    loamx_densemap_carve_config c;
    if (cfg) c = *cfg; else loamx_densemap_carve_default_config(&c);
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
int loamx_densemap_download_misses(loamx_densemap* h, uint32_t* out, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    LX_REQUIRE_CARVING(h);
    std::vector<uint32_t> m;
    h->d.misses(m);
    *n = m.size();
    if (m.size() > capacity) return LOAMX_E_CAPACITY;
    if (!m.empty()) memcpy(out, m.data(), sizeof(uint32_t) * m.size());
    return LOAMX_OK;
  });
}
int loamx_densemap_download_static(loamx_densemap* h, loamx_cloud* out, int axes, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && out, "NULL argument");
    checked_axes(axes);
    const loamx_densemap_static_rule r = checked_rule(rule);
    LX_REQUIRE_CARVING(h);
    check_cloud(out, false);
    std::vector<float4> rec;
    h->d.records(rec, axes, &r);
    if (rec.size() > out->count) { out->count = (uint32_t)rec.size(); return LOAMX_E_CAPACITY; }
    return unpack_cloud(rec.data(), (uint32_t)rec.size(), out);
  });
}
int loamx_densemap_save_pcd_static(loamx_densemap* h, const char* path, int axes, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    checked_axes(axes);
    const loamx_densemap_static_rule r = checked_rule(rule);
    LX_REQUIRE_CARVING(h);
    std::vector<float4> rec;
    h->d.records(rec, axes, &r);
    write_pcd_records(path, rec.data(), rec.size());
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

void loamx_densemap_surfel_default_config(loamx_densemap_surfel_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->min_points = 5u;
  cfg->min_planar_ratio = 0.01f;
}

// the surfel settings of a call, checked (NULL: the defaults)
static loamx_densemap_surfel_config checked_surfel_config(const loamx_densemap_surfel_config* cfg) {
  loamx_densemap_surfel_config c;
  if (cfg) c = *cfg; else loamx_densemap_surfel_default_config(&c);
  LX_REQUIRE(c.min_points >= 3u, "min_points must be >= 3");
  LX_REQUIRE(c.min_planar_ratio >= 0.f, "min_planar_ratio must be >= 0");   // (NaN too)
  return c;
}
#define LX_REQUIRE_MOMENTS(h) LX_REQUIRE((h)->d.moments(), "moments are not enabled")

int loamx_densemap_surfel_of(float leaf, const int32_t idx[3], const uint64_t vals[4], const uint64_t mom[9],
                             const loamx_densemap_surfel_config* cfg, int axes, loamx_surfel* out) {
  return guard([&]() {
    LX_REQUIRE(idx && vals && mom && out, "NULL argument");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    checked_axes(axes);
    LX_REQUIRE(vals[0] != 0ull, "a voxel holds at least one point");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    const long long ia[3] = {idx[0], idx[1], idx[2]};
    const unsigned long long v4[4] = {vals[0], vals[1], vals[2], vals[3]};
    unsigned long long m9[DM_MOM_WORDS];
    for (int k = 0; k < DM_MOM_WORDS; k++) m9[k] = mom[k];
    dm_surfel((double)leaf, ia, v4, m9, c, axes, *out);
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
int loamx_densemap_download_moments(loamx_densemap* h, uint64_t* out, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    LX_REQUIRE_MOMENTS(h);
    std::vector<unsigned long long> m;
    h->d.moment_words(m);
    *n = m.size() / DM_MOM_WORDS;
    if (*n > capacity) return LOAMX_E_CAPACITY;
    if (!m.empty()) memcpy(out, m.data(), sizeof(uint64_t) * m.size());
    return LOAMX_OK;
  });
}
// the surfels of a call: arguments checked in the order of download_static (a rule needs carving)
static void surfels_of_call(loamx_densemap* h, int axes, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                            std::vector<loamx_surfel>& out) {
  checked_axes(axes);
  const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
  LX_REQUIRE_MOMENTS(h);
  loamx_densemap_static_rule r;
  h->d.surfels(out, axes, c, checked_optional_rule(h, rule, r));
}
int loamx_densemap_download_surfels(loamx_densemap* h, loamx_surfel* out, uint64_t capacity, uint64_t* n, int axes,
                                    const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    std::vector<loamx_surfel> s;
    surfels_of_call(h, axes, cfg, rule, s);
    *n = s.size();
    if (s.size() > capacity) return LOAMX_E_CAPACITY;
    if (!s.empty()) memcpy(out, s.data(), sizeof(loamx_surfel) * s.size());
    return LOAMX_OK;
  });
}
int loamx_densemap_save_pcd_surfels(loamx_densemap* h, const char* path, int axes, const loamx_densemap_surfel_config* cfg,
                                    const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    std::vector<loamx_surfel> s;
    surfels_of_call(h, axes, cfg, rule, s);
    write_pcd_surfels(path, s.data(), s.size());
    return LOAMX_OK;
  });
}

int loamx_densemap_freeze(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                          uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    const uint64_t n = h->d.freeze(c, checked_optional_rule(h, rule, r));
    if (n_surfels) *n_surfels = n;
    return LOAMX_OK;
  });
}
int loamx_densemap_frozen_size(loamx_densemap* h, uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h && n_surfels, "NULL argument");
    *n_surfels = h->d.frozen.valid() ? h->d.frozen.size() : 0;
    return LOAMX_OK;
  });
}

int loamx_densemap_save(loamx_densemap* h, const char* path) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    h->d.save(path);
    return LOAMX_OK;
  });
}
int loamx_densemap_load(loamx_densemap* h, const char* path) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    return h->d.merge_file(path, true);
  });
}
int loamx_densemap_merge(loamx_densemap* dst, loamx_densemap* src) {
  return guard([&]() {
    LX_REQUIRE(dst && src, "NULL argument");
    return dst->d.merge(src->d);
  });
}
int loamx_densemap_merge_file(loamx_densemap* dst, const char* path) {
  return guard([&]() {
    LX_REQUIRE(dst && path, "NULL argument");
    return dst->d.merge_file(path, false);
  });
}
int loamx_densemap_file_info(const char* path, struct loamx_densemap_file_info* info, int deep) {
  return guard([&]() {
    LX_REQUIRE(path && info, "NULL argument");
    DmFile F;
    const std::string e = dmf_read(path, deep != 0, F);
    LX_REQUIRE(e.empty(), std::string(path) + ": " + e);
    memset(info, 0, sizeof(*info));
    info->version = F.h.version; info->flags = F.h.flags;
    info->leaf = F.h.leaf;
    info->voxels = F.h.count;
    info->offered = F.h.offered; info->dropped_range = F.h.dropped_range; info->dropped_key = F.h.dropped_key;
    for (int k = 0; k < 6; k++) info->carve_stats[k] = F.h.carve_stats[k];
    info->carve.max_range = F.h.carve_max_range;
    info->carve.ray_stride = F.h.ray_stride; info->carve.end_margin = F.h.end_margin; info->carve.max_steps = F.h.max_steps;
    return LOAMX_OK;
  });
}

void loamx_densemap_history_default_config(loamx_densemap_history_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_bytes = 0;
  cfg->initial_points = 1ull << 20;
}
int loamx_densemap_enable_history(loamx_densemap* h, const loamx_densemap_history_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    loamx_densemap_history_config c;
    if (cfg) c = *cfg; else loamx_densemap_history_default_config(&c);
    h->d.enable_history(c);
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

void loamx_densemap_raycast_default_config(loamx_densemap_raycast_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_steps = 4096u;
  cfg->skip_steps = 0u;
  cfg->min_points = 1u;
}

// the settings and the rule of a cast, checked (cfg NULL: the defaults; rule NULL stays NULL: every voxel)
static loamx_densemap_raycast_config checked_raycast(loamx_densemap* h, const loamx_densemap_raycast_config* cfg,
                                                     const loamx_densemap_static_rule* rule, const uint64_t* counts) {
  LX_REQUIRE(counts, "counts is NULL");
  loamx_densemap_raycast_config c;
  if (cfg) c = *cfg; else loamx_densemap_raycast_default_config(&c);
  LX_REQUIRE(c.max_steps >= 1u && c.max_steps <= 65536u, "max_steps must be in [1, 65536]");
  LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
  if (rule) {
    LX_REQUIRE(rule->den != 0u, "the rule's den must not be 0");
    LX_REQUIRE(h->d.carving(), "a rule needs carving, which is not enabled");
  }
  return c;
}

int loamx_densemap_raycast(loamx_densemap* h, const loamx_cloud* ends, const float origin[3], const loamx_densemap_raycast_config* cfg,
                           const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(ends, "ends is NULL");
    LX_REQUIRE(origin, "origin is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    return h->d.raycast_host(ends, origin, c, rule, out, capacity, counts);
  });
}
int loamx_densemap_raycast_from_map(loamx_densemap* h, loamx_map* m, const loamx_densemap_raycast_config* cfg,
                                    const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(m, "m is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.raycast_device(s, c, rule, out, capacity, counts);
  });
}
int loamx_densemap_raycast_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const loamx_densemap_raycast_config* cfg,
                                         const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity,
                                         uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(p, "p is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.raycast_device(s, c, rule, out, capacity, counts);
  });
}

int loamx_densemap_grid(loamx_densemap* h, const loamx_densemap_grid_config* cfg, const loamx_densemap_static_rule* rule,
                        loamx_grid_cell* out) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(out, "out is NULL");
    loamx_densemap_grid_config c;
    if (cfg) c = *cfg; else loamx_densemap_grid_default_config(&c);
    dm_grid_check(c);
    if (rule) {
      LX_REQUIRE(rule->den != 0u, "the rule's den must not be 0");
      LX_REQUIRE(h->d.carving(), "a rule needs carving, which is not enabled");
    }
    h->d.grid(c, rule, out);
    return LOAMX_OK;
  });
}

// the checks the route's entry points share: the configuration (NULL: the defaults), the goals and the window's size
static loamx_grid_route_config checked_route(const loamx_grid_route_config* cfg, const uint32_t* goals_xz, uint32_t n_goals, uint32_t nx,
                                             uint32_t nz) {
  loamx_grid_route_config rc;
  if (cfg) rc = *cfg; else loamx_grid_route_default_config(&rc);
  dm_route_check(rc);
  LX_REQUIRE(goals_xz, "goals_xz is NULL");
  LX_REQUIRE(n_goals >= 1u && n_goals <= 4096u, "n_goals must be in [1, 4096]");
  LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= (1ull << 22), "nx * nz must be in [1, 2^22] for a route");
  return rc;
}

int loamx_densemap_route(loamx_densemap* h, const loamx_densemap_grid_config* grid_cfg, const loamx_densemap_static_rule* rule,
                         const loamx_grid_route_config* cfg, const uint32_t* goals_xz, uint32_t n_goals, loamx_grid_cell* out_cells,
                         loamx_route_cell* out_field, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    loamx_densemap_grid_config c;
    if (grid_cfg) c = *grid_cfg; else loamx_densemap_grid_default_config(&c);
    dm_grid_check(c);
    if (rule) {
      LX_REQUIRE(rule->den != 0u, "the rule's den must not be 0");
      LX_REQUIRE(h->d.carving(), "a rule needs carving, which is not enabled");
    }
    const loamx_grid_route_config rc = checked_route(cfg, goals_xz, n_goals, c.nx, c.nz);
    h->d.route(c, rule, rc, goals_xz, n_goals, out_cells, out_field, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_route_cells(loamx_densemap* h, const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config* cfg,
                               const uint32_t* goals_xz, uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(cells, "cells is NULL");
    const loamx_grid_route_config rc = checked_route(cfg, goals_xz, n_goals, nx, nz);
    for (size_t i = 0; i < (size_t)nx * nz; i++)
      LX_REQUIRE(cells[i].cls <= LOAMX_GRID_STEP, "cells: the cls of record " + std::to_string(i) + " is not a class");
    h->d.route_cells(cells, nx, nz, rc, goals_xz, n_goals, out_field, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_route_trace(loamx_densemap* h, const uint32_t* starts_xz, uint32_t n_starts, uint32_t* out_xz, uint32_t capacity,
                               uint32_t* lengths) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(starts_xz, "starts_xz is NULL");
    LX_REQUIRE(n_starts >= 1u && n_starts <= 4096u, "n_starts must be in [1, 4096]");
    LX_REQUIRE(out_xz || !capacity, "out_xz is NULL");
    LX_REQUIRE(lengths, "lengths is NULL");
    h->d.route_trace(starts_xz, n_starts, out_xz, capacity, lengths);
    return LOAMX_OK;
  });
}

int loamx_densemap_segment(loamx_densemap* h, const loamx_densemap_segment_config* cfg, const loamx_densemap_static_rule* rule, uint32_t* labels,
                           uint64_t label_capacity, uint64_t* n_voxels, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs,
                           uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(n_voxels, "n_voxels is NULL");
    LX_REQUIRE(n_segs, "n_segs is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    loamx_densemap_segment_config c;
    if (cfg) c = *cfg; else loamx_densemap_segment_default_config(&c);
    dm_segment_check(c);
    loamx_densemap_static_rule r;
    loamx_densemap_static_rule_default(&r);
    if (c.which != LOAMX_SEGMENT_ALL) {
      LX_REQUIRE(h->d.carving(), "which: a selection by the rule needs carving, which is not enabled");
      if (rule) r = *rule;
      LX_REQUIRE(r.den != 0u, "the rule's den must not be 0");
    }
    return h->d.segment(c, r, labels, label_capacity, n_voxels, segs, seg_capacity, n_segs, stats);
  });
}

// bench / test hooks (not in include/loamx.h): the in-wave combining of equal keys on or off, and the number of rehashes so far
int loamx_densemap_set_combine(loamx_densemap* h, int on) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->d.combine = on != 0; return LOAMX_OK; });
}
uint64_t loamx_densemap_rehashes(loamx_densemap* h) { return h ? h->d.rehashes : 0; }
// the route's rounds per look (1..64), and the rounds of the last route in which a tile ran
int loamx_densemap_route_set_batch(loamx_densemap* h, uint32_t batch) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(batch >= 1u && batch <= 64u, "batch must be in [1, 64]");
    h->d.router().batch = batch;
    return LOAMX_OK;
  });
}
uint64_t loamx_densemap_route_active_rounds(loamx_densemap* h) { return h ? h->d.router().active_rounds : 0; }

}  // extern "C"

DmFrozen& loamx_densemap_frozen(loamx_densemap* h) { return h->d.frozen; }
hipStream_t loamx_densemap_own_stream(loamx_densemap* h) { return h->d.own_stream(); }
const loamx_densemap_config& loamx_densemap_cfg(loamx_densemap* h) { return h->d.cfg; }
