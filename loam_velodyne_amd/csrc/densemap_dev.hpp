// Dense map, device side: what the kernels of more than one file share (densemap.hip, densemap_rebuild.hip, densemap_raycast.hip,
// densemap_merge.hip, place_views.hip) — the arguments of the insert and of the carve, the claim of a slot, the wave-aggregated counters, the key rule
// and the voxel walk of the rays.  dm_hash, dm_find and dm_dynamic are in densemap.hpp: the files that only read the table use them too.
#pragma once
#include "densemap.hpp"

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

// the same for a 64-bit value per lane (modulo 2^64): one atomic per wave
__device__ inline void dm_wave_sum64(unsigned long long* ctr, unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  if (v && (threadIdx.x & 63) == 0) atomicAdd(ctr, v);
}

// A window of voxel indices as the kernels test it (include/loamx.h, loamx_densemap_region): lo <= i <= hi on every axis, or with
// `outside` the negation.  Integer compares on the three 21-bit fields of the key; the caller has an occupied slot's key
struct DmWindow {
  int lo[3], hi[3];
  uint32_t outside;
};
__device__ inline bool dm_in_window(unsigned long long key, const DmWindow& W) {
  const int ix = (int)(key & 0x1FFFFFull) - (1 << DM_QBITS), iy = (int)((key >> DM_KBITS) & 0x1FFFFFull) - (1 << DM_QBITS),
            iz = (int)((key >> (2 * DM_KBITS)) & 0x1FFFFFull) - (1 << DM_QBITS);
  const bool in = ix >= W.lo[0] && ix <= W.hi[0] && iy >= W.lo[1] && iy <= W.hi[1] && iz >= W.lo[2] && iz <= W.hi[2];
  return in != (W.outside != 0u);
}

// what a rehash leaves behind (k_dm_rehash, densemap.hip)
constexpr int DM_DROP_NONE = 0, DM_DROP_RULE = 1, DM_DROP_WINDOW = 2;

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

}  // namespace loamx
