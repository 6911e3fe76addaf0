// Sub-map index: host classes and the device helpers shared with the kernels that search it (registration.hip, odometry.hip).
// Kernels and host code live in submap_index.hip.
#pragma once
#include <cfloat>
#include "common.h"
#include "grid_fit.hpp"   // GridDesc, grid_fit()

namespace loamx {

constexpr uint32_t LX_MAX_CELLS = 16u * 1024 * 1024 - 2048;   // scan limit (scan.hpp)

class SubMapIndex {
 public:
  void init(hipStream_t st);
  // (re)build over n device points (packed float4; .w ignored).  Asynchronous on the stream.
  // bounds_done: the kernel that produced d_pts has folded every point into d_bounds() as it wrote it (enc_f32 atomicMin / atomicMax on
  // words 0-2 / 3-5; the accumulators are left reset by every build) — the bounding-box launch is skipped
  void build(const float4* d_pts, uint32_t n, bool bounds_done = false);
  // room for sub-maps of up to n points without another allocation (a live map grows: Mapper::ensure)
  void reserve_points(uint32_t n) { sorted_.reserve(n); cell_of_.reserve(n); rank_of_.reserve(n); }
  uint32_t* d_bounds() const { return scratch_.p; }
  // exchange contents with another index (buffers, sizes and the streams they are bound to stay with the contents' owner)
  void swap(SubMapIndex& o);
  void bind(hipStream_t st) { st_ = st; }
  uint32_t size() const { return n_; }
  const float4* sorted() const { return sorted_.p; }          // .w = original index (bit pattern)
  const uint32_t* cell_start() const { return cell_start_.p; }
  const GridDesc* desc() const { return d_desc_.p; }

 private:
  hipStream_t st_ = nullptr;
  uint32_t n_ = 0;
  DevBuf<float4> sorted_;
  DevBuf<uint32_t> cell_of_, rank_of_, cell_start_, cursor_, tile_sums_, scratch_;   // scratch_: bbox enc[6], ncell+1, total; cursor_: the cell counters (empty between builds)
  DevBuf<GridDesc> d_desc_;
};

// The same index over K clouds at once (one set of launches): clouds are concatenated, cloud c = [off[c], off[c+1]).
// All cell tables live in one array (cloud c's table starts at desc[c].cell_base) and one global scan yields start
// offsets that index the concatenated sorted array directly; .w of a sorted point = its index inside its own cloud.
struct GridDescB {
  GridDesc g;
  uint32_t cell_base;   // first entry of this cloud's cell table
  uint32_t pt_base;     // off[c]
};
// order-preserving float <-> uint32 (bounds accumulated with integer atomicMin / atomicMax)
__device__ inline uint32_t enc_f32(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float dec_f32(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}
// Bounds accumulators: six words per cloud, each in a cache line of its own (BB_STRIDE words apart) — atomics on one line serialise
// (~12 ns each, measured), and a producer kernel sends a few hundred per word.
constexpr uint32_t BB_STRIDE = 32;
__device__ __host__ inline uint32_t bb_word(uint32_t c, uint32_t a) { return (6u * c + a) * BB_STRIDE; }
// A producer kernel folds its output points into the bounds of cloud c (SubMapIndexBatch::d_bounds) as it writes them: reduced per wave
// (shuffles) and per workgroup (LDS) when their points belong to one cloud — all but the few waves that straddle a boundary — so a
// cloud's words see one atomic per workgroup.  EVERY thread of the workgroup must call (inactive ones with active = false);
// workgroups of at most 1024 threads.
__device__ inline void cloud_bounds_update(uint32_t* __restrict__ enc, bool active, uint32_t c, float x, float y, float z) {
  constexpr uint32_t NONE = 0xffffffffu, MIXED = 0xfffffffeu;
  __shared__ float s_red[16][6];
  __shared__ uint32_t s_cloud[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (int)((blockDim.x + 63) >> 6);
  const unsigned long long m = __ballot(active);
  uint32_t wc = NONE;
  if (m) {
    const uint32_t c0 = (uint32_t)__shfl((int)c, __ffsll((long long)m) - 1, 64);
    wc = __ballot(active && c != c0) == 0ull ? c0 : MIXED;
  }
  if (wc < MIXED) {
    float mn[3] = {active ? x : FLT_MAX, active ? y : FLT_MAX, active ? z : FLT_MAX};
    float mx[3] = {active ? x : -FLT_MAX, active ? y : -FLT_MAX, active ? z : -FLT_MAX};
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, 64));
        mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, 64));
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 3; a++) { s_red[wid][a] = mn[a]; s_red[wid][3 + a] = mx[a]; }
    }
  } else if (wc == MIXED && active) {   // a wave across a cloud boundary: every lane for itself
    atomicMin(&enc[bb_word(c, 0)], enc_f32(x)); atomicMin(&enc[bb_word(c, 1)], enc_f32(y)); atomicMin(&enc[bb_word(c, 2)], enc_f32(z));
    atomicMax(&enc[bb_word(c, 3)], enc_f32(x)); atomicMax(&enc[bb_word(c, 4)], enc_f32(y)); atomicMax(&enc[bb_word(c, 5)], enc_f32(z));
  }
  if (lane == 0) s_cloud[wid] = wc;
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = (int)threadIdx.x;
    for (int w = 0; w < nw; w++) {
      const uint32_t cw = s_cloud[w];
      if (cw >= MIXED) continue;
      bool first = true;
      for (int v = 0; v < w; v++) first = first && s_cloud[v] != cw;
      if (!first) continue;   // (combined with an earlier wave of the same cloud)
      float r = s_red[w][a];
      for (int u = w + 1; u < nw; u++)
        if (s_cloud[u] == cw) r = a < 3 ? fminf(r, s_red[u][a]) : fmaxf(r, s_red[u][a]);
      if (a < 3) atomicMin(&enc[bb_word(cw, a)], enc_f32(r)); else atomicMax(&enc[bb_word(cw, a)], enc_f32(r));
    }
  }
}
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline void cell_coords(const GridDesc& g, float x, float y, float z, int& cx, int& cy, int& cz) {
  cx = clampi((int)floorf((x - g.ox) * g.inv_h), 0, g.nx - 1);
  cy = clampi((int)floorf((y - g.oy) * g.inv_h), 0, g.ny - 1);
  cz = clampi((int)floorf((z - g.oz) * g.inv_h), 0, g.nz - 1);
}

// Points arrive in scan order, so neighbouring lanes mostly fall into the same cell: one atomic per RUN of equal cells
// in a wave instead of one per point (64 lanes hammering two or three counters serialise in L2).
// run_head_len: for the calling lane, the lane that starts its run and, if it is that lane, the run's length.
__device__ inline void wave_runs(uint32_t key, bool active, int& head_lane, int& run_len) {
  const int lane = (int)__lane_id();
  const uint32_t prev = __shfl_up(key, 1, 64);
  const unsigned long long act = __ballot(active);
  const unsigned long long heads = __ballot(active && (lane == 0 || prev != key || !((act >> (lane > 0 ? lane - 1 : 0)) & 1ull)));
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const unsigned long long below = heads & upto;
  head_lane = below ? 63 - __builtin_clzll(below) : lane;
  const unsigned long long stops = (heads | ~act) & ~upto;   // next head, or the first inactive lane
  const int end = stops ? __builtin_ctzll(stops) : 64;
  run_len = end - lane;   // meaningful on the head lane
}

class SubMapIndexBatch {
 public:
  void init(hipStream_t st);
  // d_pts: concatenated points; h_off: K+1 host offsets.  Asynchronous on the stream.
  // d_off_ready: the K+1 offsets already on the device (skips the upload)
  // bounds_done: the kernel that produced d_pts has folded them into d_bounds() already (cloud_bounds_update; prepare(K) came first)
  void build(const float4* d_pts, const uint32_t* h_off, uint32_t K, const uint32_t* d_off_ready = nullptr, bool bounds_done = false);
  void prepare(uint32_t K);
  uint32_t* d_bounds() const { return enc_.p; }
  float cell_size = 1.05f;   // initial cell edge (grown by 1.25x while the cell table would exceed its budget)
  bool pack_ring = false;    // .w of a sorted point = (ring << 24) | index inside its cloud, ring = (int) of the input's .w (255: does not fit)
  const float4* sorted() const { return sorted_.p; }
  const GridDescB* desc(uint32_t c) const { return d_desc_.p + c; }
  const uint32_t* cell_table() const { return cell_start_.p; }   // one array for all clouds, addressed through desc(c)->cell_base

 private:
  hipStream_t st_ = nullptr;
  DevBuf<float4> sorted_;
  void reset_bounds_(uint32_t K);
  uint32_t enc_ready_ = 0;   // clouds whose bounds accumulators are known to be reset
  DevBuf<uint32_t> cell_of_, rank_of_, cell_start_, cursor_, tile_sums_, scratch_, d_off_, enc_;   // cursor_: the cell counters (empty between builds)
  DevBuf<GridDescB> d_desc_;
  PinBuf<uint32_t> h_off_pin_;
};

}  // namespace loamx
