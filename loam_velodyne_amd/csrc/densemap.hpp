// Dense global map (include/loamx.h, loamx_densemap_*): an open-addressing hash table of voxels in HBM, fed with registered sweeps on the
// device.  Each slot holds a 64-bit key (EMPTY = all ones; a key is < 2^63) and four 64-bit words: n, Sx, Sy, Sz (integer sums of the
// 20-bit fixed-point offsets inside the voxel, so the table does not depend on the order of the additions).
#pragma once
#include "common.h"
#include "cloud_stage.hpp"
#include "densemap_growth.hpp"
#include "pinned_copy.hpp"
#include "scan.hpp"
#include <vector>

namespace loamx {

constexpr unsigned long long DM_EMPTY = ~0ull;
constexpr int DM_QBITS = 20;              // fixed-point bits of the offset inside a voxel
constexpr int DM_KBITS = 21;              // bits per axis of the key: i + 2^20, |i| < 2^20
constexpr float DM_QSCALE = 1048576.f;    // 2^20
constexpr float DM_IMAX = 1048576.f;      // |i| must stay below this
constexpr int DM_MOM_WORDS = 9;           // moments: 64-bit words per slot (dm_insert_body.inc)

// the key of the voxel (ix, iy, iz), each |i| < 2^20, and its inverse
__host__ __device__ inline unsigned long long dm_key(int ix, int iy, int iz) {
  return (unsigned long long)(uint32_t)(ix + (1 << DM_QBITS)) | ((unsigned long long)(uint32_t)(iy + (1 << DM_QBITS)) << DM_KBITS) |
         ((unsigned long long)(uint32_t)(iz + (1 << DM_QBITS)) << (2 * DM_KBITS));
}
inline void dm_key_indices(unsigned long long k, long long ia[3]) {
  const unsigned long long km = (1ull << DM_KBITS) - 1ull;
  for (int a = 0; a < 3; a++) ia[a] = (long long)((k >> (DM_KBITS * a)) & km) - (1ll << DM_QBITS);
}

inline uint32_t log2u(uint64_t v) { uint32_t r = 0; while ((1ull << r) < v) r++; return r; }

// The map's table in HBM: `slots` (a power of two) keys, four value words per slot and, where the feature is on, aux (carving: 2 x 32
// bits per slot, [2 * slot] miss, [2 * slot + 1] stamp) and mom (moments: nine words per slot).  Owns its arrays; the kernels take them
// as scalar arguments, expanded at the launch sites
struct DmTable {
  unsigned long long *keys = nullptr, *vals = nullptr, *mom = nullptr;
  uint32_t* aux = nullptr;
  uint32_t slots = 0;

  DmTable() = default;
  DmTable(const DmTable&) = delete;
  DmTable& operator=(const DmTable&) = delete;
  ~DmTable() { (void)hipFree(keys); (void)hipFree(vals); (void)hipFree(aux); (void)hipFree(mom); }
  void swap(DmTable& o) {
    std::swap(keys, o.keys); std::swap(vals, o.vals); std::swap(mom, o.mom); std::swap(aux, o.aux); std::swap(slots, o.slots);
  }
  uint32_t mask() const { return slots - 1u; }
  uint32_t shift() const { return 64u - log2u(slots); }   // (dm_hash)

  // an empty table becomes one of n <= 2^31 slots, its contents undefined; nothing is kept when an allocation fails
  void alloc(uint64_t n, bool with_aux, bool with_mom) {
    slots = (uint32_t)n;
    try {
      LX_HIP(hipMalloc((void**)&keys, sizeof(unsigned long long) * n));
      LX_HIP(hipMalloc((void**)&vals, sizeof(unsigned long long) * 4 * n));
      if (with_aux) add_aux();
      if (with_mom) add_mom();
    } catch (...) {
      DmTable().swap(*this);   // (freed by the temporary)
      throw;
    }
  }
  // a feature's array beside a table that stands; the caller clears it
  void add_aux() { LX_HIP(hipMalloc((void**)&aux, sizeof(uint32_t) * 2 * (size_t)slots)); }
  void add_mom() { LX_HIP(hipMalloc((void**)&mom, sizeof(unsigned long long) * DM_MOM_WORDS * (size_t)slots)); }
  void clear_aux(hipStream_t st) { LX_HIP(hipMemsetAsync(aux, 0, sizeof(uint32_t) * 2 * (size_t)slots, st)); }
  void clear_mom(hipStream_t st) { LX_HIP(hipMemsetAsync(mom, 0, sizeof(unsigned long long) * DM_MOM_WORDS * (size_t)slots, st)); }
  // every key EMPTY, every word zero (slots claimed later accumulate from zero), enqueued on st
  void clear(hipStream_t st) {
    LX_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)slots, st));
    LX_HIP(hipMemsetAsync(vals, 0, sizeof(unsigned long long) * 4 * (size_t)slots, st));
    if (mom) clear_mom(st);
    if (aux) clear_aux(st);
  }
  // the arrays go to the graveyard (work enqueued earlier may still read them: freed where the host waits anyway); the table is empty
  void retire(std::vector<void*>& graveyard) {
    for (void* p : {(void*)keys, (void*)vals, (void*)aux, (void*)mom})
      if (p) graveyard.push_back(p);
    keys = vals = mom = nullptr;
    aux = nullptr;
    slots = 0;
  }
};

// The chained scan (scan.hpp) of the per-block counts behind a ballot compaction: its chain state, zero-filled once, on first use, and
// its two scratch words.  scan.hpp lets one state serve all scans of ONE stream and no others: a DenseMap owns one DmScan and hands
// it to compact_of, DmSegment::run and DmFrontier::run, all three of which scan on the map's own stream, own_
struct DmScan {
  // the nblk counts at blk become their exclusive prefix sums in place and blk[nblk] their total, enqueued on st
  void run(uint32_t* blk, uint32_t nblk, hipStream_t st) {
    scratch_.reserve(2);
    if (!state_.p) {
      state_.reserve(chained_scan_state_words());
      LX_HIP(hipMemsetAsync(state_.p, 0, sizeof(unsigned long long) * state_.cap, st));
    }
    exclusive_scan_u32_n(blk, blk, (uint32_t*)state_.p, scratch_.p, nblk, st);
  }

 private:
  DevBuf<unsigned long long> state_;
  DevBuf<uint32_t> scratch_;
};

// the home slot of a key in a table of 2^(64 - shift) slots (the map's table and the frozen snapshot's)
__device__ inline unsigned long long dm_hash(unsigned long long key, uint32_t shift) {
  return (key * 0x9E3779B97F4A7C15ull) >> shift;
}

// the probe loop of dm_find_or_claim (densemap_dev.hpp) without the CAS: 1 the key is at `slot`, 0 it is absent, -1 the probe bound was reached
__device__ inline int dm_find(const unsigned long long* keys, uint32_t mask, uint32_t shift, unsigned long long key, uint32_t& slot) {
  uint32_t h = (uint32_t)dm_hash(key, shift);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    const unsigned long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) { slot = h; return 1; }
    if (cur == DM_EMPTY) return 0;
    h = (h + 1u) & mask;
  }
  return -1;
}

// include/loamx.h, loamx_densemap_static_rule: the voxel with n points and `miss` crossings is dynamic
__host__ __device__ inline bool dm_dynamic(const loamx_densemap_static_rule& r, unsigned long long n, uint32_t miss) {
  return miss >= r.min_misses && (unsigned long long)miss * r.den > n * r.num;
}

// Frozen surfel snapshot (include/loamx.h, loamx_densemap_freeze / loamx_densemap_align_*; densemap_align.hip): an open-addressing
// table of its own, one 32-byte entry per slot — the voxel's key and the six f32 of its surfel record — so that a probe that hits
// reads one 32-byte sector.  Built once per freeze, read-only afterwards; the live map never touches it.
struct DmFrozenEntry {
  unsigned long long key;   // DM_EMPTY: a free slot
  float mean[3], normal[3];
};
static_assert(sizeof(DmFrozenEntry) == 32, "one entry, one 32-byte sector");

class DmFrozen {
 public:
  DmFrozen() = default;
  DmFrozen(const DmFrozen&) = delete;
  DmFrozen& operator=(const DmFrozen&) = delete;
  ~DmFrozen() { drop(); }
  bool valid() const { return tab_ != nullptr; }
  uint64_t size() const { return count_; }
  uint32_t slots() const { return slots_; }
  void drop();
  // replaces the snapshot by the n voxels (keys[i], rec[6 * i ..]); blocks until the table stands
  void build(const unsigned long long* keys, const float* rec, size_t n, hipStream_t st);
  // the same from arrays that lie on the device, written by work enqueued on st (k_dm_surfels, densemap_freeze.hip): no upload
  void build_device(const unsigned long long* d_keys, const float* d_rec, size_t n, hipStream_t st);
  // the entries on the host in ascending key order: keys[i], rec[6 * i ..]; blocks
  void download(std::vector<unsigned long long>& keys, std::vector<float>& rec, hipStream_t st) const;
  DmCloudStage cloud{false};   // the cloud of the steps that follow from the host, in the feature's own device block (level 0's serves every level; every step blocks: no guard)
  // one linearisation (include/loamx.h, loamx_densemap_align_step); blocks until the 33 words are back
  void step(const float4* pts, uint32_t n, const float rtc[15], float inv, uint32_t neighbourhood, float max_residual, hipStream_t st,
            int64_t sums[28], uint64_t counts[5]);
  // the same about n_poses poses in one memset, one launch and one readback (loamx_densemap_align_step_many): pose_table() hands out
  // room for n_poses records of 16 floats in pinned memory (R, t, c, one unused), to be filled before the call; the result is the 33
  // words per pose in pinned memory, valid until the next step of either kind
  float* pose_table(uint32_t n_poses);
  const unsigned long long* step_many(const float4* pts, uint32_t n, uint32_t n_poses, float inv, uint32_t neighbourhood, float max_residual,
                                      hipStream_t st);
  // launches of either step kernel, readbacks of accumulator words, pose-steps (loamx_densemap_get_align_stats); never cleared
  const uint64_t* stats() const { return stats_; }

 private:
  DmFrozenEntry* tab_ = nullptr;
  uint32_t slots_ = 0;
  uint64_t count_ = 0;
  DevBuf<unsigned long long> acc_;
  PinLanding<unsigned long long> h_acc_;
  PinBuf<float4> h_poses_;
  DevBuf<float4> d_poses_;
  uint64_t stats_[3] = {0, 0, 0};
};

// Ray casts (include/loamx.h, loamx_densemap_raycast ...; densemap_raycast.hip): the five count words and the records on the device,
// and the pinned blocks they come back through.  Allocated by the first cast, grow to the largest one; the live map is only read.
class DmCaster {
 public:
  DmCaster() = default;
  DmCaster(const DmCaster&) = delete;
  DmCaster& operator=(const DmCaster&) = delete;
  // n >= 1 rays from origin to pts (readable on st) against the table T under a checked configuration and rule (NULL: every voxel),
  // enqueued on st: one memset, the kernel (a probe overflow goes to word 3 of map_ctr, the map's counters) and the stores of the
  // counts and, when want_hits, of the n records.  No wait
  void enqueue(const DmTable& T, unsigned long long* map_ctr, float inv, double leaf, const float4* pts, uint32_t n, const float origin[3],
               const loamx_densemap_raycast_config& c, const loamx_densemap_static_rule* rule, bool want_hits, hipStream_t st);
  // what the last enqueue stored, once the caller has waited for its stream: the five counts and, with out, the n records
  void results(uint32_t n, loamx_ray_hit* out, uint64_t counts[5]) const;

 private:
  DevBuf<unsigned long long> rc_;
  DevBuf<loamx_ray_hit> d_hits_;
  PinLanding<unsigned long long> h_rc_;
  PinLanding<loamx_ray_hit> h_hits_;
};

// Navigation grid (include/loamx.h, loamx_densemap_grid; densemap_grid.hip): the accumulator planes of a window and its records on the
// device, and the pinned block the records come back through.  Grow to the largest window asked for; the live map is only read.
class DmGrid {
 public:
  DmGrid() = default;
  DmGrid(const DmGrid&) = delete;
  DmGrid& operator=(const DmGrid&) = delete;
  // the grid of a checked configuration over the table T (every add waited for) on st: one memset, the four kernels, one readback;
  // blocks until the c.nx * c.nz records are in pinned memory and returns them, valid until the next run
  const loamx_grid_cell* run(const DmTable& T, const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, double leaf,
                             hipStream_t st) {
    return fetch(enqueue(T, c, rule, leaf, st), (size_t)c.nx * c.nz, st);
  }
  // the two halves of run (DmRoute, densemap_route_core.hpp, routes on the records where enqueue leaves them): the memset and the four kernels, enqueued;
  // returns the records on the device, valid until the next enqueue.  fetch: the readback of n of them, blocking
  const loamx_grid_cell* enqueue(const DmTable& T, const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, double leaf,
                                 hipStream_t st);
  const loamx_grid_cell* fetch(const loamx_grid_cell* d_cells, size_t n, hipStream_t st);

 private:
  DevBuf<uint32_t> planes_;   // DM_GRID_PLANE_WORDS 32-bit words per cell, plane after plane (densemap_grid.hip)
  DevBuf<loamx_grid_cell> cells_;
  PinLanding<loamx_grid_cell> h_cells_;
};

// include/loamx.h, loamx_densemap_grid_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_grid_check(const loamx_densemap_grid_config& c);

// include/loamx.h, weight of a cell under a checked configuration: 0 = blocked, otherwise 1..32 (loamx_grid_route_weight, the
// device's k_dm_route_weights<DmRouteGrid> and a caller's own planner share this one expression)
__host__ __device__ inline uint32_t dm_route_weight(uint32_t cls, uint32_t clear2, const loamx_grid_route_config& c) {
  if (clear2 < c.min_clear2) return 0u;
  if (cls != LOAMX_GRID_FREE && !(cls == LOAMX_GRID_UNKNOWN && c.unknown_weight > 0u)) return 0u;
  const uint32_t p = clear2 < c.soft_clear2 ? c.soft_weight * (c.soft_clear2 - clear2) / c.soft_clear2 : 0u;   // (<= 15 * 4225)
  return 1u + p + (cls == LOAMX_GRID_UNKNOWN ? c.unknown_weight : 0u);
}
// include/loamx.h, loamx_grid_route_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_route_check(const loamx_grid_route_config& c);
// (the route over these weights: DmRoute, an instance of the route engine of densemap_route_core.hpp)

// include/loamx.h, loamx_grid_frontier_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_frontier_check(const loamx_grid_frontier_config& c);

// the accumulator of one frontier on the device: loamx_frontier with best_cost and best_cell as one aligned 64-bit word,
// (cost << 32) | cell, so that one atomicMin keeps "the smallest cost, then the smallest index"
struct DmFrAcc {
  uint32_t min_cell, cells, lo[2], hi[2];
  unsigned long long sum_rx, sum_rz, links, best;
  uint32_t reachable, reserved;
};
static_assert(sizeof(DmFrAcc) == 64 && sizeof(loamx_frontier) == 64, "64-byte records");

// Frontiers of the navigation grid (include/loamx.h, loamx_densemap_frontiers ...; densemap_frontier.hip): one parent word, one id word
// and one byte per cell of a window, the per-block root counts, the frontiers' accumulators, the labels, and the pinned blocks the
// counters, the accumulators, the ranks and the labels cross through.  Allocated by the first call, grow to the largest window asked
// for; the map, the grid's records and the route's field are only read.
class DmFrontier {
 public:
  DmFrontier() = default;
  DmFrontier(const DmFrontier&) = delete;
  DmFrontier& operator=(const DmFrontier&) = delete;
  // the frontiers of nx * nz <= 2^26 records d_cells on the device (written by work enqueued on st) under a checked configuration:
  // mark, link, flatten, the scan (through the map's DmScan: st is the stream of its scans), ids and reduce, and the host's min_cells
  // and ranks.  d_field (NULL: none): the nx * nz records of a route's field on the device, whose costs give reachable and best.
  // Blocks.  out: the kept frontiers in ascending min_cell; stats as in include/loamx.h.  Returns, when want_labels, the nx * nz
  // labels in pinned memory, valid until the next run
  const uint32_t* run(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_frontier_config& c,
                      const loamx_route_cell* d_field, bool want_labels, std::vector<loamx_frontier>& out, uint64_t stats[6], DmScan& scan,
                      hipStream_t st);

 private:
  DevBuf<uint32_t> parent_, rootid_;   // per cell: the union-find word (NONE: no frontier cell); the compact id of a root
  DevBuf<unsigned char> u8_;           // per cell: unknown8 of a frontier cell
  DevBuf<uint32_t> blk_;               // roots per 256-cell block, + 1 word for the total
  DevBuf<uint32_t> ctr_;               // frontier cells, hook attempts lost, a loop bound reached, roots
  DevBuf<DmFrAcc> acc_;                // one accumulator per frontier, by compact id
  DevBuf<uint32_t> rank_, lab_;        // with labels: per compact id its rank (NONE: dropped); per cell its label
  PinBuf<uint32_t> h_ctr_, h_rank_, h_lab_;
  PinLanding<DmFrAcc> h_acc_;
};

// include/loamx.h, loamx_densemap_dist_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_dist_check(const loamx_densemap_dist_config& c);

// Distance field (include/loamx.h, loamx_densemap_dist and loamx_densemap_dist_query; densemap_dist.hip): per cell of a 3-D window
// 1/8 byte of the bit volume, the 4-byte word of the y pass, 2 bytes of d2 and 4 of near, 10 1/8 bytes per cell in all (0.68 GB at
// 2^26 cells), and the pinned blocks that the stats, the planes wanted, the query's points and its samples cross through.  Allocated
// by the first call, grow to the largest window asked for; the live map is only read.
class DmDist {
 public:
  DmDist() = default;
  DmDist(const DmDist&) = delete;
  DmDist& operator=(const DmDist&) = delete;
  // the field of a checked configuration over the table T (every add waited for) under a checked rule or none, on st: one memset
  // and three kernels.  Blocks until the four stats and the planes wanted are in pinned memory (valid until the next run); the
  // field stays on the device for query()
  void run(const DmTable& T, const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, bool want_d2, bool want_near,
           uint64_t stats[4], hipStream_t st);
  const uint16_t* d2_on_host() const { return (const uint16_t*)h_d2_.data(); }
  const uint32_t* near_on_host() const { return h_near_.data(); }
  bool has_field() const { return valid_; }
  // the d2 plane of the field that stands where it lies on the device, 16 bits per cell, and its configuration (DmRoute3 routes there)
  const unsigned short* d2_on_device() const { return (const unsigned short*)d2_.p; }
  const loamx_densemap_dist_config& config() const { return cfg_; }
  void drop() { valid_ = false; }   // (the buffers stay for the next field)
  DmCloudStage cloud{false};   // the query's points from the host, in the feature's own device block (query() blocks: no guard)
  // n >= 1 points (readable on st) against the field of the last run: the five stats and, when want_samples, the n samples in
  // pinned memory, valid until the next query.  Blocks
  const loamx_dist_sample* query(const float4* pts, uint32_t n, float inv, uint32_t min_d2, bool want_samples, uint64_t stats[5],
                                 hipStream_t st);

 private:
  DevBuf<unsigned long long> vol_;   // the four stats words, then the bit volume: ceil(nx / 64) words per row (rz, ry)
  DevBuf<uint32_t> yx_;              // per cell: rx | ry << 10 of the nearest occupied cell of its plane, NONE
  DevBuf<uint32_t> d2_;              // per cell 16 bits, two cells per word
  DevBuf<uint32_t> near_;
  DevBuf<unsigned long long> qc_;    // the query's five words
  DevBuf<loamx_dist_sample> d_out_;
  PinLanding<unsigned long long> h_ctr_, h_qc_;
  PinLanding<uint32_t> h_d2_, h_near_;
  PinLanding<loamx_dist_sample> h_out_;
  loamx_densemap_dist_config cfg_ = {};   // of the field that stands
  bool valid_ = false;
};

// include/loamx.h, weight of a cell of the distance field under a checked configuration: 0 = blocked, otherwise 1..16
// (loamx_route3_weight, the device's k_dm_route_weights<DmRouteVol> and a caller's own planner share this one expression)
__host__ __device__ inline uint32_t dm_route3_weight(uint32_t d2, const loamx_route3_config& c) {
  if (d2 < c.min_d2) return 0u;
  return 1u + (d2 < c.soft_d2 ? c.soft_weight * (c.soft_d2 - d2) / c.soft_d2 : 0u);   // (<= 15 * 65025)
}
// include/loamx.h, the moves: (dx, dy, dz) of direction d < 26
__host__ __device__ inline void dm_route3_move(uint32_t d, int& dx, int& dy, int& dz) {
  dx = dy = dz = 0;
  if (d < 6u) {
    const int s = (d & 1u) ? -1 : 1;
    if (d < 2u) dx = s; else if (d < 4u) dy = s; else dz = s;
  } else if (d < 18u) {
    const uint32_t i = d - 6u;
    const int a = (i & 1u) ? -1 : 1, b = (i & 2u) ? -1 : 1;
    if (i < 4u) { dx = a; dy = b; } else if (i < 8u) { dx = a; dz = b; } else { dy = a; dz = b; }
  } else {
    const uint32_t i = d - 18u;
    dx = (i & 1u) ? -1 : 1;
    dy = (i & 2u) ? -1 : 1;
    dz = (i & 4u) ? -1 : 1;
  }
}
// include/loamx.h, loamx_route3_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_route3_check(const loamx_route3_config& c);
// (the route over these weights and moves: DmRoute3, the other instance of the route engine of densemap_route_core.hpp)

// include/loamx.h, loamx_densemap_tsdf_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_tsdf_check(const loamx_densemap_tsdf_config& c);

constexpr int DM_TSDF_CTR = 8;   // counter words of the field: [0] traced, [2] filter, [3] steps or key, [4] zero length, [5] visited
                                 // inside, and at a download [6] cells with W > 0, [7] the largest W ([1], stride, is the host's)

// Signed distance field and its mesh (include/loamx.h, loamx_densemap_tsdf_* and loamx_densemap_mesh; densemap_mesh.hip): per cell
// of the window 4 bytes of W and 8 of D and, from the first mesh on, one byte of edge bits and 4 bytes of vertex base; the counters,
// the per-block counts of the two scans and the mesh's buffers.  Allocated by loamx_densemap_tsdf_begin and by the first mesh, grow
// to the largest window asked for; the live map and its log are only read.
struct DmTsdf {
  DmTsdf() = default;
  DmTsdf(const DmTsdf&) = delete;
  DmTsdf& operator=(const DmTsdf&) = delete;
  bool has_field() const { return valid_; }
  void drop() { valid_ = false; }   // (the buffers stay for the next field)
  size_t cells() const { return (size_t)cfg_.nx * cfg_.ny * cfg_.nz; }

  DmCloudStage cloud;                 // a cloud from the host, in the feature's own device block (the adds do not block: guarded)
  DevBuf<uint32_t> w_;                // per cell: W
  DevBuf<unsigned long long> d_;      // per cell: D, two's complement
  DevBuf<unsigned long long> ctr_;    // DM_TSDF_CTR words, then the mesh's four (valid, inside, tetrahedra, holes)
  DevBuf<uint32_t> mask_;             // per cell one byte, four cells per word: bit e = the edge e of this owner has a vertex
  DevBuf<uint32_t> vbase_;            // per cell: the index of its first vertex
  DevBuf<uint32_t> blk_;              // two runs of blocks + 1 words: triangles, then vertices, per 256-cell block
  DevBuf<float> verts_;
  DevBuf<uint32_t> tris_;
  loamx_densemap_tsdf_config cfg_ = {};   // of the field that stands
  uint64_t stride_skipped_ = 0;           // stats[1]: decided on the host, per call
  bool valid_ = false;
};

// include/loamx.h, loamx_densemap_segment_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_segment_check(const loamx_densemap_segment_config& c);

// Connected components of the voxel table (include/loamx.h, loamx_densemap_segment; densemap_segment.hip): one parent word and one
// component id per slot, the per-block counts of the two compactions, the components' accumulators, and the pinned blocks the totals,
// the components and the (key, id) pairs come back through.  Allocated by the first call, sized by the table's slots, grown when the
// table has grown; the map is only read.
class DmSegment {
 public:
  DmSegment() = default;
  DmSegment(const DmSegment&) = delete;
  DmSegment& operator=(const DmSegment&) = delete;
  // the components of the table T (every add waited for, `occ` voxels, occ >= 1) under a checked configuration and rule, on st:
  // select, link, flatten, the two scans (through the map's DmScan: st is the stream of its scans), ids and reduce, and the host's
  // ordering by key.  Blocks.  segs: the kept components in ascending min_key; labels (when want_labels): one word per voxel in
  // ascending key order; stats as in include/loamx.h
  // rank_of_id (optional): per compact id the component's place in segs, NONE when min_voxels dropped it
  void run(const DmTable& T, const loamx_densemap_segment_config& c, const loamx_densemap_static_rule& rule, uint64_t occ, bool want_labels,
           std::vector<uint32_t>& labels, std::vector<loamx_segment>& segs, uint64_t stats[6], DmScan& scan, hipStream_t st,
           std::vector<uint32_t>* rank_of_id = nullptr);
  // what the last run left on the device, per slot of its table: the root of a selected slot (NONE: not selected), and a root's
  // compact id (DmSegCloud labels points through them)
  const uint32_t* parent() const { return parent_.p; }
  const uint32_t* rootid() const { return rootid_.p; }

 private:
  DevBuf<uint32_t> parent_, rootid_;       // per slot: the union-find word (NONE: not selected); the compact id of a root
  DevBuf<uint32_t> blk_;                   // two runs of blocks + 1 words: roots, then occupied slots, per 256-slot block
  DevBuf<unsigned long long> ctr_;         // voxels selected, hook attempts lost, the two totals, a loop bound reached
  DevBuf<loamx_segment> acc_;              // one accumulator per component, by compact id
  DevBuf<unsigned long long> okeys_;       // with labels: the occupied slots' keys in slot order ...
  DevBuf<uint32_t> oids_;                  // ... and their compact ids (NONE: not selected)
  PinBuf<uint32_t> h_tot_, h_ids_;
  PinLanding<loamx_segment> h_acc_;
  PinLanding<unsigned long long> h_keys_;
};

struct DmFilter;   // densemap_dev.hpp

// include/loamx.h, loamx_densemap_segment_cloud_check: throws LOAMX_E_INVALID with a message that names the first field out of its bounds
void dm_segment_cloud_check(const loamx_densemap_segment_cloud_config& c);

// Objects of a cloud that is not in the map (include/loamx.h, loamx_densemap_segment_cloud; densemap_segment_cloud.hip): a scratch
// table of the map's format without aux or mom (a power of two of at least twice the cloud's count, at least 1024 slots: kept, grown
// to the largest call, cleared per call), one key word and one id word per point, six counters, and the staging and pinned blocks of
// its own that the cloud, the counters and the ids cross through.  The live map is only read.
class DmSegCloud {
 public:
  DmSegCloud() = default;
  DmSegCloud(const DmSegCloud&) = delete;
  DmSegCloud& operator=(const DmSegCloud&) = delete;
  DmCloudStage cloud{false};   // the cloud from the host, in the feature's own device block (insert() blocks: no guard)
  // n >= 1 points (readable on st) under the filter F of their origin against the live table M (every add waited for): the scratch
  // table cleared, the admitted points that pass the map test of a checked configuration and rule (NULL: every voxel) inserted.
  // Blocks.  counts: dropped by range, by the key rule, rejected by the map test, entered, voxels of the scratch table
  void insert(const DmTable& M, const DmFilter& F, const loamx_densemap_segment_cloud_config& c, const loamx_densemap_static_rule* rule,
              const float4* pts, uint32_t n, hipStream_t st, uint64_t counts[5]);
  const DmTable& table() const { return tab_; }
  // behind seg.run on table(): per point of the last insert the compact id (< n_roots) of its voxel's component, NONE when the point
  // did not enter or its voxel was not selected; in pinned memory, valid until the next call.  Blocks
  const uint32_t* ids(const DmSegment& seg, uint32_t n_roots, uint32_t n, hipStream_t st);

 private:
  DmTable tab_;               // (slots: the size this call uses, the front of an allocation of cap_slots_)
  uint32_t cap_slots_ = 0;
  DevBuf<unsigned long long> pkey_, ctr_;   // per point: its key, EMPTY when it did not enter; the counters
  DevBuf<uint32_t> ids_;
  PinLanding<unsigned long long> h_ctr_;
  PinLanding<uint32_t> h_ids_;
};

}  // namespace loamx
