// Connected components of the dense map (densemap.hpp DmSegment, include/loamx.h loamx_densemap_segment and what goes with it): the
// selected voxels of the table grouped under 6-, 18- or 26-connectivity, each component named by the smallest key in it.
//
// Five plain launches over the table's slots, one thread per slot, with two chained scans and one look at the totals (k_dm_seg_totals,
// through pinned memory: the second half is sized by them) between the third and the fourth:
//   k_dm_seg_select   parent[slot] = slot for a selected voxel, NONE otherwise; counts the selected.
//   k_dm_seg_link     per selected slot, the forward half of its neighbourhood (the offsets that are lexicographically positive in
//                     (dz, dy, dx): 3, 9 or 13 of them); the index-range test comes before the neighbour's key is formed; dm_find, and
//                     a union when the neighbour is selected: the lock-free union-find of densemap_label.hpp over parent[] in HBM
//                     (agent scope; the argument for it is there), a slot's rank being its KEY, so that the root of a finished
//                     component is its smallest key whatever the slot layout.  The bound of every loop is the number of slots; one
//                     that is reached raises ctr[3], and the host reports LOAMX_E_INTERNAL.
//   k_dm_seg_flatten  parent[slot] = root, and the roots and the occupied slots of each 256-slot block counted (dm_block_count2);
//                     the scans of the two count runs give every root a compact id and every voxel its place in slot order.
//   k_dm_seg_ids      a root writes its id and the empty accumulator of its component (min_key = its own key).
//   k_dm_seg_reduce   per selected voxel: voxels, points and the three index sums by 64-bit integer adds, the box by 32-bit signed min
//                     and max: integer, commutative, exact.  With labels it also writes (key, id) of every occupied slot, compacted.
//
// The reduce kernel combines inside the block before it touches HBM (kept; the unreduced form was not measured on a device).  Real
// maps have one giant component, the ground and all that stands on it, so nearly every thread of nearly every block adds to the same
// 72 bytes: the shape the kernel guide calls an order of magnitude slower, and with eleven atomics per voxel.  A wave whose selected
// lanes all share one component (the common case) sums them by shuffles; the sums go to a 256-entry table in LDS keyed by the compact id
// (open addressing; a block meets at most 256 ids, so a probe always ends), and each used entry is flushed by one thread: one global
// atomic per (block, component, word).  LDS: 256 x (4 + 40 + 24) bytes = 17 KiB per block.
//
// The host orders the results, as loamx_densemap_download does: components by min_key, voxels by key; it applies min_voxels, maps compact
// ids to ranks and fills the labels.  Compact ids follow the slot layout and never leave this file.
#include "densemap_label.hpp"
#include "densemap_map.hpp"
#include "pinned_copy.hpp"
#include <algorithm>
#include <climits>
#include <numeric>

namespace loamx {

constexpr uint32_t DM_SEG_NONE = DM_UF_NONE;
constexpr int DM_SEG_AGENT = __HIP_MEMORY_SCOPE_AGENT;   // parent[] is in HBM: other workgroups of the launch hook into it

struct DmSegArgs {
  uint32_t which, maxsum, min_points;   // maxsum: 1, 2 or 3, the largest |dx| + |dy| + |dz| of a neighbour
  int lo[3], hi[3];
  loamx_densemap_static_rule rule;
};

__device__ inline void dm_seg_indices(unsigned long long key, int ia[3]) {
  const uint32_t km = (1u << DM_KBITS) - 1u;
#pragma unroll
  for (int a = 0; a < 3; a++) ia[a] = (int)((uint32_t)(key >> (DM_KBITS * a)) & km) - (1 << DM_QBITS);
}

__global__ __launch_bounds__(256) void k_dm_seg_select(DmSegArgs G, const unsigned long long* __restrict__ keys,
                                                       const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                       uint32_t slots, uint32_t* __restrict__ parent, unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool sel = false;
  if (i < slots) {
    const unsigned long long key = keys[i];
    if (key != DM_EMPTY) {
      int ia[3];
      dm_seg_indices(key, ia);
      const unsigned long long n = vals[4ull * i];
      sel = n >= G.min_points && ia[0] >= G.lo[0] && ia[0] <= G.hi[0] && ia[1] >= G.lo[1] && ia[1] <= G.hi[1] && ia[2] >= G.lo[2] && ia[2] <= G.hi[2];
      if (sel && G.which != LOAMX_SEGMENT_ALL) sel = dm_dynamic(G.rule, n, aux[2ull * i]) == (G.which == LOAMX_SEGMENT_DYNAMIC);
    }
    parent[i] = sel ? i : DM_SEG_NONE;
  }
  const unsigned long long m = __ballot(sel);
  if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
}

// ctr: [0] voxels selected, [1] hooks lost, [2] the two totals (k_dm_seg_totals), [3] a loop bound was reached
__global__ __launch_bounds__(256) void k_dm_seg_link(uint32_t maxsum, const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t mask,
                                                     uint32_t shift, uint32_t* parent, unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots || dm_uf_load<DM_SEG_AGENT>(&parent[i]) == DM_SEG_NONE) return;
  int ia[3];
  dm_seg_indices(keys[i], ia);
  uint32_t lost = 0u, bad = 0u;
  for (int o = 14; o < 27; o++) {   // (dz, dy, dx) lexicographically positive
    const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
    if ((uint32_t)((dx != 0) + (dy != 0) + (dz != 0)) > maxsum) continue;
    const int nx = ia[0] + dx, ny = ia[1] + dy, nz = ia[2] + dz;
    const int lim = (1 << DM_QBITS) - 1;
    if (nx < -lim || nx > lim || ny < -lim || ny > lim || nz < -lim || nz > lim) continue;   // no such voxel: not looked up
    uint32_t nb = 0;
    if (dm_find(keys, mask, shift, dm_key(nx, ny, nz), nb) != 1) continue;
    if (dm_uf_load<DM_SEG_AGENT>(&parent[nb]) == DM_SEG_NONE) continue;
    if (!dm_uf_union<DM_SEG_AGENT>(parent, i, nb, slots, [keys](uint32_t s) { return keys[s]; }, lost)) bad = 1u;
  }
  if (lost) atomicAdd(&ctr[1], (unsigned long long)lost);
  if (bad) atomicOr(&ctr[3], 1ull);
}

__global__ __launch_bounds__(256) void k_dm_seg_flatten(const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t* parent,
                                                        uint32_t* __restrict__ blk_roots, uint32_t* __restrict__ blk_occ,
                                                        unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool occ = false, root = false;
  if (i < slots) {
    occ = keys[i] != DM_EMPTY;
    const uint32_t x = dm_uf_load<DM_SEG_AGENT>(&parent[i]);
    if (x != DM_SEG_NONE) {
      root = x == i;
      const uint32_t r = dm_uf_root<DM_SEG_AGENT>(parent, x, slots);
      if (r == DM_SEG_NONE) atomicOr(&ctr[3], 1ull);
      else if (!root) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, DM_SEG_AGENT);
    }
  }
  uint32_t n_roots, n_occ;
  dm_block_count2(root, occ, n_roots, n_occ);
  if (threadIdx.x == 0) {
    blk_roots[blockIdx.x] = n_roots;
    blk_occ[blockIdx.x] = n_occ;
  }
}

// the two totals of the scans beside the counters: the eight words that go back before the second half is sized
__global__ void k_dm_seg_totals(const uint32_t* __restrict__ total_roots, const uint32_t* __restrict__ total_occ, unsigned long long* __restrict__ ctr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctr[2] = (unsigned long long)*total_roots | ((unsigned long long)*total_occ << 32);
}

// behind the scan of the root counts: a root's compact id and the empty accumulator of its component
__global__ __launch_bounds__(256) void k_dm_seg_ids(const unsigned long long* __restrict__ keys, uint32_t slots, const uint32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ off_roots, uint32_t n_roots, uint32_t* __restrict__ rootid,
                                                    loamx_segment* __restrict__ acc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = i < slots && parent[i] == i;
  const unsigned long long m = dm_block_vote(root);
  if (!root) return;
  const uint32_t id = dm_block_rank(m, off_roots[blockIdx.x]);
  if (id >= n_roots) return;   // (cannot happen: the scan counted these roots)
  rootid[i] = id;
  loamx_segment s;
  s.min_key = keys[i];
  s.voxels = s.points = 0ull;
  for (int a = 0; a < 3; a++) { s.lo[a] = INT_MAX; s.hi[a] = INT_MIN; s.sum_idx[a] = 0; }
  acc[id] = s;
}

template <bool LABELS>
__global__ __launch_bounds__(256) void k_dm_seg_reduce(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                       uint32_t slots, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rootid,
                                                       uint32_t n_roots, loamx_segment* __restrict__ acc, const uint32_t* __restrict__ off_occ,
                                                       uint32_t n_occ, unsigned long long* __restrict__ okeys, uint32_t* __restrict__ oids) {
  __shared__ uint32_t s_id[DM_LDS_IDS];
  __shared__ unsigned long long s_sum[DM_LDS_IDS][5];   // voxels, points, sum_idx
  __shared__ int s_box[DM_LDS_IDS][6];                  // lo, hi
  const uint32_t t = threadIdx.x, i = blockIdx.x * blockDim.x + t;
  const int lane = (int)(t & 63);
  s_id[t] = DM_SEG_NONE;
#pragma unroll
  for (int k = 0; k < 5; k++) s_sum[t][k] = 0ull;
#pragma unroll
  for (int a = 0; a < 3; a++) { s_box[t][a] = INT_MAX; s_box[t][3 + a] = INT_MIN; }
  unsigned long long key = DM_EMPTY;
  uint32_t id = DM_SEG_NONE;
  if (i < slots) {
    key = keys[i];
    if (key != DM_EMPTY) {
      const uint32_t r = parent[i];
      if (r != DM_SEG_NONE) id = rootid[r];
    }
  }
  if (id != DM_SEG_NONE && id >= n_roots) id = DM_SEG_NONE;   // (cannot happen: every root got an id below n_roots)
  const bool occ = key != DM_EMPTY, sel = id != DM_SEG_NONE;
  unsigned long long mo = 0ull;   // (the one barrier behind the table's initial values, with labels in the vote, without on its own)
  if (LABELS) mo = dm_block_vote(occ); else __syncthreads();
  if (LABELS && occ) {
    const uint32_t pos = dm_block_rank(mo, off_occ[blockIdx.x]);
    if (pos < n_occ) { okeys[pos] = key; oids[pos] = id; }
  }
  // this lane's contribution (the identities when it is not selected)
  unsigned long long sum[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
  int box[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  if (sel) {
    int ia[3];
    dm_seg_indices(key, ia);
    sum[0] = 1ull;
    sum[1] = vals[4ull * i];
#pragma unroll
    for (int a = 0; a < 3; a++) { sum[2 + a] = (unsigned long long)(long long)ia[a]; box[a] = box[3 + a] = ia[a]; }
  }
  const unsigned long long ms = __ballot(sel);
  bool put = sel;
  if (ms) {   // (wave-uniform)
    const int leader = __builtin_ctzll(ms);
    const uint32_t lid = (uint32_t)__shfl((int)id, leader, 64);
    if (__ballot(sel && id == lid) == ms && __popcll(ms) > 1) {   // one component in the wave: its lanes' sum by shuffles, the leader adds it
#pragma unroll
      for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; k++) sum[k] += (unsigned long long)__shfl_xor((long long)sum[k], o, 64);
#pragma unroll
        for (int a = 0; a < 3; a++) {
          box[a] = min(box[a], __shfl_xor(box[a], o, 64));
          box[3 + a] = max(box[3 + a], __shfl_xor(box[3 + a], o, 64));
        }
      }
      put = lane == leader;
    }
  }
  if (put) {
    const uint32_t h = dm_lds_claim(s_id, id);
#pragma unroll
    for (int k = 0; k < 5; k++) atomicAdd(&s_sum[h][k], sum[k]);
#pragma unroll
    for (int a = 0; a < 3; a++) { atomicMin(&s_box[h][a], box[a]); atomicMax(&s_box[h][3 + a], box[3 + a]); }
  }
  __syncthreads();
  const uint32_t fid = s_id[t];
  if (fid == DM_SEG_NONE) return;
  loamx_segment* s = acc + fid;
  atomicAdd((unsigned long long*)&s->voxels, s_sum[t][0]);
  atomicAdd((unsigned long long*)&s->points, s_sum[t][1]);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    atomicAdd((unsigned long long*)&s->sum_idx[a], s_sum[t][2 + a]);
    atomicMin(&s->lo[a], s_box[t][a]);
    atomicMax(&s->hi[a], s_box[t][3 + a]);
  }
}

void DmSegment::run(const DmTable& T, const loamx_densemap_segment_config& c, const loamx_densemap_static_rule& rule, uint64_t occ,
                    bool want_labels, std::vector<uint32_t>& labels, std::vector<loamx_segment>& segs, uint64_t stats[6], DmScan& scan_state,
                    hipStream_t st, std::vector<uint32_t>* rank_of_id) {
  const uint32_t slots = T.slots, nblk = (slots + 255u) / 256u;
  parent_.reserve(slots);
  rootid_.reserve(slots);
  blk_.reserve(2 * ((size_t)nblk + 1));
  ctr_.reserve(4);
  h_tot_.reserve(8);
  uint32_t *blk_roots = blk_.p, *blk_occ = blk_.p + nblk + 1;
  DmSegArgs G;
  G.which = c.which;
  G.maxsum = c.connectivity == 6u ? 1u : (c.connectivity == 18u ? 2u : 3u);
  G.min_points = c.min_points;
  for (int a = 0; a < 3; a++) { G.lo[a] = c.lo[a]; G.hi[a] = c.hi[a]; }
  G.rule = rule;
  const dim3 scan(nblk), block(256);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long) * 4, st));
  hipLaunchKernelGGL(k_dm_seg_select, scan, block, 0, st, G, T.keys, T.vals, T.aux, slots, parent_.p, ctr_.p);
  hipLaunchKernelGGL(k_dm_seg_link, scan, block, 0, st, G.maxsum, T.keys, slots, T.mask(), T.shift(), parent_.p, ctr_.p);
  hipLaunchKernelGGL(k_dm_seg_flatten, scan, block, 0, st, T.keys, slots, parent_.p, blk_roots, blk_occ, ctr_.p);
  scan_state.run(blk_roots, nblk, st);   // ([nblk]: the total)
  scan_state.run(blk_occ, nblk, st);
  hipLaunchKernelGGL(k_dm_seg_totals, dim3(1), dim3(64), 0, st, blk_roots + nblk, blk_occ + nblk, ctr_.p);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_tot_.p, (const uint32_t*)ctr_.p, 8, st);
  LX_HIP(hipStreamSynchronize(st));
  scan_check_errors();
  const uint64_t selected = h_tot_.p[0] | ((uint64_t)h_tot_.p[1] << 32), lost = h_tot_.p[2] | ((uint64_t)h_tot_.p[3] << 32);
  const uint32_t n_roots = h_tot_.p[4];
  if (h_tot_.p[6]) throw Error(LOAMX_E_INTERNAL, "segment: a union-find loop reached its bound");
  if (h_tot_.p[5] != occ) throw Error(LOAMX_E_INTERNAL, "segment: the compaction disagrees with the occupancy count");
  if (n_roots > selected) throw Error(LOAMX_E_INTERNAL, "segment: more components than selected voxels");

  if (n_roots || want_labels) {
    acc_.reserve(n_roots);
    if (want_labels) { okeys_.reserve(occ); oids_.reserve(occ); }
    if (n_roots) hipLaunchKernelGGL(k_dm_seg_ids, scan, block, 0, st, T.keys, slots, parent_.p, blk_roots, n_roots, rootid_.p, acc_.p);
    if (want_labels)
      hipLaunchKernelGGL(k_dm_seg_reduce<true>, scan, block, 0, st, T.keys, T.vals, slots, parent_.p, rootid_.p, n_roots, acc_.p, blk_occ,
                         (uint32_t)occ, okeys_.p, oids_.p);
    else
      hipLaunchKernelGGL(k_dm_seg_reduce<false>, scan, block, 0, st, T.keys, T.vals, slots, parent_.p, rootid_.p, n_roots, acc_.p, blk_occ,
                         (uint32_t)occ, okeys_.p, oids_.p);
    LX_HIP(hipGetLastError());
    h_acc_.fetch(acc_.p, n_roots, st);
    if (want_labels) {
      h_ids_.reserve(occ);
      h_keys_.fetch(okeys_.p, occ, st);
      store_to_pinned_u32(h_ids_.p, oids_.p, occ, st);
    }
    LX_HIP(hipStreamSynchronize(st));
  }

  // the host's half: components by min_key, min_voxels, ranks; voxels by key
  const loamx_segment* all = h_acc_.data();
  std::vector<uint32_t> order(n_roots), rank(n_roots, DM_SEG_NONE);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return all[a].min_key < all[b].min_key; });
  segs.clear();
  uint64_t total = 0, kept_voxels = 0, largest = 0;
  for (uint32_t id : order) {
    total += all[id].voxels;
    largest = std::max<uint64_t>(largest, all[id].voxels);
    if (all[id].voxels < c.min_voxels) continue;
    rank[id] = (uint32_t)segs.size();
    kept_voxels += all[id].voxels;
    segs.push_back(all[id]);
  }
  if (total != selected) throw Error(LOAMX_E_INTERNAL, "segment: the components do not add up to the selected voxels");
  labels.clear();
  if (want_labels) {
    const unsigned long long* k = h_keys_.data();
    std::vector<std::pair<unsigned long long, uint32_t>> kv(occ);   // (key, label): sorted as records, the keys are distinct
    for (size_t j = 0; j < kv.size(); j++) {
      const uint32_t id = h_ids_.p[j];
      kv[j] = {k[j], id == DM_SEG_NONE ? DM_SEG_NONE : rank[id]};
    }
    std::sort(kv.begin(), kv.end());
    labels.resize(occ);
    for (size_t r = 0; r < kv.size(); r++) labels[r] = kv[r].second;
  }
  if (rank_of_id) rank_of_id->swap(rank);
  stats[0] = selected; stats[1] = n_roots; stats[2] = segs.size(); stats[3] = kept_voxels; stats[4] = largest; stats[5] = lost;
}

void dm_segment_check(const loamx_densemap_segment_config& c) {
  const int32_t lim = (1 << DM_QBITS) - 1;
  LX_REQUIRE(c.which <= LOAMX_SEGMENT_DYNAMIC, "which must be LOAMX_SEGMENT_ALL, _STATIC or _DYNAMIC");
  LX_REQUIRE(c.connectivity == 6u || c.connectivity == 18u || c.connectivity == 26u, "connectivity must be 6, 18 or 26");
  LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
  LX_REQUIRE(c.min_voxels >= 1u, "min_voxels must be >= 1");
  for (int a = 0; a < 3; a++) {
    const std::string ax = "[" + std::to_string(a) + "]";
    LX_REQUIRE(c.lo[a] >= -lim && c.lo[a] <= lim, "lo" + ax + " must be in [-(2^20 - 1), 2^20 - 1]");
    LX_REQUIRE(c.hi[a] >= -lim && c.hi[a] <= lim, "hi" + ax + " must be in [-(2^20 - 1), 2^20 - 1]");
    LX_REQUIRE(c.lo[a] <= c.hi[a], "lo" + ax + " must be <= hi" + ax);
  }
}

// include/loamx.h, loamx_densemap_segment: a checked configuration and rule.  LOAMX_E_CAPACITY: only the two counts are written
int DenseMap::segment(const loamx_densemap_segment_config& c, const loamx_densemap_static_rule& rule, uint32_t* labels, uint64_t label_capacity,
                      uint64_t* n_voxels, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[6]) {
  read_counters();   // (waits for every add; the exact voxel count)
  const uint64_t occ = occ_.occ;
  std::vector<uint32_t> lab;
  std::vector<loamx_segment> sg;
  uint64_t s[6] = {0, 0, 0, 0, 0, 0};
  if (occ) seg_.run(tab_, c, rule, occ, labels != nullptr, lab, sg, s, scan_, own_);
  *n_voxels = occ;
  *n_segs = sg.size();
  if ((labels && label_capacity < occ) || (segs && seg_capacity < sg.size())) return LOAMX_E_CAPACITY;
  if (labels && occ) memcpy(labels, lab.data(), sizeof(uint32_t) * occ);
  if (segs && !sg.empty()) memcpy(segs, sg.data(), sizeof(loamx_segment) * sg.size());
  memcpy(stats, s, sizeof(s));
  return LOAMX_OK;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_segment_default_config(loamx_densemap_segment_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->which = LOAMX_SEGMENT_ALL;
  cfg->connectivity = 26u;
  cfg->min_points = 1u;
  cfg->min_voxels = 1u;
  for (int a = 0; a < 3; a++) { cfg->lo[a] = -((1 << DM_QBITS) - 1); cfg->hi[a] = (1 << DM_QBITS) - 1; }
}

int loamx_densemap_segment_check(const loamx_densemap_segment_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_segment_check(*cfg);
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
    const loamx_densemap_segment_config c = or_default(cfg, loamx_densemap_segment_default_config);
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

int loamx_segment_box(const loamx_segment* s, float leaf, float lo_m[3], float hi_m[3], float centre[3]) {
  return guard([&]() {
    LX_REQUIRE(s, "s is NULL");
    LX_REQUIRE(lo_m, "lo_m is NULL");
    LX_REQUIRE(hi_m, "hi_m is NULL");
    LX_REQUIRE(centre, "centre is NULL");
    LX_REQUIRE(s->voxels != 0ull, "s: voxels is 0");
    for (int a = 0; a < 3; a++) {
      lo_m[a] = (float)((double)s->lo[a] * (double)leaf);
      hi_m[a] = (float)((double)(s->hi[a] + 1) * (double)leaf);
      centre[a] = (float)(((double)s->sum_idx[a] / (double)s->voxels + 0.5) * (double)leaf);
    }
    return LOAMX_OK;
  });
}

}  // extern "C"
