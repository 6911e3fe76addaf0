// What the dense map's connected-component labellers share on the device (densemap_segment.hip over the slots of the hash table,
// densemap_frontier.hip over the cells of the navigation grid) and, of the block compaction, densemap_region.hip too: the lock-free
// union-find, the ballot compaction of a 256-thread block and the claim of an entry in a block's LDS table of compact ids.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace loamx {

constexpr uint32_t DM_UF_NONE = 0xffffffffu;   // no element: a parent word outside every set; a walk that reached its bound
constexpr int DM_LDS_IDS = 256;                // entries of a reduce kernel's LDS table: the block's threads, the most ids it can meet

// ---- The union-find over an array parent[] of element indices (NONE: the element is in no set; such a word never changes and is
// never passed in here).  SCOPE is the memory scope of every access: __HIP_MEMORY_SCOPE_WORKGROUP for an array in LDS,
// __HIP_MEMORY_SCOPE_AGENT for one in HBM that other workgroups of the launch hook into.
//
// Why it is correct and why it ends.  Every element has a rank, distinct among the elements (a cell's index; a slot's key), and a
// union hooks the root of LARGER rank under the root of smaller rank by atomicCAS(&parent[hi], hi, lo), so the rank falls strictly
// along every parent chain: there are no cycles, a chain visits an element once, and the root of a finished set is its element of
// smallest rank whatever the schedule and whatever the layout.  An element that is no root never becomes one again, so any ancestor
// is a valid parent: find may halve the paths it walks while other threads hook.  A CAS is lost only because its root stopped being
// one, which happens once per element; the union then starts again from the finds.  No thread waits for another: no spin-wait, no
// grid barrier.  Every word another workgroup may write in the launch is read and written with relaxed atomics of SCOPE.
//
// The proof gives the bounds, and the code holds them anyway (a kernel that cannot end is the worst failure on a shared device):
// with `bound` = the number of elements, a walk takes at most `bound` steps and a union at most `bound + 1` tries.  A bound that is
// reached comes back as NONE / false; the caller raises a counter word and the host reports LOAMX_E_INTERNAL.

template <int SCOPE> __device__ inline uint32_t dm_uf_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root above x, halving the path on the way
template <int SCOPE> __device__ inline uint32_t dm_uf_find(uint32_t* parent, uint32_t x, uint32_t bound) {
  for (uint32_t k = 0; k < bound; k++) {
    const uint32_t p = dm_uf_load<SCOPE>(&parent[x]);
    if (p == x) return x;
    const uint32_t g = dm_uf_load<SCOPE>(&parent[p]);
    if (g == p) return p;
    __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, SCOPE);   // (x is no root and stays none: g is an ancestor)
    x = g;
  }
  return DM_UF_NONE;
}

// the root above x by the plain walk, nothing written: for the flatten pass, where every thread stores its own element's root
template <int SCOPE> __device__ inline uint32_t dm_uf_root(const uint32_t* parent, uint32_t x, uint32_t bound) {
  for (uint32_t k = 0; k < bound; k++) {
    const uint32_t p = dm_uf_load<SCOPE>(&parent[x]);
    if (p == x) return x;
    x = p;
  }
  return DM_UF_NONE;
}

// the sets of a and b become one.  rank(e): the rank of element e (above); lost: counts the CASes lost.  false: a bound was reached
template <int SCOPE, class Rank>
__device__ inline bool dm_uf_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t bound, Rank rank, uint32_t& lost) {
  bool ok = true;
  uint32_t tries = 0u;
  for (; tries <= bound; tries++) {   // (the loop breaks and the count is tested behind it: the shape the compiler does best with)
    a = dm_uf_find<SCOPE>(parent, a, bound);
    b = dm_uf_find<SCOPE>(parent, b, bound);
    if (a == DM_UF_NONE || b == DM_UF_NONE) { ok = false; break; }
    if (a == b) break;
    if (rank(a) < rank(b)) { const uint32_t t = a; a = b; b = t; }   // a: the root of larger rank
    if (atomicCAS(&parent[a], a, b) == a) break;
    lost++;   // (a was hooked by another thread meanwhile: from the finds again)
  }
  return ok && tries <= bound;
}

// ---- The compaction of one flag per thread in a block of 256 threads, four waves: a ballot, one count per wave in LDS, one barrier.
// Every thread of the block calls; a kernel calls one form, once (a second call would write the words while a slow wave reads them).

__device__ inline uint32_t* dm_block_words() {
  __shared__ uint32_t w[4];
  return w;
}
// the ballot of the wave, behind the block's barrier: the four waves' counts stand in dm_block_words()
__device__ inline unsigned long long dm_block_vote(bool flag) {
  uint32_t* w = dm_block_words();
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  return m;
}
// the block's number of set flags; read it in thread 0
__device__ inline uint32_t dm_block_count(bool flag) {
  dm_block_vote(flag);
  const uint32_t* w = dm_block_words();
  return w[0] + w[1] + w[2] + w[3];
}
// the same of two flags behind one barrier
__device__ inline void dm_block_count2(bool fa, bool fb, uint32_t& na, uint32_t& nb) {
  __shared__ uint32_t wa[4], wb[4];
  const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
  if ((threadIdx.x & 63) == 0) { wa[threadIdx.x >> 6] = (uint32_t)__popcll(ma); wb[threadIdx.x >> 6] = (uint32_t)__popcll(mb); }
  __syncthreads();
  na = wa[0] + wa[1] + wa[2] + wa[3];
  nb = wb[0] + wb[1] + wb[2] + wb[3];
}
// base + the number of set flags in the threads below this one, from the ballot m that dm_block_vote gave: behind the exclusive scan
// of the blocks' counts, with the block's offset as base, the place of this thread's element among the flagged ones.  In two steps,
// so that the threads without a flag can leave in between, before base is read
__device__ inline uint32_t dm_block_rank(unsigned long long m, uint32_t base) {
  const uint32_t* w = dm_block_words();
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  uint32_t n = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wid; k++) n += w[k];
  return n;
}

// ---- The entry of a compact id in a block's table s_id[DM_LDS_IDS] in LDS (every word NONE at the start): open addressing from
// id % 256; a block meets at most 256 ids, so a probe always ends
__device__ inline uint32_t dm_lds_claim(uint32_t* s_id, uint32_t id) {
  uint32_t h = id & (DM_LDS_IDS - 1);
  for (int probe = 0; probe < DM_LDS_IDS; probe++) {
    const uint32_t prev = atomicCAS(&s_id[h], DM_UF_NONE, id);
    if (prev == DM_UF_NONE || prev == id) break;
    h = (h + 1u) & (DM_LDS_IDS - 1);
  }
  return h;
}

}  // namespace loamx
