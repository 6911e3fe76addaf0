// Bucketed voxel grid of the registration's stack clouds (see voxbucket.hpp).  gfx950, wave64.
#include "voxbucket.hpp"
#include "scan.hpp"
#include "voxel.hpp"

namespace loamx {

struct VbArgs {
  const float4* in;             // concatenated input points, or
  const float4* const* src;     // one pointer per segment
  const uint32_t* seg_off;      // [nseg + 1]
  const Pose* poses;            // per sweep (segment / 2)
  VbSeg* segs;
  unsigned long long* lo;       // per bucket: smallest voxel key
  VbBk* bk;                     // per bucket: what k_vb_reduce needs of its segment, in one record
  int* box;                     // [nseg][6]
  uint32_t* cnt;
  uint32_t* heads;
  uint32_t* ctl;                // [0] fail epoch, [1] buckets of k_vb_reduce that have arrived (back to 0 when the last one has)
  uint32_t* h_fail;             // pinned: [0] fail epoch, [1] timeout, [2 + r] epoch of the last run that met reason r
  uint16_t* bword;              // per point: bucket inside its segment, or VB_REFUSED
  uint2* crange;                // per chunk: smallest / largest bucket of its accepted points ({~0, 0}: none)
  VbPoseInit init;
  float4* stack;
  float4* out;
  uint32_t* out_off;
  uint32_t n, nseg, nb, epoch;
  float inv_even, inv_odd;
  unsigned long long* dbg;      // LOAMX_PROF_VB: per bucket 16 wall-clock stamps of k_vb_reduce
};

__device__ inline uint32_t vb_bits(unsigned long long v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }
// reasons (h_fail[2 + reason] = epoch, for the diagnostics of VoxBucket::why()): 0 a coordinate beyond +-2^20 voxels (or not finite),
// 1 more buckets than a segment may have, 2 segment box beyond INT_MAX voxels (PCL passes the cloud through), 3 a bucket whose own
// box needs more than 64 sort bits, 5 a bucket over capacity
__device__ inline void vb_fail(const VbArgs& A, int reason) {
  A.ctl[0] = A.epoch;      // (every writer stores the same value)
  A.h_fail[0] = A.epoch;
  A.h_fail[2 + reason] = A.epoch;
}
// a give-up raised INSIDE k_vb_reduce, by one thread of the bucket: the device word also goes out write-through (agent scope), so that the
// bucket that arrives last (vb_arrive) sees it whichever XCD raised it; a plain store would stay in the raising XCD's L2 until the
// kernel ends.  (k_vb_plan and k_vb_stack end before k_vb_reduce starts: their plain stores are visible to it.)
__device__ inline void vb_fail_reduce(const VbArgs& A, int reason) {
  vb_fail(A, reason);
  __hip_atomic_store(&A.ctl[0], A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// "The kernels leave an empty result": every bucket of k_vb_reduce arrives ONCE (ctl[1]), after its offsets and its give-up, if any,
// have been stored write-through and have completed; the bucket that arrives last therefore stores behind every other bucket's
// offsets, and zeroes them when the run has given up.  (Before, only a bucket that found the fail word up when it STARTED zeroed
// them: a give-up raised inside the kernel — reason 2, by the last bucket, at its end; reason 3 — left the offsets of a run that
// looked complete.  The registration never read them: it tests the fail word.)  One thread per bucket; vb_arrive_last() by the same
// thread, later, with the value vb_arrive() returned.
__device__ inline uint32_t vb_arrive(const VbArgs& A) {
  xchg_stores_done();
  return __hip_atomic_fetch_add(&A.ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void vb_arrive_last(const VbArgs& A, uint32_t before) {
  if (before + 1u != A.nb) return;
  __hip_atomic_store(&A.ctl[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (for the next run)
  if (__hip_atomic_load(&A.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.epoch) return;
  for (uint32_t s = 0; s <= A.nseg; s++) __hip_atomic_store(&A.out_off[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// voxel coordinate of one axis exactly as pcl::VoxelGrid forms it: floor(v * inverse leaf), float arithmetic
constexpr int VB_OFF = 1 << 20;
__device__ inline bool vb_voxel(float v, float inv, int& i) {
  const float f = floorf(v * inv);
  if (!(fabsf(f) < (float)VB_OFF)) return false;   // also catches NaN / inf
  i = (int)f;
  return true;
}
// voxel order = pcl::VoxelGrid's linear index order inside any box: (iz, iy, ix) lexicographically
__device__ inline unsigned long long vb_key(int ix, int iy, int iz) {
  return ((unsigned long long)(uint32_t)(iz + VB_OFF) << 42) | ((unsigned long long)(uint32_t)(iy + VB_OFF) << 21) | (unsigned long long)(uint32_t)(ix + VB_OFF);
}

// ----------------------------------------------------------------------------------------------------------------
// k_vb_plan: grid = segments x VB_PLAN_PARTS, VB_SAMPLE threads.  Ranking the sample is 512 x 512 key compares, the arithmetic of one
// CU for ~10 us: the VB_PLAN_PARTS workgroups of a segment each take the sample (every one loads it) and rank a quarter of its keys,
// four threads to a key, each against a quarter of the sample.  Nothing is sorted into a table: the thread that finds its key at
// rank k * m / buckets IS splitter k and stores it.  Part 0 writes the rest of the segment's plan; the last part of an even segment
// sets its sweep up (VbPoseInit).
// ----------------------------------------------------------------------------------------------------------------
constexpr int VB_PLAN_PARTS = 4, VB_PLAN_KEYS = VB_SAMPLE / VB_PLAN_PARTS;
__global__ __launch_bounds__(VB_SAMPLE) void k_vb_plan(const VbArgs A) {
  __shared__ alignas(16) unsigned long long s_key[VB_SAMPLE];
  __shared__ uint32_t s_part[VB_PLAN_PARTS][VB_PLAN_KEYS];
  __shared__ uint32_t s_scan[17];
  __shared__ uint32_t s_bad;
  const int tid = (int)threadIdx.x;
  const uint32_t seg = blockIdx.x / VB_PLAN_PARTS, part = blockIdx.x % VB_PLAN_PARTS;
  const uint32_t a0 = A.seg_off[seg], ns = A.seg_off[seg + 1] - a0;
  const float4* __restrict__ pts = A.src ? A.src[seg] : A.in + a0;
  const float inv = (seg & 1) ? A.inv_odd : A.inv_even;
  // the registration's set-up of sweep seg / 2 (k_pose_init's stores, word for word): k_vb_stack, one launch later, reads the pose.
  // The twelve words of the pose one to a lane — sine and cosine through double, then rounded (pose_set_angles).
  if (A.init.guess && part == VB_PLAN_PARTS - 1 && !(seg & 1u) && (seg >> 1) < A.init.ns) {
    const uint32_t s = seg >> 1;
    if (tid < 12) {
      A.init.seg_minmax[12 * s + tid] = (tid % 6) < 3 ? 2147483647 : (-2147483647 - 1);
      const float* __restrict__ g = A.init.guess + 6 * s;
      float v;
      if (tid < 6) v = g[tid];
      else {
        const float ang = g[(tid - 6) >> 1];
        v = (float)((tid & 1) ? cos((double)ang) : sin((double)ang));
      }
      reinterpret_cast<float*>(A.init.poses + s)[tid] = v;
    }
    if (tid >= 64 && tid < 72) A.init.stats[8 * s + (tid - 64)] = 0;
    if (tid == 72) { A.init.ticket[s] = 0u; A.init.full_done[s] = 0u; }
  }
  // first bucket of this segment: every segment owns max(1, ceil(points / T)) buckets
  uint32_t bucket0;
  {
    uint32_t sum = 0;
    for (uint32_t s = (uint32_t)tid; s < seg; s += VB_SAMPLE) {
      const uint32_t m = A.seg_off[s + 1] - A.seg_off[s];
      sum += m ? (m + VB_T - 1) / VB_T : 1u;
    }
    uint32_t tot;
    (void)block_excl_scan(sum, s_scan, tot);
    bucket0 = tot;
  }
  const uint32_t nbuckets = ns ? (ns + VB_T - 1) / VB_T : 1u;
  const uint32_t m = ns < (uint32_t)VB_SAMPLE ? ns : (uint32_t)VB_SAMPLE;
  if (tid == 0) s_bad = nbuckets > (uint32_t)VB_SAMPLE ? 2u : 0u;
  __syncthreads();
  unsigned long long key = ~0ull;
  if (nbuckets > 1u && (uint32_t)tid < m) {   // (one bucket needs no splitter)
    const float4 p = pts[(uint32_t)(((unsigned long long)tid * ns) / m)];
    int v[3];
    if (vb_voxel(p.x, inv, v[0]) && vb_voxel(p.y, inv, v[1]) && vb_voxel(p.z, inv, v[2])) key = vb_key(v[0], v[1], v[2]);
    else atomicOr(&s_bad, 1u);
  }
  s_key[tid] = key;
  __syncthreads();
  const uint32_t bad = s_bad;
  // rank among the sample (ties by sample position) of key `own`, this thread's quarter of the sample: 16 keys (eight 16-byte LDS
  // broadcasts) in flight at a time.  The entries behind the sample hold ~0, which is below no key and, as a tie, lies behind every
  // key that is ranked (u >= m > own): the ranks are those of the sample.
  const uint32_t own = part * VB_PLAN_KEYS + ((uint32_t)tid % VB_PLAN_KEYS), quarter = (uint32_t)tid / VB_PLAN_KEYS;
  const bool ranked = nbuckets > 1u && !bad && own < m;
  if (ranked) {
    const unsigned long long mine = s_key[own];
    const ulonglong2* __restrict__ k2 = reinterpret_cast<const ulonglong2*>(s_key);
    uint32_t r = 0;
    for (uint32_t u = quarter * VB_PLAN_KEYS; u < (quarter + 1u) * VB_PLAN_KEYS; u += 16u) {
      ulonglong2 k[8];
#pragma unroll
      for (int q = 0; q < 8; q++) k[q] = k2[(u >> 1) + (uint32_t)q];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t ua = u + 2u * (uint32_t)q;
        r += (k[q].x < mine || (k[q].x == mine && ua < own)) ? 1u : 0u;
        r += (k[q].y < mine || (k[q].y == mine && ua + 1u < own)) ? 1u : 0u;
      }
    }
    s_part[quarter][(uint32_t)tid % VB_PLAN_KEYS] = r;
  }
  __syncthreads();
  if (ranked && tid < VB_PLAN_KEYS) {
    uint32_t r = 0;
#pragma unroll
    for (int q = 0; q < VB_PLAN_PARTS; q++) r += s_part[q][tid];
    // splitter k (1 <= k < buckets) is the key of rank k * m / buckets: at most one k for a rank (m >= buckets)
    const uint32_t k = (uint32_t)(((unsigned long long)r * nbuckets + m - 1u) / m);
    if (k >= 1u && k < nbuckets && (uint32_t)(((unsigned long long)k * m) / nbuckets) == r) A.lo[bucket0 + k] = s_key[own];
  }
  if (part != 0u) return;
  if (bad && tid == 0) vb_fail(A, (bad & 2u) ? 1 : 0);
  for (uint32_t k = (uint32_t)tid; k < nbuckets && k < (uint32_t)VB_SAMPLE; k += VB_SAMPLE) {
    if (k == 0u || bad) A.lo[bucket0 + k] = 0ull;
    VbBk K;
    K.seg = seg; K.sbeg = a0; K.send = a0 + ns; K.bucket0 = bucket0;
    K.pos_bits = vb_bits(ns ? (unsigned long long)(ns - 1) : 0ull);
    if (K.pos_bits == 0) K.pos_bits = 1;
    K.pad[0] = K.pad[1] = K.pad[2] = 0u;
    A.bk[bucket0 + k] = K;
    A.cnt[bucket0 + k] = 0u;
    A.heads[bucket0 + k] = 0u;
  }
  if (tid < 6) A.box[6 * seg + tid] = tid < 3 ? 2147483647 : (-2147483647 - 1);
  if (tid == 0) {
    VbSeg P;
    P.bucket0 = bucket0;
    P.nbuckets = bad ? 0u : nbuckets;   // a given-up segment takes no points (its points raise the fail word again, harmlessly)
    P.pos_bits = vb_bits(ns ? (unsigned long long)(ns - 1) : 0ull);
    if (P.pos_bits == 0) P.pos_bits = 1;
    P.pad = 0u;
    A.segs[seg] = P;
  }
}

// ----------------------------------------------------------------------------------------------------------------
// k_vb_stack: grid = ceil(n / VB_CHUNK), VB_CHUNK threads (a workgroup = a chunk of the bucket words)
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VB_CHUNK) void k_vb_stack(const VbArgs A) {
  __shared__ unsigned long long s_lo[64];   // the splitters of the segment of the workgroup's first point
  __shared__ uint32_t s_tag[256], s_cnt[256], s_gbase[256];
  __shared__ uint32_t s_gmin, s_gmax;       // the chunk's bucket range
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t lead = vox_find_seg(A.seg_off, A.nseg, blockIdx.x * blockDim.x);
  const VbSeg PL = A.segs[lead];
  if (threadIdx.x < 64) s_lo[threadIdx.x] = threadIdx.x < PL.nbuckets ? A.lo[PL.bucket0 + threadIdx.x] : ~0ull;
  s_tag[threadIdx.x] = 0xffffffffu;
  s_cnt[threadIdx.x] = 0u;
  if (threadIdx.x == 0) { s_gmin = 0xffffffffu; s_gmax = 0u; }
  __syncthreads();
  bool act = i < A.n;
  uint32_t g = 0u, rel = 0u;
  if (act) {
    const uint32_t seg = vox_find_seg(A.seg_off, A.nseg, i);
    const uint32_t a0 = A.seg_off[seg];
    const Pose T = A.poses[seg >> 1];
    const float4 p = A.src ? A.src[seg][i - a0] : A.in[i];
    float x = p.x, y = p.y, z = p.z;
    to_map(T, x, y, z);          // BasicLaserMapping.cpp:282-292 via :512-516
    to_be_mapped(T, x, y, z);
    A.stack[i] = make_float4(x, y, z, p.w);
    const float inv = (seg & 1) ? A.inv_odd : A.inv_even;
    int v[3];
    const VbSeg P = seg == lead ? PL : A.segs[seg];
    if (!(vb_voxel(x, inv, v[0]) && vb_voxel(y, inv, v[1]) && vb_voxel(z, inv, v[2])) || P.nbuckets == 0u) {
      vb_fail(A, 0);
      act = false;
    } else {
      const unsigned long long key = vb_key(v[0], v[1], v[2]);
      // bucket = number of splitters (of buckets 1 ..) that are <= key
      uint32_t lo = 0u, hi = P.nbuckets;   // splitter[lo] <= key < splitter[hi]  (splitter[0] = 0, splitter[nbuckets] = infinity)
      if (seg == lead && P.nbuckets <= 64u) {
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_lo[mid] <= key) lo = mid; else hi = mid; }
      } else {
        const unsigned long long* __restrict__ sp = A.lo + P.bucket0;
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (sp[mid] <= key) lo = mid; else hi = mid; }
      }
      g = P.bucket0 + lo;
      rel = lo;
    }
    A.bword[i] = act ? (uint16_t)rel : VB_REFUSED;
  }
  {   // the chunk's bucket range: one LDS atomic pair per wave
    uint32_t gmn = act ? g : 0xffffffffu, gmx = act ? g : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t a = (uint32_t)__shfl_xor((int)gmn, d, 64), b = (uint32_t)__shfl_xor((int)gmx, d, 64);
      gmn = a < gmn ? a : gmn;
      gmx = b > gmx ? b : gmx;
    }
    if (lane == 0 && gmn != 0xffffffffu) { atomicMin(&s_gmin, gmn); atomicMax(&s_gmax, gmx); }
  }
  // Counts (a point's rank in its bucket only decides whether the bucket is over capacity): the lanes of a wave that go to the same bucket are counted together, the waves of the workgroup meet in an LDS table
  // (256 entries, bucket % 256 with a tag: the buckets a workgroup touches are a few neighbours of one or two segments), and ONE
  // thread per touched bucket bumps the global counter — hundreds of waves hammering ~150 counters serialise in memory otherwise.
  // A bucket that finds its table entry taken by another one goes to the global counter directly.
  unsigned long long rem = __ballot(act);
  uint32_t slot = 0u;      // rank inside the workgroup's share of the bucket (table path) or the final slot (direct path)
  bool direct = false;
  while (rem) {
    const int l0 = __builtin_ctzll(rem);
    const uint32_t g0 = (uint32_t)__shfl((int)g, l0, 64);
    const unsigned long long m = __ballot(act && g == g0);
    uint32_t base = 0u, dir = 0u;
    if (lane == l0) {
      const uint32_t h = g0 & 255u;
      const uint32_t old = atomicCAS(&s_tag[h], 0xffffffffu, g0);
      if (old == 0xffffffffu || old == g0) base = atomicAdd(&s_cnt[h], (uint32_t)__popcll(m));
      else { base = atomicAdd(&A.cnt[g0], (uint32_t)__popcll(m)); dir = 1u; }
    }
    base = (uint32_t)__shfl((int)base, l0, 64);
    dir = (uint32_t)__shfl((int)dir, l0, 64);
    if (act && g == g0) { slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); direct = dir != 0u; }
    rem &= ~m;
  }
  __syncthreads();
  if (s_tag[threadIdx.x] != 0xffffffffu) s_gbase[threadIdx.x] = atomicAdd(&A.cnt[s_tag[threadIdx.x]], s_cnt[threadIdx.x]);
  __syncthreads();
  if (act) {
    if (!direct) slot += s_gbase[g & 255u];
    if (slot >= (uint32_t)VB_CAP) vb_fail(A, 5);
  }
  if (threadIdx.x == 0) A.crange[blockIdx.x] = make_uint2(s_gmin, s_gmax);   // (behind the two barriers above)
}

// ----------------------------------------------------------------------------------------------------------------
// k_vb_reduce: grid = buckets, VB_CAP / 8 threads, 8 elements per thread
// ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t VB_SPIN_LIMIT = 1u << 20;
#ifdef LOAMX_PROF_VB
#define VB_TS(k) do { if (threadIdx.x == 0) A.dbg[(size_t)blockIdx.x * 16 + (k)] = wall_clock64(); } while (0)
#else
#define VB_TS(k) do { } while (0)
#endif
constexpr int VB_THREADS = VB_CAP / 8, VB_WAVES = VB_THREADS / 64;
// the points of bucket-inside-segment `want` among the eight bucket words of one 16-byte group, as a bit mask (little-endian halves:
// the low one is the earlier point)
__device__ inline uint32_t vb_match8(const uint4& v, uint32_t want) {
  const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0u;
#pragma unroll
  for (int h = 0; h < 4; h++) {
    m |= ((w4[h] & 0xffffu) == want ? 1u : 0u) << (2 * h);
    m |= ((w4[h] >> 16) == want ? 1u : 0u) << (2 * h + 1);
  }
  return m;
}

// adds the sorted elements [l, min(l + W, l_end)) to a voxel's sums, in order; W reads in flight
template <int W>
__device__ inline void vb_sum_run(const unsigned long long* s_w, const float4* s_pts, uint32_t l, uint32_t l_end, uint32_t c, uint32_t emask,
                                  float& sx, float& sy, float& sz, float& si) {
  float4 ts[W];
#pragma unroll
  for (int q = 0; q < W; q++) ts[q] = s_pts[(uint32_t)s_w[min(l + (uint32_t)q, c)] & emask];   // (behind the run: any point, unused)
#pragma unroll
  for (int q = 0; q < W; q++) {
    if (l + (uint32_t)q < l_end) { sx += ts[q].x; sy += ts[q].y; sz += ts[q].z; si += ts[q].w; }
  }
}

__global__ __launch_bounds__(VB_THREADS) void k_vb_reduce(const VbArgs A) {
  // the bucket's points, gathered ONCE, at their rank e in input order; they stay for the whole kernel (one workgroup per CU)
  __shared__ float4 s_pts[VB_CAP];
  // the sort's words (every thread holds its eight words in registers while a pass scatters); before the sort, the collected input
  // positions (4 B each) live in the same buffer
  __shared__ alignas(16) unsigned long long s_w[VB_CAP + 8];
  uint32_t* s_pos = (uint32_t*)s_w;
  __shared__ uint32_t s_wcnt[VB_WAVES][256];
  __shared__ uint32_t s_base[256];
  __shared__ uint32_t s_scan[17];
  __shared__ uint32_t s_pk[VB_WAVES][4];
  __shared__ int s_box[6];
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // workgroups start in index order, so everything a look-back waits for is already running (or done)
  const uint32_t b = blockIdx.x;
  VB_TS(0);
  if (__hip_atomic_load(&A.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.epoch) {   // given up: an empty, well-formed result
    //  EVERY bucket publishes a count — a bucket that started before the give-up may be looking back at this one —
    // and arrives: the offsets are zeroed by whichever bucket arrives last (vb_arrive), behind every bucket that ran to its end and
    // wrote some — the Gauss-Newton launches already enqueued behind this kernel read them
    if (tid == 0) {
      __hip_atomic_store(&A.heads[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      vb_arrive_last(A, vb_arrive(A));
    }
    return;
  }
  const VbBk K = A.bk[b];   // (one round trip: segment, its range, its first bucket, its position bits)
  const uint32_t seg = K.seg, sbeg = K.sbeg, send = K.send;
  const float inv = (seg & 1) ? A.inv_odd : A.inv_even;
  const uint32_t pbits = K.pos_bits;
  if (tid < 6) s_box[tid] = tid < 3 ? 2147483647 : (-2147483647 - 1);
  // ---- collect: the input positions of the bucket's points, in input order.  The segment's bucket words are scanned in rounds of
  // eight steps; in a step the workgroup takes 4096 consecutive points, thread t the eight words (16 bytes) from 8 t — so a stretch
  // of input that belongs to this bucket spreads over all threads.  A round's eight loads per thread are independent; its matches
  // are ordered by (step, thread, word): the eight per-step counts of a thread travel as 16-bit fields of four words through ONE
  // scan over the workgroup (a count is at most 4096).  Segments of more than one round (over 32 Ki points) first look at the
  // chunk's bucket range and leave out the chunks that cannot hold the bucket; shorter ones load everything at once, which costs
  // less than the dependent round trip.  A chunk at a segment boundary holds the neighbour's words, which may be equal, and the
  // words behind the run's last point are never written: only points of [sbeg, send) count.
  const uint32_t want = b - K.bucket0;
  const uint32_t o0 = sbeg / 8u, o1 = send > sbeg ? (send + 7u) / 8u : o0;   // the 16-byte groups the segment meets
  const uint32_t nround = (o1 - o0 + 8u * (uint32_t)VB_THREADS - 1u) / (8u * (uint32_t)VB_THREADS);
  const bool skip = nround > 1u;
  const uint4* __restrict__ bw = reinterpret_cast<const uint4*>(A.bword);
  uint32_t found = 0u;   // (block-uniform) matches of the rounds so far
  for (uint32_t r = 0; r < nround; r++) {
    uint4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t o = o0 + (r * 8u + (uint32_t)k) * (uint32_t)VB_THREADS + (uint32_t)tid;
      bool ld = o < o1;
      if (ld && skip) {
        const uint2 cr = A.crange[o / (VB_CHUNK / 8u)];
        ld = b >= cr.x && b <= cr.y;
      }
      v[k] = ld ? bw[o] : make_uint4(~0u, ~0u, ~0u, ~0u);   // (VB_REFUSED: matches nothing)
    }
    uint32_t mk[8], pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t o = o0 + (r * 8u + (uint32_t)k) * (uint32_t)VB_THREADS + (uint32_t)tid;
      uint32_t m = 0u;
      if (o < o1) {
        const uint32_t i0 = o * 8u;
        const uint32_t lo = sbeg > i0 ? sbeg - i0 : 0u;                 // < 8: the group meets the segment
        const uint32_t hi = send - i0 < 8u ? send - i0 : 8u;            // >= 1
        m = vb_match8(v[k], want) & (0xffu << lo) & (0xffu >> (8u - hi));
      }
      mk[k] = m;
      pk[k >> 1] |= (uint32_t)__popc(m) << (16 * (k & 1));
    }
    uint32_t inc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      inc[q] = wave_incl_scan(pk[q], lane);
      if (lane == 63) s_pk[wid][q] = inc[q];
    }
    __syncthreads();
    uint32_t before[4] = {0u, 0u, 0u, 0u}, all[4] = {0u, 0u, 0u, 0u};   // fields: matches in the waves before this one / in all waves
#pragma unroll
    for (int u = 0; u < VB_WAVES; u++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t t = s_pk[u][q];
        all[q] += t;
        before[q] += u < wid ? t : 0u;
      }
    }
    uint32_t step_base = found;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int q = k >> 1, sh = 16 * (k & 1);
      uint32_t off = step_base + ((before[q] >> sh) & 0xffffu) + ((inc[q] >> sh) & 0xffffu) - ((pk[q] >> sh) & 0xffffu);
      const uint32_t rel = (o0 + (r * 8u + (uint32_t)k) * (uint32_t)VB_THREADS + (uint32_t)tid) * 8u - sbeg;   // (may wrap for the segment's first group: the set bits bring it back)
      uint32_t m = mk[k];
      while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        if (off < (uint32_t)VB_CAP) s_pos[off] = rel + bit;
        off++;
      }
      step_base += (all[q] >> sh) & 0xffffu;
    }
    found = step_base;
    __syncthreads();   // (the wave totals are read; after the last round: the positions are written)
  }
  const uint32_t c = min(found, (uint32_t)VB_CAP);   // (= cnt[b]: a bucket over capacity has given the run up in k_vb_stack)
  VB_TS(15);
  // ---- slots: the eight waves share the c elements evenly, wave w takes the S consecutive ranks from w * S (S a multiple of 64), in
  // rank order — so "wave, then step, then lane" is rank order, which is what keeps the counting sort stable
  const uint32_t S = ((c + (uint32_t)VB_CAP / 8u - 1u) / ((uint32_t)VB_CAP / 8u)) * 64u;
  const uint32_t w0 = (uint32_t)wid * S;
#define VB_SLOT(j) (w0 + (uint32_t)(j) * 64u + (uint32_t)lane)
#define VB_LIVE(j, i) ((uint32_t)(j) * 64u < S && (i) < c)
  // ---- the elements' points (into LDS at their rank), their voxels (recomputed from the stack points: the same floor(x / leaf)
  // k_vb_stack took) and the bucket's box
  int vx[8], vy[8], vz[8];
  {
    float4 pt[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t i = VB_SLOT(j);
      pt[j] = VB_LIVE(j, i) ? A.stack[sbeg + s_pos[i]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int mn[3] = {2147483647, 2147483647, 2147483647}, mx[3] = {-2147483647 - 1, -2147483647 - 1, -2147483647 - 1};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t i = VB_SLOT(j);
      vx[j] = vy[j] = vz[j] = 0;
      if (VB_LIVE(j, i)) {
        s_pts[i] = pt[j];
        (void)vb_voxel(pt[j].x, inv, vx[j]); (void)vb_voxel(pt[j].y, inv, vy[j]); (void)vb_voxel(pt[j].z, inv, vz[j]);
        mn[0] = vx[j] < mn[0] ? vx[j] : mn[0]; mx[0] = vx[j] > mx[0] ? vx[j] : mx[0];
        mn[1] = vy[j] < mn[1] ? vy[j] : mn[1]; mx[1] = vy[j] > mx[1] ? vy[j] : mx[1];
        mn[2] = vz[j] < mn[2] ? vz[j] : mn[2]; mx[2] = vz[j] > mx[2] ? vz[j] : mx[2];
      }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const int lo = __shfl_xor(mn[a], d, 64), hi = __shfl_xor(mx[a], d, 64);
        mn[a] = lo < mn[a] ? lo : mn[a];
        mx[a] = hi > mx[a] ? hi : mx[a];
      }
    }
    if (lane == 0 && w0 < c) {
#pragma unroll
      for (int a = 0; a < 3; a++) { atomicMin(&s_box[a], mn[a]); atomicMax(&s_box[3 + a], mx[a]); }
    }
  }
  __syncthreads();   // (also: every thread has read its positions, the buffer may take the sort's words)
  VB_TS(1);
  unsigned long long dimx = 1ull, dimy = 1ull, dimz = 1ull;
  int bx0 = 0, by0 = 0, bz0 = 0;
  if (c) {
    bx0 = s_box[0]; by0 = s_box[1]; bz0 = s_box[2];
    dimx = (unsigned long long)(s_box[3] - bx0 + 1); dimy = (unsigned long long)(s_box[4] - by0 + 1); dimz = (unsigned long long)(s_box[5] - bz0 + 1);
    if (tid < 6) {   // the segment's box, for PCL's pass-through test by the last bucket (released by the fence in front of the head count)
      if (tid < 3) atomicMin(&A.box[6 * seg + tid], s_box[tid]); else atomicMax(&A.box[6 * seg + tid], s_box[tid]);
    }
  }
  const uint32_t key_bits = vb_bits(dimx * dimy * dimz - 1ull);   // each extent < 2^21
  // The give-up rule is the one of the sort on (voxel index, input position): the sort below needs fewer bits and could go on, but
  // the set of inputs that give up is part of the stage's contract.
  const uint32_t total_bits = (key_bits ? key_bits : 1u) + pbits;
  if (total_bits > 63u) {   // (block-uniform)
    if (tid == 0) vb_fail_reduce(A, 3);
  }
  // sort word: voxel index inside the bucket's box << ebits | rank e in input order — all distinct.  ebits = min(pos_bits, 12) holds
  // every rank (c <= points of the segment <= 2^pos_bits, c <= VB_CAP), and key_bits + ebits <= 63 wherever the run goes on.  Only
  // the voxel bits are sorted on: the words arrive in rank order and every pass is stable.
  const uint32_t ebits = pbits < (uint32_t)VB_CAP_LOG2 ? pbits : (uint32_t)VB_CAP_LOG2;
  const uint32_t emask = (1u << ebits) - 1u;
  const uint32_t npass = total_bits > 63u ? 0u : ((key_bits ? key_bits : 1u) + 7u) / 8u;
  unsigned long long w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t i = VB_SLOT(j);
    const unsigned long long lin = (unsigned long long)(vx[j] - bx0) + dimx * ((unsigned long long)(vy[j] - by0) + dimy * (unsigned long long)(vz[j] - bz0));
    w[j] = VB_LIVE(j, i) ? ((lin << ebits) | (unsigned long long)i) : ~0ull;
  }
  const bool wave_has = w0 < c;   // wave-uniform: a wave without elements only keeps the barriers
  if (npass == 0u) {   // (given up: keep the buffer defined)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t i = VB_SLOT(j);
      if (VB_LIVE(j, i)) s_w[i] = w[j];
    }
    __syncthreads();
  }
  for (uint32_t p = 0; p < npass; p++) {
    const uint32_t shift = ebits + 8u * p;
    VB_TS(2 + (p < 7u ? p : 7u));
    if (tid < 256) {
#pragma unroll
      for (int k = 0; k < VB_WAVES; k++) s_wcnt[k][tid] = 0u;
    }
    __syncthreads();
    uint32_t rank[8];
#pragma unroll
    for (int j = 0; j < 8; j++) rank[j] = 0u;
    if (wave_has) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if ((uint32_t)j * 64u < S) {   // (wave-uniform)
          const uint32_t i = VB_SLOT(j);
          const bool in = i < c;
          const uint32_t d = (uint32_t)((w[j] >> shift) & 255ull);
          unsigned long long m = __ballot(in);
#pragma unroll
          for (int bit = 0; bit < 8; bit++) {
            const unsigned long long bal = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? bal : ~bal;
          }
          const unsigned long long below = m & ((1ull << lane) - 1ull);
          const int leader = __builtin_ctzll(m | (1ull << 63));
          uint32_t old = 0u;
          if (in && lane == leader) {
            old = s_wcnt[wid][d];
            s_wcnt[wid][d] = old + (uint32_t)__popcll(m);
          }
          old = (uint32_t)__shfl((int)old, leader, 64);
          rank[j] = old + (uint32_t)__popcll(below);
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    __syncthreads();
    {   // thread d < 256: exclusive prefix over the waves, then (all threads) over the digits
      uint32_t run = 0u;
      if (tid < 256) {
#pragma unroll
        for (int k = 0; k < VB_WAVES; k++) { const uint32_t v = s_wcnt[k][tid]; s_wcnt[k][tid] = run; run += v; }
      }
      uint32_t tot;
      const uint32_t ex = block_excl_scan(run, s_scan, tot);
      if (tid < 256) s_base[tid] = ex;
    }
    __syncthreads();   // (also: every thread has its words in registers, the buffer may be overwritten)
    if (wave_has) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint32_t i = VB_SLOT(j);
        if (VB_LIVE(j, i)) {
          const uint32_t d = (uint32_t)((w[j] >> shift) & 255ull);
          s_w[s_base[d] + s_wcnt[wid][d] + rank[j]] = w[j];
        }
      }
    }
    __syncthreads();
    if (p + 1 < npass) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint32_t i = VB_SLOT(j);
        w[j] = VB_LIVE(j, i) ? s_w[i] : ~0ull;
      }
    }
  }
#undef VB_SLOT
#undef VB_LIVE
  // s_w holds the sorted words.  Every thread looks at eight CONSECUTIVE sorted elements for run heads and lists its heads (sorted
  // positions, 2 bytes each, in the sort's counter table, which is free by now) behind those of the threads before it.  The means are
  // then dealt out one VOXEL to a thread: a voxel's mean is the sequential sum of its run in sorted = input order, its points read
  // from LDS through the ranks in the words, and the means leave in voxel order, 16 bytes a lane.  (Before, every thread summed the
  // runs that START among its own eight elements, one after the other, and went on through LDS for a run that left them: eight
  // unrolled bodies a thread, each as long as the longest run of its wave.  Round 3 continued through global memory, one dependent
  // gather per point: profiles/r04_vb_reduce.md.)
  VB_TS(10);
  if (tid == 0) s_w[c] = ~0ull;   // sentinel behind the last element
  __syncthreads();
  const uint32_t l0 = (uint32_t)tid * 8u;
  unsigned long long vox[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t l = l0 + (uint32_t)j;
    vox[j] = (l < c ? s_w[l] : ~0ull) >> ebits;   // (the sentinel's is larger than any index of the box)
  }
  bool head[8];
  uint32_t nh = 0u;
  unsigned long long prev = (l0 == 0u || l0 > c) ? ~0ull : (s_w[l0 - 1u] >> ebits);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t l = l0 + (uint32_t)j;
    head[j] = l < c && (l == 0u || vox[j] != prev);   // (a voxel never straddles two buckets: buckets are ranges of the voxel order)
    nh += head[j] ? 1u : 0u;
    prev = vox[j];
  }
  VB_TS(11);
  uint32_t tot;
  const uint32_t ex = block_excl_scan(nh, s_scan, tot);
  uint16_t* s_head = (uint16_t*)s_wcnt;   // tot <= c <= VB_CAP entries (read behind the barriers of the scan below)
  {
    uint32_t k = ex;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (head[j]) s_head[k++] = (uint16_t)(l0 + (uint32_t)j);
    }
  }
  if (tid == 0) {
    xchg_stores_done();   // the box atomics above (this wave's lanes 0-5) have been performed before the count is published; no cache-wide fence (dev_math.hpp)
    __hip_atomic_store(&A.heads[b], tot + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  uint32_t part = 0u;
  for (uint32_t t = (uint32_t)tid; t < b; t += VB_THREADS) {
    uint32_t v = __hip_atomic_load(&A.heads[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), spins = 0u;
    while (v == 0u) {
      __builtin_amdgcn_s_sleep(2);
      v = __hip_atomic_load(&A.heads[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (++spins > VB_SPIN_LIMIT) { A.h_fail[1] = 1u; v = 1u; }
    }
    part += v - 1u;
  }
  VB_TS(12);
  uint32_t base;
  (void)block_excl_scan(part, s_scan, base);   // voxels emitted by all earlier buckets
  if (tid == 0) {   // (write-through: vb_arrive)
    if (K.bucket0 == b) __hip_atomic_store(&A.out_off[seg], base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b + 1u == A.nb) __hip_atomic_store(&A.out_off[A.nseg], base + tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (b + 1u == A.nb) {   // the last bucket has seen every other bucket's count, hence every segment's final box: PCL's pass-through test
    int through = 0;
    for (uint32_t s = (uint32_t)tid; s < A.nseg; s += VB_THREADS) {
      int bb[6];
#pragma unroll
      for (int k = 0; k < 6; k++) bb[k] = __hip_atomic_load(&A.box[6 * s + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bb[3] >= bb[0]) {
        const long long dx = (long long)bb[3] - bb[0] + 1, dy = (long long)bb[4] - bb[1] + 1, dz = (long long)bb[5] - bb[2] + 1;
        if (dx * dy > 2147483647LL || dx * dy * dz > 2147483647LL) through = 1;   // (each extent < 2^21)
      }
    }
    if (__syncthreads_or(through) && tid == 0) vb_fail_reduce(A, 2);   // (block-uniform branch; thread 0 raises it, and arrives behind it)
  }
  const uint32_t arrived = tid == 0 ? vb_arrive(A) : 0u;
#ifdef LOAMX_PROF_VB
  uint32_t longest = 0u;
#endif
  for (uint32_t h = (uint32_t)tid; h < tot; h += (uint32_t)VB_THREADS) {
    const uint32_t l_beg = s_head[h], l_end = h + 1u < tot ? (uint32_t)s_head[h + 1u] : c;
    // (the reference's accumulators start at zero: 0 + x, kept for the sign of a zero coordinate)
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    // the first four elements (most runs are shorter), then sixteen at a time: a run of hundreds of points — dense ground next to
    // the sensor — is one thread's chain of dependent LDS round trips, which is the tail of the whole launch
    vb_sum_run<4>(s_w, s_pts, l_beg, l_end, c, emask, sx, sy, sz, si);
    for (uint32_t l = l_beg + 4u; l < l_end; l += 16u) vb_sum_run<16>(s_w, s_pts, l, l_end, c, emask, sx, sy, sz, si);
#ifdef LOAMX_PROF_VB
    longest = max(longest, l_end - l_beg);
#endif
    const float cf = (float)(l_end - l_beg);
    A.out[base + h] = make_float4(sx / cf, sy / cf, sz / cf, si / cf);
  }
#ifdef LOAMX_PROF_VB
  if (longest) atomicMax((unsigned long long*)&A.dbg[(size_t)blockIdx.x * 16 + 14], (unsigned long long)longest);
#endif
  if (tid == 0) vb_arrive_last(A, arrived);
  VB_TS(13);
}

// ----------------------------------------------------------------------------------------------------------------
void VoxBucket::run(const float4* in, const float4* const* d_src, uint32_t n, const uint32_t* d_seg_off, const uint32_t* h_seg_off, uint32_t nseg,
                    const Pose* d_poses, float inv_even, float inv_odd, float4* stack, float4* out, uint32_t* d_out_off,
                    const VbPoseInit* init) {
  LX_REQUIRE(fits(n, nseg), "internal: VoxBucket::run outside its limits");
  uint32_t nb = 0;
  for (uint32_t s = 0; s < nseg; s++) {
    const uint32_t m = h_seg_off[s + 1] - h_seg_off[s];
    nb += m ? (m + VB_T - 1) / VB_T : 1u;
  }
  nb_ = nb;
  segs_.reserve(nseg);
  lo_.reserve(nb);
  bk_.reserve(nb);
  box_.reserve((size_t)6 * nseg);
  cnt_.reserve(nb);
  heads_.reserve(nb);
  const uint32_t nchunk = (n + VB_CHUNK - 1) / VB_CHUNK;
  bword_.reserve((size_t)nchunk * VB_CHUNK);
  crange_.reserve(nchunk);
  if (!ctl_ready_) {
    ctl_.reserve(4);
    h_fail_.reserve(16);
    for (int k = 0; k < 16; k++) h_fail_.p[k] = 0u;
    LX_HIP(hipMemsetAsync(ctl_.p, 0, sizeof(uint32_t) * 4, st_));
    ctl_ready_ = true;
  }
  if (++epoch_ == 0u) epoch_ = 1u;
  VbArgs a;
  a.in = in; a.src = d_src; a.seg_off = d_seg_off; a.poses = d_poses;
  a.segs = segs_.p; a.lo = lo_.p; a.bk = bk_.p; a.box = box_.p; a.cnt = cnt_.p; a.heads = heads_.p;
  a.ctl = ctl_.p; a.h_fail = h_fail_.p; a.bword = bword_.p; a.crange = crange_.p; a.stack = stack; a.out = out; a.out_off = d_out_off;
  a.n = n; a.nseg = nseg; a.nb = nb; a.epoch = epoch_;
  a.inv_even = inv_even; a.inv_odd = inv_odd;
  a.init = init ? *init : VbPoseInit();
  a.dbg = nullptr;
#ifdef LOAMX_PROF_VB
  static DevBuf<unsigned long long> dbg;
  dbg.reserve((size_t)nb * 16 + 16);
  LX_HIP(hipMemsetAsync(dbg.p, 0, sizeof(unsigned long long) * ((size_t)nb * 16), st_));
  a.dbg = dbg.p;
#endif
  hipLaunchKernelGGL(k_vb_plan, dim3(nseg * VB_PLAN_PARTS), dim3(VB_SAMPLE), 0, st_, a);
  hipLaunchKernelGGL(k_vb_stack, dim3(nchunk), dim3(VB_CHUNK), 0, st_, a);
  hipLaunchKernelGGL(k_vb_reduce, dim3(nb), dim3(VB_THREADS), 0, st_, a);
  LX_HIP(hipGetLastError());
#ifdef LOAMX_PROF_VB
  {
    std::vector<unsigned long long> h((size_t)nb * 16);
    LX_HIP(hipStreamSynchronize(st_));
    LX_HIP(hipMemcpy(h.data(), dbg.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, t1 = 0;
    for (uint32_t b = 0; b < nb; b++) { if (h[16 * b]) t0 = std::min(t0, h[16 * b]); t1 = std::max(t1, h[16 * b + 13]); }
    fprintf(stderr, "[k_vb_reduce %u buckets, %.1f us first start -> last end] bucket: start | box | passes ... | sorted | heads | look-back | end (us since first start)\n", nb, (t1 - t0) * 0.01);
    uint32_t slow = 0;
    for (uint32_t b = 0; b < nb; b++) if (h[16 * b + 13] > h[16 * slow + 13]) slow = b;
    for (uint32_t b : {0u, nb / 4, nb / 2, nb - 1, slow}) {
      fprintf(stderr, "  b%-4u", b);
      for (int k = 0; k < 14; k++) if (h[16 * b + k]) fprintf(stderr, " %d:%.1f", k, (h[16 * b + k] - t0) * 0.01);
      if (h[16 * b + 15]) fprintf(stderr, " collected:%.1f", (h[16 * b + 15] - t0) * 0.01);
      fprintf(stderr, " longest run %llu", h[16 * b + 14]);
      fprintf(stderr, "\n");
    }
  }
#endif
}

// after failed(): which conditions the last run met (bit r = reason r of vb_fail)
uint32_t VoxBucket::why() const {
  uint32_t m = 0;
  for (int r = 0; r < 8; r++)
    if (((volatile uint32_t*)h_fail_.p)[2 + r] == epoch_) m |= 1u << r;
  return m;
}

void VoxBucket::check() {
  if (h_fail_.p && ((volatile uint32_t*)h_fail_.p)[1]) {
    h_fail_.p[1] = 0u;
    throw Error(LOAMX_E_HIP, "voxel grid: a look-back wait inside k_vb_reduce timed out");
  }
}

}  // namespace loamx
