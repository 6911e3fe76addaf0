// C-ABI: parity hooks for five device primitives that otherwise only run inside whole pipelines — the segmented voxel grid
// (voxel.hpp), the chained scan (scan.hpp), the sub-map grid index (submap_index.hpp), the bucketed voxel grid (voxbucket.hpp) and the
// sweep re-projection (odometry.hpp).  Host glue only (plus one small kernel that
// stands in for the producers which fold the index's bounds): each hook stages the caller's arrays, runs the primitive the way its
// callers do, waits, checks the error word and copies the results back.  Each keeps ONE object per process (never freed, guarded by a
// mutex), so consecutive calls reuse its buffers and its state — which is part of what the tests look at.
#include <mutex>
#include "odometry.hpp"
#include "submap_index.hpp"
#include "voxbucket.hpp"
#include "voxel.hpp"

using namespace loamx;

namespace {

hipStream_t probe_stream() {   // (under the caller's lock)
  static hipStream_t st = nullptr;
  if (!st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    select_device(dev);
    st = create_stream(0);
  }
  return st;
}

struct VoxelProbe {
  VoxelPipeline vox;
  DevBuf<float4> pts, out;
  DevBuf<uint8_t> valid;
  DevBuf<uint32_t> seg, out_off;
  bool ready = false;
};

struct ScanProbe {
  DevBuf<unsigned long long> state;   // zero-filled once: the scan's epoch-tagged words live on from call to call
  DevBuf<uint32_t> in, out, out2, words;   // words: [0] the count, [1] the total
  bool ready = false;
};

struct IndexProbe {
  SubMapIndex single;
  SubMapIndexBatch batch;
  DevBuf<float4> pts, folded;
  DevBuf<uint32_t> off;
  std::vector<GridDescB> h_desc;
  bool ready = false;
};
static_assert(sizeof(GridDescB) == sizeof(loamx_index_desc) && sizeof(GridDesc) == 32, "loamx_index_desc mirrors GridDescB");

// The producer of an index's points as the probe plays it: copies the points and folds them into the bounds accumulators the way
// k_transform_to_end_batch does for SubMapIndexBatch (one thread per point, the cloud by the same binary search, every thread of the
// workgroup calling cloud_bounds_update) or, for the single index, with the six atomics k_map_split sends to SubMapIndex::d_bounds().
__global__ __launch_bounds__(256) void k_probe_fold(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t n, const uint32_t* __restrict__ off,
                                                    uint32_t K, uint32_t* __restrict__ bounds, int single) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t lo = 0;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    uint32_t hi = K;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (off[mid] <= i) lo = mid; else hi = mid;
    }
    q = src[i];
    dst[i] = q;
  }
  if (single) {
    if (active) {
      atomicMin(&bounds[0], enc_f32(q.x)); atomicMin(&bounds[1], enc_f32(q.y)); atomicMin(&bounds[2], enc_f32(q.z));
      atomicMax(&bounds[3], enc_f32(q.x)); atomicMax(&bounds[4], enc_f32(q.y)); atomicMax(&bounds[5], enc_f32(q.z));
    }
  } else {
    cloud_bounds_update(bounds, active, lo, q.x, q.y, q.z);
  }
}

struct VoxBucketProbe {
  VoxBucket vb;
  DevBuf<float4> pts, src, stack, out;   // src: the segments once more, last segment first (what the pointer table points into)
  DevBuf<uint32_t> seg_off, out_off;
  DevBuf<Pose> poses;
  DevBuf<const float4*> table;
  std::vector<const float4*> h_table;
  bool ready = false;
};
static_assert(sizeof(Pose) == 48 && sizeof(VbSeg) == sizeof(loamx_voxbucket_seg), "poses12 / loamx_voxbucket_seg mirror Pose / VbSeg");

struct ReprojectProbeState {
  DevBuf<float4> pts, src, src_s, rev;   // src: the caller's points; src_s: points [n_corner_all, n) once more; rev: the clouds last cloud first
  DevBuf<uint32_t> off, sid, rf, bounds;
  DevBuf<ToEndParams> params;
  DevBuf<const float4*> table;
  std::vector<const float4*> h_table;
  std::vector<uint32_t> h_sid, h_bounds;
};
static_assert(sizeof(ToEndParams) == sizeof(loamx_reproject_params) && sizeof(ToEndParams) == 29 * 4, "loamx_reproject_params mirrors ToEndParams");
static_assert(offsetof(ToEndParams, shift) == offsetof(loamx_reproject_params, shift) && offsetof(ToEndParams, s_end) == offsetof(loamx_reproject_params, s_end) &&
              offsetof(ToEndParams, enabled) == offsetof(loamx_reproject_params, enabled), "loamx_reproject_params mirrors ToEndParams");

template <class T> void upload(T* dst, const T* src, size_t n, hipStream_t st) {
  if (n) LX_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st));
}
template <class T> void download(T* dst, const T* src, size_t n, hipStream_t st) {
  if (n) LX_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st));
}

}  // namespace

extern "C" {

int loamx_voxel_probe(const float* pts_xyzi, uint32_t n, const uint32_t* seg_off, const uint32_t* seg_ids, const uint8_t* valid, uint32_t nseg,
                      float leaf_even, float leaf_odd, float* out_xyzi, uint32_t* out_off) {
  return guard([&]() {
    LX_REQUIRE(out_off && (out_xyzi || n == 0) && (pts_xyzi || n == 0), "NULL argument");
    LX_REQUIRE((seg_off != nullptr) != (seg_ids != nullptr), "exactly one of seg_off / seg_ids must be given");
    LX_REQUIRE(nseg >= 1 && nseg < (1u << 20), "nseg must be in [1, 2^20)");
    LX_REQUIRE(n + 1 < SCAN_MAX_N, "too many points for one voxel pass");
    LX_REQUIRE(leaf_even > 0.f && leaf_odd > 0.f && std::isfinite(leaf_even) && std::isfinite(leaf_odd), "leaf sizes must be positive");
    if (seg_off) {
      LX_REQUIRE(seg_off[0] == 0u && seg_off[nseg] == n, "seg_off must run from 0 to n");
      for (uint32_t s = 0; s < nseg; s++) LX_REQUIRE(seg_off[s] <= seg_off[s + 1], "seg_off must not decrease");
    } else {
      for (uint32_t i = 0; i < n; i++) LX_REQUIRE(seg_ids[i] < nseg, "segment id out of range");
    }
    LX_REQUIRE(packed_all_finite(reinterpret_cast<const float4*>(pts_xyzi), n), "non-finite coordinate");
    static std::mutex mu;
    static VoxelProbe* P = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t st = probe_stream();
    if (!P) P = new VoxelProbe;
    if (!P->ready) { P->vox.init(st); P->ready = true; }
    P->pts.reserve((size_t)n + 1); P->out.reserve((size_t)n + 1);
    P->valid.reserve((size_t)n + 1);
    P->seg.reserve(std::max<size_t>(n, (size_t)nseg + 1) + 1);
    P->out_off.reserve((size_t)nseg + 2);
    P->vox.reserve(n + 1, nseg);
    upload(P->pts.p, reinterpret_cast<const float4*>(pts_xyzi), n, st);
    if (valid) upload(P->valid.p, valid, n, st);
    upload(P->seg.p, seg_off ? seg_off : seg_ids, seg_off ? (size_t)nseg + 1 : (size_t)n, st);
    const uint8_t* d_valid = valid ? P->valid.p : nullptr;
    const uint32_t* d_off = seg_off ? P->seg.p : nullptr;
    const uint32_t* d_ids = seg_ids ? P->seg.p : nullptr;
    P->vox.compute_ijk(P->pts.p, d_valid, n, d_off, nseg, 1.0f / leaf_even, 1.0f / leaf_odd, d_ids);
    LX_HIP(hipGetLastError());
    P->vox.sort_reduce(P->pts.p, d_valid, n, d_off, nseg, P->out.p, P->out_off.p, d_ids);
    download(reinterpret_cast<float4*>(out_xyzi), P->out.p, n, st);
    download(out_off, P->out_off.p, (size_t)nseg + 1, st);
    LX_HIP(hipStreamSynchronize(st));
    P->vox.check();
    return LOAMX_OK;
  });
}

int loamx_scan_probe(uint32_t* in, uint32_t n, uint32_t max_n, uint32_t flags, uint32_t* out, uint32_t* total, uint32_t* out2) {
  return guard([&]() {
    const bool on_device = (flags & LOAMX_SCAN_COUNT_ON_DEVICE) != 0, in_place = (flags & LOAMX_SCAN_IN_PLACE) != 0,
               zero_in = (flags & LOAMX_SCAN_ZERO_IN) != 0;
    const size_t len = std::max(n, max_n);
    LX_REQUIRE((flags & ~7u) == 0u, "unknown flag");
    LX_REQUIRE(out && total && (in || len == 0), "NULL argument");
    LX_REQUIRE(!(in_place && zero_in), "zero_in needs an input buffer of its own");
    LX_REQUIRE(len <= (size_t)CHAINED_SCAN_MAX_TILES * SCAN_TILE, "too many elements for one scan");
    static std::mutex mu;
    static ScanProbe* P = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t st = probe_stream();
    if (!P) P = new ScanProbe;
    if (!P->ready) {
      P->state.reserve(chained_scan_state_words());
      LX_HIP(hipMemsetAsync(P->state.p, 0, sizeof(unsigned long long) * chained_scan_state_words(), st));
      P->words.reserve(2);
      P->ready = true;
    }
    P->in.reserve(len + 1); P->out.reserve(len + 1); P->out2.reserve(len + 1);
    // the result buffers start from the caller's contents, so that the caller sees which words the scan wrote
    upload(P->out.p, out, len + 1, st);
    if (out2) upload(P->out2.p, out2, len + 1, st);
    uint32_t* d_in = in_place ? P->out.p : P->in.p;
    upload(d_in, in, len, st);
    const uint32_t h_words[2] = {n, 0xdeadbeefu};
    upload(P->words.p, h_words, 2, st);
    exclusive_scan_u32_chained(d_in, P->out.p, P->state.p, P->words.p, P->words.p + 1, max_n, st, out2 ? P->out2.p : nullptr,
                               zero_in ? d_in : nullptr, on_device ? 0xffffffffu : n);
    LX_HIP(hipGetLastError());
    download(out, P->out.p, len + 1, st);
    if (out2) download(out2, P->out2.p, len + 1, st);
    if (zero_in) download(in, P->in.p, len, st);
    download(total, P->words.p + 1, 1, st);
    LX_HIP(hipStreamSynchronize(st));
    scan_check_errors();
    return LOAMX_OK;
  });
}

int loamx_index_probe(const float* pts_xyzw, uint32_t n, const uint32_t* off, uint32_t K, float cell_edge, uint32_t flags, loamx_index_desc* desc,
                      uint32_t* table, uint32_t table_cap, uint32_t* table_len, float* sorted_xyzw) {
  return guard([&]() {
    const bool single = (flags & LOAMX_INDEX_SINGLE) != 0, pack_ring = (flags & LOAMX_INDEX_PACK_RING) != 0, fold = (flags & LOAMX_INDEX_FOLD_BOUNDS) != 0;
    LX_REQUIRE((flags & ~7u) == 0u, "unknown flag");
    LX_REQUIRE(off && desc && table && table_len && (pts_xyzw || n == 0) && (sorted_xyzw || n == 0), "NULL argument");
    LX_REQUIRE(K >= 1 && K <= 4096, "K must be in [1, 4096]");
    LX_REQUIRE(n <= (1u << 24), "too many points for one probe");
    LX_REQUIRE(off[0] == 0u && off[K] == n, "offsets must run from 0 to n");
    for (uint32_t c = 0; c < K; c++) LX_REQUIRE(off[c] <= off[c + 1], "offsets must not decrease");
    LX_REQUIRE(std::isfinite(cell_edge) && cell_edge >= 0.25f && cell_edge <= 16.f, "cell edge must be in [0.25, 16]");
    LX_REQUIRE(!single || (K == 1 && n >= 1 && cell_edge == 1.05f && !pack_ring), "the single index: one non-empty cloud, cell edge 1.05, no ring packing");
    LX_REQUIRE(packed_all_finite(reinterpret_cast<const float4*>(pts_xyzw), n), "non-finite coordinate");
    static std::mutex mu;
    static IndexProbe* P = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t st = probe_stream();
    if (!P) P = new IndexProbe;
    if (!P->ready) { P->single.init(st); P->batch.init(st); P->ready = true; }
    P->pts.reserve((size_t)n + 1); P->folded.reserve((size_t)n + 1);
    P->off.reserve((size_t)K + 2);
    upload(P->pts.p, reinterpret_cast<const float4*>(pts_xyzw), n, st);
    const float4* d_pts = P->pts.p;
    const uint32_t nb = (n + 255) / 256;
    uint32_t total = 0;
    if (single) {
      if (fold) {
        upload(P->off.p, off, (size_t)K + 1, st);
        hipLaunchKernelGGL(k_probe_fold, dim3(nb), dim3(256), 0, st, P->pts.p, P->folded.p, n, P->off.p, K, P->single.d_bounds(), 1);
        LX_HIP(hipGetLastError());
        d_pts = P->folded.p;
      }
      P->single.build(d_pts, n, fold);
      GridDesc g;
      download(&g, P->single.desc(), 1, st);
      LX_HIP(hipStreamSynchronize(st));
      memcpy(&desc[0], &g, sizeof(g));
      desc[0].cell_base = 0; desc[0].pt_base = 0;
      total = g.ncell;
    } else {
      P->batch.cell_size = cell_edge;
      P->batch.pack_ring = pack_ring;
      if (fold) {
        P->batch.prepare(K);
        upload(P->off.p, off, (size_t)K + 1, st);
        if (n) hipLaunchKernelGGL(k_probe_fold, dim3(nb), dim3(256), 0, st, P->pts.p, P->folded.p, n, P->off.p, K, P->batch.d_bounds(), 0);
        LX_HIP(hipGetLastError());
        d_pts = P->folded.p;
      }
      P->batch.build(d_pts, off, K, fold ? P->off.p : nullptr, fold);
      P->h_desc.resize(K);
      download(P->h_desc.data(), P->batch.desc(0), K, st);
      LX_HIP(hipStreamSynchronize(st));
      memcpy(desc, P->h_desc.data(), sizeof(GridDescB) * K);
      total = P->h_desc[K - 1].cell_base + P->h_desc[K - 1].g.ncell;
    }
    *table_len = total + 1;
    if (total > LX_MAX_CELLS) throw Error(LOAMX_E_HIP, "the descriptors name more cells than the table holds");
    if (total + 1 > table_cap) throw Error(LOAMX_E_CAPACITY, "table_cap is smaller than the cell table");
    download(table, single ? P->single.cell_start() : P->batch.cell_table(), (size_t)total + 1, st);
    download(reinterpret_cast<float4*>(sorted_xyzw), single ? P->single.sorted() : P->batch.sorted(), n, st);
    LX_HIP(hipStreamSynchronize(st));
    return LOAMX_OK;
  });
}

int loamx_voxbucket_probe(const float* pts_xyzi, uint32_t n, const uint32_t* seg_off, uint32_t nseg, const float* poses12, float leaf_even,
                          float leaf_odd, uint32_t flags, float* stack_xyzi, float* out_xyzi, uint32_t* out_off,
                          loamx_voxbucket_status* status, loamx_voxbucket_seg* segs, uint64_t* lo, uint32_t* cnt, uint32_t bucket_cap) {
  return guard([&]() {
    const bool by_pointer = (flags & LOAMX_VOXBUCKET_SRC_POINTERS) != 0;
    LX_REQUIRE((flags & ~1u) == 0u, "unknown flag");
    LX_REQUIRE(pts_xyzi && seg_off && poses12 && stack_xyzi && out_xyzi && out_off && status && segs && lo && cnt, "NULL argument");
    LX_REQUIRE(VoxBucket::fits(n, nseg), "n must be in [1, 2^24) and nseg in [1, 4096]");
    LX_REQUIRE(leaf_even > 0.f && leaf_odd > 0.f && std::isfinite(leaf_even) && std::isfinite(leaf_odd), "leaf sizes must be positive");
    LX_REQUIRE(seg_off[0] == 0u && seg_off[nseg] == n, "seg_off must run from 0 to n");
    uint32_t nb = 0;
    for (uint32_t s = 0; s < nseg; s++) {
      LX_REQUIRE(seg_off[s] <= seg_off[s + 1], "seg_off must not decrease");
      const uint32_t m = seg_off[s + 1] - seg_off[s];
      nb += m ? (m + VB_T - 1) / VB_T : 1u;
    }
    status->gave_up = 0u; status->why = 0u; status->buckets = nb; status->pad = 0u;
    if (nb > bucket_cap) throw Error(LOAMX_E_CAPACITY, "bucket_cap is smaller than the run's bucket count");
    static std::mutex mu;
    static VoxBucketProbe* P = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t st = probe_stream();
    if (!P) P = new VoxBucketProbe;
    if (!P->ready) { P->vb.init(st); P->ready = true; }
    const uint32_t nsweep = (nseg + 1) / 2;
    P->pts.reserve((size_t)n + 1); P->stack.reserve((size_t)n + 1); P->out.reserve((size_t)n + 1);
    P->seg_off.reserve((size_t)nseg + 2); P->out_off.reserve((size_t)nseg + 2);
    P->poses.reserve(nsweep);
    upload(P->seg_off.p, seg_off, (size_t)nseg + 1, st);
    upload(P->poses.p, reinterpret_cast<const Pose*>(poses12), nsweep, st);
    const float4* const* d_src = nullptr;
    if (by_pointer) {
      // as the registration's device-resident inputs: every segment lives where its producer left it (here: the segments in reverse
      // order in a buffer of their own) and the concatenated array holds nothing of use (here: all-ones words, NaN)
      P->src.reserve((size_t)n + 1);
      P->table.reserve(nseg);
      P->h_table.resize(nseg);
      for (uint32_t s = 0; s < nseg; s++) {
        P->h_table[s] = P->src.p + (n - seg_off[s + 1]);
        upload(P->src.p + (n - seg_off[s + 1]), reinterpret_cast<const float4*>(pts_xyzi) + seg_off[s], (size_t)(seg_off[s + 1] - seg_off[s]), st);
      }
      upload(P->table.p, P->h_table.data(), nseg, st);
      LX_HIP(hipMemsetAsync(P->pts.p, 0xff, sizeof(float4) * (size_t)n, st));
      d_src = P->table.p;
    } else {
      upload(P->pts.p, reinterpret_cast<const float4*>(pts_xyzi), n, st);
    }
    P->vb.run(P->pts.p, d_src, n, P->seg_off.p, seg_off, nseg, P->poses.p, 1.0f / leaf_even, 1.0f / leaf_odd, P->stack.p, P->out.p, P->out_off.p);
    download(reinterpret_cast<float4*>(stack_xyzi), P->stack.p, n, st);
    download(reinterpret_cast<float4*>(out_xyzi), P->out.p, n, st);
    download(out_off, P->out_off.p, (size_t)nseg + 1, st);
    download(reinterpret_cast<VbSeg*>(segs), P->vb.d_segs(), nseg, st);
    download(reinterpret_cast<unsigned long long*>(lo), P->vb.d_lo(), nb, st);
    download(cnt, P->vb.d_cnt(), nb, st);
    LX_HIP(hipStreamSynchronize(st));
    P->vb.check();
    status->gave_up = P->vb.failed() ? 1u : 0u;
    status->why = P->vb.why();
    status->buckets = P->vb.last_buckets();
    return LOAMX_OK;
  });
}

int loamx_reproject_probe(const float* pts_xyzw, uint32_t n, const uint32_t* off, uint32_t K, const loamx_reproject_params* params, uint32_t ns,
                          uint32_t epoch, uint32_t n_corner_all, uint32_t flags, float* out_xyzw, uint32_t* ring_first, uint32_t* bounds) {
  return guard([&]() {
    const uint32_t variant = flags & 7u;
    const bool batch = variant <= LOAMX_REPROJECT_FUSED;
    const bool with_rf = batch && !(flags & LOAMX_REPROJECT_NO_RING_TABLE), with_bounds = batch && !(flags & LOAMX_REPROJECT_NO_BOUNDS);
    LX_REQUIRE((flags & ~31u) == 0u && variant <= LOAMX_REPROJECT_TO_START, "unknown flag or variant");
    LX_REQUIRE(off && params && (pts_xyzw || n == 0) && (out_xyzw || n == 0), "NULL argument");
    LX_REQUIRE((ring_first || !with_rf) && (bounds || !with_bounds), "NULL argument");
    LX_REQUIRE(K >= 1 && K <= 4096, "K must be in [1, 4096]");
    LX_REQUIRE(ns >= 1 && ns <= K, "ns must be in [1, K]");
    LX_REQUIRE(epoch >= 1 && epoch <= 255, "epoch must be in [1, 255]");
    LX_REQUIRE(n <= (1u << 24), "too many points for one probe");
    LX_REQUIRE(off[0] == 0u && off[K] == n, "offsets must run from 0 to n");
    for (uint32_t c = 0; c < K; c++) LX_REQUIRE(off[c] <= off[c + 1], "offsets must not decrease");
    LX_REQUIRE(n_corner_all <= n, "n_corner_all must not exceed n");
    const float4* h_pts = reinterpret_cast<const float4*>(pts_xyzw);
    LX_REQUIRE(packed_all_finite(h_pts, n), "non-finite coordinate");
    for (uint32_t i = 0; i < n; i++) LX_REQUIRE(h_pts[i].w >= 0.f && h_pts[i].w < 1024.f, "w must be in [0, 1024)");   // ((int)w is defined only for values that fit)
    static std::mutex mu;
    static ReprojectProbeState* P = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t st = probe_stream();
    if (!P) P = new ReprojectProbeState;
    const ToEndParams* h_params = reinterpret_cast<const ToEndParams*>(params);
    P->pts.reserve((size_t)n + 1); P->src.reserve((size_t)n + 1);
    P->off.reserve((size_t)K + 2); P->params.reserve(ns);
    upload(P->off.p, off, (size_t)K + 1, st);
    upload(P->params.p, h_params, ns, st);
    upload(P->src.p, h_pts, n, st);
    ReprojectProbe a = {};
    a.variant = (int)variant;
    a.pts = P->pts.p; a.n = n;
    a.d_off = P->off.p; a.h_off = off; a.K = K; a.ns = ns;
    a.d_params = P->params.p; a.h_params = h_params;
    a.src = P->src.p; a.n_corner_all = n_corner_all;
    a.rf_epoch = epoch;
    if (variant == LOAMX_REPROJECT_BATCH) {
      upload(P->pts.p, h_pts, n, st);
    } else if (n) {
      LX_HIP(hipMemsetAsync(P->pts.p, 0xff, sizeof(float4) * (size_t)n, st));   // (all-ones words, NaN: nothing of use where the kernels only write)
    }
    if (variant == LOAMX_REPROJECT_FUSED) {
      P->src_s.reserve((size_t)n + 1);
      upload(P->src_s.p, h_pts + n_corner_all, (size_t)(n - n_corner_all), st);
      a.src_s = P->src_s.p;
    }
    if (variant == LOAMX_REPROJECT_GATHER) {
      P->rev.reserve((size_t)n + 1); P->table.reserve(K); P->sid.reserve(K);
      P->h_table.resize(K); P->h_sid.resize(K);
      for (uint32_t c = 0; c < K; c++) {
        P->h_table[c] = P->rev.p + (n - off[c + 1]);
        P->h_sid[c] = c % ns;
        upload(P->rev.p + (n - off[c + 1]), h_pts + off[c], (size_t)(off[c + 1] - off[c]), st);
      }
      upload(P->table.p, P->h_table.data(), K, st);
      upload(P->sid.p, P->h_sid.data(), K, st);
      a.table = P->table.p; a.sid = P->sid.p;
    }
    if (with_rf) {
      P->rf.reserve((size_t)K * OD_RF_N);
      upload(P->rf.p, ring_first, (size_t)K * OD_RF_N, st);
      a.ring_first = P->rf.p;
    }
    if (with_bounds) {   // the caller's six words per cloud, each in its own cache line as SubMapIndexBatch keeps them
      const size_t words = (size_t)6 * K * BB_STRIDE;
      P->bounds.reserve(words);
      P->h_bounds.assign(words, 0u);
      for (uint32_t c = 0; c < K; c++)
        for (uint32_t k = 0; k < 6; k++) P->h_bounds[bb_word(c, k)] = bounds[6 * c + k];
      upload(P->bounds.p, P->h_bounds.data(), words, st);
      a.bounds = P->bounds.p;
    }
    reproject_probe_launch(a, st);
    download(reinterpret_cast<float4*>(out_xyzw), P->pts.p, n, st);
    if (with_rf) download(ring_first, P->rf.p, (size_t)K * OD_RF_N, st);
    if (with_bounds) download(P->h_bounds.data(), P->bounds.p, P->h_bounds.size(), st);
    LX_HIP(hipStreamSynchronize(st));
    if (with_bounds)
      for (uint32_t c = 0; c < K; c++)
        for (uint32_t k = 0; k < 6; k++) bounds[6 * c + k] = P->h_bounds[bb_word(c, k)];
    return LOAMX_OK;
  });
}

}  // extern "C"
