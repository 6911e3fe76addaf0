// Sub-map index for gfx950 (MI355X): a counting-sorted uniform grid over one cloud (SubMapIndex) or over K clouds with one set of
// launches (SubMapIndexBatch).  Replaces the kd-tree rebuilds of the reference (BasicLaserMapping.cpp:636-637, BasicLaserOdometry.cpp);
// the registration's and the odometry's neighbour searches walk the cell tables built here.
#include "submap_index.hpp"
#include "scan.hpp"

namespace loamx {

// ----------------------------------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------------------------------

__global__ void k_init_bbox(uint32_t* scratch) {
  const uint32_t t = threadIdx.x;
  if (t < 3) scratch[t] = 0xffffffffu;
  else if (t < 16) scratch[t] = 0u;
}
__global__ void k_zero_u32_dn(uint32_t* p, const uint32_t* d_n) {
  const uint32_t n = *d_n;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

// ----------------------------------------------------------------------------------------------------------------
// SubMapIndex: bounding box -> grid descriptor -> cell histogram -> exclusive scan -> scatter
// scratch layout (uint32): [0..5] encoded min xyz / max xyz, [6] ncell+1, [7] scan total, [8] ncell
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bbox(const float4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ enc) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float4 p = pts[i];
    mn[0] = fminf(mn[0], p.x); mx[0] = fmaxf(mx[0], p.x);
    mn[1] = fminf(mn[1], p.y); mx[1] = fmaxf(mx[1], p.y);
    mn[2] = fminf(mn[2], p.z); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, 64));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, 64));
    }
  }
  __shared__ float red[4][6];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { red[wid][a] = mn[a]; red[wid][3 + a] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = red[0][a];
    for (int w = 1; w < 4; w++) v = a < 3 ? fminf(v, red[w][a]) : fmaxf(v, red[w][a]);
    if (a < 3) atomicMin(&enc[a], enc_f32(v)); else atomicMax(&enc[a], enc_f32(v));
  }
}

// grid descriptor from the bounds (k_bbox, or the producer of the points through SubMapIndex::d_bounds()): the cell edge starts at
// 1.05 m and grows by 1.25x while the table would not fit (grid_fit.hpp)
__device__ inline GridDesc grid_from_bounds(const uint32_t* __restrict__ scratch, uint32_t max_cells) {
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = dec_f32(scratch[a]); mx[a] = dec_f32(scratch[3 + a]); }
  return grid_fit(mn, mx, 1.05f, max_cells);
}

// count: every workgroup derives the descriptor itself (the same arithmetic everywhere; workgroup 0 records it and the scan's count);
// a point's rank inside its cell is the counter's value before its run's bump, so the scatter needs no atomics and the counters can
// be cleared behind the scan (rounds 1-4: k_init_bbox, k_grid_setup and k_zero_u32_dn were three launches of their own)
__global__ __launch_bounds__(256) void k_cell_count(const float4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ scratch, GridDesc* __restrict__ desc,
                                                    uint32_t max_cells, uint32_t* __restrict__ cell_of, uint32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ rank_of) {
  __shared__ GridDesc s_g;
  if (threadIdx.x == 0) {
    s_g = grid_from_bounds(scratch, max_cells);
    if (blockIdx.x == 0) {
      *desc = s_g;
      scratch[6] = s_g.ncell + 1;
      scratch[8] = s_g.ncell;
    }
  }
  __syncthreads();
  const GridDesc g = s_g;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t c = 0;
  if (active) {
    const float4 p = pts[i];
    int cx, cy, cz;
    cell_coords(g, p.x, p.y, p.z, cx, cy, cz);
    c = ((uint32_t)cz * g.ny + cy) * g.nx + cx;
    cell_of[i] = c;
  }
  int head, len;
  wave_runs(c, active, head, len);
  uint32_t base = 0;
  if (active && head == (int)__lane_id()) base = atomicAdd(&counts[c], (uint32_t)len);
  base = __shfl(base, head, 64);
  if (active) rank_of[i] = base + (uint32_t)((int)__lane_id() - head);
}

// scatter; its first thread leaves the bounds accumulators reset for the next build
__global__ __launch_bounds__(256) void k_cell_scatter(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ cell_of,
                                                      const uint32_t* __restrict__ rank_of, const uint32_t* __restrict__ cell_start,
                                                      float4* __restrict__ sorted, uint32_t* __restrict__ scratch) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
#pragma unroll
    for (int a = 0; a < 6; a++) scratch[a] = a < 3 ? 0xffffffffu : 0u;
  }
  if (i >= n) return;
  float4 p = pts[i];
  p.w = __uint_as_float(i);   // original index: kNN ties are broken on it, so the slot order inside a cell is irrelevant
  sorted[cell_start[cell_of[i]] + rank_of[i]] = p;
}

void SubMapIndex::init(hipStream_t st) {
  st_ = st;
  scratch_.reserve(16);
  hipLaunchKernelGGL(k_init_bbox, dim3(1), dim3(16), 0, st, scratch_.p);   // (once: every build's scatter leaves the bounds reset)
  d_desc_.reserve(1);
  tile_sums_.reserve(SCAN_SCRATCH_WORDS);
  LX_HIP(hipMemsetAsync(tile_sums_.p, 0, sizeof(uint32_t) * tile_sums_.cap, st));
}

void SubMapIndex::swap(SubMapIndex& o) {
  std::swap(n_, o.n_);
  auto sw = [](auto& a, auto& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); };
  sw(sorted_, o.sorted_); sw(cell_of_, o.cell_of_); sw(rank_of_, o.rank_of_); sw(cell_start_, o.cell_start_); sw(cursor_, o.cursor_);
  sw(tile_sums_, o.tile_sums_); sw(scratch_, o.scratch_); sw(d_desc_, o.d_desc_);
}

void SubMapIndex::build(const float4* d_pts, uint32_t n, bool bounds_done) {
  n_ = n;
  if (n == 0) return;
  sorted_.reserve(n);
  cell_of_.reserve(n);
  rank_of_.reserve(n);
  cell_start_.reserve((size_t)LX_MAX_CELLS + 2);
  if (!cursor_.p) {   // the cell counters: cleared once, kept clear by every build (the scan clears them behind itself)
    cursor_.reserve((size_t)LX_MAX_CELLS + 2);
    LX_HIP(hipMemsetAsync(cursor_.p, 0, sizeof(uint32_t) * cursor_.cap, st_));
  }
  const uint32_t nb = (n + 255) / 256;
  // bounds (unless the kernel that produced the points folded them into d_bounds() as it wrote them) -> count (+ grid set-up) -> scan
  // (+ counters cleared) -> scatter (+ bounds reset): 3 - 4 launches (rounds 1-4: 7)
  if (!bounds_done) hipLaunchKernelGGL(k_bbox, dim3(nb < 128 ? nb : 128), dim3(256), 0, st_, d_pts, n, scratch_.p);
  hipLaunchKernelGGL(k_cell_count, dim3(nb), dim3(256), 0, st_, d_pts, n, scratch_.p, d_desc_.p, LX_MAX_CELLS, cell_of_.p, cursor_.p, rank_of_.p);
  exclusive_scan_u32(cursor_.p, cell_start_.p, tile_sums_.p, scratch_.p + 8, scratch_.p + 7, LX_MAX_CELLS, st_, nullptr, cursor_.p);
  hipLaunchKernelGGL(k_cell_scatter, dim3(nb), dim3(256), 0, st_, d_pts, n, cell_of_.p, rank_of_.p, cell_start_.p, sorted_.p, scratch_.p);
  LX_HIP(hipGetLastError());
}

// ----------------------------------------------------------------------------------------------------------------
// SubMapIndexBatch: the same counting-sort build for K clouds with one set of launches
// scratch: [0] total cells + 1, [1] scan total, [2] total cells
// ----------------------------------------------------------------------------------------------------------------
__global__ void k_bb_init(uint32_t* enc, uint32_t K) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * K) enc[i * BB_STRIDE] = (i % 6) < 3 ? 0xffffffffu : 0u;
}
// grid = (blocks, K)
__global__ __launch_bounds__(256) void k_bb_bbox(const float4* __restrict__ pts, const uint32_t* __restrict__ off, uint32_t* __restrict__ enc) {
  const uint32_t c = blockIdx.y;
  const uint32_t a0 = off[c], a1 = off[c + 1];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (uint32_t i = a0 + blockIdx.x * blockDim.x + threadIdx.x; i < a1; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    mn[0] = fminf(mn[0], p.x); mx[0] = fmaxf(mx[0], p.x);
    mn[1] = fminf(mn[1], p.y); mx[1] = fmaxf(mx[1], p.y);
    mn[2] = fminf(mn[2], p.z); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, 64));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, 64));
    }
  }
  __shared__ float red[4][6];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { red[wid][a] = mn[a]; red[wid][3 + a] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6 && a1 > a0 + blockIdx.x * blockDim.x) {
    const int a = threadIdx.x;
    float v = red[0][a];
    for (int w = 1; w < 4; w++) v = a < 3 ? fminf(v, red[w][a]) : fmaxf(v, red[w][a]);
    if (a < 3) atomicMin(&enc[bb_word(c, a)], enc_f32(v)); else atomicMax(&enc[bb_word(c, a)], enc_f32(v));
  }
}
// grid descriptor of cloud c from its accumulated bounds, within the per-cloud cell budget (cell_base is the caller's scan)
__device__ inline GridDescB bb_make_desc(const uint32_t* __restrict__ enc, const uint32_t* __restrict__ off, uint32_t c, uint32_t budget, float cell0) {
  GridDescB d;
  d.g.ox = d.g.oy = d.g.oz = 0.f; d.g.inv_h = 1.f; d.g.nx = d.g.ny = d.g.nz = 1;
  d.pt_base = off[c];
  d.cell_base = 0;
  d.g.ncell = 1;   // an empty cloud: a 1-cell grid
  if (off[c + 1] != off[c]) {
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) { mn[a] = dec_f32(enc[bb_word(c, a)]); mx[a] = dec_f32(enc[bb_word(c, 3 + a)]); }
    d.g = grid_fit(mn, mx, cell0, budget);
  }
  return d;
}
// one thread per cloud (one workgroup, K <= 4096 in rounds of 1024): grid descriptors within the per-cloud cell budget, table bases by a scan
// (leaves the bounds accumulators reset for the next build: k_bb_init runs only when K grows)
__global__ __launch_bounds__(1024) void k_bb_setup(uint32_t* __restrict__ enc, const uint32_t* __restrict__ off, uint32_t K, GridDescB* __restrict__ desc,
                                                   uint32_t* __restrict__ scratch, uint32_t max_cells_total, float cell0) {
  __shared__ uint32_t lds[17];
  const uint32_t budget = max_cells_total / (K ? K : 1);
  uint32_t carry = 0;
  for (uint32_t c0 = 0; c0 < K; c0 += 1024) {
    const uint32_t c = c0 + threadIdx.x;
    GridDescB d;
    d.g.ox = d.g.oy = d.g.oz = 0.f; d.g.inv_h = 1.f; d.g.nx = d.g.ny = d.g.nz = 1; d.g.ncell = 0;
    d.pt_base = 0; d.cell_base = 0;
    if (c < K) {
      d = bb_make_desc(enc, off, c, budget, cell0);
#pragma unroll
      for (int a = 0; a < 6; a++) enc[bb_word(c, a)] = a < 3 ? 0xffffffffu : 0u;
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan(c < K ? d.g.ncell : 0u, lds, tot);
    if (c < K) {
      d.cell_base = carry + ex;
      desc[c] = d;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) {
    scratch[0] = carry + 1;
    scratch[2] = carry;
  }
}
// Round 6: for a handful of clouds (K <= BB_FUSE_MAXK: the odometry's 2 x streams of a chain) the set-up above is folded into the count —
// every workgroup derives the K descriptors from the bounds itself (a few dependent loads, in parallel over the workgroups), workgroup 0
// publishes them and the table size; the bounds accumulators are reset by the scatter, the build's last kernel.  One launch (and one
// dependent-launch gap) less in the tail of every odometry pass.
constexpr uint32_t BB_FUSE_MAXK = 64;
template <bool FUSED>
__global__ __launch_bounds__(256) void k_bb_count(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ off, uint32_t K,
                                                  GridDescB* __restrict__ desc, uint32_t* __restrict__ cell_of,
                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ rank_of, const uint32_t* __restrict__ enc,
                                                  uint32_t* __restrict__ scratch, uint32_t max_cells_total, float cell0) {
  __shared__ GridDescB s_desc[FUSED ? BB_FUSE_MAXK : 1];
  if (FUSED) {
    __shared__ uint32_t lds[17];
    const uint32_t cc = threadIdx.x;
    GridDescB d;
    d.g.ncell = 0;
    if (cc < K) d = bb_make_desc(enc, off, cc, max_cells_total / (K ? K : 1), cell0);
    uint32_t tot;
    const uint32_t ex = block_excl_scan(cc < K ? d.g.ncell : 0u, lds, tot);
    if (cc < K) {
      d.cell_base = ex;
      s_desc[cc] = d;
      if (blockIdx.x == 0) desc[cc] = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { scratch[0] = tot + 1; scratch[2] = tot; }
    __syncthreads();
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t c = 0;
  if (active) {
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const GridDescB d = FUSED ? s_desc[lo] : desc[lo];
    const float4 p = pts[i];
    int cx, cy, cz;
    cell_coords(d.g, p.x, p.y, p.z, cx, cy, cz);
    c = d.cell_base + ((uint32_t)cz * d.g.ny + cy) * d.g.nx + cx;
    cell_of[i] = c;
  }
  // the counter's value before a run's bump is where the run's points go inside their cell: the scatter needs no atomics of its own
  int head, len;
  wave_runs(c, active, head, len);
  uint32_t base = 0;
  if (active && head == (int)__lane_id()) base = atomicAdd(&counts[c], (uint32_t)len);
  base = __shfl(base, head, 64);
  if (active) rank_of[i] = base + (uint32_t)((int)__lane_id() - head);
}

__global__ __launch_bounds__(256) void k_bb_scatter(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ off, uint32_t K,
                                                    const uint32_t* __restrict__ cell_of, const uint32_t* __restrict__ rank_of,
                                                    const uint32_t* __restrict__ cell_start, float4* __restrict__ sorted, int pack_ring,
                                                    uint32_t* __restrict__ enc_reset) {
  if (enc_reset && blockIdx.x == 0 && threadIdx.x < K) {   // (the fused set-up: every workgroup of the count has read the bounds by now)
#pragma unroll
    for (int a = 0; a < 6; a++) enc_reset[bb_word(threadIdx.x, a)] = a < 3 ? 0xffffffffu : 0u;
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  float4 p = pts[i];
  const uint32_t li = i - off[lo];      // index inside its own cloud
  // pack_ring (the odometry's clouds: .w = ring id): the top byte carries the ring so that a search can filter by ring without a
  // second gather; 255 = unknown (ring id or index too large for the packing — its user then falls back, odometry.hip)
  uint32_t w = li;
  if (pack_ring) {
    const int ring = (int)p.w;
    w = (li <= 0xffffffu && ring >= 0 && ring < 255) ? (((uint32_t)ring << 24) | li) : (0xff000000u | (li & 0xffffffu));
  }
  p.w = __uint_as_float(w);
  sorted[cell_start[cell_of[i]] + rank_of[i]] = p;
}

void SubMapIndexBatch::init(hipStream_t st) {
  st_ = st;
  scratch_.reserve(16);
  tile_sums_.reserve(SCAN_SCRATCH_WORDS);
  LX_HIP(hipMemsetAsync(tile_sums_.p, 0, sizeof(uint32_t) * tile_sums_.cap, st));
}

// the bounding-box accumulators can be reset long before the points exist (e.g. ahead of the iterations whose result the
// points depend on): build() then finds them reset and skips that launch
void SubMapIndexBatch::prepare(uint32_t K) {
  LX_REQUIRE(K >= 1 && K <= 4096, "too many clouds in one index batch");
  reset_bounds_(K);
}
void SubMapIndexBatch::reset_bounds_(uint32_t K) {
  if (K <= enc_ready_) return;   // every build's k_bb_setup leaves the accumulators of its K clouds reset
  const uint32_t cap = std::max<uint32_t>(K, 64u);
  enc_.reserve(((size_t)6 * cap + 6) * BB_STRIDE);   // (growing discards the contents: all of it is initialised below)
  hipLaunchKernelGGL(k_bb_init, dim3((6 * cap + 255) / 256), dim3(256), 0, st_, enc_.p, cap);
  enc_ready_ = cap;
}

void SubMapIndexBatch::build(const float4* d_pts, const uint32_t* h_off, uint32_t K, const uint32_t* d_off_ready, bool bounds_done) {
  LX_REQUIRE(K >= 1 && K <= 4096, "too many clouds in one index batch");
  const uint32_t n = h_off[K];
  d_off_.reserve(K + 2);
  d_desc_.reserve(K + 1);
  const uint32_t* d_off = d_off_ready;   // the caller may already hold the offsets on the device
  if (!d_off) {
    h_off_pin_.reserve(K + 2);
    memcpy(h_off_pin_.p, h_off, sizeof(uint32_t) * (K + 1));
    LX_HIP(hipMemcpyAsync(d_off_.p, h_off_pin_.p, sizeof(uint32_t) * (K + 1), hipMemcpyHostToDevice, st_));
    d_off = d_off_.p;
  }
  sorted_.reserve((size_t)n + 1);
  cell_of_.reserve((size_t)n + 1);
  rank_of_.reserve((size_t)n + 1);
  cell_start_.reserve((size_t)LX_MAX_CELLS + 2);
  if (!cursor_.p) {   // the cell counters: cleared once, kept clear by every build
    cursor_.reserve((size_t)LX_MAX_CELLS + 2);
    LX_HIP(hipMemsetAsync(cursor_.p, 0, sizeof(uint32_t) * cursor_.cap, st_));
  }
  reset_bounds_(K);
  uint32_t max_len = 0;
  for (uint32_t c = 0; c < K; c++) max_len = std::max(max_len, h_off[c + 1] - h_off[c]);
  const uint32_t nbx = std::min<uint32_t>(std::max<uint32_t>((max_len + 255) / 256, 1u), 32u);
  if (!bounds_done) hipLaunchKernelGGL(k_bb_bbox, dim3(nbx, K), dim3(256), 0, st_, d_pts, d_off, enc_.p);
  const bool fused = n > 0 && K <= BB_FUSE_MAXK;   // (see k_bb_count: set-up folded into the count, bounds reset by the scatter)
  if (!fused) hipLaunchKernelGGL(k_bb_setup, dim3(1), dim3(1024), 0, st_, enc_.p, d_off, K, d_desc_.p, scratch_.p, LX_MAX_CELLS, cell_size);
  if (n) {
    if (fused) hipLaunchKernelGGL(k_bb_count<true>, dim3((n + 255) / 256), dim3(256), 0, st_, d_pts, n, d_off, K, d_desc_.p, cell_of_.p, cursor_.p, rank_of_.p,
                                  enc_.p, scratch_.p, LX_MAX_CELLS, cell_size);
    else hipLaunchKernelGGL(k_bb_count<false>, dim3((n + 255) / 256), dim3(256), 0, st_, d_pts, n, d_off, K, d_desc_.p, cell_of_.p, cursor_.p, rank_of_.p,
                            enc_.p, scratch_.p, LX_MAX_CELLS, cell_size);
  }
  // (the cell counters are cleared behind the scan: they are empty again when the next build starts)
  exclusive_scan_u32(cursor_.p, cell_start_.p, tile_sums_.p, scratch_.p + 2, scratch_.p + 1, LX_MAX_CELLS, st_, nullptr, cursor_.p);
  if (n) hipLaunchKernelGGL(k_bb_scatter, dim3((n + 255) / 256), dim3(256), 0, st_, d_pts, n, d_off, K, cell_of_.p, rank_of_.p, cell_start_.p, sorted_.p, pack_ring ? 1 : 0,
                            fused ? enc_.p : nullptr);
  LX_HIP(hipGetLastError());
}

}  // namespace loamx
