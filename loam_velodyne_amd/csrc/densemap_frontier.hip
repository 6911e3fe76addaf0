// Frontiers of the navigation grid (densemap.hpp DmFrontier, include/loamx.h loamx_densemap_frontiers and what goes with it): the FREE
// cells of a window that touch UNKNOWN ones, grouped under 4- or 8-connectivity, each group named by the smallest record index in it,
// with its size, box, sums and the cheapest cell of the route's field.  Integer atomics only; every output word but stats[5] is a
// function of the grid's integers and of the field, not of the schedule.
//
// What was built, launch by launch (one look at the totals between flatten and ids: the accumulators are sized by them):
//   k_dm_fr_mark      one block per tile of 32 x 32 cells.  The class of every cell of the tile and of a halo of one (0 other, 1 UNKNOWN,
//                     2 FREE with clear2 >= min_clear2; outside the window: 0) goes to LDS as a byte, each thread counts the unknown
//                     neighbours of its four cells there, and the tile's frontier cells are labelled INSIDE the tile at once, by a
//                     union-find over a 1024-word LDS array (densemap_label.hpp, workgroup scope, on local indices).  It writes
//                     parent[c] = the record index of the cell's root inside the tile (NONE: no frontier cell) and unknown8 as a
//                     byte, and counts the frontier cells with one atomic per block.  Only the owning tile writes a word, so these
//                     are plain stores.  Marking and the in-tile labelling share a launch because they share the staged tile; the
//                     suggested order had the labelling in the link kernel, which would have read parent[] again to rebuild the flags.
//   k_dm_fr_link      the joins across tile borders, in a launch of its own so that no hook can meet a plain store of the launch
//                     before: 128 threads per tile, 96 at work, one per border cell: the last row joins its three neighbours below, the
//                     last column its neighbours to the right, the first column the one below to the left (the forward half of
//                     the neighbourhood: 2 offsets under connectivity 4, 4 under 8; the pairs inside a tile were joined in LDS).  The
//                     union-find of densemap_label.hpp over parent[] in HBM (agent scope; the argument for it is there), a cell's
//                     rank being its index, so that the root of a finished frontier is its min_cell whatever the schedule.  The bound
//                     of every loop is the number of cells (of a tile in k_dm_fr_mark); one that is reached raises ctr[2], and the
//                     host reports LOAMX_E_INTERNAL.
//   k_dm_fr_flatten   parent[c] = root, the roots of each 256-cell block counted (dm_block_count); the chained scan of scan.hpp over
//                     the counts gives every root a compact id.  Roots are cell indices, so the ids ascend with min_cell: the final
//                     order.
//   k_dm_fr_ids       a root writes its id and the empty accumulator of its frontier.
//   k_dm_fr_reduce    per frontier cell: cells, the sums of rx, rz and unknown8 and the reachable count by integer adds, the box by
//                     min / max, best by one 64-bit atomicMin of (cost << 32) | cell: "smallest cost, then smallest index".  Combined
//                     inside the block in a 256-entry LDS table keyed by the id (dm_lds_claim), then one global atomic per
//                     (block, frontier, word).
//   k_dm_fr_labels    only when labels are wanted: the host has applied min_cells and ranked the kept frontiers; the ranks go up, one
//                     word per cell comes down.
//
// Resources, from scripts/kernel_resources.py on the gfx950 code object (VGPRs, static LDS bytes, scratch bytes; no spills, 8 waves
// per SIMD each):  k_dm_fr_mark 34, 5264, 0;  k_dm_fr_link 20, 0, 0;  k_dm_fr_flatten 10, 16, 0;  k_dm_fr_ids 14, 16, 0;
// k_dm_fr_reduce 12, 15360, 0;  k_dm_fr_labels 4, 0, 0;  k_dm_fr_totals 2, 0, 0.
//
// Measured on one MI355X (BASELINE.md section 6 has the table and the spread), a synthetic 2048 x 2048 grid with 87,374 frontier
// cells in 169 frontiers, `python scripts/bench_densemap_frontier.py`, and device times from a run of its own,
// `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_densemap_frontier.py --no-copies --reps 10`, then
// `--summarise DIR`: mark 63 us, link 18, flatten 19, scan 6, totals 5, ids 8, reduce 250, labels 9: 0.38 ms on the device, and
// 0.42 ms more wall time than route_cells alone on the same grid, against 2.37 ms to bring both record arrays to pinned memory; at
// 512 x 512, 0.09 ms on the device against 0.17 ms.  The reduce kernel is two thirds of it: about ten global atomics per (block,
// frontier), and the long frontiers take them from thousands of blocks on the same 64 bytes.  Tried against that and rejected: a
// plain read of the accumulator in front of each minimum and maximum, to send only those that change something, with cells and
// reachable in one 64-bit add.  Same bytes, but reduce took 489 us instead of 250 (86 instead of 40 at 512 x 512): an atomic whose
// result nobody reads is sent and forgotten, a read of the same contended line is waited for.
#include "densemap_label.hpp"
#include "densemap_map.hpp"
#include "pinned_copy.hpp"

namespace loamx {

constexpr int DM_FR_TILE = 32;
constexpr int DM_FR_SIDE = DM_FR_TILE + 2;   // with the halo
constexpr uint32_t DM_FR_NONE = LOAMX_FRONTIER_NONE;
static_assert(DM_FR_NONE == DM_UF_NONE, "the union-find's NONE is the label of a cell in no frontier");
constexpr int DM_FR_LDS_SCOPE = __HIP_MEMORY_SCOPE_WORKGROUP, DM_FR_AGENT = __HIP_MEMORY_SCOPE_AGENT;   // a tile's array; parent[] in HBM
constexpr uint32_t DM_FR_MAX_CELLS = 1u << 26;
constexpr uint32_t DM_FR_MAX_ROUTED = 1u << 22;
constexpr unsigned long long DM_FR_NO_BEST = ~0ull;   // (LOAMX_ROUTE_UNREACHABLE << 32) | LOAMX_FRONTIER_NONE

// grid: tiles_x x tiles_z.  ctr: [0] frontier cells, [1] hooks lost, [2] a loop bound was reached
__global__ __launch_bounds__(256) void k_dm_fr_mark(const loamx_grid_cell* __restrict__ cells, uint32_t nx, uint32_t nz, int diag,
                                                    uint32_t min_unknown, uint32_t min_clear2, uint32_t* __restrict__ parent,
                                                    unsigned char* __restrict__ u8, uint32_t* __restrict__ ctr) {
  __shared__ unsigned char s_k[DM_FR_SIDE * DM_FR_SIDE];
  __shared__ uint32_t s_par[DM_FR_TILE * DM_FR_TILE];
  __shared__ uint32_t s_n, s_lost, s_bad;
  if (threadIdx.x == 0) s_n = s_lost = s_bad = 0u;
  const int bx = (int)blockIdx.x * DM_FR_TILE, bz = (int)blockIdx.y * DM_FR_TILE;
  for (int e = (int)threadIdx.x; e < DM_FR_SIDE * DM_FR_SIDE; e += 256) {
    const int x = bx - 1 + e % DM_FR_SIDE, z = bz - 1 + e / DM_FR_SIDE;
    unsigned char k = 0;   // a cell outside the window is neither unknown nor free
    if (x >= 0 && x < (int)nx && z >= 0 && z < (int)nz) {
      const loamx_grid_cell* r = cells + ((size_t)z * nx + (uint32_t)x);
      const uint32_t cls = r->cls;
      k = cls == LOAMX_GRID_UNKNOWN ? 1 : (cls == LOAMX_GRID_FREE && r->clear2 >= min_clear2 ? 2 : 0);
    }
    s_k[e] = k;
  }
  __syncthreads();
  // this thread's four cells: column lx, rows lz0 + 8 j
  const int lx = (int)threadIdx.x % DM_FR_TILE, lz0 = (int)threadIdx.x / DM_FR_TILE;
  uint32_t un[4];
  uint32_t mine = 0u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int lz = lz0 + 8 * j, e = (lz + 1) * DM_FR_SIDE + lx + 1;
    uint32_t u = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        if (dx || dz) u += s_k[e + dz * DM_FR_SIDE + dx] == 1 ? 1u : 0u;
    const bool fr = s_k[e] == 2 && u >= min_unknown;   // (s_k is 0 outside the window)
    un[j] = fr ? u : 0u;
    s_par[lz * DM_FR_TILE + lx] = fr ? (uint32_t)(lz * DM_FR_TILE + lx) : DM_FR_NONE;
    mine += fr ? 1u : 0u;
  }
  __syncthreads();
  // the joins inside the tile: the forward half of the neighbourhood, (dx, dz) = (1, 0), (-1, 1), (0, 1), (1, 1)
  uint32_t lost = 0u, bad = 0u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int lz = lz0 + 8 * j;
    const uint32_t l = (uint32_t)(lz * DM_FR_TILE + lx);
    if (s_par[l] == DM_FR_NONE) continue;   // (NONE never changes)
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int dx = o == 0 ? 1 : o - 2, dz = o == 0 ? 0 : 1;
      if (dx && dz && !diag) continue;
      const int ax = lx + dx, az = lz + dz;
      if (ax < 0 || ax >= DM_FR_TILE || az >= DM_FR_TILE) continue;   // (across the border: k_dm_fr_link)
      const uint32_t nb = (uint32_t)(az * DM_FR_TILE + ax);
      if (dm_uf_load<DM_FR_LDS_SCOPE>(&s_par[nb]) == DM_FR_NONE) continue;
      if (!dm_uf_union<DM_FR_LDS_SCOPE>(s_par, l, nb, DM_FR_TILE * DM_FR_TILE, [](uint32_t e) { return e; }, lost)) bad = 1u;
    }
  }
  if (mine) atomicAdd(&s_n, mine);
  if (lost) atomicAdd(&s_lost, lost);
  if (bad) atomicOr(&s_bad, 1u);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int lz = lz0 + 8 * j;
    const uint32_t x = (uint32_t)(bx + lx), z = (uint32_t)(bz + lz);
    if (x >= nx || z >= nz) continue;
    const uint32_t l = (uint32_t)(lz * DM_FR_TILE + lx);
    uint32_t root = DM_FR_NONE;
    if (s_par[l] != DM_FR_NONE) {
      const uint32_t r = dm_uf_find<DM_FR_LDS_SCOPE>(s_par, l, DM_FR_TILE * DM_FR_TILE);
      if (r == DM_FR_NONE) atomicOr(&s_bad, 1u);
      // (a cell whose find gave up stays a root of its own: still a frontier cell, and the host reports the bound)
      const uint32_t rl = r == DM_FR_NONE ? l : r;
      root = ((uint32_t)bz + rl / DM_FR_TILE) * nx + (uint32_t)bx + rl % DM_FR_TILE;
    }
    const size_t c = (size_t)z * nx + x;
    parent[c] = root;
    u8[c] = (unsigned char)un[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n) atomicAdd(&ctr[0], s_n);
    if (s_lost) atomicAdd(&ctr[1], s_lost);
    if (s_bad) atomicOr(&ctr[2], 1u);
  }
}

// grid: tiles_x x tiles_z, 128 threads: 0..31 the tile's last row, 32..63 its last column, 64..95 its first column
__global__ __launch_bounds__(128) void k_dm_fr_link(uint32_t nx, uint32_t nz, int diag, uint32_t* parent, uint32_t* __restrict__ ctr) {
  const uint32_t t = threadIdx.x, part = t / DM_FR_TILE, i = t % DM_FR_TILE;
  if (part > 2u) return;
  const uint32_t lx = part == 0u ? i : (part == 1u ? (uint32_t)DM_FR_TILE - 1u : 0u), lz = part == 0u ? (uint32_t)DM_FR_TILE - 1u : i;
  if (part != 0u && lz == (uint32_t)DM_FR_TILE - 1u) return;   // (the corner cells belong to the last row)
  const uint32_t x = blockIdx.x * DM_FR_TILE + lx, z = blockIdx.y * DM_FR_TILE + lz;
  if (x >= nx || z >= nz) return;
  const uint32_t cells = nx * nz, c = z * nx + x;
  if (dm_uf_load<DM_FR_AGENT>(&parent[c]) == DM_FR_NONE) return;
  uint32_t lost = 0u, bad = 0u;
  for (int o = 0; o < 4; o++) {   // (dx, dz) = (1, 0), (-1, 1), (0, 1), (1, 1)
    const int dx = o == 0 ? 1 : o - 2, dz = o == 0 ? 0 : 1;
    if (dx && dz && !diag) continue;
    const int ax = (int)lx + dx, az = (int)lz + dz;
    if (ax >= 0 && ax < DM_FR_TILE && az < DM_FR_TILE) continue;   // (inside the tile: joined by k_dm_fr_mark)
    const uint32_t qx = x + (uint32_t)dx, qz = z + (uint32_t)dz;    // (a cell before the window wraps)
    if (qx >= nx || qz >= nz) continue;
    const uint32_t nb = qz * nx + qx;
    if (dm_uf_load<DM_FR_AGENT>(&parent[nb]) == DM_FR_NONE) continue;
    if (!dm_uf_union<DM_FR_AGENT>(parent, c, nb, cells, [](uint32_t e) { return e; }, lost)) bad = 1u;
  }
  if (lost) atomicAdd(&ctr[1], lost);
  if (bad) atomicOr(&ctr[2], 1u);
}

__global__ __launch_bounds__(256) void k_dm_fr_flatten(uint32_t cells, uint32_t* parent, uint32_t* __restrict__ blk_roots,
                                                       uint32_t* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false;
  if (i < cells) {
    const uint32_t x = dm_uf_load<DM_FR_AGENT>(&parent[i]);
    if (x != DM_FR_NONE) {
      root = x == i;
      const uint32_t r = dm_uf_root<DM_FR_AGENT>(parent, x, cells);
      if (r == DM_FR_NONE) atomicOr(&ctr[2], 1u);
      else if (!root) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, DM_FR_AGENT);
    }
  }
  const uint32_t n_roots = dm_block_count(root);
  if (threadIdx.x == 0) blk_roots[blockIdx.x] = n_roots;
}

// the total of the scan beside the three counters: the four words that go back before the second half is sized
__global__ void k_dm_fr_totals(const uint32_t* __restrict__ total_roots, uint32_t* __restrict__ ctr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctr[3] = *total_roots;
}

// behind the scan of the root counts: a root's compact id and the empty accumulator of its frontier
__global__ __launch_bounds__(256) void k_dm_fr_ids(uint32_t cells, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ off_roots,
                                                   uint32_t n_roots, uint32_t* __restrict__ rootid, DmFrAcc* __restrict__ acc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = i < cells && parent[i] == i;
  const unsigned long long m = dm_block_vote(root);
  if (!root) return;
  const uint32_t id = dm_block_rank(m, off_roots[blockIdx.x]);
  if (id >= n_roots) return;   // (cannot happen: the scan counted these roots)
  rootid[i] = id;
  DmFrAcc a;
  a.min_cell = i;
  a.cells = 0u;
  a.lo[0] = a.lo[1] = 0xffffffffu;
  a.hi[0] = a.hi[1] = 0u;
  a.sum_rx = a.sum_rz = a.links = 0ull;
  a.best = DM_FR_NO_BEST;
  a.reachable = a.reserved = 0u;
  acc[id] = a;
}

// one thread per cell in record order.  field NULL: no cost (reachable 0, best untouched)
__global__ __launch_bounds__(256) void k_dm_fr_reduce(uint32_t nx, uint32_t cells, const uint32_t* __restrict__ parent,
                                                      const uint32_t* __restrict__ rootid, uint32_t n_roots,
                                                      const unsigned char* __restrict__ u8, const loamx_route_cell* __restrict__ field,
                                                      DmFrAcc* __restrict__ acc) {
  __shared__ uint32_t s_id[DM_LDS_IDS];
  __shared__ uint32_t s_w[DM_LDS_IDS][6];               // cells, reachable, lo, hi
  __shared__ unsigned long long s_sum[DM_LDS_IDS][4];   // sum_rx, sum_rz, links, best
  const uint32_t t = threadIdx.x, i = blockIdx.x * blockDim.x + t;
  s_id[t] = DM_FR_NONE;
  s_w[t][0] = s_w[t][1] = 0u;
  s_w[t][2] = s_w[t][3] = 0xffffffffu;
  s_w[t][4] = s_w[t][5] = 0u;
  s_sum[t][0] = s_sum[t][1] = s_sum[t][2] = 0ull;
  s_sum[t][3] = DM_FR_NO_BEST;
  __syncthreads();
  uint32_t id = DM_FR_NONE;
  if (i < cells) {
    const uint32_t r = parent[i];
    if (r != DM_FR_NONE) id = rootid[r];
  }
  if (id != DM_FR_NONE && id >= n_roots) id = DM_FR_NONE;   // (cannot happen: every root got an id below n_roots)
  if (id != DM_FR_NONE) {
    const uint32_t rx = i % nx, rz = i / nx;
    const uint32_t cost = field ? field[i].cost : LOAMX_ROUTE_UNREACHABLE;
    const uint32_t h = dm_lds_claim(s_id, id);
    atomicAdd(&s_w[h][0], 1u);
    atomicMin(&s_w[h][2], rx);
    atomicMin(&s_w[h][3], rz);
    atomicMax(&s_w[h][4], rx);
    atomicMax(&s_w[h][5], rz);
    atomicAdd(&s_sum[h][0], (unsigned long long)rx);
    atomicAdd(&s_sum[h][1], (unsigned long long)rz);
    atomicAdd(&s_sum[h][2], (unsigned long long)u8[i]);
    if (cost != LOAMX_ROUTE_UNREACHABLE) {
      atomicAdd(&s_w[h][1], 1u);
      atomicMin(&s_sum[h][3], ((unsigned long long)cost << 32) | i);
    }
  }
  __syncthreads();
  const uint32_t fid = s_id[t];
  if (fid == DM_FR_NONE) return;
  // (no read in front of the minima and maxima to skip those that change nothing: measured, twice as slow, the file's head comment)
  DmFrAcc* a = acc + fid;
  atomicAdd(&a->cells, s_w[t][0]);
  atomicMin(&a->lo[0], s_w[t][2]);
  atomicMin(&a->lo[1], s_w[t][3]);
  atomicMax(&a->hi[0], s_w[t][4]);
  atomicMax(&a->hi[1], s_w[t][5]);
  atomicAdd(&a->sum_rx, s_sum[t][0]);
  atomicAdd(&a->sum_rz, s_sum[t][1]);
  atomicAdd(&a->links, s_sum[t][2]);
  if (s_w[t][1]) {
    atomicAdd(&a->reachable, s_w[t][1]);
    atomicMin(&a->best, s_sum[t][3]);
  }
}

// the label of every cell: the rank of its frontier (NONE: no frontier cell, or its frontier was dropped)
__global__ __launch_bounds__(256) void k_dm_fr_labels(uint32_t cells, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rootid,
                                                      const uint32_t* __restrict__ rank, uint32_t n_roots, uint32_t* __restrict__ lab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cells) return;
  const uint32_t r = parent[i];
  uint32_t v = DM_FR_NONE;
  if (r != DM_FR_NONE) {
    const uint32_t id = rootid[r];
    if (id < n_roots) v = rank[id];
  }
  lab[i] = v;
}

void dm_frontier_check(const loamx_grid_frontier_config& c) {
  LX_REQUIRE(c.connectivity == 4u || c.connectivity == 8u, "connectivity must be 4 or 8");
  LX_REQUIRE(c.min_unknown >= 1u && c.min_unknown <= 8u, "min_unknown must be in [1, 8]");
  LX_REQUIRE(c.min_clear2 >= 1u, "min_clear2 must be >= 1");
  LX_REQUIRE(c.min_cells >= 1u, "min_cells must be >= 1");
}

const uint32_t* DmFrontier::run(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_frontier_config& c,
                                const loamx_route_cell* d_field, bool want_labels, std::vector<loamx_frontier>& out, uint64_t stats[6],
                                DmScan& scan, hipStream_t st) {
  const uint32_t n = nx * nz, nblk = (n + 255u) / 256u;
  const uint32_t tiles_x = (nx + DM_FR_TILE - 1) / DM_FR_TILE, tiles_z = (nz + DM_FR_TILE - 1) / DM_FR_TILE;
  parent_.reserve(n);
  rootid_.reserve(n);
  u8_.reserve(n);
  blk_.reserve((size_t)nblk + 1);
  ctr_.reserve(4);
  h_ctr_.reserve(4);
  const int diag = c.connectivity == 8u ? 1 : 0;
  const dim3 per_tile(tiles_x, tiles_z), per_cell(nblk), block(256);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(uint32_t) * 4, st));
  hipLaunchKernelGGL(k_dm_fr_mark, per_tile, block, 0, st, d_cells, nx, nz, diag, c.min_unknown, c.min_clear2, parent_.p, u8_.p, ctr_.p);
  hipLaunchKernelGGL(k_dm_fr_link, per_tile, dim3(128), 0, st, nx, nz, diag, parent_.p, ctr_.p);
  hipLaunchKernelGGL(k_dm_fr_flatten, per_cell, block, 0, st, n, parent_.p, blk_.p, ctr_.p);
  scan.run(blk_.p, nblk, st);   // ([nblk]: the total)
  hipLaunchKernelGGL(k_dm_fr_totals, dim3(1), dim3(64), 0, st, blk_.p + nblk, ctr_.p);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_ctr_.p, ctr_.p, 4, st);
  LX_HIP(hipStreamSynchronize(st));
  scan_check_errors();
  const uint32_t marked = h_ctr_.p[0], lost = h_ctr_.p[1], n_roots = h_ctr_.p[3];
  if (h_ctr_.p[2]) throw Error(LOAMX_E_INTERNAL, "frontiers: a union-find loop reached its bound");
  if (n_roots > marked) throw Error(LOAMX_E_INTERNAL, "frontiers: more frontiers than frontier cells");

  if (n_roots) {
    acc_.reserve(n_roots);
    hipLaunchKernelGGL(k_dm_fr_ids, per_cell, block, 0, st, n, parent_.p, blk_.p, n_roots, rootid_.p, acc_.p);
    hipLaunchKernelGGL(k_dm_fr_reduce, per_cell, block, 0, st, nx, n, parent_.p, rootid_.p, n_roots, u8_.p, d_field, acc_.p);
    LX_HIP(hipGetLastError());
    h_acc_.fetch(acc_.p, n_roots, st);
    LX_HIP(hipStreamSynchronize(st));
  }

  // the host's half: min_cells and the ranks (the ids are in ascending min_cell already)
  const DmFrAcc* all = h_acc_.data();
  h_rank_.reserve(std::max<size_t>(n_roots, 1));
  out.clear();
  uint64_t total = 0, kept_cells = 0, kept_reachable = 0;
  for (uint32_t id = 0; id < n_roots; id++) {
    const DmFrAcc& a = all[id];
    total += a.cells;
    if (id && a.min_cell <= all[id - 1].min_cell) throw Error(LOAMX_E_INTERNAL, "frontiers: the compact ids do not ascend with min_cell");
    h_rank_.p[id] = DM_FR_NONE;
    if (a.cells < c.min_cells) continue;
    h_rank_.p[id] = (uint32_t)out.size();
    kept_cells += a.cells;
    kept_reachable += a.reachable ? 1u : 0u;
    loamx_frontier f;
    f.min_cell = a.min_cell;
    f.cells = a.cells;
    for (int k = 0; k < 2; k++) { f.lo[k] = a.lo[k]; f.hi[k] = a.hi[k]; }
    f.sum_rx = a.sum_rx;
    f.sum_rz = a.sum_rz;
    f.unknown_links = a.links;
    f.reachable = a.reachable;
    f.best_cost = (uint32_t)(a.best >> 32);
    f.best_cell = (uint32_t)a.best;
    f.reserved = 0u;
    out.push_back(f);
  }
  if (total != marked) throw Error(LOAMX_E_INTERNAL, "frontiers: the frontiers do not add up to the frontier cells");
  const uint32_t* labels = nullptr;
  if (want_labels) {
    lab_.reserve(n);
    h_lab_.reserve(n);
    if (n_roots) {
      rank_.reserve(n_roots);
      LX_HIP(hipMemcpyAsync(rank_.p, h_rank_.p, sizeof(uint32_t) * n_roots, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_dm_fr_labels, per_cell, block, 0, st, n, parent_.p, rootid_.p, rank_.p, n_roots, lab_.p);
      LX_HIP(hipGetLastError());
    } else {
      LX_HIP(hipMemsetAsync(lab_.p, 0xff, sizeof(uint32_t) * n, st));
    }
    store_to_pinned_u32(h_lab_.p, lab_.p, n, st);
    LX_HIP(hipStreamSynchronize(st));
    labels = h_lab_.p;
  }
  stats[0] = marked; stats[1] = n_roots; stats[2] = out.size(); stats[3] = kept_cells; stats[4] = kept_reachable; stats[5] = lost;
  return labels;
}

// what the two entry points share behind the grid's records: the route towards the start (when given), the frontiers, the outputs
int DenseMap::frontiers_on(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc,
                           const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out,
                           uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]) {
  const loamx_route_cell* d_field = nullptr;
  if (start_xz) {
    uint64_t rs[6];
    route_.run(d_cells, nx, nz, rc, start_xz, 1u, false, rs, own_);
    d_field = route_.field_on_device();
  }
  std::vector<loamx_frontier> fr;
  uint64_t s[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t* lab = fr_.run(d_cells, nx, nz, fc, d_field, labels != nullptr, fr, s, scan_, own_);
  *n_frontiers = fr.size();
  if (out && capacity < fr.size()) return LOAMX_E_CAPACITY;
  if (labels) memcpy(labels, lab, sizeof(uint32_t) * (size_t)nx * nz);
  if (out && !fr.empty()) memcpy(out, fr.data(), sizeof(loamx_frontier) * fr.size());
  memcpy(stats, s, sizeof(s));
  return LOAMX_OK;
}

// include/loamx.h, loamx_densemap_frontiers: the grid's kernels as grid() runs them, the rest on their records where they lie
int DenseMap::frontiers(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
                        const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out,
                        uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const loamx_grid_cell* d_cells = grid_.enqueue(tab_, c, rule, (double)cfg.leaf, own_);
  return frontiers_on(d_cells, c.nx, c.nz, rc, fc, start_xz, labels, out, capacity, n_frontiers, stats);
}
// loamx_densemap_frontiers_cells: the same on the caller's records (every cls checked), in the route's buffer for uploads
int DenseMap::frontiers_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc,
                              const loamx_grid_frontier_config& fc, const uint32_t* start_xz, uint32_t* labels, loamx_frontier* out,
                              uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const loamx_grid_cell* d_cells = route_.upload(cells, (size_t)nx * nz, own_);
  return frontiers_on(d_cells, nx, nz, rc, fc, start_xz, labels, out, capacity, n_frontiers, stats);
}

// the checks the two entry points share: the outputs that must be there, both configurations (NULL: the defaults), the window's size
static void checked_frontiers(const loamx_grid_route_config* route_cfg, const loamx_grid_frontier_config* cfg, const uint32_t* start_xz,
                              uint32_t nx, uint32_t nz, const uint64_t* n_frontiers, const uint64_t* stats, loamx_grid_route_config& rc,
                              loamx_grid_frontier_config& fc) {
  LX_REQUIRE(n_frontiers, "n_frontiers is NULL");
  LX_REQUIRE(stats, "stats is NULL");
  fc = or_default(cfg, loamx_grid_frontier_default_config);
  dm_frontier_check(fc);
  rc = or_default(route_cfg, loamx_grid_route_default_config);
  dm_route_check(rc);
  LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= DM_FR_MAX_CELLS, "nx * nz must be in [1, 2^26]");
  LX_REQUIRE(!start_xz || (uint64_t)nx * nz <= DM_FR_MAX_ROUTED, "nx * nz must be in [1, 2^22] with a start_xz: it is routed");
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_grid_frontier_default_config(loamx_grid_frontier_config* cfg) {
  if (!cfg) return;
  cfg->connectivity = 8u;
  cfg->min_unknown = 1u;
  cfg->min_clear2 = 1u;
  cfg->min_cells = 1u;
}

int loamx_grid_frontier_check(const loamx_grid_frontier_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_frontier_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_densemap_frontiers(loamx_densemap* h, const loamx_densemap_grid_config* grid_cfg, const loamx_densemap_static_rule* rule,
                             const loamx_grid_route_config* route_cfg, const loamx_grid_frontier_config* cfg, const uint32_t start_xz[2],
                             uint32_t* labels, loamx_frontier* out, uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    const loamx_densemap_grid_config c = or_default(grid_cfg, loamx_densemap_grid_default_config);
    dm_grid_check(c);
    checked_optional_rule(h, rule);
    loamx_grid_route_config rc;
    loamx_grid_frontier_config fc;
    checked_frontiers(route_cfg, cfg, start_xz, c.nx, c.nz, n_frontiers, stats, rc, fc);
    return h->d.frontiers(c, rule, rc, fc, start_xz, labels, out, capacity, n_frontiers, stats);
  });
}

int loamx_densemap_frontiers_cells(loamx_densemap* h, const loamx_grid_cell* cells, uint32_t nx, uint32_t nz,
                                   const loamx_grid_route_config* route_cfg, const loamx_grid_frontier_config* cfg, const uint32_t start_xz[2],
                                   uint32_t* labels, loamx_frontier* out, uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(cells, "cells is NULL");
    loamx_grid_route_config rc;
    loamx_grid_frontier_config fc;
    checked_frontiers(route_cfg, cfg, start_xz, nx, nz, n_frontiers, stats, rc, fc);
    for (size_t i = 0; i < (size_t)nx * nz; i++)
      LX_REQUIRE(cells[i].cls <= LOAMX_GRID_STEP, "cells: the cls of record " + std::to_string(i) + " is not a class");
    return h->d.frontiers_cells(cells, nx, nz, rc, fc, start_xz, labels, out, capacity, n_frontiers, stats);
  });
}

int loamx_frontiers_best(const loamx_frontier* f, uint64_t n, uint32_t min_cost, uint32_t* best) {
  return guard([&]() {
    LX_REQUIRE(f || !n, "f is NULL");
    LX_REQUIRE(best, "best is NULL");
    LX_REQUIRE(n < LOAMX_FRONTIER_NONE, "n must be below 2^32 - 1");
    uint32_t pick = LOAMX_FRONTIER_NONE, cost = LOAMX_ROUTE_UNREACHABLE;
    for (uint64_t i = 0; i < n; i++)
      if (f[i].best_cost >= min_cost && f[i].best_cost < cost) {   // (strictly below: a tie stays with the smaller index)
        cost = f[i].best_cost;
        pick = (uint32_t)i;
      }
    *best = pick;
    return LOAMX_OK;
  });
}

}  // extern "C"
