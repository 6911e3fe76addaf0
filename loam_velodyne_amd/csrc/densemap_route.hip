// Routing on the navigation grid (densemap.hpp DmRoute, include/loamx.h loamx_densemap_route and what goes with it): the cost-to-go of
// every cell of a window towards a set of goal cells, the next step per cell and routes traced from many starts.
//
// k_dm_route_weights gives every cell its weight (a byte) and the cost UINT32_MAX, k_dm_route_seed puts 0 on the used goals and marks
// their tiles, k_dm_route_relax is launched round after round (densemap_route_schedule.hpp) until no tile is marked, k_dm_route_next
// derives next from the final costs and counts, k_dm_route_trace walks next from many starts.  Integer atomics only; the costs are the
// unique fixed point of cost[c] = min over legal moves of cost[nb] + move, so no word depends on the schedule.
//
// k_dm_route_relax, one block per tile of 32 x 32 cells: the tile's weights and costs with a halo of one cell go to LDS, the block
// relaxes there until no cell of the tile changes, and writes back the cells that fell.  Only the owning tile writes a cell.  A halo
// read of a neighbour that is writing in the same launch is benign: costs only fall, an aligned 32-bit read is whole, and every value
// ever stored is the cost of a real path, an upper bound of the final cost.  Why the rounds reach the fixed point:
//   * a tile whose border cell fell marks, AFTER its stores, every neighbour tile whose halo holds that cell, in the plane of the next
//     round.  A neighbour that read the old value in this launch therefore re-runs behind the kernel boundary, where the new value is
//     visible; a tile that is not marked has a halo that did not change since it last ran, and is at its fixed point already;
//   * so after round r (r = 0: the goals' tiles) every cell whose cheapest path crosses at most r tile borders is final: by induction,
//     the path's last cell h before it enters the tile is final after round r - 1, the round that made it final marked this tile, the
//     tile runs behind that round, reads h final and relaxes the path's stretch inside the tile to the end in LDS.
// With M the largest such count over the reachable cells the costs are final after round M, round M + 1 runs what those last falls
// marked and changes nothing, and no later round runs a tile: at most M + 2 rounds run a tile, M < nx * nz.
// Inside LDS a sweep lowers at least the next cell of every unfinished cheapest path, so 32 * 32 sweeps and one that finds nothing
// bound the loop; the bound is in the code, and a tile that ever left it unsettled would mark itself.
#include "densemap_map.hpp"
#include "densemap_route_schedule.hpp"
#include "pinned_copy.hpp"

namespace loamx {

constexpr int DM_ROUTE_TILE = 32;
constexpr int DM_ROUTE_SIDE = DM_ROUTE_TILE + 2;   // with the halo
constexpr uint32_t DM_ROUTE_MAX_CELLS = 1u << 22;
constexpr uint32_t DM_ROUTE_MAX_XZ = 4096;         // goals, starts
constexpr uint32_t DM_ROUTE_INF = LOAMX_ROUTE_UNREACHABLE;

// (dx, dz) of direction d
__host__ __device__ inline int dm_route_dx(uint32_t d) { return d == 0u || d == 1u || d == 7u ? 1 : (d >= 3u && d <= 5u ? -1 : 0); }
__host__ __device__ inline int dm_route_dz(uint32_t d) { return d >= 1u && d <= 3u ? 1 : (d >= 5u ? -1 : 0); }

__global__ __launch_bounds__(256) void k_dm_route_weights(const loamx_grid_cell* __restrict__ cells, uint32_t n, loamx_grid_route_config C,
                                                          unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                          unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t wt = 0u;
  if (c < n) {
    wt = dm_route_weight(cells[c].cls, cells[c].clear2, C);
    w[c] = (unsigned char)wt;
    cost[c] = DM_ROUTE_INF;
  }
  const unsigned long long b = __ballot(wt > 0u);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&s_n, (uint32_t)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&st[0], (unsigned long long)s_n);
}

// one thread per goal pair: 0 on a used goal (every writer stores the same word), its tile marked for round 0
__global__ __launch_bounds__(256) void k_dm_route_seed(const uint32_t* __restrict__ goals, uint32_t n_goals, uint32_t nx, uint32_t nz,
                                                       uint32_t tiles_x, const unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                       uint32_t* __restrict__ dirty, unsigned long long* __restrict__ st) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_goals) return;
  const uint32_t x = goals[2u * i], z = goals[2u * i + 1u];
  if (x >= nx || z >= nz) return;
  const uint32_t c = z * nx + x;
  if (!w[c]) return;
  cost[c] = 0u;
  dirty[(z / DM_ROUTE_TILE) * tiles_x + x / DM_ROUTE_TILE] = 1u;
  atomicAdd(&st[2], 1ull);
}

// one round (the file's head comment).  grid: tiles_x x tiles_z; slot: {tiles that ran, tiles that marked} of this round
__global__ __launch_bounds__(256) void k_dm_route_relax(uint32_t nx, uint32_t nz, int diag, const unsigned char* __restrict__ w, uint32_t* cost,
                                                        uint32_t* dirty_read, uint32_t* dirty_mark, uint32_t* slot) {
  __shared__ unsigned char s_w[DM_ROUTE_SIDE * DM_ROUTE_SIDE];
  __shared__ uint32_t s_c[DM_ROUTE_SIDE * DM_ROUTE_SIDE];
  __shared__ uint32_t s_flag, s_fell;
  const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x == 0) {
    s_flag = dirty_read[tile];
    s_fell = 0u;
  }
  __syncthreads();
  if (!s_flag) return;   // (the whole block alike)
  if (threadIdx.x == 0) dirty_read[tile] = 0u;   // nothing else touches this word in this round
  const int bx = (int)blockIdx.x * DM_ROUTE_TILE, bz = (int)blockIdx.y * DM_ROUTE_TILE;
  for (int e = (int)threadIdx.x; e < DM_ROUTE_SIDE * DM_ROUTE_SIDE; e += 256) {
    const int x = bx - 1 + e % DM_ROUTE_SIDE, z = bz - 1 + e / DM_ROUTE_SIDE;
    const bool in = x >= 0 && x < (int)nx && z >= 0 && z < (int)nz;
    const size_t c = (size_t)(in ? z : 0) * nx + (uint32_t)(in ? x : 0);
    s_w[e] = in ? w[c] : (unsigned char)0;   // a cell outside the window is blocked: no move enters it
    s_c[e] = in ? cost[c] : DM_ROUTE_INF;
  }
  __syncthreads();
  // this thread's four cells: column lx, rows lz0 + 8 j; per cell the cost of each legal move (0: none) and the cost it came with
  const int lx = (int)threadIdx.x % DM_ROUTE_TILE, lz0 = (int)threadIdx.x / DM_ROUTE_TILE;
  uint32_t mv[4][8], orig[4];
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = (lz0 + 8 * j + 1) * DM_ROUTE_SIDE + lx + 1;
    const uint32_t wa = s_w[e];
    orig[j] = s_c[e];
    live[j] = false;
#pragma unroll
    for (int d = 0; d < 8; d++) {
      const int dx = dm_route_dx((uint32_t)d), dz = dm_route_dz((uint32_t)d);
      const uint32_t wb = s_w[e + dz * DM_ROUTE_SIDE + dx];
      bool ok = wa > 0u && wb > 0u && (!(d & 1) || diag);
      if (d & 1) ok = ok && s_w[e + dx] > 0u && s_w[e + dz * DM_ROUTE_SIDE] > 0u;   // no corner cutting
      mv[j][d] = ok ? ((d & 1) ? 7u : 5u) * (wa + wb) : 0u;
      live[j] = live[j] || ok;
    }
  }
  bool more = true;
  for (int sweep = 0; sweep < DM_ROUTE_TILE * DM_ROUTE_TILE + 2 && more; sweep++) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!live[j]) continue;
      const int e = (lz0 + 8 * j + 1) * DM_ROUTE_SIDE + lx + 1;
      const uint32_t cur = s_c[e];
      uint32_t best = cur;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        const uint32_t cn = s_c[e + dm_route_dz((uint32_t)d) * DM_ROUTE_SIDE + dm_route_dx((uint32_t)d)];
        if (mv[j][d] && cn != DM_ROUTE_INF && cn + mv[j][d] < best) best = cn + mv[j][d];   // (cn < 2^31: no wrap)
      }
      if (best < cur) {
        s_c[e] = best;   // only this thread writes the word; readers take the old or the new value, both upper bounds
        changed = 1;
      }
    }
    more = __syncthreads_or(changed) != 0;
  }
  // the cells that fell go back; which neighbours' halos hold one of them: bit (dz + 1) * 3 + (dx + 1)
  uint32_t fell = 0u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int lz = lz0 + 8 * j, e = (lz + 1) * DM_ROUTE_SIDE + lx + 1;
    const uint32_t x = (uint32_t)(bx + lx), z = (uint32_t)(bz + lz);
    const uint32_t v = s_c[e];
    if (x < nx && z < nz && v < orig[j]) {
      cost[(size_t)z * nx + x] = v;
      const uint32_t xs = 2u | (lx == 0 ? 1u : 0u) | (lx == DM_ROUTE_TILE - 1 ? 4u : 0u);
      if (lz == 0) fell |= xs;
      fell |= xs << 3;
      if (lz == DM_ROUTE_TILE - 1) fell |= xs << 6;
    }
  }
  if (fell) atomicOr(&s_fell, fell);
  __syncthreads();
  if (threadIdx.x == 0) {
    bool marked = false;
    if (more) {   // (the sweep bound was reached unsettled, which the head comment excludes: run again)
      dirty_mark[tile] = 1u;
      marked = true;
    }
    for (int k = 0; k < 9; k++) {
      const int tx = (int)blockIdx.x + k % 3 - 1, tz = (int)blockIdx.y + k / 3 - 1;
      if (k == 4 || !((s_fell >> k) & 1u) || tx < 0 || tx >= (int)gridDim.x || tz < 0 || tz >= (int)gridDim.y) continue;
      dirty_mark[(uint32_t)tz * gridDim.x + (uint32_t)tx] = 1u;
      marked = true;
    }
    atomicAdd(&slot[0], 1u);
    if (marked) atomicAdd(&slot[1], 1u);
  }
}

// one thread per cell: the record from the final costs, the smallest d first; the reachable cells and the largest finite cost
__global__ __launch_bounds__(256) void k_dm_route_next(uint32_t nx, uint32_t nz, int diag, const unsigned char* __restrict__ w,
                                                       const uint32_t* __restrict__ cost, loamx_route_cell* __restrict__ field,
                                                       unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n, s_max;
  if (threadIdx.x == 0) s_n = s_max = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  bool reach = false;
  if (c < nx * nz) {
    const uint32_t x = c % nx, z = c / nx, cc = cost[c], wa = w[c];
    uint32_t next = LOAMX_ROUTE_NONE;
    reach = cc != DM_ROUTE_INF;
    if (cc == 0u) next = LOAMX_ROUTE_GOAL;
    else if (reach) {
      for (uint32_t d = 0; d < 8u && next == LOAMX_ROUTE_NONE; d += diag ? 1u : 2u) {
        const int dx = dm_route_dx(d), dz = dm_route_dz(d);
        const uint32_t bxx = x + (uint32_t)dx, bzz = z + (uint32_t)dz;   // (a cell before the window wraps)
        if (bxx >= nx || bzz >= nz) continue;
        const uint32_t nb = bzz * nx + bxx, wb = w[nb], cn = cost[nb];
        if (!wb || cn == DM_ROUTE_INF) continue;
        if ((d & 1u) && (!w[z * nx + bxx] || !w[bzz * nx + x])) continue;
        if (cn + ((d & 1u) ? 7u : 5u) * (wa + wb) == cc) next = d;
      }
      atomicMax(&s_max, cc);
    }
    loamx_route_cell r;
    r.cost = cc;
    r.next = next;
    field[c] = r;
  }
  const unsigned long long b = __ballot(reach);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&s_n, (uint32_t)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) {
    atomicAdd(&st[1], (unsigned long long)s_n);
    atomicMax(&st[3], (unsigned long long)s_max);
  }
}

// one thread per start, walking next; bounded by nx * nz steps.  offsets NULL: the lengths only.  Otherwise start i's pairs go to
// out + 2 * offsets[i], the first min(length, capacity) of them (the same walk as the counting pass over the same field)
__global__ __launch_bounds__(256) void k_dm_route_trace(const loamx_route_cell* __restrict__ field, uint32_t nx, uint32_t nz,
                                                        const uint32_t* __restrict__ starts, uint32_t n_starts, uint32_t capacity,
                                                        const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ lengths,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_starts) return;
  uint32_t x = starts[2u * i], z = starts[2u * i + 1u], len = 0u;
  if (x < nx && z < nz) {
    const uint32_t cells = nx * nz;
    for (uint32_t step = 0; step < cells; step++) {
      const uint32_t next = field[(size_t)z * nx + x].next;
      if (next >= LOAMX_ROUTE_NONE) break;
      if (offsets && len < capacity) {
        out[2ull * (offsets[i] + len)] = x;
        out[2ull * (offsets[i] + len) + 1ull] = z;
      }
      len++;
      if (next == LOAMX_ROUTE_GOAL) break;
      x += (uint32_t)dm_route_dx(next);
      z += (uint32_t)dm_route_dz(next);
      if (x >= nx || z >= nz) break;   // (never on a field of k_dm_route_next)
    }
  }
  if (!offsets) lengths[i] = len;
}

void dm_route_check(const loamx_grid_route_config& c) {
  LX_REQUIRE(c.connectivity == 4u || c.connectivity == 8u, "connectivity must be 4 or 8");
  LX_REQUIRE(c.min_clear2 >= 1u, "min_clear2 must be >= 1");
  LX_REQUIRE(c.soft_clear2 <= 4225u, "soft_clear2 must be in [0, 4225]");
  LX_REQUIRE(c.soft_weight <= 15u, "soft_weight must be in [0, 15]");
  LX_REQUIRE(c.unknown_weight <= 16u, "unknown_weight must be in [0, 16]");
}

const loamx_grid_cell* DmRoute::upload(const loamx_grid_cell* cells, size_t n, hipStream_t st) {
  own_cells_.reserve(n);
  LX_HIP(hipMemcpyAsync(own_cells_.p, cells, sizeof(loamx_grid_cell) * n, hipMemcpyHostToDevice, st));
  return own_cells_.p;
}

// Rounds per look: DmRoute::batch = 16.  Measured on one MI355X, one run (scripts/bench_densemap_route.py --batches 1,2,4,8,16,32,64;
// the blocking call with nothing back, median of 30 / of 10; a look is about 14 us, an idle round of 1024 blocks 2 to 5):
//   batch                                   1       2       4       8      16      32      64
//   terrain, 1024 x 1024, 33 rounds      2.27    2.01    1.89    1.87    1.82    1.88    1.81  ms
//   serpentine, 1024 x 1024, 7969 rounds 454.9   391.5   359.8   349.5   338.6   333.2   330.3 ms
// From 8 to 16 both still gain; beyond 16 the terrain gains nothing and the serpentine 2.4 % at most, while a window of a few tiles,
// which settles in two or three rounds, would pay for up to 63 idle launches instead of 15.
const loamx_route_cell* DmRoute::run(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& c,
                                     const uint32_t* goals_xz, uint32_t n_goals, bool want_field, uint64_t stats[6], hipStream_t st) {
  const uint32_t n = nx * nz, tiles_x = (nx + DM_ROUTE_TILE - 1) / DM_ROUTE_TILE, tiles_z = (nz + DM_ROUTE_TILE - 1) / DM_ROUTE_TILE;
  const uint32_t tiles = tiles_x * tiles_z;
  constexpr uint32_t CTR_WORDS = 2u * ROUTE_MAX_BATCH, ST_WORDS = 8u;   // the slots; the four 64-bit stats as 32-bit words
  valid_ = false;
  w_.reserve(n);
  cost_.reserve(n);
  field_.reserve(n);
  dirty_.reserve(2 * (size_t)tiles);
  ctr_.reserve(CTR_WORDS);
  st_.reserve(ST_WORDS / 2);
  d_xz_.reserve(2 * DM_ROUTE_MAX_XZ);
  h_xz_.reserve(2 * DM_ROUTE_MAX_XZ);
  h_ctr_.reserve(CTR_WORDS + ST_WORDS);
  if (want_field) h_field_.reserve(n);
  memcpy(h_xz_.p, goals_xz, sizeof(uint32_t) * 2 * n_goals);
  LX_HIP(hipMemcpyAsync(d_xz_.p, h_xz_.p, sizeof(uint32_t) * 2 * n_goals, hipMemcpyHostToDevice, st));
  LX_HIP(hipMemsetAsync(dirty_.p, 0, sizeof(uint32_t) * 2 * (size_t)tiles, st));
  LX_HIP(hipMemsetAsync(st_.p, 0, sizeof(uint32_t) * ST_WORDS, st));
  const dim3 per_cell((n + 255u) / 256u), per_tile(tiles_x, tiles_z);
  const int diag = c.connectivity == 8u ? 1 : 0;
  hipLaunchKernelGGL(k_dm_route_weights, per_cell, dim3(256), 0, st, d_cells, n, c, w_.p, cost_.p, st_.p);
  hipLaunchKernelGGL(k_dm_route_seed, dim3((n_goals + 255u) / 256u), dim3(256), 0, st, d_xz_.p, n_goals, nx, nz, tiles_x, w_.p, cost_.p,
                     dirty_.p, st_.p);
  LX_HIP(hipGetLastError());
  struct Ops {
    DmRoute& r;
    uint32_t nx, nz, tiles;
    int diag;
    dim3 per_tile;
    hipStream_t st;
    void begin(uint32_t) { LX_HIP(hipMemsetAsync(r.ctr_.p, 0, sizeof(uint32_t) * CTR_WORDS, st)); }
    void round(uint64_t, uint32_t read_plane, uint32_t mark_plane, uint32_t slot) {
      hipLaunchKernelGGL(k_dm_route_relax, per_tile, dim3(256), 0, st, nx, nz, diag, r.w_.p, r.cost_.p, r.dirty_.p + (size_t)read_plane * tiles,
                         r.dirty_.p + (size_t)mark_plane * tiles, r.ctr_.p + 2u * slot);
    }
    const RouteSlot* look(uint32_t k) {
      LX_HIP(hipGetLastError());
      store_to_pinned_u32(r.h_ctr_.p, r.ctr_.p, 2u * k, st);
      LX_HIP(hipStreamSynchronize(st));
      return (const RouteSlot*)r.h_ctr_.p;
    }
  } ops{*this, nx, nz, tiles, diag, per_tile, st};
  const RouteOutcome o = route_schedule(ops, RoutePlan{batch, (uint64_t)n + 2u});
  if (!o.settled) throw Error(LOAMX_E_INTERNAL, "route: the relaxation did not settle within nx * nz + 2 rounds");
  hipLaunchKernelGGL(k_dm_route_next, per_cell, dim3(256), 0, st, nx, nz, diag, w_.p, cost_.p, field_.p, st_.p);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_ctr_.p + CTR_WORDS, (const uint32_t*)st_.p, ST_WORDS, st);
  if (want_field) h_field_.fetch(field_.p, n, st);
  LX_HIP(hipStreamSynchronize(st));
  uint64_t s4[4];
  memcpy(s4, h_ctr_.p + CTR_WORDS, sizeof(s4));
  for (int k = 0; k < 4; k++) stats[k] = s4[k];
  stats[4] = o.rounds;
  stats[5] = o.tile_runs;
  active_rounds = o.active_rounds;
  nx_ = nx;
  nz_ = nz;
  valid_ = true;
  return want_field ? h_field_.data() : nullptr;
}

void DmRoute::trace(const uint32_t* starts_xz, uint32_t n_starts, uint32_t* out_xz, uint32_t capacity, uint32_t* lengths, hipStream_t st) {
  d_xz_.reserve(2 * DM_ROUTE_MAX_XZ);
  h_xz_.reserve(2 * DM_ROUTE_MAX_XZ);
  d_len_.reserve(DM_ROUTE_MAX_XZ);
  d_off_.reserve(DM_ROUTE_MAX_XZ);
  h_len_.reserve(DM_ROUTE_MAX_XZ);
  h_off_.reserve(DM_ROUTE_MAX_XZ);
  memcpy(h_xz_.p, starts_xz, sizeof(uint32_t) * 2 * n_starts);
  LX_HIP(hipMemcpyAsync(d_xz_.p, h_xz_.p, sizeof(uint32_t) * 2 * n_starts, hipMemcpyHostToDevice, st));
  const dim3 per_start((n_starts + 255u) / 256u);
  hipLaunchKernelGGL(k_dm_route_trace, per_start, dim3(256), 0, st, field_.p, nx_, nz_, d_xz_.p, n_starts, capacity,
                     (const unsigned long long*)nullptr, d_len_.p, (uint32_t*)nullptr);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_len_.p, d_len_.p, n_starts, st);
  LX_HIP(hipStreamSynchronize(st));
  // the routes back to back on the device: start i's min(length, capacity) pairs begin at pair offsets[i]
  size_t total = 0;
  for (uint32_t i = 0; i < n_starts; i++) {
    h_off_.p[i] = total;
    total += std::min(h_len_.p[i], capacity);
  }
  if (total) {
    d_routes_.reserve(2 * total);
    h_routes_.reserve(2 * total);
    LX_HIP(hipMemcpyAsync(d_off_.p, h_off_.p, sizeof(unsigned long long) * n_starts, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dm_route_trace, per_start, dim3(256), 0, st, field_.p, nx_, nz_, d_xz_.p, n_starts, capacity, d_off_.p, d_len_.p,
                       d_routes_.p);
    LX_HIP(hipGetLastError());
    store_to_pinned_u32(h_routes_.p, d_routes_.p, 2 * total, st);
    LX_HIP(hipStreamSynchronize(st));
  }
  for (uint32_t i = 0; i < n_starts; i++) {
    const size_t m = std::min(h_len_.p[i], capacity);
    if (m) memcpy(out_xz + 2 * (size_t)capacity * i, h_routes_.p + 2 * (size_t)h_off_.p[i], sizeof(uint32_t) * 2 * m);
    lengths[i] = h_len_.p[i];
  }
}

// include/loamx.h, loamx_densemap_route: the grid's kernels as grid() runs them, the route on their records where they lie
void DenseMap::route(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
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
void DenseMap::route_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc, const uint32_t* goals_xz,
                           uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const size_t n = (size_t)nx * nz;
  uint64_t s[6];
  const loamx_route_cell* field = route_.run(route_.upload(cells, n, own_), nx, nz, rc, goals_xz, n_goals, out_field != nullptr, s, own_);
  if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * n);
  if (stats) memcpy(stats, s, sizeof(s));
}
void DenseMap::route_trace(const uint32_t* starts_xz, uint32_t n_starts, uint32_t* out_xz, uint32_t capacity, uint32_t* lengths) {
  LX_REQUIRE(route_.has_field(), "the handle has no field yet (loamx_densemap_route, loamx_densemap_route_cells)");
  LX_HIP(hipSetDevice(cfg.device));
  route_.trace(starts_xz, n_starts, out_xz, capacity, lengths, own_);
}

// the checks the route's entry points share: the configuration (NULL: the defaults), the goals and the window's size
static loamx_grid_route_config checked_route(const loamx_grid_route_config* cfg, const uint32_t* goals_xz, uint32_t n_goals, uint32_t nx,
                                             uint32_t nz) {
  const loamx_grid_route_config rc = or_default(cfg, loamx_grid_route_default_config);
  dm_route_check(rc);
  LX_REQUIRE(goals_xz, "goals_xz is NULL");
  LX_REQUIRE(n_goals >= 1u && n_goals <= 4096u, "n_goals must be in [1, 4096]");
  LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= (1ull << 22), "nx * nz must be in [1, 2^22] for a route");
  return rc;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_grid_route_default_config(loamx_grid_route_config* cfg) {
  if (!cfg) return;
  cfg->connectivity = 8u;
  cfg->min_clear2 = 1u;
  cfg->soft_clear2 = 0u;
  cfg->soft_weight = 0u;
  cfg->unknown_weight = 0u;
}

int loamx_grid_route_check(const loamx_grid_route_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_route_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_grid_route_weight(const loamx_grid_cell* cell, const loamx_grid_route_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cell, "cell is NULL");
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_route_check(*cfg);
    return (int)dm_route_weight(cell->cls, cell->clear2, *cfg);
  });
}

int loamx_densemap_route(loamx_densemap* h, const loamx_densemap_grid_config* grid_cfg, const loamx_densemap_static_rule* rule,
                         const loamx_grid_route_config* cfg, const uint32_t* goals_xz, uint32_t n_goals, loamx_grid_cell* out_cells,
                         loamx_route_cell* out_field, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    const loamx_densemap_grid_config c = or_default(grid_cfg, loamx_densemap_grid_default_config);
    dm_grid_check(c);
    checked_optional_rule(h, rule);
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

// bench / test hooks (not in include/loamx.h): the route's rounds per look (1..64), and the rounds of the last route in which a tile ran
int loamx_densemap_route_set_batch(loamx_densemap* h, uint32_t batch) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(batch >= 1u && batch <= 64u, "batch must be in [1, 64]");
    h->d.router().batch = batch;
    return LOAMX_OK;
  });
}
uint64_t loamx_densemap_route_active_rounds(loamx_densemap* h) { return h ? h->d.router().active_rounds : 0; }

int loamx_grid_route_trace(const loamx_route_cell* field, uint32_t nx, uint32_t nz, uint32_t start_x, uint32_t start_z, uint32_t* out_xz,
                           uint32_t capacity, uint32_t* length) {
  return guard([&]() {
    LX_REQUIRE(field, "field is NULL");
    LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= DM_ROUTE_MAX_CELLS, "nx * nz must be in [1, 2^22]");
    LX_REQUIRE(out_xz || !capacity, "out_xz is NULL");
    LX_REQUIRE(length, "length is NULL");
    uint32_t len = 0;
    // the walk twice: checked to its end first, so that a field that is not one of ours leaves nothing written
    for (int pass = 0; pass < 2; pass++) {
      uint32_t x = start_x, z = start_z;
      len = 0;
      if (x >= nx || z >= nz) break;
      for (;;) {
        const loamx_route_cell& r = field[(size_t)z * nx + x];
        LX_REQUIRE(r.next <= LOAMX_ROUTE_NONE, "field: a next above 9");
        if (r.next == LOAMX_ROUTE_NONE) {
          LX_REQUIRE(len == 0u, "field: the route ends on a cell that is no goal");
          break;
        }
        if (pass && len < capacity) {
          out_xz[2 * (size_t)len] = x;
          out_xz[2 * (size_t)len + 1] = z;
        }
        len++;
        if (r.next == LOAMX_ROUTE_GOAL) break;
        const uint32_t bx = x + (uint32_t)dm_route_dx(r.next), bz = z + (uint32_t)dm_route_dz(r.next);
        LX_REQUIRE(bx < nx && bz < nz, "field: a step leaves the window");
        LX_REQUIRE(field[(size_t)bz * nx + bx].cost < r.cost, "field: a step to a cell whose cost is not strictly smaller");
        x = bx;
        z = bz;
      }
    }
    *length = len;
    return LOAMX_OK;
  });
}

int loamx_grid_route_points(const loamx_densemap_grid_config* grid_cfg, float leaf, const loamx_grid_cell* cells, const uint32_t* route_xz,
                            uint32_t n, float* out_xyz) {
  return guard([&]() {
    LX_REQUIRE(grid_cfg, "grid_cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(route_xz || !n, "route_xz is NULL");
    LX_REQUIRE(out_xyz || !n, "out_xyz is NULL");
    dm_grid_check(*grid_cfg);
    const loamx_densemap_grid_config& g = *grid_cfg;
    for (uint32_t i = 0; i < n; i++)
      LX_REQUIRE(route_xz[2 * (size_t)i] < g.nx && route_xz[2 * (size_t)i + 1] < g.nz,
                 "route_xz: pair " + std::to_string(i) + " is outside the window");
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t rx = route_xz[2 * (size_t)i], rz = route_xz[2 * (size_t)i + 1];
      float y = 0.f;
      if (cells) {
        const loamx_grid_cell& c = cells[(size_t)rz * g.nx + rx];
        if (c.cls != LOAMX_GRID_UNKNOWN) y = c.elevation;
      }
      out_xyz[3 * (size_t)i] = (float)(((double)g.x0 + (double)rx + 0.5) * (double)leaf * (double)g.cell_leaves);
      out_xyz[3 * (size_t)i + 1] = y;
      out_xyz[3 * (size_t)i + 2] = (float)(((double)g.z0 + (double)rz + 0.5) * (double)leaf * (double)g.cell_leaves);
    }
    return LOAMX_OK;
  });
}

int loamx_densemap_grid_cell_of(const loamx_densemap_grid_config* grid_cfg, float leaf, float x, float z, uint32_t* rx, uint32_t* rz,
                                int* inside) {
  return guard([&]() {
    LX_REQUIRE(grid_cfg, "grid_cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(std::isfinite(x), "x must be finite");
    LX_REQUIRE(std::isfinite(z), "z must be finite");
    LX_REQUIRE(rx, "rx is NULL");
    LX_REQUIRE(rz, "rz is NULL");
    LX_REQUIRE(inside, "inside is NULL");
    dm_grid_check(*grid_cfg);
    const double e = (double)leaf * (double)grid_cfg->cell_leaves;
    const double fx = std::floor((double)x / e) - (double)grid_cfg->x0, fz = std::floor((double)z / e) - (double)grid_cfg->z0;
    const bool in = fx >= 0.0 && fx < (double)grid_cfg->nx && fz >= 0.0 && fz < (double)grid_cfg->nz;
    if (in) {
      *rx = (uint32_t)fx;
      *rz = (uint32_t)fz;
    }
    *inside = in ? 1 : 0;
    return LOAMX_OK;
  });
}

}  // extern "C"
