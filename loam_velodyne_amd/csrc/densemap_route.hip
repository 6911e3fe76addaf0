// Routing on the navigation grid (DmRoute, include/loamx.h loamx_densemap_route and what goes with it): the route engine of
// densemap_route_core.hpp for the kind DmRouteGrid, compiled here, the relax kernel of that kind, and the entry points.
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

namespace loamx {

constexpr int DM_ROUTE_TILE = DmRouteGrid::TILE;
constexpr int DM_ROUTE_SIDE = DM_ROUTE_TILE + 2;   // with the halo

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

// Rounds per look: DmRoute::batch = 16.  Measured on one MI355X, one run (scripts/bench_densemap_route.py --batches 1,2,4,8,16,32,64;
// the blocking call with nothing back, median of 30 / of 10; a look is about 14 us, an idle round of 1024 blocks 2 to 5):
//   batch                                   1       2       4       8      16      32      64
//   terrain, 1024 x 1024, 33 rounds      2.27    2.01    1.89    1.87    1.82    1.88    1.81  ms
//   serpentine, 1024 x 1024, 7969 rounds 454.9   391.5   359.8   349.5   338.6   333.2   330.3 ms
// From 8 to 16 both still gain; beyond 16 the terrain gains nothing and the serpentine 2.4 % at most, while a window of a few tiles,
// which settles in two or three rounds, would pay for up to 63 idle launches instead of 15.
void DmRouteGrid::relax(uint32_t nx, uint32_t, uint32_t nz, uint32_t connectivity, const unsigned char* w, uint32_t* cost,
                        uint32_t* dirty_read, uint32_t* dirty_mark, uint32_t* slot, hipStream_t st) {
  hipLaunchKernelGGL(k_dm_route_relax, dim3(dm_route_tiles<DmRouteGrid>(nx), dm_route_tiles<DmRouteGrid>(nz)), dim3(256), 0, st, nx, nz,
                     connectivity == 8u ? 1 : 0, w, cost, dirty_read, dirty_mark, slot);
}
template class DmRouteT<DmRouteGrid>;   // upload, run and trace of the engine, and its four kernels, for the grid

void dm_route_check(const loamx_grid_route_config& c) {
  LX_REQUIRE(c.connectivity == 4u || c.connectivity == 8u, "connectivity must be 4 or 8");
  LX_REQUIRE(c.min_clear2 >= 1u, "min_clear2 must be >= 1");
  LX_REQUIRE(c.soft_clear2 <= 4225u, "soft_clear2 must be in [0, 4225]");
  LX_REQUIRE(c.soft_weight <= 15u, "soft_weight must be in [0, 15]");
  LX_REQUIRE(c.unknown_weight <= 16u, "unknown_weight must be in [0, 16]");
}

// include/loamx.h, loamx_densemap_route: the grid's kernels as grid() runs them, the route on their records where they lie
void DenseMap::route(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, const loamx_grid_route_config& rc,
                     const uint32_t* goals_xz, uint32_t n_goals, loamx_grid_cell* out_cells, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const size_t n = (size_t)c.nx * c.nz;
  const loamx_grid_cell* d_cells = grid_.enqueue(tab_, c, rule, (double)cfg.leaf, own_);
  route_on(route_, d_cells, c.nx, 1u, c.nz, rc, goals_xz, n_goals, out_field, stats, [&] {
    if (out_cells) memcpy(out_cells, grid_.fetch(d_cells, n, own_), sizeof(loamx_grid_cell) * n);
  });
}
// loamx_densemap_route_cells: the same on the caller's records (every cls checked), in a buffer of the route's own
void DenseMap::route_cells(const loamx_grid_cell* cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& rc, const uint32_t* goals_xz,
                           uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  route_on(route_, route_.upload(cells, (size_t)nx * nz, own_), nx, 1u, nz, rc, goals_xz, n_goals, out_field, stats);
}

// the checks the route's entry points share: the configuration (NULL: the defaults), the goals and the window's size
static loamx_grid_route_config checked_route(const loamx_grid_route_config* cfg, const uint32_t* goals_xz, uint32_t n_goals, uint32_t nx,
                                             uint32_t nz) {
  const loamx_grid_route_config rc = or_default(cfg, loamx_grid_route_default_config);
  dm_route_check(rc);
  dm_route_check_tuples<DmRouteGrid>(goals_xz, n_goals, "goals");
  LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= DM_ROUTE_MAX_CELLS, "nx * nz must be in [1, 2^22] for a route");
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
  return dm_route_trace_entry<DmRouteGrid>(h, &DenseMap::router, starts_xz, n_starts, out_xz, capacity, lengths);
}

// bench / test hooks (not in include/loamx.h): the route's rounds per look (1..64), and the rounds of the last route in which a tile ran
int loamx_densemap_route_set_batch(loamx_densemap* h, uint32_t batch) { return dm_route_set_batch_entry(h, &DenseMap::router, batch); }
uint64_t loamx_densemap_route_active_rounds(loamx_densemap* h) { return h ? h->d.router().active_rounds : 0; }

int loamx_grid_route_trace(const loamx_route_cell* field, uint32_t nx, uint32_t nz, uint32_t start_x, uint32_t start_z, uint32_t* out_xz,
                           uint32_t capacity, uint32_t* length) {
  return guard([&]() {
    LX_REQUIRE(field, "field is NULL");
    LX_REQUIRE(nx >= 1u && nz >= 1u && (uint64_t)nx * nz <= DM_ROUTE_MAX_CELLS, "nx * nz must be in [1, 2^22]");
    LX_REQUIRE(out_xz || !capacity, "out_xz is NULL");
    LX_REQUIRE(length, "length is NULL");
    const uint32_t start[2] = {start_x, start_z};
    *length = dm_route_walk<DmRouteGrid>(field, nx, 1u, nz, start, out_xz, capacity);
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
