// Routing in 3-D over the distance field (DmRoute3, include/loamx.h loamx_densemap_route3 and what goes with it): the route engine of
// densemap_route_core.hpp for the kind DmRouteVol, compiled here, the relax kernel of that kind, and the entry points.
//
// k_dm_route3_relax, one block of 256 threads per brick of 8 x 8 x 8 cells: the brick's weights and costs with a halo of one cell
// (10^3 cells, 1,000 + 4,000 bytes) go to LDS, every thread works out once, for its two cells, which of the 26 moves are legal and
// what they cost (every intermediate cell of the corner rule lies in the halo, the steps being +-1), the block relaxes in LDS until
// no cell of the brick changes, and writes back the cells that fell.  Only the owning brick writes a cell.  Why the rounds reach the
// fixed point is argued in the head comment of densemap_route.hip, with "brick" for "tile"; three dimensions add to it only that
//   * a brick whose border cell fell marks up to 26 neighbour bricks, every one whose halo holds that cell: a face cell one, an edge
//     cell three, a corner cell seven;
//   * a move is one step on every axis, so the last cell of a cheapest path before it enters a brick lies in that brick's halo, as
//     the induction needs;
//   * the corner rule does not disturb the argument: it only decides which moves exist, from weights, which never change;
//   * the bounds are M < nx * ny * nz for the rounds and 8 * 8 * 8 sweeps and one that finds nothing (512 + 2 in the code) in LDS.
#include "densemap_map.hpp"

namespace loamx {

constexpr int DM_ROUTE3_BRICK = DmRouteVol::TILE;
constexpr int DM_ROUTE3_SIDE = DM_ROUTE3_BRICK + 2;   // with the halo
constexpr int DM_ROUTE3_LDS = DM_ROUTE3_SIDE * DM_ROUTE3_SIDE * DM_ROUTE3_SIDE;
constexpr int DM_ROUTE3_SWEEPS = DM_ROUTE3_BRICK * DM_ROUTE3_BRICK * DM_ROUTE3_BRICK + 2;
constexpr uint32_t DM_ROUTE3_MAX_SIDE = 1024;
constexpr uint32_t DM_ROUTE3_INF = DM_ROUTE_INF;

// one round (the file's head comment).  grid: bricks_x x bricks_y x bricks_z; slot: {bricks that ran, bricks that marked} of this round
__global__ __launch_bounds__(256) void k_dm_route3_relax(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn,
                                                         const unsigned char* __restrict__ w, uint32_t* cost, uint32_t* dirty_read,
                                                         uint32_t* dirty_mark, uint32_t* slot) {
  __shared__ unsigned char s_w[DM_ROUTE3_LDS];
  __shared__ uint32_t s_c[DM_ROUTE3_LDS];
  __shared__ uint32_t s_flag, s_fell;
  const uint32_t brick = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (threadIdx.x == 0) {
    s_flag = dirty_read[brick];
    s_fell = 0u;
  }
  __syncthreads();
  if (!s_flag) return;   // (the whole block alike)
  if (threadIdx.x == 0) dirty_read[brick] = 0u;   // nothing else touches this word in this round
  const int bx = (int)blockIdx.x * DM_ROUTE3_BRICK, by = (int)blockIdx.y * DM_ROUTE3_BRICK, bz = (int)blockIdx.z * DM_ROUTE3_BRICK;
  for (int e = (int)threadIdx.x; e < DM_ROUTE3_LDS; e += 256) {
    const int x = bx - 1 + e % DM_ROUTE3_SIDE, y = by - 1 + (e / DM_ROUTE3_SIDE) % DM_ROUTE3_SIDE,
              z = bz - 1 + e / (DM_ROUTE3_SIDE * DM_ROUTE3_SIDE);
    const bool in = x >= 0 && x < (int)nx && y >= 0 && y < (int)ny && z >= 0 && z < (int)nz;
    const size_t c = in ? ((size_t)(uint32_t)z * ny + (uint32_t)y) * nx + (uint32_t)x : 0;
    s_w[e] = in ? w[c] : (unsigned char)0;   // a cell outside the window is blocked: no move enters it
    s_c[e] = in ? cost[c] : DM_ROUTE3_INF;
  }
  __syncthreads();
  // this thread's two cells: (lx, ly, lz0 + 4 j); per cell the cost of each legal move (0: none) and the cost it came with
  const int lx = (int)threadIdx.x % DM_ROUTE3_BRICK, ly = ((int)threadIdx.x / DM_ROUTE3_BRICK) % DM_ROUTE3_BRICK,
            lz0 = (int)threadIdx.x / (DM_ROUTE3_BRICK * DM_ROUTE3_BRICK);
  constexpr int SY = DM_ROUTE3_SIDE, SZ = DM_ROUTE3_SIDE * DM_ROUTE3_SIDE;
  uint32_t mv[2][26], orig[2];
  bool live[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int e = (lz0 + 4 * j + 1) * SZ + (ly + 1) * SY + lx + 1;
    const uint32_t wa = s_w[e];
    orig[j] = s_c[e];
    live[j] = false;
#pragma unroll
    for (int d = 0; d < 26; d++) {
      int dx, dy, dz;
      dm_route3_move((uint32_t)d, dx, dy, dz);
      const uint32_t wb = s_w[e + dz * SZ + dy * SY + dx];
      bool ok = (uint32_t)d < conn && wa > 0u && wb > 0u;
      // no corner cutting: the cells a + (sx, sy, sz), s in {0, d} per axis, but for a and b
#pragma unroll
      for (int m = 1; m < 7; m++) {
        const int sx = (m & 1) ? dx : 0, sy = (m & 2) ? dy : 0, sz = (m & 4) ? dz : 0;
        if ((sx | sy | sz) && !(sx == dx && sy == dy && sz == dz)) ok = ok && s_w[e + sz * SZ + sy * SY + sx] > 0u;
      }
      mv[j][d] = ok ? dm_route3_scale(dx, dy, dz) * (wa + wb) : 0u;
      live[j] = live[j] || ok;
    }
  }
  bool more = true;
  for (int sweep = 0; sweep < DM_ROUTE3_SWEEPS && more; sweep++) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      if (!live[j]) continue;
      const int e = (lz0 + 4 * j + 1) * SZ + (ly + 1) * SY + lx + 1;
      const uint32_t cur = s_c[e];
      uint32_t best = cur;
#pragma unroll
      for (int d = 0; d < 26; d++) {
        int dx, dy, dz;
        dm_route3_move((uint32_t)d, dx, dy, dz);
        const uint32_t cn = s_c[e + dz * SZ + dy * SY + dx];
        if (mv[j][d] && cn != DM_ROUTE3_INF && cn + mv[j][d] < best) best = cn + mv[j][d];   // (cn < 2^31: no wrap)
      }
      if (best < cur) {
        s_c[e] = best;   // only this thread writes the word; readers take the old or the new value, both upper bounds
        changed = 1;
      }
    }
    more = __syncthreads_or(changed) != 0;
  }
  // the cells that fell go back; which neighbours' halos hold one of them: bit ((dz + 1) * 3 + (dy + 1)) * 3 + (dx + 1)
  uint32_t fell = 0u;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int lz = lz0 + 4 * j, e = (lz + 1) * SZ + (ly + 1) * SY + lx + 1;
    const uint32_t x = (uint32_t)(bx + lx), y = (uint32_t)(by + ly), z = (uint32_t)(bz + lz);
    const uint32_t v = s_c[e];
    if (x < nx && y < ny && z < nz && v < orig[j]) {
      cost[((size_t)z * ny + y) * nx + x] = v;
      const uint32_t xs = 2u | (lx == 0 ? 1u : 0u) | (lx == DM_ROUTE3_BRICK - 1 ? 4u : 0u);
      uint32_t xy = xs << 3;
      if (ly == 0) xy |= xs;
      if (ly == DM_ROUTE3_BRICK - 1) xy |= xs << 6;
      if (lz == 0) fell |= xy;
      fell |= xy << 9;
      if (lz == DM_ROUTE3_BRICK - 1) fell |= xy << 18;
    }
  }
  if (fell) atomicOr(&s_fell, fell);
  __syncthreads();
  if (threadIdx.x == 0) {
    bool marked = false;
    if (more) {   // (the sweep bound was reached unsettled, which the head comment excludes: run again)
      dirty_mark[brick] = 1u;
      marked = true;
    }
    for (int k = 0; k < 27; k++) {
      const int tx = (int)blockIdx.x + k % 3 - 1, ty = (int)blockIdx.y + (k / 3) % 3 - 1, tz = (int)blockIdx.z + k / 9 - 1;
      if (k == 13 || !((s_fell >> k) & 1u) || tx < 0 || tx >= (int)gridDim.x || ty < 0 || ty >= (int)gridDim.y || tz < 0 ||
          tz >= (int)gridDim.z)
        continue;
      dirty_mark[((uint32_t)tz * gridDim.y + (uint32_t)ty) * gridDim.x + (uint32_t)tx] = 1u;
      marked = true;
    }
    atomicAdd(&slot[0], 1u);
    if (marked) atomicAdd(&slot[1], 1u);
  }
}

// Rounds per look: DmRoute3::batch = 16.  Measured on one MI355X, one run (scripts/bench_densemap_route3.py --batches 1,2,4,8,16,32,64;
// the blocking route3_cells with nothing back, the 2 MB upload of the d2 plane included, median of 30 / of 10 after 3 warm-up calls):
//   batch                                            1       2       4       8      16      32      64
//   open, 128 x 64 x 128, goal at the centre      1.17    1.06    1.00    0.99    1.00    0.96    1.03  ms  (17 rounds at batch 1)
//   serpentine3, 128 x 64 x 128                  26.36   21.45   18.97   18.19   17.38   16.97   16.84  ms  (642 rounds at batch 1)
// From 8 to 16 the serpentine still gains 4.5 %; beyond 16 it gains 2.3 % and 3.1 % at the most, the open window nothing outside its
// spread (min .. max of a row's cell is about 3 %), while a window of a few bricks, which settles in two or three rounds, would pay
// for up to 63 idle launches instead of 15.  So the 2-D route's 16 holds here as well.  A round of the serpentine, 2,048 blocks of which
// about 32 run their brick, takes 26 us on average (656 rounds, 20,852 brick runs in 17.4 ms); nothing in the table speaks for a brick
// other than 8 x 8 x 8, and none was tried.
void DmRouteVol::relax(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t connectivity, const unsigned char* w, uint32_t* cost,
                       uint32_t* dirty_read, uint32_t* dirty_mark, uint32_t* slot, hipStream_t st) {
  hipLaunchKernelGGL(k_dm_route3_relax, dim3(dm_route_tiles<DmRouteVol>(nx), dm_route_tiles<DmRouteVol>(ny), dm_route_tiles<DmRouteVol>(nz)),
                     dim3(256), 0, st, nx, ny, nz, connectivity, w, cost, dirty_read, dirty_mark, slot);
}
template class DmRouteT<DmRouteVol>;   // upload, run and trace of the engine, and its four kernels, for the distance field

void dm_route3_check(const loamx_route3_config& c) {
  LX_REQUIRE(c.connectivity == 6u || c.connectivity == 18u || c.connectivity == 26u, "connectivity must be 6, 18 or 26");
  LX_REQUIRE(c.min_d2 >= 1u, "min_d2 must be >= 1");
  LX_REQUIRE(c.soft_d2 <= 65025u, "soft_d2 must be in [0, 65025]");
  LX_REQUIRE(c.soft_weight <= 15u, "soft_weight must be in [0, 15]");
}

// include/loamx.h, loamx_densemap_route3: the distance field as dist() runs it with both planes NULL, the route on its d2 where it lies
void DenseMap::route3(const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, const loamx_route3_config& rc,
                      const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  uint64_t ds[4];
  dist_.run(tab_, c, rule, false, false, ds, own_);
  route3_last(rc, goals_xyz, n_goals, out_field, stats);
}
// loamx_densemap_route3_last: on the field that stands
void DenseMap::route3_last(const loamx_route3_config& rc, const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field,
                           uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const loamx_densemap_dist_config& c = dist_.config();
  route_on(route3_, dist_.d2_on_device(), c.nx, c.ny, c.nz, rc, goals_xyz, n_goals, out_field, stats);
}
// loamx_densemap_route3_cells: the same on the caller's plane, in a buffer of the route's own
void DenseMap::route3_cells(const uint16_t* d2, uint32_t nx, uint32_t ny, uint32_t nz, const loamx_route3_config& rc, const uint32_t* goals_xyz,
                            uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  route_on(route3_, route3_.upload(d2, (size_t)nx * ny * nz, own_), nx, ny, nz, rc, goals_xyz, n_goals, out_field, stats);
}

// the checks the route3 entry points share: the configuration (NULL: the defaults), the goals and the window's size
static loamx_route3_config checked_route3(const loamx_route3_config* cfg, const uint32_t* goals_xyz, uint32_t n_goals, uint32_t nx, uint32_t ny,
                                          uint32_t nz) {
  const loamx_route3_config rc = or_default(cfg, loamx_route3_default_config);
  dm_route3_check(rc);
  dm_route_check_tuples<DmRouteVol>(goals_xyz, n_goals, "goals");
  LX_REQUIRE((uint64_t)nx * ny * nz <= DM_ROUTE_MAX_CELLS, "nx * ny * nz must be <= 2^22 for a route");
  return rc;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_route3_default_config(loamx_route3_config* cfg) {
  if (!cfg) return;
  cfg->connectivity = 26u;
  cfg->min_d2 = 1u;
  cfg->soft_d2 = 0u;
  cfg->soft_weight = 0u;
}

int loamx_route3_check(const loamx_route3_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_route3_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_route3_weight(uint32_t d2, const loamx_route3_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_route3_check(*cfg);
    return (int)dm_route3_weight(d2, *cfg);
  });
}

int loamx_route3_move(uint32_t d, int32_t dxyz[3]) {
  return guard([&]() {
    LX_REQUIRE(d < 26u, "d must be in [0, 25]");
    LX_REQUIRE(dxyz, "dxyz is NULL");
    int dx, dy, dz;
    dm_route3_move(d, dx, dy, dz);
    dxyz[0] = dx;
    dxyz[1] = dy;
    dxyz[2] = dz;
    return LOAMX_OK;
  });
}

int loamx_densemap_route3(loamx_densemap* h, const loamx_densemap_dist_config* dist_cfg, const loamx_densemap_static_rule* rule,
                          const loamx_route3_config* cfg, const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field,
                          uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    const loamx_densemap_dist_config c = or_default(dist_cfg, loamx_densemap_dist_default_config);
    dm_dist_check(c);
    checked_optional_rule(h, rule);
    const loamx_route3_config rc = checked_route3(cfg, goals_xyz, n_goals, c.nx, c.ny, c.nz);
    h->d.route3(c, rule, rc, goals_xyz, n_goals, out_field, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_route3_last(loamx_densemap* h, const loamx_route3_config* cfg, const uint32_t* goals_xyz, uint32_t n_goals,
                               loamx_route_cell* out_field, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(h->d.has_dist(), "the handle has no distance field (loamx_densemap_dist, loamx_densemap_route3)");
    const loamx_densemap_dist_config& c = h->d.dist_config();
    const loamx_route3_config rc = checked_route3(cfg, goals_xyz, n_goals, c.nx, c.ny, c.nz);
    h->d.route3_last(rc, goals_xyz, n_goals, out_field, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_route3_cells(loamx_densemap* h, const uint16_t* d2, uint32_t nx, uint32_t ny, uint32_t nz, const loamx_route3_config* cfg,
                                const uint32_t* goals_xyz, uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(d2, "d2 is NULL");
    LX_REQUIRE(nx >= 1u && nx <= DM_ROUTE3_MAX_SIDE, "nx must be in [1, 1024]");
    LX_REQUIRE(ny >= 1u && ny <= DM_ROUTE3_MAX_SIDE, "ny must be in [1, 1024]");
    LX_REQUIRE(nz >= 1u && nz <= DM_ROUTE3_MAX_SIDE, "nz must be in [1, 1024]");
    const loamx_route3_config rc = checked_route3(cfg, goals_xyz, n_goals, nx, ny, nz);
    h->d.route3_cells(d2, nx, ny, nz, rc, goals_xyz, n_goals, out_field, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_route3_trace(loamx_densemap* h, const uint32_t* starts_xyz, uint32_t n_starts, uint32_t* out_xyz, uint32_t capacity,
                                uint32_t* lengths) {
  return dm_route_trace_entry<DmRouteVol>(h, &DenseMap::router3, starts_xyz, n_starts, out_xyz, capacity, lengths);
}

// bench / test hooks (not in include/loamx.h): the rounds per look (1..64), and the rounds of the last route3 in which a brick ran
int loamx_densemap_route3_set_batch(loamx_densemap* h, uint32_t batch) { return dm_route_set_batch_entry(h, &DenseMap::router3, batch); }
uint64_t loamx_densemap_route3_active_rounds(loamx_densemap* h) { return h ? h->d.router3().active_rounds : 0; }

int loamx_route3_trace(const loamx_route_cell* field, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t start[3], uint32_t* out_xyz,
                       uint32_t capacity, uint32_t* length) {
  return guard([&]() {
    LX_REQUIRE(field, "field is NULL");
    LX_REQUIRE(nx >= 1u && ny >= 1u && nz >= 1u && (uint64_t)nx * ny * nz <= DM_ROUTE_MAX_CELLS && (uint64_t)nx * ny <= DM_ROUTE_MAX_CELLS,
               "nx * ny * nz must be in [1, 2^22]");
    LX_REQUIRE(start, "start is NULL");
    LX_REQUIRE(out_xyz || !capacity, "out_xyz is NULL");
    LX_REQUIRE(length, "length is NULL");
    *length = dm_route_walk<DmRouteVol>(field, nx, ny, nz, start, out_xyz, capacity);
    return LOAMX_OK;
  });
}

int loamx_route3_points(const loamx_densemap_dist_config* dist_cfg, float leaf, const uint32_t* route_xyz, uint32_t n, float* out_xyz) {
  return guard([&]() {
    LX_REQUIRE(dist_cfg, "dist_cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(route_xyz || !n, "route_xyz is NULL");
    LX_REQUIRE(out_xyz || !n, "out_xyz is NULL");
    dm_dist_check(*dist_cfg);
    const loamx_densemap_dist_config& g = *dist_cfg;
    for (uint32_t i = 0; i < n; i++)
      LX_REQUIRE(route_xyz[3 * (size_t)i] < g.nx && route_xyz[3 * (size_t)i + 1] < g.ny && route_xyz[3 * (size_t)i + 2] < g.nz,
                 "route_xyz: triple " + std::to_string(i) + " is outside the window");
    const int32_t first[3] = {g.x0, g.y0, g.z0};
    for (uint32_t i = 0; i < n; i++)
      for (int a = 0; a < 3; a++)
        out_xyz[3 * (size_t)i + a] =
            (float)(((double)first[a] + (double)route_xyz[3 * (size_t)i + a] + 0.5) * (double)leaf * (double)g.cell_leaves);
    return LOAMX_OK;
  });
}

int loamx_densemap_dist_cell_of(const loamx_densemap_dist_config* dist_cfg, float leaf, float x, float y, float z, uint32_t r[3], int* inside) {
  return guard([&]() {
    LX_REQUIRE(dist_cfg, "dist_cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(std::isfinite(x), "x must be finite");
    LX_REQUIRE(std::isfinite(y), "y must be finite");
    LX_REQUIRE(std::isfinite(z), "z must be finite");
    LX_REQUIRE(r, "r is NULL");
    LX_REQUIRE(inside, "inside is NULL");
    dm_dist_check(*dist_cfg);
    const loamx_densemap_dist_config& g = *dist_cfg;
    const double e = (double)leaf * (double)g.cell_leaves;
    const double f[3] = {std::floor((double)x / e) - (double)g.x0, std::floor((double)y / e) - (double)g.y0,
                         std::floor((double)z / e) - (double)g.z0};
    const bool in = f[0] >= 0.0 && f[0] < (double)g.nx && f[1] >= 0.0 && f[1] < (double)g.ny && f[2] >= 0.0 && f[2] < (double)g.nz;
    if (in)
      for (int a = 0; a < 3; a++) r[a] = (uint32_t)f[a];
    *inside = in ? 1 : 0;
    return LOAMX_OK;
  });
}

}  // extern "C"
