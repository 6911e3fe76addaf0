// Navigation grid of the dense map (densemap.hpp DmGrid, include/loamx.h loamx_densemap_grid and what goes with it): a window of the
// voxel table projected along +y to nx * nz cells of ground, elevation, obstacle count, overhead, class and clearance.
//
// Four plain launches behind one memset.  Two scans of the table, one thread per slot, coalesced over the keys: the first takes the
// minimum iy per cell, the second, with that ground final, adds the ground layer's n and Sy, counts the voxels of the body band and
// takes the minimum iy above it.  Then one thread per cell writes the record, and a tiled pass through LDS gives clear2 in the exact
// separable form.  Integer atomics only, so no word depends on the schedule; the one f32 rounding is the elevation's.
//
// The planes are zeroed by the one memset, so the two minima are kept as iy - 2^20: always negative, 0 = no voxel yet.
#include "densemap_map.hpp"
#include "pinned_copy.hpp"
#include <climits>

namespace loamx {

// 32-bit words per cell in DmGrid::planes_, plane after plane: SSn and SSy (64-bit each), then ground, overhead and obstacles
constexpr int DM_GRID_PLANE_WORDS = 7;
constexpr int DM_GRID_TILE = 32;       // k_dm_grid_clear: cells per tile side
constexpr int DM_GRID_MAX_R = 64;      // the largest clear_max
constexpr int DM_GRID_HALO_SIDE = DM_GRID_TILE + 2 * DM_GRID_MAX_R;

struct DmGridArgs {
  uint32_t k, nx, nz, min_points;
  int x0, z0, y_min, y_max;
  uint32_t band_lo, band_hi, min_obstacles, max_step, R;
  int use_rule;
  loamx_densemap_static_rule rule;
  double leaf;
};
struct DmGridPlanes {
  unsigned long long *ssn, *ssy;
  int *ground, *overhead;   // iy - 2^20 of the minimum; 0: none
  uint32_t* obstacles;
};

// the voxel of slot i against the window and the qualifying rule of include/loamx.h: false for a slot beyond the table, a free slot
// and a voxel that does not qualify; otherwise its record index, iy and point count
__device__ inline bool dm_grid_voxel(const DmGridArgs& G, uint32_t i, uint32_t slots, const unsigned long long* __restrict__ keys,
                                     const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux, uint32_t& cell, int& iy,
                                     unsigned long long& n) {
  if (i >= slots) return false;
  const unsigned long long key = keys[i];
  if (key == DM_EMPTY) return false;
  const uint32_t km = (1u << DM_KBITS) - 1u;
  const uint32_t fx = (uint32_t)key & km, fy = (uint32_t)(key >> DM_KBITS) & km, fz = (uint32_t)(key >> (2 * DM_KBITS)) & km;   // i + 2^20
  // floor(i / k) = (i + k * 2^20) / k - 2^20: the dividend is unsigned and below 2^27 for k <= 64
  const uint32_t bias = (G.k - 1u) << DM_QBITS;
  const int cx = (int)((fx + bias) / G.k) - (1 << DM_QBITS), cz = (int)((fz + bias) / G.k) - (1 << DM_QBITS);
  const uint32_t rx = (uint32_t)(cx - G.x0), rz = (uint32_t)(cz - G.z0);   // (|c| <= 2^20, |x0| <= 2^21; a cell before the window wraps)
  if (rx >= G.nx || rz >= G.nz) return false;
  iy = (int)fy - (1 << DM_QBITS);
  if (iy < G.y_min || iy > G.y_max) return false;
  n = vals[4ull * i];
  if (n < G.min_points) return false;
  if (G.use_rule && dm_dynamic(G.rule, n, aux[2ull * i])) return false;
  cell = rz * G.nx + rx;
  return true;
}

__global__ __launch_bounds__(256) void k_dm_grid_ground(DmGridArgs G, const unsigned long long* __restrict__ keys,
                                                        const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                        uint32_t slots, DmGridPlanes P) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t cell = 0;
  int iy = 0;
  unsigned long long n = 0;
  if (dm_grid_voxel(G, i, slots, keys, vals, aux, cell, iy, n)) atomicMin(&P.ground[cell], iy - (1 << DM_QBITS));
}

// the same scan with the ground final (the launch before this one): the ground layer's sums, the body band's count, the overhead
__global__ __launch_bounds__(256) void k_dm_grid_fill(DmGridArgs G, const unsigned long long* __restrict__ keys,
                                                      const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                      uint32_t slots, DmGridPlanes P) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t cell = 0;
  int iy = 0;
  unsigned long long n = 0;
  if (!dm_grid_voxel(G, i, slots, keys, vals, aux, cell, iy, n)) return;
  const uint32_t d = (uint32_t)(iy - (P.ground[cell] + (1 << DM_QBITS)));   // (>= 0: the ground is the minimum over this voxel too)
  if (d == 0u) {
    atomicAdd(&P.ssn[cell], n);
    atomicAdd(&P.ssy[cell], vals[4ull * i + 2]);
  } else if (d >= G.band_lo && d <= G.band_hi) {
    atomicAdd(&P.obstacles[cell], 1u);
  } else if (d > G.band_hi) {
    atomicMin(&P.overhead[cell], iy - (1 << DM_QBITS));
  }
}

// one thread per cell: the record but for clear2.  A neighbour is UNKNOWN exactly when its ground word is 0
__global__ __launch_bounds__(256) void k_dm_grid_classify(DmGridArgs G, DmGridPlanes P, loamx_grid_cell* __restrict__ out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= G.nx * G.nz) return;
  const int gv = P.ground[c];
  loamx_grid_cell r;
  r.ground = INT_MAX;
  r.elevation = 0.f;
  r.obstacles = 0u;
  r.overhead = INT_MAX;
  r.clear2 = 0u;
  r.cls = LOAMX_GRID_UNKNOWN;
  if (gv != 0) {
    r.ground = gv + (1 << DM_QBITS);
    r.elevation = (float)(((double)r.ground + (double)P.ssy[c] / ((double)P.ssn[c] * 1048576.0)) * G.leaf);
    r.obstacles = P.obstacles[c];
    const int ov = P.overhead[c];
    if (ov != 0) r.overhead = ov + (1 << DM_QBITS);
    const uint32_t x = c % G.nx, z = c / G.nx;
    auto steps = [&](uint32_t nb) {
      const int gn = P.ground[nb];
      return gn != 0 && (uint32_t)(gn > gv ? gn - gv : gv - gn) > G.max_step;
    };
    if (r.obstacles >= G.min_obstacles) r.cls = LOAMX_GRID_OBSTACLE;
    else if ((x > 0u && steps(c - 1u)) || (x + 1u < G.nx && steps(c + 1u)) || (z > 0u && steps(c - G.nx)) || (z + 1u < G.nz && steps(c + G.nx)))
      r.cls = LOAMX_GRID_STEP;
    else r.cls = LOAMX_GRID_FREE;
  }
  out[c] = r;
}

// clear2, exact and separable, one block per tile of 32 x 32 cells: the obstacle flags of the tile and a halo of R cells go to LDS
// (a byte each; cells outside the window are no obstacles), a row pass gives every cell of the tile's columns, over the tile's rows
// and the halo's, the distance g <= R in x to the nearest flag of its row (R + 1: none), and the column pass takes the minimum of
// g*g + dz*dz over |dz| <= R.  If the nearest obstacle lies within R it has |dx|, |dz| <= R, so the column pass meets it; a sum above
// R*R is capped like no obstacle at all.  Lanes of a wave read consecutive bytes of a row (one dword serves four lanes) and every
// loop is bounded by R <= 64 or by the halo's size.  LDS: 160 x 160 + 160 x 32 bytes at R = 64, 30 KiB per block
__global__ __launch_bounds__(256) void k_dm_grid_clear(uint32_t nx, uint32_t nz, int R, loamx_grid_cell* __restrict__ out) {
  __shared__ unsigned char s_flag[DM_GRID_HALO_SIDE * DM_GRID_HALO_SIDE];
  __shared__ unsigned char s_g[DM_GRID_HALO_SIDE * DM_GRID_TILE];
  const int side = DM_GRID_TILE + 2 * R;   // of the halo square, in x and in z
  const int bx = (int)blockIdx.x * DM_GRID_TILE, bz = (int)blockIdx.y * DM_GRID_TILE;   // the tile's first cell, window-relative
  for (int e = (int)threadIdx.x; e < side * side; e += 256) {
    const int x = bx - R + e % side, z = bz - R + e / side;
    const bool in = x >= 0 && x < (int)nx && z >= 0 && z < (int)nz;
    s_flag[e] = in && out[(size_t)z * nx + (uint32_t)x].cls >= LOAMX_GRID_OBSTACLE ? 1 : 0;
  }
  __syncthreads();
  for (int e = (int)threadIdx.x; e < side * DM_GRID_TILE; e += 256) {
    const int xl = e % DM_GRID_TILE, zr = e / DM_GRID_TILE;   // column of the tile, row of the halo square
    const unsigned char* row = s_flag + zr * side + R + xl;   // (row[-R .. R] lies inside the halo square's row)
    int g = R + 1;
    for (int d = 0; d <= R; d++)
      if (row[d] | row[-d]) { g = d; break; }
    s_g[e] = (unsigned char)g;
  }
  __syncthreads();
  const uint32_t cap = (uint32_t)((R + 1) * (R + 1));
  for (int e = (int)threadIdx.x; e < DM_GRID_TILE * DM_GRID_TILE; e += 256) {
    const int xl = e % DM_GRID_TILE, zl = e / DM_GRID_TILE;
    const uint32_t x = (uint32_t)(bx + xl), z = (uint32_t)(bz + zl);
    if (x >= nx || z >= nz) continue;
    uint32_t best = cap;
    for (int dz = -R; dz <= R; dz++) {
      const int g = s_g[(zl + R + dz) * DM_GRID_TILE + xl];
      const uint32_t v = (uint32_t)(g * g + dz * dz);
      if (g <= R && v < best) best = v;
    }
    out[(size_t)z * nx + x].clear2 = best <= (uint32_t)(R * R) ? best : cap;
  }
}

const loamx_grid_cell* DmGrid::enqueue(const DmTable& T, const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule,
                                       double leaf, hipStream_t st) {
  const size_t cells = (size_t)c.nx * c.nz;   // (<= 2^26)
  planes_.reserve(DM_GRID_PLANE_WORDS * cells);
  cells_.reserve(cells);
  DmGridArgs G;
  G.k = c.cell_leaves; G.nx = c.nx; G.nz = c.nz; G.min_points = c.min_points;
  G.x0 = c.x0; G.z0 = c.z0; G.y_min = c.y_min; G.y_max = c.y_max;
  G.band_lo = c.band_lo; G.band_hi = c.band_hi; G.min_obstacles = c.min_obstacle_voxels; G.max_step = c.max_step; G.R = c.clear_max;
  G.use_rule = rule ? 1 : 0;
  G.rule = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
  G.leaf = leaf;
  DmGridPlanes P;
  P.ssn = (unsigned long long*)planes_.p;
  P.ssy = P.ssn + cells;
  P.ground = (int*)(planes_.p + 4 * cells);
  P.overhead = P.ground + cells;
  P.obstacles = planes_.p + 6 * cells;
  LX_HIP(hipMemsetAsync(planes_.p, 0, sizeof(uint32_t) * DM_GRID_PLANE_WORDS * cells, st));
  const dim3 scan((T.slots + 255u) / 256u), per_cell((uint32_t)((cells + 255) / 256));
  hipLaunchKernelGGL(k_dm_grid_ground, scan, dim3(256), 0, st, G, T.keys, T.vals, T.aux, T.slots, P);
  hipLaunchKernelGGL(k_dm_grid_fill, scan, dim3(256), 0, st, G, T.keys, T.vals, T.aux, T.slots, P);
  hipLaunchKernelGGL(k_dm_grid_classify, per_cell, dim3(256), 0, st, G, P, cells_.p);
  hipLaunchKernelGGL(k_dm_grid_clear, dim3((c.nx + DM_GRID_TILE - 1) / DM_GRID_TILE, (c.nz + DM_GRID_TILE - 1) / DM_GRID_TILE), dim3(256), 0, st,
                     c.nx, c.nz, (int)c.clear_max, cells_.p);
  LX_HIP(hipGetLastError());
  return cells_.p;
}

const loamx_grid_cell* DmGrid::fetch(const loamx_grid_cell* d_cells, size_t n, hipStream_t st) {
  const loamx_grid_cell* cells = h_cells_.fetch(d_cells, n, st);
  LX_HIP(hipStreamSynchronize(st));
  return cells;
}

void dm_grid_check(const loamx_densemap_grid_config& c) {
  LX_REQUIRE(c.cell_leaves >= 1u && c.cell_leaves <= 64u, "cell_leaves must be in [1, 64]");
  LX_REQUIRE(c.x0 >= -(1 << 21) && c.x0 <= (1 << 21), "x0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.z0 >= -(1 << 21) && c.z0 <= (1 << 21), "z0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.nx >= 1u && c.nx <= 8192u, "nx must be in [1, 8192]");
  LX_REQUIRE(c.nz >= 1u && c.nz <= 8192u, "nz must be in [1, 8192]");
  LX_REQUIRE((uint64_t)c.nx * c.nz <= (1ull << 26), "nx * nz must be <= 2^26");
  LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
  LX_REQUIRE(c.y_min <= c.y_max, "y_min must be <= y_max");
  LX_REQUIRE(c.band_lo >= 1u, "band_lo must be >= 1");
  LX_REQUIRE(c.band_hi >= c.band_lo, "band_hi must be >= band_lo");
  LX_REQUIRE(c.min_obstacle_voxels >= 1u, "min_obstacle_voxels must be >= 1");
  LX_REQUIRE(c.clear_max <= (uint32_t)DM_GRID_MAX_R, "clear_max must be in [0, 64]");
}

// the window of one axis (include/loamx.h, loamx_densemap_grid_window)
static void grid_window_axis(double e, float centre, float half, const char* first, const char* count, int32_t& lo_out, uint32_t& n_out) {
  const double lo = std::floor(((double)centre - (double)half) / e), hi = std::floor(((double)centre + (double)half) / e);
  LX_REQUIRE(std::fabs(lo) <= 2097152.0, std::string(first) + " of the window is outside [-2^21, 2^21]");
  LX_REQUIRE(hi - lo + 1.0 <= 8192.0, std::string(count) + " of the window is above 8192");
  lo_out = (int32_t)lo;
  n_out = (uint32_t)(hi - lo + 1.0);
}

static unsigned char grid_pixel(uint32_t cls) { return cls == LOAMX_GRID_UNKNOWN ? 205 : (cls == LOAMX_GRID_FREE ? 254 : 0); }

// include/loamx.h, loamx_densemap_grid
void DenseMap::grid(const loamx_densemap_grid_config& c, const loamx_densemap_static_rule* rule, loamx_grid_cell* out) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const loamx_grid_cell* cells = grid_.run(tab_, c, rule, (double)cfg.leaf, own_);
  memcpy(out, cells, sizeof(loamx_grid_cell) * (size_t)c.nx * c.nz);
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_grid_default_config(loamx_densemap_grid_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->cell_leaves = 2u;
  cfg->x0 = cfg->z0 = 0;
  cfg->nx = cfg->nz = 256u;
  cfg->min_points = 2u;
  cfg->y_min = -(1 << 20);
  cfg->y_max = 1 << 20;
  cfg->band_lo = 3u;
  cfg->band_hi = 20u;
  cfg->min_obstacle_voxels = 1u;
  cfg->max_step = 2u;
  cfg->clear_max = 10u;
}

int loamx_densemap_grid_check(const loamx_densemap_grid_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_grid_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_densemap_grid(loamx_densemap* h, const loamx_densemap_grid_config* cfg, const loamx_densemap_static_rule* rule,
                        loamx_grid_cell* out) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(out, "out is NULL");
    const loamx_densemap_grid_config c = or_default(cfg, loamx_densemap_grid_default_config);
    dm_grid_check(c);
    checked_optional_rule(h, rule);
    h->d.grid(c, rule, out);
    return LOAMX_OK;
  });
}

int loamx_densemap_grid_window(float leaf, float centre_x, float centre_z, float half_extent, loamx_densemap_grid_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(std::isfinite(centre_x), "centre_x must be finite");
    LX_REQUIRE(std::isfinite(centre_z), "centre_z must be finite");
    LX_REQUIRE(half_extent >= 0.f && std::isfinite(half_extent), "half_extent must be >= 0");
    LX_REQUIRE(cfg->cell_leaves >= 1u && cfg->cell_leaves <= 64u, "cell_leaves must be in [1, 64]");
    const double e = (double)leaf * (double)cfg->cell_leaves;
    loamx_densemap_grid_config c = *cfg;
    grid_window_axis(e, centre_x, half_extent, "x0", "nx", c.x0, c.nx);
    grid_window_axis(e, centre_z, half_extent, "z0", "nz", c.z0, c.nz);
    *cfg = c;
    return LOAMX_OK;
  });
}

int loamx_grid_occupancy(const loamx_grid_cell* cells, uint64_t n, int8_t* out) {
  return guard([&]() {
    LX_REQUIRE(cells || !n, "cells is NULL");
    LX_REQUIRE(out || !n, "out is NULL");
    for (uint64_t i = 0; i < n; i++)
      LX_REQUIRE(cells[i].cls <= LOAMX_GRID_STEP, "cells: the cls of record " + std::to_string(i) + " is not a class");
    for (uint64_t i = 0; i < n; i++)
      out[i] = cells[i].cls == LOAMX_GRID_UNKNOWN ? (int8_t)-1 : (cells[i].cls == LOAMX_GRID_FREE ? (int8_t)0 : (int8_t)100);
    return LOAMX_OK;
  });
}

int loamx_write_grid_pgm(const char* stem, const loamx_grid_cell* cells, const loamx_densemap_grid_config* cfg, float leaf) {
  return guard([&]() {
    LX_REQUIRE(stem, "stem is NULL");
    LX_REQUIRE(cells, "cells is NULL");
    LX_REQUIRE(cfg, "cfg is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    dm_grid_check(*cfg);
    const uint32_t nx = cfg->nx, nz = cfg->nz;
    std::vector<unsigned char> px((size_t)nx * nz);
    for (uint32_t r = 0; r < nx; r++)   // file row r, column u: cell (x0 + nx - 1 - r, z0 + u)
      for (uint32_t u = 0; u < nz; u++) px[(size_t)r * nz + u] = grid_pixel(cells[(size_t)u * nx + (nx - 1u - r)].cls);
    const std::string pgm = std::string(stem) + ".pgm", yaml = std::string(stem) + ".yaml";
    FILE* f = fopen(pgm.c_str(), "wb");
    LX_REQUIRE(f, "cannot open " + pgm + " for writing");
    bool ok = fprintf(f, "P5\n%u %u\n255\n", nz, nx) > 0 && fwrite(px.data(), 1, px.size(), f) == px.size();
    ok = (fclose(f) == 0) && ok;
    LX_REQUIRE(ok, "write to " + pgm + " failed");
    const size_t slash = pgm.find_last_of('/');
    const double res = (double)leaf * (double)cfg->cell_leaves;
    f = fopen(yaml.c_str(), "wb");
    LX_REQUIRE(f, "cannot open " + yaml + " for writing");
    ok = fprintf(f, "image: %s\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
                 pgm.c_str() + (slash == std::string::npos ? 0 : slash + 1), res, (double)cfg->z0 * res, (double)cfg->x0 * res) > 0;
    ok = (fclose(f) == 0) && ok;
    LX_REQUIRE(ok, "write to " + yaml + " failed");
    return LOAMX_OK;
  });
}

}  // extern "C"
