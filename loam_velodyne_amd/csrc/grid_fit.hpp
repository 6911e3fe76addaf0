// Grid descriptor of one cloud from its bounds (no HIP in here: tests/test_grid_fit.py drives it on a CPU; k_cell_count and the batch
// index's set-up call it on the device).
//
// The cell edge starts at cell0 and grows by 1.25x while the cell table would not fit its budget (a coarser grid is still exact: the
// 27-cell neighbourhood of a query only grows).  Per axis the cell count is floorf((mx - mn) * inv_h) + 1, inv_h = 1.0f / h in float.
//
// Defined for every input, the bounds of a cloud whose coordinates are merely finite included (the API rejects non-finite
// coordinates and nothing else).  "Does not fit" is decided on the FLOAT quotient, before anything is converted to int:
//   * an axis whose quotient is not in [0, 2^31) does not fit (2^31 cells or more; +inf when mx - mn overflowed; NaN);
//   * otherwise the three counts are ints in [1, 2^31) and their product is taken in two steps, nx * ny <= 2^62 first and, only when
//     that is within the budget (< 2^32), times nz < 2^31: no step can wrap 64 bits, so a product beyond the budget is always seen.
// (Until this routine both builds converted first and multiplied all three in unsigned long long: undefined from 2^31 cells on an
// axis, and a product that wrapped past 2^64 could land under the budget — (-2^31) * (-2^31) * 4 is 0 — with ncell != nx * ny * nz.)
// The edge grows until the table fits.  When h has left the float range (inv_h no longer positive: ~400 steps, reached only with an
// extent near FLT_MAX or one that overflowed) the result is the one-cell grid with inv_h = 0 — every point in cell 0, which is what
// cell_coords' clamp makes of it.  So for budget >= 1 the routine terminates with nx, ny, nz >= 1, ncell == nx * ny * nz <= budget and
// inv_h <= 1 / cell0; wherever the former arithmetic was defined (every axis count below 2^31 at every edge tried, products below
// 2^64) the result is the former one bit for bit: the same float expressions in the same order, the same decisions.
// Expects mn <= mx per axis (bounds of at least one point) and cell0 > 0.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define LX_HOST_DEVICE __host__ __device__
#else
#define LX_HOST_DEVICE
#endif

namespace loamx {

// uniform grid over a sub-map: cell edge >= 1.05 m so the 3x3x3 neighbourhood of a query's cell contains every
// point within the 1 m gate of BasicLaserMapping.cpp:671/:760.
struct GridDesc {
  float ox, oy, oz, inv_h;
  int nx, ny, nz;
  uint32_t ncell;
};

LX_HOST_DEVICE inline GridDesc grid_fit(const float mn[3], const float mx[3], float cell0, uint32_t budget) {
  GridDesc g;
  g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
  float h = cell0;
  for (;;) {
    g.inv_h = 1.0f / h;
    if (!(g.inv_h > 0.f)) {   // h beyond the float range: one cell
      g.inv_h = 0.f;
      g.nx = g.ny = g.nz = 1;
      g.ncell = 1u;
      return g;
    }
    const float qx = floorf((mx[0] - mn[0]) * g.inv_h), qy = floorf((mx[1] - mn[1]) * g.inv_h), qz = floorf((mx[2] - mn[2]) * g.inv_h);
    const float lim = 2147483648.0f;
    if (qx >= 0.f && qx < lim && qy >= 0.f && qy < lim && qz >= 0.f && qz < lim) {   // (false for NaN)
      g.nx = (int)qx + 1; g.ny = (int)qy + 1; g.nz = (int)qz + 1;
      const unsigned long long nxy = (unsigned long long)g.nx * (unsigned long long)g.ny;
      if (nxy <= budget && nxy * (unsigned long long)g.nz <= budget) {
        g.ncell = (uint32_t)(nxy * (unsigned long long)g.nz);
        return g;
      }
    }
    h *= 1.25f;
  }
}

}  // namespace loamx
