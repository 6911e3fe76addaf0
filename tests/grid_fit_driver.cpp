// Host driver of loam_velodyne_amd/csrc/grid_fit.hpp for tests/test_grid_fit.py (built with -fsanitize=undefined,float-cast-overflow
// -fno-sanitize-recover: any undefined conversion or overflow inside grid_fit() ends the run).
//   grid_fit_driver check   the routine against a literal copy of the loop the two index builds used to hold, wherever that loop's
//                           arithmetic is defined; the post-conditions alone wherever it is not.  Prints one line of counts per group.
//   grid_fit_driver eval    stdin: lines of "mn0 mn1 mn2 mx0 mx1 mx2 cell0" as hex float words and the budget in decimal;
//                           stdout: "ox oy oz inv_h" as hex words, "nx ny nz ncell" in decimal.
#include <cfloat>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "grid_fit.hpp"

using loamx::GridDesc;
using loamx::grid_fit;

static const uint32_t MAX_CELLS = 16u * 1024 * 1024 - 2048;

// ---- the former loop, word for word (grid_from_bounds / bb_make_desc before grid_fit.hpp) ----------------------------------------
static GridDesc former_loop(const float mn[3], const float mx[3], float cell0, uint32_t max_cells) {
  float h = cell0;
  GridDesc g;
  for (;;) {
    g.inv_h = 1.0f / h;
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    g.nx = (int)floorf((mx[0] - mn[0]) * g.inv_h) + 1;
    g.ny = (int)floorf((mx[1] - mn[1]) * g.inv_h) + 1;
    g.nz = (int)floorf((mx[2] - mn[2]) * g.inv_h) + 1;
    unsigned long long nc = (unsigned long long)g.nx * g.ny * g.nz;
    if (nc <= max_cells) { g.ncell = (uint32_t)nc; break; }
    h *= 1.25f;
  }
  return g;
}

// one edge length of the former loop looked at without its conversions: the axis quotients as the loop computes them (float), whether
// each count stays below 2^31 and the product below 2^64 (long double holds both exactly enough: the bounds are powers of two and the
// counts integers below 2^31), and whether the table fits
struct Step { bool defined, fits; };
static Step look(const float mn[3], const float mx[3], float h, uint32_t budget) {
  const float inv_h = 1.0f / h;
  long double prod = 1.0L;
  bool ok = true;
  for (int a = 0; a < 3; a++) {
    const float q = floorf((mx[a] - mn[a]) * inv_h);
    if (!(q >= 0.f && q < 2147483648.0f)) { ok = false; continue; }
    prod *= (long double)q + 1.0L;
  }
  Step s;
  s.defined = ok && prod < 18446744073709551616.0L;
  s.fits = ok && prod <= (long double)budget;
  return s;
}
// steps the former loop takes when every edge it tries is defined, -1 otherwise
static int former_defined_steps(const float mn[3], const float mx[3], float cell0, uint32_t budget) {
  float h = cell0;
  for (int k = 0; k < 2000; k++) {
    const Step s = look(mn, mx, h, budget);
    if (!s.defined) return -1;
    if (s.fits) return k;
    h *= 1.25f;
  }
  return -1;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static bool same(const GridDesc& a, const GridDesc& b) {
  return bits(a.ox) == bits(b.ox) && bits(a.oy) == bits(b.oy) && bits(a.oz) == bits(b.oz) && bits(a.inv_h) == bits(b.inv_h) && a.nx == b.nx &&
         a.ny == b.ny && a.nz == b.nz && a.ncell == b.ncell;
}

static void fail(const char* what, const float mn[3], const float mx[3], float cell0, uint32_t budget, const GridDesc& g) {
  printf("FAIL %s: mn %a %a %a mx %a %a %a cell0 %a budget %u -> inv_h %a n %d %d %d ncell %u\n", what, mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], cell0,
         budget, g.inv_h, g.nx, g.ny, g.nz, g.ncell);
  exit(1);
}

// what the routine promises for every input; returns the number of growth steps (found by walking the same edges again)
static int post_conditions(const float mn[3], const float mx[3], float cell0, uint32_t budget) {
  const GridDesc g = grid_fit(mn, mx, cell0, budget);
  if (!(g.nx >= 1 && g.ny >= 1 && g.nz >= 1)) fail("axis counts", mn, mx, cell0, budget, g);
  const unsigned __int128 prod = (unsigned __int128)g.nx * (unsigned __int128)g.ny * (unsigned __int128)g.nz;
  if (prod != g.ncell || g.ncell > budget) fail("ncell", mn, mx, cell0, budget, g);
  if (!(g.inv_h <= 1.0f / cell0 && g.inv_h >= 0.f)) fail("cell edge", mn, mx, cell0, budget, g);
  if (bits(g.ox) != bits(mn[0]) || bits(g.oy) != bits(mn[1]) || bits(g.oz) != bits(mn[2])) fail("origin", mn, mx, cell0, budget, g);
  // the edge is the first of cell0 * 1.25^k that fits
  float h = cell0;
  int k = 0;
  for (; k < 2000; k++) {
    if (bits(1.0f / h) == bits(g.inv_h) || !(1.0f / h > 0.f)) break;
    if (look(mn, mx, h, budget).fits) fail("an earlier edge fitted", mn, mx, cell0, budget, g);
    h *= 1.25f;
  }
  if (1.0f / h > 0.f) {
    if (!look(mn, mx, h, budget).fits) fail("the edge does not fit", mn, mx, cell0, budget, g);
    if (g.nx != (int)floorf((mx[0] - mn[0]) * g.inv_h) + 1 || g.ny != (int)floorf((mx[1] - mn[1]) * g.inv_h) + 1 || g.nz != (int)floorf((mx[2] - mn[2]) * g.inv_h) + 1)
      fail("counts of the edge", mn, mx, cell0, budget, g);
  } else if (g.inv_h != 0.f || g.ncell != 1u) {
    fail("edge beyond the float range", mn, mx, cell0, budget, g);
  }
  return k;
}

struct Counts { long total = 0, defined = 0, grew = 0; int max_steps = 0; };
static void one(const float mn[3], const float mx[3], float cell0, uint32_t budget, Counts& c) {
  const int steps = post_conditions(mn, mx, cell0, budget);
  c.total++;
  if (steps > 0) c.grew++;
  if (steps > c.max_steps) c.max_steps = steps;
  const int fs = former_defined_steps(mn, mx, cell0, budget);
  if (fs >= 0) {
    c.defined++;
    const GridDesc a = grid_fit(mn, mx, cell0, budget), b = former_loop(mn, mx, cell0, budget);
    if (!same(a, b) || fs != steps) fail("differs from the former loop", mn, mx, cell0, budget, a);
  }
}
static void report(const char* name, const Counts& c) {
  printf("%s total %ld defined %ld grew %ld max_steps %d\n", name, c.total, c.defined, c.grew, c.max_steps);
}

static int check() {
  std::mt19937_64 rng(20240607);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  const float cells[] = {1.05f, 2.1f, 0.25f, 16.f, 0.7f, 3.3f};
  const uint32_t Ks[] = {1, 1, 1, 2, 16, 32, 64, 65, 1024, 2048, 4096};
  Counts r;
  for (int it = 0; it < 300000; it++) {
    float mn[3], mx[3];
    // extents log-uniform over 1e-4 .. 1e7 m (the former loop is defined up to about 1e6 m cubes), some axes flat; origins up to +-1e6
    for (int a = 0; a < 3; a++) {
      const double o = (u01(rng) - 0.5) * 2.0 * pow(10.0, u01(rng) * 6.0);
      const double e = u01(rng) < 0.1 ? 0.0 : pow(10.0, -4.0 + 11.0 * u01(rng));
      mn[a] = (float)o;
      mx[a] = (float)(o + e);
      if (mx[a] < mn[a]) mx[a] = mn[a];
    }
    const uint32_t K = Ks[rng() % 11];
    uint32_t budget = MAX_CELLS / K;
    if (rng() % 16 == 0) budget = 1 + (uint32_t)(rng() % 9);
    one(mn, mx, cells[rng() % 6], budget, r);
  }
  report("random", r);

  // the edges of the defined region
  Counts e;
  {
    const float z[3] = {0.f, 0.f, 0.f};
    // cubes around 2642245 cells per axis (2642245^3 < 2^64 < 2642246^3), and exact integer quotients
    for (int n = 2642240; n <= 2642250; n++)
      for (float frac : {0.0f, 0.25f, 0.5f, 0.999f}) {
        const float ext = ((float)n - 1.0f + frac) * 1.05f;
        const float mx[3] = {ext, ext, ext};
        one(z, mx, 1.05f, MAX_CELLS, e);
      }
    // one axis around 2^31 cells, the others flat (defined below 2^31, not from there on)
    for (double q : {2147483000.0, 2147483520.0, 2147483648.0, 2147483904.0, 4294967296.0}) {
      const float ext = (float)(q * 1.05);
      for (int a = 0; a < 3; a++) {
        float mx[3] = {0.f, 0.f, 0.f};
        mx[a] = ext;
        one(z, mx, 1.05f, MAX_CELLS, e);
      }
    }
    // the largest cube the GPU tests use, zero extents, signed zeros, budgets of 1, quotients that are exact integers
    const float big[3] = {1e6f, 1e6f, 1e6f};
    one(z, big, 1.05f, MAX_CELLS, e);
    one(z, z, 1.05f, 1u, e);
    const float nz[3] = {-0.0f, -0.0f, -0.0f};
    one(nz, z, 2.1f, 4095u, e);
    for (int n = 1; n <= 300; n++) {
      const float mx[3] = {0.25f * n, 0.5f * n, 16.f * n}, lo[3] = {-0.25f * n, -7.f, 3.f};
      one(lo, mx, 0.25f, MAX_CELLS / 64, e);
      one(z, mx, 16.f, 1u + (uint32_t)n, e);
    }
  }
  report("edges", e);

  // beyond the former loop: only the post-conditions can be asked for
  Counts x;
  {
    const float z[3] = {0.f, 0.f, 0.f};
    for (float ext : {3e6f, 1e12f, 1e30f, FLT_MAX})
      for (uint32_t budget : {MAX_CELLS, MAX_CELLS / 64, 4095u, 1u}) {
        const float mx[3] = {ext, ext, ext}, lo[3] = {-ext, -ext, -ext};
        one(z, mx, 1.05f, budget, x);
        one(lo, z, 1.05f, budget, x);
      }
    for (int axes = 1; axes <= 7; axes++) {   // +-FLT_MAX on one, two and three axes: mx - mn overflows to infinity
      float mn[3] = {-1.f, -1.f, -1.f}, mx[3] = {2.f, 2.f, 2.f};
      for (int a = 0; a < 3; a++)
        if (axes >> a & 1) { mn[a] = -FLT_MAX; mx[a] = FLT_MAX; }
      one(mn, mx, 1.05f, MAX_CELLS, x);
      one(mn, mx, 16.f, 4095u, x);
    }
    // two axes of 2^31 cells or more and four cells on the third: converted first, the counts are -2^31, -2^31 and 4, whose 64-bit product is 0
    const float wrap[3] = {3e9f, 3e9f, 3.5f};
    one(z, wrap, 1.05f, MAX_CELLS, x);
    const GridDesc g = grid_fit(z, wrap, 1.05f, MAX_CELLS);
    if (g.inv_h >= 1.0f / 1.05f) fail("the wrapped product was accepted", z, wrap, 1.05f, MAX_CELLS, g);
  }
  report("beyond", x);
  if (x.defined != 0) { printf("FAIL: a case of the last group is defined for the former loop\n"); return 1; }
  printf("OK\n");
  return 0;
}

static int eval() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    uint32_t w[7], budget;
    if (sscanf(line, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNu32, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6],
               &budget) != 8)
      return 2;
    const float mn[3] = {from_bits(w[0]), from_bits(w[1]), from_bits(w[2])}, mx[3] = {from_bits(w[3]), from_bits(w[4]), from_bits(w[5])};
    const GridDesc g = grid_fit(mn, mx, from_bits(w[6]), budget);
    printf("%08x %08x %08x %08x %d %d %d %u\n", bits(g.ox), bits(g.oy), bits(g.oz), bits(g.inv_h), g.nx, g.ny, g.nz, g.ncell);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "check")) return check();
  if (argc == 2 && !strcmp(argv[1], "eval")) return eval();
  fprintf(stderr, "usage: grid_fit_driver check | eval\n");
  return 2;
}
