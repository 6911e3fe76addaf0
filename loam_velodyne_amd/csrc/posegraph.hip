// Pose graph (posegraph.hpp, posegraph_schedule.hpp, include/loamx.h loamx_posegraph_*): Levenberg-Marquardt over SE(3) poses in FP64,
// every step on the device.
//
// One step: k_pg_linearise (an edge per 12 lanes: the residual and the Jacobians by the edge's first lane into LDS, then one column
// of (J_i | J_j) per lane: the three 6x6 blocks and the two 6-vectors of the edge, stored per edge), k_pg_gather (per node the diagonal
// block and the gradient along the node's row of the node -> incident-edge table), k_pg_precond (per node the inverse of
// (1 + lambda) * diagonal block by a 6x6 Cholesky), then block-Jacobi PCG over the stored blocks: per iteration k_pg_cg_ap,
// k_pg_final, k_pg_cg_update, k_pg_final, k_pg_cg_p, all of which return at once when the `done` word is set.  k_pg_apply backs the
// poses up and applies the step, k_pg_cost and k_pg_sum give the trial cost.
//
// No floating-point atomics.  A row of the table lists (edge, side) in ascending edge id (built on the host when the edges change), and
// a lane walks its row from the first entry to the last, however long the row is: a sum over a node's edges has that one order.  Dot
// products and costs go through per-block partials of a fixed tree shape and one block that adds the partials in a fixed order.  A
// run is reproducible to the bit, and does not depend on cg_batch.
#include "posegraph.hpp"
#include "posegraph_schedule.hpp"
#include "common.h"
#include "pinned_copy.hpp"
#include <algorithm>
#include <memory>
#include <numeric>

namespace loamx {

struct PgScalars {
  double rz, rz0, pAp, alpha, beta, cost, trial, max_delta, tol2, reserved;
  uint32_t done, iterations, bad_pivots, pad;
};
enum PgFinal : int { PG_F_RZ0 = 0, PG_F_PAP = 1, PG_F_RZ = 2, PG_F_COST = 3, PG_F_TRIAL = 4, PG_F_MAXD = 5 };

constexpr int PG_LIN_EDGES = 16;                  // edges per workgroup of k_pg_linearise
constexpr int PG_LIN_THREADS = 12 * PG_LIN_EDGES;
constexpr int PG_GATHER_LANES = 42;               // per node: 36 entries of the diagonal block, 6 of the gradient

// sum (or maximum) of one value per thread over a workgroup of 256, by a tree of fixed shape; the result is valid in every thread
__device__ inline double pg_block_reduce(double v, double* sh, bool is_max) {
  const int t = (int)threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] = is_max ? fmax(sh[t], sh[t + s]) : sh[t] + sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(PG_LIN_THREADS) void k_pg_linearise(const double* __restrict__ poses, const uint32_t* __restrict__ eij,
                                                                 const uint32_t* __restrict__ eflags, const double* __restrict__ ez,
                                                                 const double* __restrict__ einfo, uint32_t n_edges, double huber,
                                                                 double* __restrict__ H, double* __restrict__ gE, double* __restrict__ chi2,
                                                                 double* __restrict__ rho) {
  __shared__ double sJ[PG_LIN_EDGES][72];
  __shared__ double sr[PG_LIN_EDGES][6];
  __shared__ double sw[PG_LIN_EDGES];
  const int le = (int)threadIdx.x / 12, c = (int)threadIdx.x % 12;
  const uint32_t e = blockIdx.x * PG_LIN_EDGES + le;
  if (c == 0 && e < n_edges) {
    const uint32_t i = eij[2 * e], j = eij[2 * e + 1];
    PgResidual s;
    pg_residual(poses + 12 * (size_t)i, poses + 12 * (size_t)j, ez + 12 * (size_t)e, s);
    pg_jacobians(ez + 12 * (size_t)e, s, sJ[le]);
    const double x2 = pg_chi2(einfo + 21 * (size_t)e, s.r);
    double w, rh;
    pg_huber(x2, (eflags[e] & LOAMX_PG_EDGE_ROBUST) != 0u && huber > 0.0, huber, w, rh);
#pragma unroll
    for (int k = 0; k < 6; k++) sr[le][k] = s.r[k];
    sw[le] = w;
    chi2[e] = x2;
    rho[e] = rh;
  }
  __syncthreads();
  if (e >= n_edges) return;
  const double* info = einfo + 21 * (size_t)e;
  const double* J = sJ[le];
  const double w = sw[le];
  double u[6];   // column c of (w Omega) (J_i | J_j)
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double row = 0.0;
#pragma unroll
    for (int m = 0; m < 6; m++) row = row + info[pg_tri(k, m)] * J[12 * m + c];
    u[k] = w * row;
  }
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) g = g + u[k] * sr[le][k];
  gE[12 * (size_t)e + c] = g;
  double* He = H + 108 * (size_t)e;
  if (c < 6) {
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double h = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) h = h + J[12 * k + a] * u[k];
      He[6 * a + c] = h;                       // J_i^T W J_i
    }
  } else {
    const int b = c - 6;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double hij = 0.0, hjj = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        hij = hij + J[12 * k + a] * u[k];
        hjj = hjj + J[12 * k + 6 + a] * u[k];
      }
      He[36 + 6 * a + b] = hij;                // J_i^T W J_j
      He[72 + 6 * a + b] = hjj;                // J_j^T W J_j
    }
  }
}

// per edge rho(chi2) at the current poses (the trial cost)
__global__ __launch_bounds__(256) void k_pg_cost(const double* __restrict__ poses, const uint32_t* __restrict__ eij, const uint32_t* __restrict__ eflags,
                                                 const double* __restrict__ ez, const double* __restrict__ einfo, uint32_t n_edges, double huber,
                                                 double* __restrict__ rho) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_edges) return;
  PgResidual s;
  pg_residual(poses + 12 * (size_t)eij[2 * e], poses + 12 * (size_t)eij[2 * e + 1], ez + 12 * (size_t)e, s);
  const double x2 = pg_chi2(einfo + 21 * (size_t)e, s.r);
  double w, rh;
  pg_huber(x2, (eflags[e] & LOAMX_PG_EDGE_ROBUST) != 0u && huber > 0.0, huber, w, rh);
  rho[e] = rh;
}

// lane (node, q): q < 36 entry q of the node's diagonal block, else entry q - 36 of its gradient; zeros for a fixed node
__global__ __launch_bounds__(256) void k_pg_gather(const uint32_t* __restrict__ row, const uint32_t* __restrict__ ents, const uint32_t* __restrict__ fixed,
                                                   const double* __restrict__ H, const double* __restrict__ gE, uint32_t n_nodes,
                                                   double* __restrict__ D, double* __restrict__ grad) {
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = (uint32_t)(g / PG_GATHER_LANES);
  const int q = (int)(g % PG_GATHER_LANES);
  if (n >= n_nodes) return;
  double acc = 0.0;
  if (!fixed[n]) {
    const uint32_t lo = row[n], hi = row[n + 1];
    for (uint32_t k = lo; k < hi; k++) {
      const uint32_t ent = ents[k], e = ent >> 1, side = ent & 1u;
      acc = acc + (q < 36 ? H[108 * (size_t)e + (side ? 72 : 0) + q] : gE[12 * (size_t)e + 6 * side + (q - 36)]);
    }
  }
  if (q < 36) D[36 * (size_t)n + q] = acc;
  else grad[6 * (size_t)n + (q - 36)] = acc;
}

__global__ void k_pg_begin(PgScalars* S, double tol2) {
  S->done = 0u;
  S->iterations = 0u;
  S->bad_pivots = 0u;
  S->tol2 = tol2;
}

// per node: Minv = ((1 + lambda) D)^-1 by Cholesky (the lower triangle of D is read); zeros for a fixed node and for a node with a
// pivot that is not positive, which is counted
__global__ __launch_bounds__(256) void k_pg_precond(const double* __restrict__ D, const uint32_t* __restrict__ fixed, uint32_t n_nodes, double lambda,
                                                    double* __restrict__ Minv, PgScalars* S) {
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  if (n >= n_nodes) return;
  double L[6][6];
  bool ok = !fixed[n];
  if (ok) {
    const double* Dn = D + 36 * (size_t)n;
    const double scale = 1.0 + lambda;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = 0; b <= a; b++) {
        double s = scale * Dn[6 * a + b];
#pragma unroll
        for (int k = 0; k < b; k++) s = s - L[a][k] * L[b][k];
        if (a == b) {
          if (!(s > 0.0)) ok = false;
          L[a][a] = sqrt(s);
        } else {
          L[a][b] = s / L[b][b];
        }
      }
    }
    if (!ok) atomicAdd(&S->bad_pivots, 1u);
  }
  double* Mn = Minv + 36 * (size_t)n;
  if (!ok) {
#pragma unroll
    for (int q = 0; q < 36; q++) Mn[q] = 0.0;
    return;
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double y[6], x[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double s = a == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < a; k++) s = s - L[a][k] * y[k];
      y[a] = s / L[a][a];
    }
#pragma unroll
    for (int a = 5; a >= 0; a--) {
      double s = y[a];
#pragma unroll
      for (int k = a + 1; k < 6; k++) s = s - L[k][a] * x[k];
      x[a] = s / L[a][a];
    }
#pragma unroll
    for (int a = 0; a < 6; a++) Mn[6 * a + c] = x[a];
  }
}

// per node: x = 0, r = -g, z = Minv r, p = z; per workgroup the partial of r.z
__global__ __launch_bounds__(256) void k_pg_cg_init(const double* __restrict__ grad, const double* __restrict__ Minv, uint32_t n_nodes,
                                                    double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                                                    double* __restrict__ partials) {
  __shared__ double sh[256];
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  double dot = 0.0;
  if (n < n_nodes) {
    double rn[6];
#pragma unroll
    for (int a = 0; a < 6; a++) rn[a] = -grad[6 * (size_t)n + a];
    const double* Mn = Minv + 36 * (size_t)n;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double zn = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) zn = zn + Mn[6 * a + b] * rn[b];
      x[6 * (size_t)n + a] = 0.0;
      r[6 * (size_t)n + a] = rn[a];
      z[6 * (size_t)n + a] = zn;
      p[6 * (size_t)n + a] = zn;
      dot = dot + rn[a] * zn;
    }
  }
  const double s = pg_block_reduce(dot, sh, false);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// lane (node, a): Ap = row a of (H + lambda D) p, the edges of the node in the order of its row; per workgroup the partial of p.Ap
__global__ __launch_bounds__(256) void k_pg_cg_ap(const uint32_t* __restrict__ row, const uint32_t* __restrict__ ents, const uint32_t* __restrict__ eij,
                                                  const uint32_t* __restrict__ fixed, const double* __restrict__ H, const double* __restrict__ D,
                                                  const double* __restrict__ p, uint32_t n_nodes, double lambda, double* __restrict__ Ap,
                                                  double* __restrict__ partials, const PgScalars* S) {
  __shared__ double sh[256];
  if (S->done) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = (uint32_t)(g / 6);
  const int a = (int)(g % 6);
  double dot = 0.0;
  if (n < n_nodes) {
    double acc = 0.0;
    if (!fixed[n]) {
      const double* pn = p + 6 * (size_t)n;
      const uint32_t lo = row[n], hi = row[n + 1];
      for (uint32_t k = lo; k < hi; k++) {
        const uint32_t ent = ents[k], e = ent >> 1, side = ent & 1u;
        const double* He = H + 108 * (size_t)e;
        const double* pm = p + 6 * (size_t)eij[2 * e + (side ^ 1u)];
        double own = 0.0, other = 0.0;
        if (side == 0u) {
#pragma unroll
          for (int b = 0; b < 6; b++) { own = own + He[6 * a + b] * pn[b]; other = other + He[36 + 6 * a + b] * pm[b]; }
        } else {
#pragma unroll
          for (int b = 0; b < 6; b++) { own = own + He[72 + 6 * a + b] * pn[b]; other = other + He[36 + 6 * b + a] * pm[b]; }
        }
        acc = acc + own;
        acc = acc + other;
      }
      double damp = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) damp = damp + D[36 * (size_t)n + 6 * a + b] * pn[b];
      acc = acc + lambda * damp;
      dot = pn[a] * acc;
    }
    Ap[6 * (size_t)n + a] = acc;
  }
  const double s = pg_block_reduce(dot, sh, false);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// per node: x += alpha p, r -= alpha Ap, z = Minv r; per workgroup the partial of r.z
__global__ __launch_bounds__(256) void k_pg_cg_update(const double* __restrict__ Minv, const double* __restrict__ p, const double* __restrict__ Ap,
                                                      uint32_t n_nodes, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                      double* __restrict__ partials, const PgScalars* S) {
  __shared__ double sh[256];
  if (S->done) return;
  const double alpha = S->alpha;
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  double dot = 0.0;
  if (n < n_nodes) {
    double rn[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
      const size_t q = 6 * (size_t)n + a;
      x[q] = x[q] + alpha * p[q];
      rn[a] = r[q] - alpha * Ap[q];
      r[q] = rn[a];
    }
    const double* Mn = Minv + 36 * (size_t)n;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double zn = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) zn = zn + Mn[6 * a + b] * rn[b];
      z[6 * (size_t)n + a] = zn;
      dot = dot + rn[a] * zn;
    }
  }
  const double s = pg_block_reduce(dot, sh, false);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_pg_cg_p(const double* __restrict__ z, uint64_t n, double* __restrict__ p, const PgScalars* S) {
  if (S->done) return;
  const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (q < n) p[q] = z[q] + S->beta * p[q];
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, the tree adds the 256 sums; thread 0 then does what `mode` asks
__global__ __launch_bounds__(256) void k_pg_final(const double* __restrict__ partials, uint32_t n, PgScalars* S, int mode) {
  __shared__ double sh[256];
  if ((mode == PG_F_PAP || mode == PG_F_RZ) && S->done) return;
  const bool is_max = mode == PG_F_MAXD;
  double v = 0.0;
  for (uint32_t k = threadIdx.x; k < n; k += 256u) v = is_max ? fmax(v, partials[k]) : v + partials[k];
  const double s = pg_block_reduce(v, sh, is_max);
  if (threadIdx.x != 0) return;
  switch (mode) {
    case PG_F_RZ0:
      S->rz = s;
      S->rz0 = s;
      if (!(s > 0.0)) S->done = 1u;
      break;
    case PG_F_PAP:
      S->pAp = s;
      if (s > 0.0) S->alpha = S->rz / s;
      else { S->alpha = 0.0; S->done = 1u; }   // (no descent along p: the solve ends with the iterate it has)
      break;
    case PG_F_RZ:
      S->iterations = S->iterations + 1u;
      if (s <= S->tol2 * S->rz0) S->done = 1u;
      else S->beta = s / S->rz;
      S->rz = s;
      break;
    case PG_F_COST: S->cost = s; break;
    case PG_F_TRIAL: S->trial = s; break;
    default: S->max_delta = s; break;
  }
}

// per workgroup the partial sum of v[0..n)
__global__ __launch_bounds__(256) void k_pg_sum(const double* __restrict__ v, uint32_t n, double* __restrict__ partials) {
  __shared__ double sh[256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const double s = pg_block_reduce(i < n ? v[i] : 0.0, sh, false);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// per node: backup <- pose; a free node is retracted by its part of x; per workgroup the largest |x| entry
__global__ __launch_bounds__(256) void k_pg_apply(const double* __restrict__ x, const uint32_t* __restrict__ fixed, uint32_t n_nodes,
                                                  double* __restrict__ poses, double* __restrict__ backup, double* __restrict__ partials) {
  __shared__ double sh[256];
  const uint32_t n = blockIdx.x * 256u + threadIdx.x;
  double m = 0.0;
  if (n < n_nodes) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
      T[k] = poses[12 * (size_t)n + k];
      backup[12 * (size_t)n + k] = T[k];
    }
    if (!fixed[n]) {
      double d[6];
#pragma unroll
      for (int a = 0; a < 6; a++) {
        d[a] = x[6 * (size_t)n + a];
        m = fmax(m, fabs(d[a]));
      }
      pg_retract(T, d);
#pragma unroll
      for (int k = 0; k < 12; k++) poses[12 * (size_t)n + k] = T[k];
    }
  }
  const double s = pg_block_reduce(m, sh, true);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_pg_copy(const double* __restrict__ src, uint64_t n, double* __restrict__ dst) {
  const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (q < n) dst[q] = src[q];
}

// ---- host-side checks (no device) -------------------------------------------------------------------------------------------------
static void pg_check_pose(const double* T, const std::string& what) {
  for (int k = 0; k < 12; k++) LX_REQUIRE(std::isfinite(T[k]), what + ": a non-finite entry");
  double R[9], G[9];
  pg_rot(T, R);
  pg_mtm(R, R, G);
  double worst = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) worst = std::max(worst, std::fabs(G[3 * i + j] - (i == j ? 1.0 : 0.0)));
  LX_REQUIRE(worst <= 1e-6, what + ": the rotation is not orthonormal (max |R^T R - I| > 1e-6)");
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  LX_REQUIRE(det > 0.0, what + ": the rotation has a negative determinant");
}
static void pg_check_edge(const loamx_posegraph_edge& e, uint32_t n_nodes, const std::string& what) {
  LX_REQUIRE(e.i < n_nodes, what + ".i: no such node");
  LX_REQUIRE(e.j < n_nodes, what + ".j: no such node");
  LX_REQUIRE(e.i != e.j, what + ": i == j");
  pg_check_pose(e.z, what + ".z");
  for (int k = 0; k < 21; k++) LX_REQUIRE(std::isfinite(e.info[k]), what + ".info: a non-finite entry");
  for (int k = 0; k < 6; k++) LX_REQUIRE(e.info[pg_tri(k, k)] >= 0.0, what + ".info: a negative diagonal entry");
}
// the smallest node of a component without a fixed node, or n_nodes when every component has one
static uint32_t pg_gauge(uint32_t n_nodes, const uint8_t* fixed, const loamx_posegraph_edge* edges, uint64_t n_edges) {
  std::vector<uint32_t> parent(n_nodes);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&](uint32_t a) {
    while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
    return a;
  };
  for (uint64_t k = 0; k < n_edges; k++) {
    const uint32_t a = find(edges[k].i), b = find(edges[k].j);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);   // (the root of a component is its smallest node)
  }
  std::vector<uint8_t> has(n_nodes, 0);
  for (uint32_t n = 0; n < n_nodes; n++)
    if (fixed[n]) has[find(n)] = 1;
  for (uint32_t n = 0; n < n_nodes; n++)
    if (!has[find(n)]) return find(n);
  return n_nodes;
}
static void pg_check_config(const loamx_posegraph_config& c) {
  LX_REQUIRE(c.max_iterations <= 10000u, "max_iterations must be in [0, 10000]");
  LX_REQUIRE(c.max_cg_iterations >= 1u && c.max_cg_iterations <= 100000u, "max_cg_iterations must be in [1, 100000]");
  LX_REQUIRE(c.cg_batch >= 1u && c.cg_batch <= PG_MAX_CG_BATCH, "cg_batch must be in [1, 64]");
  LX_REQUIRE(c.initial_nodes >= 1u && c.initial_nodes <= (1u << 26), "initial_nodes must be in [1, 2^26]");
  LX_REQUIRE(c.initial_edges >= 1u && c.initial_edges <= (1u << 26), "initial_edges must be in [1, 2^26]");
  LX_REQUIRE(c.cg_tolerance > 0.0 && c.cg_tolerance < 1.0, "cg_tolerance must be in (0, 1)");
  LX_REQUIRE(std::isfinite(c.eps_step) && c.eps_step > 0.0, "eps_step must be positive");
  LX_REQUIRE(std::isfinite(c.eps_cost) && c.eps_cost >= 0.0, "eps_cost must be >= 0");
  LX_REQUIRE(std::isfinite(c.lambda_init) && c.lambda_init >= 0.0, "lambda_init must be >= 0");
  LX_REQUIRE(std::isfinite(c.huber_delta) && c.huber_delta >= 0.0, "huber_delta must be >= 0");
  LX_REQUIRE(c.device >= 0, "device must be >= 0");
}

// ---- the handle ---------------------------------------------------------------------------------------------------------------------
// device arrays sized by a capacity; alloc() gets all or none
struct PgBlock {
  std::vector<void*> ptrs;
  ~PgBlock() { release(); }
  void release() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
  template <class T> bool get(T*& out, size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
    ptrs.push_back(p);
    out = (T*)p;
    return true;
  }
};
struct PgNodeArrays {
  PgBlock mem;
  double *pose = nullptr, *backup = nullptr, *grad = nullptr, *D = nullptr, *Minv = nullptr, *x = nullptr, *r = nullptr, *z = nullptr, *p = nullptr,
         *Ap = nullptr, *partials = nullptr;
  uint32_t *fixed = nullptr, *row = nullptr;
  bool alloc(size_t cap) {
    const size_t c = cap;
    return mem.get(pose, 12 * c) && mem.get(backup, 12 * c) && mem.get(grad, 6 * c) && mem.get(D, 36 * c) && mem.get(Minv, 36 * c) &&
           mem.get(x, 6 * c) && mem.get(r, 6 * c) && mem.get(z, 6 * c) && mem.get(p, 6 * c) && mem.get(Ap, 6 * c) &&
           mem.get(partials, (6 * c + 255) / 256 + 1) && mem.get(fixed, c) && mem.get(row, c + 1);
  }
};
struct PgEdgeArrays {
  PgBlock mem;
  uint32_t *ij = nullptr, *flags = nullptr, *ents = nullptr;
  double *z = nullptr, *info = nullptr, *H = nullptr, *gE = nullptr, *chi2 = nullptr, *rho = nullptr, *partials = nullptr;
  bool alloc(size_t cap) {
    const size_t c = cap;
    return mem.get(ij, 2 * c) && mem.get(flags, c) && mem.get(ents, 2 * c) && mem.get(z, 12 * c) && mem.get(info, 21 * c) && mem.get(H, 108 * c) &&
           mem.get(gE, 12 * c) && mem.get(chi2, c) && mem.get(rho, c) && mem.get(partials, (c + 255) / 256 + 1);
  }
};

class PoseGraph {
 public:
  explicit PoseGraph(const loamx_posegraph_config& c) : cfg(c) {
    select_device(cfg.device);
    LX_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    LX_HIP(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
    nodes_.reset(new PgNodeArrays);
    edges_dev_.reset(new PgEdgeArrays);
    if (!nodes_->alloc(cfg.initial_nodes) || !edges_dev_->alloc(cfg.initial_edges)) throw Error(LOAMX_E_CAPACITY, "pose graph: no device memory for the initial room");
    node_cap_ = cfg.initial_nodes;
    edge_cap_ = cfg.initial_edges;
    LX_HIP(hipMalloc((void**)&S_, sizeof(PgScalars)));
    LX_HIP(hipMemset(S_, 0, sizeof(PgScalars)));
    landing_.reserve(1);
  }
  ~PoseGraph() {
    (void)hipSetDevice(cfg.device);
    (void)hipStreamSynchronize(st_);
    nodes_.reset();
    edges_dev_.reset();
    (void)hipFree(S_);
    (void)hipEventDestroy(ev_);
    (void)hipStreamDestroy(st_);
    (void)hipGetLastError();
  }
  loamx_posegraph_config cfg;
  uint64_t stats[4] = {0, 0, 0, 0};   // launches, looks, CG iterations, linearisations

  uint32_t n_nodes() const { return (uint32_t)fixed_.size(); }
  uint64_t n_edges() const { return edges_.size(); }

  void reset() {
    LX_HIP(hipSetDevice(cfg.device));
    LX_HIP(hipStreamSynchronize(st_));
    fixed_.clear();
    edges_.clear();
    uploaded_ = 0;
    table_dirty_ = fixed_dirty_ = true;
  }

  int add_nodes(const double* poses, uint32_t n, uint32_t* first) {
    LX_REQUIRE((uint64_t)n_nodes() + n <= (1u << 30), "n: more nodes than the graph can index");
    for (uint32_t k = 0; k < n; k++) pg_check_pose(poses + 12 * (size_t)k, "poses[" + std::to_string(k) + "]");
    LX_HIP(hipSetDevice(cfg.device));
    const size_t have = fixed_.size(), want = have + n;
    if (want > node_cap_) {
      size_t cap = node_cap_;
      while (cap < want) cap *= 2;
      std::unique_ptr<PgNodeArrays> grown(new PgNodeArrays);
      if (!grown->alloc(cap)) throw Error(LOAMX_E_CAPACITY, "pose graph: no device memory for more nodes");
      if (have) LX_HIP(hipMemcpyAsync(grown->pose, nodes_->pose, sizeof(double) * 12 * have, hipMemcpyDeviceToDevice, st_));
      LX_HIP(hipStreamSynchronize(st_));
      nodes_ = std::move(grown);
      node_cap_ = cap;
    }
    if (n) {
      LX_HIP(hipMemcpyAsync(nodes_->pose + 12 * have, poses, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st_));
      LX_HIP(hipStreamSynchronize(st_));
    }
    fixed_.resize(want, 0);
    table_dirty_ = fixed_dirty_ = true;
    if (first) *first = (uint32_t)have;
    return LOAMX_OK;
  }

  void set_fixed(uint32_t id, int fixed) {
    LX_REQUIRE(id < n_nodes(), "id: no such node");
    fixed_[id] = fixed ? 1 : 0;
    fixed_dirty_ = true;
  }

  void set_poses(uint32_t first, uint32_t n, const double* poses) {
    LX_REQUIRE((uint64_t)first + n <= n_nodes(), "first + n: beyond the nodes");
    for (uint32_t k = 0; k < n; k++) pg_check_pose(poses + 12 * (size_t)k, "poses[" + std::to_string(k) + "]");
    if (!n) return;
    LX_HIP(hipSetDevice(cfg.device));
    LX_HIP(hipMemcpyAsync(nodes_->pose + 12 * (size_t)first, poses, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st_));
    LX_HIP(hipStreamSynchronize(st_));
  }

  void get_poses(uint32_t first, uint32_t n, double* poses) {
    LX_REQUIRE((uint64_t)first + n <= n_nodes(), "first + n: beyond the nodes");
    if (!n) return;
    LX_HIP(hipSetDevice(cfg.device));
    LX_HIP(hipMemcpyAsync(poses, nodes_->pose + 12 * (size_t)first, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, st_));
    LX_HIP(hipStreamSynchronize(st_));
  }

  int add_edges(const loamx_posegraph_edge* e, uint64_t n) {
    LX_REQUIRE(edges_.size() + n <= (1u << 30), "n: more edges than the graph can index");
    for (uint64_t k = 0; k < n; k++) pg_check_edge(e[k], n_nodes(), "edges[" + std::to_string(k) + "]");
    LX_HIP(hipSetDevice(cfg.device));
    const size_t want = edges_.size() + n;
    if (want > edge_cap_) {   // (the edges go up again from the host's copy: nothing to carry over)
      size_t cap = edge_cap_;
      while (cap < want) cap *= 2;
      std::unique_ptr<PgEdgeArrays> grown(new PgEdgeArrays);
      if (!grown->alloc(cap)) throw Error(LOAMX_E_CAPACITY, "pose graph: no device memory for more edges");
      LX_HIP(hipStreamSynchronize(st_));
      edges_dev_ = std::move(grown);
      edge_cap_ = cap;
      uploaded_ = 0;
    }
    edges_.insert(edges_.end(), e, e + n);
    if (n) table_dirty_ = true;
    return LOAMX_OK;
  }

  void linearise(double* chi2, double* grad, double* diag, double* cost) {
    prepare();
    enqueue_linearise();
    const PgScalars s = look();
    const size_t N = n_nodes(), E = edges_.size();
    if (chi2 && E) LX_HIP(hipMemcpyAsync(chi2, edges_dev_->chi2, sizeof(double) * E, hipMemcpyDeviceToHost, st_));
    if (grad && N) LX_HIP(hipMemcpyAsync(grad, nodes_->grad, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, st_));
    if (diag && N) LX_HIP(hipMemcpyAsync(diag, nodes_->D, sizeof(double) * 36 * N, hipMemcpyDeviceToHost, st_));
    LX_HIP(hipStreamSynchronize(st_));
    if (cost) *cost = s.cost;
  }

  void optimize(loamx_posegraph_result* res) {
    prepare();
    struct Ops {
      PoseGraph& g;
      uint32_t cg_iterations = 0, bad_pivots = 0;
      double lambda = 0.0;
      void linearise() { g.enqueue_linearise(); }
      double cost() { return g.look().cost; }
      void cg_begin() { g.enqueue_cg_begin(lambda); }
      void cg_iterate() { g.enqueue_cg_iteration(lambda); }
      PgCgLook cg_look() {
        const PgScalars s = g.look();
        bad_pivots = s.bad_pivots;
        return PgCgLook{s.done, s.iterations};
      }
      void solve(double l) {
        lambda = l;
        const PgCgOutcome o = pg_cg_schedule(*this, PgCgPlan{g.cfg.cg_batch, g.cfg.max_cg_iterations});
        cg_iterations += o.iterations;
        g.stats[2] += o.iterations;
      }
      PgTrial apply() {
        g.enqueue_apply();
        const PgScalars s = g.look();
        return PgTrial{s.trial, s.max_delta};
      }
      void restore() { g.enqueue_restore(); }
    } ops{*this};
    const uint64_t looks0 = stats[1];
    const PgLmOutcome o = pg_lm_schedule(ops, PgLmRule{cfg.max_iterations, cfg.eps_step, cfg.eps_cost, cfg.lambda_init});
    LX_HIP(hipStreamSynchronize(st_));   // (a restore may still be in flight)
    if (res) {
      res->iterations = o.iterations;
      res->accepted = o.accepted;
      res->cg_iterations = ops.cg_iterations;
      res->looks = (uint32_t)(stats[1] - looks0);
      res->status = o.status;
      res->cost_initial = o.cost_initial;
      res->cost_final = o.cost_final;
      res->last_step = o.last_step;
      res->lambda_final = o.lambda_final;
    }
    last_bad_pivots = ops.bad_pivots;
  }
  uint32_t last_bad_pivots = 0;   // of the last solve of the last optimize

 private:
  hipStream_t st_ = nullptr;
  hipEvent_t ev_ = nullptr;
  std::unique_ptr<PgNodeArrays> nodes_;
  std::unique_ptr<PgEdgeArrays> edges_dev_;
  size_t node_cap_ = 0, edge_cap_ = 0;
  std::vector<uint8_t> fixed_;                   // per node
  std::vector<loamx_posegraph_edge> edges_;      // the host's copy: the gauge check, the table, and the upload after a growth
  size_t uploaded_ = 0;                          // edges whose records are in device memory
  bool table_dirty_ = true, fixed_dirty_ = true;
  PgScalars* S_ = nullptr;
  PinLanding<PgScalars> landing_;

  static uint32_t blocks(uint64_t n) { return (uint32_t)std::max<uint64_t>((n + 255) / 256, 1); }   // (never an empty grid)
  void launched() { stats[0]++; }

  // gauge check, then whatever changed on the host goes up: new edges, the fixed flags, the node -> incident-edge table
  void prepare() {
    const uint32_t N = n_nodes();
    const uint32_t bad = pg_gauge(N, fixed_.data(), edges_.data(), edges_.size());
    LX_REQUIRE(bad == N, "gauge: the component of node " + std::to_string(bad) + " has no fixed node");
    LX_HIP(hipSetDevice(cfg.device));
    const size_t E = edges_.size();
    std::vector<uint32_t> ij, fl, row, ents, fx;
    std::vector<double> z, info;
    if (uploaded_ < E) {
      const size_t m = E - uploaded_;
      ij.resize(2 * m); fl.resize(m); z.resize(12 * m); info.resize(21 * m);
      for (size_t k = 0; k < m; k++) {
        const loamx_posegraph_edge& e = edges_[uploaded_ + k];
        ij[2 * k] = e.i; ij[2 * k + 1] = e.j; fl[k] = e.flags;
        memcpy(&z[12 * k], e.z, sizeof(e.z));
        memcpy(&info[21 * k], e.info, sizeof(e.info));
      }
      LX_HIP(hipMemcpyAsync(edges_dev_->ij + 2 * uploaded_, ij.data(), sizeof(uint32_t) * 2 * m, hipMemcpyHostToDevice, st_));
      LX_HIP(hipMemcpyAsync(edges_dev_->flags + uploaded_, fl.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, st_));
      LX_HIP(hipMemcpyAsync(edges_dev_->z + 12 * uploaded_, z.data(), sizeof(double) * 12 * m, hipMemcpyHostToDevice, st_));
      LX_HIP(hipMemcpyAsync(edges_dev_->info + 21 * uploaded_, info.data(), sizeof(double) * 21 * m, hipMemcpyHostToDevice, st_));
    }
    if (fixed_dirty_ && N) {
      fx.assign(fixed_.begin(), fixed_.end());
      LX_HIP(hipMemcpyAsync(nodes_->fixed, fx.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice, st_));
    }
    if (table_dirty_) {   // rows in ascending edge id: the edges are walked in that order
      row.assign((size_t)N + 1, 0u);
      for (const auto& e : edges_) { row[e.i + 1]++; row[e.j + 1]++; }
      for (uint32_t n = 0; n < N; n++) row[n + 1] += row[n];
      ents.resize(2 * E);
      std::vector<uint32_t> at(row.begin(), row.end() - 1);
      for (size_t k = 0; k < E; k++) {
        ents[at[edges_[k].i]++] = (uint32_t)(k << 1);
        ents[at[edges_[k].j]++] = (uint32_t)(k << 1) | 1u;
      }
      LX_HIP(hipMemcpyAsync(nodes_->row, row.data(), sizeof(uint32_t) * row.size(), hipMemcpyHostToDevice, st_));
      if (E) LX_HIP(hipMemcpyAsync(edges_dev_->ents, ents.data(), sizeof(uint32_t) * 2 * E, hipMemcpyHostToDevice, st_));
    }
    LX_HIP(hipStreamSynchronize(st_));   // (the staging vectors above go out of scope)
    uploaded_ = E;
    table_dirty_ = fixed_dirty_ = false;
  }

  PgScalars look() {
    const PgScalars* h = landing_.fetch(S_, 1, st_);
    LX_HIP(hipEventRecord(ev_, st_));
    wait_event(ev_);
    stats[1]++;
    return *h;
  }

  void final_(const double* partials, uint32_t n, int mode) {
    hipLaunchKernelGGL(k_pg_final, dim3(1), dim3(256), 0, st_, partials, n, S_, mode);
    launched();
  }
  void enqueue_cost(int mode) {   // rho per edge is in place
    const uint32_t E = (uint32_t)edges_.size();
    hipLaunchKernelGGL(k_pg_sum, dim3(blocks(E)), dim3(256), 0, st_, edges_dev_->rho, E, edges_dev_->partials);
    launched();
    final_(edges_dev_->partials, blocks(E), mode);
  }
  void enqueue_linearise() {
    const uint32_t N = n_nodes(), E = (uint32_t)edges_.size();
    PgEdgeArrays& d = *edges_dev_;
    if (E) {
      hipLaunchKernelGGL(k_pg_linearise, dim3((E + PG_LIN_EDGES - 1) / PG_LIN_EDGES), dim3(PG_LIN_THREADS), 0, st_, nodes_->pose, d.ij, d.flags, d.z,
                         d.info, E, cfg.huber_delta, d.H, d.gE, d.chi2, d.rho);
      launched();
    }
    if (N) {
      hipLaunchKernelGGL(k_pg_gather, dim3(blocks((uint64_t)N * PG_GATHER_LANES)), dim3(256), 0, st_, nodes_->row, d.ents, nodes_->fixed, d.H, d.gE, N,
                         nodes_->D, nodes_->grad);
      launched();
    }
    enqueue_cost(PG_F_COST);
    LX_HIP(hipGetLastError());
    stats[3]++;
  }
  void enqueue_cg_begin(double lambda) {
    const uint32_t N = n_nodes();
    hipLaunchKernelGGL(k_pg_begin, dim3(1), dim3(1), 0, st_, S_, cfg.cg_tolerance * cfg.cg_tolerance);
    hipLaunchKernelGGL(k_pg_precond, dim3(blocks(N)), dim3(256), 0, st_, nodes_->D, nodes_->fixed, N, lambda, nodes_->Minv, S_);
    hipLaunchKernelGGL(k_pg_cg_init, dim3(blocks(N)), dim3(256), 0, st_, nodes_->grad, nodes_->Minv, N, nodes_->x, nodes_->r, nodes_->z, nodes_->p,
                       nodes_->partials);
    stats[0] += 3;
    final_(nodes_->partials, blocks(N), PG_F_RZ0);
    LX_HIP(hipGetLastError());
  }
  void enqueue_cg_iteration(double lambda) {
    const uint32_t N = n_nodes();
    PgNodeArrays& a = *nodes_;
    hipLaunchKernelGGL(k_pg_cg_ap, dim3(blocks(6ull * N)), dim3(256), 0, st_, a.row, edges_dev_->ents, edges_dev_->ij, a.fixed, edges_dev_->H, a.D, a.p, N,
                       lambda, a.Ap, a.partials, S_);
    launched();
    final_(a.partials, blocks(6ull * N), PG_F_PAP);
    hipLaunchKernelGGL(k_pg_cg_update, dim3(blocks(N)), dim3(256), 0, st_, a.Minv, a.p, a.Ap, N, a.x, a.r, a.z, a.partials, S_);
    launched();
    final_(a.partials, blocks(N), PG_F_RZ);
    hipLaunchKernelGGL(k_pg_cg_p, dim3(blocks(6ull * N)), dim3(256), 0, st_, a.z, 6ull * N, a.p, S_);
    launched();
    LX_HIP(hipGetLastError());
  }
  void enqueue_apply() {
    const uint32_t N = n_nodes(), E = (uint32_t)edges_.size();
    PgEdgeArrays& d = *edges_dev_;
    hipLaunchKernelGGL(k_pg_apply, dim3(blocks(N)), dim3(256), 0, st_, nodes_->x, nodes_->fixed, N, nodes_->pose, nodes_->backup, nodes_->partials);
    launched();
    final_(nodes_->partials, blocks(N), PG_F_MAXD);
    if (E) {
      hipLaunchKernelGGL(k_pg_cost, dim3(blocks(E)), dim3(256), 0, st_, nodes_->pose, d.ij, d.flags, d.z, d.info, E, cfg.huber_delta, d.rho);
      launched();
    }
    enqueue_cost(PG_F_TRIAL);
    LX_HIP(hipGetLastError());
  }
  void enqueue_restore() {
    const uint64_t n = 12ull * n_nodes();
    hipLaunchKernelGGL(k_pg_copy, dim3(blocks(n)), dim3(256), 0, st_, nodes_->backup, n, nodes_->pose);
    launched();
    LX_HIP(hipGetLastError());
  }
};

}  // namespace loamx

using namespace loamx;

struct loamx_posegraph {
  PoseGraph g;
  explicit loamx_posegraph(const loamx_posegraph_config& c) : g(c) {}
};

extern "C" {

void loamx_posegraph_default_config(loamx_posegraph_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_iterations = 50;
  cfg->max_cg_iterations = 500;
  // measured (profiles/posegraph_kernels.md): a look costs ~14 us; 16 is within 3 % of 64 where every solve runs to its cap, and a solve
  // that stops early leaves at most 15 idle iterations (75 launches that return at once) behind it instead of 63
  cfg->cg_batch = 16;
  cfg->initial_nodes = 1024;
  cfg->initial_edges = 2048;
  cfg->cg_tolerance = 1e-8;
  cfg->eps_step = 1e-9;
  cfg->eps_cost = 1e-12;
  cfg->lambda_init = 1e-6;
  cfg->huber_delta = 0.0;
  cfg->device = 0;
}
int loamx_posegraph_check(const loamx_posegraph_config* cfg) {
  return guard([&]() { LX_REQUIRE(cfg, "NULL cfg"); pg_check_config(*cfg); return LOAMX_OK; });
}
int loamx_posegraph_between(const double Ti[12], const double Tj[12], double z[12]) {
  return guard([&]() {
    LX_REQUIRE(Ti && Tj && z, "NULL argument");
    pg_check_pose(Ti, "Ti");
    pg_check_pose(Tj, "Tj");
    pg_between(Ti, Tj, z);
    return LOAMX_OK;
  });
}
int loamx_posegraph_residual(const double Ti[12], const double Tj[12], const double z[12], double r[6]) {
  return guard([&]() {
    LX_REQUIRE(Ti && Tj && z && r, "NULL argument");
    pg_check_pose(Ti, "Ti");
    pg_check_pose(Tj, "Tj");
    pg_check_pose(z, "z");
    PgResidual s;
    pg_residual(Ti, Tj, z, s);
    memcpy(r, s.r, sizeof(s.r));
    return LOAMX_OK;
  });
}
int loamx_posegraph_info_diagonal(double sigma_t, double sigma_r, double info[21]) {
  return guard([&]() {
    LX_REQUIRE(info, "NULL info");
    LX_REQUIRE(std::isfinite(sigma_t) && sigma_t > 0.0, "sigma_t must be positive");
    LX_REQUIRE(std::isfinite(sigma_r) && sigma_r > 0.0, "sigma_r must be positive");
    for (int k = 0; k < 21; k++) info[k] = 0.0;
    for (int k = 0; k < 6; k++) info[pg_tri(k, k)] = k < 3 ? 1.0 / (sigma_t * sigma_t) : 1.0 / (sigma_r * sigma_r);
    return LOAMX_OK;
  });
}
int loamx_posegraph_check_gauge(uint32_t n_nodes, const uint8_t* fixed, const loamx_posegraph_edge* edges, uint64_t n_edges, uint32_t* bad_node) {
  return guard([&]() {
    LX_REQUIRE(n_nodes == 0 || fixed, "NULL fixed");
    LX_REQUIRE(n_edges == 0 || edges, "NULL edges");
    for (uint64_t k = 0; k < n_edges; k++) {
      LX_REQUIRE(edges[k].i < n_nodes && edges[k].j < n_nodes, "edges[" + std::to_string(k) + "]: no such node");
      LX_REQUIRE(edges[k].i != edges[k].j, "edges[" + std::to_string(k) + "]: i == j");
    }
    const uint32_t bad = pg_gauge(n_nodes, fixed, edges, n_edges);
    if (bad == n_nodes) return LOAMX_OK;
    if (bad_node) *bad_node = bad;
    throw Error(LOAMX_E_INVALID, "gauge: the component of node " + std::to_string(bad) + " has no fixed node");
  });
}
int loamx_posegraph_corrections(const double* before, const double* after, uint32_t n, double* out) {
  return guard([&]() {
    LX_REQUIRE(n == 0 || (before && after && out), "NULL argument");
    for (uint32_t k = 0; k < n; k++) {
      pg_check_pose(before + 12 * (size_t)k, "before[" + std::to_string(k) + "]");
      pg_check_pose(after + 12 * (size_t)k, "after[" + std::to_string(k) + "]");
    }
    for (uint32_t k = 0; k < n; k++) {   // C = after * before^-1: R_c = R_a R_b^T, t_c = t_a - R_c t_b
      const double* B = before + 12 * (size_t)k;
      const double* A = after + 12 * (size_t)k;
      double Ra[9], Rb[9], Rc[9], t[3];
      pg_rot(A, Ra);
      pg_rot(B, Rb);
      pg_mmt(Ra, Rb, Rc);
      const double tb[3] = {B[3], B[7], B[11]};
      pg_mv(Rc, tb, t);
      double* o = out + 12 * (size_t)k;
      for (int i = 0; i < 3; i++) {
        o[4 * i] = Rc[3 * i]; o[4 * i + 1] = Rc[3 * i + 1]; o[4 * i + 2] = Rc[3 * i + 2];
        o[4 * i + 3] = A[4 * i + 3] - t[i];
      }
    }
    return LOAMX_OK;
  });
}

loamx_posegraph* loamx_posegraph_create(const loamx_posegraph_config* cfg) {
  loamx_posegraph* h = nullptr;
  guard([&]() {
    loamx_posegraph_config c;
    if (cfg) c = *cfg; else loamx_posegraph_default_config(&c);
    pg_check_config(c);
    h = new loamx_posegraph(c);
    return LOAMX_OK;
  });
  return h;
}
void loamx_posegraph_destroy(loamx_posegraph* h) { delete h; }
int loamx_posegraph_reset(loamx_posegraph* h) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->g.reset(); return LOAMX_OK; });
}
int loamx_posegraph_add_nodes(loamx_posegraph* h, const double* poses, uint32_t n, uint32_t* first_id) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(poses || n == 0, "NULL poses");
    return h->g.add_nodes(poses, n, first_id);
  });
}
int loamx_posegraph_set_fixed(loamx_posegraph* h, uint32_t id, int fixed) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->g.set_fixed(id, fixed); return LOAMX_OK; });
}
int loamx_posegraph_set_poses(loamx_posegraph* h, uint32_t first, uint32_t n, const double* poses) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(poses || n == 0, "NULL poses");
    h->g.set_poses(first, n, poses);
    return LOAMX_OK;
  });
}
int loamx_posegraph_get_poses(loamx_posegraph* h, uint32_t first, uint32_t n, double* poses) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(poses || n == 0, "NULL poses");
    h->g.get_poses(first, n, poses);
    return LOAMX_OK;
  });
}
int loamx_posegraph_add_edges(loamx_posegraph* h, const loamx_posegraph_edge* edges, uint64_t n) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(edges || n == 0, "NULL edges");
    return h->g.add_edges(edges, n);
  });
}
int loamx_posegraph_size(loamx_posegraph* h, uint32_t* nodes, uint64_t* edges) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    if (nodes) *nodes = h->g.n_nodes();
    if (edges) *edges = h->g.n_edges();
    return LOAMX_OK;
  });
}
int loamx_posegraph_linearise(loamx_posegraph* h, double* chi2, double* grad, double* diag, double* cost) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->g.linearise(chi2, grad, diag, cost); return LOAMX_OK; });
}
int loamx_posegraph_optimize(loamx_posegraph* h, loamx_posegraph_result* result) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->g.optimize(result); return LOAMX_OK; });
}
int loamx_posegraph_get_stats(loamx_posegraph* h, uint64_t stats[4]) {
  return guard([&]() {
    LX_REQUIRE(h && stats, "NULL argument");
    for (int k = 0; k < 4; k++) stats[k] = h->g.stats[k];
    return LOAMX_OK;
  });
}

// test / bench hook (not in include/loamx.h): nodes whose preconditioner had a pivot that was not positive in the last solve
uint32_t loamx_posegraph_bad_pivots(loamx_posegraph* h) { return h ? h->g.last_bad_pivots : 0u; }

}  // extern "C"
