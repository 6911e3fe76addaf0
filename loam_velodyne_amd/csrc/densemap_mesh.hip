// Signed distance along the sweep rays and its triangle mesh (densemap.hpp DmTsdf; include/loamx.h, loamx_densemap_tsdf_* and
// loamx_densemap_mesh).  The field is two integer sums per cell of a dense window, W and D, fed by one kernel that walks every ray's
// band with the carve's own walk (densemap_dev.hpp); the mesh is marching tetrahedra over the lattice of cell centres, indexed, in a
// fixed order.  Integer atomics only: every word has one value whatever the schedule.
//
//   k_dm_tsdf         one thread per traced-or-not ray (the points i % ray_stride == 0 of each call): filter, walk, two atomics per
//                     visited cell inside the window.  TABLE: the calls of a window of the sweep log (a binary search over the first
//                     ray of each call, the point under its call's correction, as k_dm_rebuild); otherwise one call by value.
//   k_dm_tsdf_stats   at a download: cells with W > 0 and the largest W, a fixed number of blocks striding over the cells.
//   k_dm_mesh_mark    one thread per cell as the lower cell of a cube: the 8 corners' validity and sign, the six tetrahedra; every
//                     crossing edge of a processed tetrahedron sets its bit in the owner's byte (atomicOr on the word of four cells:
//                     idempotent); the cube's triangles are summed per block, the four stats per wave.
//   k_dm_mesh_count   one thread per cell: the set bits of its byte, summed per block (the bytes are complete only behind the launch
//                     of k_dm_mesh_mark: other blocks' cubes set bits of this block's cells).
//   the chained scan of scan.hpp over the two runs of block sums (the map's DmScan); the host reads the two totals.
//   k_dm_mesh_verts   one thread per cell: its vertex base = the block's offset + an in-block exclusive scan, kept per cell; the
//                     vertices of its set bits in ascending e.
//   k_dm_mesh_tris    one thread per cube: the cases again, the indices looked up through the owner's base and byte, written at the
//                     block's offset + an in-block exclusive scan of the cubes' triangle counts.
// No block waits for another beyond the chained scan's own bounded wait; every loop is bounded by max_steps, the six tetrahedra or
// the seven edges.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include <cstdio>

namespace loamx {

constexpr uint32_t DM_TSDF_MAX_SIDE = 1024;
constexpr uint32_t DM_TSDF_STATS_BLOCKS = 1024;
constexpr int DM_MESH_CTR = 4;   // behind the DM_TSDF_CTR words: valid cells, inside cells, tetrahedra processed, holes

// one call as the kernel reads it: where its cloud starts (TABLE: in the log), its first ray among the launch's, its correction and
// its corrected origin (densemap_history.hpp, dm_replay_call)
struct DmTsdfCall {
  uint64_t first, ray_first;
  uint32_t count, identity;
  float m[12];
  float o[3];
  uint32_t pad;
};
static_assert(sizeof(DmTsdfCall) == 88, "8-byte aligned, no padding");

struct DmTsdfArgs {
  float inv, leaf, tau, min2, max2;
  int use_max, free_space;
  uint32_t stride, max_steps;
  int x0, y0, z0;
  uint32_t nx, ny, nz;
};

template <bool TABLE>
__global__ __launch_bounds__(256) void k_dm_tsdf(const float4* __restrict__ pts, unsigned long long n_rays,
                                                 const DmTsdfCall* __restrict__ calls, uint32_t n_calls, DmTsdfCall one, DmTsdfArgs A,
                                                 uint32_t* __restrict__ W, unsigned long long* __restrict__ D,
                                                 unsigned long long* __restrict__ ctr) {
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool traced = false, filtered = false, steps = false, zero = false;
  uint32_t visited = 0u;
  if (t < n_rays) {
    float4 p;
    DmFilter F;
    F.inv = A.inv; F.min2 = A.min2; F.max2 = A.max2; F.use_max = A.use_max;
    if (TABLE) {
      // the last call whose first ray is at or before t (call 0's is 0)
      uint32_t lo = 0u, hi = n_calls;
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (calls[mid].ray_first <= t) lo = mid; else hi = mid;
      }
      const DmTsdfCall& c = calls[lo];
      p = pts[c.first + (t - c.ray_first) * A.stride];   // (< c.first + c.count: the call has ceil(count / stride) rays)
      if (!c.identity) {
        float o[3];
        dm_correct(c.m, p.x, p.y, p.z, o);
        p.x = o[0]; p.y = o[1]; p.z = o[2];
      }
      F.ox = c.o[0]; F.oy = c.o[1]; F.oz = c.o[2];
    } else {
      p = pts[t * A.stride];
      F.ox = one.o[0]; F.oy = one.o[1]; F.oz = one.o[2];
    }
    float d2;
    if (!dm_added(p, F, d2)) {
      filtered = true;
    } else {
      const float len = sqrtf(d2);
      if (len == 0.f) {
        zero = true;
      } else {
        const float dx = p.x - F.ox, dy = p.y - F.oy, dz = p.z - F.oz;
        const float ux = dx / len, uy = dy / len, uz = dz / len;
        const float back = A.free_space ? len : fminf(A.tau, len);
        DmAxis X, Y, Z;
        const bool okx = dm_axis_setup(p.x - ux * back, p.x + ux * A.tau, A.inv, X), oky = dm_axis_setup(p.y - uy * back, p.y + uy * A.tau, A.inv, Y),
                   okz = dm_axis_setup(p.z - uz * back, p.z + uz * A.tau, A.inv, Z);
        const uint32_t n_steps = X.rem + Y.rem + Z.rem;
        if (!(okx && oky && okz) || n_steps > A.max_steps) {
          steps = true;
        } else {
          traced = true;
          for (uint32_t k = 0;; k++) {
            const uint32_t rx = (uint32_t)(X.c - A.x0), ry = (uint32_t)(Y.c - A.y0), rz = (uint32_t)(Z.c - A.z0);
            if (rx < A.nx && ry < A.ny && rz < A.nz) {
              const float mx = ((float)X.c + 0.5f) * A.leaf, my = ((float)Y.c + 0.5f) * A.leaf, mz = ((float)Z.c + 0.5f) * A.leaf;
              const float sd = ((p.x - mx) * ux + (p.y - my) * uy) + (p.z - mz) * uz;
              const float r = fminf(fmaxf(sd / A.tau, -1.f), 1.f);
              const int q = (int)rintf(r * 1024.0f);
              const size_t c = ((size_t)rz * A.ny + ry) * A.nx + rx;   // (< nx * ny * nz: the three compares above)
              atomicAdd(&W[c], 1u);
              atomicAdd(&D[c], (unsigned long long)(long long)q);
              visited++;
            }
            if (k == n_steps) break;
            dm_walk_step(X, Y, Z);   // (k < n_steps: some axis has cells left)
          }
        }
      }
    }
  }
  dm_wave_count(&ctr[0], traced);
  dm_wave_count(&ctr[2], filtered);
  dm_wave_count(&ctr[3], steps);
  dm_wave_count(&ctr[4], zero);
  dm_wave_sum(&ctr[5], visited);   // (a wave's sum: 64 rays of at most 65,537 cells)
}

// ctr[6] += cells with W > 0, ctr[7] = max(ctr[7], the largest W): both cleared by the caller
__global__ __launch_bounds__(256) void k_dm_tsdf_stats(const uint32_t* __restrict__ W, uint32_t cells, unsigned long long* __restrict__ ctr) {
  uint32_t n = 0u, mx = 0u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x) {   // (cells <= 2^26, the stride <= 2^18)
    const uint32_t w = W[i];
    n += w ? 1u : 0u;
    mx = w > mx ? w : mx;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    n += (uint32_t)__shfl_xor((int)n, o, 64);
    const uint32_t v = (uint32_t)__shfl_xor((int)mx, o, 64);
    mx = v > mx ? v : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    if (n) atomicAdd(&ctr[6], (unsigned long long)n);
    if (mx) atomicMax(&ctr[7], (unsigned long long)mx);
  }
}

// ---- the mesh

struct DmMeshArgs {
  uint32_t nx, ny, nz, cells, min_weight;
  int x0, y0, z0, axes;
  double leaf;
};

// this thread's v summed over the block's 256 threads: its exclusive prefix, and the block's total.  Every thread calls, once
__device__ inline uint32_t dm_mesh_block_scan(uint32_t v, uint32_t& total) {
  __shared__ uint32_t w[4];
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) w[wid] = inc;
  __syncthreads();
  uint32_t base = 0u;
  for (int k = 0; k < wid; k++) base += w[k];
  total = w[0] + w[1] + w[2] + w[3];
  return base + inc - v;
}

// the cell's record from its window-relative indices
__device__ inline uint32_t dm_mesh_rec(const DmMeshArgs& A, uint32_t rx, uint32_t ry, uint32_t rz) { return (rz * A.ny + ry) * A.nx + rx; }

// The cube whose lower cell is record c: false when c is no lower cell (beyond the cells, or on an upper face of the window).
// valid / inside: bit n = corner n = bx | by << 1 | bz << 2
__device__ inline bool dm_mesh_cube(const DmMeshArgs& A, uint32_t c, const uint32_t* __restrict__ W, const unsigned long long* __restrict__ D,
                                    uint32_t& valid, uint32_t& inside) {
  valid = inside = 0u;
  if (c >= A.cells) return false;
  const uint32_t rx = c % A.nx, ry = (c / A.nx) % A.ny, rz = c / (A.nx * A.ny);
  if (rx + 1u >= A.nx || ry + 1u >= A.ny || rz + 1u >= A.nz) return false;
#pragma unroll
  for (uint32_t n = 0; n < 8u; n++) {
    const uint32_t cc = dm_mesh_rec(A, rx + (n & 1u), ry + ((n >> 1) & 1u), rz + (n >> 2));   // (inside the window: the test above)
    if (W[cc] >= A.min_weight) {
      valid |= 1u << n;
      if ((long long)D[cc] < 0ll) inside |= 1u << n;
    }
  }
  return true;
}

// the four corners of tetrahedron t (include/loamx.h): t0 = 0, t1 = a, t2 = a | b, t3 = 7 for its axis order (a, b, c); parity f
__device__ inline void dm_mesh_tet(int t, uint32_t corner[4], int& f) {
  const uint32_t a = t < 2 ? 1u : (t < 4 ? 2u : 4u);
  const uint32_t b = (t == 0 || t == 5) ? 2u : ((t == 1 || t == 3) ? 4u : 1u);
  corner[0] = 0u; corner[1] = a; corner[2] = a | b; corner[3] = 7u;
  f = (t == 1 || t == 2 || t == 5) ? 1 : 0;
}

// The triangles of a processed tetrahedron with parity f whose inside corners are the bits of in4 (bit i: position i): 0, 1 or 2;
// tri[k][v] = lo << 2 | hi, the two positions of the edge that vertex v of triangle k lies on
__device__ inline int dm_mesh_case(uint32_t in4, int f, uint32_t tri[2][3]) {
  const int k = __popc(in4);
  if (k == 0 || k == 4) return 0;
  auto E = [](uint32_t i, uint32_t j) { return i < j ? (i << 2) | j : (j << 2) | i; };
  if (k == 1 || k == 3) {
    const uint32_t a = (uint32_t)__builtin_ctz(k == 1 ? in4 : (~in4 & 15u));
    uint32_t o[3];
    int n = 0;
    for (uint32_t i = 0; i < 4u; i++)
      if (i != a) o[n++] = i;
    const bool swap = ((f + (int)a + (k == 3 ? 1 : 0)) & 1) != 0;
    tri[0][0] = E(a, o[0]);
    tri[0][1] = E(a, swap ? o[2] : o[1]);
    tri[0][2] = E(a, swap ? o[1] : o[2]);
    return 1;
  }
  const uint32_t out4 = ~in4 & 15u;
  const uint32_t a = (uint32_t)__builtin_ctz(in4), b = 31u - (uint32_t)__builtin_clz(in4);
  const uint32_t c = (uint32_t)__builtin_ctz(out4), d = 31u - (uint32_t)__builtin_clz(out4);
  // the inversions of (a, b, c, d), a < b and c < d: the pairs (inside, outside) with inside > outside
  const int inv = (a > c) + (a > d) + (b > c) + (b > d);
  uint32_t q[4] = {E(a, c), E(a, d), E(b, d), E(b, c)};
  if ((f + inv) & 1) {
    const uint32_t q0 = q[0], q1 = q[1];
    q[0] = q[3]; q[1] = q[2]; q[2] = q1; q[3] = q0;
  }
  tri[0][0] = q[0]; tri[0][1] = q[1]; tri[0][2] = q[2];
  tri[1][0] = q[0]; tri[1][1] = q[2]; tri[1][2] = q[3];
  return 2;
}

// blk_t[block] = the triangles of the block's cubes; mctr: [0] valid cells, [1] inside cells, [2] tetrahedra processed, [3] holes
__global__ __launch_bounds__(256) void k_dm_mesh_mark(DmMeshArgs A, const uint32_t* __restrict__ W, const unsigned long long* __restrict__ D,
                                                      uint32_t* __restrict__ mask, uint32_t* __restrict__ blk_t,
                                                      unsigned long long* __restrict__ mctr) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t valid, inside, n_tri = 0u, n_tet = 0u, n_hole = 0u;
  bool cell_valid = false, cell_inside = false;
  if (c < A.cells && W[c] >= A.min_weight) {
    cell_valid = true;
    cell_inside = (long long)D[c] < 0ll;
  }
  if (dm_mesh_cube(A, c, W, D, valid, inside)) {
    const uint32_t rx = c % A.nx, ry = (c / A.nx) % A.ny, rz = c / (A.nx * A.ny);
    uint32_t bits[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // per corner as an owner: the edges that cross
#pragma unroll
    for (int t = 0; t < 6; t++) {
      uint32_t corner[4];
      int f;
      dm_mesh_tet(t, corner, f);
      uint32_t v4 = 0u, in4 = 0u;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        v4 |= ((valid >> corner[i]) & 1u) << i;
        in4 |= ((inside >> corner[i]) & 1u) << i;
      }
      if (v4 != 15u) {
        if (in4 != 0u && in4 != v4) n_hole++;   // (inside is a subset of valid)
        continue;
      }
      n_tet++;
      const int k = __popc(in4);
      n_tri += (k == 1 || k == 3) ? 1u : (k == 2 ? 2u : 0u);
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++)
          if (((in4 >> i) ^ (in4 >> j)) & 1u) bits[corner[i]] |= 1u << ((corner[j] ^ corner[i]) - 1u);
    }
#pragma unroll
    for (uint32_t n = 0; n < 8u; n++)
      if (bits[n]) {
        const uint32_t cc = dm_mesh_rec(A, rx + (n & 1u), ry + ((n >> 1) & 1u), rz + (n >> 2));
        atomicOr(&mask[cc >> 2], bits[n] << (8u * (cc & 3u)));
      }
  }
  uint32_t total;
  dm_mesh_block_scan(n_tri, total);
  if (threadIdx.x == 0) blk_t[blockIdx.x] = total;
  dm_wave_count(&mctr[0], cell_valid);
  dm_wave_count(&mctr[1], cell_inside);
  dm_wave_sum(&mctr[2], n_tet);
  dm_wave_sum(&mctr[3], n_hole);
}

__global__ __launch_bounds__(256) void k_dm_mesh_count(uint32_t cells, const unsigned char* __restrict__ mask, uint32_t* __restrict__ blk_v) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t total;
  dm_mesh_block_scan(c < cells ? (uint32_t)__popc((uint32_t)mask[c]) : 0u, total);
  if (threadIdx.x == 0) blk_v[blockIdx.x] = total;
}

// off_v: the exclusive scan of the blocks' vertex counts.  vbase[c] = the index of cell c's first vertex; verts: 3 f32 per vertex
__global__ __launch_bounds__(256) void k_dm_mesh_verts(DmMeshArgs A, const uint32_t* __restrict__ W, const unsigned long long* __restrict__ D,
                                                       const unsigned char* __restrict__ mask, const uint32_t* __restrict__ off_v,
                                                       uint32_t* __restrict__ vbase, float* __restrict__ verts) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = c < A.cells ? (uint32_t)mask[c] : 0u;
  uint32_t total;
  const uint32_t base = off_v[blockIdx.x] + dm_mesh_block_scan((uint32_t)__popc(m), total);
  if (c >= A.cells) return;
  vbase[c] = base;
  if (!m) return;
  const uint32_t rx = c % A.nx, ry = (c / A.nx) % A.ny, rz = c / (A.nx * A.ny);
  const long long da = (long long)D[c], wa = (long long)W[c];
  const int ia[3] = {A.x0 + (int)rx, A.y0 + (int)ry, A.z0 + (int)rz};
  uint32_t at = base;
  for (uint32_t e = 0; e < 7u; e++) {
    if (!((m >> e) & 1u)) continue;
    const uint32_t bit = e + 1u;   // (the far cell is inside the window: a cube that holds both set the bit)
    const uint32_t cb = dm_mesh_rec(A, rx + (bit & 1u), ry + ((bit >> 1) & 1u), rz + (bit >> 2));
    const long long db = (long long)D[cb], wb = (long long)W[cb];
    const long long N = da * wb, M = N - db * wa;   // (M != 0: the signs of D_A and D_B differ as "D < 0" has them)
    const double t = (double)N / (double)M;
    float v[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double ma = ((double)ia[a] + 0.5) * A.leaf, mb = ((double)(ia[a] + (int)((bit >> a) & 1u)) + 0.5) * A.leaf;
      v[a] = (float)(ma + t * (mb - ma));
    }
    float* o = verts + 3ull * at;
    if (A.axes == 1) { o[0] = v[2]; o[1] = v[0]; o[2] = v[1]; } else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
    at++;
  }
}

// off_t: the exclusive scan of the blocks' triangle counts.  tris: 3 indices per triangle
__global__ __launch_bounds__(256) void k_dm_mesh_tris(DmMeshArgs A, const uint32_t* __restrict__ W, const unsigned long long* __restrict__ D,
                                                      const unsigned char* __restrict__ mask, const uint32_t* __restrict__ vbase,
                                                      const uint32_t* __restrict__ off_t, uint32_t* __restrict__ tris) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t valid, inside, n_tri = 0u;
  const bool cube = dm_mesh_cube(A, c, W, D, valid, inside);
  uint32_t in4s[6], proc = 0u;
  if (cube) {
    for (int t = 0; t < 6; t++) {
      uint32_t corner[4];
      int f;
      dm_mesh_tet(t, corner, f);
      uint32_t v4 = 0u, in4 = 0u;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        v4 |= ((valid >> corner[i]) & 1u) << i;
        in4 |= ((inside >> corner[i]) & 1u) << i;
      }
      in4s[t] = in4;
      if (v4 != 15u) continue;
      proc |= 1u << t;
      const int k = __popc(in4);
      n_tri += (k == 1 || k == 3) ? 1u : (k == 2 ? 2u : 0u);
    }
  }
  uint32_t total;
  uint32_t at = off_t[blockIdx.x] + dm_mesh_block_scan(n_tri, total);
  if (!n_tri) return;
  const uint32_t rx = c % A.nx, ry = (c / A.nx) % A.ny, rz = c / (A.nx * A.ny);
  for (int t = 0; t < 6; t++) {
    if (!((proc >> t) & 1u)) continue;
    uint32_t corner[4], tri[2][3];
    int f;
    dm_mesh_tet(t, corner, f);
    const int n = dm_mesh_case(in4s[t], f, tri);
    for (int k = 0; k < n; k++) {
      uint32_t* o = tris + 3ull * at;
      for (int v = 0; v < 3; v++) {
        const uint32_t ca = corner[tri[k][v] >> 2], cb = corner[tri[k][v] & 3u];   // (ca's bits are a subset of cb's: ca owns the edge)
        const uint32_t e = (cb ^ ca) - 1u;
        const uint32_t owner = dm_mesh_rec(A, rx + (ca & 1u), ry + ((ca >> 1) & 1u), rz + (ca >> 2));
        o[v] = vbase[owner] + (uint32_t)__popc((uint32_t)mask[owner] & ((1u << e) - 1u));
      }
      at++;
    }
  }
}

void dm_tsdf_check(const loamx_densemap_tsdf_config& c) {
  LX_REQUIRE(c.x0 >= -(1 << 21) && c.x0 <= (1 << 21), "x0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.y0 >= -(1 << 21) && c.y0 <= (1 << 21), "y0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.z0 >= -(1 << 21) && c.z0 <= (1 << 21), "z0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.nx >= 2u && c.nx <= DM_TSDF_MAX_SIDE, "nx must be in [2, 1024]");
  LX_REQUIRE(c.ny >= 2u && c.ny <= DM_TSDF_MAX_SIDE, "ny must be in [2, 1024]");
  LX_REQUIRE(c.nz >= 2u && c.nz <= DM_TSDF_MAX_SIDE, "nz must be in [2, 1024]");
  LX_REQUIRE((uint64_t)c.nx * c.ny * c.nz <= (1ull << 26), "nx * ny * nz must be <= 2^26");
  LX_REQUIRE(c.trunc_leaves >= 1.f && c.trunc_leaves <= 16.f, "trunc_leaves must be in [1, 16]");   // (NaN too)
  LX_REQUIRE(c.free_space <= 1u, "free_space must be 0 or 1");
  LX_REQUIRE(c.ray_stride >= 1u, "ray_stride must be >= 1");
  LX_REQUIRE(c.max_steps >= 1u && c.max_steps <= 65536u, "max_steps must be in [1, 65536]");
  LX_REQUIRE(c.min_range >= 0.f && std::isfinite(c.min_range), "min_range must be >= 0");
  LX_REQUIRE(c.max_range >= 0.f && std::isfinite(c.max_range) && (c.max_range == 0.f || c.max_range >= c.min_range),
             "max_range must be 0 or >= min_range");
}

// the window of one axis (include/loamx.h, loamx_densemap_tsdf_window)
static void tsdf_window_axis(double leaf, float centre, float half, const char* first, const char* count, int32_t& lo_out, uint32_t& n_out) {
  const double lo = std::floor(((double)centre - (double)half) / leaf), hi = std::floor(((double)centre + (double)half) / leaf);
  LX_REQUIRE(std::fabs(lo) <= 2097152.0, std::string(first) + " of the window is outside [-2^21, 2^21]");
  LX_REQUIRE(hi - lo + 1.0 <= (double)DM_TSDF_MAX_SIDE, std::string(count) + " of the window is above 1024");
  lo_out = (int32_t)lo;
  n_out = (uint32_t)std::max(hi - lo + 1.0, 2.0);
}

static DmTsdfArgs tsdf_args(const loamx_densemap_tsdf_config& c, float leaf, float inv) {
  DmTsdfArgs A;
  A.inv = inv; A.leaf = leaf; A.tau = c.trunc_leaves * leaf;
  A.min2 = c.min_range * c.min_range; A.max2 = c.max_range * c.max_range;
  A.use_max = c.max_range > 0.f ? 1 : 0;
  A.free_space = (int)c.free_space;
  A.stride = c.ray_stride; A.max_steps = c.max_steps;
  A.x0 = c.x0; A.y0 = c.y0; A.z0 = c.z0;
  A.nx = c.nx; A.ny = c.ny; A.nz = c.nz;
  return A;
}

// include/loamx.h, loamx_densemap_tsdf_begin: the volume of a checked configuration, zero, and the counters, on own_
void DenseMap::tsdf_begin(const loamx_densemap_tsdf_config& c) {
  LX_HIP(hipSetDevice(cfg.device));
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  if (cells > tsdf_.w_.cap || cells > tsdf_.d_.cap) LX_HIP(hipStreamSynchronize(own_));   // (a buffer that grows: nothing reads the old one)
  tsdf_.valid_ = false;   // (a buffer that grows drops what it held)
  tsdf_.w_.reserve(cells);
  tsdf_.d_.reserve(cells);
  tsdf_.ctr_.reserve(DM_TSDF_CTR + DM_MESH_CTR);
  LX_HIP(hipMemsetAsync(tsdf_.w_.p, 0, sizeof(uint32_t) * cells, own_));
  LX_HIP(hipMemsetAsync(tsdf_.d_.p, 0, sizeof(unsigned long long) * cells, own_));
  LX_HIP(hipMemsetAsync(tsdf_.ctr_.p, 0, sizeof(unsigned long long) * (DM_TSDF_CTR + DM_MESH_CTR), own_));
  tsdf_.cfg_ = c;
  tsdf_.stride_skipped_ = 0;
  tsdf_.valid_ = true;
}

// include/loamx.h, loamx_densemap_tsdf_add and its from_map / from_pipeline forms: the rays of s on own_, behind the stream that
// wrote the cloud; that stream then runs behind own_, so that whatever rewrites the cloud waits for the rays.  No host wait
int DenseMap::tsdf_add(const DenseSource& s) {
  LX_REQUIRE(tsdf_.has_field(), "the handle has no signed distance field (loamx_densemap_tsdf_begin)");
  LX_REQUIRE(s.device == cfg.device, "the dense map and its source live on different devices");
  if (!s.has_cloud) return LOAMX_SKIPPED;
  if (!s.n) return LOAMX_OK;
  LX_HIP(hipSetDevice(cfg.device));
  const DmTsdfArgs A = tsdf_args(tsdf_.cfg_, cfg.leaf, inv_);
  const uint64_t rays = ((uint64_t)s.n + A.stride - 1u) / A.stride;   // (the points i % ray_stride == 0; in 64 bits: no wrap)
  dm_stream_behind(own_, s.stream);
  const float4* pts = s.points();
  DmTsdfCall one = {};
  one.count = s.n;
  one.identity = 1u;
  for (int a = 0; a < 3; a++) one.o[a] = s.origin[a];
  hipLaunchKernelGGL(k_dm_tsdf<false>, dim3((uint32_t)((rays + 255u) / 256u)), dim3(256), 0, own_, pts, (unsigned long long)rays,
                     (const DmTsdfCall*)nullptr, 0u, one, A, tsdf_.w_.p, tsdf_.d_.p, tsdf_.ctr_.p);
  LX_HIP(hipGetLastError());
  dm_stream_behind(s.stream, own_);
  tsdf_.stride_skipped_ += s.n - rays;
  return LOAMX_OK;
}

// include/loamx.h, loamx_densemap_tsdf_add_from_history: the calls of the window where they lie in the log, one launch; waits
int DenseMap::tsdf_add_history(uint64_t first_call, uint64_t n_calls, const double* corrections) {
  LX_REQUIRE(tsdf_.has_field(), "the handle has no signed distance field (loamx_densemap_tsdf_begin)");
  LX_REQUIRE(history_, "history is not enabled (loamx_densemap_enable_history)");
  LX_REQUIRE(n_calls != 0, "n_calls must be at least 1");
  LX_REQUIRE(first_call < hist_.calls.size() && n_calls <= hist_.calls.size() - first_call,
             "first_call + n_calls reaches beyond the log (loamx_densemap_history_size)");
  const DmTsdfArgs A = tsdf_args(tsdf_.cfg_, cfg.leaf, inv_);
  std::vector<DmTsdfCall> calls(n_calls);
  uint64_t rays = 0, points = 0;
  for (uint64_t k = 0; k < n_calls; k++) {
    const DmHistoryCall& h = hist_.calls[first_call + k];
    DmReplayCall r;
    LX_REQUIRE(dm_replay_call(h, corrections ? corrections + 12 * k : nullptr, r),
               "corrections: the correction of call " + std::to_string(k) + " of the window has an entry that is not finite");
    DmTsdfCall& c = calls[k];
    c.first = h.first;
    c.ray_first = rays;
    c.count = h.count;
    c.identity = r.identity;
    for (int j = 0; j < 12; j++) c.m[j] = r.m[j];
    for (int a = 0; a < 3; a++) c.o[a] = r.o[a];
    c.pad = 0u;
    rays += ((uint64_t)h.count + A.stride - 1u) / A.stride;   // (a logged call has count >= 1: every call has a ray)
    points += h.count;
  }
  LX_REQUIRE((rays + 255) / 256 < (1ull << 31), "the window holds more rays than one launch covers");
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();   // (the log's points are in place, whichever stream appended them)
  DevBuf<DmTsdfCall> d_calls;
  d_calls.reserve(n_calls);
  LX_HIP(hipMemcpyAsync(d_calls.p, calls.data(), sizeof(DmTsdfCall) * n_calls, hipMemcpyHostToDevice, own_));
  hipLaunchKernelGGL(k_dm_tsdf<true>, dim3((uint32_t)((rays + 255u) / 256u)), dim3(256), 0, own_, (const float4*)log_, (unsigned long long)rays,
                     (const DmTsdfCall*)d_calls.p, (uint32_t)n_calls, DmTsdfCall{}, A, tsdf_.w_.p, tsdf_.d_.p, tsdf_.ctr_.p);
  LX_HIP(hipGetLastError());
  LX_HIP(hipStreamSynchronize(own_));   // (d_calls goes with this frame)
  tsdf_.stride_skipped_ += points - rays;
  return LOAMX_OK;
}

void DenseMap::tsdf_download(uint32_t* out_w, int64_t* out_d, uint64_t stats[8]) {
  LX_REQUIRE(tsdf_.has_field(), "the handle has no signed distance field (loamx_densemap_tsdf_begin)");
  LX_HIP(hipSetDevice(cfg.device));
  const size_t cells = tsdf_.cells();
  LX_HIP(hipMemsetAsync(tsdf_.ctr_.p + 6, 0, sizeof(unsigned long long) * 2, own_));
  hipLaunchKernelGGL(k_dm_tsdf_stats, dim3(std::min((uint32_t)((cells + 255) / 256), DM_TSDF_STATS_BLOCKS)), dim3(256), 0, own_, tsdf_.w_.p,
                     (uint32_t)cells, tsdf_.ctr_.p);
  LX_HIP(hipGetLastError());
  unsigned long long s[DM_TSDF_CTR];
  LX_HIP(hipMemcpyAsync(s, tsdf_.ctr_.p, sizeof(s), hipMemcpyDeviceToHost, own_));
  LX_HIP(hipStreamSynchronize(own_));
  if (out_w) LX_HIP(hipMemcpy(out_w, tsdf_.w_.p, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
  if (out_d) LX_HIP(hipMemcpy(out_d, tsdf_.d_.p, sizeof(unsigned long long) * cells, hipMemcpyDeviceToHost));
  for (int k = 0; k < DM_TSDF_CTR; k++) stats[k] = s[k];
  stats[1] = tsdf_.stride_skipped_;
}

// include/loamx.h, loamx_densemap_mesh: a checked configuration; the outputs are written last
int DenseMap::mesh(const loamx_densemap_mesh_config& c, float* verts, uint64_t cap_v, uint32_t* tris, uint64_t cap_t, uint64_t* n_verts,
                   uint64_t* n_tris, uint64_t stats[6]) {
  LX_REQUIRE(tsdf_.has_field(), "the handle has no signed distance field (loamx_densemap_tsdf_begin)");
  LX_HIP(hipSetDevice(cfg.device));
  const loamx_densemap_tsdf_config& f = tsdf_.cfg_;
  const size_t cells = tsdf_.cells();
  const uint32_t nblk = (uint32_t)((cells + 255) / 256);
  const size_t mask_words = (cells + 3) / 4;
  if (mask_words > tsdf_.mask_.cap || cells > tsdf_.vbase_.cap || 2 * ((size_t)nblk + 1) > tsdf_.blk_.cap)
    LX_HIP(hipStreamSynchronize(own_));   // (a buffer that grows: nothing reads the old one)
  tsdf_.mask_.reserve(mask_words);
  tsdf_.vbase_.reserve(cells);
  tsdf_.blk_.reserve(2 * ((size_t)nblk + 1));
  DmMeshArgs A;
  A.nx = f.nx; A.ny = f.ny; A.nz = f.nz; A.cells = (uint32_t)cells; A.min_weight = c.min_weight;
  A.x0 = f.x0; A.y0 = f.y0; A.z0 = f.z0; A.axes = c.axes;
  A.leaf = (double)cfg.leaf;
  uint32_t *blk_t = tsdf_.blk_.p, *blk_v = tsdf_.blk_.p + nblk + 1;
  unsigned long long* mctr = tsdf_.ctr_.p + DM_TSDF_CTR;
  const unsigned char* mask = (const unsigned char*)tsdf_.mask_.p;
  LX_HIP(hipMemsetAsync(tsdf_.mask_.p, 0, sizeof(uint32_t) * mask_words, own_));
  LX_HIP(hipMemsetAsync(mctr, 0, sizeof(unsigned long long) * DM_MESH_CTR, own_));
  hipLaunchKernelGGL(k_dm_mesh_mark, dim3(nblk), dim3(256), 0, own_, A, tsdf_.w_.p, tsdf_.d_.p, tsdf_.mask_.p, blk_t, mctr);
  hipLaunchKernelGGL(k_dm_mesh_count, dim3(nblk), dim3(256), 0, own_, A.cells, mask, blk_v);
  scan_.run(blk_t, nblk, own_);
  scan_.run(blk_v, nblk, own_);
  LX_HIP(hipGetLastError());
  uint32_t total_t = 0, total_v = 0;
  unsigned long long m[DM_MESH_CTR];
  LX_HIP(hipMemcpyAsync(&total_t, blk_t + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, own_));
  LX_HIP(hipMemcpyAsync(&total_v, blk_v + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, own_));
  LX_HIP(hipMemcpyAsync(m, mctr, sizeof(m), hipMemcpyDeviceToHost, own_));
  LX_HIP(hipStreamSynchronize(own_));
  scan_check_errors();
  *n_verts = total_v;
  *n_tris = total_t;
  if (verts && (cap_v < total_v || cap_t < total_t)) return LOAMX_E_CAPACITY;
  if (verts && (total_v || total_t)) {
    tsdf_.verts_.reserve(3 * (size_t)total_v + 1);   // (the host has waited: nothing reads an old block)
    tsdf_.tris_.reserve(3 * (size_t)total_t + 1);
    hipLaunchKernelGGL(k_dm_mesh_verts, dim3(nblk), dim3(256), 0, own_, A, tsdf_.w_.p, tsdf_.d_.p, mask, blk_v, tsdf_.vbase_.p, tsdf_.verts_.p);
    hipLaunchKernelGGL(k_dm_mesh_tris, dim3(nblk), dim3(256), 0, own_, A, tsdf_.w_.p, tsdf_.d_.p, mask, tsdf_.vbase_.p, blk_t, tsdf_.tris_.p);
    LX_HIP(hipGetLastError());
    LX_HIP(hipStreamSynchronize(own_));
    if (total_v) LX_HIP(hipMemcpy(verts, tsdf_.verts_.p, sizeof(float) * 3 * (size_t)total_v, hipMemcpyDeviceToHost));
    if (total_t) LX_HIP(hipMemcpy(tris, tsdf_.tris_.p, sizeof(uint32_t) * 3 * (size_t)total_t, hipMemcpyDeviceToHost));
  }
  for (int k = 0; k < DM_MESH_CTR; k++) stats[k] = m[k];
  stats[4] = total_v;
  stats[5] = total_t;
  return LOAMX_OK;
}

static loamx_densemap_mesh_config checked_mesh(const loamx_densemap_mesh_config* cfg) {
  const loamx_densemap_mesh_config c = or_default(cfg, loamx_densemap_mesh_default_config);
  LX_REQUIRE(c.min_weight >= 1u, "min_weight must be >= 1");
  LX_REQUIRE(c.axes == 0 || c.axes == 1, "axes must be 0 (LOAM frame) or 1 (sensor axes)");
  return c;
}

// include/loamx.h, loamx_write_ply
static void write_ply(const char* path, const float* verts, uint64_t n_verts, const uint32_t* tris, uint64_t n_tris) {
  for (uint64_t k = 0; k < 3 * n_tris; k++) LX_REQUIRE(tris[k] < n_verts && tris[k] <= 0x7fffffffu, "tris: an index is beyond the vertices");
  FILE* fp = fopen(path, "wb");
  LX_REQUIRE(fp, std::string("cannot open ") + path + " for writing");
  bool ok = fprintf(fp,
                    "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n"
                    "element face %llu\nproperty list uchar int vertex_indices\nend_header\n",
                    (unsigned long long)n_verts, (unsigned long long)n_tris) > 0;
  if (ok && n_verts) ok = fwrite(verts, sizeof(float) * 3, n_verts, fp) == n_verts;
  std::vector<unsigned char> faces(13 * (size_t)n_tris);
  for (uint64_t k = 0; k < n_tris; k++) {
    faces[13 * k] = 3;
    memcpy(&faces[13 * k + 1], tris + 3 * k, 12);
  }
  if (ok && n_tris) ok = fwrite(faces.data(), 13, n_tris, fp) == n_tris;
  ok = (fclose(fp) == 0) && ok;
  if (!ok) throw Error(LOAMX_E_INTERNAL, std::string("writing ") + path + " failed");
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_tsdf_default_config(loamx_densemap_tsdf_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->x0 = cfg->y0 = cfg->z0 = -64;
  cfg->nx = cfg->ny = cfg->nz = 128u;
  cfg->trunc_leaves = 3.f;
  cfg->free_space = 0u;
  cfg->ray_stride = 1u;
  cfg->max_steps = 4096u;
  cfg->min_range = 0.f;
  cfg->max_range = 0.f;
}

int loamx_densemap_tsdf_check(const loamx_densemap_tsdf_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_tsdf_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_densemap_tsdf_window(float leaf, const float centre[3], const float half_extent[3], loamx_densemap_tsdf_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    LX_REQUIRE(centre, "centre is NULL");
    LX_REQUIRE(half_extent, "half_extent is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    for (int a = 0; a < 3; a++) {
      LX_REQUIRE(std::isfinite(centre[a]), "centre must be finite");
      LX_REQUIRE(half_extent[a] >= 0.f && std::isfinite(half_extent[a]), "half_extent must be >= 0");
    }
    loamx_densemap_tsdf_config c = *cfg;
    tsdf_window_axis((double)leaf, centre[0], half_extent[0], "x0", "nx", c.x0, c.nx);
    tsdf_window_axis((double)leaf, centre[1], half_extent[1], "y0", "ny", c.y0, c.ny);
    tsdf_window_axis((double)leaf, centre[2], half_extent[2], "z0", "nz", c.z0, c.nz);
    LX_REQUIRE((uint64_t)c.nx * c.ny * c.nz <= (1ull << 26), "nx * ny * nz of the window is above 2^26");
    *cfg = c;
    return LOAMX_OK;
  });
}

int loamx_densemap_tsdf_begin(loamx_densemap* h, const loamx_densemap_tsdf_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    const loamx_densemap_tsdf_config c = or_default(cfg, loamx_densemap_tsdf_default_config);
    dm_tsdf_check(c);
    h->d.tsdf_begin(c);
    return LOAMX_OK;
  });
}

int loamx_densemap_tsdf_add(loamx_densemap* h, const loamx_cloud* cloud, const float origin[3]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(cloud, "cloud is NULL");
    LX_REQUIRE(origin, "origin is NULL");
    return h->d.tsdf_add(h->d.host_source(h->d.tsdf_stage(), cloud, origin));
  });
}
int loamx_densemap_tsdf_add_from_map(loamx_densemap* h, loamx_map* m) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(m, "m is NULL");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.tsdf_add(s);
  });
}
int loamx_densemap_tsdf_add_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(p, "p is NULL");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.tsdf_add(s);
  });
}
int loamx_densemap_tsdf_add_from_history(loamx_densemap* h, uint64_t first_call, uint64_t n_calls, const double* corrections) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    return h->d.tsdf_add_history(first_call, n_calls, corrections);
  });
}

int loamx_densemap_tsdf_download(loamx_densemap* h, uint32_t* out_w, int64_t* out_d, uint64_t stats[8]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    h->d.tsdf_download(out_w, out_d, stats);
    return LOAMX_OK;
  });
}

void loamx_densemap_mesh_default_config(loamx_densemap_mesh_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->min_weight = 2u;
  cfg->axes = 0;
}

int loamx_densemap_mesh(loamx_densemap* h, const loamx_densemap_mesh_config* cfg, float* verts, uint64_t cap_v, uint32_t* tris, uint64_t cap_t,
                        uint64_t* n_verts, uint64_t* n_tris, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(n_verts, "n_verts is NULL");
    LX_REQUIRE(n_tris, "n_tris is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    LX_REQUIRE((verts != nullptr) == (tris != nullptr), "verts and tris must both be given or both be NULL");
    LX_REQUIRE(verts || (!cap_v && !cap_t), "cap_v and cap_t must be 0 when verts and tris are NULL");
    const loamx_densemap_mesh_config c = checked_mesh(cfg);
    return h->d.mesh(c, verts, cap_v, tris, cap_t, n_verts, n_tris, stats);
  });
}

int loamx_write_ply(const char* path, const float* verts, uint64_t n_verts, const uint32_t* tris, uint64_t n_tris) {
  return guard([&]() {
    LX_REQUIRE(path, "path is NULL");
    LX_REQUIRE(verts || !n_verts, "verts is NULL");
    LX_REQUIRE(tris || !n_tris, "tris is NULL");
    write_ply(path, verts, n_verts, tris, n_tris);
    return LOAMX_OK;
  });
}

int loamx_densemap_save_ply(loamx_densemap* h, const loamx_densemap_mesh_config* cfg, const char* path, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(path, "path is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    const loamx_densemap_mesh_config c = checked_mesh(cfg);
    uint64_t nv = 0, nt = 0, s[6];
    int rc = h->d.mesh(c, nullptr, 0, nullptr, 0, &nv, &nt, s);
    if (rc != LOAMX_OK) return rc;
    std::vector<float> v(3 * nv + 3);
    std::vector<uint32_t> t(3 * nt + 3);
    rc = h->d.mesh(c, v.data(), nv, t.data(), nt, &nv, &nt, s);
    if (rc != LOAMX_OK) return rc;
    write_ply(path, v.data(), nv, t.data(), nt);
    memcpy(stats, s, sizeof(s));
    return LOAMX_OK;
  });
}

}  // extern "C"
