// Distance field of the dense map (densemap.hpp DmDist, include/loamx.h loamx_densemap_dist and what goes with it): the exact squared
// Euclidean distance, in cells, from every cell of a 3-D window to the nearest occupied cell of the window, capped at d_max, and the
// cell that is nearest; then point queries against the field where it lies.  Integers only (the one f32 product is the query's
// p * inv), integer atomics only, and every word has one value whatever the schedule.
//
// Three launches behind one memset (the four stats words lie in front of the bit volume, so the one memset clears both):
//   k_dm_dist_mark   2048 blocks stride over the slots of the table, coalesced over the keys: a qualifying voxel inside the window sets
//                    the bit of its cell by atomicOr in a bit volume of one 64-bit word per 64 cells of a row (a row: the cells of one (rz, ry)
//                    along x, ceil(nx / 64) words), and is counted per wave, then per block.
//   k_dm_dist_xy     the x pass and the y pass in one: one block per tile of 32 (x) x 64 (y) cells of one z.  For the tile's rows and
//                    a halo of H = min(R, ny - 1) rows either side, the x of the nearest set bit of the row within R goes to LDS as
//                    16 bits (NONE: none; the smaller x on a tie): count-leading-zeros to the left and count-trailing-zeros to the
//                    right on the row's words, at most a few words each way, no loop over the distance.  The lanes of a wave share
//                    the words they read.  Then every cell takes the minimum of (sx - x)^2 + dy^2 over |dy| <= H, outwards from
//                    dy = 0, the lower row first: the lower row wins with <=, the upper one with <, which is "ascending y with a
//                    strict <", and the scan ends once dy^2 exceeds the best sum so far or R^2 (the terms are non-negative, so
//                    nothing later can win or tie).  Written: one word per cell, rx | ry << 10 of the winning cell of the plane, NONE.
//                    Keeping the x pass out of HBM saves three bytes per cell; its price is that the halo's rows are worked out by
//                    every tile that stages them.
//   k_dm_dist_z      one block per tile of 32 (x) x 64 (z) cells of one y.  The partial sums of the tile's planes and of a halo of
//                    min(R, nz - 1) planes, recomputed from the words of the pass before as 16 bits (they are <= R^2 <= 64516), go
//                    to LDS; the same outward scan along z; d2, near (the winner's word | rz << 20) and the three cell counts.
// Every loop is bounded by R, the halo or the row's words; no block waits for another.  LDS, dynamic: 64 bytes per staged row or
// plane, (64 + 2 * 254) * 64 = 36,608 bytes at the most.
//
// Resources on the gfx950 code object (VGPRs, static LDS bytes; no scratch, no spills, 8 waves per SIMD each): k_dm_dist_mark 16, 4;
// k_dm_dist_xy 20, 0;  k_dm_dist_z 28, 12;  k_dm_dist_query 10, 24.  Measured: CHANGELOG.md (scripts/bench_densemap_dist.py).
//
// Bytes per cell on the device: 1/8 (bits) + 4 (the y pass's word) + 2 (d2) + 4 (near) = 10 1/8: 0.68 GB at 2^26 cells.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include "pinned_copy.hpp"

namespace loamx {

constexpr int DM_DIST_TX = 32;            // cells of a tile along x
constexpr int DM_DIST_TL = 64;            // cells of a tile along the line's axis (y, then z)
constexpr uint32_t DM_DIST_MAX_R = 254;   // the largest d_max: (R + 1)^2 = 65025 fits 16 bits
constexpr uint32_t DM_DIST_MAX_SIDE = 1024;
constexpr uint32_t DM_DIST_NONE = LOAMX_DIST_NONE;
constexpr uint32_t DM_DIST_NO_X = 0xffffu;   // in LDS: no set bit within R; no partial sum within R^2
constexpr int DM_DIST_CTR = 4;               // 64-bit words in front of the bit volume: the four stats

struct DmDistArgs {
  uint32_t k, nx, ny, nz, min_points;
  int x0, y0, z0;
  uint32_t R, words;   // words: 64-bit words per row of the bit volume
  int use_rule;
  loamx_densemap_static_rule rule;
};

// floor(i / k) - first for the key field f = i + 2^20, as dm_grid_voxel: (f + (k - 1) * 2^20) / k - 2^20, the dividend unsigned and
// below 2^27 for k <= 64.  (|c| <= 2^20 and |first| <= 2^21: a cell before the window wraps to a large unsigned)
__device__ inline uint32_t dm_dist_rel(uint32_t f, uint32_t k, int first) {
  const uint32_t bias = (k - 1u) << DM_QBITS;
  return (uint32_t)((int)((f + bias) / k) - (1 << DM_QBITS) - first);
}

// the sum of v over the wave, in every lane
__device__ inline uint32_t dm_dist_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// a fixed number of blocks strides over the slots and each adds its count with one global atomic: with one atomic per wave, as
// dm_wave_count has it, the 65,536 waves over a table of 4 Mi slots queued on the one word for 0.7 ms
constexpr uint32_t DM_DIST_MARK_BLOCKS = 2048;
__global__ __launch_bounds__(256) void k_dm_dist_mark(DmDistArgs A, const unsigned long long* __restrict__ keys,
                                                      const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                      uint32_t slots, unsigned long long* __restrict__ vol) {
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  uint32_t mine = 0u;
  const uint32_t km = (1u << DM_KBITS) - 1u;
  // (slots <= 2^31 and the stride is <= 2^19: i does not wrap)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    if (key == DM_EMPTY) continue;
    const uint32_t rx = dm_dist_rel((uint32_t)key & km, A.k, A.x0), ry = dm_dist_rel((uint32_t)(key >> DM_KBITS) & km, A.k, A.y0),
                   rz = dm_dist_rel((uint32_t)(key >> (2 * DM_KBITS)) & km, A.k, A.z0);
    if (rx >= A.nx || ry >= A.ny || rz >= A.nz) continue;
    const unsigned long long n = vals[4ull * i];
    if (n < A.min_points || (A.use_rule && dm_dynamic(A.rule, n, aux[2ull * i]))) continue;
    mine++;
    atomicOr(&vol[DM_DIST_CTR + ((size_t)rz * A.ny + ry) * A.words + (rx >> 6)], 1ull << (rx & 63u));
  }
  mine = dm_dist_wave_sum(mine);
  if (mine && (threadIdx.x & 63) == 0) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&vol[0], (unsigned long long)s_n);
}

// the x of the set bit of a row that is nearest to x < nx within R, the smaller x on a tie; NO_X: none.  `row`: the row's `words`
// words; no bit at or beyond nx is ever set.  At most R / 64 + 2 words each way
__device__ inline uint32_t dm_dist_row_nearest(const unsigned long long* __restrict__ row, uint32_t x, uint32_t R, uint32_t nx) {
  uint32_t left = DM_DIST_NO_X, right = DM_DIST_NO_X;
  {
    const uint32_t first = (x >= R ? x - R : 0u) >> 6;
    uint32_t w = x >> 6;
    unsigned long long m = row[w] & (~0ull >> (63u - (x & 63u)));   // the bits at or below x
    for (;;) {
      if (m) { left = w * 64u + 63u - (uint32_t)__builtin_clzll(m); break; }
      if (w == first) break;
      m = row[--w];
    }
    if (left != DM_DIST_NO_X && x - left > R) left = DM_DIST_NO_X;
  }
  {
    const uint32_t far = x + R < nx - 1u ? x + R : nx - 1u, last = far >> 6;
    uint32_t w = x >> 6;
    unsigned long long m = row[w] & (~0ull << (x & 63u));   // the bits at or above x
    for (;;) {
      if (m) { right = w * 64u + (uint32_t)__builtin_ctzll(m); break; }
      if (w == last) break;
      m = row[++w];
    }
    if (right != DM_DIST_NO_X && right - x > R) right = DM_DIST_NO_X;
  }
  if (left == DM_DIST_NO_X) return right;
  if (right == DM_DIST_NO_X) return left;
  return x - left <= right - x ? left : right;
}

// The minimum along a line that both passes share.  term(j): the partial sum at the line's staged entry j (NO_X: none), the cell at
// entry c, entries c - H .. c + H staged.  Returns the winning offset d in -H .. H and its sum in best, or false.  Outwards, the lower
// side first: the lower side wins a tie, which gives the smallest coordinate among equal sums
template <class F> __device__ inline bool dm_dist_line_min(F&& term, int H, uint32_t R2, uint32_t& best, int& off) {
  best = 0xffffffffu;
  off = 0;
  for (int d = 0; d <= H; d++) {
    const uint32_t dd = (uint32_t)(d * d);
    if (dd > R2 || dd > best) break;
    const uint32_t lo = term(-d);
    if (lo != DM_DIST_NO_X && lo + dd <= R2 && lo + dd <= best) { best = lo + dd; off = -d; }
    if (d) {
      const uint32_t hi = term(d);
      if (hi != DM_DIST_NO_X && hi + dd <= R2 && hi + dd < best) { best = hi + dd; off = d; }
    }
  }
  return best != 0xffffffffu;
}

// grid: tiles along x, tiles along y, nz.  LDS: (TL + 2 H) rows of TX entries of 16 bits
__global__ __launch_bounds__(256) void k_dm_dist_xy(DmDistArgs A, int H, const unsigned long long* __restrict__ vol, uint32_t* __restrict__ yx) {
  extern __shared__ unsigned short s_sx[];
  const int bx = (int)blockIdx.x * DM_DIST_TX, by = (int)blockIdx.y * DM_DIST_TL;
  const uint32_t z = blockIdx.z;
  const int rows = DM_DIST_TL + 2 * H;
  for (int e = (int)threadIdx.x; e < rows * DM_DIST_TX; e += 256) {
    const int x = bx + e % DM_DIST_TX, y = by - H + e / DM_DIST_TX;
    uint32_t sx = DM_DIST_NO_X;
    if (x < (int)A.nx && y >= 0 && y < (int)A.ny)
      sx = dm_dist_row_nearest(vol + DM_DIST_CTR + ((size_t)z * A.ny + (uint32_t)y) * A.words, (uint32_t)x, A.R, A.nx);
    s_sx[e] = (unsigned short)sx;
  }
  __syncthreads();
  const uint32_t R2 = A.R * A.R;
  for (int e = (int)threadIdx.x; e < DM_DIST_TL * DM_DIST_TX; e += 256) {
    const int xl = e % DM_DIST_TX, yl = e / DM_DIST_TX;
    const uint32_t x = (uint32_t)(bx + xl), y = (uint32_t)(by + yl);
    if (x >= A.nx || y >= A.ny) continue;
    const unsigned short* line = s_sx + (yl + H) * DM_DIST_TX + xl;   // (line[-H * TX .. H * TX] lies inside the staged rows)
    uint32_t best;
    int off;
    const bool found = dm_dist_line_min(
        [&](int d) {
          const uint32_t sx = line[d * DM_DIST_TX];
          if (sx == DM_DIST_NO_X) return DM_DIST_NO_X;
          const uint32_t g = sx > x ? sx - x : x - sx;   // (<= R <= 254)
          return g * g;
        },
        H, R2, best, off);
    yx[((size_t)z * A.ny + y) * A.nx + x] = found ? (uint32_t)line[off * DM_DIST_TX] | ((uint32_t)((int)y + off) << 10) : DM_DIST_NONE;
  }
}

// grid: tiles along x, tiles along z, ny.  LDS: (TL + 2 H) planes of TX entries of 16 bits.  ctr: [1] occupied cells, [2] cells with
// d2 <= R^2, [3] the largest such d2
__global__ __launch_bounds__(256) void k_dm_dist_z(DmDistArgs A, int H, const uint32_t* __restrict__ yx, unsigned short* __restrict__ d2,
                                                   uint32_t* __restrict__ near, unsigned long long* __restrict__ ctr) {
  extern __shared__ unsigned short s_g[];
  __shared__ uint32_t s_c[3];   // of the block: occupied, within, the largest d2
  if (threadIdx.x < 3) s_c[threadIdx.x] = 0u;
  const int bx = (int)blockIdx.x * DM_DIST_TX, bz = (int)blockIdx.y * DM_DIST_TL;
  const uint32_t y = blockIdx.z;
  const int planes = DM_DIST_TL + 2 * H;
  for (int e = (int)threadIdx.x; e < planes * DM_DIST_TX; e += 256) {
    const int x = bx + e % DM_DIST_TX, z = bz - H + e / DM_DIST_TX;
    uint32_t g = DM_DIST_NO_X;
    if (x < (int)A.nx && z >= 0 && z < (int)A.nz) {
      const uint32_t w = yx[((size_t)(uint32_t)z * A.ny + y) * A.nx + (uint32_t)x];
      if (w != DM_DIST_NONE) {
        const int dx = (int)(w & 1023u) - x, dy = (int)(w >> 10) - (int)y;
        g = (uint32_t)(dx * dx + dy * dy);   // (<= R^2: the pass before kept nothing larger)
      }
    }
    s_g[e] = (unsigned short)g;
  }
  __syncthreads();
  const uint32_t R2 = A.R * A.R, cap = (A.R + 1u) * (A.R + 1u);
  uint32_t n_occ = 0u, n_in = 0u, d_max = 0u;
  for (int e = (int)threadIdx.x; e < DM_DIST_TL * DM_DIST_TX; e += 256) {
    const int xl = e % DM_DIST_TX, zl = e / DM_DIST_TX;
    const uint32_t x = (uint32_t)(bx + xl), z = (uint32_t)(bz + zl);
    if (x >= A.nx || z >= A.nz) continue;
    const unsigned short* line = s_g + (zl + H) * DM_DIST_TX + xl;
    uint32_t best;
    int off;
    const bool found = dm_dist_line_min([&](int d) { return (uint32_t)line[d * DM_DIST_TX]; }, H, R2, best, off);
    const size_t c = ((size_t)z * A.ny + y) * A.nx + x;
    uint32_t nr = DM_DIST_NONE;
    if (found) {
      const uint32_t sz = (uint32_t)((int)z + off);   // (inside the window: only its planes hold a sum)
      nr = yx[((size_t)sz * A.ny + y) * A.nx + x] | (sz << 20);
      n_in++;
      n_occ += best == 0u ? 1u : 0u;
      d_max = best > d_max ? best : d_max;
    }
    d2[c] = (unsigned short)(found ? best : cap);
    near[c] = nr;
  }
  n_occ = dm_dist_wave_sum(n_occ);
  n_in = dm_dist_wave_sum(n_in);
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t v = (uint32_t)__shfl_xor((int)d_max, o, 64);
    d_max = v > d_max ? v : d_max;
  }
  if ((threadIdx.x & 63) == 0) {   // (s_c was zeroed before the barrier above)
    if (n_occ) atomicAdd(&s_c[0], n_occ);
    if (n_in) atomicAdd(&s_c[1], n_in);
    if (d_max) atomicMax(&s_c[2], d_max);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_c[threadIdx.x]) atomicAdd(&ctr[1 + threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
  if (threadIdx.x == 2 && s_c[2]) atomicMax(&ctr[3], (unsigned long long)s_c[2]);
}

struct DmDistField {
  uint32_t k, nx, ny, nz;
  int x0, y0, z0;
};

// one point per lane against the field.  qc: [0] inside, [1] outside, [2] inside and capped, [3] inside with d2 < min_d2,
// [4] ~((smallest d2 of an inside point) << 32 | the smallest index with it), taken by atomicMax from 0 = no point inside
__global__ __launch_bounds__(256) void k_dm_dist_query(const float4* __restrict__ pts, uint32_t n, float inv, DmDistField F,
                                                       const unsigned short* __restrict__ d2, const uint32_t* __restrict__ near,
                                                       uint32_t min_d2, loamx_dist_sample* __restrict__ out,
                                                       unsigned long long* __restrict__ qc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  loamx_dist_sample s;
  s.d2 = LOAMX_DIST_OUTSIDE;
  s.near = DM_DIST_NONE;
  bool in = false;
  if (i < n) {
    const float4 p = pts[i];
    if (dm_in_key_range(p, inv)) {
      const int ix = (int)floorf(p.x * inv), iy = (int)floorf(p.y * inv), iz = (int)floorf(p.z * inv);
      const uint32_t rx = dm_dist_rel((uint32_t)(ix + (1 << DM_QBITS)), F.k, F.x0), ry = dm_dist_rel((uint32_t)(iy + (1 << DM_QBITS)), F.k, F.y0),
                     rz = dm_dist_rel((uint32_t)(iz + (1 << DM_QBITS)), F.k, F.z0);
      if (rx < F.nx && ry < F.ny && rz < F.nz) {
        const size_t c = ((size_t)rz * F.ny + ry) * F.nx + rx;
        s.d2 = d2[c];
        s.near = near[c];
        in = true;
      }
    }
    if (out) out[i] = s;
  }
  // the block's counts and minimum in LDS, then one global atomic per word
  __shared__ uint32_t s_c[4];
  __shared__ unsigned long long s_m;
  if (threadIdx.x < 4) s_c[threadIdx.x] = 0u;
  if (threadIdx.x == 4) s_m = ~0ull;
  __syncthreads();
  const uint32_t c0 = (uint32_t)__popcll(__ballot(in)), c1 = (uint32_t)__popcll(__ballot(i < n && !in)),
                 c2 = (uint32_t)__popcll(__ballot(in && s.near == DM_DIST_NONE)), c3 = (uint32_t)__popcll(__ballot(in && s.d2 < min_d2));
  unsigned long long m = in ? ((unsigned long long)s.d2 << 32) | i : ~0ull;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned long long v = __shfl_xor(m, o, 64);
    m = v < m ? v : m;
  }
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(&s_c[0], c0);
    if (c1) atomicAdd(&s_c[1], c1);
    if (c2) atomicAdd(&s_c[2], c2);
    if (c3) atomicAdd(&s_c[3], c3);
    if (m != ~0ull) atomicMin(&s_m, m);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_c[threadIdx.x]) atomicAdd(&qc[threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
  if (threadIdx.x == 4 && s_m != ~0ull) atomicMax(&qc[4], ~s_m);
}

void DmDist::run(const DmTable& T, const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, bool want_d2, bool want_near,
                 uint64_t stats[4], hipStream_t st) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;   // (<= 2^26)
  const uint32_t words = (c.nx + 63u) / 64u;
  const size_t vol_words = DM_DIST_CTR + (size_t)words * c.ny * c.nz;
  valid_ = false;   // (a buffer that grows drops what it held)
  vol_.reserve(vol_words);
  yx_.reserve(cells);
  d2_.reserve((cells + 1) / 2);
  near_.reserve(cells);
  h_ctr_.reserve(DM_DIST_CTR);
  if (want_d2) h_d2_.reserve((cells + 1) / 2);
  if (want_near) h_near_.reserve(cells);
  DmDistArgs A;
  A.k = c.cell_leaves; A.nx = c.nx; A.ny = c.ny; A.nz = c.nz; A.min_points = c.min_points;
  A.x0 = c.x0; A.y0 = c.y0; A.z0 = c.z0;
  A.R = c.d_max; A.words = words;
  A.use_rule = rule ? 1 : 0;
  A.rule = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
  const int hy = (int)std::min(c.d_max, c.ny - 1u), hz = (int)std::min(c.d_max, c.nz - 1u);
  const uint32_t tiles_x = (c.nx + DM_DIST_TX - 1) / DM_DIST_TX;
  LX_HIP(hipMemsetAsync(vol_.p, 0, sizeof(unsigned long long) * vol_words, st));
  hipLaunchKernelGGL(k_dm_dist_mark, dim3(std::min((T.slots + 255u) / 256u, DM_DIST_MARK_BLOCKS)), dim3(256), 0, st, A, T.keys, T.vals, T.aux, T.slots, vol_.p);
  hipLaunchKernelGGL(k_dm_dist_xy, dim3(tiles_x, (c.ny + DM_DIST_TL - 1) / DM_DIST_TL, c.nz), dim3(256),
                     sizeof(unsigned short) * (DM_DIST_TL + 2 * hy) * DM_DIST_TX, st, A, hy, vol_.p, yx_.p);
  hipLaunchKernelGGL(k_dm_dist_z, dim3(tiles_x, (c.nz + DM_DIST_TL - 1) / DM_DIST_TL, c.ny), dim3(256),
                     sizeof(unsigned short) * (DM_DIST_TL + 2 * hz) * DM_DIST_TX, st, A, hz, yx_.p, (unsigned short*)d2_.p, near_.p, vol_.p);
  LX_HIP(hipGetLastError());
  h_ctr_.fetch(vol_.p, DM_DIST_CTR, st);
  if (want_d2) h_d2_.fetch(d2_.p, (cells + 1) / 2, st);
  if (want_near) h_near_.fetch(near_.p, cells, st);
  LX_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < DM_DIST_CTR; k++) stats[k] = h_ctr_.data()[k];
  cfg_ = c;
  valid_ = true;
}

const loamx_dist_sample* DmDist::query(const float4* pts, uint32_t n, float inv, uint32_t min_d2, bool want_samples, uint64_t stats[5],
                                       hipStream_t st) {
  qc_.reserve(5);
  h_qc_.reserve(5);
  if (want_samples) {
    d_out_.reserve(n);
    h_out_.reserve(n);
  }
  DmDistField F;
  F.k = cfg_.cell_leaves; F.nx = cfg_.nx; F.ny = cfg_.ny; F.nz = cfg_.nz;
  F.x0 = cfg_.x0; F.y0 = cfg_.y0; F.z0 = cfg_.z0;
  LX_HIP(hipMemsetAsync(qc_.p, 0, sizeof(unsigned long long) * 5, st));
  hipLaunchKernelGGL(k_dm_dist_query, dim3((n + 255u) / 256u), dim3(256), 0, st, pts, n, inv, F, (const unsigned short*)d2_.p, near_.p, min_d2,
                     want_samples ? d_out_.p : nullptr, qc_.p);
  LX_HIP(hipGetLastError());
  h_qc_.fetch(qc_.p, 5, st);
  if (want_samples) h_out_.fetch(d_out_.p, n, st);
  LX_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < 4; k++) stats[k] = h_qc_.data()[k];
  stats[4] = ~h_qc_.data()[4];
  return want_samples ? h_out_.data() : nullptr;
}

void dm_dist_check(const loamx_densemap_dist_config& c) {
  LX_REQUIRE(c.cell_leaves >= 1u && c.cell_leaves <= 64u, "cell_leaves must be in [1, 64]");
  LX_REQUIRE(c.x0 >= -(1 << 21) && c.x0 <= (1 << 21), "x0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.y0 >= -(1 << 21) && c.y0 <= (1 << 21), "y0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.z0 >= -(1 << 21) && c.z0 <= (1 << 21), "z0 must be in [-2^21, 2^21]");
  LX_REQUIRE(c.nx >= 1u && c.nx <= DM_DIST_MAX_SIDE, "nx must be in [1, 1024]");
  LX_REQUIRE(c.ny >= 1u && c.ny <= DM_DIST_MAX_SIDE, "ny must be in [1, 1024]");
  LX_REQUIRE(c.nz >= 1u && c.nz <= DM_DIST_MAX_SIDE, "nz must be in [1, 1024]");
  LX_REQUIRE((uint64_t)c.nx * c.ny * c.nz <= (1ull << 26), "nx * ny * nz must be <= 2^26");
  LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
  LX_REQUIRE(c.d_max <= DM_DIST_MAX_R, "d_max must be in [0, 254]");
}

// the window of one axis (include/loamx.h, loamx_densemap_dist_window)
static void dist_window_axis(double e, float centre, float half, const char* first, const char* count, int32_t& lo_out, uint32_t& n_out) {
  const double lo = std::floor(((double)centre - (double)half) / e), hi = std::floor(((double)centre + (double)half) / e);
  LX_REQUIRE(std::fabs(lo) <= 2097152.0, std::string(first) + " of the window is outside [-2^21, 2^21]");
  LX_REQUIRE(hi - lo + 1.0 <= (double)DM_DIST_MAX_SIDE, std::string(count) + " of the window is above 1024");
  lo_out = (int32_t)lo;
  n_out = (uint32_t)(hi - lo + 1.0);
}

// include/loamx.h, loamx_densemap_dist
void DenseMap::dist(const loamx_densemap_dist_config& c, const loamx_densemap_static_rule* rule, uint16_t* out_d2, uint32_t* out_near,
                    uint64_t stats[4]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  uint64_t s[4];
  dist_.run(tab_, c, rule, out_d2 != nullptr, out_near != nullptr, s, own_);
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  if (out_d2) memcpy(out_d2, dist_.d2_on_host(), sizeof(uint16_t) * cells);
  if (out_near) memcpy(out_near, dist_.near_on_host(), sizeof(uint32_t) * cells);
  memcpy(stats, s, sizeof(s));
}

// include/loamx.h, loamx_densemap_dist_query: the points go up through the feature's own staging block
int DenseMap::dist_query(const loamx_cloud* points, uint32_t min_d2, loamx_dist_sample* out, uint64_t capacity, uint64_t stats[5]) {
  LX_REQUIRE(dist_.has_field(), "the handle has no distance field (loamx_densemap_dist)");
  check_cloud(points, false);
  const uint32_t n = points->count;
  if (out && capacity < n) throw Error(LOAMX_E_CAPACITY, "capacity is smaller than the cloud's count");
  uint64_t s[5] = {0, 0, 0, 0, ~0ull};
  if (n) {
    LX_HIP(hipSetDevice(cfg.device));
    const float4* pts = dist_.cloud.stage(points, own_);
    const loamx_dist_sample* got = dist_.query(pts, n, inv_, min_d2, out != nullptr, s, own_);
    if (out) memcpy(out, got, sizeof(loamx_dist_sample) * n);
  }
  memcpy(stats, s, sizeof(s));
  return LOAMX_OK;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_dist_default_config(loamx_densemap_dist_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->cell_leaves = 2u;
  cfg->x0 = cfg->y0 = cfg->z0 = 0;
  cfg->nx = 128u;
  cfg->ny = 32u;
  cfg->nz = 128u;
  cfg->min_points = 2u;
  cfg->d_max = 16u;
}

int loamx_densemap_dist_check(const loamx_densemap_dist_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    dm_dist_check(*cfg);
    return LOAMX_OK;
  });
}

int loamx_densemap_dist_window(float leaf, const float centre[3], const float half_extent[3], loamx_densemap_dist_config* cfg) {
  return guard([&]() {
    LX_REQUIRE(cfg, "cfg is NULL");
    LX_REQUIRE(centre, "centre is NULL");
    LX_REQUIRE(half_extent, "half_extent is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    for (int a = 0; a < 3; a++) {
      LX_REQUIRE(std::isfinite(centre[a]), "centre must be finite");
      LX_REQUIRE(half_extent[a] >= 0.f && std::isfinite(half_extent[a]), "half_extent must be >= 0");
    }
    LX_REQUIRE(cfg->cell_leaves >= 1u && cfg->cell_leaves <= 64u, "cell_leaves must be in [1, 64]");
    const double e = (double)leaf * (double)cfg->cell_leaves;
    loamx_densemap_dist_config c = *cfg;
    dist_window_axis(e, centre[0], half_extent[0], "x0", "nx", c.x0, c.nx);
    dist_window_axis(e, centre[1], half_extent[1], "y0", "ny", c.y0, c.ny);
    dist_window_axis(e, centre[2], half_extent[2], "z0", "nz", c.z0, c.nz);
    LX_REQUIRE((uint64_t)c.nx * c.ny * c.nz <= (1ull << 26), "nx * ny * nz of the window is above 2^26");
    *cfg = c;
    return LOAMX_OK;
  });
}

int loamx_densemap_dist(loamx_densemap* h, const loamx_densemap_dist_config* cfg, const loamx_densemap_static_rule* rule, uint16_t* out_d2,
                        uint32_t* out_near, uint64_t stats[4]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    const loamx_densemap_dist_config c = or_default(cfg, loamx_densemap_dist_default_config);
    dm_dist_check(c);
    checked_optional_rule(h, rule);
    h->d.dist(c, rule, out_d2, out_near, stats);
    return LOAMX_OK;
  });
}

int loamx_densemap_dist_query(loamx_densemap* h, const loamx_cloud* points, uint32_t min_d2, loamx_dist_sample* out, uint64_t capacity,
                              uint64_t stats[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(points, "points is NULL");
    LX_REQUIRE(stats, "stats is NULL");
    return h->d.dist_query(points, min_d2, out, capacity, stats);
  });
}

// (loamx_dist_near_unpack and loamx_dist_metres, host only, are defined in api_dist.hip: tests/test_build_options.py asks that every
// loamx_dist_* entry point of the header is defined by that translation unit)

}  // extern "C"
