// Routing in 3-D over the distance field (densemap.hpp DmRoute3, include/loamx.h loamx_densemap_route3 and what goes with it): the
// cost-to-go of every cell of a 3-D window towards a set of goal cells, the next step per cell and routes traced from many starts.
//
// k_dm_route3_weights gives every cell its weight (a byte, from its 16-bit d2) and the cost UINT32_MAX, k_dm_route3_seed puts 0 on the
// used goals and marks their bricks, k_dm_route3_relax is launched round after round (densemap_route_schedule.hpp, as it is) until no
// brick is marked, k_dm_route3_next derives next from the final costs and counts, k_dm_route3_trace walks next from many starts.
// Integer atomics only; the costs are the unique fixed point of cost[c] = min over legal moves of cost[nb] + move, so no word
// depends on the schedule, the number of rounds or the rounds per look.
//
// k_dm_route3_relax, one block of 256 threads per brick of 8 x 8 x 8 cells: the brick's weights and costs with a halo of one cell
// (10^3 cells, 1,000 + 4,000 bytes) go to LDS, every thread works out once, for its two cells, which of the 26 moves are legal and
// what they cost (every intermediate cell of the corner rule lies in the halo, the steps being +-1), the block relaxes in LDS until
// no cell of the brick changes, and writes back the cells that fell.  Only the owning brick writes a cell.  The argument of
// densemap_route.hip, restated for three dimensions:
//   * a halo read of a neighbour brick that is writing in the same launch is benign: costs only fall, an aligned 32-bit read is
//     whole, and every value ever stored is the cost of a real path, an upper bound of the final cost;
//   * a brick whose border cell fell marks, AFTER its stores, every one of the up to 26 neighbour bricks whose halo holds that cell
//     (a face cell one, an edge cell three, a corner cell seven), in the plane of the next round.  A neighbour that read the old
//     value in this launch therefore re-runs behind the kernel boundary, where the new value is visible; a brick that is not marked
//     has a halo that did not change since it last ran, and is at its fixed point already;
//   * so after round r (r = 0: the goals' bricks) every cell whose cheapest path crosses at most r brick borders is final: by
//     induction, the path's last cell h before it enters the brick is final after round r - 1, the round that made it final marked
//     this brick (a move is one step on every axis, so h lies in this brick's halo), the brick runs behind that round, reads h final
//     and relaxes the path's stretch inside the brick to the end in LDS.  The corner rule does not disturb this: it only decides
//     which moves exist, from weights, which never change.
// With M the largest such count over the reachable cells the costs are final after round M, round M + 1 runs what those last falls
// marked and changes nothing, and no later round runs a brick: at most M + 2 rounds run a brick, M < nx * ny * nz.
// Inside LDS a sweep lowers at least the next cell of every unfinished cheapest path, so 512 sweeps and one that finds nothing
// bound the loop; the bound (512 + 2) is in the code, and a brick that ever left it unsettled would mark itself.
#include "densemap_map.hpp"
#include "densemap_route_schedule.hpp"
#include "pinned_copy.hpp"

namespace loamx {

constexpr int DM_ROUTE3_BRICK = 8;
constexpr int DM_ROUTE3_SIDE = DM_ROUTE3_BRICK + 2;   // with the halo
constexpr int DM_ROUTE3_LDS = DM_ROUTE3_SIDE * DM_ROUTE3_SIDE * DM_ROUTE3_SIDE;
constexpr int DM_ROUTE3_SWEEPS = DM_ROUTE3_BRICK * DM_ROUTE3_BRICK * DM_ROUTE3_BRICK + 2;
constexpr uint32_t DM_ROUTE3_MAX_CELLS = 1u << 22;
constexpr uint32_t DM_ROUTE3_MAX_SIDE = 1024;
constexpr uint32_t DM_ROUTE3_MAX_XYZ = 4096;   // goals, starts
constexpr uint32_t DM_ROUTE3_INF = LOAMX_ROUTE_UNREACHABLE;

__host__ __device__ inline uint32_t dm_route3_scale(int dx, int dy, int dz) { return 3u + 2u * (uint32_t)((dx != 0) + (dy != 0) + (dz != 0)); }

__global__ __launch_bounds__(256) void k_dm_route3_weights(const unsigned short* __restrict__ d2, uint32_t n, loamx_route3_config C,
                                                           unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                           unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t wt = 0u;
  if (c < n) {
    wt = dm_route3_weight(d2[c], C);   // (16 bits per cell, two cells per word of the distance field's plane)
    w[c] = (unsigned char)wt;
    cost[c] = DM_ROUTE3_INF;
  }
  const unsigned long long b = __ballot(wt > 0u);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&s_n, (uint32_t)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&st[0], (unsigned long long)s_n);
}

// one thread per goal triple: 0 on a used goal (every writer stores the same word), its brick marked for round 0
__global__ __launch_bounds__(256) void k_dm_route3_seed(const uint32_t* __restrict__ goals, uint32_t n_goals, uint32_t nx, uint32_t ny,
                                                        uint32_t nz, uint32_t bricks_x, uint32_t bricks_y,
                                                        const unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                        uint32_t* __restrict__ dirty, unsigned long long* __restrict__ st) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_goals) return;
  const uint32_t x = goals[3u * i], y = goals[3u * i + 1u], z = goals[3u * i + 2u];
  if (x >= nx || y >= ny || z >= nz) return;
  const uint32_t c = (z * ny + y) * nx + x;
  if (!w[c]) return;
  cost[c] = 0u;
  dirty[((z / DM_ROUTE3_BRICK) * bricks_y + y / DM_ROUTE3_BRICK) * bricks_x + x / DM_ROUTE3_BRICK] = 1u;
  atomicAdd(&st[2], 1ull);
}

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

// one thread per cell: the record from the final costs, the smallest d first; the reachable cells and the largest finite cost
__global__ __launch_bounds__(256) void k_dm_route3_next(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn,
                                                        const unsigned char* __restrict__ w, const uint32_t* __restrict__ cost,
                                                        loamx_route_cell* __restrict__ field, unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n, s_max;
  if (threadIdx.x == 0) s_n = s_max = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  bool reach = false;
  if (c < nx * ny * nz) {
    const uint32_t x = c % nx, y = (c / nx) % ny, z = c / (nx * ny), cc = cost[c], wa = w[c];
    uint32_t next = LOAMX_ROUTE3_NONE;
    reach = cc != DM_ROUTE3_INF;
    if (cc == 0u) next = LOAMX_ROUTE3_GOAL;
    else if (reach) {
      for (uint32_t d = 0; d < conn && next == LOAMX_ROUTE3_NONE; d++) {
        int dx, dy, dz;
        dm_route3_move(d, dx, dy, dz);
        const uint32_t bxx = x + (uint32_t)dx, byy = y + (uint32_t)dy, bzz = z + (uint32_t)dz;   // (a cell before the window wraps)
        if (bxx >= nx || byy >= ny || bzz >= nz) continue;
        const uint32_t nb = (bzz * ny + byy) * nx + bxx, wb = w[nb], cn = cost[nb];
        if (!wb || cn == DM_ROUTE3_INF) continue;
        bool ok = true;   // no corner cutting (the cells between lie in the box of a and b, inside the window)
        for (int m = 1; m < 7 && ok; m++) {
          const uint32_t sx = (m & 1) ? bxx : x, sy = (m & 2) ? byy : y, sz = (m & 4) ? bzz : z;
          ok = w[(sz * ny + sy) * nx + sx] > 0u;   // (a or b again where an axis does not move: both > 0)
        }
        if (ok && cn + dm_route3_scale(dx, dy, dz) * (wa + wb) == cc) next = d;
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

// one thread per start, walking next; bounded by nx * ny * nz steps.  offsets NULL: the lengths only.  Otherwise start i's triples go
// to out + 3 * offsets[i], the first min(length, capacity) of them (the same walk as the counting pass over the same field)
__global__ __launch_bounds__(256) void k_dm_route3_trace(const loamx_route_cell* __restrict__ field, uint32_t nx, uint32_t ny, uint32_t nz,
                                                         const uint32_t* __restrict__ starts, uint32_t n_starts, uint32_t capacity,
                                                         const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ lengths,
                                                         uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_starts) return;
  uint32_t x = starts[3u * i], y = starts[3u * i + 1u], z = starts[3u * i + 2u], len = 0u;
  if (x < nx && y < ny && z < nz) {
    const uint32_t cells = nx * ny * nz;
    for (uint32_t step = 0; step < cells; step++) {
      const uint32_t next = field[((size_t)z * ny + y) * nx + x].next;
      if (next >= LOAMX_ROUTE3_NONE) break;
      if (offsets && len < capacity) {
        uint32_t* o = out + 3ull * (offsets[i] + len);
        o[0] = x;
        o[1] = y;
        o[2] = z;
      }
      len++;
      if (next == LOAMX_ROUTE3_GOAL) break;
      int dx, dy, dz;
      dm_route3_move(next, dx, dy, dz);
      x += (uint32_t)dx;
      y += (uint32_t)dy;
      z += (uint32_t)dz;
      if (x >= nx || y >= ny || z >= nz) break;   // (never on a field of k_dm_route3_next)
    }
  }
  if (!offsets) lengths[i] = len;
}

void dm_route3_check(const loamx_route3_config& c) {
  LX_REQUIRE(c.connectivity == 6u || c.connectivity == 18u || c.connectivity == 26u, "connectivity must be 6, 18 or 26");
  LX_REQUIRE(c.min_d2 >= 1u, "min_d2 must be >= 1");
  LX_REQUIRE(c.soft_d2 <= 65025u, "soft_d2 must be in [0, 65025]");
  LX_REQUIRE(c.soft_weight <= 15u, "soft_weight must be in [0, 15]");
}

const unsigned short* DmRoute3::upload(const uint16_t* d2, size_t n, hipStream_t st) {
  own_d2_.reserve((n + 1) / 2);
  LX_HIP(hipMemcpyAsync(own_d2_.p, d2, sizeof(uint16_t) * n, hipMemcpyHostToDevice, st));
  return (const unsigned short*)own_d2_.p;
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
const loamx_route_cell* DmRoute3::run(const unsigned short* d_d2, uint32_t nx, uint32_t ny, uint32_t nz, const loamx_route3_config& c,
                                      const uint32_t* goals_xyz, uint32_t n_goals, bool want_field, uint64_t stats[6], hipStream_t st) {
  const uint32_t n = nx * ny * nz;
  const uint32_t bricks_x = (nx + DM_ROUTE3_BRICK - 1) / DM_ROUTE3_BRICK, bricks_y = (ny + DM_ROUTE3_BRICK - 1) / DM_ROUTE3_BRICK,
                 bricks_z = (nz + DM_ROUTE3_BRICK - 1) / DM_ROUTE3_BRICK;
  const uint32_t bricks = bricks_x * bricks_y * bricks_z;
  constexpr uint32_t CTR_WORDS = 2u * ROUTE_MAX_BATCH, ST_WORDS = 8u;   // the slots; the four 64-bit stats as 32-bit words
  valid_ = false;
  w_.reserve(n);
  cost_.reserve(n);
  field_.reserve(n);
  dirty_.reserve(2 * (size_t)bricks);
  ctr_.reserve(CTR_WORDS);
  st_.reserve(ST_WORDS / 2);
  d_xyz_.reserve(3 * DM_ROUTE3_MAX_XYZ);
  h_xyz_.reserve(3 * DM_ROUTE3_MAX_XYZ);
  h_ctr_.reserve(CTR_WORDS + ST_WORDS);
  if (want_field) h_field_.reserve(n);
  memcpy(h_xyz_.p, goals_xyz, sizeof(uint32_t) * 3 * n_goals);
  LX_HIP(hipMemcpyAsync(d_xyz_.p, h_xyz_.p, sizeof(uint32_t) * 3 * n_goals, hipMemcpyHostToDevice, st));
  LX_HIP(hipMemsetAsync(dirty_.p, 0, sizeof(uint32_t) * 2 * (size_t)bricks, st));
  LX_HIP(hipMemsetAsync(st_.p, 0, sizeof(uint32_t) * ST_WORDS, st));
  const dim3 per_cell((n + 255u) / 256u), per_brick(bricks_x, bricks_y, bricks_z);
  hipLaunchKernelGGL(k_dm_route3_weights, per_cell, dim3(256), 0, st, d_d2, n, c, w_.p, cost_.p, st_.p);
  hipLaunchKernelGGL(k_dm_route3_seed, dim3((n_goals + 255u) / 256u), dim3(256), 0, st, d_xyz_.p, n_goals, nx, ny, nz, bricks_x, bricks_y,
                     w_.p, cost_.p, dirty_.p, st_.p);
  LX_HIP(hipGetLastError());
  struct Ops {
    DmRoute3& r;
    uint32_t nx, ny, nz, bricks, conn;
    dim3 per_brick;
    hipStream_t st;
    void begin(uint32_t) { LX_HIP(hipMemsetAsync(r.ctr_.p, 0, sizeof(uint32_t) * CTR_WORDS, st)); }
    void round(uint64_t, uint32_t read_plane, uint32_t mark_plane, uint32_t slot) {
      hipLaunchKernelGGL(k_dm_route3_relax, per_brick, dim3(256), 0, st, nx, ny, nz, conn, r.w_.p, r.cost_.p,
                         r.dirty_.p + (size_t)read_plane * bricks, r.dirty_.p + (size_t)mark_plane * bricks, r.ctr_.p + 2u * slot);
    }
    const RouteSlot* look(uint32_t k) {
      LX_HIP(hipGetLastError());
      store_to_pinned_u32(r.h_ctr_.p, r.ctr_.p, 2u * k, st);
      LX_HIP(hipStreamSynchronize(st));
      return (const RouteSlot*)r.h_ctr_.p;
    }
  } ops{*this, nx, ny, nz, bricks, c.connectivity, per_brick, st};
  const RouteOutcome o = route_schedule(ops, RoutePlan{batch, (uint64_t)n + 2u});
  if (!o.settled) throw Error(LOAMX_E_INTERNAL, "route3: the relaxation did not settle within nx * ny * nz + 2 rounds");
  hipLaunchKernelGGL(k_dm_route3_next, per_cell, dim3(256), 0, st, nx, ny, nz, c.connectivity, w_.p, cost_.p, field_.p, st_.p);
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
  ny_ = ny;
  nz_ = nz;
  valid_ = true;
  return want_field ? h_field_.data() : nullptr;
}

// the counting pass, the offsets and the writing pass of DmRoute::trace, with triples
void DmRoute3::trace(const uint32_t* starts_xyz, uint32_t n_starts, uint32_t* out_xyz, uint32_t capacity, uint32_t* lengths, hipStream_t st) {
  d_xyz_.reserve(3 * DM_ROUTE3_MAX_XYZ);
  h_xyz_.reserve(3 * DM_ROUTE3_MAX_XYZ);
  d_len_.reserve(DM_ROUTE3_MAX_XYZ);
  d_off_.reserve(DM_ROUTE3_MAX_XYZ);
  h_len_.reserve(DM_ROUTE3_MAX_XYZ);
  h_off_.reserve(DM_ROUTE3_MAX_XYZ);
  memcpy(h_xyz_.p, starts_xyz, sizeof(uint32_t) * 3 * n_starts);
  LX_HIP(hipMemcpyAsync(d_xyz_.p, h_xyz_.p, sizeof(uint32_t) * 3 * n_starts, hipMemcpyHostToDevice, st));
  const dim3 per_start((n_starts + 255u) / 256u);
  hipLaunchKernelGGL(k_dm_route3_trace, per_start, dim3(256), 0, st, field_.p, nx_, ny_, nz_, d_xyz_.p, n_starts, capacity,
                     (const unsigned long long*)nullptr, d_len_.p, (uint32_t*)nullptr);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_len_.p, d_len_.p, n_starts, st);
  LX_HIP(hipStreamSynchronize(st));
  // the routes back to back on the device: start i's min(length, capacity) triples begin at triple offsets[i]
  size_t total = 0;
  for (uint32_t i = 0; i < n_starts; i++) {
    h_off_.p[i] = total;
    total += std::min(h_len_.p[i], capacity);
  }
  if (total) {
    d_routes_.reserve(3 * total);
    h_routes_.reserve(3 * total);
    LX_HIP(hipMemcpyAsync(d_off_.p, h_off_.p, sizeof(unsigned long long) * n_starts, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dm_route3_trace, per_start, dim3(256), 0, st, field_.p, nx_, ny_, nz_, d_xyz_.p, n_starts, capacity, d_off_.p,
                       d_len_.p, d_routes_.p);
    LX_HIP(hipGetLastError());
    store_to_pinned_u32(h_routes_.p, d_routes_.p, 3 * total, st);
    LX_HIP(hipStreamSynchronize(st));
  }
  for (uint32_t i = 0; i < n_starts; i++) {
    const size_t m = std::min(h_len_.p[i], capacity);
    if (m) memcpy(out_xyz + 3 * (size_t)capacity * i, h_routes_.p + 3 * (size_t)h_off_.p[i], sizeof(uint32_t) * 3 * m);
    lengths[i] = h_len_.p[i];
  }
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
  const size_t n = (size_t)c.nx * c.ny * c.nz;
  uint64_t s[6];
  const loamx_route_cell* field = route3_.run(dist_.d2_on_device(), c.nx, c.ny, c.nz, rc, goals_xyz, n_goals, out_field != nullptr, s, own_);
  if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * n);
  if (stats) memcpy(stats, s, sizeof(s));
}
// loamx_densemap_route3_cells: the same on the caller's plane, in a buffer of the route's own
void DenseMap::route3_cells(const uint16_t* d2, uint32_t nx, uint32_t ny, uint32_t nz, const loamx_route3_config& rc, const uint32_t* goals_xyz,
                            uint32_t n_goals, loamx_route_cell* out_field, uint64_t stats[6]) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  const size_t n = (size_t)nx * ny * nz;
  uint64_t s[6];
  const loamx_route_cell* field = route3_.run(route3_.upload(d2, n, own_), nx, ny, nz, rc, goals_xyz, n_goals, out_field != nullptr, s, own_);
  if (out_field) memcpy(out_field, field, sizeof(loamx_route_cell) * n);
  if (stats) memcpy(stats, s, sizeof(s));
}
void DenseMap::route3_trace(const uint32_t* starts_xyz, uint32_t n_starts, uint32_t* out_xyz, uint32_t capacity, uint32_t* lengths) {
  LX_REQUIRE(route3_.has_field(), "the handle has no field yet (loamx_densemap_route3, loamx_densemap_route3_last, loamx_densemap_route3_cells)");
  LX_HIP(hipSetDevice(cfg.device));
  route3_.trace(starts_xyz, n_starts, out_xyz, capacity, lengths, own_);
}

// the checks the route3 entry points share: the configuration (NULL: the defaults), the goals and the window's size
static loamx_route3_config checked_route3(const loamx_route3_config* cfg, const uint32_t* goals_xyz, uint32_t n_goals, uint32_t nx, uint32_t ny,
                                          uint32_t nz) {
  const loamx_route3_config rc = or_default(cfg, loamx_route3_default_config);
  dm_route3_check(rc);
  LX_REQUIRE(goals_xyz, "goals_xyz is NULL");
  LX_REQUIRE(n_goals >= 1u && n_goals <= DM_ROUTE3_MAX_XYZ, "n_goals must be in [1, 4096]");
  LX_REQUIRE((uint64_t)nx * ny * nz <= DM_ROUTE3_MAX_CELLS, "nx * ny * nz must be <= 2^22 for a route");
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
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(starts_xyz, "starts_xyz is NULL");
    LX_REQUIRE(n_starts >= 1u && n_starts <= DM_ROUTE3_MAX_XYZ, "n_starts must be in [1, 4096]");
    LX_REQUIRE(out_xyz || !capacity, "out_xyz is NULL");
    LX_REQUIRE(lengths, "lengths is NULL");
    h->d.route3_trace(starts_xyz, n_starts, out_xyz, capacity, lengths);
    return LOAMX_OK;
  });
}

// bench / test hooks (not in include/loamx.h): the rounds per look (1..64), and the rounds of the last route3 in which a brick ran
int loamx_densemap_route3_set_batch(loamx_densemap* h, uint32_t batch) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    LX_REQUIRE(batch >= 1u && batch <= 64u, "batch must be in [1, 64]");
    h->d.router3().batch = batch;
    return LOAMX_OK;
  });
}
uint64_t loamx_densemap_route3_active_rounds(loamx_densemap* h) { return h ? h->d.router3().active_rounds : 0; }

int loamx_route3_trace(const loamx_route_cell* field, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t start[3], uint32_t* out_xyz,
                       uint32_t capacity, uint32_t* length) {
  return guard([&]() {
    LX_REQUIRE(field, "field is NULL");
    LX_REQUIRE(nx >= 1u && ny >= 1u && nz >= 1u && (uint64_t)nx * ny * nz <= DM_ROUTE3_MAX_CELLS && (uint64_t)nx * ny <= DM_ROUTE3_MAX_CELLS,
               "nx * ny * nz must be in [1, 2^22]");
    LX_REQUIRE(start, "start is NULL");
    LX_REQUIRE(out_xyz || !capacity, "out_xyz is NULL");
    LX_REQUIRE(length, "length is NULL");
    uint32_t len = 0;
    // the walk twice: checked to its end first, so that a field that is not one of ours leaves nothing written
    for (int pass = 0; pass < 2; pass++) {
      uint32_t x = start[0], y = start[1], z = start[2];
      len = 0;
      if (x >= nx || y >= ny || z >= nz) break;
      for (;;) {
        const loamx_route_cell& r = field[((size_t)z * ny + y) * nx + x];
        LX_REQUIRE(r.next <= LOAMX_ROUTE3_NONE, "field: a next above 27");
        if (r.next == LOAMX_ROUTE3_NONE) {
          LX_REQUIRE(len == 0u, "field: the route ends on a cell that is no goal");
          break;
        }
        if (pass && len < capacity) {
          out_xyz[3 * (size_t)len] = x;
          out_xyz[3 * (size_t)len + 1] = y;
          out_xyz[3 * (size_t)len + 2] = z;
        }
        len++;
        if (r.next == LOAMX_ROUTE3_GOAL) break;
        int dx, dy, dz;
        dm_route3_move(r.next, dx, dy, dz);
        const uint32_t bx = x + (uint32_t)dx, by = y + (uint32_t)dy, bz = z + (uint32_t)dz;
        LX_REQUIRE(bx < nx && by < ny && bz < nz, "field: a step leaves the window");
        LX_REQUIRE(field[((size_t)bz * ny + by) * nx + bx].cost < r.cost, "field: a step to a cell whose cost is not strictly smaller");
        x = bx;
        y = by;
        z = bz;
      }
    }
    *length = len;
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
