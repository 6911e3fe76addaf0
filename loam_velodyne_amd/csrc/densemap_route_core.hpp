// The route engine (include/loamx.h, loamx_densemap_route ... and loamx_densemap_route3 ...): the cost-to-go of every cell of a window
// towards a set of goal cells, the next step per cell and routes traced from many starts, written once over a "kind".  A kind is a
// struct of static members that says in what the 2-D route over the navigation grid (DmRouteGrid, densemap_route.hip) and the 3-D
// route over the distance field (DmRouteVol, densemap_route3.hip) differ: the tile, the input element and its weight, the moves,
// their order and scale, the two values of next past the directions, the words of the messages, and the launch of its relax kernel.
// A window is (nx, ny, nz) with the linear index (z * ny + y) * nx + x; a 2-D window is (nx, 1, nz) and its tuples are (x, z) pairs.
//
// k_dm_route_weights gives every cell its weight (a byte) and the cost UINT32_MAX, k_dm_route_seed puts 0 on the used goals and marks
// their tiles, the kind's relax kernel is launched round after round (densemap_route_schedule.hpp) until no tile is marked,
// k_dm_route_next derives next from the final costs and counts, k_dm_route_trace walks next from many starts.  Integer atomics only;
// the costs are the unique fixed point of cost[c] = min over legal moves of cost[nb] + move, so no word depends on the schedule, the
// number of rounds or the rounds per look.  Why the rounds reach that fixed point: the head comment of densemap_route.hip.
#pragma once
#include "densemap.hpp"
#include "densemap_route_schedule.hpp"
#include "pinned_copy.hpp"
#include <string>

namespace loamx {

constexpr uint32_t DM_ROUTE_MAX_CELLS = 1u << 22;
constexpr uint32_t DM_ROUTE_MAX_TUPLES = 4096;   // goals, starts
constexpr uint32_t DM_ROUTE_INF = LOAMX_ROUTE_UNREACHABLE;

// (dx, dz) of direction d of the grid route
__host__ __device__ inline int dm_route_dx(uint32_t d) { return d == 0u || d == 1u || d == 7u ? 1 : (d >= 3u && d <= 5u ? -1 : 0); }
__host__ __device__ inline int dm_route_dz(uint32_t d) { return d >= 1u && d <= 3u ? 1 : (d >= 5u ? -1 : 0); }
__host__ __device__ inline uint32_t dm_route3_scale(int dx, int dy, int dz) { return 3u + 2u * (uint32_t)((dx != 0) + (dy != 0) + (dz != 0)); }

// the grid route: tiles of 32 x 32 cells, eight directions of which the odd ones are diagonal
struct DmRouteGrid {
  static constexpr int DIM = 2, TILE = 32;
  static constexpr uint32_t GOAL = LOAMX_ROUTE_GOAL, NONE = LOAMX_ROUTE_NONE;
  using Config = loamx_grid_route_config;
  using Cell = loamx_grid_cell;
  using Store = loamx_grid_cell;   // the element of upload's buffer
  static constexpr const char *NAME = "route", *AXES = "xz", *NONE_TEXT = "9", *CELLS = "nx * nz";
  static constexpr const char* FIELD_FROM = "loamx_densemap_route, loamx_densemap_route_cells";
  __host__ __device__ static uint32_t weight(const Cell& c, const Config& C) { return dm_route_weight(c.cls, c.clear2, C); }
  __host__ __device__ static void move(uint32_t d, int& dx, int& dy, int& dz) { dx = dm_route_dx(d); dy = 0; dz = dm_route_dz(d); }
  // the directions of a connectivity: d = 0, step, 2 * step ... below end
  __host__ __device__ static uint32_t dir_end(uint32_t) { return 8u; }
  __host__ __device__ static uint32_t dir_step(uint32_t connectivity) { return connectivity == 8u ? 1u : 2u; }
  __host__ __device__ static uint32_t scale(uint32_t d, int, int, int) { return (d & 1u) ? 7u : 5u; }
  // one round of k_dm_route_relax over the window, enqueued on st
  static void relax(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t connectivity, const unsigned char* w, uint32_t* cost,
                    uint32_t* dirty_read, uint32_t* dirty_mark, uint32_t* slot, hipStream_t st);
};

// the 3-D route: bricks of 8 x 8 x 8 cells, the first 6, 18 or 26 directions
struct DmRouteVol {
  static constexpr int DIM = 3, TILE = 8;
  static constexpr uint32_t GOAL = LOAMX_ROUTE3_GOAL, NONE = LOAMX_ROUTE3_NONE;
  using Config = loamx_route3_config;
  using Cell = unsigned short;   // d2, 16 bits per cell
  using Store = uint32_t;        // two cells per word, as the distance field's plane
  static constexpr const char *NAME = "route3", *AXES = "xyz", *NONE_TEXT = "27", *CELLS = "nx * ny * nz";
  static constexpr const char* FIELD_FROM = "loamx_densemap_route3, loamx_densemap_route3_last, loamx_densemap_route3_cells";
  __host__ __device__ static uint32_t weight(const Cell& d2, const Config& C) { return dm_route3_weight(d2, C); }
  __host__ __device__ static void move(uint32_t d, int& dx, int& dy, int& dz) { dm_route3_move(d, dx, dy, dz); }
  __host__ __device__ static uint32_t dir_end(uint32_t connectivity) { return connectivity; }
  __host__ __device__ static uint32_t dir_step(uint32_t) { return 1u; }
  __host__ __device__ static uint32_t scale(uint32_t, int dx, int dy, int dz) { return dm_route3_scale(dx, dy, dz); }
  // one round of k_dm_route3_relax over the window, enqueued on st
  static void relax(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t connectivity, const unsigned char* w, uint32_t* cost,
                    uint32_t* dirty_read, uint32_t* dirty_mark, uint32_t* slot, hipStream_t st);
};

template <class K> constexpr uint32_t dm_route_tiles(uint32_t n) { return (n + K::TILE - 1) / K::TILE; }   // along one axis
// tuple i of an array of tuples of K::DIM words as a cell, and back (a pair has no y).  Word by word under a 32-bit index, as the
// kernels of both kinds read their goals and starts before they were one: the device code of the 3-D trace is what it was
template <class K> __host__ __device__ inline void dm_route_get(const uint32_t* t, uint32_t i, uint32_t& x, uint32_t& y, uint32_t& z) {
  constexpr uint32_t DIM = K::DIM;
  x = t[DIM * i];
  y = DIM == 3u ? t[DIM * i + 1u] : 0u;
  z = t[DIM * i + (DIM - 1u)];
}
template <class K> __host__ __device__ inline void dm_route_put(uint32_t* t, unsigned long long i, uint32_t x, uint32_t y, uint32_t z) {
  uint32_t* o = t + (unsigned long long)K::DIM * i;
  o[0] = x;
  if (K::DIM == 3) o[1] = y;
  o[K::DIM - 1] = z;
}

template <class K>
__global__ __launch_bounds__(256) void k_dm_route_weights(const typename K::Cell* __restrict__ cells, uint32_t n, typename K::Config C,
                                                          unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                          unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t wt = 0u;
  if (c < n) {
    wt = K::weight(cells[c], C);
    w[c] = (unsigned char)wt;
    cost[c] = DM_ROUTE_INF;
  }
  const unsigned long long b = __ballot(wt > 0u);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&s_n, (uint32_t)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&st[0], (unsigned long long)s_n);
}

// one thread per goal tuple: 0 on a used goal (every writer stores the same word), its tile marked for round 0
template <class K>
__global__ __launch_bounds__(256) void k_dm_route_seed(const uint32_t* __restrict__ goals, uint32_t n_goals, uint32_t nx, uint32_t ny,
                                                       uint32_t nz, const unsigned char* __restrict__ w, uint32_t* __restrict__ cost,
                                                       uint32_t* __restrict__ dirty, unsigned long long* __restrict__ st) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_goals) return;
  uint32_t x, y, z;
  dm_route_get<K>(goals, i, x, y, z);
  if (x >= nx || y >= ny || z >= nz) return;
  const uint32_t c = (z * ny + y) * nx + x;
  if (!w[c]) return;
  cost[c] = 0u;
  dirty[((z / K::TILE) * dm_route_tiles<K>(ny) + y / K::TILE) * dm_route_tiles<K>(nx) + x / K::TILE] = 1u;
  atomicAdd(&st[2], 1ull);
}

// one thread per cell: the record from the final costs, the first d in the kind's order whose move reproduces the cost; the
// reachable cells and the largest finite cost
template <class K>
__global__ __launch_bounds__(256) void k_dm_route_next(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn,
                                                       const unsigned char* __restrict__ w, const uint32_t* __restrict__ cost,
                                                       loamx_route_cell* __restrict__ field, unsigned long long* __restrict__ st) {
  __shared__ uint32_t s_n, s_max;
  if (threadIdx.x == 0) s_n = s_max = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  bool reach = false;
  if (c < nx * ny * nz) {
    const uint32_t x = c % nx, y = K::DIM == 3 ? (c / nx) % ny : 0u, z = c / (nx * ny), cc = cost[c], wa = w[c];
    uint32_t next = K::NONE;
    reach = cc != DM_ROUTE_INF;
    if (cc == 0u) next = K::GOAL;
    else if (reach) {
      for (uint32_t d = 0; d < K::dir_end(conn) && next == K::NONE; d += K::dir_step(conn)) {
        int dx, dy, dz;
        K::move(d, dx, dy, dz);
        const uint32_t bxx = x + (uint32_t)dx, byy = y + (uint32_t)dy, bzz = z + (uint32_t)dz;   // (a cell before the window wraps)
        if (bxx >= nx || byy >= ny || bzz >= nz) continue;
        const uint32_t nb = (bzz * ny + byy) * nx + bxx, wb = w[nb], cn = cost[nb];
        if (!wb || cn == DM_ROUTE_INF) continue;
        // no corner cutting: the cells between, which lie in the box of a and b, inside the window; bit k of m: axis k of the
        // tuple is b's (a or b again where an axis does not move: both > 0)
        bool ok = true;
        for (int m = 1; m < (1 << K::DIM) - 1 && ok; m++) {
          const uint32_t sx = (m & 1) ? bxx : x, sy = K::DIM == 3 && (m & 2) ? byy : y, sz = (m & (1 << (K::DIM - 1))) ? bzz : z;
          ok = w[(sz * ny + sy) * nx + sx] > 0u;
        }
        if (ok && cn + K::scale(d, dx, dy, dz) * (wa + wb) == cc) next = d;
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

// one thread per start, walking next; bounded by as many steps as the window has cells.  offsets NULL: the lengths only.  Otherwise
// start i's tuples go to out + K::DIM * offsets[i], the first min(length, capacity) of them (the same walk as the counting pass over
// the same field)
template <class K>
__global__ __launch_bounds__(256) void k_dm_route_trace(const loamx_route_cell* __restrict__ field, uint32_t nx, uint32_t ny, uint32_t nz,
                                                        const uint32_t* __restrict__ starts, uint32_t n_starts, uint32_t capacity,
                                                        const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ lengths,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_starts) return;
  uint32_t x, y, z, len = 0u;
  dm_route_get<K>(starts, i, x, y, z);
  if (x < nx && y < ny && z < nz) {
    const uint32_t cells = nx * ny * nz;
    for (uint32_t step = 0; step < cells; step++) {
      const uint32_t next = field[((size_t)z * ny + y) * nx + x].next;
      if (next >= K::NONE) break;
      if (offsets && len < capacity) dm_route_put<K>(out, offsets[i] + len, x, y, z);
      len++;
      if (next == K::GOAL) break;
      int dx, dy, dz;
      K::move(next, dx, dy, dz);
      x += (uint32_t)dx;
      y += (uint32_t)dy;
      z += (uint32_t)dz;
      if (x >= nx || y >= ny || z >= nz) break;   // (never on a field of k_dm_route_next)
    }
  }
  if (!offsets) lengths[i] = len;
}

// The buffers of one kind's routes: the weight, cost and dirty planes of a window, its field records and the pinned blocks that goals,
// starts, counters, field and routes cross through.  Allocated by the first call, grow to the largest window asked for; the map and
// the buffers of the grid and of the distance field are only read.
template <class K> class DmRouteT {
 public:
  using Cell = typename K::Cell;
  using Config = typename K::Config;
  DmRouteT() = default;
  DmRouteT(const DmRouteT&) = delete;
  DmRouteT& operator=(const DmRouteT&) = delete;
  // the caller's n input elements (checked) in a device buffer of the route's own, enqueued on st
  const Cell* upload(const Cell* cells, size_t n, hipStream_t st);
  // the field of nx * ny * nz <= 2^22 cells whose input lies at d_in on the device (written by work enqueued on st) under a checked
  // configuration towards n_goals in 1..4096 tuples: weights, seeding, the relaxation rounds of densemap_route_schedule.hpp, next
  // and the four exact stats.  Blocks; the field stays on the device for trace() and, when want_field, lies in pinned memory at the
  // return (valid until the next run).  LOAMX_E_INTERNAL when the rounds reach their cap unsettled
  const loamx_route_cell* run(const Cell* d_in, uint32_t nx, uint32_t ny, uint32_t nz, const Config& c, const uint32_t* goals,
                              uint32_t n_goals, bool want_field, uint64_t stats[6], hipStream_t st);
  bool has_field() const { return valid_; }
  void drop() { valid_ = false; }   // (the buffers stay for the next field)
  // the routes of n_starts in 1..4096 starts over the field of the last run (include/loamx.h, loamx_densemap_route_trace and
  // loamx_densemap_route3_trace); blocks
  void trace(const uint32_t* starts, uint32_t n_starts, uint32_t* out, uint32_t capacity, uint32_t* lengths, hipStream_t st);
  // the field of the last run where it lies on the device (DmFrontier reads the costs there), valid until the next run
  const loamx_route_cell* field_on_device() const { return field_.p; }

  uint32_t batch = 16;          // rounds per look (bench / test hook; the choice and its measurement: beside the kind's relax kernel)
  uint64_t active_rounds = 0;   // of the last run: rounds in which a tile ran (test hook)

 private:
  static constexpr uint32_t CTR_WORDS = 2u * ROUTE_MAX_BATCH, ST_WORDS = 8u;   // the slots; the four 64-bit stats as 32-bit words
  DevBuf<typename K::Store> own_in_;    // upload's elements
  DevBuf<unsigned char> w_;             // weight per cell
  DevBuf<uint32_t> cost_;               // cost per cell
  DevBuf<uint32_t> dirty_;              // two planes of one word per tile
  DevBuf<loamx_route_cell> field_;
  DevBuf<uint32_t> ctr_;                // ROUTE_MAX_BATCH slots of two words (densemap_route_schedule.hpp)
  DevBuf<unsigned long long> st_;       // the four exact stats
  DevBuf<uint32_t> d_tup_, d_len_, d_routes_;   // goals or starts; the routes' lengths; the routes back to back
  DevBuf<unsigned long long> d_off_;            // the first tuple of each route in d_routes_
  PinBuf<uint32_t> h_tup_, h_ctr_, h_len_, h_routes_;
  PinLanding<loamx_route_cell> h_field_;
  PinBuf<unsigned long long> h_off_;
  uint32_t nx_ = 0, ny_ = 0, nz_ = 0;
  bool valid_ = false;
};

template <class K> const typename K::Cell* DmRouteT<K>::upload(const Cell* cells, size_t n, hipStream_t st) {
  own_in_.reserve((n * sizeof(Cell) + sizeof(typename K::Store) - 1) / sizeof(typename K::Store));
  LX_HIP(hipMemcpyAsync(own_in_.p, cells, sizeof(Cell) * n, hipMemcpyHostToDevice, st));
  return (const Cell*)own_in_.p;
}

template <class K>
const loamx_route_cell* DmRouteT<K>::run(const Cell* d_in, uint32_t nx, uint32_t ny, uint32_t nz, const Config& c, const uint32_t* goals,
                                         uint32_t n_goals, bool want_field, uint64_t stats[6], hipStream_t st) {
  const uint32_t n = nx * ny * nz, tiles = dm_route_tiles<K>(nx) * dm_route_tiles<K>(ny) * dm_route_tiles<K>(nz);
  valid_ = false;
  w_.reserve(n);
  cost_.reserve(n);
  field_.reserve(n);
  dirty_.reserve(2 * (size_t)tiles);
  ctr_.reserve(CTR_WORDS);
  st_.reserve(ST_WORDS / 2);
  d_tup_.reserve(K::DIM * DM_ROUTE_MAX_TUPLES);
  h_tup_.reserve(K::DIM * DM_ROUTE_MAX_TUPLES);
  h_ctr_.reserve(CTR_WORDS + ST_WORDS);
  if (want_field) h_field_.reserve(n);
  memcpy(h_tup_.p, goals, sizeof(uint32_t) * K::DIM * n_goals);
  LX_HIP(hipMemcpyAsync(d_tup_.p, h_tup_.p, sizeof(uint32_t) * K::DIM * n_goals, hipMemcpyHostToDevice, st));
  LX_HIP(hipMemsetAsync(dirty_.p, 0, sizeof(uint32_t) * 2 * (size_t)tiles, st));
  LX_HIP(hipMemsetAsync(st_.p, 0, sizeof(uint32_t) * ST_WORDS, st));
  const dim3 per_cell((n + 255u) / 256u);
  hipLaunchKernelGGL(k_dm_route_weights<K>, per_cell, dim3(256), 0, st, d_in, n, c, w_.p, cost_.p, st_.p);
  hipLaunchKernelGGL(k_dm_route_seed<K>, dim3((n_goals + 255u) / 256u), dim3(256), 0, st, d_tup_.p, n_goals, nx, ny, nz, w_.p, cost_.p,
                     dirty_.p, st_.p);
  LX_HIP(hipGetLastError());
  struct Ops {
    DmRouteT& r;
    uint32_t nx, ny, nz, tiles, conn;
    hipStream_t st;
    void begin(uint32_t) { LX_HIP(hipMemsetAsync(r.ctr_.p, 0, sizeof(uint32_t) * CTR_WORDS, st)); }
    void round(uint64_t, uint32_t read_plane, uint32_t mark_plane, uint32_t slot) {
      K::relax(nx, ny, nz, conn, r.w_.p, r.cost_.p, r.dirty_.p + (size_t)read_plane * tiles, r.dirty_.p + (size_t)mark_plane * tiles,
               r.ctr_.p + 2u * slot, st);
    }
    const RouteSlot* look(uint32_t k) {
      LX_HIP(hipGetLastError());
      store_to_pinned_u32(r.h_ctr_.p, r.ctr_.p, 2u * k, st);
      LX_HIP(hipStreamSynchronize(st));
      return (const RouteSlot*)r.h_ctr_.p;
    }
  } ops{*this, nx, ny, nz, tiles, c.connectivity, st};
  const RouteOutcome o = route_schedule(ops, RoutePlan{batch, (uint64_t)n + 2u});
  if (!o.settled)
    throw Error(LOAMX_E_INTERNAL, std::string(K::NAME) + ": the relaxation did not settle within " + K::CELLS + " + 2 rounds");
  hipLaunchKernelGGL(k_dm_route_next<K>, per_cell, dim3(256), 0, st, nx, ny, nz, c.connectivity, w_.p, cost_.p, field_.p, st_.p);
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

template <class K>
void DmRouteT<K>::trace(const uint32_t* starts, uint32_t n_starts, uint32_t* out, uint32_t capacity, uint32_t* lengths, hipStream_t st) {
  constexpr size_t DIM = K::DIM;
  d_tup_.reserve(DIM * DM_ROUTE_MAX_TUPLES);
  h_tup_.reserve(DIM * DM_ROUTE_MAX_TUPLES);
  d_len_.reserve(DM_ROUTE_MAX_TUPLES);
  d_off_.reserve(DM_ROUTE_MAX_TUPLES);
  h_len_.reserve(DM_ROUTE_MAX_TUPLES);
  h_off_.reserve(DM_ROUTE_MAX_TUPLES);
  memcpy(h_tup_.p, starts, sizeof(uint32_t) * DIM * n_starts);
  LX_HIP(hipMemcpyAsync(d_tup_.p, h_tup_.p, sizeof(uint32_t) * DIM * n_starts, hipMemcpyHostToDevice, st));
  const dim3 per_start((n_starts + 255u) / 256u);
  hipLaunchKernelGGL(k_dm_route_trace<K>, per_start, dim3(256), 0, st, field_.p, nx_, ny_, nz_, d_tup_.p, n_starts, capacity,
                     (const unsigned long long*)nullptr, d_len_.p, (uint32_t*)nullptr);
  LX_HIP(hipGetLastError());
  store_to_pinned_u32(h_len_.p, d_len_.p, n_starts, st);
  LX_HIP(hipStreamSynchronize(st));
  // the routes back to back on the device: start i's min(length, capacity) tuples begin at tuple offsets[i]
  size_t total = 0;
  for (uint32_t i = 0; i < n_starts; i++) {
    h_off_.p[i] = total;
    total += std::min(h_len_.p[i], capacity);
  }
  if (total) {
    d_routes_.reserve(DIM * total);
    h_routes_.reserve(DIM * total);
    LX_HIP(hipMemcpyAsync(d_off_.p, h_off_.p, sizeof(unsigned long long) * n_starts, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dm_route_trace<K>, per_start, dim3(256), 0, st, field_.p, nx_, ny_, nz_, d_tup_.p, n_starts, capacity, d_off_.p,
                       d_len_.p, d_routes_.p);
    LX_HIP(hipGetLastError());
    store_to_pinned_u32(h_routes_.p, d_routes_.p, DIM * total, st);
    LX_HIP(hipStreamSynchronize(st));
  }
  for (uint32_t i = 0; i < n_starts; i++) {
    const size_t m = std::min(h_len_.p[i], capacity);
    if (m) memcpy(out + DIM * capacity * i, h_routes_.p + DIM * (size_t)h_off_.p[i], sizeof(uint32_t) * DIM * m);
    lengths[i] = h_len_.p[i];
  }
}

// each instance is compiled once, in the file of its kind's relax kernel
extern template class DmRouteT<DmRouteGrid>;
extern template class DmRouteT<DmRouteVol>;

// The 2-D route as the callers that know only a grid see it (densemap_frontier.hip): a window is nx x nz.  This run hides the
// engine's and only puts the 1 between; DenseMap::route_on, which serves both kinds, takes a DmRouteT<K>& and so calls the engine's
// run with (nx, 1, nz) itself.  Both spellings end in the one DmRouteT<DmRouteGrid>::run
struct DmRoute : DmRouteT<DmRouteGrid> {
  const loamx_route_cell* run(const loamx_grid_cell* d_cells, uint32_t nx, uint32_t nz, const loamx_grid_route_config& c,
                              const uint32_t* goals_xz, uint32_t n_goals, bool want_field, uint64_t stats[6], hipStream_t st) {
    return DmRouteT::run(d_cells, nx, 1u, nz, c, goals_xz, n_goals, want_field, stats, st);
  }
};
using DmRoute3 = DmRouteT<DmRouteVol>;

// the checks the entry points share on their goals ("goals") and starts ("starts")
template <class K> void dm_route_check_tuples(const uint32_t* tuples, uint32_t n, const char* what) {
  LX_REQUIRE(tuples, std::string(what) + "_" + K::AXES + " is NULL");
  LX_REQUIRE(n >= 1u && n <= DM_ROUTE_MAX_TUPLES, std::string("n_") + what + " must be in [1, 4096]");
}

// The host's walk of next over a field from `start` (include/loamx.h, loamx_grid_route_trace and loamx_route3_trace): the first
// min(length, capacity) tuples to `out`, returns the length.  The walk twice: checked to its end first, so that a field that is not
// one of ours leaves nothing written
template <class K>
uint32_t dm_route_walk(const loamx_route_cell* field, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t* start, uint32_t* out,
                       uint32_t capacity) {
  uint32_t len = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint32_t x, y, z;
    dm_route_get<K>(start, 0u, x, y, z);
    len = 0;
    if (x >= nx || y >= ny || z >= nz) break;
    for (;;) {
      const loamx_route_cell& r = field[((size_t)z * ny + y) * nx + x];
      LX_REQUIRE(r.next <= K::NONE, std::string("field: a next above ") + K::NONE_TEXT);
      if (r.next == K::NONE) {
        LX_REQUIRE(len == 0u, "field: the route ends on a cell that is no goal");
        break;
      }
      if (pass && len < capacity) dm_route_put<K>(out, len, x, y, z);
      len++;
      if (r.next == K::GOAL) break;
      int dx, dy, dz;
      K::move(r.next, dx, dy, dz);
      const uint32_t bx = x + (uint32_t)dx, by = y + (uint32_t)dy, bz = z + (uint32_t)dz;
      LX_REQUIRE(bx < nx && by < ny && bz < nz, "field: a step leaves the window");
      LX_REQUIRE(field[((size_t)bz * ny + by) * nx + bx].cost < r.cost, "field: a step to a cell whose cost is not strictly smaller");
      x = bx;
      y = by;
      z = bz;
    }
  }
  return len;
}

}  // namespace loamx
