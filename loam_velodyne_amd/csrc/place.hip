// Place recognition (place.hpp, include/loamx.h loamx_place_*): scan-context descriptors of sweeps in HBM, and the search over them.
//
// add: one streaming pass over the cloud (k_pl_describe: a ring x sector grid of maximum heights per workgroup in LDS, merged into the
// entry's slot with integer atomicMax) and the ring key of the new entry (k_pl_keys).  query: one workgroup per candidate compares the
// query with it at every column shift (k_pl_distance); the best n_results by (distance, id) are selected on the device and stored into
// pinned memory (k_pl_select).  With n_candidates > 0 the candidates are first cut to the K nearest ring keys (k_pl_ringkey_topk,
// k_pl_merge).  Every order used is total ((value, id) with distinct ids), and every sum has a fixed order: results are reproducible
// to the bit and equal tests/place_model.py.
#include "place.hpp"
#include <algorithm>

namespace loamx {

// f32 -> u32 with the same order (negative values too: a distance can round to a hair below zero)
__device__ inline uint32_t pl_orderable(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline unsigned long long pl_key(float v, uint32_t id) { return ((unsigned long long)pl_orderable(v) << 32) | id; }

// PL_DESCRIBE_SPAN consecutive points per workgroup.  LDS: R*S cells (u32, rounded up to an even count), then the S boundary directions
__global__ __launch_bounds__(256) void k_pl_describe(const float4* __restrict__ pts, uint32_t n, PlParams P, const float2* __restrict__ table,
                                                     uint32_t* __restrict__ cells) {
  extern __shared__ uint32_t pl_grid[];
  const int RS = P.R * P.S;
  float2* tab = (float2*)(pl_grid + ((RS + 1) & ~1));
  for (int c = (int)threadIdx.x; c < RS; c += 256) pl_grid[c] = 0u;
  for (int k = (int)threadIdx.x; k < P.S; k += 256) tab[k] = table[k];
  __syncthreads();
  const uint32_t lo = blockIdx.x * PL_DESCRIBE_SPAN;
  const uint32_t hi = n - lo < PL_DESCRIBE_SPAN ? n : lo + PL_DESCRIBE_SPAN;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float4 p = pts[i];
    float h = 0.f;
    const int cell = pl_cell_of(P, tab, p.x, p.y, p.z, P.ox, P.oy, P.oz, h);   // (place.hpp: the use rule, the ring, the sector)
    if (cell >= 0) atomicMax(&pl_grid[cell], __float_as_uint(h));   // (h > 0: its bits order like the value)
  }
  __syncthreads();
  for (int c = (int)threadIdx.x; c < RS; c += 256) {
    const uint32_t v = pl_grid[c];
    if (v) atomicMax(&cells[c], v);
  }
}

__global__ __launch_bounds__(256) void k_pl_clear(uint32_t* __restrict__ cells, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cells[i] = 0u;
}

// ring key of one entry: thread i sums row i in ascending k
__global__ __launch_bounds__(64) void k_pl_keys(const float* __restrict__ cells, float* __restrict__ key, int R, int S) {
  const int i = (int)threadIdx.x;
  if (i >= R) return;
  float acc = 0.f;
  for (int k = 0; k < S; k++) acc = acc + cells[i * S + k];
  key[i] = acc / (float)S;
}

__device__ inline float pl_ringkey_dist(const float* __restrict__ rq, const float* __restrict__ rc, int R) {
  float acc = 0.f;
  for (int i = 0; i < R; i++) {
    const float t = rq[i] - rc[i];
    acc = acc + t * t;
  }
  return acc;
}

__device__ inline unsigned long long pl_block_min(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < 4; w++) r = red[w] < r ? red[w] : r;
  __syncthreads();
  return r;
}

// out[0..K) <- the K smallest of keys[0..m) in ascending order, PL_NO_KEY where there are fewer.  The keys are distinct (they end in an
// id) and none is 0, so "the smallest key above the last one taken" needs no removal.  Called by all 256 threads of the workgroup
__device__ inline void pl_take_smallest(const unsigned long long* keys, uint32_t m, uint32_t K, unsigned long long* out, unsigned long long* red) {
  unsigned long long prev = 0ull;
  for (uint32_t t = 0; t < K; t++) {
    unsigned long long best = PL_NO_KEY;
    if (prev != PL_NO_KEY)
      for (uint32_t i = threadIdx.x; i < m; i += 256) {
        const unsigned long long k = keys[i];
        if (k > prev && k < best) best = k;
      }
    best = pl_block_min(best, red);
    if (threadIdx.x == 0) out[t] = best;
    prev = best;
  }
}

// ring-key distance of the entries [0, limit) to the query, and per workgroup (PL_CHUNK entries) its K nearest by (distance, id)
__global__ __launch_bounds__(256) void k_pl_ringkey_topk(const float* __restrict__ keys, const float* __restrict__ rq, uint32_t limit, int R, uint32_t K,
                                                         unsigned long long* __restrict__ part) {
  __shared__ unsigned long long ks[PL_CHUNK];
  __shared__ unsigned long long red[4];
  const uint32_t base = blockIdx.x * PL_CHUNK;
  const uint32_t cnt = limit - base < PL_CHUNK ? limit - base : PL_CHUNK;
  for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
    const uint32_t id = base + i;
    ks[i] = pl_key(pl_ringkey_dist(rq, keys + (size_t)id * R, R), id);
  }
  __syncthreads();
  pl_take_smallest(ks, cnt, K, part + (size_t)blockIdx.x * K, red);
}

// one workgroup: the K smallest of the workgroups' lists -> candidate ids (ascending by (ring-key distance, id))
__global__ __launch_bounds__(256) void k_pl_merge(const unsigned long long* __restrict__ part, uint32_t m, uint32_t K, uint32_t* __restrict__ cand) {
  __shared__ unsigned long long out[PL_MAX_CANDIDATES];
  __shared__ unsigned long long red[4];
  pl_take_smallest(part, m, K, out, red);
  __syncthreads();
  if (threadIdx.x < K) cand[threadIdx.x] = (uint32_t)out[threadIdx.x];
}

// One workgroup per candidate.  LDS (f32): Q[R*S], C[R*S], nq[S], nc[S], V[S*S] (the normalised column products), ds[S]
__global__ __launch_bounds__(256) void k_pl_distance(const float* __restrict__ Qg, const float* __restrict__ rq, const float* __restrict__ desc,
                                                     const float* __restrict__ keys, const uint32_t* __restrict__ cand, int R, int S,
                                                     unsigned long long* __restrict__ dkey, float* __restrict__ dist, uint32_t* __restrict__ shift,
                                                     float* __restrict__ rkd) {
  extern __shared__ float pl_f[];
  const int RS = R * S, t = (int)threadIdx.x;
  float* Q = pl_f;
  float* C = Q + RS;
  float* nq = C + RS;
  float* nc = nq + S;
  float* V = nc + S;
  float* ds = V + S * S;
  const uint32_t id = cand ? cand[blockIdx.x] : blockIdx.x;
  const float* Cg = desc + (size_t)id * RS;
  for (int c = t; c < RS; c += 256) { Q[c] = Qg[c]; C[c] = Cg[c]; }
  __syncthreads();
  if (t < 2 * S) {   // (S <= 128: one thread per column of Q, then of C)
    const float* D = t < S ? Q : C;
    const int j = t < S ? t : t - S;
    float acc = 0.f;
    for (int i = 0; i < R; i++) { const float v = D[i * S + j]; acc = acc + v * v; }
    (t < S ? nq : nc)[j] = sqrtf(acc);
  }
  __syncthreads();
  // every column of Q against every column of C: plain f32 multiplies and adds in ascending i (an MFMA would fuse them)
  for (int p = t; p < S * S; p += 256) {
    const int j = p / S, jc = p - j * S;
    float acc = 0.f;
    for (int i = 0; i < R; i++) acc = acc + Q[i * S + j] * C[i * S + jc];
    V[p] = acc / (nq[j] * nc[jc]);   // (not read where a norm is 0)
  }
  __syncthreads();
  if (t < S) {   // shift t: the diagonal sum in ascending j
    float sum = 0.f;
    int count = 0;
    for (int j = 0; j < S; j++) {
      int jc = j + t;
      jc = jc >= S ? jc - S : jc;
      if (nq[j] > 0.f && nc[jc] > 0.f) { sum = sum + V[j * S + jc]; count++; }
    }
    ds[t] = count ? 1.f - sum / (float)count : 1.f;
  }
  if (t == 255) rkd[id] = pl_ringkey_dist(rq, keys + (size_t)id * R, R);
  __syncthreads();
  if (t == 0) {
    float best = ds[0];
    int bs = 0;
    for (int s = 1; s < S; s++)
      if (ds[s] < best) { best = ds[s]; bs = s; }
    dist[id] = best;
    shift[id] = (uint32_t)bs;
    dkey[blockIdx.x] = pl_key(best, id);
  }
}

// per workgroup (PL_CHUNK keys) its K smallest: the first level of the final selection when there are more than PL_CHUNK candidates
__global__ __launch_bounds__(256) void k_pl_part(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t K, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long red[4];
  const uint32_t base = blockIdx.x * PL_CHUNK;
  const uint32_t cnt = n - base < PL_CHUNK ? n - base : PL_CHUNK;
  pl_take_smallest(keys + base, cnt, K, part + (size_t)blockIdx.x * K, red);
}

// one workgroup: the K best by (distance, id) as match records, stored into the pinned block the host reads behind an event
__global__ __launch_bounds__(256) void k_pl_select(const unsigned long long* __restrict__ keys, uint32_t m, uint32_t K, const float* __restrict__ dist,
                                                   const uint32_t* __restrict__ shift, const float* __restrict__ rkd, uint4* __restrict__ host_out) {
  __shared__ unsigned long long out[LOAMX_PLACE_MAX_RESULTS];
  __shared__ unsigned long long red[4];
  pl_take_smallest(keys, m, K, out, red);
  __syncthreads();
  if (threadIdx.x < K && out[threadIdx.x] != PL_NO_KEY) {
    const uint32_t id = (uint32_t)out[threadIdx.x];
    host_out[threadIdx.x] = make_uint4(id, shift[id], __float_as_uint(dist[id]), __float_as_uint(rkd[id]));
  }
}

PlaceDB::PlaceDB(const loamx_place_config& c) : cfg(c), R(c.n_rings), S(c.n_sectors), RS((size_t)c.n_rings * c.n_sectors) {
  select_device(cfg.device);
  lds_describe_ = sizeof(uint32_t) * ((RS + 1) & ~(size_t)1) + sizeof(float2) * S;
  lds_distance_ = sizeof(float) * (2 * RS + 3 * (size_t)S + (size_t)S * S);
  int lds_max = 0;
  LX_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg.device));
  LX_REQUIRE(lds_distance_ <= (size_t)lds_max, "n_rings x n_sectors needs more LDS per workgroup than this device has");
  if (lds_distance_ > 48u * 1024u) {
    (void)hipFuncSetAttribute((const void*)k_pl_distance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_distance_);
    (void)hipGetLastError();
  }
  LX_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
  LX_HIP(hipEventCreateWithFlags(&ev_last_, hipEventDisableTiming));
  LX_HIP(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
  std::vector<float> tab(2 * (size_t)S);
  place_sector_table(S, tab.data());
  d_table_.reserve(S);
  LX_HIP(hipMemcpy(d_table_.p, tab.data(), sizeof(float2) * S, hipMemcpyHostToDevice));
  q_desc_.reserve(RS);
  q_key_.reserve(R);
  h_res_.reserve(LOAMX_PLACE_MAX_RESULTS);
  alloc_entries(cfg.initial_entries, desc_, keys_);
  cap_ = cfg.initial_entries;
  P_.min2 = cfg.min_range * cfg.min_range;
  P_.max2 = cfg.max_range * cfg.max_range;
  P_.hoff = cfg.height_offset;
  P_.ring_scale = (float)R / cfg.max_range;
  P_.R = R;
  P_.S = S;
}
PlaceDB::~PlaceDB() {
  (void)hipSetDevice(cfg.device);
  (void)hipStreamSynchronize(own_);   // (behind every add: add())
  free_graveyard();
  (void)hipFree(desc_);
  (void)hipFree(keys_);
  (void)hipEventDestroy(ev_last_);
  (void)hipEventDestroy(ev_done_);
  (void)hipStreamDestroy(own_);
  (void)hipGetLastError();   // (whatever the calls above were answered with is not the next caller's error)
}

DenseSource PlaceDB::host_source(const loamx_cloud* c, const float origin[3]) {
  check_cloud(c, false);
  check_origin(origin);
  LX_HIP(hipSetDevice(cfg.device));
  return stage_.source(c, origin, own_, cfg.device);
}

void PlaceDB::grow_to(uint32_t want, hipStream_t st) {
  float *nd = nullptr, *nk = nullptr;
  alloc_entries(want, nd, nk);
  LX_HIP(hipMemcpyAsync(nd, desc_, sizeof(float) * RS * n_, hipMemcpyDeviceToDevice, st));
  LX_HIP(hipMemcpyAsync(nk, keys_, sizeof(float) * R * n_, hipMemcpyDeviceToDevice, st));
  graveyard_.push_back(desc_);
  graveyard_.push_back(keys_);
  desc_ = nd;
  keys_ = nk;
  cap_ = want;
  growths++;
}

// The order is handed on to own_ at once: a source's stream may be destroyed before the database next waits, and an event that was
// last recorded on a destroyed stream must not be waited for, queried or synchronised (the runtime looks at that stream and has
// answered "event last recorded in a capturing stream").  Outside add() and add_views() ev_last_ is an event of own_.
void PlaceDB::hand_on(hipStream_t st) {
  LX_HIP(hipEventRecord(ev_last_, st));
  if (st != own_) {
    LX_HIP(hipStreamWaitEvent(own_, ev_last_, 0));
    LX_HIP(hipEventRecord(ev_last_, own_));
  }
  added_ = true;
}

int PlaceDB::add(const DenseSource& s, uint32_t* id) {
  LX_REQUIRE(s.device == cfg.device, "the place database and its source live on different devices");
  if (!s.has_cloud) return LOAMX_SKIPPED;
  LX_HIP(hipSetDevice(cfg.device));
  if (full()) return LOAMX_E_CAPACITY;
  hipStream_t st = s.stream;
  order_behind(st);
  check_origin(s.origin);
  if (n_ + 1u > cap_) {   // growth by doubling: a device-to-device copy on the stream of this add, the old arrays freed later
    LX_REQUIRE(cap_ <= (1u << 29), "place database: more entries than it can index");
    grow_to(cap_ * 2u, st);
  }
  describe(s.points(), s.n, s.origin, desc_ + (size_t)n_ * RS, keys_ + (size_t)n_ * R, st);
  hand_on(st);
  if (id) *id = n_;
  n_++;
  return LOAMX_OK;
}

int PlaceDB::query_entry(uint32_t id, loamx_place_match* out, uint32_t n_results, uint32_t* n_found) {
  LX_REQUIRE(id < n_, "no such entry");
  LX_HIP(hipSetDevice(cfg.device));
  order_behind(own_);
  return search(desc_ + (size_t)id * RS, keys_ + (size_t)id * R, id, cfg.exclude_recent, out, n_results, n_found);
}

int PlaceDB::query_cloud(const loamx_cloud* c, const float origin[3], uint32_t exclude_recent, loamx_place_match* out, uint32_t n_results,
                         uint32_t* n_found) {
  const DenseSource s = host_source(c, origin);
  order_behind(own_);
  describe(s.points(), s.n, s.origin, q_desc_.p, q_key_.p, own_);
  return search(q_desc_.p, q_key_.p, n_, exclude_recent, out, n_results, n_found);
}

void PlaceDB::get_descriptor(uint32_t id, float* desc, float* key) {
  LX_REQUIRE(id < n_, "no such entry");
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  if (desc) LX_HIP(hipMemcpyAsync(desc, desc_ + (size_t)id * RS, sizeof(float) * RS, hipMemcpyDeviceToHost, own_));
  if (key) LX_HIP(hipMemcpyAsync(key, keys_ + (size_t)id * R, sizeof(float) * R, hipMemcpyDeviceToHost, own_));
  LX_HIP(hipStreamSynchronize(own_));
}

void PlaceDB::reset() {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  LX_HIP(hipStreamSynchronize(own_));
  n_ = 0;
}

void PlaceDB::save(const char* path) {
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  std::vector<float> d(RS * n_), k((size_t)R * n_);
  if (n_) {
    LX_HIP(hipMemcpyAsync(d.data(), desc_, sizeof(float) * d.size(), hipMemcpyDeviceToHost, own_));
    LX_HIP(hipMemcpyAsync(k.data(), keys_, sizeof(float) * k.size(), hipMemcpyDeviceToHost, own_));
  }
  LX_HIP(hipStreamSynchronize(own_));
  FILE* f = fopen(path, "wb");
  LX_REQUIRE(f, std::string("cannot open ") + path + " for writing");
  const uint32_t hdr[5] = {PL_FILE_MAGIC, PL_FILE_VERSION, (uint32_t)R, (uint32_t)S, n_};
  const float par[3] = {cfg.max_range, cfg.min_range, cfg.height_offset};
  bool ok = fwrite(hdr, sizeof(hdr), 1, f) == 1 && fwrite(par, sizeof(par), 1, f) == 1;
  ok = ok && (d.empty() || fwrite(d.data(), sizeof(float), d.size(), f) == d.size());
  ok = ok && (k.empty() || fwrite(k.data(), sizeof(float), k.size(), f) == k.size());
  const bool closed = fclose(f) == 0;
  LX_REQUIRE(ok && closed, std::string("write to ") + path + " failed");
}

void PlaceDB::load(const char* path) {
  FILE* f = fopen(path, "rb");
  LX_REQUIRE(f, std::string("cannot open ") + path);
  uint32_t hdr[5] = {0, 0, 0, 0, 0};
  float par[3] = {0.f, 0.f, 0.f};
  std::vector<float> d, k;
  bool ok = fread(hdr, sizeof(hdr), 1, f) == 1 && fread(par, sizeof(par), 1, f) == 1;
  const bool fits = ok && hdr[0] == PL_FILE_MAGIC && hdr[1] == PL_FILE_VERSION && hdr[2] == (uint32_t)R && hdr[3] == (uint32_t)S &&
                    par[0] == cfg.max_range && par[1] == cfg.min_range && par[2] == cfg.height_offset && hdr[4] <= (1u << 30) &&
                    (!cfg.max_entries || hdr[4] <= cfg.max_entries);
  if (fits) {
    d.resize(RS * hdr[4]);
    k.resize((size_t)R * hdr[4]);
    ok = (d.empty() || fread(d.data(), sizeof(float), d.size(), f) == d.size()) && (k.empty() || fread(k.data(), sizeof(float), k.size(), f) == k.size());
  }
  fclose(f);
  LX_REQUIRE(ok, std::string(path) + " is not a complete place database file");
  LX_REQUIRE(fits, std::string(path) + ": not a place database of this handle's n_rings, n_sectors, ranges and height_offset");
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  LX_HIP(hipStreamSynchronize(own_));
  const uint32_t n = hdr[4];
  if (n > cap_) {
    uint32_t want = cap_;
    while (want < n) want *= 2;
    float *nd = nullptr, *nk = nullptr;
    alloc_entries(want, nd, nk);
    (void)hipFree(desc_);
    (void)hipFree(keys_);
    desc_ = nd;
    keys_ = nk;
    cap_ = want;
  }
  if (n) {
    LX_HIP(hipMemcpy(desc_, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice));
    LX_HIP(hipMemcpy(keys_, k.data(), sizeof(float) * k.size(), hipMemcpyHostToDevice));
  }
  n_ = n;
}

void PlaceDB::alloc_entries(uint32_t cap, float*& d, float*& k) {
  LX_HIP(hipMalloc((void**)&d, sizeof(float) * RS * cap));
  LX_HIP(hipMalloc((void**)&k, sizeof(float) * R * cap));
}
void PlaceDB::free_graveyard() {
  for (void* p : graveyard_) (void)hipFree(p);
  graveyard_.clear();
}
void PlaceDB::wait_adds() {
  if (added_) LX_HIP(hipEventSynchronize(ev_last_));
  stage_.settle();
  free_graveyard();
}
void PlaceDB::describe(const float4* pts, uint32_t n, const float origin[3], float* cells, float* key, hipStream_t st) {
  hipLaunchKernelGGL(k_pl_clear, dim3((uint32_t)((RS + 255) / 256)), dim3(256), 0, st, (uint32_t*)cells, (uint32_t)RS);
  if (n) {
    PlParams P = P_;
    P.ox = origin[0]; P.oy = origin[1]; P.oz = origin[2];
    hipLaunchKernelGGL(k_pl_describe, dim3((n + PL_DESCRIBE_SPAN - 1) / PL_DESCRIBE_SPAN), dim3(256), lds_describe_, st, pts, n, P, d_table_.p,
                       (uint32_t*)cells);
  }
  hipLaunchKernelGGL(k_pl_keys, dim3(1), dim3(64), 0, st, cells, key, R, S);
  LX_HIP(hipGetLastError());
}
int PlaceDB::search(const float* Q, const float* rq, uint32_t q, uint32_t exclude_recent, loamx_place_match* out, uint32_t n_results,
                    uint32_t* n_found) {
  LX_REQUIRE(n_results >= 1 && n_results <= LOAMX_PLACE_MAX_RESULTS, "n_results must be in [1, LOAMX_PLACE_MAX_RESULTS]");
  const uint32_t limit = q > exclude_recent ? std::min(q - exclude_recent, n_) : 0u;   // the candidates are the ids [0, limit)
  uint32_t found = 0;
  if (limit) {
    const uint32_t K = (uint32_t)cfg.n_candidates;
    const bool preselect = K > 0 && limit > K;
    const uint32_t ncand = preselect ? K : limit;
    const uint32_t nwg = (limit + PL_CHUNK - 1) / PL_CHUNK;
    found = std::min(n_results, ncand);
    dist_.reserve(n_);
    rkd_.reserve(n_);
    shift_.reserve(n_);
    dkey_.reserve(ncand);
    part_.reserve((size_t)nwg * std::max(K, (uint32_t)LOAMX_PLACE_MAX_RESULTS));
    const uint32_t* cand = nullptr;
    if (preselect) {
      cand_.reserve(PL_MAX_CANDIDATES);
      hipLaunchKernelGGL(k_pl_ringkey_topk, dim3(nwg), dim3(256), 0, own_, keys_, rq, limit, R, K, part_.p);
      hipLaunchKernelGGL(k_pl_merge, dim3(1), dim3(256), 0, own_, part_.p, nwg * K, K, cand_.p);
      cand = cand_.p;
    }
    hipLaunchKernelGGL(k_pl_distance, dim3(ncand), dim3(256), lds_distance_, own_, Q, rq, desc_, keys_, cand, R, S, dkey_.p, dist_.p, shift_.p,
                       rkd_.p);
    void* d_res = nullptr;
    LX_HIP(hipHostGetDevicePointer(&d_res, h_res_.p, 0));
    if (ncand > PL_CHUNK) {
      const uint32_t nwg2 = (ncand + PL_CHUNK - 1) / PL_CHUNK;
      hipLaunchKernelGGL(k_pl_part, dim3(nwg2), dim3(256), 0, own_, dkey_.p, ncand, found, part_.p);
      hipLaunchKernelGGL(k_pl_select, dim3(1), dim3(256), 0, own_, part_.p, nwg2 * found, found, dist_.p, shift_.p, rkd_.p, (uint4*)d_res);
    } else {
      hipLaunchKernelGGL(k_pl_select, dim3(1), dim3(256), 0, own_, dkey_.p, ncand, found, dist_.p, shift_.p, rkd_.p, (uint4*)d_res);
    }
    LX_HIP(hipGetLastError());
  }
  LX_HIP(hipEventRecord(ev_done_, own_));
  wait_event(ev_done_);
  free_graveyard();   // (own_ ran behind every add: nothing reads the replaced arrays any more)
  for (uint32_t i = 0; i < found; i++) out[i] = h_res_.p[i];
  if (n_found) *n_found = found;
  return LOAMX_OK;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_place_default_config(loamx_place_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->n_rings = 20;
  cfg->n_sectors = 60;
  cfg->max_range = 80.f;
  cfg->min_range = 0.f;
  cfg->height_offset = 2.f;
  cfg->n_candidates = 0;
  cfg->exclude_recent = 50;
  cfg->max_entries = 0;
  cfg->initial_entries = 1024;
  cfg->device = 0;
}

loamx_place* loamx_place_create(const loamx_place_config* cfg) {
  loamx_place* h = nullptr;
  guard([&]() {
    loamx_place_config c;
    if (cfg) c = *cfg; else loamx_place_default_config(&c);
    LX_REQUIRE(c.n_rings >= 1 && c.n_rings <= PL_MAX_RINGS, "n_rings must be in [1, 64]");
    LX_REQUIRE(c.n_sectors >= 4 && c.n_sectors <= PL_MAX_SECTORS, "n_sectors must be in [4, 128]");
    LX_REQUIRE(std::isfinite(c.max_range) && c.max_range > 0.f, "max_range must be positive");
    LX_REQUIRE(std::isfinite(c.min_range) && c.min_range >= 0.f && c.min_range < c.max_range, "min_range must be in [0, max_range)");
    LX_REQUIRE(std::isfinite(c.height_offset), "height_offset must be finite");
    LX_REQUIRE(c.n_candidates >= 0 && c.n_candidates <= PL_MAX_CANDIDATES, "n_candidates must be in [0, 256]");
    LX_REQUIRE(c.initial_entries >= 1u && c.initial_entries <= (1u << 24) && (c.initial_entries & (c.initial_entries - 1u)) == 0u,
               "initial_entries must be a power of two in [1, 2^24]");
    h = new loamx_place(c);
    return LOAMX_OK;
  });
  return h;
}
void loamx_place_destroy(loamx_place* h) { delete h; }

int loamx_place_reset(loamx_place* h) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->d.reset(); return LOAMX_OK; });
}
uint32_t loamx_place_size(loamx_place* h) { return h ? h->d.size() : 0u; }

int loamx_place_sector_table(int n_sectors, float* table) {
  return guard([&]() {
    LX_REQUIRE(table, "NULL argument");
    LX_REQUIRE(n_sectors >= 4 && n_sectors <= PL_MAX_SECTORS, "n_sectors must be in [4, 128]");
    place_sector_table(n_sectors, table);
    return LOAMX_OK;
  });
}
int loamx_place_add(loamx_place* h, const loamx_cloud* points, const float origin[3], uint32_t* id) {
  return guard([&]() {
    LX_REQUIRE(h && points && origin, "NULL argument");
    return h->d.add(h->d.host_source(points, origin), id);
  });
}
int loamx_place_add_from_map(loamx_place* h, loamx_map* m, uint32_t* id) {
  return guard([&]() {
    LX_REQUIRE(h && m, "NULL argument");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.add(s, id);
  });
}
int loamx_place_add_from_pipeline(loamx_place* h, loamx_pipeline* p, uint32_t slot, uint32_t* id) {
  return guard([&]() {
    LX_REQUIRE(h && p, "NULL argument");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.add(s, id);
  });
}
int loamx_place_query_entry(loamx_place* h, uint32_t id, loamx_place_match* matches, uint32_t n_results, uint32_t* n_found) {
  return guard([&]() {
    LX_REQUIRE(h && matches, "NULL argument");
    return h->d.query_entry(id, matches, n_results, n_found);
  });
}
int loamx_place_query(loamx_place* h, const loamx_cloud* points, const float origin[3], uint32_t exclude_recent, loamx_place_match* matches,
                      uint32_t n_results, uint32_t* n_found) {
  return guard([&]() {
    LX_REQUIRE(h && points && origin && matches, "NULL argument");
    return h->d.query_cloud(points, origin, exclude_recent, matches, n_results, n_found);
  });
}
int loamx_place_get_descriptor(loamx_place* h, uint32_t id, float* desc, float* ring_key) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    h->d.get_descriptor(id, desc, ring_key);
    return LOAMX_OK;
  });
}
int loamx_place_save(loamx_place* h, const char* path) {
  return guard([&]() { LX_REQUIRE(h && path, "NULL argument"); h->d.save(path); return LOAMX_OK; });
}
int loamx_place_load(loamx_place* h, const char* path) {
  return guard([&]() { LX_REQUIRE(h && path, "NULL argument"); h->d.load(path); return LOAMX_OK; });
}

// test / bench hook (not in include/loamx.h): how often the table of entries has doubled
uint64_t loamx_place_growths(loamx_place* h) { return h ? h->d.growths : 0; }

}  // extern "C"
