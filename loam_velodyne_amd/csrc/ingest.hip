// Raw-sweep ingestion for gfx950 — see ingest.hpp.  The reference walks the points once, sequentially; the only
// order-dependent pieces are (a) the halfPassed flag — it flips at the FIRST kept point whose unwrapped azimuth is more
// than pi past the start and stays set, so it is "index > j*" with j* a min-reduction — and (b) the per-ring push_back,
// i.e. a stable split by ring id: per-workgroup ring histograms, a column scan over the workgroups, and a stable rank
// inside the workgroup (wave ballots per distinct ring + wave-order prefix).
// A sensor model (include/loamx.h, loamx_sensor_model) changes two things only: where a point's ring comes from (classify) and where its
// relTime comes from (classify, IMU need, scatter).  Each source is an argument struct and the kernels are templates over them; the
// reference's mapper is k_raw_classify<BoundsRing, AzimuthTime>, k_raw_imu_need<AzimuthTime>, k_raw_scatter<AzimuthTime>.
#include "ingest.hpp"

namespace loamx {

namespace {

constexpr double PI_D = 3.14159265358979323846;

// atan / atan2 of floats: evaluated in double and rounded (within an ulp of the C library's float versions the
// reference calls, and reproducible)
__device__ inline float atan2_f(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ inline float atan_f(float v) { return (float)atan((double)v); }

// scan start / end orientation, MultiScanRegistration.cpp:165-173
__device__ inline void sweep_oris(const float4* __restrict__ raw, uint32_t n, float& startOri, float& endOri) {
  const float4 a = raw[0], b = raw[n - 1];
  startOri = -atan2_f(a.y, a.x);
  endOri = -atan2_f(b.y, b.x) + 2 * (float)PI_D;
  if ((double)(endOri - startOri) > 3 * PI_D) endOri = (float)((double)endOri - 2 * PI_D);
  else if ((double)(endOri - startOri) < PI_D) endOri = (float)((double)endOri + 2 * PI_D);
}

// :184-205: remapped point and ring id (-1: rejected)
__device__ inline int classify(const float4 r, const MapperParams& M, float& x, float& y, float& z) {
  x = r.y; y = r.z; z = r.x;
  if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return -1;
  if ((double)(x * x + y * y + z * z) < 0.0001) return -1;
  const float angle = atan_f(y / sqrtf(x * x + z * z));
  const int id = (int)((((double)(angle * 180) / PI_D) - (double)M.lower) * (double)M.factor + 0.5);   // getRingForAngle :64-66
  return (id >= (int)M.n_rings || id < 0) ? -1 : id;
}

// the !halfPassed branch of :209-219; returns the unwrapped azimuth, `passes` = this point sets halfPassed
__device__ inline float ori_first_half(float x, float z, float startOri, bool& passes) {
  float ori = -atan2_f(x, z);
  if ((double)ori < (double)startOri - PI_D / 2) ori = (float)((double)ori + 2 * PI_D);
  else if ((double)ori > (double)startOri + PI_D * 3 / 2) ori = (float)((double)ori - 2 * PI_D);
  passes = (double)(ori - startOri) > PI_D;
  return ori;
}
// the halfPassed branch, :220-226
__device__ inline float ori_second_half(float x, float z, float endOri) {
  float ori = -atan2_f(x, z);
  ori = (float)((double)ori + 2 * PI_D);
  if ((double)ori < (double)endOri - PI_D * 3 / 2) ori = (float)((double)ori + 2 * PI_D);
  else if ((double)ori > (double)endOri + PI_D / 2) ori = (float)((double)ori - 2 * PI_D);
  return ori;
}

// scratch: [0] j* (first kept point that sets halfPassed), [1] last kept point, [2] startOri, [3] endOri (float bits)
__global__ void k_raw_init(const float4* __restrict__ raw, uint32_t n, uint32_t* scratch, uint32_t* imu_first, uint32_t H) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) {
    scratch[0] = 0xffffffffu;
    scratch[1] = 0u;
    float startOri, endOri;
    sweep_oris(raw, n, startOri, endOri);
    scratch[2] = __float_as_uint(startOri);
    scratch[3] = __float_as_uint(endOri);
  }
  if (e < H) imu_first[e] = 0xffffffffu;
}

// ---- where relTime comes from (TimeSrc): one argument struct and one rel_time() per source.  The kernels that need relTime are
// templates over the struct, so a trace names the source: k_raw_scatter<AzimuthTime>, k_raw_scatter<FieldTime>.

// TIME_FROM_AZIMUTH: the records and the sweep's scratch words (k_raw_init, k_raw_colscan)
struct AzimuthTime {
  static constexpr int src = TIME_AZIMUTH;
  const float4* raw;
  const uint32_t* sweep;
};
// relTime of kept point i (:209-228)
__device__ inline float rel_time(const AzimuthTime& a, uint32_t i, float scan_period) {
  const float startOri = __uint_as_float(a.sweep[2]), endOri = __uint_as_float(a.sweep[3]);
  const float x = a.raw[i].y, z = a.raw[i].x;   // LOAM frame
  bool passes;
  float ori = ori_first_half(x, z, startOri, passes);
  if (i > a.sweep[0]) ori = ori_second_half(x, z, endOri);   // halfPassed was set by an earlier kept point
  return scan_period * (ori - startOri) / (endOri - startOri);
}

// TIME_FROM_FIELD: t_i of every record (k_sensor_unpack), the sweep's t_ref (k_sns_tref), seconds per unit
struct FieldTime {
  static constexpr int src = TIME_FIELD;
  const double* t;
  const double* tref;
  double scale;
};
__device__ inline float rel_time(const FieldTime& f, uint32_t i, float scan_period) {
  const float rt = (float)((f.t[i] - *f.tref) * f.scale);
  return rt > scan_period ? scan_period : rt;
}

// interpolateIMUStateFor's index search for one point on its own (:135-139): smallest j with dt[j] + relTime <= 0, else H-1
__device__ inline uint32_t imu_need(const ImuTable& I, float relTime) {
  uint32_t lo = 0, hi = I.H - 1;   // dt is decreasing in j
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (I.dt[mid] + (double)relTime > 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// _imuIdx only ever moves forward while the points are walked in firing order: idx(i) = max(idx0, max_{kept j <= i} need(j)).
// k_raw_imu_need records, per history index v, the first kept point that needs at least ... exactly v; the suffix minimum
// over v turns that into "first point that needs >= v", which is non-decreasing in v and binary-searchable per point.
template <class Time>
__global__ __launch_bounds__(256) void k_raw_imu_need(uint32_t n, float scan_period, const int* __restrict__ ring_of, ImuTable I,
                                                      uint32_t* __restrict__ first, Time time) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n && ring_of[i] >= 0;
  const uint32_t v = active ? imu_need(I, rel_time(time, i, scan_period)) : 0u;
  // neighbouring points need the same history index: only the first lane of a run of equal v (it has the run's smallest
  // point index) issues the atomic
  const int lane = threadIdx.x & 63;
  const uint32_t pv = __shfl_up(v, 1, 64);
  const unsigned long long act = __ballot(active);
  const bool head = active && (lane == 0 || pv != v || !((act >> (lane > 0 ? lane - 1 : 0)) & 1ull));
  if (head && v > I.idx0) atomicMin(&first[v], i);
}
// first[v] = min over u >= v (one workgroup; H <= 4096: Hillis-Steele steps over LDS)
__global__ __launch_bounds__(1024) void k_raw_imu_suffix(uint32_t* __restrict__ first, uint32_t H) {
  __shared__ uint32_t a[4096];
  for (uint32_t v = threadIdx.x; v < H; v += blockDim.x) a[v] = first[v];
  __syncthreads();
  for (uint32_t d = 1; d < H; d <<= 1) {
    uint32_t t[4];
    int k = 0;
    for (uint32_t v = threadIdx.x; v < H; v += blockDim.x, k++) t[k] = v + d < H ? min(a[v], a[v + d]) : a[v];
    __syncthreads();
    k = 0;
    for (uint32_t v = threadIdx.x; v < H; v += blockDim.x, k++) a[v] = t[k];
    __syncthreads();
  }
  for (uint32_t v = threadIdx.x; v < H; v += blockDim.x) first[v] = a[v];
}

// Angle(float): cached sin / cos of a float angle (Angle.h:16-30); double-then-round, within an ulp of the host's float libm
struct DAngle { float c, s; };
__device__ inline DAngle dangle(float r) { return {(float)cos((double)r), (float)sin((double)r)}; }
__device__ inline void d_rot_x(float& y, float& z, float c, float s) { const float y0 = y; y = c * y0 - s * z; z = s * y0 + c * z; }
__device__ inline void d_rot_y(float& x, float& z, float c, float s) { const float x0 = x; x = c * x0 + s * z; z = c * z - s * x0; }
__device__ inline void d_rot_z(float& x, float& y, float c, float s) { const float x0 = x; x = c * x0 - s * y; y = s * x0 + c * y; }

// setIMUTransformFor + transformToStartIMU for kept point i (:112-131)
__device__ inline void imu_project(const ImuTable& I, const uint32_t* __restrict__ first, uint32_t i, float relTime, float& x, float& y, float& z,
                                   ImuLast* last_out) {
  // _imuIdx after this point
  uint32_t idx = I.idx0;
  {
    uint32_t lo = I.idx0, hi = I.H - 1;   // largest v in (idx0, H-1] with first[v] <= i
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    idx = lo;
  }
  const double timeDiff = I.dt[idx] + (double)relTime;
  float cur[9];
  if (idx == 0 || timeDiff > 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) cur[k] = I.state[9 * idx + k];
  } else {
    const float ratio = (float)(-timeDiff / I.dstamp[idx]), inv = 1 - ratio;   // IMUState::interpolate(hist[idx], hist[idx-1], ratio)
    const float* a = I.state + 9 * idx;
    const float* b = I.state + 9 * (idx - 1);
    cur[0] = a[0] * inv + b[0] * ratio;
    cur[1] = a[1] * inv + b[1] * ratio;
    if ((double)(a[2] - b[2]) > PI_D) cur[2] = (float)((double)(a[2] * inv) + ((double)b[2] + 2 * PI_D) * (double)ratio);
    else if ((double)(a[2] - b[2]) < -PI_D) cur[2] = (float)((double)(a[2] * inv) + ((double)b[2] - 2 * PI_D) * (double)ratio);
    else cur[2] = a[2] * inv + b[2] * ratio;
#pragma unroll
    for (int k = 3; k < 9; k++) cur[k] = a[k] * inv + b[k] * ratio;
  }
  const float relSweepTime = (float)(I.rel_sweep_base + (double)relTime);
  const float sx = cur[3] - I.start_pos[0] - I.start_vel[0] * relSweepTime;
  const float sy = cur[4] - I.start_pos[1] - I.start_vel[1] * relSweepTime;
  const float sz = cur[5] - I.start_pos[2] - I.start_vel[2] * relSweepTime;
  const DAngle ro = dangle(cur[0]), pi = dangle(cur[1]), ya = dangle(cur[2]);
  d_rot_z(x, y, ro.c, ro.s); d_rot_x(y, z, pi.c, pi.s); d_rot_y(x, z, ya.c, ya.s);   // rotateZXY(roll, pitch, yaw)
  x += sx; y += sy; z += sz;
  d_rot_y(x, z, I.start_c[2], -I.start_s[2]); d_rot_x(y, z, I.start_c[1], -I.start_s[1]); d_rot_z(x, y, I.start_c[0], -I.start_s[0]);   // rotateYXZ(-yaw, -pitch, -roll)
  if (last_out) {
    last_out->roll = cur[0]; last_out->pitch = cur[1]; last_out->yaw = cur[2];
    for (int k = 0; k < 3; k++) { last_out->pos[k] = cur[3 + k]; last_out->vel[k] = cur[6 + k]; }
    last_out->shift[0] = sx; last_out->shift[1] = sy; last_out->shift[2] = sz;
    last_out->idx = idx; last_out->valid = 1u;
  }
}

// ---- where a point's ring comes from (RingSrc): one argument struct per source (each with the ring count, n_rings), so a classify
// instantiation is handed only what its source reads (the 1 KB table travels in the kernel arguments of k_raw_classify<TableRing, ...> alone)
struct BoundsRing : MapperParams {   // RING_FROM_BOUNDS: the reference's linear mapper
  static constexpr int src = RING_BOUNDS;
};
struct TableRing {    // RING_FROM_TABLE: the lasers' elevations (degrees, strictly increasing), max_angle_error_deg
  static constexpr int src = RING_TABLE;
  float table[RawBinner::MAX_RINGS];
  float max_err;
  uint32_t n_rings;
};
struct FieldRing {    // RING_FROM_FIELD: the ring field of every record (k_sensor_unpack)
  static constexpr int src = RING_FIELD;
  const uint32_t* ring;
  uint32_t n_rings;
};

// :184-196 (the first half of classify): remapped point; false = rejected (NaN / zero return)
__device__ inline bool remap_keep(const float4 r, float& x, float& y, float& z) {
  x = r.y; y = r.z; z = r.x;
  if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return false;
  return (double)(x * x + y * y + z * z) >= 0.0001;
}

// RING_FROM_TABLE: the entry of the sorted table `tab` (LDS) nearest to the vertical angle, in double, ties to the smaller index; -1 when
// it is farther than max_err.  deg is taken exactly as classify() takes it.
__device__ inline int ring_from_table(float x, float y, float z, const float* tab, uint32_t nr, float max_err) {
  const float angle = atan_f(y / sqrtf(x * x + z * z));
  const double deg = (double)(angle * 180) / PI_D;
  uint32_t lo = 0, hi = nr;   // first k with tab[k] >= deg: the nearest entry is k or k - 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((double)tab[mid] < deg) lo = mid + 1; else hi = mid;
  }
  uint32_t k = lo < nr ? lo : nr - 1;
  double best = fabs(deg - (double)tab[k]);
  // (rounded distances grow weakly away from deg on either side: a tie with a smaller index can only lie further left)
  while (k > 0 && fabs(deg - (double)tab[k - 1]) <= best) { k--; best = fabs(deg - (double)tab[k]); }
  return best > (double)max_err ? -1 : (int)k;
}

// smallest double of a workgroup of 256 (every thread passes one value; w: 4 doubles of LDS), valid in thread 0
__device__ inline double block_min_256(double t, double* w) {
  for (int d = 32; d >= 1; d >>= 1) t = fmin(t, __shfl_xor(t, d, 64));
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = t;
  __syncthreads();
  return fmin(fmin(w[0], w[1]), fmin(w[2], w[3]));
}

// per workgroup: ring histogram and last kept point, and per time source: TIME_FROM_AZIMUTH the first point that would set halfPassed
// (k_raw_colscan reduces the two index arrays — thousands of atomics on ONE global word per launch serialise for tens of
// microseconds), TIME_FROM_FIELD the smallest time of the kept points (k_sns_tref reduces it to t_ref); a time that is not finite
// rejects the point.  The mapper path is <BoundsRing, AzimuthTime>: no table and no time minimum in LDS, no field read.
template <class Ring, class Time>
__global__ __launch_bounds__(256) void k_raw_classify(const float4* __restrict__ raw, uint32_t n, Ring ring, Time time,
                                                      int* __restrict__ ring_of, uint32_t* __restrict__ blk_cnt,
                                                      uint32_t* __restrict__ blk_first_pass, uint32_t* __restrict__ blk_last_kept,
                                                      double* __restrict__ blk_tmin) {
  __shared__ uint32_t hist[RawBinner::MAX_RINGS];
  __shared__ uint32_t s_first, s_last;
  __shared__ float tab[RawBinner::MAX_RINGS];
  __shared__ double w_tmin[4];
  const uint32_t nr = ring.n_rings;
  if (threadIdx.x == 0) { s_first = 0xffffffffu; s_last = 0u; }
  for (uint32_t r = threadIdx.x; r < nr; r += blockDim.x) {
    hist[r] = 0;
    if constexpr (Ring::src == RING_TABLE) tab[r] = ring.table[r];
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool kept = false, passes = false;
  double t = HUGE_VAL;
  if (i < n) {
    float x, y, z;
    int id;
    if constexpr (Ring::src == RING_BOUNDS) id = classify(raw[i], ring, x, y, z);
    else if (!remap_keep(raw[i], x, y, z)) id = -1;
    else if constexpr (Ring::src == RING_TABLE) id = ring_from_table(x, y, z, tab, nr, ring.max_err);
    else id = ring.ring[i] < nr ? (int)ring.ring[i] : -1;
    if constexpr (Time::src == TIME_FIELD) {
      if (id >= 0) {
        t = time.t[i];
        if (!isfinite(t)) { id = -1; t = HUGE_VAL; }
      }
    }
    ring_of[i] = id;
    if (id >= 0) {
      kept = true;
      atomicAdd(&hist[id], 1u);
      if constexpr (Time::src == TIME_AZIMUTH) (void)ori_first_half(x, z, __uint_as_float(time.sweep[2]), passes);
    }
  }
  // one atomic per wave: the lowest passing lane holds the wave's smallest index, the highest kept lane its largest
  const unsigned long long mp = __ballot(passes), mk = __ballot(kept);
  const int lane = threadIdx.x & 63;
  if (mp && lane == __builtin_ctzll(mp)) atomicMin(&s_first, i);
  if (mk && lane == 63 - __builtin_clzll(mk)) atomicMax(&s_last, i + 1u);   // (+1: 0 = no kept point in this workgroup)
  double tmin = 0.0;
  if constexpr (Time::src == TIME_FIELD) tmin = block_min_256(t, w_tmin);   // (its barrier also orders the LDS atomics above)
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_first_pass[blockIdx.x] = s_first;
    blk_last_kept[blockIdx.x] = s_last;
    if constexpr (Time::src == TIME_FIELD) blk_tmin[blockIdx.x] = tmin;
  }
  for (uint32_t r = threadIdx.x; r < nr; r += blockDim.x) blk_cnt[(size_t)blockIdx.x * nr + r] = hist[r];
}

// one workgroup per ring: exclusive scan of the ring's column of workgroup counts
// (workgroup 0 also reduces the per-workgroup first-pass / last-kept indices into scratch[0] / scratch[1])
__global__ __launch_bounds__(256) void k_raw_colscan(const uint32_t* __restrict__ blk_cnt, uint32_t nblk, uint32_t nrings,
                                                     uint32_t* __restrict__ blk_pre, uint32_t* __restrict__ ring_cnt,
                                                     const uint32_t* __restrict__ blk_first_pass, const uint32_t* __restrict__ blk_last_kept,
                                                     uint32_t* __restrict__ scratch) {
  __shared__ uint32_t sc[256];
  const uint32_t r = blockIdx.x;
  if (r == 0) {
    __shared__ uint32_t s_first, s_last;
    if (threadIdx.x == 0) { s_first = 0xffffffffu; s_last = 0u; }
    __syncthreads();
    uint32_t f = 0xffffffffu, l = 0u;
    for (uint32_t b = threadIdx.x; b < nblk; b += 256) { f = min(f, blk_first_pass[b]); l = max(l, blk_last_kept[b]); }
    atomicMin(&s_first, f);
    atomicMax(&s_last, l);
    __syncthreads();
    if (threadIdx.x == 0) { scratch[0] = s_first; scratch[1] = s_last ? s_last - 1u : 0u; }
  }
  uint32_t base = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += 256) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < nblk ? blk_cnt[(size_t)b * nrings + r] : 0u;
    sc[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {   // Hillis-Steele inclusive scan
      const uint32_t t = threadIdx.x >= d ? sc[threadIdx.x - d] : 0u;
      __syncthreads();
      sc[threadIdx.x] += t;
      __syncthreads();
    }
    if (b < nblk) blk_pre[(size_t)b * nrings + r] = base + sc[threadIdx.x] - v;
    base += sc[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) ring_cnt[r] = base;
}

// stable rank of this lane among the lanes of its wave that hold the same ring id (id < 0: not ranked): one round of ballots per
// distinct ring in the wave; the first lane of every ring leaves the wave's count of it in wave_cnt[ring]
__device__ inline uint32_t wave_rank(int id, uint32_t* wave_cnt) {
  const int lane = threadIdx.x & 63;
  uint32_t rank = 0;
  unsigned long long todo = __ballot(id >= 0);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    const int r0 = __shfl(id, src, 64);
    const unsigned long long m = __ballot(id == r0);
    if (id == r0) {
      rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (lane == src) wave_cnt[r0] = (uint32_t)__popcll(m);
    }
    todo &= ~m;
  }
  return rank;
}

// every kept point to its place: ring offset + the counts of the workgroups before this one + the waves before this one + wave_rank
template <class Time>
__global__ __launch_bounds__(256) void k_raw_scatter(const float4* __restrict__ raw, uint32_t n, uint32_t nr, float scan_period,
                                                     const int* __restrict__ ring_of, const uint32_t* __restrict__ blk_pre,
                                                     const uint32_t* __restrict__ ring_cnt, const uint32_t* __restrict__ sweep,
                                                     float4* __restrict__ out, ImuTable I, const uint32_t* __restrict__ imu_first,
                                                     ImuLast* __restrict__ d_last, Time time) {
  __shared__ uint32_t ring_off[RawBinner::MAX_RINGS];
  __shared__ uint32_t wcnt[4][RawBinner::MAX_RINGS];
  // ring offsets (exclusive scan of the ring totals; <= 256 rings)
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (uint32_t r = 0; r < nr; r++) { ring_off[r] = acc; acc += ring_cnt[r]; }
  }
  for (uint32_t e = threadIdx.x; e < 4 * RawBinner::MAX_RINGS; e += blockDim.x) (&wcnt[0][0])[e] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int wid = threadIdx.x >> 6;
  const int id = i < n ? ring_of[i] : -1;
  uint32_t rank = wave_rank(id, wcnt[wid]);
  __syncthreads();
  if (id < 0) return;
  for (int w = 0; w < wid; w++) rank += wcnt[w][id];
  const uint32_t pos = ring_off[id] + blk_pre[(size_t)blockIdx.x * nr + id] + rank;
  const float4 r = raw[i];
  float x = r.y, y = r.z, z = r.x;
  const float relTime = rel_time(time, i, scan_period);                                         // :228
  if (I.H) imu_project(I, imu_first, i, relTime, x, y, z, i == sweep[1] ? d_last : nullptr);   // :231
  out[pos] = make_float4(x, y, z, (float)id + relTime);                                         // :229
}

// TIME_FROM_FIELD: t_ref = the smallest time of the kept points, over the per-workgroup minima (one workgroup; k_raw_colscan reduces
// the indices the same way)
__global__ __launch_bounds__(256) void k_sns_tref(const double* __restrict__ blk_tmin, uint32_t nblk, double* __restrict__ tref) {
  __shared__ double w[4];
  double t = HUGE_VAL;
  for (uint32_t b = threadIdx.x; b < nblk; b += 256) t = fmin(t, blk_tmin[b]);
  t = block_min_256(t, w);
  if (threadIdx.x == 0) *tref = t;
}
}  // namespace

// raw records (x, y, z float32 at byte offsets 0 / 4 / 8, `stride` bytes apart) -> float4 (x, y, z, 0): the payload crosses PCIe as
// it came and is re-strided on the device
__global__ __launch_bounds__(256) void k_raw_unpack(const char* __restrict__ bytes, uint32_t stride, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = (const float*)(bytes + (size_t)i * stride);
  out[i] = make_float4(r[0], r[1], r[2], 0.f);
}

// sensor records: as k_raw_unpack, plus the ring field (-> uint32) and the time field (-> double) where the model reads them.  Fields are
// read as aligned dwords (stride % 4 == 0, natural alignment inside the record): u8 / u16 are shifted out, an f64 is two dwords.
__device__ inline uint32_t rec_dword(const char* rec, uint32_t off) { return *(const uint32_t*)(rec + (off & ~3u)); }
__global__ __launch_bounds__(256) void k_sensor_unpack(const char* __restrict__ bytes, uint32_t stride, uint32_t n, uint32_t ring_off,
                                                       uint32_t ring_type, uint32_t time_off, uint32_t time_type, float4* __restrict__ out,
                                                       uint32_t* __restrict__ ring, double* __restrict__ time) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* rec = bytes + (size_t)i * stride;
  const float* r = (const float*)rec;
  out[i] = make_float4(r[0], r[1], r[2], 0.f);
  if (ring) {
    const uint32_t w = rec_dword(rec, ring_off);
    ring[i] = ring_type == LOAMX_FIELD_U8 ? (w >> (8 * (ring_off & 3u))) & 0xffu
            : ring_type == LOAMX_FIELD_U16 ? (w >> (8 * (ring_off & 2u))) & 0xffffu : w;
  }
  if (time) {
    const uint32_t w = rec_dword(rec, time_off);
    time[i] = time_type == LOAMX_FIELD_U32 ? (double)w
            : time_type == LOAMX_FIELD_F32 ? (double)__uint_as_float(w)
            : __hiloint2double((int)rec_dword(rec, time_off + 4), (int)w);   // (little endian: the low word first)
  }
}
void unpack_records(const void* d_bytes, uint32_t stride, uint32_t n, const SensorParams& sp, float4* d_out, hipStream_t st) {
  if (!n) return;
  const dim3 grid((n + 255) / 256), block(256);
  if (sp.ring_src != RING_FIELD && sp.time_src != TIME_FIELD)
    hipLaunchKernelGGL(k_raw_unpack, grid, block, 0, st, (const char*)d_bytes, stride, n, d_out);
  else
    hipLaunchKernelGGL(k_sensor_unpack, grid, block, 0, st, (const char*)d_bytes, stride, n, sp.ring_off, sp.ring_type, sp.time_off, sp.time_type,
                       d_out, sp.ring_src == RING_FIELD ? sp.ring_fld : nullptr, sp.time_src == TIME_FIELD ? sp.time_fld : nullptr);
}

static uint32_t field_size(uint32_t type) {
  switch (type) {
    case LOAMX_FIELD_U8: return 1;
    case LOAMX_FIELD_U16: return 2;
    case LOAMX_FIELD_U32: case LOAMX_FIELD_F32: return 4;
    case LOAMX_FIELD_F64: return 8;
    default: return 0;
  }
}
static void check_field(uint32_t off, uint32_t type, uint32_t stride, const char* what) {
  const uint32_t sz = field_size(type);
  if (off % sz) throw Error(LOAMX_E_INVALID, std::string(what) + " field is not naturally aligned in the record");
  if ((uint64_t)off + sz > stride) throw Error(LOAMX_E_INVALID, std::string(what) + " field does not fit inside the record stride");
}

static void check_stride(uint32_t stride) { LX_REQUIRE(stride >= 12 && stride % 4 == 0, "raw stride must be a multiple of 4 and at least 12"); }
static void check_ring_count(uint32_t n_rings) {
  LX_REQUIRE(n_rings >= 1 && n_rings <= RawBinner::MAX_RINGS, "n_scan_rings must be in [1, 256]");
}

void mapper_check(float lower, float upper, uint32_t n_rings, uint32_t stride) {
  check_stride(stride);
  check_ring_count(n_rings);
  LX_REQUIRE(upper != lower, "vertical bounds must differ");
}

void sensor_model_check(const loamx_sensor_model& m, uint32_t stride) {
  check_stride(stride);
  LX_REQUIRE(m.ring_source <= LOAMX_RING_FROM_FIELD, "unknown ring source");
  LX_REQUIRE(m.time_source <= LOAMX_TIME_FROM_FIELD, "unknown time source");
  check_ring_count(m.n_scan_rings);
  if (m.ring_source == LOAMX_RING_FROM_BOUNDS) {   // as loamx_scanreg_process_raw (MultiScanRegistration.cpp:107-127)
    LX_REQUIRE(m.upper_bound_deg > m.lower_bound_deg, "invalid vertical range (upper <= lower)");
    LX_REQUIRE(m.n_scan_rings >= 2, "invalid number of scan rings (n < 2)");
  } else if (m.ring_source == LOAMX_RING_FROM_TABLE) {
    LX_REQUIRE(m.ring_angles_deg, "ring angle table is NULL");
    for (uint32_t k = 0; k < m.n_scan_rings; k++) {
      LX_REQUIRE(std::isfinite(m.ring_angles_deg[k]), "ring angle table holds a value that is not finite");
      LX_REQUIRE(k == 0 || m.ring_angles_deg[k] > m.ring_angles_deg[k - 1], "ring angle table is not strictly increasing");
    }
    LX_REQUIRE(m.max_angle_error_deg > 0, "max_angle_error_deg must be > 0");
  } else {
    LX_REQUIRE(m.ring_type == LOAMX_FIELD_U8 || m.ring_type == LOAMX_FIELD_U16 || m.ring_type == LOAMX_FIELD_U32,
               "unknown ring field type (U8, U16 or U32)");
    check_field(m.ring_offset, m.ring_type, stride, "ring");
  }
  if (m.time_source == LOAMX_TIME_FROM_FIELD) {
    LX_REQUIRE(m.time_type == LOAMX_FIELD_U32 || m.time_type == LOAMX_FIELD_F32 || m.time_type == LOAMX_FIELD_F64,
               "unknown time field type (U32, F32 or F64)");
    check_field(m.time_offset, m.time_type, stride, "time");
    LX_REQUIRE(std::isfinite(m.time_scale) && m.time_scale > 0, "time_scale must be finite and > 0");
  }
}

SensorParams mapper_params(float lower, float upper, uint32_t n_rings) {
  SensorParams sp;
  sp.M = {lower, upper, (float)((int)n_rings - 1) / (upper - lower), n_rings};   // (nScanRings - 1) / (upperBound - lowerBound), :41-50
  return sp;
}

SensorParams sensor_params(const loamx_sensor_model& m) {
  SensorParams sp = mapper_params(m.lower_bound_deg, m.upper_bound_deg, m.n_scan_rings);
  if (m.ring_source != LOAMX_RING_FROM_BOUNDS) sp.M.factor = 0.f;   // (the bounds are not read, and not checked either)
  sp.ring_src = (int)m.ring_source;
  sp.time_src = (int)m.time_source;
  for (uint32_t k = 0; m.ring_source == LOAMX_RING_FROM_TABLE && k < m.n_scan_rings; k++) sp.table[k] = m.ring_angles_deg[k];
  sp.max_err = m.max_angle_error_deg;
  sp.ring_off = m.ring_offset; sp.ring_type = m.ring_type;
  sp.time_off = m.time_offset; sp.time_type = m.time_type;
  sp.time_scale = m.time_scale;
  return sp;
}

void RawBinner::run(const float4* d_raw, uint32_t n, const SensorParams& sp, float scan_period, float4* d_out, uint32_t* d_ring_cnt,
                    const ImuTable* imu, ImuLast* d_last) {
  const uint32_t nr = sp.M.n_rings;
  check_ring_count(nr);
  if (n == 0) {
    LX_HIP(hipMemsetAsync(d_ring_cnt, 0, sizeof(uint32_t) * nr, st_));
    return;
  }
  const dim3 grid((n + 255) / 256), block(256);
  const uint32_t nb = grid.x;
  ring_of_.reserve(n + 1);
  blk_cnt_.reserve((size_t)nb * nr + 1);
  blk_pre_.reserve((size_t)nb * nr + 1);
  blk_idx_.reserve(2 * (size_t)nb + 2);
  scratch_.reserve(8);
  if (sp.time_src == TIME_FIELD) {
    blk_tmin_.reserve((size_t)nb + 1);
    tref_.reserve(1);
  }
  ImuTable I;
  if (imu) I = *imu;
  LX_REQUIRE(I.H <= 4096, "IMU history longer than 4096 states");
  imu_first_.reserve(I.H + 1);
  hipLaunchKernelGGL(k_raw_init, dim3((I.H + 256) / 256), block, 0, st_, d_raw, n, scratch_.p, imu_first_.p, I.H);
  // the launches of one sweep, for the time source `time` (the mapper path is BoundsRing + AzimuthTime)
  auto bin = [&](auto time) {
    using Time = decltype(time);
    auto classify = [&](auto ring) {
      hipLaunchKernelGGL((k_raw_classify<decltype(ring), Time>), grid, block, 0, st_, d_raw, n, ring, time, ring_of_.p, blk_cnt_.p, blk_idx_.p,
                         blk_idx_.p + nb, blk_tmin_.p);
    };
    if (sp.ring_src == RING_BOUNDS) {
      classify(BoundsRing{sp.M});
    } else if (sp.ring_src == RING_TABLE) {
      TableRing tr;
      memcpy(tr.table, sp.table, sizeof(tr.table));
      tr.max_err = sp.max_err;
      tr.n_rings = nr;
      classify(tr);
    } else {
      classify(FieldRing{sp.ring_fld, nr});
    }
    if (Time::src == TIME_FIELD) hipLaunchKernelGGL(k_sns_tref, dim3(1), block, 0, st_, blk_tmin_.p, nb, tref_.p);
    hipLaunchKernelGGL(k_raw_colscan, dim3(nr), block, 0, st_, blk_cnt_.p, nb, nr, blk_pre_.p, d_ring_cnt, blk_idx_.p, blk_idx_.p + nb, scratch_.p);
    if (I.H) {
      hipLaunchKernelGGL(k_raw_imu_need<Time>, grid, block, 0, st_, n, scan_period, ring_of_.p, I, imu_first_.p, time);
      hipLaunchKernelGGL(k_raw_imu_suffix, dim3(1), dim3(1024), 0, st_, imu_first_.p, I.H);
    }
    hipLaunchKernelGGL(k_raw_scatter<Time>, grid, block, 0, st_, d_raw, n, nr, scan_period, ring_of_.p, blk_pre_.p, d_ring_cnt, scratch_.p, d_out, I,
                       imu_first_.p, d_last, time);
  };
  if (sp.time_src == TIME_FIELD) bin(FieldTime{sp.time_fld, tref_.p, sp.time_scale});
  else bin(AzimuthTime{d_raw, scratch_.p});
  LX_HIP(hipGetLastError());
}

}  // namespace loamx
