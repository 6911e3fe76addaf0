// Alignment of a cloud to the dense map's frozen surfel snapshot (include/loamx.h, loamx_densemap_freeze / loamx_densemap_align_*).
//
// The snapshot (densemap.hpp, DmFrozen) is an open-addressing table of 32-byte entries: key, mean, normal.  k_dm_freeze_insert fills it
// once per freeze; after that it is only read.
//
// One Gauss-Newton linearisation is one launch of k_dm_align_step, one point per thread: transform, the point's cell, one or 27
// dependent random probes of the table (the other waves of the CU hide their latency: 68 VGPRs, seven waves per SIMD, no scratch),
// the point-to-plane residual and the 28 fixed-point terms of J^T J, J^T r and r^2.  All 33 words are integers: they are summed in the wave (shuffles), then in the block
// (LDS), and one lane per word adds the block's sum to the global accumulator, so the result depends on no order.  The words come back
// through pinned memory; the 6x6 solve and the pose update are the host's, in double.
//
// k_dm_align_step_many is the same linearisation about many poses at once, a second grid dimension over a table of poses in device
// memory: one launch and one readback per iteration for all the start poses of loamx_densemap_align_many, which runs the Gauss-Newton
// loops of its hypotheses in lockstep.  Both kernels compile from one text (dm_align_step_body.inc), so every word equals the single step's.
//
// Levels (densemap_pyramid.hip builds them): every form reads the snapshot DenseMap::level(align_level) with inv = 1 / level_leaf —
// to the kernels a level is another table and another inv.  loamx_densemap_align_pyramid is the single loop per level, coarse to
// fine, over a cloud staged once through level 0's buffers.
#include "densemap_map.hpp"
#include <algorithm>

namespace loamx {

constexpr int DM_ALIGN_SUMS = 28, DM_ALIGN_COUNTS = 5, DM_ALIGN_WORDS = DM_ALIGN_SUMS + DM_ALIGN_COUNTS;
constexpr float DM_ALIGN_FAR = 1024.0f;          // |a_k| must stay below this
constexpr float DM_ALIGN_HSCALE = 65536.0f;      // 2^16: J_k * J_l
constexpr float DM_ALIGN_GSCALE = 16777216.0f;   // 2^24: J_k * r and r * r

struct DmAlign {
  float R[9], t[3], c[3];
  float inv, max_residual;
  int nb;
};

// one pose of k_dm_align_step_many's table: 64 bytes, so that a table is a whole number of float4 for the pinned-memory fetch
struct DmAlignPose {
  float R[9], t[3], c[3], pad;
};
static_assert(sizeof(DmAlignPose) == 64, "a pose is four float4");

// keys are unique: the first free slot of the probe sequence is claimed and its payload written (read by later launches only)
__global__ __launch_bounds__(256) void k_dm_freeze_insert(const unsigned long long* __restrict__ keys, const float* __restrict__ rec, uint32_t n,
                                                          DmFrozenEntry* __restrict__ tab, uint32_t mask, uint32_t shift,
                                                          unsigned long long* __restrict__ overflow) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  uint32_t h = (uint32_t)dm_hash(key, shift);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    if (atomicCAS(&tab[h].key, DM_EMPTY, key) == DM_EMPTY) {
      const float* r = rec + 6ull * i;
      tab[h].mean[0] = r[0]; tab[h].mean[1] = r[1]; tab[h].mean[2] = r[2];
      tab[h].normal[0] = r[3]; tab[h].normal[1] = r[4]; tab[h].normal[2] = r[5];
      return;
    }
    h = (h + 1u) & mask;
  }
  *overflow = 1ull;   // (cannot happen at a load <= 1/2)
}

__device__ inline unsigned long long dm_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// dm_find's loop on the snapshot's entries: the first 16 bytes of an entry (key, mean x, y) in one load.  false: the key is absent
__device__ inline bool dm_frozen_find(const DmFrozenEntry* tab, uint32_t mask, uint32_t shift, unsigned long long key, uint32_t& slot,
                                      float& mx, float& my) {
  uint32_t h = (uint32_t)dm_hash(key, shift);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    const uint4 w = *(const uint4*)(tab + h);
    const unsigned long long cur = ((unsigned long long)w.y << 32) | w.x;
    if (cur == key) { slot = h; mx = __uint_as_float(w.z); my = __uint_as_float(w.w); return true; }
    if (cur == DM_EMPTY) return false;
    h = (h + 1u) & mask;
  }
  return false;
}

__global__ __launch_bounds__(256) void k_dm_align_step(const float4* __restrict__ pts, uint32_t n, DmAlign A, const DmFrozenEntry* __restrict__ tab,
                                                       uint32_t mask, uint32_t shift, unsigned long long* __restrict__ acc) {
#include "dm_align_step_body.inc"
}

// The same linearisation about gridDim.y poses in one launch: block (x, y) takes the points of block x about poses[y] and adds its 33
// words to acc[33 * y ..].  The pose is uniform in the block, so its 15 floats arrive by scalar loads as the kernel arguments of
// k_dm_align_step do; registers and occupancy are those of the single step, and the poses fill the CUs a small cloud leaves idle
__global__ __launch_bounds__(256) void k_dm_align_step_many(const float4* __restrict__ pts, uint32_t n, const DmAlignPose* __restrict__ poses,
                                                            float inv, float max_residual, int nb, const DmFrozenEntry* __restrict__ tab,
                                                            uint32_t mask, uint32_t shift, unsigned long long* __restrict__ acc_all) {
  const DmAlignPose& P = poses[blockIdx.y];
  DmAlign A;
#pragma unroll
  for (int k = 0; k < 9; k++) A.R[k] = P.R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) { A.t[k] = P.t[k]; A.c[k] = P.c[k]; }
  A.inv = inv;
  A.max_residual = max_residual;
  A.nb = nb;
  unsigned long long* __restrict__ acc = acc_all + (size_t)DM_ALIGN_WORDS * blockIdx.y;
#include "dm_align_step_body.inc"
}

void DmFrozen::drop() {
  if (tab_) (void)hipFree(tab_);
  tab_ = nullptr;
  slots_ = 0;
  count_ = 0;
}

void DmFrozen::build(const unsigned long long* keys, const float* rec, size_t n, hipStream_t st) {
  DevBuf<unsigned long long> d_keys;
  DevBuf<float> d_rec;
  if (n) {
    d_keys.reserve(n);
    d_rec.reserve(6 * n);
    LX_HIP(hipMemcpyAsync(d_keys.p, keys, sizeof(unsigned long long) * n, hipMemcpyHostToDevice, st));
    LX_HIP(hipMemcpyAsync(d_rec.p, rec, sizeof(float) * 6 * n, hipMemcpyHostToDevice, st));
  }
  build_device(d_keys.p, d_rec.p, n, st);   // (blocks: the two blocks are read before they go)
}

void DmFrozen::build_device(const unsigned long long* d_keys, const float* d_rec, size_t n, hipStream_t st) {
  const uint64_t slots = dm_slots_for(1024, n);
  LX_REQUIRE(slots <= (1ull << 31), "dense map: more surfels than the snapshot can index");
  DmFrozenEntry* tab = nullptr;
  LX_HIP(hipMalloc((void**)&tab, sizeof(DmFrozenEntry) * slots));
  try {
    DevBuf<unsigned long long> d_flag;
    d_flag.reserve(1);
    unsigned long long flag = 0ull;
    LX_HIP(hipMemsetAsync(tab, 0xff, sizeof(DmFrozenEntry) * slots, st));   // (every key EMPTY; a free slot's payload is never read)
    LX_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(unsigned long long), st));
    if (n) {
      hipLaunchKernelGGL(k_dm_freeze_insert, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_keys, d_rec, (uint32_t)n, tab,
                         (uint32_t)(slots - 1), 64u - log2u(slots), d_flag.p);
      LX_HIP(hipGetLastError());
    }
    LX_HIP(hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
    LX_HIP(hipStreamSynchronize(st));
    LX_REQUIRE(flag == 0ull, "dense map: snapshot table overflow");
  } catch (...) {
    (void)hipFree(tab);
    throw;
  }
  drop();
  tab_ = tab;
  slots_ = (uint32_t)slots;
  count_ = n;
}

// the entries of the snapshot on the host in ascending key order (include/loamx.h, loamx_densemap_download_frozen); blocks
void DmFrozen::download(std::vector<unsigned long long>& keys, std::vector<float>& rec, hipStream_t st) const {
  LX_REQUIRE(valid(), "nothing is frozen (loamx_densemap_freeze)");
  std::vector<DmFrozenEntry> tab(slots_);
  LX_HIP(hipMemcpyAsync(tab.data(), tab_, sizeof(DmFrozenEntry) * slots_, hipMemcpyDeviceToHost, st));
  LX_HIP(hipStreamSynchronize(st));
  std::vector<uint32_t> idx;
  idx.reserve(count_);
  for (uint32_t i = 0; i < slots_; i++)
    if (tab[i].key != DM_EMPTY) idx.push_back(i);
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return tab[a].key < tab[b].key; });
  keys.resize(idx.size());
  rec.resize(6 * idx.size());
  for (size_t i = 0; i < idx.size(); i++) {
    const DmFrozenEntry& e = tab[idx[i]];
    keys[i] = e.key;
    for (int k = 0; k < 3; k++) { rec[6 * i + k] = e.mean[k]; rec[6 * i + 3 + k] = e.normal[k]; }
  }
}

void DmFrozen::step(const float4* pts, uint32_t n, const float rtc[15], float inv, uint32_t neighbourhood, float max_residual, hipStream_t st,
                    int64_t sums[28], uint64_t counts[5]) {
  LX_REQUIRE(valid(), "nothing is frozen (loamx_densemap_freeze)");
  acc_.reserve(DM_ALIGN_WORDS);
  h_acc_.reserve(DM_ALIGN_WORDS);
  LX_HIP(hipMemsetAsync(acc_.p, 0, sizeof(unsigned long long) * DM_ALIGN_WORDS, st));
  if (n) {
    DmAlign A;
    for (int k = 0; k < 9; k++) A.R[k] = rtc[k];
    for (int k = 0; k < 3; k++) { A.t[k] = rtc[9 + k]; A.c[k] = rtc[12 + k]; }
    A.inv = inv;
    A.max_residual = max_residual;
    A.nb = (int)neighbourhood;
    hipLaunchKernelGGL(k_dm_align_step, dim3((n + 255u) / 256u), dim3(256), 0, st, pts, n, A, tab_, slots_ - 1u, 64u - log2u(slots_), acc_.p);
    LX_HIP(hipGetLastError());
    stats_[0]++;
    stats_[2]++;
  }
  const unsigned long long* w = h_acc_.fetch(acc_.p, DM_ALIGN_WORDS, st);
  LX_HIP(hipStreamSynchronize(st));
  stats_[1]++;
  for (int k = 0; k < DM_ALIGN_SUMS; k++) sums[k] = (int64_t)w[k];
  for (int k = 0; k < DM_ALIGN_COUNTS; k++) counts[k] = w[DM_ALIGN_SUMS + k];
}

float* DmFrozen::pose_table(uint32_t n_poses) {
  h_poses_.reserve(4 * (size_t)n_poses);
  return (float*)h_poses_.p;
}

const unsigned long long* DmFrozen::step_many(const float4* pts, uint32_t n, uint32_t n_poses, float inv, uint32_t neighbourhood,
                                              float max_residual, hipStream_t st) {
  LX_REQUIRE(valid(), "nothing is frozen (loamx_densemap_freeze)");
  LX_REQUIRE(n_poses >= 1u && n_poses <= LOAMX_ALIGN_MAX_POSES && h_poses_.cap >= 4 * (size_t)n_poses, "align: pose table out of range");
  const size_t words = (size_t)DM_ALIGN_WORDS * n_poses;
  acc_.reserve(words);
  h_acc_.reserve(words);
  LX_HIP(hipMemsetAsync(acc_.p, 0, sizeof(unsigned long long) * words, st));
  if (n) {
    d_poses_.reserve(4 * (size_t)n_poses);
    fetch_from_pinned(d_poses_.p, h_poses_.p, 4 * (size_t)n_poses, st);
    // (grid y = n_poses <= 4096 records of the table just fetched; acc_ holds 33 words for each of them)
    hipLaunchKernelGGL(k_dm_align_step_many, dim3((n + 255u) / 256u, n_poses), dim3(256), 0, st, pts, n, (const DmAlignPose*)d_poses_.p, inv,
                       max_residual, (int)neighbourhood, tab_, slots_ - 1u, 64u - log2u(slots_), acc_.p);
    LX_HIP(hipGetLastError());
    stats_[0]++;
    stats_[2] += n_poses;
  }
  const unsigned long long* w = h_acc_.fetch(acc_.p, words, st);
  LX_HIP(hipStreamSynchronize(st));
  stats_[1]++;
  return w;
}

// Eigen-decomposition of a symmetric 6x6 matrix in double by cyclic Jacobi rotations (host_math.h's jacobi_eig3 at n = 6): a is
// overwritten, its diagonal becomes the eigenvalues (unsorted), column k of v the unit eigenvector of a[k][k].  An off-diagonal
// element that is exactly 0 is left alone, so a coordinate the matrix does not touch stays an exact unit axis
static void jacobi_eig6(double a[6][6], double v[6][6]) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 6; i++) {
      diag += std::fabs(a[i][i]);
      for (int j = i + 1; j < 6; j++) off += std::fabs(a[i][j]);
    }
    if (off == 0.0 || off <= 1e-300 + diag * 1e-22) break;
    for (int p = 0; p < 5; p++)
      for (int q = p + 1; q < 6; q++) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, apq = a[p][q];
        a[p][p] -= t * apq;
        a[q][q] += t * apq;
        a[p][q] = a[q][p] = 0.0;
        for (int r = 0; r < 6; r++) {
          if (r == p || r == q) continue;
          const double arp = a[r][p], arq = a[r][q];
          a[r][p] = a[p][r] = c * arp - s * arq;
          a[r][q] = a[q][r] = s * arp + c * arq;
        }
        for (int k = 0; k < 6; k++) {
          const double vp = v[k][p], vq = v[k][q];
          v[k][p] = c * vp - s * vq;
          v[k][q] = s * vp + c * vq;
        }
      }
  }
}

// include/loamx.h, loamx_densemap_align_solve
static void align_solve(const int64_t sums[28], double ratio, double x[6], uint32_t& dropped) {
  double H[6][6], V[6][6], g[6];
  int w = 0;
  for (int k = 0; k < 6; k++)
    for (int l = k; l < 6; l++) H[k][l] = H[l][k] = (double)sums[w++] / 65536.0;
  for (int k = 0; k < 6; k++) g[k] = (double)sums[21 + k] / 16777216.0;
  jacobi_eig6(H, V);
  double lmax = 0.0;
  for (int k = 0; k < 6; k++) lmax = std::max(lmax, H[k][k]);
  dropped = 0;
  for (int k = 0; k < 6; k++) x[k] = 0.0;
  for (int k = 0; k < 6; k++) {
    const double lam = H[k][k];
    if (!(lam > 0.0 && lam > ratio * lmax)) { dropped++; continue; }
    double vg = 0.0;
    for (int i = 0; i < 6; i++) vg += V[i][k] * g[i];
    for (int i = 0; i < 6; i++) x[i] -= V[i][k] * (vg / lam);
  }
}

// R <- exp([w]) R (Rodrigues), row-major
static void rotate_left(double R[9], const double w[3]) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(th2);
  // sin(th)/th and (1 - cos(th))/th^2, by their series where th is small
  const double A = th < 1e-4 ? 1.0 - th2 / 6.0 : std::sin(th) / th, B = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9], out[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double kk = 0.0;
      for (int m = 0; m < 3; m++) kk += K[3 * i + m] * K[3 * m + j];
      E[3 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * kk;
    }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) out[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
  for (int k = 0; k < 9; k++) R[k] = out[k];
}

static loamx_densemap_align_config checked_align_config(const loamx_densemap_align_config* cfg, float leaf) {
  loamx_densemap_align_config c = or_default(cfg, loamx_densemap_align_default_config);
  LX_REQUIRE(c.max_iterations >= 1u && c.max_iterations <= 1000u, "max_iterations must be in [1, 1000]");
  LX_REQUIRE(c.neighbourhood <= 1u, "neighbourhood must be 0 or 1");
  if (c.max_residual == 0.f) c.max_residual = leaf;
  LX_REQUIRE(c.max_residual > 0.f && c.max_residual <= 16.f, "max_residual must be in (0, 16] (0: the leaf)");
  LX_REQUIRE(c.eps_rot >= 0.f && c.eps_trans >= 0.f, "eps_rot and eps_trans must be >= 0");
  LX_REQUIRE(c.degenerate_ratio >= 0.f && c.degenerate_ratio < 1.f, "degenerate_ratio must be in [0, 1)");
  return c;
}

// One hypothesis of the Gauss-Newton loop of include/loamx.h: the host's pose in double, about the centre cc.  begin() and update() are
// the whole arithmetic of the loop, shared by the single alignment and the lockstep loop over many start poses
struct AlignHyp {
  double R[9], t[3];

  // pose_in NULL: identity
  void begin(const double pose_in[12], const double cc[3], loamx_densemap_align_result* out) {
    static const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const double* P = pose_in ? pose_in : ident;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) R[3 * i + j] = P[4 * i + j];
      t[i] = ((R[3 * i] * cc[0] + R[3 * i + 1] * cc[1]) + R[3 * i + 2] * cc[2]) + P[4 * i + 3];
    }
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < 12; k++) out->pose[k] = P[k];
    out->status = 1;
  }
  // the f32 roundings a step takes: R, t, c
  void rtc(const double cc[3], float out[15]) const {
    for (int k = 0; k < 9; k++) out[k] = (float)R[k];
    for (int k = 0; k < 3; k++) { out[9 + k] = (float)t[k]; out[12 + k] = (float)cc[k]; }
  }
  // iteration `it` from the sums of its step (out->counts hold its counts already); true: the loop of this hypothesis has ended
  bool update(uint32_t it, const int64_t sums[28], const double cc[3], const loamx_densemap_align_config& c, loamx_densemap_align_result* out) {
    out->iterations = it + 1;
    const uint64_t matched = out->counts[4];
    out->rms = matched ? std::sqrt(((double)sums[27] / 16777216.0) / (double)matched) : 0.0;
    if (matched < c.min_matched) { out->status = 2; return true; }
    double x[6];
    align_solve(sums, (double)c.degenerate_ratio, x, out->degenerate_dims);
    rotate_left(R, x);
    for (int k = 0; k < 3; k++) t[k] += x[3 + k];
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) out->pose[4 * i + j] = R[3 * i + j];
      out->pose[4 * i + 3] = t[i] - ((R[3 * i] * cc[0] + R[3 * i + 1] * cc[1]) + R[3 * i + 2] * cc[2]);
    }
    const double wn = std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), vn = std::sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (wn < (double)c.eps_rot && vn < (double)c.eps_trans) { out->status = 0; return true; }
    return it + 1 >= c.max_iterations;
  }
};

static void pose_must_be_finite(const double* P, size_t n_words) {
  for (size_t k = 0; k < n_words; k++) LX_REQUIRE(std::isfinite(P[k]), "the pose must be finite");
}

// the loop of include/loamx.h over a cloud that lies on the device, against the snapshot of `level` (c checked with that level's leaf);
// pose_in NULL: identity
static int align_loop(loamx_densemap* h, const float4* pts, uint32_t n, const double pose_in[12], const float centre[3],
                      const loamx_densemap_align_config& c, hipStream_t st, uint32_t level, loamx_densemap_align_result* out) {
  if (pose_in) pose_must_be_finite(pose_in, 12);
  const double cc[3] = {centre ? (double)centre[0] : 0.0, centre ? (double)centre[1] : 0.0, centre ? (double)centre[2] : 0.0};
  AlignHyp hyp;
  hyp.begin(pose_in, cc, out);
  DmFrozen& F = h->d.level(level);
  const float inv = 1.0f / h->d.level_leaf(level);
  for (uint32_t it = 0; it < c.max_iterations; it++) {
    float rtc[15];
    hyp.rtc(cc, rtc);
    int64_t sums[28];
    F.step(pts, n, rtc, inv, c.neighbourhood, c.max_residual, st, sums, out->counts);
    if (hyp.update(it, sums, cc, c, out)) break;
  }
  return LOAMX_OK;
}

// loamx_densemap_align_best
static uint32_t align_best(const loamx_densemap_align_result* r, uint32_t n) {
  uint32_t best = UINT32_MAX;
  for (uint32_t k = 0; k < n; k++) {
    if (r[k].status == 2) continue;
    if (best == UINT32_MAX || r[k].counts[4] > r[best].counts[4] || (r[k].counts[4] == r[best].counts[4] && r[k].rms < r[best].rms)) best = k;
  }
  return best;
}

// The loops of n_poses hypotheses in lockstep (include/loamx.h, loamx_densemap_align_many): per iteration the hypotheses still running,
// compacted in ascending index, go up as one table and come back as 33 words each.  The poses have been checked; poses_in NULL
// (n_poses 1): identity
static int align_many_loop(loamx_densemap* h, const float4* pts, uint32_t n, const double* poses_in, uint32_t n_poses, const float centre[3],
                           const loamx_densemap_align_config& c, hipStream_t st, loamx_densemap_align_result* out, uint32_t* best) {
  const double cc[3] = {centre ? (double)centre[0] : 0.0, centre ? (double)centre[1] : 0.0, centre ? (double)centre[2] : 0.0};
  std::vector<AlignHyp> hyp(n_poses);
  std::vector<uint32_t> active(n_poses);
  for (uint32_t k = 0; k < n_poses; k++) {
    hyp[k].begin(poses_in ? poses_in + 12 * (size_t)k : nullptr, cc, out + k);
    active[k] = k;
  }
  DmFrozen& F = h->d.level(h->d.align_level);
  const float inv = 1.0f / h->d.level_leaf(h->d.align_level);
  for (uint32_t it = 0; it < c.max_iterations && !active.empty(); it++) {
    const uint32_t n_active = (uint32_t)active.size();
    float* table = F.pose_table(n_active);
    for (uint32_t a = 0; a < n_active; a++) {
      hyp[active[a]].rtc(cc, table + 16 * (size_t)a);
      table[16 * (size_t)a + 15] = 0.f;
    }
    const unsigned long long* w = F.step_many(pts, n, n_active, inv, c.neighbourhood, c.max_residual, st);
    size_t kept = 0;
    for (uint32_t a = 0; a < n_active; a++) {
      const uint32_t k = active[a];
      const unsigned long long* wk = w + (size_t)DM_ALIGN_WORDS * a;
      int64_t sums[28];
      for (int j = 0; j < DM_ALIGN_SUMS; j++) sums[j] = (int64_t)wk[j];
      for (int j = 0; j < DM_ALIGN_COUNTS; j++) out[k].counts[j] = wk[DM_ALIGN_SUMS + j];
      if (!hyp[k].update(it, sums, cc, c, out + k)) active[kept++] = k;
    }
    active.resize(kept);
  }
  if (best) *best = align_best(out, n_poses);
  return LOAMX_OK;
}

// The one body of each alignment form takes the cloud as a DenseSource where it lies: a mapper's, a pipeline slot's, a logged call's, or
// a cloud from the host that comes up through the snapshot's stager on the handle's own stream, its centre (NULL: zeros) the origin.
// What differs between the forms and is kept: the single form looks at the pose last, in align_loop, so that a non-finite pose on a
// source without a cloud is SKIPPED; the pyramid looks at it before the cloud, and the many form at its poses first of all.  pose_in
// NULL is the identity here; the host entry points refuse it before they come here.
//
// what the single and the many form check alike; the handle's own stream then runs behind the stream that wrote the cloud,
// unconditionally (an empty cloud too).  false: no cloud
static bool align_source_ready(loamx_densemap* h, const DenseSource& s, const loamx_densemap_align_config* cfg, loamx_densemap_align_config& c,
                               hipStream_t& st) {
  const loamx_densemap_config& mc = h->d.cfg;
  LX_REQUIRE(s.device == mc.device, "the dense map and its source live on different devices");
  c = checked_align_config(cfg, h->d.level_leaf(h->d.align_level));
  LX_REQUIRE(h->d.frozen.valid(), "nothing is frozen (loamx_densemap_freeze)");
  if (!s.has_cloud) return false;
  LX_HIP(hipSetDevice(mc.device));
  st = h->d.own_stream();
  dm_stream_behind(st, s.stream);
  return true;
}

static int align_from_source(loamx_densemap* h, const DenseSource& s, const double pose_in[12], const loamx_densemap_align_config* cfg,
                             loamx_densemap_align_result* out) {
  loamx_densemap_align_config c;
  hipStream_t st = nullptr;
  if (!align_source_ready(h, s, cfg, c, st)) return LOAMX_SKIPPED;
  return align_loop(h, s.points(), s.n, pose_in, s.origin, c, st, h->d.align_level, out);
}

static void not_null(const void* p, const char* name) {
  if (!p) throw Error(LOAMX_E_INVALID, std::string("NULL argument: ") + name);
}

static void check_start_poses(const double* poses_in, uint32_t n_poses) {
  LX_REQUIRE(n_poses >= 1u && n_poses <= LOAMX_ALIGN_MAX_POSES, "n_poses must be in [1, LOAMX_ALIGN_MAX_POSES]");
  if (!poses_in) {
    LX_REQUIRE(n_poses == 1u, "poses_in may be NULL (the identity) only with n_poses == 1");
    return;
  }
  pose_must_be_finite(poses_in, 12 * (size_t)n_poses);
}

static int align_many_from_source(loamx_densemap* h, const DenseSource& s, const double* poses_in, uint32_t n_poses,
                                  const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best) {
  check_start_poses(poses_in, n_poses);
  loamx_densemap_align_config c;
  hipStream_t st = nullptr;
  if (!align_source_ready(h, s, cfg, c, st)) return LOAMX_SKIPPED;
  return align_many_loop(h, s.points(), s.n, poses_in, n_poses, s.origin, c, st, out, best);
}

// Coarse to fine (include/loamx.h, loamx_densemap_align_pyramid): the settings of every level first_level .. 0, each checked with its
// own leaf before anything runs; c[k] belongs to level first_level - k
static void checked_pyramid_configs(loamx_densemap* h, const loamx_densemap_align_config* cfg, uint32_t first_level,
                                    loamx_densemap_align_config c[LOAMX_PYRAMID_MAX_LEVELS]) {
  LX_REQUIRE(h->d.frozen.valid(), "nothing is frozen (loamx_densemap_freeze_pyramid)");
  LX_REQUIRE(first_level < h->d.frozen_levels(), "first_level must be a level that stands (loamx_densemap_frozen_levels)");
  for (uint32_t k = 0; k <= first_level; k++) c[k] = checked_align_config(cfg, h->d.level_leaf(first_level - k));
}
// the loop of align_loop against level first_level, then against each finer one from the pose the level before reported (after status
// 2 that is its last good pose, its input when it had none).  The selected level is neither read nor changed
static int align_pyramid_loop(loamx_densemap* h, const float4* pts, uint32_t n, const double pose_in[12], const float centre[3],
                              const loamx_densemap_align_config* c, hipStream_t st, uint32_t first_level, loamx_densemap_align_result* out) {
  const double* pose = pose_in;
  for (uint32_t k = 0; k <= first_level; k++) {
    align_loop(h, pts, n, pose, centre, c[k], st, first_level - k, out + k);
    pose = out[k].pose;
  }
  return LOAMX_OK;
}
static int align_pyramid_from_source(loamx_densemap* h, const DenseSource& s, const double pose_in[12], const loamx_densemap_align_config* cfg,
                                     uint32_t first_level, loamx_densemap_align_result* out) {
  LX_REQUIRE(s.device == h->d.cfg.device, "the dense map and its source live on different devices");
  loamx_densemap_align_config c[LOAMX_PYRAMID_MAX_LEVELS];
  checked_pyramid_configs(h, cfg, first_level, c);
  if (pose_in) pose_must_be_finite(pose_in, 12);
  if (!s.has_cloud) return LOAMX_SKIPPED;
  LX_HIP(hipSetDevice(h->d.cfg.device));
  hipStream_t st = h->d.own_stream();
  dm_stream_behind(st, s.stream);
  return align_pyramid_loop(h, s.points(), s.n, pose_in, s.origin, c, st, first_level, out);
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_align_default_config(loamx_densemap_align_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_iterations = 20u;
  cfg->neighbourhood = 1u;
  cfg->max_residual = 0.f;
  cfg->min_matched = 50u;
  cfg->eps_rot = 1e-5f;
  cfg->eps_trans = 1e-5f;
  cfg->degenerate_ratio = 1e-4f;
}

int loamx_densemap_align_solve(const int64_t sums[28], float degenerate_ratio, double x[6], uint32_t* dropped) {
  return guard([&]() {
    LX_REQUIRE(sums && x && dropped, "NULL argument");
    LX_REQUIRE(degenerate_ratio >= 0.f && degenerate_ratio < 1.f, "degenerate_ratio must be in [0, 1)");   // (NaN too)
    align_solve(sums, (double)degenerate_ratio, x, *dropped);
    return LOAMX_OK;
  });
}

int loamx_densemap_align_step(loamx_densemap* h, const loamx_cloud* points, const float rtc[15], uint32_t neighbourhood, float max_residual,
                              int64_t sums[28], uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h && points && rtc && sums && counts, "NULL argument");
    LX_REQUIRE(neighbourhood <= 1u, "neighbourhood must be 0 or 1");
    LX_REQUIRE(max_residual > 0.f && max_residual <= 16.f, "max_residual must be in (0, 16]");   // (NaN too)
    DmFrozen& F = h->d.level(h->d.align_level);
    LX_REQUIRE(F.valid(), "nothing is frozen (loamx_densemap_freeze)");
    const DenseSource s = h->d.host_source(h->d.frozen.cloud, points, nullptr);
    F.step(s.points(), s.n, rtc, 1.0f / h->d.level_leaf(h->d.align_level), neighbourhood, max_residual, s.stream, sums, counts);
    return LOAMX_OK;
  });
}

int loamx_densemap_align(loamx_densemap* h, const loamx_cloud* points, const double pose_in[12], const float centre[3],
                         const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out) {
  return guard([&]() {
    LX_REQUIRE(h && points && pose_in && out, "NULL argument");
    return align_from_source(h, h->d.host_source(h->d.frozen.cloud, points, centre), pose_in, cfg, out);
  });
}

int loamx_densemap_align_step_many(loamx_densemap* h, const loamx_cloud* points, const float* rtc, uint32_t n_poses, uint32_t neighbourhood,
                                   float max_residual, int64_t* sums, uint64_t* counts) {
  return guard([&]() {
    not_null(h, "h");
    not_null(points, "points");
    not_null(rtc, "rtc");
    not_null(sums, "sums");
    not_null(counts, "counts");
    LX_REQUIRE(n_poses >= 1u && n_poses <= LOAMX_ALIGN_MAX_POSES, "n_poses must be in [1, LOAMX_ALIGN_MAX_POSES]");
    LX_REQUIRE(neighbourhood <= 1u, "neighbourhood must be 0 or 1");
    LX_REQUIRE(max_residual > 0.f && max_residual <= 16.f, "max_residual must be in (0, 16]");   // (NaN too)
    DmFrozen& F = h->d.level(h->d.align_level);
    LX_REQUIRE(F.valid(), "nothing is frozen (loamx_densemap_freeze)");
    const DenseSource s = h->d.host_source(h->d.frozen.cloud, points, nullptr);
    float* table = F.pose_table(n_poses);
    for (uint32_t k = 0; k < n_poses; k++) {
      for (int j = 0; j < 15; j++) table[16 * (size_t)k + j] = rtc[15 * (size_t)k + j];
      table[16 * (size_t)k + 15] = 0.f;
    }
    const unsigned long long* w = F.step_many(s.points(), s.n, n_poses, 1.0f / h->d.level_leaf(h->d.align_level), neighbourhood, max_residual, s.stream);
    for (uint32_t k = 0; k < n_poses; k++) {
      for (int j = 0; j < DM_ALIGN_SUMS; j++) sums[DM_ALIGN_SUMS * (size_t)k + j] = (int64_t)w[DM_ALIGN_WORDS * (size_t)k + j];
      for (int j = 0; j < DM_ALIGN_COUNTS; j++) counts[DM_ALIGN_COUNTS * (size_t)k + j] = w[DM_ALIGN_WORDS * (size_t)k + DM_ALIGN_SUMS + j];
    }
    return LOAMX_OK;
  });
}

int loamx_densemap_align_many(loamx_densemap* h, const loamx_cloud* points, const double* poses_in, uint32_t n_poses, const float centre[3],
                              const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best) {
  return guard([&]() {
    not_null(h, "h");
    not_null(points, "points");
    not_null(poses_in, "poses_in");
    not_null(out, "out");
    return align_many_from_source(h, h->d.host_source(h->d.frozen.cloud, points, centre), poses_in, n_poses, cfg, out, best);
  });
}

int loamx_densemap_align_many_from_map(loamx_densemap* h, loamx_map* m, const double* poses_in, uint32_t n_poses,
                                       const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best) {
  return guard([&]() {
    not_null(h, "h");
    not_null(m, "m");
    not_null(out, "out");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return align_many_from_source(h, s, poses_in, n_poses, cfg, out, best);
  });
}

int loamx_densemap_align_many_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double* poses_in, uint32_t n_poses,
                                            const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best) {
  return guard([&]() {
    not_null(h, "h");
    not_null(p, "p");
    not_null(out, "out");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return align_many_from_source(h, s, poses_in, n_poses, cfg, out, best);
  });
}

int loamx_densemap_align_best(const loamx_densemap_align_result* results, uint32_t n, uint32_t* best) {
  return guard([&]() {
    not_null(results, "results");
    not_null(best, "best");
    *best = align_best(results, n);
    return LOAMX_OK;
  });
}

int loamx_densemap_get_align_stats(loamx_densemap* h, uint64_t stats[3]) {
  return guard([&]() {
    not_null(h, "h");
    not_null(stats, "stats");
    for (int k = 0; k < 3; k++) stats[k] = 0;
    for (uint32_t l = 0; l <= DenseMap::COARSE_LEVELS; l++)   // (a level's counters outlive its table)
      for (int k = 0; k < 3; k++) stats[k] += h->d.level(l).stats()[k];
    return LOAMX_OK;
  });
}

int loamx_densemap_align_from_map(loamx_densemap* h, loamx_map* m, const double pose_in[12], const loamx_densemap_align_config* cfg,
                                  loamx_densemap_align_result* out) {
  return guard([&]() {
    LX_REQUIRE(h && m && out, "NULL argument");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return align_from_source(h, s, pose_in, cfg, out);
  });
}

int loamx_densemap_align_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double pose_in[12],
                                       const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out) {
  return guard([&]() {
    LX_REQUIRE(h && p && out, "NULL argument");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return align_from_source(h, s, pose_in, cfg, out);
  });
}

// The from_history forms: the cloud is logged call `call` where it lies in the sweep log (DenseMap::history_source waits for the adds),
// its logged origin the centre; everything else is the from_* forms'
int loamx_densemap_align_from_history(loamx_densemap* h, uint64_t call, const double pose_in[12], const loamx_densemap_align_config* cfg,
                                      loamx_densemap_align_result* out) {
  return guard([&]() {
    not_null(h, "h");
    not_null(out, "out");
    DenseSource s;
    h->d.history_source(call, s);
    return align_from_source(h, s, pose_in, cfg, out);
  });
}

int loamx_densemap_align_many_from_history(loamx_densemap* h, uint64_t call, const double* poses_in, uint32_t n_poses,
                                           const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best) {
  return guard([&]() {
    not_null(h, "h");
    not_null(out, "out");
    DenseSource s;
    h->d.history_source(call, s);
    return align_many_from_source(h, s, poses_in, n_poses, cfg, out, best);
  });
}

int loamx_densemap_align_pyramid_from_history(loamx_densemap* h, uint64_t call, const double pose_in[12], const loamx_densemap_align_config* cfg,
                                              uint32_t first_level, loamx_densemap_align_result* out) {
  return guard([&]() {
    not_null(h, "h");
    not_null(out, "out");
    DenseSource s;
    h->d.history_source(call, s);
    return align_pyramid_from_source(h, s, pose_in, cfg, first_level, out);
  });
}

int loamx_densemap_align_select_level(loamx_densemap* h, uint32_t level) {
  return guard([&]() {
    not_null(h, "h");
    LX_REQUIRE(level < h->d.frozen_levels(), "level must be a level that stands (loamx_densemap_frozen_levels)");
    h->d.align_level = level;
    return LOAMX_OK;
  });
}

int loamx_densemap_align_pyramid(loamx_densemap* h, const loamx_cloud* points, const double pose_in[12], const float centre[3],
                                 const loamx_densemap_align_config* cfg, uint32_t first_level, loamx_densemap_align_result* out) {
  return guard([&]() {
    not_null(h, "h");
    not_null(points, "points");
    not_null(pose_in, "pose_in");
    not_null(out, "out");
    // (staged once: every level's step reads it where level 0 put it)
    return align_pyramid_from_source(h, h->d.host_source(h->d.frozen.cloud, points, centre), pose_in, cfg, first_level, out);
  });
}

int loamx_densemap_align_pyramid_from_map(loamx_densemap* h, loamx_map* m, const double pose_in[12], const loamx_densemap_align_config* cfg,
                                          uint32_t first_level, loamx_densemap_align_result* out) {
  return guard([&]() {
    not_null(h, "h");
    not_null(m, "m");
    not_null(out, "out");
    DenseSource s;
    loamx_map_dense_source(m, s);
    return align_pyramid_from_source(h, s, pose_in, cfg, first_level, out);
  });
}

int loamx_densemap_align_pyramid_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double pose_in[12],
                                               const loamx_densemap_align_config* cfg, uint32_t first_level,
                                               loamx_densemap_align_result* out) {
  return guard([&]() {
    not_null(h, "h");
    not_null(p, "p");
    not_null(out, "out");
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return align_pyramid_from_source(h, s, pose_in, cfg, first_level, out);
  });
}

}  // extern "C"
