// Dense map, ray casts (include/loamx.h: loamx_densemap_raycast, _from_map, _from_pipeline): the first voxel of the table that each
// ray from an origin to an end point crosses, by the voxel walk of the carve kernel (densemap_dev.hpp) with the end cell included.
// The table is only read.  DmCaster (densemap.hpp) holds the kernel's outputs and their landing blocks; the handle owns one.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"

namespace loamx {

// what a ray cast needs (include/loamx.h, loamx_densemap_raycast): the origin, the checked configuration and, with use_rule, the rule
struct DmCast {
  float inv, ox, oy, oz;
  double leaf;
  uint32_t max_steps, skip_steps, min_points;
  int use_rule;
  loamx_densemap_static_rule rule;
};

// First hit along a ray (include/loamx.h, loamx_densemap_raycast): one ray per lane, from the origin to pts[i], the walk of k_dm_carve
// with the end cell included.  The table is only read: a cell costs one dm_find, a found key one read of its n (and, with a rule, of
// its miss word); the position, in double as the export computes it, and the range are computed once, for the hit, and the record
// leaves as one 40-byte store per lane.  A wave runs as long as its longest ray and stops probing for the lanes that have hit: the
// rays of a sweep or of a range image are neighbours in direction, so the lanes of a wave hit after similar step counts, and the
// other waves of the CU hide the latency of the dependent probes as they do for the carve kernel.  Every loop is bounded by an
// integer: n_steps <= max_steps <= 65536, mask + 1 probes.  rc: [0] not traced, [1] miss, [2] hit, [3] hit in the end cell,
// [4] cells looked up; ctr[3]: the probe-overflow flag of the map's counters
__global__ __launch_bounds__(256) void k_dm_raycast(const float4* __restrict__ pts, uint32_t n, DmCast C, const unsigned long long* keys,
                                                    const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux,
                                                    uint32_t mask, uint32_t shift, unsigned long long* __restrict__ ctr,
                                                    unsigned long long* __restrict__ rc, loamx_ray_hit* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  loamx_ray_hit r;
  r.key = 0ull;
  r.x = r.y = r.z = r.range = 0.f;
  r.n = r.miss = r.steps = 0u;
  r.status = 0u;
  uint32_t looked = 0u;
  bool overflow = false;
  if (i < n) {
    const float4 p = pts[i];
    if (dm_in_key_range(p, C.inv)) {   // (the end's cell)
      DmAxis X, Y, Z;
      const bool okx = dm_axis_setup(C.ox, p.x, C.inv, X), oky = dm_axis_setup(C.oy, p.y, C.inv, Y), okz = dm_axis_setup(C.oz, p.z, C.inv, Z);
      const uint32_t n_steps = X.rem + Y.rem + Z.rem;   // (each < 2^21)
      if (okx && oky && okz && n_steps <= C.max_steps) {
        r.status = 1u;
        // cells k = skip_steps .. n_steps are looked up; cell k is the cell after k steps
        if (C.skip_steps <= n_steps) {
          for (uint32_t k = 0; k <= n_steps; k++) {
            if (k >= C.skip_steps) {
              const unsigned long long key = dm_key(X.c, Y.c, Z.c);
              uint32_t slot = 0u;
              const int f = dm_find(keys, mask, shift, key, slot);
              looked++;
              if (f < 0) overflow = true;
              if (f > 0) {
                const unsigned long long* v = vals + 4ull * slot;
                const unsigned long long cnt = v[0];
                if (cnt >= C.min_points && !(C.use_rule && dm_dynamic(C.rule, cnt, aux[2ull * slot]))) {
                  const double den = (double)cnt * 1048576.0;
                  r.key = key;
                  r.x = (float)(((double)X.c + (double)v[1] / den) * C.leaf);
                  r.y = (float)(((double)Y.c + (double)v[2] / den) * C.leaf);
                  r.z = (float)(((double)Z.c + (double)v[3] / den) * C.leaf);
                  const float dx = p.x - C.ox, dy = p.y - C.oy, dz = p.z - C.oz;
                  const float ex = r.x - C.ox, ey = r.y - C.oy, ez = r.z - C.oz;
                  const float l2 = (dx * dx + dy * dy) + dz * dz;
                  r.range = l2 == 0.f ? 0.f : ((dx * ex + dy * ey) + dz * ez) / sqrtf(l2);
                  r.n = cnt > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt;
                  r.miss = aux ? aux[2ull * slot] : 0u;
                  r.steps = k;
                  r.status = k < n_steps ? 2u : 3u;
                  break;
                }
              }
            }
            if (k == n_steps) break;
            dm_walk_step(X, Y, Z);   // (k < n_steps: some axis has cells left)
          }
        }
        if (r.status == 1u) r.steps = looked;
      }
    }
    if (out) out[i] = r;
  }
  if (overflow) ctr[3] = 1ull;
  dm_wave_count(&rc[0], i < n && r.status == 0u);
  dm_wave_count(&rc[1], r.status == 1u);
  dm_wave_count(&rc[2], r.status == 2u);
  dm_wave_count(&rc[3], r.status == 3u);
  dm_wave_sum(&rc[4], looked);
}

void DmCaster::enqueue(const DmTable& T, unsigned long long* map_ctr, float inv, double leaf, const float4* pts, uint32_t n,
                       const float origin[3], const loamx_densemap_raycast_config& c, const loamx_densemap_static_rule* rule, bool want_hits,
                       hipStream_t st) {
  rc_.reserve(5);
  h_rc_.reserve(5);
  if (want_hits) {   // (both blocks stand before anything is enqueued)
    d_hits_.reserve(n);
    h_hits_.reserve(n);
  }
  DmCast C;
  C.inv = inv;
  C.ox = origin[0]; C.oy = origin[1]; C.oz = origin[2];
  C.leaf = leaf;
  C.max_steps = c.max_steps; C.skip_steps = c.skip_steps; C.min_points = c.min_points;
  C.use_rule = rule ? 1 : 0;
  C.rule = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
  LX_HIP(hipMemsetAsync(rc_.p, 0, sizeof(unsigned long long) * 5, st));
  hipLaunchKernelGGL(k_dm_raycast, dim3((n + 255u) / 256u), dim3(256), 0, st, pts, n, C, T.keys, T.vals, T.aux, T.mask(), T.shift(), map_ctr,
                     rc_.p, want_hits ? d_hits_.p : nullptr);
  LX_HIP(hipGetLastError());
  h_rc_.fetch(rc_.p, 5, st);
  if (want_hits) h_hits_.fetch(d_hits_.p, n, st);
}

void DmCaster::results(uint32_t n, loamx_ray_hit* out, uint64_t counts[5]) const {
  for (int k = 0; k < 5; k++) counts[k] = h_rc_.data()[k];
  if (out) memcpy(out, h_hits_.data(), sizeof(loamx_ray_hit) * n);
}

// include/loamx.h, loamx_densemap_raycast: the rays from s.origin to the points of s where they lie, against the live table, own_
// behind the stream that wrote them (ends from the host go up through the staging block of the adds, on own_, behind the wait for the adds).  capacity is looked
// at after has_cloud: a source without a cloud is SKIPPED whatever the room.  Returns when the counts and, with out, the records are
// back; read_counters() is the wait: it also reports a probe overflow
int DenseMap::raycast(const DenseSource& s, const loamx_densemap_raycast_config& c, const loamx_densemap_static_rule* rule, loamx_ray_hit* out,
                      uint64_t capacity, uint64_t counts[5]) {
  LX_REQUIRE(s.device == cfg.device, "the dense map and its source live on different devices");
  if (!s.has_cloud) return LOAMX_SKIPPED;
  if (out && capacity < s.n) throw Error(LOAMX_E_CAPACITY, "capacity is smaller than the cloud's count");
  LX_HIP(hipSetDevice(cfg.device));
  wait_adds();
  for (int k = 0; k < 5; k++) counts[k] = 0;
  if (!s.n) return LOAMX_OK;
  dm_stream_behind(own_, s.stream);
  caster_.enqueue(tab_, ctr_.p, inv_, (double)cfg.leaf, s.points(), s.n, s.origin, c, rule, out != nullptr, own_);
  read_counters();
  caster_.results(s.n, out, counts);
  return LOAMX_OK;
}

// the settings and the rule of a cast, checked (cfg NULL: the defaults; rule NULL stays NULL: every voxel)
static loamx_densemap_raycast_config checked_raycast(loamx_densemap* h, const loamx_densemap_raycast_config* cfg,
                                                     const loamx_densemap_static_rule* rule, const uint64_t* counts) {
  LX_REQUIRE(counts, "counts is NULL");
  const loamx_densemap_raycast_config c = or_default(cfg, loamx_densemap_raycast_default_config);
  LX_REQUIRE(c.max_steps >= 1u && c.max_steps <= 65536u, "max_steps must be in [1, 65536]");
  LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
  checked_optional_rule(h, rule);
  return c;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_raycast_default_config(loamx_densemap_raycast_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_steps = 4096u;
  cfg->skip_steps = 0u;
  cfg->min_points = 1u;
}

int loamx_densemap_raycast(loamx_densemap* h, const loamx_cloud* ends, const float origin[3], const loamx_densemap_raycast_config* cfg,
                           const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(ends, "ends is NULL");
    LX_REQUIRE(origin, "origin is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    return h->d.raycast(h->d.host_source(h->d.stage, ends, origin), c, rule, out, capacity, counts);
  });
}
int loamx_densemap_raycast_from_map(loamx_densemap* h, loamx_map* m, const loamx_densemap_raycast_config* cfg,
                                    const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(m, "m is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    DenseSource s;
    loamx_map_dense_source(m, s);
    return h->d.raycast(s, c, rule, out, capacity, counts);
  });
}
int loamx_densemap_raycast_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const loamx_densemap_raycast_config* cfg,
                                         const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity,
                                         uint64_t counts[5]) {
  return guard([&]() {
    LX_REQUIRE(h, "h is NULL");
    LX_REQUIRE(p, "p is NULL");
    const loamx_densemap_raycast_config c = checked_raycast(h, cfg, rule, counts);
    DenseSource s;
    loamx_pipeline_dense_source(p, slot, s);
    return h->d.raycast(s, c, rule, out, capacity, counts);
  });
}

}  // extern "C"
