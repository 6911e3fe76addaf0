// Place recognition in a prior map (include/loamx.h, loamx_place_add_views and the host-only calls around it): the dense map described
// from many virtual view points in one call, so that a map that arrived by load or merge_file, which has no sweeps, gets place entries.
//
// CAST: one launch walks every ray of every view (k_pl_views_cast: grid (ray blocks, origins); a lane walks one ray with the functions
// of densemap_dev.hpp, as k_dm_raycast does, and puts the height of its hit into the workgroup's ring x sector grid in LDS, which is
// merged into the view's entry with integer atomicMax).  No ray, hit or voxel crosses PCIe.  VOXELS: the qualifying voxels' exported
// positions are compacted once (k_pl_views_compact) and described about every origin (k_pl_views_voxels: the body of k_pl_describe
// with the origin from the table).  Behind either: the ring keys of the new entries (k_pl_views_keys).  Cells are maxima and counts are
// integer sums: nothing depends on the order of origins or rays, on the split into calls, on the table's size or on the schedule.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"
#include "place.hpp"

namespace loamx {

// what the walk of a view's rays needs (include/loamx.h, loamx_densemap_raycast): the checked configuration and, with use_rule, the rule
struct PlViewCast {
  float inv;
  double leaf;
  uint32_t max_steps, skip_steps, min_points;
  int use_rule;
  loamx_densemap_static_rule rule;
};

// the exported position of the voxel `key` with the words v = n, Sx, Sy, Sz, in double as the export and k_dm_raycast compute it
__device__ inline void pl_voxel_position(int ix, int iy, int iz, const unsigned long long* v, double leaf, float& x, float& y, float& z) {
  const double den = (double)v[0] * 1048576.0;
  x = (float)(((double)ix + (double)v[1] / den) * leaf);
  y = (float)(((double)iy + (double)v[2] / den) * leaf);
  z = (float)(((double)iz + (double)v[3] / den) * leaf);
}

// Ray blockIdx.x * 256 + lane of view blockIdx.y: from org[view] to org[view] + off[ray] (one f32 addition per component), cast as
// k_dm_raycast casts it (the end's key rule, the walk, max_steps, skip_steps, min_points, the rule, the end cell included); the hit's
// exported position goes through the cell rule of place.hpp about the view's origin into the LDS grid (k_pl_describe's layout: R*S
// cells, u32, rounded up to an even count, then the S boundary directions), and the grid's non-zero cells into entry blockIdx.y of
// `cells`.  No record is written.  Every loop is bounded by an integer: n_steps <= max_steps <= 65536, mask + 1 probes, S sectors.
// rc: [0] not traced, [1] miss, [2] hit, [3] hit in the end cell, [4] cells looked up, summed over all views; ctr[3]: the
// probe-overflow flag of the map's counters
__global__ __launch_bounds__(256) void k_pl_views_cast(const float4* __restrict__ org, const float4* __restrict__ off, uint32_t n_rays, PlViewCast C,
                                                       PlParams P, const float2* __restrict__ table, const unsigned long long* keys,
                                                       const unsigned long long* __restrict__ vals, const uint32_t* __restrict__ aux, uint32_t mask,
                                                       uint32_t shift, unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ rc,
                                                       uint32_t* __restrict__ cells) {
  extern __shared__ uint32_t pl_grid[];
  const int RS = P.R * P.S;
  float2* tab = (float2*)(pl_grid + ((RS + 1) & ~1));
  for (int c = (int)threadIdx.x; c < RS; c += 256) pl_grid[c] = 0u;
  for (int k = (int)threadIdx.x; k < P.S; k += 256) tab[k] = table[k];
  __syncthreads();
  const float4 o = org[blockIdx.y];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t status = 0u, looked = 0u;
  bool overflow = false;
  if (j < n_rays) {
    const float4 d = off[j];
    float4 p;
    p.x = o.x + d.x; p.y = o.y + d.y; p.z = o.z + d.z; p.w = 0.f;
    if (dm_in_key_range(p, C.inv)) {   // (the end's cell)
      DmAxis X, Y, Z;
      const bool okx = dm_axis_setup(o.x, p.x, C.inv, X), oky = dm_axis_setup(o.y, p.y, C.inv, Y), okz = dm_axis_setup(o.z, p.z, C.inv, Z);
      const uint32_t n_steps = X.rem + Y.rem + Z.rem;   // (each < 2^21)
      if (okx && oky && okz && n_steps <= C.max_steps) {
        status = 1u;
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
                  float x, y, z, h = 0.f;
                  pl_voxel_position(X.c, Y.c, Z.c, v, C.leaf, x, y, z);
                  const int cell = pl_cell_of(P, tab, x, y, z, o.x, o.y, o.z, h);
                  if (cell >= 0) atomicMax(&pl_grid[cell], __float_as_uint(h));   // (h > 0: its bits order like the value)
                  status = k < n_steps ? 2u : 3u;
                  break;
                }
              }
            }
            if (k == n_steps) break;
            dm_walk_step(X, Y, Z);   // (k < n_steps: some axis has cells left)
          }
        }
      }
    }
  }
  if (overflow) ctr[3] = 1ull;
  dm_wave_count(&rc[0], j < n_rays && status == 0u);
  dm_wave_count(&rc[1], status == 1u);
  dm_wave_count(&rc[2], status == 2u);
  dm_wave_count(&rc[3], status == 3u);
  dm_wave_sum(&rc[4], looked);
  __syncthreads();
  uint32_t* entry = cells + (size_t)blockIdx.y * RS;
  for (int c = (int)threadIdx.x; c < RS; c += 256) {
    const uint32_t v = pl_grid[c];
    if (v) atomicMax(&entry[c], v);
  }
}

// VOXELS mode, the list: the exported position of every voxel with n >= min_points that the rule, if any, does not call dynamic, in
// any order (a wave takes its places with one atomic on the cursor); out has room for `cap` = the map's voxel count
__global__ __launch_bounds__(256) void k_pl_views_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                          const uint32_t* __restrict__ aux, uint32_t slots, double leaf, uint32_t min_points,
                                                          int use_rule, loamx_densemap_static_rule rule, unsigned long long* __restrict__ cursor,
                                                          float4* __restrict__ out, uint32_t cap) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long key = DM_EMPTY;
  bool q = false;
  if (s < slots) {
    key = keys[s];
    if (key != DM_EMPTY) {
      const unsigned long long cnt = vals[4ull * s];
      q = cnt >= min_points && !(use_rule && dm_dynamic(rule, cnt, aux[2ull * s]));
    }
  }
  const unsigned long long m = __ballot(q);
  if (!m) return;   // (the whole wave)
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __builtin_ctzll(m);
  uint32_t base = 0u;
  if ((int)lane == leader) base = (uint32_t)atomicAdd(cursor, (unsigned long long)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader, 64);
  if (q) {
    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (at < cap) {
      float4 r;
      pl_voxel_position((int)(key & 0x1FFFFFull) - (1 << DM_QBITS), (int)((key >> DM_KBITS) & 0x1FFFFFull) - (1 << DM_QBITS),
                        (int)((key >> (2 * DM_KBITS)) & 0x1FFFFFull) - (1 << DM_QBITS), vals + 4ull * s, leaf, r.x, r.y, r.z);
      r.w = 0.f;
      out[at] = r;
    }
  }
}

// VOXELS mode, the views: k_pl_describe over the *n_ptr listed positions about org[blockIdx.y], into entry blockIdx.y.  The grid covers
// the map's voxel count; a workgroup beyond the list leaves at once
__global__ __launch_bounds__(256) void k_pl_views_voxels(const float4* __restrict__ pts, const unsigned long long* __restrict__ n_ptr, uint32_t cap,
                                                         const float4* __restrict__ org, PlParams P, const float2* __restrict__ table,
                                                         uint32_t* __restrict__ cells) {
  extern __shared__ uint32_t pl_grid[];
  const unsigned long long listed = *n_ptr;
  const uint32_t n = listed < cap ? (uint32_t)listed : cap;
  const uint32_t lo = blockIdx.x * PL_DESCRIBE_SPAN;
  if (lo >= n) return;
  const int RS = P.R * P.S;
  float2* tab = (float2*)(pl_grid + ((RS + 1) & ~1));
  for (int c = (int)threadIdx.x; c < RS; c += 256) pl_grid[c] = 0u;
  for (int k = (int)threadIdx.x; k < P.S; k += 256) tab[k] = table[k];
  __syncthreads();
  const float4 o = org[blockIdx.y];
  const uint32_t hi = n - lo < PL_DESCRIBE_SPAN ? n : lo + PL_DESCRIBE_SPAN;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float4 p = pts[i];
    float h = 0.f;
    const int cell = pl_cell_of(P, tab, p.x, p.y, p.z, o.x, o.y, o.z, h);
    if (cell >= 0) atomicMax(&pl_grid[cell], __float_as_uint(h));
  }
  __syncthreads();
  uint32_t* entry = cells + (size_t)blockIdx.y * RS;
  for (int c = (int)threadIdx.x; c < RS; c += 256) {
    const uint32_t v = pl_grid[c];
    if (v) atomicMax(&entry[c], v);
  }
}

// ring keys of the entries blockIdx.x = 0 .. n - 1 behind `cells`: k_pl_keys per entry, thread i sums row i in ascending k
__global__ __launch_bounds__(64) void k_pl_views_keys(const float* __restrict__ cells, float* __restrict__ key, int R, int S) {
  const int i = (int)threadIdx.x;
  if (i >= R) return;
  const float* row = cells + (size_t)blockIdx.x * R * S + (size_t)i * S;
  float acc = 0.f;
  for (int k = 0; k < S; k++) acc = acc + row[k];
  key[(size_t)blockIdx.x * R + i] = acc / (float)S;
}

DenseMap::TableView DenseMap::table_view() {
  read_counters();
  return TableView{&tab_, ctr_.p, inv_, (double)cfg.leaf, occ_.occ, own_};
}

int PlaceDB::add_views(DenseMap& dm, const float* origins, uint32_t n, const float* offsets, uint32_t n_rays, const loamx_place_view_config& c,
                       const loamx_densemap_static_rule* rule, uint32_t* first_id, uint64_t stats[6]) {
  LX_REQUIRE(dm.cfg.device == cfg.device, "pl and dm live on different devices");
  LX_HIP(hipSetDevice(cfg.device));
  if (cfg.max_entries && (uint64_t)n_ + n > cfg.max_entries) throw Error(LOAMX_E_CAPACITY, "n: max_entries would be passed");
  LX_REQUIRE((uint64_t)n_ + n <= (1u << 30), "place database: more entries than it can index");
  const bool cast = c.mode == LOAMX_PLACE_VIEW_CAST;
  const DenseMap::TableView V = dm.table_view();   // (waits for the map's adds; the map's own stream is idle behind it)
  const DmTable& T = *V.tab;
  hipStream_t st = V.stream;
  // the origins, then the offsets, four floats each, up in one copy
  const size_t n_in = (size_t)n + (cast ? n_rays : 0u);
  h_view_in_.reserve(n_in);
  d_view_in_.reserve(n_in);
  view_ctr_.reserve(6);
  h_view_ctr_.reserve(6);
  for (uint32_t i = 0; i < n; i++) h_view_in_.p[i] = make_float4(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2], 0.f);
  if (cast)
    for (uint32_t j = 0; j < n_rays; j++)
      h_view_in_.p[(size_t)n + j] = make_float4(offsets[3 * (size_t)j], offsets[3 * (size_t)j + 1], offsets[3 * (size_t)j + 2], 0.f);
  const bool list = !cast && V.voxels > 0;
  if (list) d_view_vox_.reserve(V.voxels);
  order_behind(st);
  if (n_ + n > cap_) {   // growth in one step to the power of two that holds the new entries
    uint32_t want = cap_;
    while (want < n_ + n) want *= 2u;
    grow_to(want, st);
  }
  float* cells = desc_ + (size_t)n_ * RS;
  fetch_from_pinned(d_view_in_.p, h_view_in_.p, n_in, st);
  LX_HIP(hipMemsetAsync(cells, 0, sizeof(float) * RS * n, st));
  LX_HIP(hipMemsetAsync(view_ctr_.p, 0, sizeof(unsigned long long) * 6, st));
  const loamx_densemap_static_rule r = rule ? *rule : loamx_densemap_static_rule{0u, 0u, 0u};
  if (cast) {
    PlViewCast C;
    C.inv = V.inv;
    C.leaf = V.leaf;
    C.max_steps = c.max_steps; C.skip_steps = c.skip_steps; C.min_points = c.min_points;
    C.use_rule = rule ? 1 : 0;
    C.rule = r;
    hipLaunchKernelGGL(k_pl_views_cast, dim3((n_rays + 255u) / 256u, n), dim3(256), lds_describe_, st, d_view_in_.p, d_view_in_.p + n, n_rays, C, P_,
                       d_table_.p, T.keys, T.vals, T.aux, T.mask(), T.shift(), V.ctr, view_ctr_.p, (uint32_t*)cells);
  } else if (list) {
    const uint32_t cap = (uint32_t)V.voxels;   // (<= slots / 2 <= 2^30)
    hipLaunchKernelGGL(k_pl_views_compact, dim3((T.slots + 255u) / 256u), dim3(256), 0, st, T.keys, T.vals, T.aux, T.slots, V.leaf, c.min_points,
                       rule ? 1 : 0, r, view_ctr_.p + 5, d_view_vox_.p, cap);
    hipLaunchKernelGGL(k_pl_views_voxels, dim3((cap + PL_DESCRIBE_SPAN - 1u) / PL_DESCRIBE_SPAN, n), dim3(256), lds_describe_, st, d_view_vox_.p,
                       view_ctr_.p + 5, cap, d_view_in_.p, P_, d_table_.p, (uint32_t*)cells);
  }
  hipLaunchKernelGGL(k_pl_views_keys, dim3(n), dim3(64), 0, st, cells, keys_ + (size_t)n_ * R, R, S);
  LX_HIP(hipGetLastError());
  const unsigned long long* w = h_view_ctr_.fetch(view_ctr_.p, 6, st);
  hand_on(st);
  LX_HIP(hipStreamSynchronize(st));
  free_graveyard();   // (st ran behind every add: nothing reads the replaced arrays any more)
  if (first_id) *first_id = n_;
  n_ += n;
  if (stats) {
    stats[0] = n;
    for (int k = 0; k < 5; k++) stats[1 + k] = cast ? w[k] : 0ull;
    if (!cast) stats[1] = w[5];
  }
  return LOAMX_OK;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_place_view_default_config(loamx_place_view_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->mode = LOAMX_PLACE_VIEW_CAST;
  cfg->max_steps = 4096u;
  cfg->skip_steps = 0u;
  cfg->min_points = 1u;
}

int loamx_place_view_rays(uint32_t n_azimuth, const float* elevations, uint32_t n_elevations, float range, float* offsets) {
  return guard([&]() {
    LX_REQUIRE(elevations, "elevations is NULL");
    LX_REQUIRE(offsets, "offsets is NULL");
    LX_REQUIRE(n_azimuth >= 1u, "n_azimuth must be >= 1");
    LX_REQUIRE(n_elevations >= 1u, "n_elevations must be >= 1");
    LX_REQUIRE((uint64_t)n_azimuth * n_elevations <= LOAMX_PLACE_VIEW_MAX_RAYS, "n_azimuth * n_elevations must be <= LOAMX_PLACE_VIEW_MAX_RAYS");
    LX_REQUIRE(std::isfinite(range) && range > 0.f, "range must be finite and positive");
    for (uint32_t e = 0; e < n_elevations; e++) LX_REQUIRE(std::isfinite(elevations[e]), "elevations: entry " + std::to_string(e) + " is not finite");
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (uint32_t e = 0; e < n_elevations; e++) {
      const double el = (double)elevations[e];
      const double ce = cos(el), se = sin(el);
      for (uint32_t a = 0; a < n_azimuth; a++) {
        const double az = two_pi * (double)a / (double)n_azimuth;
        float* o = offsets + 3 * ((size_t)e * n_azimuth + a);
        o[0] = (float)((double)range * ce * sin(az));
        o[1] = (float)((double)range * se);
        o[2] = (float)((double)range * ce * cos(az));
      }
    }
    return LOAMX_OK;
  });
}

int loamx_place_add_views(loamx_place* pl, loamx_densemap* dm, const float* origins, uint32_t n, const float* offsets, uint32_t n_rays,
                          const loamx_place_view_config* cfg, const loamx_densemap_static_rule* rule, uint32_t* first_id, uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(pl, "pl is NULL");
    LX_REQUIRE(dm, "dm is NULL");
    LX_REQUIRE(origins, "origins is NULL");
    const loamx_place_view_config c = or_default(cfg, loamx_place_view_default_config);
    LX_REQUIRE(c.mode == LOAMX_PLACE_VIEW_CAST || c.mode == LOAMX_PLACE_VIEW_VOXELS, "mode must be LOAMX_PLACE_VIEW_CAST or LOAMX_PLACE_VIEW_VOXELS");
    LX_REQUIRE(n >= 1u && n <= LOAMX_PLACE_VIEW_MAX_ORIGINS, "n must be in [1, LOAMX_PLACE_VIEW_MAX_ORIGINS]");
    if (c.mode == LOAMX_PLACE_VIEW_CAST) {
      LX_REQUIRE(offsets, "offsets is NULL");
      LX_REQUIRE(n_rays >= 1u && n_rays <= LOAMX_PLACE_VIEW_MAX_RAYS, "n_rays must be in [1, LOAMX_PLACE_VIEW_MAX_RAYS]");
      LX_REQUIRE(c.max_steps >= 1u && c.max_steps <= 65536u, "max_steps must be in [1, 65536]");
    } else {
      LX_REQUIRE(!offsets, "offsets must be NULL in LOAMX_PLACE_VIEW_VOXELS mode");
      LX_REQUIRE(n_rays == 0u, "n_rays must be 0 in LOAMX_PLACE_VIEW_VOXELS mode");
    }
    LX_REQUIRE(c.min_points >= 1u, "min_points must be >= 1");
    checked_optional_rule(dm, rule);
    for (size_t i = 0; i < 3 * (size_t)n; i++) LX_REQUIRE(std::isfinite(origins[i]), "origins: origin " + std::to_string(i / 3) + " is not finite");
    for (size_t j = 0; j < 3 * (size_t)n_rays; j++) LX_REQUIRE(std::isfinite(offsets[j]), "offsets: offset " + std::to_string(j / 3) + " is not finite");
    return pl->d.add_views(dm->d, origins, n, offsets, n_rays, c, rule, first_id, stats);
  });
}

int loamx_grid_view_origins(const loamx_grid_cell* cells, const loamx_densemap_grid_config* cfg, float leaf, uint32_t stride, uint32_t min_clear2,
                            float sensor_height, float* origins, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(cells, "cells is NULL");
    LX_REQUIRE(cfg, "cfg is NULL");
    LX_REQUIRE(n, "n is NULL");
    LX_REQUIRE(origins || !capacity, "origins is NULL");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    LX_REQUIRE(stride >= 1u, "stride must be >= 1");
    LX_REQUIRE(std::isfinite(sensor_height), "sensor_height must be finite");
    dm_grid_check(*cfg);
    const loamx_densemap_grid_config& g = *cfg;
    uint64_t found = 0;
    for (uint32_t rz = 0; rz < g.nz; rz += stride)
      for (uint32_t rx = 0; rx < g.nx; rx += stride) {
        const loamx_grid_cell& c = cells[(size_t)rz * g.nx + rx];
        if (c.cls != LOAMX_GRID_FREE || c.clear2 < min_clear2) continue;
        if (found < capacity) {
          float* o = origins + 3 * found;
          o[0] = (float)(((double)g.x0 + (double)rx + 0.5) * (double)leaf * (double)g.cell_leaves);
          o[1] = c.elevation + sensor_height;
          o[2] = (float)(((double)g.z0 + (double)rz + 0.5) * (double)leaf * (double)g.cell_leaves);
        }
        found++;
      }
    *n = found;
    return LOAMX_OK;
  });
}

int loamx_place_view_pose(const float view_origin[3], uint32_t shift, int n_sectors, const float query_origin[3], double pose[12]) {
  return guard([&]() {
    LX_REQUIRE(view_origin, "view_origin is NULL");
    LX_REQUIRE(pose, "pose is NULL");
    LX_REQUIRE(n_sectors >= 4 && n_sectors <= PL_MAX_SECTORS, "n_sectors must be in [4, 128]");
    LX_REQUIRE(shift < (uint32_t)n_sectors, "shift must be below n_sectors");
    double v[3], q[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3; a++) {
      LX_REQUIRE(std::isfinite(view_origin[a]), "view_origin must be finite");
      v[a] = (double)view_origin[a];
      if (query_origin) {
        LX_REQUIRE(std::isfinite(query_origin[a]), "query_origin must be finite");
        q[a] = (double)query_origin[a];
      }
    }
    const double two_pi = 2.0 * 3.14159265358979323846;
    const double psi = (double)shift * two_pi / (double)n_sectors;
    const double c = cos(psi), s = sin(psi);
    const double out[12] = {c,   0.0, s, v[0] - (c * q[0] + s * q[2]),
                            0.0, 1.0, 0.0, v[1] - q[1],
                            -s,  0.0, c, v[2] - (c * q[2] - s * q[0])};
    memcpy(pose, out, sizeof(out));
    return LOAMX_OK;
  });
}

}  // extern "C"
