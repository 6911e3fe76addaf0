// Dense map, exports (include/loamx.h: loamx_densemap_download ..., save_pcd ..., the surfel calls, freeze): the voxels of a snapshot
// (DenseMap::snapshot, densemap.hip) on the host as records, miss words, moment words or surfels, in ascending key order, with or
// without the voxels a rule calls dynamic; the PCD files of the records and of the surfels; and the frozen snapshot, which is the
// surfel export uploaded into the table that densemap_align.hip reads.  No kernel of its own.
#include "densemap_map.hpp"
#include "host_math.h"

namespace loamx {

// the exported position of a voxel (include/loamx.h): its indices and its words n, Sx, Sy, Sz; f64 arithmetic, one f32 rounding
static void dm_position(double leaf, const long long ia[3], const unsigned long long* v4, float out[3]) {
  const double cnt = (double)v4[0], qs = (double)(1u << DM_QBITS);
  for (int a = 0; a < 3; a++) out[a] = (float)(((double)ia[a] + (double)v4[1 + a] / (cnt * qs)) * leaf);
}

// the surfel of a voxel (include/loamx.h): the scatter n*M_ab - S_a*S_b as an exact integer, the rest in double
void dm_surfel(double leaf, const long long ia[3], const unsigned long long* v4, const unsigned long long* m9,
               const loamx_densemap_surfel_config& c, int axes, loamx_surfel& out) {
  typedef __int128 i128;
  float p[3];
  dm_position(leaf, ia, v4, p);
  double nrm[3] = {0.0, 0.0, 0.0}, curv = 0.0;
  const unsigned long long n = v4[0];
  static const int A[6] = {0, 1, 2, 0, 0, 1}, B[6] = {0, 1, 2, 1, 2, 2};   // Mxx, Myy, Mzz, Mxy, Mxz, Myz
  i128 N[6];
  for (int k = 0; k < 6; k++) N[k] = (i128)n * (i128)m9[k] - (i128)v4[1 + A[k]] * (i128)v4[1 + B[k]];
  if (n >= c.min_points && N[0] + N[1] + N[2] > 0) {
    const double nn = (double)n * (double)n;
    double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, w[3], v[3][3];
    for (int k = 0; k < 6; k++) a[A[k]][B[k]] = a[B[k]][A[k]] = (double)N[k] / nn;
    jacobi_eig3(a, w, v);
    if (w[1] >= (double)c.min_planar_ratio * w[2]) {
      const double e[3] = {v[0][0], v[1][0], v[2][0]};
      const double dot = (e[0] * (double)(long long)m9[6] + e[1] * (double)(long long)m9[7]) + e[2] * (double)(long long)m9[8];
      bool flip = dot > 0.0;
      if (dot == 0.0) {
        const double first = e[0] != 0.0 ? e[0] : (e[1] != 0.0 ? e[1] : e[2]);
        flip = first < 0.0;
      }
      for (int k = 0; k < 3; k++) nrm[k] = (flip ? -e[k] : e[k]) + 0.0;   // (+ 0.0: no negative zero in the output)
      curv = w[0] / ((w[0] + w[1]) + w[2]);
    }
  }
  const int o[3] = {axes == 1 ? 2 : 0, axes == 1 ? 0 : 1, axes == 1 ? 1 : 2};   // (sensor axes: x_s = z, y_s = x, z_s = y)
  out.x = p[o[0]]; out.y = p[o[1]]; out.z = p[o[2]];
  out.intensity = (float)(double)n;
  out.normal_x = (float)nrm[o[0]]; out.normal_y = (float)nrm[o[1]]; out.normal_z = (float)nrm[o[2]];
  out.curvature = (float)curv;
}

void DenseMap::records(std::vector<float4>& out, int axes, const loamx_densemap_static_rule* rule, const DmWindow* W) {
  Snapshot S;
  if (W) select(*W, &S, false, nullptr); else snapshot(S);
  out.clear();
  out.reserve(S.idx.size());
  const double leaf = (double)cfg.leaf;
  for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
    const double cnt = (double)S.v[4 * j];
    float v[3];
    dm_position(leaf, ia, &S.v[4 * j], v);
    out.push_back(axes == 1 ? make_float4(v[2], v[0], v[1], (float)cnt) : make_float4(v[0], v[1], v[2], (float)cnt));
  });
}

void DenseMap::misses(std::vector<uint32_t>& out) {
  Snapshot S;
  snapshot(S);
  out.clear();
  out.reserve(S.idx.size());
  for_each_voxel(S, nullptr, [&](size_t j, const long long*) { out.push_back(S.miss[j]); });
}

void DenseMap::moment_words(std::vector<unsigned long long>& out) {
  Snapshot S;
  snapshot(S, true);
  out.clear();
  out.reserve(DM_MOM_WORDS * S.idx.size());
  for_each_voxel(S, nullptr, [&](size_t j, const long long*) { out.insert(out.end(), &S.mom[DM_MOM_WORDS * j], &S.mom[DM_MOM_WORDS * j] + DM_MOM_WORDS); });
}

void DenseMap::surfels(std::vector<loamx_surfel>& out, int axes, const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule) {
  Snapshot S;
  snapshot(S, true);
  out.clear();
  out.reserve(S.idx.size());
  const double leaf = (double)cfg.leaf;
  for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
    loamx_surfel s;
    dm_surfel(leaf, ia, &S.v[4 * j], &S.mom[DM_MOM_WORDS * j], sc, axes, s);
    out.push_back(s);
  });
}

uint64_t DenseMap::freeze(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule) {
  Snapshot S;
  snapshot(S, true);
  std::vector<unsigned long long> keys;
  std::vector<float> rec;
  const double leaf = (double)cfg.leaf;
  for_each_voxel(S, rule, [&](size_t j, const long long ia[3]) {
    loamx_surfel s;
    dm_surfel(leaf, ia, &S.v[4 * j], &S.mom[DM_MOM_WORDS * j], sc, 0, s);
    if (s.normal_x == 0.f && s.normal_y == 0.f && s.normal_z == 0.f) return;
    keys.push_back(S.k[j]);
    const float six[6] = {s.x, s.y, s.z, s.normal_x, s.normal_y, s.normal_z};
    rec.insert(rec.end(), six, six + 6);
  });
  frozen.build(keys.data(), rec.data(), keys.size(), own_);
  drop_coarse();
  return frozen.size();
}

// a binary PCD file of n records of rec_bytes each; fields: the header's FIELDS, SIZE, TYPE and COUNT lines
static void write_pcd(const char* path, const char* fields, const void* rec, size_t rec_bytes, size_t n) {
  FILE* f = fopen(path, "wb");
  LX_REQUIRE(f, std::string("cannot open ") + path + " for writing");
  const int hl = fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n%sWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n",
                         fields, n, n);
  const bool ok = hl > 0 && (n == 0 || fwrite(rec, rec_bytes, n, f) == n);
  const bool closed = fclose(f) == 0;
  LX_REQUIRE(ok && closed, std::string("write to ") + path + " failed");
}
static void write_pcd_records(const char* path, const std::vector<float4>& rec) {
  write_pcd(path, "FIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n", rec.data(), sizeof(float4), rec.size());
}

static void checked_axes(int axes) { LX_REQUIRE(axes == 0 || axes == 1, "axes must be 0 (LOAM frame) or 1 (sensor axes)"); }

// the records of a download or save_pcd call behind its NULL check.  is_static (the *_static forms): without the voxels that the
// checked rule (NULL: the default rule) calls dynamic, which needs carving.  out: the download's cloud, checked where it was
static void records_of_call(loamx_densemap* h, int axes, bool is_static, const loamx_densemap_static_rule* rule, const loamx_cloud* out,
                            std::vector<float4>& rec) {
  checked_axes(axes);
  loamx_densemap_static_rule r;
  if (is_static) {
    r = checked_rule(rule);
    LX_REQUIRE_CARVING(h);
  }
  if (out) check_cloud(out, false);
  h->d.records(rec, axes, is_static ? &r : nullptr);
}
static int download_call(loamx_densemap* h, loamx_cloud* out, int axes, bool is_static, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && out, "NULL argument");
    std::vector<float4> rec;
    records_of_call(h, axes, is_static, rule, out, rec);
    if (rec.size() > out->count) { out->count = (uint32_t)rec.size(); return LOAMX_E_CAPACITY; }
    return unpack_cloud(rec.data(), (uint32_t)rec.size(), out);
  });
}
static int save_pcd_call(loamx_densemap* h, const char* path, int axes, bool is_static, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    std::vector<float4> rec;
    records_of_call(h, axes, is_static, rule, nullptr, rec);
    write_pcd_records(path, rec);
    return LOAMX_OK;
  });
}

// the count of records in v (`per` elements each) to *n; LOAMX_E_CAPACITY when they do not fit, else the copy
template <class T> static int copy_out(const std::vector<T>& v, void* out, uint64_t capacity, uint64_t* n, size_t per = 1) {
  *n = v.size() / per;
  if (*n > capacity) return LOAMX_E_CAPACITY;
  if (!v.empty()) memcpy(out, v.data(), sizeof(T) * v.size());
  return LOAMX_OK;
}

// the surfel settings of a call, checked (NULL: the defaults)
loamx_densemap_surfel_config checked_surfel_config(const loamx_densemap_surfel_config* cfg) {
  const loamx_densemap_surfel_config c = or_default(cfg, loamx_densemap_surfel_default_config);
  LX_REQUIRE(c.min_points >= 3u, "min_points must be >= 3");
  LX_REQUIRE(c.min_planar_ratio >= 0.f, "min_planar_ratio must be >= 0");   // (NaN too)
  return c;
}
// the optional rule of a surfel call: NULL stays NULL (every voxel); a rule is checked into `r` and needs carving
const loamx_densemap_static_rule* checked_optional_rule(loamx_densemap* h, const loamx_densemap_static_rule* rule,
                                                        loamx_densemap_static_rule& r) {
  if (!rule) return nullptr;
  r = checked_rule(rule);
  LX_REQUIRE_CARVING(h);
  return &r;
}
// the surfels of a call: arguments checked in the order of download_static (a rule needs carving)
static void surfels_of_call(loamx_densemap* h, int axes, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                            std::vector<loamx_surfel>& out) {
  checked_axes(axes);
  const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
  LX_REQUIRE_MOMENTS(h);
  loamx_densemap_static_rule r;
  h->d.surfels(out, axes, c, checked_optional_rule(h, rule, r));
}

}  // namespace loamx

using namespace loamx;

extern "C" {

int loamx_densemap_download(loamx_densemap* h, loamx_cloud* out, int axes) { return download_call(h, out, axes, false, nullptr); }
int loamx_densemap_download_static(loamx_densemap* h, loamx_cloud* out, int axes, const loamx_densemap_static_rule* rule) {
  return download_call(h, out, axes, true, rule);
}
int loamx_densemap_save_pcd(loamx_densemap* h, const char* path, int axes) { return save_pcd_call(h, path, axes, false, nullptr); }
int loamx_densemap_save_pcd_static(loamx_densemap* h, const char* path, int axes, const loamx_densemap_static_rule* rule) {
  return save_pcd_call(h, path, axes, true, rule);
}
int loamx_write_pcd(const char* path, const loamx_cloud* c, int axes) {
  return guard([&]() {
    LX_REQUIRE(path && c, "NULL argument");
    checked_axes(axes);
    check_cloud(c, false);
    std::vector<float4> rec(c->count);
    pack_cloud(c, rec.data());
    if (axes == 1)
      for (float4& r : rec) r = make_float4(r.z, r.x, r.y, r.w);
    write_pcd_records(path, rec);
    return LOAMX_OK;
  });
}

int loamx_densemap_download_misses(loamx_densemap* h, uint32_t* out, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    LX_REQUIRE_CARVING(h);
    std::vector<uint32_t> m;
    h->d.misses(m);
    return copy_out(m, out, capacity, n);
  });
}

void loamx_densemap_surfel_default_config(loamx_densemap_surfel_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->min_points = 5u;
  cfg->min_planar_ratio = 0.01f;
}
int loamx_densemap_surfel_of(float leaf, const int32_t idx[3], const uint64_t vals[4], const uint64_t mom[9],
                             const loamx_densemap_surfel_config* cfg, int axes, loamx_surfel* out) {
  return guard([&]() {
    LX_REQUIRE(idx && vals && mom && out, "NULL argument");
    LX_REQUIRE(leaf > 0.f && std::isfinite(leaf), "leaf must be positive");
    checked_axes(axes);
    LX_REQUIRE(vals[0] != 0ull, "a voxel holds at least one point");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    const long long ia[3] = {idx[0], idx[1], idx[2]};
    const unsigned long long v4[4] = {vals[0], vals[1], vals[2], vals[3]};
    unsigned long long m9[DM_MOM_WORDS];
    for (int k = 0; k < DM_MOM_WORDS; k++) m9[k] = mom[k];
    dm_surfel((double)leaf, ia, v4, m9, c, axes, *out);
    return LOAMX_OK;
  });
}
int loamx_densemap_download_moments(loamx_densemap* h, uint64_t* out, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    LX_REQUIRE_MOMENTS(h);
    std::vector<unsigned long long> m;
    h->d.moment_words(m);
    return copy_out(m, out, capacity, n, DM_MOM_WORDS);
  });
}
int loamx_densemap_download_surfels(loamx_densemap* h, loamx_surfel* out, uint64_t capacity, uint64_t* n, int axes,
                                    const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && n && (out || !capacity), "NULL argument");
    std::vector<loamx_surfel> s;
    surfels_of_call(h, axes, cfg, rule, s);
    return copy_out(s, out, capacity, n);
  });
}
int loamx_densemap_save_pcd_surfels(loamx_densemap* h, const char* path, int axes, const loamx_densemap_surfel_config* cfg,
                                    const loamx_densemap_static_rule* rule) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    std::vector<loamx_surfel> s;
    surfels_of_call(h, axes, cfg, rule, s);
    write_pcd(path, "FIELDS x y z intensity normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\n",
              s.data(), sizeof(loamx_surfel), s.size());
    return LOAMX_OK;
  });
}

int loamx_densemap_freeze(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                          uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    const uint64_t n = h->d.freeze(c, checked_optional_rule(h, rule, r));
    if (n_surfels) *n_surfels = n;
    return LOAMX_OK;
  });
}
int loamx_densemap_frozen_size(loamx_densemap* h, uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h && n_surfels, "NULL argument");
    *n_surfels = h->d.frozen.valid() ? h->d.frozen.size() : 0;
    return LOAMX_OK;
  });
}

}  // extern "C"
