// Dense map, regions (include/loamx.h: loamx_densemap_region_* ... loamx_densemap_page): the voxels of a window counted, exported and
// written to a file; the same voxels taken out of the table (evict), and the map kept around a moving centre with the rest in tile
// files (page).  The window arithmetic, the tiles and the merge of records are plain C++ (densemap_tiles.hpp).
//
// The compaction is one pass over the keys.  REGION: a thread decodes the three 21-bit fields of its slot's key and tests the window
// (integer compares); without REGION every occupied slot is selected, which is the compaction that every export of the whole map
// (DenseMap::snapshot_of) has always run.  k_dm_count: selected slots per 256-slot block by wave ballot and, with REGION, the n of the
// selected slots wave-reduced into one 64-bit atomic per wave.  Behind an exclusive scan of the block counts, k_dm_compact writes the
// keys, the four value words, the miss word and the nine moment words of the selected slots at their offsets.  Only those records
// cross to the host, which orders them by key.  Integer arithmetic only.
//
// evict: the count, the smaller table allocated, (with a path) the compaction and the file, then k_dm_rehash with the window as what
// stays behind (densemap.hip), then the swap.  Everything that can fail comes before the first change of the handle.
#include "densemap_dev.hpp"
#include "densemap_label.hpp"
#include "densemap_map.hpp"
#include "densemap_tiles.hpp"
#include <algorithm>
#include <cstddef>
#include <dirent.h>
#include <numeric>
#include <unistd.h>

namespace loamx {

static_assert(sizeof(DmRegion) == sizeof(loamx_densemap_region) && offsetof(DmRegion, side) == offsetof(loamx_densemap_region, side),
              "densemap_tiles.hpp mirrors the region of include/loamx.h");

// The sum of n goes to DM_SEL_SUMS partial sums, one per 128-byte line, the wave's by its number: a table's selected voxels are
// spread over its slots, so nearly every wave has a sum to add, and atomics on one address are served one after the other (measured
// on a 1 M-voxel map in 4 M slots: 131 us with one address for a window of 1 % of the voxels and 790 us for its outside, against 7 us
// for the pass without the sum).  The host adds the partial sums
constexpr uint32_t DM_SEL_SUMS = 64, DM_SEL_STRIDE = 16;   // (words)

// selected slots per 256-slot block (ballot); REGION: the window's, and their n summed into points (above)
template <bool REGION>
__global__ __launch_bounds__(256) void k_dm_count(const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t* __restrict__ blk,
                                                  DmWindow W, const unsigned long long* __restrict__ vals,
                                                  unsigned long long* __restrict__ points) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < slots ? keys[i] : DM_EMPTY;
  bool sel = key != DM_EMPTY;
  if (REGION && sel) sel = dm_in_window(key, W);
  if (REGION) dm_wave_sum64(points + (size_t)((i >> 6) & (DM_SEL_SUMS - 1u)) * DM_SEL_STRIDE, sel ? vals[4ull * i] : 0ull);
  const uint32_t n_sel = dm_block_count(sel);
  if (threadIdx.x == 0) blk[blockIdx.x] = n_sel;
}

// behind the exclusive scan of those counts each block writes its selected slots at its offset, in slot order (AUX: the slot's miss
// word too; MOM: its nine moment words)
template <bool AUX, bool MOM, bool REGION>
__global__ __launch_bounds__(256) void k_dm_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                    uint32_t slots, const uint32_t* __restrict__ blk_off, unsigned long long* __restrict__ okeys,
                                                    unsigned long long* __restrict__ ovals, const uint32_t* __restrict__ aux,
                                                    uint32_t* __restrict__ omiss, const unsigned long long* __restrict__ mom,
                                                    unsigned long long* __restrict__ omom, DmWindow W) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < slots ? keys[i] : DM_EMPTY;
  bool occ = key != DM_EMPTY;
  if (REGION && occ) occ = dm_in_window(key, W);
  const unsigned long long m = dm_block_vote(occ);
  if (!occ) return;
  const uint32_t pos = dm_block_rank(m, blk_off[blockIdx.x]);
  okeys[pos] = key;
  const ulonglong2* s = (const ulonglong2*)(vals + 4ull * i);
  ulonglong2* d = (ulonglong2*)(ovals + 4ull * pos);
  d[0] = s[0];
  d[1] = s[1];
  if (AUX) omiss[pos] = aux[2ull * i];
  if (MOM) {
    const unsigned long long* ms = mom + (unsigned long long)DM_MOM_WORDS * i;
    unsigned long long* md = omom + (unsigned long long)DM_MOM_WORDS * pos;
#pragma unroll
    for (int k = 0; k < DM_MOM_WORDS; k++) md[k] = ms[k];
  }
}

void DenseMap::compact_of(const DmTable& T, const DmWindow* W, uint64_t occ, Snapshot* S, bool want_mom, uint64_t counts[2]) {
  const uint32_t nblk = (T.slots + 255) / 256;
  DevBuf<uint32_t> blk, omiss;
  DevBuf<unsigned long long> okeys, ovals, omom, points;
  blk.reserve((size_t)nblk + 1);
  uint32_t total = 0;
  if (W) {
    constexpr size_t sum_words = (size_t)DM_SEL_SUMS * DM_SEL_STRIDE;
    points.reserve(sum_words);
    LX_HIP(hipMemsetAsync(points.p, 0, sizeof(unsigned long long) * sum_words, own_));
    hipLaunchKernelGGL(k_dm_count<true>, dim3(nblk), dim3(256), 0, own_, T.keys, T.slots, blk.p, *W, T.vals, points.p);
    scan_.run(blk.p, nblk, own_);
    LX_HIP(hipGetLastError());
    std::vector<unsigned long long> sums(sum_words);
    LX_HIP(hipMemcpyAsync(&total, blk.p + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, own_));
    LX_HIP(hipMemcpyAsync(sums.data(), points.p, sizeof(unsigned long long) * sum_words, hipMemcpyDeviceToHost, own_));
    LX_HIP(hipStreamSynchronize(own_));
    scan_check_errors();
    unsigned long long pts = 0;
    for (uint32_t k = 0; k < DM_SEL_SUMS; k++) pts += sums[(size_t)k * DM_SEL_STRIDE];
    occ = total;
    if (counts) { counts[0] = total; counts[1] = pts; }
    if (!S) return;
  } else {
    hipLaunchKernelGGL(k_dm_count<false>, dim3(nblk), dim3(256), 0, own_, T.keys, T.slots, blk.p, DmWindow(), nullptr, nullptr);
    scan_.run(blk.p, nblk, own_);
  }
  okeys.reserve(occ + 1);
  ovals.reserve(4 * (occ + 1));
  if (T.aux) omiss.reserve(occ + 1);
  if (want_mom) omom.reserve(DM_MOM_WORDS * (occ + 1));
  dm_dispatch2(T.aux != nullptr, want_mom, [&](auto A, auto M) {   // (an array that is off is not read: omiss.p, omom.p are NULL then)
    constexpr bool AUX = decltype(A)::value, MOM = decltype(M)::value;
    if (W)
      hipLaunchKernelGGL((k_dm_compact<AUX, MOM, true>), dim3(nblk), dim3(256), 0, own_, T.keys, T.vals, T.slots, blk.p, okeys.p, ovals.p, T.aux,
                         omiss.p, T.mom, omom.p, *W);
    else
      hipLaunchKernelGGL((k_dm_compact<AUX, MOM, false>), dim3(nblk), dim3(256), 0, own_, T.keys, T.vals, T.slots, blk.p, okeys.p, ovals.p, T.aux,
                         omiss.p, T.mom, omom.p, DmWindow());
  });
  LX_HIP(hipGetLastError());
  S->k.resize(occ);
  S->v.resize(4 * (size_t)occ);
  S->miss.assign(T.aux ? occ : 0, 0u);
  S->mom.resize(want_mom ? DM_MOM_WORDS * (size_t)occ : 0);
  if (!W) LX_HIP(hipMemcpyAsync(&total, blk.p + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, own_));
  if (occ) {
    LX_HIP(hipMemcpyAsync(S->k.data(), okeys.p, sizeof(unsigned long long) * occ, hipMemcpyDeviceToHost, own_));
    LX_HIP(hipMemcpyAsync(S->v.data(), ovals.p, sizeof(unsigned long long) * 4 * occ, hipMemcpyDeviceToHost, own_));
    if (T.aux) LX_HIP(hipMemcpyAsync(S->miss.data(), omiss.p, sizeof(uint32_t) * occ, hipMemcpyDeviceToHost, own_));
    if (want_mom)
      LX_HIP(hipMemcpyAsync(S->mom.data(), omom.p, sizeof(unsigned long long) * DM_MOM_WORDS * occ, hipMemcpyDeviceToHost, own_));
  }
  LX_HIP(hipStreamSynchronize(own_));
  scan_check_errors();
  LX_REQUIRE(total == occ, "dense map: the compaction disagrees with the occupancy count");
  S->idx.resize(occ);
  std::iota(S->idx.begin(), S->idx.end(), 0u);
  std::sort(S->idx.begin(), S->idx.end(), [&](uint32_t a, uint32_t b) { return S->k[a] < S->k[b]; });
}

void DenseMap::select(const DmWindow& W, Snapshot* S, bool want_mom, uint64_t counts[2]) {
  read_counters();
  compact_of(tab_, &W, 0, S, want_mom, counts);
}

void DenseMap::region_header(DmFileHeader& H) const {
  H = DmFileHeader();
  H.flags = flags();
  H.leaf = cfg.leaf;
  if (carving()) {
    H.carve_max_range = carve_.max_range;
    H.ray_stride = carve_.ray_stride; H.end_margin = carve_.end_margin; H.max_steps = carve_.max_steps;
  }
}

// the voxels of a snapshot in ascending key order as the records of a file under the header rule of a region (densemap_tiles.hpp)
static void file_of(const DenseMap::Snapshot& S, const DmFileHeader& like, DmFile& F) {
  const bool aux = (like.flags & DMF_CARVING) != 0, mom = (like.flags & DMF_MOMENTS) != 0;
  const size_t n = S.idx.size();
  F = DmFile();
  F.keys.reserve(n);
  F.vals.reserve(4 * n);
  DenseMap::for_each_voxel(S, nullptr, [&](size_t j, const long long*) {
    F.keys.push_back(S.k[j]);
    F.vals.insert(F.vals.end(), &S.v[4 * j], &S.v[4 * j] + 4);
    if (aux) F.miss.push_back(S.miss[j]);
    if (mom) F.mom.insert(F.mom.end(), &S.mom[DM_MOM_WORDS * j], &S.mom[DM_MOM_WORDS * j] + DM_MOM_WORDS);
  });
  F.h = dmt_region_header(like, F.keys, F.vals);
}

void DenseMap::save_region(const DmWindow& W, const char* path) {
  Snapshot S;
  select(W, &S, moments(), nullptr);
  DmFileHeader like;
  region_header(like);
  DmFile F;
  file_of(S, like, F);
  const std::string e = dmt_write(path, F);
  LX_REQUIRE(e.empty(), e);
}

// The order is the contract (include/loamx.h): count, allocate, write, and only then the first change of the handle
void DenseMap::evict(const DmWindow& W, const char* path, uint64_t removed[2]) {
  uint64_t sel[2] = {0, 0};
  select(W, nullptr, false, sel);
  DmTable nt;
  nt.alloc(dm_slots_for(cfg.initial_slots, occ_.occ - sel[0]), tab_.aux != nullptr, tab_.mom != nullptr);
  if (path) save_region(W, path);
  nt.clear(own_);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long), own_));   // (the occupancy: recounted by the kernel)
  launch_rehash<DM_DROP_WINDOW>(own_, nt, loamx_densemap_static_rule{0u, 0u, 0u}, W);
  LX_HIP(hipGetLastError());
  LX_HIP(hipStreamSynchronize(own_));
  replace_table(nt);
  offered_ -= sel[1];
  read_counters();
  removed[0] = sel[0]; removed[1] = sel[1];
}

static std::string join(const std::string& dir, const std::string& name) { return dir + "/" + name; }

int DenseMap::page(const char* dir, uint32_t T, const uint32_t radius[3], const float centre[3], uint64_t stats[6]) {
  std::string e = dmt_check_tile_voxels(T);
  LX_REQUIRE(e.empty(), e);
  int32_t ci[3], ct[3];
  for (int a = 0; a < 3; a++) {
    LX_REQUIRE(std::isfinite(centre[a]), "centre: must be finite");
    ci[a] = dmt_index_of((double)centre[a], (double)cfg.leaf);
  }
  (void)dmt_tile_of(ci, T, ct);
  // the keep box in tiles and in voxels
  int64_t tlo[3], thi[3];
  DmWindow W;
  for (int a = 0; a < 3; a++) {
    tlo[a] = (int64_t)ct[a] - (int64_t)radius[a];
    thi[a] = (int64_t)ct[a] + (int64_t)radius[a];
    W.lo[a] = (int)dmt_clamp(tlo[a] * (int64_t)T);   // (|tile| < 2^33, T <= 2^20)
    W.hi[a] = (int)dmt_clamp(thi[a] * (int64_t)T + (int64_t)T - 1);
  }
  W.outside = 1u;
  for (int k = 0; k < 6; k++) stats[k] = 0;

  // page in: the tile files of the keep box, in the order of their tiles
  std::vector<std::array<int32_t, 3>> in;
  {
    DIR* d = opendir(dir);
    LX_REQUIRE(d, std::string("dir: cannot open ") + dir);
    while (const dirent* ent = readdir(d)) {
      int32_t t[3];
      if (!dmt_parse_tile_name(ent->d_name, t)) continue;
      bool keep = true;
      for (int a = 0; a < 3; a++) keep = keep && t[a] >= tlo[a] && t[a] <= thi[a];
      if (keep) in.push_back({t[0], t[1], t[2]});
    }
    closedir(d);
    std::sort(in.begin(), in.end(), DmTileLess());
  }
  for (const auto& t : in) {
    const std::string path = join(dir, dmt_tile_name(t.data()));
    DmFile head;
    e = dmf_read(path.c_str(), false, head);
    LX_REQUIRE(e.empty(), path + ": " + e);
    const int rc = merge_file(path.c_str(), false);
    if (rc != LOAMX_OK) { stats[5] = occ_.occ; return rc; }
    (void)unlink(path.c_str());
    stats[0] += 1;
    stats[1] += head.h.count;
  }

  // page out: what lies outside the keep box comes down once, is bucketed by tile and merged into the files that exist already
  uint64_t sel[2] = {0, 0};
  select(W, nullptr, false, sel);
  stats[5] = occ_.occ;
  if (!sel[0]) return LOAMX_OK;
  DmTable nt;
  nt.alloc(dm_slots_for(cfg.initial_slots, occ_.occ - sel[0]), tab_.aux != nullptr, tab_.mom != nullptr);
  Snapshot S;
  compact_of(tab_, &W, 0, &S, moments(), nullptr);
  DmFileHeader like;
  region_header(like);
  DmFile out;
  file_of(S, like, out);
  DmTileBuckets buckets;
  (void)dmt_bucket(out, T, buckets);
  std::vector<std::string> written;
  uint64_t merged = 0;
  try {
    for (auto& kv : buckets) {
      const std::string path = join(dir, dmt_tile_name(kv.first.data()));
      DmFile* f = &kv.second;
      DmFile old, sum;
      if (access(path.c_str(), F_OK) == 0) {
        e = dmf_read(path.c_str(), true, old);
        LX_REQUIRE(e.empty(), path + ": " + e);
        e = dmt_merge(old, *f, sum);
        LX_REQUIRE(e.empty(), path + ": " + e);
        f = &sum;
        merged++;
      }
      const std::string part = path + ".part";
      e = dmf_write_part(part, path.c_str(), f->h, f->keys.data(), f->vals.data(), (f->h.flags & DMF_CARVING) ? f->miss.data() : nullptr,
                         (f->h.flags & DMF_MOMENTS) ? f->mom.data() : nullptr);
      LX_REQUIRE(e.empty(), e);
      written.push_back(path);
    }
    for (size_t k = 0; k < written.size(); k++) {
      if (rename((written[k] + ".part").c_str(), written[k].c_str()) != 0) throw Error(LOAMX_E_INVALID, "write to " + written[k] + " failed");
    }
  } catch (...) {
    for (const std::string& p : written) (void)remove((p + ".part").c_str());
    throw;
  }
  nt.clear(own_);
  LX_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(unsigned long long), own_));
  launch_rehash<DM_DROP_WINDOW>(own_, nt, loamx_densemap_static_rule{0u, 0u, 0u}, W);
  LX_HIP(hipGetLastError());
  LX_HIP(hipStreamSynchronize(own_));
  replace_table(nt);
  offered_ -= sel[1];
  read_counters();
  stats[2] = written.size();
  stats[3] = sel[0];
  stats[4] = merged;
  stats[5] = occ_.occ;
  return LOAMX_OK;
}

// the region of a call, checked, as the kernels' window
static DmWindow checked_window(const loamx_densemap_region* region) {
  DmRegion r;
  memcpy(&r, region, sizeof(r));
  const std::string e = dmt_region_check(r);
  LX_REQUIRE(e.empty(), "region " + e);
  DmWindow W;
  for (int a = 0; a < 3; a++) { W.lo[a] = r.lo[a]; W.hi[a] = r.hi[a]; }
  W.outside = r.side;
  return W;
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_region_default(loamx_densemap_region* region) {
  if (!region) return;
  DmRegion r;
  dmt_region_default(r);
  memcpy(region, &r, sizeof(r));
}
int loamx_densemap_region_check(const loamx_densemap_region* region) {
  return guard([&]() {
    LX_REQUIRE(region, "NULL argument");
    (void)checked_window(region);
    return LOAMX_OK;
  });
}
int loamx_densemap_region_about(float leaf, const float centre[3], const float half[3], loamx_densemap_region* region) {
  return guard([&]() {
    LX_REQUIRE(centre && half && region, "NULL argument");
    DmRegion r;
    const std::string e = dmt_region_about(leaf, centre, half, r);
    LX_REQUIRE(e.empty(), e);
    memcpy(region, &r, sizeof(r));
    return LOAMX_OK;
  });
}
int loamx_densemap_tile_of(const int32_t idx[3], uint32_t tile_voxels, int32_t tile[3]) {
  return guard([&]() {
    LX_REQUIRE(idx && tile, "NULL argument");
    const std::string e = dmt_tile_of(idx, tile_voxels, tile);
    LX_REQUIRE(e.empty(), e);
    return LOAMX_OK;
  });
}
int loamx_densemap_tile_region(const int32_t tile[3], uint32_t tile_voxels, loamx_densemap_region* region) {
  return guard([&]() {
    LX_REQUIRE(tile && region, "NULL argument");
    DmRegion r;
    const std::string e = dmt_tile_region(tile, tile_voxels, r);
    LX_REQUIRE(e.empty(), e);
    memcpy(region, &r, sizeof(r));
    return LOAMX_OK;
  });
}
int loamx_densemap_tile_name(const int32_t tile[3], char* buf, uint64_t cap) {
  return guard([&]() {
    LX_REQUIRE(tile && buf, "NULL argument");
    const std::string s = dmt_tile_name(tile);
    LX_REQUIRE(s.size() + 1 <= cap, "cap: the name needs " + std::to_string(s.size() + 1) + " bytes");
    memcpy(buf, s.c_str(), s.size() + 1);
    return LOAMX_OK;
  });
}
int loamx_densemap_file_merge(const char* path_a, const char* path_b, const char* path_out) {
  return guard([&]() {
    LX_REQUIRE(path_a && path_b && path_out, "NULL argument");
    const std::string e = dmt_file_merge(path_a, path_b, path_out);
    LX_REQUIRE(e.empty(), e);
    return LOAMX_OK;
  });
}

int loamx_densemap_count_region(loamx_densemap* h, const loamx_densemap_region* region, uint64_t counts[2]) {
  return guard([&]() {
    LX_REQUIRE(h && region && counts, "NULL argument");
    const DmWindow W = checked_window(region);
    uint64_t c[2] = {0, 0};
    h->d.select(W, nullptr, false, c);
    counts[0] = c[0]; counts[1] = c[1];
    return LOAMX_OK;
  });
}
int loamx_densemap_download_region(loamx_densemap* h, const loamx_densemap_region* region, loamx_cloud* out, int axes) {
  return guard([&]() {
    LX_REQUIRE(h && region && out, "NULL argument");
    LX_REQUIRE(axes == 0 || axes == 1, "axes must be 0 (LOAM frame) or 1 (sensor axes)");
    const DmWindow W = checked_window(region);
    check_cloud(out, false);
    std::vector<float4> rec;
    h->d.records(rec, axes, nullptr, &W);
    if (rec.size() > out->count) { out->count = (uint32_t)rec.size(); return LOAMX_E_CAPACITY; }
    return unpack_cloud(rec.data(), (uint32_t)rec.size(), out);
  });
}
int loamx_densemap_save_region(loamx_densemap* h, const loamx_densemap_region* region, const char* path) {
  return guard([&]() {
    LX_REQUIRE(h && region && path, "NULL argument");
    h->d.save_region(checked_window(region), path);
    return LOAMX_OK;
  });
}
int loamx_densemap_evict(loamx_densemap* h, const loamx_densemap_region* region, const char* path, uint64_t removed[2]) {
  return guard([&]() {
    LX_REQUIRE(h && region && removed, "NULL argument");
    const DmWindow W = checked_window(region);
    uint64_t r[2] = {0, 0};
    h->d.evict(W, path, r);
    removed[0] = r[0]; removed[1] = r[1];
    return LOAMX_OK;
  });
}
int loamx_densemap_page(loamx_densemap* h, const loamx_densemap_page_config* cfg, const float centre[3], uint64_t stats[6]) {
  return guard([&]() {
    LX_REQUIRE(h && cfg && centre && stats, "NULL argument");
    LX_REQUIRE(cfg->dir, "dir: NULL");
    uint64_t s[6];
    const int rc = h->d.page(cfg->dir, cfg->tile_voxels, cfg->radius, centre, s);
    for (int k = 0; k < 6; k++) stats[k] = s[k];
    return rc;
  });
}

}  // extern "C"
