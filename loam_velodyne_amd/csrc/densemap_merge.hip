// Dense map, files and merges (include/loamx.h: loamx_densemap_save / load / merge / merge_file / file_info).  The file is the
// compaction of a snapshot in ascending key order with the statistics in its header; reader, writer and validator are plain C++
// (densemap_file.hpp).  A merge adds every record of a source — another map's table, or the arrays of a file — into the live table by
// one kernel; load is a merge of a file into an empty map.
#include "densemap_dev.hpp"
#include "densemap_file.hpp"
#include "densemap_map.hpp"

namespace loamx {

// the statistics a merge adds to dst's counters: [0] dropped by range, [1] dropped outside the key range, [2..8) the six of carving
struct DmCtrAdd {
  unsigned long long v[8];
};

// Merge (include/loamx.h, loamx_densemap_merge / merge_file): every record of a source is added into the live table, its voxel claimed
// when absent.  The source is another map's table (sn slots, the DM_EMPTY ones skipped, miss at smiss[2 * i]: miss_stride 2) or the
// compact arrays of a file (sn records, miss_stride 1).  AUX: the miss word is added too, the stamp of dst stays (0 in a fresh slot: the
// words beside a free slot are zero).  MOM: the nine moment words.
// Only the key claim is atomic.  The keys of one source are unique, so within the launch one thread at most holds a given slot of
// dst, and nothing else writes dst meanwhile: the launch runs on dst's stream behind its adds, and the host waits for it before it
// returns.  The up to 14 value words are therefore plain loads, integer adds and plain stores (16 bytes at a time for n, Sx, Sy, Sz;
// the 72-byte moment rows are only 8-byte aligned) instead of 14 atomics that each make a trip to the memory side; a slot the CAS
// has just claimed reads as the zeros that the memset of an earlier launch left there.  Integer adds modulo 2^64 (miss: 2^32); no floating point anywhere.
// ctr[0] counts the slots claimed, as the insert does; ctr[3] reports a probe loop that ran out.  The first thread also adds the
// source's statistics to dst's counters
template <bool AUX, bool MOM>
__global__ __launch_bounds__(256) void k_dm_merge(const unsigned long long* __restrict__ skeys, const unsigned long long* __restrict__ svals,
                                                  uint32_t sn, const uint32_t* __restrict__ smiss, uint32_t miss_stride,
                                                  const unsigned long long* __restrict__ smom, unsigned long long* __restrict__ keys,
                                                  unsigned long long* __restrict__ vals, uint32_t mask, uint32_t shift,
                                                  unsigned long long* __restrict__ ctr, uint32_t* __restrict__ aux,
                                                  unsigned long long* __restrict__ mom, DmCtrAdd add) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < sn ? skeys[i] : DM_EMPTY;
  const bool live = key != DM_EMPTY;
  uint32_t slot = 0;
  bool won = false, ok = true;
  if (live) ok = dm_find_or_claim(keys, mask, shift, key, slot, won);
  dm_wave_count(&ctr[0], won);
  if (live && !ok) ctr[3] = 1ull;
  if (live && ok) {
    const ulonglong2* s = (const ulonglong2*)(svals + 4ull * i);
    ulonglong2* d = (ulonglong2*)(vals + 4ull * slot);
    const ulonglong2 s0 = s[0], s1 = s[1];
    ulonglong2 d0 = d[0], d1 = d[1];
    d0.x += s0.x; d0.y += s0.y; d1.x += s1.x; d1.y += s1.y;
    d[0] = d0;
    d[1] = d1;
    if (AUX) aux[2ull * slot] += smiss[(unsigned long long)miss_stride * i];
    if (MOM) {
      const unsigned long long* ms = smom + (unsigned long long)DM_MOM_WORDS * i;
      unsigned long long* md = mom + (unsigned long long)DM_MOM_WORDS * slot;
#pragma unroll
      for (int k = 0; k < DM_MOM_WORDS; k++) md[k] += ms[k];
    }
  }
  if (i == 0) {
    if (add.v[0]) atomicAdd(&ctr[1], add.v[0]);
    if (add.v[1]) atomicAdd(&ctr[2], add.v[1]);
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (add.v[2 + k]) atomicAdd(&ctr[4 + k], add.v[2 + k]);
  }
}

uint32_t DenseMap::flags() const { return (tab_.aux ? DMF_CARVING : 0u) | (tab_.mom ? DMF_MOMENTS : 0u); }

// the records of snapshot() in ascending key order, with the statistics
void DenseMap::save(const char* path) {
  Snapshot S;
  const bool aux = carving(), mom = moments();
  snapshot(S, mom);
  const size_t n = S.idx.size();
  DmFileHeader H;
  H.flags = flags();
  H.leaf = cfg.leaf;
  H.count = n;
  H.offered = offered_; H.dropped_range = drop_range_; H.dropped_key = drop_key_;
  if (aux) {
    for (int k = 0; k < 6; k++) H.carve_stats[k] = carve_ctr_[k];
    H.carve_max_range = carve_.max_range;
    H.ray_stride = carve_.ray_stride; H.end_margin = carve_.end_margin; H.max_steps = carve_.max_steps;
  }
  std::vector<uint64_t> k, v, m;
  std::vector<uint32_t> ms;
  k.reserve(n);
  v.reserve(4 * n);
  for_each_voxel(S, nullptr, [&](size_t j, const long long*) {
    k.push_back(S.k[j]);
    v.insert(v.end(), &S.v[4 * j], &S.v[4 * j] + 4);
    if (aux) ms.push_back(S.miss[j]);
    if (mom) m.insert(m.end(), &S.mom[DM_MOM_WORDS * j], &S.mom[DM_MOM_WORDS * j] + DM_MOM_WORDS);
  });
  const std::string e = dmf_write(path, H, k.data(), v.data(), aux ? ms.data() : nullptr, mom ? m.data() : nullptr);
  LX_REQUIRE(e.empty(), e);
}

int DenseMap::merge(DenseMap& src) {
  LX_REQUIRE(&src != this, "a dense map cannot be merged into itself");
  LX_REQUIRE(!history_, "the destination keeps a sweep log (loamx_densemap_enable_history): a merged map has no sweeps behind it to rebuild from");
  LX_REQUIRE(src.cfg.device == cfg.device, "the two dense maps live on different devices");
  LX_REQUIRE(memcmp(&src.cfg.leaf, &cfg.leaf, sizeof(float)) == 0, "the two dense maps differ in their leaf");
  LX_REQUIRE(src.flags() == flags(), "the two dense maps do not have the same features enabled (carving, moments)");
  src.read_counters();
  read_counters();
  if (!occ_.admits_exact(src.occ_.occ, cfg.max_voxels)) return LOAMX_E_CAPACITY;
  DmCtrAdd add;
  add.v[0] = src.drop_range_; add.v[1] = src.drop_key_;
  for (int k = 0; k < 6; k++) add.v[2 + k] = src.carve_ctr_[k];
  merge_records(src.tab_.keys, src.tab_.vals, src.tab_.slots, src.occ_.occ, src.tab_.aux, 2u, src.tab_.mom, add, src.offered_);
  return LOAMX_OK;
}

// The file is validated on the host before the device is touched; every refusal comes before the first change of the handle
int DenseMap::merge_file(const char* path, bool loading) {
  LX_REQUIRE(!history_, "the dense map keeps a sweep log (loamx_densemap_enable_history): a map from a file has no sweeps behind it to rebuild from");
  DmFile F;
  const std::string e = dmf_read(path, true, F);
  LX_REQUIRE(e.empty(), std::string(path) + ": " + e);
  LX_REQUIRE(memcmp(&F.h.leaf, &cfg.leaf, sizeof(float)) == 0, "the file's leaf differs from the dense map's");
  const uint64_t n = F.h.count;
  read_counters();
  if (loading) {
    LX_REQUIRE(occ_.occ == 0 && offered_ == 0, "a file can only be loaded into an empty map (a fresh handle, or right after reset)");
    LX_REQUIRE((flags() & ~F.h.flags) == 0u, "the dense map has a feature enabled (carving, moments) that the file lacks");
    if (!occ_.admits_exact(n, cfg.max_voxels)) return LOAMX_E_CAPACITY;   // (occ is 0)
    if (F.h.flags & DMF_CARVING) {
      const loamx_densemap_carve_config c = {F.h.carve_max_range, F.h.ray_stride, F.h.end_margin, F.h.max_steps};
      enable_carving(c);
    }
    if (F.h.flags & DMF_MOMENTS) enable_moments();
    // the smallest table the file's voxels fit at a load of one half (a handle reset after it grew holds a larger one)
    const uint64_t target = dm_slots_for(cfg.initial_slots, n);
    if (tab_.slots > target) {
      // (not the sequence of the other replacements, and kept: the host waits for own_ before the old table retires, and the new
      // one is cleared together with the counters once it is the map's)
      DmTable nt;
      nt.alloc(target, tab_.aux != nullptr, tab_.mom != nullptr);
      LX_HIP(hipStreamSynchronize(own_));
      replace_table(nt);
      clear(own_);
    }
  } else {
    LX_REQUIRE(F.h.flags == flags(), "the file and the dense map do not have the same features (carving, moments)");
    if (!occ_.admits_exact(n, cfg.max_voxels)) return LOAMX_E_CAPACITY;
  }
  // one pinned block, one copy: values (first: the kernel reads them 16 bytes at a time), moment words, keys, then the 32-bit miss words
  const size_t nn = (size_t)n, w_mom = moments() ? DM_MOM_WORDS * nn : 0, w_miss = carving() ? (nn + 1) / 2 : 0;
  const size_t o_mom = 4 * nn, o_keys = o_mom + w_mom, o_miss = o_keys + nn, words = o_miss + w_miss;
  PinBuf<unsigned long long> h_up;
  DevBuf<unsigned long long> d_up;
  h_up.reserve(words + 1);
  d_up.reserve(words + 1);
  if (nn) {
    for (size_t i = 0; i < 4 * nn; i++) h_up.p[i] = F.vals[i];
    for (size_t i = 0; i < w_mom; i++) h_up.p[o_mom + i] = F.mom[i];
    for (size_t i = 0; i < nn; i++) h_up.p[o_keys + i] = F.keys[i];
    if (carving()) {
      h_up.p[words - 1] = 0ull;
      memcpy(h_up.p + o_miss, F.miss.data(), sizeof(uint32_t) * nn);
    }
    LX_HIP(hipMemcpyAsync(d_up.p, h_up.p, sizeof(unsigned long long) * words, hipMemcpyHostToDevice, own_));
  }
  DmCtrAdd add;
  add.v[0] = F.h.dropped_range; add.v[1] = F.h.dropped_key;
  for (int k = 0; k < 6; k++) add.v[2 + k] = F.h.carve_stats[k];
  const unsigned long long* d = d_up.p;
  merge_records(d + o_keys, d, (uint32_t)n, n, (const uint32_t*)(d + o_miss), 1u, d + o_mom, add, F.h.offered);
  return LOAMX_OK;
}

// the tail of merge / merge_file, behind a read_counters() (every add waited for, occ_ exact): sn source slots or records holding
// s_occ voxels go into the table on own_; returns when the table holds the result
void DenseMap::merge_records(const unsigned long long* skeys, const unsigned long long* svals, uint32_t sn, uint64_t s_occ,
                             const uint32_t* smiss, uint32_t miss_stride, const unsigned long long* smom, const DmCtrAdd& add,
                             uint64_t s_offered) {
  grow_for(s_occ, own_);
  const dim3 grid(sn ? (sn + 255u) / 256u : 1u), block(256);   // (one block at least: its first thread adds the statistics)
  const DmTable& T = tab_;
  dm_dispatch2(T.aux != nullptr, T.mom != nullptr, [&](auto A, auto M) {
    hipLaunchKernelGGL((k_dm_merge<decltype(A)::value, decltype(M)::value>), grid, block, 0, own_, skeys, svals, sn, smiss, miss_stride, smom, T.keys,
                       T.vals, T.mask(), T.shift(), ctr_.p, T.aux, T.mom, add);
  });
  LX_HIP(hipGetLastError());
  offered_ += s_offered;
  LX_HIP(hipStreamSynchronize(own_));   // (the rehash of a growth still read the table that read_counters is about to free)
  read_counters();
}

}  // namespace loamx

using namespace loamx;

extern "C" {

int loamx_densemap_save(loamx_densemap* h, const char* path) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    h->d.save(path);
    return LOAMX_OK;
  });
}
int loamx_densemap_load(loamx_densemap* h, const char* path) {
  return guard([&]() {
    LX_REQUIRE(h && path, "NULL argument");
    return h->d.merge_file(path, true);
  });
}
int loamx_densemap_merge(loamx_densemap* dst, loamx_densemap* src) {
  return guard([&]() {
    LX_REQUIRE(dst && src, "NULL argument");
    return dst->d.merge(src->d);
  });
}
int loamx_densemap_merge_file(loamx_densemap* dst, const char* path) {
  return guard([&]() {
    LX_REQUIRE(dst && path, "NULL argument");
    return dst->d.merge_file(path, false);
  });
}
int loamx_densemap_file_info(const char* path, struct loamx_densemap_file_info* info, int deep) {
  return guard([&]() {
    LX_REQUIRE(path && info, "NULL argument");
    DmFile F;
    const std::string e = dmf_read(path, deep != 0, F);
    LX_REQUIRE(e.empty(), std::string(path) + ": " + e);
    memset(info, 0, sizeof(*info));
    info->version = F.h.version; info->flags = F.h.flags;
    info->leaf = F.h.leaf;
    info->voxels = F.h.count;
    info->offered = F.h.offered; info->dropped_range = F.h.dropped_range; info->dropped_key = F.h.dropped_key;
    for (int k = 0; k < 6; k++) info->carve_stats[k] = F.h.carve_stats[k];
    info->carve.max_range = F.h.carve_max_range;
    info->carve.ray_stride = F.h.ray_stride; info->carve.end_margin = F.h.end_margin; info->carve.max_steps = F.h.max_steps;
    return LOAMX_OK;
  });
}

}  // extern "C"
