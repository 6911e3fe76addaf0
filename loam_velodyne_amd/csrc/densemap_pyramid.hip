// Dense map, coarser levels (include/loamx.h, loamx_densemap_coarsen / loamx_densemap_freeze_pyramid / loamx_densemap_frozen_levels).
//
// A level-l voxel (l >= 1) is the union of the up to eight level-(l-1) voxels whose indices halve to its own (i >> 1, arithmetic), with
// the leaf leaf * 2^l.  Its thirteen words are integer sums over those children of the children's words re-expressed in its own 20-bit
// units (q' = q / 2 + b * 2^19, b = i & 1, one floor per child and word), so a level is a table of the map's own format, depends on no
// order, and its surfels come from dm_surfel at the level's leaf with no arithmetic of their own.
//
// k_dm_coarsen serves every level: one thread per source slot; an occupied, selected slot computes its parent's key, finds or claims
// it in a fresh table (dm_find_or_claim) and adds its thirteen integers with no-return 64-bit atomics.  The children of a parent lie in
// unrelated slots of the source, so there is nothing to combine inside a wave.  The destination holds the source's occupancy at a load
// of at most one half and never grows; a probe bound reached is reported through an error word.  Level 1 reads the map's live table
// (read-only, behind the adds) and leaves out the voxels a rule calls dynamic; level l + 1 reads level l.
//
// The pyramid of snapshots is one DmFrozen per level: level 0 is what DenseMap::freeze builds; level l is built from the words of the
// cascade through dm_surfel, with the same entry format and slot rule.  The alignment against a level is densemap_align.hip's.
#include "densemap_dev.hpp"
#include "densemap_map.hpp"

namespace loamx {

// ctr: [0] slots claimed in the destination (its occupancy), [1] probe overflow.  SELECT (level 1 with a rule; the source has aux): the
// voxels the rule calls dynamic stay behind.  Every source index is < sn, every destination slot comes from dm_find_or_claim (<= mask)
template <bool SELECT>
__global__ __launch_bounds__(256) void k_dm_coarsen(const unsigned long long* __restrict__ skeys, const unsigned long long* __restrict__ svals,
                                                    const unsigned long long* __restrict__ smom, const uint32_t* __restrict__ saux, uint32_t sn,
                                                    loamx_densemap_static_rule rule, unsigned long long* __restrict__ keys,
                                                    unsigned long long* __restrict__ vals, unsigned long long* __restrict__ mom, uint32_t mask,
                                                    uint32_t shift, unsigned long long* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long key = i < sn ? skeys[i] : DM_EMPTY;
  bool live = key != DM_EMPTY;
  unsigned long long n = 0ull, S[3] = {0ull, 0ull, 0ull};
  if (live) {
    const ulonglong2* s = (const ulonglong2*)(svals + 4ull * i);
    const ulonglong2 lo = s[0], hi = s[1];
    n = lo.x; S[0] = lo.y; S[1] = hi.x; S[2] = hi.y;
    if (SELECT) live = !dm_dynamic(rule, n, saux[2ull * i]);
  }
  uint32_t slot = 0;
  bool won = false;
  if (live) {
    // a key field is i + 2^20: its low bit is b = i & 1, and (field >> 1) + 2^19 is (i >> 1) + 2^20, floor for negative i
    const unsigned long long km = (1ull << DM_KBITS) - 1ull;
    unsigned long long b[3], pkey = 0ull;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const unsigned long long f = (key >> (DM_KBITS * a)) & km;
      b[a] = f & 1ull;
      pkey |= ((f >> 1) + (1ull << (DM_QBITS - 1))) << (DM_KBITS * a);
    }
    if (dm_find_or_claim(keys, mask, shift, pkey, slot, won)) {
      unsigned long long* v = vals + 4ull * slot;
      atomicAdd(&v[0], n);   // (results unused: no-return atomics)
#pragma unroll
      for (int a = 0; a < 3; a++) atomicAdd(&v[1 + a], (S[a] >> 1) + n * b[a] * (1ull << 19));
      const unsigned long long* ms = smom + (unsigned long long)DM_MOM_WORDS * i;
      unsigned long long* md = mom + (unsigned long long)DM_MOM_WORDS * slot;
      const int A[6] = {0, 1, 2, 0, 0, 1}, B[6] = {0, 1, 2, 1, 2, 2};   // Mxx, Myy, Mzz, Mxy, Mxz, Myz
#pragma unroll
      for (int k = 0; k < 6; k++)
        atomicAdd(&md[k], (ms[k] >> 2) + b[A[k]] * (1ull << 18) * S[B[k]] + b[B[k]] * (1ull << 18) * S[A[k]] + n * b[A[k]] * b[B[k]] * (1ull << 38));
#pragma unroll
      for (int k = 6; k < DM_MOM_WORDS; k++) atomicAdd(&md[k], ms[k]);   // (V: signed sums, two's complement in the word)
    } else {
      ctr[1] = 1ull;   // (cannot happen at a load <= 1/2)
    }
  }
  dm_wave_count(&ctr[0], won);
}

void DenseMap::cascade(uint32_t top, const loamx_densemap_static_rule* rule, uint32_t first, std::vector<Snapshot>& out) {
  out.clear();
  cascade_each(top, rule, [&](uint32_t l, const DmTable& T, uint64_t occ) {
    if (l < first) return;
    out.emplace_back();
    snapshot_of(T, occ, out.back(), true);
  });
}

void DenseMap::cascade_each(uint32_t top, const loamx_densemap_static_rule* rule,
                            const std::function<void(uint32_t, const DmTable&, uint64_t)>& f) {
  read_counters();
  DevBuf<unsigned long long> ctr;
  ctr.reserve(2);
  DmTable below;   // level l - 1 once l >= 2
  const DmTable* src = &tab_;
  uint64_t src_occ = occ_.occ;
  for (uint32_t l = 1; l <= top; l++) {
    DmTable dst;
    dst.alloc(dm_slots_for(1024, src_occ), false, true);   // (<= the source's slots: no more voxels than the source holds)
    dst.clear(own_);
    LX_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned long long) * 2, own_));
    const dim3 grid((src->slots + 255u) / 256u), block(256);
    if (l == 1 && rule)
      hipLaunchKernelGGL(k_dm_coarsen<true>, grid, block, 0, own_, src->keys, src->vals, src->mom, src->aux, src->slots, *rule, dst.keys, dst.vals,
                         dst.mom, dst.mask(), dst.shift(), ctr.p);
    else
      hipLaunchKernelGGL(k_dm_coarsen<false>, grid, block, 0, own_, src->keys, src->vals, src->mom, (const uint32_t*)nullptr, src->slots,
                         loamx_densemap_static_rule{0u, 0u, 1u}, dst.keys, dst.vals, dst.mom, dst.mask(), dst.shift(), ctr.p);
    LX_HIP(hipGetLastError());
    unsigned long long c[2] = {0ull, 0ull};
    LX_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, own_));
    LX_HIP(hipStreamSynchronize(own_));
    if (c[1] != 0ull) throw Error(LOAMX_E_INTERNAL, "dense map: a coarse level's table overflowed");
    f(l, dst, c[0]);
    below.swap(dst);   // (the level below it, now in dst, is freed here: everything that read it has been waited for)
    src = &below;
    src_occ = c[0];
  }
}

void DenseMap::coarsen(uint32_t level, const loamx_densemap_static_rule* rule, Snapshot& S) {
  std::vector<Snapshot> out;
  cascade(level, rule, level, out);
  S = std::move(out.back());
}

void DenseMap::drop_coarse() {
  for (DmFrozen& F : coarse) F.drop();
  align_level = 0;
}

uint32_t DenseMap::frozen_levels() const {
  if (!frozen.valid()) return 0;
  uint32_t n = 1;
  while (n <= COARSE_LEVELS && coarse[n - 1].valid()) n++;
  return n;
}

void DenseMap::freeze_pyramid(const loamx_densemap_surfel_config& sc, const loamx_densemap_static_rule* rule,
                              const loamx_densemap_pyramid_config& pc, uint64_t* n_surfels) {
  // the coarse levels' entries on the host first, so that a failure of the cascade leaves the snapshots that stand
  std::vector<Snapshot> lv;
  if (pc.levels > 1u) cascade(pc.levels - 1u, rule, 1u, lv);
  std::vector<std::vector<unsigned long long>> keys(lv.size());
  std::vector<std::vector<float>> rec(lv.size());
  for (size_t k = 0; k < lv.size(); k++) {
    const double leaf = (double)level_leaf((uint32_t)k + 1u);
    for_each_voxel(lv[k], nullptr, [&](size_t j, const long long ia[3]) {
      loamx_surfel s;
      dm_surfel(leaf, ia, &lv[k].v[4 * j], &lv[k].mom[DM_MOM_WORDS * j], sc, 0, s);
      if (s.normal_x == 0.f && s.normal_y == 0.f && s.normal_z == 0.f) return;
      if (pc.max_curvature > 0.f && s.curvature > pc.max_curvature) return;   // (a coarse voxel that spans a corner is no plane)
      keys[k].push_back(lv[k].k[j]);
      const float six[6] = {s.x, s.y, s.z, s.normal_x, s.normal_y, s.normal_z};
      rec[k].insert(rec[k].end(), six, six + 6);
    });
  }
  const uint64_t n0 = freeze(sc, rule);   // (level 0: the snapshot of loamx_densemap_freeze; drops the coarse levels and the selection)
  if (n_surfels) n_surfels[0] = n0;
  for (size_t k = 0; k < lv.size(); k++) {
    coarse[k].build(keys[k].data(), rec[k].data(), keys[k].size(), own_);
    if (n_surfels) n_surfels[k + 1] = coarse[k].size();
  }
}

}  // namespace loamx

using namespace loamx;

extern "C" {

void loamx_densemap_pyramid_default_config(loamx_densemap_pyramid_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->levels = 3u;
  cfg->max_curvature = 0.f;
}

int loamx_densemap_coarsen(loamx_densemap* h, uint32_t level, const loamx_densemap_static_rule* rule, uint64_t* keys, uint64_t* vals,
                           uint64_t* mom, uint64_t capacity, uint64_t* n) {
  return guard([&]() {
    LX_REQUIRE(h && n && ((keys && vals && mom) || !capacity), "NULL argument");
    LX_REQUIRE(level >= 1u && level < LOAMX_PYRAMID_MAX_LEVELS, "level must be in [1, LOAMX_PYRAMID_MAX_LEVELS - 1]");
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    const loamx_densemap_static_rule* rp = checked_optional_rule(h, rule, r);
    DenseMap::Snapshot S;
    h->d.coarsen(level, rp, S);
    *n = S.idx.size();
    if (*n > capacity) return LOAMX_E_CAPACITY;
    for (size_t i = 0; i < S.idx.size(); i++) {   // ascending key order
      const size_t j = S.idx[i];
      keys[i] = S.k[j];
      for (int k = 0; k < 4; k++) vals[4 * i + k] = S.v[4 * j + k];
      for (int k = 0; k < DM_MOM_WORDS; k++) mom[DM_MOM_WORDS * i + k] = S.mom[DM_MOM_WORDS * j + k];
    }
    return LOAMX_OK;
  });
}

int loamx_densemap_freeze_pyramid(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                  const loamx_densemap_pyramid_config* pyramid, uint64_t* n_surfels) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const loamx_densemap_surfel_config c = checked_surfel_config(cfg);
    const loamx_densemap_pyramid_config pc = or_default(pyramid, loamx_densemap_pyramid_default_config);
    LX_REQUIRE(pc.levels >= 1u && pc.levels <= LOAMX_PYRAMID_MAX_LEVELS, "levels must be in [1, LOAMX_PYRAMID_MAX_LEVELS]");
    LX_REQUIRE(pc.max_curvature >= 0.f, "max_curvature must be >= 0 (0: no limit)");   // (NaN too)
    LX_REQUIRE_MOMENTS(h);
    loamx_densemap_static_rule r;
    h->d.freeze_pyramid(c, checked_optional_rule(h, rule, r), pc, n_surfels);
    return LOAMX_OK;
  });
}

int loamx_densemap_frozen_levels(loamx_densemap* h, uint32_t* levels) {
  return guard([&]() {
    LX_REQUIRE(h && levels, "NULL argument");
    *levels = h->d.frozen_levels();
    return LOAMX_OK;
  });
}

}  // extern "C"
