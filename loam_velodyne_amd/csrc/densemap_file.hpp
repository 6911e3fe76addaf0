// The dense map's file ('LXDM', include/loamx.h: loamx_densemap_save and what follows it): reader, writer and validator.  No HIP in
// here: densemap_merge.hip includes it for save / load / merge_file / file_info, and tests/densemap_file_driver.cpp drives it on a CPU under
// the sanitizers.
//
// The reader takes untrusted bytes.  Its order of work is what keeps it safe: the 128 header bytes are read and checked first; the size
// the body must have is computed from the header's count in 64 bits, every step checked for overflow, and compared with the size of
// the file; only then is anything allocated (exactly the bytes the file was shown to hold) and read, and the record checks index
// nothing beyond count.  Every function answers with a message, empty when all is well, that names the offending field.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace loamx {

#if defined(__BYTE_ORDER__) && defined(__ORDER_LITTLE_ENDIAN__)
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the file is little-endian, and so must be the host that copies words into it");
#endif

constexpr uint32_t DMF_VERSION = 1u;
constexpr uint32_t DMF_CARVING = 1u, DMF_MOMENTS = 2u;
constexpr uint64_t DMF_HEADER_BYTES = 128u;
constexpr uint64_t DMF_MAX_COUNT = 1ull << 30;
constexpr int DMF_MOM_WORDS = 9;

struct DmFileHeader {
  uint32_t version = DMF_VERSION, flags = 0;
  float leaf = 0.f;
  uint64_t count = 0, offered = 0, dropped_range = 0, dropped_key = 0;
  uint64_t carve_stats[6] = {0, 0, 0, 0, 0, 0};
  float carve_max_range = 0.f;
  uint32_t ray_stride = 0, end_margin = 0, max_steps = 0;
};

// a file in memory: the header, and (when the body was asked for) the four arrays in file order
struct DmFile {
  DmFileHeader h;
  std::vector<uint64_t> keys, vals, mom;
  std::vector<uint32_t> miss;
};

// bytes of the miss array in the file (padded to a multiple of 8) and of the whole body; false when a step overflows 64 bits
inline bool dmf_body_bytes(uint32_t flags, uint64_t count, uint64_t& miss_bytes, uint64_t& body) {
  uint64_t words = 0, b = 0, per = 1u + 4u + ((flags & DMF_MOMENTS) ? (uint64_t)DMF_MOM_WORDS : 0u);   // 8-byte words per voxel
  miss_bytes = 0;
  if (__builtin_mul_overflow(count, per, &words) || __builtin_mul_overflow(words, (uint64_t)8, &b)) return false;
  if (flags & DMF_CARVING) {
    uint64_t m = 0;
    if (__builtin_mul_overflow(count, (uint64_t)4, &m) || __builtin_add_overflow(m, (uint64_t)7, &m)) return false;
    miss_bytes = m & ~(uint64_t)7;
    if (__builtin_add_overflow(b, miss_bytes, &b)) return false;
  }
  body = b;
  return true;
}

// what loamx_densemap_enable_carving accepts
inline std::string dmf_check_carve(float max_range, uint32_t ray_stride, uint32_t max_steps) {
  if (!(max_range >= 0.f) || !std::isfinite(max_range)) return "carve max_range must be >= 0";
  if (ray_stride < 1u) return "carve ray_stride must be >= 1";
  if (max_steps < 1u || max_steps > 65536u) return "carve max_steps must be in [1, 65536]";
  return "";
}

inline void dmf_put(unsigned char* p, const void* v, size_t n) { memcpy(p, v, n); }
template <class T> inline T dmf_get(const unsigned char* p) { T v; memcpy(&v, p, sizeof(T)); return v; }

inline void dmf_pack_header(const DmFileHeader& h, unsigned char out[DMF_HEADER_BYTES]) {
  memset(out, 0, DMF_HEADER_BYTES);
  memcpy(out, "LXDM", 4);
  dmf_put(out + 4, &h.version, 4);
  dmf_put(out + 8, &h.flags, 4);
  dmf_put(out + 12, &h.leaf, 4);
  dmf_put(out + 16, &h.count, 8);
  dmf_put(out + 24, &h.offered, 8);
  dmf_put(out + 32, &h.dropped_range, 8);
  dmf_put(out + 40, &h.dropped_key, 8);
  if (h.flags & DMF_CARVING) {
    dmf_put(out + 48, h.carve_stats, 48);
    dmf_put(out + 96, &h.carve_max_range, 4);
    dmf_put(out + 100, &h.ray_stride, 4);
    dmf_put(out + 104, &h.end_margin, 4);
    dmf_put(out + 108, &h.max_steps, 4);
  }
}

// the header's own checks (include/loamx.h, loamx_densemap_file_info with deep == 0, but for the size of the file)
inline std::string dmf_parse_header(const unsigned char in[DMF_HEADER_BYTES], DmFileHeader& h) {
  if (memcmp(in, "LXDM", 4) != 0) return "magic: not a dense map file";
  h.version = dmf_get<uint32_t>(in + 4);
  if (h.version != DMF_VERSION) return "version: " + std::to_string(h.version) + " is not supported";
  h.flags = dmf_get<uint32_t>(in + 8);
  if (h.flags & ~(DMF_CARVING | DMF_MOMENTS)) return "flags: unknown bits";
  h.leaf = dmf_get<float>(in + 12);
  if (!(h.leaf > 0.f) || !std::isfinite(h.leaf)) return "leaf: must be finite and > 0";
  h.count = dmf_get<uint64_t>(in + 16);
  if (h.count > DMF_MAX_COUNT) return "count: more than 2^30 voxels";
  h.offered = dmf_get<uint64_t>(in + 24);
  h.dropped_range = dmf_get<uint64_t>(in + 32);
  h.dropped_key = dmf_get<uint64_t>(in + 40);
  for (int k = 0; k < 6; k++) h.carve_stats[k] = dmf_get<uint64_t>(in + 48 + 8 * k);
  h.carve_max_range = dmf_get<float>(in + 96);
  h.ray_stride = dmf_get<uint32_t>(in + 100);
  h.end_margin = dmf_get<uint32_t>(in + 104);
  h.max_steps = dmf_get<uint32_t>(in + 108);
  if (h.flags & DMF_CARVING) {
    const std::string e = dmf_check_carve(h.carve_max_range, h.ray_stride, h.max_steps);
    if (!e.empty()) return e;
  } else {
    for (int k = 48; k < 112; k++)
      if (in[k]) return "carve fields: must be zero without carving";
  }
  for (int k = 112; k < 128; k++)
    if (in[k]) return "reserved bytes: must be zero";
  return "";
}

// the record checks of the deep validation over count keys and 4 * count value words
inline std::string dmf_check_records(const uint64_t* keys, const uint64_t* vals, uint64_t count) {
  const uint64_t fm = (1ull << 21) - 1ull;
  for (uint64_t i = 0; i < count; i++) {
    const uint64_t k = keys[i];
    if (k >> 63) return "keys[" + std::to_string(i) + "]: not below 2^63";
    for (int a = 0; a < 3; a++)
      if (((k >> (21 * a)) & fm) == 0ull) return "keys[" + std::to_string(i) + "]: a 21-bit field outside [1, 2^21 - 1]";
    if (i && !(keys[i - 1] < k)) return "keys[" + std::to_string(i) + "]: not strictly ascending";
    if (vals[4 * i] == 0ull) return "vals[" + std::to_string(4 * i) + "]: n must be >= 1";
  }
  return "";
}

// fread of exactly n bytes into p
inline bool dmf_read_exact(FILE* f, void* p, uint64_t n) { return n == 0 || fread(p, 1, (size_t)n, f) == (size_t)n; }

// the file at `path`: header and size checked; with deep, the body read into `out` and every record checked.  "" or the reason
inline std::string dmf_read(const char* path, bool deep, DmFile& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return std::string("cannot open ") + path;
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  unsigned char hdr[DMF_HEADER_BYTES];
  if (fread(hdr, 1, DMF_HEADER_BYTES, f) != DMF_HEADER_BYTES) return "size: shorter than the 128-byte header";
  std::string e = dmf_parse_header(hdr, out.h);
  if (!e.empty()) return e;
  uint64_t miss_bytes = 0, body = 0, want = 0;
  if (!dmf_body_bytes(out.h.flags, out.h.count, miss_bytes, body) || __builtin_add_overflow(body, DMF_HEADER_BYTES, &want))
    return "count: the size of the body overflows";
  if (fseeko(f, 0, SEEK_END) != 0) return "size: cannot seek";
  const off_t end = ftello(f);
  if (end < 0 || (uint64_t)end != want)
    return "size: the file holds " + std::to_string((long long)end) + " bytes, count and flags ask for " + std::to_string(want);
  if (!deep) return "";
  if (fseeko(f, (off_t)DMF_HEADER_BYTES, SEEK_SET) != 0) return "size: cannot seek";
  const uint64_t n = out.h.count;   // (n * 14 words were shown to exist in the file)
  out.keys.resize((size_t)n);
  out.vals.resize((size_t)(4 * n));
  out.miss.assign((out.h.flags & DMF_CARVING) ? (size_t)(miss_bytes / 4) : 0, 0u);
  out.mom.resize((out.h.flags & DMF_MOMENTS) ? (size_t)(DMF_MOM_WORDS * n) : 0);
  if (!dmf_read_exact(f, out.keys.data(), 8 * n) || !dmf_read_exact(f, out.vals.data(), 32 * n) ||
      !dmf_read_exact(f, out.miss.data(), miss_bytes) || !dmf_read_exact(f, out.mom.data(), 8 * out.mom.size()))
    return "size: the body could not be read";
  if ((out.h.flags & DMF_CARVING) && (n & 1ull) && out.miss[(size_t)n] != 0u) return "miss padding: must be zero";
  out.miss.resize((out.h.flags & DMF_CARVING) ? (size_t)n : 0);
  return dmf_check_records(out.keys.data(), out.vals.data(), n);
}

// header and records (ascending keys; miss / mom NULL without the feature) under the name `tmp` itself; a write that fails leaves
// nothing there.  "" or the reason (`path`: the name the messages speak of)
inline std::string dmf_write_part(const std::string& tmp, const char* path, const DmFileHeader& h, const uint64_t* keys, const uint64_t* vals,
                                  const uint32_t* miss, const uint64_t* mom) {
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return "cannot open " + tmp + " for writing";
  unsigned char hdr[DMF_HEADER_BYTES];
  dmf_pack_header(h, hdr);
  const size_t n = (size_t)h.count;
  bool ok = fwrite(hdr, 1, DMF_HEADER_BYTES, f) == DMF_HEADER_BYTES;
  ok = ok && (n == 0 || (fwrite(keys, 8, n, f) == n && fwrite(vals, 32, n, f) == n));
  if (ok && (h.flags & DMF_CARVING) && n) {
    const uint32_t zero = 0u;
    ok = fwrite(miss, 4, n, f) == n && (!(n & 1u) || fwrite(&zero, 4, 1, f) == 1);
  }
  if (ok && (h.flags & DMF_MOMENTS) && n) ok = fwrite(mom, 8 * DMF_MOM_WORDS, n, f) == n;
  const bool closed = fclose(f) == 0;
  if (ok && closed) return "";
  (void)remove(tmp.c_str());
  return std::string("write to ") + path + " failed";
}

// the same to a temporary name beside `path`, renamed when complete: a write that fails leaves nothing under `path`.  "" or the reason
inline std::string dmf_write(const char* path, const DmFileHeader& h, const uint64_t* keys, const uint64_t* vals, const uint32_t* miss,
                             const uint64_t* mom) {
  const std::string tmp = std::string(path) + ".part";
  const std::string e = dmf_write_part(tmp, path, h, keys, vals, miss, mom);
  if (!e.empty()) return e;
  if (rename(tmp.c_str(), path) == 0) return "";
  (void)remove(tmp.c_str());
  return std::string("write to ") + path + " failed";
}

}  // namespace loamx
