// Stand-alone driver of loam_velodyne_amd/csrc/densemap_tiles.hpp (the dense map's regions and tiles on the host: window arithmetic,
// buckets, the merge of records; no HIP), built by tests/test_densemap_region_cpu.py with -fsanitize=address,undefined
// -fno-sanitize-recover=all and run over the files of the model.
//   densemap_tiles_driver merge A B OUT                     one line: "OK count" or "INVALID reason"
//   densemap_tiles_driver bucket IN T OUTDIR                the records of IN by tile into OUTDIR, one line per tile: "name count"
//   densemap_tiles_driver tiles T i...                      one line per index i: "tile lo hi name" of the tile (t, t, t) of (i, i, i)
// Exit status 0 unless the arguments are wrong or a file cannot be read or written: a refused merge is a verdict, not a failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "densemap_tiles.hpp"

using namespace loamx;

static int fail(const std::string& e) {
  fprintf(stderr, "%s\n", e.c_str());
  return 1;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "merge")) {
    const std::string e = dmt_file_merge(argv[2], argv[3], argv[4]);
    if (!e.empty()) {
      printf("INVALID %s\n", e.c_str());
      return 0;
    }
    DmFile f;
    const std::string r = dmf_read(argv[4], true, f);
    if (!r.empty()) return fail(r);
    printf("OK %llu\n", (unsigned long long)f.h.count);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "bucket")) {
    DmFile f;
    std::string e = dmf_read(argv[2], true, f);
    if (!e.empty()) return fail(e);
    DmTileBuckets b;
    e = dmt_bucket(f, (uint32_t)strtoul(argv[3], nullptr, 10), b);
    if (!e.empty()) return fail(e);
    for (const auto& kv : b) {
      const std::string name = dmt_tile_name(kv.first.data());
      int32_t back[3];
      if (!dmt_parse_tile_name(name, back) || back[0] != kv.first[0] || back[1] != kv.first[1] || back[2] != kv.first[2])
        return fail("the name of a tile does not parse back: " + name);
      e = dmt_write((std::string(argv[4]) + "/" + name).c_str(), kv.second);
      if (!e.empty()) return fail(e);
      printf("%s %llu\n", name.c_str(), (unsigned long long)kv.second.h.count);
    }
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "tiles")) {
    const uint32_t T = (uint32_t)strtoul(argv[2], nullptr, 10);
    for (int k = 3; k < argc; k++) {
      const int32_t i = (int32_t)strtol(argv[k], nullptr, 10), idx[3] = {i, i, i};
      int32_t t[3];
      DmRegion r;
      std::string e = dmt_tile_of(idx, T, t);
      if (e.empty()) e = dmt_tile_region(t, T, r);
      if (!e.empty()) return fail(e);
      printf("%d %d %d %s\n", t[0], r.lo[0], r.hi[0], dmt_tile_name(t).c_str());
    }
    return 0;
  }
  fprintf(stderr, "usage: densemap_tiles_driver merge A B OUT | bucket IN T OUTDIR | tiles T i...\n");
  return 2;
}
