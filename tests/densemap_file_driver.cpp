// Stand-alone driver of loam_velodyne_amd/csrc/densemap_file.hpp (the dense map's file: reader, writer, validator; no HIP), built by
// tests/test_densemap_file_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all and run over valid and corrupt files.
//   densemap_file_driver check FILE...        one line per file: "shallow <verdict> | deep <verdict>", a verdict being "OK count flags"
//                                             or "INVALID reason"
//   densemap_file_driver copy IN OUT          reads IN with the deep validation and writes its records to OUT through the writer
// Exit status 0 unless the arguments are wrong or a copy fails: a refused file is a verdict, not a failure of the driver.
#include <cstdio>
#include <cstring>
#include <string>

#include "densemap_file.hpp"

static volatile unsigned long long sink;

static std::string verdict(const char* path, bool deep) {
  loamx::DmFile f;
  const std::string e = loamx::dmf_read(path, deep, f);
  if (!e.empty()) return "INVALID " + e;
  if (deep && (f.keys.size() != f.h.count || f.vals.size() != 4 * f.h.count)) return "INVALID the reader kept another count than the header's";
  // touch every word the reader says it holds: the sanitizer sees a vector that is shorter than that
  unsigned long long sum = 0;
  for (uint64_t v : f.keys) sum += v;
  for (uint64_t v : f.vals) sum += v;
  for (uint32_t v : f.miss) sum += v;
  for (uint64_t v : f.mom) sum += v;
  sink = sum;
  return "OK " + std::to_string(f.h.count) + " " + std::to_string(f.h.flags);
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "check")) {
    for (int i = 2; i < argc; i++) printf("shallow %s | deep %s\n", verdict(argv[i], false).c_str(), verdict(argv[i], true).c_str());
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "copy")) {
    loamx::DmFile f;
    std::string e = loamx::dmf_read(argv[2], true, f);
    if (e.empty())
      e = loamx::dmf_write(argv[3], f.h, f.keys.data(), f.vals.data(), (f.h.flags & loamx::DMF_CARVING) ? f.miss.data() : nullptr,
                           (f.h.flags & loamx::DMF_MOMENTS) ? f.mom.data() : nullptr);
    if (!e.empty()) {
      fprintf(stderr, "%s\n", e.c_str());
      return 1;
    }
    return 0;
  }
  fprintf(stderr, "usage: densemap_file_driver check FILE... | copy IN OUT\n");
  return 2;
}
