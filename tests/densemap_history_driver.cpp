// Driver of loam_velodyne_amd/csrc/densemap_history.hpp for tests/test_densemap_history_cpu.py: the header used the way DenseMap uses
// it, with the HIP calls left out.  Built stand-alone with g++ -fsanitize=undefined.
//   log MAX_BYTES INITIAL_POINTS     stdin: "add N OX OY OZ" | "reset" | "call K"; one line of state per event
//   attempts INITIAL_SLOTS BEFORE    stdin: "OCC TOO_SMALL OVERFLOW" as read back after each attempt; one line per attempt
//   replay_call FIRST COUNT OX OY OZ [C0 .. C11]    the record of the call under the correction (none: NULL), floats as bit patterns
#include "densemap_history.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace loamx;

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static int run_log(uint64_t max_bytes, uint64_t initial_points) {
  DmHistory h;
  if (!h.configure(max_bytes, initial_points)) {
    printf("refused\n");
    return 0;
  }
  uint64_t blocks = 1;   // allocations of the block so far
  char op[16];
  while (scanf("%15s", op) == 1) {
    int admitted = -1;
    if (!strcmp(op, "add")) {
      unsigned long long n;
      float o[3];
      if (scanf("%llu %f %f %f", &n, &o[0], &o[1], &o[2]) != 4) return 2;
      // DenseMap::add: the cap first, then (a call that reaches the insert) the block, the copy, the record
      admitted = h.admits(n) ? 1 : 0;
      if (admitted && n) {
        const uint64_t want = h.capacity_for(n);
        if (want != h.capacity) { h.capacity = want; blocks++; }
        if (h.points + n > h.capacity) return 3;   // the copy would leave the block
        h.append((uint32_t)n, o);
      }
    } else if (!strcmp(op, "reset")) {
      h.clear();
    } else if (!strcmp(op, "call")) {
      unsigned long long k;
      if (scanf("%llu", &k) != 1 || k >= h.calls.size()) return 2;
      const DmHistoryCall& c = h.calls[k];
      printf("first=%" PRIu64 " count=%u o0=%08x o1=%08x o2=%08x\n", c.first, c.count, bits(c.origin[0]), bits(c.origin[1]), bits(c.origin[2]));
      continue;
    } else {
      return 2;
    }
    printf("admitted=%d capacity=%" PRIu64 " points=%" PRIu64 " calls=%zu blocks=%" PRIu64 "\n", admitted, h.capacity, h.points, h.calls.size(),
           blocks);
  }
  return 0;
}

static int run_attempts(uint64_t initial_slots, uint64_t before) {
  // DenseMap::rebuild: the loop over the table sizes
  unsigned long long occ, small, ovf;
  for (uint64_t slots = dm_rebuild_first_slots(initial_slots, before);; slots *= 2) {
    if (slots > DM_MAX_SLOTS) {
      printf("refused\n");
      return 0;
    }
    if (scanf("%llu %llu %llu", &occ, &small, &ovf) != 3) return 2;
    const bool failed = dm_rebuild_attempt_failed(slots, occ, small, ovf);
    printf("slots=%" PRIu64 " failed=%d\n", slots, failed ? 1 : 0);
    if (!failed) return 0;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "log" && argc == 4) return run_log(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  if (mode == "attempts" && argc == 4) return run_attempts(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  if (mode == "replay_call" && (argc == 7 || argc == 19)) {
    DmHistoryCall h;
    h.first = strtoull(argv[2], nullptr, 10);
    h.count = (uint32_t)strtoul(argv[3], nullptr, 10);
    for (int a = 0; a < 3; a++) h.origin[a] = strtof(argv[4 + a], nullptr);
    double c[12];
    for (int k = 0; argc == 19 && k < 12; k++) c[k] = strtod(argv[7 + k], nullptr);
    DmReplayCall r;
    if (!dm_replay_call(h, argc == 19 ? c : nullptr, r)) {
      printf("refused\n");
      return 0;
    }
    printf("first=%" PRIu64 " identity=%u", r.first, r.identity);
    for (int k = 0; k < 12; k++) printf(" m%d=%08x", k, bits(r.m[k]));
    for (int a = 0; a < 3; a++) printf(" o%d=%08x", a, bits(r.o[a]));
    printf("\n");
    return 0;
  }
  return 2;
}
