// Stand-alone driver of loam_velodyne_amd/csrc/densemap_route_schedule.hpp for tests/test_densemap_route_cpu.py (no device, no HIP).
// usage: route_schedule_driver BATCH CAP, then on stdin one line "ran marked" per simulated round (rounds beyond the input: 0 0).
// Prints what the schedule asks of its Ops, one line each, and its outcome.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "densemap_route_schedule.hpp"

using namespace loamx;

struct SimOps {
  std::vector<RouteSlot> rounds;   // the simulated counters of round r
  std::vector<RouteSlot> slots = std::vector<RouteSlot>(ROUTE_MAX_BATCH, RouteSlot{7u, 7u});   // (dirty until begin zeroes them)
  void begin(uint32_t n) {
    printf("begin %u\n", n);
    for (uint32_t j = 0; j < n; j++) slots[j] = RouteSlot{0u, 0u};
  }
  void round(uint64_t r, uint32_t read_plane, uint32_t mark_plane, uint32_t slot) {
    printf("round %llu read %u mark %u slot %u\n", (unsigned long long)r, read_plane, mark_plane, slot);
    if (slot >= ROUTE_MAX_BATCH) { printf("slot out of range\n"); exit(2); }
    const RouteSlot s = r < rounds.size() ? rounds[(size_t)r] : RouteSlot{0u, 0u};
    slots[slot].ran += s.ran;
    slots[slot].marked += s.marked;
  }
  const RouteSlot* look(uint32_t n) {
    printf("look %u\n", n);
    return slots.data();
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  SimOps ops;
  unsigned ran = 0, marked = 0;
  while (scanf("%u %u", &ran, &marked) == 2) ops.rounds.push_back(RouteSlot{ran, marked});
  const RouteOutcome o = route_schedule(ops, RoutePlan{(uint32_t)strtoul(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10)});
  printf("outcome rounds %llu active %llu tile_runs %llu looks %u settled %d\n", (unsigned long long)o.rounds,
         (unsigned long long)o.active_rounds, (unsigned long long)o.tile_runs, o.looks, o.settled ? 1 : 0);
  return 0;
}
