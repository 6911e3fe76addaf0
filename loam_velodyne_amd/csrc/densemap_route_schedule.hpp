// Which relaxation rounds one route call launches, and when the host looks (DmRouteT<K>::run, densemap_route_core.hpp, for the 2-D
// and the 3-D route alike; no HIP in here: tests/test_densemap_route_cpu.py drives it on a CPU through tests/route_schedule_driver.cpp).
//
// Round r = 0, 1, ... is one launch of the kind's relax kernel (k_dm_route_relax, k_dm_route3_relax) over every tile or brick.  A tile runs in round r only when it is marked in dirty plane
// r & 1, which the goals' seeding (r = 0) or the tiles of round r - 1 wrote; it clears its own mark there and marks its neighbours in
// plane (r + 1) & 1.  Nothing marks plane r & 1 during round r and only the owner clears, so the two planes never need a memset
// between rounds.  Every round has a slot of two counters: the tiles that ran and the tiles that marked a neighbour.
//
// A look costs a host round trip (~tens of microseconds), an idle round a few, so the rounds go out in batches of `batch`: the slots
// are zeroed, the rounds enqueued, the slots read back once.  A batch whose LAST round marked nothing ends the call: a round that marks
// nothing leaves no mark for any later round.  Otherwise the next batch follows, up to `cap` rounds in all (nx * nz + 2: after round r
// every cell whose cheapest path crosses at most r tile borders is final, a path crosses fewer borders than it has cells, and two more
// rounds see the last marks run dry).  Reaching the cap with marks left is reported (settled = false) and never loops on.
#pragma once
#include <algorithm>
#include <cstdint>

namespace loamx {

constexpr uint32_t ROUTE_MAX_BATCH = 64;   // slots of the counter block

struct RoutePlan {
  uint32_t batch;   // rounds per look, 1..ROUTE_MAX_BATCH
  uint64_t cap;     // rounds in all, >= 1
};
struct RouteSlot {
  uint32_t ran, marked;   // tiles of the round that ran; that marked a neighbour for the next round
};
struct RouteOutcome {
  uint64_t rounds = 0;          // launched
  uint64_t active_rounds = 0;   // of them, those in which a tile ran
  uint64_t tile_runs = 0;
  uint32_t looks = 0;
  bool settled = false;         // the last round looked at marked nothing
};

// Ops: begin(n) zeroes the first n slots; round(r, read_plane, mark_plane, slot) enqueues round r; look(n) waits and returns the n slots.
template <class Ops> RouteOutcome route_schedule(Ops&& ops, const RoutePlan& p) {
  RouteOutcome o;
  const uint64_t batch = std::min<uint64_t>(std::max<uint32_t>(p.batch, 1u), ROUTE_MAX_BATCH);
  while (o.rounds < p.cap && !o.settled) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(batch, p.cap - o.rounds);
    ops.begin(n);
    for (uint32_t j = 0; j < n; j++) ops.round(o.rounds + j, (uint32_t)((o.rounds + j) & 1u), (uint32_t)((o.rounds + j + 1u) & 1u), j);
    const RouteSlot* s = ops.look(n);
    o.looks++;
    for (uint32_t j = 0; j < n; j++) {
      o.tile_runs += s[j].ran;
      o.active_rounds += s[j].ran != 0u;
    }
    o.rounds += n;
    o.settled = s[n - 1].marked == 0u;
  }
  return o;
}

}  // namespace loamx
