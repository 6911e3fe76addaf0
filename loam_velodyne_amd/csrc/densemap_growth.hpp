// The dense map's growth and capacity rule (densemap.hip; no HIP in here: tests/test_densemap_growth_cpu.py drives it on a CPU).
//
// The device never waits for the host, so the host decides on a bound: occ, the occupancy as of the last count it has seen, plus pend,
// every point enqueued since (each could be a voxel of its own).  Before an add of n records is enqueued the table is doubled until
// bound + n <= slots / 2; the true occupancy behind the add is at most that, so the load never passes one half, every probe loop on
// the device ends at a free slot and the overflow flag is never set.
// The count is refreshed without a wait: an add with no snapshot in flight starts one behind itself (a store of the counter into pinned
// memory and an event).  A snapshot carries the truth as of the add that started it; pend_snap collects what is enqueued behind it and
// becomes pend when it lands.  A call that waits for every add abandons the snapshot in flight (its event is not looked at again: occ
// and pend stay, which only keeps the bound above the truth) and usually goes on to read the exact count.
#pragma once
#include <cstdint>

namespace loamx {

// the smallest table, by doubling from `slots` (a power of two >= 2), that holds `records` at a load of one half.  Not clamped: the
// caller refuses a size it cannot index
inline uint64_t dm_slots_for(uint64_t slots, uint64_t records) {
  while (records > slots / 2) slots *= 2;
  return slots;
}

struct DmOccupancy {
  uint64_t occ = 0, pend = 0, pend_snap = 0;
  bool snap_pending = false;

  uint64_t bound() const { return occ + pend; }
  // the table size an add or a merge of n records needs before it is enqueued
  uint64_t slots_wanted(uint64_t slots, uint64_t n) const { return dm_slots_for(slots, bound() + n); }

  // an add of n points was enqueued.  true: no snapshot is in flight, the caller starts one behind the add
  bool enqueued(uint64_t n) {
    pend += n;
    if (snap_pending) { pend_snap += n; return false; }
    snap_pending = true;
    pend_snap = 0;
    return true;
  }
  // the snapshot in flight (snap_pending) has landed with the count v
  void snapshot_landed(uint64_t v) { occ = v; pend = pend_snap; snap_pending = false; }
  // the host waited for every add: the snapshot in flight, if any, is not looked at again
  void snapshot_abandoned() { snap_pending = false; }
  // the exact count, read behind a wait for every add
  void exact(uint64_t v) { occ = v; pend = pend_snap = 0; }
  // the table was cleared behind a wait for every add
  void reset() { *this = DmOccupancy(); }

  // capacity rule (include/loamx.h; max_voxels 0: no cap), decided before anything is enqueued.  false from the first: the bound is
  // over the cap, the caller reads the exact count and asks the second
  bool admits_by_bound(uint64_t n, uint64_t max_voxels) const { return !max_voxels || bound() + n <= max_voxels; }
  bool admits_exact(uint64_t n, uint64_t max_voxels) const { return !max_voxels || occ + n <= max_voxels; }
};

}  // namespace loamx
