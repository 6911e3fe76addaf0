// Drives loam_velodyne_amd/csrc/densemap_growth.hpp on a CPU (tests/test_densemap_growth_cpu.py): Host below is DenseMap's use of the
// header with the HIP calls left out, statement for statement (admit, grow_for, enqueue_add, poll_snapshot, wait_adds, read_counters,
// merge, reset).
//   replay SLOTS MAX_VOXELS   events on stdin, one line of state per event on stdout:
//       add N V        an add of N points; V: the exact count, should admission ask for it
//       land V         the snapshot in flight, if any, has landed with V
//       wait           a call that waits for every add
//       read V         a call that reads the exact count V
//       merge S V V2   a merge of S records: exact count V before it, V2 behind it
//       size SLOTS N   the table size N records need by doubling from SLOTS (the load path, the frozen snapshot)
//       reset
//   (no argument)             the simulated device, one line per scenario
#include "densemap_growth.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>

using namespace loamx;

struct Host {
  DmOccupancy o;
  uint64_t slots, max_voxels;
  // what the last event decided (-1: not asked)
  long long want = -1;
  int start = -1, by_bound = -1, admitted = -1, refused = 0;

  void wait_adds() { o.snapshot_abandoned(); }
  void read_counters(uint64_t v) { wait_adds(); o.exact(v); }
  void poll_snapshot(uint64_t v) { if (o.snap_pending) o.snapshot_landed(v); }
  bool admit(uint64_t n, uint64_t v) {
    by_bound = o.admits_by_bound(n, max_voxels) ? 1 : 0;
    if (by_bound) return true;
    read_counters(v);
    return o.admits_exact(n, max_voxels);
  }
  bool grow_for(uint64_t n) {
    const uint64_t w = o.slots_wanted(slots, n);
    want = (long long)w;
    if (w > (1ull << 31)) { refused = 1; return false; }   // (DenseMap throws here: nothing has changed)
    slots = w;
    return true;
  }
  void add(uint64_t n, uint64_t v) {
    admitted = admit(n, v) ? 1 : 0;
    if (!admitted) return;
    if (!grow_for(n)) return;
    start = o.enqueued(n) ? 1 : 0;
  }
  void merge(uint64_t s_occ, uint64_t v, uint64_t v2) {
    read_counters(v);
    admitted = o.admits_exact(s_occ, max_voxels) ? 1 : 0;
    if (!admitted) return;
    if (!grow_for(s_occ)) return;
    read_counters(v2);
  }
  void reset() { wait_adds(); o.reset(); }
  void begin_event() { want = -1; start = by_bound = admitted = -1; refused = 0; }
  void print() const {
    printf("occ=%" PRIu64 " pend=%" PRIu64 " pend_snap=%" PRIu64 " snap_pending=%d slots=%" PRIu64 " want=%lld start=%d by_bound=%d admitted=%d refused=%d\n",
           o.occ, o.pend, o.pend_snap, o.snap_pending ? 1 : 0, slots, want, start, by_bound, admitted, refused);
  }
};

static int replay(uint64_t slots, uint64_t max_voxels) {
  Host h;
  h.slots = slots;
  h.max_voxels = max_voxels;
  char op[16];
  while (scanf("%15s", op) == 1) {
    uint64_t a = 0, b = 0, c = 0;
    h.begin_event();
    if (!strcmp(op, "add") && scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) h.add(a, b);
    else if (!strcmp(op, "land") && scanf("%" SCNu64, &a) == 1) h.poll_snapshot(a);
    else if (!strcmp(op, "wait")) h.wait_adds();
    else if (!strcmp(op, "read") && scanf("%" SCNu64, &a) == 1) h.read_counters(a);
    else if (!strcmp(op, "merge") && scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) h.merge(a, b, c);
    else if (!strcmp(op, "size") && scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) h.want = (long long)dm_slots_for(a, b);
    else if (!strcmp(op, "reset")) h.reset();
    else { fprintf(stderr, "bad event %s\n", op); return 2; }
    h.print();
  }
  return 0;
}

// The simulated device: adds run in order, `truth` is the occupancy behind the last one.  new_per_1024: how many of 1024 points make
// a voxel of their own (1024: every point; 0: every point falls into one voxel; -1: a seeded fraction per add).  A snapshot carries
// the truth behind the add that started it and lands a few events later, unless a wait abandons it first
static void simulate(const char* name, int new_per_1024, uint32_t seed) {
  std::mt19937 rng(seed);
  Host h;
  h.slots = 1024;
  h.max_voxels = 0;
  uint64_t truth = 0, snap_value = 0;
  int snap_due = 0;   // events until the snapshot in flight lands
  uint64_t adds = 0, grows = 0, landed = 0, abandoned = 0, exact_reads = 0, over_half = 0, bound_below_truth = 0, max_load_x1000 = 0;
  for (int ev = 0; ev < 4000; ev++) {
    const uint32_t r = rng() % 100;
    h.begin_event();
    if (h.o.snap_pending && --snap_due <= 0) {
      h.poll_snapshot(snap_value);
      landed++;
    }
    if (r < 80) {
      const uint64_t n = rng() % 7 == 0 ? 0 : rng() % 3000;
      const uint64_t before = h.slots;
      h.add(n, truth);
      adds++;
      grows += h.slots != before;
      const int frac = new_per_1024 >= 0 ? new_per_1024 : (int)(rng() % 1025);
      uint64_t fresh = n * (uint64_t)frac / 1024;
      if (n && !fresh && truth == 0) fresh = 1;   // (the first point of a map makes a voxel)
      truth += fresh;
      if (h.start == 1) { snap_value = truth; snap_due = 1 + (int)(rng() % 6); }
      if (2 * truth > h.slots) over_half++;
      if (truth * 1000 / h.slots > max_load_x1000) max_load_x1000 = truth * 1000 / h.slots;
    } else if (r < 90) {
      abandoned += h.o.snap_pending;
      h.wait_adds();
    } else {
      abandoned += h.o.snap_pending;
      h.read_counters(truth);
      exact_reads++;
    }
    if (h.o.bound() < truth) bound_below_truth++;
  }
  printf("%s adds=%" PRIu64 " grows=%" PRIu64 " landed=%" PRIu64 " abandoned=%" PRIu64 " exact_reads=%" PRIu64 " truth=%" PRIu64 " slots=%" PRIu64
         " max_load_x1000=%" PRIu64 " over_half=%" PRIu64 " bound_below_truth=%" PRIu64 "\n",
         name, adds, grows, landed, abandoned, exact_reads, truth, h.slots, max_load_x1000, over_half, bound_below_truth);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "replay")) return replay(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  simulate("every_point_new", 1024, 1u);
  simulate("every_point_same", 0, 2u);
  simulate("mixed", -1, 3u);
  return 0;
}
