// Which launches one odometry pass enqueues, and when (OdometryBatch::process; no HIP in here: tests/test_odom_schedule.py drives it on a CPU).
//
// A pass is up to maxp launch pairs, pair k = correspondences C_k + up to five iterations L_k, i.e. the launches C_0 L_0 C_1 L_1 ... in this
// order.  The reference leaves its loop when the stop test fires (BasicLaserOdometry.cpp:613-620); launches enqueued behind a sweep that
// has converged cost ~10 us each, so they are enqueued as they turn out to be needed: the host reads from the pinned mirror (k_odom_lm
// writes a stream's state there at the end of every launch) whether a pair left any stream unconverged.  Round 5 enqueued all five pairs
// up front (1.6 empty pairs per pass on average).  Result-neutral by construction: a launch that is not enqueued would have returned at
// its first instruction (pb.done / the iteration bound).
#pragma once
#include <algorithm>

namespace loamx {

// LOAMX_ODOM_PAIRS: how many launches run AHEAD of what the mirror has shown to be needed
enum class OdomPairMode {
  All,     // every pair up front (round 5)
  Lag,     // (default) ONE launch, the next pair's correspondences: when pair k's iterations have ended the host knows whether pair k + 1 is
           // needed; if so it enqueues L_k+1 and C_k+2 while C_k+1 runs — the queue never runs dry; if not, C_k+1 is the pass's only empty launch
  Exact,   // none: pred_pairs pairs (what the previous sweep needed) to begin with, then a host round trip in front of every further pair
  Lag2,    // one PAIR (round 6's first form)
};

// Ops: corr(k) / lm(k) enqueue C_k / L_k; wait_settled(k) waits until every stream is through pair k (false: the mirror did not answer in
// time); converged(): no stream has anything left to iterate; after_first() is called once, behind the launches that need no answer.
// Returns the number of pairs whose iterations were enqueued.
template <class Ops> int odom_schedule_pairs(Ops&& ops, OdomPairMode mode, int maxp, int pred_pairs) {
  const int total = 2 * maxp, ahead = mode == OdomPairMode::Lag ? 1 : mode == OdomPairMode::Lag2 ? 2 : 0;
  int n = 0;   // launches enqueued: launch j is C_j/2 (j even) or L_j/2 (j odd)
  auto enqueue_to = [&](int end) { for (; n < std::min(end, total); n++) (n & 1) ? ops.lm(n / 2) : ops.corr(n / 2); };
  enqueue_to(mode == OdomPairMode::All ? total : 2 * (mode == OdomPairMode::Exact ? std::max(1, pred_pairs) : 1) + ahead);
  ops.after_first();
  bool blind = false;   // the mirror did not answer in time: everything that is left, unconditionally (always correct)
  while (n < total) {
    if (!blind) {
      if (!ops.wait_settled((n - ahead) / 2 - 1)) blind = true;   // (the last pair of the launches that are not ahead of need)
      else if (ops.converged()) break;
    }
    enqueue_to(n + 2);
  }
  return n / 2;
}

}  // namespace loamx
