// Which launches one registration run enqueues, and when (Registrar::run_iterations; no HIP in here: tests/test_reg_schedule.py drives it
// on a CPU).
//
// A run is up to max_iterations Gauss-Newton launches G_0 G_1 ... (k_gn_iter) and the registration of the full-resolution clouds F
// (k_transform_full, mode 0 / 1 / 2).  A launch over sweeps that have all converged returns at once (stats.done) and costs a few
// microseconds of the stream; a host round trip in the middle of the chain costs ~90.  Without early_exit the host therefore enqueues
// every G and never looks; the caller enqueues F0 behind them.  With early_exit (the caller blocks for the poses anyway):
//   * first chunk: max(pred_iters + ahead, 2) launches, never more than the bound — what the previous run needed plus `ahead`;
//   * F1 behind them, before the host has seen a flag: it registers the clouds of the sweeps that are done when it runs and marks each
//     with its tag (full_done[s] = tag != 0; k_pose_init zeroed the marks in front of the run);
//   * a look (mark = record the event, first_wait = the caller's hand-off, once, look = wait for the mirrors): every sweep done -> the
//     run is over, pred_iters becomes what the slowest sweep needed; the bucketed voxel stage gave up -> return at once, the caller
//     repeats the run; otherwise one more launch, pred_iters = launches so far + 1, look again, until the bound;
//   * a launch that reaches the bound is not looked at: nothing could follow it.
// Closing launch: F0 when no F1 went out (clouds wanted, zero iterations); F2 when an F1 went out and the FIRST look did not find every
// sweep done (no look at all included): the sweeps that converged later, or ran into the bound, still hold sensor-frame points.  F2
// skips every sweep whose mark is set — a mode-2 thread returns on full_done[s] != 0 before it reads a pose or a point, and nothing
// writes the marks in that mode — so it is a no-op for the sweeps F1 registered and each cloud is transformed exactly once.  Every sweep
// done at the first look: F1 ran behind the launches that finished them and took them all; no closing launch.
// Known and kept: once pred_iters + ahead reaches the bound the first chunk is the whole budget, no look is taken and
// pred_iters is never lowered again.
#pragma once
#include <algorithm>

namespace loamx {

struct RegPlan {
  bool early_exit;
  int max_iterations, pred_iters, ahead;
  bool want_full;   // full-resolution clouds are staged and their registration is not deferred
};
struct RegLook {
  bool gave_up, all_done;
  int need;   // the largest iteration count among the sweeps
};
struct RegOutcome {
  int launched = 0, pred_iters_next = 0, looks = 0;
  bool gave_up = false, all_done = false;   // all_done: the last look found every sweep done (poses and statistics are on the host)
  bool full_enqueued = false;               // the schedule took care of the full-resolution clouds
};

// Ops: gn(it) enqueues G_it; full(mode) enqueues F_mode; mark() records the point of the stream the next look waits for; first_wait() is
// called once, between the first mark and the first wait; look() waits and reports.
template <class Ops> RegOutcome reg_schedule(Ops&& ops, const RegPlan& p) {
  RegOutcome o;
  o.pred_iters_next = p.pred_iters;
  const int maxit = p.max_iterations;
  auto gn_to = [&](int end) { for (; o.launched < std::min(end, maxit); o.launched++) ops.gn(o.launched); };
  if (!p.early_exit) { gn_to(maxit); return o; }
  bool spec_full = false, settled_at_first_look = false;
  int chunk = std::min(std::max(p.pred_iters + p.ahead, 2), maxit);
  while (o.launched < maxit) {
    gn_to(o.launched + chunk);
    if (p.want_full && !spec_full) { ops.full(1); spec_full = true; }
    if (o.launched >= maxit) break;
    ops.mark();
    if (o.looks++ == 0) ops.first_wait();
    const RegLook l = ops.look();
    if (l.gave_up) { o.gave_up = true; return o; }
    o.all_done = l.all_done;
    if (o.looks == 1) settled_at_first_look = l.all_done;
    if (l.all_done) { o.pred_iters_next = l.need; break; }
    o.pred_iters_next = o.launched + 1;
    chunk = 1;
  }
  if (p.want_full) {
    if (!spec_full) ops.full(0);
    else if (!settled_at_first_look) ops.full(2);
    o.full_enqueued = true;
  }
  return o;
}

}  // namespace loamx
