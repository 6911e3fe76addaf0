// What one loamx_posegraph_optimize launches and when the host looks (PoseGraph::optimize, posegraph.hip; no HIP in here:
// tests/test_posegraph_cpu.py drives both schedules on a CPU through tests/posegraph_schedule_driver.cpp).
//
// The conjugate-gradient solve of one step.  begin() enqueues the start (x = 0, r = -g, z = M^-1 r, p = z, r.z); iterate() enqueues one
// iteration, a fixed sequence of plain launches.  The stop rule is evaluated on the device: the first iteration k with
// r_k.z_k <= tol^2 r_0.z_0 sets a `done` word (the start sets it when r_0.z_0 is not positive, k = 0), and every kernel enqueued behind
// it reads the word and returns, so the solution is the iterate at that k however many iterations were enqueued after it.  A look costs
// a host round trip, an idle iteration a few microseconds, so the iterations go out in batches of `batch`, followed by one look at
// (done, iterations run).  At most `cap` iterations are enqueued in all; reaching the cap without `done` ends the solve with the
// iterate at the cap.
//
// The Levenberg-Marquardt rule around it.  F is the cost at the linearisation point.  A step is solved with the damping lambda, applied
// to a backup of the poses, and its trial cost read together with max |delta|:
//   trial < F   accepted: F <- trial, lambda <- lambda * PG_LAMBDA_DOWN.  Converged (status 0) when max |delta| <= eps_step or
//               F_old - trial <= eps_cost * F_old; otherwise the next step linearises again.
//   otherwise   rejected (a NaN trial cost too): the poses are restored, the linearisation is kept.  A rejected step with
//               max |delta| <= eps_step also ends the run as converged: at the minimum the step is below the resolution asked for and
//               rounding alone decides the sign of the change in F.  Otherwise lambda <- lambda * PG_LAMBDA_UP (PG_LAMBDA_FIRST from
//               0); above PG_LAMBDA_CAP the run ends with status 2.
// max_iterations counts the steps tried, accepted or not; running out of them is status 1.
#pragma once
#include <algorithm>
#include <cstdint>

namespace loamx {

constexpr uint32_t PG_MAX_CG_BATCH = 64;
constexpr double PG_LAMBDA_UP = 10.0, PG_LAMBDA_DOWN = 0.1, PG_LAMBDA_FIRST = 1e-6, PG_LAMBDA_CAP = 1e12;

struct PgCgPlan {
  uint32_t batch;   // iterations per look, 1..PG_MAX_CG_BATCH
  uint32_t cap;     // iterations in all, >= 1
};
struct PgCgLook {
  uint32_t done;         // the stop rule was met
  uint32_t iterations;   // iterations that ran (those enqueued behind `done` do not count)
};
struct PgCgOutcome {
  uint32_t enqueued = 0, iterations = 0, looks = 0;
  bool stopped = false;   // by the stop rule (false: by the cap)
};

// Ops: cg_begin() enqueues the start; cg_iterate() enqueues one iteration; cg_look() waits and returns the two words.
template <class Ops> PgCgOutcome pg_cg_schedule(Ops&& ops, const PgCgPlan& p) {
  PgCgOutcome o;
  const uint32_t batch = std::min(std::max(p.batch, 1u), PG_MAX_CG_BATCH);
  ops.cg_begin();
  while (o.enqueued < p.cap && !o.stopped) {
    const uint32_t n = std::min(batch, p.cap - o.enqueued);
    for (uint32_t j = 0; j < n; j++) ops.cg_iterate();
    const PgCgLook s = ops.cg_look();
    o.looks++;
    o.enqueued += n;
    o.iterations = s.iterations;
    o.stopped = s.done != 0u;
  }
  return o;
}

struct PgLmRule {
  uint32_t max_iterations;
  double eps_step, eps_cost, lambda_init;
};
struct PgTrial {
  double cost, max_delta;
};
struct PgLmOutcome {
  uint32_t iterations = 0, accepted = 0;
  int status = 1;
  double cost_initial = 0.0, cost_final = 0.0, last_step = 0.0, lambda_final = 0.0;
};

// Ops: linearise() enqueues the linearisation at the current poses; cost() waits and returns its F; solve(lambda) runs the CG solve;
// apply() backs the poses up, applies the step and returns the trial cost and max |delta|; restore() puts the backup back.
template <class Ops> PgLmOutcome pg_lm_schedule(Ops&& ops, const PgLmRule& rule) {
  PgLmOutcome o;
  ops.linearise();
  double F = ops.cost();
  double lambda = rule.lambda_init;
  o.cost_initial = F;
  bool fresh = true;
  for (uint32_t it = 0; it < rule.max_iterations; it++) {
    if (!fresh) ops.linearise();
    fresh = true;
    ops.solve(lambda);
    const PgTrial t = ops.apply();
    o.iterations++;
    o.last_step = t.max_delta;
    if (t.cost < F) {
      const double before = F;
      F = t.cost;
      o.accepted++;
      fresh = false;
      lambda = lambda * PG_LAMBDA_DOWN;
      if (t.max_delta <= rule.eps_step || before - F <= rule.eps_cost * before) { o.status = 0; break; }
    } else {
      ops.restore();
      if (t.max_delta <= rule.eps_step) { o.status = 0; break; }
      lambda = lambda > 0.0 ? lambda * PG_LAMBDA_UP : PG_LAMBDA_FIRST;
      if (lambda > PG_LAMBDA_CAP) { o.status = 2; break; }
    }
  }
  o.cost_final = F;
  o.lambda_final = lambda;
  return o;
}

}  // namespace loamx
