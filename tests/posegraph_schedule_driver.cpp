// Stand-alone driver of loam_velodyne_amd/csrc/posegraph_schedule.hpp for tests/test_posegraph_cpu.py (no device, no HIP).
// usage: posegraph_schedule_driver cg BATCH CAP STOP
//          STOP: the iteration whose stop test is met (0: the start already meets it; above CAP: never).
//        posegraph_schedule_driver lm MAX_ITERATIONS EPS_STEP EPS_COST LAMBDA_INIT F0
//          then on stdin one line "trial_cost max_delta" per step tried.
// Prints what the schedule asks of its Ops, one line each, and its outcome.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "posegraph_schedule.hpp"

using namespace loamx;

struct CgSim {
  uint32_t stop, ran = 0, done = 0;
  void cg_begin() {
    printf("begin\n");
    ran = 0;
    done = stop == 0u;
  }
  void cg_iterate() {
    printf("iterate\n");
    if (done) return;   // (the kernels behind `done` return at once)
    ran++;
    if (ran == stop) done = 1;
  }
  PgCgLook cg_look() {
    printf("look done %u iterations %u\n", done, ran);
    return PgCgLook{done, ran};
  }
};

struct LmSim {
  double f0;
  void linearise() { printf("linearise\n"); }
  double cost() {
    printf("cost\n");
    return f0;
  }
  void solve(double lambda) { printf("solve %.17g\n", lambda); }
  PgTrial apply() {
    PgTrial t{0.0, 0.0};
    if (scanf("%lf %lf", &t.cost, &t.max_delta) != 2) { printf("out of script\n"); exit(3); }
    printf("apply\n");
    return t;
  }
  void restore() { printf("restore\n"); }
};

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "cg")) {
    CgSim ops{(uint32_t)strtoul(argv[4], nullptr, 10)};
    const PgCgOutcome o = pg_cg_schedule(ops, PgCgPlan{(uint32_t)strtoul(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10)});
    printf("outcome enqueued %u iterations %u looks %u stopped %d\n", o.enqueued, o.iterations, o.looks, o.stopped ? 1 : 0);
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "lm")) {
    LmSim ops{strtod(argv[6], nullptr)};
    const PgLmOutcome o = pg_lm_schedule(ops, PgLmRule{(uint32_t)strtoul(argv[2], nullptr, 10), strtod(argv[3], nullptr), strtod(argv[4], nullptr),
                                                       strtod(argv[5], nullptr)});
    printf("outcome iterations %u accepted %u status %d cost_initial %.17g cost_final %.17g last_step %.17g lambda_final %.17g\n", o.iterations,
           o.accepted, o.status, o.cost_initial, o.cost_final, o.last_step, o.lambda_final);
    return 0;
  }
  return 1;
}
