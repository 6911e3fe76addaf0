// Drives odom_schedule_pairs() (loam_velodyne_amd/csrc/odom_schedule.hpp) against a scripted mirror and prints every call in order:
//   odom_schedule_driver MODE MAXP PRED N SILENT [MODE MAXP PRED N SILENT ...]      (one line of output per script)
// MODE all | lag | exact | lag2; N: every stream has converged once pair N - 1 has run (N > MAXP: never before the iteration bound);
// SILENT: the mirror stops answering at pair SILENT (wait_settled(k) fails for k >= SILENT; -1: it always answers).
// Output: C<k> / L<k> = correspondence / iteration launch of pair k, late = after_first(), W<k> / W<k>! = wait_settled(k) answered / did
// not, conv0 / conv1 = converged(), STUCK<k> = a wait for a pair whose iterations were never enqueued (a schedule that does that would
// spin into its time-out on the device), ret=<return value>.  The scripted device is as slow as the waits allow: the mirror shows the
// pairs the host has waited for and nothing behind them (the case in which every mode enqueues the most).
#include "odom_schedule.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Script {
  int maxp, n, silent;
  int lm_done = 0;   // pairs whose iterations have been enqueued
  int seen = 0;      // pairs the mirror has shown to be through
  void corr(int k) { printf("C%d ", k); }
  void lm(int k) { printf("L%d ", k); lm_done = k + 1; }
  void after_first() { printf("late "); }
  bool converged() {
    const bool c = seen >= std::min(n, maxp);
    printf("conv%d ", (int)c);
    return c;
  }
  bool wait_settled(int k) {
    if (silent >= 0 && k >= silent) { printf("W%d! ", k); return false; }
    if (k >= lm_done && k < std::min(n, maxp)) { printf("STUCK%d ", k); return false; }
    printf("W%d ", k);
    seen = std::max(seen, k + 1);
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5) return 2;
  for (char** a = argv + 1; a < argv + argc; a += 5) {
    loamx::OdomPairMode mode;
    if (!strcmp(a[0], "all")) mode = loamx::OdomPairMode::All;
    else if (!strcmp(a[0], "lag")) mode = loamx::OdomPairMode::Lag;
    else if (!strcmp(a[0], "exact")) mode = loamx::OdomPairMode::Exact;
    else if (!strcmp(a[0], "lag2")) mode = loamx::OdomPairMode::Lag2;
    else return 2;
    Script s{atoi(a[1]), atoi(a[3]), atoi(a[4])};
    const int ret = loamx::odom_schedule_pairs(s, mode, s.maxp, atoi(a[2]));
    printf("ret=%d\n", ret);
  }
  return 0;
}
