// Drives reg_schedule() (loam_velodyne_amd/csrc/reg_schedule.hpp) against a scripted mirror and prints every call in order.  One script
// per line of standard input, one line of output per script:
//   EARLY MAXIT PRED AHEAD WANT GAVEUP NEED[,NEED...]
// EARLY / WANT: early_exit / want_full (0 | 1); NEED: sweep s is done once NEED[s] launches have run; GAVEUP 1: the first look finds that
// the bucketed voxel stage gave up.  The scripted device has run, at a look, every launch enqueued so far (a look waits for the event
// behind them); a sweep's iteration count is min(NEED[s], launches run).
// Output: G<it> = gn(it), F<mode> = full(mode), mark, late = first_wait(), wait = look(), then the outcome:
//   launched=<n> pred=<pred_iters_next> looks=<n> gave_up=<0|1> all_done=<0|1> full=<0|1>
#include "reg_schedule.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Script {
  std::vector<int> need;
  bool gave_up_at_first_look;
  int launched = 0, looks = 0;
  void gn(int it) { printf("G%d ", it); launched++; }
  void full(int mode) { printf("F%d ", mode); }
  void mark() { printf("mark "); }
  void first_wait() { printf("late "); }
  loamx::RegLook look() {
    printf("wait ");
    loamx::RegLook l{looks++ == 0 && gave_up_at_first_look, true, 0};
    for (int n : need) {
      l.all_done = l.all_done && n <= launched;
      l.need = std::max(l.need, std::min(n, launched));
    }
    return l;
  }
};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int early, maxit, pred, ahead, want, gave_up;
    std::string needs;
    if (!(in >> early >> maxit >> pred >> ahead >> want >> gave_up >> needs)) return 2;
    Script s{{}, gave_up != 0};
    std::istringstream ns(needs);
    for (std::string tok; std::getline(ns, tok, ',');) s.need.push_back(std::stoi(tok));
    const loamx::RegOutcome o = loamx::reg_schedule(s, loamx::RegPlan{early != 0, maxit, pred, ahead, want != 0});
    printf("launched=%d pred=%d looks=%d gave_up=%d all_done=%d full=%d\n", o.launched, o.pred_iters_next, o.looks, (int)o.gave_up, (int)o.all_done,
           (int)o.full_enqueued);
  }
  return 0;
}
