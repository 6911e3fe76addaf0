// Drives loamx::LookAhead and lookahead_window (csrc/odom_lookahead.hpp) on a CPU: one line per scenario, read by
// tests/test_odom_lookahead.py.  Jobs are plain callables that record (chain, step) and are gated with atomics: what a scenario asserts
// never depends on timing.  One figure is not forced, `returned_early` of the park / reset scenarios: a helper gives a wrong gate time
// to return before it opens the job's gate, which can miss such a gate but never blames a right one; the forced evidence there is
// `job_ended_at_return` and the positions.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include "odom_lookahead.hpp"

using loamx::LookAhead;

// (the driver's own polling yields: on a machine with fewer cores than threads a poller must not burn its time slice)
static void spin_for(const std::atomic<bool>& flag) {
  while (!flag.load(std::memory_order_acquire)) std::this_thread::yield();
}
template <class P> static void spin_while_not(P&& p) {
  while (!p()) std::this_thread::yield();
}
static void work(int turns) {
  for (int k = 0; k < turns; k++) std::this_thread::yield();
}
// "ok" when f returns, "stopped" for the gate's own "a chain stopped before the requested step", what() of anything else
template <class F> static std::string outcome(F&& f) {
  try { f(); } catch (const std::logic_error&) { return "stopped"; } catch (const std::exception& e) { return e.what(); }
  return "ok";
}

// what the jobs of one scenario record: per chain the steps it started, in order (inline runs of the caller included)
struct Log {
  std::mutex mu;
  std::vector<std::vector<int>> started;
  explicit Log(uint32_t n) : started(n) {}
  void add(uint32_t g, int k) { std::lock_guard<std::mutex> lk(mu); started[g].push_back(k); }
  std::string str(uint32_t g) {   // "0,1,2"
    std::lock_guard<std::mutex> lk(mu);
    std::string s;
    for (int k : started[g]) s += (s.empty() ? "" : ",") + std::to_string(k);
    return s.empty() ? "-" : s;
  }
};
static const auto no_start = [] {};

// 1. order and bound: the caller mimics step() — allow up to min(t + D, last), wait for t
static void order(uint32_t n_chains, int D) {
  const int N = 12, last = N - 1;
  Log log(n_chains);
  std::vector<std::unique_ptr<std::atomic<bool>[]>> ended;
  for (uint32_t g = 0; g < n_chains; g++) {
    ended.emplace_back(new std::atomic<bool>[N]);
    for (int k = 0; k < N; k++) ended[g][k].store(false);
  }
  std::atomic<bool> above_limit{false};
  std::atomic<int> thread_starts{0};
  LookAhead* gate = nullptr;
  LookAhead la(
      n_chains,
      [&](uint32_t g, int k) {
        if (k > gate->limit()) above_limit.store(true);   // (the limit only rises in this scenario)
        log.add(g, k);
        work((int)g * 150 + (k % 3) * 100);   // unequal job lengths
        ended[g][k].store(true, std::memory_order_release);
      },
      [&] { thread_starts++; });
  gate = &la;
  bool wait_ok = true;
  for (int t = 0; t < N; t++) {
    la.allow(std::min(t + D, last));
    la.wait(t);
    for (uint32_t g = 0; g < n_chains; g++) wait_ok = wait_ok && ended[g][t].load(std::memory_order_acquire) && la.done(g) >= t;
  }
  const int drained = la.drain();
  std::string want;
  for (int k = 0; k < N; k++) want += (k ? "," : "") + std::to_string(k);
  bool in_order_once = true;
  for (uint32_t g = 0; g < n_chains; g++) in_order_once = in_order_once && log.str(g) == want;
  printf("order_c%u_d%d in_order_once=%d above_limit=%d wait_ok=%d drained=%d done_max=%d thread_starts=%d\n", n_chains, D, (int)in_order_once,
         (int)above_limit.load(), (int)wait_ok, drained, la.done_max(), thread_starts.load());
}

// runs `blocking` (park / reset) on this thread while a job is held at `gate`: a helper opens the gate only after it has given a wrong
// implementation time to return; `returned` is what it saw just before it opened the gate
template <class F> static bool with_late_release(std::atomic<bool>& gate, F&& blocking) {
  std::atomic<bool> begun{false}, returned{false};
  bool early = false;
  std::thread helper([&] {
    spin_for(begun);
    work(20000);
    early = returned.load(std::memory_order_acquire);
    gate.store(true, std::memory_order_release);
  });
  begun.store(true, std::memory_order_release);
  blocking();
  returned.store(true, std::memory_order_release);
  helper.join();
  return early;
}

// 2. park while a worker is inside step 2: the positions are the ones AFTER that step
static void park_mid_flight() {
  Log log(2);
  std::atomic<bool> entered{false}, gate{false}, job_ended{false};
  LookAhead la(
      2,
      [&](uint32_t g, int k) {
        log.add(g, k);
        if (g == 0 && k == 2) { entered.store(true, std::memory_order_release); spin_for(gate); job_ended.store(true, std::memory_order_release); }
      },
      no_start);
  la.allow(2);
  spin_for(entered);
  spin_while_not([&] { return la.done(1) >= 2; });
  const int done0_inside = la.done(0);
  bool ended_at_return = false;
  const bool early = with_late_release(gate, [&] { la.park(-1); ended_at_return = job_ended.load(std::memory_order_acquire); });
  const int d0 = la.done(0), d1 = la.done(1), lim = la.limit();
  const bool jumped3 = la.jumped(3);
  for (int t = 3; t <= 4; t++)   // the no-look-ahead path of step(): the caller runs the steps itself
    for (uint32_t g = 0; g < 2; g++)
      if (t > la.done(g)) { log.add(g, t); la.ran_inline(g, t); }
  la.allow(6);
  la.wait(6);
  printf("park_mid_flight done0_inside=%d returned_early=%d job_ended_at_return=%d done0=%d done1=%d limit=%d jumped3=%d c0=%s c1=%s\n",
         done0_inside, (int)early, (int)ended_at_return, d0, d1, lim, (int)jumped3, log.str(0).c_str(), log.str(1).c_str());
}

// 3. a jump to step 3: chain 0 has finished it, chain 1 stands at it, chain 2 is behind — only chain 2 is moved
static void jump() {
  Log log(3);
  LookAhead la(3, [&](uint32_t g, int k) { log.add(g, k); }, no_start);
  const bool j0 = la.jumped(0);
  la.ran_inline(0, 3);   // (the workers have not been started: the caller sets the positions)
  la.ran_inline(1, 2);
  la.ran_inline(2, 0);
  const bool j3 = la.jumped(3), j1 = la.jumped(1), j4 = la.jumped(4);
  la.park(3);
  const int d0 = la.done(0), d1 = la.done(1), d2 = la.done(2);
  const bool j3_after = la.jumped(3);
  la.allow(4);
  la.wait(4);
  printf("jump jumped0_fresh=%d jumped3=%d jumped1=%d jumped4=%d done0=%d done1=%d done2=%d jumped3_after=%d c0=%s c1=%s c2=%s\n", (int)j0, (int)j3, (int)j1,
         (int)j4, d0, d1, d2, (int)j3_after, log.str(0).c_str(), log.str(1).c_str(), log.str(2).c_str());
}

// 4a. chain 1 throws in step 3 while chain 0 is inside step 4, allowed up to 6
static void failing_step() {
  Log log(2);
  std::atomic<bool> in_k{false}, fail_go{false}, in_4{false}, go_4{false}, fail{true};
  LookAhead la(
      2,
      [&](uint32_t g, int k) {
        log.add(g, k);
        if (g == 1 && k == 3 && fail.load()) { in_k.store(true, std::memory_order_release); spin_for(fail_go); throw std::runtime_error("E1"); }
        if (g == 0 && k == 4 && !go_4.load()) { in_4.store(true, std::memory_order_release); spin_for(go_4); }
      },
      no_start);
  la.allow(6);
  spin_for(in_k);
  spin_for(in_4);
  const std::string w_pub = outcome([&] { la.wait(2); });   // published by both chains; the failing step is still running
  fail_go.store(true, std::memory_order_release);
  spin_while_not([&] { return la.limit() == -1; });         // the error is kept: every chain stops
  go_4.store(true, std::memory_order_release);
  const std::string w_k = outcome([&] { la.wait(3); });     // (returns once chain 0 has gone idle too)
  const std::string c0_stopped = log.str(0);
  const int d0 = la.done(0), d1 = la.done(1);
  const std::string w_pub2 = outcome([&] { la.wait(2); }), w_k2 = outcome([&] { la.wait(3); });
  fail.store(false);
  la.allow(6);
  const std::string w_end = outcome([&] { la.wait(6); });
  printf("failing_step wait_published=%s wait_k=%s c0_when_stopped=%s done0=%d done1=%d wait_published_again=%s wait_k_again=%s wait_end=%s c0=%s c1=%s\n",
         w_pub.c_str(), w_k.c_str(), c0_stopped.c_str(), d0, d1, w_pub2.c_str(), w_k2.c_str(), w_end.c_str(), log.str(0).c_str(), log.str(1).c_str());
}

// 4b. both chains throw in step 2, chain 1 first and only once chain 0 is inside its step 2: the first error is the one reported, the
// second is dropped (the wait for step 2 ends when both chains are idle)
static void two_failing() {
  std::atomic<bool> in_2{false}, go0{false}, e0_thrown{false};
  LookAhead la(
      2,
      [&](uint32_t g, int k) {
        if (k != 2) return;
        if (g == 0) {
          in_2.store(true, std::memory_order_release);
          spin_for(go0);
          e0_thrown.store(true, std::memory_order_release);
          throw std::runtime_error("E0");
        }
        spin_for(in_2);
        throw std::runtime_error("E1");
      },
      no_start);
  la.allow(5);
  spin_while_not([&] { return la.limit() == -1; });   // E1 is kept
  go0.store(true, std::memory_order_release);
  const std::string w1 = outcome([&] { la.wait(2); });
  const bool e0 = e0_thrown.load(std::memory_order_acquire);
  const std::string w2 = outcome([&] { la.wait(2); }), w3 = outcome([&] { la.wait(1); });
  printf("two_failing wait_k=%s e0_thrown=%d wait_k_again=%s wait_published=%s done_min=%d done_max=%d\n", w1.c_str(), (int)e0, w2.c_str(), w3.c_str(),
         la.done_min(), la.done_max());
}

// 4c. a kept error comes out of the FIRST wait() behind it, also one for a step that is published (Pipeline::wait_odometry did so)
static void error_first_wait() {
  std::atomic<bool> go{false};
  LookAhead la(2, [&](uint32_t g, int k) { if (g == 1 && k == 2) { spin_for(go); throw std::runtime_error("E"); } }, no_start);
  la.allow(5);
  spin_while_not([&] { return la.done_min() >= 0; });   // (step 0 is published by both chains before chain 1 fails)
  go.store(true, std::memory_order_release);
  spin_while_not([&] { return la.limit() == -1; });
  const std::string w1 = outcome([&] { la.wait(0); }), w2 = outcome([&] { la.wait(0); });
  printf("error_first_wait wait_published=%s wait_again=%s\n", w1.c_str(), w2.c_str());
}

// 4d. park drops a kept error
static void park_drops_error() {
  Log log(2);
  std::atomic<bool> fail{true};
  LookAhead la(2, [&](uint32_t g, int k) { log.add(g, k); if (g == 1 && k == 1 && fail.load()) throw std::runtime_error("E"); }, no_start);
  la.allow(1);
  spin_while_not([&] { return la.limit() == -1; });
  la.park(-1);
  fail.store(false);
  la.allow(2);
  const std::string w = outcome([&] { la.wait(2); });
  printf("park_drops_error wait=%s c0=%s c1=%s\n", w.c_str(), log.str(0).c_str(), log.str(1).c_str());
}

// 5. reset while a worker is inside step 1: it waits, then every chain restarts at 0
static void reset_running() {
  Log log(2);
  std::atomic<bool> entered{false}, gate{false}, job_ended{false};
  LookAhead la(
      2,
      [&](uint32_t g, int k) {
        log.add(g, k);
        if (g == 0 && k == 1 && !gate.load()) { entered.store(true, std::memory_order_release); spin_for(gate); job_ended.store(true, std::memory_order_release); }
      },
      no_start);
  la.allow(3);
  spin_for(entered);
  bool ended_at_return = false;
  const bool early = with_late_release(gate, [&] { la.reset(); ended_at_return = job_ended.load(std::memory_order_acquire); });
  const int dmin = la.done_min(), dmax = la.done_max(), lim = la.limit();
  const bool j0 = la.jumped(0);
  const std::string c0_before = log.str(0);
  la.allow(1);
  la.wait(1);
  const std::string c0 = log.str(0);
  printf("reset_running returned_early=%d job_ended_at_return=%d done_min=%d done_max=%d limit=%d jumped0=%d c0_before=%s c0=%s\n", (int)early,
         (int)ended_at_return, dmin, dmax, lim, (int)j0, c0_before.c_str(), c0.c_str());
}

// 6. the destructor ends: workers never started, blocked on the condition variable, still spinning, inside a job, with an untaken error
static void destructor() {
  { LookAhead never(2, [](uint32_t, int) {}, no_start); }
  {
    LookAhead blocked(2, [](uint32_t, int) {}, no_start, std::chrono::microseconds(0));   // (no spin phase: the workers sleep at once)
    blocked.allow(0);
    blocked.wait(0);
  }
  {
    LookAhead spinning(2, [](uint32_t, int) {}, no_start, std::chrono::milliseconds(50));
    spinning.allow(0);
    spinning.wait(0);
  }
  std::atomic<bool> started{false}, finished{false};
  {
    LookAhead running(2, [&](uint32_t g, int) {
      if (g != 0) return;
      started.store(true, std::memory_order_release);
      work(20000);   // (so that the destructor finds the job running)
      finished.store(true, std::memory_order_release);
    }, no_start);
    running.allow(0);
    spin_for(started);
  }
  const bool job_finished = finished.load();
  {
    LookAhead failed(2, [](uint32_t, int) { throw std::runtime_error("dropped"); }, no_start);
    failed.allow(0);
    spin_while_not([&] { return failed.limit() == -1; });
  }
  printf("destructor never=ok blocked=ok spinning=ok job_finished=%d untaken=ok\n", (int)job_finished);
}

// 7. allow / wait rounds with empty jobs: no lost wake-up
static void rounds(int n) {
  std::atomic<int> ran{0};
  LookAhead la(2, [&](uint32_t, int) { ran.fetch_add(1, std::memory_order_relaxed); }, no_start);
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n; k++) {
    la.allow(k);
    la.wait(k);
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("rounds n=%d ran=%d ms=%.1f\n", n, ran.load(), ms);
}

// 8. the look-ahead window, every row the test's table has
static void window_rows() {
  const int lasts[5] = {0, 1, 2, 5, 20};
  for (int p = 0; p < 2; p++)
    for (int last : lasts)
      for (int d = 0; d <= 14; d++)
        for (int t = 0; t <= last; t++) {
          const loamx::LookaheadWindow w = loamx::lookahead_window(t, d, last, p != 0);
          printf("window_p%d_l%d_d%d_t%d v=%d,%d,%d,%d,%d,%d,%d\n", p, last, d, t, w.feat_join, w.odom_join, w.feat_reg, w.odom_reg, w.feat_late, w.odom_late,
                 (int)w.late);
        }
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "window") { window_rows(); return 0; }
  for (uint32_t n : {2u, 3u})
    for (int D : {0, 1, 2, 6}) order(n, D);
  park_mid_flight();
  jump();
  failing_step();
  two_failing();
  error_first_wait();
  park_drops_error();
  reset_running();
  destructor();
  rounds(1000);
  return 0;
}
