// Drives loamx::HelperThread (csrc/helper_thread.hpp) on a CPU: one line per scenario, read by tests/test_helper_thread.py.
// Jobs are gated with atomics and promises; no scenario uses a sleep as synchronisation.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <future>
#include <memory>
#include <stdexcept>
#include <string>
#include "helper_thread.hpp"

using loamx::HelperThread;

static void spin_for(const std::atomic<bool>& flag) {
  while (!flag.load(std::memory_order_acquire)) loamx::cpu_relax();
}
// "ok" when f returns, what() of what it throws otherwise
template <class F> static std::string outcome(F&& f) {
  try { f(); } catch (const std::exception& e) { return e.what(); }
  return "ok";
}
static std::function<void()> failing(const char* what) { return [what]() { throw std::runtime_error(what); }; }

// 1. a job that throws: wait() rethrows it once
static void throw_once() {
  HelperThread h;
  h.post(failing("A"));
  const std::string w1 = outcome([&]() { h.wait(); }), w2 = outcome([&]() { h.wait(); });
  printf("throw_once wait1=%s wait2=%s\n", w1.c_str(), w2.c_str());
}

// 2. job A releases its front, then throws in its tail; the caller sees front_done, does not wait() and posts B
static void tail_error() {
  HelperThread h;
  std::atomic<bool> go{false}, b_ran{false}, c_ran{false};
  h.post([&]() {
    HelperThread::Front front(h);
    front.release();
    spin_for(go);
    throw std::runtime_error("A");
  });
  spin_for(h.front_done);
  const bool front_failed = h.front_failed.load();
  go.store(true, std::memory_order_release);
  const std::string pb = outcome([&]() { h.post([&]() { b_ran = true; }); });
  const std::string wb = outcome([&]() { h.wait(); });   // (whatever was accepted has run behind this)
  const bool b = b_ran.load();
  const std::string pc = outcome([&]() { h.post([&]() { c_ran = true; }); });
  const std::string wc = outcome([&]() { h.wait(); });
  printf("tail_error front_failed=%d post_b=%s b_ran=%d wait_b=%s post_c=%s c_ran=%d wait_c=%s\n", (int)front_failed, pb.c_str(), (int)b,
         wb.c_str(), pc.c_str(), (int)c_ran.load(), wc.c_str());
}

// 3. an error is taken exactly once
static void taken_once() {
  HelperThread h;
  h.post(failing("A"));
  const std::string p1 = outcome([&]() { h.post(failing("B")); });
  const std::string p2 = outcome([&]() { h.post(failing("B")); });
  const std::string w1 = outcome([&]() { h.wait(); }), w2 = outcome([&]() { h.wait(); });
  printf("taken_once post1=%s post2=%s wait1=%s wait2=%s\n", p1.c_str(), p2.c_str(), w1.c_str(), w2.c_str());
}

// 4. a front that throws
static void front_throws() {
  HelperThread h;
  std::promise<void> left;   // (fulfilled when the job has unwound past its guard)
  h.post([&]() {
    struct Tell { std::promise<void>& p; ~Tell() { p.set_value(); } } tell{left};
    HelperThread::Front front(h);
    throw std::runtime_error("F");
  });
  left.get_future().wait();
  const bool ff = h.front_failed.load(std::memory_order_acquire), fd = h.front_done.load(std::memory_order_acquire);
  const std::string w = outcome([&]() { h.wait(); });
  printf("front_throws front_failed=%d front_done=%d wait=%s\n", (int)ff, (int)fd, w.c_str());
}

// 5. the destructor joins with a job still running, and with no job ever posted
static void destructor() {
  std::atomic<bool> started{false}, finished{false};
  {
    HelperThread h;
    h.post([&]() {
      started.store(true, std::memory_order_release);
      for (int k = 0; k < 20000; k++) std::this_thread::yield();   // (work, so that the destructor finds the job running)
      finished.store(true, std::memory_order_release);
    });
    spin_for(started);
  }
  const bool done = finished.load();
  { HelperThread idle; }
  { HelperThread failed; failed.post(failing("dropped")); }   // (an error nobody took goes with the object)
  printf("destructor job_finished=%d idle=ok untaken=ok\n", (int)done);
}

// 6. post / wait rounds with an empty job: no lost wake-up
static void rounds(int n) {
  HelperThread h;
  int ran = 0;   // (written by the job, read behind wait(): ordered by the helper's mutex)
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n; k++) {
    h.post([&]() { ran++; });
    h.wait();
  }
  // ... and without the wait: post() itself waits for the job before
  for (int k = 0; k < n; k++) h.post([&]() { ran++; });
  h.wait();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("rounds n=%d ran=%d ms=%.1f\n", n, ran, ms);
}

int main() {
  throw_once();
  tail_error();
  taken_once();
  front_throws();
  destructor();
  rounds(1000);
  return 0;
}
