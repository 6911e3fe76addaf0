// The look-ahead gate of the batched pipeline: which odometry chain may run which step, and how the calling thread waits for, parks and
// restarts the chains' worker threads.  Standard library only — no HIP in here: tests/test_odom_lookahead.py drives it on a CPU.
//
// Every chain has a worker thread and a position: `next`, the step it runs next, and `done`, the last step it has published (-1: none).
// One thread, "the caller", uses everything below except the worker rule; done_min() / done_max() / limit() may be read by any thread.
//
// The contract:
//   worker rule    a chain runs step `next` when next <= limit.  When run(chain, k) returns it publishes done = k, next = k + 1.  When it
//                  throws, the worker keeps the error if none is kept yet (the FIRST error stays), sets the limit to -1 so that every
//                  chain stops behind the step it is in, and leaves its positions alone: the step is run again when it is allowed again.
//                  `busy` and the limit change under the mutex only, so whoever holds the mutex sees them together.
//   allow(k)       raises the limit to k, never lowers it; starts the workers on first use; notifies.
//   wait(t)        returns when every chain has published step t.  If the chains have stopped short of t (none busy, limit below t) it
//                  rethrows and clears a kept error, else throws std::logic_error ("internal: an odometry chain stopped before the
//                  requested step").  A kept error is also rethrown when t itself was published: it comes out of the first wait()
//                  that ends behind it, once.
//   drain()        waits for the step the limit names, if the workers have ever been started; returns done_min().
//   park(restart)  limit to -1, waits until no worker is busy, and only then reads the positions, under the mutex (a position read before
//                  the wait is stale by the step a worker was inside).  restart >= 0: a chain that has neither finished that step nor
//                  stands at it continues there (next = restart, done = restart - 1); restart < 0: every chain continues where it is.
//                  A kept error is DROPPED: whoever parks starts the chains over from a state of their own choosing.
//   reset()        park, then every chain back to step 0 (done = -1).  Drops a kept error as well.
//   jumped(t)      true when, for some chain, t is neither a finished step nor its next one (t > done and t != next).
//   ran_inline(chain, t)   the caller ran the step itself while the workers are parked: next = t + 1, done = t.
//   The destructor sets quit, notifies and joins: it ends whether a worker is spinning, blocked, inside a job (it waits for the job) or
//   was never started; an error nobody took is dropped there.
//
// Hand-overs happen every ~0.4 ms in the pipeline, so both sides spin briefly before they fall back to the condition variable (a sleeping
// thread costs tens of microseconds to wake, on the critical path of every step): a worker for `worker_spin`, wait() for 2 ms.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include "host_wait.hpp"

namespace loamx {

// How far step t of Pipeline::step() launches features (feat_*) and allows odometry (odom_*; -1: it allows nothing) at its three points
// of release: before it waits for its own odometry (join: only reached when that is not published yet), before the registration is
// enqueued (reg), and in the late release behind the registration's first launches (late: exists when `late` is set).  `depth` steps of
// odometry look-ahead go with max(depth, 2) of features; everything is capped at the last staged step.  Without prefetch a step
// launches its own features and nothing else.
struct LookaheadWindow {
  int feat_join = -1, odom_join = -1;
  int feat_reg = -1, odom_reg = -1;
  int feat_late = -1, odom_late = -1;
  bool late = false;
};
inline LookaheadWindow lookahead_window(int t, int depth, int last_staged, bool prefetch) {
  LookaheadWindow w;
  auto cap = [&](int k) { return std::min(k, last_staged); };
  if (!prefetch) { w.feat_join = cap(t); return w; }
  const int fd = std::max(depth, 2);
  w.feat_join = w.odom_join = cap(t + 1);
  w.feat_reg = cap(t + fd - 1);
  w.odom_reg = cap(t + std::min(depth, fd - 1));
  w.late = t + 2 <= last_staged;
  if (w.late) { w.feat_late = cap(t + fd); if (depth >= 2) w.odom_late = cap(t + depth); }
  return w;
}

class LookAhead {
 public:
  using Run = std::function<void(uint32_t chain, int step)>;
  // thread_start runs first on every worker thread; worker_spin: how long an idle worker polls before it sleeps
  LookAhead(uint32_t n_chains, Run run, std::function<void()> thread_start,
            std::chrono::steady_clock::duration worker_spin = std::chrono::microseconds(400))
      : n_(n_chains), ch_(new Chain[n_chains]), run_(std::move(run)), thread_start_(std::move(thread_start)), worker_spin_(worker_spin) {}
  LookAhead(const LookAhead&) = delete;
  LookAhead& operator=(const LookAhead&) = delete;
  ~LookAhead() {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; limit_.store(-1, std::memory_order_release); }
    cv_.notify_all();   // (a worker leaves its spin phase after worker_spin and then sees quit)
    for (uint32_t g = 0; g < n_; g++) if (ch_[g].worker.joinable()) ch_[g].worker.join();
  }

  uint32_t n_chains() const { return n_; }
  int done(uint32_t g) const { return ch_[g].done.load(std::memory_order_acquire); }
  int done_min() const { int m = INT_MAX; for (uint32_t g = 0; g < n_; g++) m = std::min(m, done(g)); return m; }
  int done_max() const { int m = -1; for (uint32_t g = 0; g < n_; g++) m = std::max(m, done(g)); return m; }
  int limit() const { return limit_.load(std::memory_order_acquire); }
  bool jumped(int t) const {
    for (uint32_t g = 0; g < n_; g++) if (t > done(g) && t != ch_[g].next.load(std::memory_order_acquire)) return true;
    return false;
  }

  void allow(int k) {
    if (k <= limit()) return;
    if (!started_) {
      started_ = true;
      for (uint32_t g = 0; g < n_; g++) ch_[g].worker = std::thread([this, g] { work(g); });
    }
    { std::lock_guard<std::mutex> lk(mu_); limit_.store(k, std::memory_order_release); }
    cv_.notify_all();
  }
  void wait(int t) {
    auto ready = [&] { return done_min() >= t || (!any_busy() && limit() < t); };
    if (!spin_until(ready, std::chrono::milliseconds(2))) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, ready);
    }
    std::lock_guard<std::mutex> lk(mu_);
    if (err_) { std::exception_ptr e = err_; err_ = nullptr; std::rethrow_exception(e); }
    if (done_min() < t) throw std::logic_error("internal: an odometry chain stopped before the requested step");
  }
  int drain() {
    const int lim = limit();
    if (lim >= 0 && started_) wait(lim);
    return done_min();
  }
  void park(int restart) {
    std::unique_lock<std::mutex> lk(mu_);
    limit_.store(-1, std::memory_order_release);
    cv_.wait(lk, [&] { return !any_busy(); });
    if (restart >= 0)
      for (uint32_t g = 0; g < n_; g++)
        if (restart > ch_[g].done.load() && restart != ch_[g].next.load()) set_position(g, restart);
    err_ = nullptr;
  }
  void reset() {
    std::unique_lock<std::mutex> lk(mu_);
    limit_.store(-1, std::memory_order_release);
    cv_.wait(lk, [&] { return !any_busy(); });
    for (uint32_t g = 0; g < n_; g++) set_position(g, 0);
    err_ = nullptr;
  }
  void ran_inline(uint32_t g, int t) { set_position(g, t + 1); }

 private:
  struct Chain {
    std::atomic<int> done{-1};   // steps <= done are complete and published
    std::atomic<int> next{0};    // the next step of this chain (written by its worker; by the caller only while the workers are parked)
    std::atomic<bool> busy{false};
    std::thread worker;
  };
  const uint32_t n_;
  std::unique_ptr<Chain[]> ch_;
  Run run_;
  std::function<void()> thread_start_;
  const std::chrono::steady_clock::duration worker_spin_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<int> limit_{-1};   // the chains may run steps <= limit (raised by the caller only)
  bool quit_ = false, started_ = false;
  std::exception_ptr err_;       // the first error nobody has taken

  bool any_busy() const { for (uint32_t g = 0; g < n_; g++) if (ch_[g].busy.load(std::memory_order_acquire)) return true; return false; }
  void set_position(uint32_t g, int next) {
    ch_[g].next.store(next, std::memory_order_release);
    ch_[g].done.store(next - 1, std::memory_order_release);
  }
  void work(uint32_t g) {
    Chain& c = ch_[g];
    thread_start_();
    for (;;) {
      auto ready = [&] { return c.next.load(std::memory_order_acquire) <= limit(); };
      if (!spin_until(ready, worker_spin_)) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return ready() || quit_; });
        if (quit_) return;
      }
      {
        std::lock_guard<std::mutex> lk(mu_);   // (busy and the limit change under the mutex: park() relies on seeing them together)
        if (quit_) return;
        if (!ready()) continue;
        c.busy.store(true, std::memory_order_release);
      }
      std::exception_ptr err;
      const int k = c.next.load(std::memory_order_acquire);
      try { run_(g, k); } catch (...) { err = std::current_exception(); }
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (err) { if (!err_) err_ = err; limit_.store(-1, std::memory_order_release); }   // every chain stops; the caller's wait() rethrows
        else { c.next.store(k + 1, std::memory_order_release); c.done.store(k, std::memory_order_release); }
        c.busy.store(false, std::memory_order_release);
      }
      cv_.notify_all();
    }
  }
};

}  // namespace loamx
