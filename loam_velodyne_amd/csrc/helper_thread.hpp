// A helper thread that runs one posted job at a time (the mapper's: it enqueues a sweep's map update while the caller fetches the sweep's
// results).  Standard library only — no HIP in here: tests/test_helper_thread.py drives it on a CPU.
//
// The contract:
//   post(f)   waits until the previous job has ended, then hands f over.  If an earlier job left an error that nobody has taken, post
//             rethrows it (and clears it) and does NOT accept f: the next post is accepted again.
//   the worker keeps the FIRST untaken error; a later job that ends normally does not clear it.
//   wait()    returns when the posted job has run; rethrows and clears a kept error.
//   An error is therefore reported exactly once, by the first post() or wait() behind the job that threw.
//   A job has a front part, which the next post's caller must see ended before it touches what the job works on, and a tail that may
//   still run then.  front_done: the job has left its front part behind (also by an exception, and at the latest when it ends);
//   front_failed: ... by an exception (wait() rethrows it); running: a job has been posted and has not ended.  The job marks the end of
//   its front part with a Front guard.
//   The destructor waits for a running job and joins; an error nobody took is dropped there.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include "host_wait.hpp"

namespace loamx {

struct HelperThread {
  std::mutex mu;                 // (public with cv: the owner may guard words it shares with its jobs with them)
  std::condition_variable cv;
  std::atomic<bool> running{false};
  std::atomic<bool> front_done{true};
  std::atomic<bool> front_failed{false};

  // "the front part has ended", also when it throws: the caller's next wait must end — it goes on to wait(), which rethrows
  struct Front {
    HelperThread& h;
    bool open = true;
    explicit Front(HelperThread& h_) : h(h_) {}
    Front(const Front&) = delete;
    Front& operator=(const Front&) = delete;
    void release() {
      if (!open) return;
      open = false;
      if (std::uncaught_exceptions() > 0) h.front_failed.store(true, std::memory_order_release);
      h.front_done.store(true, std::memory_order_release);
    }
    ~Front() { release(); }
  };

  void post(std::function<void()> f) {
    std::unique_lock<std::mutex> lk(mu);
    if (!th.joinable()) th = std::thread([this]() { work(); });
    cv.wait(lk, [this]() { return !busy; });
    take_error();
    job = std::move(f);
    busy = true;
    front_failed.store(false, std::memory_order_release);
    front_done.store(false, std::memory_order_release);
    running.store(true, std::memory_order_release);
    posted.fetch_add(1, std::memory_order_release);
    cv.notify_all();
  }
  void wait() {
    // (the job is a few hundred microseconds of enqueueing as a rule: spin for it before sleeping on the condition variable)
    spin_until([this]() { return !running.load(std::memory_order_acquire); }, std::chrono::milliseconds(2));
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this]() { return !busy; });
    take_error();
  }
  ~HelperThread() {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [this]() { return !busy; });
      quit = true;
      posted.fetch_add(1, std::memory_order_release);
      cv.notify_all();
    }
    if (th.joinable()) th.join();
  }

 private:
  std::thread th;
  std::function<void()> job;
  bool busy = false, quit = false;
  std::atomic<uint32_t> posted{0};   // bumped by post(): the worker spins on it for a while before it sleeps on cv
  std::exception_ptr err;            // the first error nobody has taken
  void take_error() {                // (mu held)
    if (!err) return;
    std::exception_ptr e = err;
    err = nullptr;
    std::rethrow_exception(e);
  }
  void work() {
    std::unique_lock<std::mutex> l(mu);
    for (;;) {
      // a job arrives every ~0.7 ms while sweeps flow: waking from a condition variable costs tens of microseconds as a rule and ~10 ms
      // when the thread has lost its time slice (measured: one such call per ~100 sweeps on some hosts, profiles/r06_ab.md section 8),
      // so the worker spins for up to 2 ms on the post counter before it goes to sleep — an idle handle costs nothing after that
      if (!(quit || (busy && job))) {
        const uint32_t seen = posted.load(std::memory_order_acquire);
        l.unlock();
        spin_until([&]() { return posted.load(std::memory_order_acquire) != seen; }, std::chrono::milliseconds(2));
        l.lock();
      }
      cv.wait(l, [this]() { return quit || (busy && job); });
      if (quit) return;
      std::function<void()> j = std::move(job);
      job = nullptr;
      l.unlock();
      std::exception_ptr e;
      try { j(); } catch (...) { e = std::current_exception(); }
      j = nullptr;   // (what the job captured goes before the job counts as ended)
      l.lock();
      if (e && !err) err = e;
      busy = false;
      front_done.store(true, std::memory_order_release);
      running.store(false, std::memory_order_release);
      cv.notify_all();
    }
  }
};

}  // namespace loamx
