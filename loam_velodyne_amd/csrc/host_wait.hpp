// Polling waits of the host (standard library only: no HIP in here).
#pragma once
#include <chrono>
#include <thread>

namespace loamx {

// one turn of a polling loop: tell the core that this is a spin-wait
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  std::this_thread::yield();
#endif
}

// Polls pred() until it holds (returns true) or `budget` has passed (returns false: the caller falls back to a blocking wait).  The clock
// is looked at on every `every`-th spin only (a power of two); what pred() throws passes through.
template <class Pred> bool spin_until(Pred&& pred, std::chrono::steady_clock::duration budget, unsigned every = 256) {
  const auto t_in = std::chrono::steady_clock::now();
  for (unsigned spins = 0; !pred();) {
    if ((++spins & (every - 1u)) == 0u && std::chrono::steady_clock::now() - t_in > budget) return false;
    cpu_relax();
  }
  return true;
}

}  // namespace loamx
