// mfx_pool.h -- host threads that stay parked between the jobs of their owner (the packers of a streamed run, the readers of the
// ingest): starting 16 threads costs ~0.45 ms, 1.3 % of a 3 Gb run, waking them ~0.05 ms.  Host only.
#pragma once
#include <stdint.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

void mfx_pin_spread(unsigned w);          // pins the calling thread to L3 domain w mod n (all NUMA nodes); mfx_stream.cpp, with the encoder placement

struct WorkerPool {
  unsigned W;
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable wake, idle;
  std::function<void(unsigned)> job;
  uint64_t gen = 0;
  unsigned running = 0;
  bool quit = false;
  // spread: thread i is pinned to L3 domain i mod n of the machine (mfx_pin_spread) -- threads that move memory
  // share their CCD's link to it, and threads started by one parent tend to land next to each other
  explicit WorkerPool(unsigned w, bool spread = false) : W(w) {
    for (unsigned i = 0; i < W; ++i)
      th.emplace_back([this, i, spread]() {
        if (spread) mfx_pin_spread(i);
        uint64_t seen = 0;
        for (;;) {
          std::function<void(unsigned)> f;
          {
            std::unique_lock<std::mutex> lk(m);
            wake.wait(lk, [&] { return quit || gen != seen; });
            if (quit) return;
            seen = gen;
            f = job;
          }
          f(i);
          std::lock_guard<std::mutex> lk(m);
          if (--running == 0) idle.notify_all();
        }
      });
  }
  void start(std::function<void(unsigned)> f) {
    std::lock_guard<std::mutex> lk(m);
    job = std::move(f);
    running = W;
    ++gen;
    wake.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m);
    idle.wait(lk, [&] { return running == 0; });
  }
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(m); quit = true; }
    wake.notify_all();
    for (auto &t : th) t.join();
  }
};
