/*
 * batch_pipeline.hpp -- the ordered three-stage pipeline under `guidescan enumerate`: workers search batches, one thread
 * per batch formats it, the calling thread writes the batches in index order.  It knows batch indexes and three
 * callables, nothing of guides, of the library or of the GPU, so it is checked on the CPU under the thread and address
 * sanitizers (tools/batch_pipeline_check.cpp, make pipeline-check).
 *
 * The contract (workers >= 1, max_in_flight >= 1):
 *   - Workers take batch indexes in order from one counter, and take one only while fewer than max_in_flight batches
 *     are handed out but not yet released.
 *   - When search(batch, worker) returns, a formatter thread for that batch starts and the worker goes on to the next
 *     batch.  format(batch) runs only if search gave no error (an empty string).
 *   - The calling thread is the only writer.  It takes the batches in index order, waits for each to be ready, calls
 *     write(batch) and releases the batch.
 *   - After the first failed batch (search or format) nothing more is written and no more batches are handed out; its
 *     error is the one returned.  Batches already handed out are finished and released, a batch that no worker took is
 *     never waited for.
 *   - write(batch) -> false is a short write: it is noted in result::write_ok and the run goes on, the caller reports
 *     it once at the end.
 *   - Every thread is joined before run() returns.
 */
#ifndef GS_BATCH_PIPELINE_HPP
#define GS_BATCH_PIPELINE_HPP

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace batch_pipeline {

struct result {
  std::string error;    /* of the first failed batch, or empty */
  bool write_ok = true; /* no write(batch) said false */
  double s_search = 0, s_format = 0, s_write = 0; /* seconds spent per stage, summed over its threads (stages overlap) */
};

template <class Search, class Format, class Write>
result run(size_t n_batches, unsigned workers, size_t max_in_flight, Search search, Format format, Write write) {
  struct slot {
    std::string error;
    std::thread formatter;
    bool handed = false; /* a worker took it */
    bool ready = false;  /* searched and formatted, or failed */
  };
  using clock = std::chrono::steady_clock;
  auto since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
  std::vector<slot> slots(n_batches);
  std::mutex mtx; /* guards everything below, the slots' flags and threads, and out's seconds */
  std::condition_variable cv;
  size_t next_batch = 0; /* the work queue */
  size_t in_flight = 0;  /* handed out, not yet released: bounds the memory held by results and text */
  result out;
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < workers; w++)
    pool.emplace_back([&, w]() {
      for (;;) {
        size_t bi;
        {
          std::unique_lock<std::mutex> lk(mtx);
          cv.wait(lk, [&] { return in_flight < max_in_flight || next_batch >= n_batches; });
          if (next_batch >= n_batches) return;
          bi = next_batch++;
          slots[bi].handed = true;
          in_flight++;
        }
        slot *s = &slots[bi];
        const auto ts = clock::now();
        s->error = search(bi, w);
        /* the thread object is stored under the mutex the formatter takes before it sets `ready`: the writer joins it
         * only after it has seen `ready`, i.e. after this assignment is complete */
        std::lock_guard<std::mutex> lk(mtx);
        out.s_search += since(ts);
        s->formatter = std::thread([&, s, bi]() {
          const auto tf = clock::now();
          if (s->error.empty()) s->error = format(bi);
          std::lock_guard<std::mutex> lk2(mtx);
          out.s_format += since(tf);
          s->ready = true;
          cv.notify_all();
        });
      }
    });

  for (size_t bi = 0; bi < n_batches; bi++) {
    slot &s = slots[bi];
    {
      /* after a failure next_batch stands at the end: a batch that no worker took will never become ready, and neither
       * will any behind it */
      std::unique_lock<std::mutex> lk(mtx);
      cv.wait(lk, [&] { return s.ready || (!s.handed && next_batch >= n_batches); });
      if (!s.ready) break;
    }
    s.formatter.join();
    const bool failed = !out.error.empty() || !s.error.empty();
    if (out.error.empty()) out.error = s.error;
    double tw = 0;
    if (!failed) { /* after a failed batch nothing more is written: rows behind a hole are not a database */
      const auto t0 = clock::now();
      if (!write(bi)) out.write_ok = false;
      tw = since(t0);
    }
    std::lock_guard<std::mutex> lk(mtx);
    out.s_write += tw;
    in_flight--;
    if (failed) next_batch = n_batches; /* stop handing out work */
    cv.notify_all();
  }
  for (auto &th : pool) th.join();
  return out;
}

}  // namespace batch_pipeline

#endif
