/* batch_pipeline_check.cpp -- the ordered pipeline of `guidescan enumerate` (csrc/host/batch_pipeline.hpp) as a
 * stand-alone host program with stand-in stages, meant to be built with -fsanitize=thread and with
 * -fsanitize=address,undefined (make -C guidescan-cli_amd/csrc pipeline-check).  The stand-ins sleep for pseudo-random
 * microseconds from a fixed seed and count what the header's contract promises: order, exactly-once, the bound on the
 * batches held, and what happens around a failed batch.  Exit status 0: every check held. */
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "batch_pipeline.hpp"

static int fails = 0;
#define CHECK(c)                                                                                      \
  do {                                                                                                \
    if (!(c)) {                                                                                       \
      fprintf(stderr, "line %d (%s): %s\n", __LINE__, where.c_str(), #c);                             \
      fails++;                                                                                        \
    }                                                                                                 \
  } while (0)

/* 0..299 microseconds, a function of (seed, batch, stage) alone */
static void nap(uint32_t seed, size_t batch, unsigned stage) {
  uint64_t x = 0x9E3779B97F4A7C15ull * (seed + 1) + batch * 3 + stage;
  x ^= x >> 31;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 29;
  std::this_thread::sleep_for(std::chrono::microseconds(x % 300));
}

enum fail_stage { NONE, SEARCH, FORMAT };

static void one_run(size_t n, unsigned workers, size_t max_in_flight, fail_stage fs, size_t fail_at) {
  const std::string where = "batches " + std::to_string(n) + " workers " + std::to_string(workers) + " max_in_flight " +
                            std::to_string(max_in_flight) +
                            (fs == NONE ? "" : (fs == SEARCH ? " search fails at " : " format fails at ") + std::to_string(fail_at));
  const uint32_t seed = (uint32_t)(n * 131 + workers * 17 + max_in_flight * 5 + fs * 3 + fail_at);
  std::vector<std::atomic<int>> searched(n), formatted(n), written(n);
  for (size_t i = 0; i < n; i++) searched[i] = formatted[i] = written[i] = 0;
  std::atomic<long> held{0}, peak{0}; /* between the start of a batch's search and the end of its write */
  std::atomic<int> bad_worker{0}, format_before_search{0};
  std::vector<size_t> order; /* the writer's alone */
  const std::thread::id caller = std::this_thread::get_id();
  bool writer_is_caller = true;

  const batch_pipeline::result r = batch_pipeline::run(
      n, workers, max_in_flight,
      [&](size_t b, unsigned w) -> std::string {
        const long h = ++held;
        long p = peak.load();
        while (h > p && !peak.compare_exchange_weak(p, h)) {
        }
        if (w >= workers) bad_worker++;
        nap(seed, b, 0);
        searched[b]++;
        return fs == SEARCH && b == fail_at ? "search " + std::to_string(b) + " failed" : "";
      },
      [&](size_t b) -> std::string {
        if (searched[b] != 1) format_before_search++;
        nap(seed, b, 1);
        formatted[b]++;
        return fs == FORMAT && b == fail_at ? "format " + std::to_string(b) + " failed" : "";
      },
      [&](size_t b) -> bool {
        if (std::this_thread::get_id() != caller) writer_is_caller = false;
        nap(seed, b, 2);
        order.push_back(b);
        written[b]++;
        --held;
        return true;
      });

  CHECK(bad_worker == 0 && format_before_search == 0 && writer_is_caller && r.write_ok);
  CHECK(r.s_search >= 0 && r.s_format >= 0 && r.s_write >= 0);
  const size_t n_written = fs == NONE ? n : fail_at;
  CHECK(order.size() == n_written);
  for (size_t i = 0; i < order.size(); i++) CHECK(order[i] == i); /* in order, which also says: none twice */
  for (size_t i = 0; i < n; i++) CHECK(written[i] == (i < n_written ? 1 : 0));
  if (fs == NONE) {
    CHECK(r.error.empty());
    for (size_t i = 0; i < n; i++) CHECK(searched[i] == 1 && formatted[i] == 1);
    CHECK(peak <= (long)max_in_flight);
    CHECK(held == 0);
    return;
  }
  CHECK(r.error == std::string(fs == SEARCH ? "search " : "format ") + std::to_string(fail_at) + " failed");
  /* When the writer sees the failure at batch f, the batches f .. next-1 are handed out and none of them is released
   * (the writer has not passed them), so next - f <= max_in_flight; from then on nothing is handed out.  So what was
   * searched is a prefix of the batches that ends before f + max_in_flight, each of it once, and every batch that was
   * searched without an error was formatted: handed-out batches are finished. */
  size_t n_searched = 0;
  while (n_searched < n && searched[n_searched] == 1) n_searched++;
  for (size_t i = n_searched; i < n; i++) CHECK(searched[i] == 0);
  CHECK(n_searched > fail_at && n_searched <= fail_at + max_in_flight);
  for (size_t i = 0; i < n; i++) CHECK(formatted[i] == (i < n_searched && !(fs == SEARCH && i == fail_at) ? 1 : 0));
}

int main() {
  int runs = 0;
  for (size_t n : {0, 1, 2, 37})
    for (unsigned workers : {1u, 3u})
      for (size_t mif : {1, 2, 9}) {
        one_run(n, workers, mif, NONE, 0);
        runs++;
        if (!n) continue;
        for (fail_stage fs : {SEARCH, FORMAT})
          for (size_t at : std::set<size_t>{0, n / 2, n - 1}) { /* the first, a middle and the last batch */
            one_run(n, workers, mif, fs, at);
            runs++;
          }
      }
  printf("batch_pipeline_check: %d runs, %d failed check(s)\n", runs, fails);
  return fails ? 1 : 0;
}
