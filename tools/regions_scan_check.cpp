/* regions_scan_check.cpp -- gs_regions_scan.h as a host program (make -C guidescan-cli_amd/csrc regions-check, under the
 * address and undefined-behaviour sanitizers; no GPU and no library):
 *   1. on random interval sets - short and long intervals, nested to several depths, abutting, sharing starts, touching
 *      base 0 and the last base, and the empty set - the walk of gs_rg_visit finds, for every query position and several
 *      footprint widths, exactly the intervals a loop over all of them finds, each once;
 *   2. the order of (gs_rg_key_high, gs_rg_key_low) is the order of the tuple (group, [specificity descending,]
 *      chromosome, position, sense with '+' first) on random records, ties in specificity included. */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

#include "gs_regions_scan.h"

namespace {

struct table {
  std::vector<uint32_t> start, end, maxend, group;
  gs_rg_table view() const { return gs_rg_table{start.data(), end.data(), maxend.data(), group.data(), (uint32_t)start.size()}; }
};

table make(std::mt19937 &rng, uint32_t len, uint32_t n, uint32_t style) {
  struct iv {
    uint32_t s, e, g;
  };
  std::vector<iv> v;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t s, e;
    if (style == 0) { /* anything */
      s = (uint32_t)rng() % len;
      e = s + 1 + (uint32_t)rng() % (len - s);
    } else if (style == 1) { /* nested around the middle */
      const uint32_t h = 1 + (uint32_t)rng() % (len / 2);
      s = len / 2 - h;
      e = len / 2 + ((uint32_t)rng() % 2 ? h : 1 + (uint32_t)rng() % h);
    } else if (style == 2) { /* abutting tiles of a few widths */
      const uint32_t w = 1 + (uint32_t)rng() % 7;
      s = ((uint32_t)rng() % (len / w)) * w;
      e = std::min(len, s + w);
    } else { /* one long interval first, short ones behind it */
      s = i == 0 ? 0 : 1 + (uint32_t)rng() % (len - 1);
      e = i == 0 ? len : std::min(len, s + 1 + (uint32_t)rng() % 4);
    }
    v.push_back(iv{s, e, (uint32_t)((uint32_t)rng() % 5)});
  }
  std::sort(v.begin(), v.end(), [](const iv &a, const iv &b) { return std::tie(a.s, a.e, a.g) < std::tie(b.s, b.e, b.g); });
  table t;
  for (const iv &x : v) {
    t.start.push_back(x.s);
    t.end.push_back(x.e);
    t.maxend.push_back(t.maxend.empty() ? x.e : std::max(t.maxend.back(), x.e));
    t.group.push_back(x.g);
  }
  return t;
}

int fail(const char *what, uint32_t a, uint32_t b, uint32_t c) {
  fprintf(stderr, "regions-check: %s (%u, %u, %u)\n", what, a, b, c);
  return 1;
}

}  // namespace

int main() {
  std::mt19937 rng(20240607);
  uint64_t queries = 0;
  for (uint32_t round = 0; round < 600; round++) {
    const uint32_t len = 8 + (uint32_t)rng() % 120, n = round % 7 == 0 ? 0 : (uint32_t)rng() % 40, style = round % 4;
    const table t = make(rng, len, n, style);
    const gs_rg_table v = t.view();
    for (uint32_t w : {1u, 2u, 5u, 23u, 27u})
      for (uint32_t q = 0; q < len + 2; q++) {
        std::vector<uint32_t> got, want;
        const uint32_t cnt = gs_rg_visit(v, q, w, [&](uint32_t i) { got.push_back(i); });
        for (uint32_t i = 0; i < v.n; i++)
          if (t.start[i] <= q && (uint64_t)q + w <= t.end[i]) want.push_back(i);
        std::sort(got.begin(), got.end());
        if (cnt != got.size() || got != want || gs_rg_count(v, q, w) != cnt) return fail("membership differs", round, w, q);
        queries++;
      }
    /* the last position of a 32-bit coordinate does not wrap */
    if (gs_rg_count(v, 0xFFFFFFFFu, 27) != 0) return fail("a query at 2^32 - 1 found an interval", round, 0, 0);
  }
  struct rec {
    uint32_t group, chr, pos;
    uint8_t sense;
    float spec;
  };
  static const float specs[] = {0.0f, 1.0f, 0.5f, 0.25f, 1.0f / 3.0f, 0.1f, 1e-6f, 0.999999f};
  for (int ranked = 0; ranked < 2; ranked++) {
    std::vector<rec> r;
    for (int i = 0; i < 4000; i++)
      r.push_back(rec{(uint32_t)((uint32_t)rng() % 6), (uint32_t)((uint32_t)rng() % 4), 1 + (uint32_t)((uint32_t)rng() % 50), (uint8_t)((uint32_t)rng() % 2 ? '+' : '-'),
                      specs[(uint32_t)rng() % 8]});
    r.push_back(rec{0xFFFFFFFFu, 0x7FFFFFFFu, 0xFFFFFFFFu, '-', 0.5f});
    for (size_t i = 0; i + 1 < r.size(); i++) {
      const rec &a = r[i], &b = r[i + 1];
      const auto ka = std::make_pair(gs_rg_key_high(a.group, ranked, a.spec), gs_rg_key_low(a.chr, a.pos, a.sense));
      const auto kb = std::make_pair(gs_rg_key_high(b.group, ranked, b.spec), gs_rg_key_low(b.chr, b.pos, b.sense));
      const auto ta = std::make_tuple(a.group, ranked ? -a.spec : 0.0f, a.chr, a.pos, a.sense == '-');
      const auto tb = std::make_tuple(b.group, ranked ? -b.spec : 0.0f, b.chr, b.pos, b.sense == '-');
      if ((ka < kb) != (ta < tb) || (ka == kb) != (ta == tb)) return fail("key order differs from the tuple order", (uint32_t)i, ranked, 0);
    }
  }
  printf("regions-check: %llu membership queries and 8,002 key pairs agree\n", (unsigned long long)queries);
  return 0;
}
