/* pairs_scan_check.cpp -- gs_pairs_scan.h as a host program (make -C guidescan-cli_amd/csrc pairs-check, under the address
 * and undefined-behaviour sanitizers; no GPU and no library).  On random records - several groups and chromosomes, both
 * senses with and without --start, positions dense enough for equal cuts and, in some rounds, cuts next to 2^32 - under
 * random rules - all three orientations, cut offsets 0 to k, min_span 0, max_span from 0 to 2^63 and beyond:
 *   1. gs_pr_cut is the boundary that leaves cut_offset protospacer bases between cut and PAM, restated from where the
 *      PAM lies in the footprint;
 *   2. the sorted order of (group, gs_pr_key) is the order of the tuple (group, chromosome, cut, sense with '+' first);
 *   3. for every record, the range of gs_pr_range and the count of gs_pr_count hold exactly the partners a loop over all
 *      records finds, and gs_pr_partner names them in order, each once;
 *   4. gs_pr_owner over the offsets inverts the enumeration, records without partners included;
 *   5. the order of (gs_pr_word_min, gs_pr_word_max) is the order of (group, min descending, max descending). */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

#include "gs_pairs_scan.h"

namespace {

struct rec {
  uint32_t group, chr, pos;
  uint8_t sense;
  float spec;
};

int fail(const char *what, uint32_t a, uint32_t b, uint32_t c) {
  fprintf(stderr, "pairs-check: %s (%u, %u, %u)\n", what, a, b, c);
  return 1;
}

/* the cut restated from where the PAM lies in the footprint: cut_offset protospacer bases away from it */
uint64_t cut_by_bases(const rec &r, uint32_t k, uint32_t P, uint32_t C, bool start) {
  const uint64_t q = (uint64_t)r.pos - 1;
  const bool forward = r.sense == '+';
  const bool pam_first = forward == start; /* on the forward strand the PAM comes first: --start and '+', or neither */
  if (pam_first) return q + P + C;         /* PAM [q, q + P), protospacer behind it: C bases in */
  return q + k - C;                        /* protospacer [q, q + k), PAM behind it: C bases back from its end */
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240911);
  static const float specs[] = {0.0f, 1.0f, 0.5f, 0.25f, 1.0f / 3.0f, 0.1f, 1e-6f, 0.999999f};
  static const uint64_t spans[] = {0, 1, 2, 5, 17, 40, 400, 1ull << 31, (1ull << 32) - 1, 1ull << 32, (1ull << 63) - 1, 1ull << 63, ~0ull};
  uint64_t records = 0, pairs = 0;
  for (uint32_t round = 0; round < 400; round++) {
    const uint32_t k = round % 3 == 0 ? 23 : 20, P = round % 3 == 0 ? 4 : 3;
    const bool start = round % 2;
    const uint32_t C = round % 5 == 0 ? 0 : round % 5 == 1 ? k : (uint32_t)(rng() % (k + 1));
    const uint32_t n = round % 11 == 0 ? (uint32_t)(rng() % 2) : 1 + (uint32_t)(rng() % 120);
    const uint32_t base = round % 7 == 3 ? 0xFFFFFFFFu - k - P - 64 : (uint32_t)(rng() % 1000); /* cuts next to 2^32 */
    std::vector<rec> r;
    for (uint32_t i = 0; i < n; i++)
      r.push_back(rec{(uint32_t)(rng() % 3), (uint32_t)(rng() % 2) * 0x7FFFFFFFu, base + 1 + (uint32_t)(rng() % 60), (uint8_t)(rng() % 2 ? '+' : '-'),
                      specs[rng() % 8]});
    /* distinct (group, chromosome, position, sense), as a design's records are */
    std::sort(r.begin(), r.end(), [](const rec &a, const rec &b) {
      return std::tie(a.group, a.chr, a.pos, a.sense) < std::tie(b.group, b.chr, b.pos, b.sense);
    });
    r.erase(std::unique(r.begin(), r.end(),
                        [](const rec &a, const rec &b) { return std::tie(a.group, a.chr, a.pos, a.sense) == std::tie(b.group, b.chr, b.pos, b.sense); }),
            r.end());
    std::shuffle(r.begin(), r.end(), rng);
    const uint32_t E = (uint32_t)r.size();
    std::vector<uint64_t> x(E);
    for (uint32_t i = 0; i < E; i++) {
      x[i] = cut_by_bases(r[i], k, P, C, start);
      if (gs_pr_cut(r[i].pos, r[i].sense, k, P, C, start) != x[i] || x[i] > 0xFFFFFFFFull) return fail("the cut differs", round, i, C);
      if (gs_pr_pam_right(r[i].sense, start) != ((r[i].sense == '+') != start)) return fail("the PAM side differs", round, i, 0);
    }
    /* the order */
    std::vector<uint32_t> order(E);
    for (uint32_t i = 0; i < E; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return std::make_tuple(r[a].group, r[a].chr, x[a], r[a].sense == '-') < std::make_tuple(r[b].group, r[b].chr, x[b], r[b].sense == '-');
    });
    std::vector<uint32_t> group(E), pp(E + 1, 0);
    std::vector<uint64_t> key(E);
    for (uint32_t i = 0; i < E; i++) {
      const rec &a = r[order[i]];
      group[i] = a.group;
      key[i] = gs_pr_key(a.chr, (uint32_t)x[order[i]], a.sense);
      if (gs_pr_key_cut(key[i]) != x[order[i]] || gs_pr_key_chr(key[i]) != a.chr) return fail("the key does not give its parts back", round, i, 0);
      pp[i + 1] = pp[i] + (gs_pr_pam_right(a.sense, start) ? 1u : 0u);
      if (i && !(std::make_pair(group[i - 1], key[i - 1]) < std::make_pair(group[i], key[i]))) return fail("the key order differs from the tuple order", round, i, 0);
    }
    records += E;
    for (int rule = 0; rule < 12; rule++) {
      const uint64_t s1 = spans[rng() % 13], s2 = spans[rng() % 13];
      const uint64_t min_span = rule == 0 ? 0 : std::min(s1, s2), max_span = rule == 0 ? 0 : std::max(s1, s2);
      const uint32_t orientation = (uint32_t)rule % 3;
      std::vector<uint64_t> off(E + 1, 0);
      std::vector<std::pair<uint32_t, uint32_t>> want, got;
      for (uint32_t a = 0; a < E; a++) {
        for (uint32_t b = a + 1; b < E; b++) { /* a before b in the order */
          if (group[a] != group[b] || r[order[a]].chr != r[order[b]].chr) continue;
          const uint64_t span = x[order[b]] - x[order[a]];
          if (span < min_span || span > max_span) continue;
          const bool ra = gs_pr_pam_right(r[order[a]].sense, start), rb = gs_pr_pam_right(r[order[b]].sense, start);
          if (orientation == GS_PR_PAM_OUT && !(!ra && rb)) continue;
          if (orientation == GS_PR_PAM_IN && !(ra && !rb)) continue;
          want.emplace_back(a, b);
        }
        uint32_t lo = 0, hi = 0;
        gs_pr_range(group.data(), key.data(), E, a, min_span, max_span, &lo, &hi);
        if (lo < a + 1 || hi < lo || hi > E) return fail("a range outside the records behind a", round, a, (uint32_t)rule);
        const uint32_t cnt = gs_pr_count(orientation, pp[a + 1] != pp[a], pp.data(), lo, hi);
        off[a + 1] = off[a] + cnt;
        uint32_t before = a;
        for (uint32_t q = 0; q < cnt; q++) {
          const uint32_t b = gs_pr_partner(orientation, pp.data(), lo, hi, q);
          if (b < lo || b >= hi || b <= before) return fail("a partner outside its range or out of order", round, a, q);
          before = b;
          got.emplace_back(a, b);
        }
      }
      if (got != want) return fail("the pairs differ from the double loop", round, (uint32_t)rule, (uint32_t)want.size());
      for (uint64_t t = 0; t < off[E]; t++)
        if (gs_pr_owner(off.data(), E, t) != got[t].first) return fail("the owner of a pair differs", round, (uint32_t)rule, (uint32_t)t);
      pairs += want.size();
    }
    /* a min_span above max_span has no pair */
    for (uint32_t a = 0; a < E; a++) {
      uint32_t lo = 0, hi = 0;
      gs_pr_range(group.data(), key.data(), E, a, 5, 4, &lo, &hi);
      if (lo != hi) return fail("min_span > max_span found a partner", round, a, 0);
    }
  }
  /* the rank words */
  std::vector<std::tuple<uint32_t, float, float>> w;
  for (int i = 0; i < 4000; i++) w.emplace_back((uint32_t)(rng() % 6), specs[rng() % 8], specs[rng() % 8]);
  w.emplace_back(0xFFFFFFFFu, 0.0f, 0.0f);
  for (size_t i = 0; i + 1 < w.size(); i++) {
    const auto &[ga, a1, a2] = w[i];
    const auto &[gb, b1, b2] = w[i + 1];
    const auto ka = std::make_pair(gs_pr_word_min(ga, a1, a2), gs_pr_word_max(a1, a2));
    const auto kb = std::make_pair(gs_pr_word_min(gb, b1, b2), gs_pr_word_max(b1, b2));
    const auto ta = std::make_tuple(ga, -std::min(a1, a2), -std::max(a1, a2));
    const auto tb = std::make_tuple(gb, -std::min(b1, b2), -std::max(b1, b2));
    if ((ka < kb) != (ta < tb) || (ka == kb) != (ta == tb)) return fail("the rank words' order differs from the tuple order", (uint32_t)i, 0, 0);
    if (ka != std::make_pair(gs_pr_word_min(ga, a2, a1), gs_pr_word_max(a2, a1))) return fail("the rank words depend on the order of a and b", (uint32_t)i, 0, 0);
  }
  printf("pairs-check: %llu records, %llu pairs under 4,800 rules and 4,000 rank word pairs agree\n", (unsigned long long)records,
         (unsigned long long)pairs);
  return 0;
}
