/* annot_check.cpp -- gs_annot_scan.h as a host program under the address and undefined-behaviour sanitizers
 * (make -C guidescan-cli_amd/csrc annot-check): the segment table's construction and the lookup, at every footprint of
 * small chromosomes, against a quadratic restatement - every row against every interval - that builds no table. */
#include "gs_annot_scan.h"

#include <cstdio>
#include <cstdlib>
#include <set>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fputc('\n', stderr);               \
      if (++failures > 20) exit(1);      \
    }                                    \
  } while (0)

/* every s in [0, len - w + 1] (the rows resolve_absolute lets through) and a few beyond on both sides */
static void check_case(const char *what, const std::vector<std::vector<gs_an_iv>> &per_chr, const std::vector<uint32_t> &len, uint32_t w) {
  gs_an_host h;
  uint64_t need = 0;
  CHECK(gs_an_build(per_chr, GS_AN_MAX_ENTRIES, h, &need), "%s: build refused", what);
  CHECK(need == h.ent.size(), "%s: need %llu, entries %zu", what, (unsigned long long)need, h.ent.size());
  const gs_an_table t = h.table();
  uint64_t segs = 0;
  for (size_t c = 0; c < per_chr.size(); c++) {
    const uint32_t b = h.chr_bp[c], e = h.chr_bp[c + 1];
    if (e - b > 1) segs += e - b - 1;
    for (uint32_t i = b; i + 1 < e; i++) CHECK(h.bp[i] < h.bp[i + 1], "%s: breakpoints of chromosome %zu do not ascend", what, c);
    if (e > b) CHECK(h.seg_off[e - 1] == h.seg_off[e], "%s: the last breakpoint of chromosome %zu opens a list", what, c);
    for (uint32_t i = b; i < e; i++)
      for (uint32_t x = h.seg_off[i]; x + 1 < h.seg_off[i + 1]; x++) CHECK(h.ent[x] < h.ent[x + 1], "%s: a segment's groups do not ascend", what);
  }
  CHECK(segs == h.n_segments, "%s: n_segments", what);
  for (size_t c = 0; c < per_chr.size(); c++) {
    for (long long s = -3; s <= (long long)len[c] + 3; s++) {
      /* the restatement: clip, then every interval */
      long long lo = s - 1, hi = s - 1 + (long long)w;
      if (lo < 0) lo = 0;
      if (hi > (long long)len[c]) hi = len[c];
      std::set<uint32_t> want;
      if (lo < hi)
        for (const gs_an_iv &x : per_chr[c])
          if ((long long)x.start < hi && (long long)x.end > lo) want.insert(x.group);
      std::vector<uint32_t> got;
      const uint32_t n = gs_an_visit(t, (uint32_t)c, s, w, len[c], [&](uint32_t g) { got.push_back(g); });
      CHECK(n == got.size() && n == gs_an_count(t, (uint32_t)c, s, w, len[c]), "%s: chromosome %zu s %lld: counts differ", what, c, s);
      CHECK(got == std::vector<uint32_t>(want.begin(), want.end()), "%s: chromosome %zu s %lld: %zu features, %zu expected", what, c, s,
            got.size(), want.size());
    }
  }
  /* a chromosome the table does not have */
  CHECK(gs_an_count(t, (uint32_t)per_chr.size(), 5, w, 100) == 0, "%s: a chromosome beyond the table", what);
}

int main() {
  /* one base at either end of the footprint, and abutting it: w = 5, footprint of s = 11 is [10, 15) */
  check_case("touch", {{{0, 5, 11}, {1, 14, 20}, {2, 5, 10}, {3, 15, 20}}}, {40}, 5);
  {
    gs_an_host h;
    gs_an_build({{{0, 5, 11}, {1, 14, 20}, {2, 5, 10}, {3, 15, 20}}}, GS_AN_MAX_ENTRIES, h, nullptr);
    std::vector<uint32_t> got;
    gs_an_visit(h.table(), 0, 11, 5, 40, [&](uint32_t g) { got.push_back(g); });
    CHECK((got == std::vector<uint32_t>{0, 1}), "touch: the footprint [10, 15) has the groups that touch it by one base only");
  }
  /* a gene over five exons, the gene's group also the exons' parent: once, not twice */
  check_case("gene", {{{0, 100, 400}, {1, 100, 130}, {2, 160, 190}, {3, 220, 250}, {4, 280, 310}, {5, 370, 400}, {0, 120, 125}}}, {500}, 23);
  /* one group in pieces nearer than a footprint: it is in two segments that are not neighbours */
  check_case("pieces", {{{0, 10, 12}, {1, 13, 14}, {0, 15, 18}, {2, 11, 16}}}, {60}, 9);
  /* 70 and 300 groups over one base; an empty chromosome; a group on two chromosomes */
  for (uint32_t depth : {70u, 300u}) {
    std::vector<gs_an_iv> v;
    for (uint32_t g = 0; g < depth; g++) v.push_back({g, 50 - (g % 7), 51 + (g % 5)});
    check_case("stacked", {v, {}, {{3, 0, 9}, {depth, 4, 30}}}, {120, 77, 30}, 23);
  }
  /* s == 0 and the chromosome's ends */
  check_case("ends", {{{0, 0, 1}, {1, 29, 30}}}, {30}, 4);
  /* random sets: short intervals under long ones, few groups so that groups repeat, overlap and abut */
  for (int round = 0; round < 300; round++) {
    const uint32_t n_chr = 1 + rnd(3), w = 1 + rnd(30);
    std::vector<std::vector<gs_an_iv>> per_chr(n_chr);
    std::vector<uint32_t> len(n_chr);
    const uint32_t n_groups = 1 + rnd(12);
    for (uint32_t c = 0; c < n_chr; c++) {
      len[c] = 1 + rnd(200);
      const uint32_t n_iv = rnd(25);
      for (uint32_t i = 0; i < n_iv; i++) {
        const uint32_t a = rnd(len[c]), span = rnd(4) ? 1 + rnd(12) : 1 + rnd(len[c]);
        per_chr[c].push_back({rnd(n_groups), a, std::min(len[c], a + span)});
      }
    }
    check_case("random", per_chr, len, w);
  }
  /* the cap is checked before the entries are allocated */
  {
    std::vector<gs_an_iv> v;
    for (uint32_t g = 0; g < 100; g++) v.push_back({g, 0, 1000});
    gs_an_host h;
    uint64_t need = 0;
    CHECK(!gs_an_build({v}, 99, h, &need) && need == 100 && h.ent.empty(), "cap: 100 entries under a cap of 99");
    CHECK(gs_an_build({v}, 100, h, &need) && h.ent.size() == 100, "cap: 100 entries under a cap of 100");
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("annot_check ok\n");
  return 0;
}
