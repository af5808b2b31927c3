/* decode_annot_check.cpp -- the footprint of a decoded off-target (gs_an_decoded_footprint, gs_annot_scan.h) and the lookup
 * behind it as a host program under the address and undefined-behaviour sanitizers
 * (make -C guidescan-cli_amd/csrc decode-annot-check): for every coordinate x < LN, both strands, every stored length
 * n <= 24 and every chromosome length LN <= 40, over a handful of small interval sets, against a quadratic restatement -
 * the interval spelled out from the slices scripts/decode_database.py takes, clipped, then every interval - that builds no
 * table and shares no arithmetic with the header. */
#include "gs_annot_scan.h"

#include <cstdio>
#include <cstdlib>
#include <set>

static int failures = 0;
static unsigned long long checked = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fputc('\n', stderr);                   \
      if (++failures > 20) exit(1);          \
    }                                        \
  } while (0)

/* the set over chromosome 0, cut to the chromosome's length; chromosome 1 is there and empty, chromosome 2 has one group */
static void check_set(const char *what, const std::vector<gs_an_iv> &set) {
  for (uint32_t ln = 1; ln <= 40; ln++) {
    std::vector<gs_an_iv> v;
    for (gs_an_iv x : set) {
      if (x.end > ln) x.end = ln;
      if (x.start < x.end) v.push_back(x);
    }
    gs_an_host h;
    CHECK(gs_an_build({v, {}, {{7, 0, ln}}}, GS_AN_MAX_ENTRIES, h, nullptr), "%s: build refused", what);
    const gs_an_table t = h.table();
    for (uint32_t n = 0; n <= 24; n++)
      for (uint32_t x = 0; x < ln; x++)
        for (int plus = 0; plus < 2; plus++) {
          /* the restatement: the bases, one by one */
          std::set<uint32_t> want;
          bool any = false;
          for (long long i = 0; i < (long long)n; i++) {
            const long long base = plus ? (long long)x - i : (long long)x + i; /* '+' ends at x, '-' begins at x */
            if (base < 0 || base >= (long long)ln) continue;
            any = true;
            for (const gs_an_iv &iv : v)
              if ((long long)iv.start <= base && base < (long long)iv.end) want.insert(iv.group);
          }
          uint64_t a = 0, b = 0;
          CHECK(gs_an_decoded_footprint(x, plus != 0, n, ln, a, b) == any, "%s: LN %u n %u x %u %c: empty or not", what, ln, n, x,
                plus ? '+' : '-');
          if (any) CHECK(a < b && b <= ln, "%s: LN %u n %u x %u %c: footprint [%llu, %llu)", what, ln, n, x, plus ? '+' : '-',
                         (unsigned long long)a, (unsigned long long)b);
          std::vector<uint32_t> got;
          const uint32_t k = gs_an_decoded_visit(t, 0, x, plus != 0, n, ln, [&](uint32_t g) { got.push_back(g); });
          CHECK(k == got.size() && k == gs_an_decoded_count(t, 0, x, plus != 0, n, ln), "%s: LN %u n %u x %u %c: counts differ", what, ln, n, x,
                plus ? '+' : '-');
          CHECK(got == std::vector<uint32_t>(want.begin(), want.end()), "%s: LN %u n %u x %u %c: %zu features, %zu expected", what, ln, n, x,
                plus ? '+' : '-', got.size(), want.size());
          CHECK(gs_an_decoded_count(t, 1, x, plus != 0, n, ln) == 0, "%s: the empty chromosome has a feature", what);
          CHECK(gs_an_decoded_count(t, 2, x, plus != 0, n, ln) == (any ? 1u : 0u), "%s: LN %u n %u x %u %c: the covered chromosome", what, ln,
                n, x, plus ? '+' : '-');
          CHECK(gs_an_decoded_count(t, 3, x, plus != 0, n, ln) == 0, "%s: a chromosome beyond the table", what);
          checked++;
        }
  }
}

int main() {
  check_set("none", {});
  check_set("ends", {{0, 0, 1}, {1, 39, 40}, {2, 22, 23}});
  check_set("abutting", {{0, 5, 10}, {1, 10, 15}, {2, 15, 16}, {0, 16, 30}});
  check_set("gene over exons", {{0, 3, 37}, {1, 3, 8}, {2, 12, 17}, {3, 20, 26}, {0, 30, 33}, {4, 30, 37}});
  check_set("one group in pieces", {{0, 2, 4}, {1, 5, 6}, {0, 7, 9}, {2, 3, 8}, {0, 20, 21}, {1, 22, 24}, {0, 25, 26}});
  {
    std::vector<gs_an_iv> v;
    for (uint32_t g = 0; g < 70; g++) v.push_back({g, 18 - (g % 7), 19 + (g % 5)});
    check_set("stacked", v);
  }
  /* the words of the rule, once: n = 23, LN = 40, x = 30: '+' is [8, 31), '-' is [30, 40) after the clip */
  uint64_t a, b;
  CHECK(gs_an_decoded_footprint(30, true, 23, 40, a, b) && a == 8 && b == 31, "'+' at 30: [%llu, %llu)", (unsigned long long)a,
        (unsigned long long)b);
  CHECK(gs_an_decoded_footprint(30, false, 23, 40, a, b) && a == 30 && b == 40, "'-' at 30: [%llu, %llu)", (unsigned long long)a,
        (unsigned long long)b);
  CHECK(gs_an_decoded_footprint(3, true, 23, 40, a, b) && a == 0 && b == 4, "'+' at 3 is clipped, not wrapped: [%llu, %llu)",
        (unsigned long long)a, (unsigned long long)b);
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("decode_annot_check ok (%llu footprints)\n", checked);
  return 0;
}
