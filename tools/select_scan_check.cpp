/* select_scan_check.cpp -- gs_select_scan.h as a host program (make -C guidescan-cli_amd/csrc select-check, under the
 * address and undefined-behaviour sanitizers; no GPU and no library).
 *   1. The sequence rules on a few thousand random short sequences - low-complexity alphabets so that runs and motifs
 *      happen, motifs planted at offset 0 and at the last offset, runs that end on the last base, lower case - under
 *      random rules, against a restatement per offset and per letter: the IUPAC sets spelled as strings, the run counted
 *      by comparing neighbours, the GC bound in integers.  The charge order GC, run, motif; a motif of k + 1 letters.
 *   2. The packed motif sets: put and get at every position, and the complement as the set of the complemented letters.
 *   3. The greedy walk on random record sets - several chromosomes, both senses with and without --start, positions dense
 *      enough for equal cuts, unmarked records in between, D from 1 beyond the span, N from 1 beyond the group - against a
 *      quadratic restatement that tests every candidate against every earlier record it kept. */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "gs_select_scan.h"

namespace {

int fail(const char *what, uint64_t a, uint64_t b, uint64_t c) {
  fprintf(stderr, "select-check: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
  return 1;
}

const char *iupac_letters(char c) {
  switch (c) {
    case 'A': return "A";
    case 'C': return "C";
    case 'G': return "G";
    case 'T': return "T";
    case 'R': return "AG";
    case 'Y': return "CT";
    case 'S': return "CG";
    case 'W': return "AT";
    case 'K': return "GT";
    case 'M': return "AC";
    case 'B': return "CGT";
    case 'D': return "AGT";
    case 'H': return "ACT";
    case 'V': return "ACG";
    case 'N': return "ACGT";
  }
  return "";
}
char upper(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 32) : c; }
char complement_base(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C'; }

/* the rule restated over strings */
uint32_t charge_by_letters(const std::string &seq, uint32_t gc_min, uint32_t gc_max, uint32_t max_run, const std::vector<std::string> &motifs) {
  const long k = (long)seq.size();
  long gc = 0, longest = 0;
  for (long i = 0; i < k; i++) {
    if (upper(seq[i]) == 'G' || upper(seq[i]) == 'C') gc++;
    long run = 1;
    while (i + run < k && upper(seq[i + run]) == upper(seq[i])) run++;
    longest = std::max(longest, run);
  }
  if (!((long)gc_min * k <= 100 * gc && 100 * gc <= (long)gc_max * k)) return 1;
  if (max_run && longest > (long)max_run) return 2;
  for (const std::string &m : motifs)
    for (long o = 0; o + (long)m.size() <= k; o++) {
      bool all = true;
      for (size_t p = 0; p < m.size() && all; p++) all = std::string(iupac_letters(upper(m[p]))).find(upper(seq[o + p])) != std::string::npos;
      if (all) return 3;
    }
  return 0;
}

struct rec {
  uint32_t chr, pos;
  uint8_t sense, mark;
};

}  // namespace

int main() {
  std::mt19937_64 rng(20241021);
  static const char ALPHABET[] = "ACGTRYSWKMBDHVN";

  /* 2. packing and complement */
  for (uint32_t round = 0; round < 200; round++) {
    gs_seq_rule r;
    memset(&r, 0, sizeof r);
    uint32_t want[GS_SEQ_MOTIFS][GS_SEQ_MOTIF_LETTERS];
    for (uint32_t m = 0; m < GS_SEQ_MOTIFS; m++)
      for (uint32_t p = 0; p < GS_SEQ_MOTIF_LETTERS; p++) gs_sl_motif_put(r, m, p, want[m][p] = (uint32_t)(rng() % 16));
    for (uint32_t m = 0; m < GS_SEQ_MOTIFS; m++)
      for (uint32_t p = 0; p < GS_SEQ_MOTIF_LETTERS; p++)
        if (gs_sl_motif_set(r, m, p) != want[m][p]) return fail("packed set", round, m, p);
  }
  for (const char *c = ALPHABET; *c; c++) {
    uint32_t by_letters = 0;
    for (const char *l = iupac_letters(*c); *l; l++) by_letters |= gs_sl_base_bit((uint8_t)complement_base(*l));
    if (gs_sl_complement(gs_sl_iupac((uint8_t)*c)) != by_letters) return fail("complement", (uint64_t)*c, 0, 0);
    if (gs_sl_iupac((uint8_t)(*c + 32)) != gs_sl_iupac((uint8_t)*c)) return fail("lower case letter", (uint64_t)*c, 0, 0);
    uint32_t set = 0;
    for (const char *l = iupac_letters(*c); *l; l++) set |= gs_sl_base_bit((uint8_t)*l);
    if (gs_sl_iupac((uint8_t)*c) != set) return fail("letter set", (uint64_t)*c, 0, 0);
  }
  if (gs_sl_iupac('X') || gs_sl_iupac('U') || gs_sl_iupac(0) || gs_sl_base_bit('N')) return fail("a letter outside the alphabet", 0, 0, 0);

  /* 1. the sequence rules */
  uint64_t sequences = 0, charged[4] = {0, 0, 0, 0}, at_first = 0, at_last = 0, run_at_end = 0;
  for (uint32_t round = 0; round < 300; round++) {
    const uint32_t k = round % 4 == 0 ? 23 : round % 4 == 1 ? 1 + (uint32_t)(rng() % 8) : 20;
    /* a rule */
    gs_seq_rule r;
    memset(&r, 0, sizeof r);
    r.gc_max = 100;
    if (round % 3) {
      r.gc_min = (uint32_t)(rng() % 60);
      r.gc_max = r.gc_min + (uint32_t)(rng() % (101 - r.gc_min));
    }
    r.max_run = round % 5 == 0 ? 0 : 1 + (uint32_t)(rng() % 5);
    std::vector<std::string> motifs;
    const uint32_t nm = round % 7 == 0 ? 0 : 1 + (uint32_t)(rng() % GS_SEQ_MOTIFS);
    for (uint32_t m = 0; m < nm; m++) {
      uint32_t len = 1 + (uint32_t)(rng() % 7);
      if (m == 0 && round % 2) len = std::min(k + 1, GS_SEQ_MOTIF_LETTERS); /* longer than k: matches nothing */
      if (m == 1 && round % 2) len = std::min(k, GS_SEQ_MOTIF_LETTERS);     /* the whole protospacer */
      std::string s;
      for (uint32_t p = 0; p < len; p++) s += ALPHABET[rng() % (len > 4 ? 15 : 4 + rng() % 12)];
      if (round % 9 == 4) s[rng() % len] = (char)(s[0] + 32);
      motifs.push_back(s);
      r.motif_len[m] = (uint8_t)len;
      for (uint32_t p = 0; p < len; p++) gs_sl_motif_put(r, m, p, gs_sl_iupac((uint8_t)s[p]));
    }
    r.n_motifs = nm;
    if (!gs_sl_rule_ok(r)) return fail("a rule within its bounds refused", round, 0, 0);
    for (uint32_t i = 0; i < 16; i++) {
      const uint32_t letters = 1 + (uint32_t)(rng() % 4);
      std::string s;
      for (uint32_t t = 0; t < k; t++) s += "ACGT"[(rng() % 3 == 0 ? rng() % 4 : rng() % letters)];
      if (i % 4 == 1 && nm > 2) { /* a concrete instance of a short motif at offset 0 or at the last one */
        const std::string &m = motifs[2 + rng() % (nm - 2)];
        if (m.size() <= k) {
          const size_t o = i % 8 == 1 ? 0 : k - m.size();
          for (size_t p = 0; p < m.size(); p++) s[o + p] = iupac_letters(upper(m[p]))[0];
        }
      }
      if (i % 4 == 2 && r.max_run && r.max_run < k) /* a run one too long that ends on the last base */
        for (uint32_t t = 0; t <= r.max_run; t++) s[k - 1 - t] = 'T';
      if (i % 8 == 7) s[rng() % k] = (char)(s[0] + 32);
      const uint32_t got = gs_sl_charge(r, (const uint8_t *)s.data(), k);
      const uint32_t want = charge_by_letters(s, r.gc_min, r.gc_max, r.max_run, motifs);
      if (got != want) {
        fprintf(stderr, "select-check: %s under gc %u:%u run %u\n", s.c_str(), r.gc_min, r.gc_max, r.max_run);
        return fail("charge", round, got, want);
      }
      sequences++;
      charged[got]++;
      /* where the first matching motif offset lies, and whether the longest run ends the sequence */
      for (uint32_t m = 0; m < nm && got == 3; m++) {
        if (r.motif_len[m] > k) continue;
        if (gs_sl_motif_at(r, m, (const uint8_t *)s.data(), 0)) at_first++;
        if (gs_sl_motif_at(r, m, (const uint8_t *)s.data(), k - r.motif_len[m])) at_last++;
      }
      if (got == 2 && i % 4 == 2) run_at_end++;
    }
  }
  for (int c = 0; c < 4; c++)
    if (charged[c] < 50) return fail("too few sequences with this charge: the inputs decide nothing", (uint64_t)c, charged[c], sequences);
  if (at_first < 20 || at_last < 20 || run_at_end < 20) return fail("too few matches at the ends", at_first, at_last, run_at_end);

  /* 3. the walk */
  uint64_t groups = 0, kept_total = 0, passed_total = 0, cut_short = 0, equal_cuts = 0;
  for (uint32_t round = 0; round < 3000; round++) {
    const uint32_t k = round % 3 == 0 ? 23 : 20, P = round % 3 == 0 ? 4 : 3;
    const bool start = round % 2;
    const uint32_t C = round % 5 == 0 ? 0 : round % 5 == 1 ? k : 3;
    const uint32_t n = round % 13 == 0 ? (uint32_t)(rng() % 2) : 1 + (uint32_t)(rng() % 150);
    const uint32_t spread = 1 + (uint32_t)(rng() % 400);
    const uint32_t base = round % 7 == 3 ? 0xFFFFFFFFu - k - P - spread - 2 : (uint32_t)(rng() % 1000);
    const uint32_t D = round % 6 == 0 ? 1 : round % 6 == 1 ? spread + 64 : 1 + (uint32_t)(rng() % 60);
    const uint32_t N = round % 4 == 0 ? 1 + (uint32_t)(rng() % 3) : round % 4 == 1 ? n + 5 : 1 + (uint32_t)(rng() % (n + 1));
    std::vector<rec> r;
    for (uint32_t i = 0; i < n; i++)
      r.push_back(rec{(uint32_t)(rng() % 3) * 0x7FFFFFFFu, base + 1 + (uint32_t)(rng() % spread), (uint8_t)(rng() % 2 ? '+' : '-'),
                      (uint8_t)(rng() % 5 != 0)});
    std::vector<uint64_t> key(n), list(std::min(n, N) + 1);
    std::vector<uint8_t> mark(n), keep(n + 1, 7);
    for (uint32_t i = 0; i < n; i++) {
      key[i] = gs_sl_key(r[i].chr, r[i].pos, r[i].sense, k, P, C, start);
      mark[i] = r[i].mark;
      if ((uint32_t)key[i] != gs_pr_cut(r[i].pos, r[i].sense, k, P, C, start) || (uint32_t)(key[i] >> 32) != r[i].chr)
        return fail("key", round, i, 0);
    }
    uint32_t passed = 0, marked = 0;
    const uint32_t kept = gs_sl_walk(key.data(), mark.data(), n, D, N, list.data(), keep.data(), &passed, &marked);
    if (keep[n] != 7) return fail("the walk wrote beyond its records", round, n, 0);
    /* the restatement: a record is kept iff it is marked, fewer than N are kept, and no earlier kept record of its
     * chromosome has its cut within D - found by looking back over every earlier record */
    std::vector<uint8_t> want(n, 0);
    uint32_t want_kept = 0, want_passed = 0, want_marked = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (!r[i].mark) continue;
      want_marked++;
      if (want_kept >= N) {
        cut_short++;
        continue;
      }
      bool clear = true;
      const int64_t x = gs_pr_cut(r[i].pos, r[i].sense, k, P, C, start);
      for (uint32_t j = 0; j < i; j++) {
        if (!want[j] || r[j].chr != r[i].chr) continue;
        const int64_t y = gs_pr_cut(r[j].pos, r[j].sense, k, P, C, start);
        if (llabs(x - y) < (int64_t)D) clear = false;
        if (x == y) equal_cuts++;
      }
      if (clear) {
        want[i] = 1;
        want_kept++;
      } else {
        want_passed++;
      }
    }
    if (kept != want_kept || passed != want_passed || marked != want_marked) return fail("the walk's counts", round, kept, want_kept);
    for (uint32_t i = 0, t = 0; i < n; i++) {
      if (keep[i] != want[i]) return fail("keep", round, i, keep[i]);
      if (keep[i] && list[t++] != key[i]) return fail("the kept list", round, i, t);
    }
    groups++;
    kept_total += kept;
    passed_total += passed;
  }
  if (passed_total < 1000 || cut_short < 1000 || equal_cuts < 100) return fail("the walks decide too little", passed_total, cut_short, equal_cuts);
  printf("select-check: %llu sequences (%llu pass, %llu GC, %llu run, %llu motif; motif at offset 0 %llu, at the last %llu), "
         "%llu walks with %llu kept and %llu passed over, all as restated\n",
         (unsigned long long)sequences, (unsigned long long)charged[0], (unsigned long long)charged[1], (unsigned long long)charged[2],
         (unsigned long long)charged[3], (unsigned long long)at_first, (unsigned long long)at_last, (unsigned long long)groups,
         (unsigned long long)kept_total, (unsigned long long)passed_total);
  return 0;
}
