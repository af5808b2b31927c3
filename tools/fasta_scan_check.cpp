/* fasta_scan_check.cpp -- gs_fasta_scan.h as a host program (make -C guidescan-cli_amd/csrc fasta-check, under the
 * address and undefined-behaviour sanitizers; no GPU and no library):
 *   1. every string of at most 8 bytes over {'\n', '>', ' ', '\r', 'a', 'C'}, under both rule sets, cut into tiles of 1, 2, 3
 *      and 5 bytes and put through summarize / compose / walk as the device passes do, against a plain line-by-line
 *      reader written out below: the text, and each record's title, extents and untrimmed length;
 *   2. gs_fa_compose is associative on random triples of summaries (of random strings, the left one with or without the
 *      file's start in front), and gs_fa_identity() is neutral on both sides. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gs_fasta_scan.h"

namespace {

struct record {
  uint64_t title_off, title_len, text_off, text_len, line_len;
  bool operator==(const record &o) const {
    return title_off == o.title_off && title_len == o.title_len && text_off == o.text_off && text_len == o.text_len && line_len == o.line_len;
  }
};
struct parsed {
  std::string text;
  std::vector<record> recs;
};

bool blank(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

/* the plain reader: one line after the other */
parsed plain(const std::string &raw, uint32_t rules) {
  parsed p;
  size_t at = 0;
  while (at < raw.size()) {
    size_t e = raw.find('\n', at);
    if (e == std::string::npos) e = raw.size();
    if (raw[at] == '>' && e > at) {
      if (!p.recs.empty()) p.recs.back().text_len = p.text.size() - p.recs.back().text_off;
      p.recs.push_back({at, e - at, p.text.size(), 0, 0});
    } else {
      if (!p.recs.empty()) p.recs.back().line_len += e - at;
      if (rules == GS_FA_RULES_INDEX) {
        size_t b = at, z = e;
        while (b < z && blank((unsigned char)raw[b])) b++;
        while (z > b && blank((unsigned char)raw[z - 1])) z--;
        for (size_t i = b; i < z; i++) p.text.push_back(raw[i] >= 'a' && raw[i] <= 'z' ? (char)(raw[i] - 32) : raw[i]);
      } else if (!p.recs.empty()) {
        for (size_t i = at; i < e; i++)
          if (!blank((unsigned char)raw[i])) p.text.push_back(raw[i]);
      }
    }
    at = e + 1;
  }
  if (!p.recs.empty()) p.recs.back().text_len = p.text.size() - p.recs.back().text_off;
  return p;
}

struct emitter {
  std::string *text;
  std::vector<gs_fa_title> *titles;
  void keep(uint64_t at, uint8_t b) {
    if (at >= text->size()) {
      fprintf(stderr, "a kept byte beyond the counted text\n");
      exit(1);
    }
    (*text)[at] = (char)b;
  }
  void title(uint64_t i, uint64_t off, uint64_t nls, uint64_t kept) {
    gs_fa_title &t = titles->at(i);
    t.off = off, t.nls = nls, t.kept = kept;
  }
  void title_end(uint64_t i, uint64_t end) { titles->at(i).end = end; }
};

/* the device passes, sequentially, with tiles of T bytes */
parsed tiled(const std::string &raw, uint32_t rules, size_t T) {
  const uint8_t *p = (const uint8_t *)raw.data();
  const size_t len = raw.size(), nt = (len + T - 1) / T;
  auto tl = [&](size_t k) { return std::min(T, len - k * T); };
  std::vector<gs_fa_sum> sums(nt), fwd(nt + 1), bwd(nt + 1);
  for (size_t k = 0; k < nt; k++) sums[k] = gs_fa_summarize(p + k * T, tl(k));
  fwd[0] = gs_fa_file_start();
  for (size_t k = 0; k < nt; k++) fwd[k + 1] = gs_fa_compose(fwd[k], sums[k]);
  bwd[nt] = gs_fa_identity();
  for (size_t k = nt; k-- > 0;) bwd[k] = gs_fa_compose(sums[k], bwd[k + 1]);
  std::vector<uint64_t> koff(nt + 1, 0);
  gs_fa_count_only none;
  for (size_t k = 0; k < nt; k++) koff[k + 1] = koff[k] + gs_fa_walk(p + k * T, tl(k), k * T, rules, gs_fa_edge_of(fwd[k], bwd[k + 1], 0), none);
  parsed out;
  out.text.assign(koff[nt], '?');
  std::vector<gs_fa_title> titles(fwd[nt].n_titles);
  for (gs_fa_title &t : titles) t.end = len, t.off = ~0ull;
  emitter em{&out.text, &titles};
  for (size_t k = 0; k < nt; k++) {
    const uint64_t kept = gs_fa_walk(p + k * T, tl(k), k * T, rules, gs_fa_edge_of(fwd[k], bwd[k + 1], koff[k]), em);
    if (kept != koff[k + 1] - koff[k]) {
      fprintf(stderr, "the two walks of a tile disagree\n");
      exit(1);
    }
  }
  for (size_t r = 0; r < titles.size(); r++) {
    record rec;
    rec.title_off = titles[r].off;
    gs_fa_extents(titles.data(), titles.size(), r, len, fwd[nt].n_nl, koff[nt], &rec.title_len, &rec.text_off, &rec.text_len, &rec.line_len);
    out.recs.push_back(rec);
  }
  return out;
}

std::string show(const std::string &s) {
  std::string o;
  for (char c : s) o += c == '\n' ? "\\n" : c == '\r' ? "\\r" : std::string(1, c);
  return o;
}

bool same(const gs_fa_sum &a, const gs_fa_sum &b) {
  return a.len == b.len && a.n_nl == b.n_nl && a.n_titles == b.n_titles && a.tail_cls == b.tail_cls && a.first_gt == b.first_gt &&
         a.head_nb == b.head_nb && a.tail_nb == b.tail_nb;
}

}  // namespace

int main() {
  static const char alphabet[] = {'\n', '>', ' ', '\r', 'a', 'C'};
  static const size_t tiles[] = {1, 2, 3, 5};
  uint64_t strings = 0, runs = 0;
  for (int len = 0; len <= 8; len++) {
    uint64_t count = 1;
    for (int i = 0; i < len; i++) count *= 6;
    std::string s((size_t)len, ' ');
    for (uint64_t v = 0; v < count; v++) {
      uint64_t x = v;
      for (int i = 0; i < len; i++, x /= 6) s[(size_t)i] = alphabet[x % 6];
      strings++;
      for (uint32_t rules = 0; rules < 2; rules++) {
        const parsed want = plain(s, rules);
        for (size_t T : tiles) {
          const parsed got = tiled(s, rules, T);
          runs++;
          if (got.text != want.text || !(got.recs == want.recs)) {
            fprintf(stderr, "FAIL: \"%s\" rules %u tile %zu: text \"%s\" for \"%s\", %zu records for %zu\n", show(s).c_str(), rules, T,
                    show(got.text).c_str(), show(want.text).c_str(), got.recs.size(), want.recs.size());
            for (size_t r = 0; r < got.recs.size() && r < want.recs.size(); r++)
              fprintf(stderr, "  record %zu: title %llu+%llu text %llu+%llu lines %llu  for  title %llu+%llu text %llu+%llu lines %llu\n", r,
                      (unsigned long long)got.recs[r].title_off, (unsigned long long)got.recs[r].title_len, (unsigned long long)got.recs[r].text_off,
                      (unsigned long long)got.recs[r].text_len, (unsigned long long)got.recs[r].line_len, (unsigned long long)want.recs[r].title_off,
                      (unsigned long long)want.recs[r].title_len, (unsigned long long)want.recs[r].text_off, (unsigned long long)want.recs[r].text_len,
                      (unsigned long long)want.recs[r].line_len);
            return 1;
          }
        }
      }
    }
  }
  /* associativity */
  std::mt19937_64 rng(12345);
  auto random_sum = [&](bool may_start) {
    std::string s((size_t)(rng() % 7), ' ');
    for (char &c : s) c = alphabet[rng() % 6];
    gs_fa_sum x = gs_fa_summarize((const uint8_t *)s.data(), s.size());
    if (may_start && (rng() & 1)) x = gs_fa_compose(gs_fa_file_start(), x);
    return x;
  };
  const uint64_t triples = 2000000;
  for (uint64_t i = 0; i < triples; i++) {
    const gs_fa_sum a = random_sum(true), b = random_sum(false), c = random_sum(false);
    if (!same(gs_fa_compose(gs_fa_compose(a, b), c), gs_fa_compose(a, gs_fa_compose(b, c)))) {
      fprintf(stderr, "FAIL: the composition is not associative (triple %llu)\n", (unsigned long long)i);
      return 1;
    }
    if (!same(gs_fa_compose(gs_fa_identity(), b), b) || !same(gs_fa_compose(b, gs_fa_identity()), b)) {
      fprintf(stderr, "FAIL: the identity is not neutral\n");
      return 1;
    }
  }
  printf("fasta-check ok: %llu strings, %llu tiled runs against the plain reader, %llu triples\n", (unsigned long long)strings,
         (unsigned long long)runs, (unsigned long long)triples);
  return 0;
}
