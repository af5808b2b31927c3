/* kmers_scan_check.cpp -- gs_kmers_scan.h as a host program (make -C guidescan-cli_amd/csrc kmers-check, under the
 * address and undefined-behaviour sanitizers; no GPU and no library):
 *   1. every string of at most 6 bytes over {',', '\n', '\r', ' ', 'A', '+', '1'} (7 behind the plain header), placed
 *      behind three headers (the plain one; permuted with another column; a name given twice) in three ways - as the
 *      whole body behind a good row, in front of a good row, and as the tail of a row whose first fields are given - goes
 *      through the passes of the device reader (gs_km_host_parse: summaries, composition, line starts, the line walk,
 *      the emit) at several tile sizes, window sizes and alignments, down to 1 byte, and through cli::read_kmers itself:
 *      the same rows and fields, the same first error, and "several shapes" exactly when the host's rows have several;
 *   2. gs_km_compose is associative on random triples of summaries and gs_km_identity() is neutral on both sides. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "cli_common.hpp"
#include "gs_kmers_scan.h"

namespace {

struct config {
  uint64_t tile;
  uint32_t win, phase;
};
const config configs[] = {{1, 1, 0}, {2, 2, 1}, {3, 3, 5}, {5, 16, 0}, {7, 5, 9}, {16, 16, 3}, {4096, 16, 15}};

struct header_form {
  const char *header, *good, *prefix; /* a row that parses; the first fields of a row whose tail is the string */
};
const header_form forms[] = {
    {"id,sequence,pam,chromosome,position,sense", "i1,AC,GG,c,5,+", "i,AC,GG,c,"},
    {"x,pam,sequence ,id,chromosome,sense,\tposition", "x,GG,AC,i1,c,+,5", "x,GG,AC,i,c,+,"},
    {"id,sequence,pam,chromosome,sense,position,id", "i0,AC,GG,c,-,5,i1", "i,AC,GG,c,-,"},
};

std::string show(const std::string &s) {
  std::string o;
  for (char c : s) o += c == '\n' ? "\\n" : c == '\r' ? "\\r" : c == '\t' ? "\\t" : std::string(1, c);
  return o;
}

uint64_t g_runs = 0;

bool check(const std::string &file, bool all_configs) {
  std::vector<cli::kmer_row> rows;
  std::string err;
  std::istringstream in(file);
  const bool ok = cli::read_kmers(in, rows, err);
  bool mixed = false;
  for (const cli::kmer_row &r : rows) mixed = mixed || r.sequence.size() != rows[0].sequence.size() || r.pam.size() != rows[0].pam.size();
  mixed = mixed || (!rows.empty() && rows[0].sequence.empty());
  for (const config &c : configs) {
    if (!all_configs && c.tile != 1 && c.tile != 4096) continue;
    gs_km_parsed p;
    gs_km_host_parse((const uint8_t *)file.data(), file.size(), c.tile, c.win, c.phase, p);
    g_runs++;
    static const char *const what[5] = {"", "kmers row with too few columns: ", "kmers position is not an integer: ", "empty kmers file",
                                        "kmers file lacks column "};
    const std::string got_err = p.bad_kind ? what[p.bad_kind] + p.bad_text : "";
    bool same = ok == (p.bad_kind == GS_KM_OK) && got_err == (ok ? "" : err);
    if (same && ok) {
      same = p.mixed == mixed && p.n == rows.size();
      if (same && !mixed) {
        std::string seqs, pams, ids;
        for (size_t r = 0; r < rows.size() && same; r++) {
          seqs += rows[r].sequence, pams += rows[r].pam, ids += rows[r].id;
          same = p.id_off[r + 1] == ids.size() && p.sense01[r] == (rows[r].sense == "+" ? 1 : 0);
        }
        same = same && seqs == std::string(p.seqs.begin(), p.seqs.end()) && pams == std::string(p.pams.begin(), p.pams.end()) &&
               ids == std::string(p.ids.begin(), p.ids.end()) && (rows.empty() || (p.L == rows[0].sequence.size() && p.P == rows[0].pam.size()));
      }
    } else if (same && (p.bad_kind == GS_KM_FEW || p.bad_kind == GS_KM_POSITION)) {
      same = file.compare((size_t)p.bad_off, (size_t)p.bad_len, p.bad_text) == 0; /* the bytes stand where the report says */
    }
    if (!same) {
      fprintf(stderr, "FAIL: \"%s\" tile %llu window %u phase %u: host %s \"%s\" %zu row(s)%s, model kind %u \"%s\" %llu row(s)%s\n",
              show(file).c_str(), (unsigned long long)c.tile, c.win, c.phase, ok ? "ok" : "error", show(err).c_str(), rows.size(),
              mixed ? " mixed" : "", p.bad_kind, show(got_err).c_str(), (unsigned long long)p.n, p.mixed ? " mixed" : "");
      return false;
    }
  }
  return true;
}

}  // namespace

int main() {
  static const char alphabet[] = {',', '\n', '\r', ' ', 'A', '+', '1'};
  const uint64_t A = sizeof alphabet;
  uint64_t strings = 0;
  if (!check("", true) || !check("\n", true) || !check("\r\n", true) || !check("id,sequence\n", true) || !check("sense,position,chromosome\n", true))
    return 1;
  for (int len = 0; len <= 7; len++) {
    uint64_t count = 1;
    for (int i = 0; i < len; i++) count *= A;
    std::string s((size_t)len, ' ');
    for (uint64_t v = 0; v < count; v++) {
      uint64_t x = v;
      for (int i = 0; i < len; i++, x /= A) s[(size_t)i] = alphabet[x % A];
      strings++;
      for (size_t f = 0; f < (len <= 6 ? 3u : 1u); f++) {
        const header_form &h = forms[f];
        const std::string head = std::string(h.header) + "\n";
        const bool all = len <= 5;
        if (!check(head + h.good + "\n" + s, all) || !check(head + s + "\n" + h.good + "\r\n", all) || !check(head + h.prefix + s, all)) return 1;
        if (len <= 4 && (!check(std::string(h.header) + s, all) || !check(s + head + h.good, all))) return 1; /* the string in and ahead of the header */
      }
    }
  }
  /* associativity */
  std::mt19937_64 rng(12345);
  auto random_sum = [&]() {
    std::string s((size_t)(rng() % 5), ' ');
    for (char &c : s) c = alphabet[rng() % A];
    return gs_km_summarize((const uint8_t *)s.data(), s.size());
  };
  auto same = [](const gs_km_sum &a, const gs_km_sum &b) { return a.len == b.len && a.n_nl == b.n_nl && a.open == b.open; };
  const uint64_t triples = 2000000;
  for (uint64_t i = 0; i < triples; i++) {
    const gs_km_sum a = random_sum(), b = random_sum(), c = random_sum();
    if (!same(gs_km_compose(gs_km_compose(a, b), c), gs_km_compose(a, gs_km_compose(b, c)))) {
      fprintf(stderr, "FAIL: the composition is not associative (triple %llu)\n", (unsigned long long)i);
      return 1;
    }
    if (!same(gs_km_compose(gs_km_identity(), b), b) || !same(gs_km_compose(b, gs_km_identity()), b)) {
      fprintf(stderr, "FAIL: the identity is not neutral\n");
      return 1;
    }
  }
  printf("kmers-check ok: %llu strings, %llu runs of the passes against cli::read_kmers, %llu triples\n", (unsigned long long)strings,
         (unsigned long long)g_runs, (unsigned long long)triples);
  return 0;
}
