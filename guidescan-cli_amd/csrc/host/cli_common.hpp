/*
 * cli_common.hpp -- what `guidescan index`, `kmers` and `enumerate` share: the readers of PREFIX.gs, PREFIX.dna and the
 * kmers file, the options of the candidate scan, and the guard that closes a command's index handles.
 */
#ifndef GS_CLI_COMMON_HPP
#define GS_CLI_COMMON_HPP

#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "guidescan_amd.h"

namespace cli {

struct genome_structure {
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
};

inline bool read_gs(const std::string &path, genome_structure &gs, std::string &err) { /* seq_io.cxx:124-144 */
  std::ifstream in(path);
  if (!in) {
    err = "No genome structure file " + path;
    return false;
  }
  std::string name, len;
  while (std::getline(in, name) && std::getline(in, len)) {
    char *end = nullptr;
    const unsigned long long v = strtoull(len.c_str(), &end, 10);
    if (end == len.c_str() || (*end && *end != '\r')) {
      err = "malformed genome structure file " + path + ": length '" + len + "' of " + name;
      return false;
    }
    gs.names.push_back(name);
    gs.lengths.push_back(v);
  }
  return true;
}

/* a BED file (`enumerate --regions`, `--annotate`; `decode --annotate`) against a genome structure; the parser's message
 * with its line number, "regions" replaced by `what` */
inline bool read_bed(const std::string &path, const genome_structure &gs, const std::string &prefix, const std::string &what,
                     gs_regions **out) {
  std::vector<const char *> names;
  for (auto &n : gs.names) names.push_back(n.c_str());
  const gs_genome_structure cgs{names.data(), gs.lengths.data(), (uint32_t)names.size()};
  gs_regions_report rep;
  const gs_status rc = gs_regions_parse_file(path.c_str(), &cgs, prefix.c_str(), out, &rep);
  if (rc == GS_OK) return true;
  if (rc == GS_ERR_FORMAT && rep.bad_text) { /* the parser says "regions line N: ..." / "regions file: ..." */
    const std::string msg = rep.bad_text;
    std::cerr << "error: " << (msg.compare(0, 7, "regions") == 0 ? what + msg.substr(7) : msg) << " (" << path << ")\n";
  } else if (rc == GS_ERR_IO)
    std::cerr << "error: cannot read the " << what << " file " << path << "\n";
  else
    std::cerr << "error: " << what << " file " << path << ": " << gs_status_string(rc) << "\n";
  gs_free(rep.bad_text);
  return false;
}

/* what the candidate scan takes (scripts/generate_kmers.py:14-47) */
struct candidate_opts {
  std::string pam = "NGG", prefix;
  long long k = 20, min_chr = 0;
  bool start = false, have_chromosomes = false;
  std::vector<std::string> chromosomes;
};
inline std::vector<std::string> split_commas(const std::string &v) {
  std::vector<std::string> out;
  std::stringstream ss(v);
  std::string f;
  while (std::getline(ss, f, ',')) out.push_back(f);
  return out;
}
inline bool read_file(const std::string &path, std::string &text) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in) return false;
  text.resize((size_t)in.tellg());
  in.seekg(0);
  in.read(&text[0], (std::streamsize)text.size());
  return (bool)in;
}
/* the chromosomes a candidate scan takes, in .gs order, and where each begins in the .dna text */
inline bool select_chromosomes(const std::string &prefix, const genome_structure &gs, uint64_t dna_size, const candidate_opts &co,
                        std::vector<size_t> &sel, std::vector<uint64_t> &begin, std::string &err) {
  begin.assign(gs.lengths.size() + 1, 0);
  for (size_t c = 0; c < gs.lengths.size(); c++) begin[c + 1] = begin[c] + gs.lengths[c];
  if (begin.back() != dna_size) {
    /* the reference counts untrimmed line lengths (seq_io.cxx:103): blanks at line ends make the two disagree */
    err = "the chromosome lengths in " + prefix + ".gs sum to " + std::to_string(begin.back()) + " but " + prefix + ".dna holds " +
          std::to_string(dna_size) + " bases: the chromosomes cannot be cut from it";
    return false;
  }
  for (const std::string &want : co.chromosomes) {
    bool found = false;
    for (const std::string &n : gs.names) found = found || n == want;
    if (!found) {
      err = "--chromosomes: no chromosome named '" + want + "' in " + prefix + ".gs";
      return false;
    }
  }
  for (size_t c = 0; c < gs.names.size(); c++) {
    if ((long long)gs.lengths[c] < co.min_chr) continue; /* scripts/generate_kmers.py:132 */
    if (co.have_chromosomes && std::find(co.chromosomes.begin(), co.chromosomes.end(), gs.names[c]) == co.chromosomes.end()) continue;
    sel.push_back(c);
  }
  return true;
}
/* one of the candidate options? (i advances over its value) */
inline bool candidate_option(const std::string &a, int &i, int argc, char **argv, candidate_opts &co, bool &bad) {
  auto val = [&]() -> const char * {
    if (i + 1 >= argc) {
      std::cerr << "error: " << a << " needs a value\n";
      bad = true;
      return "";
    }
    return argv[++i];
  };
  if (a == "--pam") co.pam = val();
  else if (a == "--kmer-length") co.k = atoll(val());
  else if (a == "--min-chr-length") co.min_chr = atoll(val());
  else if (a == "--prefix") co.prefix = val();
  else if (a == "--chromosomes") {
    co.have_chromosomes = true;
    for (auto &n : split_commas(val())) co.chromosomes.push_back(n);
  } else return false;
  return true;
}

/* the sequence rules on the candidates of a scan (`kmers`, `enumerate --all-candidates`; csrc/gs_select_scan.h, no
 * counterpart in the reference): --gc MIN:MAX, --max-run R, --exclude-motif M1,M2,..., --exclude-site M1,M2,... */
struct seq_rule_opts {
  gs_seq_rule rule;
  bool given = false;
  seq_rule_opts() { gs_seq_rule_init(&rule); }
};
/* one of them? (i advances over its value); a value that is refused is one line on stderr and `bad` */
inline bool seq_rule_option(const std::string &a, int &i, int argc, char **argv, seq_rule_opts &so, bool &bad) {
  if (a != "--gc" && a != "--max-run" && a != "--exclude-motif" && a != "--exclude-site") return false;
  so.given = true;
  if (i + 1 >= argc) {
    std::cerr << "error: " << a << " needs a value\n";
    bad = true;
    return true;
  }
  const std::string v = argv[++i];
  auto digits = [](const std::string &s, unsigned long &out) {
    if (s.empty() || s.size() > 9 || s.find_first_not_of("0123456789") != std::string::npos) return false;
    out = strtoul(s.c_str(), nullptr, 10);
    return true;
  };
  if (a == "--gc") {
    const size_t colon = v.find(':');
    unsigned long lo = 0, hi = 0;
    if (colon == std::string::npos || !digits(v.substr(0, colon), lo) || !digits(v.substr(colon + 1), hi) || lo > hi || hi > 100) {
      std::cerr << "error: --gc " << v << ": MIN:MAX, integer percentages with 0 <= MIN <= MAX <= 100\n";
      bad = true;
      return true;
    }
    so.rule.gc_min = (uint32_t)lo;
    so.rule.gc_max = (uint32_t)hi;
  } else if (a == "--max-run") {
    unsigned long r = 0;
    if (!digits(v, r) || r < 1) {
      std::cerr << "error: --max-run " << v << ": the longest run of one letter, at least 1\n";
      bad = true;
      return true;
    }
    so.rule.max_run = (uint32_t)r;
  } else {
    std::vector<std::string> motifs = split_commas(v);
    if (motifs.empty() || v.back() == ',') motifs.push_back(""); /* refused below, as an empty motif */
    for (const std::string &m : motifs)
      if (gs_seq_rule_add_motif(&so.rule, m.c_str(), a == "--exclude-site") != GS_OK) {
        std::cerr << "error: " << a << ": " << gs_status_string(GS_ERR_FORMAT) << "\n";
        bad = true;
        return true;
      }
  }
  return true;
}
/* "Sequence rules: kept K of N candidate(s); F failed --gc, F --max-run, F a motif" */
inline std::string seq_rule_line(const uint64_t counts[4]) {
  return "Sequence rules: kept " + std::to_string(counts[0] - counts[1] - counts[2] - counts[3]) + " of " + std::to_string(counts[0]) +
         " candidate(s); " + std::to_string(counts[1]) + " failed --gc, " + std::to_string(counts[2]) + " --max-run, " +
         std::to_string(counts[3]) + " a motif\n";
}
/* the scan's candidates through the rule on the scan's device: *km becomes the filtered object, counts add up */
inline gs_status apply_seq_rule(const seq_rule_opts &so, gs_kmers **km, uint64_t counts[4]) {
  if (!so.given) return GS_OK;
  gs_kmers *f = nullptr;
  uint64_t c[4] = {0, 0, 0, 0};
  const gs_status rc = gs_kmers_filter(*km, &so.rule, nullptr, &f, c);
  if (rc != GS_OK) return rc;
  gs_kmers_free(*km);
  *km = f;
  for (int i = 0; i < 4; i++) counts[i] += c[i];
  return GS_OK;
}

struct kmer_row {
  std::string id, sequence, pam, chromosome, sense;
  long long position;
};

inline std::string trim_field(const std::string &s) { /* include/csv.hpp:1110-1116: ' ' and '\t' */
  size_t b = 0, e = s.size();
  while (b < e && (s[b] == ' ' || s[b] == '\t')) b++;
  while (e > b && (s[e - 1] == ' ' || s[e - 1] == '\t')) e--;
  return s.substr(b, e - b);
}
inline std::vector<std::string> split_csv(const std::string &line) {
  std::vector<std::string> out;
  size_t b = 0;
  for (;;) {
    const size_t c = line.find(',', b);
    out.push_back(trim_field(line.substr(b, c == std::string::npos ? std::string::npos : c - b)));
    if (c == std::string::npos) break;
    b = c + 1;
  }
  return out;
}
/* src/genomics/kmer.cxx:9-25, from an open stream */
inline bool read_kmers(std::istream &in, std::vector<kmer_row> &rows, std::string &err) {
  std::string line;
  if (!std::getline(in, line)) {
    err = "empty kmers file";
    return false;
  }
  if (!line.empty() && line.back() == '\r') line.pop_back();
  const std::vector<std::string> header = split_csv(line);
  const char *want[6] = {"id", "sequence", "pam", "chromosome", "position", "sense"};
  int col[6];
  for (int i = 0; i < 6; i++) {
    col[i] = -1;
    for (size_t j = 0; j < header.size(); j++)
      if (header[j] == want[i]) col[i] = (int)j;
    if (col[i] < 0) {
      err = std::string("kmers file lacks column ") + want[i];
      return false;
    }
  }
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const std::vector<std::string> f = split_csv(line);
    if (f.size() < header.size()) {
      err = "kmers row with too few columns: " + line;
      return false;
    }
    kmer_row r;
    r.id = f[col[0]];
    r.sequence = f[col[1]];
    r.pam = f[col[2]];
    r.chromosome = f[col[3]];
    char *end = nullptr;
    r.position = strtoll(f[col[4]].c_str(), &end, 10);
    if (end == f[col[4]].c_str() || *end) {
      err = "kmers position is not an integer: " + f[col[4]];
      return false;
    }
    r.sense = f[col[5]];
    rows.push_back(std::move(r));
  }
  return true;
}
/* src/genomics/kmer.cxx:9-25 */
inline bool read_kmers(const std::string &path, std::vector<kmer_row> &rows, std::string &err) {
  std::ifstream in(path);
  if (!in) {
    err = "cannot open kmers file";
    return false;
  }
  return read_kmers((std::istream &)in, rows, err);
}

/* the index handles of a command, one per device: closed when the command returns, whichever way */
struct index_set {
  std::vector<gs_index *> ix;
  explicit index_set(size_t n) : ix(n, nullptr) {}
  index_set(const index_set &) = delete;
  index_set &operator=(const index_set &) = delete;
  ~index_set() {
    for (gs_index *p : ix)
      if (p) gs_index_close(p);
  }
};

}  // namespace cli

#endif
