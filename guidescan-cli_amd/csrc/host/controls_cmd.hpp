/*
 * controls_cmd.hpp -- `guidescan controls`: non-targeting controls for a library (no counterpart in the reference, whose
 * manual strips the CTRL guides out of its example library, manual/manual.tex:403-411).  Control plane only: the genome and
 * the index come through the stages `enumerate` uses, the walk is gs_controls_generate, the rows gs_controls_rows.
 *
 *   guidescan controls PREFIX -o KMERS -n N [--seed S] [--first I] [--pam NGG] [--kmer-length 20] [--start] [-m 3] [-a PAM]...
 *       [--gc MIN:MAX] [--max-run R] [--exclude-motif ...] [--exclude-site ...] [--min-distance H] [--max-candidates C]
 *       [--allow-short] [--prefix control_] [--device D] [--round R] [--verbose]
 *       KMERS is a kmers file for `enumerate -f`: the header and one row "id,sequence,pam,NA,0,+" per control, the id
 *       "{prefix}{i}" with i the candidate's counter.  Candidate i of seed S is a fixed word (csrc/gs_controls_scan.h); it is
 *       dropped by the sequence rules, by having any site within -m mismatches under the PAM and the -a PAMs, or by having
 *       fewer than H mismatches to a control already kept; the first N that remain, in counter order, are written.  The
 *       same options give the same file on any device, and the file for a smaller N is the head of the file for a larger.
 *       Fewer than N after C candidates: nothing is written, exit status 1; --allow-short writes what was found.
 *       --round R (for tests; not in the usage text): the counters the device takes per round (default 2^20, at most
 *       2^24); the file does not depend on it.
 */
#ifndef GS_CONTROLS_CMD_HPP
#define GS_CONTROLS_CMD_HPP

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <unistd.h>
#include <vector>

#include "guidescan_amd.h"
#include "cli_common.hpp"
#include "enumerate_cmd.hpp"

namespace controls_cmd {

inline int run(int argc, char **argv, int (*usage)()) {
  enumerate_cmd::options eo; /* the genome and index stages of `enumerate` read prefix, device and gpus from it */
  cli::seq_rule_opts so;
  std::string output, pam = "NGG", id_prefix = "control_";
  std::vector<std::string> alt_pams;
  unsigned long long n = 0, seed = 0, first = 0, max_candidates = 1ull << 32, round = 0;
  unsigned long long L = 20, mismatches = 3, min_distance = 1;
  bool start = false, allow_short = false, verbose = false, have_n = false;
  auto number = [](const char *s, unsigned long long &out) {
    if (!*s || strspn(s, "0123456789") != strlen(s) || strlen(s) > 20) return false;
    errno = 0;
    out = strtoull(s, nullptr, 10);
    return errno == 0;
  };
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    bool bad = false;
    auto val = [&]() -> const char * {
      if (i + 1 >= argc) {
        std::cerr << "error: " << a << " needs a value\n";
        bad = true;
        return "";
      }
      return argv[++i];
    };
    auto count = [&](unsigned long long &out) {
      const char *v = val();
      if (!bad && !number(v, out)) {
        std::cerr << "error: " << a << " " << v << ": a non-negative integer below 2^64\n";
        bad = true;
      }
    };
    if (cli::seq_rule_option(a, i, argc, argv, so, bad)) {
    } else if (a == "--regions" || a == "--per-region") {
      std::cerr << "error: " << a << ": controls have no site in the genome, so no region; safe-targeting controls are enumerate "
                << "--all-candidates --regions SAFE.bed --max-feature-hits 0\n";
      return 2;
    } else if (a == "-f" || a == "--kmers-file") {
      std::cerr << "error: " << a << ": the command draws its own candidates; it writes a kmers file (-o), it reads none\n";
      return 2;
    } else if (a == "--gpus") {
      std::cerr << "error: --gpus: the walk runs on one device (--device D)\n";
      return 2;
    } else if (a == "-o" || a == "--output")
      output = val();
    else if (a == "-n") {
      count(n);
      have_n = true;
    } else if (a == "--seed")
      count(seed);
    else if (a == "--first")
      count(first);
    else if (a == "--max-candidates" || a == "-C")
      count(max_candidates);
    else if (a == "--round")
      count(round);
    else if (a == "--pam")
      pam = val();
    else if (a == "--kmer-length")
      count(L);
    else if (a == "-m" || a == "--mismatches")
      count(mismatches);
    else if (a == "-a" || a == "--alt-pam")
      alt_pams.push_back(val());
    else if (a == "--min-distance")
      count(min_distance);
    else if (a == "--prefix")
      id_prefix = val();
    else if (a == "--device")
      eo.device = atoi(val());
    else if (a == "--start")
      start = true;
    else if (a == "--allow-short")
      allow_short = true;
    else if (a == "--verbose")
      verbose = true;
    else if (!a.empty() && a[0] != '-' && eo.prefix.empty())
      eo.prefix = a;
    else
      return usage();
    if (bad) return 2;
  }
  if (eo.prefix.empty() || output.empty() || !have_n) return usage();
  auto refuse = [](const std::string &why) {
    std::cerr << "error: " << why << "\n";
    return 2;
  };
  if (L < 1 || L > 31) return refuse("--kmer-length: 1 to 31");
  if (pam.empty() || pam.size() > 8 || 2 * (size_t)L + 3 * pam.size() > 59) return refuse("--pam / --kmer-length: 2L + 3P <= 59, the fast path's key");
  if (mismatches > 7) return refuse("-m: 0 to 7");
  if (min_distance > 64) return refuse("--min-distance: 0 to 64");
  if (n < 1 || n > 16384ull) return refuse("-n: 1 to 16384 (the device keeps a round's controls in its local memory)");
  if (max_candidates < 1 || max_candidates - 1 > ~0ull - first) return refuse("--max-candidates: at least 1, and --first + --max-candidates at most 2^64");
  if (round > (1ull << 24)) return refuse("--round: at most 16777216");
  if (id_prefix.size() > 255) return refuse("--prefix: at most 255 bytes");
  std::string alts;
  for (const std::string &p : alt_pams) {
    if (p.size() != pam.size()) return refuse("-a " + p + ": an alt PAM has the PAM's length");
    alts += p;
  }
  if (alt_pams.size() > 31) return refuse("-a: at most 31");

  cli::genome_structure gs;
  std::string text;
  bool from_sdsl = false;
  if (!enumerate_cmd::load_genome(eo, gs, text, from_sdsl)) return 1;
  cli::index_set idx(1);
  if (!enumerate_cmd::build_indexes(eo, text, from_sdsl, idx)) return 1;
  gs_controls_rule rule;
  memset(&rule, 0, sizeof rule);
  rule.seed = seed;
  rule.first = first;
  rule.n = n;
  rule.max_candidates = max_candidates;
  rule.round = round;
  rule.L = (uint32_t)L;
  rule.n_alt = (uint32_t)alt_pams.size();
  rule.mismatches = (uint32_t)mismatches;
  rule.flags = start ? GS_FLAG_PAM_AT_START : 0u; /* the derived tables: the library's own rule (gs_controls_rule.flags) */
  rule.min_distance = (uint32_t)min_distance;
  rule.pam = pam.c_str();
  rule.alt_pams = alts.empty() ? nullptr : alts.data();
  rule.seq_rule = so.given ? &so.rule : nullptr;
  rule.id_prefix = id_prefix.c_str();

  const auto t0 = std::chrono::steady_clock::now();
  gs_kmers *km = nullptr;
  gs_controls_report rep;
  gs_status rc = gs_controls_generate(idx.ix[0], &rule, nullptr, &km, &rep);
  if (rc != GS_OK) {
    std::cerr << "error: controls: " << gs_status_string(rc) << "\n";
    return 1;
  }
  struct km_guard {
    gs_kmers *km;
    ~km_guard() { gs_kmers_free(km); }
  } guard{km};
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const bool is_short = rep.kept < n;
  if (is_short && !allow_short) {
    std::cerr << "error: kept " << rep.kept << " of -n " << n << " control(s) after --max-candidates " << max_candidates
              << " candidate(s): nothing written; try a smaller -m or a larger -C (--max-candidates), or --allow-short\n";
    return 1;
  }
  char *rows = nullptr;
  uint64_t len = 0;
  if ((rc = gs_controls_rows(km, &rows, &len)) != GS_OK) {
    std::cerr << "error: controls: " << gs_status_string(rc) << "\n";
    return 1;
  }
  /* -o is all or nothing: a temporary file, renamed when it is whole */
  const std::string tmp = output + ".tmp";
  FILE *out = fopen(tmp.c_str(), "wb");
  if (!out) {
    gs_free(rows);
    std::cerr << "error: cannot write " << tmp << "\n";
    return 1;
  }
  static const char header[] = "id,sequence,pam,chromosome,position,sense\n";
  bool ok = fwrite(header, 1, sizeof(header) - 1, out) == sizeof(header) - 1;
  ok = ok && fwrite(rows, 1, len, out) == len;
  gs_free(rows);
  ok = (fclose(out) == 0) && ok;
  if (!ok || rename(tmp.c_str(), output.c_str()) != 0) {
    std::cerr << "error: cannot write " << output << "\n";
    unlink(tmp.c_str());
    return 1;
  }
  std::cout << "Controls: kept " << rep.kept << " of " << rep.looked_at << " candidate(s) looked at; " << rep.gc << " failed --gc, " << rep.run
            << " --max-run, " << rep.motif << " a motif, " << rep.targeting << " targeting, " << rep.close << " close; " << rep.rounds
            << " round(s), " << secs << " s\n";
  if (is_short) std::cout << "Short of -n " << n << " after --max-candidates " << max_candidates << ": wrote what was found (--allow-short)\n";
  if (verbose)
    fprintf(stderr, "Stages: generate and rule %.3f ms, search %.3f ms, keep %.3f ms, distance %.3f ms, ids %.3f ms\n", rep.ms[0], rep.ms[1],
            rep.ms[2], rep.ms[3], rep.ms[4]);
  return 0;
}

}  // namespace controls_cmd

#endif
