/*
 * guidescan_main.cpp -- C++ host that keeps guidescan's `index` / `enumerate` command line
 * (src/guidescan.cxx:28-95, 316-358) and database output, and calls the MI355X path through the
 * C-ABI (include/guidescan_amd.h).  Control plane only: no search logic lives here.
 * Here: the dispatch, usage, `index`, `kmers` and `sam2bam`.  `enumerate` is enumerate_cmd.hpp over the ordered batch
 * pipeline of batch_pipeline.hpp, `decode` is decode_cmd.hpp, `controls` is controls_cmd.hpp, the readers and candidate options the commands share are
 * cli_common.hpp, the BAM records and BGZF blocks of the host are bam_writer.hpp.
 *
 *   guidescan index  [--index PREFIX] [--store-sa] [--sdsl] [--device D] [--fasta host|gpu] [--verbose] GENOME.fa
 *       writes PREFIX.gs (chromosome names/lengths, src/genomics/seq_io.cxx:112-122) and
 *       PREFIX.dna (= the reference's <fasta>.forward.dna: upper-cased concatenated sequence,
 *       seq_io.cxx:57-63).  The FM-index itself is built on the GPU when `enumerate` starts
 *       (~25 s at hg38 size, about what the reference needs to load its index files).
 *       --sdsl: builds the index on the GPU now and also writes PREFIX.forward / PREFIX.reverse, the reference's
 *       own index files (src/guidescan.cxx:168-175), byte for byte what its `index` command writes: the
 *       reference binary opens them, and so does `enumerate` here when PREFIX.dna is absent.
 *       --fasta gpu: GENOME.fa is parsed on the device (gs_fasta_parse_file under GS_FASTA_INDEX_RULES); PREFIX.gs comes from
 *       its record table and PREFIX.dna from the text copied back, byte for byte the files of --fasta host (the default).
 *       GENOME.fa must then be a regular file (the device buffer is sized from its length): a pipe, which --fasta host
 *       reads, is "cannot read".  --verbose: one line on stderr with the seconds of the FASTA read and of the two writes.
 *   guidescan kmers PREFIX -o KMERS.csv [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S] [--start]
 *       [--chromosomes a,b,...] [--device D]
 *       the kmers file of every candidate guide of the indexed genome, byte for byte what the reference's
 *       scripts/generate_kmers.py prints for the FASTA: PREFIX.gs cuts PREFIX.dna into chromosomes, each is scanned
 *       and its rows are encoded on the device (gs_kmers_generate, gs_kmers_csv).  --chromosomes: these only.
 *       --regions BED: only the candidates whose protospacer and PAM lie inside an interval of the file (columns:
 *       chromosome, start, end, 0-based half-open, and optionally the name of the line's group), one row per group a
 *       candidate lies in, the id "{prefix}{group}:{chr}:{position}:{sense}", ordered by group (first appearance in the
 *       file), chromosome, position, sense (gs_design_restrict, gs_design_rows).  --per-region and --min-specificity
 *       are refused here: this command has no index to search.
 *   guidescan enumerate PREFIX (-f KMERS.csv | --all-candidates) -o OUT [-m 3] [-a PAM ...] [--format csv|sam|bam]
 *       [--mode succinct|complete] [--max-off-targets N] [--start] [--device D] [--gpus N] [--batch-size B]
 *       --all-candidates [--pam ...] [--kmer-length ...] [--min-chr-length ...] [--prefix ...] [--chromosomes ...]:
 *       the guides are the candidates `guidescan kmers` would write with the same options, and OUT is the file
 *       `enumerate -f` writes for that kmers file.  With --encoder gpu on one device the candidates, their ids and
 *       senses stay in HBM from the scan to the text (gs_enumerate_text_device); any other batch is copied to the
 *       host and takes the route of a kmers file's batch.
 *       --all-candidates --regions BED [--per-region N] [--min-specificity S]: the guides are the candidates inside the
 *       file's intervals, as `kmers --regions` writes them.  --per-region N keeps the N most specific guides of each
 *       group, --min-specificity S those of specificity >= S; the specificity is the CSV column's with no cap on the
 *       off-targets, from a search with the command's own -m, -a and --start, and with -t a guide the threshold would
 *       drop is not eligible.  That score phase runs on the first device only, on the fast path (2L + 3P <= 59, alt
 *       PAMs of the PAM's length, no bulges).  A group left without a guide writes nothing; --verbose counts them.
 *       --annotate BED (CSV only, any guide source, both encoders, any number of devices): every row gets a last column,
 *       match_features, with the names of the BED file's groups that the printed off-target overlaps (its footprint
 *       [match_position - 1, match_position - 1 + L + P) clipped to the chromosome; gs_annot_scan.h), joined by ';', or NA.
 *       The file follows the rules of --regions.  --max-feature-hits K [--feature-distance D] (with --regions): the score
 *       phase also counts, per candidate, the off-targets within D mismatches (default: -m) that have a feature, the
 *       candidate's own site left out; more than K and the candidate is not eligible.
 *       --pairs PAIRS.csv --max-span X [--min-span Y] [--cut-offset C] [--pair-orientation any|pam-out|pam-in] (with
 *       --regions): pairs of guides inside each group whose cuts lie Y (default 1) to X bases apart on one chromosome
 *       (gs_design_pairs; the rule is csrc/gs_pairs_scan.h's).  The cut leaves C (default 3) protospacer bases between it
 *       and the PAM.  pam-out: the PAMs face away from each other; pam-in: towards each other.  Pairs are ranked by the
 *       smaller of the two specificities, then the larger; --per-region N then keeps the best N pairs of each group, and
 *       --min-specificity, -t and --max-feature-hits say which guides may pair.  PAIRS.csv is the table
 *       group,id_a,id_b,chromosome,cut_a,cut_b,span,specificity_a,specificity_b,pair_specificity; the guides of the kept
 *       pairs are the guides of the command, so OUT is their database in any format.  The score phase always runs.
 *       --gc MIN:MAX, --max-run R, --exclude-motif M1,..., --exclude-site M1,... (`kmers` too; no counterpart in the
 *       reference): candidates dropped for their own protospacer, on the scan's device and before anything is restricted
 *       or scored (gs_kmers_filter; the rule is csrc/gs_select_scan.h's).  One line reports kept of scanned and the three
 *       counts.  With -f they are refused: a given file is the user's own choice of guides.
 *       --min-spacing D [--cut-offset C] (with --regions --per-region N, N <= 1024; no counterpart in the reference): best
 *       first, a guide whose cut lies fewer than D bases from one already picked for the group on the same chromosome is
 *       passed over (gs_design_set_spacing; one wave walks a group).  Not with --pairs, which has its own span rule.
 *       With -t and neither selection option there is no score phase: the pipeline's own threshold pass drops the guides.
 *       -f KMERS.csv --kmers gpu: the kmers file is parsed on the first device (gs_kmers_parse_file, the rules of
 *       cli::read_kmers) and the command goes on as --all-candidates does from its scan: sequences, PAMs, ids and
 *       senses stay in HBM where the batch allows it.  Same output, messages and exit status as --kmers host (the
 *       default); a file whose rows differ in shape is read on the host after all.  --verbose: the reader's stage line.
 *       --format bam --bgzf gpu: batches that are all fast path leave the device as BGZF members (BAM records and
 *       deflate made in HBM: gs_enumerate_text with GS_TEXT_BAM | GS_TEXT_BGZF); any other batch, and every batch
 *       under the default --bgzf host, takes bam_writer.hpp's records and zlib.  Same records either way.
 *       --gpus N: one index per device (devices D .. D+N-1), one host thread per device pulling batches
 *       from a shared queue, output written in input order (src/guidescan.cxx:226-251 is the
 *       reference's fan-out over threads).  On every device the search of batch i+1 overlaps the text
 *       formatting of batch i.
 *   guidescan decode [--mode succinct|complete] [--device D] [-o OUT] [--batch-size RECORDS] [--bgzf host|gpu] [--fasta host|gpu]
 *       [--annotate BED [--features-only]] DATABASE GENOME.fa
 *       the CSV scripts/decode_database.py prints for a SAM/BAM database, decoded on the device (decode_cmd.hpp);
 *       stdout unless -o.  SEQ of at most 32 symbols.  The table streams, so only -o is all or nothing: stdout has
 *       the header and the earlier batches' rows when a later record fails.
 */
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unistd.h>

#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "guidescan_amd.h"
#include "bam_writer.hpp"
#include "cli_common.hpp"
#include "controls_cmd.hpp"
#include "decode_cmd.hpp"
#include "enumerate_cmd.hpp"
#include "fasta_names.hpp"

namespace {

using namespace cli;

std::string trim_ws(const std::string &s) { /* seq_io.cxx:47-55: both ends, isspace */
  size_t b = 0, e = s.size();
  while (b < e && isspace((unsigned char)s[b])) b++;
  while (e > b && isspace((unsigned char)s[e - 1])) e--;
  return s.substr(b, e - b);
}

/* seq_io.cxx:57-63 (sequence) and :74-110 (structure) in one pass */
bool parse_fasta(const std::string &path, std::string &text, genome_structure &gs) {
  std::ifstream in(path);
  if (!in) return false;
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line[0] == '>') {
      size_t nb, nl;
      fasta_names::index_name(line.data(), line.size(), &nb, &nl);
      gs.names.push_back(line.substr(nb, nl));
      gs.lengths.push_back(0);
      continue;
    }
    if (!gs.lengths.empty()) gs.lengths.back() += line.length(); /* untrimmed: seq_io.cxx:100-104 */
    std::string t = trim_ws(line);
    for (auto &c : t) c = (char)toupper((unsigned char)c);
    text += t;
  }
  return true;
}

/* --fasta gpu: the same two results from the device reader (GS_FASTA_INDEX_RULES); the text is the object's host copy */
struct fasta_holder {
  gs_fasta *fa = nullptr;
  ~fasta_holder() { gs_fasta_free(fa); }
};
gs_status parse_fasta_gpu(const std::string &path, int device, fasta_holder &h, genome_structure &gs, const char **text, size_t *text_len,
                          double *s_text_back) {
  gs_status rc = gs_fasta_parse_file(device, path.c_str(), GS_FASTA_INDEX_RULES, &h.fa);
  if (rc != GS_OK) return rc;
  uint64_t n = 0, tl = 0, nb = 0;
  gs_fasta_info(h.fa, &n, &tl, &nb);
  std::vector<uint64_t> line_len(n), name_off(n + 1);
  std::string names(nb, '\0');
  gs_fasta_records(h.fa, nullptr, nullptr, nullptr, nullptr, line_len.data(), name_off.data(), nb ? &names[0] : nullptr);
  for (uint64_t r = 0; r < n; r++) {
    gs.names.push_back(names.substr(name_off[r], name_off[r + 1] - name_off[r]));
    gs.lengths.push_back(line_len[r]);
  }
  const void *p = nullptr;
  const double t0 = decode_cmd::now_s();
  if ((rc = gs_fasta_text(h.fa, 0, &p)) != GS_OK) return rc;
  *s_text_back = decode_cmd::now_s() - t0;
  *text = (const char *)p;
  *text_len = (size_t)tl;
  return GS_OK;
}

bool write_gs(const std::string &path, const genome_structure &gs) {
  std::ofstream out(path);
  if (!out) return false;
  for (size_t i = 0; i < gs.names.size(); i++) out << gs.names[i] << "\n" << gs.lengths[i] << "\n";
  return (bool)out;
}

int usage() {
  std::cerr << "usage: guidescan index [--index PREFIX] [--store-sa] [--sdsl] [--device D] [--fasta host|gpu] [--verbose] GENOME.fa\n"
               "                 --fasta gpu: GENOME.fa is parsed on the device; the files are those of --fasta host.  GENOME.fa\n"
               "                 must then be a regular file (no pipe).\n"
               "       guidescan kmers PREFIX -o KMERS [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S]\n"
               "                 [--start] [--chromosomes a,b,...] [--device D] [--regions BED]\n"
               "                 --regions BED: only candidates inside the file's intervals (chromosome, start, end, [group]),\n"
               "                 one row per group, ids {prefix}{group}:{chr}:{position}:{sense}, ordered by group\n"
               "                 [--gc MIN:MAX] [--max-run R] [--exclude-motif M1,M2,...] [--exclude-site M1,M2,...]\n"
               "                 sequence rules on the protospacer as the sequence column prints it (the PAM is not looked at):\n"
               "                 G+C percentage within MIN:MAX, no letter more than R times in a row, none of the IUPAC motifs\n"
               "                 (at most 16 of 1 to 32 letters); --exclude-site also excludes each reverse complement\n"
               "       guidescan enumerate PREFIX (-f KMERS | --all-candidates) -o OUT [-m N] [-a PAM]... [--format csv|sam|bam]\n"
               "                 [--mode succinct|complete] [--max-off-targets N] [--start]\n"
               "                 [--rna-bulges N] [--dna-bulges N] [--bulge-form walk|seeded] [-t THRESHOLD] [-n FORMAT_THREADS]\n"
               "                 [--device D] [--gpus N] [--batch-size B] [--encoder host|gpu] [--bgzf host|gpu]\n"
               "                 [--kmers host|gpu] [--verbose]\n"
               "                 --kmers gpu (with -f): the kmers file is parsed on the first device; same output and messages\n"
               "                 with --all-candidates: [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S]\n"
               "                 [--chromosomes a,b,...] [--regions BED [--per-region N] [--min-specificity S]]\n"
               "                 --regions: the guides are the candidates inside the BED file's intervals, one per group of\n"
               "                 intervals they lie in; --per-region N: the N most specific of each group; --min-specificity S:\n"
               "                 those of specificity >= S.  That score phase uses the first device only.\n"
               "                 [--pairs PAIRS.csv --max-span X [--min-span Y] [--cut-offset C] [--pair-orientation any|pam-out|pam-in]]\n"
               "                 --pairs (with --regions): pairs of guides of one group and chromosome whose cuts lie Y (default 1)\n"
               "                 to X bases apart, the cut C (default 3) protospacer bases from the PAM; pam-out: the PAMs face\n"
               "                 away from each other.  Ranked by the smaller specificity of the two; --per-region N keeps the best\n"
               "                 N pairs of each group.  PAIRS.csv is their table, OUT the database of their guides.\n"
               "                 [--gc MIN:MAX] [--max-run R] [--exclude-motif M1,M2,...] [--exclude-site M1,M2,...]\n"
               "                 (with --all-candidates) the sequence rules of `kmers`: a candidate they drop is never scored\n"
               "                 [--min-spacing D [--cut-offset C]] (with --regions --per-region N, N <= 1024, not with --pairs):\n"
               "                 best first, a guide is skipped when its cut lies fewer than D bases from a guide already\n"
               "                 picked for the group on the same chromosome\n"
               "                 [--annotate BED [--max-feature-hits K [--feature-distance D]]]\n"
               "                 --annotate (CSV only): a match_features column, the groups of the BED file that each printed\n"
               "                 off-target overlaps, joined by ';', or NA.  --max-feature-hits K (with --regions): a candidate\n"
               "                 with more than K off-targets within D mismatches (default: -m) inside a feature is not eligible\n"
               "       guidescan controls PREFIX -o KMERS -n N [--seed S] [--first I] [--pam NGG] [--kmer-length 20] [--start]\n"
               "                 [-m 3] [-a PAM]... [--gc MIN:MAX] [--max-run R] [--exclude-motif M1,...] [--exclude-site M1,...]\n"
               "                 [--min-distance H] [--max-candidates C] [--allow-short] [--prefix control_] [--device D] [--verbose]\n"
               "                 non-targeting controls as a kmers file for enumerate -f: candidate I of seed S is a fixed random\n"
               "                 protospacer; it is dropped by the sequence rules, by any site within -m mismatches (the -a PAMs\n"
               "                 included), or by fewer than H (default 1) mismatches to a control already kept; the first N that\n"
               "                 remain are written, ids {prefix}{I}.  Fewer than N after C (default 2^32) candidates: exit 1 and no\n"
               "                 file, unless --allow-short.  A smaller N (at most 16384) gives the head of the same file.\n"
               "       guidescan decode [--mode succinct|complete] [--device D] [-o OUT] [--batch-size RECORDS] [--verbose]\n"
               "                 [--bgzf host|gpu] [--fasta host|gpu] [--annotate BED [--features-only]] DATABASE GENOME.fa\n"
               "                 --annotate: the features of a BED file, read against the database's @SQ lines, in the pass that\n"
               "                 decodes: --mode complete gains the column match_features (the groups each off-target overlaps,\n"
               "                 joined by ';', or NA), --mode succinct the columns distance_k_feature_matches.  --features-only\n"
               "                 (--mode complete): only the rows with a feature; match_number as in the full table.\n"
               "                 --bgzf gpu (a BAM database only): the file is inflated and split into records on the device.\n"
               "                 --fasta gpu: GENOME.fa is parsed on the device and its text stays there; same table and messages,\n"
               "                 but GENOME.fa must be a regular file (a pipe, which --fasta host reads, is \"cannot read\").\n"
               "                 a stored guide (SEQ) may have at most 32 symbols.  The table streams: without -o the header\n"
               "                 and the rows of earlier batches are on stdout already when a later record fails (exit\n"
               "                 status 1); with -o a failure leaves no file.\n";
  return 2;
}

int do_index(int argc, char **argv) {
  std::string fasta, prefix, fasta_on = "host";
  bool store_sa = false, sdsl = false, verbose = false;
  int device = 0;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--verbose")
      verbose = true;
    else if (a == "--index" && i + 1 < argc)
      prefix = argv[++i];
    else if (a == "--store-sa")
      store_sa = true;
    else if (a == "--sdsl")
      sdsl = true;
    else if (a == "--device" && i + 1 < argc)
      device = atoi(argv[++i]);
    else if (a == "--fasta" && i + 1 < argc)
      fasta_on = argv[++i];
    else if (!a.empty() && a[0] != '-')
      fasta = a;
    else
      return usage();
  }
  if (fasta.empty() || (fasta_on != "host" && fasta_on != "gpu")) return usage();
  if (prefix.empty()) prefix = fasta + ".index"; /* src/guidescan.cxx:112-117 */
  std::string host_text;
  genome_structure gs;
  fasta_holder parsed; /* --fasta gpu: owns the text copied back */
  const char *text_p = nullptr;
  size_t text_n = 0;
  double s_text_back = 0;
  const double t_start = decode_cmd::now_s();
  if (fasta_on == "gpu") {
    const gs_status rc = parse_fasta_gpu(fasta, device, parsed, gs, &text_p, &text_n, &s_text_back);
    if (rc != GS_OK) {
      std::cerr << "error: " << (rc == GS_ERR_IO ? "cannot read " + fasta : std::string(gs_status_string(rc))) << "\n";
      return 1;
    }
  } else {
    if (!parse_fasta(fasta, host_text, gs)) {
      std::cerr << "error: cannot read " << fasta << "\n";
      return 1;
    }
    text_p = host_text.data();
    text_n = host_text.size();
  }
  struct text_view {
    const char *p;
    size_t n;
    const char *data() const { return p; }
    size_t size() const { return n; }
  } const text{text_p, text_n};
  const double t_read = decode_cmd::now_s();
  if (!write_gs(prefix + ".gs", gs)) {
    std::cerr << "error: cannot write " << prefix << ".gs\n";
    return 1;
  }
  std::ofstream dna(prefix + ".dna", std::ios::binary);
  dna.write(text.data(), (std::streamsize)text.size());
  dna.close();
  if (!dna) {
    std::cerr << "error: cannot write " << prefix << ".dna\n";
    return 1;
  }
  std::cout << "Wrote " << prefix << ".gs and " << prefix << ".dna (" << text.size() << " bases, "
            << gs.names.size() << " sequences)\n";
  if (verbose) { /* the two stages of this command; what the wall clock shows beyond them is the process's start and end */
    fprintf(stderr, "Stages: FASTA read %.3f s, .gs and .dna writes %.3f s", t_read - t_start, decode_cmd::now_s() - t_read);
    if (fasta_on == "gpu") {
      double ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      gs_debug_fasta_ms(parsed.fa, ms);
      fprintf(stderr, "; fasta gpu: file reads %.3f s, waits for the uploads %.3f s, device stage %.3f s (its five passes %.3f s), titles and names "
                      "%.3f s, text back %.3f s",
              1e-3 * ms[0], 1e-3 * ms[1], 1e-3 * ms[2], 1e-3 * (ms[4] + ms[5] + ms[6] + ms[7] + ms[8]), 1e-3 * ms[3], s_text_back);
    }
    fprintf(stderr, "\n");
  }
  if (store_sa || sdsl) {
    /* the part of the index worth storing: both suffix arrays (built on the GPU now), so that
     * `enumerate` skips the sort; 8 bytes per base on disk (--store-sa) - or the reference's own
     * index files, about half a byte per base and strand (--sdsl) */
    index_set idx(1);
    gs_index *&ix = idx.ix[0];
    gs_status rc = gs_index_build((const uint8_t *)text.data(), text.size(), device, &ix);
    if (rc == GS_OK && store_sa) rc = gs_index_save_sa(ix, (const uint8_t *)text.data(), text.size(), (prefix + ".sa").c_str());
    if (rc == GS_OK && sdsl) rc = gs_index_save_sdsl(ix, (const uint8_t *)text.data(), text.size(), prefix.c_str());
    if (rc != GS_OK) {
      std::cerr << "error: " << gs_status_string(rc) << "\n";
      return 1;
    }
    if (store_sa) std::cout << "Wrote " << prefix << ".sa\n";
    if (sdsl) std::cout << "Wrote " << prefix << ".forward and " << prefix << ".reverse\n";
  }
  return 0;
}

int do_kmers(int argc, char **argv) {
  std::string prefix, output, regions;
  candidate_opts co;
  cli::seq_rule_opts so;
  uint64_t rule_counts[4] = {0, 0, 0, 0};
  int device = 0;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    bool bad = false;
    if (candidate_option(a, i, argc, argv, co, bad) || cli::seq_rule_option(a, i, argc, argv, so, bad)) {
      if (bad) return 2;
    } else if ((a == "-o" || a == "--output") && i + 1 < argc)
      output = argv[++i];
    else if (a == "--regions" && i + 1 < argc)
      regions = argv[++i];
    else if (a == "--per-region" || a == "--min-specificity" || a == "--pairs" || a == "--min-spacing") {
      std::cerr << "error: " << a << " ranks guides by specificity, which takes the index: use guidescan enumerate --all-candidates --regions\n";
      return 2;
    }
    else if (a == "--start")
      co.start = true;
    else if (a == "--device" && i + 1 < argc)
      device = atoi(argv[++i]);
    else if (!a.empty() && a[0] != '-' && prefix.empty())
      prefix = a;
    else
      return usage();
  }
  if (prefix.empty() || output.empty() || co.k < 1) return usage();
  genome_structure gs;
  std::string err, text;
  if (!read_gs(prefix + ".gs", gs, err)) {
    std::cerr << "error: " << err << "\n";
    return 1;
  }
  if (!read_file(prefix + ".dna", text)) {
    std::cerr << "error: cannot read " << prefix << ".dna (the genome text `guidescan index` writes)\n";
    return 1;
  }
  std::vector<size_t> sel;
  std::vector<uint64_t> begin;
  if (!select_chromosomes(prefix, gs, text.size(), co, sel, begin, err)) {
    std::cerr << "error: " << err << "\n";
    return 1;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const std::string tmp = output + ".tmp";
  FILE *out = fopen(tmp.c_str(), "wb");
  if (!out) {
    std::cerr << "error: cannot write " << tmp << "\n";
    return 1;
  }
  static const char header[] = "id,sequence,pam,chromosome,position,sense\n";
  bool ok = fwrite(header, 1, sizeof(header) - 1, out) == sizeof(header) - 1;
  uint64_t total = 0;
  double s_scan = 0, s_rows = 0, s_write = 0;
  gs_status rc = GS_OK;
  enumerate_cmd::candidate_set rset; /* --regions: owns the file's tables */
  std::vector<gs_design *> dparts;
  if (!regions.empty() && !enumerate_cmd::read_regions(regions, gs, co.prefix, rset)) {
    fclose(out);
    unlink(tmp.c_str());
    return 1;
  }
  for (size_t c : sel) {
    auto t1 = std::chrono::steady_clock::now();
    gs_kmers *km = nullptr;
    rc = gs_kmers_generate(device, (const uint8_t *)text.data() + begin[c], gs.lengths[c], 0, co.pam.c_str(), (uint32_t)co.k,
                           co.start ? GS_FLAG_PAM_AT_START : 0u, nullptr, &km);
    if (rc == GS_OK && (rc = cli::apply_seq_rule(so, &km, rule_counts)) != GS_OK) gs_kmers_free(km);
    if (rc != GS_OK) break;
    auto t2 = std::chrono::steady_clock::now();
    s_scan += std::chrono::duration<double>(t2 - t1).count();
    if (rset.regions) { /* the rows come once every chromosome is restricted: they are ordered by group */
      gs_design *dp = nullptr;
      rc = gs_design_restrict(rset.regions, (uint32_t)c, km, nullptr, &dp);
      gs_kmers_free(km);
      if (rc != GS_OK) break;
      dparts.push_back(dp);
      continue;
    }
    uint64_t n = 0, len = 0;
    char *rows = nullptr;
    gs_kmers_get(km, 1, &n, nullptr, nullptr, nullptr, nullptr);
    rc = gs_kmers_csv(km, co.prefix.c_str(), gs.names[c].c_str(), &rows, &len);
    gs_kmers_free(km);
    if (rc != GS_OK) break;
    auto t3 = std::chrono::steady_clock::now();
    s_rows += std::chrono::duration<double>(t3 - t2).count();
    ok = ok && fwrite(rows, 1, len, out) == len;
    gs_free(rows);
    s_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - t3).count();
    total += n;
  }
  if (rset.regions && rc == GS_OK) {
    auto t2 = std::chrono::steady_clock::now();
    uint64_t len = 0, last[4] = {0, 0, 0, 0};
    char *rows = nullptr;
    if (dparts.empty()) {
      std::cerr << "error: --regions: no chromosome selected\n";
      rc = GS_ERR_ARG;
    } else {
      rc = gs_design_concat(dparts.data(), (uint32_t)dparts.size(), &rset.design);
    }
    if (rc == GS_OK) rc = gs_design_rows(rset.design, co.prefix.c_str(), 0, -1.0f, nullptr, &rows, &len);
    if (rc == GS_OK) {
      gs_design_last_select(rset.design, last);
      total = last[1];
      auto t3 = std::chrono::steady_clock::now();
      s_rows += std::chrono::duration<double>(t3 - t2).count();
      ok = ok && fwrite(rows, 1, len, out) == len;
      gs_free(rows);
      s_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - t3).count();
    }
  }
  for (gs_design *dp : dparts) gs_design_free(dp);
  ok = (fclose(out) == 0) && ok;
  if (rc != GS_OK || !ok) {
    if (rc != GS_OK)
      std::cerr << "error: candidate scan (--pam " << co.pam << ", --kmer-length " << co.k << "): " << gs_status_string(rc) << "\n";
    else
      std::cerr << "error: short write to " << tmp << "\n";
    unlink(tmp.c_str());
    return 1;
  }
  if (rename(tmp.c_str(), output.c_str()) != 0) {
    std::cerr << "error: cannot rename " << tmp << " to " << output << "\n";
    unlink(tmp.c_str());
    return 1;
  }
  std::cout << "Wrote " << total << " candidate(s) of " << sel.size() << " chromosome(s) to " << output << " in "
            << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s\n";
  if (so.given) std::cout << cli::seq_rule_line(rule_counts);
  std::cout << "Stages: scan " << s_scan << " s, rows " << s_rows << " s, file writes " << s_write << " s\n";
  return 0;
}

/* guidescan sam2bam IN.sam OUT.bam: the encoder of `enumerate --format bam` on a SAM file (what the reference's
 * manual does with `samtools view -b`); the references come from the file's @SQ lines */
int do_sam2bam(int argc, char **argv) {
  if (argc != 2) return usage();
  std::ifstream in(argv[0], std::ios::binary);
  if (!in) {
    std::cerr << "error: cannot read " << argv[0] << "\n";
    return 1;
  }
  std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::string head;
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
  std::map<std::string, int32_t> refid;
  size_t at = 0;
  while (at < text.size() && text[at] == '@') {
    size_t e = text.find('\n', at);
    e = e == std::string::npos ? text.size() : e + 1;
    const std::string line = text.substr(at, e - at);
    if (line.compare(0, 3, "@SQ") == 0) {
      std::string sn;
      uint64_t ln = 0;
      std::stringstream ss(line);
      std::string f;
      while (std::getline(ss, f, '\t')) {
        while (!f.empty() && (f.back() == '\n' || f.back() == '\r')) f.pop_back();
        if (f.compare(0, 3, "SN:") == 0) sn = f.substr(3);
        if (f.compare(0, 3, "LN:") == 0) ln = strtoull(f.c_str() + 3, nullptr, 10);
      }
      refid[sn] = (int32_t)names.size();
      names.push_back(sn);
      lengths.push_back(ln);
    }
    head += line;
    at = e;
  }
  std::string out, raw;
  if (!bam::bgzf_append(bam::header(head, names, lengths), out) || !bam::records(text.data() + at, text.size() - at, refid, raw) ||
      !bam::bgzf_append(raw, out)) {
    std::cerr << "error: malformed SAM line in " << argv[0] << "\n";
    return 1;
  }
  bam::bgzf_eof(out);
  std::ofstream o(argv[1], std::ios::binary);
  o.write(out.data(), (std::streamsize)out.size());
  return o.good() ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && (!strcmp(argv[1], "--version") || !strcmp(argv[1], "-v"))) {
    std::cout << "2.0.0 (" << gs_version() << ")\n";
    return 0;
  }
  if (argc < 2) return usage();
  if (!strcmp(argv[1], "sam2bam")) return do_sam2bam(argc - 2, argv + 2);
  if (!strcmp(argv[1], "index")) return do_index(argc - 2, argv + 2);
  if (!strcmp(argv[1], "kmers")) return do_kmers(argc - 2, argv + 2);
  if (!strcmp(argv[1], "enumerate")) return enumerate_cmd::run(argc - 2, argv + 2, usage);
  if (!strcmp(argv[1], "controls")) return controls_cmd::run(argc - 2, argv + 2, usage);
  if (!strcmp(argv[1], "decode")) {
    const int rc = decode_cmd::run(argc - 2, argv + 2);
    return rc == 2 ? usage() : rc;
  }
  return usage();
}