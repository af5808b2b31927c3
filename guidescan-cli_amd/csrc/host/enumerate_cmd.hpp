/*
 * enumerate_cmd.hpp -- `guidescan enumerate PREFIX (-f KMERS.csv | --all-candidates) -o OUT ...`: the off-target database
 * of a set of guides (src/guidescan.cxx:181-258), searched, scored and - where the batch allows it - encoded on the device
 * through the C-ABI.  Control plane only.  run() is a sequence of stages: options, genome text, guides (a kmers file or
 * the candidate scan; a kmers file under --kmers gpu is parsed on the device and then treated as a scan's candidates),
 * one index per device, the job, the output file, the batches, the pipeline, the report.
 *
 * A batch takes one of three routes to its text: the device's text or BGZF members (--encoder gpu, --bgzf gpu: a batch
 * that is all fast path, from device pointers under --all-candidates on one device, else from host pointers), the fast
 * path's hit lists with the general path for the guides it flags, or the general path for every guide (bulges, alt PAMs
 * of another length, match sequences beyond the fast path's key).  The pipeline that overlaps the search of batch i+1
 * with the formatting of batch i and writes in input order is batch_pipeline.hpp.
 */
#ifndef GS_ENUMERATE_CMD_HPP
#define GS_ENUMERATE_CMD_HPP

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "guidescan_amd.h"
#include "bam_writer.hpp"
#include "batch_pipeline.hpp"
#include "cli_common.hpp"

namespace enumerate_cmd {

using cli::genome_structure;
using cli::kmer_row;
using cli::read_bed;

/* --bulge-form's default.  Measured at hg38 size (profiles/bulge_seeded.json): 4,096 guides at -m 1 with one
 * bulge of each kind take the walk 0.22 s and the seeded form 1.10 s at best, so the walk stays the default */
static const char *const BULGE_FORM_DEFAULT = "walk";

struct options {
  std::string prefix, kmers_file, output, format = "csv", mode = "complete";
  /* GS_ENCODER: the default of --encoder (the end-to-end rows of a benchmark run either way with one command line) */
  std::string encoder = getenv("GS_ENCODER") ? getenv("GS_ENCODER") : "host";
  std::string bgzf = "host";
  std::vector<std::string> alt_pams;
  /* which form of the bulge-aware search serves a job with a bulge budget (gs_enumerate_general): the same lines either way */
  std::string bulge_form = BULGE_FORM_DEFAULT;
  long long mismatches = 3, max_off = -1, threshold = -1, rna = 0, dna = 0;
  int device = 0, gpus = 1;
  size_t batch_size = 0;
  unsigned fmt_threads = 0;
  bool all_candidates = false, verbose = false;
  std::string kmers; /* --kmers host|gpu: who reads the kmers file; empty: not given (host) */
  cli::candidate_opts co; /* co.start is --start, with or without --all-candidates */
  /* --regions BED [--per-region N] [--min-specificity S] (with --all-candidates): the candidates inside the file's
   * intervals, one record per group of intervals, the best N of each group (gs_design_*) */
  std::string regions;
  long long per_region = 0; /* 0: not given */
  float min_spec = -1.0f;   /* < 0: not given */
  /* --annotate BED: the CSV's match_features column, the groups of the file that each printed off-target touches
   * (gs_annot_*); --max-feature-hits K [--feature-distance D] (with --regions): a candidate with more than K off-targets
   * within D mismatches (default: -m) inside a feature is not eligible */
  std::string annotate;
  long long max_feature_hits = -1, feature_distance = -1; /* -1: not given */
  /* --pairs FILE --max-span X [--min-span Y] [--cut-offset C] [--pair-orientation any|pam-out|pam-in] (with --regions): the
   * guides are those of the best --per-region pairs of each group (gs_design_pairs), and FILE is the table of the pairs */
  std::string pairs, pair_orientation;
  long long max_span = -1, min_span = -1, cut_offset = -1; /* -1: not given */
  /* --gc, --max-run, --exclude-motif, --exclude-site (with --all-candidates): candidates dropped for their own sequence,
   * before they are restricted or scored (gs_kmers_filter); --min-spacing D [--cut-offset C] (with --regions --per-region N):
   * the picks of a group lie D bases apart or more (gs_design_set_spacing) */
  cli::seq_rule_opts seq;
  long long min_spacing = -1; /* -1: not given */
  bool selects() const { return per_region > 0 || min_spec >= 0.0f || max_feature_hits >= 0 || !pairs.empty(); }
};

/* the command line into `o`, validated.  0: go on; otherwise the exit status */
inline int parse_options(int argc, char **argv, int (*usage)(), options &o) {
  bool candidate_opts_given = false;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    bool bad = false;
    if (cli::candidate_option(a, i, argc, argv, o.co, bad)) {
      if (bad) return 2;
      candidate_opts_given = true;
      continue;
    }
    if (cli::seq_rule_option(a, i, argc, argv, o.seq, bad)) {
      if (bad) return 2;
      continue;
    }
    auto need = [&](const char *what) -> const char * {
      if (i + 1 >= argc) {
        std::cerr << "error: " << what << " needs a value\n";
        exit(2);
      }
      return argv[++i];
    };
    if (a == "-f" || a == "--kmers-file") o.kmers_file = need("-f");
    else if (a == "-o" || a == "--output") o.output = need("-o");
    else if (a == "-m" || a == "--mismatches") o.mismatches = atoll(need("-m"));
    else if (a == "-a" || a == "--alt-pam") o.alt_pams.push_back(need("-a"));
    else if (a == "-n" || a == "--threads") o.fmt_threads = (unsigned)atoi(need("-n")); /* text formatting threads; the search runs on the GPU */
    else if (a == "-t" || a == "--threshold") o.threshold = atoll(need("-t"));
    else if (a == "--rna-bulges") o.rna = atoll(need("--rna-bulges"));
    else if (a == "--dna-bulges") o.dna = atoll(need("--dna-bulges"));
    else if (a == "--bulge-form") o.bulge_form = need("--bulge-form");
    else if (a == "--max-off-targets") o.max_off = atoll(need("--max-off-targets"));
    else if (a == "--format") o.format = need("--format");
    else if (a == "--mode") o.mode = need("--mode");
    else if (a == "--start") o.co.start = true;
    else if (a == "--all-candidates") o.all_candidates = true;
    else if (a == "--device") o.device = atoi(need("--device"));
    else if (a == "--gpus") o.gpus = atoi(need("--gpus"));
    else if (a == "--batch-size") o.batch_size = (size_t)atoll(need("--batch-size"));
    else if (a == "--encoder") o.encoder = need("--encoder");
    else if (a == "--bgzf") o.bgzf = need("--bgzf");
    else if (a == "--kmers") o.kmers = need("--kmers");
    else if (a == "--verbose") o.verbose = true;
    else if (a == "--regions") o.regions = need("--regions");
    else if (a == "--per-region") {
      const char *v = need("--per-region");
      char *end = nullptr;
      o.per_region = strtoll(v, &end, 10);
      if (end == v || *end || o.per_region < 1) {
        std::cerr << "error: --per-region " << v << ": a number of guides per group, at least 1\n";
        return 2;
      }
    } else if (a == "--min-specificity") {
      const char *v = need("--min-specificity");
      char *end = nullptr;
      o.min_spec = strtof(v, &end);
      if (end == v || *end || !(o.min_spec >= 0.0f && o.min_spec <= 1.0f)) {
        std::cerr << "error: --min-specificity " << v << ": a specificity, 0 to 1\n";
        return 2;
      }
    }
    else if (a == "--annotate") o.annotate = need("--annotate");
    else if (a == "--max-feature-hits" || a == "--feature-distance") {
      const char *v = need(a.c_str());
      char *end = nullptr;
      const long long k = strtoll(v, &end, 10);
      if (end == v || *end || k < 0 || k > 0xFFFFFFFFll) {
        std::cerr << "error: " << a << " " << v << ": a number, 0 or more\n";
        return 2;
      }
      (a == "--max-feature-hits" ? o.max_feature_hits : o.feature_distance) = k;
    }
    else if (a == "--pairs") o.pairs = need("--pairs");
    else if (a == "--max-span" || a == "--min-span" || a == "--cut-offset" || a == "--min-spacing") {
      const char *v = need(a.c_str());
      char *end = nullptr;
      const long long k = v[0] >= '0' && v[0] <= '9' && strlen(v) <= 18 ? strtoll(v, &end, 10) : -1;
      if (k < 0 || !end || *end || (a == "--min-spacing" && k > 0xFFFFFFFFll)) {
        std::cerr << "error: " << a << " " << v << ": a number, 0 or more\n";
        return 2;
      }
      (a == "--max-span" ? o.max_span : a == "--min-span" ? o.min_span : a == "--cut-offset" ? o.cut_offset : o.min_spacing) = k;
    } else if (a == "--pair-orientation") {
      o.pair_orientation = need("--pair-orientation");
      if (o.pair_orientation != "any" && o.pair_orientation != "pam-out" && o.pair_orientation != "pam-in") {
        std::cerr << "error: --pair-orientation " << o.pair_orientation << ": any, pam-out or pam-in\n";
        return 2;
      }
    }
    else if (!a.empty() && a[0] != '-' && o.prefix.empty()) o.prefix = a;
    else return usage();
  }
  if (o.pairs.empty() && (o.max_span >= 0 || o.min_span >= 0 || (o.cut_offset >= 0 && o.min_spacing < 0) || !o.pair_orientation.empty())) {
    std::cerr << "error: --max-span, --min-span, --cut-offset and --pair-orientation describe the pairs of --pairs FILE\n";
    return 2;
  }
  if (o.min_spacing >= 0 || o.seq.given) { /* refused with one line each, before the genome is read */
    const char *why = nullptr;
    if (o.seq.given && !o.kmers_file.empty())
      why = "--gc, --max-run, --exclude-motif and --exclude-site drop candidates of the scan of --all-candidates; with -f the kmers file is "
            "the user's own choice of guides";
    else if (o.seq.given && !o.all_candidates)
      why = "--gc, --max-run, --exclude-motif and --exclude-site drop candidates of the scan of --all-candidates";
    else if (o.min_spacing >= 0 && !o.pairs.empty()) why = "--min-spacing spaces single guides; the pairs of --pairs have their own span rule";
    else if (o.min_spacing >= 0 && (o.regions.empty() || !o.all_candidates))
      why = "--min-spacing spaces the picks within the groups of --all-candidates --regions BED";
    else if (o.min_spacing >= 0 && (o.per_region < 1 || o.per_region > 1024))
      why = "--min-spacing needs --per-region N with N from 1 to 1024: the picks of a group are spaced one after the other";
    else if (o.min_spacing >= 0 && o.cut_offset > (long long)o.co.k) why = "--cut-offset lies beyond the k-mer length";
    if (why) {
      std::cerr << "error: " << why << "\n";
      return 2;
    }
  }
  if (!o.pairs.empty()) { /* refused with one line each, before the genome is read */
    const char *why = nullptr;
    if (o.regions.empty() || !o.all_candidates) why = "--pairs pairs the guides within the groups of --all-candidates --regions BED";
    else if (o.max_span < 0) why = "--pairs needs --max-span X, the largest distance between the two cuts";
    else if (o.min_span > o.max_span) why = "--min-span is larger than --max-span";
    else if (o.cut_offset > (long long)o.co.k) why = "--cut-offset lies beyond the k-mer length";
    else if (o.rna > 0 || o.dna > 0 || o.mismatches > 7 || o.threshold > 7)
      why = "--pairs scores on the fast path: no bulges, at most 7 mismatches";
    else if (o.co.k > 31 || 2 * o.co.k + 3 * (long long)o.co.pam.size() > 59)
      why = "--pairs scores on the fast path: 2L + 3P > 59, the shape is outside its key";
    for (auto &a : o.alt_pams)
      if (!why && a.size() != o.co.pam.size()) why = "--pairs scores on the fast path: an alt PAM is not of the PAM's length";
    if (why) {
      std::cerr << "error: " << why << "\n";
      return 2;
    }
  }
  if (!o.prefix.empty() && !o.output.empty() && o.kmers_file.empty() == !o.all_candidates) {
    std::cerr << (o.all_candidates ? "error: -f KMERS and --all-candidates exclude each other: the guides come from the file or from the scan\n"
                                   : "error: no guides: give -f KMERS or --all-candidates\n");
    return usage();
  }
  if (o.prefix.empty() || o.output.empty()) return usage();
  if (!o.kmers.empty() && o.kmers != "host" && o.kmers != "gpu") return usage();
  if (!o.kmers.empty() && o.kmers_file.empty()) {
    std::cerr << "error: --kmers says who reads the kmers file of -f\n";
    return usage();
  }
  if (o.all_candidates && o.co.k < 1) return usage();
  if (!o.all_candidates && candidate_opts_given) {
    std::cerr << "error: --pam, --kmer-length, --min-chr-length, --prefix and --chromosomes describe the scan of --all-candidates; with -f the kmers file says what the guides are\n";
    return usage();
  }
  if (!o.regions.empty() && !o.all_candidates) {
    std::cerr << "error: --regions restricts the scan of --all-candidates; with -f the kmers file says what the guides are\n";
    return usage();
  }
  if ((o.per_region > 0 || o.min_spec >= 0.0f) && o.regions.empty()) {
    std::cerr << "error: --per-region and --min-specificity select within the groups of --regions\n";
    return usage();
  }
  if (o.max_feature_hits >= 0 && (o.regions.empty() || o.annotate.empty())) {
    std::cerr << "error: --max-feature-hits selects among the candidates of --regions by the features of --annotate: give both\n";
    return usage();
  }
  if (o.feature_distance >= 0 && o.max_feature_hits < 0) {
    std::cerr << "error: --feature-distance is the distance --max-feature-hits counts within\n";
    return usage();
  }
  if (!o.annotate.empty() && o.format != "csv") {
    std::cerr << "error: --annotate adds a column to the CSV database; --format " << o.format << " has none\n";
    return 2;
  }
  if ((o.format != "csv" && o.format != "sam" && o.format != "bam") || (o.mode != "succinct" && o.mode != "complete")) return usage();
  if (o.gpus < 1 || o.mismatches < 0 || o.rna < 0 || o.dna < 0) return usage();
  if (o.encoder != "host" && o.encoder != "gpu") return usage();
  if ((o.bgzf != "host" && o.bgzf != "gpu") || (o.bgzf == "gpu" && o.format != "bam")) return usage();
  if (o.bulge_form != "walk" && o.bulge_form != "seeded") return usage();
  /* alt PAMs are searched whatever their length, next to each guide's own PAM (process.hpp:51-56): a batch
   * whose PAM length they all share goes through the fast path, any other through the general path */
  for (auto &a : o.alt_pams)
    if (a.empty() || a.size() > 8) {
      std::cerr << "error: alt PAM " << a << ": 1 to 8 symbols\n";
      return 1;
    }
  if (!o.batch_size) {
    /* The hit lists of a batch live in HBM and on the host until it is written: ~13 hits per guide at <= 3 mismatches,
     * ~1.4e3 at 5, ~1.1e4 at 6 on a human-sized genome, so deeper searches take smaller batches.
     * At <= 3 mismatches a batch of 2^17 guides: the search is 3 ms of device time per batch at hg38 size (a million guides in
     * one batch: 17.5 ms, in eight: 24), but its 1.1 GB of text took 0.22 s to format and 0.19 s to write BEHIND the search when
     * the set was one batch - three stages that overlap only from batch to batch (bench.py's e2e_cli row: 0.60 -> 0.4 s). */
    const long long m = o.mismatches;
    o.batch_size = m <= 3 ? (1u << 17) : m == 4 ? (1u << 18) : m == 5 ? (1u << 16) : (1u << 13);
  }
  return 0;
}

/* One batch of kmers with equal (L, P), as it moves through the pipeline: a device thread searches
 * and scores it, a formatting task turns the hit lists into text, the main thread writes the text
 * in input order. */
struct text_part { /* the lines of one contiguous range of a batch */
  char *p = nullptr; /* a buffer of the library (gs_free), or */
  size_t n = 0;
  std::string s;     /* lines gathered guide by guide */
};
struct batch {
  size_t lo = 0, hi = 0;
  uint32_t L = 0, P = 0;
  const kmer_row *rows = nullptr; /* hi - lo rows: the kmers file's, or `own` */
  std::vector<kmer_row> own;      /* --all-candidates: the batch's candidates, once they had to come to the host */
  std::vector<text_part> parts;
  std::string seqs, pams;
  gs_result *res = nullptr;
  gs_result_ex *resx = nullptr;       /* general path: every guide (bulges) or the flagged ones */
  std::vector<uint32_t> gen_of;       /* guide -> its position in resx, or ~0u */
  std::vector<float> spec;
  std::vector<char> skip;
  char *text = nullptr; /* --encoder gpu: the batch's lines as the device wrote them (gs_enumerate_text) */
  uint64_t text_len = 0;
  bool text_done = false;
  std::vector<uint64_t> text_goff; /* --format bam: where each guide begins in it, n + 1 entries */
  bool text_members = false; /* --bgzf gpu: `text` holds the batch's BGZF members, ready for the file */
};
/* everything a batch holds goes back: after it is written, and for the batches of a failed run that never were */
inline void release_batch(batch &b) {
  for (text_part &pt : b.parts) gs_free(pt.p);
  if (b.res) gs_result_free(b.res);
  if (b.resx) gs_result_ex_free(b.resx);
  if (b.text) gs_free(b.text);
  const size_t lo = b.lo, hi = b.hi;
  b = batch();
  b.lo = lo;
  b.hi = hi;
}

/* the arrays of a candidate set where they lie, in HBM or in the host copy the object keeps */
struct kmers_view {
  const char *seqs = nullptr, *pams = nullptr, *ids = nullptr;
  const uint64_t *id_off = nullptr;
  const uint8_t *sense = nullptr;
};
inline gs_status view_kmers(gs_kmers *km, int on_device, uint64_t *n, kmers_view &v) {
  const void *a = nullptr, *p = nullptr, *i = nullptr, *o = nullptr, *s = nullptr;
  gs_status rc = gs_kmers_get(km, on_device, n, &a, &p, nullptr, nullptr);
  if (rc == GS_OK) rc = gs_kmers_get_ids(km, on_device, &i, &o, &s);
  if (rc == GS_OK) v = kmers_view{(const char *)a, (const char *)p, (const char *)i, (const uint64_t *)o, (const uint8_t *)s};
  return rc;
}

/* --all-candidates: every candidate of the selected chromosomes in one stream in HBM (gs_kmers_concat), ids included;
 * host copies only when a batch takes the host route.  Freed with the command. */
struct candidate_set {
  gs_kmers *all = nullptr;
  uint64_t n = 0;
  size_t n_chr = 0;
  uint32_t L = 0, P = 0;
  bool from_file = false; /* --kmers gpu: the rows of the kmers file, parsed on the device */
  kmers_view d, h; /* h: once on_host */
  std::mutex mtx;
  bool on_host = false;
  std::string host_error;
  /* --regions: the file's tables and, while a selection waits for the index, the records of (candidate, group) */
  gs_regions *regions = nullptr;
  gs_design *design = nullptr;
  uint64_t n_scanned = 0;
  ~candidate_set() {
    if (all) gs_kmers_free(all);
    if (design) gs_design_free(design);
    if (regions) gs_regions_free(regions);
  }
};

struct enumerate_job {
  std::vector<kmer_row> kmers;
  candidate_set *cand = nullptr;
  bool cand_device = false; /* batches go to gs_enumerate_text_device first */
  std::vector<batch> batches;
  genome_structure gs;
  gs_genome_structure cgs{};
  std::vector<const char *> names;
  std::string alts;
  std::vector<uint32_t> alt_lens; /* symbols of each alt PAM: any length next to the guides' PAM (process.hpp:51-56) */
  uint32_t n_alt = 0;
  uint32_t mismatches = 3, rna = 0, dna = 0, tflags = 0, sflags = 0;
  long long max_off = -1, threshold = -1;
  unsigned fmt_threads = 1;
  size_t window = 2; /* batches searched but not yet written, at most: bounds the host memory held by results */
  /* --format bam: the SAM lines of the encoder, turned into BAM records and BGZF blocks by the formatting
   * threads (bam_writer.hpp; the reference leaves that step to `samtools view -b`, manual/manual.tex:581-582) */
  bool bam = false;
  std::map<std::string, int32_t> refid;
  /* --encoder gpu: a batch that is all fast path leaves the device as text (gs_enumerate_text: search, scoring and the
   * CSV / SAM encoder in HBM), any other batch - and one that answers GS_ERR_UNSUPPORTED - takes the host encoders */
  bool encoder_gpu = false;
  /* --bgzf gpu (with --format bam): a batch that is all fast path leaves the device as BGZF members (gs_enumerate_text with
   * GS_TEXT_BAM | GS_TEXT_BGZF: search, scoring, the record encoder and the compressor in HBM); any other batch takes the
   * host's records and zlib.  Members are independent, so the file is one BAM either way. */
  bool bgzf_gpu = false;
  std::mutex tally_mtx;   /* the device threads count under it: */
  size_t enc_device = 0;  /* batches the device encoded; every other batch went to the host encoders */
  size_t bgzf_device = 0; /* batches the device compressed */
  const gs_annot *annot = nullptr; /* --annotate: what the host encoders look rows up in (tflags has GS_TEXT_FEATURES) */
  uint32_t text_flags() const { return bgzf_gpu ? (tflags & ~GS_TEXT_SAM) | GS_TEXT_BAM | GS_TEXT_BGZF : tflags; }
};

/* the output file: written at its own offset by one thread, closed by finish() or with the command */
struct output_file {
  std::string path;
  int fd = -1;
  uint64_t off = 0;
  bool ok = true; /* no short write so far */
  bool open(const std::string &p) {
    path = p;
    fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) std::cerr << "error: cannot write " << p << "\n";
    return fd >= 0;
  }
  void append(const char *p, size_t n) {
    uint64_t at = off;
    off += n;
    while (n) {
      const ssize_t w = pwrite(fd, p, n, (off_t)at);
      if (w <= 0) {
        ok = false;
        return;
      }
      p += w;
      n -= (size_t)w;
      at += (uint64_t)w;
    }
  }
  /* closes the file; a run that failed leaves no file that looks like a database (CSV/SAM rows up to the failed batch,
   * a BAM without its end-of-file block).  true: the file is whole */
  bool finish(bool failed) {
    /* only a regular file is ever removed: -o /dev/stdout, a FIFO or a device node stays (written through pwrite they
     * fail with ESPIPE, and unlinking them would delete the node itself) */
    struct stat fst;
    const bool regular = fstat(fd, &fst) == 0 && S_ISREG(fst.st_mode);
    if (::close(fd) != 0) ok = false;
    fd = -1;
    if (!ok) std::cerr << "error: short write to " << path << "\n";
    if ((failed || !ok) && regular && unlink(path.c_str()) == 0) std::cerr << "error: " << path << " removed (incomplete)\n";
    return ok && !failed;
  }
  ~output_file() {
    if (fd >= 0) ::close(fd);
  }
};

/* a part's SAM text -> BGZF-compressed BAM records (in place: the text is released) */
inline bool part_to_bam(const enumerate_job &job, text_part &part) {
  std::string raw;
  bool ok = true;
  if (part.p) ok = bam::records(part.p, part.n, job.refid, raw);
  if (ok && !part.s.empty()) ok = bam::records(part.s.data(), part.s.size(), job.refid, raw);
  if (part.p) gs_free(part.p);
  part.p = nullptr;
  part.n = 0;
  part.s.clear();
  return ok && bam::bgzf_append(raw, part.s);
}

/* fn(part, lo, hi) -> gs_status on the batch's guides cut into nt contiguous ranges (at most one per guide), each on a
 * thread of its own with a part of its own; the first range's failure.  BGZF blocks start anew with every part, so
 * every route of a BAM batch must cut here */
template <class F>
gs_status for_ranges(batch &b, unsigned nt, F fn) {
  const size_t n = b.hi - b.lo;
  nt = (unsigned)std::min<size_t>(std::max(nt, 1u), n);
  b.parts.assign(nt, text_part());
  std::vector<gs_status> prc(nt, GS_OK);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nt; t++)
    pool.emplace_back([&, t]() { prc[t] = fn(b.parts[t], n * t / nt, n * (t + 1) / nt); });
  for (auto &th : pool) th.join();
  for (unsigned t = 0; t < nt; t++)
    if (prc[t] != GS_OK) return prc[t];
  return GS_OK;
}

/* one range of a batch from its hit lists */
inline gs_status format_range(const enumerate_job &job, const batch &b, const gs_result_view &v, const uint64_t *xoff,
                              const gs_hit_ex *xhits, text_part &part, size_t lo, size_t hi) {
  if (b.gen_of.empty() && !b.resx) {
    /* the whole range in one buffer, rows written in place (no per-hit strings) */
    std::vector<gs_kmer> ck(hi - lo);
    for (size_t g = lo; g < hi; g++) {
      const kmer_row &k = b.rows[g];
      ck[g - lo] = gs_kmer{k.id.c_str(), k.sequence.c_str(), k.pam.c_str(), k.sense == "+" ? 1 : 0};
    }
    const gs_status rc = gs_format_guides_features(&job.cgs, ck.data(), hi - lo, v.guide_offsets + lo, v.hits, b.spec.data() + lo,
                                                   b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data() + lo, job.mismatches,
                                                   job.tflags | job.sflags, job.max_off, job.annot, &part.p, &part.n);
    if (rc != GS_OK) return rc;
    return job.bam && !part_to_bam(job, part) ? GS_ERR_FORMAT : GS_OK;
  }
  char *tx = nullptr;
  size_t tl = 0;
  for (size_t g = lo; g < hi; g++) {
    if (!b.skip.empty() && b.skip[g]) continue;
    const kmer_row &k = b.rows[g];
    gs_kmer ck{k.id.c_str(), k.sequence.c_str(), k.pam.c_str(), k.sense == "+" ? 1 : 0};
    gs_status r;
    const uint32_t gx = b.gen_of.empty() ? ~0u : b.gen_of[g];
    if (gx == ~0u) {
      const uint64_t s0 = v.guide_offsets[g], s1 = v.guide_offsets[g + 1];
      r = gs_format_guide_features(&job.cgs, &ck, v.hits + s0, s1 - s0, job.mismatches, job.tflags | job.sflags,
                                   job.max_off, b.spec[g], job.annot, &tx, &tl);
    } else {
      const uint64_t s0 = xoff[gx], s1 = xoff[gx + 1];
      r = gs_format_guide_ex_features(&job.cgs, &ck, xhits + s0, s1 - s0, job.mismatches, job.tflags | job.sflags,
                                      job.max_off, job.annot, &tx, &tl);
    }
    if (r != GS_OK) return r;
    part.s.append(tx, tl);
    gs_free(tx);
  }
  return job.bam && !part_to_bam(job, part) ? GS_ERR_FORMAT : GS_OK;
}

/* text of one batch: as the device left it, or from its hit lists, contiguous guide ranges formatted in parallel */
inline std::string format_batch(const enumerate_job &job, batch &b) {
  gs_status rc;
  if (b.text_done && (!job.bam || b.text_members)) { /* CSV / SAM lines or BGZF members: to the writer as they are */
    b.parts.assign(1, text_part());
    b.parts[0].p = b.text;
    b.parts[0].n = (size_t)b.text_len;
    b.text = nullptr;
    return "";
  }
  if (b.text_done) {
    /* SAM lines for a BAM: part t begins where the host path's range t begins, at its first guide's place in the text
     * (gs_index_last_text_offsets, taken when the text was), and is turned into records by the formatting threads */
    rc = for_ranges(b, job.fmt_threads, [&](text_part &part, size_t lo, size_t hi) {
      std::string raw;
      const bool ok = bam::records(b.text + b.text_goff[lo], (size_t)(b.text_goff[hi] - b.text_goff[lo]), job.refid, raw) &&
                      bam::bgzf_append(raw, part.s);
      return ok ? GS_OK : GS_ERR_FORMAT;
    });
    gs_free(b.text);
    b.text = nullptr;
  } else {
    gs_result_view v;
    memset(&v, 0, sizeof v);
    if (b.res) gs_result_get(b.res, &v);
    const uint64_t *xoff = nullptr;
    const gs_hit_ex *xhits = nullptr;
    if (b.resx) gs_result_ex_get(b.resx, nullptr, &xoff, &xhits);
    rc = for_ranges(b, job.fmt_threads,
                    [&](text_part &part, size_t lo, size_t hi) { return format_range(job, b, v, xoff, xhits, part, lo, hi); });
    if (b.res) gs_result_free(b.res);
    if (b.resx) gs_result_ex_free(b.resx);
    b.res = nullptr;
    b.resx = nullptr;
    b.spec = std::vector<float>();
  }
  return rc == GS_OK ? "" : gs_status_string(rc);
}

/* --all-candidates: the batch's candidates as rows on the host, for the route a kmers file's batch takes */
inline std::string candidates_to_host(enumerate_job &job, batch &b) {
  candidate_set &cs = *job.cand;
  {
    std::lock_guard<std::mutex> lk(cs.mtx);
    if (!cs.on_host && cs.host_error.empty()) {
      const gs_status rc = view_kmers(cs.all, 0, nullptr, cs.h);
      cs.on_host = rc == GS_OK;
      if (rc != GS_OK) cs.host_error = gs_status_string(rc);
    }
    if (!cs.host_error.empty()) return cs.host_error;
  }
  const size_t n = b.hi - b.lo;
  b.own.resize(n);
  b.seqs.assign(cs.h.seqs + b.lo * cs.L, n * cs.L);
  b.pams.assign(cs.h.pams + b.lo * cs.P, n * cs.P);
  for (size_t g = 0; g < n; g++) {
    kmer_row &r = b.own[g];
    const size_t at = b.lo + g;
    r.id.assign(cs.h.ids + cs.h.id_off[at], (size_t)(cs.h.id_off[at + 1] - cs.h.id_off[at]));
    r.sequence.assign(cs.h.seqs + at * cs.L, cs.L);
    r.pam.assign(cs.h.pams + at * cs.P, cs.P);
    r.sense = cs.h.sense[at] ? "+" : "-";
    r.position = 0;
  }
  b.rows = b.own.data();
  return "";
}

/* --threshold t (process.hpp:66-76): a guide with more than one hit within t mismatches (both indexes, bulges off;
 * counted per PAM pattern, before duplicate sequences collapse: a site that two PAM patterns of the list match counts
 * twice, as off_target_counter does) is dropped before the real search.  raw: the batch's raw counts of a search at
 * t mismatches, whichever route counted them */
inline void threshold_skip(batch &b, const uint32_t *raw) {
  const size_t n = b.hi - b.lo;
  b.skip.resize(n);
  for (size_t g = 0; g < n; g++) b.skip[g] = raw[g] > 1;
}

/* the batch left the device as text or as BGZF members: counted, its guides' places fetched where the formatting threads
 * cut the text (BAM by the host's records), and marked as needing no hit lists */
inline gs_status batch_left_as_text(enumerate_job &job, gs_index *ix, batch &b) {
  const size_t n = b.hi - b.lo;
  if (job.bam && !job.bgzf_gpu) { /* this thread alone uses the handle: the last text is still this one */
    b.text_goff.resize(n + 1);
    const gs_status rc = gs_index_last_text_offsets(ix, b.text_goff.data(), n);
    if (rc != GS_OK) return rc;
  }
  {
    std::lock_guard<std::mutex> lk(job.tally_mtx);
    job.enc_device++;
    if (job.bgzf_gpu) job.bgzf_device++;
  }
  b.text_members = job.bgzf_gpu;
  b.text_done = true;
  return GS_OK;
}

/* the guides of the batch that the fast path flagged (GS_GUIDE_NEEDS_GENERAL: symbols it does not encode,
 * index.hpp:218-247) through the general path at `mismatches`, for them alone: idx[j] is the batch's guide that is
 * guide j of *out */
inline gs_status search_flagged(const enumerate_job &job, gs_index *ix, const batch &b, const uint8_t *guide_flags,
                                uint32_t mismatches, std::vector<uint32_t> &idx, gs_result_ex **out) {
  std::string s2, p2;
  idx.clear();
  for (size_t g = 0; g < b.hi - b.lo; g++)
    if (guide_flags[g] & GS_GUIDE_NEEDS_GENERAL) {
      idx.push_back((uint32_t)g);
      s2.append(b.seqs, g * b.L, b.L);
      p2.append(b.pams, g * b.P, b.P);
    }
  return gs_enumerate_general(ix, s2.data(), idx.size(), b.L, p2.data(), b.P, job.alts.data(), b.P ? job.n_alt : 0, mismatches, 0, 0,
                              job.sflags, out);
}

/* the threshold filter of a batch on the host route: b.skip */
inline gs_status threshold_filter(const enumerate_job &job, gs_index *ix, batch &b, bool all_general) {
  const size_t n = b.hi - b.lo;
  const uint32_t n_alt = b.P ? job.n_alt : 0, t = (uint32_t)job.threshold;
  const uint32_t *xraw = nullptr;
  if (all_general) {
    gs_result_ex *cx = nullptr;
    const gs_status rc = gs_enumerate_general_pams(ix, b.seqs.data(), n, b.L, b.pams.data(), b.P, job.alts.data(), job.alt_lens.data(),
                                                   n_alt, t, 0, 0, job.sflags, &cx);
    if (rc != GS_OK) return rc;
    gs_result_ex_raw_hits(cx, &xraw);
    threshold_skip(b, xraw);
    gs_result_ex_free(cx);
    return GS_OK;
  }
  gs_result *cres = nullptr;
  gs_status rc = gs_enumerate(ix, b.seqs.data(), n, b.L, b.pams.data(), b.P, job.alts.data(), n_alt, t, job.sflags | GS_FLAG_RAW_COUNTS, &cres);
  if (rc != GS_OK) return rc;
  gs_result_view cv;
  gs_result_get(cres, &cv);
  std::vector<uint32_t> raw(cv.raw_hits, cv.raw_hits + n);
  if (cv.n_unsupported) { /* guides the fast path cannot count: through the general path (rare, exact) */
    std::vector<uint32_t> idx;
    gs_result_ex *cx = nullptr;
    rc = search_flagged(job, ix, b, cv.guide_flags, t, idx, &cx);
    if (rc == GS_OK) {
      gs_result_ex_raw_hits(cx, &xraw);
      for (size_t j = 0; j < idx.size(); j++) raw[idx[j]] = xraw[j];
      gs_result_ex_free(cx);
    }
  }
  gs_result_free(cres);
  if (rc == GS_OK) threshold_skip(b, raw.data());
  return rc;
}

/* --all-candidates with --encoder gpu: the batch from HBM to text (gs_enumerate_text_device).  GS_ERR_UNSUPPORTED: the
 * batch takes the host route */
inline gs_status search_batch_device(enumerate_job &job, gs_index *ix, batch &b) {
  const candidate_set &cs = *job.cand;
  const size_t n = b.hi - b.lo;
  const uint32_t n_alt = cs.P ? job.n_alt : 0;
  for (uint32_t j = 0; j < n_alt; j++)
    if (job.alt_lens[j] != cs.P) return GS_ERR_UNSUPPORTED;
  if (job.rna > 0 || job.dna > 0 || job.mismatches > 7 || job.threshold > 7) return GS_ERR_UNSUPPORTED;
  const char *d_g = cs.d.seqs + b.lo * cs.L, *d_p = cs.d.pams + b.lo * cs.P;
  gs_status rc;
  if (job.threshold > 0) { /* the raw counts of a search at t mismatches, as threshold_filter takes them */
    std::vector<uint32_t> raw(n);
    rc = gs_enumerate_text_device(ix, d_g, n, cs.L, d_p, cs.P, job.alts.data(), n_alt, (uint32_t)job.threshold,
                                  job.sflags | GS_FLAG_RAW_COUNTS, -1, &job.cgs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, raw.data());
    if (rc != GS_OK) return rc;
    threshold_skip(b, raw.data());
  }
  rc = gs_enumerate_text_device(ix, d_g, n, cs.L, d_p, cs.P, job.alts.data(), n_alt, job.mismatches, job.sflags | job.text_flags(),
                                job.max_off, &job.cgs, cs.d.ids, cs.d.id_off + b.lo, cs.d.sense + b.lo,
                                b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data(), &b.text, &b.text_len, nullptr, nullptr);
  return rc == GS_OK ? batch_left_as_text(job, ix, b) : rc;
}

/* --encoder gpu / --bgzf gpu on the host route: the batch from host pointers to text (gs_enumerate_text).
 * GS_ERR_UNSUPPORTED: a guide of the batch needs the general path, the batch is redone the usual way */
inline gs_status search_batch_text(enumerate_job &job, gs_index *ix, batch &b) {
  const size_t n = b.hi - b.lo;
  std::string ids;
  std::vector<uint64_t> id_off(n + 1, 0);
  std::vector<uint8_t> senses(n);
  for (size_t g = 0; g < n; g++) {
    const kmer_row &k = b.rows[g];
    ids += k.id;
    id_off[g + 1] = ids.size();
    senses[g] = k.sense == "+" ? 1 : 0;
  }
  const gs_status rc = gs_enumerate_text(ix, b.seqs.data(), n, b.L, b.pams.data(), b.P, job.alts.data(), b.P ? job.n_alt : 0,
                                         job.mismatches, job.sflags | job.text_flags(), job.max_off, &job.cgs, ids.data(),
                                         id_off.data(), senses.data(), b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data(),
                                         &b.text, &b.text_len, nullptr);
  return rc == GS_OK ? batch_left_as_text(job, ix, b) : rc;
}

/* the host route of one batch: threshold filter, search (fast path; general path for the guides it flags, or for all of
 * them with bulges), scoring */
inline gs_status search_batch_as(enumerate_job &job, gs_index *ix, batch &b, bool all_general) {
  const size_t n = b.hi - b.lo;
  const uint32_t L = b.L, P = b.P;
  const uint32_t n_alt = P ? job.n_alt : 0;
  /* an alt PAM shorter or longer than the batch's PAM: the fixed-width fast path does not take it; the
   * general path searches every pattern at its own length, as the reference does */
  for (uint32_t j = 0; j < n_alt; j++) all_general = all_general || job.alt_lens[j] != P;
  gs_status rc;
  if (job.threshold > 0 && (rc = threshold_filter(job, ix, b, all_general)) != GS_OK) return rc;
  if (all_general || job.rna > 0 || job.dna > 0) {
    /* bulge-aware search: index.hpp:250-375 behind gs_enumerate_general; alt PAMs of other lengths: the same entry */
    rc = gs_enumerate_general_pams(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), job.alt_lens.data(), n_alt,
                                   job.mismatches, job.rna, job.dna, job.sflags, &b.resx);
    if (rc != GS_OK) return rc;
    b.gen_of.resize(n);
    for (size_t g = 0; g < n; g++) b.gen_of[g] = (uint32_t)g;
    return GS_OK;
  }
  if ((job.encoder_gpu || job.bgzf_gpu) && job.mismatches <= 7) {
    rc = search_batch_text(job, ix, b);
    if (rc != GS_ERR_UNSUPPORTED) return rc;
  }
  rc = gs_enumerate(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), n_alt, job.mismatches, job.sflags, &b.res);
  if (rc != GS_OK) return rc;
  gs_result_view v;
  gs_result_get(b.res, &v);
  if (v.n_unsupported) { /* the rest of the batch is untouched */
    std::vector<uint32_t> idx;
    rc = search_flagged(job, ix, b, v.guide_flags, job.mismatches, idx, &b.resx);
    if (rc != GS_OK) return rc;
    b.gen_of.assign(n, ~0u);
    for (size_t j = 0; j < idx.size(); j++) b.gen_of[idx[j]] = (uint32_t)j;
  }
  /* specificity of every guide of the batch on the device (printer.hpp:98-170, 251-297 behind
   * gs_score): the formatting threads only print */
  b.spec.resize(n);
  return gs_score(ix, b.seqs.data(), n, L, P, job.tflags | job.sflags, job.max_off, &job.cgs, v.guide_offsets, v.hits, nullptr,
                  b.spec.data());
}

/* the device side of one batch, on the route that takes it */
inline std::string search_batch(enumerate_job &job, gs_index *ix, batch &b) {
  if (job.cand) {
    if (job.cand_device) {
      const gs_status rc = search_batch_device(job, ix, b);
      if (rc != GS_ERR_UNSUPPORTED) return rc == GS_OK ? "" : gs_status_string(rc);
      b.skip.clear();
    }
    const std::string err = candidates_to_host(job, b);
    if (!err.empty()) return err;
  } else {
    for (size_t g = b.lo; g < b.hi; g++) {
      b.seqs += job.kmers[g].sequence;
      b.pams += job.kmers[g].pam;
    }
  }
  /* Match sequences beyond the fast path's key: up to 59 bits (23-mers with a four-symbol PAM: 58) the table-seeded
   * kernels carry them; the reference-order walk (small genomes whose table is too shallow for the context arrays)
   * stops at 52 and says GS_ERR_UNSUPPORTED - then, and beyond 59 bits, the general path carries sequences as bytes */
  const uint32_t bits = 2 * b.L + 3 * b.P;
  gs_status rc = search_batch_as(job, ix, b, bits > 59);
  if (rc == GS_ERR_UNSUPPORTED && bits > 52 && bits <= 59) {
    if (b.res) gs_result_free(b.res);
    b.res = nullptr;
    b.skip.clear();
    rc = search_batch_as(job, ix, b, true);
  }
  return rc == GS_OK ? "" : gs_status_string(rc);
}

/* PREFIX.gs, and PREFIX.dna (this tool's `index`) or, for indices made by the reference, PREFIX.forward */
inline bool load_genome(const options &o, genome_structure &gs, std::string &text, bool &from_sdsl) {
  std::string err;
  if (!cli::read_gs(o.prefix + ".gs", gs, err)) {
    std::cerr << "error: " << err << "\n";
    return false;
  }
  if (std::ifstream(o.prefix + ".dna")) {
    cli::read_file(o.prefix + ".dna", text);
  } else if (std::ifstream(o.prefix + ".forward")) {
    if (o.all_candidates) {
      std::cerr << "error: --all-candidates needs " << o.prefix << ".dna, the genome text the candidates are cut from: " << o.prefix
                << " has only the .forward / .reverse index files\n";
      return false;
    }
    from_sdsl = true;
  } else {
    std::cerr << "error: neither " << o.prefix << ".dna nor " << o.prefix << ".forward exists\n";
    return false;
  }
  return true;
}

/* -f: the guides are the rows of the kmers file */
inline bool read_guides(const options &o, enumerate_job &job) {
  std::string err;
  const auto t0 = std::chrono::steady_clock::now();
  if (!cli::read_kmers(o.kmers_file, job.kmers, err)) {
    std::cerr << "error: " << err << "\n";
    return false;
  }
  if (o.verbose)
    std::cout << "kmers host: read_kmers " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s\n";
  std::cout << "Read in " << job.kmers.size() << " kmer(s).\n";
  return true;
}

/* -f --kmers gpu: the file is parsed on the first device (gs_kmers_parse_file) into a candidate set, and the command goes
 * on as --all-candidates does from its scan.  The host reader's messages and status; a file the device reader does not
 * take (rows of several shapes) is read by the host reader after all */
inline bool read_guides_device(const options &o, enumerate_job &job, candidate_set &cand) {
  gs_kmers_report rep;
  gs_status rc = gs_kmers_parse_file(o.device, o.kmers_file.c_str(), &cand.all, &rep);
  if (rc == GS_ERR_UNSUPPORTED) {
    if (o.verbose) std::cout << "kmers gpu: rows of several shapes, the file is read on the host\n";
    return read_guides(o, job);
  }
  if (rc == GS_ERR_FORMAT && rep.bad_kind >= GS_KMERS_BAD_FEW && rep.bad_kind <= GS_KMERS_BAD_LACKS) { /* cli::read_kmers' messages */
    static const char *const what[5] = {"", "kmers row with too few columns: ", "kmers position is not an integer: ", "empty kmers file",
                                        "kmers file lacks column "};
    std::cerr << "error: " << what[rep.bad_kind] << std::string(rep.bad_text ? rep.bad_text : "", (size_t)rep.bad_len) << "\n";
    gs_free(rep.bad_text);
    return false;
  }
  if (rc == GS_ERR_IO) {
    std::cerr << "error: cannot open kmers file\n";
    return false;
  }
  if (rc == GS_OK) rc = view_kmers(cand.all, 1, &cand.n, cand.d);
  if (rc != GS_OK) {
    std::cerr << "error: kmers file on the device: " << gs_status_string(rc) << "\n";
    return false;
  }
  cand.from_file = true;
  cand.L = (uint32_t)rep.L;
  cand.P = (uint32_t)rep.P;
  job.cand = &cand;
  /* as scan_candidates: one device, and a shape the fast path's key takes; every other batch takes the host route */
  job.cand_device = (o.encoder == "gpu" || o.bgzf == "gpu") && o.gpus == 1 && cand.L <= 31 && 2 * cand.L + 3 * cand.P <= 59;
  if (o.verbose)
    std::cout << "kmers gpu: file reads " << rep.ms[0] / 1e3 << " s, waits for the uploads " << rep.ms[1] / 1e3 << " s, device stage "
              << rep.ms[2] / 1e3 << " s\n";
  std::cout << "Read in " << cand.n << " kmer(s).\n";
  return true;
}

/* --regions: the BED file against PREFIX.gs (cli::read_bed) */
inline bool read_regions(const std::string &path, const genome_structure &gs, const std::string &prefix, candidate_set &cand) {
  return read_bed(path, gs, prefix, "regions", &cand.regions);
}

/* --annotate: the BED file under the rules and messages of --regions, then one lookup table per device, attached to its
 * index; the host encoders read the first one's host copy.  Declared before the indexes: freed after they are closed */
struct annotation_set {
  gs_regions *bed = nullptr;
  std::vector<gs_annot *> an;
  ~annotation_set() {
    for (gs_annot *a : an) gs_annot_free(a);
    if (bed) gs_regions_free(bed);
  }
};
inline bool read_annotation(const options &o, const genome_structure &gs, annotation_set &as) {
  return read_bed(o.annotate, gs, "", "annotation", &as.bed);
}
inline bool attach_annotation(const options &o, const std::vector<gs_index *> &ix, annotation_set &as, enumerate_job &job) {
  const int dev_step = getenv("GS_CLI_SAME_DEVICE") ? 0 : 1; /* as build_indexes places the indexes */
  for (size_t d = 0; d < ix.size(); d++) {
    gs_annot *a = nullptr;
    gs_status rc = gs_annot_build(as.bed, o.device + (int)d * dev_step, &a);
    if (rc == GS_OK) {
      as.an.push_back(a);
      rc = gs_index_set_annotation(ix[d], a);
    }
    if (rc != GS_OK) {
      std::cerr << "error: annotation file " << o.annotate << ": " << gs_status_string(rc) << "\n";
      return false;
    }
  }
  uint64_t groups = 0, segments = 0, entries = 0;
  gs_annot_info(as.an[0], &groups, &segments, &entries);
  std::cout << "Annotation: " << groups << " group(s), " << segments << " segment(s), " << entries << " table entries on "
            << ix.size() << " device(s)\n";
  job.annot = as.an[0];
  return true;
}

/* --regions: the records scored on the first device where an option asks for it (ix; the search options are the
 * command's own -m, -a, --start, and -t marks what the counting pass would drop as not eligible), ordered, cut to the
 * best of each group, and handed to the candidate set as the guides of the command */
inline bool select_design(const options &o, enumerate_job &job, candidate_set &cand, gs_index *ix) {
  if (ix && o.max_feature_hits >= 0 &&
      gs_design_set_feature_rule(cand.design, job.annot, (uint32_t)(o.feature_distance >= 0 ? o.feature_distance : o.mismatches),
                                 (uint32_t)o.max_feature_hits) != GS_OK) {
    std::cerr << "error: --max-feature-hits: " << gs_status_string(GS_ERR_ARG) << "\n";
    return false;
  }
  const auto ts = std::chrono::steady_clock::now();
  gs_status rc = GS_OK;
  if (ix) {
    std::string alts;
    for (auto &a : o.alt_pams) {
      if (a.size() != cand.P) {
        std::cerr << "error: --regions with --per-region, --min-specificity or --max-feature-hits scores on the fast path: alt PAM " << a
                  << " is not of the PAM's length\n";
        return false;
      }
      alts += a;
    }
    if (o.rna > 0 || o.dna > 0 || o.mismatches > 7 || o.threshold > 7) {
      std::cerr << "error: --regions with --per-region, --min-specificity or --max-feature-hits scores on the fast path: no bulges, at most 7 mismatches\n";
      return false;
    }
    uint64_t n_rec = 0, glen = 0;
    gs_design_info(cand.design, &n_rec, nullptr);
    for (uint64_t l : job.gs.lengths) glen += l;
    const uint32_t flags = (o.co.start ? GS_FLAG_PAM_AT_START : 0u) | ((double)n_rec < 6e-4 * (double)glen ? GS_FLAG_NO_NEW_TABLES : 0u);
    rc = gs_design_score(ix, cand.design, alts.data(), (uint32_t)o.alt_pams.size(), (uint32_t)o.mismatches, flags,
                         o.threshold > 0 ? o.threshold : -1, o.batch_size, nullptr);
    if (rc == GS_ERR_UNSUPPORTED) {
      std::cerr << "error: --regions with --per-region, --min-specificity or --max-feature-hits scores on the fast path, which does not take this job: "
                << gs_status_string(rc) << "\n";
      return false;
    }
  }
  const bool paired = !o.pairs.empty();
  uint64_t last[4] = {0, 0, 0, 0}, plast[6] = {0, 0, 0, 0, 0, 0}, spaced[2] = {0, 0};
  if (rc == GS_OK && paired) { /* --per-region counts pairs: the guides are the members of the kept ones */
    gs_pair_rule rule;
    memset(&rule, 0, sizeof rule);
    rule.min_span = o.min_span >= 0 ? (uint64_t)o.min_span : 1;
    rule.max_span = (uint64_t)o.max_span;
    rule.cut_offset = o.cut_offset >= 0 ? (uint32_t)o.cut_offset : 3;
    rule.orientation = o.pair_orientation == "pam-out" ? GS_PAIRS_PAM_OUT : o.pair_orientation == "pam-in" ? GS_PAIRS_PAM_IN : GS_PAIRS_ANY;
    rule.per_region = (uint32_t)o.per_region;
    rule.flags = o.co.start ? GS_FLAG_PAM_AT_START : 0u;
    rule.min_specificity = o.min_spec;
    gs_pairs *pr = nullptr;
    rc = gs_design_pairs(cand.design, o.co.prefix.c_str(), &rule, nullptr, &cand.all, &pr);
    char *table = nullptr;
    uint64_t len = 0;
    if (rc == GS_OK) rc = gs_pairs_rows(pr, cand.all, &table, &len);
    if (rc == GS_OK) gs_pairs_last(pr, plast);
    gs_pairs_free(pr);
    if (rc == GS_OK) { /* all or nothing, as -o is */
      output_file pf;
      bool ok = pf.open(o.pairs);
      if (ok) {
        pf.append(table, (size_t)len);
        ok = pf.finish(false);
      }
      gs_free(table);
      if (!ok) return false;
    }
  } else if (rc == GS_OK) {
    if (o.min_spacing > 0)
      rc = gs_design_set_spacing(cand.design, (uint32_t)o.min_spacing, o.cut_offset >= 0 ? (uint32_t)o.cut_offset : 3,
                                 o.co.start ? GS_FLAG_PAM_AT_START : 0u);
    if (rc == GS_OK) rc = gs_design_select(cand.design, o.co.prefix.c_str(), (uint32_t)o.per_region, o.min_spec, nullptr, &cand.all);
    if (rc == GS_OK) gs_design_last_select(cand.design, last);
    if (rc == GS_OK) gs_design_last_spacing(cand.design, spaced);
  }
  if (rc == GS_OK) rc = view_kmers(cand.all, 1, &cand.n, cand.d);
  if (rc != GS_OK) {
    std::cerr << "error: " << (paired ? "pairs" : "selection") << " for --regions: " << gs_status_string(rc) << "\n";
    return false;
  }
  gs_design_free(cand.design);
  cand.design = nullptr;
  job.cand = &cand;
  job.cand_device = (o.encoder == "gpu" || o.bgzf == "gpu") && o.gpus == 1 && cand.L <= 31 && 2 * cand.L + 3 * cand.P <= 59;
  if (paired) {
    uint64_t n_groups = 0;
    gs_regions_info(cand.regions, &n_groups, nullptr);
    std::cout << "Paired " << plast[2] << " pair(s) of " << cand.n << " guide(s) in " << n_groups - plast[4] << " group(s)\n";
    if (o.verbose)
      std::cout << "Pairs: " << plast[1] << " counted among " << plast[0] << " eligible record(s) in " << plast[3] << " chunk(s); "
                << plast[4] << " group(s) left without a pair, " << plast[5] << " group(s) short of --per-region\n";
    return true;
  }
  std::cout << "Selected " << cand.n << " guide(s) of " << last[0] << " record(s) in "
            << std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count() << " s\n";
  if (o.verbose)
    std::cout << "Regions: " << last[2] << " group(s) left without a guide, " << last[3] << " group(s) short of --per-region\n";
  if (o.min_spacing > 0)
    std::cout << "Spacing: " << spaced[0] << " record(s) passed over within " << o.min_spacing << " base(s) of a pick, " << spaced[1]
              << " group(s) short of --per-region for it\n";
  return true;
}

/* --all-candidates: scan first, search afterwards - the table rule of derive_job needs the true candidate count.  Every
 * selected chromosome is scanned and its ids are encoded on the first device; one concatenation makes the stream the
 * batches are cut from */
inline bool scan_candidates(const options &o, const std::string &text, enumerate_job &job, candidate_set &cand) {
  const cli::candidate_opts &co = o.co;
  const auto ts = std::chrono::steady_clock::now();
  std::vector<size_t> sel;
  std::vector<uint64_t> begin;
  std::string err;
  if (!cli::select_chromosomes(o.prefix, job.gs, text.size(), co, sel, begin, err)) {
    std::cerr << "error: " << err << "\n";
    return false;
  }
  std::vector<gs_kmers *> parts;
  std::vector<gs_design *> dparts;
  gs_status rc = GS_OK;
  uint64_t rule_counts[4] = {0, 0, 0, 0};
  if (!o.regions.empty() && !read_regions(o.regions, job.gs, co.prefix, cand)) return false;
  for (size_t c : sel) {
    gs_kmers *km = nullptr;
    rc = gs_kmers_generate(o.device, (const uint8_t *)text.data() + begin[c], job.gs.lengths[c], 0, co.pam.c_str(), (uint32_t)co.k,
                           co.start ? GS_FLAG_PAM_AT_START : 0u, nullptr, &km);
    /* the sequence rules, on the scan's device and before anything is restricted or scored */
    if (rc == GS_OK && (rc = cli::apply_seq_rule(o.seq, &km, rule_counts)) != GS_OK) gs_kmers_free(km);
    if (rc != GS_OK) break;
    if (cand.regions) { /* the chromosome's candidates inside the intervals; the scan itself is dropped */
      gs_design *dp = nullptr;
      uint64_t n = 0;
      gs_kmers_get(km, 1, &n, nullptr, nullptr, nullptr, nullptr);
      cand.n_scanned += n;
      rc = gs_design_restrict(cand.regions, (uint32_t)c, km, nullptr, &dp);
      gs_kmers_free(km);
      if (rc != GS_OK) break;
      dparts.push_back(dp);
      continue;
    }
    parts.push_back(km);
    rc = gs_kmers_encode_ids(km, co.prefix.c_str(), job.gs.names[c].c_str(), nullptr);
    if (rc != GS_OK) break;
  }
  if (cand.regions) {
    if (rc == GS_OK && dparts.empty()) {
      std::cerr << "error: --regions: no chromosome selected\n";
      rc = GS_ERR_ARG;
    } else if (rc == GS_OK) {
      rc = gs_design_concat(dparts.data(), (uint32_t)dparts.size(), &cand.design);
    }
    for (gs_design *dp : dparts) gs_design_free(dp);
    if (rc != GS_OK) {
      std::cerr << "error: candidate scan for --regions (--pam " << co.pam << ", --kmer-length " << co.k << "): " << gs_status_string(rc) << "\n";
      return false;
    }
    cand.n_chr = sel.size();
    cand.L = (uint32_t)co.k;
    cand.P = (uint32_t)co.pam.size();
    uint64_t n_rec = 0;
    gs_design_info(cand.design, &n_rec, nullptr);
    if (o.seq.given) {
      cand.n_scanned = rule_counts[0];
      std::cout << cli::seq_rule_line(rule_counts);
    }
    std::cout << "Scanned " << cand.n_scanned << " candidate(s) of " << sel.size() << " chromosome(s), " << n_rec
              << " record(s) inside the regions, in " << std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count() << " s\n";
    /* a selection by specificity waits for the index (select_design); otherwise the records are ordered now, and -t is the
     * pipeline's own threshold pass over them, on whatever route a batch takes */
    return o.selects() ? true : select_design(o, job, cand, nullptr);
  }
  if (rc == GS_OK && parts.empty()) { /* no chromosome selected: an empty set with ids */
    gs_kmers *km = nullptr;
    rc = gs_kmers_generate(o.device, nullptr, 0, 0, co.pam.c_str(), (uint32_t)co.k, 0u, nullptr, &km);
    if (rc == GS_OK) {
      parts.push_back(km);
      rc = gs_kmers_encode_ids(km, "", "", nullptr);
    }
  }
  if (rc == GS_OK) rc = gs_kmers_concat(parts.data(), (uint32_t)parts.size(), &cand.all);
  for (gs_kmers *km : parts) gs_kmers_free(km);
  if (rc == GS_OK) rc = view_kmers(cand.all, 1, &cand.n, cand.d);
  if (rc != GS_OK) {
    std::cerr << "error: candidate scan (--pam " << co.pam << ", --kmer-length " << co.k << "): " << gs_status_string(rc) << "\n";
    return false;
  }
  cand.n_chr = sel.size();
  cand.L = (uint32_t)co.k;
  cand.P = (uint32_t)co.pam.size();
  job.cand = &cand;
  /* 2L + 3P > 59: no batch fits the fast path's key, every one takes the host route */
  job.cand_device = (o.encoder == "gpu" || o.bgzf == "gpu") && o.gpus == 1 && cand.L <= 31 && 2 * cand.L + 3 * cand.P <= 59;
  if (o.seq.given) std::cout << cli::seq_rule_line(rule_counts);
  std::cout << "Scanned " << cand.n << " candidate(s) of " << sel.size() << " chromosome(s) in "
            << std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count() << " s\n";
  return true;
}

/* one index per device, built side by side (src/guidescan.cxx:226-251 fans the guides out over
 * threads that share one index; here every GPU holds its own copy in HBM) */
inline bool build_indexes(const options &o, const std::string &text, bool from_sdsl, cli::index_set &idx) {
  const auto t0 = std::chrono::steady_clock::now();
  /* GS_CLI_SAME_DEVICE=1: every worker builds its index on the first device itself - the fan-out, the batch queue
   * and the ordered writer run with N workers on a box with one GPU (tests) */
  const int dev_step = getenv("GS_CLI_SAME_DEVICE") ? 0 : 1;
  std::vector<gs_status> brc((size_t)o.gpus, GS_OK);
  std::vector<std::thread> bt;
  for (int d = 0; d < o.gpus; d++)
    bt.emplace_back([&, d]() {
      const int dev = o.device + d * dev_step;
      if (from_sdsl) {
        brc[d] = gs_index_open_sdsl(o.prefix.c_str(), dev, &idx.ix[d]);
        return;
      }
      /* stored suffix arrays (guidescan index --store-sa) skip the sort; a file that does not
       * belong to this text is ignored */
      brc[d] = GS_ERR_IO;
      if (std::ifstream(o.prefix + ".sa"))
        brc[d] = gs_index_open_sa((const uint8_t *)text.data(), text.size(), (o.prefix + ".sa").c_str(), dev, &idx.ix[d]);
      if (brc[d] == GS_ERR_IO || brc[d] == GS_ERR_FORMAT)
        brc[d] = gs_index_build((const uint8_t *)text.data(), text.size(), dev, &idx.ix[d]);
    });
  for (auto &th : bt) th.join();
  for (int d = 0; d < o.gpus; d++)
    if (brc[d] != GS_OK) {
      std::cerr << "error: device " << o.device + d << ": " << gs_status_string(brc[d]) << "\n";
      return false;
    }
  if (o.rna > 0 || o.dna > 0)
    for (gs_index *p : idx.ix) gs_index_set_option(p, "GS_BULGE_FORM", o.bulge_form == "seeded" ? "1" : "0");
  std::cout << "Built the forward and reverse index on " << o.gpus << " device(s) from " << o.device << " in "
            << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s\n";
  return true;
}

/* what every batch's calls take, from the options, the genome structure and the number of guides */
inline void derive_job(const options &o, size_t n_guides, enumerate_job &job) {
  for (auto &n : job.gs.names) job.names.push_back(n.c_str());
  job.cgs = gs_genome_structure{job.names.data(), job.gs.lengths.data(), (uint32_t)job.names.size()};
  job.tflags = (o.format != "csv" ? GS_TEXT_SAM : 0u) | (o.mode == "complete" ? GS_TEXT_COMPLETE : 0u) |
               (job.annot ? GS_TEXT_FEATURES : 0u);
  job.bam = o.format == "bam";
  job.encoder_gpu = o.encoder == "gpu";
  job.bgzf_gpu = o.bgzf == "gpu";
  for (size_t i = 0; i < job.gs.names.size(); i++) job.refid[job.gs.names[i]] = (int32_t)i;
  job.sflags = o.co.start ? GS_FLAG_PAM_AT_START : 0u;
  /* the PAM-pair and deep tables cost ~0.23 s per device at hg38 size (the strand tables' rotated copies, which a
   * job without them builds instead: ~0.1 s) and - since the seeding launches read them (gs_seed.hip) - save ~85 ms
   * per million guides in batches of 2^17 (3.5 against 14 ms per batch): jobs below ~1.9 M guides per device at
   * that size go without (the library's default is to build them).  Measured with bench.py's e2e row, 1 M guides:
   * 0.35 s without the tables, 0.45 s with them - the first batch's build also keeps the writer waiting.  (Until
   * round 6 the saving was 15 ms per million and the bar stood at 15 M guides.) */
  uint64_t glen = 0;
  for (uint64_t l : job.gs.lengths) glen += l;
  if ((double)n_guides / (double)o.gpus < 6e-4 * (double)glen) job.sflags |= GS_FLAG_NO_NEW_TABLES;
  job.mismatches = (uint32_t)o.mismatches;
  job.rna = (uint32_t)o.rna;
  job.dna = (uint32_t)o.dna;
  job.max_off = o.max_off;
  job.threshold = o.threshold;
  job.fmt_threads = o.fmt_threads ? o.fmt_threads : std::max(1u, std::thread::hardware_concurrency());
  /* searched, being formatted, being written: three batches in flight per device where a batch's hit lists and text are
   * small (m <= 4: ~0.2 GB), two where they are gigabytes */
  job.window = (o.mismatches <= 4 ? 3 : 2) * (size_t)o.gpus;
  for (auto &a : o.alt_pams) {
    job.alts += a;
    job.alt_lens.push_back((uint32_t)a.size());
    job.n_alt++;
  }
}

/* the file's header: the CSV / SAM header lines, or the BAM's first block (magic, the SAM header text, the reference list) */
inline void write_header(const enumerate_job &job, output_file &out) {
  char *txt = nullptr;
  size_t len = 0;
  gs_format_header(&job.cgs, job.tflags, &txt, &len);
  if (job.bam) {
    std::string hz;
    if (!bam::bgzf_append(bam::header(std::string(txt, len), job.gs.names, job.gs.lengths), hz)) out.ok = false;
    out.append(hz.data(), hz.size());
  } else {
    out.append(txt, len);
  }
  gs_free(txt);
}

/* batches of equal (L, P) in input order: the device call takes fixed-width rows */
inline void cut_batches(const options &o, size_t n_guides, enumerate_job &job) {
  for (size_t done = 0; done < n_guides;) {
    batch b;
    b.lo = done;
    size_t end = done;
    if (job.cand) { /* the concatenated stream, whatever chromosome a candidate is of */
      b.L = job.cand->L;
      b.P = job.cand->P;
      end = std::min(n_guides, done + o.batch_size);
    } else {
      const size_t L = job.kmers[done].sequence.size(), P = job.kmers[done].pam.size();
      b.L = (uint32_t)L;
      b.P = (uint32_t)P;
      b.rows = &job.kmers[done];
      while (end < job.kmers.size() && end - done < o.batch_size && job.kmers[end].sequence.size() == L &&
             job.kmers[end].pam.size() == P)
        end++;
    }
    b.hi = end;
    job.batches.push_back(std::move(b));
    done = end;
  }
}

/* --gpus N: one host thread per device pulling batches from a shared queue, output written in input order; on every
 * device the search of batch i+1 overlaps the text formatting of batch i (batch_pipeline.hpp) */
inline batch_pipeline::result run_pipeline(enumerate_job &job, const std::vector<gs_index *> &ix, output_file &out) {
  batch_pipeline::result r = batch_pipeline::run(
      job.batches.size(), (unsigned)ix.size(), job.window,
      [&](size_t bi, unsigned d) { return search_batch(job, ix[d], job.batches[bi]); },
      [&](size_t bi) { return format_batch(job, job.batches[bi]); },
      [&](size_t bi) {
        /* one writer: page-cache writes to one file serialise on the inode anyway (eight pwrite
         * threads were slower on tmpfs, 1.6 s against 1.1 s for 4.6 GB) */
        for (const text_part &pt : job.batches[bi].parts) {
          if (pt.p) out.append(pt.p, pt.n);
          out.append(pt.s.data(), pt.s.size());
        }
        release_batch(job.batches[bi]);
        return out.ok;
      });
  for (batch &b : job.batches) release_batch(b); /* of a failed run: the batches behind the failed one */
  if (job.bam && r.error.empty()) { /* the empty block that ends a BGZF file */
    std::string eof;
    bam::bgzf_eof(eof);
    out.append(eof.data(), eof.size());
  }
  return r;
}

/* the lines on stdout, the first failed batch's error, the file closed - or removed: the exit status */
inline int report(const enumerate_job &job, const batch_pipeline::result &r, size_t n_guides, double secs,
                  output_file &out) {
  if (!r.error.empty()) std::cerr << "error: " << r.error << "\n";
  std::cout << "Processed " << n_guides << " kmers in " << secs << " seconds.\n";
  std::cout << "Stages (overlapping): device " << r.s_search << " s, text formatting " << r.s_format << " s, file writes " << r.s_write
            << " s\n";
  if (job.cand && job.cand->from_file)
    std::cout << "Kmers: " << job.cand->n << " row(s) parsed on the device in " << job.batches.size() << " batch(es)\n";
  else if (job.cand)
    std::cout << "Candidates: " << job.cand->n << " guide(s) from " << job.cand->n_chr << " chromosome(s) in " << job.batches.size()
              << " batch(es)\n";
  if (job.encoder_gpu)
    std::cout << "Encoder: gpu (" << job.enc_device << " batch(es) encoded on the device, " << job.batches.size() - job.enc_device
              << " by the host encoders)\n";
  if (job.bgzf_gpu)
    std::cout << "encoder: bgzf gpu (" << job.bgzf_device << " batch(es) compressed on the device, "
              << job.batches.size() - job.bgzf_device << " by the host's zlib)\n";
  return out.finish(!r.error.empty()) ? 0 : 1;
}

/* usage: prints the command lines, returns 2 */
inline int run(int argc, char **argv, int (*usage)()) {
  options o;
  if (const int rc = parse_options(argc, argv, usage, o)) return rc;
  enumerate_job job;
  std::string text;
  bool from_sdsl = false;
  if (!load_genome(o, job.gs, text, from_sdsl)) return 1;
  annotation_set annot;
  if (!o.annotate.empty() && !read_annotation(o, job.gs, annot)) return 1;
  candidate_set cand;
  if (!(o.all_candidates ? scan_candidates(o, text, job, cand) : o.kmers == "gpu" ? read_guides_device(o, job, cand) : read_guides(o, job)))
    return 1;
  cli::index_set idx((size_t)o.gpus);
  if (!build_indexes(o, text, from_sdsl, idx)) return 1;
  text = std::string();
  if (annot.bed && !attach_annotation(o, idx.ix, annot, job)) return 1;
  if (cand.design && !select_design(o, job, cand, idx.ix[0])) return 1; /* the score phase: on the first device */
  const size_t n_guides = job.cand ? (size_t)cand.n : job.kmers.size();
  derive_job(o, n_guides, job);
  output_file out;
  if (!out.open(o.output)) return 1;
  write_header(job, out);
  cut_batches(o, n_guides, job);
  const auto t0 = std::chrono::steady_clock::now();
  const batch_pipeline::result r = run_pipeline(job, idx.ix, out);
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return report(job, r, n_guides, secs, out);
}

}  // namespace enumerate_cmd

#endif
