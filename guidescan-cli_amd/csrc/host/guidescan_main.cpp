/*
 * guidescan_main.cpp -- C++ host that keeps guidescan's `index` / `enumerate` command line
 * (src/guidescan.cxx:28-95, 316-358) and database output, and calls the MI355X path through the
 * C-ABI (include/guidescan_amd.h).  Control plane only: no search logic lives here.
 *
 *   guidescan index  [--index PREFIX] [--store-sa] [--sdsl] [--device D] GENOME.fa
 *       writes PREFIX.gs (chromosome names/lengths, src/genomics/seq_io.cxx:112-122) and
 *       PREFIX.dna (= the reference's <fasta>.forward.dna: upper-cased concatenated sequence,
 *       seq_io.cxx:57-63).  The FM-index itself is built on the GPU when `enumerate` starts
 *       (~25 s at hg38 size, about what the reference needs to load its index files).
 *       --sdsl: builds the index on the GPU now and also writes PREFIX.forward / PREFIX.reverse, the reference's
 *       own index files (src/guidescan.cxx:168-175), byte for byte what its `index` command writes: the
 *       reference binary opens them, and so does `enumerate` here when PREFIX.dna is absent.
 *   guidescan kmers PREFIX -o KMERS.csv [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S] [--start]
 *       [--chromosomes a,b,...] [--device D]
 *       the kmers file of every candidate guide of the indexed genome, byte for byte what the reference's
 *       scripts/generate_kmers.py prints for the FASTA: PREFIX.gs cuts PREFIX.dna into chromosomes, each is scanned
 *       and its rows are encoded on the device (gs_kmers_generate, gs_kmers_csv).  --chromosomes: these only.
 *   guidescan enumerate PREFIX (-f KMERS.csv | --all-candidates) -o OUT [-m 3] [-a PAM ...] [--format csv|sam|bam]
 *       [--mode succinct|complete] [--max-off-targets N] [--start] [--device D] [--gpus N] [--batch-size B]
 *       --all-candidates [--pam ...] [--kmer-length ...] [--min-chr-length ...] [--prefix ...] [--chromosomes ...]:
 *       the guides are the candidates `guidescan kmers` would write with the same options, and OUT is the file
 *       `enumerate -f` writes for that kmers file.  With --encoder gpu on one device the candidates, their ids and
 *       senses stay in HBM from the scan to the text (gs_enumerate_text_device); any other batch is copied to the
 *       host and takes the route of a kmers file's batch.
 *       --format bam --bgzf gpu: batches that are all fast path leave the device as BGZF members (BAM records and
 *       deflate made in HBM: gs_enumerate_text with GS_TEXT_BAM | GS_TEXT_BGZF); any other batch, and every batch
 *       under the default --bgzf host, takes bam_writer.hpp's records and zlib.  Same records either way.
 *       --gpus N: one index per device (devices D .. D+N-1), one host thread per device pulling batches
 *       from a shared queue, output written in input order (src/guidescan.cxx:226-251 is the
 *       reference's fan-out over threads).  On every device the search of batch i+1 overlaps the text
 *       formatting of batch i.
 *   guidescan decode [--mode succinct|complete] [--device D] [-o OUT] [--batch-size RECORDS] DATABASE GENOME.fa
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
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "guidescan_amd.h"
#include "bam_writer.hpp"
#include "decode_cmd.hpp"

namespace {

struct genome_structure {
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
};

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
      const size_t sp = line.find(' ');
      gs.names.push_back(line.substr(1, sp == std::string::npos ? std::string::npos : sp - 1));
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

bool write_gs(const std::string &path, const genome_structure &gs) {
  std::ofstream out(path);
  if (!out) return false;
  for (size_t i = 0; i < gs.names.size(); i++) out << gs.names[i] << "\n" << gs.lengths[i] << "\n";
  return (bool)out;
}
bool read_gs(const std::string &path, genome_structure &gs, std::string &err) { /* seq_io.cxx:124-144 */
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

/* what the candidate scan takes (scripts/generate_kmers.py:14-47) */
struct candidate_opts {
  std::string pam = "NGG", prefix;
  long long k = 20, min_chr = 0;
  bool start = false, have_chromosomes = false;
  std::vector<std::string> chromosomes;
};
std::vector<std::string> split_commas(const std::string &v) {
  std::vector<std::string> out;
  std::stringstream ss(v);
  std::string f;
  while (std::getline(ss, f, ',')) out.push_back(f);
  return out;
}
bool read_file(const std::string &path, std::string &text) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in) return false;
  text.resize((size_t)in.tellg());
  in.seekg(0);
  in.read(&text[0], (std::streamsize)text.size());
  return (bool)in;
}
/* the chromosomes a candidate scan takes, in .gs order, and where each begins in the .dna text */
bool select_chromosomes(const std::string &prefix, const genome_structure &gs, uint64_t dna_size, const candidate_opts &co,
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
bool candidate_option(const std::string &a, int &i, int argc, char **argv, candidate_opts &co, bool &bad) {
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

struct kmer_row {
  std::string id, sequence, pam, chromosome, sense;
  long long position;
};

std::string trim_field(const std::string &s) { /* include/csv.hpp:1110-1116: ' ' and '\t' */
  size_t b = 0, e = s.size();
  while (b < e && (s[b] == ' ' || s[b] == '\t')) b++;
  while (e > b && (s[e - 1] == ' ' || s[e - 1] == '\t')) e--;
  return s.substr(b, e - b);
}
std::vector<std::string> split_csv(const std::string &line) {
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
/* src/genomics/kmer.cxx:9-25 */
bool read_kmers(const std::string &path, std::vector<kmer_row> &rows, std::string &err) {
  std::ifstream in(path);
  if (!in) {
    err = "cannot open kmers file";
    return false;
  }
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

/* --bulge-form's default.  Measured at hg38 size (profiles/bulge_seeded.json): 4,096 guides at -m 1 with one
 * bulge of each kind take the walk 0.22 s and the seeded form 1.10 s at best, so the walk stays the default */
static const char *const BULGE_FORM_DEFAULT = "walk";

int usage() {
  std::cerr << "usage: guidescan index [--index PREFIX] [--store-sa] [--sdsl] [--device D] GENOME.fa\n"
               "       guidescan kmers PREFIX -o KMERS [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S]\n"
               "                 [--start] [--chromosomes a,b,...] [--device D]\n"
               "       guidescan enumerate PREFIX (-f KMERS | --all-candidates) -o OUT [-m N] [-a PAM]... [--format csv|sam|bam]\n"
               "                 [--mode succinct|complete] [--max-off-targets N] [--start]\n"
               "                 [--rna-bulges N] [--dna-bulges N] [--bulge-form walk|seeded] [-t THRESHOLD] [-n FORMAT_THREADS]\n"
               "                 [--device D] [--gpus N] [--batch-size B] [--encoder host|gpu] [--bgzf host|gpu]\n"
               "                 with --all-candidates: [--pam NGG] [--kmer-length 20] [--min-chr-length 0] [--prefix S]\n"
               "                 [--chromosomes a,b,...]\n"
               "       guidescan decode [--mode succinct|complete] [--device D] [-o OUT] [--batch-size RECORDS] [--verbose]\n"
               "                 DATABASE GENOME.fa\n"
               "                 a stored guide (SEQ) may have at most 32 symbols.  The table streams: without -o the header\n"
               "                 and the rows of earlier batches are on stdout already when a later record fails (exit\n"
               "                 status 1); with -o a failure leaves no file.\n";
  return 2;
}

int do_index(int argc, char **argv) {
  std::string fasta, prefix;
  bool store_sa = false, sdsl = false;
  int device = 0;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--index" && i + 1 < argc)
      prefix = argv[++i];
    else if (a == "--store-sa")
      store_sa = true;
    else if (a == "--sdsl")
      sdsl = true;
    else if (a == "--device" && i + 1 < argc)
      device = atoi(argv[++i]);
    else if (!a.empty() && a[0] != '-')
      fasta = a;
    else
      return usage();
  }
  if (fasta.empty()) return usage();
  if (prefix.empty()) prefix = fasta + ".index"; /* src/guidescan.cxx:112-117 */
  std::string text;
  genome_structure gs;
  if (!parse_fasta(fasta, text, gs)) {
    std::cerr << "error: cannot read " << fasta << "\n";
    return 1;
  }
  if (!write_gs(prefix + ".gs", gs)) {
    std::cerr << "error: cannot write " << prefix << ".gs\n";
    return 1;
  }
  std::ofstream dna(prefix + ".dna", std::ios::binary);
  dna.write(text.data(), (std::streamsize)text.size());
  if (!dna) {
    std::cerr << "error: cannot write " << prefix << ".dna\n";
    return 1;
  }
  std::cout << "Wrote " << prefix << ".gs and " << prefix << ".dna (" << text.size() << " bases, "
            << gs.names.size() << " sequences)\n";
  if (store_sa || sdsl) {
    /* the part of the index worth storing: both suffix arrays (built on the GPU now), so that
     * `enumerate` skips the sort; 8 bytes per base on disk (--store-sa) - or the reference's own
     * index files, about half a byte per base and strand (--sdsl) */
    gs_index *ix = nullptr;
    gs_status rc = gs_index_build((const uint8_t *)text.data(), text.size(), device, &ix);
    if (rc == GS_OK && store_sa) rc = gs_index_save_sa(ix, (const uint8_t *)text.data(), text.size(), (prefix + ".sa").c_str());
    if (rc == GS_OK && sdsl) rc = gs_index_save_sdsl(ix, (const uint8_t *)text.data(), text.size(), prefix.c_str());
    if (ix) gs_index_close(ix);
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
  std::string prefix, output;
  candidate_opts co;
  int device = 0;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    bool bad = false;
    if (candidate_option(a, i, argc, argv, co, bad)) {
      if (bad) return 2;
    } else if ((a == "-o" || a == "--output") && i + 1 < argc)
      output = argv[++i];
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
  for (size_t c : sel) {
    auto t1 = std::chrono::steady_clock::now();
    gs_kmers *km = nullptr;
    rc = gs_kmers_generate(device, (const uint8_t *)text.data() + begin[c], gs.lengths[c], 0, co.pam.c_str(), (uint32_t)co.k,
                           co.start ? GS_FLAG_PAM_AT_START : 0u, nullptr, &km);
    if (rc != GS_OK) break;
    auto t2 = std::chrono::steady_clock::now();
    s_scan += std::chrono::duration<double>(t2 - t1).count();
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
  std::cout << "Stages: scan " << s_scan << " s, rows " << s_rows << " s, file writes " << s_write << " s\n";
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
  std::string error;
  bool handed = false; /* a device thread took it (set under enumerate_job::mtx) */
  bool ready = false;
};

/* --all-candidates: every candidate of the selected chromosomes in one stream in HBM (gs_kmers_concat), ids included;
 * host copies only when a batch takes the host route */
struct candidate_set {
  gs_kmers *all = nullptr;
  uint64_t n = 0;
  size_t n_chr = 0;
  uint32_t L = 0, P = 0;
  const char *d_seqs = nullptr, *d_pams = nullptr, *d_ids = nullptr, *d_sense = nullptr;
  const uint64_t *d_id_off = nullptr;
  std::mutex mtx;
  bool on_host = false;
  std::string host_error;
  const char *h_seqs = nullptr, *h_pams = nullptr, *h_ids = nullptr;
  const uint8_t *h_sense = nullptr;
  const uint64_t *h_id_off = nullptr;
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
  std::mutex mtx;
  std::condition_variable cv;
  size_t next_batch = 0;   /* work queue of the device threads */
  size_t in_flight = 0;    /* searched but not yet written: bounds the host memory held by results */
  size_t max_in_flight = 2;
  double s_device = 0, s_format = 0, s_write = 0; /* seconds spent per stage (stages overlap) */
  /* --format bam: the SAM lines of the encoder, turned into BAM records and BGZF blocks by the formatting
   * threads (bam_writer.hpp; the reference leaves that step to `samtools view -b`, manual/manual.tex:581-582) */
  bool bam = false;
  std::map<std::string, int32_t> refid;
  /* --encoder gpu: a batch that is all fast path leaves the device as text (gs_enumerate_text: search, scoring and the
   * CSV / SAM encoder in HBM), any other batch - and one that answers GS_ERR_UNSUPPORTED - takes the host encoders */
  bool encoder_gpu = false;
  size_t enc_device = 0; /* batches the device encoded (under mtx); every other batch went to the host encoders */
  /* --bgzf gpu (with --format bam): a batch that is all fast path leaves the device as BGZF members (gs_enumerate_text with
   * GS_TEXT_BAM | GS_TEXT_BGZF: search, scoring, the record encoder and the compressor in HBM); any other batch takes the
   * host's records and zlib.  Members are independent, so the file is one BAM either way. */
  bool bgzf_gpu = false;
  size_t bgzf_device = 0; /* batches the device compressed (under mtx) */
  uint32_t text_flags() const { return bgzf_gpu ? (tflags & ~GS_TEXT_SAM) | GS_TEXT_BAM | GS_TEXT_BGZF : tflags; }
};

/* a part's SAM text -> BGZF-compressed BAM records (in place: the text is released) */
static bool part_to_bam(const enumerate_job &job, text_part &part) {
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

/* text of one batch from its hit lists: contiguous guide ranges formatted in parallel */
static void format_batch(enumerate_job &job, batch &b) {
  const size_t n = b.hi - b.lo;
  if (b.text_done) {
    /* the text is there.  CSV / SAM: it goes to the writer as it is.  BAM: split at the line ends where the host
     * path's guide ranges end - BGZF blocks start anew with every part, so the parts must be the same ones - and turned
     * into records by the formatting threads. */
    unsigned nt = job.bam ? job.fmt_threads : 1;
    if (nt < 1) nt = 1;
    if (nt > n) nt = (unsigned)n;
    if (b.text_members) nt = 1;
    b.parts.assign(nt, text_part());
    if (!job.bam || b.text_members) {
      b.parts[0].p = b.text;
      b.parts[0].n = (size_t)b.text_len;
      b.text = nullptr;
      return;
    }
    /* part t begins where guide n t / nt begins (gs_index_last_text_offsets, taken when the text was) */
    std::vector<size_t> cut(nt + 1, (size_t)b.text_len);
    for (unsigned t = 0; t <= nt; t++) cut[t] = (size_t)b.text_goff[n * t / nt];
    std::vector<char> okp(nt, 1);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++)
      pool.emplace_back([&, t]() {
        std::string raw;
        okp[t] = bam::records(b.text + cut[t], cut[t + 1] - cut[t], job.refid, raw) && bam::bgzf_append(raw, b.parts[t].s);
      });
    for (auto &th : pool) th.join();
    for (unsigned t = 0; t < nt; t++)
      if (!okp[t] && b.error.empty()) b.error = gs_status_string(GS_ERR_FORMAT);
    gs_free(b.text);
    b.text = nullptr;
    return;
  }
  gs_result_view v;
  memset(&v, 0, sizeof v);
  if (b.res) gs_result_get(b.res, &v);
  const uint64_t *xoff = nullptr;
  const gs_hit_ex *xhits = nullptr;
  if (b.resx) gs_result_ex_get(b.resx, nullptr, &xoff, &xhits);
  unsigned nt = job.fmt_threads;
  if (nt < 1) nt = 1;
  if (nt > n) nt = (unsigned)n;
  b.parts.assign(nt, text_part());
  std::vector<gs_status> prc(nt, GS_OK);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nt; t++) {
    pool.emplace_back([&, t]() {
      const size_t lo = n * t / nt, hi = n * (t + 1) / nt;
      text_part &part = b.parts[t];
      if (b.gen_of.empty() && !b.resx) {
        /* the whole range in one buffer, rows written in place (no per-hit strings) */
        std::vector<gs_kmer> ck(hi - lo);
        for (size_t g = lo; g < hi; g++) {
          const kmer_row &k = b.rows[g];
          ck[g - lo] = gs_kmer{k.id.c_str(), k.sequence.c_str(), k.pam.c_str(), k.sense == "+" ? 1 : 0};
        }
        prc[t] = gs_format_guides_scored(&job.cgs, ck.data(), hi - lo, v.guide_offsets + lo, v.hits, b.spec.data() + lo,
                                         b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data() + lo, job.mismatches,
                                         job.tflags | job.sflags, job.max_off, &part.p, &part.n);
        if (prc[t] == GS_OK && job.bam && !part_to_bam(job, part)) prc[t] = GS_ERR_FORMAT;
        return;
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
          r = gs_format_guide_scored(&job.cgs, &ck, v.hits + s0, s1 - s0, job.mismatches, job.tflags | job.sflags,
                                     job.max_off, b.spec[g], &tx, &tl);
        } else {
          const uint64_t s0 = xoff[gx], s1 = xoff[gx + 1];
          r = gs_format_guide_ex(&job.cgs, &ck, xhits + s0, s1 - s0, job.mismatches, job.tflags | job.sflags,
                                 job.max_off, &tx, &tl);
        }
        if (r != GS_OK) {
          prc[t] = r;
          return;
        }
        part.s.append(tx, tl);
        gs_free(tx);
      }
      if (job.bam && !part_to_bam(job, part)) prc[t] = GS_ERR_FORMAT;
    });
  }
  for (auto &th : pool) th.join();
  for (unsigned t = 0; t < nt; t++)
    if (prc[t] != GS_OK && b.error.empty()) b.error = gs_status_string(prc[t]);
  if (b.res) gs_result_free(b.res);
  if (b.resx) gs_result_ex_free(b.resx);
  b.res = nullptr;
  b.resx = nullptr;
  b.spec = std::vector<float>();
}

/* the device side of one batch: threshold filter, search (fast path; general path for the guides it
 * flags, or for all of them with bulges), scoring */
static std::string search_batch_as(enumerate_job &job, gs_index *ix, batch &b, bool all_general, gs_status &rc);
/* --all-candidates: the batch's candidates as rows on the host, for the route a kmers file's batch takes */
static std::string candidates_to_host(enumerate_job &job, batch &b) {
  candidate_set &cs = *job.cand;
  {
    std::lock_guard<std::mutex> lk(cs.mtx);
    if (!cs.on_host && cs.host_error.empty()) {
      const void *a = nullptr, *p = nullptr, *i = nullptr, *o = nullptr, *s = nullptr;
      gs_status rc = gs_kmers_get(cs.all, 0, nullptr, &a, &p, nullptr, nullptr);
      if (rc == GS_OK) rc = gs_kmers_get_ids(cs.all, 0, &i, &o, &s);
      if (rc != GS_OK) {
        cs.host_error = gs_status_string(rc);
      } else {
        cs.h_seqs = (const char *)a;
        cs.h_pams = (const char *)p;
        cs.h_ids = (const char *)i;
        cs.h_id_off = (const uint64_t *)o;
        cs.h_sense = (const uint8_t *)s;
        cs.on_host = true;
      }
    }
    if (!cs.host_error.empty()) return cs.host_error;
  }
  const size_t n = b.hi - b.lo;
  b.own.resize(n);
  b.seqs.assign(cs.h_seqs + b.lo * cs.L, n * cs.L);
  b.pams.assign(cs.h_pams + b.lo * cs.P, n * cs.P);
  for (size_t g = 0; g < n; g++) {
    kmer_row &r = b.own[g];
    const size_t at = b.lo + g;
    r.id.assign(cs.h_ids + cs.h_id_off[at], (size_t)(cs.h_id_off[at + 1] - cs.h_id_off[at]));
    r.sequence.assign(cs.h_seqs + at * cs.L, cs.L);
    r.pam.assign(cs.h_pams + at * cs.P, cs.P);
    r.sense = cs.h_sense[at] ? "+" : "-";
    r.position = 0;
  }
  b.rows = b.own.data();
  return "";
}
/* --all-candidates with --encoder gpu: the batch from HBM to text (gs_enumerate_text_device).  true: done, or failed
 * (err); false: the batch takes the host route */
static bool search_batch_device(enumerate_job &job, gs_index *ix, batch &b, std::string &err) {
  const candidate_set &cs = *job.cand;
  const size_t n = b.hi - b.lo;
  const uint32_t n_alt = cs.P ? job.n_alt : 0;
  for (uint32_t j = 0; j < n_alt; j++)
    if (job.alt_lens[j] != cs.P) return false;
  if (job.rna > 0 || job.dna > 0 || job.mismatches > 7) return false;
  const char *d_g = cs.d_seqs + b.lo * cs.L, *d_p = cs.d_pams + b.lo * cs.P;
  gs_status rc;
  if (job.threshold > 0) { /* process.hpp:66-76, as search_batch_as does it: the raw counts of a search at t mismatches */
    if (job.threshold > 7) return false;
    std::vector<uint32_t> raw(n);
    rc = gs_enumerate_text_device(ix, d_g, n, cs.L, d_p, cs.P, job.alts.data(), n_alt, (uint32_t)job.threshold,
                                  job.sflags | GS_FLAG_RAW_COUNTS, -1, &job.cgs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, raw.data());
    if (rc == GS_ERR_UNSUPPORTED) return false;
    if (rc != GS_OK) {
      err = gs_status_string(rc);
      return true;
    }
    b.skip.assign(n, 0);
    for (size_t g = 0; g < n; g++) b.skip[g] = raw[g] > 1;
  }
  rc = gs_enumerate_text_device(ix, d_g, n, cs.L, d_p, cs.P, job.alts.data(), n_alt, job.mismatches, job.sflags | job.text_flags(),
                                job.max_off, &job.cgs, cs.d_ids, cs.d_id_off + b.lo, cs.d_sense + b.lo,
                                b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data(), &b.text, &b.text_len, nullptr, nullptr);
  if (rc == GS_ERR_UNSUPPORTED) {
    b.skip.clear();
    return false;
  }
  if (rc == GS_OK && job.bam && !job.bgzf_gpu) { /* this thread alone uses the handle: the last text is still this one */
    b.text_goff.resize(n + 1);
    rc = gs_index_last_text_offsets(ix, b.text_goff.data(), n);
  }
  if (rc != GS_OK) {
    err = gs_status_string(rc);
    return true;
  }
  {
    std::lock_guard<std::mutex> lk(job.mtx);
    job.enc_device++;
    if (job.bgzf_gpu) job.bgzf_device++;
  }
  b.text_members = job.bgzf_gpu;
  b.text_done = true;
  return true;
}
static std::string search_batch(enumerate_job &job, gs_index *ix, batch &b) {
  if (job.cand) {
    std::string err;
    if (job.cand_device && search_batch_device(job, ix, b, err)) return err;
    err = candidates_to_host(job, b);
    if (!err.empty()) return err;
  }
  const uint32_t L = b.L, P = b.P;
  /* Match sequences beyond the fast path's key: up to 59 bits (23-mers with a four-symbol PAM: 58) the table-seeded
   * kernels carry them; the reference-order walk (small genomes whose table is too shallow for the context arrays)
   * stops at 52 and says GS_ERR_UNSUPPORTED - then, and beyond 59 bits, the general path carries sequences as bytes */
  const uint32_t bits = 2 * L + 3 * P;
  gs_status rc = GS_OK;
  std::string err = search_batch_as(job, ix, b, bits > 59, rc);
  if (!err.empty() && rc == GS_ERR_UNSUPPORTED && bits > 52 && bits <= 59) {
    if (b.res) gs_result_free(b.res);
    b.res = nullptr;
    b.skip.clear();
    err = search_batch_as(job, ix, b, true, rc);
  }
  return err;
}
static std::string search_batch_as(enumerate_job &job, gs_index *ix, batch &b, bool all_general, gs_status &rc) {
  const size_t n = b.hi - b.lo;
  const uint32_t L = b.L, P = b.P;
  const uint32_t n_alt = P ? job.n_alt : 0;
  const bool bulges = job.rna > 0 || job.dna > 0;
  /* an alt PAM shorter or longer than the batch's PAM: the fixed-width fast path does not take it; the
   * general path searches every pattern at its own length, as the reference does */
  bool mixed = false;
  for (uint32_t j = 0; j < n_alt; j++) mixed = mixed || job.alt_lens[j] != P;
  if (all_general) mixed = true;
  /* --threshold t (process.hpp:66-76): a guide with more than one hit within t mismatches (both
   * indexes, bulges off; counted per PAM pattern, before duplicate sequences collapse) is dropped
   * before the real search */
  if (job.threshold > 0 && mixed) {
    gs_result_ex *cx = nullptr;
    rc = gs_enumerate_general_pams(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), job.alt_lens.data(), n_alt,
                                   (uint32_t)job.threshold, 0, 0, job.sflags, &cx);
    if (rc != GS_OK) return gs_status_string(rc);
    const uint32_t *xraw = nullptr;
    gs_result_ex_raw_hits(cx, &xraw);
    b.skip.assign(n, 0);
    for (size_t g = 0; g < n; g++) b.skip[g] = xraw[g] > 1;
    gs_result_ex_free(cx);
  } else if (job.threshold > 0) {
    gs_result *cres = nullptr;
    rc = gs_enumerate(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), n_alt, (uint32_t)job.threshold,
                      job.sflags | GS_FLAG_RAW_COUNTS, &cres);
    if (rc != GS_OK) return gs_status_string(rc);
    gs_result_view cv;
    gs_result_get(cres, &cv);
    b.skip.assign(n, 0);
    /* raw counts: a site that two PAM patterns of the list match counts twice, as off_target_counter does */
    for (size_t g = 0; g < n; g++) b.skip[g] = cv.raw_hits[g] > 1;
    /* guides the fast path cannot count: through the general path (rare, exact) */
    if (cv.n_unsupported) {
      std::string s2, p2;
      std::vector<size_t> idx;
      for (size_t g = 0; g < n; g++)
        if (cv.guide_flags[g] & GS_GUIDE_NEEDS_GENERAL) {
          idx.push_back(g);
          s2.append(b.seqs, g * L, L);
          p2.append(b.pams, g * P, P);
        }
      gs_result_ex *cx = nullptr;
      rc = gs_enumerate_general(ix, s2.data(), idx.size(), L, p2.data(), P, job.alts.data(), n_alt,
                                (uint32_t)job.threshold, 0, 0, job.sflags, &cx);
      if (rc != GS_OK) {
        gs_result_free(cres);
        return gs_status_string(rc);
      }
      const uint32_t *xraw = nullptr;
      gs_result_ex_raw_hits(cx, &xraw);
      for (size_t j = 0; j < idx.size(); j++) b.skip[idx[j]] = xraw[j] > 1;
      gs_result_ex_free(cx);
    }
    gs_result_free(cres);
  }
  if (bulges || mixed) {
    /* bulge-aware search: index.hpp:250-375 behind gs_enumerate_general; alt PAMs of other lengths: the same entry */
    rc = gs_enumerate_general_pams(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), job.alt_lens.data(), n_alt,
                                   job.mismatches, job.rna, job.dna, job.sflags, &b.resx);
    if (rc != GS_OK) return gs_status_string(rc);
    b.gen_of.resize(n);
    for (size_t g = 0; g < n; g++) b.gen_of[g] = (uint32_t)g;
    return "";
  }
  if ((job.encoder_gpu || job.bgzf_gpu) && job.mismatches <= 7) {
    std::string ids;
    std::vector<uint64_t> id_off(n + 1, 0);
    std::vector<uint8_t> senses(n);
    for (size_t g = 0; g < n; g++) {
      const kmer_row &k = b.rows[g];
      ids += k.id;
      id_off[g + 1] = ids.size();
      senses[g] = k.sense == "+" ? 1 : 0;
    }
    rc = gs_enumerate_text(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), n_alt, job.mismatches,
                           job.sflags | job.text_flags(), job.max_off, &job.cgs, ids.data(), id_off.data(), senses.data(),
                           b.skip.empty() ? nullptr : (const uint8_t *)b.skip.data(), &b.text, &b.text_len, nullptr);
    {
      std::lock_guard<std::mutex> lk(job.mtx);
      if (rc == GS_OK) job.enc_device++;
      if (rc == GS_OK && job.bgzf_gpu) job.bgzf_device++;
    }
    b.text_members = rc == GS_OK && job.bgzf_gpu;
    if (rc == GS_OK && job.bam && !job.bgzf_gpu) { /* this thread alone uses the handle: the last text is still this one */
      b.text_goff.resize(n + 1);
      rc = gs_index_last_text_offsets(ix, b.text_goff.data(), n);
      if (rc != GS_OK) return gs_status_string(rc);
    }
    if (rc == GS_OK) {
      b.text_done = true;
      return "";
    }
    if (rc != GS_ERR_UNSUPPORTED) return gs_status_string(rc);
    /* a guide of the batch needs the general path: the batch is redone the usual way */
  }
  rc = gs_enumerate(ix, b.seqs.data(), n, L, b.pams.data(), P, job.alts.data(), n_alt, job.mismatches, job.sflags,
                    &b.res);
  if (rc != GS_OK) return gs_status_string(rc);
  gs_result_view v;
  gs_result_get(b.res, &v);
  if (v.n_unsupported) {
    /* guides with symbols the fast path does not encode (index.hpp:218-247): the general path, for
     * them alone; the rest of the batch is untouched */
    std::string s2, p2;
    b.gen_of.assign(n, ~0u);
    uint32_t k = 0;
    for (size_t g = 0; g < n; g++)
      if (v.guide_flags[g] & GS_GUIDE_NEEDS_GENERAL) {
        b.gen_of[g] = k++;
        s2.append(b.seqs, g * L, L);
        p2.append(b.pams, g * P, P);
      }
    rc = gs_enumerate_general(ix, s2.data(), k, L, p2.data(), P, job.alts.data(), n_alt, job.mismatches, 0, 0,
                              job.sflags, &b.resx);
    if (rc != GS_OK) return gs_status_string(rc);
  }
  /* specificity of every guide of the batch on the device (printer.hpp:98-170, 251-297 behind
   * gs_score): the formatting threads only print */
  b.spec.resize(n);
  rc = gs_score(ix, b.seqs.data(), n, L, P, job.tflags | job.sflags, job.max_off, &job.cgs, v.guide_offsets, v.hits,
                nullptr, b.spec.data());
  if (rc != GS_OK) return gs_status_string(rc);
  return "";
}

int do_enumerate(int argc, char **argv) {
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
  bool start = false, all_candidates = false, candidate_opts_given = false;
  candidate_opts co;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    bool bad = false;
    if (candidate_option(a, i, argc, argv, co, bad)) {
      if (bad) return 2;
      candidate_opts_given = true;
      continue;
    }
    auto need = [&](const char *what) -> const char * {
      if (i + 1 >= argc) {
        std::cerr << "error: " << what << " needs a value\n";
        exit(2);
      }
      return argv[++i];
    };
    if (a == "-f" || a == "--kmers-file") kmers_file = need("-f");
    else if (a == "-o" || a == "--output") output = need("-o");
    else if (a == "-m" || a == "--mismatches") mismatches = atoll(need("-m"));
    else if (a == "-a" || a == "--alt-pam") alt_pams.push_back(need("-a"));
    else if (a == "-n" || a == "--threads") fmt_threads = (unsigned)atoi(need("-n")); /* text formatting threads; the search runs on the GPU */
    else if (a == "-t" || a == "--threshold") threshold = atoll(need("-t"));
    else if (a == "--rna-bulges") rna = atoll(need("--rna-bulges"));
    else if (a == "--dna-bulges") dna = atoll(need("--dna-bulges"));
    else if (a == "--bulge-form") bulge_form = need("--bulge-form");
    else if (a == "--max-off-targets") max_off = atoll(need("--max-off-targets"));
    else if (a == "--format") format = need("--format");
    else if (a == "--mode") mode = need("--mode");
    else if (a == "--start") start = true;
    else if (a == "--all-candidates") all_candidates = true;
    else if (a == "--device") device = atoi(need("--device"));
    else if (a == "--gpus") gpus = atoi(need("--gpus"));
    else if (a == "--batch-size") batch_size = (size_t)atoll(need("--batch-size"));
    else if (a == "--encoder") encoder = need("--encoder");
    else if (a == "--bgzf") bgzf = need("--bgzf");
    else if (!a.empty() && a[0] != '-' && prefix.empty()) prefix = a;
    else return usage();
  }
  if (!prefix.empty() && !output.empty() && kmers_file.empty() == !all_candidates) {
    std::cerr << (all_candidates ? "error: -f KMERS and --all-candidates exclude each other: the guides come from the file or from the scan\n"
                                 : "error: no guides: give -f KMERS or --all-candidates\n");
    return usage();
  }
  if (prefix.empty() || output.empty()) return usage();
  if (all_candidates && co.k < 1) return usage();
  if (!all_candidates && candidate_opts_given) {
    std::cerr << "error: --pam, --kmer-length, --min-chr-length, --prefix and --chromosomes describe the scan of --all-candidates; with -f the kmers file says what the guides are\n";
    return usage();
  }
  co.start = start;
  if ((format != "csv" && format != "sam" && format != "bam") || (mode != "succinct" && mode != "complete")) return usage();
  if (gpus < 1 || mismatches < 0 || rna < 0 || dna < 0) return usage();
  if (encoder != "host" && encoder != "gpu") return usage();
  if ((bgzf != "host" && bgzf != "gpu") || (bgzf == "gpu" && format != "bam")) return usage();
  if (bulge_form != "walk" && bulge_form != "seeded") return usage();
  enumerate_job job;
  job.encoder_gpu = encoder == "gpu";
  job.bgzf_gpu = bgzf == "gpu";
  std::string err;
  if (!read_gs(prefix + ".gs", job.gs, err)) {
    std::cerr << "error: " << err << "\n";
    return 1;
  }
  /* PREFIX.dna (this tool's `index`) or, for indices made by the reference, PREFIX.forward */
  std::string text;
  bool from_sdsl = false;
  {
    std::ifstream dna_in(prefix + ".dna", std::ios::binary | std::ios::ate);
    if (dna_in) {
      text.resize((size_t)dna_in.tellg());
      dna_in.seekg(0);
      dna_in.read(&text[0], (std::streamsize)text.size());
    } else if (std::ifstream(prefix + ".forward")) {
      if (all_candidates) {
        std::cerr << "error: --all-candidates needs " << prefix << ".dna, the genome text the candidates are cut from: " << prefix
                  << " has only the .forward / .reverse index files\n";
        return 1;
      }
      from_sdsl = true;
    } else {
      std::cerr << "error: neither " << prefix << ".dna nor " << prefix << ".forward exists\n";
      return 1;
    }
  }
  candidate_set cand;
  struct cand_guard {
    candidate_set &c;
    ~cand_guard() {
      if (c.all) gs_kmers_free(c.all);
    }
  } cand_guard_{cand};
  if (all_candidates) {
    /* scan first, search afterwards: the table rule below needs the true candidate count.  Every selected chromosome
     * is scanned and its ids are encoded on `device`; one concatenation makes the stream the batches are cut from */
    const auto ts = std::chrono::steady_clock::now();
    std::vector<size_t> sel;
    std::vector<uint64_t> begin;
    if (!select_chromosomes(prefix, job.gs, text.size(), co, sel, begin, err)) {
      std::cerr << "error: " << err << "\n";
      return 1;
    }
    std::vector<gs_kmers *> parts;
    gs_status rc = GS_OK;
    for (size_t c : sel) {
      gs_kmers *km = nullptr;
      rc = gs_kmers_generate(device, (const uint8_t *)text.data() + begin[c], job.gs.lengths[c], 0, co.pam.c_str(), (uint32_t)co.k,
                             start ? GS_FLAG_PAM_AT_START : 0u, nullptr, &km);
      if (rc != GS_OK) break;
      parts.push_back(km);
      rc = gs_kmers_encode_ids(km, co.prefix.c_str(), job.gs.names[c].c_str(), nullptr);
      if (rc != GS_OK) break;
    }
    if (rc == GS_OK && parts.empty()) { /* no chromosome selected: an empty set with ids */
      gs_kmers *km = nullptr;
      rc = gs_kmers_generate(device, nullptr, 0, 0, co.pam.c_str(), (uint32_t)co.k, 0u, nullptr, &km);
      if (rc == GS_OK) {
        parts.push_back(km);
        rc = gs_kmers_encode_ids(km, "", "", nullptr);
      }
    }
    if (rc == GS_OK) rc = gs_kmers_concat(parts.data(), (uint32_t)parts.size(), &cand.all);
    for (gs_kmers *km : parts) gs_kmers_free(km);
    const void *a = nullptr, *p = nullptr, *i = nullptr, *o = nullptr, *s = nullptr;
    if (rc == GS_OK) rc = gs_kmers_get(cand.all, 1, &cand.n, &a, &p, nullptr, nullptr);
    if (rc == GS_OK) rc = gs_kmers_get_ids(cand.all, 1, &i, &o, &s);
    if (rc != GS_OK) {
      std::cerr << "error: candidate scan (--pam " << co.pam << ", --kmer-length " << co.k << "): " << gs_status_string(rc) << "\n";
      return 1;
    }
    cand.d_seqs = (const char *)a;
    cand.d_pams = (const char *)p;
    cand.d_ids = (const char *)i;
    cand.d_id_off = (const uint64_t *)o;
    cand.d_sense = (const char *)s;
    cand.n_chr = sel.size();
    cand.L = (uint32_t)co.k;
    cand.P = (uint32_t)co.pam.size();
    job.cand = &cand;
    /* 2L + 3P > 59: no batch fits the fast path's key, every one takes the host route */
    job.cand_device = (job.encoder_gpu || job.bgzf_gpu) && gpus == 1 && cand.L <= 31 && 2 * cand.L + 3 * cand.P <= 59;
    std::cout << "Scanned " << cand.n << " candidate(s) of " << sel.size() << " chromosome(s) in "
              << std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count() << " s\n";
  } else {
    if (!read_kmers(kmers_file, job.kmers, err)) {
      std::cerr << "error: " << err << "\n";
      return 1;
    }
    std::cout << "Read in " << job.kmers.size() << " kmer(s).\n";
  }
  const size_t n_guides = all_candidates ? (size_t)cand.n : job.kmers.size();

  /* one index per device, built side by side (src/guidescan.cxx:226-251 fans the guides out over
   * threads that share one index; here every GPU holds its own copy in HBM) */
  auto t0 = std::chrono::steady_clock::now();
  /* GS_CLI_SAME_DEVICE=1: every worker builds its index on `device` itself - the fan-out, the batch queue
   * and the ordered writer run with N workers on a box with one GPU (tests) */
  const int dev_step = getenv("GS_CLI_SAME_DEVICE") ? 0 : 1;
  std::vector<gs_index *> ix((size_t)gpus, nullptr);
  {
    std::vector<gs_status> brc((size_t)gpus, GS_OK);
    std::vector<std::string> bmsg((size_t)gpus);
    std::vector<std::thread> bt;
    for (int d = 0; d < gpus; d++)
      bt.emplace_back([&, d]() {
        if (from_sdsl) {
          brc[d] = gs_index_open_sdsl(prefix.c_str(), device + d * dev_step, &ix[d]);
        } else {
          /* stored suffix arrays (guidescan index --store-sa) skip the sort; a file that does not
           * belong to this text is ignored */
          brc[d] = GS_ERR_IO;
          if (std::ifstream(prefix + ".sa"))
            brc[d] = gs_index_open_sa((const uint8_t *)text.data(), text.size(), (prefix + ".sa").c_str(), device + d * dev_step, &ix[d]);
          if (brc[d] == GS_ERR_IO || brc[d] == GS_ERR_FORMAT)
            brc[d] = gs_index_build((const uint8_t *)text.data(), text.size(), device + d * dev_step, &ix[d]);
        }
        if (brc[d] != GS_OK) bmsg[d] = gs_status_string(brc[d]);
      });
    for (auto &th : bt) th.join();
    for (int d = 0; d < gpus; d++)
      if (brc[d] != GS_OK) {
        std::cerr << "error: device " << device + d << ": " << bmsg[d] << "\n";
        for (gs_index *p : ix) gs_index_close(p);
        return 1;
      }
  }
  text = std::string();
  if (rna > 0 || dna > 0)
    for (gs_index *p : ix) gs_index_set_option(p, "GS_BULGE_FORM", bulge_form == "seeded" ? "1" : "0");
  std::cout << "Built the forward and reverse index on " << gpus << " device(s) from " << device << " in "
            << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s\n";

  const int fd = open(output.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) {
    std::cerr << "error: cannot write " << output << "\n";
    return 1;
  }
  uint64_t file_off = 0;
  bool write_ok = true;
  auto pwrite_all = [&](const char *p, size_t n, uint64_t at) -> bool {
    while (n) {
      const ssize_t w = pwrite(fd, p, n, (off_t)at);
      if (w <= 0) return false;
      p += w;
      n -= (size_t)w;
      at += (uint64_t)w;
    }
    return true;
  };
  for (auto &n : job.gs.names) job.names.push_back(n.c_str());
  job.cgs = gs_genome_structure{job.names.data(), job.gs.lengths.data(), (uint32_t)job.names.size()};
  job.tflags = (format != "csv" ? GS_TEXT_SAM : 0u) | (mode == "complete" ? GS_TEXT_COMPLETE : 0u);
  job.bam = format == "bam";
  for (size_t i = 0; i < job.gs.names.size(); i++) job.refid[job.gs.names[i]] = (int32_t)i;
  job.sflags = start ? GS_FLAG_PAM_AT_START : 0u;
  {
    /* the PAM-pair and deep tables cost ~0.23 s per device at hg38 size (the strand tables' rotated copies, which a
     * job without them builds instead: ~0.1 s) and - since the seeding launches read them (gs_seed.hip) - save ~85 ms
     * per million guides in batches of 2^17 (3.5 against 14 ms per batch): jobs below ~1.9 M guides per device at
     * that size go without (the library's default is to build them).  Measured with bench.py's e2e row, 1 M guides:
     * 0.35 s without the tables, 0.45 s with them - the first batch's build also keeps the writer waiting.  (Until
     * round 6 the saving was 15 ms per million and the bar stood at 15 M guides.) */
    uint64_t glen = 0;
    for (uint64_t l : job.gs.lengths) glen += l;
    if ((double)n_guides / (double)gpus < 6e-4 * (double)glen) job.sflags |= GS_FLAG_NO_NEW_TABLES;
  }
  job.mismatches = (uint32_t)mismatches;
  job.rna = (uint32_t)rna;
  job.dna = (uint32_t)dna;
  job.max_off = max_off;
  job.threshold = threshold;
  job.fmt_threads = fmt_threads ? fmt_threads : std::max(1u, std::thread::hardware_concurrency());
  job.max_in_flight = 2 * (size_t)gpus;
  char *txt = nullptr;
  size_t len = 0;
  gs_format_header(&job.cgs, job.tflags, &txt, &len);
  if (job.bam) { /* the header block: magic, the SAM header text, the reference list */
    std::string hz;
    write_ok = bam::bgzf_append(bam::header(std::string(txt, len), job.gs.names, job.gs.lengths), hz) &&
               pwrite_all(hz.data(), hz.size(), file_off);
    file_off += hz.size();
  } else {
    write_ok = pwrite_all(txt, len, file_off);
    file_off += len;
  }
  gs_free(txt);

  /* batches of equal (L, P) in input order: the device call takes fixed-width rows.  The hit lists
   * of a batch live in HBM and on the host until it is written: ~13 hits per guide at <= 3
   * mismatches, ~1.4e3 at 5, ~1.1e4 at 6 on a human-sized genome, so deeper searches take smaller batches */
  /* At <= 3 mismatches a batch of 2^17 guides: the search is 3 ms of device time per batch at hg38 size (a million guides in
   * one batch: 17.5 ms, in eight: 24), but its 1.1 GB of text took 0.22 s to format and 0.19 s to write BEHIND the search when
   * the set was one batch - three stages that overlap only from batch to batch (bench.py's e2e_cli row: 0.60 -> 0.4 s). */
  if (!batch_size) batch_size = mismatches <= 3 ? (1u << 17) : mismatches == 4 ? (1u << 18) : mismatches == 5 ? (1u << 16) : (1u << 13);
  /* searched, being formatted, being written: three batches in flight per device where a batch's hit lists and text are
   * small (m <= 4: ~0.2 GB), two where they are gigabytes */
  if (mismatches <= 4) job.max_in_flight = 3 * (size_t)gpus;
  for (size_t done = 0; done < n_guides;) {
    batch b;
    b.lo = done;
    size_t end = done;
    if (all_candidates) { /* the concatenated stream, whatever chromosome a candidate is of */
      b.L = cand.L;
      b.P = cand.P;
      end = std::min(n_guides, done + batch_size);
    } else {
      const size_t L = job.kmers[done].sequence.size(), P = job.kmers[done].pam.size();
      b.L = (uint32_t)L;
      b.P = (uint32_t)P;
      b.rows = &job.kmers[done];
      while (end < job.kmers.size() && end - done < batch_size && job.kmers[end].sequence.size() == L &&
             job.kmers[end].pam.size() == P)
        end++;
    }
    b.hi = end;
    job.batches.push_back(std::move(b));
    done = end;
  }
  /* alt PAMs are searched whatever their length, next to each guide's own PAM (process.hpp:51-56): a batch
   * whose PAM length they all share goes through the fast path, any other through the general path */
  for (auto &a : alt_pams) {
    if (a.empty() || a.size() > 8) {
      std::cerr << "error: alt PAM " << a << ": 1 to 8 symbols\n";
      for (gs_index *p : ix) gs_index_close(p);
      return 1;
    }
    job.alts += a;
    job.alt_lens.push_back((uint32_t)a.size());
    job.n_alt++;
  }

  t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> formatters(job.batches.size());
  std::vector<std::thread> devs;
  for (int d = 0; d < gpus; d++)
    devs.emplace_back([&, d]() {
      for (;;) {
        size_t bi;
        {
          std::unique_lock<std::mutex> lk(job.mtx);
          job.cv.wait(lk, [&] { return job.in_flight < job.max_in_flight || job.next_batch >= job.batches.size(); });
          if (job.next_batch >= job.batches.size()) return;
          bi = job.next_batch++;
          job.batches[bi].handed = true;
          job.in_flight++;
        }
        batch &b = job.batches[bi];
        for (size_t g = b.lo; g < b.hi && !job.cand; g++) {
          b.seqs += job.kmers[g].sequence;
          b.pams += job.kmers[g].pam;
        }
        const auto ts = std::chrono::steady_clock::now();
        b.error = search_batch(job, ix[d], b);
        {
          std::lock_guard<std::mutex> lk(job.mtx);
          job.s_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
        }
        /* text formatting of this batch overlaps the device work of the next one.  The thread object is
         * stored under the mutex the formatter takes before it sets `ready`: the writer joins
         * formatters[bi] only after it has seen `ready`, i.e. after this assignment is complete */
        std::lock_guard<std::mutex> lk(job.mtx);
        formatters[bi] = std::thread([&job, &b]() {
          const auto tf = std::chrono::steady_clock::now();
          if (b.error.empty()) format_batch(job, b);
          std::lock_guard<std::mutex> lk2(job.mtx);
          job.s_format += std::chrono::duration<double>(std::chrono::steady_clock::now() - tf).count();
          b.ready = true;
          job.cv.notify_all();
        });
      }
    });
  int rcode = 0;
  for (size_t bi = 0; bi < job.batches.size(); bi++) {
    batch &b = job.batches[bi];
    {
      /* after an error no more batches are handed out (next_batch is moved to the end below): a batch
       * that no device thread took will never become ready, and neither will any behind it */
      std::unique_lock<std::mutex> lk(job.mtx);
      job.cv.wait(lk, [&] { return b.ready || (!b.handed && job.next_batch >= job.batches.size()); });
      if (!b.ready) break;
    }
    formatters[bi].join();
    if (!b.error.empty()) {
      if (!rcode) std::cerr << "error: " << b.error << "\n";
      rcode = 1;
    } else if (!rcode) { /* after a failed batch nothing more is written: rows behind a hole are not a database */
      const auto tw = std::chrono::steady_clock::now();
      /* one writer: page-cache writes to one file serialise on the inode anyway (eight pwrite
       * threads were slower on tmpfs, 1.6 s against 1.1 s for 4.6 GB) */
      for (const text_part &pt : b.parts) {
        if (pt.p && !pwrite_all(pt.p, pt.n, file_off)) write_ok = false;
        file_off += pt.n;
        if (!pt.s.empty() && !pwrite_all(pt.s.data(), pt.s.size(), file_off)) write_ok = false;
        file_off += pt.s.size();
      }
      job.s_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    }
    for (text_part &pt : b.parts) gs_free(pt.p);
    b.parts = std::vector<text_part>();
    b.seqs = std::string();
    b.pams = std::string();
    b.own = std::vector<kmer_row>();
    {
      std::lock_guard<std::mutex> lk(job.mtx);
      job.in_flight--;
      if (rcode) job.next_batch = job.batches.size(); /* stop handing out work */
      job.cv.notify_all();
    }
  }
  for (auto &th : devs) th.join();
  if (job.bam && !rcode) { /* the empty block that ends a BGZF file */
    std::string eof;
    bam::bgzf_eof(eof);
    if (!pwrite_all(eof.data(), eof.size(), file_off)) write_ok = false;
    file_off += eof.size();
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "Processed " << n_guides << " kmers in " << secs << " seconds.\n";
  std::cout << "Stages (overlapping): device " << job.s_device << " s, text formatting " << job.s_format
            << " s, file writes " << job.s_write << " s\n";
  if (job.cand)
    std::cout << "Candidates: " << cand.n << " guide(s) from " << cand.n_chr << " chromosome(s) in " << job.batches.size() << " batch(es)\n";
  if (job.encoder_gpu)
    std::cout << "Encoder: gpu (" << job.enc_device << " batch(es) encoded on the device, " << job.batches.size() - job.enc_device
              << " by the host encoders)\n";
  if (job.bgzf_gpu)
    std::cout << "encoder: bgzf gpu (" << job.bgzf_device << " batch(es) compressed on the device, " << job.batches.size() - job.bgzf_device
              << " by the host's zlib)\n";
  for (gs_index *p : ix) gs_index_close(p);
  /* only a regular file is ever removed: -o /dev/stdout, a FIFO or a device node stays (written through pwrite they
   * fail with ESPIPE, and unlinking them would delete the node itself) */
  struct stat fst;
  const bool regular = fstat(fd, &fst) == 0 && S_ISREG(fst.st_mode);
  if (close(fd) != 0) write_ok = false;
  if (!write_ok) std::cerr << "error: short write to " << output << "\n";
  if (rcode || !write_ok) {
    /* a run that failed leaves no file that looks like a database (CSV/SAM rows up to the failed batch, a BAM
     * without its end-of-file block) */
    if (regular && unlink(output.c_str()) == 0) std::cerr << "error: " << output << " removed (incomplete)\n";
  }
  return (write_ok && !rcode) ? 0 : 1;
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
  if (!strcmp(argv[1], "enumerate")) return do_enumerate(argc - 2, argv + 2);
  if (!strcmp(argv[1], "decode")) {
    const int rc = decode_cmd::run(argc - 2, argv + 2);
    return rc == 2 ? usage() : rc;
  }
  return usage();
}
