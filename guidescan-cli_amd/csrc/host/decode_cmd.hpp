/*
 * decode_cmd.hpp -- `guidescan decode [--mode succinct|complete] [--device D] [-o OUT] [--batch-size RECORDS] [--bgzf host|gpu]
 * [--fasta host|gpu] [--verbose] DATABASE GENOME.fa`: the CSV
 * that the reference's scripts/decode_database.py prints for a SAM/BAM off-target database (manual, "Off-Target
 * Databases"), through the device decoder (gs_decoder_open / gs_decode_sam / gs_decode_records).  Control plane only:
 * the FASTA records are read and handed over once (SeqIO.to_dict, :223), the database is read in batches of whole
 * records, so a database larger than host memory streams; the output does not depend on where the batches are cut.
 * DATABASE is SAM text, or BAM when it begins with the gzip magic: the BGZF blocks are inflated with zlib and the
 * records read per SAMv1 section 4 (@SQ from the text header, else from the binary reference list).
 * On a failure the exit status is 1, the message names the record, and an OUT file is removed.  Without -o the table
 * streams to stdout, so the header line and the rows of earlier batches have already gone out when a later batch
 * fails (usage() says so): only -o gives all or nothing.  --batch-size: records per batch (2^20; a batch also ends at 256 MB of
 * lines or hex digits).  --verbose: one line on stderr with the seconds of each stage.
 * --bgzf gpu (BAM only; on a SAM database a usage error): the BGZF members are inflated, the records found and split
 * into the decoder's arrays on the device (gs_decode_bam).  The host still reads the BAM header with bgzf_reader (header
 * text, reference list, where the first record begins); the file is then read in groups of whole members by their BSIZE
 * fields, a group of about --batch-size records (judged by the bytes per record of the groups before it; 36 bytes, the
 * least a record takes, for the first) or 256 MB of inflated bytes by the ISIZE sums.  The table is byte for byte that
 * of --bgzf host.  A damaged file ends with exit status 1 and the library's message: the member that does not inflate
 * (its index and byte offset in the file, the reason) or the record that is
 * malformed (index in the file, decode_bam_file's words).  --verbose then adds the members and bytes inflated on the device.
 * --fasta gpu: GENOME.fa is parsed on the device (gs_fasta_parse_file under GS_FASTA_RECORD_RULES: read in chunks, uploaded
 * while the next chunk is read) and its text goes to the decoder inside HBM (gs_decoder_open_fasta); read_fasta does not
 * run.  The table and the messages are those of --fasta host, with one difference: GENOME.fa must be a regular file (the
 * device buffer is sized from its length), so a pipe or a process substitution, which read_fasta takes, is "cannot read".
 * --verbose's "FASTA read" then covers file read, upload and the device stage, and a second line gives them apart.
 * --annotate BED [--features-only]: the table gains the features of a BED file in the pass that decodes it (no counterpart
 * in the reference; the rule is gs_an_decoded_footprint, gs_annot_scan.h).  The file is parsed against the database's @SQ
 * names and lengths under the rules and with the messages of `enumerate --annotate` (cli::read_bed: 1-based line and reason;
 * ';' in a group name), and its table is built and attached once, when the decoder is opened, before the first batch.
 * Complete mode gains the column match_features, succinct mode the four columns distance_k_feature_matches.
 * --features-only (complete mode, with --annotate; anything else is a usage error before any file is read): only the rows
 * that have a feature, match_number as in the full table.  Every --bgzf, --fasta, input and output choice takes it.
 */
#ifndef GS_DECODE_CMD_HPP
#define GS_DECODE_CMD_HPP

#include <time.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "guidescan_amd.h"
#include "cli_common.hpp"
#include "fasta_names.hpp"

namespace decode_cmd {

struct fasta_records { /* name (first word of the title) -> its symbols as they stand, blanks removed */
  std::string text;
  std::map<std::string, std::pair<uint64_t, uint64_t>> where;
};
/* the file is read whole and compacted where it is: title lines and blanks drop out, the symbols move up */
inline bool read_fasta(const std::string &path, fasta_records &fa, std::string &err) {
  {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) {
      err = "cannot read " + path;
      return false;
    }
    fa.text.resize((size_t)in.tellg());
    in.seekg(0);
    in.read(&fa.text[0], (std::streamsize)fa.text.size());
    if (!in) {
      err = "cannot read " + path;
      return false;
    }
  }
  std::string &t = fa.text, name;
  const size_t size = t.size();
  bool have = false;
  size_t w = 0, begin = 0;
  auto close_record = [&]() {
    if (have) fa.where[name] = {begin, w - begin};
  };
  for (size_t r = 0; r < size;) {
    const char *nl = (const char *)memchr(t.data() + r, '\n', size - r);
    const size_t end = nl ? (size_t)(nl - t.data()) : size;
    if (t[r] == '>') {
      close_record();
      size_t b, n;
      fasta_names::record_name(t.data() + r, end - r, &b, &n);
      name = t.substr(r + b, n);
      if (fa.where.count(name)) {
        err = "FASTA record '" + name + "' occurs twice in " + path;
        return false;
      }
      have = true;
      begin = w;
    } else if (have) {
      size_t e = end;
      while (e > r && isspace((unsigned char)t[e - 1])) e--;
      bool blanks = false;
      for (const char c : {' ', '\t', '\r', '\v', '\f'}) blanks = blanks || memchr(t.data() + r, c, e - r) != nullptr;
      if (!blanks) {
        memmove(&t[w], &t[r], e - r);
        w += e - r;
      } else {
        for (size_t i = r; i < e; i++)
          if (!isspace((unsigned char)t[i])) t[w++] = t[i];
      }
    }
    r = end + 1;
  }
  close_record();
  t.resize(w);
  return true;
}

struct sq_list {
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
};
/* the @SQ lines of a SAM header text */
inline void read_sq(const std::string &head, sq_list &sq) {
  size_t at = 0;
  while (at < head.size()) {
    size_t e = head.find('\n', at);
    if (e == std::string::npos) e = head.size();
    if (head.compare(at, 4, "@SQ\t") == 0) {
      std::string sn;
      uint64_t ln = 0;
      size_t f = at;
      while (f < e) {
        size_t t = head.find('\t', f);
        if (t == std::string::npos || t > e) t = e;
        size_t fe = t;
        while (fe > f && head[fe - 1] == '\r') fe--;
        if (head.compare(f, 3, "SN:") == 0) sn = head.substr(f + 3, fe - f - 3);
        if (head.compare(f, 3, "LN:") == 0) ln = strtoull(head.c_str() + f + 3, nullptr, 10);
        f = t + 1;
      }
      sq.names.push_back(sn);
      sq.lengths.push_back(ln);
    }
    at = e + 1;
  }
}

/* the inflated bytes of a BGZF file (a series of gzip members), pulled in pieces */
struct bgzf_reader {
  std::ifstream in;
  z_stream zs;
  std::vector<unsigned char> ibuf;
  bool open_ok = false, eof = false, bad = false;
  explicit bgzf_reader(const std::string &path) : in(path, std::ios::binary), ibuf(1 << 20) {
    memset(&zs, 0, sizeof zs);
    open_ok = (bool)in && inflateInit2(&zs, 15 + 32) == Z_OK;
  }
  ~bgzf_reader() {
    if (open_ok) inflateEnd(&zs);
  }
  /* n bytes, or false at the end of the data (*got: what there was) */
  bool read(void *dst, size_t n, size_t *got = nullptr) {
    zs.next_out = (Bytef *)dst;
    zs.avail_out = (uInt)n;
    while (zs.avail_out && !bad) {
      if (zs.avail_in == 0) {
        if (eof) break;
        in.read((char *)ibuf.data(), (std::streamsize)ibuf.size());
        zs.next_in = ibuf.data();
        zs.avail_in = (uInt)in.gcount();
        if (zs.avail_in == 0) {
          eof = true;
          break;
        }
      }
      const int rc = inflate(&zs, Z_NO_FLUSH);
      if (rc == Z_STREAM_END)
        inflateReset(&zs); /* the next member */
      else if (rc != Z_OK && rc != Z_BUF_ERROR)
        bad = true;
    }
    if (got) *got = n - zs.avail_out;
    return zs.avail_out == 0 && !bad;
  }
};

/* does the file end with the empty BGZF block that marks its end (SAMv1 section 4.1.2)? */
inline bool ends_with_bgzf_eof(const std::string &path) {
  static const unsigned char eof_block[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                              0x02, 0,    0x1b, 0,    3, 0, 0, 0, 0, 0,    0,    0, 0,    0};
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in || in.tellg() < 28) return false;
  unsigned char tail[28];
  in.seekg(-28, std::ios::end);
  in.read((char *)tail, 28);
  return (bool)in && !memcmp(tail, eof_block, 28);
}

struct record_batch {
  std::string ids, seqs, hex;
  std::vector<uint64_t> id_off{0}, seq_off{0}, hex_off{0};
  std::vector<uint8_t> reverse;
  std::vector<int32_t> chr;
  std::vector<int64_t> pos0;
  void clear() {
    ids.clear(), seqs.clear(), hex.clear();
    id_off.assign(1, 0), seq_off.assign(1, 0), hex_off.assign(1, 0);
    reverse.clear(), chr.clear(), pos0.clear();
  }
  size_t size() const { return chr.size(); }
};

inline double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct job {
  double t_decode = 0, t_write = 0; /* seconds in the library's calls, in the output's writes */
  gs_decoder *dec = nullptr;
  gs_fasta *gfa = nullptr; /* --fasta gpu: the parsed file, until the decoder has its text */
  uint32_t flags = 0;
  uint64_t done = 0; /* records decoded so far */
  FILE *out = nullptr;
  std::string err;
  std::string annotate;      /* --annotate BED: parsed against the database's @SQ lines when the decoder is opened */
  gs_annot *annot = nullptr; /* its table on the decoder's device; freed after the decoder is closed */
  bool reported = false;     /* the failure has been printed already (cli::read_bed prints its own) */
  /* the annotation, once, before the first batch: the rules and messages of `enumerate --annotate` */
  bool attach_annotation(int device, const cli::genome_structure &gs) {
    gs_regions *bed = nullptr;
    if (!cli::read_bed(annotate, gs, "", "annotation", &bed)) {
      reported = true;
      return false;
    }
    gs_status rc = gs_annot_build(bed, device, &annot);
    gs_regions_free(bed);
    if (rc == GS_OK) rc = gs_decoder_set_annotation(dec, annot);
    if (rc != GS_OK) {
      err = "annotation file " + annotate + ": " + gs_status_string(rc);
      return false;
    }
    return true;
  }
  bool write(const char *p, size_t n) {
    const double t0 = now_s();
    const bool ok = !n || fwrite(p, 1, n, out) == n;
    t_write += now_s() - t0;
    if (!ok) err = "cannot write the output";
    return ok;
  }
  /* the header line is the library's (gs_decode_sam of no lines): the command keeps no copy of it */
  bool write_header() {
    char *text = nullptr;
    uint64_t len = 0;
    const gs_status rc = gs_decode_sam(dec, "", 0, flags, 0, &text, &len, nullptr);
    if (rc != GS_OK) {
      err = gs_status_string(rc);
      return false;
    }
    const bool ok = write(text, len);
    gs_free(text);
    return ok;
  }
  bool flush_sam(std::string &lines) {
    if (lines.empty()) return true;
    char *text = nullptr;
    uint64_t len = 0, n = 0;
    const double t0 = now_s();
    const gs_status rc = gs_decode_sam(dec, lines.data(), lines.size(), flags | GS_DECODE_NO_HEADER, done, &text, &len, &n);
    t_decode += now_s() - t0;
    if (rc != GS_OK) {
      err = gs_status_string(rc);
      return false;
    }
    const bool ok = write(text, len);
    gs_free(text);
    done += n;
    lines.clear();
    return ok;
  }
  bool flush_records(record_batch &b) {
    if (!b.size()) return true;
    gs_decode_batch gb;
    memset(&gb, 0, sizeof gb);
    gb.n = b.size();
    gb.ids = b.ids.data();
    gb.id_off = b.id_off.data();
    gb.seqs = b.seqs.data();
    gb.seq_off = b.seq_off.data();
    gb.reverse = b.reverse.data();
    gb.chr = b.chr.data();
    gb.pos0 = b.pos0.data();
    gb.hex = b.hex.data();
    gb.hex_off = b.hex_off.data();
    char *text = nullptr;
    uint64_t len = 0;
    const double t0 = now_s();
    const gs_status rc = gs_decode_records(dec, &gb, flags, done, &text, &len, nullptr);
    t_decode += now_s() - t0;
    if (rc != GS_OK) {
      err = gs_status_string(rc);
      return false;
    }
    const bool ok = write(text, len);
    gs_free(text);
    done += b.size();
    b.clear();
    return ok;
  }
};

inline bool open_decoder(job &j, int device, const sq_list &sq, const fasta_records &fa) {
  std::vector<const char *> names;
  std::vector<uint64_t> off, len;
  for (const std::string &n : sq.names) {
    names.push_back(n.c_str());
    auto it = fa.where.find(n);
    off.push_back(it == fa.where.end() ? 0 : it->second.first);
    len.push_back(it == fa.where.end() ? ~0ull : it->second.second); /* fails only when an off-target lies on it */
  }
  gs_genome_structure gs;
  gs.chr_names = names.data();
  gs.chr_lengths = sq.lengths.data();
  gs.n_chr = (uint32_t)names.size();
  gs_status rc;
  if (j.gfa) {
    rc = gs_decoder_open_fasta(device, j.gfa, &gs, &j.dec);
    gs_fasta_free(j.gfa); /* the decoder has its own copy */
    j.gfa = nullptr;
  } else {
    rc = gs_decoder_open(device, (const uint8_t *)fa.text.data(), fa.text.size(), &gs, off.data(), len.data(), &j.dec);
  }
  if (rc != GS_OK) {
    j.err = gs_status_string(rc);
    return false;
  }
  if (!j.annotate.empty() && !j.attach_annotation(device, cli::genome_structure{sq.names, sq.lengths})) return false;
  return j.write_header();
}

inline bool decode_sam_file(job &j, const std::string &path, int device, const fasta_records &fa, uint64_t batch_records, size_t batch_bytes) {
  std::ifstream in(path, std::ios::binary);
  if (!in) {
    j.err = "cannot read " + path;
    return false;
  }
  std::string line, head, lines;
  uint64_t n_lines = 0;
  bool opened = false;
  auto ensure_open = [&]() {
    if (opened) return true;
    sq_list sq;
    read_sq(head, sq);
    opened = open_decoder(j, device, sq, fa);
    return opened;
  };
  while (std::getline(in, line)) {
    if (!opened && !line.empty() && line[0] == '@') {
      head += line;
      head += '\n';
      continue;
    }
    if (line.empty() || line[0] == '@') continue;
    if (!ensure_open()) return false;
    lines += line;
    lines += '\n';
    if (++n_lines >= batch_records || lines.size() >= batch_bytes) {
      if (!j.flush_sam(lines)) return false;
      n_lines = 0;
    }
  }
  if (!ensure_open()) return false;
  return j.flush_sam(lines);
}

/* what stands in front of a BAM file's records (SAMv1 section 4.2) */
struct bam_header {
  sq_list refs, sq;               /* the binary reference list; the @SQ lines of the text header */
  std::vector<int32_t> ref_to_sq; /* refID -> the decoder's chromosome, negative: none */
  bool from_text = false;         /* the decoder's chromosomes are the @SQ lines */
  int32_t n_ref = 0;
  uint64_t bytes = 0;             /* inflated bytes up to the first record */
};
/* -> nullptr, or what is wrong */
inline const char *read_bam_header(bgzf_reader &rd, bam_header &h) {
  sq_list &refs = h.refs, &sq = h.sq;
  std::vector<int32_t> &ref_to_sq = h.ref_to_sq;
  char magic[4];
  int32_t l_text = 0, n_ref = 0;
  if (!rd.read(magic, 4) || memcmp(magic, "BAM\1", 4) || !rd.read(&l_text, 4) || l_text < 0) return "no BAM header";
  std::string head((size_t)l_text, '\0');
  if (l_text && !rd.read(&head[0], (size_t)l_text)) return "the header text is cut";
  head.resize(strlen(head.c_str()));
  if (!rd.read(&n_ref, 4) || n_ref < 0) return "no reference list";
  h.bytes = 12ull + (uint64_t)l_text;
  for (int32_t i = 0; i < n_ref; i++) {
    int32_t l_name = 0, l_ref = 0;
    if (!rd.read(&l_name, 4) || l_name < 1) return "a reference name";
    std::string name((size_t)l_name, '\0');
    if (!rd.read(&name[0], (size_t)l_name) || !rd.read(&l_ref, 4)) return "a reference";
    name.resize(strlen(name.c_str()));
    refs.names.push_back(name);
    refs.lengths.push_back((uint64_t)(uint32_t)l_ref);
    h.bytes += 8ull + (uint64_t)l_name;
  }
  read_sq(head, sq);
  /* refID indexes the binary list; the decoder's chromosomes are the @SQ lines when the text header has them */
  const bool from_text = !sq.names.empty();
  ref_to_sq.assign((size_t)n_ref, -2);
  if (from_text) {
    std::map<std::string, int32_t> first;
    for (size_t c = 0; c < sq.names.size(); c++) first.emplace(sq.names[c], (int32_t)c);
    for (int32_t i = 0; i < n_ref; i++) {
      auto it = first.find(refs.names[(size_t)i]);
      if (it != first.end()) ref_to_sq[(size_t)i] = it->second;
    }
  } else {
    for (int32_t i = 0; i < n_ref; i++) ref_to_sq[(size_t)i] = i;
  }
  h.from_text = from_text;
  h.n_ref = n_ref;
  return nullptr;
}

inline bool decode_bam_file(job &j, const std::string &path, int device, const fasta_records &fa, uint64_t batch_records, size_t batch_bytes) {
  bgzf_reader rd(path);
  if (!rd.open_ok) {
    j.err = "cannot read " + path;
    return false;
  }
  auto malformed = [&](const char *what) {
    j.err = "malformed BAM file " + path + ": " + what;
    return false;
  };
  bam_header hd;
  if (const char *what = read_bam_header(rd, hd)) return malformed(what);
  const sq_list &refs = hd.refs, &sq = hd.sq;
  const std::vector<int32_t> &ref_to_sq = hd.ref_to_sq;
  const bool from_text = hd.from_text;
  const int32_t n_ref = hd.n_ref;
  if (!open_decoder(j, device, from_text ? sq : refs, fa)) return false;
  record_batch b;
  std::vector<unsigned char> rec;
  static const char nt16[] = "=ACMGRSVTWYHKDBN";
  for (;;) {
    int32_t block = 0;
    size_t got = 0;
    if (!rd.read(&block, 4, &got)) {
      if (got == 0 && !rd.bad) break;
      return malformed("a record's size");
    }
    if (block < 32) return malformed("a record shorter than its fixed part");
    rec.resize((size_t)block);
    if (!rd.read(rec.data(), rec.size())) return malformed("a record is cut");
    int32_t ref_id, pos, l_seq;
    uint16_t n_cigar, flag;
    memcpy(&ref_id, &rec[0], 4);
    memcpy(&pos, &rec[4], 4);
    const uint32_t l_name = rec[8];
    memcpy(&n_cigar, &rec[12], 2);
    memcpy(&flag, &rec[14], 2);
    memcpy(&l_seq, &rec[16], 4);
    size_t p = 32;
    if (l_name < 1 || l_seq < 0 || p + l_name + 4ull * n_cigar + ((size_t)l_seq + 1) / 2 + (size_t)l_seq > rec.size())
      return malformed("a record's fields outrun it");
    if (ref_id >= n_ref) return malformed("a record's reference is beyond the list");
    b.ids.append((const char *)&rec[p], l_name - 1);
    b.id_off.push_back(b.ids.size());
    p += l_name + 4ull * n_cigar;
    for (int32_t i = 0; i < l_seq; i++) b.seqs.push_back(nt16[(rec[p + (size_t)(i >> 1)] >> ((i & 1) ? 0 : 4)) & 15]);
    b.seq_off.push_back(b.seqs.size());
    p += ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
    b.reverse.push_back((flag & 16) ? 1 : 0);
    b.chr.push_back(ref_id < 0 || ref_to_sq[(size_t)ref_id] < 0 ? -1 : ref_to_sq[(size_t)ref_id]); /* no @SQ line: unmapped */
    b.pos0.push_back(pos);
    size_t hb = 0, hl = 0;
    while (p + 3 <= rec.size()) { /* the tags: the last of:H: */
      const unsigned char t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2];
      p += 3;
      size_t sz = 0;
      if (ty == 'Z' || ty == 'H') {
        const void *z = memchr(&rec[p], 0, rec.size() - p);
        if (!z) return malformed("a text tag without its end");
        sz = (size_t)((const unsigned char *)z - &rec[p]);
        if (t0 == 'o' && t1 == 'f' && ty == 'H') hb = p, hl = sz;
        sz += 1;
      } else if (ty == 'B') {
        if (p + 5 > rec.size()) return malformed("an array tag");
        const unsigned char sub = rec[p];
        int32_t cnt;
        memcpy(&cnt, &rec[p + 1], 4);
        const size_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
        sz = 5 + w * (size_t)(cnt < 0 ? 0 : cnt);
      } else {
        sz = (ty == 'A' || ty == 'c' || ty == 'C') ? 1 : (ty == 's' || ty == 'S') ? 2 : (ty == 'i' || ty == 'I' || ty == 'f') ? 4 : 0;
        if (!sz) return malformed("a tag of unknown type");
      }
      if (p + sz > rec.size()) return malformed("a tag outruns its record");
      p += sz;
    }
    b.hex.append((const char *)&rec[hb], hl);
    b.hex_off.push_back(b.hex.size());
    if (b.size() >= batch_records || b.hex.size() >= batch_bytes)
      if (!j.flush_records(b)) return false;
  }
  if (rd.bad) return malformed("a BGZF block does not inflate");
  if (!ends_with_bgzf_eof(path)) /* the records ended on a block boundary: nothing shows whether more were written (htslib warns too) */
    std::cerr << "warning: " << path << " has no BGZF end-of-file block and may be cut short\n";
  return j.flush_records(b);
}

/* the member at p, `avail` bytes there (SAMv1 section 4.1) -> its size and ISIZE; 0: it is cut; -1: no BGZF member.  The
 * library checks the members again, and in full */
inline long bgzf_member_size(const unsigned char *p, size_t avail, uint32_t *isize) {
  if (avail < 12) return 0;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return -1;
  const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
  if (12 + xlen > avail) return 0;
  for (size_t q = 12; q + 4 <= 12 + xlen;) {
    const size_t slen = (size_t)p[q + 2] | ((size_t)p[q + 3] << 8);
    if (q + 4 + slen > 12 + xlen) break;
    if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) {
      const size_t size = ((size_t)p[q + 4] | ((size_t)p[q + 5] << 8)) + 1;
      if (size < 12 + xlen + 8) return -1;
      if (size > avail) return 0;
      *isize = (uint32_t)p[size - 4] | ((uint32_t)p[size - 3] << 8) | ((uint32_t)p[size - 2] << 16) | ((uint32_t)p[size - 1] << 24);
      return (long)size;
    }
    q += 4 + slen;
  }
  return -1;
}

/* --bgzf gpu: the header on the host, then groups of whole members through gs_decode_bam */
inline bool decode_bam_file_gpu(job &j, const std::string &path, int device, const fasta_records &fa, uint64_t batch_records, size_t batch_bytes,
                                uint64_t *members, uint64_t *inflated) {
  auto malformed = [&](const char *what) {
    j.err = "malformed BAM file " + path + ": " + what;
    return false;
  };
  bam_header hd;
  {
    bgzf_reader rd(path);
    if (!rd.open_ok) {
      j.err = "cannot read " + path;
      return false;
    }
    if (const char *what = read_bam_header(rd, hd)) return malformed(what);
  }
  if (!open_decoder(j, device, hd.from_text ? hd.sq : hd.refs, fa)) return false;
  std::ifstream in(path, std::ios::binary);
  if (!in) {
    j.err = "cannot read " + path;
    return false;
  }
  std::vector<unsigned char> buf;
  size_t have = 0; /* bytes of buf that are file bytes not yet handed over */
  bool at_eof = false;
  auto fill = [&](size_t want) { /* `want` bytes in buf, or all there are */
    if (buf.size() < want) buf.resize(want + (want >> 1));
    while (have < want && !at_eof) {
      in.read((char *)buf.data() + have, (std::streamsize)(buf.size() - have));
      const size_t got = (size_t)in.gcount();
      have += got;
      if (got == 0) at_eof = true;
    }
  };
  uint64_t seen_bytes = 0, seen_records = 0; /* inflated record bytes and records of the groups so far */
  uint64_t file_at = 0;                      /* where the group begins in the file */
  bool first = true;
  for (;;) {
    /* a group: members until their ISIZE sum reaches the target; the first holds the header at least */
    const uint64_t per_record = seen_records ? (seen_bytes + seen_records - 1) / seen_records : 36;
    const uint64_t by_records = batch_records > (uint64_t)batch_bytes / per_record ? (uint64_t)batch_bytes : batch_records * per_record;
    const uint64_t target = std::min<uint64_t>(batch_bytes, by_records) + (first ? hd.bytes : 0);
    size_t glen = 0;
    uint64_t isum = 0, n_members = 0;
    for (;;) {
      fill(glen + 65536);
      if (glen == have) break; /* the end of the file */
      uint32_t isize = 0;
      const long size = bgzf_member_size(buf.data() + glen, have - glen, &isize);
      if (size < 0) return malformed("a BGZF block's header");
      if (size == 0) return malformed("a BGZF block is cut");
      glen += (size_t)size;
      isum += isize;
      n_members++;
      if (isum >= target && (!first || isum > hd.bytes)) break;
    }
    if (first && isum < hd.bytes) return malformed("the header is cut");
    if (glen == 0) break;
    fill(glen + 1);
    const bool last = glen == have;
    char *text = nullptr;
    uint64_t len = 0, n = 0, tail = 0;
    gs_bgzf_inflate_base(j.dec, *members, file_at); /* a member that fails is named by its place in the file */
    const double t0 = now_s();
    const gs_status rc = gs_decode_bam(j.dec, buf.data(), glen, first ? hd.bytes : 0, hd.ref_to_sq.data(), (uint32_t)hd.n_ref,
                                       j.flags | (last ? GS_DECODE_BAM_END : 0u), j.done, &text, &len, &n, &tail);
    j.t_decode += now_s() - t0;
    if (rc != GS_OK) {
      j.err = rc == GS_ERR_FORMAT ? "malformed BAM file " + path + ": " + gs_status_string(rc) : std::string(gs_status_string(rc));
      return false;
    }
    const bool ok = j.write(text, len);
    gs_free(text);
    if (!ok) return false;
    j.done += n;
    seen_records += n;
    seen_bytes += isum - (first ? hd.bytes : 0);
    *members += n_members;
    *inflated += isum;
    file_at += glen;
    memmove(buf.data(), buf.data() + glen, have - glen);
    have -= glen;
    first = false;
    if (last) break;
  }
  if (!ends_with_bgzf_eof(path)) /* as decode_bam_file */
    std::cerr << "warning: " << path << " has no BGZF end-of-file block and may be cut short\n";
  return true;
}

/* -> exit status; 2 = usage */
inline int run(int argc, char **argv) {
  std::string mode = "succinct", output, database, fasta, bgzf = "host", fasta_on = "host", annotate;
  int device = 0;
  bool verbose = false, features_only = false;
  long long batch_records = 1 << 20;
  std::vector<std::string> positional;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    char *end = nullptr;
    if (a == "--mode" && i + 1 < argc) {
      mode = argv[++i];
    } else if (a == "--device" && i + 1 < argc) {
      device = (int)strtol(argv[++i], &end, 10);
      if (*end || end == argv[i]) return 2;
    } else if (a == "--batch-size" && i + 1 < argc) {
      batch_records = strtoll(argv[++i], &end, 10);
      if (*end || end == argv[i] || batch_records < 1) return 2;
    } else if (a == "--bgzf" && i + 1 < argc) {
      bgzf = argv[++i];
    } else if (a == "--fasta" && i + 1 < argc) {
      fasta_on = argv[++i];
    } else if (a == "--annotate" && i + 1 < argc) {
      annotate = argv[++i];
    } else if (a == "--features-only") {
      features_only = true;
    } else if (a == "--verbose") {
      verbose = true;
    } else if (a == "-o" && i + 1 < argc) {
      output = argv[++i];
    } else if (!a.empty() && a[0] != '-') {
      positional.push_back(a);
    } else {
      return 2;
    }
  }
  if (positional.size() != 2 || (mode != "succinct" && mode != "complete") || (bgzf != "host" && bgzf != "gpu") ||
      (fasta_on != "host" && fasta_on != "gpu"))
    return 2;
  if (features_only && (annotate.empty() || mode != "complete")) { /* before any file is read */
    std::cerr << "error: --features-only leaves out the rows of --mode complete that have no feature of --annotate: give both\n";
    return 2;
  }
  database = positional[0];
  fasta = positional[1];
  job j;
  j.annotate = annotate;
  j.flags = (mode == "complete" ? GS_TEXT_COMPLETE : 0u) | (annotate.empty() ? 0u : GS_TEXT_FEATURES) |
            (features_only ? GS_DECODE_FEATURES_ONLY : 0u);
  unsigned char magic[2] = {0, 0};
  {
    std::ifstream in(database, std::ios::binary);
    if (!in) {
      std::cerr << "error: cannot read " << database << "\n";
      return 1;
    }
    in.read((char *)magic, 2);
  }
  const bool is_bam = magic[0] == 0x1f && magic[1] == 0x8b;
  if (bgzf == "gpu" && !is_bam) return 2; /* --bgzf is about BAM databases */
  const double t_start = now_s();
  fasta_records fa;
  double fasta_ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (fasta_on == "gpu") {
    const gs_status rc = gs_fasta_parse_file(device, fasta.c_str(), GS_FASTA_RECORD_RULES, &j.gfa);
    if (rc != GS_OK) { /* read_fasta's words */
      std::cerr << "error: " << gs_status_string(rc) << (rc == GS_ERR_FORMAT ? " in " + fasta : std::string()) << "\n";
      return 1;
    }
    gs_debug_fasta_ms(j.gfa, fasta_ms);
  } else if (!read_fasta(fasta, fa, j.err)) {
    std::cerr << "error: " << j.err << "\n";
    return 1;
  }
  const double t_fasta = now_s() - t_start;
  j.out = output.empty() ? stdout : fopen(output.c_str(), "wb");
  if (!j.out) {
    std::cerr << "error: cannot write " << output << "\n";
    gs_fasta_free(j.gfa);
    return 1;
  }
  const size_t batch_bytes = (size_t)256 << 20;
  uint64_t dev_members = 0, dev_inflated = 0;
  bool ok = !is_bam          ? decode_sam_file(j, database, device, fa, (uint64_t)batch_records, batch_bytes)
            : bgzf == "gpu" ? decode_bam_file_gpu(j, database, device, fa, (uint64_t)batch_records, batch_bytes, &dev_members, &dev_inflated)
                            : decode_bam_file(j, database, device, fa, (uint64_t)batch_records, batch_bytes);
  if (j.dec) gs_decoder_close(j.dec);
  gs_annot_free(j.annot); /* after the decoder it was attached to */
  gs_fasta_free(j.gfa); /* still there when the database failed before the decoder was opened */
  if (ok && fflush(j.out) != 0) {
    ok = false;
    j.err = "cannot write the output";
  }
  if (!output.empty()) fclose(j.out);
  if (!ok) {
    if (!j.reported) std::cerr << "error: " << j.err << "\n";
    if (!output.empty()) remove(output.c_str());
    return 1;
  }
  if (verbose) { /* stderr: stdout may be the table */
    const double all = now_s() - t_start;
    fprintf(stderr, "Decoded %llu records in %.3f s: FASTA read %.3f s, library calls (decoder's batches, text back) %.3f s, output writes %.3f s, "
                    "database read and decoder set-up %.3f s",
            (unsigned long long)j.done, all, t_fasta, j.t_decode, j.t_write, all - t_fasta - j.t_decode - j.t_write);
    if (bgzf == "gpu")
      fprintf(stderr, "; bgzf gpu: %llu members, %llu bytes inflated on the device", (unsigned long long)dev_members,
              (unsigned long long)dev_inflated);
    fprintf(stderr, "\n");
    if (fasta_on == "gpu")
      fprintf(stderr, "fasta gpu: file reads %.3f s, waits for the uploads %.3f s, device stage %.3f s (its five passes %.3f s), titles and names "
                      "%.3f s\n",
              1e-3 * fasta_ms[0], 1e-3 * fasta_ms[1], 1e-3 * fasta_ms[2],
              1e-3 * (fasta_ms[4] + fasta_ms[5] + fasta_ms[6] + fasta_ms[7] + fasta_ms[8]), 1e-3 * fasta_ms[3]);
  }
  return 0;
}

}  // namespace decode_cmd

#endif
