/* gs_kmers_scan.h -- the kmers-file reader's sequential core, host and device: the summary of a
 * byte range, the composition of two summaries, and the walk of one line.  gs_kmersfile.hip runs these per lane and per
 * tile; gs_km_host_parse (below, host only) runs them sequentially with any tile and window size;
 * tools/kmers_scan_check.cpp checks them against cli::read_kmers itself.
 *
 * The rules are those of cli::read_kmers (host/cli_common.hpp; src/genomics/kmer.cxx:9-25), not of a CSV library:
 *   - The file splits at '\n'; a last line without a newline is a line, a newline at the end of the file starts none.  One
 *     trailing '\r' is dropped from each line.
 *   - The first line is the header, even when it is empty; a file of no bytes is "empty kmers file".  Every later line
 *     that is empty after the '\r' drop is skipped; a line of blanks is not empty.
 *   - A line splits at every ','; there is no quoting.  Each field loses its leading and trailing ' ' and '\t' only.
 *   - Header: the names id, sequence, pam, chromosome, position, sense in any order among other columns; of a name given
 *     twice the last occurrence counts; the first missing name in that order is "kmers file lacks column NAME".
 *   - A row with fewer fields than the header: "kmers row with too few columns: LINE" (the line after the '\r' drop);
 *     more fields are ignored.
 *   - position must be what strtoll(.., 10) consumes to the end of the trimmed field (C-locale blanks, an optional sign,
 *     at least one digit; a NUL byte behind the digits ends the field as it ends the C string): otherwise
 *     "kmers position is not an integer: FIELD".  The value is not used and overflow is no error.
 *   - The first failing row in file order decides; within a row too few columns comes before the position.
 *   - sense is "+" iff the trimmed field is exactly "+".
 * A line may be longer than any tile, and ids are free text. */
#ifndef GS_KMERS_SCAN_H
#define GS_KMERS_SCAN_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_KM_HD __host__ __device__ __forceinline__
#else
#define GS_KM_HD inline
#endif

#define GS_KM_WIN 16u /* bytes of one load: a window */

/* the six columns in the order cli::read_kmers asks for them */
#define GS_KM_ID 0
#define GS_KM_SEQ 1
#define GS_KM_PAM 2
#define GS_KM_CHR 3
#define GS_KM_POS 4
#define GS_KM_SENSE 5

/* what is wrong with a row / with the file (gs_kmers_report.bad_kind) */
#define GS_KM_OK 0u
#define GS_KM_FEW 1u      /* kmers row with too few columns */
#define GS_KM_POSITION 2u /* kmers position is not an integer */
#define GS_KM_EMPTY 3u    /* empty kmers file */
#define GS_KM_LACKS 4u    /* kmers file lacks column NAME */

/* ---- the summary of a byte range and its composition ---------------------------------------------------------- */
struct gs_km_sum {
  uint64_t len;  /* bytes */
  uint64_t n_nl; /* newlines */
  uint64_t open; /* 1: the range's last line is still open (its last byte is no newline) */
};
GS_KM_HD gs_km_sum gs_km_identity() {
  gs_km_sum s;
  s.len = s.n_nl = s.open = 0;
  return s;
}
GS_KM_HD gs_km_sum gs_km_summarize(const uint8_t *p, uint64_t n) {
  gs_km_sum s = gs_km_identity();
  s.len = n;
  for (uint64_t i = 0; i < n; i++) s.n_nl += p[i] == '\n';
  s.open = n && p[n - 1] != '\n';
  return s;
}
/* the summary of a's bytes followed by b's; associative, gs_km_identity() on either side changes nothing */
GS_KM_HD gs_km_sum gs_km_compose(const gs_km_sum &a, const gs_km_sum &b) {
  gs_km_sum s;
  s.len = a.len + b.len;
  s.n_nl = a.n_nl + b.n_nl;
  s.open = b.len ? b.open : a.open;
  return s;
}
/* the lines of a file with that summary */
GS_KM_HD uint64_t gs_km_lines(const gs_km_sum &whole) { return whole.n_nl + whole.open; }

/* ---- windows of sixteen bytes and the bit masks of their delimiters -------------------------------------------- */
/* Offsets are "virtual": file offset + phase, phase = the low four bits of the first byte's address, so that a window
 * that begins at a virtual multiple of 16 is one aligned 16-byte load wherever the caller's buffer begins.  Bytes outside
 * the file read as 0 (they are masked out by every user). */
GS_KM_HD void gs_km_load(const uint8_t *raw, uint64_t len, uint32_t phase, uint64_t v0, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  if ((v0 & 15u) == 0 && v0 >= phase && v0 - phase + GS_KM_WIN <= len) {
    const uint4 q = *(const uint4 *)(raw + (v0 - phase));
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    return;
  }
#endif
  w[0] = w[1] = w[2] = w[3] = 0;
  for (uint32_t j = 0; j < GS_KM_WIN; j++) {
    const uint64_t v = v0 + j;
    if (v >= phase && v - phase < len) w[j >> 2] |= (uint32_t)raw[v - phase] << (8u * (j & 3u));
  }
}
GS_KM_HD uint32_t gs_km_byte(const uint32_t w[4], uint32_t j) { return (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu; }
/* bit i = byte i of the word equals c: the exact zero-byte test on w ^ cccc, its four flags gathered by one multiply
 * (the sixteen partial products fall on sixteen different bits: no carries) */
GS_KM_HD uint32_t gs_km_eq4(uint32_t w, uint32_t c) {
  const uint32_t x = w ^ (c * 0x01010101u);
  const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
  return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}
GS_KM_HD uint32_t gs_km_eq16(const uint32_t w[4], uint32_t c) {
  return gs_km_eq4(w[0], c) | (gs_km_eq4(w[1], c) << 4) | (gs_km_eq4(w[2], c) << 8) | (gs_km_eq4(w[3], c) << 12);
}
GS_KM_HD uint32_t gs_km_bits_below(uint32_t n) { return (1u << n) - 1u; } /* n <= 16 */

/* ---- the header and the walk of one line ---------------------------------------------------------------------- */
struct gs_km_header {
  uint64_t n_cols; /* fields of the header line */
  uint64_t col[6]; /* the field that carries each of the six names */
};

/* strtoll's acceptance of the position field as a machine over its bytes, blanks at both ends included:
 * 0 blanks in front, 1 behind the sign, 2 in the digits, 3 in ' ' / '\t' behind the digits (trimmed away if the field
 * ends there), 4 a NUL behind the digits (the C string ends: accepted whatever follows), 5 refused */
GS_KM_HD uint32_t gs_km_pos_step(uint32_t st, uint32_t c) {
  const bool digit = c >= '0' && c <= '9', trimmed = c == ' ' || c == '\t';
  switch (st) {
    case 0: return digit ? 2u : (c == '+' || c == '-') ? 1u : (trimmed || (c >= 9u && c <= 13u)) ? 0u : 5u;
    case 1: return digit ? 2u : 5u;
    case 2: return digit ? 2u : c == 0 ? 4u : trimmed ? 3u : 5u;
    case 3: return trimmed ? 3u : 5u;
    default: return st;
  }
}
GS_KM_HD bool gs_km_pos_ok(uint32_t st) { return st >= 2u && st <= 4u; }

struct gs_km_line {
  uint64_t b[6], e[6]; /* the trimmed bounds (file offsets) of the five fields read; chromosome is only counted */
  uint64_t n_fields;
  uint32_t err;   /* GS_KM_OK, GS_KM_FEW or GS_KM_POSITION */
  uint32_t sense; /* 1: the sense field is "+" */
};

/* The walk of the line raw[s, e) (e: its newline or the file's end, the trailing '\r' dropped already; s < e), in windows
 * of `win` bytes (16 on the device; 1 .. 16 in the host model) that begin at virtual multiples of win.  Per window the
 * commas and the bytes that trimming leaves are two bit masks, and a field's part of the window is a run of bits: its
 * first and last kept byte are a count of trailing and of leading zeros.  Only the position field is read byte by byte,
 * out of the loaded words. */
GS_KM_HD void gs_km_walk_line(const uint8_t *raw, uint64_t len, uint32_t phase, uint32_t win, uint64_t s, uint64_t e,
                              const gs_km_header &h, gs_km_line &o) {
  for (int k = 0; k < 6; k++) o.b[k] = o.e[k] = s;
  uint32_t seen = 0, ps = 0, sense_first = 0;
  uint64_t f = 0;
  const uint64_t vs = s + phase, ve = e + phase;
  for (uint64_t v0 = vs - vs % win; v0 < ve; v0 += win) {
    uint32_t w[4];
    gs_km_load(raw, len, phase, v0, w);
    const uint32_t lo = vs > v0 ? (uint32_t)(vs - v0) : 0u, hi = ve - v0 < win ? (uint32_t)(ve - v0) : win;
    const uint32_t valid = gs_km_bits_below(hi) & ~gs_km_bits_below(lo);
    uint32_t commas = gs_km_eq16(w, ',') & valid;
    const uint32_t kept = ~(gs_km_eq16(w, ' ') | gs_km_eq16(w, '\t')) & valid;
    uint32_t cur = lo;
    for (;;) {
      const uint32_t end = commas ? (uint32_t)__builtin_ctz(commas) : hi;
      const uint32_t nb = kept & gs_km_bits_below(end) & ~gs_km_bits_below(cur);
      if (nb) {
        const uint32_t first = (uint32_t)__builtin_ctz(nb), last = 32u - (uint32_t)__builtin_clz(nb);
#define GS_KM_FIELD(K)                              \
  if (f == h.col[K]) {                              \
    if (!(seen & (1u << K))) {                      \
      o.b[K] = v0 + first - phase;                  \
      seen |= 1u << K;                              \
      if (K == GS_KM_SENSE) sense_first = gs_km_byte(w, first); \
    }                                               \
    o.e[K] = v0 + last - phase;                     \
  }
        GS_KM_FIELD(GS_KM_ID)
        GS_KM_FIELD(GS_KM_SEQ)
        GS_KM_FIELD(GS_KM_PAM)
        GS_KM_FIELD(GS_KM_POS)
        GS_KM_FIELD(GS_KM_SENSE)
#undef GS_KM_FIELD
      }
      if (f == h.col[GS_KM_POS])
        for (uint32_t j = cur; j < end; j++) ps = gs_km_pos_step(ps, gs_km_byte(w, j));
      if (!commas) break;
      commas &= commas - 1u;
      f++;
      cur = end + 1u;
    }
  }
  o.n_fields = f + 1;
  o.err = o.n_fields < h.n_cols ? GS_KM_FEW : gs_km_pos_ok(ps) ? GS_KM_OK : GS_KM_POSITION;
  o.sense = (o.e[GS_KM_SENSE] - o.b[GS_KM_SENSE] == 1 && sense_first == '+') ? 1u : 0u;
}

/* the line [s, e) that lines start at s and at next (next - 1: its newline, or one past the file's end): the '\r' drop */
GS_KM_HD uint64_t gs_km_line_end(const uint8_t *raw, uint64_t s, uint64_t next) {
  const uint64_t e = next - 1;
  return e > s && raw[e - 1] == '\r' ? e - 1 : e;
}

/* ---- host only: the header line, and the passes one after the other -------------------------------------------- */
#include <string>
#include <vector>

/* the header line (after its '\r' drop) -> h; the index of the first missing name, or -1 */
inline int gs_km_parse_header(const uint8_t *line, uint64_t n, gs_km_header &h) {
  static const char *const want[6] = {"id", "sequence", "pam", "chromosome", "position", "sense"};
  bool have[6] = {false, false, false, false, false, false};
  uint64_t f = 0, b = 0;
  for (uint64_t i = 0; i <= n; i++) {
    if (i < n && line[i] != ',') continue;
    uint64_t fb = b, fe = i;
    while (fb < fe && (line[fb] == ' ' || line[fb] == '\t')) fb++;
    while (fe > fb && (line[fe - 1] == ' ' || line[fe - 1] == '\t')) fe--;
    const std::string name((const char *)line + fb, (size_t)(fe - fb));
    for (int k = 0; k < 6; k++)
      if (name == want[k]) h.col[k] = f, have[k] = true;
    f++;
    b = i + 1;
  }
  h.n_cols = f;
  for (int k = 0; k < 6; k++)
    if (!have[k]) return k;
  return -1;
}
inline const char *gs_km_column_name(int k) {
  static const char *const want[6] = {"id", "sequence", "pam", "chromosome", "position", "sense"};
  return want[k];
}

struct gs_km_parsed {
  uint32_t bad_kind = GS_KM_OK; /* the file's or the first failing row's */
  uint64_t bad_line = 0, bad_row = 0, bad_off = 0, bad_len = 0;
  std::string bad_text;
  bool mixed = false; /* rows of several shapes, or a first row without a sequence */
  uint64_t n = 0, L = 0, P = 0, n_lines = 0;
  std::vector<uint8_t> seqs, pams, ids, sense01;
  std::vector<uint64_t> id_off;
};

/* what a failing line reports: the line itself, or its trimmed position field */
inline void gs_km_describe(const uint8_t *raw, uint64_t s, uint64_t e, const gs_km_line &ln, gs_km_parsed &out) {
  out.bad_kind = ln.err;
  out.bad_off = ln.err == GS_KM_FEW ? s : ln.b[GS_KM_POS];
  out.bad_len = ln.err == GS_KM_FEW ? e - s : ln.e[GS_KM_POS] - ln.b[GS_KM_POS];
  out.bad_text.assign((const char *)raw + out.bad_off, (size_t)out.bad_len);
}

/* The passes of gs_kmersfile.hip, sequentially: tile summaries and their scan (line starts), the line walk, the scan of
 * the id lengths with the reductions, the emit.  tile_bytes >= 1; win in 1 .. 16; phase in 0 .. 15. */
inline void gs_km_host_parse(const uint8_t *raw, uint64_t len, uint64_t tile_bytes, uint32_t win, uint32_t phase, gs_km_parsed &out) {
  out = gs_km_parsed();
  const uint64_t nt = (len + tile_bytes - 1) / tile_bytes;
  std::vector<gs_km_sum> fwd(nt + 1);
  fwd[0] = gs_km_identity();
  for (uint64_t k = 0; k < nt; k++)
    fwd[k + 1] = gs_km_compose(fwd[k], gs_km_summarize(raw + k * tile_bytes, tile_bytes < len - k * tile_bytes ? tile_bytes : len - k * tile_bytes));
  const uint64_t n_lines = gs_km_lines(fwd[nt]);
  out.n_lines = n_lines;
  if (n_lines == 0) {
    out.bad_kind = GS_KM_EMPTY;
    return;
  }
  std::vector<uint64_t> starts(n_lines + 1, 0);
  for (uint64_t k = 0; k < nt; k++) { /* a tile knows the rank of its first newline */
    uint64_t rank = fwd[k].n_nl;
    for (uint64_t i = k * tile_bytes; i < len && i < (k + 1) * tile_bytes; i++)
      if (raw[i] == '\n') starts[++rank] = i + 1;
  }
  if (fwd[nt].open) starts[n_lines] = len + 1;
  gs_km_header h;
  const uint64_t he = gs_km_line_end(raw, 0, starts[1]);
  const int missing = gs_km_parse_header(raw, he, h);
  if (missing >= 0) {
    out.bad_kind = GS_KM_LACKS;
    out.bad_text = gs_km_column_name(missing);
    return;
  }
  struct rec {
    uint64_t id_len, L, P;
    uint32_t row, sense;
  };
  std::vector<rec> recs(n_lines, rec{0, 0, 0, 0, 0});
  for (uint64_t i = 1; i < n_lines; i++) {
    const uint64_t s = starts[i], e = gs_km_line_end(raw, s, starts[i + 1]);
    if (e == s) continue;
    gs_km_line ln;
    gs_km_walk_line(raw, len, phase, win, s, e, h, ln);
    if (ln.err != GS_KM_OK) {
      out.bad_line = i;
      out.bad_row = out.n;
      gs_km_describe(raw, s, e, ln, out);
      return;
    }
    recs[i] = rec{ln.e[GS_KM_ID] - ln.b[GS_KM_ID], ln.e[GS_KM_SEQ] - ln.b[GS_KM_SEQ], ln.e[GS_KM_PAM] - ln.b[GS_KM_PAM], 1u, ln.sense};
    if (out.n == 0) out.L = recs[i].L, out.P = recs[i].P;
    out.mixed = out.mixed || recs[i].L != out.L || recs[i].P != out.P;
    out.n++;
  }
  out.mixed = out.mixed || (out.n && out.L == 0);
  if (out.mixed) return;
  out.id_off.assign(out.n + 1, 0);
  out.sense01.resize(out.n);
  out.seqs.resize(out.n * out.L);
  out.pams.resize(out.n * out.P);
  uint64_t r = 0;
  for (uint64_t i = 1; i < n_lines; i++)
    if (recs[i].row) out.id_off[r + 1] = out.id_off[r] + recs[i].id_len, r++;
  out.ids.resize(out.id_off[out.n]);
  r = 0;
  for (uint64_t i = 1; i < n_lines; i++) {
    if (!recs[i].row) continue;
    const uint64_t s = starts[i], e = gs_km_line_end(raw, s, starts[i + 1]);
    gs_km_line ln;
    gs_km_walk_line(raw, len, phase, win, s, e, h, ln);
    for (uint64_t j = 0; j < out.L; j++) out.seqs[r * out.L + j] = raw[ln.b[GS_KM_SEQ] + j];
    for (uint64_t j = 0; j < out.P; j++) out.pams[r * out.P + j] = raw[ln.b[GS_KM_PAM] + j];
    for (uint64_t j = 0; j < recs[i].id_len; j++) out.ids[out.id_off[r] + j] = raw[ln.b[GS_KM_ID] + j];
    out.sense01[r] = (uint8_t)ln.sense;
    r++;
  }
}

#endif
