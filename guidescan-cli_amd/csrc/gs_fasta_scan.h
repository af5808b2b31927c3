/* gs_fasta_scan.h -- the FASTA reader's sequential core, host and device: the summary of a byte
 * range, the composition of two summaries, and the walk that counts or emits a range's kept bytes and titles once the
 * state at its two edges is known.  gs_fasta.hip runs these per lane (sixteen bytes) and per tile; gs_debug_fasta_host
 * runs them sequentially with any tile size; tools/fasta_scan_check.cpp checks them against a plain reader.
 *
 * A file is split at '\n' only; a last line without a newline is a line, a newline at the end of the file starts none.
 * A line is a title iff its first byte is '>'.  Blank = C-locale isspace.
 *   GS_FASTA_INDEX_RULES  (src/genomics/seq_io.cxx:47-63, :74-110): a non-title line keeps its bytes between its first
 *                         and its last non-blank byte, a-z folded to upper case; lines ahead of the first title count.
 *   GS_FASTA_RECORD_RULES (Bio.SeqIO.to_dict as scripts/decode_database.py:223 uses it): a non-title line behind a title
 *                         keeps its non-blank bytes as they stand.
 * So whether a byte is kept depends on its line's class, on a non-blank byte before it in the line and (index rules) on
 * one after it - each of which may lie many tiles away: a line may be longer than any tile. */
#ifndef GS_FASTA_SCAN_H
#define GS_FASTA_SCAN_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_FA_HD __host__ __device__ __forceinline__
#else
#define GS_FA_HD inline
#endif

#define GS_FA_RULES_INDEX 0u
#define GS_FA_RULES_RECORD 1u

/* the class of the line a range's last byte leaves unfinished */
#define GS_FA_INHERIT 0u /* the range holds no newline: the line is the one its left neighbour leaves */
#define GS_FA_OPEN 1u    /* the range ends in a newline: the next byte, not seen yet, begins a line and decides */
#define GS_FA_TITLE 2u
#define GS_FA_SEQ 3u

struct gs_fa_sum {
  uint64_t len;      /* bytes */
  uint64_t n_nl;     /* newlines */
  uint64_t n_titles; /* title lines that begin inside the range for certain: a '>' behind a newline of the range (a '>' as the
                        first byte is counted by the composition, once the left neighbour is known to be open) */
  uint8_t tail_cls;  /* GS_FA_* of the line behind the last newline */
  uint8_t first_gt;  /* the first byte is '>' */
  uint8_t head_nb;   /* a non-blank byte in front of the first newline (anywhere, when there is none) */
  uint8_t tail_nb;   /* a non-blank byte behind the last newline (anywhere, when there is none) */
  uint8_t pad[4];
};

GS_FA_HD bool gs_fa_blank(uint8_t b) { return b == 32u || (b >= 9u && b <= 13u); }

GS_FA_HD gs_fa_sum gs_fa_identity() {
  gs_fa_sum s;
  s.len = s.n_nl = s.n_titles = 0;
  s.tail_cls = GS_FA_INHERIT;
  s.first_gt = s.head_nb = s.tail_nb = 0;
  s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
  return s;
}
/* what stands to the left of the file's first byte: nothing, and the first byte begins a line */
GS_FA_HD gs_fa_sum gs_fa_file_start() {
  gs_fa_sum s = gs_fa_identity();
  s.tail_cls = GS_FA_OPEN;
  return s;
}

GS_FA_HD gs_fa_sum gs_fa_summarize(const uint8_t *p, uint64_t n) {
  gs_fa_sum s = gs_fa_identity();
  s.len = n;
  if (n == 0) return s;
  s.first_gt = p[0] == '>';
  uint8_t nb = 0; /* a non-blank byte since the last newline */
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t b = p[i];
    if (b == '\n') {
      if (s.n_nl == 0) s.head_nb = nb;
      s.n_nl++;
      nb = 0;
      if (i + 1 < n) {
        s.tail_cls = p[i + 1] == '>' ? GS_FA_TITLE : GS_FA_SEQ;
        s.n_titles += p[i + 1] == '>';
      } else {
        s.tail_cls = GS_FA_OPEN;
      }
    } else if (!gs_fa_blank(b)) {
      nb = 1;
    }
  }
  if (s.n_nl == 0) s.head_nb = nb;
  s.tail_nb = nb;
  return s;
}

/* the summary of a's bytes followed by b's; associative, gs_fa_identity() on either side changes nothing */
GS_FA_HD gs_fa_sum gs_fa_compose(const gs_fa_sum &a, const gs_fa_sum &b) {
  if (b.len == 0) return a;
  if (a.len == 0 && a.tail_cls == GS_FA_INHERIT) return b;
  gs_fa_sum s;
  const bool begins = a.tail_cls == GS_FA_OPEN; /* b's first byte begins a line */
  s.len = a.len + b.len;
  s.n_nl = a.n_nl + b.n_nl;
  s.n_titles = a.n_titles + b.n_titles + (begins && b.first_gt ? 1u : 0u);
  s.tail_cls = b.n_nl ? b.tail_cls : begins ? (b.first_gt ? GS_FA_TITLE : GS_FA_SEQ) : a.tail_cls;
  s.first_gt = a.len ? a.first_gt : b.first_gt;
  s.head_nb = a.n_nl ? a.head_nb : (uint8_t)(a.head_nb | b.head_nb);
  s.tail_nb = b.n_nl ? b.tail_nb : (uint8_t)(a.tail_nb | b.tail_nb);
  s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
  return s;
}

/* what a range needs from outside: from everything to its left (gs_fa_file_start() composed with the summaries before it)
 * and whether a non-blank byte follows its last byte within that byte's line */
struct gs_fa_edge {
  uint8_t cls;       /* GS_FA_OPEN, GS_FA_TITLE or GS_FA_SEQ: the line the first byte belongs to */
  uint8_t nb_before; /* that line has a non-blank byte already */
  uint8_t nb_after;  /* a non-blank byte follows the range in the line of its last byte */
  uint64_t titles, nls, kept; /* titles begun, newlines and kept bytes in front of the range */
};
GS_FA_HD gs_fa_edge gs_fa_edge_of(const gs_fa_sum &left, const gs_fa_sum &right, uint64_t kept) {
  gs_fa_edge e;
  e.cls = left.tail_cls;
  e.nb_before = left.tail_cls == GS_FA_OPEN ? 0 : left.tail_nb;
  e.nb_after = right.head_nb;
  e.titles = left.n_titles;
  e.nls = left.n_nl;
  e.kept = kept;
  return e;
}

/* One record of the table as the kernels leave it: where the title line begins and where its newline stands (the file's
 * length when it has none), the newlines and the kept bytes in front of it.  The extents follow without a walk
 * (gs_fa_extents). */
struct gs_fa_title {
  uint64_t off, end, nls, kept;
};

/* The walk over p[0, n), the bytes at file offset `base`.  E has keep(uint64_t at, uint8_t byte), title(uint64_t index,
 * uint64_t off, uint64_t nls, uint64_t kept) and title_end(uint64_t index, uint64_t end).  Returns the kept bytes of the range. */
template <class E>
GS_FA_HD uint64_t gs_fa_walk(const uint8_t *p, uint64_t n, uint64_t base, uint32_t rules, const gs_fa_edge &edge, E &emit) {
  uint32_t cls = edge.cls;
  bool nbb = edge.nb_before != 0;
  uint64_t titles = edge.titles, nls = edge.nls, kept = edge.kept;
  uint64_t i = 0;
  while (i < n) {
    if (cls == GS_FA_OPEN) {
      cls = p[i] == '>' ? GS_FA_TITLE : GS_FA_SEQ;
      nbb = false;
      if (cls == GS_FA_TITLE) emit.title(titles++, base + i, nls, kept);
    }
    uint64_t e = i, last_nb = i; /* last_nb: one past the segment's last non-blank byte */
    for (; e < n && p[e] != '\n'; e++)
      if (!gs_fa_blank(p[e])) last_nb = e + 1;
    const bool cut = e == n; /* the line goes on behind the range */
    if (cls == GS_FA_SEQ && (rules == GS_FA_RULES_INDEX || titles != 0)) {
      for (uint64_t j = i; j < e; j++) {
        const uint8_t b = p[j];
        if (!gs_fa_blank(b)) {
          nbb = true;
          emit.keep(kept++, rules == GS_FA_RULES_INDEX && b >= 'a' && b <= 'z' ? (uint8_t)(b - 32u) : b);
        } else if (rules == GS_FA_RULES_INDEX && nbb && (j < last_nb || (cut && edge.nb_after))) {
          emit.keep(kept++, b);
        }
      }
    }
    if (cut) break;
    if (cls == GS_FA_TITLE) emit.title_end(titles - 1, base + e);
    nls++;
    cls = GS_FA_OPEN;
    i = e + 1;
  }
  return kept - edge.kept;
}

struct gs_fa_count_only {
  GS_FA_HD void keep(uint64_t, uint8_t) {}
  GS_FA_HD void title(uint64_t, uint64_t, uint64_t, uint64_t) {}
  GS_FA_HD void title_end(uint64_t, uint64_t) {}
};

/* Record r's extents from the table, the file's length, its newlines and its kept bytes: the symbols are
 * text[*text_off, + *text_len); *line_len = the raw bytes between the end of the title line and the next title (or the
 * end of the file) minus the newlines among them - the sum of the lines' untrimmed lengths (seq_io.cxx:100-104) */
inline void gs_fa_extents(const gs_fa_title *t, uint64_t n, uint64_t r, uint64_t file_len, uint64_t file_nls, uint64_t file_kept,
                          uint64_t *title_len, uint64_t *text_off, uint64_t *text_len, uint64_t *line_len) {
  const uint64_t next_off = r + 1 < n ? t[r + 1].off : file_len, next_nls = r + 1 < n ? t[r + 1].nls : file_nls,
                 next_kept = r + 1 < n ? t[r + 1].kept : file_kept;
  const bool has_nl = t[r].end < file_len; /* a title that the file ends in has no newline and no lines behind it */
  *title_len = t[r].end - t[r].off;
  *text_off = t[r].kept;
  *text_len = next_kept - t[r].kept;
  *line_len = has_nl ? (next_off - (t[r].end + 1)) - (next_nls - t[r].nls - 1) : 0;
}

#endif
