/*
 * gs_decode.hip -- an off-target database (SAM / BAM records with the hex-packed of:H: field) back to the readable CSV
 * of the reference's scripts/decode_database.py, on the device: gs_textdev.hip turned round.  Byte for byte what the
 * script prints where it prints (its lines are cited at each step); where it would raise, GS_ERR_FORMAT with the
 * first offending record and the reason, and no partial text.
 *
 * A decoder (gs_decoder, an opaque object of its own like gs_kmers: no FM-index) holds the genome's FASTA records in
 * HBM as bytes, case folded on upload (.upper(), :59), the @SQ prefix sums and names, where each @SQ chromosome's
 * record lies in the text and its OWN length (the coordinate walk uses LN, :38-50; the slice clamps at the record's
 * length, :52-59), the 240 + 16 CFD values (__constant__) and the 125-bit powers of five of the double printer.
 *
 * One batch of records (ids, stored SEQ, reverse bit, chromosome index, POS-1, hex spans; 64-bit offsets):
 *   k_dc_hex    16 hex digits -> one little-endian int64 word (:26-27), digits validated; marks the delimiters
 *   (rocPRIM)   inclusive min-scan over the reversed delimiter marks: every word's next delimiter (the segmented
 *               look-ahead; a delimiter of a later record is beyond the word's own record end and does not count)
 *   k_dc_rec    per record: hex length, SEQ length, a list that begins with the delimiter (:29-36 slices words[0:-1] then)
 *   k_dc_eval   per word: its role (position iff it is no delimiter, a delimiter follows in its record and the next
 *               word is none; its distance is the word before that delimiter), then per position the chromosome
 *               lookup, the Python slice arithmetic, a gather of <= 32 symbols, revcom, the CFD in double (:67-83,
 *               :106-127) kept per word
 *   (rocPRIM)   exclusive scan of the position marks: row slots, match_number = rank - rank at the record's first word
 *   k_dc_fold   succinct mode, a wave per record: counters per distance, and the CFDs folded strictly in list order
 *               ((0 + c0) + c1) + ... - the lanes load 64 at a time, every lane adds them one after the other (:156-187)
 *   k_dc_len / (rocPRIM scan of the tile sums) / k_dc_write   the tile composer of gs_rowtext.h (gs_tile_len, gs_tile_write:
 *               the one gs_textdev.hip uses) over dc_slot_row: a tile is 64 slots (words in complete mode, records in
 *               succinct mode), one row routine over the counting and the writing sink, the tile composed in the wave's
 *               LDS slice and streamed out in 16-byte stores.  Doubles are printed as Python's repr by gs_repr.h
 *               (integer arithmetic).
 * The error word travels back with the total length: (record << 8 | reason), the smallest over the batch.
 *
 * With an annotation attached (gs_decoder_set_annotation) and GS_TEXT_FEATURES, the rows carry the features of a BED file:
 * the rule is gs_an_decoded_footprint (gs_annot_scan.h), the table the one `enumerate --annotate` looks up.
 *   k_dc_feat   behind k_dc_eval, one lane per word: a position is placed again (chromosome and x only, no gather), its
 *               footprint looked up by two binary searches, the number of distinct groups kept per word
 *   k_dc_fold   counts, next to the counters per distance, the off-targets at that distance that have a feature
 *   k_dc_len / k_dc_write   complete mode: the row routine appends ',' and the names joined by ';', or NA, through the
 *               same two sinks; under GS_DECODE_FEATURES_ONLY a word without a feature has a row of length 0.  A lane with
 *               features walks its segments' lists while the lanes without wait: nearly every row has none or one or two
 *               groups (a footprint is about 23 bases), so the wave pays for its longest list, as it pays for its longest
 *               id or number already.  A row longer than the LDS slice takes k_dc_write's straight-to-HBM branch.
 * The script's failures are found by k_dc_hex, k_dc_rec and k_dc_eval before any row is measured, and k_dc_len gives up
 * when one is recorded: they win over a row that the annotation makes too long.
 */
#include "gs_device.h"
#include "gs_rowtext.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "cfd_table.h"
#include "gs_pow5_table.h"
#include "gs_repr.h"
#include "gs_decoder.h"
#include "gs_scratch.h"
#include "gs_annot_scan.h"
#include "gs_annot_obj.h"

#define DC_FOLD_WAVES 4 /* waves of a k_dc_fold block, a record each */
#define DC_MAX_SEQ 32u
#define DC_NONE 0xFFFFFFFFu
#define DC_ERR_HEX 1u
#define DC_ERR_WORD 2u
#define DC_ERR_PAM 3u
#define DC_ERR_DISTANCE 4u
#define DC_ERR_CHROMOSOME 5u
#define DC_ERR_LONG 6u
#define DC_ERR_RECORD 7u
#define DC_ERR_BIG 8u
#define DC_ABSENT (-1.0) /* a position without a CFD (the script's None): every CFD is >= 0 */

__constant__ double c_dc_mm[320]; /* [(r * 4 + d) * 20 + i]: r of A,C,G,U, d of A,C,G,T */
__constant__ double c_dc_pam[16];

struct dc_args {
  /* the batch */
  const uint8_t *ids, *seqs, *hex, *reverse;
  const uint64_t *id_off, *seq_off, *hex_off, *word_off;
  const int32_t *chr;
  const int64_t *pos0;
  /* the decoder */
  const uint8_t *text, *names;
  const uint64_t *cum, *toff, *flen;
  const uint32_t *name_off;
  gs_pow5_tables pw;
  /* scratch */
  int64_t *words;
  uint32_t *rec, *mark, *next, *ispos, *rank, *lens, *cnt;
  double *cfd, *spec;
  uint64_t *tile_sum, *tile_off;
  unsigned long long *err;
  char *out;
  uint64_t slots, total;
  int64_t delim;
  uint32_t n, n_words, n_chr, complete;
  /* the annotation (features != 0): its table and names; per word the number of its features, per record and distance the
   * off-targets that have one; only != 0: rows without a feature are left out */
  gs_an_table an;
  const uint32_t *an_name_off;
  const uint8_t *an_names;
  uint32_t *nfeat, *fcnt;
  uint32_t features, only;
};

/* ---- small pieces -------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t dc_comp(uint32_t c) { /* :93-97 */
  switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'U': return 'A';
    default: return c; /* N and everything else */
  }
}
__device__ __forceinline__ int dc_hexval(uint32_t c) {
  if (c >= '0' && c <= '9') return (int)(c - '0');
  c |= 0x20u;
  if (c >= 'a' && c <= 'f') return (int)(c - 'a' + 10u);
  return -1;
}
__device__ __forceinline__ void dc_fail(const dc_args &a, uint32_t r, uint32_t reason) {
  atomicMin(a.err, ((unsigned long long)r << 8) | reason);
}

/* one off-target of record r: where it lies and the symbols the script prints for it */
struct dc_site {
  uint32_t c, len;
  uint64_t x;
  char strand;
  uint8_t seq[DC_MAX_SEQ];
};
/* map_int_to_coord (:38-50): the chromosome that holds |word| and the coordinate on it -> 0 or the reason it fails */
__device__ __forceinline__ uint32_t dc_place(const dc_args &a, int64_t word, uint32_t &c, uint64_t &x) {
  const uint64_t ab = word < 0 ? 0ull - (uint64_t)word : (uint64_t)word;
  c = 0;
  x = 0;
  if (ab >= a.total) return DC_ERR_WORD;
  uint32_t lo = 0, hi = a.n_chr; /* first chromosome whose end exceeds ab: the walk `while LN <= x` */
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ab < a.cum[mid + 1u])
      hi = mid;
    else
      lo = mid + 1u;
  }
  if (lo >= a.n_chr) return DC_ERR_WORD;
  c = lo;
  x = ab - a.cum[lo];
  return 0u;
}
/* dc_place and map_coord_to_sequence (:52-59) with revcom for '-' (:135) -> 0 or the reason it fails */
__device__ __forceinline__ uint32_t dc_resolve(const dc_args &a, int64_t word, uint32_t n, dc_site &s) {
  s.strand = word > 0 ? '+' : '-';
  s.len = 0;
  if (const uint32_t bad = dc_place(a, word, s.c, s.x)) return bad;
  const uint32_t lo = s.c;
  const uint64_t fl = a.flen[lo];
  if (fl == ~0ull) return DC_ERR_CHROMOSOME;
  /* a Python slice of a sequence of fl symbols */
  const long long L = (long long)fl, x = (long long)s.x;
  long long b = s.strand == '+' ? x + 1 - (long long)n : x, e = s.strand == '+' ? x + 1 : x + (long long)n;
  if (b < 0) {
    b += L;
    if (b < 0) b = 0;
  }
  if (b > L) b = L;
  if (e > L) e = L;
  const uint32_t len = e > b ? (uint32_t)(e - b) : 0u; /* <= n */
  s.len = len;
  const uint8_t *src = a.text + a.toff[lo] + (uint64_t)b;
  if (s.strand == '+') {
    for (uint32_t i = 0; i < len; i++) s.seq[i] = src[i];
  } else {
    for (uint32_t i = 0; i < len; i++) s.seq[i] = (uint8_t)dc_comp(src[len - 1u - i]);
  }
  return 0u;
}
/* the guide as the script compares it: SEQ as stored, reverse-complemented under FLAG 16 (:117-119) */
__device__ __forceinline__ uint32_t dc_guide(const dc_args &a, uint32_t r, uint8_t *sg) {
  const uint64_t b = a.seq_off[r];
  const uint64_t stored = a.seq_off[r + 1u] - b;
  const uint32_t n = stored > DC_MAX_SEQ ? DC_MAX_SEQ : (uint32_t)stored; /* longer: k_dc_rec refuses the batch */
  if (a.reverse[r]) {
    for (uint32_t i = 0; i < n; i++) sg[i] = (uint8_t)dc_comp(a.seqs[b + n - 1u - i]);
  } else {
    for (uint32_t i = 0; i < n; i++) sg[i] = a.seqs[b + i];
  }
  return n;
}
__device__ __forceinline__ int dc_base(uint32_t c, uint32_t fourth) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == fourth ? 3 : -1; }
/* calc_cfd_e (:67-83) of a 23-symbol off-target; the products in the script's order */
__device__ __forceinline__ uint32_t dc_cfd(const uint8_t *sg, const uint8_t *seq, double &out) {
  double score = 1.0;
  for (uint32_t i = 0; i < 20u; i++) {
    const uint32_t g = sg[i] == 'T' ? 'U' : sg[i], w = seq[i] == 'T' ? 'U' : seq[i];
    if (g == w) continue;
    const int r = dc_base(g, 'U'), d = dc_base(dc_comp(w), 'T');
    if (r < 0 || d < 0) continue; /* no such key: the factor is skipped (:80-81) */
    score *= c_dc_mm[(r * 4 + d) * 20 + (int)i];
  }
  const int p1 = dc_base(seq[21], 'T'), p2 = dc_base(seq[22], 'T');
  if (p1 < 0 || p2 < 0) return DC_ERR_PAM;
  out = score * c_dc_pam[p1 * 4 + p2];
  return 0u;
}
/* a word's role: is it a position, and if so where its distance stands */
__device__ __forceinline__ bool dc_is_position(const dc_args &a, uint32_t w, uint32_t r, uint32_t &dist_at) {
  if (a.words[w] == a.delim) return false;
  const uint32_t nx = a.next[a.n_words - 1u - w]; /* the scan ran over the reversed marks */
  if (nx == DC_NONE || (uint64_t)nx >= a.word_off[r + 1u] || nx == w + 1u) return false;
  dist_at = nx - 1u;
  return true;
}

/* .upper() of the FASTA bytes where they are (:59): sixteen per lane, a-z found in all four bytes of a word at once */
__global__ __launch_bounds__(256) void k_dc_upper(uint4 *text, uint64_t n16) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) {
    uint4 v = text[i];
    uint32_t *w = &v.x;
    for (int k = 0; k < 4; k++) {
      const uint32_t x = w[k], x7 = x & 0x7F7F7F7Fu;
      const uint32_t lower = (x7 + 0x1F1F1F1Fu) & ~(x7 + 0x05050505u) & ~x & 0x80808080u; /* 0x61 <= byte <= 0x7a */
      w[k] = x - (lower >> 2);
    }
    text[i] = v;
  }
}

/* ---- the evaluation kernels ------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void k_dc_hex(dc_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint32_t lo = 0, hi = a.n; /* the last record whose first word is at or before w and that is not empty before it */
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.word_off[mid] <= w)
        lo = mid;
      else
        hi = mid;
    }
    const uint32_t r = lo;
    const uint8_t *p = a.hex + a.hex_off[r] + 16ull * (w - a.word_off[r]);
    uint64_t v = 0;
    bool ok = true;
    for (uint32_t k = 0; k < 8u; k++) {
      const int h = dc_hexval(p[2u * k]), l = dc_hexval(p[2u * k + 1u]);
      ok = ok && h >= 0 && l >= 0;
      v |= (uint64_t)(uint32_t)((h << 4) | l) << (8u * k);
    }
    if (!ok) dc_fail(a, r, DC_ERR_HEX);
    a.words[w] = (int64_t)v;
    a.rec[w] = r;
    a.mark[a.n_words - 1u - w] = (int64_t)v == a.delim ? w : DC_NONE;
  }
}

__global__ __launch_bounds__(256) void k_dc_rec(dc_args a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const uint64_t hl = a.hex_off[r + 1u] - a.hex_off[r];
  if (hl & 15ull) dc_fail(a, r, DC_ERR_HEX);
  for (uint64_t i = hl & ~15ull; i < hl; i++) /* the digits behind the last whole word */
    if (dc_hexval(a.hex[a.hex_off[r] + i]) < 0) dc_fail(a, r, DC_ERR_HEX);
  if (a.seq_off[r + 1u] - a.seq_off[r] > DC_MAX_SEQ) dc_fail(a, r, DC_ERR_LONG);
  if (a.chr[r] >= (int32_t)a.n_chr) dc_fail(a, r, DC_ERR_RECORD);
  const uint64_t w0 = a.word_off[r], w1 = a.word_off[r + 1u];
  if (w1 - w0 >= 2u && a.words[w0] == a.delim) dc_fail(a, r, DC_ERR_WORD);
}

__global__ __launch_bounds__(256) void k_dc_eval(dc_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.n_words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    if (w == a.n_words) {
      a.ispos[w] = 0u;
      continue;
    }
    const uint32_t r = a.rec[w];
    uint32_t dist_at = 0;
    const bool pos = dc_is_position(a, w, r, dist_at);
    a.ispos[w] = pos ? 1u : 0u;
    if (!pos) continue;
    double cfd = DC_ABSENT;
    if (a.seq_off[r + 1u] - a.seq_off[r] <= DC_MAX_SEQ) {
      uint8_t sg[DC_MAX_SEQ];
      const uint32_t n = dc_guide(a, r, sg);
      dc_site s;
      uint32_t bad = dc_resolve(a, a.words[w], n, s);
      if (!bad && s.len == 23u) bad = dc_cfd(sg, s.seq, cfd);
      if (bad) dc_fail(a, r, bad);
    }
    a.cfd[w] = cfd;
    if (!a.complete) {
      const int64_t d = a.words[dist_at];
      if (d < 0 || d > 3) dc_fail(a, r, DC_ERR_DISTANCE);
    }
  }
}

/* GS_TEXT_FEATURES: how many groups of the annotation every off-target touches (gs_an_decoded_footprint); the site is placed
 * again, without the gather of its symbols.  A word that is no position, or one that k_dc_eval has refused the batch for,
 * has none */
__global__ __launch_bounds__(256) void k_dc_feat(dc_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint32_t k = 0;
    if (a.ispos[w]) {
      const uint32_t r = a.rec[w];
      const uint64_t stored = a.seq_off[r + 1u] - a.seq_off[r];
      uint32_t c;
      uint64_t x;
      if (stored <= DC_MAX_SEQ && !dc_place(a, a.words[w], c, x))
        k = gs_an_decoded_count(a.an, c, x, a.words[w] > 0, (uint32_t)stored, a.cum[c + 1u] - a.cum[c]);
    }
    a.nfeat[w] = k;
  }
}

/* output_succinct (:156-187): a wave per record */
__global__ __launch_bounds__(WAVE *DC_FOLD_WAVES) void k_dc_fold(dc_args a) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  for (uint32_t r = wave0; r < a.n; r += n_waves) {
    const uint64_t w0 = a.word_off[r], w1 = a.word_off[r + 1u];
    uint32_t cnt[4] = {0, 0, 0, 0}, fcnt[4] = {0, 0, 0, 0};
    bool any = false, all_have = true, seen0 = false;
    double sum = 0.0, first0 = 0.0;
    for (uint64_t base = w0; base < w1; base += WAVE) {
      const uint64_t w = base + lane;
      bool pos = false;
      double c = 0.0;
      uint32_t d = 4u;
      if (w < w1 && a.ispos[w]) {
        uint32_t dist_at = 0;
        pos = dc_is_position(a, (uint32_t)w, r, dist_at);
        c = a.cfd[w];
        const int64_t dv = a.words[dist_at];
        d = dv >= 0 && dv <= 3 ? (uint32_t)dv : 4u; /* outside 0..3: k_dc_eval has refused the batch */
      }
      const uint64_t m = __ballot(pos);
      if (m == 0ull) continue;
      any = true;
      for (uint32_t k = 0; k < 4u; k++) cnt[k] += (uint32_t)__popcll(__ballot(pos && d == k));
      if (a.features) { /* counted as cnt is: every off-target of the list, the record's own site among them */
        const bool has = pos && a.nfeat[w] != 0u;
        for (uint32_t k = 0; k < 4u; k++) fcnt[k] += (uint32_t)__popcll(__ballot(has && d == k));
      }
      if (__ballot(pos && c == DC_ABSENT)) all_have = false;
      /* the ordered part: every lane folds the same 64 values one after the other */
      uint64_t todo = m;
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const double cl = __shfl(c, l);
        const uint32_t dl = (uint32_t)__shfl((int)d, l);
        sum = sum + cl;
        if (dl == 0u && !seen0) {
          seen0 = true;
          first0 = cl;
        }
      }
    }
    if (lane == 0u) {
      for (uint32_t k = 0; k < 4u; k++) a.cnt[(size_t)r * 4u + k] = cnt[k];
      if (a.features)
        for (uint32_t k = 0; k < 4u; k++) a.fcnt[(size_t)r * 4u + k] = fcnt[k];
      double spec = 0.0; /* 0.0: the column is empty (a specificity is never 0) */
      if (any && all_have) {
        if (seen0) sum = sum - first0;
        if (sum != 0.0) spec = 1.0 / (1.0 + sum);
      }
      a.spec[r] = spec;
    }
  }
}

/* ---- the rows: templates over the sinks of gs_rowtext.h -------------------------------------------------------- */
template <class S>
__device__ __forceinline__ void dc_i64(S &o, int64_t v) {
  if (v < 0) {
    o.ch('-');
    o.u64(0ull - (uint64_t)v);
  } else {
    o.u64((uint64_t)v);
  }
}
template <class S>
__device__ __forceinline__ void dc_double(S &o, const dc_args &a, double v) {
  char buf[GS_REPR_MAX];
  const uint32_t k = gs_repr_double((uint64_t)__double_as_longlong(v), a.pw, buf);
  o.put((const uint8_t *)buf, k);
}
template <class S>
__device__ __forceinline__ void dc_chr_name(S &o, const dc_args &a, uint32_t c) {
  const uint32_t b = a.name_off[c];
  o.put(a.names + b, a.name_off[c + 1u] - b);
}

/* complete mode (:148-154): the row of word w, if it is a position */
/* the match_features column of the off-target of word w: ',' and the names of its groups joined by ';', or NA */
template <class S>
__device__ __forceinline__ void dc_features(S &o, const dc_args &a, uint32_t w, const dc_site &s, uint32_t n) {
  o.ch(',');
  if (!a.nfeat[w]) {
    o.ch('N'), o.ch('A');
    return;
  }
  bool first = true;
  gs_an_decoded_visit(a.an, s.c, s.x, s.strand == '+', n, a.cum[s.c + 1u] - a.cum[s.c], [&](uint32_t g) {
    if (!first) o.ch(';');
    first = false;
    const uint32_t b = a.an_name_off[g];
    o.put(a.an_names + b, a.an_name_off[g + 1u] - b);
  });
}
template <class S>
__device__ __forceinline__ void dc_complete_row(S &o, const dc_args &a, uint32_t w) {
  if (!a.ispos[w]) return;
  if (a.only && !a.nfeat[w]) return; /* GS_DECODE_FEATURES_ONLY: no row; match_number below is the rank among all rows */
  const uint32_t r = a.rec[w];
  uint32_t dist_at = 0;
  dc_is_position(a, w, r, dist_at);
  uint8_t sg[DC_MAX_SEQ];
  const uint32_t n = dc_guide(a, r, sg);
  dc_site s;
  dc_resolve(a, a.words[w], n, s);
  o.put(a.ids + a.id_off[r], a.id_off[r + 1u] - a.id_off[r]);
  o.ch(',');
  o.u64(a.rank[w] - a.rank[a.word_off[r]]);
  o.ch(',');
  o.put(s.seq, s.len);
  o.ch(',');
  dc_chr_name(o, a, s.c);
  o.ch(',');
  o.u64(s.x);
  o.ch(',');
  o.ch(s.strand);
  o.ch(',');
  dc_i64(o, a.words[dist_at]);
  o.ch(',');
  const double cfd = a.cfd[w];
  if (cfd != DC_ABSENT && cfd != 0.0) dc_double(o, a, cfd); /* `cfd or ''` */
  if (a.features) dc_features(o, a, w, s, n);
  o.ch('\n');
}
/* succinct mode (:185-187): the row of record r */
template <class S>
__device__ __forceinline__ void dc_succinct_row(S &o, const dc_args &a, uint32_t r) {
  o.put(a.ids + a.id_off[r], a.id_off[r + 1u] - a.id_off[r]);
  o.ch(',');
  o.put(a.seqs + a.seq_off[r], a.seq_off[r + 1u] - a.seq_off[r]);
  o.ch(',');
  if (a.chr[r] >= 0) {
    dc_chr_name(o, a, (uint32_t)a.chr[r]);
  } else { /* an unmapped record's reference_name */
    o.ch('N'), o.ch('o'), o.ch('n'), o.ch('e');
  }
  o.ch(',');
  dc_i64(o, a.pos0[r]);
  o.ch(',');
  o.ch(a.reverse[r] ? '-' : '+');
  for (uint32_t k = 0; k < 4u; k++) {
    o.ch(',');
    o.u64(a.cnt[(size_t)r * 4u + k]);
  }
  o.ch(',');
  if (a.spec[r] != 0.0) dc_double(o, a, a.spec[r]);
  if (a.features)
    for (uint32_t k = 0; k < 4u; k++) {
      o.ch(',');
      o.u64(a.fcnt[(size_t)r * 4u + k]);
    }
  o.ch('\n');
}
template <class S>
__device__ __forceinline__ void dc_slot_row(S &o, const dc_args &a, uint64_t s) {
  if (a.complete)
    dc_complete_row(o, a, (uint32_t)s);
  else
    dc_succinct_row(o, a, (uint32_t)s);
}

/* the tile composer of gs_rowtext.h over dc_slot_row; a row that is too long fails its record */
__global__ __launch_bounds__(WAVE *GS_ROW_WAVES) void k_dc_len(dc_args a, uint32_t n_tiles) {
  if (*(volatile unsigned long long *)a.err != ~0ull) return; /* the batch is refused already: no text */
  gs_tile_len(
      a, a.slots, n_tiles, a.lens, a.tile_sum,
      [](const dc_args &a, gs_row_count &o, uint64_t s, uint64_t, uint32_t &) { dc_slot_row(o, a, s); },
      [](const dc_args &a, uint64_t s, uint32_t, bool too_long) {
        if (too_long) dc_fail(a, a.complete ? a.rec[s] : (uint32_t)s, DC_ERR_BIG);
        return !too_long;
      });
}

__global__ __launch_bounds__(WAVE *GS_ROW_WAVES) void k_dc_write(dc_args a, uint32_t n_tiles) {
  gs_tile_write<gs_row_write>(a, a.slots, n_tiles, a.lens, a.tile_off, a.out,
                              [](const dc_args &a, gs_row_write &o, uint64_t s, uint64_t) { dc_slot_row(o, a, s); });
}

/* ---- host ---------------------------------------------------------------------------------------------------- */
namespace {
struct bump { /* one buffer, parts behind each other on 256-byte boundaries */
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t r = at;
    at += (bytes + 255) & ~(size_t)255;
    return r;
  }
};
struct dc_min {
  __host__ __device__ uint32_t operator()(uint32_t x, uint32_t y) const { return x < y ? x : y; }
};
const char *const dc_reasons[] = {"",
                                  "hex digits that are no multiple of 16, or a symbol that is no hex digit",
                                  "an off-target word beyond the genome (|word| >= sum of @SQ LN), or a list that begins with the delimiter",
                                  "a PAM pair outside A,C,G,T in a 23-symbol off-target",
                                  "a distance outside 0..3 in succinct mode",
                                  "an off-target on a chromosome that the FASTA does not hold",
                                  "a stored sequence longer than 32 symbols",
                                  "a line or field that is no SAM record, or a chromosome index beyond the @SQ lines",
                                  "a row of 32 MB or more"};
const char dc_header_succinct[] =
    "id,sequence,chromosome,position,sense,distance_0_matches,distance_1_matches,distance_2_matches,distance_3_matches,specificity\n";
const char dc_header_complete[] = "id,match_number,sequence,chromosome,position,sense,distance,cfd\n";
/* GS_TEXT_FEATURES, in front of the newline.  distance_k_feature_matches: the off-targets that distance_k_matches counts and
 * that have at least one feature - counted exactly as that column counts, the record's own site included */
const char dc_header_succinct_features[] =
    ",distance_0_feature_matches,distance_1_feature_matches,distance_2_feature_matches,distance_3_feature_matches";
const char dc_header_complete_features[] = ",match_features";
struct dc_widen_nonzero {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return v ? 1ull : 0ull; }
};

gs_status dc_record_error(const gs_decode_batch *b, uint64_t first_record, uint64_t r, uint32_t reason) {
  std::string id;
  if (b && r < b->n) id.assign(b->ids + b->id_off[r], b->ids + b->id_off[r + 1]);
  gs_set_error("gs_decode: record " + std::to_string(first_record + r) + " (" + id + "): " + dc_reasons[reason < 9 ? reason : 0]);
  return GS_ERR_FORMAT;
}
}  // namespace

extern "C" gs_status gs_decoder_open(int device, const uint8_t *text, uint64_t len, const gs_genome_structure *sq,
                                     const uint64_t *chr_text_off, const uint64_t *chr_text_len, gs_decoder **out) {
  return gs_decoder_open_text(device, text, len, 0, sq, chr_text_off, chr_text_len, out);
}

gs_status gs_decoder_open_text(int device, const uint8_t *text, uint64_t len, int text_on_device, const gs_genome_structure *sq,
                               const uint64_t *chr_text_off, const uint64_t *chr_text_len, gs_decoder **out) {
  if (!out || !sq || (len && !text) || (sq->n_chr && (!sq->chr_names || !sq->chr_lengths || !chr_text_off || !chr_text_len))) return GS_ERR_ARG;
  *out = nullptr;
  for (uint32_t c = 0; c < sq->n_chr; c++) {
    if (!sq->chr_names[c]) return GS_ERR_ARG;
    if (chr_text_len[c] != ~0ull && (chr_text_off[c] > len || chr_text_len[c] > len - chr_text_off[c])) return GS_ERR_ARG;
  }
  gs_decoder *d = nullptr;
  try {
    d = new gs_decoder();
    d->device = device;
    d->n_chr = sq->n_chr;
    GS_HIP(hipSetDevice(device));
    gs_status rc;
    const uint32_t nc = sq->n_chr;
    std::vector<uint32_t> name_off(nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++) {
      d->names.emplace_back(sq->chr_names[c]);
      name_off[c + 1] = name_off[c] + (uint32_t)d->names[c].size();
      d->lengths.push_back(sq->chr_lengths[c]);
    }
    bump in;
    const size_t i_cum = in.take(8 * ((size_t)nc + 1)), i_toff = in.take(8 * (size_t)nc), i_flen = in.take(8 * (size_t)nc),
                 i_noff = in.take(4 * ((size_t)nc + 1)), i_names = in.take(name_off[nc]), i_p5 = in.take(sizeof gs_pow5),
                 i_p5i = in.take(sizeof gs_pow5_inv);
    std::vector<uint8_t> host(in.at + 16);
    uint64_t *cum = (uint64_t *)(host.data() + i_cum);
    cum[0] = 0;
    for (uint32_t c = 0; c < nc; c++) cum[c + 1] = cum[c] + sq->chr_lengths[c];
    d->total = cum[nc];
    if (nc) {
      memcpy(host.data() + i_toff, chr_text_off, 8 * (size_t)nc);
      memcpy(host.data() + i_flen, chr_text_len, 8 * (size_t)nc);
    }
    memcpy(host.data() + i_noff, name_off.data(), 4 * name_off.size());
    for (uint32_t c = 0; c < nc; c++) memcpy(host.data() + i_names + name_off[c], d->names[c].data(), d->names[c].size());
    memcpy(host.data() + i_p5, gs_pow5, sizeof gs_pow5);
    memcpy(host.data() + i_p5i, gs_pow5_inv, sizeof gs_pow5_inv);
    if ((rc = gs_reserve(d->tabs, in.at + 16)) != GS_OK || (rc = gs_reserve(d->text, len + 16)) != GS_OK) {
      gs_decoder_close(d);
      return rc;
    }
    const uint8_t *dt = (const uint8_t *)d->tabs.p;
    d->d_cum = (const uint64_t *)(dt + i_cum);
    d->d_toff = (const uint64_t *)(dt + i_toff);
    d->d_flen = (const uint64_t *)(dt + i_flen);
    d->d_name_off = (const uint32_t *)(dt + i_noff);
    d->d_names = dt + i_names;
    d->pw.pow5 = (const uint64_t(*)[2])(dt + i_p5);
    d->pw.pow5_inv = (const uint64_t(*)[2])(dt + i_p5i);
    hipError_t e = hipMemcpy(d->tabs.p, host.data(), in.at, hipMemcpyHostToDevice);
    if (e == hipSuccess && len) e = hipMemcpy(d->text.p, text, len, text_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e == hipSuccess && len) { /* .upper() once, in place: the slices are printed upper-cased (:59); the buffer has 16 bytes to spare */
      const uint64_t n16 = (len + 15) / 16;
      const uint32_t g = (uint32_t)std::min<uint64_t>((n16 + 255) / 256, (uint64_t)gs_num_cus(device) * 32u);
      hipLaunchKernelGGL(k_dc_upper, dim3(g), dim3(256), 0, nullptr, (uint4 *)d->text.p, n16);
      e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_dc_mm), gs_cfd_mm, sizeof gs_cfd_mm);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_dc_pam), gs_cfd_pam, sizeof gs_cfd_pam);
    if (e != hipSuccess) {
      gs_set_error(std::string("gs_decoder_open: ") + hipGetErrorString(e));
      gs_decoder_close(d);
      return GS_ERR_DEVICE;
    }
    *out = d;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    if (d) gs_decoder_close(d);
    return GS_ERR_NOMEM;
  }
}

extern "C" void gs_decoder_close(gs_decoder *d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  delete d;
}

extern "C" gs_status gs_decoder_set_annotation(gs_decoder *d, const gs_annot *an) {
  GS_HANDLE_LOCK(d);
  if (!d) return GS_ERR_ARG;
  if (an && an->device != d->device) {
    gs_set_error("gs_decoder_set_annotation: the annotation was built for another device, or for the host only");
    return GS_ERR_ARG;
  }
  if (an && an->chr_lengths != d->lengths) { /* as an_same_structure (gs_annot.hip): the count and every length */
    gs_set_error("gs_decoder_set_annotation: the @SQ lines are not the genome structure the annotation was made against");
    return GS_ERR_ARG;
  }
  d->annot = an;
  return GS_OK;
}

extern "C" gs_status gs_debug_decode_annot_ms(gs_decoder *d, double *ms) {
  GS_HANDLE_LOCK(d);
  if (!d || !ms) return GS_ERR_ARG;
  *ms = d->last_annot_ms;
  return GS_OK;
}

gs_status gs_decode_check_flags(const gs_decoder *d, uint32_t flags) {
  if ((flags & GS_TEXT_FEATURES) && !d->annot) {
    gs_set_error("gs_decode: GS_TEXT_FEATURES without an annotation (gs_decoder_set_annotation)");
    return GS_ERR_ARG;
  }
  if ((flags & GS_DECODE_FEATURES_ONLY) && (flags & (GS_TEXT_FEATURES | GS_TEXT_COMPLETE)) != (GS_TEXT_FEATURES | GS_TEXT_COMPLETE)) {
    gs_set_error("gs_decode: GS_DECODE_FEATURES_ONLY selects rows of the complete table by their features: it needs GS_TEXT_FEATURES | GS_TEXT_COMPLETE");
    return GS_ERR_ARG;
  }
  return GS_OK;
}

static gs_status decode_device(gs_decoder *d, const gs_decode_batch *b, uint32_t flags, uint64_t first_record, const void **d_text,
                               uint64_t *text_len, uint64_t *n_rows) {
  *d_text = nullptr;
  *text_len = 0;
  if (n_rows) *n_rows = 0;
  const uint64_t n = b->n;
  if (n == 0) return GS_OK;
  if (n >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
  hipStream_t st = nullptr;
  GS_HIP(hipSetDevice(d->device));
  /* the words of each record: whole groups of 16 digits (what is left over fails on the device, with the record) */
  std::vector<uint64_t> word_off(n + 1, 0);
  for (uint64_t r = 0; r < n; r++) {
    if (b->id_off[r + 1] < b->id_off[r] || b->seq_off[r + 1] < b->seq_off[r] || b->hex_off[r + 1] < b->hex_off[r]) return GS_ERR_ARG;
    word_off[r + 1] = word_off[r] + (b->hex_off[r + 1] - b->hex_off[r]) / 16;
  }
  const uint64_t nw = word_off[n];
  if (nw >= DC_NONE - 1u) {
    gs_set_error("gs_decode: 2^32 off-target words or more in one batch");
    return GS_ERR_UNSUPPORTED;
  }
  const uint64_t id0 = b->id_off[0], idb = b->id_off[n] - id0, sq0 = b->seq_off[0], sqb = b->seq_off[n] - sq0, hx0 = b->hex_off[0],
                 hxb = b->hex_off[n] - hx0;
  bump in;
  const size_t i_idoff = in.take(8 * (n + 1)), i_sqoff = in.take(8 * (n + 1)), i_hxoff = in.take(8 * (n + 1)), i_woff = in.take(8 * (n + 1)),
               i_pos = in.take(8 * n), i_chr = in.take(4 * n), i_rev = in.take(n), i_ids = in.take(idb), i_seqs = in.take(sqb),
               i_hex = in.take(hxb);
  std::vector<uint8_t> host(i_hex + 16); /* the hex digits, the bulk, are copied from where they are */
  {
    uint64_t *po = (uint64_t *)(host.data() + i_idoff), *ps = (uint64_t *)(host.data() + i_sqoff), *ph = (uint64_t *)(host.data() + i_hxoff);
    for (uint64_t r = 0; r <= n; r++) {
      po[r] = b->id_off[r] - id0;
      ps[r] = b->seq_off[r] - sq0;
      ph[r] = b->hex_off[r] - hx0;
    }
    memcpy(host.data() + i_woff, word_off.data(), 8 * (n + 1));
    memcpy(host.data() + i_pos, b->pos0, 8 * n);
    memcpy(host.data() + i_chr, b->chr, 4 * n);
    for (uint64_t r = 0; r < n; r++) host[i_rev + r] = b->reverse[r] ? 1 : 0;
    if (idb) memcpy(host.data() + i_ids, b->ids + id0, idb);
    if (sqb) memcpy(host.data() + i_seqs, b->seqs + sq0, sqb);
  }
  GS_TRY(gs_reserve(d->w_in, in.at + 16));
  uint8_t *din = (uint8_t *)d->w_in.p;
  GS_HIP(hipMemcpyAsync(din, host.data(), i_hex, hipMemcpyHostToDevice, st));
  if (hxb) GS_HIP(hipMemcpyAsync(din + i_hex, b->hex + hx0, hxb, hipMemcpyHostToDevice, st));
  gs_decode_batch_dev db;
  db.ids = din + i_ids;
  db.seqs = din + i_seqs;
  db.hex = din + i_hex;
  db.reverse = din + i_rev;
  db.id_off = (const uint64_t *)(din + i_idoff);
  db.seq_off = (const uint64_t *)(din + i_sqoff);
  db.hex_off = (const uint64_t *)(din + i_hxoff);
  db.word_off = (const uint64_t *)(din + i_woff);
  db.chr = (const int32_t *)(din + i_chr);
  db.pos0 = (const int64_t *)(din + i_pos);
  return gs_decode_run_device(d, db, n, nw, flags, first_record, b, d_text, text_len, n_rows);
}

/* the kernels over a batch whose arrays are in HBM already (decode_device uploads them; gs_bamsplit.hip makes them there).
 * hb: the same batch on the host, or nullptr: the id of a record that fails is then fetched from the device */
gs_status gs_decode_run_device(gs_decoder *d, const gs_decode_batch_dev &db, uint64_t n, uint64_t nw, uint32_t flags, uint64_t first_record,
                               const gs_decode_batch *b, const void **d_text, uint64_t *text_len, uint64_t *n_rows) {
  *d_text = nullptr;
  *text_len = 0;
  if (n_rows) *n_rows = 0;
  if (n == 0) return GS_OK;
  if (n >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
  if (nw >= DC_NONE - 1u) {
    gs_set_error("gs_decode: 2^32 off-target words or more in one batch");
    return GS_ERR_UNSUPPORTED;
  }
  hipStream_t st = nullptr;
  GS_HIP(hipSetDevice(d->device));
  const bool complete = (flags & GS_TEXT_COMPLETE) != 0;
  const gs_annot *an = (flags & GS_TEXT_FEATURES) ? d->annot : nullptr; /* the entry points have checked the flags */
  const bool only = an && complete && (flags & GS_DECODE_FEATURES_ONLY);
  const uint64_t slots = complete ? nw : n;
  const uint32_t n_tiles = (uint32_t)((slots + WAVE - 1) / WAVE);
  size_t tb_next = 0, tb_rank = 0, tb_tiles = 0, tb_rows = 0;
  if (only) /* the rows written: the words with a feature */
    GS_HIP(rocprim::reduce(nullptr, tb_rows, rocprim::make_transform_iterator((const uint32_t *)nullptr, dc_widen_nonzero()), (uint64_t *)nullptr,
                           0ull, (size_t)nw, rocprim::plus<uint64_t>(), st));
  GS_HIP(rocprim::inclusive_scan(nullptr, tb_next, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)nw, dc_min(), st));
  GS_HIP(rocprim::exclusive_scan(nullptr, tb_rank, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)nw + 1, rocprim::plus<uint32_t>(), st));
  GS_HIP(rocprim::exclusive_scan(nullptr, tb_tiles, (uint64_t *)nullptr, (uint64_t *)nullptr, 0ull, (size_t)n_tiles + 1,
                                 rocprim::plus<uint64_t>(), st));
  bump tm;
  const size_t t_err = tm.take(16), t_words = tm.take(8 * nw), t_cfd = tm.take(8 * nw), t_rec = tm.take(4 * nw), t_mark = tm.take(4 * nw),
               t_next = tm.take(4 * nw), t_ispos = tm.take(4 * (nw + 1)), t_rank = tm.take(4 * (nw + 1)), t_lens = tm.take(4 * slots),
               t_cnt = tm.take(complete ? 0 : 16 * n), t_spec = tm.take(complete ? 0 : 8 * n), t_tsum = tm.take(8 * ((size_t)n_tiles + 1)),
               t_toff = tm.take(8 * ((size_t)n_tiles + 1)), tb_scan = std::max(std::max(tb_next, tb_rows), std::max(tb_rank, tb_tiles)),
               t_scan = tm.take(tb_scan), t_nfeat = tm.take(an ? 4 * nw : 0), t_fcnt = tm.take(an && !complete ? 16 * n : 0),
               t_nrows = tm.take(only ? 8 : 0);
  GS_TRY(gs_reserve(d->w_tmp, tm.at + 16));
  char *tmp = (char *)d->w_tmp.p;

  dc_args a;
  memset(&a, 0, sizeof a);
  a.ids = db.ids;
  a.seqs = db.seqs;
  a.hex = db.hex;
  a.reverse = db.reverse;
  a.id_off = db.id_off;
  a.seq_off = db.seq_off;
  a.hex_off = db.hex_off;
  a.word_off = db.word_off;
  a.chr = db.chr;
  a.pos0 = db.pos0;
  a.text = (const uint8_t *)d->text.p;
  a.names = d->d_names;
  a.cum = d->d_cum;
  a.toff = d->d_toff;
  a.flen = d->d_flen;
  a.name_off = d->d_name_off;
  a.pw = d->pw;
  a.words = (int64_t *)(tmp + t_words);
  a.cfd = (double *)(tmp + t_cfd);
  a.rec = (uint32_t *)(tmp + t_rec);
  a.mark = (uint32_t *)(tmp + t_mark);
  a.next = (uint32_t *)(tmp + t_next);
  a.ispos = (uint32_t *)(tmp + t_ispos);
  a.rank = (uint32_t *)(tmp + t_rank);
  a.lens = (uint32_t *)(tmp + t_lens);
  a.cnt = (uint32_t *)(tmp + t_cnt);
  a.spec = (double *)(tmp + t_spec);
  a.tile_sum = (uint64_t *)(tmp + t_tsum);
  a.tile_off = (uint64_t *)(tmp + t_toff);
  a.err = (unsigned long long *)(tmp + t_err);
  a.slots = slots;
  a.total = d->total;
  a.delim = -((int64_t)d->total + 1);
  a.n = (uint32_t)n;
  a.n_words = (uint32_t)nw;
  a.n_chr = d->n_chr;
  a.complete = complete ? 1u : 0u;
  if (an) {
    a.an = an->d_table;
    a.an_name_off = an->d_name_off;
    a.an_names = an->d_names;
    a.nfeat = (uint32_t *)(tmp + t_nfeat);
    a.fcnt = (uint32_t *)(tmp + t_fcnt);
    a.features = 1u;
    a.only = only ? 1u : 0u;
  }
  uint64_t *d_nrows = (uint64_t *)(tmp + t_nrows);
  gs_events<2> ev;
  if (an)
    for (hipEvent_t &e : ev.e) GS_HIP(hipEventCreate(&e));

  const uint32_t cus = (uint32_t)gs_num_cus(d->device);
  const uint32_t gw = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nw + 256) / 256, (uint64_t)cus * 32u));
  const uint32_t grid = gs_tile_grid(n_tiles, cus);
  GS_HIP(hipMemsetAsync(tmp + t_err, 0xFF, 16, st));
  GS_HIP(hipMemsetAsync(a.tile_sum + n_tiles, 0, 8, st));
  if (nw) {
    hipLaunchKernelGGL(k_dc_hex, dim3(gw), dim3(256), 0, st, a);
    GS_TRY(gs_prim_carved("gs_decode: scan of the marks", tmp + t_scan, tb_scan, [&](void *t, size_t &tb) {
      return rocprim::inclusive_scan(t, tb, a.mark, a.next, (size_t)nw, dc_min(), st);
    }));
  }
  hipLaunchKernelGGL(k_dc_rec, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_dc_eval, dim3(gw), dim3(256), 0, st, a);
  if (an) {
    GS_HIP(hipEventRecord(ev.e[0], st));
    if (nw) hipLaunchKernelGGL(k_dc_feat, dim3(gw), dim3(256), 0, st, a);
    GS_HIP(hipEventRecord(ev.e[1], st));
    if (only) {
      GS_HIP(hipMemsetAsync(d_nrows, 0, 8, st));
      if (nw)
        GS_TRY(gs_prim_carved("gs_decode: count of the rows with a feature", tmp + t_scan, tb_scan, [&](void *t, size_t &tb) {
          return rocprim::reduce(t, tb, rocprim::make_transform_iterator((const uint32_t *)a.nfeat, dc_widen_nonzero()), d_nrows, 0ull,
                                 (size_t)nw, rocprim::plus<uint64_t>(), st);
        }));
    }
  }
  GS_TRY(gs_prim_carved("gs_decode: scan of the positions", tmp + t_scan, tb_scan, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, a.ispos, a.rank, 0u, (size_t)nw + 1, rocprim::plus<uint32_t>(), st);
  }));
  if (!complete) {
    const uint32_t gf = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + DC_FOLD_WAVES - 1) / DC_FOLD_WAVES, (uint64_t)cus * 32u));
    hipLaunchKernelGGL(k_dc_fold, dim3(gf), dim3(WAVE * DC_FOLD_WAVES), 0, st, a);
  }
  if (n_tiles) hipLaunchKernelGGL(k_dc_len, dim3(grid), dim3(WAVE * GS_ROW_WAVES), 0, st, a, n_tiles);
  GS_TRY(gs_prim_carved("gs_decode: scan of the tiles", tmp + t_scan, tb_scan, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, a.tile_sum, a.tile_off, 0ull, (size_t)n_tiles + 1, rocprim::plus<uint64_t>(), st);
  }));
  /* the length, the rows and the device's verdict come back together */
  uint64_t total = 0;
  unsigned long long err = 0;
  uint32_t n_pos = 0;
  GS_HIP(hipMemcpyAsync(&total, a.tile_off + n_tiles, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(&err, a.err, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(&n_pos, a.rank + nw, 4, hipMemcpyDeviceToHost, st));
  uint64_t n_featured = 0;
  if (only) GS_HIP(hipMemcpyAsync(&n_featured, d_nrows, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  if (an) {
    const int from = 0;
    GS_TRY(ev.elapsed(&from, 1, &d->last_annot_ms));
  }
  if (err != ~0ull) {
    const uint32_t reason = (uint32_t)(err & 255u);
    if (reason == DC_ERR_BIG) {
      gs_set_error("gs_decode: a row of 32 MB or more");
      return GS_ERR_UNSUPPORTED;
    }
    if (b) return dc_record_error(b, first_record, err >> 8, reason);
    /* the batch is in HBM only: the record's id comes back for the message */
    const uint64_t r = err >> 8;
    uint64_t span[2] = {0, 0};
    GS_HIP(hipMemcpy(span, db.id_off + r, 16, hipMemcpyDeviceToHost));
    std::string id((size_t)(span[1] - span[0]), '\0');
    if (!id.empty()) GS_HIP(hipMemcpy(&id[0], db.ids + span[0], id.size(), hipMemcpyDeviceToHost));
    gs_set_error("gs_decode: record " + std::to_string(first_record + r) + " (" + id + "): " + dc_reasons[reason < 9 ? reason : 0]);
    return GS_ERR_FORMAT;
  }
  GS_TRY(gs_reserve(d->w_text, total + 16));
  a.out = (char *)d->w_text.p;
  if (total) hipLaunchKernelGGL(k_dc_write, dim3(grid), dim3(WAVE * GS_ROW_WAVES), 0, st, a, n_tiles);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  *d_text = d->w_text.p;
  *text_len = total;
  if (n_rows) *n_rows = only ? n_featured : complete ? (uint64_t)n_pos : n;
  return GS_OK;
}

static bool dc_batch_ok(const gs_decode_batch *b) {
  return b && (b->n == 0 || (b->ids && b->id_off && b->seqs && b->seq_off && b->reverse && b->chr && b->pos0 && b->hex_off &&
                             (b->hex || b->hex_off[b->n] == b->hex_off[0])));
}

extern "C" gs_status gs_decode_records_device(gs_decoder *d, const gs_decode_batch *b, uint32_t flags, uint64_t first_record,
                                              const void **d_text, uint64_t *len, uint64_t *n_rows) {
  GS_HANDLE_LOCK(d);
  if (!d || !d_text || !len || !dc_batch_ok(b)) return GS_ERR_ARG;
  GS_TRY(gs_decode_check_flags(d, flags));
  try {
    return decode_device(d, b, flags, first_record, d_text, len, n_rows);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_decode_records(gs_decoder *d, const gs_decode_batch *b, uint32_t flags, uint64_t first_record, char **text,
                                       uint64_t *len, uint64_t *n_rows) {
  GS_HANDLE_LOCK(d);
  if (!d || !text || !len || !dc_batch_ok(b)) return GS_ERR_ARG;
  *text = nullptr;
  *len = 0;
  const void *dt = nullptr;
  uint64_t tl = 0;
  gs_status rc = gs_decode_records_device(d, b, flags, first_record, &dt, &tl, n_rows);
  if (rc != GS_OK) return rc;
  if ((rc = gs_text_to_host(dt, tl, text)) != GS_OK) return rc;
  *len = tl;
  return GS_OK;
}

/* the lines of a SAM text as a batch: header lines are skipped (the @SQ lines went into gs_decoder_open) */
extern "C" gs_status gs_decode_sam(gs_decoder *d, const char *sam, uint64_t sam_len, uint32_t flags, uint64_t first_record, char **text,
                                   uint64_t *len, uint64_t *n_records) {
  GS_HANDLE_LOCK(d);
  if (!d || (sam_len && !sam) || !text || !len) return GS_ERR_ARG;
  *text = nullptr;
  *len = 0;
  if (n_records) *n_records = 0;
  GS_TRY(gs_decode_check_flags(d, flags));
  try {
    std::string ids, seqs;
    std::vector<uint64_t> id_off{0}, seq_off{0}, hex_off;
    std::vector<uint8_t> reverse;
    std::vector<int32_t> chr;
    std::vector<int64_t> pos0;
    std::map<std::string, int32_t> by_name;
    for (uint32_t c = 0; c < d->n_chr; c++) by_name.emplace(d->names[c], (int32_t)c); /* the first of equal names */
    auto bad = [&](const char *what) {
      gs_set_error("gs_decode: record " + std::to_string(first_record + chr.size()) + ": " + what);
      return GS_ERR_FORMAT;
    };
    for (uint64_t at = 0; at < sam_len;) {
      const char *nl = (const char *)memchr(sam + at, '\n', sam_len - at);
      const uint64_t end = nl ? (uint64_t)(nl - sam) : sam_len;
      uint64_t le = end;
      if (le > at && sam[le - 1] == '\r') le--;
      const uint64_t b0 = at;
      at = end + 1;
      if (le == b0 || sam[b0] == '@') continue;
      uint64_t f[12], nf = 0; /* where the first eleven fields begin, and the tags */
      f[nf++] = b0;
      for (uint64_t i = b0; i < le && nf < 12; i++)
        if (sam[i] == '\t') f[nf++] = i + 1;
      if (nf < 11) return bad(dc_reasons[DC_ERR_RECORD]);
      auto field = [&](int k) { return std::string(sam + f[k], (k + 1 < (int)nf ? f[k + 1] - 1 : le) - f[k]); };
      const std::string flag_s = field(1), rname = field(2), pos_s = field(3);
      char *e1 = nullptr, *e2 = nullptr;
      const long long flag = strtoll(flag_s.c_str(), &e1, 10), pos = strtoll(pos_s.c_str(), &e2, 10);
      if (flag_s.empty() || *e1 || pos_s.empty() || *e2) return bad(dc_reasons[DC_ERR_RECORD]);
      const auto it = by_name.find(rname); /* '*' or a name no @SQ line has: unmapped (htslib), printed as None */
      const int32_t c = it == by_name.end() ? -1 : it->second;
      uint64_t hb = 0, he = 0; /* the last of:H: field */
      for (uint64_t t = nf == 12 ? f[11] : le; t < le;) {
        const char *tab = (const char *)memchr(sam + t, '\t', le - t);
        const uint64_t te = tab ? (uint64_t)(tab - sam) : le;
        if (te - t >= 5 && !memcmp(sam + t, "of:H:", 5)) hb = t + 5, he = te;
        t = te + 1;
      }
      ids.append(sam + f[0], f[1] - 1 - f[0]);
      id_off.push_back(ids.size());
      seqs.append(sam + f[9], f[10] - 1 - f[9]);
      seq_off.push_back(seqs.size());
      reverse.push_back((flag & 16) ? 1 : 0);
      chr.push_back(c);
      pos0.push_back(pos - 1);
      hex_off.push_back(hb);
      hex_off.push_back(he);
    }
    /* the hex spans stay where they are in the SAM text: one more span per record (the gap to the next field) would need
     * offsets in pairs, so the digits are gathered */
    const uint64_t n = chr.size();
    std::string hex;
    std::vector<uint64_t> hoff(n + 1, 0);
    for (uint64_t r = 0; r < n; r++) {
      hex.append(sam + hex_off[2 * r], hex_off[2 * r + 1] - hex_off[2 * r]);
      hoff[r + 1] = hex.size();
    }
    gs_decode_batch b;
    memset(&b, 0, sizeof b);
    b.n = n;
    b.ids = ids.data();
    b.id_off = id_off.data();
    b.seqs = seqs.data();
    b.seq_off = seq_off.data();
    b.reverse = reverse.data();
    b.chr = chr.data();
    b.pos0 = pos0.data();
    b.hex = hex.data();
    b.hex_off = hoff.data();
    char *rows = nullptr;
    uint64_t rl = 0;
    gs_status rc = n ? gs_decode_records(d, &b, flags, first_record, &rows, &rl, nullptr) : GS_OK;
    if (rc != GS_OK) return rc;
    const bool header = !(flags & GS_DECODE_NO_HEADER);
    std::string h;
    if (header) {
      const bool complete = (flags & GS_TEXT_COMPLETE) != 0;
      h = complete ? dc_header_complete : dc_header_succinct;
      if (flags & GS_TEXT_FEATURES) h.insert(h.size() - 1, complete ? dc_header_complete_features : dc_header_succinct_features);
    }
    const size_t hl = h.size();
    char *outp = (char *)malloc(hl + rl + 1);
    if (!outp) {
      free(rows);
      return GS_ERR_NOMEM;
    }
    memcpy(outp, h.data(), hl);
    if (rl) memcpy(outp + hl, rows, rl);
    outp[hl + rl] = 0;
    free(rows);
    *text = outp;
    *len = hl + rl;
    if (n_records) *n_records = n;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_debug_repr_doubles(const double *v, uint64_t n, char *out) {
  if (n && (!v || !out)) return GS_ERR_ARG;
  const gs_pow5_tables t{gs_pow5, gs_pow5_inv};
  for (uint64_t i = 0; i < n; i++) {
    uint64_t bits;
    memcpy(&bits, v + i, 8);
    char *o = out + GS_REPR_MAX * i;
    memset(o, 0, GS_REPR_MAX);
    gs_repr_double(bits, t, o);
  }
  return GS_OK;
}

extern "C" gs_status gs_debug_decode_tables(double *mm, double *pam) {
  if (!mm || !pam) return GS_ERR_ARG;
  memcpy(mm, gs_cfd_mm, sizeof gs_cfd_mm);
  memcpy(pam, gs_cfd_pam, sizeof gs_cfd_pam);
  return GS_OK;
}
