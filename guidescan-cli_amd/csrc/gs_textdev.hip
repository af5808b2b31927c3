/*
 * gs_textdev.hip -- the database text on the device ("at scale"): the bytes
 * gs_format_guides_scored writes (gs_text.hip: get_csv_lines / get_sam_lines, include/genomics/printer.hpp:115-360,
 * resolve_absolute, src/genomics/structures.cxx:7-52), produced from the CSR hit lists, the guides and the per-guide
 * specificities where they already are: in HBM.  Integer arithmetic only - the specificity's "%f" included.
 *
 * Rows are the unit of work, not guides.  Every guide owns one guide slot (its `NA` row, the checks made once per
 * guide) followed by one slot per hit: slot of guide g = (offsets[g] - offsets[0]) + g.  A tile is 64 consecutive slots,
 * one wavefront:
 *   k_tx_len    the byte length of every slot's row (0: no row), the tile's sum;
 *   (rocPRIM)   64-bit exclusive scan of the tile sums: a batch of 4 M guides is more than 4 GB of text;
 *   k_tx_write  every lane composes its row into the wave's LDS slice at its offset inside the tile, then the wave
 *               streams the tile's contiguous span out with 16-byte stores (LDS and HBM addresses are congruent mod 16;
 *               only the span's ragged head and tail are byte stores).  A tile whose span outgrows the slice (very long
 *               ids or chromosome names, long of:H: fields) is composed in HBM directly.
 * Both kernels run ONE row routine over two sinks, a counting one and a writing one: the lengths cannot disagree.  The
 * sinks and the two tile passes themselves (gs_tile_len, gs_tile_write) are gs_rowtext.h's, shared with gs_decode.hip: this
 * file keeps the rows, the SAM tables and the host driver; k_tx_len and k_tx_write hand tx_slot_row to the templates.
 * SAM needs three per-guide facts first (k_tx_sam_ok, k_tx_sam_guide): the unfiltered count per distance, the hits kept
 * per distance (the cap counts kept hits, after the boundary drop: printer.hpp:129 - the CSV cap counts raw indices,
 * :259), and the of:H: field, which is composed once per guide into a scratch span (k_tx_sam_hex) and copied into each
 * of the guide's lines by the whole wave.
 * GS_TEXT_BAM: a third row routine over the same sinks and the same SAM tables writes each SAM line as the BAM alignment
 * block host/bam_writer.hpp makes of it (tx_bam_row); GS_TEXT_BGZF hands the blocks to gs_bgzf.hip.
 */
#include "gs_device.h"
#include "gs_rowtext.h"
#include "gs_bgzf_huff.h"
#include "gs_scratch.h"
#include "gs_resolve.h"
#include "gs_annot_obj.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

#define TX_ERR_ARG 1u
#define TX_ERR_BIG 2u
#define TX_ERR_ID 4u /* BAM: an id of more than 254 bytes (l_read_name is one byte and counts the NUL) */

struct tx_args {
  const uint8_t *guides, *pams;   /* n*L, n*P ASCII */
  const uint8_t *ids;             /* the ids back to back */
  const uint64_t *id_off;         /* n+1, from 0 */
  const uint8_t *senses, *skip;   /* n bytes each, or nullptr */
  const uint64_t *offsets;        /* n+1 positions into hits */
  const gs_hit *hits;
  const float *spec;
  const uint64_t *chr_cum;        /* n_chr+1 prefix sums of the chromosome lengths */
  const uint8_t *chr_names;
  const uint32_t *chr_name_off;   /* n_chr+1 */
  uint32_t *lens;                 /* per slot */
  uint64_t *tile_sum, *tile_off;  /* per tile (+1) */
  char *text;
  uint32_t *err;
  /* SAM: boundary flags and their prefix sums per hit; per guide and distance the unfiltered count, the prefix sum at
   * the distance's first hit, the 16-character units of the of:H: field before the distance's positions */
  uint32_t *okf, *S, *cnt, *sbase, *kbase;
  uint64_t *hex_units, *hex_off;
  char *hex;
  uint64_t slots, off0, n_hits;
  long long max_off, delim;
  uint32_t n, L, P, n_chr, m, start, sam, complete;
  uint32_t bam; /* with sam: the lines as BAM alignment blocks (tx_bam_row) */
  /* GS_TEXT_FEATURES: what gs_annotate_device left for the same hit list (offsets from 0, by hit - off0), the group names */
  const uint64_t *feat_off;
  const uint32_t *feats, *gname_off;
  const uint8_t *gnames;
  uint32_t features;
};

/* ---- small pieces -------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t tx_comp(uint32_t c) { /* src/genomics/sequences.cxx:14-26 */
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    default: return c;
  }
}

/* "%f" of a float in [0, 1] as round(f * 10^6) under round-half-even on the exact value (what glibc prints):
 * f = m * 2^e with m < 2^24, so m * 10^6 < 2^44; shifted right by -e with the exact remainder deciding. */
__device__ __forceinline__ bool tx_spec_ok(uint32_t bits) { return bits <= 0x3F800000u; } /* +0 .. 1.0; no sign, NaN, inf */
__device__ __forceinline__ uint32_t tx_spec_q(uint32_t bits) {
  const uint32_t ex = bits >> 23, mant = bits & 0x7FFFFFu;
  const uint64_t m = ex ? (uint64_t)(mant | 0x800000u) : (uint64_t)mant;
  const uint32_t sh = ex ? 150u - ex : 149u; /* f = m * 2^-sh, sh >= 23 for f <= 1 */
  const uint64_t x = m * 1000000ull;
  if (sh >= 64u) return 0u; /* x < 2^44 <= half an ulp of the last digit */
  uint64_t q = x >> sh;
  const uint64_t rem = x & ((1ull << sh) - 1ull), half = 1ull << (sh - 1u);
  if (rem > half || (rem == half && (q & 1ull))) q++;
  return (uint32_t)q;
}

/* src/genomics/structures.cxx:7-52 by binary search over the prefix sums (gs_resolve.h: the annotation kernels share it) */
typedef gs_loc tx_loc;
__device__ __forceinline__ tx_loc tx_resolve(const tx_args &a, long long pos) { return gs_resolve_abs(a.chr_cum, a.n_chr, a.L, a.P, pos); }

/* slots: guide g's own slot, then its hits */
__device__ __forceinline__ uint64_t tx_slot_of(const tx_args &a, uint32_t g) { return a.offsets[g] - a.off0 + g; }
/* the guide of a tile's first slot (wave-uniform), then each lane walks to its own */
__device__ __forceinline__ uint32_t tx_guide_of(const tx_args &a, uint64_t s0, uint64_t s) {
  uint32_t lo = 0, hi = a.n; /* last g with slot_of(g) <= s0 */
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tx_slot_of(a, mid) <= s0)
      lo = mid;
    else
      hi = mid;
  }
  uint32_t g = lo;
  while (g + 1u < a.n && tx_slot_of(a, g + 1u) <= s) g++;
  return g;
}
/* first hit of [b, e) at distance d or more (hits are in canonical order: distance ascending) */
__device__ __forceinline__ uint64_t tx_first_at(const gs_hit *hits, uint64_t b, uint64_t e, uint32_t d) {
  while (b < e) {
    const uint64_t mid = (b + e) >> 1;
    if ((uint32_t)(hits[mid].key >> 61) < d)
      b = mid + 1u;
    else
      e = mid;
  }
  return b;
}

/* ---- the rows: templates over the sinks of gs_rowtext.h (the of:H: field of a SAM line is a `span`) ------------ */
template <class S>
__device__ __forceinline__ void tx_id(S &o, const tx_args &a, uint32_t g) {
  const uint64_t b = a.id_off[g], e = a.id_off[g + 1u];
  o.put(a.ids + b, e >= b ? (uint32_t)(e - b) : 0u); /* e < b: GS_ERR_ARG from the guide's own slot */
}
template <class S>
__device__ __forceinline__ void tx_sequence(S &o, const tx_args &a, uint32_t g) { /* sequence + pam, or pam + sequence under --start */
  const uint8_t *gd = a.guides + (size_t)g * a.L, *pm = a.pams + (size_t)g * a.P;
  if (a.start) o.put(pm, a.P);
  o.put(gd, a.L);
  if (!a.start) o.put(pm, a.P);
}
template <class S>
__device__ __forceinline__ void tx_specificity(S &o, uint32_t q) { /* std::to_string(float): d.dddddd */
  o.ch('0' + q / 1000000u);
  o.ch('.');
  uint32_t r = q % 1000000u, div = 100000u;
  for (int i = 0; i < 6; i++) {
    o.ch('0' + r / div);
    r %= div;
    div /= 10u;
  }
}
template <class S>
__device__ __forceinline__ void tx_chr_name(S &o, const tx_args &a, int c) {
  const uint32_t b = a.chr_name_off[c];
  o.put(a.chr_names + b, a.chr_name_off[c + 1] - b);
}

/* GS_TEXT_FEATURES: the row's tail, ",name;name" or ",NA" (i: the hit's index from off0) */
template <class S>
__device__ __forceinline__ void tx_features(S &o, const tx_args &a, uint64_t i) {
  o.ch(',');
  const uint64_t b = a.feat_off[i], e = a.feat_off[i + 1u];
  if (b == e) {
    GS_ROW_LIT(o, "NA");
    return;
  }
  for (uint64_t x = b; x < e; x++) {
    if (x > b) o.ch(';');
    const uint32_t g = a.feats[x], nb = a.gname_off[g];
    o.put(a.gnames + nb, a.gname_off[g + 1u] - nb);
  }
}

/* the guide's own slot: its NA row (printer.hpp:189-199), and the checks made once per guide */
template <class S>
__device__ __forceinline__ void tx_guide_row(S &o, const tx_args &a, uint32_t g, uint32_t &err) {
  if (a.id_off[g + 1u] < a.id_off[g]) err |= TX_ERR_ARG; /* offsets that came from the device: not checked on the host */
  if (a.skip && a.skip[g]) return;
  const uint64_t nh = a.offsets[g + 1u] - a.offsets[g];
  if (nh) {
    if (!tx_spec_ok(__float_as_uint(a.spec[g]))) err |= TX_ERR_ARG;
    if ((uint32_t)(a.hits[a.offsets[g + 1u] - 1u].key >> 61) > a.m) err |= TX_ERR_ARG; /* the last hit has the largest distance */
    /* BAM: a guide with lines (its first hit is at distance 0) whose id a record cannot hold */
    if (a.bam && (uint32_t)(a.hits[a.offsets[g]].key >> 61) == 0u && a.id_off[g + 1u] > a.id_off[g] + 254u) err |= TX_ERR_ID;
    return;
  }
  if (a.sam) return;
  tx_id(o, a, g);
  o.ch(',');
  tx_sequence(o, a, g);
  GS_ROW_LIT(o, ",NA,NA,NA,0");
  if (a.complete) GS_ROW_LIT(o, ",NA,NA,NA");
  if (a.features)
    GS_ROW_LIT(o, ",1.0,NA\n");
  else
    GS_ROW_LIT(o, ",1.0\n");
}

/* one CSV row (printer.hpp:245-300 as format_csv_fast restates it) */
template <class S>
__device__ __forceinline__ void tx_csv_row(S &o, const tx_args &a, uint32_t g, uint64_t h, uint32_t &err) {
  if (a.skip && a.skip[g]) return;
  const gs_hit hit = a.hits[h];
  const uint32_t d = (uint32_t)(hit.key >> 61);
  if (d > a.m) {
    err |= TX_ERR_ARG;
    return;
  }
  if (a.max_off != -1) { /* the raw index within the distance, :259 */
    const uint64_t first = tx_first_at(a.hits, a.offsets[g], h, d);
    if ((long long)(h - first) >= a.max_off) return;
  }
  const tx_loc loc = tx_resolve(a, (long long)hit.pos);
  if (loc.c < 0) return; /* boundary hit: no row (:280-283) */
  tx_id(o, a, g);
  o.ch(',');
  tx_sequence(o, a, g);
  o.ch(',');
  tx_chr_name(o, a, loc.c);
  o.ch(',');
  o.u64((uint64_t)loc.s);
  o.ch(',');
  o.ch(loc.st);
  o.ch(',');
  o.ch('0' + d);
  if (a.complete) {
    o.ch(',');
    /* complement(match.sequence) from key bits 59:1 (gs_decode_sequence + printer.hpp:232,264) */
    const uint8_t *gd = a.guides + (size_t)g * a.L;
    const uint64_t path = (hit.key >> 1) & ((1ull << 59) - 1ull);
    for (uint32_t t = 0; t < a.L; t++) {
      const uint32_t gq = a.start ? gd[a.L - 1u - t] : gd[t];
      const uint32_t qc = a.start ? gq : tx_comp(gq); /* the query symbol of this step (index.hpp:218) */
      const uint32_t code = (uint32_t)(path >> (57u - 2u * t)) & 3u;
      if (code == 0u) {
        o.ch(tx_comp(qc));
      } else {
        const int q = qc == 'A' ? 0 : qc == 'C' ? 1 : qc == 'G' ? 2 : qc == 'T' ? 3 : -1;
        if (q < 0) {
          err |= TX_ERR_ARG;
          return;
        }
        int b = (int)code - 1;
        if (b >= q) b++;
        o.ch(b == 0 ? 't' : b == 1 ? 'g' : b == 2 ? 'c' : 'a'); /* complement, lower case: the mismatch (index.hpp:243) */
      }
    }
    for (uint32_t u = 0; u < a.P; u++) {
      const uint32_t code = (uint32_t)(path >> (56u - 2u * a.L - 3u * u)) & 7u;
      if (code > 4u) {
        err |= TX_ERR_ARG;
        return;
      }
      o.ch(code == 0u ? 'T' : code == 1u ? 'G' : code == 2u ? 'C' : code == 3u ? 'N' : 'A'); /* complement of A,C,G,N,T */
    }
    GS_ROW_LIT(o, ",0,0"); /* rna_bulges, dna_bulges */
  }
  o.ch(',');
  tx_specificity(o, tx_spec_q(__float_as_uint(a.spec[g])));
  if (a.features) tx_features(o, a, h - a.off0);
  o.ch('\n');
}

/* one SAM line: a distance-0 hit (printer.hpp:314-357) */
template <class S>
__device__ __forceinline__ void tx_sam_row(S &o, const tx_args &a, uint32_t g, uint64_t h) {
  if (a.skip && a.skip[g]) return;
  const gs_hit hit = a.hits[h];
  if ((uint32_t)(hit.key >> 61) != 0u) return;
  const bool pos_sense = a.senses ? a.senses[g] != 0 : true;
  const tx_loc loc = tx_resolve(a, (long long)hit.pos);
  tx_id(o, a, g);
  o.ch('\t');
  if (pos_sense)
    o.ch('0');
  else
    GS_ROW_LIT(o, "16");
  o.ch('\t');
  if (loc.c >= 0) tx_chr_name(o, a, loc.c); /* no sentinel check in the reference: empty RNAME */
  o.ch('\t');
  o.u64(loc.c >= 0 ? (uint64_t)loc.s : 0ull);
  GS_ROW_LIT(o, "\t100\t");
  o.u64((uint64_t)a.L + a.P);
  GS_ROW_LIT(o, "M\t*\t0\t0\t");
  if (pos_sense) {
    tx_sequence(o, a, g);
  } else { /* reverse_complement(sequence) */
    const uint8_t *gd = a.guides + (size_t)g * a.L, *pm = a.pams + (size_t)g * a.P;
    const uint32_t lp = a.L + a.P;
    for (uint32_t i = 0; i < lp; i++) {
      const uint32_t j = lp - 1u - i; /* sequence[j] */
      const uint32_t c = a.start ? (j < a.P ? pm[j] : gd[j - a.P]) : (j < a.L ? gd[j] : pm[j - a.L]);
      o.ch(tx_comp(c));
    }
  }
  GS_ROW_LIT(o, "\t*");
  for (uint32_t d = 0; d <= a.m; d++) {
    GS_ROW_LIT(o, "\tk");
    o.ch('0' + d);
    GS_ROW_LIT(o, ":i:");
    o.u64(a.cnt[(size_t)g * 8u + d]); /* unfiltered */
  }
  if (a.complete) {
    GS_ROW_LIT(o, "\tof:H:");
    o.span(a.hex + 16u * a.hex_off[g], 16u * (a.hex_off[g + 1u] - a.hex_off[g]));
  }
  GS_ROW_LIT(o, "\tsp:f:");
  tx_specificity(o, tx_spec_q(__float_as_uint(a.spec[g])));
  o.ch('\n');
}

/* the same line as one BAM alignment block (SAMv1 section 4.2), field for field what host/bam_writer.hpp: bam::record
 * derives from the SAM line above: the route of manual/manual.tex:581-582 over the lines of printer.hpp:302-360 */
template <class S>
__device__ __forceinline__ void tx_le(S &o, uint32_t v, uint32_t bytes) {
  for (uint32_t i = 0; i < bytes; i++) o.ch((v >> (8u * i)) & 255u);
}
__device__ __forceinline__ uint32_t tx_reg2bin(uint32_t beg, uint32_t end) { /* SAMv1 section 5.3; beg < end <= 2^31 */
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
  return 0u;
}
__device__ __forceinline__ uint32_t tx_nt16(uint32_t c) { /* =ACMGRSVTWYHKDBN, lower case as upper, anything else N */
  if (c >= 'a' && c <= 'z') c -= 32u;
  switch (c) {
    case '=': return 0;
    case 'A': return 1;
    case 'C': return 2;
    case 'M': return 3;
    case 'G': return 4;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'T': return 8;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    default: return 15;
  }
}
/* symbol i of the line's SEQ field: the sequence as printed, or its reverse complement */
__device__ __forceinline__ uint32_t tx_seq_at(const tx_args &a, uint32_t g, uint32_t i, bool pos_sense) {
  const uint8_t *gd = a.guides + (size_t)g * a.L, *pm = a.pams + (size_t)g * a.P;
  const uint32_t lp = a.L + a.P, j = pos_sense ? i : lp - 1u - i;
  const uint32_t c = a.start ? (j < a.P ? pm[j] : gd[j - a.P]) : (j < a.L ? gd[j] : pm[j - a.L]);
  return pos_sense ? c : tx_comp(c);
}
template <class S>
__device__ __forceinline__ void tx_bam_row(S &o, const tx_args &a, uint32_t g, uint64_t h) {
  if (a.skip && a.skip[g]) return;
  const gs_hit hit = a.hits[h];
  if ((uint32_t)(hit.key >> 61) != 0u) return;
  const bool pos_sense = a.senses ? a.senses[g] != 0 : true;
  const tx_loc loc = tx_resolve(a, (long long)hit.pos);
  const uint64_t ib = a.id_off[g], ie = a.id_off[g + 1u];
  const uint32_t idn = ie >= ib ? (uint32_t)(ie - ib) : 0u, lp = a.L + a.P; /* idn > 254: GS_ERR_ARG from the guide's slot */
  const uint64_t hexn = a.complete ? 16u * (a.hex_off[g + 1u] - a.hex_off[g]) : 0u;
  uint32_t tags = 7u; /* sp */
  for (uint32_t d = 0; d <= a.m; d++) {
    const uint32_t v = a.cnt[(size_t)g * 8u + d];
    tags += 3u + (v <= 255u ? 1u : v <= 65535u ? 2u : 4u);
  }
  const uint64_t body = 32ull + idn + 1u + 4u + (lp + 1u) / 2u + lp + tags + (a.complete ? 4ull + hexn : 0ull);
  const int32_t pos = loc.c >= 0 ? (int32_t)(loc.s - 1) : -1; /* POS - 1; the reference prints 0 with its empty RNAME */
  tx_le(o, (uint32_t)body, 4);
  tx_le(o, (uint32_t)(loc.c >= 0 ? loc.c : -1), 4);
  tx_le(o, (uint32_t)pos, 4);
  o.ch((idn + 1u) & 255u);
  o.ch(100);
  tx_le(o, pos < 0 ? 4680u : tx_reg2bin((uint32_t)pos, (uint32_t)pos + lp), 2);
  tx_le(o, 1u, 2);
  tx_le(o, pos_sense ? 0u : 16u, 2);
  tx_le(o, lp, 4);
  tx_le(o, 0xFFFFFFFFu, 4);
  tx_le(o, 0xFFFFFFFFu, 4);
  tx_le(o, 0u, 4);
  tx_id(o, a, g);
  o.ch(0);
  tx_le(o, lp << 4, 4);
  for (uint32_t i = 0; i < lp; i += 2u)
    o.ch((tx_nt16(tx_seq_at(a, g, i, pos_sense)) << 4) | (i + 1u < lp ? tx_nt16(tx_seq_at(a, g, i + 1u, pos_sense)) : 0u));
  for (uint32_t i = 0; i < lp; i++) o.ch(0xFF);
  for (uint32_t d = 0; d <= a.m; d++) {
    const uint32_t v = a.cnt[(size_t)g * 8u + d]; /* unfiltered */
    o.ch('k');
    o.ch('0' + d);
    o.ch(v <= 255u ? 'C' : v <= 65535u ? 'S' : 'I');
    tx_le(o, v, v <= 255u ? 1u : v <= 65535u ? 2u : 4u);
  }
  if (a.complete) {
    GS_ROW_LIT(o, "ofH");
    o.span(a.hex + 16u * a.hex_off[g], hexn);
    o.ch(0);
  }
  GS_ROW_LIT(o, "spf");
  tx_le(o, gb_sp_float_bits(tx_spec_q(__float_as_uint(a.spec[g]))), 4);
}

template <class S>
__device__ __forceinline__ void tx_slot_row(S &o, const tx_args &a, uint64_t s0, uint64_t s, uint32_t &err) {
  const uint32_t g = tx_guide_of(a, s0, s);
  const uint64_t gs0 = tx_slot_of(a, g);
  if (s == gs0)
    tx_guide_row(o, a, g, err);
  else if (a.bam)
    tx_bam_row(o, a, g, a.offsets[g] + (s - gs0 - 1u));
  else if (a.sam)
    tx_sam_row(o, a, g, a.offsets[g] + (s - gs0 - 1u));
  else
    tx_csv_row(o, a, g, a.offsets[g] + (s - gs0 - 1u), err);
}

/* ---- kernels ------------------------------------------------------------------------------------------------- */
/* the tile composer of gs_rowtext.h over tx_slot_row; a slot's flags are ORed into the error word, and its row is left out */
__global__ __launch_bounds__(WAVE *GS_ROW_WAVES) void k_tx_len(tx_args a, uint32_t n_tiles) {
  gs_tile_len(
      a, a.slots, n_tiles, a.lens, a.tile_sum,
      [](const tx_args &a, gs_row_count &o, uint64_t s, uint64_t s0, uint32_t &err) { tx_slot_row(o, a, s0, s, err); },
      [](const tx_args &a, uint64_t, uint32_t err, bool too_long) {
        if (too_long) err |= TX_ERR_BIG;
        if (err) atomicOr(a.err, err);
        return err == 0u;
      });
}

__global__ __launch_bounds__(WAVE *GS_ROW_WAVES) void k_tx_write(tx_args a, uint32_t n_tiles) {
  gs_tile_write<gs_row_write_span>(a, a.slots, n_tiles, a.lens, a.tile_off, a.text, [](const tx_args &a, gs_row_write_span &o, uint64_t s, uint64_t s0) {
    uint32_t err = 0; /* k_tx_len has had the verdict */
    tx_slot_row(o, a, s0, s, err);
  });
}

/* SAM: 1 = the hit survives resolve_absolute */
__global__ __launch_bounds__(256) void k_tx_sam_ok(tx_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.n_hits; i += (uint64_t)gridDim.x * blockDim.x)
    a.okf[i] = i < a.n_hits && tx_resolve(a, (long long)a.hits[a.off0 + i].pos).c >= 0 ? 1u : 0u;
}
/* SAM: per guide and distance the unfiltered count (k{d}:i:), and where its kept positions stand in the of:H: field
 * (off_target_fields, printer.hpp:115-170: the cap counts hits that passed the boundary check) */
__global__ __launch_bounds__(256) void k_tx_sam_guide(tx_args a) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > a.n) return;
  if (g == a.n) {
    a.hex_units[g] = 0;
    return;
  }
  const uint64_t b = a.offsets[g], e = a.offsets[g + 1u];
  uint64_t lo = b;
  uint32_t units = 0;
  bool lines = false;
  for (uint32_t d = 0; d <= a.m; d++) {
    const uint64_t hi = tx_first_at(a.hits, lo, e, d + 1u);
    const uint32_t okc = a.S[hi - a.off0] - a.S[lo - a.off0];
    const uint32_t kept = a.max_off == -1 ? okc : (uint32_t)((long long)okc < a.max_off ? (long long)okc : a.max_off);
    a.cnt[(size_t)g * 8u + d] = (uint32_t)(hi - lo);
    a.sbase[(size_t)g * 8u + d] = a.S[lo - a.off0];
    a.kbase[(size_t)g * 8u + d] = units;
    units += kept + 2u; /* the positions, the distance, the delimiter */
    if (d == 0u) lines = hi > lo && !(a.skip && a.skip[g]); /* a line per distance-0 hit: none, no field */
    lo = hi;
  }
  a.hex_units[g] = (a.complete && lines) ? units : 0u;
}
__device__ __forceinline__ uint4 tx_hex_le(uint64_t v) { /* printer.hpp:18-79: the bytes low to high, two digits each */
  uint32_t w[4];
  for (int j = 0; j < 4; j++) {
    uint32_t x = 0;
    for (int k = 0; k < 2; k++) {
      const uint32_t byte = (uint32_t)(v >> (16 * j + 8 * k)) & 0xFFu;
      const uint32_t hi = byte >> 4, lo = byte & 15u;
      const uint32_t ch = (hi < 10u ? '0' + hi : 'a' + hi - 10u), cl = (lo < 10u ? '0' + lo : 'a' + lo - 10u);
      x |= (ch | (cl << 8)) << (16 * k);
    }
    w[j] = x;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
/* SAM: the of:H: field of every guide that has lines, once, in the scratch span hex[16 * hex_off[g] ...).  No client of the
 * composer, but it walks the same tiles under the same grid (gs_tile_grid): hence its blocks of GS_ROW_WAVES waves */
__global__ __launch_bounds__(WAVE *GS_ROW_WAVES) void k_tx_sam_hex(tx_args a, uint32_t n_tiles) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  uint4 *hex = (uint4 *)a.hex;
  for (uint32_t tile = wave0; tile < n_tiles; tile += n_waves) {
    const uint64_t s0 = (uint64_t)tile * WAVE, s = s0 + lane;
    if (s >= a.slots) continue;
    const uint32_t g = tx_guide_of(a, s0, s);
    const uint64_t units = a.hex_off[g + 1u] - a.hex_off[g], u0 = a.hex_off[g];
    if (units == 0u) continue;
    const uint64_t gs0 = tx_slot_of(a, g);
    const uint32_t *kb = a.kbase + (size_t)g * 8u;
    if (s == gs0) {
      for (uint32_t d = 0; d <= a.m; d++) {
        const uint64_t at = u0 + (d < a.m ? kb[d + 1u] : (uint32_t)units) - 2u;
        hex[at] = tx_hex_le(d);
        hex[at + 1u] = tx_hex_le((uint64_t)a.delim);
      }
      continue;
    }
    const uint64_t h = a.offsets[g] + (s - gs0 - 1u), i = h - a.off0;
    const gs_hit hit = a.hits[h];
    const uint32_t d = (uint32_t)(hit.key >> 61);
    if (d > a.m || a.S[i + 1u] == a.S[i]) continue; /* dropped at a boundary */
    const uint32_t before = a.S[i] - a.sbase[(size_t)g * 8u + d];
    if (a.max_off != -1 && (long long)before >= a.max_off) continue;
    hex[u0 + kb[d] + before] = tx_hex_le((uint64_t)hit.pos);
  }
}

/* where each guide's lines begin in the text: the tile's offset plus the lengths of the slots before the guide's own */
__global__ __launch_bounds__(256) void k_tx_guide_off(const uint64_t *offsets, uint64_t off0, uint32_t n, const uint32_t *lens,
                                                      const uint64_t *tile_off, uint64_t *out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n) return;
  const uint64_t s = offsets[g] - off0 + g, s0 = s & ~(uint64_t)(WAVE - 1u); /* g == n: one past the last slot */
  uint64_t at = tile_off[s / WAVE];
  for (uint64_t i = s0; i < s; i++) at += lens[i];
  out[g] = at;
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
}  // namespace

/* the body of both entry points: ids / id_offsets / senses are host arrays that this call uploads, or d_ids /
 * d_id_offsets / d_senses are in HBM already (the offsets index d_ids as they stand) */
static gs_status format_device(gs_index *ix, const gs_genome_structure *gs, const void *d_guides, uint64_t n, uint32_t L,
                               const void *d_guide_pams, uint32_t P, const char *ids, const uint64_t *id_offsets,
                               const uint8_t *senses, const void *d_ids, const void *d_id_offsets, const void *d_senses,
                               const uint8_t *skip, const void *d_offsets, const void *d_hits, const void *d_specificity,
                               uint32_t mismatches, uint32_t flags, int64_t max_off_targets, void *stream, const void **d_text,
                               uint64_t *text_len) {
  const bool up = d_ids == nullptr; /* the ids come from the host */
  *d_text = nullptr;
  *text_len = 0;
  ix->tx_n = 0;
  if ((flags & GS_TEXT_BAM) && (flags & GS_TEXT_SAM)) return GS_ERR_ARG;
  if ((flags & GS_TEXT_BGZF) && !(flags & GS_TEXT_BAM)) return GS_ERR_ARG;
  const bool features = (flags & GS_TEXT_FEATURES) != 0;
  if (features && (flags & (GS_TEXT_SAM | GS_TEXT_BAM))) return GS_ERR_ARG;
  if (features && !ix->annot) {
    gs_set_error("GS_TEXT_FEATURES without an annotation attached to the handle (gs_index_set_annotation)");
    return GS_ERR_ARG;
  }
  if (n == 0) return GS_OK;
  try {
    hipStream_t st = (hipStream_t)stream;
    GS_HIP(hipSetDevice(ix->device));
    /* the features of every hit, left in the handle's annotation workspace: nothing below touches it */
    const void *d_foff = nullptr, *d_feats = nullptr, *d_gcnt = nullptr;
    if (features)
      GS_TRY(gs_annotate_device_own(ix, ix->annot, gs, n, L, P, mismatches, d_offsets, d_hits, stream, nullptr, &d_foff, &d_feats, &d_gcnt));
    /* what the call uploads: id offsets and bytes, chromosome prefix sums and names, senses, skip */
    const uint64_t id0 = up ? id_offsets[0] : 0, id_bytes = up ? id_offsets[n] - id0 : 0;
    std::vector<uint32_t> name_off(gs->n_chr + 1, 0);
    for (uint32_t c = 0; c < gs->n_chr; c++) name_off[c + 1] = name_off[c] + (uint32_t)strlen(gs->chr_names[c]);
    bump in;
    const size_t i_idoff = in.take(up ? 8 * (n + 1) : 0), i_cum = in.take(8 * ((size_t)gs->n_chr + 1)), i_noff = in.take(4 * ((size_t)gs->n_chr + 1)),
                 i_ids = in.take(id_bytes), i_names = in.take(name_off[gs->n_chr]), i_sense = in.take(senses ? n : 0),
                 i_skip = in.take(skip ? n : 0);
    std::vector<uint8_t> host(in.at + 16);
    {
      uint64_t *po = (uint64_t *)(host.data() + i_idoff);
      for (uint64_t g = 0; up && g <= n; g++) po[g] = id_offsets[g] - id0;
      uint64_t *pc = (uint64_t *)(host.data() + i_cum);
      pc[0] = 0;
      for (uint32_t c = 0; c < gs->n_chr; c++) pc[c + 1] = pc[c] + gs->chr_lengths[c];
      memcpy(host.data() + i_noff, name_off.data(), 4 * name_off.size());
      if (id_bytes) memcpy(host.data() + i_ids, ids + id0, id_bytes);
      for (uint32_t c = 0; c < gs->n_chr; c++) memcpy(host.data() + i_names + name_off[c], gs->chr_names[c], name_off[c + 1] - name_off[c]);
      if (senses) memcpy(host.data() + i_sense, senses, n);
      if (skip) memcpy(host.data() + i_skip, skip, n);
    }
    uint64_t genome = 0;
    for (uint32_t c = 0; c < gs->n_chr; c++) genome += gs->chr_lengths[c];
    GS_TRY(gs_reserve(ix->w_text.in, in.at + 16));
    const uint8_t *din = (const uint8_t *)ix->w_text.in.p;
    GS_HIP(hipMemcpyAsync(ix->w_text.in.p, host.data(), in.at, hipMemcpyHostToDevice, st));
    uint64_t ends[2] = {0, 0};
    GS_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(&ends[1], (const uint64_t *)d_offsets + n, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st)); /* `host` and `ends` are locals */
    if (ends[1] < ends[0]) return GS_ERR_ARG;
    const uint64_t nh = ends[1] - ends[0];
    if (nh && !d_hits) return GS_ERR_ARG;
    ix->tx_n = 0;
    if (nh >= (1ull << 32) && (flags & (GS_TEXT_SAM | GS_TEXT_BAM))) { /* the SAM side tables count hits in 32 bits */
      gs_set_error("gs_format_device: SAM text of 2^32 hits or more in one batch");
      return GS_ERR_UNSUPPORTED;
    }
    const uint64_t slots = nh + n;
    if ((slots + WAVE - 1) / WAVE >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
    const uint32_t n_tiles = (uint32_t)((slots + WAVE - 1) / WAVE);
    const bool bam = (flags & GS_TEXT_BAM) != 0, sam = bam || (flags & GS_TEXT_SAM) != 0, complete = (flags & GS_TEXT_COMPLETE) != 0;

    /* scratch: lengths, tile sums and offsets, the scans' temporary storage, the SAM tables */
    size_t tb_tiles = 0, tb_hits = 0, tb_guides = 0;
    GS_HIP(rocprim::exclusive_scan(nullptr, tb_tiles, (uint64_t *)nullptr, (uint64_t *)nullptr, 0ull, (size_t)n_tiles + 1,
                                   rocprim::plus<uint64_t>(), st));
    if (sam) {
      GS_HIP(rocprim::exclusive_scan(nullptr, tb_hits, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)nh + 1,
                                     rocprim::plus<uint32_t>(), st));
      GS_HIP(rocprim::exclusive_scan(nullptr, tb_guides, (uint64_t *)nullptr, (uint64_t *)nullptr, 0ull, (size_t)n + 1,
                                     rocprim::plus<uint64_t>(), st));
    }
    bump tm;
    const size_t t_err = tm.take(16), t_lens = tm.take(4 * slots), t_tsum = tm.take(8 * ((size_t)n_tiles + 1)),
                 t_toff = tm.take(8 * ((size_t)n_tiles + 1)), tb_scan = std::max(tb_tiles, std::max(tb_hits, tb_guides)), t_scan = tm.take(tb_scan),
                 t_okf = tm.take(sam ? 4 * (nh + 1) : 0), t_S = tm.take(sam ? 4 * (nh + 1) : 0), t_cnt = tm.take(sam ? 32 * n : 0),
                 t_sbase = tm.take(sam ? 32 * n : 0), t_kbase = tm.take(sam ? 32 * n : 0), t_hu = tm.take(sam ? 8 * (n + 1) : 0),
                 t_ho = tm.take(sam ? 8 * (n + 1) : 0);
    GS_TRY(gs_reserve(ix->w_text.tmp, tm.at + 16));
    char *tmp = (char *)ix->w_text.tmp.p;

    tx_args a;
    memset(&a, 0, sizeof a);
    a.guides = (const uint8_t *)d_guides;
    a.pams = (const uint8_t *)d_guide_pams;
    a.ids = up ? din + i_ids : (const uint8_t *)d_ids;
    a.id_off = up ? (const uint64_t *)(din + i_idoff) : (const uint64_t *)d_id_offsets;
    a.senses = senses ? din + i_sense : (const uint8_t *)d_senses;
    a.skip = skip ? din + i_skip : nullptr;
    a.offsets = (const uint64_t *)d_offsets;
    a.hits = (const gs_hit *)d_hits;
    a.spec = (const float *)d_specificity;
    a.chr_cum = (const uint64_t *)(din + i_cum);
    a.chr_names = din + i_names;
    a.chr_name_off = (const uint32_t *)(din + i_noff);
    a.lens = (uint32_t *)(tmp + t_lens);
    a.tile_sum = (uint64_t *)(tmp + t_tsum);
    a.tile_off = (uint64_t *)(tmp + t_toff);
    a.err = (uint32_t *)(tmp + t_err);
    a.okf = (uint32_t *)(tmp + t_okf);
    a.S = (uint32_t *)(tmp + t_S);
    a.cnt = (uint32_t *)(tmp + t_cnt);
    a.sbase = (uint32_t *)(tmp + t_sbase);
    a.kbase = (uint32_t *)(tmp + t_kbase);
    a.hex_units = (uint64_t *)(tmp + t_hu);
    a.hex_off = (uint64_t *)(tmp + t_ho);
    a.slots = slots;
    a.off0 = ends[0];
    a.n_hits = nh;
    a.max_off = (long long)max_off_targets;
    a.delim = -((long long)genome + 1);
    a.n = (uint32_t)n;
    a.L = L;
    a.P = P;
    a.n_chr = gs->n_chr;
    a.m = mismatches;
    a.start = (flags & GS_FLAG_PAM_AT_START) ? 1u : 0u;
    a.sam = sam ? 1u : 0u;
    a.bam = bam ? 1u : 0u;
    a.complete = complete ? 1u : 0u;
    if (features) {
      a.features = 1u;
      a.feat_off = (const uint64_t *)d_foff;
      a.feats = (const uint32_t *)d_feats;
      a.gname_off = ix->annot->d_name_off;
      a.gnames = ix->annot->d_names;
    }

    const uint32_t cus = (uint32_t)gs_num_cus(ix->device);
    const uint32_t grid = gs_tile_grid(n_tiles, cus);
    GS_HIP(hipMemsetAsync(tmp + t_err, 0, 16, st));
    GS_HIP(hipMemsetAsync(a.tile_sum + n_tiles, 0, 8, st));
    if (sam) {
      const uint32_t gh = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nh + 256) / 256, (uint64_t)cus * 32u));
      hipLaunchKernelGGL(k_tx_sam_ok, dim3(gh), dim3(256), 0, st, a);
      GS_TRY(gs_prim_carved("gs_format_device: scan of the hits", tmp + t_scan, tb_scan, [&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, a.okf, a.S, 0u, (size_t)nh + 1, rocprim::plus<uint32_t>(), st);
      }));
      hipLaunchKernelGGL(k_tx_sam_guide, dim3((uint32_t)((n + 256) / 256)), dim3(256), 0, st, a);
      GS_TRY(gs_prim_carved("gs_format_device: scan of the guides' fields", tmp + t_scan, tb_scan, [&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, a.hex_units, a.hex_off, 0ull, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
      }));
      uint64_t units = 0;
      GS_HIP(hipMemcpyAsync(&units, a.hex_off + n, 8, hipMemcpyDeviceToHost, st));
      GS_HIP(hipStreamSynchronize(st));
      if (units) {
        GS_TRY(gs_reserve(ix->w_text.hex, 16 * units + 16));
        a.hex = (char *)ix->w_text.hex.p;
        hipLaunchKernelGGL(k_tx_sam_hex, dim3(grid), dim3(WAVE * GS_ROW_WAVES), 0, st, a, n_tiles);
      }
    }
    hipLaunchKernelGGL(k_tx_len, dim3(grid), dim3(WAVE * GS_ROW_WAVES), 0, st, a, n_tiles);
    GS_TRY(gs_prim_carved("gs_format_device: scan of the tiles", tmp + t_scan, tb_scan, [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, a.tile_sum, a.tile_off, 0ull, (size_t)n_tiles + 1, rocprim::plus<uint64_t>(), st);
    }));
    /* the length and the device's verdict come back together */
    uint64_t total = 0;
    uint32_t err = 0;
    GS_HIP(hipMemcpyAsync(&total, a.tile_off + n_tiles, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    if (err & TX_ERR_ARG) {
      gs_set_error("gs_format_device: a specificity outside [0, 1], a distance beyond `mismatches`, a key that does not decode or id offsets that descend");
      return GS_ERR_ARG;
    }
    if (err & TX_ERR_ID) {
      gs_set_error("gs_format_device: an id of more than 254 bytes: a BAM record's l_read_name is one byte");
      return GS_ERR_ARG;
    }
    if (err & TX_ERR_BIG) {
      gs_set_error("gs_format_device: a line of 32 MB or more");
      return GS_ERR_UNSUPPORTED;
    }
    GS_TRY(gs_reserve(ix->w_text.text, total + 16));
    a.text = (char *)ix->w_text.text.p;
    GS_TRY(gs_reserve(ix->w_text.goff, 8 * (n + 1) + 16));
    if (total) hipLaunchKernelGGL(k_tx_write, dim3(grid), dim3(WAVE * GS_ROW_WAVES), 0, st, a, n_tiles);
    /* where each guide's lines begin (gs_index_last_text_offsets): 8 bytes per guide, kept beside the text */
    hipLaunchKernelGGL(k_tx_guide_off, dim3((uint32_t)((n + 256) / 256)), dim3(256), 0, st, a.offsets, a.off0, a.n, (const uint32_t *)a.lens,
                       (const uint64_t *)a.tile_off, (uint64_t *)ix->w_text.goff.p);
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    *d_text = ix->w_text.text.p;
    *text_len = total;
    ix->tx_n = n;
    /* the records as BGZF members (gs_bgzf.hip): its output is a buffer of its own */
    if (flags & GS_TEXT_BGZF) return gs_bgzf_compress_device(ix, ix->w_text.text.p, total, stream, d_text, text_len);
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_format_device(gs_index *ix, const gs_genome_structure *gs, const void *d_guides, uint64_t n, uint32_t L,
                                      const void *d_guide_pams, uint32_t P, const char *ids, const uint64_t *id_offsets,
                                      const uint8_t *senses, const uint8_t *skip, const void *d_offsets, const void *d_hits,
                                      const void *d_specificity, uint32_t mismatches, uint32_t flags, int64_t max_off_targets,
                                      void *stream, const void **d_text, uint64_t *text_len) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !gs || !d_text || !text_len) return GS_ERR_ARG;
  if (n && (!d_guides || !ids || !id_offsets || !d_offsets || !d_specificity || (P && !d_guide_pams))) return GS_ERR_ARG;
  if (gs->n_chr && (!gs->chr_names || !gs->chr_lengths)) return GS_ERR_ARG;
  if (n >= (1ull << 31) || max_off_targets < -1 || mismatches > 7) return GS_ERR_ARG;
  if (L < 1 || L > 31 || P > 8 || 2 * L + 3 * P > 59) return GS_ERR_ARG;
  for (uint64_t g = 0; g < n; g++)
    if (id_offsets[g + 1] < id_offsets[g]) return GS_ERR_ARG;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (!gs->chr_names[c]) return GS_ERR_ARG;
  return format_device(ix, gs, d_guides, n, L, d_guide_pams, P, ids, id_offsets, senses, nullptr, nullptr, nullptr, skip, d_offsets,
                       d_hits, d_specificity, mismatches, flags, max_off_targets, stream, d_text, text_len);
}

extern "C" gs_status gs_format_device_ids(gs_index *ix, const gs_genome_structure *gs, const void *d_guides, uint64_t n, uint32_t L,
                                          const void *d_guide_pams, uint32_t P, const void *d_ids, const void *d_id_offsets,
                                          const void *d_senses, const uint8_t *skip, const void *d_offsets, const void *d_hits,
                                          const void *d_specificity, uint32_t mismatches, uint32_t flags, int64_t max_off_targets,
                                          void *stream, const void **d_text, uint64_t *text_len) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !gs || !d_text || !text_len) return GS_ERR_ARG;
  if (n && (!d_guides || !d_ids || !d_id_offsets || !d_offsets || !d_specificity || (P && !d_guide_pams))) return GS_ERR_ARG;
  if (gs->n_chr && (!gs->chr_names || !gs->chr_lengths)) return GS_ERR_ARG;
  if (n >= (1ull << 31) || max_off_targets < -1 || mismatches > 7) return GS_ERR_ARG;
  if (L < 1 || L > 31 || P > 8 || 2 * L + 3 * P > 59) return GS_ERR_ARG;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (!gs->chr_names[c]) return GS_ERR_ARG;
  return format_device(ix, gs, d_guides, n, L, d_guide_pams, P, nullptr, nullptr, nullptr, d_ids, d_id_offsets, d_senses, skip,
                       d_offsets, d_hits, d_specificity, mismatches, flags, max_off_targets, stream, d_text, text_len);
}

extern "C" gs_status gs_index_last_text_offsets(gs_index *ix, uint64_t *out, uint64_t n) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !out || ix->tx_n == 0 || n != ix->tx_n) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(ix->device));
  GS_HIP(hipMemcpy(out, ix->w_text.goff.p, 8 * (n + 1), hipMemcpyDeviceToHost));
  return GS_OK;
}
