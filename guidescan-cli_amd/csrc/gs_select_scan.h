/* gs_select_scan.h -- the two rules of library selection that the device kernels (k_km_rule of gs_kmers.hip, k_ds_space of
 * gs_design.hip), the host twins (gs_debug_kmers_filter_host, gs_debug_design_host_spaced) and the stand-alone check
 * (tools/select_scan_check.cpp) share: which candidates a sequence rule drops, and which records of a group a minimum
 * spacing between the picks keeps.  No counterpart in the reference: its users filter the genome-wide table in a script.
 *
 * Sequence rule.  Over the k protospacer bytes of a candidate as the kmers file's `sequence` column prints them: guide
 * orientation, for both senses, with and without --start.  The PAM is not looked at; letters compare without regard to
 * case.  With g the number of G and C among the k bytes the candidate passes --gc MIN:MAX iff MIN*k <= 100*g <= MAX*k, in
 * integers; it passes --max-run R iff no letter stands more than R times in a row; it fails --exclude-motif iff some
 * motif matches at some offset, a position matching when the base is in the IUPAC letter's set, so a motif longer than k
 * matches nothing.  --exclude-site adds each motif and its reverse complement.  A motif is stored as one 4-bit set per
 * position (A = 1, C = 2, G = 4, T = 8), two positions to a byte, the even one in the low half.  A failing candidate is
 * charged to the first rule it fails in the order GC, run, motif.
 *
 * Spacing.  Over the record order gs_design_select produces: group, then the rank word, then chromosome, position,
 * sense.  Walk a group's marked records (eligible and, where given, specificity >= S) in that order and keep a record iff
 * every record already kept in this group on the same chromosome has |cut - cut'| >= D, the cut being gs_pr_cut of
 * gs_pairs_scan.h; stop at N kept.  Records on different chromosomes never conflict, a record that is not marked neither
 * counts nor blocks, and a candidate that lies in several groups is spaced in each by itself.  A marked record the walk
 * reaches before the N-th pick and does not keep is "passed over".  The walk is sequential within a group: its cost is
 * the number of records it visits times the length of the kept list, and a group that cannot fill N is visited to its
 * end. */
#ifndef GS_SELECT_SCAN_H
#define GS_SELECT_SCAN_H

#include "guidescan_amd.h"
#include "gs_pairs_scan.h"

#define GS_SL_PASS 0u
#define GS_SL_GC 1u
#define GS_SL_RUN 2u
#define GS_SL_MOTIF 3u
#define GS_SL_MAX_PER_REGION 1024u /* the kept cuts of a group live in LDS, 8 B each */

/* the 4-bit set of a base; 0 for a symbol outside A,C,G,T */
GS_RG_HD uint32_t gs_sl_base_bit(uint8_t c) {
  if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 0u;
}
/* the set of an IUPAC letter over ACGTRYSWKMBDHVN, either case; 0 for any other symbol */
GS_RG_HD uint32_t gs_sl_iupac(uint8_t c) {
  if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  switch (c) {
    case 'A': return 1u;
    case 'C': return 2u;
    case 'G': return 4u;
    case 'T': return 8u;
    case 'R': return 1u | 4u;
    case 'Y': return 2u | 8u;
    case 'S': return 2u | 4u;
    case 'W': return 1u | 8u;
    case 'K': return 4u | 8u;
    case 'M': return 1u | 2u;
    case 'B': return 2u | 4u | 8u;
    case 'D': return 1u | 4u | 8u;
    case 'H': return 1u | 2u | 8u;
    case 'V': return 1u | 2u | 4u;
    case 'N': return 15u;
    default: return 0u;
  }
}
/* the set of the complementary letter: A <-> T and C <-> G swap, so the four bits reverse */
GS_RG_HD uint32_t gs_sl_complement(uint32_t set) {
  return ((set & 1u) << 3) | ((set & 2u) << 1) | ((set & 4u) >> 1) | ((set & 8u) >> 3);
}
GS_RG_HD uint32_t gs_sl_motif_set(const gs_seq_rule &r, uint32_t m, uint32_t p) {
  return (r.motif_set[m][p >> 1] >> ((p & 1u) << 2)) & 15u;
}
GS_RG_HD void gs_sl_motif_put(gs_seq_rule &r, uint32_t m, uint32_t p, uint32_t set) {
  const uint32_t sh = (p & 1u) << 2;
  r.motif_set[m][p >> 1] = (uint8_t)((r.motif_set[m][p >> 1] & ~(15u << sh)) | ((set & 15u) << sh));
}

/* is the rule one gs_kmers_filter takes */
GS_RG_HD bool gs_sl_rule_ok(const gs_seq_rule &r) {
  if (r.gc_min > r.gc_max || r.gc_max > 100u || r.n_motifs > GS_SEQ_MOTIFS) return false;
  for (uint32_t m = 0; m < r.n_motifs; m++) {
    if (r.motif_len[m] < 1u || r.motif_len[m] > GS_SEQ_MOTIF_LETTERS) return false;
    for (uint32_t p = 0; p < r.motif_len[m]; p++)
      if (!gs_sl_motif_set(r, m, p)) return false;
  }
  return true;
}

GS_RG_HD bool gs_sl_motif_at(const gs_seq_rule &r, uint32_t m, const uint8_t *seq, uint32_t offset) {
  const uint32_t len = r.motif_len[m];
  for (uint32_t p = 0; p < len; p++)
    if (!(gs_sl_motif_set(r, m, p) & gs_sl_base_bit(seq[offset + p]))) return false;
  return true;
}

/* the rule a candidate is charged to: GS_SL_PASS, or the first it fails of GS_SL_GC, GS_SL_RUN, GS_SL_MOTIF */
GS_RG_HD uint32_t gs_sl_charge(const gs_seq_rule &r, const uint8_t *seq, uint32_t k) {
  uint32_t gc = 0, run = 0, longest = 0, prev = 0x100u;
  for (uint32_t t = 0; t < k; t++) {
    uint32_t c = seq[t];
    if (c >= 'a' && c <= 'z') c -= 32u;
    gc += (c == 'G' || c == 'C') ? 1u : 0u;
    run = c == prev ? run + 1u : 1u;
    prev = c;
    longest = run > longest ? run : longest;
  }
  if (r.gc_min * k > 100u * gc || 100u * gc > r.gc_max * k) return GS_SL_GC;
  if (r.max_run && longest > r.max_run) return GS_SL_RUN;
  for (uint32_t m = 0; m < r.n_motifs; m++) {
    const uint32_t len = r.motif_len[m];
    if (len > k) continue;
    for (uint32_t o = 0; o + len <= k; o++)
      if (gs_sl_motif_at(r, m, seq, o)) return GS_SL_MOTIF;
  }
  return GS_SL_PASS;
}

/* ---- spacing ----------------------------------------------------------------------------------------------------- */

/* what a record is spaced by: chromosome << 32 | cut */
GS_RG_HD uint64_t gs_sl_key(uint32_t chr, uint32_t position, uint8_t sense, uint32_t k, uint32_t P, uint32_t C, bool pam_at_start) {
  return ((uint64_t)chr << 32) | gs_pr_cut(position, sense, k, P, C, pam_at_start);
}
/* do two records of one group lie too close: one chromosome, cuts fewer than D bases apart */
GS_RG_HD bool gs_sl_conflict(uint64_t a, uint64_t b, uint32_t D) {
  if ((a >> 32) != (b >> 32)) return false;
  const uint32_t x = (uint32_t)a, y = (uint32_t)b;
  return (x < y ? y - x : x - y) < D;
}

/* The walk over one group's n records in order.  key: gs_sl_key of each; mark: nonzero where the record is marked; list:
 * room for min(N, n) keys, the kept ones in the order they were kept.  keep[i] becomes 1 for a kept record and 0 for
 * every other.  -> the number kept; *passed: the marked records passed over; *marked: the marked records of the group. */
GS_RG_HD uint32_t gs_sl_walk(const uint64_t *key, const uint8_t *mark, uint32_t n, uint32_t D, uint32_t N, uint64_t *list, uint8_t *keep,
                             uint32_t *passed, uint32_t *marked) {
  uint32_t kept = 0, over = 0, all = 0;
  for (uint32_t i = 0; i < n; i++) {
    keep[i] = 0;
    if (!mark[i]) continue;
    all++;
    if (kept >= N) continue;
    bool clear = true;
    for (uint32_t t = 0; t < kept && clear; t++) clear = !gs_sl_conflict(list[t], key[i], D);
    if (clear) {
      list[kept++] = key[i];
      keep[i] = 1;
    } else {
      over++;
    }
  }
  *passed = over;
  *marked = all;
  return kept;
}

#endif
