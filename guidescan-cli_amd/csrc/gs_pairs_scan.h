/* gs_pairs_scan.h -- the rules of `--pairs` that the device kernels (gs_pairs.hip), the host model (gs_debug_pairs_host)
 * and the stand-alone check (tools/pairs_scan_check.cpp) share: where a record cuts, which records of a group are its
 * partners, and the words the pairs are ranked by.  The reference has no counterpart.
 *
 * A record is what gs_design_restrict makes: group, chromosome, 1-based `position`, sense.  Its footprint is the
 * forward-strand bases [q, q + k + P), q = position - 1 (gs_regions_scan.h).
 *
 * PAM side.  pam_right = (sense == '+') != pam_at_start: the protospacer lies in front of the PAM on the forward strand
 * exactly then.  This is `before` of kmers.find_all_kmers (scripts/generate_kmers.py:79-93): (end and forward) or (not end
 * and not forward), with end = not --start.
 *
 * Cut.  The forward-strand boundary x: the cut falls between bases x - 1 and x.  C = cut_offset is the number of
 * protospacer bases between cut and PAM, 0 <= C <= k.  pam_right: x = q + k - C; otherwise x = q + P + C.  Cut and sense
 * determine position, so (chromosome, cut, sense with '+' first) is a total order within a group.
 *
 * Pair.  Two distinct eligible records a, b of one group and one chromosome, a before b in that order, with
 * min_span <= x_b - x_a <= max_span in 64 bits.  Orientation: any; pam-out: a has pam_right false and b true (the PAMs
 * face away from each other); pam-in: the reverse.
 *
 * The records of all groups are sorted by (group, key), key = chromosome << 33 | cut << 1 | (sense == '-').  The partners
 * of the record at place a are then the records of the wanted side in one range [lo, hi) of places behind a: two binary
 * searches.  With the exclusive prefix counts pp of pam_right over the sorted order, the number of partners comes in O(1)
 * and the r-th partner from one more binary search, so no lane ever walks over partners.
 *
 * Rank within a group: min(spec_a, spec_b) descending, then max descending, then the place in the enumeration (a
 * ascending, then b ascending); specificities by their float bits, as gs_rg_key_high. */
#ifndef GS_PAIRS_SCAN_H
#define GS_PAIRS_SCAN_H

#include "gs_regions_scan.h"

#define GS_PR_ANY 0u
#define GS_PR_PAM_OUT 1u
#define GS_PR_PAM_IN 2u

GS_RG_HD bool gs_pr_pam_right(uint8_t sense, bool pam_at_start) { return (sense == '+') != pam_at_start; }

/* the cut of a record; at most position - 1 + k + P, so it fits 32 bits wherever the position does */
GS_RG_HD uint32_t gs_pr_cut(uint32_t position, uint8_t sense, uint32_t k, uint32_t P, uint32_t C, bool pam_at_start) {
  const uint32_t q = position - 1u;
  return gs_pr_pam_right(sense, pam_at_start) ? q + k - C : q + P + C;
}

GS_RG_HD uint64_t gs_pr_key(uint32_t chr, uint32_t cut, uint8_t sense) {
  return ((uint64_t)chr << 33) | ((uint64_t)cut << 1) | (sense == '-' ? 1u : 0u);
}
GS_RG_HD uint32_t gs_pr_key_cut(uint64_t key) { return (uint32_t)(key >> 1); }
GS_RG_HD uint32_t gs_pr_key_chr(uint64_t key) { return (uint32_t)(key >> 33); }

/* the first place in [from, n) whose (group, key) is >= (g, target) - with `beyond`: > (g, target); (group, key) ascend */
GS_RG_HD uint32_t gs_pr_lower(const uint32_t *group, const uint64_t *key, uint32_t from, uint32_t n, uint32_t g, uint64_t target,
                              bool beyond = false) {
  uint32_t lo = from, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint32_t mg = group[mid];
    const uint64_t mk = key[mid];
    if (mg < g || (mg == g && (beyond ? mk <= target : mk < target)))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* [lo, hi): the places behind a, in a's group and chromosome, whose cut lies in [x_a + min_span, x_a + max_span].  The
 * sums are taken in 64 bits; a bound beyond every cut (2^32 - 1) is clamped, so spans near 2^64 are safe. */
GS_RG_HD void gs_pr_range(const uint32_t *group, const uint64_t *key, uint32_t n, uint32_t a, uint64_t min_span, uint64_t max_span,
                          uint32_t *lo, uint32_t *hi) {
  const uint32_t g = group[a];
  const uint64_t ka = key[a], chr_word = ka >> 33 << 33;
  const uint64_t x = gs_pr_key_cut(ka), room = 0xFFFFFFFFull - x;
  if (min_span > room || min_span > max_span) {
    *lo = *hi = a + 1;
    return;
  }
  const uint64_t top = max_span > room ? 0xFFFFFFFFull : x + max_span;
  const uint32_t l = gs_pr_lower(group, key, a + 1, n, g, chr_word | ((x + min_span) << 1));
  const uint32_t h = gs_pr_lower(group, key, l, n, g, chr_word | (top << 1) | 1u, true); /* beyond (chromosome, top, '-') */
  *lo = l;
  *hi = h;
}

/* is the record at a place on the side that the a of a pair must have under the orientation */
GS_RG_HD bool gs_pr_a_side(uint32_t orientation, bool pam_right) {
  return orientation == GS_PR_ANY || (orientation == GS_PR_PAM_OUT ? !pam_right : pam_right);
}

/* the places of [lo, i) that a b of the orientation may have; pp: n + 1 exclusive prefix counts of pam_right */
GS_RG_HD uint32_t gs_pr_side_count(uint32_t orientation, const uint32_t *pp, uint32_t lo, uint32_t i) {
  const uint32_t right = pp[i] - pp[lo];
  return orientation == GS_PR_ANY ? i - lo : orientation == GS_PR_PAM_OUT ? right : (i - lo) - right;
}
/* the partners of the record at a place with range [lo, hi) */
GS_RG_HD uint32_t gs_pr_count(uint32_t orientation, bool a_pam_right, const uint32_t *pp, uint32_t lo, uint32_t hi) {
  if (hi <= lo || !gs_pr_a_side(orientation, a_pam_right)) return 0;
  return gs_pr_side_count(orientation, pp, lo, hi);
}
/* the place of the r-th partner (r from 0, r < gs_pr_count): the first i in [lo, hi) with more than r wanted places in
 * [lo, i + 1) */
GS_RG_HD uint32_t gs_pr_partner(uint32_t orientation, const uint32_t *pp, uint32_t lo, uint32_t hi, uint32_t r) {
  if (orientation == GS_PR_ANY) return lo + r;
  uint32_t l = lo, h = hi;
  while (l < h) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (gs_pr_side_count(orientation, pp, lo, mid + 1) > r)
      h = mid;
    else
      l = mid + 1;
  }
  return l;
}

/* the record that pair t belongs to: the last a with off[a] <= t; off: n + 1 ascending offsets, off[0] <= t < off[n] */
GS_RG_HD uint32_t gs_pr_owner(const uint64_t *off, uint32_t n, uint64_t t) {
  uint32_t lo = 0, hi = n; /* the answer lies in [lo, hi) */
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

/* the rank words of a pair, ascending: group << 32 | ~bits(min), then ~bits(max) */
GS_RG_HD uint64_t gs_pr_word_min(uint32_t group, float sa, float sb) {
  const uint32_t a = gs_rg_float_bits(sa), b = gs_rg_float_bits(sb);
  return ((uint64_t)group << 32) | (uint32_t)~(a < b ? a : b);
}
GS_RG_HD uint32_t gs_pr_word_max(float sa, float sb) {
  const uint32_t a = gs_rg_float_bits(sa), b = gs_rg_float_bits(sb);
  return ~(a < b ? b : a);
}

#endif
