/* gs_controls_scan.h -- the rules of `guidescan controls` (non-targeting controls for a library), stated once for the device
 * passes (k_ct_* of gs_controls.hip), the host twin (gs_debug_controls_host) and the stand-alone check
 * (tools/controls_scan_check.cpp).  No counterpart in the reference: its users draw random protospacers and search them.
 *
 * Candidate.  Candidate i is a 64-bit counter.  For seed s its protospacer is a pure function of (s, i, L), 1 <= L <= 31,
 * with no state and no dependence on batch or device:
 *     mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *              return x ^ x >> 31                                                                    (all mod 2^64)
 *     w = mix(mix(s) ^ i)
 *     base j of the `sequence` column (guide orientation, j from 0) is "ACGT"[(w >> 2j) & 3]
 * mix is a bijection, so one seed never repeats a word; repeats of the low 2L bits do happen and the distance rule deals
 * with them.  The PAM column is the command's pattern.  The packed word of a candidate is w's low 2L bits.
 *
 * Walk.  Candidates are walked in ascending i from `first`; each is charged to the first thing it fails:
 *   1. the sequence rule of gs_select_scan.h (GS_SL_GC, GS_SL_RUN, GS_SL_MOTIF), unchanged;
 *   2. GS_CT_TARGETING: its hit list under the command's -m, PAM, alt PAMs and --start is not empty;
 *   3. GS_CT_CLOSE: it has fewer than H mismatches (Hamming distance over the L letters) to a control already kept.
 * Otherwise it is kept.  The walk stops at the candidate that makes N kept, or after C candidates.  Counts cover the
 * candidates from `first` to the last one looked at, inclusive; the kept list, its order and every count are functions of
 * (s, first, L, PAM, alts, M, start, rule, H, N, C) and the genome only - not of how the device cuts the walk into rounds.
 *
 * Distance.  Two packed words differ at letter j iff bits 2j or 2j + 1 of their XOR are set: fold the odd bits onto the
 * even ones and count.  H = 0 keeps everything, H = 1 drops exact repeats, H > L keeps at most one control.
 *
 * Bounds.  The walk of a round holds the words it has kept in LDS, 8 B each: N <= GS_CT_MAX_N = 16,384 (128 KiB of the CU's
 * 160), for every H.  The distance passes are quadratic - every non-targeting candidate against every control kept so far -
 * and the bound on N is what bounds them: at most N entries per candidate, on one wave within a round. */
#ifndef GS_CONTROLS_SCAN_H
#define GS_CONTROLS_SCAN_H

#include "guidescan_amd.h"
#include "gs_rowtext.h"
#include "gs_select_scan.h"

#define GS_CT_HD GS_RG_HD

#define GS_CT_KEPT 0u /* = GS_SL_PASS; 1, 2, 3 are GS_SL_GC, GS_SL_RUN, GS_SL_MOTIF */
#define GS_CT_TARGETING 4u
#define GS_CT_CLOSE 5u
#define GS_CT_CHARGES 6u
#define GS_CT_MAX_L 31u
#define GS_CT_MAX_N 16384u           /* N at most: a round's kept words fit in LDS */
#define GS_CT_ROUND_DEFAULT (1u << 20)
#define GS_CT_ROUND_MAX (1u << 24)   /* counters of a round at most: a candidate's place in its round is 32 bits */
#define GS_CT_MAX_PREFIX 255u        /* bytes of the id prefix at most */

GS_CT_HD uint64_t gs_ct_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
/* the word of candidate i; seed_mixed = gs_ct_mix(seed) */
GS_CT_HD uint64_t gs_ct_word(uint64_t seed_mixed, uint64_t i) { return gs_ct_mix(seed_mixed ^ i); }
GS_CT_HD uint64_t gs_ct_packed(uint64_t w, uint32_t L) { return w & ((1ull << (2u * L)) - 1ull); }
GS_CT_HD uint8_t gs_ct_base(uint64_t w, uint32_t j) { return (uint8_t)((0x54474341u >> (8u * (uint32_t)((w >> (2u * j)) & 3ull))) & 0xFFu); } /* "ACGT" */
GS_CT_HD void gs_ct_ascii(uint64_t w, uint32_t L, uint8_t *out) {
  for (uint32_t j = 0; j < L; j++) out[j] = gs_ct_base(w, j);
}
/* the letters at which two packed words differ */
GS_CT_HD uint32_t gs_ct_distance(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b;
  const uint64_t f = (x | (x >> 1)) & 0x5555555555555555ull;
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(f);
#else
  return (uint32_t)__builtin_popcountll(f);
#endif
}
GS_CT_HD bool gs_ct_close(uint64_t a, uint64_t b, uint32_t H) { return gs_ct_distance(a, b) < H; }

/* are L, H and N ones the walk takes */
GS_CT_HD bool gs_ct_bounds_ok(uint32_t L, uint32_t H, uint64_t N) {
  (void)H; /* the bound is the same for every H */
  return L >= 1u && L <= GS_CT_MAX_L && N >= 1u && N <= GS_CT_MAX_N;
}

/* a control's id "{prefix}{counter}", or its kmers-file row "id,sequence,pam,NA,0,+\n": the reference's reader wants the
 * three location columns, its printers never look at them (src/genomics/kmer.cxx:9-25, printer.hpp:193,213,326-337) */
template <class S>
GS_RT_HD void gs_ct_row(S &o, const uint8_t *prefix, uint32_t prefix_len, uint64_t counter, const uint8_t *seq, uint32_t L, const uint8_t *pam,
                        uint32_t P, bool rows) {
  o.put(prefix, prefix_len);
  o.u64(counter);
  if (!rows) return;
  o.ch(',');
  o.put(seq, L);
  o.ch(',');
  o.put(pam, P);
  GS_ROW_LIT(o, ",NA,0,+\n");
}

/* The walk itself, one candidate after the other (the host twin and the check; the device passes must give the same).
 * targeting[j] != 0: candidate first + j has a hit.  n_candidates: how many the walk may look at (min of C and what
 * `targeting` covers).  kept_counter / kept_word: room for N.  counts[GS_CT_CHARGES]: per charge, counts[GS_CT_KEPT] the
 * kept.  -> the candidates looked at. */
inline uint64_t gs_ct_walk(uint64_t seed, uint64_t first, uint64_t n_candidates, uint32_t L, const gs_seq_rule *rule, const uint8_t *targeting,
                           uint32_t H, uint64_t N, uint64_t *kept_counter, uint64_t *kept_word, uint64_t *counts) {
  const uint64_t sm = gs_ct_mix(seed);
  for (uint32_t c = 0; c < GS_CT_CHARGES; c++) counts[c] = 0;
  uint64_t kept = 0, looked = 0;
  for (uint64_t j = 0; j < n_candidates && kept < N; j++) {
    const uint64_t w = gs_ct_word(sm, first + j), pw = gs_ct_packed(w, L);
    uint8_t seq[GS_CT_MAX_L];
    gs_ct_ascii(w, L, seq);
    uint32_t ch = rule ? gs_sl_charge(*rule, seq, L) : GS_SL_PASS;
    if (ch == GS_SL_PASS && targeting[j]) ch = GS_CT_TARGETING;
    for (uint64_t t = 0; t < kept && ch == GS_SL_PASS; t++)
      if (gs_ct_close(kept_word[t], pw, H)) ch = GS_CT_CLOSE;
    if (ch == GS_CT_KEPT) {
      kept_counter[kept] = first + j;
      kept_word[kept++] = pw;
    }
    counts[ch]++;
    looked = j + 1;
  }
  return looked;
}

#endif
