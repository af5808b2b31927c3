/* gs_regions_scan.h -- the rules of `--regions` that the host parser, the device kernels (gs_design.hip) and the host model
 * (gs_debug_design_host) share: which groups of intervals a candidate lies in, and the two words the records are ordered
 * by.  The reference has no counterpart: its pipelines (manual/manual.tex:321-656) filter by coordinate in scripts.
 *
 * A candidate the scan prints at 1-based `position` occupies the forward-strand bases [position - 1, position - 1 + w),
 * w = k + P, whatever its sense and with or without --start (scripts/generate_kmers.py:70-100).  It belongs to a group
 * iff that footprint lies inside one of the group's intervals on its chromosome.  The intervals of one group on one
 * chromosome are merged beforehand where they overlap or abut, so they are disjoint and a footprint lies in at most one
 * of them: a candidate gives at most one record per group.
 *
 * A chromosome's table holds the merged intervals of all groups sorted by start (then end, then group), and for each the
 * largest end among it and those before it.  The intervals that hold q = position - 1 are found from the last start <= q
 * backwards: the walk goes on while that running maximum still reaches q + w, since once it does not, no earlier interval
 * does.  Intervals nested to any depth are found.  The walk ends, but its length depends on the data: it passes every
 * interval that starts at or before q behind the earliest one whose end reaches the footprint, whether it holds q or not.
 * Under one long interval - a whole gene as one group over thousands of exon groups - every candidate of the gene walks
 * back over the exons before it to the gene's start: linear in them, not a fixed bound.  Nobody has measured that case. */
#ifndef GS_REGIONS_SCAN_H
#define GS_REGIONS_SCAN_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_RG_HD __host__ __device__ __forceinline__
#else
#define GS_RG_HD inline
#endif

struct gs_rg_table { /* one chromosome: n intervals, 0-based half-open [start, end) */
  const uint32_t *start, *end, *maxend, *group;
  uint32_t n;
};

/* how many starts are <= q (the starts ascend) */
GS_RG_HD uint32_t gs_rg_count_le(const uint32_t *start, uint32_t n, uint32_t q) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (start[mid] <= q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* f(interval index) for every interval of the table that holds [q, q + w); -> how many */
template <class F>
GS_RG_HD uint32_t gs_rg_visit(const gs_rg_table &t, uint32_t q, uint32_t w, F f) {
  const uint64_t reach = (uint64_t)q + w;
  uint32_t i = gs_rg_count_le(t.start, t.n, q), cnt = 0;
  while (i > 0 && (uint64_t)t.maxend[i - 1] >= reach) {
    --i;
    if ((uint64_t)t.end[i] >= reach) {
      f(i);
      ++cnt;
    }
  }
  return cnt;
}
GS_RG_HD uint32_t gs_rg_count(const gs_rg_table &t, uint32_t q, uint32_t w) {
  return gs_rg_visit(t, q, w, [](uint32_t) {});
}

/* The order of the records: ascending (high word, low word).
 *   high: group << 32 | rankword, rankword = ~bits(specificity) with --per-region (specificity descending: it is a float
 *         in [0, 1], so its bits ascend with it), otherwise 0
 *   low : chromosome << 33 | position << 1 | (sense == '-') */
GS_RG_HD uint32_t gs_rg_float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
GS_RG_HD uint64_t gs_rg_key_high(uint32_t group, int ranked, float specificity) {
  return ((uint64_t)group << 32) | (ranked ? ~gs_rg_float_bits(specificity) : 0u);
}
GS_RG_HD uint64_t gs_rg_key_low(uint32_t chr, uint32_t position, uint8_t sense) {
  return ((uint64_t)chr << 33) | ((uint64_t)position << 1) | (sense == '-' ? 1u : 0u);
}

#endif
