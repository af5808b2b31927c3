/* gs_annot_scan.h -- the rule of `--annotate` that the host encoders (gs_text.hip), the device kernels (gs_annot.hip) and
 * the host model (gs_debug_annotate_host) share: which groups of a BED file a printed off-target row touches.  The
 * reference has no counterpart: its pipelines (manual/manual.tex:321-656) join the CSV against a BED file in scripts.
 *
 * Footprint of a printed row.  The row's match_position is s, as resolve_absolute returns it (gs_resolve.h); the row
 * occupies the forward-strand bases [s - 1, s - 1 + L + P) of match_chrm, clipped to [0, chromosome length).  The reference
 * prints rows with s == 0 (structures.cxx:46-48 tests s < 0, not s < 1): the clip is what makes that row well defined.  L
 * and P are the guide's own lengths for every row, bulged and alt-PAM hits included: the width the printers resolve with.
 * A hit that resolve_absolute drops has no row, no feature, and is counted nowhere.
 * Feature of a row.  A row has feature g iff its footprint shares at least one base with an interval of group g on that
 * chromosome: overlap, not the containment of `--regions` (gs_regions_scan.h).  A row's features are distinct and ascend
 * by group number, the order of first appearance in the BED file.
 *
 * The table, per chromosome, built on the host: the sorted distinct interval ends (breakpoints) cut the chromosome into
 * elementary segments, segment i = [bp[i], bp[i + 1]); each carries the ascending list of the groups that cover it, the
 * lists stored CSR.  The last breakpoint of a chromosome opens a segment with an empty list, so segments and breakpoints
 * share one index.  A lookup is two binary searches over the breakpoints, for the footprint's first and last base, and a
 * merge of the lists of the segments in between without duplicates.  One segment - nearly every row, a footprint is L + P
 * bases - is a copy of its list: O(log breakpoints + features).  Over k segments (k <= L + P: a segment has a base) every
 * feature costs one binary search per segment: O(log breakpoints + features * k * log depth).  No step depends on
 * intervals that do not touch the footprint, unlike the backward walk of gs_regions_scan.h.  Memory is the sum of the
 * segments' depths; a table of more than GS_AN_MAX_ENTRIES entries is refused before it is allocated. */
#ifndef GS_ANNOT_SCAN_H
#define GS_ANNOT_SCAN_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_AN_HD __host__ __device__ __forceinline__
#else
#define GS_AN_HD inline
#endif

#define GS_AN_MAX_ENTRIES (1ull << 31)
#define GS_AN_NONE 0xFFFFFFFFu

struct gs_an_table { /* every chromosome: 0-based half-open coordinates */
  const uint32_t *chr_bp;  /* n_chr + 1: chromosome c has the breakpoints bp[chr_bp[c] .. chr_bp[c + 1]) */
  const uint32_t *bp;      /* ascending and distinct within a chromosome */
  const uint32_t *seg_off; /* one per breakpoint, and one more: segment i has the groups ent[seg_off[i] .. seg_off[i + 1]) */
  const uint32_t *ent;     /* group numbers, ascending and distinct within a segment */
  uint32_t n_chr;
};

/* the footprint [a, b) of a row printed at s with width w = L + P on a chromosome of len bases; false: no base left */
GS_AN_HD bool gs_an_footprint(long long s, uint32_t w, uint64_t len, uint64_t &a, uint64_t &b) {
  long long lo = s - 1, hi = s - 1 + (long long)w;
  if (lo < 0) lo = 0;
  if (hi > (long long)len) hi = (long long)len;
  a = (uint64_t)lo;
  b = (uint64_t)(hi > 0 ? hi : 0);
  return lo < hi;
}
/* Footprint of a decoded off-target (gs_decode.hip, `decode --annotate`).  A database word gives a chromosome, the
 * coordinate x that the script's map_int_to_coord returns and a strand; the record's stored SEQ has n symbols and the
 * chromosome has ln bases by its @SQ line.  The row occupies the forward-strand bases whose symbols the script slices,
 * [x + 1 - n, x + 1) on '+' and [x, x + n) on '-', clipped to [0, ln): by LN, not by the FASTA record's length, and
 * without Python's wrap of a negative slice start, so a row whose printed sequence is short or wrapped is annotated by
 * where it lies.  These are the L + P bases of the row `enumerate` prints at s = x + 2 - n ('+') or s = x + 1 ('-'), so
 * the two commands give a site the same features.  false: no base left */
GS_AN_HD bool gs_an_decoded_footprint(uint64_t x, bool plus, uint32_t n, uint64_t ln, uint64_t &a, uint64_t &b) {
  return gs_an_footprint(plus ? (long long)x + 2 - (long long)n : (long long)x + 1, n, ln, a, b);
}
/* how many of the n ascending breakpoints are <= q */
GS_AN_HD uint32_t gs_an_count_le(const uint32_t *bp, uint32_t n, uint64_t q) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)bp[mid] <= q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
/* the segments [i0, i1] that hold bases of [a, b), a < b, on chromosome c; false: the footprint lies before the first
 * breakpoint or the chromosome has none */
GS_AN_HD bool gs_an_range(const gs_an_table &t, uint32_t c, uint64_t a, uint64_t b, uint32_t &i0, uint32_t &i1) {
  const uint32_t lo = t.chr_bp[c], n = t.chr_bp[c + 1] - lo;
  const uint32_t k1 = gs_an_count_le(t.bp + lo, n, b - 1);
  if (k1 == 0) return false;
  const uint32_t k0 = gs_an_count_le(t.bp + lo, k1, a); /* a <= b - 1: among the first k1 */
  i0 = lo + (k0 ? k0 - 1 : 0);
  i1 = lo + k1 - 1;
  return true;
}
/* first entry of [b, e) that is >= from, or e */
GS_AN_HD uint32_t gs_an_lower(const uint32_t *ent, uint32_t b, uint32_t e, uint64_t from) {
  while (b < e) {
    const uint32_t mid = b + ((e - b) >> 1);
    if ((uint64_t)ent[mid] < from)
      b = mid + 1;
    else
      e = mid;
  }
  return b;
}
/* f(group) for every distinct group of the segments [i0, i1], ascending; -> how many */
template <class F>
GS_AN_HD uint32_t gs_an_merge(const gs_an_table &t, uint32_t i0, uint32_t i1, F f) {
  if (i0 == i1) {
    const uint32_t b = t.seg_off[i0], e = t.seg_off[i0 + 1];
    for (uint32_t x = b; x < e; x++) f(t.ent[x]);
    return e - b;
  }
  uint32_t cnt = 0;
  uint64_t from = 0;
  for (;;) {
    uint32_t best = GS_AN_NONE;
    for (uint32_t i = i0; i <= i1; i++) {
      const uint32_t e = t.seg_off[i + 1], x = gs_an_lower(t.ent, t.seg_off[i], e, from);
      if (x < e && t.ent[x] < best) best = t.ent[x];
    }
    if (best == GS_AN_NONE) return cnt;
    f(best);
    cnt++;
    from = (uint64_t)best + 1;
  }
}
/* f(group) for every feature of the row printed at s on chromosome c (len bases), ascending; -> how many */
template <class F>
GS_AN_HD uint32_t gs_an_visit(const gs_an_table &t, uint32_t c, long long s, uint32_t w, uint64_t len, F f) {
  uint64_t a, b;
  uint32_t i0, i1;
  if (c >= t.n_chr || !gs_an_footprint(s, w, len, a, b) || !gs_an_range(t, c, a, b, i0, i1)) return 0;
  return gs_an_merge(t, i0, i1, f);
}
GS_AN_HD uint32_t gs_an_count(const gs_an_table &t, uint32_t c, long long s, uint32_t w, uint64_t len) {
  return gs_an_visit(t, c, s, w, len, [](uint32_t) {});
}
/* the same for a decoded off-target at x on chromosome c (ln bases), the record's SEQ of n symbols */
template <class F>
GS_AN_HD uint32_t gs_an_decoded_visit(const gs_an_table &t, uint32_t c, uint64_t x, bool plus, uint32_t n, uint64_t ln, F f) {
  uint64_t a, b;
  uint32_t i0, i1;
  if (c >= t.n_chr || !gs_an_decoded_footprint(x, plus, n, ln, a, b) || !gs_an_range(t, c, a, b, i0, i1)) return 0;
  return gs_an_merge(t, i0, i1, f);
}
GS_AN_HD uint32_t gs_an_decoded_count(const gs_an_table &t, uint32_t c, uint64_t x, bool plus, uint32_t n, uint64_t ln) {
  return gs_an_decoded_visit(t, c, x, plus, n, ln, [](uint32_t) {});
}

/* ---- construction, on the host ------------------------------------------------------------------------------------ */
#include <algorithm>
#include <vector>

struct gs_an_iv {
  uint32_t group, start, end; /* [start, end), start < end */
};
struct gs_an_host {
  std::vector<uint32_t> chr_bp, bp, seg_off, ent;
  uint64_t n_segments = 0; /* elementary segments between the first and last breakpoint of every chromosome */
  gs_an_table table() const { return gs_an_table{chr_bp.data(), bp.data(), seg_off.data(), ent.data(), (uint32_t)(chr_bp.size() - 1)}; }
};
/* per_chr[c]: the intervals of chromosome c in any order; intervals of one group may overlap or abut.  false: the table
 * would hold more than max_entries entries (*need says how many); nothing of that size was allocated */
inline bool gs_an_build(std::vector<std::vector<gs_an_iv>> per_chr, uint64_t max_entries, gs_an_host &out, uint64_t *need) {
  out = gs_an_host();
  out.chr_bp.push_back(0);
  /* breakpoints; per group the intervals merged, so a segment sees a group once */
  for (std::vector<gs_an_iv> &v : per_chr) {
    std::sort(v.begin(), v.end(), [](const gs_an_iv &x, const gs_an_iv &y) {
      return x.group != y.group ? x.group < y.group : x.start != y.start ? x.start < y.start : x.end < y.end;
    });
    size_t m = 0;
    for (const gs_an_iv &x : v) {
      if (m && v[m - 1].group == x.group && x.start <= v[m - 1].end)
        v[m - 1].end = std::max(v[m - 1].end, x.end);
      else
        v[m++] = x;
    }
    v.resize(m);
    std::vector<uint32_t> b;
    for (const gs_an_iv &x : v) {
      b.push_back(x.start);
      b.push_back(x.end);
    }
    std::sort(b.begin(), b.end());
    b.erase(std::unique(b.begin(), b.end()), b.end());
    out.bp.insert(out.bp.end(), b.begin(), b.end());
    out.chr_bp.push_back((uint32_t)out.bp.size());
    if (b.size() > 1) out.n_segments += b.size() - 1;
  }
  /* depths by differences: the size is known before the entries exist */
  std::vector<int64_t> diff(out.bp.size() + 1, 0);
  for (size_t c = 0; c < per_chr.size(); c++) {
    const uint32_t *b = out.bp.data() + out.chr_bp[c], *e = out.bp.data() + out.chr_bp[c + 1];
    for (const gs_an_iv &x : per_chr[c]) {
      diff[(size_t)(std::lower_bound(b, e, x.start) - out.bp.data())]++;
      diff[(size_t)(std::lower_bound(b, e, x.end) - out.bp.data())]--;
    }
  }
  uint64_t total = 0;
  int64_t depth = 0;
  for (size_t i = 0; i < out.bp.size(); i++) {
    depth += diff[i];
    total += (uint64_t)depth;
  }
  if (need) *need = total;
  if (total > max_entries) return false;
  out.seg_off.resize(out.bp.size() + 1);
  depth = 0;
  uint64_t at = 0;
  for (size_t i = 0; i < out.bp.size(); i++) {
    out.seg_off[i] = (uint32_t)at;
    depth += diff[i];
    at += (uint64_t)depth;
  }
  out.seg_off[out.bp.size()] = (uint32_t)at;
  out.ent.resize((size_t)total);
  /* groups ascend within a chromosome's (merged) list: every segment's entries arrive in order */
  std::vector<uint32_t> cursor(out.seg_off.begin(), out.seg_off.end() - 1);
  for (size_t c = 0; c < per_chr.size(); c++) {
    const uint32_t *b = out.bp.data() + out.chr_bp[c], *e = out.bp.data() + out.chr_bp[c + 1];
    for (const gs_an_iv &x : per_chr[c]) {
      const size_t i0 = (size_t)(std::lower_bound(b, e, x.start) - out.bp.data()), i1 = (size_t)(std::lower_bound(b, e, x.end) - out.bp.data());
      for (size_t i = i0; i < i1; i++) out.ent[cursor[i]++] = x.group;
    }
  }
  return true;
}

#endif
