/* gs_resolve.h -- resolve_absolute (src/genomics/structures.cxx:7-52) by binary search over the prefix sums of the
 * chromosome lengths, for host and device: the one arithmetic behind the device text encoder (gs_textdev.hip: tx_resolve),
 * the annotation kernels (gs_annot.hip) and their host model. */
#ifndef GS_RESOLVE_H
#define GS_RESOLVE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_RS_HD __host__ __device__ __forceinline__
#else
#define GS_RS_HD inline
#endif

struct gs_loc {
  int c; /* chromosome, -1: dropped at a boundary */
  long long s;
  char st;
};
/* chr_cum: n_chr + 1 prefix sums of the chromosome lengths; pos: a hit's signed absolute coordinate */
GS_RS_HD gs_loc gs_resolve_abs(const uint64_t *chr_cum, uint32_t n_chr, uint32_t L, uint32_t P, long long pos) {
  gs_loc r;
  r.c = -1;
  r.s = 0;
  r.st = '+';
  unsigned long long ab = (unsigned long long)pos;
  if (pos < 0) {
    ab = 0ull - ab;
    r.st = '-';
  }
  if (n_chr == 0u || ab >= chr_cum[n_chr]) return r;
  uint32_t lo = 0, hi = n_chr; /* first chromosome whose end exceeds ab */
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ab < chr_cum[mid + 1u])
      hi = mid;
    else
      lo = mid + 1u;
  }
  if (lo >= n_chr) return r;
  const long long in_chr = (long long)(ab - chr_cum[lo]), len = (long long)(chr_cum[lo + 1u] - chr_cum[lo]);
  long long s, e;
  if (r.st == '+') {
    e = in_chr + 1;
    s = e - (long long)L - (long long)P + 1;
  } else {
    s = in_chr + 1;
    e = s + (long long)L + (long long)P - 1;
  }
  if (s < 0 || e > len) return r; /* :46-48, s < 0 not s < 1 */
  r.c = (int)lo;
  r.s = s;
  return r;
}

#endif
