/* gs_repr.h -- Python's repr() of a double in integer arithmetic, one routine for host and device (gs_decode.hip).
 *
 * repr(float) is the shortest digit string that reads back as the same double, the nearest to the value where several
 * are that short, printed in fixed notation for 1e-4 <= |v| < 1e16 (at least `d.d`) and as d[.ddd]e+XX / e-XX (two
 * exponent digits or more) otherwise.  The digits come from the Ryu scheme (Adams, "Ryu: fast float-to-string
 * conversion", PLDI 2018): the double's interval of round-trip values [m-, m+] is scaled by a power of ten as a
 * 64 x 128-bit multiplication with a 125-bit power of five (gs_pow5_table.h, exact, from tools/gen_pow5_tables.py),
 * and digits are dropped while the interval still holds a shorter number.  No floating-point operation is used. */
#ifndef GS_REPR_H
#define GS_REPR_H

#include <stdint.h>

#ifndef __HIPCC__
#define GS_REPR_HD
#else
#define GS_REPR_HD __host__ __device__
#endif

#define GS_REPR_MAX 32 /* bytes a caller provides; the longest result has 24 */

struct gs_pow5_tables {
  const uint64_t (*pow5)[2];
  const uint64_t (*pow5_inv)[2];
};

GS_REPR_HD static inline uint64_t gs_repr_mul64(uint64_t a, uint64_t b, uint64_t *hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umul64hi(a, b);
  return a * b;
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *hi = (uint64_t)(p >> 64);
  return (uint64_t)p;
#endif
}
/* (m * mul) >> j for a 128-bit mul = {low, high}, 64 < j < 128 */
GS_REPR_HD static inline uint64_t gs_repr_mulshift(uint64_t m, const uint64_t *mul, int j) {
  uint64_t high1, high0;
  const uint64_t low1 = gs_repr_mul64(m, mul[1], &high1);
  gs_repr_mul64(m, mul[0], &high0);
  const uint64_t sum = high0 + low1;
  if (sum < high0) high1++;
  const int s = j - 64;
  return (high1 << (64 - s)) | (sum >> s);
}
GS_REPR_HD static inline uint32_t gs_repr_pow5_factor(uint64_t v) {
  uint32_t c = 0;
  while (v && v % 5u == 0u) {
    v /= 5u;
    c++;
  }
  return c;
}
GS_REPR_HD static inline int gs_repr_pow5bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }
GS_REPR_HD static inline int gs_repr_log10pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }
GS_REPR_HD static inline int gs_repr_log10pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }

/* the shortest decimal of a finite non-zero double's magnitude: *digits x 10^*exp10 */
GS_REPR_HD static inline void gs_repr_shortest(uint64_t mant, uint32_t expo, const gs_pow5_tables &t, uint64_t *digits, int *exp10) {
  int e2;
  uint64_t m2;
  if (expo == 0u) {
    e2 = 1 - 1023 - 52 - 2;
    m2 = mant;
  } else {
    e2 = (int)expo - 1023 - 52 - 2;
    m2 = (1ull << 52) | mant;
  }
  const bool accept = (m2 & 1ull) == 0ull;
  const uint64_t mv = 4ull * m2;
  const uint32_t mm_shift = (mant != 0ull || expo <= 1u) ? 1u : 0u;
  uint64_t vr, vp, vm;
  int e10;
  bool vm_tz = false, vr_tz = false;
  if (e2 >= 0) {
    const int q = gs_repr_log10pow2(e2) - (e2 > 3);
    e10 = q;
    const int k = 125 + gs_repr_pow5bits(q) - 1, i = -e2 + q + k;
    vr = gs_repr_mulshift(4ull * m2, t.pow5_inv[q], i);
    vp = gs_repr_mulshift(4ull * m2 + 2ull, t.pow5_inv[q], i);
    vm = gs_repr_mulshift(4ull * m2 - 1ull - mm_shift, t.pow5_inv[q], i);
    if (q <= 21) {
      if (mv % 5ull == 0ull)
        vr_tz = gs_repr_pow5_factor(mv) >= (uint32_t)q;
      else if (accept)
        vm_tz = gs_repr_pow5_factor(mv - 1ull - mm_shift) >= (uint32_t)q;
      else
        vp -= gs_repr_pow5_factor(mv + 2ull) >= (uint32_t)q ? 1ull : 0ull;
    }
  } else {
    const int q = gs_repr_log10pow5(-e2) - (-e2 > 1);
    e10 = q + e2;
    const int i = -e2 - q, k = gs_repr_pow5bits(i) - 125, j = q - k;
    vr = gs_repr_mulshift(4ull * m2, t.pow5[i], j);
    vp = gs_repr_mulshift(4ull * m2 + 2ull, t.pow5[i], j);
    vm = gs_repr_mulshift(4ull * m2 - 1ull - mm_shift, t.pow5[i], j);
    if (q <= 1) {
      vr_tz = true;
      if (accept)
        vm_tz = mm_shift == 1u;
      else
        --vp;
    } else if (q < 63) {
      vr_tz = (mv & ((1ull << q) - 1ull)) == 0ull;
    }
  }
  int removed = 0;
  uint32_t last = 0;
  uint64_t out;
  if (vm_tz || vr_tz) {
    while (vp / 10ull > vm / 10ull) {
      vm_tz &= vm % 10ull == 0ull;
      vr_tz &= last == 0u;
      last = (uint32_t)(vr % 10ull);
      vr /= 10ull;
      vp /= 10ull;
      vm /= 10ull;
      ++removed;
    }
    if (vm_tz) {
      while (vm % 10ull == 0ull) {
        vr_tz &= last == 0u;
        last = (uint32_t)(vr % 10ull);
        vr /= 10ull;
        vp /= 10ull;
        vm /= 10ull;
        ++removed;
      }
    }
    if (vr_tz && last == 5u && vr % 2ull == 0ull) last = 4u; /* exactly half: to even */
    out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5u) ? 1ull : 0ull);
  } else {
    bool up = false;
    while (vp / 10ull > vm / 10ull) {
      up = vr % 10ull >= 5ull;
      vr /= 10ull;
      vp /= 10ull;
      vm /= 10ull;
      ++removed;
    }
    out = vr + ((vr == vm || up) ? 1ull : 0ull);
  }
  *digits = out;
  *exp10 = e10 + removed;
}

/* repr(v) into out (GS_REPR_MAX bytes, not terminated) -> its length */
GS_REPR_HD static inline uint32_t gs_repr_double(uint64_t bits, const gs_pow5_tables &t, char *out) {
  uint32_t n = 0;
  if (bits >> 63) out[n++] = '-';
  const uint64_t mant = bits & ((1ull << 52) - 1ull);
  const uint32_t expo = (uint32_t)(bits >> 52) & 0x7FFu;
  if (expo == 0x7FFu) {
    if (mant) {
      out[0] = 'n', out[1] = 'a', out[2] = 'n';
      return 3;
    }
    out[n++] = 'i', out[n++] = 'n', out[n++] = 'f';
    return n;
  }
  if (expo == 0u && mant == 0ull) {
    out[n++] = '0', out[n++] = '.', out[n++] = '0';
    return n;
  }
  uint64_t dg;
  int e10;
  gs_repr_shortest(mant, expo, t, &dg, &e10);
  char d[20];
  int nd = 0;
  {
    char r[20];
    while (dg) {
      r[nd++] = (char)('0' + (uint32_t)(dg % 10ull));
      dg /= 10ull;
    }
    for (int i = 0; i < nd; i++) d[i] = r[nd - 1 - i];
  }
  while (nd > 1 && d[nd - 1] == '0') { /* digits x 10^e10 with no trailing zero: the value is 0.d1..dn x 10^decpt */
    nd--;
    e10++;
  }
  const int decpt = e10 + nd;
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) {
      out[n++] = '0', out[n++] = '.';
      for (int i = 0; i < -decpt; i++) out[n++] = '0';
      for (int i = 0; i < nd; i++) out[n++] = d[i];
    } else if (decpt >= nd) {
      for (int i = 0; i < nd; i++) out[n++] = d[i];
      for (int i = nd; i < decpt; i++) out[n++] = '0';
      out[n++] = '.', out[n++] = '0';
    } else {
      for (int i = 0; i < decpt; i++) out[n++] = d[i];
      out[n++] = '.';
      for (int i = decpt; i < nd; i++) out[n++] = d[i];
    }
    return n;
  }
  out[n++] = d[0];
  if (nd > 1) {
    out[n++] = '.';
    for (int i = 1; i < nd; i++) out[n++] = d[i];
  }
  out[n++] = 'e';
  int ex = decpt - 1;
  out[n++] = ex < 0 ? '-' : '+';
  if (ex < 0) ex = -ex;
  if (ex >= 100) out[n++] = (char)('0' + ex / 100);
  out[n++] = (char)('0' + ex / 10 % 10);
  out[n++] = (char)('0' + ex % 10);
  return n;
}

#endif
