/* gs_bgzf_huff.h -- the sequential part of the BGZF compressor (gs_bgzf.hip): from a block's symbol counts to the
 * code lengths, the canonical codes and the size of the dynamic block, and the float a BAM record stores for a printed
 * specificity.  One host/device implementation: a lane of k_bgzf_piece runs it between the match search and the bit
 * writer, and the host-only entry points gs_debug_huffman_lengths / gs_debug_sp_float run the same text, so the CPU
 * tests pin what the kernel runs (the way of gs_bulge_step.h).  Every loop is bounded by the symbol count or by 32. */
#ifndef GS_BGZF_HUFF_H
#define GS_BGZF_HUFF_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GB_HD __host__ __device__ __forceinline__
#else
#define GB_HD static inline
#endif

#define GB_NLL 286u      /* literal/length symbols */
#define GB_ND 30u        /* distance symbols */
#define GB_MAX_SYMS 288u /* the most symbols one call takes: the work array's size */

/* keys[0, n) ascending (heap sort: n log n steps, no recursion) */
GB_HD void gb_sort(uint32_t *keys, uint32_t n) {
  for (uint32_t start = n / 2u; start-- > 0u;) { /* heapify */
    uint32_t root = start;
    for (uint32_t guard = 0; guard < 32u; guard++) {
      uint32_t child = 2u * root + 1u;
      if (child >= n) break;
      if (child + 1u < n && keys[child] < keys[child + 1u]) child++;
      if (keys[root] >= keys[child]) break;
      const uint32_t t = keys[root];
      keys[root] = keys[child];
      keys[child] = t;
      root = child;
    }
  }
  for (uint32_t end = n; end-- > 1u;) {
    const uint32_t t0 = keys[0];
    keys[0] = keys[end];
    keys[end] = t0;
    uint32_t root = 0;
    for (uint32_t guard = 0; guard < 32u; guard++) {
      uint32_t child = 2u * root + 1u;
      if (child >= end) break;
      if (child + 1u < end && keys[child] < keys[child + 1u]) child++;
      if (keys[root] >= keys[child]) break;
      const uint32_t t = keys[root];
      keys[root] = keys[child];
      keys[child] = t;
      root = child;
    }
  }
}

/* Code lengths of a complete prefix code over the symbols with freq != 0, none longer than max_len (<= 15), of least
 * cost among the codes this construction reaches: Huffman's depths in place over the sorted counts (Moffat and
 * Katajainen, "In-place calculation of minimum-redundancy codes", 1995), the counts per length folded at max_len and
 * repaired until the Kraft sum is 1 (one deepest code leaves the last level, one code of the deepest level above it that
 * has one moves a level down next to it), the lengths dealt longest first to the rarest symbols.  One used symbol gets
 * length 1 (the incomplete code inflate accepts); none, all zeros.  freq[i] < 2^23, n <= GB_MAX_SYMS and
 * 2^max_len >= the used symbols; work: n words.  Returns 0, or 1 for arguments outside that. */
GB_HD int gb_huffman_lengths(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len, uint32_t *work) {
  if (n > GB_MAX_SYMS || max_len < 1u || max_len > 15u) return 1;
  uint32_t used = 0;
  for (uint32_t i = 0; i < n; i++) {
    len[i] = 0;
    if (freq[i] >= (1u << 23)) return 1;
    if (freq[i]) work[used++] = (freq[i] << 9) | i;
  }
  if (used == 0u) return 0;
  if (used == 1u) {
    len[work[0] & 511u] = 1;
    return 0;
  }
  if ((used - 1u) >> max_len) return 1;
  gb_sort(work, used);
  /* the in-place algorithm works on the sorted counts alone; the ranks are sorted once more at the end */
  uint32_t *A = work;
  for (uint32_t i = 0; i < used; i++) A[i] >>= 9;
  A[0] += A[1];
  uint32_t root = 0, leaf = 2;
  for (uint32_t next = 1; next + 1u < used; next++) {
    if (leaf >= used || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = next;
    } else
      A[next] = A[leaf++];
    if (leaf >= used || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = next;
    } else
      A[next] += A[leaf++];
  }
  A[used - 2u] = 0;
  for (uint32_t next = used - 2u; next-- > 0u;) A[next] = A[A[next]] + 1u;
  /* codes per depth, what lies deeper than max_len folded into it */
  uint32_t cnt[16];
  for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
  {
    int avbl = 1, usd = 0, r = (int)used - 2;
    uint32_t dpth = 0;
    for (uint32_t guard = 0; guard <= used && avbl > 0; guard++) {
      while (r >= 0 && A[r] == dpth) {
        usd++;
        r--;
      }
      while (avbl > usd) {
        cnt[dpth < max_len ? dpth : max_len]++;
        avbl--;
      }
      avbl = 2 * usd;
      dpth++;
      usd = 0;
    }
  }
  uint32_t total = 0; /* Kraft sum in units of 2^-max_len */
  for (uint32_t l = 1; l <= max_len; l++) total += cnt[l] << (max_len - l);
  for (uint32_t guard = 0; guard < GB_MAX_SYMS && total > (1u << max_len); guard++) {
    cnt[max_len]--;
    for (uint32_t l = max_len - 1u; l > 0u; l--)
      if (cnt[l]) {
        cnt[l]--;
        cnt[l + 1u] += 2u;
        break;
      }
    total--;
  }
  /* the ranks again (the depths overwrote the keys), rarest first: they take the longest codes */
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; i++)
    if (freq[i]) work[k++] = (freq[i] << 9) | i;
  gb_sort(work, used);
  uint32_t at = 0;
  for (uint32_t l = max_len; l >= 1u; l--)
    for (uint32_t c = 0; c < cnt[l] && at < used; c++) len[work[at++] & 511u] = (uint8_t)l;
  return 0;
}

/* canonical codes (RFC 1951 section 3.2.2) with their bits reversed: deflate sends a code from its top bit, the writer
 * ORs values in from bit 0 */
GB_HD void gb_codes(const uint8_t *len, uint32_t n, uint16_t *code) {
  uint32_t cnt[16], next[16];
  for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
  for (uint32_t i = 0; i < n; i++) cnt[len[i]]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (uint32_t l = 1; l < 16u; l++) {
    c = (c + cnt[l - 1u]) << 1;
    next[l] = c;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = len[i];
    uint32_t v = l ? next[l]++ : 0u, r = 0;
    for (uint32_t b = 0; b < l; b++) r |= ((v >> b) & 1u) << (l - 1u - b);
    code[i] = (uint16_t)r;
  }
}

/* length 3..258 -> symbol, extra bits and their value; distance 1..32768 the same (RFC 1951 section 3.2.5) */
GB_HD uint32_t gb_len_sym(uint32_t length, uint32_t *ebits, uint32_t *eval) {
  const uint32_t l = length - 3u;
  if (l < 8u || l == 255u) {
    *ebits = 0;
    *eval = 0;
    return l < 8u ? 257u + l : 285u;
  }
  uint32_t n = 3;
  while ((l >> (n + 1u)) != 0u) n++; /* the top bit of l, 3..7 */
  const uint32_t eb = n - 2u;
  *ebits = eb;
  *eval = l & ((1u << eb) - 1u);
  return 261u + 4u * eb + ((l >> eb) & 3u);
}
GB_HD uint32_t gb_dist_sym(uint32_t dist, uint32_t *ebits, uint32_t *eval) {
  const uint32_t d = dist - 1u;
  if (d < 4u) {
    *ebits = 0;
    *eval = 0;
    return d;
  }
  uint32_t n = 2;
  while ((d >> (n + 1u)) != 0u) n++; /* the top bit of d, 2..14 */
  *ebits = n - 1u;
  *eval = d & ((1u << (n - 1u)) - 1u);
  return 2u * n + ((d >> (n - 1u)) & 1u);
}
GB_HD uint32_t gb_len_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
GB_HD uint32_t gb_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

/* What one dynamic block is made of.  The code-length code is the fixed complete one: symbols 0..15 four bits each (their
 * canonical codes are the values themselves), 16..18 unused, every length written without run-length symbols. */
struct gb_plan {
  uint8_t ll_len[GB_NLL], d_len[GB_ND];
  uint16_t ll_code[GB_NLL], d_code[GB_ND];
  uint32_t hlit, hdist; /* codes sent: 257..286, 1..30 */
  uint32_t bits;        /* the whole block: header, tokens, end of block */
};
/* ll_freq includes the end-of-block count; work: GB_MAX_SYMS words */
GB_HD void gb_make_plan(const uint32_t *ll_freq, const uint32_t *d_freq, gb_plan *p, uint32_t *work) {
  gb_huffman_lengths(ll_freq, GB_NLL, 15u, p->ll_len, work);
  gb_huffman_lengths(d_freq, GB_ND, 15u, p->d_len, work);
  gb_codes(p->ll_len, GB_NLL, p->ll_code);
  gb_codes(p->d_len, GB_ND, p->d_code);
  uint32_t hlit = 257, hdist = 1, bits = 0;
  for (uint32_t i = 0; i < GB_NLL; i++) {
    if (p->ll_len[i] && i >= hlit) hlit = i + 1u;
    bits += ll_freq[i] * (p->ll_len[i] + (i > 256u ? gb_len_extra(i) : 0u));
  }
  for (uint32_t i = 0; i < GB_ND; i++) {
    if (p->d_len[i] && i >= hdist) hdist = i + 1u;
    bits += d_freq[i] * (p->d_len[i] + gb_dist_extra(i));
  }
  p->hlit = hlit;
  p->hdist = hdist;
  p->bits = bits + 17u + 19u * 3u + 4u * (hlit + hdist);
}
/* the order in which the header sends the code-length code's lengths */
GB_HD uint32_t gb_clc_order(uint32_t i) {
  const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}
GB_HD uint32_t gb_rev4(uint32_t v) { return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3); }

/* CRC-32 (reflected 0xEDB88320) as polynomial arithmetic: a * b mod P, and x^(8 n) mod P */
GB_HD uint32_t gb_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32u; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
GB_HD uint32_t gb_crc_shift(uint32_t n_bytes) {
  uint32_t p = 0x80000000u, sq = 0x00800000u; /* x^0, x^8 */
  for (uint32_t i = 0; i < 32u && n_bytes; i++) {
    if (n_bytes & 1u) p = gb_crc_mul(sq, p);
    n_bytes >>= 1;
    sq = gb_crc_mul(sq, sq);
  }
  return p;
}

/* The float nearest to q / 10^6 (ties to even), 0 <= q <= 10^6, as its bits: what strtof makes of the six decimals a SAM
 * line prints, in integer arithmetic.  For q != 0 take e with 2^e <= q / 10^6 < 2^(e+1) and the 24-bit significand
 * m = round(q * 2^(23 - e) / 10^6); q * 2^(23-e) < 10^6 * 2^24 < 2^44 fits 64 bits, and q / 10^6 >= 10^-6 > 2^-20 keeps
 * the result normal.  A significand that rounds up to 2^24 is 2^(e+1) exactly. */
GB_HD uint32_t gb_sp_float_bits(uint32_t q) {
  if (q == 0u) return 0u;
  if (q >= 1000000u) return 0x3F800000u;
  int e = -1; /* q < 10^6: below 1 */
  for (uint32_t guard = 0; guard < 24u && (((uint64_t)q << (uint32_t)(-e)) < 1000000ull); guard++) e--;
  /* now q * 2^-e >= 10^6 and q * 2^(-e-1) < 10^6 ... e is the exponent */
  const uint32_t sh = (uint32_t)(23 - e);
  const uint64_t num = (uint64_t)q << sh;
  uint64_t m = num / 1000000ull;
  const uint64_t rem = num % 1000000ull;
  if (2ull * rem > 1000000ull || (2ull * rem == 1000000ull && (m & 1ull))) m++;
  uint32_t ex = (uint32_t)(e + 127);
  if (m == (1ull << 24)) {
    m >>= 1;
    ex++;
  }
  return (ex << 23) | ((uint32_t)m & 0x7FFFFFu);
}

#endif
