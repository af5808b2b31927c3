/* gs_bgzf_inflate.h -- the inflate of one BGZF member (SAMv1 section 4.1; RFC 1951), the inverse of the compressor in
 * gs_bgzf.hip.  One host/device implementation (the way of gs_bgzf_huff.h and gs_bulge_step.h): a lane of
 * k_bgzf_inflate (gs_bgzf_inflate.hip) runs gbi_step between the wave's copies, and the host-only entry point
 * gs_debug_inflate_member and tools/bgzf_inflate_check.cpp run the same text, so the CPU tests and the sanitizers pin
 * what the kernel runs.
 *
 * The decoder is a step function.  A step either reads one block header (and builds the block's code tables) or turns
 * up to GBI_TOKENS symbols into tokens: a literal byte, a match (length, distance), or the bytes of a stored block.
 * It keeps the count of bytes the tokens stand for, so every bound is checked here: a step never issues a token that
 * would write beyond ISIZE or read before the member's first byte, and the code that applies tokens (gbi_apply on the
 * host, the 64 lanes in the kernel) needs no check of its own.  The compressed bytes are read through a window
 * [lo, lo + wlen) of the stream (the kernel keeps 1 KiB of it in LDS; a step needs at most 562 bytes for a dynamic
 * header, 384 for its tokens); a read outside the window is answered with GBI_ERR_WINDOW, one beyond the stream's
 * `len` bytes with GBI_ERR_EOF once its bits are used.
 *
 * What zlib accepts is accepted: several blocks, stored / fixed / dynamic, the repeat symbols 16, 17, 18, codes up to
 * 15 bits, distances up to 32,768, lengths up to 258, an incomplete code that consists of one code of length 1
 * (inftrees.c: "left > 0 && (type == CODES || max != 1)"), a distance code without any symbol as long as no match
 * uses it.  Everything else ends in a reason code. */
#ifndef GS_BGZF_INFLATE_H
#define GS_BGZF_INFLATE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GBI_HD __host__ __device__ __forceinline__
#else
#define GBI_HD static inline
#endif

#define GBI_OK 0u
#define GBI_ERR_BTYPE 1u      /* block type 3 */
#define GBI_ERR_STORED 2u     /* a stored block whose LEN and NLEN disagree */
#define GBI_ERR_OVERSUB 3u    /* an over-subscribed code set */
#define GBI_ERR_INCOMPLETE 4u /* an incomplete code set that is not one code of length 1 */
#define GBI_ERR_NOSYM 5u      /* a code with no symbol met in the stream */
#define GBI_ERR_SYMBOL 6u     /* symbol 286 or 287, or distance code 30 or 31 */
#define GBI_ERR_DIST 7u       /* a distance that reaches before the member's first byte */
#define GBI_ERR_EOF 8u        /* the stream runs out of bytes */
#define GBI_ERR_LONG 9u       /* output longer than ISIZE */
#define GBI_ERR_SHORT 10u     /* output shorter than ISIZE */
#define GBI_ERR_HEADER 11u    /* a dynamic block's header: too many codes, a repeat without a length before it or beyond the
                                 lengths, no end-of-block code */
#define GBI_ERR_TRAIL 12u     /* bytes between the last block and the CRC-32 */
#define GBI_ERR_CRC 13u       /* the CRC-32 of the output is not the trailer's */
#define GBI_ERR_WINDOW 14u    /* internal: a step read outside its window */
#define GBI_ERR_MAGIC 15u     /* the member table: not 1f 8b 08 04 */
#define GBI_ERR_NOBC 16u      /* no BC subfield of two bytes in the extra field */
#define GBI_ERR_BSIZE 17u     /* BSIZE runs past the data, or is smaller than header and trailer */
#define GBI_ERR_ISIZE 18u     /* ISIZE above 65,536 */
#define GBI_N_REASONS 19u

#define GBI_MAX_OUT 65536u
#define GBI_TOKENS 64u    /* tokens of one step: a lane each */
#define GBI_FAST_BITS 9u
#define GBI_TOK_MATCH 0x80000000u  /* | (length - 3) << 16 | (distance - 1) */
#define GBI_TOK_STORED 0x40000000u /* | bytes (1..65535), from byte gbi_state::stored_src of the stream */

#define GBI_MODE_HEADER 0u
#define GBI_MODE_CODES 1u
#define GBI_MODE_STORED 2u
#define GBI_MODE_DONE 3u

/* one canonical code: symbols by (length, value); the first GBI_FAST_BITS bits looked up at once */
struct gbi_huff {
  uint16_t count[16];
  uint16_t sym[288];
  uint16_t fast[1u << GBI_FAST_BITS]; /* symbol << 4 | length, 0: longer than the table or no symbol */
};
struct gbi_work {
  gbi_huff ll, d; /* (d holds the code-length code while a dynamic header is read) */
  uint8_t lens[320];
};
struct gbi_state {
  uint32_t bitpos; /* bits of the stream used */
  uint32_t outpos; /* bytes the tokens issued so far stand for */
  uint32_t mode, last;
  uint32_t stored_src; /* the stored token of the last step: its first byte in the stream */
};
GBI_HD void gbi_state_init(gbi_state *s) {
  s->bitpos = 0;
  s->outpos = 0;
  s->mode = GBI_MODE_HEADER;
  s->last = 0;
  s->stored_src = 0;
}

/* code lengths -> the tables.  codes_type: the code-length code, which may not be incomplete at all */
GBI_HD uint32_t gbi_build(gbi_huff *h, const uint8_t *lens, uint32_t n, bool codes_type) {
  uint32_t offs[16], next[16];
  for (uint32_t l = 0; l < 16u; l++) h->count[l] = 0;
  for (uint32_t i = 0; i < n; i++) h->count[lens[i] & 15u]++;
  for (uint32_t i = 0; i < (1u << GBI_FAST_BITS); i++) h->fast[i] = 0;
  uint32_t max = 0;
  int left = 1;
  for (uint32_t l = 1; l < 16u; l++) {
    left <<= 1;
    left -= (int)h->count[l];
    if (left < 0) return GBI_ERR_OVERSUB;
    if (h->count[l]) max = l;
  }
  h->count[0] = 0;
  if (max == 0u) return GBI_OK; /* no code at all: every use fails (zlib builds a table of invalid codes) */
  if (left > 0 && (codes_type || max != 1u)) return GBI_ERR_INCOMPLETE;
  offs[1] = 0;
  next[1] = 0;
  for (uint32_t l = 1; l < 15u; l++) {
    offs[l + 1u] = offs[l] + h->count[l];
    next[l + 1u] = (next[l] + h->count[l]) << 1;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lens[i] & 15u;
    if (!l) continue;
    h->sym[offs[l]++] = (uint16_t)i;
    const uint32_t code = next[l]++;
    if (l <= GBI_FAST_BITS) {
      uint32_t r = 0;
      for (uint32_t b = 0; b < l; b++) r |= ((code >> b) & 1u) << (l - 1u - b);
      for (uint32_t k = r; k < (1u << GBI_FAST_BITS); k += 1u << l) h->fast[k] = (uint16_t)((i << 4) | l);
    }
  }
  return GBI_OK;
}

/* the symbol the next bits (15 of them, the first in bit 0) begin with -> symbol << 4 | length, or 0: none */
GBI_HD uint32_t gbi_decode(const gbi_huff *h, uint32_t bits) {
  const uint32_t e = h->fast[bits & ((1u << GBI_FAST_BITS) - 1u)];
  if (e) return e;
  int code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16u; l++) {
    code |= (int)((bits >> (l - 1u)) & 1u);
    const int count = (int)h->count[l];
    if (code - count < first) return ((uint32_t)h->sym[index + (code - first)] << 4) | l;
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return 0u;
}

/* the bits of the stream from a byte position on; bytes beyond `len` read as 0 and are an error once used */
struct gbi_bits {
  const uint8_t *win;
  int32_t lo;
  uint32_t wlen, len;
  uint64_t buf;
  uint32_t cnt, next, err;
};
GBI_HD void gbi_refill(gbi_bits *r) { /* afterwards cnt >= 57 */
  while (r->cnt <= 56u) {
    uint64_t b = 0;
    if (r->next < r->len) {
      const int64_t i = (int64_t)r->next - (int64_t)r->lo;
      if (i < 0 || i >= (int64_t)r->wlen)
        r->err = GBI_ERR_WINDOW;
      else
        b = r->win[i];
    }
    r->buf |= b << r->cnt;
    r->cnt += 8u;
    r->next++;
  }
}
GBI_HD uint32_t gbi_bitpos(const gbi_bits *r) { return r->next * 8u - r->cnt; }
GBI_HD uint32_t gbi_take(gbi_bits *r, uint32_t n) { /* n <= 16, n <= cnt */
  const uint32_t v = (uint32_t)r->buf & ((1u << n) - 1u);
  r->buf >>= n;
  r->cnt -= n;
  return v;
}
GBI_HD uint32_t gbi_bits_status(const gbi_bits *r) {
  if (r->err) return r->err;
  return (uint64_t)gbi_bitpos(r) > 8ull * r->len ? GBI_ERR_EOF : GBI_OK;
}

/* lengths 3..258 and distances 1..32768 of the symbols (RFC 1951 section 3.2.5) */
GBI_HD uint32_t gbi_len_base(uint32_t s /* 0..28 */, uint32_t *extra) {
  if (s < 8u) {
    *extra = 0;
    return 3u + s;
  }
  if (s == 28u) {
    *extra = 0;
    return 258u;
  }
  const uint32_t eb = (s - 4u) >> 2;
  *extra = eb;
  return 3u + ((4u + (s & 3u)) << eb);
}
GBI_HD uint32_t gbi_dist_base(uint32_t s /* 0..29 */, uint32_t *extra) {
  if (s < 4u) {
    *extra = 0;
    return 1u + s;
  }
  const uint32_t eb = (s >> 1) - 1u;
  *extra = eb;
  return 1u + ((2u + (s & 1u)) << eb);
}

GBI_HD uint32_t gbi_fixed_tables(gbi_work *w) {
  for (uint32_t i = 0; i < 288u; i++) w->lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : 8u);
  uint32_t rc = gbi_build(&w->ll, w->lens, 288u, false);
  if (rc) return rc;
  for (uint32_t i = 0; i < 32u; i++) w->lens[i] = 5;
  return gbi_build(&w->d, w->lens, 32u, false); /* (30 and 31 have codes: meeting one is GBI_ERR_SYMBOL) */
}

GBI_HD uint32_t gbi_dynamic_tables(gbi_work *w, gbi_bits *r) {
  gbi_refill(r);
  const uint32_t nlen = gbi_take(r, 5) + 257u, ndist = gbi_take(r, 5) + 1u, ncode = gbi_take(r, 4) + 4u;
  if (nlen > 286u || ndist > 30u) return GBI_ERR_HEADER;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (uint32_t i = 0; i < 19u; i++) w->lens[i] = 0;
  for (uint32_t i = 0; i < ncode; i++) {
    gbi_refill(r);
    w->lens[order[i]] = (uint8_t)gbi_take(r, 3);
  }
  uint32_t rc = gbi_build(&w->d, w->lens, 19u, true);
  if (rc) return rc;
  uint32_t i = 0;
  while (i < nlen + ndist) {
    gbi_refill(r);
    const uint32_t e = gbi_decode(&w->d, (uint32_t)r->buf & 0x7FFFu);
    if (!e) return gbi_bits_status(r) ? gbi_bits_status(r) : GBI_ERR_NOSYM;
    gbi_take(r, e & 15u);
    const uint32_t s = e >> 4;
    if (s < 16u) {
      w->lens[i++] = (uint8_t)s;
      continue;
    }
    uint32_t v = 0, rep;
    if (s == 16u) {
      if (i == 0u) return GBI_ERR_HEADER;
      v = w->lens[i - 1u];
      rep = 3u + gbi_take(r, 2);
    } else if (s == 17u) {
      rep = 3u + gbi_take(r, 3);
    } else {
      rep = 11u + gbi_take(r, 7);
    }
    if (i + rep > nlen + ndist) return GBI_ERR_HEADER;
    for (uint32_t k = 0; k < rep; k++) w->lens[i++] = (uint8_t)v;
  }
  if ((rc = gbi_bits_status(r)) != GBI_OK) return rc;
  if (w->lens[256] == 0) return GBI_ERR_HEADER;
  if ((rc = gbi_build(&w->ll, w->lens, nlen, false)) != GBI_OK) return rc;
  return gbi_build(&w->d, w->lens + nlen, ndist, false);
}

/* One step (see the head of this file).  win[0, wlen) are bytes [lo, lo + wlen) of the stream of `len` bytes; the
 * member's output is `isize` bytes (<= GBI_MAX_OUT).  tok[GBI_TOKENS]; *ntok: tokens issued, standing for the output bytes
 * from the value s->outpos had before the call.  Returns a reason; the caller stops at one, or at GBI_MODE_DONE. */
GBI_HD uint32_t gbi_step(gbi_state *s, gbi_work *w, const uint8_t *win, int32_t lo, uint32_t wlen, uint32_t len, uint32_t isize,
                         uint32_t *tok, uint32_t *ntok) {
  *ntok = 0;
  if (s->mode == GBI_MODE_DONE) return GBI_OK;
  gbi_bits r;
  r.win = win;
  r.lo = lo;
  r.wlen = wlen;
  r.len = len;
  r.buf = 0;
  r.cnt = 0;
  r.next = s->bitpos >> 3;
  r.err = 0;
  gbi_refill(&r);
  gbi_take(&r, s->bitpos & 7u);
  uint32_t rc = GBI_OK;
  if (s->mode == GBI_MODE_HEADER) {
    s->last = gbi_take(&r, 1);
    const uint32_t type = gbi_take(&r, 2);
    if (type == 3u) return gbi_bits_status(&r) ? gbi_bits_status(&r) : GBI_ERR_BTYPE;
    if (type == 0u) {
      gbi_take(&r, (8u - (gbi_bitpos(&r) & 7u)) & 7u);
      gbi_refill(&r);
      const uint32_t n = gbi_take(&r, 16), nn = gbi_take(&r, 16);
      if ((rc = gbi_bits_status(&r)) != GBI_OK) return rc;
      if ((n ^ nn) != 0xFFFFu) return GBI_ERR_STORED;
      const uint32_t src = gbi_bitpos(&r) >> 3;
      if ((uint64_t)src + n > len) return GBI_ERR_EOF;
      if ((uint64_t)s->outpos + n > isize) return GBI_ERR_LONG;
      if (n) {
        tok[0] = GBI_TOK_STORED | n;
        *ntok = 1;
        s->stored_src = src;
        s->outpos += n;
      }
      s->bitpos = (src + n) * 8u;
      s->mode = s->last ? GBI_MODE_DONE : GBI_MODE_HEADER;
    } else {
      rc = type == 1u ? gbi_fixed_tables(w) : gbi_dynamic_tables(w, &r);
      if (rc) return rc;
      if ((rc = gbi_bits_status(&r)) != GBI_OK) return rc;
      s->bitpos = gbi_bitpos(&r);
      s->mode = GBI_MODE_CODES;
    }
  } else { /* GBI_MODE_CODES */
    uint32_t n = 0, outpos = s->outpos;
    while (n < GBI_TOKENS) {
      gbi_refill(&r); /* a token takes at most 15 + 5 + 15 + 13 bits */
      uint32_t e = gbi_decode(&w->ll, (uint32_t)r.buf & 0x7FFFu);
      if (!e) return gbi_bits_status(&r) ? gbi_bits_status(&r) : GBI_ERR_NOSYM;
      gbi_take(&r, e & 15u);
      const uint32_t sym = e >> 4;
      if (sym < 256u) {
        if ((rc = gbi_bits_status(&r)) != GBI_OK) return rc;
        if (outpos + 1u > isize) return GBI_ERR_LONG;
        tok[n++] = sym;
        outpos++;
        continue;
      }
      if (sym == 256u) {
        if ((rc = gbi_bits_status(&r)) != GBI_OK) return rc;
        s->mode = s->last ? GBI_MODE_DONE : GBI_MODE_HEADER;
        break;
      }
      if (sym >= 286u) return gbi_bits_status(&r) ? gbi_bits_status(&r) : GBI_ERR_SYMBOL;
      uint32_t eb;
      uint32_t length = gbi_len_base(sym - 257u, &eb);
      length += gbi_take(&r, eb);
      e = gbi_decode(&w->d, (uint32_t)r.buf & 0x7FFFu);
      if (!e) return gbi_bits_status(&r) ? gbi_bits_status(&r) : GBI_ERR_NOSYM;
      gbi_take(&r, e & 15u);
      if ((e >> 4) >= 30u) return gbi_bits_status(&r) ? gbi_bits_status(&r) : GBI_ERR_SYMBOL;
      uint32_t dist = gbi_dist_base(e >> 4, &eb);
      dist += gbi_take(&r, eb);
      if ((rc = gbi_bits_status(&r)) != GBI_OK) return rc;
      if (dist > outpos) return GBI_ERR_DIST;
      if (outpos + length > isize) return GBI_ERR_LONG;
      tok[n++] = GBI_TOK_MATCH | ((length - 3u) << 16) | (dist - 1u);
      outpos += length;
    }
    *ntok = n;
    s->outpos = outpos;
    s->bitpos = gbi_bitpos(&r);
  }
  if (s->mode == GBI_MODE_DONE) {
    if (s->outpos != isize) return GBI_ERR_SHORT; /* (longer has been refused token by token) */
    if (((s->bitpos + 7u) >> 3) != len) return GBI_ERR_TRAIL;
  }
  return GBI_OK;
}

/* the tokens of one step, one after the other: out[at ...], `in` the whole stream */
GBI_HD void gbi_apply(uint8_t *out, uint32_t at, const uint8_t *in, const gbi_state *s, const uint32_t *tok, uint32_t ntok) {
  for (uint32_t t = 0; t < ntok; t++) {
    const uint32_t k = tok[t];
    if (k & GBI_TOK_MATCH) {
      const uint32_t length = ((k >> 16) & 255u) + 3u, dist = (k & 0x7FFFu) + 1u;
      for (uint32_t i = 0; i < length; i++, at++) out[at] = out[at - dist];
    } else if (k & GBI_TOK_STORED) {
      const uint32_t n = k & 0xFFFFu;
      for (uint32_t i = 0; i < n; i++) out[at++] = in[s->stored_src + i];
    } else {
      out[at++] = (uint8_t)k;
    }
  }
}

/* the deflate stream in[0, len) of one member -> out[0, isize); a reason, and *out_len: the bytes the tokens applied so
 * far stand for (isize when the reason is GBI_OK) */
GBI_HD uint32_t gbi_inflate_member(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t isize, gbi_work *w, uint32_t *out_len) {
  *out_len = 0;
  if (isize > GBI_MAX_OUT) return GBI_ERR_ISIZE;
  gbi_state s;
  gbi_state_init(&s);
  uint32_t tok[GBI_TOKENS], ntok = 0;
  /* a step uses at least three bits of the stream or ends it: the guard is never met */
  for (uint64_t guard = 0; guard < 8ull * len + 8ull && s.mode != GBI_MODE_DONE; guard++) {
    const uint32_t at = s.outpos;
    const uint32_t rc = gbi_step(&s, w, in, 0, len, len, isize, tok, &ntok);
    if (rc) return rc;
    gbi_apply(out, at, in, &s, tok, ntok);
    *out_len = s.outpos;
  }
  return s.mode == GBI_MODE_DONE ? GBI_OK : GBI_ERR_WINDOW;
}

/* ---- the member table (host side of gs_bgzf_inflate.hip) ------------------------------------------------------- */
struct gbi_member {
  uint32_t size;      /* BSIZE + 1: the whole member */
  uint32_t cdata_off; /* the deflate stream from the member's first byte: 12 + XLEN */
  uint32_t clen;
  uint32_t crc, isize;
};
/* the member at p, of which `avail` bytes are there (SAMv1 section 4.1): ID1 ID2 CM FLG = 1f 8b 08 04, XLEN, the BC
 * subfield anywhere among the subfields, BSIZE; CRC-32 and ISIZE from the trailer */
GBI_HD uint32_t gbi_walk_member(const uint8_t *p, uint64_t avail, gbi_member *m) {
  if (avail < 12u) return GBI_ERR_BSIZE;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return GBI_ERR_MAGIC;
  const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
  if (12ull + xlen > avail) return GBI_ERR_BSIZE;
  uint32_t q = 12, bsize = 0;
  bool have = false;
  while (q + 4u <= 12u + xlen) {
    const uint32_t slen = (uint32_t)p[q + 2u] | ((uint32_t)p[q + 3u] << 8);
    if (q + 4u + slen > 12u + xlen) break;
    if (p[q] == 'B' && p[q + 1u] == 'C' && slen == 2u && !have) {
      bsize = (uint32_t)p[q + 4u] | ((uint32_t)p[q + 5u] << 8);
      have = true;
    }
    q += 4u + slen;
  }
  if (!have) return GBI_ERR_NOBC;
  const uint32_t size = bsize + 1u;
  if (size > avail || size < 12u + xlen + 8u) return GBI_ERR_BSIZE;
  m->size = size;
  m->cdata_off = 12u + xlen;
  m->clen = size - m->cdata_off - 8u;
  const uint8_t *t = p + size - 8u;
  m->crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  m->isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
  if (m->isize > GBI_MAX_OUT) return GBI_ERR_ISIZE;
  return GBI_OK;
}

GBI_HD const char *gbi_reason_string(uint32_t reason) {
  switch (reason) {
    case GBI_OK: return "no error";
    case GBI_ERR_BTYPE: return "block type 3";
    case GBI_ERR_STORED: return "a stored block whose LEN and NLEN disagree";
    case GBI_ERR_OVERSUB: return "an over-subscribed code set";
    case GBI_ERR_INCOMPLETE: return "an incomplete code set";
    case GBI_ERR_NOSYM: return "a code with no symbol";
    case GBI_ERR_SYMBOL: return "symbol 286 or 287, or distance code 30 or 31";
    case GBI_ERR_DIST: return "a distance that reaches before the member's first byte";
    case GBI_ERR_EOF: return "the deflate stream runs out of bytes";
    case GBI_ERR_LONG: return "output longer than ISIZE";
    case GBI_ERR_SHORT: return "output shorter than ISIZE";
    case GBI_ERR_HEADER: return "a dynamic block's header does not describe two codes";
    case GBI_ERR_TRAIL: return "bytes between the last block and the CRC-32";
    case GBI_ERR_CRC: return "the CRC-32 of the output is not the member's";
    case GBI_ERR_MAGIC: return "no BGZF member header (1f 8b 08 04)";
    case GBI_ERR_NOBC: return "no BC subfield in the extra field";
    case GBI_ERR_BSIZE: return "BSIZE runs past the data";
    case GBI_ERR_ISIZE: return "ISIZE above 65,536";
    default: return "internal: a step read outside its window";
  }
}

#endif
