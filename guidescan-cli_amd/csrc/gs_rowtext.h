/* gs_rowtext.h -- what the four device text writers share: the database encoder
 * (gs_textdev.hip), the database decoder (gs_decode.hip), the candidate ids and kmers-file rows (gs_kmers.hip) and the
 * design ids and rows (gs_design.hip, through gs_kmers.hip's writer).  The stand-alone check tools/rowtext_check.cpp runs
 * the host/device part under the address and undefined-behaviour sanitizers.
 *
 * A row is ONE templated function over a sink.  Run over the counting sink it gives the row's length, run over a writing
 * sink it gives the bytes: the two cannot disagree, so a writer never stores past the span its length reserved.
 *
 *   gs_dec_digits            the decimal digits of a number
 *   gs_row_count             the counting sink: ch, put, lit, u64, span
 *   gs_row_write             the writing sink: ch, put, lit, u64
 *   gs_row_write_span        the writing sink with `span`: a copy that is recorded and done by the whole wave afterwards
 *                            (the SAM of:H: field).  A row that calls span does not compile over gs_row_write, and
 *                            gs_tile_write has its span step only for this type: a client without spans pays nothing.
 *   gs_guide_row             a guide's id "{prefix}[{group}:]{chromosome}:{position}:{sense}", or its kmers-file row
 *                            "id,sequence,pam,chromosome,position,sense\n" (scripts/generate_kmers.py:120-125)
 *   gs_tile_len / gs_tile_write   (device only) the tile composer: a tile is 64 consecutive slots, one wavefront.  The
 *                            length pass measures every slot's row and sums the tile; after a 64-bit scan of the tile sums
 *                            the write pass has every lane compose its row into the wave's LDS slice at its offset inside
 *                            the tile, then the wave streams the tile's contiguous span out with 16-byte stores (LDS and HBM
 *                            addresses are congruent mod 16; only the span's ragged head and tail are byte stores).  A tile
 *                            whose span outgrows the slice is composed in HBM directly. */
#ifndef GS_ROWTEXT_H
#define GS_ROWTEXT_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <algorithm>

#include "gs_device.h"
#define GS_RT_HD __host__ __device__ __forceinline__
#else
#define GS_RT_HD inline
#endif

#define GS_ROW_WAVES 4
#define GS_ROW_LDS 12288u         /* bytes of a wave's slice */
#define GS_ROW_MAX_ROW (1u << 25) /* a row of this many bytes or more is refused: 64 of them stay below 2^31 */

GS_RT_HD uint32_t gs_dec_digits(uint64_t v) { /* 1 .. 20 */
  uint32_t k = 1;
  if (v < (1ull << 32)) {
    uint32_t w = (uint32_t)v;
    while (w >= 10u) {
      w /= 10u;
      k++;
    }
    return k;
  }
  while (v >= 10ull) {
    v /= 10ull;
    k++;
  }
  return k;
}

/* ---- the sinks ----------------------------------------------------------------------------------------------- */
struct gs_row_count {
  uint64_t n = 0;
  GS_RT_HD void ch(uint32_t) { n++; }
  template <class K>
  GS_RT_HD void put(const uint8_t *, K k) { n += k; }
  GS_RT_HD void lit(const char *, uint32_t k) { n += k; }
  GS_RT_HD void u64(uint64_t v) { n += gs_dec_digits(v); }
  GS_RT_HD void span(const char *, uint64_t k) { n += k; }
};
struct gs_row_write {
  static constexpr bool spans = false;
  char *p;
  GS_RT_HD void ch(uint32_t c) { *p++ = (char)c; }
  template <class K>
  GS_RT_HD void put(const uint8_t *s, K k) { /* K: the width the client holds the length in */
    for (K i = 0; i < k; i++) p[i] = (char)s[i];
    p += k;
  }
  GS_RT_HD void lit(const char *s, uint32_t k) {
    for (uint32_t i = 0; i < k; i++) p[i] = s[i];
    p += k;
  }
  GS_RT_HD void u64(uint64_t v) {
    const uint32_t k = gs_dec_digits(v);
    char *q = p + k;
    if (v < (1ull << 32)) {
      uint32_t w = (uint32_t)v;
      do {
        *--q = (char)('0' + w % 10u);
        w /= 10u;
      } while (w);
    } else {
      do {
        *--q = (char)('0' + (uint32_t)(v % 10ull));
        v /= 10ull;
      } while (v);
    }
    p += k;
  }
};
struct gs_row_write_span : gs_row_write {
  static constexpr bool spans = true;
  char *sp_dst = nullptr;
  const char *sp_src = nullptr;
  uint64_t sp_n = 0;
  GS_RT_HD void span(const char *s, uint64_t k) {
    sp_dst = p;
    sp_src = s;
    sp_n = k;
    p += k;
  }
};
#define GS_ROW_LIT(o, s) (o).lit(s, (uint32_t)sizeof(s) - 1u)

/* ---- a guide's id or kmers-file row --------------------------------------------------------------------------- */
struct gs_rt_span { /* p == nullptr: none (an empty name is a span of 0 bytes) */
  const uint8_t *p;
  uint32_t n;
};
template <class S>
GS_RT_HD void gs_guide_row(S &o, const uint8_t *names, uint32_t prefix_len, gs_rt_span group, gs_rt_span chr, uint32_t pos, uint8_t sense,
                           const uint8_t *seq, const uint8_t *pam, uint32_t k, uint32_t P, bool rows) {
  o.put(names, prefix_len); /* the prefix opens the name table */
  if (group.p) {
    o.put(group.p, group.n);
    o.ch(':');
  }
  o.put(chr.p, chr.n);
  o.ch(':');
  o.u64(pos);
  o.ch(':');
  o.ch(sense);
  if (!rows) return;
  o.ch(',');
  o.put(seq, k);
  o.ch(',');
  o.put(pam, P);
  o.ch(',');
  o.put(chr.p, chr.n);
  o.ch(',');
  o.u64(pos);
  o.ch(',');
  o.ch(sense);
  o.ch('\n');
}

/* ---- the tile composer ---------------------------------------------------------------------------------------- */
#if defined(__HIPCC__) || defined(__CUDACC__)
/* blocks of WAVE * GS_ROW_WAVES lanes for n_tiles tiles */
static inline uint32_t gs_tile_grid(uint32_t n_tiles, uint32_t cus) {
  return std::max(1u, std::min((n_tiles + GS_ROW_WAVES - 1) / GS_ROW_WAVES, cus * 32u));
}

/* The two passes take the client's kernel arguments `a` and callables WITHOUT captures that get `a` handed on: a closure
 * over the kernel's argument struct makes the compiler hold all of it in registers (k_tx_len: 5 VGPRs and 15 % more code).
 *
 * The length pass, lane per slot: row(a, sink, slot, the tile's first slot, found) over the counting sink - `found` is a word
 * of the client's, 0 at first, for what the row finds wrong - then the client's verdict stands(a, slot, found, too_long) ->
 * whether the row stands (false: its length is 0).  too_long: the row has GS_ROW_MAX_ROW bytes or more and cannot stand;
 * what is recorded for it and for `found` is the client's. */
template <class A, class Row, class Stands>
__device__ __forceinline__ void gs_tile_len(const A &a, uint64_t slots, uint32_t n_tiles, uint32_t *lens, uint64_t *tile_sum, Row row, Stands stands) {
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  for (uint32_t tile = wave0; tile < n_tiles; tile += n_waves) {
    const uint64_t s0 = (uint64_t)tile * WAVE, s = s0 + lane;
    uint32_t len = 0;
    if (s < slots) {
      gs_row_count o;
      uint32_t found = 0;
      row(a, o, s, s0, found);
      len = stands(a, s, found, o.n >= GS_ROW_MAX_ROW) ? (uint32_t)o.n : 0u;
      lens[s] = len;
    }
    const uint32_t incl = wave_incl_sum(len);
    if (lane == WAVE - 1u) tile_sum[tile] = incl;
  }
}

/* The write pass over the sink W (gs_row_write or gs_row_write_span): row(a, sink, slot, the tile's first slot); blocks of
 * WAVE * GS_ROW_WAVES lanes. */
template <class W, class A, class Row>
__device__ __forceinline__ void gs_tile_write(const A &a, uint64_t slots, uint32_t n_tiles, const uint32_t *lens, const uint64_t *tile_off, char *text, Row row) {
  __shared__ __attribute__((aligned(16))) char s_buf[GS_ROW_WAVES][GS_ROW_LDS];
  const uint32_t lane = threadIdx.x & (WAVE - 1u);
  char *buf = s_buf[threadIdx.x / WAVE];
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  for (uint32_t tile = wave0; tile < n_tiles; tile += n_waves) {
    const uint64_t s0 = (uint64_t)tile * WAVE, s = s0 + lane;
    const uint32_t len = s < slots ? lens[s] : 0u;
    const uint32_t incl = wave_incl_sum(len);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
    if (total == 0u) continue;
    const uint64_t base = tile_off[tile];
    const uint32_t a0 = (uint32_t)(base & 15u); /* the slice holds the span at the same address mod 16 as HBM does */
    const bool in_lds = a0 + total <= GS_ROW_LDS;
    W o;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); /* (the tile before has been read out of the slice) */
    if (in_lds) {
      o.p = buf + a0 + (incl - len);
      if (len) row(a, o, s, s0);
    } else {
      o.p = text + base + (incl - len);
      if (len) row(a, o, s, s0);
    }
    if constexpr (W::spans) { /* the recorded spans: one row after the other, 64 bytes per step */
      uint64_t todo = __ballot(o.sp_n != 0ull);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        char *dst = (char *)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)o.sp_dst >> 32), l) << 32) |
                             (uint32_t)__shfl((int)(uint32_t)(uint64_t)o.sp_dst, l));
        const char *src = (const char *)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)o.sp_src >> 32), l) << 32) |
                                         (uint32_t)__shfl((int)(uint32_t)(uint64_t)o.sp_src, l));
        const uint64_t k = ((uint64_t)(uint32_t)__shfl((int)(o.sp_n >> 32), l) << 32) | (uint32_t)__shfl((int)(uint32_t)o.sp_n, l);
        for (uint64_t i = lane; i < k; i += WAVE) dst[i] = src[i];
      }
    }
    if (!in_lds) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    char *out = text + (base - a0); /* 16-byte aligned */
    const uint32_t end = a0 + total, c_first = (a0 + 15u) >> 4, c_last = end >> 4; /* whole 16-byte chunks [c_first, c_last) */
    if (c_first >= c_last) {
      for (uint32_t i = a0 + lane; i < end; i += WAVE) out[i] = buf[i];
    } else {
      for (uint32_t i = a0 + lane; i < c_first * 16u; i += WAVE) out[i] = buf[i];
      for (uint32_t c = c_first + lane; c < c_last; c += WAVE) ((uint4 *)out)[c] = ((const uint4 *)buf)[c];
      for (uint32_t i = c_last * 16u + lane; i < end; i += WAVE) out[i] = buf[i];
    }
  }
}
#endif

#endif
