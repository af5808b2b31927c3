/*
 * gs_bgzf.hip -- BGZF on the device: bytes in HBM -> the gzip members `guidescan enumerate --format bam` writes
 * (host/bam_writer.hpp: bam::bgzf_append, the step the reference's manual leaves to `samtools view -b`,
 * manual/manual.tex:581-582), so that a batch's BAM records (gs_textdev.hip, GS_TEXT_BAM) need not cross the link
 * uncompressed.  The input is cut every 0xff00 bytes; a piece is one member: the 18-byte header with the BC field, one
 * deflate block, CRC-32, ISIZE.
 *
 * One wave takes one piece (k_bgzf_piece); the parallelism is in the pieces, thousands per batch:
 *   matches   64 positions per step, a lane each.  Three tables of last positions are in LDS, by the hash of the next 4, 8
 *             and 16 bytes: the longer the key, the longer the match its last position tends to give, and one candidate
 *             per key stands in for a hash chain.  A step reads the tables before it inserts (atomicMax: the highest
 *             position wins, whatever the order), so a candidate always lies in an earlier step.  Every candidate is
 *             compared against the data, up to 258 bytes; the longest wins, the nearer of two equals.  The wave then walks
 *             the step's candidates greedily from where the last match ended; lanes that start a token write it and
 *             count its symbols (LDS atomics: sums, order free).
 *   codes     lane 0 runs gb_make_plan (gs_bgzf_huff.h): length-limited code lengths, canonical codes, the block's size.
 *             A block that would not be smaller than the stored form is stored.
 *   bits      header fields and tokens are one list of (value, width) items, 64 per step: a scan of the widths gives
 *             the bit offsets, every lane ORs its value into an LDS window, whole words go out, the open word is carried.
 *   CRC-32    every lane folds a slice byte by byte, multiplies by x^(8 * bytes behind the slice) and the wave XORs
 *             (gs_bgzf_crc.h: the inflater checks members with the same routine).
 * k_bgzf_pack then lays the members back to back at the prefix sums of their sizes.
 * Nothing depends on timing: the bytes of member k are a function of piece k alone.  No workgroup waits for another.
 */
#include "gs_device.h"
#include "gs_bgzf_huff.h"
#include "gs_bgzf_crc.h"
#include "gs_scratch.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

#define BZ_PIECE 0xff00u
#define BZ_HASH_BITS 12u /* per table: 3 x 16 KiB, so that three workgroups share a CU's LDS */
#define BZ_TABLES 3u
#define BZ_MIN_LEN 4u    /* the shortest key: a match of three costs more than three literals of text like this */
#define BZ_MAX_DIST 32768u
#define BZ_MAX_LEN 258u
#define BZ_STAGE 0x10000u /* bytes of a piece's deflate stream in the staging area: it is stored from BZ_PIECE + 5 on */
#define BZ_WIN 128u       /* words of the bit writer's window: 64 items of at most 48 bits, and the carried word */
#define BZ_MAX_GRID 1024u /* workgroups, each with a token list of its own */

struct bz_meta {
  uint32_t len;    /* bytes of the deflate stream */
  uint32_t crc;
  uint32_t stored; /* 1: the stream is the stored block of the piece itself, not in the staging area */
  uint32_t pad;
};

typedef uint32_t bz_u32_a1 __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t bz_load4(const uint8_t *p) { return *(const bz_u32_a1 *)p; }

/* bytes that a[] and b[] share, at most lim (<= 258); a < b, b + lim inside the piece */
__device__ __forceinline__ uint32_t bz_match(const uint8_t *a, const uint8_t *b, uint32_t lim) {
  uint32_t l = 0;
  for (uint32_t it = 0; it < BZ_MAX_LEN / 4u && l + 4u <= lim; it++) { /* four bytes at a time */
    const uint32_t x = bz_load4(a + l) ^ bz_load4(b + l);
    if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
    l += 4u;
  }
  for (uint32_t it = 0; it < 4u && l < lim && a[l] == b[l]; it++) l++;
  return l;
}

/* the wave's items of one step into the stream: `bitpos` bits are out or in `carry`, every lane brings nb (<= 48) bits */
__device__ __forceinline__ void bz_emit(uint32_t *win, uint32_t *out32, uint64_t v, uint32_t nb, uint32_t &bitpos, uint32_t &carry) {
  const uint32_t lane = lane_id();
  const uint32_t incl = wave_incl_sum(nb);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
  const uint32_t w0 = bitpos >> 5;
  win[lane] = lane == 0u ? carry : 0u;
  win[lane + WAVE] = 0u;
  __syncthreads();
  if (nb) {
    const uint32_t rel = (bitpos & 31u) + (incl - nb), s = rel & 31u, w = rel >> 5;
    atomicOr(&win[w], (uint32_t)(v << s));
    const uint64_t hi = s ? v >> (32u - s) : v >> 32; /* the bits beyond the first word */
    if ((uint32_t)hi) atomicOr(&win[w + 1u], (uint32_t)hi);
    if ((uint32_t)(hi >> 32)) atomicOr(&win[w + 2u], (uint32_t)(hi >> 32));
  }
  __syncthreads();
  bitpos += total;
  const uint32_t full = (bitpos >> 5) - w0; /* <= 97 */
  if (lane < full && w0 + lane < BZ_STAGE / 4u) out32[w0 + lane] = win[lane]; /* (the caller stores a block that would not fit) */
  if (lane + WAVE < full && w0 + lane + WAVE < BZ_STAGE / 4u) out32[w0 + lane + WAVE] = win[lane + WAVE];
  carry = (bitpos & 31u) ? win[full] : 0u;
  __syncthreads();
}

__global__ __launch_bounds__(WAVE) void k_bgzf_piece(const uint8_t *raw, uint64_t raw_len, uint32_t n_pieces, uint32_t *tokens,
                                                     uint8_t *stage, bz_meta *meta) {
  __shared__ uint32_t s_tab[BZ_TABLES][1u << BZ_HASH_BITS];
  __shared__ uint32_t s_ll[GB_NLL], s_d[GB_ND + 2u], s_work[GB_MAX_SYMS], s_crc[256], s_win[BZ_WIN + 2u];
  __shared__ gb_plan s_plan;
  const uint32_t lane = lane_id();
  uint32_t *tok = tokens + (size_t)blockIdx.x * BZ_PIECE;
  gb_crc_table(s_crc);
  for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
    const uint8_t *d = raw + (uint64_t)piece * BZ_PIECE;
    const uint64_t left = raw_len - (uint64_t)piece * BZ_PIECE;
    const uint32_t n = left < BZ_PIECE ? (uint32_t)left : BZ_PIECE; /* >= 1 */
    for (uint32_t i = lane; i < (BZ_TABLES << BZ_HASH_BITS); i += WAVE) (&s_tab[0][0])[i] = 0u;
    for (uint32_t i = lane; i < GB_NLL; i += WAVE) s_ll[i] = i == 256u ? 1u : 0u; /* one end of block */
    if (lane < GB_ND) s_d[lane] = 0u;
    __syncthreads();

    /* ---- matches and tokens ---- */
    uint32_t cur = 0, ntok = 0; /* the first position no token covers yet; tokens so far */
    for (uint32_t p = 0; p < n; p += WAVE) {
      const uint32_t pos = p + lane;
      const uint32_t room = pos < n ? n - pos : 0u;
      const uint32_t keys = room >= 16u ? 3u : room >= 8u ? 2u : room >= 4u ? 1u : 0u; /* tables this position has a key for */
      uint32_t h[BZ_TABLES] = {0u, 0u, 0u}, mlen = 0, mdist = 0;
      if (keys) {
        const uint32_t w0 = bz_load4(d + pos), w1 = keys >= 2u ? bz_load4(d + pos + 4u) : 0u;
        const uint64_t lo = ((uint64_t)w1 << 32) | w0;
        h[0] = (w0 * 0x9E3779B1u) >> (32u - BZ_HASH_BITS);
        h[1] = (uint32_t)((lo * 0x9E3779B97F4A7C15ull) >> (64u - BZ_HASH_BITS));
        if (keys >= 3u) {
          const uint64_t hi = ((uint64_t)bz_load4(d + pos + 12u) << 32) | bz_load4(d + pos + 8u);
          h[2] = (uint32_t)(((lo * 0x9E3779B97F4A7C15ull) ^ (hi * 0xC2B2AE3D27D4EB4Full)) >> (64u - BZ_HASH_BITS));
        }
        const uint32_t lim = room < BZ_MAX_LEN ? room : BZ_MAX_LEN;
        for (uint32_t k = 0; k < BZ_TABLES; k++) {
          const uint32_t c1 = k < keys ? s_tab[k][h[k]] : 0u; /* position + 1 of an earlier step, or 0 */
          if (!c1 || pos < cur || pos - (c1 - 1u) > BZ_MAX_DIST) continue;
          const uint32_t dist = pos - (c1 - 1u), l = bz_match(d + (c1 - 1u), d + pos, lim);
          if (l >= BZ_MIN_LEN && (l > mlen || (l == mlen && dist < mdist))) {
            mlen = l;
            mdist = dist;
          }
        }
      }
      __syncthreads(); /* the step has read the tables: now it inserts */
      for (uint32_t k = 0; k < BZ_TABLES; k++)
        if (k < keys) atomicMax(&s_tab[k][h[k]], pos + 1u);
      /* greedy walk over the step (wave-uniform): literals up to the next candidate, the candidate, what lies behind it */
      const uint64_t mm = __ballot(mlen != 0u);
      const uint32_t lim = n - p < WAVE ? n - p : WAVE;
      uint32_t c = cur > p ? cur - p : 0u;
      uint64_t starts = 0;
      for (uint32_t it = 0; it < WAVE && c < lim; it++) {
        const uint64_t rest = mm & (~0ull << c);
        const uint32_t nxt = rest ? (uint32_t)__builtin_ctzll(rest) : WAVE; /* candidates lie below lim */
        const uint32_t e = nxt < lim ? nxt : lim;
        starts |= (e == 64u ? ~0ull : (1ull << e) - 1ull) & (~0ull << c); /* literals [c, e) */
        c = e;
        if (nxt < lim) {
          starts |= 1ull << nxt;
          c = nxt + (uint32_t)__shfl((int)mlen, (int)nxt);
        }
      }
      if (p + c > cur) cur = p + c;
      if ((starts >> lane) & 1ull) {
        const uint32_t at = ntok + (uint32_t)__popcll(starts & ((1ull << lane) - 1ull));
        if (mlen) {
          uint32_t eb, ev;
          tok[at] = 0x80000000u | ((mlen - 3u) << 16) | (mdist - 1u);
          atomicAdd(&s_ll[gb_len_sym(mlen, &eb, &ev)], 1u);
          atomicAdd(&s_d[gb_dist_sym(mdist, &eb, &ev)], 1u);
        } else {
          tok[at] = d[pos];
          atomicAdd(&s_ll[d[pos]], 1u);
        }
      }
      ntok += (uint32_t)__popcll(starts);
    }
    __syncthreads();

    /* ---- codes ---- */
    if (lane == 0u) gb_make_plan(s_ll, s_d, &s_plan, s_work);
    __syncthreads();
    const uint32_t dyn_bytes = (s_plan.bits + 7u) >> 3;
    const bool stored = dyn_bytes >= n + 5u;

    /* ---- bits ---- */
    if (!stored) {
      uint32_t *out32 = (uint32_t *)(stage + (size_t)piece * BZ_STAGE);
      const uint32_t hlit = s_plan.hlit, hdist = s_plan.hdist;
      const uint32_t i_cl = 1u, i_len = i_cl + 19u, i_tok = i_len + hlit + hdist, i_eob = i_tok + ntok, n_items = i_eob + 1u;
      uint32_t bitpos = 0, carry = 0;
      for (uint32_t k0 = 0; k0 < n_items; k0 += WAVE) {
        const uint32_t k = k0 + lane;
        uint64_t v = 0;
        uint32_t nb = 0;
        if (k == 0u) { /* BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN = 19 - 4 */
          v = 1u | (2u << 1) | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | (15u << 13);
          nb = 17u;
        } else if (k < i_len) {
          v = gb_clc_order(k - i_cl) < 16u ? 4u : 0u;
          nb = 3u;
        } else if (k < i_tok) {
          const uint32_t j = k - i_len;
          v = gb_rev4(j < hlit ? s_plan.ll_len[j] : s_plan.d_len[j - hlit]);
          nb = 4u;
        } else if (k < i_eob) {
          const uint32_t t = tok[k - i_tok];
          if (t & 0x80000000u) {
            uint32_t eb, ev;
            const uint32_t ls = gb_len_sym(((t >> 16) & 255u) + 3u, &eb, &ev);
            v = s_plan.ll_code[ls];
            nb = s_plan.ll_len[ls];
            v |= (uint64_t)ev << nb;
            nb += eb;
            const uint32_t ds = gb_dist_sym((t & 0x7FFFu) + 1u, &eb, &ev);
            v |= (uint64_t)s_plan.d_code[ds] << nb;
            nb += s_plan.d_len[ds];
            v |= (uint64_t)ev << nb;
            nb += eb;
          } else {
            v = s_plan.ll_code[t];
            nb = s_plan.ll_len[t];
          }
        } else if (k == i_eob) {
          v = s_plan.ll_code[256];
          nb = s_plan.ll_len[256];
        }
        bz_emit(s_win, out32, v, nb, bitpos, carry);
      }
      if (lane == 0u && (bitpos & 31u) && (bitpos >> 5) < BZ_STAGE / 4u) out32[bitpos >> 5] = carry;
    }

    /* ---- CRC-32 ---- */
    const uint32_t crc = gb_crc_wave(d, n, s_crc); /* gs_bgzf_crc.h */
    if (lane == 0u) {
      bz_meta m;
      m.len = stored ? n + 5u : dyn_bytes;
      m.crc = crc;
      m.stored = stored ? 1u : 0u;
      m.pad = 0u;
      meta[piece] = m;
    }
    __syncthreads();
  }
}

/* the size of every member, for the scan */
__global__ __launch_bounds__(256) void k_bgzf_sizes(const bz_meta *meta, uint32_t n_pieces, uint64_t *sizes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_pieces) sizes[i] = i < n_pieces ? 26ull + meta[i].len : 0ull;
}

/* member k at off[k]: header, stream (from the staging area, or the stored block of the piece), CRC-32, ISIZE */
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *raw, uint64_t raw_len, const uint8_t *stage, const bz_meta *meta,
                                                   const uint64_t *off, uint8_t *out) {
  const uint32_t piece = blockIdx.x, t = threadIdx.x;
  const bz_meta m = meta[piece];
  const uint64_t left = raw_len - (uint64_t)piece * BZ_PIECE;
  const uint32_t n = left < BZ_PIECE ? (uint32_t)left : BZ_PIECE;
  uint8_t *o = out + off[piece];
  const uint32_t bsize = m.len + 25u; /* the member's size - 1: at most 0xff00 + 5 + 25 */
  if (t < 18u) {
    const uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255u), (uint8_t)(bsize >> 8)};
    o[t] = head[t];
  }
  if (t < 8u) o[18u + m.len + t] = (uint8_t)((t < 4u ? m.crc >> (8u * t) : n >> (8u * (t - 4u))) & 255u);
  o += 18;
  if (m.stored) {
    if (t < 5u) {
      const uint8_t sh[5] = {1, (uint8_t)(n & 255u), (uint8_t)(n >> 8), (uint8_t)(~n & 255u), (uint8_t)((~n >> 8) & 255u)};
      o[t] = sh[t];
    }
    const uint8_t *d = raw + (uint64_t)piece * BZ_PIECE;
    for (uint32_t i = t; i < n; i += 256u) o[5u + i] = d[i];
  } else {
    const uint8_t *s = stage + (size_t)piece * BZ_STAGE;
    for (uint32_t i = t; i < m.len; i += 256u) o[i] = s[i];
  }
}

extern "C" gs_status gs_bgzf_compress_device(gs_index *ix, const void *d_raw, uint64_t raw_len, void *stream, const void **d_out,
                                             uint64_t *out_len) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !d_out || !out_len || (raw_len && !d_raw)) return GS_ERR_ARG;
  *d_out = nullptr;
  *out_len = 0;
  if (raw_len == 0) return GS_OK;
  const uint64_t np64 = (raw_len + BZ_PIECE - 1) / BZ_PIECE;
  if (np64 >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
  const uint32_t n_pieces = (uint32_t)np64;
  hipStream_t st = (hipStream_t)stream;
  GS_HIP(hipSetDevice(ix->device));
  const uint32_t grid = std::min(n_pieces, BZ_MAX_GRID);
  size_t tb = 0;
  GS_HIP(rocprim::exclusive_scan(nullptr, tb, (uint64_t *)nullptr, (uint64_t *)nullptr, 0ull, (size_t)n_pieces + 1, rocprim::plus<uint64_t>(), st));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t t_tok = 0, t_meta = t_tok + up(4 * (size_t)grid * BZ_PIECE), t_size = t_meta + up(sizeof(bz_meta) * (size_t)n_pieces),
               t_off = t_size + up(8 * ((size_t)n_pieces + 1)), t_scan = t_off + up(8 * ((size_t)n_pieces + 1)), t_stage = t_scan + up(tb),
               t_end = t_stage + (size_t)n_pieces * BZ_STAGE;
  GS_TRY(gs_reserve(ix->w_bgzf.tmp, t_end + 16));
  char *tmp = (char *)ix->w_bgzf.tmp.p;
  bz_meta *meta = (bz_meta *)(tmp + t_meta);
  uint64_t *sizes = (uint64_t *)(tmp + t_size), *off = (uint64_t *)(tmp + t_off);
  hipLaunchKernelGGL(k_bgzf_piece, dim3(grid), dim3(WAVE), 0, st, (const uint8_t *)d_raw, raw_len, n_pieces, (uint32_t *)(tmp + t_tok),
                     (uint8_t *)(tmp + t_stage), meta);
  hipLaunchKernelGGL(k_bgzf_sizes, dim3(n_pieces / 256 + 1), dim3(256), 0, st, (const bz_meta *)meta, n_pieces, sizes);
  GS_TRY(gs_prim_carved("gs_bgzf_compress: scan of the pieces' sizes", tmp + t_scan, tb, [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, sizes, off, 0ull, (size_t)n_pieces + 1, rocprim::plus<uint64_t>(), st);
  }));
  uint64_t total = 0;
  GS_HIP(hipMemcpyAsync(&total, off + n_pieces, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  if (total > (uint64_t)n_pieces * 0x10000ull) { /* a member is at most 64 KiB */
    gs_set_error("gs_bgzf_compress_device: internal: the members' sizes do not add up");
    return GS_ERR_DEVICE;
  }
  GS_TRY(gs_reserve(ix->w_bgzf.out, total + 16));
  hipLaunchKernelGGL(k_bgzf_pack, dim3(n_pieces), dim3(256), 0, st, (const uint8_t *)d_raw, raw_len, (const uint8_t *)(tmp + t_stage),
                     (const bz_meta *)meta, (const uint64_t *)off, (uint8_t *)ix->w_bgzf.out.p);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  *d_out = ix->w_bgzf.out.p;
  *out_len = total;
  return GS_OK;
}

extern "C" gs_status gs_bgzf_compress(gs_index *ix, const void *raw, uint64_t raw_len, uint8_t **out, uint64_t *out_len) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !out || !out_len || (raw_len && !raw)) return GS_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  if (raw_len == 0) return GS_OK;
  GS_HIP(hipSetDevice(ix->device));
  gs_status rc;
  GS_TRY(gs_reserve(ix->w_bgzf.in, raw_len + 16));
  GS_HIP(hipMemcpy(ix->w_bgzf.in.p, raw, raw_len, hipMemcpyHostToDevice));
  const void *d_out = nullptr;
  uint64_t n = 0;
  if ((rc = gs_bgzf_compress_device(ix, ix->w_bgzf.in.p, raw_len, nullptr, &d_out, &n)) != GS_OK) return rc;
  uint8_t *o = (uint8_t *)malloc(n ? n : 1);
  if (!o) return GS_ERR_NOMEM;
  if (hipMemcpy(o, d_out, n, hipMemcpyDeviceToHost) != hipSuccess) {
    free(o);
    gs_set_error("gs_bgzf_compress: copying the members back failed");
    return GS_ERR_DEVICE;
  }
  *out = o;
  *out_len = n;
  return GS_OK;
}

extern "C" gs_status gs_debug_huffman_lengths(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len) {
  if (!freq || !len) return GS_ERR_ARG;
  uint32_t work[GB_MAX_SYMS];
  return gb_huffman_lengths(freq, n, max_len, len, work) ? GS_ERR_ARG : GS_OK;
}

extern "C" float gs_debug_sp_float(uint32_t q) {
  const uint32_t bits = gb_sp_float_bits(q);
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
