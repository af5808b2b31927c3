/*
 * gs_bamsplit.hip -- the BAM records of a database (SAMv1 section 4.2), inflated in HBM by gs_bgzf_inflate.hip, to the
 * batch arrays of the decoder (gs_decode.hip: ids, stored SEQ, reverse bit, chromosome index, POS-1, the of:H: digits,
 * 64-bit offsets and the word offsets), the inverse of GS_TEXT_BAM (gs_textdev.hip) and the device form of
 * host/decode_cmd.hpp: decode_bam_file, whose checks and words these are.  The fields are those
 * scripts/decode_database.py reads through pysam.
 *
 * Two stages.
 *   starts   k_bs_starts.  A record's block_size names the next start, so the chain is sequential, and it is followed,
 *            not guessed: one workgroup of one wave streams the inflated bytes through a ring of two 16 KiB LDS tiles
 *            (32 KiB of LDS).  The loads of the next tile are issued into registers (16 x 16 bytes a lane) before the
 *            chain is followed through the tile that is there, and are written to LDS behind it, so a hop costs one
 *            LDS read (two words, the size may lie across them) and scalar arithmetic: the position is wave-uniform
 *            and kept in scalar registers.  A record larger than the tiles is jumped over: the next tile loaded is
 *            the one its end lies in.  The starts are collected a lane each and stored 64 at a time.  A chain cannot be
 *            split over workgroups without knowing a start in every part; the per-segment composition (for a segment,
 *            where the chain leaves it for every place it could enter) is the known parallel form and is not built here.
 *   fields   parallel over records, a wave each: k_bs_sizes (the fixed part, the checks, the tag walk over the types
 *            A c C s S i I f Z H B with a wave-wide search for the NUL of a text tag, the last of:H: kept), rocPRIM
 *            exclusive scans of the four sizes, k_bs_fill (read_name without its NUL, the SEQ nibbles as
 *            =ACMGRSVTWYHKDBN letters, the digits).
 * A malformed record leaves (record << 8 | reason) by atomicMin: the first in file order is reported.
 */
#include "gs_device.h"
#include "gs_decoder.h"
#include "gs_scratch.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <chrono>

#define BS_TILE 16384u
#define BS_RING (2u * BS_TILE)
#define BS_WAVES 4u
#define BS_ERR_SHORT 1u
#define BS_ERR_FIELDS 2u
#define BS_ERR_REF 3u
#define BS_ERR_TEXT 4u
#define BS_ERR_ARRAY 5u
#define BS_ERR_TYPE 6u
#define BS_ERR_TAG 7u
#define BS_ERR_CUT 8u
#define BS_ERR_SIZE 9u
#define BS_ERR_ROOM 10u

typedef uint32_t bs_u32_a1 __attribute__((aligned(1)));
typedef uint16_t bs_u16_a1 __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t bs_load4(const uint8_t *p) { return *(const bs_u32_a1 *)p; }
__device__ __forceinline__ uint32_t bs_load2(const uint8_t *p) { return *(const bs_u16_a1 *)p; }

/* res: [0] records, [1] where the chain stopped (the first byte of a cut record, or `total`), [2] the error word */
__global__ __launch_bounds__(WAVE) void k_bs_starts(const uint8_t *d, uint64_t begin, uint64_t total, uint64_t *starts, uint64_t cap,
                                                    unsigned long long *res) {
  __shared__ __attribute__((aligned(16))) uint8_t s_ring[BS_RING];
  const uint32_t lane = lane_id();
  const uint32_t *ring32 = (const uint32_t *)s_ring;
  uint64_t pos = begin, n = 0, mine = 0;
  unsigned long long err = ~0ull;
  uint64_t k = begin / BS_TILE; /* the tile the chain is followed through */
  uint4 regs[BS_TILE / (16u * WAVE)];
  /* tile t: bytes [t * BS_TILE, + BS_TILE) of the buffer, 16 at a time; the buffer has 16 bytes to spare behind `total` */
#pragma unroll
  for (uint32_t i = 0; i < BS_TILE / (16u * WAVE); i++) {
    const uint64_t off = k * BS_TILE + 16ull * (i * WAVE + lane);
    regs[i] = off < total ? *(const uint4 *)(d + off) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (uint32_t i = 0; i < BS_TILE / (16u * WAVE); i++) ((uint4 *)(s_ring + (k & 1u) * BS_TILE))[i * WAVE + lane] = regs[i];
  __syncthreads();
  bool done = false;
  for (uint64_t guard = 0; guard <= total / BS_TILE + 2u && !done; guard++) {
    const uint64_t loaded_end = std::min<uint64_t>(total, (k + 1u) * BS_TILE);
    const uint64_t kn = std::max<uint64_t>(k + 1u, pos / BS_TILE); /* (a record larger than the tiles is jumped over) */
    const bool more = kn * BS_TILE < total;
    if (more) {
#pragma unroll
      for (uint32_t i = 0; i < BS_TILE / (16u * WAVE); i++) {
        const uint64_t off = kn * BS_TILE + 16ull * (i * WAVE + lane);
        regs[i] = off < total ? *(const uint4 *)(d + off) : make_uint4(0, 0, 0, 0);
      }
    }
    /* the chain through what is in LDS: tile k and, for a size that lies across the border, the end of tile k - 1 */
    while (pos + 4u <= loaded_end) {
      const uint32_t idx = (uint32_t)pos & (BS_RING - 1u), w = idx >> 2;
      const uint64_t two = ((uint64_t)ring32[(w + 1u) & (BS_RING / 4u - 1u)] << 32) | ring32[w];
      const uint32_t bs = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(two >> (8u * (idx & 3u))));
      if ((int32_t)bs < 32) {
        err = ((unsigned long long)n << 8) | BS_ERR_SHORT;
        done = true;
        break;
      }
      const uint64_t next = pos + 4u + bs;
      if (next > total) { /* cut by the end of the data */
        done = true;
        break;
      }
      if (n >= cap) { /* (36 bytes a record at least: never) */
        err = ((unsigned long long)n << 8) | BS_ERR_ROOM;
        done = true;
        break;
      }
      if (lane == (uint32_t)(n & 63u)) mine = pos;
      n++;
      if ((n & 63u) == 0u) starts[n - 64u + lane] = mine;
      pos = next;
    }
    if (done || !more) break;
    __syncthreads(); /* the reads of the slot that is overwritten now are over */
#pragma unroll
    for (uint32_t i = 0; i < BS_TILE / (16u * WAVE); i++) ((uint4 *)(s_ring + (kn & 1u) * BS_TILE))[i * WAVE + lane] = regs[i];
    __syncthreads();
    k = kn;
  }
  if (lane < (uint32_t)(n & 63u)) starts[(n & ~63ull) + lane] = mine;
  if (lane == 0u) {
    res[0] = n;
    res[1] = pos;
    res[2] = err;
  }
}

struct bs_args {
  const uint8_t *d;
  const uint64_t *starts;
  const int32_t *ref_to_sq;
  uint64_t *len_id, *len_seq, *len_hex, *len_word; /* n + 1 each, the last 0 */
  uint64_t *hex_src;
  const uint64_t *id_off, *seq_off, *hex_off;
  uint8_t *ids, *seqs, *hex, *reverse;
  int32_t *chr;
  int64_t *pos0;
  unsigned long long *err;
  uint32_t n, n_ref;
};

__device__ __forceinline__ void bs_fail(const bs_args &a, uint32_t r, uint32_t reason) {
  if (lane_id() == 0u) atomicMin(a.err, ((unsigned long long)r << 8) | reason);
}

/* one record by one wave: every value here is wave-uniform but the bytes of the text-tag search */
__global__ __launch_bounds__(WAVE *BS_WAVES) void k_bs_sizes(bs_args a) {
  const uint32_t lane = lane_id();
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  for (uint32_t r = wave0; r <= a.n; r += n_waves) {
    uint64_t l_id = 0, l_sq = 0, l_hx = 0, hsrc = 0;
    int32_t chr = -1;
    int64_t pos0 = 0;
    uint32_t rev = 0;
    if (r < a.n) {
      const uint8_t *rec = a.d + a.starts[r] + 4u;
      const uint64_t size = bs_load4(rec - 4u); /* >= 32: k_bs_starts */
      const int32_t ref_id = (int32_t)bs_load4(rec), pos = (int32_t)bs_load4(rec + 4u), l_seq = (int32_t)bs_load4(rec + 16u);
      const uint32_t l_name = rec[8], n_cigar = bs_load2(rec + 12u), flag = bs_load2(rec + 14u);
      uint64_t p = 32;
      uint32_t bad = 0;
      if (l_name < 1u || l_seq < 0 || p + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + (uint64_t)l_seq > size)
        bad = BS_ERR_FIELDS;
      else if (ref_id >= (int32_t)a.n_ref)
        bad = BS_ERR_REF;
      if (!bad) {
        l_id = l_name - 1u;
        l_sq = (uint64_t)l_seq;
        rev = (flag & 16u) ? 1u : 0u;
        const int32_t m = ref_id < 0 ? -1 : a.ref_to_sq[ref_id];
        chr = m < 0 ? -1 : m;
        pos0 = pos;
        p += l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + (uint64_t)l_seq;
        for (uint64_t guard = 0; guard < size && p + 3u <= size; guard++) { /* the tags: the last of:H: */
          const uint32_t t0 = rec[p], t1 = rec[p + 1u], ty = rec[p + 2u];
          p += 3u;
          uint64_t sz = 0;
          if (ty == 'Z' || ty == 'H') {
            uint64_t at = size; /* where the NUL is */
            for (uint64_t q = p; q < size && at == size; q += WAVE) {
              const uint64_t hit = __ballot(q + lane < size && rec[q + lane] == 0);
              if (hit) at = q + (uint64_t)(__ffsll((long long)hit) - 1);
            }
            if (at == size) {
              bad = BS_ERR_TEXT;
              break;
            }
            sz = at - p;
            if (t0 == 'o' && t1 == 'f' && ty == 'H') {
              hsrc = a.starts[r] + 4u + p;
              l_hx = sz;
            }
            sz += 1u;
          } else if (ty == 'B') {
            if (p + 5u > size) {
              bad = BS_ERR_ARRAY;
              break;
            }
            const uint32_t sub = rec[p];
            const int32_t cnt = (int32_t)bs_load4(rec + p + 1u);
            const uint64_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : 4u;
            sz = 5u + w * (uint64_t)(cnt < 0 ? 0 : cnt);
          } else {
            sz = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : 0u;
            if (!sz) {
              bad = BS_ERR_TYPE;
              break;
            }
          }
          if (p + sz > size) {
            bad = BS_ERR_TAG;
            break;
          }
          p += sz;
        }
      }
      if (bad) {
        bs_fail(a, r, bad);
        l_id = l_sq = l_hx = 0;
      }
    }
    if (lane == 0u) {
      a.len_id[r] = l_id;
      a.len_seq[r] = l_sq;
      a.len_hex[r] = l_hx;
      a.len_word[r] = l_hx / 16u;
      if (r < a.n) {
        a.hex_src[r] = hsrc;
        a.chr[r] = chr;
        a.pos0[r] = pos0;
        a.reverse[r] = (uint8_t)rev;
      }
    }
  }
}

__global__ __launch_bounds__(WAVE *BS_WAVES) void k_bs_fill(bs_args a) {
  const uint32_t lane = lane_id();
  const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, n_waves = gridDim.x * blockDim.x / WAVE;
  for (uint32_t r = wave0; r < a.n; r += n_waves) {
    const uint8_t *rec = a.d + a.starts[r] + 4u;
    const uint64_t i0 = a.id_off[r], l_id = a.id_off[r + 1u] - i0, s0 = a.seq_off[r], l_sq = a.seq_off[r + 1u] - s0, h0 = a.hex_off[r],
                   l_hx = a.hex_off[r + 1u] - h0;
    for (uint64_t i = lane; i < l_id; i += WAVE) a.ids[i0 + i] = rec[32u + i];
    const uint8_t *sq = rec + 32u + rec[8] + 4ull * bs_load2(rec + 12u);
    for (uint64_t i = lane; i < l_sq; i += WAVE) a.seqs[s0 + i] = (uint8_t)"=ACMGRSVTWYHKDBN"[(sq[i >> 1] >> ((i & 1u) ? 0u : 4u)) & 15u];
    const uint8_t *hx = a.d + a.hex_src[r];
    for (uint64_t i = lane; i < l_hx; i += WAVE) a.hex[h0 + i] = hx[i];
  }
}

namespace {
struct bump {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t r = at;
    at += (bytes + 255) & ~(size_t)255;
    return r;
  }
};
const char *const bs_reasons[] = {"",
                                  "a record shorter than its fixed part",
                                  "a record's fields outrun it",
                                  "a record's reference is beyond the list",
                                  "a text tag without its end",
                                  "an array tag",
                                  "a tag of unknown type",
                                  "a tag outruns its record",
                                  "a record is cut",
                                  "a record's size",
                                  "internal: more records than their bytes allow"};
gs_status bs_record_error(uint64_t record, uint32_t reason) {
  gs_set_error("gs_decode_bam: record " + std::to_string(record) + ": " + bs_reasons[reason <= BS_ERR_ROOM ? reason : 0]);
  return reason == BS_ERR_ROOM ? GS_ERR_DEVICE : GS_ERR_FORMAT;
}
double ms_since(const std::chrono::steady_clock::time_point &t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

gs_status decode_bam_device(gs_decoder *d, const void *bgzf, uint64_t len, uint64_t skip, const int32_t *ref_to_sq, uint32_t n_ref,
                            uint32_t flags, uint64_t first_record, const void **d_text, uint64_t *text_len, uint64_t *n_records,
                            uint64_t *tail) {
  hipStream_t st = nullptr;
  gs_status rc;
  /* ---- inflate, the cut record of the call before in front ---- */
  auto t0 = std::chrono::steady_clock::now();
  const uint64_t keep = skip ? 0 : d->bam_tail; /* a header begins a file: nothing is kept from another one */
  const void *d_bytes = nullptr;
  uint64_t total = 0, n_members = 0;
  if ((rc = gs_bgzf_inflate_device(d, bgzf, len, keep, &d_bytes, &total, &n_members)) != GS_OK) return rc;
  d->last_bam[0] = n_members;
  d->last_bam[1] = len;
  d->last_bam[2] = total - keep;
  d->last_bam[3] = 0;
  d->last_bam_ms[0] = ms_since(t0);
  d->last_bam_ms[1] = d->last_bam_ms[2] = d->last_bam_ms[3] = 0;
  if (skip > total) {
    gs_set_error("gs_decode_bam: the header is longer than the bytes of these members");
    return GS_ERR_ARG;
  }
  GS_HIP(hipSetDevice(d->device));
  const uint64_t cap = (total - skip) / 36u + 1u;
  if (cap >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
  /* the starts are sized by the bytes (36 a record at least), everything per record by the records found */
  bump tm;
  const size_t t_res = tm.take(64), t_ref = tm.take(4 * (size_t)n_ref), t_starts = tm.take(8 * cap);
  GS_TRY(gs_reserve(d->w_bs_tmp, tm.at + 16));
  char *tmp = (char *)d->w_bs_tmp.p;
  unsigned long long *res = (unsigned long long *)(tmp + t_res);
  d->bam_tail = 0; /* the kept bytes are in front of these now: a call that fails from here on leaves no tail */

  /* ---- record starts ---- */
  t0 = std::chrono::steady_clock::now();
  unsigned long long h_res[4] = {0, skip, ~0ull, ~0ull};
  if (total > skip) {
    hipLaunchKernelGGL(k_bs_starts, dim3(1), dim3(WAVE), 0, st, (const uint8_t *)d_bytes, skip, total, (uint64_t *)(tmp + t_starts), cap, res);
    GS_HIP(hipMemcpyAsync(h_res, res, 24, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
  }
  d->last_bam_ms[1] = ms_since(t0);
  const uint64_t n = h_res[0], left = total - h_res[1];
  unsigned long long err = h_res[2];
  d->last_bam[3] = n;

  /* ---- fields ---- */
  t0 = std::chrono::steady_clock::now();
  bs_args a;
  memset(&a, 0, sizeof a);
  uint64_t totals[4] = {0, 0, 0, 0};
  char *rec = nullptr;
  size_t t_ow = 0;
  if (n) {
    size_t tb = 0;
    GS_HIP(rocprim::exclusive_scan(nullptr, tb, (uint64_t *)nullptr, (uint64_t *)nullptr, 0ull, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
    bump tr;
    const size_t t_lid = tr.take(8 * (n + 1)), t_lsq = tr.take(8 * (n + 1)), t_lhx = tr.take(8 * (n + 1)), t_lw = tr.take(8 * (n + 1)),
                 t_oid = tr.take(8 * (n + 1)), t_osq = tr.take(8 * (n + 1)), t_ohx = tr.take(8 * (n + 1)), t_hsrc = tr.take(8 * n),
                 t_pos = tr.take(8 * n), t_chr = tr.take(4 * n), t_rev = tr.take(n), t_scan = tr.take(tb);
    t_ow = tr.take(8 * (n + 1));
    GS_TRY(gs_reserve(d->w_bs_rec, tr.at + 16));
    rec = (char *)d->w_bs_rec.p;
    a.d = (const uint8_t *)d_bytes;
    a.starts = (const uint64_t *)(tmp + t_starts);
    a.ref_to_sq = (const int32_t *)(tmp + t_ref);
    a.len_id = (uint64_t *)(rec + t_lid);
    a.len_seq = (uint64_t *)(rec + t_lsq);
    a.len_hex = (uint64_t *)(rec + t_lhx);
    a.len_word = (uint64_t *)(rec + t_lw);
    a.hex_src = (uint64_t *)(rec + t_hsrc);
    a.id_off = (const uint64_t *)(rec + t_oid);
    a.seq_off = (const uint64_t *)(rec + t_osq);
    a.hex_off = (const uint64_t *)(rec + t_ohx);
    a.reverse = (uint8_t *)(rec + t_rev);
    a.chr = (int32_t *)(rec + t_chr);
    a.pos0 = (int64_t *)(rec + t_pos);
    a.err = res + 3;
    a.n = (uint32_t)n;
    a.n_ref = n_ref;
    if (n_ref) GS_HIP(hipMemcpyAsync(tmp + t_ref, ref_to_sq, 4 * (size_t)n_ref, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemsetAsync(res + 3, 0xFF, 8, st));
    const uint32_t cus = (uint32_t)gs_num_cus(d->device);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + BS_WAVES) / BS_WAVES, (uint64_t)cus * 32u));
    hipLaunchKernelGGL(k_bs_sizes, dim3(grid), dim3(WAVE * BS_WAVES), 0, st, a);
    uint64_t *lens[4] = {a.len_id, a.len_seq, a.len_hex, a.len_word};
    const size_t offs[4] = {t_oid, t_osq, t_ohx, t_ow};
    for (int k = 0; k < 4; k++) {
      GS_TRY(gs_prim_carved("gs_decode_bam: scan of the records' sizes", rec + t_scan, tb, [&](void *t, size_t &b) {
        return rocprim::exclusive_scan(t, b, lens[k], (uint64_t *)(rec + offs[k]), 0ull, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
      }));
      GS_HIP(hipMemcpyAsync(&totals[k], (uint64_t *)(rec + offs[k]) + n, 8, hipMemcpyDeviceToHost, st));
    }
    unsigned long long ferr = ~0ull;
    GS_HIP(hipMemcpyAsync(&ferr, res + 3, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    err = std::min(err, ferr); /* (a size below 32 ends the chain: every record before it is a lower index) */
  }
  if (err != ~0ull) return bs_record_error(first_record + (err >> 8), (uint32_t)(err & 255u));
  if (left && (flags & GS_DECODE_BAM_END)) return bs_record_error(first_record + n, left < 4 ? BS_ERR_SIZE : BS_ERR_CUT);
  if (n) {
    bump in;
    const size_t i_ids = in.take(totals[0]), i_seqs = in.take(totals[1]), i_hex = in.take(totals[2]);
    GS_TRY(gs_reserve(d->w_in, in.at + 16));
    a.ids = (uint8_t *)d->w_in.p + i_ids;
    a.seqs = (uint8_t *)d->w_in.p + i_seqs;
    a.hex = (uint8_t *)d->w_in.p + i_hex;
    const uint32_t cus = (uint32_t)gs_num_cus(d->device);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + BS_WAVES - 1) / BS_WAVES, (uint64_t)cus * 32u));
    hipLaunchKernelGGL(k_bs_fill, dim3(grid), dim3(WAVE * BS_WAVES), 0, st, a);
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
  }
  d->last_bam_ms[2] = ms_since(t0);

  /* ---- the decoder's kernels ---- */
  t0 = std::chrono::steady_clock::now();
  *d_text = nullptr;
  *text_len = 0;
  if (n) {
    gs_decode_batch_dev db;
    db.ids = a.ids;
    db.seqs = a.seqs;
    db.hex = a.hex;
    db.reverse = a.reverse;
    db.id_off = a.id_off;
    db.seq_off = a.seq_off;
    db.hex_off = a.hex_off;
    db.word_off = (const uint64_t *)(rec + t_ow);
    db.chr = a.chr;
    db.pos0 = a.pos0;
    if ((rc = gs_decode_run_device(d, db, n, totals[3], flags & (GS_TEXT_COMPLETE | GS_TEXT_FEATURES | GS_DECODE_FEATURES_ONLY), first_record, nullptr, d_text, text_len, nullptr)) != GS_OK)
      return rc;
  }
  d->last_bam_ms[3] = ms_since(t0);
  d->bam_tail = left;
  if (n_records) *n_records = n;
  if (tail) *tail = left;
  return GS_OK;
}
}  // namespace

extern "C" gs_status gs_decode_bam_device(gs_decoder *d, const void *bgzf, uint64_t len, uint64_t skip, const int32_t *ref_to_sq,
                                          uint32_t n_ref, uint32_t flags, uint64_t first_record, const void **d_text, uint64_t *text_len,
                                          uint64_t *n_records, uint64_t *tail) {
  GS_HANDLE_LOCK(d);
  if (!d || !d_text || !text_len || (len && !bgzf) || (n_ref && !ref_to_sq)) return GS_ERR_ARG;
  *d_text = nullptr;
  *text_len = 0;
  if (n_records) *n_records = 0;
  if (tail) *tail = 0;
  GS_TRY(gs_decode_check_flags(d, flags)); /* before anything is inflated or kept */
  try {
    return decode_bam_device(d, bgzf, len, skip, ref_to_sq, n_ref, flags, first_record, d_text, text_len, n_records, tail);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_decode_bam(gs_decoder *d, const void *bgzf, uint64_t len, uint64_t skip, const int32_t *ref_to_sq, uint32_t n_ref,
                                   uint32_t flags, uint64_t first_record, char **text, uint64_t *text_len, uint64_t *n_records, uint64_t *tail) {
  GS_HANDLE_LOCK(d);
  if (!d || !text || !text_len) return GS_ERR_ARG;
  *text = nullptr;
  *text_len = 0;
  const void *dt = nullptr;
  uint64_t tl = 0;
  gs_status rc = gs_decode_bam_device(d, bgzf, len, skip, ref_to_sq, n_ref, flags, first_record, &dt, &tl, n_records, tail);
  if (rc != GS_OK) return rc;
  if ((rc = gs_text_to_host(dt, tl, text)) != GS_OK) return rc;
  *text_len = tl;
  return GS_OK;
}

extern "C" gs_status gs_debug_decode_bam_last(gs_decoder *d, uint64_t *counts, double *ms) {
  GS_HANDLE_LOCK(d);
  if (!d || !counts || !ms) return GS_ERR_ARG;
  for (int k = 0; k < 4; k++) {
    counts[k] = d->last_bam[k];
    ms[k] = d->last_bam_ms[k];
  }
  return GS_OK;
}
