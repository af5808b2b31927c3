/*
 * gs_bgzf_inflate.hip -- BGZF on the device, the other way: the gzip members of a BAM database (SAMv1 section 4.1, what
 * `guidescan enumerate --format bam` and `samtools view -b` write, manual/manual.tex:581-582) -> their bytes in HBM,
 * gs_bgzf.hip turned round, so that the records `guidescan decode` reads (scripts/decode_database.py) need not be
 * inflated by one zlib stream on one host thread.
 *
 * The host makes the member table from the compressed bytes it has just read (gbi_walk_member, gs_bgzf_inflate.h:
 * header, BC subfield, BSIZE chain, CRC-32 and ISIZE of the trailer, ISIZE prefix-summed into output offsets), then the
 * compressed bytes and the table go up.
 *
 * k_bgzf_inflate: one wave takes one member (a workgroup is one wave, as in k_bgzf_piece); the parallelism is in the
 * members, thousands per group, and a deflate stream itself is sequential.  The choice: 5,936 bytes of LDS per workgroup
 * (3,584 bytes of code tables: two canonical codes with a 9-bit first-level lookup, and the lengths of a dynamic header;
 * a 1,040-byte window of the stream; 64 tokens; the 1 KiB byte table of the CRC; the state), so LDS allows 27
 * workgroups on a CU's 160 KiB and occupancy is bounded by the registers (96 VGPRs: 5 waves per SIMD), not by LDS;
 * keeping the 64 KiB output of a member in LDS instead would leave two waves per CU.  A step:
 *   window    the 64 lanes load the 1 KiB of the stream that holds the next bits (one 16-byte load each) into LDS;
 *   symbols   lane 0 runs gbi_step (gs_bgzf_inflate.h): a block header with its tables, or up to 64 tokens.  All
 *             bounds are checked there, against the stream's bytes, ISIZE and the member's first byte;
 *   copies    a scan of the tokens' lengths gives their places.  Literals are written a lane each.  Then the matches
 *             and stored runs in order, 64 bytes at a time: a match whose distance is smaller than its length is a
 *             run whose period is the distance, and lane i reads byte (i mod distance) of the period, all of which
 *             lies before the match (distance 1, length 258: 258 copies of one byte).
 * Then the CRC-32 of the output by the folding routine of the compressor (gs_bgzf_crc.h).  The output is written to
 * HBM as it is made and matches read it back through the cache: a member's window is its own 64 KiB.
 * A member that fails leaves its reason in reason[member]; the host reports the lowest one.
 * Nothing depends on timing: the bytes of member k are a function of member k alone.  No workgroup waits for another.
 */
#include "gs_device.h"
#include "gs_decoder.h"
#include "gs_bgzf_crc.h"
#include "gs_bgzf_inflate.h"

#include <algorithm>

#define BI_WIN 1024u          /* bytes of the stream a step may read: 64 lanes x 16 */
#define BI_PAD (BI_WIN + 32u) /* readable bytes behind the compressed data */
#define BI_MAX_GRID 65536u

struct bi_member {
  uint64_t in_off;  /* the deflate stream in the compressed bytes */
  uint64_t out_off; /* its output behind the kept bytes */
  uint32_t clen, crc, isize, pad;
};

__global__ __launch_bounds__(WAVE) void k_bgzf_inflate(const uint8_t *in, const bi_member *tab, uint32_t n_members, uint8_t *out,
                                                       uint32_t *reason) {
  __shared__ gbi_work s_w;
  __shared__ __attribute__((aligned(16))) uint8_t s_win[BI_WIN + 16u];
  __shared__ uint32_t s_tok[GBI_TOKENS], s_crc[256];
  __shared__ gbi_state s_st;
  __shared__ uint32_t s_ntok, s_rc, s_at;
  const uint32_t lane = lane_id();
  gb_crc_table(s_crc);
  for (uint32_t member = blockIdx.x; member < n_members; member += gridDim.x) {
    const bi_member m = tab[member];
    const uint8_t *src = in + m.in_off;
    uint8_t *dst = out + m.out_off;
    if (lane == 0u) gbi_state_init(&s_st);
    __syncthreads();
    uint32_t rc = GBI_OK;
    /* a step uses at least three bits of the stream or ends it */
    for (uint32_t guard = 0; guard < 8u * m.clen + 8u; guard++) {
      if (s_st.mode == GBI_MODE_DONE) break;
      /* ---- window: the 16-byte aligned KiB that holds the next bits (the buffer is aligned and padded) ---- */
      const uint32_t bytepos = s_st.bitpos >> 3;
      const uint32_t mis = (uint32_t)((uintptr_t)(src + bytepos) & 15u);
      const int32_t lo = (int32_t)bytepos - (int32_t)mis;
      ((uint4 *)s_win)[lane] = ((const uint4 *)(src + bytepos - mis))[lane];
      __syncthreads();
      /* ---- symbols ---- */
      if (lane == 0u) {
        s_at = s_st.outpos;
        uint32_t ntok = 0;
        s_rc = gbi_step(&s_st, &s_w, s_win, lo, BI_WIN, m.clen, m.isize, s_tok, &ntok);
        s_ntok = ntok;
      }
      __syncthreads();
      rc = s_rc;
      if (rc != GBI_OK) break;
      /* ---- copies ---- */
      const uint32_t ntok = s_ntok;
      const uint32_t k = lane < ntok ? s_tok[lane] : 0u;
      const bool wide = lane < ntok && (k & (GBI_TOK_MATCH | GBI_TOK_STORED)) != 0u;
      const uint32_t olen = lane >= ntok ? 0u : (k & GBI_TOK_MATCH) ? ((k >> 16) & 255u) + 3u : (k & GBI_TOK_STORED) ? (k & 0xFFFFu) : 1u;
      const uint32_t at = s_at + wave_incl_sum(olen) - olen;
      if (lane < ntok && !wide) dst[at] = (uint8_t)k;
      __syncthreads();
      uint64_t todo = __ballot(wide);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint32_t kk = (uint32_t)__shfl((int)k, l), a = (uint32_t)__shfl((int)at, l);
        if (kk & GBI_TOK_MATCH) {
          const uint32_t length = ((kk >> 16) & 255u) + 3u, dist = (kk & 0x7FFFu) + 1u;
          const uint8_t *from = dst + a - dist;
          if (dist >= length) {
            for (uint32_t i = lane; i < length; i += WAVE) dst[a + i] = from[i];
          } else {
            for (uint32_t i = lane; i < length; i += WAVE) dst[a + i] = from[i % dist];
          }
        } else {
          const uint32_t n = kk & 0xFFFFu;
          const uint8_t *from = src + s_st.stored_src;
          for (uint32_t i = lane; i < n; i += WAVE) dst[a + i] = from[i];
        }
        __syncthreads(); /* a later match may read these bytes */
      }
    }
    if (rc == GBI_OK && s_st.mode != GBI_MODE_DONE) rc = GBI_ERR_WINDOW;
    __syncthreads();
    if (rc == GBI_OK && gb_crc_wave(dst, m.isize, s_crc) != m.crc) rc = GBI_ERR_CRC;
    if (lane == 0u) reason[member] = rc;
    __syncthreads();
  }
}

/* ---- host ---------------------------------------------------------------------------------------------------- */
namespace {
/* index and offset count from the caller's bases: a file handed over in groups names the member in the file */
gs_status bi_member_error(const char *who, uint64_t index, uint64_t file_off, uint32_t reason) {
  gs_set_error(std::string(who) + ": member " + std::to_string(index) + " at byte " + std::to_string(file_off) + ": " +
               gbi_reason_string(reason));
  return GS_ERR_FORMAT;
}

/* the members of bgzf[0, len): the table for the device, each member's place in the data, the sum of ISIZE */
gs_status bi_table(const char *who, const uint8_t *bgzf, uint64_t len, uint64_t keep, uint64_t base_member, uint64_t base_byte,
                   std::vector<bi_member> &tab, std::vector<uint64_t> &file_off, uint64_t *total) {
  uint64_t at = 0, out = keep;
  while (at < len) {
    gbi_member gm;
    const uint32_t rc = gbi_walk_member(bgzf + at, len - at, &gm);
    if (rc != GBI_OK) return bi_member_error(who, base_member + tab.size(), base_byte + at, rc);
    bi_member m;
    m.in_off = at + gm.cdata_off;
    m.out_off = out;
    m.clen = gm.clen;
    m.crc = gm.crc;
    m.isize = gm.isize;
    m.pad = 0;
    tab.push_back(m);
    file_off.push_back(at);
    out += gm.isize;
    at += gm.size;
  }
  *total = out - keep;
  return GS_OK;
}

/* bgzf[0, len) (host) -> w_out: `keep` bytes copied from d_keep (HBM), then the members' bytes */
gs_status bi_run(const char *who, int device, gs_buffer &w_in, gs_buffer &w_tmp, gs_buffer &w_out, const uint8_t *bgzf, uint64_t len,
                 const void *d_keep, uint64_t keep, uint64_t base_member, uint64_t base_byte, uint64_t *out_len, uint64_t *n_members) {
  std::vector<bi_member> tab;
  std::vector<uint64_t> file_off;
  uint64_t total = 0;
  GS_TRY(bi_table(who, bgzf, len, keep, base_member, base_byte, tab, file_off, &total));
  if (tab.size() >= (1ull << 31)) return GS_ERR_UNSUPPORTED;
  const uint32_t n = (uint32_t)tab.size();
  hipStream_t st = nullptr;
  GS_HIP(hipSetDevice(device));
  GS_TRY(gs_reserve(w_out, keep + total + 16));
  if (keep) GS_HIP(hipMemcpyAsync(w_out.p, d_keep, keep, hipMemcpyDeviceToDevice, st));
  if (n) {
    const size_t t_bytes = sizeof(bi_member) * (size_t)n, t_reason = (t_bytes + 255) & ~(size_t)255;
    GS_TRY(gs_reserve(w_in, len + BI_PAD));
    GS_TRY(gs_reserve(w_tmp, t_reason + 4 * (size_t)n + 16));
    uint32_t *d_reason = (uint32_t *)((char *)w_tmp.p + t_reason);
    GS_HIP(hipMemcpyAsync(w_in.p, bgzf, len, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemsetAsync((char *)w_in.p + len, 0, BI_PAD, st));
    GS_HIP(hipMemcpyAsync(w_tmp.p, tab.data(), t_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min(n, BI_MAX_GRID)), dim3(WAVE), 0, st, (const uint8_t *)w_in.p,
                       (const bi_member *)w_tmp.p, n, (uint8_t *)w_out.p, d_reason);
    std::vector<uint32_t> reason(n);
    GS_HIP(hipMemcpyAsync(reason.data(), d_reason, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    for (uint32_t i = 0; i < n; i++)
      if (reason[i] != GBI_OK) return bi_member_error(who, base_member + i, base_byte + file_off[i], reason[i]);
  } else {
    GS_HIP(hipStreamSynchronize(st));
  }
  *out_len = keep + total;
  if (n_members) *n_members = n;
  return GS_OK;
}
}  // namespace

extern "C" gs_status gs_bgzf_inflate_device(gs_decoder *d, const void *bgzf, uint64_t len, uint64_t keep, const void **d_out,
                                            uint64_t *out_len, uint64_t *n_members) {
  GS_HANDLE_LOCK(d);
  if (!d || !d_out || !out_len || (len && !bgzf)) return GS_ERR_ARG;
  *d_out = nullptr;
  *out_len = 0;
  if (n_members) *n_members = 0;
  if (keep > d->inf_len) {
    gs_set_error("gs_bgzf_inflate_device: more bytes to keep than the call before left");
    return GS_ERR_ARG;
  }
  try {
    const uint32_t prev = d->inf_cur, cur = prev ^ 1u;
    const char *tail = keep ? (const char *)d->w_inf[prev].p + (d->inf_len - keep) : nullptr;
    uint64_t n = 0;
    const gs_status rc = bi_run("gs_bgzf_inflate", d->device, d->w_bi_in, d->w_bi_tmp, d->w_inf[cur], (const uint8_t *)bgzf, len, tail, keep,
                                d->inf_base_member, d->inf_base_byte, &n, n_members);
    if (rc != GS_OK) return rc; /* the call before is still what the decoder holds */
    d->inf_cur = cur;
    d->inf_len = n;
    *d_out = d->w_inf[cur].p;
    *out_len = n;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_bgzf_inflate_base(gs_decoder *d, uint64_t members_before, uint64_t bytes_before) {
  GS_HANDLE_LOCK(d);
  if (!d) return GS_ERR_ARG;
  d->inf_base_member = members_before;
  d->inf_base_byte = bytes_before;
  return GS_OK;
}

extern "C" gs_status gs_bgzf_inflate(int device, const void *bgzf, uint64_t len, uint8_t **out, uint64_t *out_len) {
  if (!out || !out_len || (len && !bgzf)) return GS_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  gs_buffer w_in, w_tmp, w_out; /* freed on every way out */
  gs_status rc;
  uint64_t n = 0;
  uint8_t *o = nullptr;
  try {
    rc = bi_run("gs_bgzf_inflate", device, w_in, w_tmp, w_out, (const uint8_t *)bgzf, len, nullptr, 0, 0, 0, &n, nullptr);
  } catch (const std::bad_alloc &) {
    rc = GS_ERR_NOMEM;
  }
  if (rc == GS_OK && !(o = (uint8_t *)malloc(n ? n : 1))) rc = GS_ERR_NOMEM;
  if (rc == GS_OK && n && hipMemcpy(o, w_out.p, n, hipMemcpyDeviceToHost) != hipSuccess) {
    gs_set_error("gs_bgzf_inflate: copying the bytes back failed");
    rc = GS_ERR_DEVICE;
  }
  if (rc != GS_OK) {
    free(o);
    return rc;
  }
  *out = o;
  *out_len = n;
  return GS_OK;
}

/* the table walk alone, for the CPU tests */
extern "C" gs_status gs_debug_bgzf_members(const void *bgzf, uint64_t len, uint64_t *member_off, uint32_t *isize, uint64_t cap, uint64_t *n,
                                           uint32_t *reason) {
  if (!n || !reason || (len && !bgzf)) return GS_ERR_ARG;
  *n = 0;
  *reason = GBI_OK;
  uint64_t at = 0;
  while (at < len) {
    gbi_member gm;
    if ((*reason = gbi_walk_member((const uint8_t *)bgzf + at, len - at, &gm)) != GBI_OK)
      return bi_member_error("gs_debug_bgzf_members", *n, at, *reason);
    if (*n < cap) {
      if (member_off) member_off[*n] = at;
      if (isize) isize[*n] = gm.isize;
    }
    ++*n;
    at += gm.size;
  }
  return GS_OK;
}

extern "C" gs_status gs_debug_inflate_member(const void *member, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint32_t *reason) {
  if (!member || !out_len || !reason || (cap && !out)) return GS_ERR_ARG;
  *out_len = 0;
  gbi_member gm;
  const uint8_t *p = (const uint8_t *)member;
  if ((*reason = gbi_walk_member(p, len, &gm)) != GBI_OK) return bi_member_error("gs_debug_inflate_member", 0, 0, *reason);
  if (gm.isize > cap) return GS_ERR_ARG;
  gbi_work *w = new (std::nothrow) gbi_work;
  if (!w) return GS_ERR_NOMEM;
  uint32_t n = 0;
  *reason = gbi_inflate_member(p + gm.cdata_off, gm.clen, out, gm.isize, w, &n);
  delete w;
  *out_len = n;
  if (*reason == GBI_OK) {
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) {
      crc ^= out[i];
      for (int k = 0; k < 8; k++) crc = (crc & 1u) ? (crc >> 1) ^ 0xEDB88320u : crc >> 1;
    }
    if ((crc ^ 0xFFFFFFFFu) != gm.crc) *reason = GBI_ERR_CRC;
  }
  return *reason == GBI_OK ? GS_OK : bi_member_error("gs_debug_inflate_member", 0, 0, *reason);
}
