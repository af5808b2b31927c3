/*
 * gs_kmers.hip -- candidate-guide generation on the device: the
 * scan of one chromosome for every PAM site, in the order the reference's helper script emits
 * them (scripts/generate_kmers.py:70-118): for each concrete expansion of the PAM pattern
 * ('N' -> A,C,T,G, first N first) every occurrence on the + strand in position order, then for
 * each reverse-complemented expansion every occurrence on the - strand; protospacers with a
 * symbol outside A,C,G,T or cut by a chromosome end are dropped; positions are 1-based.
 *
 * Three streaming kernels and two library primitives (this is the step BEFORE the hot path):
 *   k_km_count   sites per 256-position block                       (1 B read per position)
 *   (rocprim exclusive scan of the block counts)
 *   k_km_keys    key = bucket << 32 | position, compacted in position order
 *   (rocprim radix sort of the keys: bucket, then position)
 *   k_km_emit    one thread per site: protospacer (reverse-complemented on the - strand),
 *                position, sense, PAM pattern.
 * The output arrays stay in HBM in exactly the layout gs_enumerate_device takes.
 *
 * The records as text, also in HBM (a length per record, an exclusive scan, a write; gs_km_encode_text, which gs_design.hip
 * calls too, with a group and a chromosome per record and a table of their names).  The id and the row are stated once, as
 * gs_guide_row of gs_rowtext.h: the length kernel runs it over the counting sink, the write kernel over the writing one.
 *   k_km_text_len    bytes of every record's id "{prefix}[{group}:]{chromosome}:{position}:{sense}" or of its kmers-file row
 *                    "id,sequence,pam,chromosome,position,sense\n" (scripts/generate_kmers.py:120-125)   (4 B read, 8 B written)
 *   (rocprim 64-bit exclusive scan of the n + 1 lengths: the offsets)
 *   k_km_text_write  one thread per record composes its bytes at its offset (a row: 4 + 8 + k + 1 B read, ~2k + 2P + 40 B
 *                    written; an id: 4 + 8 + 1 B read, ~20 B written, plus the sense as 0/1 for the SAM encoder)
 * gs_kmers_concat joins the records of several chromosomes into one stream, ids included (k_km_rebase shifts the id
 * offsets), so that a batch can hold the tail of one chromosome and the heads of the next ones.
 */
#include "gs_common.h"
#include "gs_scratch.h"
#include "gs_kmers_obj.h"
#include "gs_rowtext.h"
#include "gs_select_scan.h"

#include <rocprim/rocprim.hpp>

#include <memory>

#define KM_BLOCK 256

struct gs_km_args {
  const uint8_t *chr;
  const uint16_t *lut; /* 4^P entries: low byte = 1 + id of the matching + strand expansion, high byte: - strand */
  uint64_t len;
  uint32_t k, P, n_exp, start;
};

__device__ __forceinline__ int km_code(uint32_t c) {
  if (c >= 'a' && c <= 'z') c -= 32u; /* chrm.upper(), scripts/generate_kmers.py:103 */
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}
__device__ __forceinline__ bool km_acgt(const uint8_t *p, uint32_t k) {
  bool ok = true;
  for (uint32_t j = 0; j < k; ++j) ok = ok && km_code(p[j]) >= 0;
  return ok;
}
/* the sites whose PAM starts at idx: bit 0 = + strand (bucket fid-1), bit 1 = - strand (bucket rid-1) */
__device__ __forceinline__ uint32_t km_sites(const gs_km_args &a, uint64_t idx, uint32_t &fid, uint32_t &rid) {
  fid = rid = 0;
  if (idx + a.P > a.len) return 0u;
  uint32_t w = 0;
  for (uint32_t j = 0; j < a.P; ++j) {
    const int c = km_code(a.chr[idx + j]);
    if (c < 0) return 0u;
    w = (w << 2) | (uint32_t)c;
  }
  const uint32_t e = a.lut[w];
  uint32_t m = 0;
  /* scripts/generate_kmers.py:79-93: protospacer before the PAM (+ strand with the PAM at the
   * end, - strand with the PAM at the start) or after it */
  const bool has_before = idx >= a.k;               /* position = idx - k >= 0 */
  const bool has_after = idx + a.P + a.k <= a.len;  /* len(kmer) == k */
  if (e & 0xFFu) {
    const bool before = !a.start;
    if (before ? (has_before && km_acgt(a.chr + idx - a.k, a.k)) : (has_after && km_acgt(a.chr + idx + a.P, a.k))) {
      m |= 1u;
      fid = e & 0xFFu;
    }
  }
  if (e >> 8) {
    const bool before = a.start != 0u;
    if (before ? (has_before && km_acgt(a.chr + idx - a.k, a.k)) : (has_after && km_acgt(a.chr + idx + a.P, a.k))) {
      m |= 2u;
      rid = e >> 8;
    }
  }
  return m;
}

__global__ __launch_bounds__(KM_BLOCK) void k_km_count(gs_km_args a, uint32_t *block_cnt) {
  __shared__ uint32_t s[KM_BLOCK / 64];
  const uint64_t idx = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  uint32_t f, r;
  const uint32_t m = idx < a.len ? km_sites(a, idx, f, r) : 0u;
  uint32_t c = (m & 1u) + (m >> 1);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(KM_BLOCK) void k_km_keys(gs_km_args a, const uint32_t *block_off, uint64_t *keys) {
  __shared__ uint32_t s[KM_BLOCK / 64];
  const uint64_t idx = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t f, r;
  const uint32_t m = idx < a.len ? km_sites(a, idx, f, r) : 0u;
  const uint32_t c = (m & 1u) + (m >> 1);
  uint32_t inc = c; /* inclusive wave scan */
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o);
    if ((int)lane >= o) inc += up;
  }
  if (lane == 63u) s[wv] = inc;
  __syncthreads();
  uint32_t base = block_off[blockIdx.x];
  for (uint32_t w = 0; w < wv; ++w) base += s[w];
  uint32_t at = base + inc - c;
  /* inside one position the + strand site comes first; the sort separates the buckets anyway */
  if (m & 1u) keys[at++] = ((uint64_t)(f - 1u) << 32) | idx;
  if (m & 2u) keys[at] = ((uint64_t)(a.n_exp + r - 1u) << 32) | idx;
}

struct gs_km_emit_args {
  const uint8_t *chr;
  const uint64_t *keys;
  uint8_t *seqs, *pams, *sense;
  uint32_t *pos;
  uint64_t n;
  uint32_t k, P, n_exp, start;
  uint8_t pam[8];
};
__global__ __launch_bounds__(KM_BLOCK) void k_km_emit(gs_km_emit_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (j >= a.n) return;
  const uint64_t key = a.keys[j];
  const uint64_t idx = key & 0xFFFFFFFFull;
  const bool minus = (uint32_t)(key >> 32) >= a.n_exp;
  const bool before = minus ? (a.start != 0u) : (a.start == 0u);
  const uint64_t s0 = before ? idx - a.k : idx + a.P;
  uint8_t *o = a.seqs + j * a.k;
  for (uint32_t t = 0; t < a.k; ++t) {
    uint32_t c = minus ? a.chr[s0 + (a.k - 1u - t)] : a.chr[s0 + t];
    if (c >= 'a' && c <= 'z') c -= 32u;
    if (minus) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C'; /* revcom, :52-53 */
    o[t] = (uint8_t)c;
  }
  for (uint32_t u = 0; u < a.P; ++u) a.pams[j * a.P + u] = a.pam[u]; /* the pattern, :110,117 */
  a.pos[j] = (uint32_t)((before ? idx - a.k : idx) + 1ull); /* 1-based, :99 */
  a.sense[j] = minus ? '-' : '+';
}

/* an array of the object: km_release frees it */
static gs_status km_alloc(size_t bytes, void **out) {
  gs_scratch one;
  GS_TRY(one.get(bytes, out));
  one.keep(*out);
  return GS_OK;
}
void km_release(gs_kmers *km) { /* gs_kmers_obj.h */
  if (!km) return;
  bool any = false; /* an empty object never touched a device */
  for (void *p : {km->d_seqs, km->d_pams, km->d_pos, km->d_sense, km->d_ids, km->d_id_off, km->d_sense01}) any = any || p;
  if (any) hipSetDevice(km->device);
  for (void *p : {km->d_seqs, km->d_pams, km->d_pos, km->d_sense, km->d_ids, km->d_id_off, km->d_sense01})
    if (p) hipFree(p);
  delete km;
}

extern "C" gs_status gs_kmers_generate(int device, const uint8_t *chr, uint64_t chr_len, int chr_on_device,
                                       const char *pam, uint32_t k, uint32_t flags, void *stream,
                                       gs_kmers **out) {
  if (!out || (chr_len && !chr) || !pam) return GS_ERR_ARG;
  const uint32_t P = (uint32_t)strlen(pam);
  if (k < 1 || k > 64 || P < 1 || P > 8 || chr_len >= (1ull << 32) - 64) {
    gs_set_error("kmer generation supports 1<=k<=64, 1<=P<=8, chromosomes shorter than 2^32");
    return GS_ERR_UNSUPPORTED;
  }
  /* generate_pam_set (scripts/generate_kmers.py:55-68): breadth-first replacement of the first
   * N by A,C,T,G == all N positions left to right as digits in the order A,C,T,G */
  uint32_t npos[8], nn = 0;
  for (uint32_t u = 0; u < P; u++) {
    const char c = pam[u];
    if (c == 'N')
      npos[nn++] = u;
    else if (c != 'A' && c != 'C' && c != 'G' && c != 'T') {
      gs_set_error("PAM symbols outside A,C,G,T,N are not expanded by the reference script and not implemented here");
      return GS_ERR_UNSUPPORTED;
    }
  }
  if (nn > 3) {
    gs_set_error("more than three N in the PAM pattern");
    return GS_ERR_UNSUPPORTED;
  }
  const uint32_t n_exp = 1u << (2 * nn);
  auto code = [](char c) -> uint32_t { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; };
  static const char NUCS[4] = {'A', 'C', 'T', 'G'}; /* :49 */
  std::vector<uint16_t> lut((size_t)1 << (2 * P), 0);
  for (uint32_t e = 0; e < n_exp; e++) {
    char p[9];
    memcpy(p, pam, P);
    for (uint32_t i = 0; i < nn; i++) p[npos[i]] = NUCS[(e >> (2 * (nn - 1 - i))) & 3u];
    uint32_t wf = 0, wr = 0;
    for (uint32_t u = 0; u < P; u++) wf = (wf << 2) | code(p[u]);
    for (uint32_t u = 0; u < P; u++) wr = (wr << 2) | (3u - code(p[P - 1 - u])); /* revcom(p) */
    lut[wf] = (uint16_t)((lut[wf] & 0xFF00u) | (e + 1u));
    lut[wr] = (uint16_t)((lut[wr] & 0x00FFu) | ((e + 1u) << 8));
  }

  hipStream_t st = (hipStream_t)stream;
  GS_HIP(hipSetDevice(device));
  std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new gs_kmers(), km_release);
  gs_kmers *km = own.get();
  km->device = device;
  km->k = k;
  km->P = P;
  if (chr_len == 0) {
    *out = own.release();
    return GS_OK;
  }
  const uint32_t nb = (uint32_t)((chr_len + KM_BLOCK - 1) / KM_BLOCK);
  gs_scratch mem;
  void *d_chr_own = nullptr, *d_lut = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_keys = nullptr,
       *d_keys2 = nullptr;
  gs_prim_tmp tmp;
  const uint8_t *d_chr = chr;
  if (!chr_on_device) {
    GS_TRY(mem.get(chr_len, &d_chr_own));
    GS_HIP(hipMemcpyAsync(d_chr_own, chr, chr_len, hipMemcpyHostToDevice, st));
    d_chr = (const uint8_t *)d_chr_own;
  }
  GS_TRY(mem.get(2 * lut.size(), &d_lut));
  GS_HIP(hipMemcpyAsync(d_lut, lut.data(), 2 * lut.size(), hipMemcpyHostToDevice, st));
  GS_TRY(mem.get(4 * ((size_t)nb + 1), &d_cnt));
  GS_TRY(mem.get(4 * ((size_t)nb + 1), &d_off));
  GS_HIP(hipMemsetAsync(d_cnt, 0, 4 * ((size_t)nb + 1), st));
  gs_km_args a;
  a.chr = d_chr;
  a.lut = (const uint16_t *)d_lut;
  a.len = chr_len;
  a.k = k;
  a.P = P;
  a.n_exp = n_exp;
  a.start = (flags & GS_FLAG_PAM_AT_START) ? 1u : 0u;
  hipLaunchKernelGGL(k_km_count, dim3(nb), dim3(KM_BLOCK), 0, st, a, (uint32_t *)d_cnt);
  GS_TRY(gs_prim("kmers: scan of the counts", mem, tmp, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, (uint32_t *)d_cnt, (uint32_t *)d_off, 0u, (size_t)nb + 1, rocprim::plus<uint32_t>(), st);
  }));
  uint32_t total = 0;
  GS_HIP(hipMemcpyAsync(&total, (uint32_t *)d_off + nb, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  km->n = total;
  if (total) {
    GS_TRY(mem.get(8 * (size_t)total, &d_keys));
    GS_TRY(mem.get(8 * (size_t)total, &d_keys2));
    hipLaunchKernelGGL(k_km_keys, dim3(nb), dim3(KM_BLOCK), 0, st, a, (const uint32_t *)d_off, (uint64_t *)d_keys);
    /* bucket (1 + 2*nn bits above bit 32), then position: the whole key, so the order does not
     * lean on the sort being stable */
    const unsigned end_bit = 32u + 1u + 2u * nn;
    GS_TRY(gs_prim("kmers: sort", mem, tmp, [&](void *t, size_t &tb) {
      return rocprim::radix_sort_keys(t, tb, (uint64_t *)d_keys, (uint64_t *)d_keys2, (size_t)total, 0u, end_bit, st);
    }));
    GS_TRY(km_alloc((size_t)total * k, &km->d_seqs));
    GS_TRY(km_alloc((size_t)total * P, &km->d_pams));
    GS_TRY(km_alloc(4 * (size_t)total, &km->d_pos));
    GS_TRY(km_alloc((size_t)total, &km->d_sense));
    gs_km_emit_args ea;
    ea.chr = d_chr;
    ea.keys = (const uint64_t *)d_keys2;
    ea.seqs = (uint8_t *)km->d_seqs;
    ea.pams = (uint8_t *)km->d_pams;
    ea.sense = (uint8_t *)km->d_sense;
    ea.pos = (uint32_t *)km->d_pos;
    ea.n = total;
    ea.k = k;
    ea.P = P;
    ea.n_exp = n_exp;
    ea.start = a.start;
    memset(ea.pam, 0, sizeof(ea.pam));
    memcpy(ea.pam, pam, P);
    hipLaunchKernelGGL(k_km_emit, dim3((unsigned)(((size_t)total + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0,
                       st, ea);
  }
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  *out = own.release();
  return GS_OK;
}

extern "C" gs_status gs_kmers_get(gs_kmers *km, int on_device, uint64_t *n, const void **seqs,
                                  const void **pams, const void **positions, const void **senses) {
  if (!km) return GS_ERR_ARG;
  if (n) *n = km->n;
  if (on_device) {
    if (km->device < 0) return GS_ERR_ARG;
    if (seqs) *seqs = km->d_seqs;
    if (pams) *pams = km->d_pams;
    if (positions) *positions = km->d_pos;
    if (senses) *senses = km->d_sense;
    return GS_OK;
  }
  if (!km->have_host) {
    GS_HIP(hipSetDevice(km->device));
    km->h_seqs.resize((size_t)km->n * km->k);
    km->h_pams.resize((size_t)km->n * km->P);
    km->h_pos.resize(km->parsed ? 0 : (size_t)km->n);
    km->h_sense.resize((size_t)km->n);
    if (km->n) {
      GS_HIP(hipMemcpy(km->h_seqs.data(), km->d_seqs, km->h_seqs.size(), hipMemcpyDeviceToHost));
      GS_HIP(hipMemcpy(km->h_pams.data(), km->d_pams, km->h_pams.size(), hipMemcpyDeviceToHost));
      if (!km->parsed) GS_HIP(hipMemcpy(km->h_pos.data(), km->d_pos, 4 * km->h_pos.size(), hipMemcpyDeviceToHost));
      GS_HIP(hipMemcpy(km->h_sense.data(), km->d_sense, km->h_sense.size(), hipMemcpyDeviceToHost));
    }
    km->have_host = true;
  }
  if (seqs) *seqs = km->h_seqs.data();
  if (pams) *pams = km->h_pams.data();
  if (positions) *positions = km->parsed ? nullptr : km->h_pos.data();
  if (senses) *senses = km->h_sense.data();
  return GS_OK;
}

/* ---- the records as text ------------------------------------------------------------------------------------- */
struct gs_km_text_args {
  const uint8_t *seqs, *pams, *sense;
  const uint32_t *pos;
  const uint32_t *group, *chr; /* per record, or nullptr: no group in the id; chromosome 0 */
  const uint8_t *names;        /* prefix, the group names, the chromosome names */
  const uint32_t *goff, *coff; /* where each name begins in `names`; one more entry closes each table */
  uint64_t *lens;              /* n + 1 */
  const uint64_t *off;         /* n + 1 */
  uint8_t *text, *sense01;
  uint64_t n;
  uint32_t k, P, prefix_len, rows;
};
/* record j through gs_guide_row: the length kernel runs it over the counting sink, the write kernel over the writing one */
template <class S>
__device__ __forceinline__ void km_text_row(S &o, const gs_km_text_args &a, uint64_t j) {
  const uint32_t c = a.chr ? a.chr[j] : 0u;
  gs_rt_span group{nullptr, 0u};
  if (a.group) {
    const uint32_t g = a.group[j];
    group = gs_rt_span{a.names + a.goff[g], a.goff[g + 1] - a.goff[g]};
  }
  gs_guide_row(o, a.names, a.prefix_len, group, gs_rt_span{a.names + a.coff[c], a.coff[c + 1] - a.coff[c]}, a.pos[j], a.sense[j],
               a.seqs + j * a.k, a.pams + j * a.P, a.k, a.P, a.rows != 0u);
}
__global__ __launch_bounds__(KM_BLOCK) void k_km_text_len(gs_km_text_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (j > a.n) return;
  gs_row_count o;
  if (j < a.n) km_text_row(o, a, j); /* one more entry closes the scan */
  a.lens[j] = o.n;
}
__global__ __launch_bounds__(KM_BLOCK) void k_km_text_write(gs_km_text_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (j >= a.n) return;
  gs_row_write o;
  o.p = (char *)a.text + a.off[j];
  km_text_row(o, a, j);
  if (!a.rows) a.sense01[j] = a.sense[j] == '+' ? 1 : 0;
}
__global__ __launch_bounds__(KM_BLOCK) void k_km_rebase(const uint64_t *in, uint64_t n, uint64_t base, uint64_t *out) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (j < n) out[j] = in[j] + base;
}

/* gs_kmers_obj.h: ids (rows == false, kept in the object) or kmers-file rows (*d_text: the caller frees it) of all records */
gs_status gs_km_encode_text(gs_kmers *km, const gs_km_names &nt, const uint32_t *d_group, const uint32_t *d_chr, bool rows, const char *what,
                            hipStream_t st, void **d_text, uint64_t *bytes) {
  const uint64_t n = km->n;
  gs_scratch mem;
  void *d_tab = nullptr, *d_lens = nullptr, *off = nullptr, *text = nullptr, *s01 = nullptr;
  /* one upload: the offsets of the group names, those of the chromosome names, the names */
  const size_t ng = nt.goff.size(), nc = nt.coff.size();
  std::vector<uint8_t> tab(4 * (ng + nc) + nt.names.size());
  if (ng) memcpy(tab.data(), nt.goff.data(), 4 * ng);
  memcpy(tab.data() + 4 * ng, nt.coff.data(), 4 * nc);
  memcpy(tab.data() + 4 * (ng + nc), nt.names.data(), nt.names.size());
  GS_TRY(mem.get(tab.size(), &d_tab));
  GS_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  GS_TRY(mem.get(8 * (n + 1), &d_lens));
  GS_TRY(mem.get(8 * (n + 1), &off));
  gs_km_text_args a;
  memset(&a, 0, sizeof a);
  a.seqs = (const uint8_t *)km->d_seqs;
  a.pams = (const uint8_t *)km->d_pams;
  a.sense = (const uint8_t *)km->d_sense;
  a.pos = (const uint32_t *)km->d_pos;
  a.group = d_group;
  a.chr = d_chr;
  a.goff = (const uint32_t *)d_tab;
  a.coff = a.goff + ng;
  a.names = (const uint8_t *)(a.coff + nc);
  a.lens = (uint64_t *)d_lens;
  a.off = (const uint64_t *)off;
  a.n = n;
  a.k = km->k;
  a.P = km->P;
  a.prefix_len = nt.prefix_len;
  a.rows = rows ? 1u : 0u;
  const unsigned grid = (unsigned)((n + 1 + KM_BLOCK - 1) / KM_BLOCK);
  hipLaunchKernelGGL(k_km_text_len, dim3(grid), dim3(KM_BLOCK), 0, st, a);
  gs_prim_tmp tmp;
  GS_TRY(gs_prim(what, mem, tmp, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, (uint64_t *)d_lens, (uint64_t *)off, 0ull, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
  }));
  uint64_t total = 0;
  GS_HIP(hipMemcpyAsync(&total, (uint64_t *)off + n, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st)); /* `tab` is a local */
  GS_TRY(mem.get(total, &text));
  if (!rows) GS_TRY(mem.get(n, &s01));
  a.text = (uint8_t *)text;
  a.sense01 = (uint8_t *)s01;
  if (n) hipLaunchKernelGGL(k_km_text_write, dim3((unsigned)((n + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, st, a);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  mem.keep(text);
  if (rows) {
    *d_text = text;
  } else {
    mem.keep(off);
    mem.keep(s01);
    for (void *p : {km->d_ids, km->d_id_off, km->d_sense01})
      if (p) hipFree(p);
    km->d_ids = text;
    km->d_id_off = off;
    km->d_sense01 = s01;
    km->id_bytes = total;
    km->have_ids = true;
    km->have_host_ids = false;
  }
  *bytes = total;
  return GS_OK;
}

/* a scan's records: no group, one chromosome */
static gs_status km_encode(gs_kmers *km, const char *prefix, const char *chr_name, bool rows, hipStream_t st, void **d_text, uint64_t *bytes) {
  const size_t pl = strlen(prefix), nl = strlen(chr_name);
  if (pl >= (1u << 20) || nl >= (1u << 20)) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(km->device));
  gs_km_names nt;
  nt.names = std::string(prefix) + chr_name;
  nt.prefix_len = (uint32_t)pl;
  nt.coff = {(uint32_t)pl, (uint32_t)(pl + nl)};
  return gs_km_encode_text(km, nt, nullptr, nullptr, rows, "kmers text: scan of the lengths", st, d_text, bytes);
}

extern "C" gs_status gs_kmers_encode_ids(gs_kmers *km, const char *prefix, const char *chr_name, void *stream) {
  if (!km || !prefix || !chr_name) return GS_ERR_ARG;
  if (km->parsed) {
    gs_set_error("gs_kmers_encode_ids on the rows of a kmers file: the ids are the file's");
    return GS_ERR_ARG;
  }
  if (km->ids_fixed) {
    gs_set_error("gs_kmers_encode_ids on the records of gs_design_select: their ids name group and chromosome");
    return GS_ERR_ARG;
  }
  uint64_t bytes = 0;
  try {
    return km_encode(km, prefix, chr_name, false, (hipStream_t)stream, nullptr, &bytes);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_kmers_get_ids(gs_kmers *km, int on_device, const void **ids, const void **id_offsets,
                                      const void **sense_positive) {
  if (!km) return GS_ERR_ARG;
  if (!km->have_ids) {
    gs_set_error("gs_kmers_get_ids before gs_kmers_encode_ids");
    return GS_ERR_ARG;
  }
  if (on_device) {
    if (km->device < 0) return GS_ERR_ARG;
    if (ids) *ids = km->d_ids;
    if (id_offsets) *id_offsets = km->d_id_off;
    if (sense_positive) *sense_positive = km->d_sense01;
    return GS_OK;
  }
  try {
    if (!km->have_host_ids) {
      GS_HIP(hipSetDevice(km->device));
      km->h_ids.resize((size_t)km->id_bytes);
      km->h_id_off.resize((size_t)km->n + 1);
      km->h_sense01.resize((size_t)km->n);
      if (km->id_bytes) GS_HIP(hipMemcpy(km->h_ids.data(), km->d_ids, km->h_ids.size(), hipMemcpyDeviceToHost));
      GS_HIP(hipMemcpy(km->h_id_off.data(), km->d_id_off, 8 * km->h_id_off.size(), hipMemcpyDeviceToHost));
      if (km->n) GS_HIP(hipMemcpy(km->h_sense01.data(), km->d_sense01, km->h_sense01.size(), hipMemcpyDeviceToHost));
      km->have_host_ids = true;
    }
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  if (ids) *ids = km->h_ids.data();
  if (id_offsets) *id_offsets = km->h_id_off.data();
  if (sense_positive) *sense_positive = km->h_sense01.data();
  return GS_OK;
}

extern "C" gs_status gs_kmers_csv(gs_kmers *km, const char *prefix, const char *chr_name, char **text, uint64_t *len) {
  if (!km || !prefix || !chr_name || !text || !len) return GS_ERR_ARG;
  if (km->parsed) {
    gs_set_error("gs_kmers_csv on the rows of a kmers file: they carry no positions");
    return GS_ERR_ARG;
  }
  *text = nullptr;
  *len = 0;
  void *d_text = nullptr;
  uint64_t bytes = 0;
  gs_status rc;
  try {
    rc = km_encode(km, prefix, chr_name, true, nullptr, &d_text, &bytes);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  if (rc != GS_OK) return rc;
  rc = gs_text_to_host(d_text, bytes, text);
  hipFree(d_text);
  if (rc == GS_OK) *len = bytes;
  return rc;
}

extern "C" gs_status gs_kmers_concat(gs_kmers *const *parts, uint32_t n_parts, gs_kmers **out) {
  if (!out || (n_parts && !parts)) return GS_ERR_ARG;
  for (uint32_t i = 0; i < n_parts; i++)
    if (!parts[i]) return GS_ERR_ARG;
  for (uint32_t i = 0; i < n_parts; i++)
    if (parts[i]->device != parts[0]->device || parts[i]->k != parts[0]->k || parts[i]->P != parts[0]->P ||
        parts[i]->have_ids != parts[0]->have_ids || parts[i]->parsed != parts[0]->parsed || parts[i]->device < 0) {
      gs_set_error("gs_kmers_concat: parts of different devices, kmer or PAM lengths or origins, or ids on some of them only");
      return GS_ERR_ARG;
    }
  std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new (std::nothrow) gs_kmers(), km_release);
  gs_kmers *km = own.get();
  if (!km) return GS_ERR_NOMEM;
  if (n_parts == 0) {
    *out = own.release();
    return GS_OK;
  }
  km->device = parts[0]->device;
  km->k = parts[0]->k;
  km->P = parts[0]->P;
  km->have_ids = parts[0]->have_ids;
  km->parsed = parts[0]->parsed;
  for (uint32_t i = 0; i < n_parts; i++) {
    km->n += parts[i]->n;
    km->id_bytes += parts[i]->id_bytes;
    km->ids_fixed = km->ids_fixed || parts[i]->ids_fixed;
  }
  const uint32_t k = km->k, P = km->P;
  GS_HIP(hipSetDevice(km->device));
  GS_TRY(km_alloc((size_t)km->n * k, &km->d_seqs));
  GS_TRY(km_alloc((size_t)km->n * P, &km->d_pams));
  if (!km->parsed) GS_TRY(km_alloc(4 * (size_t)km->n, &km->d_pos));
  GS_TRY(km_alloc((size_t)km->n, &km->d_sense));
  if (km->have_ids) {
    GS_TRY(km_alloc((size_t)km->id_bytes, &km->d_ids));
    GS_TRY(km_alloc(8 * ((size_t)km->n + 1), &km->d_id_off));
    GS_TRY(km_alloc((size_t)km->n, &km->d_sense01));
  }
  uint64_t at = 0, id_at = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const gs_kmers *p = parts[i];
    const bool last = i + 1 == n_parts;
    if (p->n) {
      GS_HIP(hipMemcpyAsync((char *)km->d_seqs + at * k, p->d_seqs, (size_t)p->n * k, hipMemcpyDeviceToDevice, nullptr));
      GS_HIP(hipMemcpyAsync((char *)km->d_pams + at * P, p->d_pams, (size_t)p->n * P, hipMemcpyDeviceToDevice, nullptr));
      if (!km->parsed) GS_HIP(hipMemcpyAsync((char *)km->d_pos + at * 4, p->d_pos, (size_t)p->n * 4, hipMemcpyDeviceToDevice, nullptr));
      GS_HIP(hipMemcpyAsync((char *)km->d_sense + at, p->d_sense, (size_t)p->n, hipMemcpyDeviceToDevice, nullptr));
    }
    if (km->have_ids) {
      if (p->n) GS_HIP(hipMemcpyAsync((char *)km->d_sense01 + at, p->d_sense01, (size_t)p->n, hipMemcpyDeviceToDevice, nullptr));
      if (p->id_bytes) GS_HIP(hipMemcpyAsync((char *)km->d_ids + id_at, p->d_ids, (size_t)p->id_bytes, hipMemcpyDeviceToDevice, nullptr));
      const uint64_t cnt = p->n + (last ? 1u : 0u); /* the last part's closing offset closes the stream */
      if (cnt)
        hipLaunchKernelGGL(k_km_rebase, dim3((unsigned)((cnt + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, nullptr,
                           (const uint64_t *)p->d_id_off, cnt, id_at, (uint64_t *)km->d_id_off + at);
    }
    at += p->n;
    id_at += p->id_bytes;
  }
  GS_HIP(hipStreamSynchronize(nullptr));
  GS_HIP(hipGetLastError());
  *out = own.release();
  return GS_OK;
}

/* ---- sequence rules on a scan's candidates (no counterpart in the reference; the rule is gs_select_scan.h's) ----------
 *   k_km_rule   one lane per candidate: the rule over its k bytes -> a 64-bit flag and the charged rule; a wave's failures
 *               go to the three counters with one atomic each                     (k B read, 9 B written)
 *   (rocprim 64-bit exclusive scan of the n + 1 flags: the places)
 *   k_km_keep   the passing candidates into a fresh object at their places: stable   (k + P + 5 + 16 B read, k + P + 5 written) */
struct gs_km_filter_args {
  const uint8_t *seqs, *pams, *sense;
  const uint32_t *pos;
  uint64_t *flag;        /* n + 1 */
  const uint64_t *place; /* n + 1 */
  uint8_t *charge;
  unsigned long long *failed; /* by GC, run, motif */
  uint8_t *o_seqs, *o_pams, *o_sense;
  uint32_t *o_pos;
  uint64_t n;
  uint32_t k, P;
};
__global__ __launch_bounds__(KM_BLOCK) void k_km_rule(gs_km_filter_args a, gs_seq_rule rule) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  const bool in = j < a.n;
  uint32_t ch = GS_SL_PASS;
  if (in) {
    ch = gs_sl_charge(rule, a.seqs + j * a.k, a.k);
    a.charge[j] = (uint8_t)ch;
  }
  if (j <= a.n) a.flag[j] = in && ch == GS_SL_PASS ? 1ull : 0ull; /* one more entry closes the scan */
  for (uint32_t r = GS_SL_GC; r <= GS_SL_MOTIF; r++) {
    const unsigned long long b = __ballot(in && ch == r);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&a.failed[r - 1u], (unsigned long long)__popcll(b));
  }
}
__global__ __launch_bounds__(KM_BLOCK) void k_km_keep(gs_km_filter_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  if (j >= a.n || !a.flag[j]) return;
  const uint64_t o = a.place[j];
  for (uint32_t u = 0; u < a.k; u++) a.o_seqs[o * a.k + u] = a.seqs[j * a.k + u];
  for (uint32_t u = 0; u < a.P; u++) a.o_pams[o * a.P + u] = a.pams[j * a.P + u];
  a.o_pos[o] = a.pos[j];
  a.o_sense[o] = a.sense[j];
}

extern "C" gs_status gs_seq_rule_init(gs_seq_rule *rule) {
  if (!rule) return GS_ERR_ARG;
  memset(rule, 0, sizeof *rule);
  rule->gc_max = 100;
  return GS_OK;
}

extern "C" gs_status gs_seq_rule_add_motif(gs_seq_rule *rule, const char *motif, int both_strands) {
  if (!rule || !motif) return GS_ERR_ARG;
  const size_t len = strlen(motif);
  auto refuse = [&](const std::string &why) {
    gs_set_error("motif '" + std::string(motif) + "': " + why);
    return GS_ERR_FORMAT;
  };
  if (len == 0) return refuse("an empty motif");
  if (len > GS_SEQ_MOTIF_LETTERS) return refuse("more than 32 letters");
  for (size_t p = 0; p < len; p++)
    if (!gs_sl_iupac((uint8_t)motif[p])) return refuse(std::string("the letter '") + motif[p] + "' is not one of ACGTRYSWKMBDHVN");
  bool twin = false; /* the reverse complement, where it is another motif */
  for (size_t p = 0; p < len && both_strands; p++)
    twin = twin || gs_sl_complement(gs_sl_iupac((uint8_t)motif[len - 1 - p])) != gs_sl_iupac((uint8_t)motif[p]);
  if (rule->n_motifs > GS_SEQ_MOTIFS || rule->n_motifs + (twin ? 2u : 1u) > GS_SEQ_MOTIFS) return refuse("more than 16 motifs");
  for (uint32_t t = 0; t < (twin ? 2u : 1u); t++) {
    const uint32_t m = rule->n_motifs++;
    rule->motif_len[m] = (uint8_t)len;
    memset(rule->motif_set[m], 0, sizeof rule->motif_set[m]);
    for (size_t p = 0; p < len; p++) {
      const uint32_t set = gs_sl_iupac((uint8_t)motif[t ? len - 1 - p : p]);
      gs_sl_motif_put(*rule, m, (uint32_t)p, t ? gs_sl_complement(set) : set);
    }
  }
  return GS_OK;
}

static gs_status km_rule_args(const gs_seq_rule *rule) {
  if (!rule) return GS_ERR_ARG;
  if (!gs_sl_rule_ok(*rule)) {
    gs_set_error("sequence rule: 0 <= gc_min <= gc_max <= 100, at most 16 motifs of 1 to 32 IUPAC letters");
    return GS_ERR_ARG;
  }
  return GS_OK;
}

extern "C" gs_status gs_kmers_filter(gs_kmers *km, const gs_seq_rule *rule, void *stream, gs_kmers **out, uint64_t counts[4]) {
  if (!km || !out) return GS_ERR_ARG;
  GS_TRY(km_rule_args(rule));
  if (km->parsed || km->device < 0) {
    gs_set_error("gs_kmers_filter takes the candidates of a scan on a device");
    return GS_ERR_ARG;
  }
  if (km->have_ids) {
    gs_set_error("gs_kmers_filter after gs_kmers_encode_ids: the ids would name candidates that are gone");
    return GS_ERR_ARG;
  }
  *out = nullptr;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n = km->n;
  const uint32_t k = km->k, P = km->P;
  uint64_t failed[3] = {0, 0, 0}, kept = 0;
  struct events { /* around the rule and the scan, and around the gather */
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~events() {
      for (hipEvent_t x : e)
        if (x) hipEventDestroy(x);
    }
  } ev;
  try {
    GS_HIP(hipSetDevice(km->device));
    std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new gs_kmers(), km_release);
    gs_kmers *f = own.get();
    f->device = km->device;
    f->k = k;
    f->P = P;
    if (n) {
      gs_scratch mem;
      gs_prim_tmp tmp;
      uint64_t *d_flag = nullptr, *d_place = nullptr;
      uint8_t *d_charge = nullptr;
      unsigned long long *d_failed = nullptr;
      GS_TRY(mem.get(8 * (n + 1), &d_flag));
      GS_TRY(mem.get(8 * (n + 1), &d_place));
      GS_TRY(mem.get(n, &d_charge));
      GS_TRY(mem.get(24, &d_failed));
      GS_HIP(hipMemsetAsync(d_failed, 0, 24, st));
      for (hipEvent_t &x : ev.e) GS_HIP(hipEventCreate(&x));
      gs_km_filter_args a;
      memset(&a, 0, sizeof a);
      a.seqs = (const uint8_t *)km->d_seqs;
      a.pams = (const uint8_t *)km->d_pams;
      a.sense = (const uint8_t *)km->d_sense;
      a.pos = (const uint32_t *)km->d_pos;
      a.flag = d_flag;
      a.place = d_place;
      a.charge = d_charge;
      a.failed = d_failed;
      a.n = n;
      a.k = k;
      a.P = P;
      GS_HIP(hipEventRecord(ev.e[0], st));
      hipLaunchKernelGGL(k_km_rule, dim3((unsigned)((n + 1 + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, st, a, *rule);
      GS_HIP(hipEventRecord(ev.e[1], st));
      GS_TRY(gs_prim("kmers filter: scan of the flags", mem, tmp, [&](void *t, size_t &tb) {
        return rocprim::exclusive_scan(t, tb, d_flag, d_place, 0ull, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
      }));
      GS_HIP(hipEventRecord(ev.e[2], st));
      GS_HIP(hipMemcpyAsync(&kept, d_place + n, 8, hipMemcpyDeviceToHost, st));
      GS_HIP(hipMemcpyAsync(failed, d_failed, 24, hipMemcpyDeviceToHost, st));
      GS_HIP(hipStreamSynchronize(st));
      if (kept > n) {
        gs_set_error("gs_kmers_filter: more candidates kept than scanned");
        return GS_ERR_DEVICE;
      }
      float ms = 0;
      GS_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
      f->filter_ms[0] = ms;
      GS_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
      f->filter_ms[1] = ms;
      f->n = kept;
      if (kept) {
        GS_TRY(km_alloc((size_t)kept * k, &f->d_seqs));
        GS_TRY(km_alloc((size_t)kept * P, &f->d_pams));
        GS_TRY(km_alloc(4 * (size_t)kept, &f->d_pos));
        GS_TRY(km_alloc((size_t)kept, &f->d_sense));
        a.o_seqs = (uint8_t *)f->d_seqs;
        a.o_pams = (uint8_t *)f->d_pams;
        a.o_sense = (uint8_t *)f->d_sense;
        a.o_pos = (uint32_t *)f->d_pos;
        GS_HIP(hipEventRecord(ev.e[3], st));
        hipLaunchKernelGGL(k_km_keep, dim3((unsigned)((n + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, st, a);
        GS_HIP(hipEventRecord(ev.e[4], st));
        GS_HIP(hipStreamSynchronize(st));
        GS_HIP(hipEventElapsedTime(&ms, ev.e[3], ev.e[4]));
        f->filter_ms[2] = ms;
      }
      GS_HIP(hipGetLastError());
    }
    if (counts) {
      counts[0] = n;
      for (int i = 0; i < 3; i++) counts[1 + i] = failed[i];
    }
    *out = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_debug_kmers_filter_ms(const gs_kmers *filtered, double out[3]) {
  if (!filtered || !out) return GS_ERR_ARG;
  for (int i = 0; i < 3; i++) out[i] = filtered->filter_ms[i];
  return GS_OK;
}

extern "C" gs_status gs_debug_kmers_filter_host(const uint8_t *seqs, uint64_t n, uint32_t k, const gs_seq_rule *rule, uint8_t *charge,
                                                uint64_t counts[4]) {
  if ((n && (!seqs || !charge)) || k < 1 || k > 64) return GS_ERR_ARG;
  GS_TRY(km_rule_args(rule));
  uint64_t c[4] = {n, 0, 0, 0};
  for (uint64_t j = 0; j < n; j++) {
    const uint32_t ch = gs_sl_charge(*rule, seqs + j * k, k);
    charge[j] = (uint8_t)ch;
    if (ch) c[ch]++;
  }
  if (counts)
    for (int i = 0; i < 4; i++) counts[i] = c[i];
  return GS_OK;
}

extern "C" void gs_kmers_free(gs_kmers *km) { km_release(km); }
