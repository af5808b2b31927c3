/*
 * gs_kmersfile.hip -- the kmers file read on the device (src/genomics/kmer.cxx:9-25 as
 * cli::read_kmers reads it): the raw bytes of a file, in HBM, to a gs_kmers object - sequences, PAMs, ids, id offsets and
 * senses in the layout gs_format_device_ids / gs_enumerate_text_device take.  The rules and the sequential core are
 * gs_kmers_scan.h.  Four passes:
 *   a. k_kf_tile<KF_SUM>     a summary per tile of 4,096 bytes (256 lanes x one 16-byte load; newlines are a bit mask of
 *                            the loaded words), a rocPRIM scan of the summaries under gs_km_compose (what stands left of
 *                            each tile), then k_kf_tile<KF_STARTS>: every newline writes the start of the line behind it
 *   b. k_kf_lines            a lane per line walks it in 16-byte windows (gs_km_walk_line: a line may be of any length):
 *                            the lengths of id, sequence and PAM, the sense bit, the error code
 *   c. a rocPRIM scan of (is a row, id length) over the lines: each row's number and id offset; and, folded into pass b,
 *                            the reductions: the smallest failing line with its kind, the least and greatest L and P
 *   d. k_kf_emit             a lane per row walks its line again and copies the three fields to their places
 * The header line is parsed on the host (gs_km_parse_header) from its bytes, which are the first thing copied back.
 * Offsets are 64 bits throughout.  Next to the raw bytes and the outputs the passes hold 40 bytes per line (its start, its
 * four 32-bit results, its scanned pair) and 48 bytes per tile; all of that, and the raw bytes where the call made the
 * copy, is freed before the call returns.
 */
#include "gs_common.h"
#include "gs_device.h"
#include "gs_scratch.h"
#include "gs_block_scan.h"
#include "gs_kmers_obj.h"
#include "gs_kmers_scan.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdlib>

#define KF_THREADS 256u
#define KF_TILE (KF_THREADS * GS_KM_WIN)

enum { KF_SUM = 0, KF_STARTS = 1 };

namespace {

struct kf_rec {
  uint32_t id_len, L, P; /* saturated at UINT32_MAX (KF_OVER) */
  uint32_t flags;
};
#define KF_ROW 1u
#define KF_PLUS 2u
#define KF_OVER 4u
struct kf_pair { /* rows and id bytes in front of a line */
  unsigned long long rows, ids;
};
struct kf_red {
  unsigned long long bad; /* line << 2 | kind of the first failing line, or all ones */
  uint32_t min_L, max_L, min_P, max_P, over, pad;
};

struct kf_args {
  const uint8_t *raw;
  uint64_t len, n_tiles, n_lines;
  uint32_t phase;
  gs_km_header hdr;
  gs_km_sum *sums;       /* pass a: sums[k + 1] = tile k */
  const gs_km_sum *fwd;  /* fwd[k] = tiles 0 .. k-1 */
  uint64_t *starts;      /* n_lines + 1 */
  kf_rec *recs;          /* n_lines + 1: the header's and the closing entry are no rows */
  const kf_pair *before; /* n_lines + 1 */
  kf_red *red;
  uint8_t *seqs, *pams, *ids, *sense01, *sense;
  uint64_t *id_off;
  uint32_t L, P;
};

struct kf_compose {
  __host__ __device__ gs_km_sum operator()(const gs_km_sum &a, const gs_km_sum &b) const { return gs_km_compose(a, b); }
};
struct kf_to_pair {
  __host__ __device__ kf_pair operator()(const kf_rec &r) const { return kf_pair{r.flags & KF_ROW, (r.flags & KF_ROW) ? r.id_len : 0u}; }
};
struct kf_pair_add {
  __host__ __device__ kf_pair operator()(const kf_pair &a, const kf_pair &b) const { return kf_pair{a.rows + b.rows, a.ids + b.ids}; }
};

template <int MODE>
__global__ __launch_bounds__(KF_THREADS) void k_kf_tile(kf_args a) {
  __shared__ gs_km_sum s_scan[KF_THREADS];
  const uint32_t t = threadIdx.x;
  const uint64_t v_end = a.len + a.phase;
  for (uint64_t k = blockIdx.x; k < a.n_tiles; k += gridDim.x) {
    const uint64_t v0 = k * KF_TILE + (uint64_t)t * GS_KM_WIN;
    uint32_t w[4];
    gs_km_load(a.raw, a.len, a.phase, v0, w);
    const uint32_t lo = v0 < a.phase ? (uint32_t)std::min<uint64_t>(a.phase - v0, GS_KM_WIN) : 0u;
    const uint32_t hi = v0 >= v_end ? 0u : (uint32_t)std::min<uint64_t>(v_end - v0, GS_KM_WIN);
    const uint32_t valid = hi > lo ? gs_km_bits_below(hi) & ~gs_km_bits_below(lo) : 0u;
    uint32_t nl = gs_km_eq16(w, '\n') & valid;
    gs_km_sum s;
    s.len = valid ? hi - lo : 0u;
    s.n_nl = (uint32_t)__builtin_popcount(nl);
    s.open = valid && !((nl >> (hi - 1u)) & 1u);
    gs_km_sum tile;
    const gs_km_sum left_in = gs_block_scan<KF_THREADS>(s_scan, s, t, kf_compose(), gs_km_identity(), &tile);
    if (MODE == KF_SUM) {
      if (t == 0) a.sums[k + 1] = tile;
      continue;
    }
    uint64_t rank = a.fwd[k].n_nl + left_in.n_nl; /* newlines in front of this window: at most n_lines - 1 follow */
    while (nl) {
      const uint32_t j = (uint32_t)__builtin_ctz(nl);
      nl &= nl - 1u;
      a.starts[++rank] = v0 + j - a.phase + 1u;
    }
  }
}

__device__ __forceinline__ uint32_t kf_sat(uint64_t v) { return v >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

/* a lane per line; every wave folds its lines' shapes and its first failing line into a.red */
__global__ __launch_bounds__(KF_THREADS) void k_kf_lines(kf_args a) {
  unsigned long long bad = ~0ull;
  uint32_t min_L = ~0u, max_L = 0, min_P = ~0u, max_P = 0, over = 0;
  const uint64_t total = a.n_lines + 1, step = (uint64_t)gridDim.x * KF_THREADS;
  for (uint64_t base = (uint64_t)blockIdx.x * KF_THREADS; base < total; base += step) {
    const uint64_t i = base + threadIdx.x;
    if (i >= total) continue;
    kf_rec r{0, 0, 0, 0};
    if (i >= 1 && i < a.n_lines) {
      const uint64_t s = a.starts[i], e = gs_km_line_end(a.raw, s, a.starts[i + 1]);
      if (e > s) {
        gs_km_line ln;
        gs_km_walk_line(a.raw, a.len, a.phase, GS_KM_WIN, s, e, a.hdr, ln);
        if (ln.err != GS_KM_OK) {
          bad = std::min<unsigned long long>(bad, (i << 2) | ln.err);
        } else {
          r.id_len = kf_sat(ln.e[GS_KM_ID] - ln.b[GS_KM_ID]);
          r.L = kf_sat(ln.e[GS_KM_SEQ] - ln.b[GS_KM_SEQ]);
          r.P = kf_sat(ln.e[GS_KM_PAM] - ln.b[GS_KM_PAM]);
          r.flags = KF_ROW | (ln.sense ? KF_PLUS : 0u);
          if (r.id_len == ~0u || r.L == ~0u || r.P == ~0u) r.flags |= KF_OVER, over = 1;
          min_L = std::min(min_L, r.L), max_L = std::max(max_L, r.L);
          min_P = std::min(min_P, r.P), max_P = std::max(max_P, r.P);
        }
      }
    }
    a.recs[i] = r;
  }
  for (int o = 32; o > 0; o >>= 1) {
    bad = std::min<unsigned long long>(bad, __shfl_xor(bad, o));
    min_L = std::min(min_L, (uint32_t)__shfl_xor(min_L, o)), max_L = std::max(max_L, (uint32_t)__shfl_xor(max_L, o));
    min_P = std::min(min_P, (uint32_t)__shfl_xor(min_P, o)), max_P = std::max(max_P, (uint32_t)__shfl_xor(max_P, o));
    over |= (uint32_t)__shfl_xor(over, o);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (bad != ~0ull) atomicMin(&a.red->bad, bad);
    if (min_L != ~0u) {
      atomicMin(&a.red->min_L, min_L), atomicMax(&a.red->max_L, max_L);
      atomicMin(&a.red->min_P, min_P), atomicMax(&a.red->max_P, max_P);
    }
    if (over) atomicOr(&a.red->over, 1u);
  }
}

/* a lane per row: its fields to their places; the closing entry writes the last id offset */
__global__ __launch_bounds__(KF_THREADS) void k_kf_emit(kf_args a) {
  const uint64_t total = a.n_lines + 1, step = (uint64_t)gridDim.x * KF_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * KF_THREADS + threadIdx.x; i < total; i += step) {
    const kf_pair at = a.before[i];
    if (i == a.n_lines) a.id_off[at.rows] = at.ids;
    if (!(a.recs[i].flags & KF_ROW)) continue;
    const uint64_t s = a.starts[i], e = gs_km_line_end(a.raw, s, a.starts[i + 1]);
    gs_km_line ln;
    gs_km_walk_line(a.raw, a.len, a.phase, GS_KM_WIN, s, e, a.hdr, ln);
    const uint64_t r = at.rows;
    const uint8_t *src = a.raw + ln.b[GS_KM_SEQ];
    for (uint32_t j = 0; j < a.L; j++) a.seqs[r * a.L + j] = src[j];
    src = a.raw + ln.b[GS_KM_PAM];
    for (uint32_t j = 0; j < a.P; j++) a.pams[r * a.P + j] = src[j];
    src = a.raw + ln.b[GS_KM_ID];
    const uint64_t id_len = ln.e[GS_KM_ID] - ln.b[GS_KM_ID];
    for (uint64_t j = 0; j < id_len; j++) a.ids[at.ids + j] = src[j];
    a.id_off[r] = at.ids;
    a.sense01[r] = (uint8_t)ln.sense;
    a.sense[r] = ln.sense ? '+' : '-';
  }
}

void kf_report_clear(gs_kmers_report *rep) {
  if (rep) memset(rep, 0, sizeof *rep);
}
gs_status kf_report_bad(gs_kmers_report *rep, uint32_t kind, uint64_t line, uint64_t row, uint64_t off, const std::string &text) {
  static const char *const what[5] = {"", "kmers row with too few columns: ", "kmers position is not an integer: ", "empty kmers file",
                                      "kmers file lacks column "};
  gs_set_error(std::string(what[kind]) + text);
  if (rep) {
    rep->bad_kind = kind;
    rep->bad_line = line;
    rep->bad_row = row;
    rep->bad_off = off;
    rep->bad_len = text.size();
    rep->bad_text = (char *)malloc(text.size() + 1);
    if (!rep->bad_text) return GS_ERR_NOMEM;
    memcpy(rep->bad_text, text.data(), text.size());
    rep->bad_text[text.size()] = 0;
  }
  return GS_ERR_FORMAT;
}
gs_status kf_unsupported(gs_kmers_report *rep, uint64_t n) {
  if (rep) rep->n = n;
  gs_set_error("kmers file with rows of several shapes, or without sequences: read on the host");
  return GS_ERR_UNSUPPORTED;
}

gs_status kf_run(int device, const uint8_t *d_raw, uint64_t len, hipStream_t st, gs_kmers *km, gs_kmers_report *rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (len == 0) return kf_report_bad(rep, GS_KM_EMPTY, 0, 0, 0, "");
  gs_scratch mem;
  kf_args a;
  memset(&a, 0, sizeof a);
  a.raw = d_raw;
  a.len = len;
  a.phase = (uint32_t)((uintptr_t)d_raw & 15u);
  const uint64_t nt = (len + a.phase + KF_TILE - 1) / KF_TILE;
  a.n_tiles = nt;
  void *sums, *fwd, *red;
  gs_prim_tmp tmp, tmp_p;
  GS_TRY(mem.get(sizeof(gs_km_sum) * (nt + 1), &sums));
  GS_TRY(mem.get(sizeof(gs_km_sum) * (nt + 1), &fwd));
  GS_TRY(mem.get(sizeof(kf_red), &red));
  a.sums = (gs_km_sum *)sums;
  a.fwd = (const gs_km_sum *)fwd;
  a.red = (kf_red *)red;
  const uint32_t cus = (uint32_t)gs_num_cus(device);
  const uint32_t tile_grid = (uint32_t)std::min<uint64_t>(nt, (uint64_t)cus * 64u);
  gs_events<8> ev;
  for (hipEvent_t &e : ev.e) GS_HIP(hipEventCreate(&e));
  /* a. */
  GS_HIP(hipMemsetAsync(sums, 0, sizeof(gs_km_sum), st)); /* gs_km_identity() */
  GS_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(k_kf_tile<KF_SUM>, dim3(tile_grid), dim3(KF_THREADS), 0, st, a);
  GS_TRY(gs_prim("kmers file: scan of the tiles", mem, tmp, [&](void *t, size_t &tb) {
    return rocprim::inclusive_scan(t, tb, a.sums, (gs_km_sum *)fwd, (size_t)nt + 1, kf_compose(), st);
  }));
  gs_km_sum whole;
  GS_HIP(hipMemcpyAsync(&whole, (const gs_km_sum *)fwd + nt, sizeof whole, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  const uint64_t n_lines = gs_km_lines(whole); /* >= 1: the file has bytes */
  a.n_lines = n_lines;
  void *starts;
  GS_TRY(mem.get(8 * (n_lines + 1), &starts));
  a.starts = (uint64_t *)starts;
  const uint64_t first = 0, past = len + 1;
  GS_HIP(hipMemcpyAsync(starts, &first, 8, hipMemcpyHostToDevice, st));
  if (whole.open) GS_HIP(hipMemcpyAsync(a.starts + n_lines, &past, 8, hipMemcpyHostToDevice, st));
  GS_HIP(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(k_kf_tile<KF_STARTS>, dim3(tile_grid), dim3(KF_THREADS), 0, st, a);
  GS_HIP(hipEventRecord(ev.e[2], st));
  /* the header line, on the host */
  uint64_t second = 0;
  GS_HIP(hipMemcpyAsync(&second, a.starts + 1, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  std::string header((size_t)(second - 1), '\0');
  if (!header.empty()) GS_HIP(hipMemcpy(&header[0], d_raw, header.size(), hipMemcpyDeviceToHost));
  if (!header.empty() && header.back() == '\r') header.pop_back();
  const int missing = gs_km_parse_header((const uint8_t *)header.data(), header.size(), a.hdr);
  if (missing >= 0) return kf_report_bad(rep, GS_KM_LACKS, 0, 0, 0, gs_km_column_name(missing));
  /* b. and c. */
  void *recs, *before;
  GS_TRY(mem.get(sizeof(kf_rec) * (n_lines + 1), &recs));
  GS_TRY(mem.get(sizeof(kf_pair) * (n_lines + 1), &before));
  a.recs = (kf_rec *)recs;
  a.before = (const kf_pair *)before;
  const kf_red none{~0ull, ~0u, 0u, ~0u, 0u, 0u, 0u};
  GS_HIP(hipMemcpyAsync(red, &none, sizeof none, hipMemcpyHostToDevice, st));
  GS_HIP(hipStreamSynchronize(st)); /* `none` is on this frame */
  const uint32_t line_grid = (uint32_t)std::min<uint64_t>((n_lines + 1 + KF_THREADS - 1) / KF_THREADS, (uint64_t)cus * 32u);
  GS_HIP(hipEventRecord(ev.e[3], st));
  hipLaunchKernelGGL(k_kf_lines, dim3(line_grid), dim3(KF_THREADS), 0, st, a);
  GS_HIP(hipEventRecord(ev.e[4], st));
  GS_TRY(gs_prim("kmers file: scan of the lines", mem, tmp_p, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, rocprim::make_transform_iterator((const kf_rec *)recs, kf_to_pair()), (kf_pair *)before,
                                   kf_pair{0, 0}, (size_t)n_lines + 1, kf_pair_add(), st);
  }));
  GS_HIP(hipEventRecord(ev.e[5], st));
  kf_red got;
  kf_pair all;
  GS_HIP(hipMemcpyAsync(&got, red, sizeof got, hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(&all, (const kf_pair *)before + n_lines, sizeof all, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  if (rep) rep->n_lines = n_lines;
  if (got.bad != ~0ull) { /* only the failing line comes back */
    const uint64_t line = got.bad >> 2;
    uint64_t se[2];
    kf_pair at;
    GS_HIP(hipMemcpy(se, a.starts + line, 16, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(&at, (const kf_pair *)before + line, sizeof at, hipMemcpyDeviceToHost));
    std::string text((size_t)(se[1] - 1 - se[0]), '\0');
    GS_HIP(hipMemcpy(&text[0], d_raw + se[0], text.size(), hipMemcpyDeviceToHost));
    if (text.back() == '\r') text.pop_back();
    gs_km_line ln;
    gs_km_walk_line((const uint8_t *)text.data(), text.size(), 0, GS_KM_WIN, 0, text.size(), a.hdr, ln);
    if (ln.err == GS_KM_FEW) return kf_report_bad(rep, GS_KM_FEW, line, at.rows, se[0], text);
    return kf_report_bad(rep, GS_KM_POSITION, line, at.rows, se[0] + ln.b[GS_KM_POS],
                         text.substr((size_t)ln.b[GS_KM_POS], (size_t)(ln.e[GS_KM_POS] - ln.b[GS_KM_POS])));
  }
  const uint64_t n = all.rows;
  km->n = n;
  km->id_bytes = all.ids;
  if (n && (got.over || got.min_L != got.max_L || got.min_P != got.max_P || got.min_L == 0)) return kf_unsupported(rep, n);
  km->k = a.L = n ? got.min_L : 0u;
  km->P = a.P = n ? got.min_P : 0u;
  /* d. */
  void *seqs, *pams, *ids, *id_off, *s01, *sense;
  GS_TRY(mem.get((size_t)n * a.L, &seqs));
  GS_TRY(mem.get((size_t)n * a.P, &pams));
  GS_TRY(mem.get((size_t)all.ids, &ids));
  GS_TRY(mem.get(8 * (n + 1), &id_off));
  GS_TRY(mem.get((size_t)n, &s01));
  GS_TRY(mem.get((size_t)n, &sense));
  a.seqs = (uint8_t *)seqs, a.pams = (uint8_t *)pams, a.ids = (uint8_t *)ids, a.id_off = (uint64_t *)id_off;
  a.sense01 = (uint8_t *)s01, a.sense = (uint8_t *)sense;
  GS_HIP(hipEventRecord(ev.e[6], st));
  hipLaunchKernelGGL(k_kf_emit, dim3(line_grid), dim3(KF_THREADS), 0, st, a);
  GS_HIP(hipEventRecord(ev.e[7], st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  for (void *q : {seqs, pams, ids, id_off, s01, sense}) mem.keep(q);
  km->d_seqs = seqs, km->d_pams = pams, km->d_ids = ids, km->d_id_off = id_off, km->d_sense01 = s01, km->d_sense = sense;
  if (rep) {
    rep->n = n, rep->L = a.L, rep->P = a.P;
    static const int from[5] = {0, 1, 3, 4, 6}; /* 0 -> 1 holds the wait for the line count and the allocation too */
    GS_TRY(ev.elapsed(from, 5, rep->ms + 3));
    rep->ms[2] = gs_ms_since(t0);
  }
  return GS_OK;
}

gs_kmers *kf_new(int device) {
  gs_kmers *km = new gs_kmers();
  km->device = device;
  km->parsed = true;
  km->have_ids = true;
  return km;
}

std::atomic<uint64_t> g_chunk_bytes{(uint64_t)32 << 20};

}  // namespace

extern "C" gs_status gs_kmers_parse_device(int device, const void *d_raw, uint64_t len, void *stream, gs_kmers **out, gs_kmers_report *rep) {
  kf_report_clear(rep);
  if (!out || (len && !d_raw)) return GS_ERR_ARG;
  *out = nullptr;
  gs_kmers *km = nullptr;
  try {
    GS_HIP(hipSetDevice(device));
    km = kf_new(device);
    const gs_status rc = kf_run(device, (const uint8_t *)d_raw, len, (hipStream_t)stream, km, rep);
    if (rc != GS_OK) {
      gs_kmers_free(km);
      return rc;
    }
    *out = km;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    gs_kmers_free(km);
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_kmers_parse(int device, const uint8_t *raw, uint64_t len, gs_kmers **out, gs_kmers_report *rep) {
  kf_report_clear(rep);
  if (!out || (len && !raw)) return GS_ERR_ARG;
  *out = nullptr;
  GS_HIP(hipSetDevice(device));
  gs_scratch mem;
  void *d_raw = nullptr;
  GS_TRY(mem.get(len, &d_raw));
  const auto t0 = std::chrono::steady_clock::now();
  if (len) GS_HIP(hipMemcpy(d_raw, raw, len, hipMemcpyHostToDevice));
  const double up = gs_ms_since(t0);
  const gs_status rc = gs_kmers_parse_device(device, d_raw, len, nullptr, out, rep);
  if (rep) rep->ms[1] = up;
  return rc;
}

extern "C" uint64_t gs_debug_kmers_chunk_bytes(uint64_t set) {
  if (set) g_chunk_bytes.store(set);
  return g_chunk_bytes.load();
}

extern "C" gs_status gs_kmers_parse_file(int device, const char *path, gs_kmers **out, gs_kmers_report *rep) {
  kf_report_clear(rep);
  if (!out || !path) return GS_ERR_ARG;
  *out = nullptr;
  gs_staged_file f;
  gs_status rc = f.open(device, path, g_chunk_bytes.load());
  if (rc == GS_OK) rc = gs_kmers_parse_device(device, f.d_raw, f.size, f.st, out, rep);
  if (rep) { /* also of a file that did not parse */
    rep->ms[0] = f.ms_read;
    rep->ms[1] = f.ms_wait;
  }
  return rc;
}

extern "C" uint64_t gs_debug_kmers_tile_bytes(void) { return KF_TILE; }

extern "C" gs_status gs_debug_kmers_host(const uint8_t *raw, uint64_t len, uint64_t tile_bytes, gs_kmers **out, gs_kmers_report *rep) {
  kf_report_clear(rep);
  if (!out || (len && !raw) || tile_bytes == 0) return GS_ERR_ARG;
  *out = nullptr;
  gs_kmers *km = nullptr;
  try {
    gs_km_parsed p;
    gs_km_host_parse(raw, len, tile_bytes, (uint32_t)std::min<uint64_t>(tile_bytes, GS_KM_WIN), 0, p);
    if (rep) rep->n_lines = p.n_lines;
    if (p.bad_kind != GS_KM_OK) return kf_report_bad(rep, p.bad_kind, p.bad_line, p.bad_row, p.bad_off, p.bad_text);
    if (p.mixed || p.L >= 0xFFFFFFFFull || p.P >= 0xFFFFFFFFull) return kf_unsupported(rep, p.n);
    km = kf_new(-1);
    km->n = p.n;
    km->k = (uint32_t)p.L;
    km->P = (uint32_t)p.P;
    km->id_bytes = p.ids.size();
    km->h_seqs.swap(p.seqs), km->h_pams.swap(p.pams), km->h_ids.swap(p.ids), km->h_id_off.swap(p.id_off), km->h_sense01.swap(p.sense01);
    km->h_sense.resize(km->n);
    for (uint64_t r = 0; r < km->n; r++) km->h_sense[r] = km->h_sense01[r] ? '+' : '-';
    km->have_host = km->have_host_ids = true;
    if (rep) rep->n = km->n, rep->L = km->k, rep->P = km->P;
    *out = km;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    if (km) gs_kmers_free(km);
    return GS_ERR_NOMEM;
  }
}
