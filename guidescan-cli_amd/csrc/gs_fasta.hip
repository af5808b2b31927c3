/*
 * gs_fasta.hip -- FASTA read on the device: the raw bytes of a file, in HBM, to the genome text
 * and the record table, under either rule set of gs_fasta_scan.h.  A streaming compaction in five passes:
 *   1. k_fa_tile<FA_SUM>    a summary per tile of 4,096 bytes (256 lanes x one 16-byte load)
 *   2. rocPRIM scans of the summaries, forward (what stands left of a tile) and backward (whether a non-blank byte follows it
 *      in its last line) - a line may span any number of tiles, so both carries may come from far away
 *   3. k_fa_tile<FA_COUNT>  kept bytes per tile, now that its edges are known
 *   4. rocPRIM scan of those counts: where each tile's bytes go
 *   5. k_fa_tile<FA_EMIT>   re-reads the tile, folds case under the index rules, writes the text and the title table
 * then k_fa_titles gathers the title lines for the host, which cuts the names out of them (host/fasta_names.hpp, the
 * functions the host readers call) and derives the extents (gs_fa_extents).  Inside a tile the same summaries are scanned
 * across the lanes in LDS, and each lane walks its sixteen bytes with gs_fa_walk - the code the host model runs.
 * Raw offsets are 64 bits throughout.
 */
#include "gs_common.h"
#include "gs_device.h"
#include "gs_scratch.h"
#include "gs_block_scan.h"
#include "gs_decoder.h"
#include "gs_fasta_scan.h"
#include "host/fasta_names.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdlib>
#include <set>

#define FA_THREADS 256u
#define FA_LANE 16u
#define FA_TILE (FA_THREADS * FA_LANE)

enum { FA_SUM = 0, FA_COUNT = 1, FA_EMIT = 2 };

struct gs_fasta {
  int device = -1; /* -1: made on the host (gs_debug_fasta_host), no text in HBM */
  uint32_t rules = 0;
  uint64_t text_len = 0, file_len = 0, file_nls = 0;
  void *d_text = nullptr;
  char *h_text = nullptr; /* the host copy, made when first asked for, under mtx */
  std::mutex mtx;
  std::vector<uint64_t> title_off, title_len, text_off, rec_len, line_len, name_off;
  std::string names;
  /* host clocks: file read, upload (waits), the device stage (its allocations, the five passes, the two waits for their
   * results), title gather + names; then the passes apart, by events in the stream: summaries, their two scans, counts, the
   * counts' scan, emit */
  double ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

struct fa_args {
  const uint8_t *raw;
  uint64_t len, n_tiles;
  uint32_t rules;
  gs_fa_sum *sums, *rsums;      /* pass 1: sums[k + 1] = tile k, rsums[n_tiles - k] = tile k */
  const gs_fa_sum *fwd, *bwd;   /* pass 2: fwd[k] = the file's start and tiles 0 .. k-1; bwd[n_tiles - 1 - k] = tiles k+1 .. */
  unsigned long long *counts;   /* pass 3 */
  const unsigned long long *koff; /* pass 4 */
  uint8_t *text;
  gs_fa_title *titles;
};

struct fa_fwd {
  __host__ __device__ gs_fa_sum operator()(const gs_fa_sum &a, const gs_fa_sum &b) const { return gs_fa_compose(a, b); }
};
struct fa_rev { /* over an array in reverse file order */
  __host__ __device__ gs_fa_sum operator()(const gs_fa_sum &a, const gs_fa_sum &b) const { return gs_fa_compose(b, a); }
};
struct fa_add {
  __host__ __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; }
};

struct fa_emitter {
  uint8_t *text;
  gs_fa_title *titles;
  __device__ __forceinline__ void keep(uint64_t at, uint8_t b) { text[at] = b; }
  __device__ __forceinline__ void title(uint64_t i, uint64_t off, uint64_t nls, uint64_t kept) {
    titles[i].off = off;
    titles[i].nls = nls;
    titles[i].kept = kept;
  }
  __device__ __forceinline__ void title_end(uint64_t i, uint64_t end) { titles[i].end = end; }
};

template <int MODE>
__global__ __launch_bounds__(FA_THREADS) void k_fa_tile(fa_args a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_bytes[FA_TILE];
  __shared__ gs_fa_sum s_scan[FA_THREADS];
  const uint32_t t = threadIdx.x;
  for (uint64_t k = blockIdx.x; k < a.n_tiles; k += gridDim.x) {
    const uint64_t at = k * FA_TILE + (uint64_t)t * FA_LANE; /* below len + FA_TILE: no overflow */
    const uint32_t n = at >= a.len ? 0u : (uint32_t)(a.len - at < FA_LANE ? a.len - at : FA_LANE);
    uint8_t *mine = s_bytes + t * FA_LANE;
    if (n == FA_LANE && (((uintptr_t)(a.raw + at)) & 15u) == 0) {
      *(uint4 *)mine = *(const uint4 *)(a.raw + at);
    } else {
      for (uint32_t i = 0; i < n; i++) mine[i] = a.raw[at + i];
    }
    /* each lane reads back its own bytes only: no barrier needed here, and the scans below begin with one */
    const gs_fa_sum s = gs_fa_summarize(mine, n);
    gs_fa_sum tile;
    const gs_fa_sum left_in = gs_block_scan<FA_THREADS>(s_scan, s, t, fa_fwd(), gs_fa_identity(), &tile);
    if (MODE == FA_SUM) {
      if (t == 0) {
        a.sums[k + 1] = tile;
        a.rsums[a.n_tiles - k] = tile;
      }
      continue;
    }
    const gs_fa_sum right_in = gs_block_scan<FA_THREADS>(s_scan, s, FA_THREADS - 1u - t, fa_rev(), gs_fa_identity(), (gs_fa_sum *)nullptr);
    const gs_fa_sum left = gs_fa_compose(a.fwd[k], left_in), right = gs_fa_compose(right_in, a.bwd[a.n_tiles - 1 - k]);
    gs_fa_edge edge = gs_fa_edge_of(left, right, 0);
    gs_fa_count_only none;
    const unsigned long long mine_kept = gs_fa_walk(mine, n, at, a.rules, edge, none);
    unsigned long long tile_kept = 0;
    const unsigned long long before = gs_block_scan<FA_THREADS>((unsigned long long *)s_scan, mine_kept, t, fa_add(), 0ull, &tile_kept);
    if (MODE == FA_COUNT) {
      if (t == 0) a.counts[k] = tile_kept;
      continue;
    }
    edge.kept = a.koff[k] + before;
    fa_emitter em{a.text, a.titles};
    gs_fa_walk(mine, n, at, a.rules, edge, em);
  }
}

__global__ void k_fa_title_fill(gs_fa_title *t, uint64_t n, uint64_t len) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) t[i].end = len;
}
/* the title lines back to back: a wave per title */
__global__ __launch_bounds__(64) void k_fa_titles(const uint8_t *raw, const gs_fa_title *t, const uint64_t *dst_off, uint64_t n, uint8_t *dst) {
  for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint64_t off = t[r].off, len = t[r].end - off, to = dst_off[r];
    for (uint64_t i = threadIdx.x; i < len; i += 64u) dst[to + i] = raw[off + i];
  }
}

/* the table and the title lines -> the arrays of gs_fasta_records; a name twice under the record rules: GS_ERR_FORMAT */
gs_status fa_finish(gs_fasta *fa, const std::vector<gs_fa_title> &t, const std::vector<uint64_t> &line_off, const std::string &lines) {
  const uint64_t n = t.size();
  fa->title_off.resize(n), fa->title_len.resize(n), fa->text_off.resize(n), fa->rec_len.resize(n), fa->line_len.resize(n);
  fa->name_off.assign(n + 1, 0);
  std::set<std::string> seen;
  for (uint64_t r = 0; r < n; r++) {
    fa->title_off[r] = t[r].off;
    gs_fa_extents(t.data(), n, r, fa->file_len, fa->file_nls, fa->text_len, &fa->title_len[r], &fa->text_off[r], &fa->rec_len[r], &fa->line_len[r]);
    size_t b = 0, l = 0;
    const char *line = lines.data() + line_off[r];
    if (fa->rules == GS_FA_RULES_INDEX)
      fasta_names::index_name(line, (size_t)fa->title_len[r], &b, &l);
    else
      fasta_names::record_name(line, (size_t)fa->title_len[r], &b, &l);
    fa->names.append(line + b, l);
    fa->name_off[r + 1] = fa->names.size();
    if (fa->rules == GS_FA_RULES_RECORD && !seen.insert(std::string(line + b, l)).second) {
      gs_set_error("FASTA record '" + std::string(line + b, l) + "' occurs twice");
      return GS_ERR_FORMAT;
    }
  }
  return GS_OK;
}

gs_status fa_run(gs_fasta *fa, const uint8_t *d_raw, uint64_t len, hipStream_t st) {
  auto t0 = std::chrono::steady_clock::now();
  fa->file_len = len;
  const uint64_t nt = (len + FA_TILE - 1) / FA_TILE;
  std::vector<gs_fa_title> titles;
  std::vector<uint64_t> line_off(1, 0);
  std::string lines;
  if (nt) {
    gs_scratch mem;
    size_t tb_f = 0, tb_r = 0, tb_c = 0;
    GS_HIP(rocprim::inclusive_scan(nullptr, tb_f, (gs_fa_sum *)nullptr, (gs_fa_sum *)nullptr, (size_t)nt + 1, fa_fwd(), st));
    GS_HIP(rocprim::inclusive_scan(nullptr, tb_r, (gs_fa_sum *)nullptr, (gs_fa_sum *)nullptr, (size_t)nt + 1, fa_rev(), st));
    GS_HIP(rocprim::exclusive_scan(nullptr, tb_c, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)nt + 1, fa_add(), st));
    const size_t sb = sizeof(gs_fa_sum) * ((size_t)nt + 1), cb = 8 * ((size_t)nt + 1);
    void *sums, *rsums, *fwd, *bwd, *counts, *koff, *tmp;
    GS_TRY(mem.get(sb, &sums));
    GS_TRY(mem.get(sb, &rsums));
    GS_TRY(mem.get(sb, &fwd));
    GS_TRY(mem.get(sb, &bwd));
    GS_TRY(mem.get(cb, &counts));
    GS_TRY(mem.get(cb, &koff));
    const size_t tb = std::max(tb_f, std::max(tb_r, tb_c));
    GS_TRY(mem.get(tb, &tmp));
    fa_args a;
    memset(&a, 0, sizeof a);
    a.raw = d_raw;
    a.len = len;
    a.n_tiles = nt;
    a.rules = fa->rules;
    a.sums = (gs_fa_sum *)sums;
    a.rsums = (gs_fa_sum *)rsums;
    a.fwd = (const gs_fa_sum *)fwd;
    a.bwd = (const gs_fa_sum *)bwd;
    a.counts = (unsigned long long *)counts;
    a.koff = (const unsigned long long *)koff;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nt, (uint64_t)gs_num_cus(fa->device) * 64u);
    const gs_fa_sum first = gs_fa_file_start(), none = gs_fa_identity();
    GS_HIP(hipMemcpyAsync(sums, &first, sizeof first, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(rsums, &none, sizeof none, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st)); /* the two sources are on this frame */
    /* the passes are timed by events in the stream: nothing waits between them */
    gs_events<7> ev;
    for (hipEvent_t &e : ev.e) GS_HIP(hipEventCreate(&e));
    GS_HIP(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(k_fa_tile<FA_SUM>, dim3(grid), dim3(FA_THREADS), 0, st, a);
    GS_HIP(hipEventRecord(ev.e[1], st));
    GS_TRY(gs_prim_carved("FASTA reader: forward scan of the tiles", tmp, tb, [&](void *t, size_t &b) {
      return rocprim::inclusive_scan(t, b, a.sums, (gs_fa_sum *)fwd, (size_t)nt + 1, fa_fwd(), st);
    }));
    GS_TRY(gs_prim_carved("FASTA reader: backward scan of the tiles", tmp, tb, [&](void *t, size_t &b) {
      return rocprim::inclusive_scan(t, b, a.rsums, (gs_fa_sum *)bwd, (size_t)nt + 1, fa_rev(), st);
    }));
    GS_HIP(hipEventRecord(ev.e[2], st));
    GS_HIP(hipMemsetAsync((unsigned long long *)counts + nt, 0, 8, st));
    hipLaunchKernelGGL(k_fa_tile<FA_COUNT>, dim3(grid), dim3(FA_THREADS), 0, st, a);
    GS_HIP(hipEventRecord(ev.e[3], st));
    GS_TRY(gs_prim_carved("FASTA reader: scan of the kept bytes", tmp, tb, [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, a.counts, (unsigned long long *)koff, 0ull, (size_t)nt + 1, fa_add(), st);
    }));
    GS_HIP(hipEventRecord(ev.e[4], st));
    gs_fa_sum whole;
    unsigned long long kept = 0;
    GS_HIP(hipMemcpyAsync(&whole, (const gs_fa_sum *)fwd + nt, sizeof whole, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(&kept, (const unsigned long long *)koff + nt, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    fa->text_len = kept;
    fa->file_nls = whole.n_nl;
    const uint64_t n = whole.n_titles;
    void *text, *tab;
    GS_TRY(mem.get(kept, &text));
    GS_TRY(mem.get(sizeof(gs_fa_title) * n, &tab));
    a.text = (uint8_t *)text;
    a.titles = (gs_fa_title *)tab;
    if (n) hipLaunchKernelGGL(k_fa_title_fill, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, a.titles, n, len);
    GS_HIP(hipEventRecord(ev.e[5], st)); /* behind the two allocations and the fill: the emit pass alone */
    hipLaunchKernelGGL(k_fa_tile<FA_EMIT>, dim3(grid), dim3(FA_THREADS), 0, st, a);
    GS_HIP(hipEventRecord(ev.e[6], st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    static const int from[5] = {0, 1, 2, 3, 5};
    GS_TRY(ev.elapsed(from, 5, fa->ms + 4));
    fa->ms[2] = gs_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (n) {
      titles.resize(n);
      GS_HIP(hipMemcpy(titles.data(), tab, sizeof(gs_fa_title) * n, hipMemcpyDeviceToHost));
      line_off.resize(n + 1);
      for (uint64_t r = 0; r < n; r++) line_off[r + 1] = line_off[r] + (titles[r].end - titles[r].off);
      void *d_off, *d_lines;
      GS_TRY(mem.get(8 * (n + 1), &d_off));
      GS_TRY(mem.get(line_off[n], &d_lines));
      GS_HIP(hipMemcpy(d_off, line_off.data(), 8 * (n + 1), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_fa_titles, dim3((uint32_t)std::min<uint64_t>(n, 65536)), dim3(64), 0, st, d_raw, (const gs_fa_title *)tab,
                         (const uint64_t *)d_off, n, (uint8_t *)d_lines);
      GS_HIP(hipStreamSynchronize(st));
      GS_HIP(hipGetLastError());
      lines.resize(line_off[n]);
      if (line_off[n]) GS_HIP(hipMemcpy(&lines[0], d_lines, line_off[n], hipMemcpyDeviceToHost));
    }
    mem.keep(text);
    fa->d_text = text;
  }
  const gs_status rc = fa_finish(fa, titles, line_off, lines);
  fa->ms[3] = nt ? gs_ms_since(t0) : 0;
  return rc;
}

gs_status fa_parse_device(int device, const void *d_raw, uint64_t len, uint32_t rules, hipStream_t st, gs_fasta *fa) {
  fa->device = device;
  fa->rules = rules;
  return fa_run(fa, (const uint8_t *)d_raw, len, st);
}

std::atomic<uint64_t> g_chunk_bytes{(uint64_t)32 << 20};

}  // namespace

extern "C" void gs_fasta_free(gs_fasta *fa) {
  if (!fa) return;
  if (fa->d_text) {
    (void)hipSetDevice(fa->device);
    (void)hipFree(fa->d_text);
  }
  free(fa->h_text);
  delete fa;
}

extern "C" gs_status gs_fasta_parse_device(int device, const void *d_raw, uint64_t len, uint32_t rules, void *stream, gs_fasta **out) {
  if (!out || (len && !d_raw) || rules > GS_FASTA_RECORD_RULES) return GS_ERR_ARG;
  *out = nullptr;
  gs_fasta *fa = nullptr;
  try {
    GS_HIP(hipSetDevice(device));
    fa = new gs_fasta();
    const gs_status rc = fa_parse_device(device, d_raw, len, rules, (hipStream_t)stream, fa);
    if (rc != GS_OK) {
      gs_fasta_free(fa);
      return rc;
    }
    *out = fa;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    gs_fasta_free(fa);
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_fasta_parse(int device, const uint8_t *raw, uint64_t len, uint32_t rules, gs_fasta **out) {
  if (!out || (len && !raw) || rules > GS_FASTA_RECORD_RULES) return GS_ERR_ARG;
  *out = nullptr;
  GS_HIP(hipSetDevice(device));
  gs_scratch mem;
  void *d_raw = nullptr;
  GS_TRY(mem.get(len, &d_raw));
  const auto t0 = std::chrono::steady_clock::now();
  if (len) GS_HIP(hipMemcpy(d_raw, raw, len, hipMemcpyHostToDevice));
  const double up = gs_ms_since(t0);
  const gs_status rc = gs_fasta_parse_device(device, d_raw, len, rules, nullptr, out);
  if (rc == GS_OK) (*out)->ms[1] = up;
  return rc;
}

extern "C" uint64_t gs_debug_fasta_chunk_bytes(uint64_t set) {
  if (set) g_chunk_bytes.store(set);
  return g_chunk_bytes.load();
}

extern "C" gs_status gs_fasta_parse_file(int device, const char *path, uint32_t rules, gs_fasta **out) {
  if (!out || !path || rules > GS_FASTA_RECORD_RULES) return GS_ERR_ARG;
  *out = nullptr;
  gs_staged_file f;
  GS_TRY(f.open(device, path, g_chunk_bytes.load()));
  GS_TRY(gs_fasta_parse_device(device, f.d_raw, f.size, rules, f.st, out));
  (*out)->ms[0] = f.ms_read;
  (*out)->ms[1] = f.ms_wait;
  return GS_OK;
}

extern "C" gs_status gs_fasta_info(const gs_fasta *fa, uint64_t *n_records, uint64_t *text_len, uint64_t *names_bytes) {
  if (!fa) return GS_ERR_ARG;
  if (n_records) *n_records = fa->title_off.size();
  if (text_len) *text_len = fa->text_len;
  if (names_bytes) *names_bytes = fa->names.size();
  return GS_OK;
}

extern "C" gs_status gs_fasta_records(const gs_fasta *fa, uint64_t *title_off, uint64_t *title_len, uint64_t *text_off, uint64_t *text_len,
                                      uint64_t *line_len, uint64_t *name_off, char *names) {
  if (!fa) return GS_ERR_ARG;
  const size_t n = fa->title_off.size();
  if (title_off && n) memcpy(title_off, fa->title_off.data(), 8 * n);
  if (title_len && n) memcpy(title_len, fa->title_len.data(), 8 * n);
  if (text_off && n) memcpy(text_off, fa->text_off.data(), 8 * n);
  if (text_len && n) memcpy(text_len, fa->rec_len.data(), 8 * n);
  if (line_len && n) memcpy(line_len, fa->line_len.data(), 8 * n);
  if (name_off) memcpy(name_off, fa->name_off.data(), 8 * (n + 1));
  if (names && !fa->names.empty()) memcpy(names, fa->names.data(), fa->names.size());
  return GS_OK;
}

extern "C" gs_status gs_fasta_text(const gs_fasta *cfa, int on_device, const void **text) {
  gs_fasta *fa = const_cast<gs_fasta *>(cfa);
  if (!fa || !text) return GS_ERR_ARG;
  *text = nullptr;
  if (on_device) {
    if (fa->device < 0) return GS_ERR_ARG;
    *text = fa->d_text;
    return GS_OK;
  }
  std::lock_guard<std::mutex> lk(fa->mtx);
  if (!fa->h_text) {
    if (fa->device < 0) return GS_ERR_ARG; /* a host-made object always has its text */
    GS_HIP(hipSetDevice(fa->device));
    const gs_status rc = gs_text_to_host(fa->d_text, fa->text_len, &fa->h_text);
    if (rc != GS_OK) return rc;
  }
  *text = fa->h_text;
  return GS_OK;
}

extern "C" gs_status gs_debug_fasta_ms(const gs_fasta *fa, double *ms) {
  if (!fa || !ms) return GS_ERR_ARG;
  for (int i = 0; i < 9; i++) ms[i] = fa->ms[i];
  return GS_OK;
}

extern "C" uint64_t gs_debug_fasta_tile_bytes(void) { return FA_TILE; }

namespace {
struct fa_host_emitter {
  uint8_t *text;
  gs_fa_title *titles;
  void keep(uint64_t at, uint8_t b) { text[at] = b; }
  void title(uint64_t i, uint64_t off, uint64_t nls, uint64_t kept) {
    titles[i].off = off;
    titles[i].nls = nls;
    titles[i].kept = kept;
  }
  void title_end(uint64_t i, uint64_t end) { titles[i].end = end; }
};
}  // namespace

extern "C" gs_status gs_debug_fasta_host(const uint8_t *raw, uint64_t len, uint32_t rules, uint64_t tile_bytes, gs_fasta **out) {
  if (!out || (len && !raw) || rules > GS_FASTA_RECORD_RULES || tile_bytes == 0) return GS_ERR_ARG;
  *out = nullptr;
  gs_fasta *fa = nullptr;
  try {
    fa = new gs_fasta();
    fa->rules = rules;
    fa->file_len = len;
    const uint64_t nt = (len + tile_bytes - 1) / tile_bytes;
    auto tile_len = [&](uint64_t k) { return std::min<uint64_t>(tile_bytes, len - k * tile_bytes); };
    /* the passes of fa_run, one after the other */
    std::vector<gs_fa_sum> sums(nt), fwd(nt + 1), bwd(nt + 1);
    for (uint64_t k = 0; k < nt; k++) sums[k] = gs_fa_summarize(raw + k * tile_bytes, tile_len(k));
    fwd[0] = gs_fa_file_start();
    for (uint64_t k = 0; k < nt; k++) fwd[k + 1] = gs_fa_compose(fwd[k], sums[k]);
    bwd[nt] = gs_fa_identity(); /* bwd[k]: tiles k .. */
    for (uint64_t k = nt; k-- > 0;) bwd[k] = gs_fa_compose(sums[k], bwd[k + 1]);
    std::vector<uint64_t> koff(nt + 1, 0);
    gs_fa_count_only none;
    for (uint64_t k = 0; k < nt; k++)
      koff[k + 1] = koff[k] + gs_fa_walk(raw + k * tile_bytes, tile_len(k), k * tile_bytes, rules, gs_fa_edge_of(fwd[k], bwd[k + 1], 0), none);
    fa->text_len = koff[nt];
    fa->file_nls = fwd[nt].n_nl;
    fa->h_text = (char *)malloc(fa->text_len + 1);
    if (!fa->h_text) throw std::bad_alloc();
    fa->h_text[fa->text_len] = 0;
    std::vector<gs_fa_title> titles(fwd[nt].n_titles);
    for (gs_fa_title &t : titles) t.end = len;
    fa_host_emitter em{(uint8_t *)fa->h_text, titles.data()};
    for (uint64_t k = 0; k < nt; k++)
      gs_fa_walk(raw + k * tile_bytes, tile_len(k), k * tile_bytes, rules, gs_fa_edge_of(fwd[k], bwd[k + 1], koff[k]), em);
    std::vector<uint64_t> line_off(titles.size() + 1, 0);
    std::string lines;
    for (size_t r = 0; r < titles.size(); r++) {
      lines.append((const char *)raw + titles[r].off, titles[r].end - titles[r].off);
      line_off[r + 1] = lines.size();
    }
    const gs_status rc = fa_finish(fa, titles, line_off, lines);
    if (rc != GS_OK) {
      gs_fasta_free(fa);
      return rc;
    }
    *out = fa;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    gs_fasta_free(fa);
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_decoder_open_fasta(int device, const gs_fasta *fa, const gs_genome_structure *sq, gs_decoder **out) {
  if (!out || !fa || !sq || fa->rules != GS_FASTA_RECORD_RULES || fa->device != device || (sq->n_chr && (!sq->chr_names || !sq->chr_lengths)))
    return GS_ERR_ARG;
  *out = nullptr;
  try {
    std::map<std::string, uint64_t> where;
    for (uint64_t r = 0; r < fa->title_off.size(); r++)
      where.emplace(std::string(fa->names.data() + fa->name_off[r], fa->name_off[r + 1] - fa->name_off[r]), r);
    std::vector<uint64_t> off(sq->n_chr, 0), len(sq->n_chr, ~0ull); /* no record of that name: UINT64_MAX, as the host path */
    for (uint32_t c = 0; c < sq->n_chr; c++) {
      if (!sq->chr_names[c]) return GS_ERR_ARG;
      const auto it = where.find(sq->chr_names[c]);
      if (it == where.end()) continue;
      off[c] = fa->text_off[it->second];
      len[c] = fa->rec_len[it->second];
    }
    return gs_decoder_open_text(device, (const uint8_t *)fa->d_text, fa->text_len, 1, sq, off.data(), len.data(), out);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}
