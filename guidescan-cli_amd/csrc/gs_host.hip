/*
 * gs_host.hip -- host-side half of the C-ABI: the host-pointer enumerate wrapper, hit
 * decoding, CFD, status strings.  No kernels here.
 */
#include "gs_common.h"
#include "gs_scratch.h"
#include "cfd_table.h"

#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

static thread_local std::string g_last_error;
void gs_set_error(const std::string &s) { g_last_error = s; }

/* ---- switches of a handle (gs_index::opts) ---- */
extern char **environ;
std::atomic<int> gs_debug_any{0};
const char *gs_opt(const gs_index *ix, const char *key) {
  if (!ix) return nullptr;
  const auto it = ix->opts.find(key);
  return it == ix->opts.end() ? nullptr : it->second.c_str();
}
/* GS_DBG_NOMEM=<n> arms a counter on the handle: the next n passes of a batch fail (enumerate_device_impl counts it down) */
static void arm_dbg_nomem(gs_index *ix) {
  const char *e = gs_opt(ix, "GS_DBG_NOMEM");
  ix->dbg_nomem = e ? (uint32_t)std::max(0l, atol(e)) : 0u;
}
void gs_opts_from_env(gs_index *ix) {
  /* the one place that looks at the environment: when a handle is made */
  for (char **e = environ; e && *e; ++e) {
    if (strncmp(*e, "GS_", 3) != 0) continue;
    const char *eq = strchr(*e, '=');
    if (!eq) continue;
    ix->opts[std::string(*e, (size_t)(eq - *e))] = std::string(eq + 1);
  }
  if (ix->opts.count("GS_DEBUG")) gs_debug_any.store(1);
  arm_dbg_nomem(ix);
}
extern "C" gs_status gs_index_set_option(gs_index *ix, const char *key, const char *value) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !key || strncmp(key, "GS_", 3) != 0) return GS_ERR_ARG;
  try {
    if (value)
      ix->opts[key] = value;
    else
      ix->opts.erase(key);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  if (value && strcmp(key, "GS_DEBUG") == 0) gs_debug_any.store(1);
  if (strcmp(key, "GS_DBG_NOMEM") == 0) arm_dbg_nomem(ix);
  return GS_OK;
}
extern "C" gs_status gs_index_get_option(const gs_index *ix, const char *key, char *out, uint64_t cap) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !key || !out || cap == 0) return GS_ERR_ARG;
  const char *v = gs_opt(ix, key);
  if (!v) {
    out[0] = 0;
    return GS_ERR_ARG; /* not set */
  }
  const size_t n = strlen(v);
  if (n + 1 > cap) return GS_ERR_ARG;
  memcpy(out, v, n + 1);
  return GS_OK;
}
extern "C" gs_status gs_index_last_sharing(const gs_index *ix, uint64_t out[8]) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !out) return GS_ERR_ARG;
  for (int i = 0; i < 8; i++) out[i] = ix->last_share[i];
  return GS_OK;
}

extern "C" const char *gs_status_string(gs_status s) {
  switch (s) {
    case GS_OK: return "ok";
    case GS_ERR_ARG: return "bad argument";
    case GS_ERR_DEVICE: return g_last_error.empty() ? "device error" : g_last_error.c_str();
    case GS_ERR_UNSUPPORTED:
      return g_last_error.empty() ? "unsupported input" : g_last_error.c_str();
    case GS_ERR_NOMEM: return "out of memory";
    case GS_ERR_IO: return g_last_error.empty() ? "i/o error" : g_last_error.c_str();
    case GS_ERR_FORMAT: return g_last_error.empty() ? "malformed index file" : g_last_error.c_str();
  }
  return "unknown";
}
extern "C" const char *gs_version(void) { return "guidescan-amd 0.3 (gfx950)"; }

/* Page-locked host buffers for the results of the host-pointer entry point, kept in a small
 * process-wide pool: a 1 M-guide batch returns ~215 MB of hits, and a fresh pageable buffer costs
 * more (page faults, staged copy) than the copy itself.  Portable: any device may fill them. */
struct gs_pinned {
  void *p = nullptr;
  size_t cap = 0;
};
static std::mutex g_pin_mtx;
static std::vector<gs_pinned> g_pin_free;
static gs_pinned pin_acquire(size_t bytes) {
  if (!bytes) bytes = 16;
  {
    std::lock_guard<std::mutex> lk(g_pin_mtx);
    int best = -1;
    for (size_t i = 0; i < g_pin_free.size(); i++)
      if (g_pin_free[i].cap >= bytes && (best < 0 || g_pin_free[i].cap < g_pin_free[best].cap)) best = (int)i;
    if (best >= 0) {
      gs_pinned b = g_pin_free[best];
      g_pin_free.erase(g_pin_free.begin() + best);
      return b;
    }
  }
  gs_pinned b;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipHostMalloc(&b.p, want, hipHostMallocPortable) == hipSuccess) {
    b.cap = want;
  } else {
    (void)hipGetLastError();
    b.p = nullptr;
    if (hipHostMalloc(&b.p, bytes, hipHostMallocPortable) == hipSuccess) b.cap = bytes;
    else (void)hipGetLastError();
  }
  return b;
}
static void pin_release(gs_pinned b) {
  if (!b.p) return;
  std::lock_guard<std::mutex> lk(g_pin_mtx);
  g_pin_free.push_back(b);
  while (g_pin_free.size() > 8) { /* keep the pool small: drop the smallest buffer */
    size_t k = 0;
    for (size_t i = 1; i < g_pin_free.size(); i++)
      if (g_pin_free[i].cap < g_pin_free[k].cap) k = i;
    hipHostFree(g_pin_free[k].p);
    g_pin_free.erase(g_pin_free.begin() + k);
  }
}

struct gs_result {
  gs_pinned offsets, hits, flags, raw;
  gs_result_view view{};
  ~gs_result() {
    pin_release(offsets);
    pin_release(hits);
    pin_release(flags);
    pin_release(raw);
  }
};

static gs_status enumerate_host(gs_index *ix, const char *guides, uint64_t n, uint32_t L, const char *guide_pams,
                                uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                gs_result **out) {
  if (!ix || !out || (n && !guides) || (n && P && !guide_pams)) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(ix->device));
  gs_status rc = gs_reserve(ix->w_batch.guides, n * (size_t)(L + P) + 16);
  if (rc != GS_OK) return rc;
  char *d_g = (char *)ix->w_batch.guides.p;
  char *d_p = d_g + n * (size_t)L;
  if (n) {
    GS_HIP(hipMemcpy(d_g, guides, n * (size_t)L, hipMemcpyHostToDevice));
    if (P) GS_HIP(hipMemcpy(d_p, guide_pams, n * (size_t)P, hipMemcpyHostToDevice));
  }
  const void *d_off = nullptr, *d_hits = nullptr;
  gs_result *r = new gs_result();
  struct guard_t {
    gs_result *p;
    ~guard_t() { delete p; }
  } guard{r};
  rc = gs_enumerate_device(ix, d_g, n, L, d_p, P, alt_pams, n_alt, mismatches, flags, nullptr, &d_off,
                           &d_hits, &r->view);
  if (rc != GS_OK) return rc;
  r->offsets = pin_acquire(8 * (n + 1));
  r->hits = pin_acquire(sizeof(gs_hit) * r->view.n_hits);
  if (!r->offsets.p || !r->hits.p) return GS_ERR_NOMEM;
  GS_HIP(hipMemcpy(r->offsets.p, d_off, 8 * (n + 1), hipMemcpyDeviceToHost));
  if (r->view.n_hits)
    GS_HIP(hipMemcpy(r->hits.p, d_hits, sizeof(gs_hit) * r->view.n_hits, hipMemcpyDeviceToHost));
  r->view.n_guides = n;
  r->view.guide_offsets = (const uint64_t *)r->offsets.p;
  r->view.hits = (const gs_hit *)r->hits.p;
  r->view.n_unsupported = ix->last_unsupported;
  r->view.guide_flags = nullptr;
  if (ix->last_unsupported) {
    r->flags = pin_acquire(n);
    if (!r->flags.p) return GS_ERR_NOMEM;
    GS_HIP(hipMemcpy(r->flags.p, ix->w_batch.flags.p, n, hipMemcpyDeviceToHost));
    r->view.guide_flags = (const uint8_t *)r->flags.p;
  }
  r->view.raw_hits = nullptr;
  if ((flags & GS_FLAG_RAW_COUNTS) && ix->last_raw_valid && n) {
    r->raw = pin_acquire(4 * n);
    if (!r->raw.p) return GS_ERR_NOMEM;
    GS_HIP(hipMemcpy(r->raw.p, ix->w_batch.raw.p, 4 * n, hipMemcpyDeviceToHost));
    r->view.raw_hits = (const uint32_t *)r->raw.p;
  }
  guard.p = nullptr;
  *out = r;
  return GS_OK;
}
extern "C" gs_status gs_enumerate(gs_index *ix, const char *guides, uint64_t n, uint32_t L,
                                  const char *guide_pams, uint32_t P, const char *alt_pams,
                                  uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                  gs_result **out) {
  GS_HANDLE_LOCK(ix);
  try { /* nothing may throw across the C boundary */
    return enumerate_host(ix, guides, n, L, guide_pams, P, alt_pams, n_alt, mismatches, flags, out);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

/* a text in HBM -> a malloc'ed, NUL-terminated copy: two page-locked staging buffers, the copy out of one overlapping
 * the transfer into the other */
gs_status gs_text_to_host(const void *d_text, uint64_t tl, char **text) {
  char *out = (char *)malloc(tl + 1);
  if (!out) return GS_ERR_NOMEM;
  const size_t CH = (size_t)32 << 20;
  gs_pinned pin[2] = {pin_acquire(std::min<size_t>(CH, tl)), tl > CH ? pin_acquire(std::min<size_t>(CH, tl - CH)) : gs_pinned()};
  hipError_t e = hipSuccess;
  if (tl && (!pin[0].p || (tl > CH && !pin[1].p))) { /* no page-locked memory: the runtime stages the copy */
    e = hipMemcpy(out, d_text, tl, hipMemcpyDeviceToHost);
  } else if (tl) {
    const size_t nch = (tl + CH - 1) / CH;
    auto bytes = [&](size_t c) { return std::min<size_t>(CH, tl - c * CH); };
    e = hipMemcpyAsync(pin[0].p, d_text, bytes(0), hipMemcpyDeviceToHost, nullptr);
    for (size_t c = 0; c < nch && e == hipSuccess; c++) {
      e = hipStreamSynchronize(nullptr);
      if (e == hipSuccess && c + 1 < nch)
        e = hipMemcpyAsync(pin[(c + 1) & 1].p, (const char *)d_text + (c + 1) * CH, bytes(c + 1), hipMemcpyDeviceToHost, nullptr);
      if (e == hipSuccess) memcpy(out + c * CH, pin[c & 1].p, bytes(c));
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(nullptr);
  }
  pin_release(pin[0]);
  pin_release(pin[1]);
  if (e != hipSuccess) {
    free(out);
    gs_set_error(std::string("copy of the text: ") + hipGetErrorString(e));
    return GS_ERR_DEVICE;
  }
  out[tl] = 0;
  *text = out;
  return GS_OK;
}

/* ---- gs_scratch.h ---- */
double gs_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

gs_scratch::~gs_scratch() {
  for (void *q : p) (void)hipFree(q);
}
gs_status gs_scratch::get(size_t bytes, void **out) {
  *out = nullptr;
  p.reserve(p.size() + 1);
  const hipError_t e = hipMalloc(out, bytes + 16);
  if (e != hipSuccess) {
    *out = nullptr;
    if (e != hipErrorOutOfMemory) {
      gs_set_error(std::string("hipMalloc(out, bytes + 16): ") + hipGetErrorString(e));
      return GS_ERR_DEVICE;
    }
    (void)hipGetLastError();
    gs_set_error("out of device memory");
    return GS_ERR_NOMEM;
  }
  p.push_back(*out);
  return GS_OK;
}
void gs_scratch::keep(const void *q) { p.erase(std::remove(p.begin(), p.end(), q), p.end()); }

/* ---- gs_common.h: gs_resident ---- */
void gs_resident::adopt(gs_scratch &from, const void *q, uint64_t bytes) {
  if (!q) return;
  v.push_back({q, bytes}); /* (before keep: a push_back that throws leaves the array with the scratch) */
  from.keep(q);
}
uint64_t gs_resident::drop(const void *q) {
  const auto it = std::find_if(v.begin(), v.end(), [&](const item &i) { return i.p == q; });
  if (it == v.end()) return 0;
  const uint64_t b = it->bytes;
  (void)hipFree((void *)q);
  v.erase(it);
  return b;
}
uint64_t gs_resident::bytes_of(const void *q) const {
  for (const item &i : v)
    if (i.p == q) return i.bytes;
  return 0;
}
void gs_resident::clear() {
  for (const item &i : v) (void)hipFree((void *)i.p);
  v.clear();
}
uint64_t gs_resident::bytes() const {
  uint64_t b = 0;
  for (const item &i : v) b += i.bytes;
  return b;
}

gs_status gs_events_elapsed(const hipEvent_t *e, const int *from, int n, double *out) {
  for (int i = 0; i < n; i++) {
    float ms = 0;
    GS_HIP(hipEventElapsedTime(&ms, e[from[i]], e[from[i] + 1]));
    out[i] = ms;
  }
  return GS_OK;
}

gs_staged_file::~gs_staged_file() {
  if (st) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
}
gs_status gs_staged_file::open(int device, const char *path, uint64_t chunk) {
  FILE *f = fopen(path, "rb");
  struct stat sb;
  if (!f || fstat(fileno(f), &sb) != 0 || !S_ISREG(sb.st_mode)) {
    if (f) fclose(f);
    gs_set_error(std::string("cannot read ") + path);
    return GS_ERR_IO;
  }
  size = (uint64_t)sb.st_size;
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint64_t at = 0;
  auto body = [&]() -> gs_status {
    GS_HIP(hipSetDevice(device));
    GS_TRY(mem.get(size, &d_raw));
    GS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
      if (hipHostMalloc(&pin[i], (size_t)std::min<uint64_t>(chunk, size ? size : 1), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        pin[i] = nullptr;
        gs_set_error("out of page-locked host memory");
        return GS_ERR_NOMEM;
      }
      GS_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    for (uint64_t c = 0; at < size; c++) {
      const int b = (int)(c & 1);
      auto t0 = std::chrono::steady_clock::now();
      if (c >= 2) GS_HIP(hipEventSynchronize(ev[b]));
      ms_wait += gs_ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      const size_t want = (size_t)std::min<uint64_t>(chunk, size - at), got = fread(pin[b], 1, want, f);
      ms_read += gs_ms_since(t0);
      if (got != want) {
        gs_set_error(std::string("cannot read ") + path);
        return GS_ERR_IO;
      }
      GS_HIP(hipMemcpyAsync((uint8_t *)d_raw + at, pin[b], got, hipMemcpyHostToDevice, st));
      GS_HIP(hipEventRecord(ev[b], st));
      at += got;
    }
    const auto t0 = std::chrono::steady_clock::now();
    GS_HIP(hipStreamSynchronize(st));
    ms_wait += gs_ms_since(t0);
    return GS_OK;
  };
  gs_status rc;
  try {
    rc = body();
  } catch (const std::bad_alloc &) {
    rc = GS_ERR_NOMEM;
  }
  fclose(f);
  if (st) (void)hipStreamSynchronize(st); /* a copy may still read a chunk when the loop ended early */
  for (int i = 0; i < 2; i++) {
    if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (pin[i]) (void)hipHostFree(pin[i]);
  }
  return rc;
}

/* search -> score -> encode on the device (gs_textdev.hip), then the text back to the host.  The guides come from the
 * host (guides / guide_pams, uploaded here) or are in HBM already (d_guides / d_guide_pams); ids, id_offsets and senses
 * are host arrays in the first case and device arrays in the second. */
static gs_status enumerate_text(gs_index *ix, bool on_device, const void *guides, uint64_t n, uint32_t L, const void *guide_pams,
                                uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                int64_t max_off_targets, const gs_genome_structure *gs, const void *ids, const void *id_offsets,
                                const void *senses, const uint8_t *skip, char **text, uint64_t *len, gs_result_view *stats,
                                uint32_t *raw_hits) {
  GS_HIP(hipSetDevice(ix->device));
  gs_status rc;
  GS_TRY(gs_reserve(ix->w_text.spec, 4 * n + 16));
  const char *d_g = (const char *)guides, *d_p = (const char *)guide_pams;
  if (!on_device) {
    GS_TRY(gs_reserve(ix->w_batch.guides, n * (size_t)(L + P) + 16));
    char *up = (char *)ix->w_batch.guides.p;
    if (n) {
      GS_HIP(hipMemcpy(up, guides, n * (size_t)L, hipMemcpyHostToDevice));
      if (P) GS_HIP(hipMemcpy(up + n * (size_t)L, guide_pams, n * (size_t)P, hipMemcpyHostToDevice));
    }
    d_g = up;
    d_p = up + n * (size_t)L;
  }
  const void *d_off = nullptr, *d_hits = nullptr, *d_text = nullptr;
  gs_result_view v;
  memset(&v, 0, sizeof v);
  const uint32_t text_bits = GS_TEXT_SAM | GS_TEXT_COMPLETE | GS_TEXT_BAM | GS_TEXT_BGZF | GS_TEXT_FEATURES;
  const uint32_t tflags = flags & text_bits, sflags = flags & ~text_bits;
  if ((tflags & GS_TEXT_BAM) && (tflags & GS_TEXT_SAM)) return GS_ERR_ARG;
  if ((tflags & GS_TEXT_FEATURES) && ((tflags & (GS_TEXT_SAM | GS_TEXT_BAM)) || !ix->annot)) { /* before the search */
    gs_set_error("GS_TEXT_FEATURES goes with CSV text and an annotation attached to the handle (gs_index_set_annotation)");
    return GS_ERR_ARG;
  }
  if ((tflags & GS_TEXT_BGZF) && !(tflags & GS_TEXT_BAM)) return GS_ERR_ARG;
  /* BAM records carry the SAM line's specificity */
  const uint32_t score_flags = ((tflags & (GS_TEXT_SAM | GS_TEXT_BAM)) ? GS_TEXT_SAM : 0u) | (sflags & GS_FLAG_PAM_AT_START);
  rc = gs_enumerate_device(ix, d_g, n, L, d_p, P, alt_pams, n_alt, mismatches, sflags, nullptr, &d_off, &d_hits, &v);
  if (rc != GS_OK) return rc;
  if (stats) *stats = v;
  if (ix->last_unsupported) {
    gs_set_error("a guide of the batch needs the general path");
    return GS_ERR_UNSUPPORTED;
  }
  if (raw_hits) { /* the counting pass of --threshold: the counts, no text */
    if (n && !ix->last_raw_valid) {
      gs_set_error("the search kept no raw counts");
      return GS_ERR_UNSUPPORTED;
    }
    if (n) GS_HIP(hipMemcpy(raw_hits, ix->w_batch.raw.p, 4 * n, hipMemcpyDeviceToHost));
    return GS_OK;
  }
  uint64_t tl = 0;
  if (n) {
    rc = gs_score_device(ix, d_g, n, L, P, score_flags, max_off_targets, gs, d_off, d_hits, nullptr,
                         nullptr, ix->w_text.spec.p);
    if (rc != GS_OK) return rc;
    const uint32_t fflags = tflags | (sflags & GS_FLAG_PAM_AT_START);
    if (on_device)
      rc = gs_format_device_ids(ix, gs, d_g, n, L, d_p, P, ids, id_offsets, senses, skip, d_off, d_hits, ix->w_text.spec.p,
                                mismatches, fflags, max_off_targets, nullptr, &d_text, &tl);
    else
      rc = gs_format_device(ix, gs, d_g, n, L, d_p, P, (const char *)ids, (const uint64_t *)id_offsets, (const uint8_t *)senses,
                            skip, d_off, d_hits, ix->w_text.spec.p, mismatches, fflags, max_off_targets, nullptr, &d_text, &tl);
    if (rc != GS_OK) return rc;
  }
  if ((rc = gs_text_to_host(d_text, tl, text)) != GS_OK) return rc;
  *len = tl;
  return GS_OK;
}
extern "C" gs_status gs_enumerate_text(gs_index *ix, const char *guides, uint64_t n, uint32_t L, const char *guide_pams,
                                       uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                       int64_t max_off_targets, const gs_genome_structure *gs, const char *ids,
                                       const uint64_t *id_offsets, const uint8_t *senses, const uint8_t *skip, char **text,
                                       uint64_t *len, gs_result_view *stats) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !gs || !text || !len) return GS_ERR_ARG;
  if (n && (!guides || !ids || !id_offsets || (P && !guide_pams))) return GS_ERR_ARG;
  if ((n_alt && !alt_pams) || (gs->n_chr && (!gs->chr_names || !gs->chr_lengths))) return GS_ERR_ARG;
  if (n >= (1ull << 31) || max_off_targets < -1 || mismatches > 7 || n_alt > 31) return GS_ERR_ARG;
  if (L < 1 || L > 31 || P > 8 || 2 * L + 3 * P > 59) return GS_ERR_ARG;
  for (uint64_t g = 0; g < n; g++)
    if (id_offsets[g + 1] < id_offsets[g]) return GS_ERR_ARG;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (!gs->chr_names[c]) return GS_ERR_ARG;
  *text = nullptr;
  *len = 0;
  try { /* nothing may throw across the C boundary */
    return enumerate_text(ix, false, guides, n, L, guide_pams, P, alt_pams, n_alt, mismatches, flags, max_off_targets, gs, ids,
                          id_offsets, senses, skip, text, len, stats, nullptr);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}
extern "C" gs_status gs_enumerate_text_device(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L, const void *d_guide_pams,
                                              uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                              int64_t max_off_targets, const gs_genome_structure *gs, const void *d_ids,
                                              const void *d_id_offsets, const void *d_senses, const uint8_t *skip, char **text,
                                              uint64_t *len, gs_result_view *stats, uint32_t *raw_hits) {
  GS_HANDLE_LOCK(ix);
  const bool counting = (flags & GS_FLAG_RAW_COUNTS) != 0;
  if (!ix || !gs) return GS_ERR_ARG;
  if (counting ? !raw_hits : (!text || !len || raw_hits)) return GS_ERR_ARG;
  if (n && (!d_guides || (P && !d_guide_pams))) return GS_ERR_ARG;
  if (n && !counting && (!d_ids || !d_id_offsets)) return GS_ERR_ARG;
  if ((n_alt && !alt_pams) || (gs->n_chr && (!gs->chr_names || !gs->chr_lengths))) return GS_ERR_ARG;
  if (n >= (1ull << 31) || max_off_targets < -1 || mismatches > 7 || n_alt > 31) return GS_ERR_ARG;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (!gs->chr_names[c]) return GS_ERR_ARG;
  if (text) *text = nullptr;
  if (len) *len = 0;
  if (L < 1 || L > 31 || P > 8 || 2 * L + 3 * P > 59) { /* as for a guide that needs the general path: the caller takes the host route for the batch */
    gs_set_error("gs_enumerate_text_device: 2L + 3P > 59 or L, P outside the fast path's key");
    return GS_ERR_UNSUPPORTED;
  }
  try { /* nothing may throw across the C boundary */
    return enumerate_text(ix, true, d_guides, n, L, d_guide_pams, P, alt_pams, n_alt, mismatches, flags, max_off_targets, gs, d_ids,
                          d_id_offsets, d_senses, skip, text, len, stats, raw_hits);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_result_get(const gs_result *r, gs_result_view *view) {
  if (!r || !view) return GS_ERR_ARG;
  *view = r->view;
  return GS_OK;
}
extern "C" void gs_result_free(gs_result *r) { delete r; }

static char comp(char c) {
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    default: return c;
  }
}

extern "C" gs_status gs_decode_sequence(const char *guide, uint32_t L, uint32_t P, uint32_t flags,
                                        uint64_t key, char *out) {
  if (!guide || !out || L < 1 || 2 * L + 3 * P > 59) return GS_ERR_ARG;
  const uint64_t path = (key >> 1) & ((1ull << 59) - 1); /* key bits 59:1, position 0 at the top */
  const bool start = flags & GS_FLAG_PAM_AT_START;
  static const char B[4] = {'A', 'C', 'G', 'T'};
  for (uint32_t t = 0; t < L; t++) {
    /* query char consumed at step t (process.hpp:63, index.hpp:218) */
    const char qc = start ? guide[L - 1 - t] : comp(guide[t]);
    const uint32_t code = (uint32_t)(path >> (57 - 2 * t)) & 3u;
    if (code == 0) {
      out[t] = qc;
    } else {
      /* code-1 = rank among the three bases other than qc, in A<C<G<T order */
      int q = qc == 'A' ? 0 : qc == 'C' ? 1 : qc == 'G' ? 2 : qc == 'T' ? 3 : -1;
      if (q < 0) return GS_ERR_ARG;
      int a = (int)code - 1;
      if (a >= q) a++;
      out[t] = (char)tolower(B[a]); /* index.hpp:243 */
    }
  }
  static const char PB[5] = {'A', 'C', 'G', 'N', 'T'};
  for (uint32_t u = 0; u < P; u++) {
    const uint32_t code = (uint32_t)(path >> (56 - 2 * L - 3 * u)) & 7u;
    if (code > 4) return GS_ERR_ARG;
    out[L + u] = PB[code];
  }
  out[L + P] = 0;
  return GS_OK;
}

static int bidx(char c) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return -1;
  }
}
/* include/genomics/printer.hpp:98-113 with the std::map tables flattened (immutable,
 * so the reference's operator[] data race, SURVEY 5.2, cannot happen here) */
extern "C" float gs_calculate_cfd(const char *sgrna, const char *seq, const char *pam) {
  if (!sgrna || !seq || !pam) return 1.0f;
  if (strlen(sgrna) != 20 || strlen(pam) != 3) return 1.0f;
  float cfd = 1.0f;
  for (int i = 0; i < 20; i++) {
    const char g = sgrna[i], t = seq[i];
    if (g != t) {
      const int r = bidx(g); /* T is looked up as U: same slot */
      const int d = bidx((char)toupper(comp(t)));
      const double sc = (r >= 0 && d >= 0) ? gs_cfd_mm[(r * 4 + d) * 20 + i] : 0.0;
      cfd = (float)((double)cfd * sc);
    }
  }
  const int b1 = bidx(pam[1]), b2 = bidx(pam[2]);
  const double ps = (b1 >= 0 && b2 >= 0) ? gs_cfd_pam[b1 * 4 + b2] : 0.0;
  return (float)((double)cfd * ps);
}

