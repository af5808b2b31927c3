/*
 * gs_annot.hip -- off-targets annotated with the features of a BED file (`--annotate BED`): which groups of intervals the
 * row of every hit touches.  The reference has no counterpart: its pipelines (manual/manual.tex:321-656) join the CSV
 * against a BED file in a script afterwards.  The rule and the table are stated once, in gs_annot_scan.h; DESIGN.md
 * section 5.9 has the passes.
 *
 *   gs_annot_build        host: the merged intervals of a parsed gs_regions -> per chromosome the breakpoints and the CSR
 *                         lists of the groups over every elementary segment, and the name blob; one upload
 *   gs_annotate_device    k_an_count   one lane per hit: resolve, two binary searches over the chromosome's breakpoints,
 *                                      the number of distinct groups over the segments in between; a hit with a feature
 *                                      adds one to its guide's count at its distance              (16 B read, 4 B written)
 *                         (rocPRIM exclusive scan of the counts, widened to 64 bits)
 *                         k_an_emit    the same lookup again, the groups written at the hit's offset
 *                                                                                   (16 + 16 B read, 4 B per feature written)
 *   gs_debug_annotate_host  the same lookup on the host through the shared header, no device
 * Measured (tools/annotate_rate.py): 33.5 M hits against 2 x 10^5 exons under 2 x 10^4 genes in 7.5 ms,
 * about 62 bytes moved per hit - a twentieth of what HBM streams.  The chains of dependent reads bind (two searches of
 * log2(breakpoints) steps, one of log2(guides) for a hit with a feature), not the stream.  Nothing is tuned yet.
 */
#include "gs_device.h"
#include "gs_scratch.h"
#include "gs_resolve.h"
#include "gs_annot_scan.h"
#include "gs_annot_obj.h"
#include "gs_regions_obj.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <memory>

#define AN_BLOCK 256
#define AN_ERR_DISTANCE 1u

static std::atomic<uint64_t> g_an_entry_cap{GS_AN_MAX_ENTRIES};
extern "C" uint64_t gs_debug_annot_entry_cap(uint64_t set) {
  if (set) g_an_entry_cap.store(std::min<uint64_t>(set, GS_AN_MAX_ENTRIES));
  return g_an_entry_cap.load();
}

/* ---- the object --------------------------------------------------------------------------------------------------- */

extern "C" gs_status gs_regions_group_name(const gs_regions *rg, uint64_t g, const char **name) {
  if (!rg || !name || g >= rg->group_names.size()) return GS_ERR_ARG;
  *name = rg->group_names[(size_t)g].c_str();
  return GS_OK;
}

static void an_release(gs_annot *an) {
  if (!an) return;
  if (an->d_blob) {
    hipSetDevice(an->device);
    hipFree(an->d_blob);
  }
  delete an;
}

extern "C" gs_status gs_annot_build(const gs_regions *rg, int device, gs_annot **out) {
  if (!rg || !out) return GS_ERR_ARG;
  *out = nullptr;
  try {
    std::unique_ptr<gs_annot, void (*)(gs_annot *)> own(new gs_annot(), an_release);
    gs_annot *an = own.get();
    for (const std::string &name : rg->group_names)
      if (name.find(';') != std::string::npos) {
        gs_set_error("annotation group '" + name + "': a name with ';' would break the joined match_features column");
        return GS_ERR_FORMAT;
      }
    an->group_names = rg->group_names;
    an->chr_lengths = rg->chr_lengths;
    for (const std::string &name : an->group_names) {
      an->name_off.push_back((uint32_t)an->names.size());
      an->names += name;
    }
    an->name_off.push_back((uint32_t)an->names.size());
    std::vector<std::vector<gs_an_iv>> per_chr(rg->chr.size());
    for (size_t c = 0; c < rg->chr.size(); c++) {
      const gs_rg_chr &t = rg->chr[c];
      for (size_t i = 0; i < t.start.size(); i++) per_chr[c].push_back(gs_an_iv{t.group[i], t.start[i], t.end[i]});
    }
    uint64_t need = 0;
    if (!gs_an_build(std::move(per_chr), g_an_entry_cap.load(), an->h, &need)) {
      gs_set_error("annotation: the segment table would hold " + std::to_string(need) + " entries, more than " +
                   std::to_string(g_an_entry_cap.load()));
      return GS_ERR_ARG;
    }
    if (device >= 0) {
      GS_HIP(hipSetDevice(device));
      an->device = device;
      const gs_an_host &h = an->h;
      const std::vector<uint32_t> *cols[5] = {&h.chr_bp, &h.bp, &h.seg_off, &h.ent, &an->name_off};
      size_t at[6], total = 0;
      for (int i = 0; i < 5; i++) {
        at[i] = total;
        total += (4 * cols[i]->size() + 15) & ~(size_t)15;
      }
      at[5] = total;
      total += an->names.size();
      gs_scratch mem;
      GS_TRY(mem.get(total, &an->d_blob));
      mem.keep(an->d_blob);
      char *d = (char *)an->d_blob;
      for (int i = 0; i < 5; i++)
        if (!cols[i]->empty()) GS_HIP(hipMemcpy(d + at[i], cols[i]->data(), 4 * cols[i]->size(), hipMemcpyHostToDevice));
      if (!an->names.empty()) GS_HIP(hipMemcpy(d + at[5], an->names.data(), an->names.size(), hipMemcpyHostToDevice));
      an->d_table = gs_an_table{(const uint32_t *)(d + at[0]), (const uint32_t *)(d + at[1]), (const uint32_t *)(d + at[2]),
                                (const uint32_t *)(d + at[3]), (uint32_t)rg->chr.size()};
      an->d_name_off = (const uint32_t *)(d + at[4]);
      an->d_names = (const uint8_t *)(d + at[5]);
    }
    *out = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_annot_info(const gs_annot *an, uint64_t *n_groups, uint64_t *n_segments, uint64_t *n_entries) {
  if (!an) return GS_ERR_ARG;
  if (n_groups) *n_groups = an->group_names.size();
  if (n_segments) *n_segments = an->h.n_segments;
  if (n_entries) *n_entries = an->h.ent.size();
  return GS_OK;
}

extern "C" void gs_annot_free(gs_annot *an) { an_release(an); }

extern "C" gs_status gs_index_set_annotation(gs_index *ix, const gs_annot *an) {
  GS_HANDLE_LOCK(ix);
  if (!ix) return GS_ERR_ARG;
  if (an && an->device != ix->device) {
    gs_set_error("gs_index_set_annotation: the annotation was built for another device, or for the host only");
    return GS_ERR_ARG;
  }
  ix->annot = an;
  return GS_OK;
}

/* does the structure a call resolves with have the chromosomes the annotation was made for? */
static bool an_same_structure(const gs_annot *an, const gs_genome_structure *gs) {
  if (gs->n_chr != an->chr_lengths.size() || (gs->n_chr && !gs->chr_lengths)) return false;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (gs->chr_lengths[c] != an->chr_lengths[c]) return false;
  return true;
}

/* ---- the lookup on the device --------------------------------------------------------------------------------------- */

struct an_args {
  gs_an_table t;
  const uint64_t *offsets; /* n + 1 positions into hits */
  const gs_hit *hits;
  const uint64_t *chr_cum; /* n_chr + 1 */
  uint32_t *cnt;           /* n_hits + 1 */
  const uint64_t *foff;    /* n_hits + 1 */
  uint32_t *feats, *gcnt, *err;
  gs_annot_own own;        /* own.hits == nullptr: no rule */
  uint64_t off0, n_hits;
  uint32_t n, n_chr, L, P, m;
};
struct an_widen {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
/* the guide whose list holds hit h: the last g with offsets[g] <= h (guides with empty lists share an offset) */
__device__ __forceinline__ uint32_t an_guide_of(const an_args &a, uint64_t h) {
  uint32_t lo = 0, hi = a.n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.offsets[mid] <= h)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(AN_BLOCK) void k_an_count(an_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * AN_BLOCK + threadIdx.x; i <= a.n_hits; i += (uint64_t)gridDim.x * AN_BLOCK) {
    uint32_t c = 0;
    if (i < a.n_hits) {
      const gs_hit hit = a.hits[a.off0 + i];
      const uint32_t d = (uint32_t)(hit.key >> 61);
      if (d > a.m) {
        atomicOr(a.err, AN_ERR_DISTANCE);
      } else {
        const gs_loc loc = gs_resolve_abs(a.chr_cum, a.n_chr, a.L, a.P, (long long)hit.pos);
        if (loc.c >= 0) c = gs_an_count(a.t, (uint32_t)loc.c, loc.s, a.L + a.P, a.chr_cum[loc.c + 1] - a.chr_cum[loc.c]);
        if (c) {
          const uint32_t g = an_guide_of(a, a.off0 + i);
          atomicAdd(&a.gcnt[(size_t)g * (a.m + 1u) + d], 1u);
          if (a.own.hits && d <= a.own.distance &&
              !(d == 0u && (uint32_t)loc.c == a.own.chr[g] && loc.s == (long long)a.own.pos[g] && (uint8_t)loc.st == a.own.sense[g]))
            atomicAdd(&a.own.hits[g], 1u);
        }
      }
    }
    a.cnt[i] = c;
  }
}
__global__ __launch_bounds__(AN_BLOCK) void k_an_emit(an_args a) {
  for (uint64_t i = (uint64_t)blockIdx.x * AN_BLOCK + threadIdx.x; i < a.n_hits; i += (uint64_t)gridDim.x * AN_BLOCK) {
    const uint64_t lo = a.foff[i], hi = a.foff[i + 1];
    if (lo == hi) continue;
    const gs_loc loc = gs_resolve_abs(a.chr_cum, a.n_chr, a.L, a.P, (long long)a.hits[a.off0 + i].pos);
    if (loc.c < 0) continue; /* the count pass saw the same hit: never */
    uint64_t r = lo;
    gs_an_visit(a.t, (uint32_t)loc.c, loc.s, a.L + a.P, a.chr_cum[loc.c + 1] - a.chr_cum[loc.c], [&](uint32_t g) {
      if (r < hi) a.feats[r++] = g; /* the count pass saw the same table: always */
    });
  }
}

gs_status gs_annotate_device_own(gs_index *ix, const gs_annot *an, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                                 uint32_t mismatches, const void *d_offsets, const void *d_hits, void *stream, const gs_annot_own *own,
                                 const void **d_feat_offsets, const void **d_feats, const void **d_guide_counts) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !an || !gs || !d_feat_offsets || !d_feats || !d_guide_counts || (n && !d_offsets)) return GS_ERR_ARG;
  if (n >= (1ull << 31) || mismatches > 7 || L < 1 || (uint64_t)L + P > 255) return GS_ERR_ARG;
  if (an->device != ix->device) {
    gs_set_error("gs_annotate_device: the annotation was built for another device, or for the host only");
    return GS_ERR_ARG;
  }
  if (!an_same_structure(an, gs)) {
    gs_set_error("gs_annotate_device: the genome structure is not the one the annotation was made against");
    return GS_ERR_ARG;
  }
  *d_feat_offsets = *d_feats = *d_guide_counts = nullptr;
  try {
    hipStream_t st = (hipStream_t)stream;
    GS_HIP(hipSetDevice(ix->device));
    std::vector<uint64_t> cum(gs->n_chr + 1, 0);
    for (uint32_t c = 0; c < gs->n_chr; c++) cum[c + 1] = cum[c] + gs->chr_lengths[c];
    GS_TRY(gs_reserve(ix->w_annot.in, 8 * cum.size() + 16));
    GS_HIP(hipMemcpyAsync(ix->w_annot.in.p, cum.data(), 8 * cum.size(), hipMemcpyHostToDevice, st));
    uint64_t ends[2] = {0, 0};
    if (n) {
      GS_HIP(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, st));
      GS_HIP(hipMemcpyAsync(&ends[1], (const uint64_t *)d_offsets + n, 8, hipMemcpyDeviceToHost, st));
    }
    GS_HIP(hipStreamSynchronize(st)); /* `cum` and `ends` are locals */
    if (ends[1] < ends[0]) return GS_ERR_ARG;
    const uint64_t nh = ends[1] - ends[0];
    if (nh && !d_hits) return GS_ERR_ARG;
    const size_t gc_bytes = 4 * (size_t)n * (mismatches + 1);
    GS_TRY(gs_reserve(ix->w_annot.cnt, 4 * (nh + 1) + 16));
    GS_TRY(gs_reserve(ix->w_annot.foff, 8 * (nh + 1) + 16));
    GS_TRY(gs_reserve(ix->w_annot.gcnt, gc_bytes + 32));
    an_args a;
    memset(&a, 0, sizeof a);
    a.t = an->d_table;
    a.offsets = (const uint64_t *)d_offsets;
    a.hits = (const gs_hit *)d_hits;
    a.chr_cum = (const uint64_t *)ix->w_annot.in.p;
    a.cnt = (uint32_t *)ix->w_annot.cnt.p;
    a.foff = (const uint64_t *)ix->w_annot.foff.p;
    a.gcnt = (uint32_t *)ix->w_annot.gcnt.p;
    a.err = (uint32_t *)((char *)ix->w_annot.gcnt.p + ((gc_bytes + 15) & ~(size_t)15));
    if (own) a.own = *own;
    a.off0 = ends[0];
    a.n_hits = nh;
    a.n = (uint32_t)n;
    a.n_chr = gs->n_chr;
    a.L = L;
    a.P = P;
    a.m = mismatches;
    GS_HIP(hipMemsetAsync(ix->w_annot.gcnt.p, 0, ((gc_bytes + 15) & ~(size_t)15) + 16, st));
    const uint64_t cap = (uint64_t)gs_num_cus(ix->device) * 32u;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nh + 1 + AN_BLOCK - 1) / AN_BLOCK, cap))), block(AN_BLOCK);
    hipLaunchKernelGGL(k_an_count, grid, block, 0, st, a);
    GS_TRY(gs_prim("gs_annotate_device: scan of the counts", ix->w_annot.tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, rocprim::make_transform_iterator((const uint32_t *)a.cnt, an_widen()), (uint64_t *)ix->w_annot.foff.p,
                                     (uint64_t)0, (size_t)nh + 1, rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    uint32_t err = 0;
    GS_HIP(hipMemcpyAsync(&total, a.foff + nh, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    if (err & AN_ERR_DISTANCE) {
      gs_set_error("gs_annotate_device: a distance beyond `mismatches`");
      return GS_ERR_ARG;
    }
    GS_TRY(gs_reserve(ix->w_annot.feats, 4 * total + 16));
    a.feats = (uint32_t *)ix->w_annot.feats.p;
    if (total) hipLaunchKernelGGL(k_an_emit, grid, block, 0, st, a);
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    *d_feat_offsets = ix->w_annot.foff.p;
    *d_feats = ix->w_annot.feats.p;
    *d_guide_counts = ix->w_annot.gcnt.p;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_annotate_device(gs_index *ix, const gs_annot *an, const gs_genome_structure *gs, uint64_t n, uint32_t L,
                                        uint32_t P, uint32_t mismatches, const void *d_offsets, const void *d_hits, void *stream,
                                        const void **d_feat_offsets, const void **d_feats, const void **d_guide_counts) {
  return gs_annotate_device_own(ix, an, gs, n, L, P, mismatches, d_offsets, d_hits, stream, nullptr, d_feat_offsets, d_feats,
                                d_guide_counts);
}

static gs_status an_feats_out(const std::vector<uint32_t> &v, uint32_t **feats, uint64_t *n_feats) {
  *feats = (uint32_t *)malloc(4 * v.size() + 4);
  if (!*feats) return GS_ERR_NOMEM;
  if (!v.empty()) memcpy(*feats, v.data(), 4 * v.size());
  *n_feats = v.size();
  return GS_OK;
}

extern "C" gs_status gs_annotate(gs_index *ix, const gs_annot *an, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                                 uint32_t mismatches, const uint64_t *offsets, const gs_hit *hits, uint64_t *feat_offsets,
                                 uint32_t **feats, uint64_t *n_feats, uint32_t *guide_counts) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !an || !gs || !feat_offsets || !feats || !n_feats || (n && (!offsets || !guide_counts))) return GS_ERR_ARG;
  *feats = nullptr;
  *n_feats = 0;
  const uint64_t b = n ? offsets[0] : 0, e = n ? offsets[n] : 0;
  if (e < b || (e > b && !hits)) return GS_ERR_ARG;
  const uint64_t nh = e - b;
  try {
    GS_HIP(hipSetDevice(ix->device));
    const size_t b_o = (8 * ((size_t)n + 1) + 15) & ~(size_t)15;
    GS_TRY(gs_reserve(ix->w_annot.io, b_o + sizeof(gs_hit) * (size_t)nh + 64));
    char *d_o = (char *)ix->w_annot.io.p, *d_h = d_o + b_o;
    /* the hits the offsets name, from 0 */
    std::vector<uint64_t> rel((size_t)n + 1, 0);
    for (uint64_t g = 0; g <= n && n; g++) rel[g] = offsets[g] - b;
    GS_HIP(hipMemcpy(d_o, rel.data(), 8 * rel.size(), hipMemcpyHostToDevice));
    if (nh) GS_HIP(hipMemcpy(d_h, hits + b, sizeof(gs_hit) * (size_t)nh, hipMemcpyHostToDevice));
    const void *d_fo = nullptr, *d_f = nullptr, *d_gc = nullptr;
    GS_TRY(gs_annotate_device(ix, an, gs, n, L, P, mismatches, d_o, d_h, nullptr, &d_fo, &d_f, &d_gc));
    GS_HIP(hipMemcpy(feat_offsets, d_fo, 8 * ((size_t)nh + 1), hipMemcpyDeviceToHost));
    std::vector<uint32_t> v((size_t)feat_offsets[nh]);
    if (!v.empty()) GS_HIP(hipMemcpy(v.data(), d_f, 4 * v.size(), hipMemcpyDeviceToHost));
    if (n) GS_HIP(hipMemcpy(guide_counts, d_gc, 4 * (size_t)n * (mismatches + 1), hipMemcpyDeviceToHost));
    return an_feats_out(v, feats, n_feats);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

/* ---- the same on the host, through the shared headers ------------------------------------------------------------------ */

extern "C" gs_status gs_debug_annotate_host(const gs_annot *an, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                                            uint32_t mismatches, const uint64_t *offsets, const gs_hit *hits, uint64_t *feat_offsets,
                                            uint32_t **feats, uint64_t *n_feats, uint32_t *guide_counts) {
  if (!an || !gs || !feat_offsets || !feats || !n_feats || (n && (!offsets || !guide_counts))) return GS_ERR_ARG;
  if (mismatches > 7 || L < 1 || (uint64_t)L + P > 255 || !an_same_structure(an, gs)) return GS_ERR_ARG;
  *feats = nullptr;
  *n_feats = 0;
  const uint64_t b = n ? offsets[0] : 0, e = n ? offsets[n] : 0;
  if (e < b || (e > b && !hits)) return GS_ERR_ARG;
  try {
    std::vector<uint64_t> cum(gs->n_chr + 1, 0);
    for (uint32_t c = 0; c < gs->n_chr; c++) cum[c + 1] = cum[c] + gs->chr_lengths[c];
    const gs_an_table t = an->h.table();
    std::vector<uint32_t> v;
    if (n) memset(guide_counts, 0, 4 * (size_t)n * (mismatches + 1));
    feat_offsets[0] = 0;
    for (uint64_t g = 0; g < n; g++) {
      if (offsets[g + 1] < offsets[g] || offsets[g + 1] > e) return GS_ERR_ARG;
      for (uint64_t h = offsets[g]; h < offsets[g + 1]; h++) {
        const uint32_t d = GS_KEY_MISMATCHES(hits[h].key);
        if (d > mismatches) return GS_ERR_ARG;
        const gs_loc loc = gs_resolve_abs(cum.data(), gs->n_chr, L, P, (long long)hits[h].pos);
        uint32_t c = 0;
        if (loc.c >= 0) c = gs_an_visit(t, (uint32_t)loc.c, loc.s, L + P, gs->chr_lengths[loc.c], [&](uint32_t f) { v.push_back(f); });
        if (c) guide_counts[g * (mismatches + 1) + d]++;
        feat_offsets[h - b + 1] = v.size();
      }
    }
    return an_feats_out(v, feats, n_feats);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}
