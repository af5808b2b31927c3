/*
 * gs_pairs.hip -- guide pairs for regions (`enumerate --regions BED --pairs FILE`): the pairing stage behind
 * gs_design_score.  The reference has no counterpart.  The rule is stated once, in gs_pairs_scan.h; DESIGN.md section
 * 5.10 has the passes.  Every pass is one lane per element; no lane walks over partners.
 *
 *   gs_design_pairs   k_pr_mark    eligible && specificity >= S                                  (5 B read, 4 written)
 *                     (rocprim exclusive scan of the marks: the places of the compacted records)
 *                     k_pr_keys    the marked records' key chromosome << 33 | cut << 1 | minus and index  (14 B read, 12 written)
 *                     (rocprim radix_sort_pairs on the key, k_pr_group_of, radix_sort_pairs on the group: stable, so the
 *                     records are ordered by (group, chromosome, cut, sense))
 *                     k_pr_sorted  in sorted order: key, pam_right, specificity                   (17 B read, 16 written)
 *                     (rocprim exclusive scan of pam_right: the prefix counts)
 *                     k_pr_count   per sorted record a: [lo, hi) from two binary searches over (group, key), the number
 *                                  of partners from the prefix counts                 (2 log2 E dependent reads, 16 B written)
 *                     (rocprim 64-bit exclusive scan of the counts: the pair offsets)
 *                     k_pr_group_heads  the offset at every group's head -> host, 8 (n_groups + 1) bytes
 *                     host: the groups dealt greedily into chunks of whole groups, at most `chunk` pairs each
 *                     per chunk:
 *                     k_pr_emit    per pair t: its record a from an upper bound over the offsets, its partner b (under an
 *                                  orientation: a binary search for the r-th record of the wanted side over the prefix
 *                                  counts), the words group << 32 | ~bits(min) and ~bits(max)
 *                                                                    (log2 E [+ log2 (hi - lo)] dependent reads, 24 B written)
 *                     (rocprim radix_sort_pairs on the max word, k_pr_regather, radix_sort_pairs on the group and min
 *                     word: stable, so the pairs are ordered by (group, min desc, max desc, t))
 *                     k_pr_keep    rank = place - the group's head; the first N of each group go to their places in the
 *                                  result, known on the host from the groups' counts       (12 B read, 8 written per kept)
 *                     k_pr_flag    per kept pair: byte 1 at a and at b (plain stores; several lanes may store the same
 *                                  value to one byte)
 *                     gs_ds_select over the flags (gs_design.hip): the guides of the result, and per record its place
 *                     k_pr_finish  per kept pair: group, chromosome, the places of a and b in the guides, cuts, specificities
 *   gs_pairs_rows     host: the table, N rows per group
 * k_pr_count and k_pr_emit are bound by their dependent reads - each step of a search waits for the load before it - not
 * by their bytes; the rest is bound by memory and by the four sorts.
 */
#include "gs_common.h"
#include "gs_scratch.h"
#include "gs_design_obj.h"
#include "gs_pairs_scan.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <memory>

#define PR_BLOCK 256
#define PR_CHUNK_DEFAULT (1ull << 26)
#define PR_CHUNK_MAX 0xFFFFFF00ull /* a pair index within a chunk is 32 bits */

static std::atomic<uint64_t> g_pr_chunk{PR_CHUNK_DEFAULT};
extern "C" uint64_t gs_debug_pairs_chunk(uint64_t set) {
  if (set) g_pr_chunk.store(std::min<uint64_t>(set, PR_CHUNK_MAX));
  return g_pr_chunk.load();
}

struct gs_pairs {
  uint64_t n = 0;
  std::vector<uint32_t> group, chr, a, b, cut_a, cut_b;
  std::vector<float> spec_a, spec_b;
  std::vector<std::string> group_names, chr_names;
  uint64_t last[6] = {0, 0, 0, 0, 0, 0};
  double ms[GS_PAIRS_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0}; /* gs_pairs_ms */
};

/* events on the stream of a call: lap(slot) adds the time since the event before it to ms[slot] (slot < 0: to nothing),
 * read once the stream is idle */
struct pr_laps {
  hipStream_t st;
  std::vector<std::pair<int, hipEvent_t>> ev;
  explicit pr_laps(hipStream_t s) : st(s) {}
  pr_laps(const pr_laps &) = delete;
  pr_laps &operator=(const pr_laps &) = delete;
  ~pr_laps() {
    for (auto &e : ev)
      if (e.second) (void)hipEventDestroy(e.second);
  }
  gs_status lap(int slot) {
    ev.emplace_back(slot, nullptr);
    GS_HIP(hipEventCreate(&ev.back().second));
    GS_HIP(hipEventRecord(ev.back().second, st));
    return GS_OK;
  }
  gs_status read(double *ms) const {
    for (size_t i = 1; i < ev.size(); i++) {
      float t = 0;
      if (ev[i].first < 0) continue;
      GS_HIP(hipEventElapsedTime(&t, ev[i - 1].second, ev[i].second));
      ms[ev[i].first] += t;
    }
    return GS_OK;
  }
};
enum { PR_MS_COMPACT, PR_MS_ORDER, PR_MS_COUNT, PR_MS_OFFSETS, PR_MS_EMIT, PR_MS_RANK, PR_MS_KEEP, PR_MS_GUIDES };

static gs_status pr_rule_args(const gs_pair_rule *rule, uint32_t k, bool &filter) {
  if (!rule) return GS_ERR_ARG;
  const char *why = nullptr;
  if (rule->min_span > rule->max_span) why = "pairs: min_span > max_span";
  else if (rule->cut_offset > k) why = "pairs: cut_offset beyond the k-mer length";
  else if (rule->orientation > GS_PAIRS_PAM_IN) why = "pairs: unknown orientation";
  else if (rule->min_specificity != rule->min_specificity || rule->min_specificity > 1.0f) why = "pairs: a specificity bound is 0 to 1";
  if (why) {
    gs_set_error(why);
    return GS_ERR_ARG;
  }
  filter = rule->min_specificity >= 0.0f;
  return GS_OK;
}

/* ---- what the host decides between the count and the emit passes --------------------------------------------------- */

struct pr_plan {
  std::vector<uint64_t> koff;                        /* n_groups + 1: where each group's kept pairs begin in the result */
  std::vector<std::pair<uint32_t, uint32_t>> chunks; /* [g0, g1) */
  uint64_t total = 0, kept = 0, without = 0, short_of = 0;
};
/* goff: n_groups + 1 pair offsets at the groups' heads */
static gs_status pr_make_plan(const std::vector<uint64_t> &goff, const std::vector<std::string> &names, uint32_t per_region,
                              uint64_t chunk, pr_plan &p) {
  const size_t ng = goff.size() - 1;
  p.koff.assign(ng + 1, 0);
  p.total = goff[ng] - goff[0];
  uint64_t acc = 0;
  uint32_t g0 = 0;
  for (size_t g = 0; g < ng; g++) {
    const uint64_t c = goff[g + 1] - goff[g];
    if (c > chunk) {
      gs_set_error("pairs: group '" + names[g] + "' has " + std::to_string(c) + " pairs, more than a chunk of " + std::to_string(chunk) +
                   " holds: narrow --max-span or split the group");
      return GS_ERR_UNSUPPORTED;
    }
    if (acc + c > chunk) {
      p.chunks.emplace_back(g0, (uint32_t)g);
      g0 = (uint32_t)g;
      acc = 0;
    }
    acc += c;
    p.koff[g + 1] = p.koff[g] + (per_region ? std::min<uint64_t>(c, per_region) : c);
    if (c == 0) p.without++;
    else if (per_region && c < per_region) p.short_of++;
  }
  if (acc) p.chunks.emplace_back(g0, (uint32_t)ng);
  p.kept = p.koff[ng];
  return GS_OK;
}

/* ---- the kernels ------------------------------------------------------------------------------------------------------ */

struct gs_pr_args {
  /* the design's records */
  const uint32_t *group, *chr, *pos;
  const uint8_t *sense, *elig;
  const float *spec;
  uint64_t n;
  uint32_t k, P, C, start, orientation, filter, per_region;
  float min_spec;
  uint64_t min_span, max_span;
  /* the compacted, sorted records: E of them */
  uint32_t E;
  const uint32_t *place;  /* n + 1 */
  uint32_t *idx;          /* record of a place, before / after the sorts */
  uint64_t *key;
  uint32_t *sgroup, *pr;  /* pr: E + 1 */
  float *sspec;
  const uint32_t *pp;     /* E + 1 */
  uint32_t *lo, *hi;
  uint64_t *cnt;          /* E + 1 */
  const uint64_t *poff;   /* E + 1 */
  /* per group */
  uint64_t *goff;         /* n_groups + 1 */
  const uint64_t *koff;   /* n_groups + 1 */
  uint32_t n_groups;
  /* a chunk: m pairs from pair P0 on */
  uint64_t P0, m;
  uint32_t *pa, *pb, *tix, *wmax;
  uint64_t *wmin;
  /* the result: K kept pairs, as places of the sorted order */
  uint32_t *res_a, *res_b;
  uint64_t K;
};

__global__ __launch_bounds__(PR_BLOCK) void k_pr_mark(gs_pr_args a, uint32_t *mark) {
  const uint64_t j = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (j > a.n) return;
  mark[j] = j < a.n && a.elig[j] && (!a.filter || a.spec[j] >= a.min_spec) ? 1u : 0u;
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_keys(gs_pr_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t o = a.place[j];
  if (a.place[j + 1] == o) return; /* not marked */
  const uint8_t s = a.sense[j];
  a.key[o] = gs_pr_key(a.chr[j], gs_pr_cut(a.pos[j], s, a.k, a.P, a.C, a.start != 0), s);
  a.idx[o] = (uint32_t)j;
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_group_of(const uint32_t *group, const uint32_t *idx, uint32_t E, uint32_t *out) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i < E) out[i] = group[idx[i]];
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_sorted(gs_pr_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i > a.E) return;
  if (i == a.E) {
    a.pr[i] = 0;
    return;
  }
  const uint32_t r = a.idx[i];
  const uint8_t s = a.sense[r];
  a.key[i] = gs_pr_key(a.chr[r], gs_pr_cut(a.pos[r], s, a.k, a.P, a.C, a.start != 0), s);
  a.pr[i] = gs_pr_pam_right(s, a.start != 0) ? 1u : 0u;
  a.sspec[i] = a.spec[r];
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_count(gs_pr_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i > a.E) return;
  if (i == a.E) {
    a.cnt[i] = 0;
    return;
  }
  uint32_t lo, hi;
  gs_pr_range(a.sgroup, a.key, a.E, (uint32_t)i, a.min_span, a.max_span, &lo, &hi);
  a.lo[i] = lo;
  a.hi[i] = hi;
  a.cnt[i] = gs_pr_count(a.orientation, a.pp[i + 1] != a.pp[i], a.pp, lo, hi);
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_group_heads(gs_pr_args a) {
  const uint64_t g = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (g > a.n_groups) return;
  a.goff[g] = a.poff[gs_pr_lower(a.sgroup, a.key, 0, a.E, (uint32_t)g, 0)]; /* g == n_groups: no such group, the end */
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_emit(gs_pr_args a) {
  const uint64_t t = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (t >= a.m) return;
  const uint64_t T = a.P0 + t;
  const uint32_t ra = gs_pr_owner(a.poff, a.E, T);
  const uint32_t r = (uint32_t)(T - a.poff[ra]);
  const uint32_t rb = gs_pr_partner(a.orientation, a.pp, a.lo[ra], a.hi[ra], r);
  const float sa = a.sspec[ra], sb = a.sspec[rb];
  a.pa[t] = ra;
  a.pb[t] = rb;
  a.wmin[t] = gs_pr_word_min(a.sgroup[ra], sa, sb);
  a.wmax[t] = gs_pr_word_max(sa, sb);
  a.tix[t] = (uint32_t)t;
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_regather(const uint64_t *w, const uint32_t *t, uint64_t m, uint64_t *out) {
  const uint64_t j = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (j < m) out[j] = w[t[j]];
}
/* wmin_s, t_s: the chunk's pairs in ranked order */
__global__ __launch_bounds__(PR_BLOCK) void k_pr_keep(gs_pr_args a, const uint64_t *wmin_s, const uint32_t *t_s) {
  const uint64_t j = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t g = (uint32_t)(wmin_s[j] >> 32);
  const uint64_t rank = a.P0 + j - a.goff[g];
  if (a.per_region && rank >= a.per_region) return;
  const uint64_t o = a.koff[g] + rank;
  const uint32_t t = t_s[j];
  a.res_a[o] = a.pa[t];
  a.res_b[o] = a.pb[t];
}
__global__ __launch_bounds__(PR_BLOCK) void k_pr_flag(gs_pr_args a, uint8_t *flag) {
  const uint64_t o = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (o >= a.K) return;
  flag[a.idx[a.res_a[o]]] = 1;
  flag[a.idx[a.res_b[o]]] = 1;
}
struct gs_pr_out {
  uint32_t *group, *chr, *a, *b, *cut_a, *cut_b;
  float *spec_a, *spec_b;
};
__global__ __launch_bounds__(PR_BLOCK) void k_pr_finish(gs_pr_args a, const uint32_t *place_of, gs_pr_out out) {
  const uint64_t o = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (o >= a.K) return;
  const uint32_t ra = a.res_a[o], rb = a.res_b[o];
  const uint64_t ka = a.key[ra], kb = a.key[rb];
  out.group[o] = a.sgroup[ra];
  out.chr[o] = gs_pr_key_chr(ka);
  out.a[o] = place_of[a.idx[ra]];
  out.b[o] = place_of[a.idx[rb]];
  out.cut_a[o] = gs_pr_key_cut(ka);
  out.cut_b[o] = gs_pr_key_cut(kb);
  out.spec_a[o] = a.sspec[ra];
  out.spec_b[o] = a.sspec[rb];
}

static dim3 pr_grid(uint64_t n) { return dim3((unsigned)((n + PR_BLOCK - 1) / PR_BLOCK)); }

static gs_status pr_device(gs_design *d, const char *prefix, const gs_pair_rule *rule, bool filter, hipStream_t st, gs_kmers **guides,
                           gs_pairs *pr) {
  const uint64_t n = d->n;
  const size_t n_groups = d->rg->group_names.size();
  GS_HIP(hipSetDevice(d->device));
  gs_scratch mem;
  gs_prim_tmp tmp;
  gs_pr_args a;
  memset(&a, 0, sizeof a);
  a.group = (const uint32_t *)d->d_group;
  a.chr = (const uint32_t *)d->d_chr;
  a.pos = (const uint32_t *)d->d_pos;
  a.sense = (const uint8_t *)d->d_sense;
  a.elig = (const uint8_t *)d->d_elig;
  a.spec = (const float *)d->d_spec;
  a.n = n;
  a.k = d->k;
  a.P = d->P;
  a.C = rule->cut_offset;
  a.start = rule->flags & GS_FLAG_PAM_AT_START ? 1u : 0u;
  a.orientation = rule->orientation;
  a.filter = filter ? 1u : 0u;
  a.per_region = rule->per_region;
  a.min_spec = rule->min_specificity;
  a.min_span = rule->min_span;
  a.max_span = rule->max_span;
  a.n_groups = (uint32_t)n_groups;
  const dim3 block(PR_BLOCK);
  pr_laps laps(st);

  uint8_t *flag = nullptr;
  uint32_t *place_of = nullptr;
  GS_TRY(mem.get(n, &flag));
  GS_TRY(mem.get(4 * n, &place_of));
  GS_HIP(hipMemsetAsync(flag, 0, n + 16, st));

  uint32_t E = 0;
  uint32_t *mark = nullptr, *place = nullptr;
  if (n) {
    GS_TRY(mem.get(4 * (n + 1), &mark));
    GS_TRY(mem.get(4 * (n + 1), &place));
    GS_TRY(laps.lap(-1));
    hipLaunchKernelGGL(k_pr_mark, pr_grid(n + 1), block, 0, st, a, mark);
    GS_TRY(gs_prim("pairs: places of the eligible records", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, mark, place, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    }));
    GS_HIP(hipMemcpyAsync(&E, place + n, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    mem.drop(mark);
  }
  pr->last[0] = E;
  pr_plan plan;
  std::vector<uint64_t> goff(n_groups + 1, 0);
  if (E) {
    uint64_t *key0 = nullptr, *key = nullptr;
    uint32_t *idx0 = nullptr, *idx1 = nullptr, *idx2 = nullptr, *grp_g = nullptr, *sgroup = nullptr, *prr = nullptr, *pp = nullptr, *lo = nullptr,
             *hi = nullptr;
    float *sspec = nullptr;
    uint64_t *cnt = nullptr, *poff = nullptr, *d_goff = nullptr, *d_koff = nullptr;
    GS_TRY(mem.get(8 * (size_t)E, &key0));
    GS_TRY(mem.get(8 * (size_t)E, &key));
    GS_TRY(mem.get(4 * (size_t)E, &idx0));
    GS_TRY(mem.get(4 * (size_t)E, &idx1));
    GS_TRY(mem.get(4 * (size_t)E, &idx2));
    GS_TRY(mem.get(4 * (size_t)E, &grp_g));
    GS_TRY(mem.get(4 * (size_t)E, &sgroup));
    a.E = E;
    a.place = place;
    a.key = key0;
    a.idx = idx0;
    hipLaunchKernelGGL(k_pr_keys, pr_grid(n), block, 0, st, a);
    GS_TRY(laps.lap(PR_MS_COMPACT));
    GS_TRY(gs_prim("pairs: sort by chromosome, cut and sense", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::radix_sort_pairs(p, b, key0, key, idx0, idx1, (size_t)E, 0u, 64u, st);
    }));
    hipLaunchKernelGGL(k_pr_group_of, pr_grid(E), block, 0, st, a.group, (const uint32_t *)idx1, E, grp_g);
    /* stable: records of one group keep the order of their keys */
    GS_TRY(gs_prim("pairs: sort by group", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::radix_sort_pairs(p, b, grp_g, sgroup, idx1, idx2, (size_t)E, 0u, 32u, st);
    }));
    GS_TRY(laps.lap(PR_MS_ORDER));
    GS_HIP(hipStreamSynchronize(st));
    mem.drop(key0);
    mem.drop(idx0);
    mem.drop(idx1);
    mem.drop(grp_g);
    mem.drop(place);
    GS_TRY(mem.get(4 * ((size_t)E + 1), &prr));
    GS_TRY(mem.get(4 * ((size_t)E + 1), &pp));
    GS_TRY(mem.get(4 * (size_t)E, &sspec));
    GS_TRY(mem.get(4 * (size_t)E, &lo));
    GS_TRY(mem.get(4 * (size_t)E, &hi));
    GS_TRY(mem.get(8 * ((size_t)E + 1), &cnt));
    GS_TRY(mem.get(8 * ((size_t)E + 1), &poff));
    GS_TRY(mem.get(8 * (n_groups + 1), &d_goff));
    GS_TRY(mem.get(8 * (n_groups + 1), &d_koff));
    a.key = key;
    a.idx = idx2;
    a.sgroup = sgroup;
    a.pr = prr;
    a.sspec = sspec;
    GS_TRY(laps.lap(-1));
    hipLaunchKernelGGL(k_pr_sorted, pr_grid((uint64_t)E + 1), block, 0, st, a);
    GS_TRY(gs_prim("pairs: prefix counts of the PAM side", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, prr, pp, 0u, (size_t)E + 1, rocprim::plus<uint32_t>(), st);
    }));
    a.pp = pp;
    a.lo = lo;
    a.hi = hi;
    a.cnt = cnt;
    GS_TRY(laps.lap(PR_MS_ORDER));
    hipLaunchKernelGGL(k_pr_count, pr_grid((uint64_t)E + 1), block, 0, st, a);
    GS_TRY(laps.lap(PR_MS_COUNT));
    GS_TRY(gs_prim("pairs: offsets of the pairs", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, cnt, poff, 0ull, (size_t)E + 1, rocprim::plus<uint64_t>(), st);
    }));
    a.poff = poff;
    a.goff = d_goff;
    hipLaunchKernelGGL(k_pr_group_heads, pr_grid(n_groups + 1), block, 0, st, a);
    GS_TRY(laps.lap(PR_MS_OFFSETS));
    GS_HIP(hipMemcpyAsync(goff.data(), d_goff, 8 * (n_groups + 1), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    mem.drop(cnt);
    GS_TRY(pr_make_plan(goff, d->rg->group_names, rule->per_region, g_pr_chunk.load(), plan));
    if (plan.kept >= (1ull << 38)) {
      gs_set_error("pairs: " + std::to_string(plan.kept) + " pairs to keep: give --per-region or narrow --max-span");
      return GS_ERR_UNSUPPORTED;
    }
    const uint64_t K = plan.kept;
    a.K = K;
    if (K) {
      uint64_t most = 0;
      for (const auto &c : plan.chunks) most = std::max(most, goff[c.second] - goff[c.first]);
      uint32_t *pa = nullptr, *pb = nullptr, *tix = nullptr, *t1 = nullptr, *t2 = nullptr, *wmax = nullptr, *wmax_s = nullptr;
      uint64_t *wmin = nullptr, *wmin_g = nullptr, *wmin_s = nullptr;
      GS_TRY(mem.get(4 * (size_t)K, &a.res_a));
      GS_TRY(mem.get(4 * (size_t)K, &a.res_b));
      for (uint32_t **q : {&pa, &pb, &tix, &t1, &t2, &wmax, &wmax_s}) GS_TRY(mem.get(4 * (size_t)most, q));
      for (uint64_t **q : {&wmin, &wmin_g, &wmin_s}) GS_TRY(mem.get(8 * (size_t)most, q));
      GS_HIP(hipMemcpyAsync(d_koff, plan.koff.data(), 8 * (n_groups + 1), hipMemcpyHostToDevice, st));
      a.koff = d_koff;
      a.pa = pa;
      a.pb = pb;
      a.tix = tix;
      a.wmax = wmax;
      a.wmin = wmin;
      for (const auto &c : plan.chunks) {
        a.P0 = goff[c.first];
        a.m = goff[c.second] - goff[c.first];
        const size_t m = (size_t)a.m;
        GS_TRY(laps.lap(-1));
        hipLaunchKernelGGL(k_pr_emit, pr_grid(m), block, 0, st, a);
        GS_TRY(laps.lap(PR_MS_EMIT));
        GS_TRY(gs_prim("pairs: sort by the larger specificity", mem, tmp, [&](void *p, size_t &b) {
          return rocprim::radix_sort_pairs(p, b, wmax, wmax_s, tix, t1, m, 0u, 32u, st);
        }));
        hipLaunchKernelGGL(k_pr_regather, pr_grid(m), block, 0, st, (const uint64_t *)wmin, (const uint32_t *)t1, (uint64_t)m, wmin_g);
        /* stable: pairs of equal group and smaller specificity keep the order of the larger one, then of t */
        GS_TRY(gs_prim("pairs: sort by group and the smaller specificity", mem, tmp, [&](void *p, size_t &b) {
          return rocprim::radix_sort_pairs(p, b, wmin_g, wmin_s, t1, t2, m, 0u, 64u, st);
        }));
        GS_TRY(laps.lap(PR_MS_RANK));
        hipLaunchKernelGGL(k_pr_keep, pr_grid(m), block, 0, st, a, (const uint64_t *)wmin_s, (const uint32_t *)t2);
        GS_TRY(laps.lap(PR_MS_KEEP));
      }
      hipLaunchKernelGGL(k_pr_flag, pr_grid(K), block, 0, st, a, flag);
      GS_TRY(laps.lap(PR_MS_KEEP));
      GS_HIP(hipStreamSynchronize(st));
      GS_HIP(hipGetLastError());
      for (uint32_t **q : {&pa, &pb, &tix, &t1, &t2, &wmax, &wmax_s}) mem.drop(*q);
      for (uint64_t **q : {&wmin, &wmin_g, &wmin_s}) mem.drop(*q);
    }
  } else {
    GS_TRY(pr_make_plan(goff, d->rg->group_names, rule->per_region, g_pr_chunk.load(), plan));
  }
  pr->last[1] = plan.total;
  pr->last[2] = plan.kept;
  pr->last[3] = plan.chunks.size();
  pr->last[4] = plan.without;
  pr->last[5] = plan.short_of;

  /* the guides: the flagged records through the ordering, gather and id passes of a selection */
  gs_kmers *km = nullptr;
  GS_TRY(laps.lap(-1));
  const gs_ds_select_rule sel{flag, 0u, false, -1.0f, place_of, false};
  GS_TRY(gs_ds_select(d, prefix, sel, st, false, &km, nullptr, nullptr));
  std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(km, km_release);

  const size_t K = (size_t)plan.kept;
  pr->n = K;
  pr->group.resize(K), pr->chr.resize(K), pr->a.resize(K), pr->b.resize(K), pr->cut_a.resize(K), pr->cut_b.resize(K);
  pr->spec_a.resize(K), pr->spec_b.resize(K);
  if (K) {
    uint32_t *cols = nullptr;
    GS_TRY(mem.get(32 * K, &cols));
    const gs_pr_out out{cols, cols + K, cols + 2 * K, cols + 3 * K, cols + 4 * K, cols + 5 * K, (float *)(cols + 6 * K), (float *)(cols + 7 * K)};
    hipLaunchKernelGGL(k_pr_finish, pr_grid(K), block, 0, st, a, (const uint32_t *)place_of, out);
    void *to[8] = {pr->group.data(), pr->chr.data(), pr->a.data(), pr->b.data(), pr->cut_a.data(), pr->cut_b.data(), pr->spec_a.data(),
                   pr->spec_b.data()};
    for (int c = 0; c < 8; c++) GS_HIP(hipMemcpyAsync(to[c], cols + (size_t)c * K, 4 * K, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
  }
  GS_TRY(laps.lap(PR_MS_GUIDES));
  GS_HIP(hipStreamSynchronize(st));
  GS_TRY(laps.read(pr->ms));
  *guides = own.release();
  return GS_OK;
}

extern "C" gs_status gs_design_pairs(gs_design *d, const char *prefix, const gs_pair_rule *rule, void *stream, gs_kmers **guides,
                                     gs_pairs **pairs) {
  if (!d || !prefix || !rule || !guides || !pairs || strlen(prefix) >= (1u << 20)) return GS_ERR_ARG;
  bool filter = false;
  GS_TRY(pr_rule_args(rule, d->k, filter));
  if (d->device < 0) return GS_ERR_ARG;
  if (!d->scored) {
    gs_set_error("pairs are ranked by specificity: gs_design_score first");
    return GS_ERR_ARG;
  }
  if (d->space_d) {
    gs_set_error("gs_design_pairs on a design with a minimum spacing: pairs have their own span rule");
    return GS_ERR_ARG;
  }
  *guides = nullptr;
  *pairs = nullptr;
  try {
    std::unique_ptr<gs_pairs> pr(new gs_pairs());
    pr->group_names = d->rg->group_names;
    pr->chr_names = d->rg->chr_names;
    GS_TRY(pr_device(d, prefix, rule, filter, (hipStream_t)stream, guides, pr.get()));
    *pairs = pr.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_pairs_get(gs_pairs *p, uint64_t *n, const void **group, const void **chr, const void **a, const void **b,
                                  const void **cut_a, const void **cut_b, const void **spec_a, const void **spec_b) {
  if (!p) return GS_ERR_ARG;
  if (n) *n = p->n;
  if (group) *group = p->group.data();
  if (chr) *chr = p->chr.data();
  if (a) *a = p->a.data();
  if (b) *b = p->b.data();
  if (cut_a) *cut_a = p->cut_a.data();
  if (cut_b) *cut_b = p->cut_b.data();
  if (spec_a) *spec_a = p->spec_a.data();
  if (spec_b) *spec_b = p->spec_b.data();
  return GS_OK;
}

extern "C" gs_status gs_pairs_last(const gs_pairs *p, uint64_t out[6]) {
  if (!p || !out) return GS_ERR_ARG;
  for (int i = 0; i < 6; i++) out[i] = p->last[i];
  return GS_OK;
}

extern "C" gs_status gs_pairs_ms(const gs_pairs *p, double out[GS_PAIRS_STAGES]) {
  if (!p || !out) return GS_ERR_ARG;
  for (int i = 0; i < GS_PAIRS_STAGES; i++) out[i] = p->ms[i];
  return GS_OK;
}

extern "C" void gs_pairs_free(gs_pairs *p) { delete p; }

#define PR_HEADER "group,id_a,id_b,chromosome,cut_a,cut_b,span,specificity_a,specificity_b,pair_specificity\n"

extern "C" gs_status gs_pairs_rows(gs_pairs *p, const gs_kmers *guides, char **text, uint64_t *len) {
  if (!p || !guides || !text || !len) return GS_ERR_ARG;
  *text = nullptr;
  *len = 0;
  const void *ids = nullptr, *off = nullptr, *s01 = nullptr;
  uint64_t m = 0;
  GS_TRY(gs_kmers_get(const_cast<gs_kmers *>(guides), 0, &m, nullptr, nullptr, nullptr, nullptr));
  GS_TRY(gs_kmers_get_ids(const_cast<gs_kmers *>(guides), 0, &ids, &off, &s01));
  const uint64_t *o = (const uint64_t *)off;
  const char *t = (const char *)ids;
  try {
    std::string out = PR_HEADER;
    for (uint64_t i = 0; i < p->n; i++) {
      const uint32_t a = p->a[i], b = p->b[i];
      if (a >= m || b >= m || p->group[i] >= p->group_names.size() || p->chr[i] >= p->chr_names.size()) {
        gs_set_error("gs_pairs_rows: these are not the guides of the pairs");
        return GS_ERR_ARG;
      }
      const float lower = gs_rg_float_bits(p->spec_a[i]) < gs_rg_float_bits(p->spec_b[i]) ? p->spec_a[i] : p->spec_b[i];
      out += p->group_names[p->group[i]];
      out += ',';
      out.append(t + o[a], (size_t)(o[a + 1] - o[a]));
      out += ',';
      out.append(t + o[b], (size_t)(o[b + 1] - o[b]));
      out += ',';
      out += p->chr_names[p->chr[i]];
      out += ',' + std::to_string(p->cut_a[i]) + ',' + std::to_string(p->cut_b[i]) + ',' + std::to_string(p->cut_b[i] - p->cut_a[i]) + ',';
      out += gs_f2s(p->spec_a[i]) + ',' + gs_f2s(p->spec_b[i]) + ',' + gs_f2s(lower) + '\n';
    }
    *text = (char *)malloc(out.size() + 1);
    if (!*text) return GS_ERR_NOMEM;
    memcpy(*text, out.c_str(), out.size() + 1);
    *len = out.size();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

/* ---- the same stages on the host, through the shared header ----------------------------------------------------------- */

extern "C" gs_status gs_debug_pairs_host(uint64_t n, const uint32_t *group, const uint32_t *chr, const uint32_t *position,
                                         const uint8_t *sense, const float *specificity, const uint8_t *eligible, uint32_t k, uint32_t P,
                                         uint32_t n_groups, const gs_pair_rule *rule, gs_pairs **out) {
  if (!out || (n && (!group || !chr || !position || !sense || !specificity)) || n >= (1ull << 32) - 1) return GS_ERR_ARG;
  bool filter = false;
  GS_TRY(pr_rule_args(rule, k, filter));
  for (uint64_t j = 0; j < n; j++)
    if (group[j] >= n_groups || position[j] < 1) return GS_ERR_ARG;
  *out = nullptr;
  try {
    std::unique_ptr<gs_pairs> pr(new gs_pairs());
    const bool start = rule->flags & GS_FLAG_PAM_AT_START;
    /* mark and compact, the two stable sorts */
    std::vector<uint32_t> idx;
    std::vector<uint64_t> key_of(n);
    for (uint64_t j = 0; j < n; j++) {
      key_of[j] = gs_pr_key(chr[j], gs_pr_cut(position[j], sense[j], k, P, rule->cut_offset, start), sense[j]);
      if ((!eligible || eligible[j]) && (!filter || specificity[j] >= rule->min_specificity)) idx.push_back((uint32_t)j);
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return key_of[x] < key_of[y]; });
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return group[x] < group[y]; });
    const uint32_t E = (uint32_t)idx.size();
    std::vector<uint32_t> sgroup(E), pp(E + 1, 0), lo(E), hi(E);
    std::vector<uint64_t> key(E), poff(E + 1, 0);
    std::vector<float> sspec(E);
    for (uint32_t i = 0; i < E; i++) {
      sgroup[i] = group[idx[i]];
      key[i] = key_of[idx[i]];
      sspec[i] = specificity[idx[i]];
      pp[i + 1] = pp[i] + (gs_pr_pam_right(sense[idx[i]], start) ? 1u : 0u);
    }
    for (uint32_t i = 0; i < E; i++) {
      gs_pr_range(sgroup.data(), key.data(), E, i, rule->min_span, rule->max_span, &lo[i], &hi[i]);
      poff[i + 1] = poff[i] + gs_pr_count(rule->orientation, pp[i + 1] != pp[i], pp.data(), lo[i], hi[i]);
    }
    std::vector<uint64_t> goff(n_groups + 1);
    for (uint32_t g = 0; g <= n_groups; g++) goff[g] = poff[gs_pr_lower(sgroup.data(), key.data(), 0, E, g, 0)];
    pr_plan plan;
    std::vector<std::string> names(n_groups);
    for (uint32_t g = 0; g < n_groups; g++) names[g] = std::to_string(g);
    GS_TRY(pr_make_plan(goff, names, rule->per_region, g_pr_chunk.load(), plan));
    /* chunk by chunk: emit, the two stable sorts, cut */
    for (const auto &c : plan.chunks) {
      const uint64_t P0 = goff[c.first], m = goff[c.second] - P0;
      std::vector<uint32_t> pa(m), pb(m), wmax(m), order(m);
      std::vector<uint64_t> wmin(m);
      for (uint64_t t = 0; t < m; t++) {
        const uint32_t ra = gs_pr_owner(poff.data(), E, P0 + t);
        const uint32_t rb = gs_pr_partner(rule->orientation, pp.data(), lo[ra], hi[ra], (uint32_t)(P0 + t - poff[ra]));
        pa[t] = ra;
        pb[t] = rb;
        wmin[t] = gs_pr_word_min(sgroup[ra], sspec[ra], sspec[rb]);
        wmax[t] = gs_pr_word_max(sspec[ra], sspec[rb]);
        order[t] = (uint32_t)t;
      }
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return wmax[x] < wmax[y]; });
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return wmin[x] < wmin[y]; });
      for (uint64_t j = 0; j < m; j++) {
        const uint32_t t = order[j], g = (uint32_t)(wmin[t] >> 32);
        if (rule->per_region && P0 + j - goff[g] >= rule->per_region) continue;
        const uint32_t ra = pa[t], rb = pb[t];
        pr->group.push_back(g);
        pr->chr.push_back(gs_pr_key_chr(key[ra]));
        pr->a.push_back(idx[ra]);
        pr->b.push_back(idx[rb]);
        pr->cut_a.push_back(gs_pr_key_cut(key[ra]));
        pr->cut_b.push_back(gs_pr_key_cut(key[rb]));
        pr->spec_a.push_back(sspec[ra]);
        pr->spec_b.push_back(sspec[rb]);
      }
    }
    pr->n = pr->group.size();
    pr->last[0] = E;
    pr->last[1] = plan.total;
    pr->last[2] = plan.kept;
    pr->last[3] = plan.chunks.size();
    pr->last[4] = plan.without;
    pr->last[5] = plan.short_of;
    *out = pr.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}
