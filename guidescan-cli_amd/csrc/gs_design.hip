/*
 * gs_design.hip -- guides for regions (`--regions BED`, `--per-region N`, `--min-specificity S`): the stages between the
 * candidate scan (gs_kmers.hip) and the batch pipeline.  The reference has no counterpart: the pipelines of its manual
 * (manual/manual.tex:321-656) end in a script that filters the genome-wide table by coordinate and specificity.  The
 * rules are stated once, in gs_regions_scan.h; DESIGN.md section 5.8 has the passes.
 *
 *   gs_regions_parse      host: the BED file against the genome structure -> per chromosome the merged intervals of all
 *                         groups sorted by start, with the running maximum of their ends
 *   gs_design_restrict    k_ds_count   one lane per candidate: the groups that hold it            (4 B read, 4 B written)
 *                         (rocprim exclusive scan of the counts)
 *                         k_ds_emit    one record per (candidate, group): sequence, PAM, position, sense, group,
 *                                      chromosome, copied next to each other so that the records are the layout
 *                                      gs_enumerate_device takes                      (k + P + 5 B read, k + P + 13 written)
 *   gs_design_score       batches of records through gs_enumerate_device and gs_score_device: the specificity lands in
 *                         the design's float[n]; with a threshold the counting pass fills an eligibility byte per record
 *   gs_design_select      k_ds_keys    the two sort words and the record's index                (13 B read, 20 B written)
 *                         (rocprim radix_sort_pairs on the low word, k_ds_regather, radix_sort_pairs on the high word:
 *                         the second pass is stable, so the records are ordered by (high, low))
 *                         k_ds_mark    eligible && specificity >= S                             (4 + 5 B read, 4 written)
 *                         (rocprim exclusive scan of the marks: a record's rank among the marked ones before it)
 *                         k_ds_heads   the first record of every group leaves its rank in the group's slot
 *                         k_ds_cut     keep = marked && rank - rank of the group's head < N
 *                         with gs_design_set_spacing, in place of the two (gs_select_scan.h, no counterpart in the reference):
 *                         k_ds_bounds  the first and last record of every group leave its begin and end place
 *                         k_ds_space   one wave per group walks its records in order, 64 a step, against the kept cuts in
 *                                      LDS: keep = marked && no kept record within D && fewer than N kept  (17 B read, 4 written)
 *                         (rocprim exclusive scan of the keeps: the places)
 *                         k_ds_gather  the kept records into a fresh gs_kmers                 (k + P + 13 B each way)
 *                         gs_km_encode_text (gs_kmers.hip: k_km_text_len / 64-bit scan / k_km_text_write over the row of
 *                         gs_rowtext.h): the ids "{prefix}{group}:{chr}:{pos}:{sense}" or the kmers-file rows, names read
 *                         from one uploaded table
 * Every kernel is one record per lane over 4- and 8-byte arrays; they are bound by memory and by the two sorts.
 */
#include "gs_common.h"
#include "gs_scratch.h"
#include "gs_kmers_obj.h"
#include "gs_regions_scan.h"
#include "gs_regions_obj.h"
#include "gs_annot_obj.h"
#include "gs_design_obj.h"
#include "gs_select_scan.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <memory>

#define DS_BLOCK 256

/* ---- the regions file ------------------------------------------------------------------------------------------ */

static const char *const RG_REASON[9] = {"",
                                         "fewer than three fields",
                                         "start or end is not a non-negative integer",
                                         "start >= end",
                                         "no such chromosome in the genome structure",
                                         "end beyond the chromosome's length",
                                         "group name contains ','",
                                         "group name too long: an id could pass 254 bytes",
                                         "no interval in the file"};

static void rg_report_clear(gs_regions_report *rep) {
  if (rep) memset(rep, 0, sizeof *rep);
}
static gs_status rg_bad(gs_regions_report *rep, uint32_t kind, uint64_t line) {
  std::string msg = kind == GS_REGIONS_BAD_EMPTY ? std::string("regions file: ") + RG_REASON[kind]
                                                 : "regions line " + std::to_string(line) + ": " + RG_REASON[kind];
  gs_set_error(msg);
  if (rep) {
    rep->bad_kind = kind;
    rep->bad_line = line;
    rep->bad_len = msg.size();
    rep->bad_text = (char *)malloc(msg.size() + 1);
    if (!rep->bad_text) return GS_ERR_NOMEM;
    memcpy(rep->bad_text, msg.c_str(), msg.size() + 1);
  }
  return GS_ERR_FORMAT;
}
/* digits only, at most 18 of them: the value */
static bool rg_integer(const std::string &f, uint64_t &v) {
  if (f.empty() || f.size() > 18) return false;
  v = 0;
  for (char c : f) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint64_t)(c - '0');
  }
  return true;
}

static gs_status rg_parse(const uint8_t *raw, uint64_t len, const gs_genome_structure *gs, const char *prefix, gs_regions *rg,
                          gs_regions_report *rep) {
  for (uint32_t c = 0; c < gs->n_chr; c++) {
    rg->chr_names.push_back(gs->chr_names[c]);
    rg->chr_lengths.push_back(gs->chr_lengths[c]);
  }
  for (const std::string &s : rg->chr_names) rg->chr_name_ptrs.push_back(s.c_str());
  std::map<std::string, uint32_t> chr_of, group_of;
  size_t longest_chr = 0;
  for (uint32_t c = 0; c < gs->n_chr; c++) {
    chr_of.emplace(rg->chr_names[c], c); /* the first of a name given twice */
    longest_chr = std::max(longest_chr, rg->chr_names[c].size());
  }
  const size_t prefix_len = prefix ? strlen(prefix) : 0;
  struct iv {
    uint32_t group, chr, start, end;
  };
  std::vector<iv> ivs;
  uint64_t line_no = 0;
  for (uint64_t at = 0; at < len;) {
    const uint8_t *nl = (const uint8_t *)memchr(raw + at, '\n', len - at);
    uint64_t e = nl ? (uint64_t)(nl - raw) : len;
    std::string line((const char *)raw + at, (size_t)(e - at));
    at = e + 1;
    line_no++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
    std::vector<std::string> f;
    for (size_t b = 0; b < line.size();) {
      while (b < line.size() && (line[b] == ' ' || line[b] == '\t')) b++;
      size_t q = b;
      while (q < line.size() && line[q] != ' ' && line[q] != '\t') q++;
      if (q > b) f.push_back(line.substr(b, q - b));
      b = q;
    }
    if (f.size() < 3) return rg_bad(rep, GS_REGIONS_BAD_FEW, line_no);
    uint64_t s = 0, t = 0;
    if (!rg_integer(f[1], s) || !rg_integer(f[2], t)) return rg_bad(rep, GS_REGIONS_BAD_INTEGER, line_no);
    if (s >= t) return rg_bad(rep, GS_REGIONS_BAD_ORDER, line_no);
    const auto ci = chr_of.find(f[0]);
    if (ci == chr_of.end()) return rg_bad(rep, GS_REGIONS_BAD_CHROMOSOME, line_no);
    if (t > rg->chr_lengths[ci->second]) return rg_bad(rep, GS_REGIONS_BAD_BEYOND, line_no);
    if (t >= (1ull << 32)) { /* the scan takes no such chromosome either */
      gs_set_error("regions on chromosomes of 2^32 bases or more");
      return GS_ERR_UNSUPPORTED;
    }
    const std::string name = f.size() > 3 ? f[3] : f[0] + ":" + f[1] + "-" + f[2];
    if (name.find(',') != std::string::npos) return rg_bad(rep, GS_REGIONS_BAD_COMMA, line_no);
    /* {prefix}{group}:{chr}:{position}:{sense} with ten position digits */
    if (prefix_len + name.size() + 1 + longest_chr + 1 + 10 + 2 > 254) return rg_bad(rep, GS_REGIONS_BAD_LONG, line_no);
    auto gi = group_of.find(name);
    if (gi == group_of.end()) {
      gi = group_of.emplace(name, (uint32_t)rg->group_names.size()).first;
      rg->group_names.push_back(name);
    }
    ivs.push_back(iv{gi->second, ci->second, (uint32_t)s, (uint32_t)t});
  }
  if (rep) rep->n_lines = line_no;
  if (ivs.empty()) return rg_bad(rep, GS_REGIONS_BAD_EMPTY, 0);
  /* per group and chromosome: merged where they overlap or abut */
  std::sort(ivs.begin(), ivs.end(), [](const iv &a, const iv &b) {
    return a.chr != b.chr ? a.chr < b.chr : a.group != b.group ? a.group < b.group : a.start != b.start ? a.start < b.start : a.end < b.end;
  });
  std::vector<iv> merged;
  for (const iv &v : ivs) {
    if (!merged.empty() && merged.back().chr == v.chr && merged.back().group == v.group && v.start <= merged.back().end)
      merged.back().end = std::max(merged.back().end, v.end);
    else
      merged.push_back(v);
  }
  std::sort(merged.begin(), merged.end(), [](const iv &a, const iv &b) {
    return a.chr != b.chr ? a.chr < b.chr : a.start != b.start ? a.start < b.start : a.end != b.end ? a.end < b.end : a.group < b.group;
  });
  rg->chr.resize(gs->n_chr);
  for (const iv &v : merged) {
    gs_rg_chr &t = rg->chr[v.chr];
    t.start.push_back(v.start);
    t.end.push_back(v.end);
    t.maxend.push_back(t.maxend.empty() ? v.end : std::max(t.maxend.back(), v.end));
    t.group.push_back(v.group);
  }
  rg->n_intervals = merged.size();
  if (rep) {
    rep->n_intervals = merged.size();
    rep->n_groups = rg->group_names.size();
  }
  return GS_OK;
}

extern "C" gs_status gs_regions_parse(const uint8_t *raw, uint64_t len, const gs_genome_structure *gs, const char *prefix,
                                      gs_regions **out, gs_regions_report *rep) {
  rg_report_clear(rep);
  if (!out || (len && !raw) || !gs || (gs->n_chr && (!gs->chr_names || !gs->chr_lengths))) return GS_ERR_ARG;
  for (uint32_t c = 0; c < gs->n_chr; c++)
    if (!gs->chr_names[c]) return GS_ERR_ARG;
  *out = nullptr;
  try {
    std::unique_ptr<gs_regions> rg(new gs_regions());
    GS_TRY(rg_parse(raw, len, gs, prefix, rg.get(), rep));
    *out = rg.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_regions_parse_file(const char *path, const gs_genome_structure *gs, const char *prefix, gs_regions **out,
                                           gs_regions_report *rep) {
  rg_report_clear(rep);
  if (!path || !out) return GS_ERR_ARG;
  FILE *f = fopen(path, "rb");
  if (!f) {
    gs_set_error(std::string("cannot read ") + path);
    return GS_ERR_IO;
  }
  std::string raw;
  bool bad = false;
  try {
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.append(buf, got);
    bad = ferror(f) != 0;
  } catch (const std::bad_alloc &) {
    fclose(f);
    return GS_ERR_NOMEM;
  }
  fclose(f);
  if (bad) {
    gs_set_error(std::string("cannot read ") + path);
    return GS_ERR_IO;
  }
  return gs_regions_parse((const uint8_t *)raw.data(), raw.size(), gs, prefix, out, rep);
}

extern "C" gs_status gs_regions_info(const gs_regions *rg, uint64_t *n_groups, uint64_t *n_intervals) {
  if (!rg) return GS_ERR_ARG;
  if (n_groups) *n_groups = rg->group_names.size();
  if (n_intervals) *n_intervals = rg->n_intervals;
  return GS_OK;
}

extern "C" void gs_regions_free(gs_regions *rg) { delete rg; }

/* ---- the design: the records of (candidate, group) ---------------------------------------------------------------- */

static void ds_release(gs_design *d) {
  if (!d) return;
  bool any = false;
  for (void *p : {d->d_seqs, d->d_pams, d->d_pos, d->d_sense, d->d_group, d->d_chr, d->d_spec, d->d_elig, d->d_fhits}) any = any || p;
  if (any) hipSetDevice(d->device);
  for (void *p : {d->d_seqs, d->d_pams, d->d_pos, d->d_sense, d->d_group, d->d_chr, d->d_spec, d->d_elig, d->d_fhits})
    if (p) hipFree(p);
  delete d;
}
typedef std::unique_ptr<gs_design, void (*)(gs_design *)> ds_owner;

gs_status gs_ds_array(size_t bytes, void **out) { /* an array of an object: its release frees it */
  gs_scratch one;
  GS_TRY(one.get(bytes, out));
  one.keep(*out);
  return GS_OK;
}
/* the arrays of n records; every record eligible and unscored */
static gs_status ds_alloc(gs_design *d, hipStream_t st) {
  const size_t n = (size_t)d->n;
  GS_TRY(gs_ds_array(n * d->k, &d->d_seqs));
  GS_TRY(gs_ds_array(n * d->P, &d->d_pams));
  GS_TRY(gs_ds_array(4 * n, &d->d_pos));
  GS_TRY(gs_ds_array(n, &d->d_sense));
  GS_TRY(gs_ds_array(4 * n, &d->d_group));
  GS_TRY(gs_ds_array(4 * n, &d->d_chr));
  GS_TRY(gs_ds_array(4 * n, &d->d_spec));
  GS_TRY(gs_ds_array(n, &d->d_elig));
  GS_HIP(hipMemsetAsync(d->d_spec, 0, 4 * n + 16, st));
  GS_HIP(hipMemsetAsync(d->d_elig, 1, n + 16, st));
  return GS_OK;
}

struct gs_ds_restrict_args {
  gs_rg_table t;
  const uint8_t *seqs, *pams, *sense;
  const uint32_t *pos;
  uint32_t *cnt;       /* n + 1 */
  const uint32_t *off; /* n + 1 */
  uint8_t *o_seqs, *o_pams, *o_sense;
  uint32_t *o_pos, *o_group, *o_chr;
  uint64_t n;
  uint32_t k, P, chr;
};
struct ds_widen {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
__global__ __launch_bounds__(DS_BLOCK) void k_ds_count(gs_ds_restrict_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j > a.n) return;
  a.cnt[j] = j < a.n ? gs_rg_count(a.t, a.pos[j] - 1u, a.k + a.P) : 0u;
}
__global__ __launch_bounds__(DS_BLOCK) void k_ds_emit(gs_ds_restrict_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t lo = a.off[j], hi = a.off[j + 1];
  if (lo == hi) return;
  const uint32_t pos = a.pos[j];
  const uint8_t sense = a.sense[j];
  uint32_t r = lo;
  gs_rg_visit(a.t, pos - 1u, a.k + a.P, [&](uint32_t i) {
    if (r >= hi) return; /* the count pass saw the same table: never */
    for (uint32_t u = 0; u < a.k; u++) a.o_seqs[(uint64_t)r * a.k + u] = a.seqs[j * a.k + u];
    for (uint32_t u = 0; u < a.P; u++) a.o_pams[(uint64_t)r * a.P + u] = a.pams[j * a.P + u];
    a.o_pos[r] = pos;
    a.o_sense[r] = sense;
    a.o_group[r] = a.t.group[i];
    a.o_chr[r] = a.chr;
    r++;
  });
}

extern "C" gs_status gs_design_restrict(const gs_regions *rg, uint32_t chr_index, gs_kmers *scan, void *stream, gs_design **part) {
  if (!rg || !scan || !part || chr_index >= rg->chr.size()) return GS_ERR_ARG;
  if (scan->parsed || scan->device < 0) {
    gs_set_error("gs_design_restrict takes the candidates of a scan on a device");
    return GS_ERR_ARG;
  }
  *part = nullptr;
  hipStream_t st = (hipStream_t)stream;
  try {
    ds_owner own(new gs_design(), ds_release);
    gs_design *d = own.get();
    d->device = scan->device;
    d->rg = rg;
    d->k = scan->k;
    d->P = scan->P;
    const gs_rg_chr &t = rg->chr[chr_index];
    const uint64_t n = scan->n;
    const uint32_t m = (uint32_t)t.start.size();
    if (n >= (1ull << 32) - 1) return GS_ERR_ARG;
    if (n == 0 || m == 0) {
      *part = own.release();
      return GS_OK;
    }
    GS_HIP(hipSetDevice(d->device));
    gs_scratch mem;
    uint32_t *d_tab = nullptr, *d_cnt = nullptr, *d_off = nullptr;
    GS_TRY(mem.get(16 * (size_t)m, &d_tab)); /* the chromosome's table: read by every lane, it stays in L2 */
    const std::vector<uint32_t> *cols[4] = {&t.start, &t.end, &t.maxend, &t.group};
    for (int c = 0; c < 4; c++) GS_HIP(hipMemcpyAsync(d_tab + (size_t)c * m, cols[c]->data(), 4 * (size_t)m, hipMemcpyHostToDevice, st));
    GS_TRY(mem.get(4 * (n + 1), &d_cnt));
    GS_TRY(mem.get(4 * (n + 1), &d_off));
    gs_ds_restrict_args a;
    memset(&a, 0, sizeof a);
    a.t = gs_rg_table{d_tab, d_tab + m, d_tab + 2 * (size_t)m, d_tab + 3 * (size_t)m, m};
    a.seqs = (const uint8_t *)scan->d_seqs;
    a.pams = (const uint8_t *)scan->d_pams;
    a.sense = (const uint8_t *)scan->d_sense;
    a.pos = (const uint32_t *)scan->d_pos;
    a.cnt = d_cnt;
    a.off = d_off;
    a.n = n;
    a.k = d->k;
    a.P = d->P;
    a.chr = chr_index;
    hipLaunchKernelGGL(k_ds_count, dim3((unsigned)((n + 1 + DS_BLOCK - 1) / DS_BLOCK)), dim3(DS_BLOCK), 0, st, a);
    gs_prim_tmp tmp;
    uint64_t *d_total = nullptr; /* a candidate gives at most one record per group: the sum may pass 2^32 */
    GS_TRY(mem.get(8, &d_total));
    GS_TRY(gs_prim("design: sum of the counts", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::reduce(p, b, rocprim::make_transform_iterator(d_cnt, ds_widen()), d_total, (uint64_t)0, (size_t)n,
                             rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    GS_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    if (total >= (1ull << 32) - 1) {
      gs_set_error("gs_design_restrict: 2^32 records or more on one chromosome");
      return GS_ERR_UNSUPPORTED;
    }
    GS_TRY(gs_prim("design: scan of the counts", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, d_cnt, d_off, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    }));
    d->n = total;
    if (total) {
      GS_TRY(ds_alloc(d, st));
      a.o_seqs = (uint8_t *)d->d_seqs;
      a.o_pams = (uint8_t *)d->d_pams;
      a.o_sense = (uint8_t *)d->d_sense;
      a.o_pos = (uint32_t *)d->d_pos;
      a.o_group = (uint32_t *)d->d_group;
      a.o_chr = (uint32_t *)d->d_chr;
      hipLaunchKernelGGL(k_ds_emit, dim3((unsigned)((n + DS_BLOCK - 1) / DS_BLOCK)), dim3(DS_BLOCK), 0, st, a);
    }
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    *part = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_design_concat(gs_design *const *parts, uint32_t n_parts, gs_design **out) {
  if (!out || !parts || n_parts == 0) return GS_ERR_ARG;
  for (uint32_t i = 0; i < n_parts; i++)
    if (!parts[i]) return GS_ERR_ARG;
  for (uint32_t i = 0; i < n_parts; i++)
    if (parts[i]->device != parts[0]->device || parts[i]->k != parts[0]->k || parts[i]->P != parts[0]->P ||
        parts[i]->rg != parts[0]->rg || parts[i]->scored != parts[0]->scored || parts[i]->device < 0) {
      gs_set_error("gs_design_concat: parts of different devices, regions, kmer or PAM lengths, or scores on some of them only");
      return GS_ERR_ARG;
    }
  *out = nullptr;
  try {
    ds_owner own(new gs_design(), ds_release);
    gs_design *d = own.get();
    d->device = parts[0]->device;
    d->rg = parts[0]->rg;
    d->k = parts[0]->k;
    d->P = parts[0]->P;
    d->scored = parts[0]->scored;
    for (uint32_t i = 0; i < n_parts; i++) d->n += parts[i]->n;
    if (d->n >= (1ull << 32) - 1) {
      gs_set_error("gs_design_concat: 2^32 records or more");
      return GS_ERR_UNSUPPORTED;
    }
    if (d->n) {
      GS_HIP(hipSetDevice(d->device));
      GS_TRY(ds_alloc(d, nullptr));
      uint64_t at = 0;
      for (uint32_t i = 0; i < n_parts; i++) {
        const gs_design *p = parts[i];
        if (!p->n) continue;
        const struct {
          void *to;
          const void *from;
          size_t width;
        } cp[8] = {{d->d_seqs, p->d_seqs, d->k}, {d->d_pams, p->d_pams, d->P}, {d->d_pos, p->d_pos, 4},   {d->d_sense, p->d_sense, 1},
                   {d->d_group, p->d_group, 4},  {d->d_chr, p->d_chr, 4},      {d->d_spec, p->d_spec, 4}, {d->d_elig, p->d_elig, 1}};
        for (const auto &c : cp)
          GS_HIP(hipMemcpyAsync((char *)c.to + at * c.width, c.from, (size_t)p->n * c.width, hipMemcpyDeviceToDevice, nullptr));
        at += p->n;
      }
      GS_HIP(hipStreamSynchronize(nullptr));
    }
    *out = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_design_get(gs_design *d, uint64_t *n, const void **groups, const void **chromosomes, const void **positions,
                                   const void **senses, const void **specificity, const void **eligible) {
  if (!d) return GS_ERR_ARG;
  try {
    if (!d->have_host) {
      const size_t m = (size_t)d->n;
      d->h_pos.resize(m), d->h_group.resize(m), d->h_chr.resize(m), d->h_spec.resize(m), d->h_sense.resize(m), d->h_elig.resize(m);
      if (m) {
        GS_HIP(hipSetDevice(d->device));
        GS_HIP(hipMemcpy(d->h_pos.data(), d->d_pos, 4 * m, hipMemcpyDeviceToHost));
        GS_HIP(hipMemcpy(d->h_group.data(), d->d_group, 4 * m, hipMemcpyDeviceToHost));
        GS_HIP(hipMemcpy(d->h_chr.data(), d->d_chr, 4 * m, hipMemcpyDeviceToHost));
        GS_HIP(hipMemcpy(d->h_spec.data(), d->d_spec, 4 * m, hipMemcpyDeviceToHost));
        GS_HIP(hipMemcpy(d->h_sense.data(), d->d_sense, m, hipMemcpyDeviceToHost));
        GS_HIP(hipMemcpy(d->h_elig.data(), d->d_elig, m, hipMemcpyDeviceToHost));
      }
      d->have_host = true;
    }
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  if (n) *n = d->n;
  if (groups) *groups = d->h_group.data();
  if (chromosomes) *chromosomes = d->h_chr.data();
  if (positions) *positions = d->h_pos.data();
  if (senses) *senses = d->h_sense.data();
  if (specificity) *specificity = d->h_spec.data();
  if (eligible) *eligible = d->h_elig.data();
  return GS_OK;
}

extern "C" gs_status gs_design_info(const gs_design *d, uint64_t *n, int *scored) {
  if (!d) return GS_ERR_ARG;
  if (n) *n = d->n;
  if (scored) *scored = d->scored ? 1 : 0;
  return GS_OK;
}

extern "C" gs_status gs_design_last_select(const gs_design *d, uint64_t out[4]) {
  if (!d || !out) return GS_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = d->last[i];
  return GS_OK;
}

extern "C" void gs_design_free(gs_design *d) { ds_release(d); }

/* ---- the score phase: the existing search and scoring, batch by batch ----------------------------------------------- */

__global__ __launch_bounds__(DS_BLOCK) void k_ds_eligible(const uint32_t *raw, uint64_t n, uint8_t *elig) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j < n) elig[j] = raw[j] > 1u ? 0 : 1; /* process.hpp:66-76: more than one hit within the threshold drops the guide */
}

__global__ __launch_bounds__(DS_BLOCK) void k_ds_feature_rule(const uint32_t *fhits, uint64_t n, uint32_t max_hits, uint8_t *elig) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j < n && fhits[j] > max_hits) elig[j] = 0; /* as a --threshold drop */
}

extern "C" gs_status gs_design_set_feature_rule(gs_design *d, const gs_annot *annot, uint32_t distance, uint32_t max_hits) {
  if (!d || d->device < 0) return GS_ERR_ARG;
  if (annot && annot->device != d->device) {
    gs_set_error("gs_design_set_feature_rule: the annotation was built for another device, or for the host only");
    return GS_ERR_ARG;
  }
  d->rule_annot = annot;
  d->rule_distance = distance;
  d->rule_max = max_hits;
  d->have_fhits = false;
  return GS_OK;
}

extern "C" gs_status gs_design_get_feature_hits(gs_design *d, const void **counts) {
  if (!d || !counts || !d->have_fhits) return GS_ERR_ARG;
  try {
    d->h_fhits.resize((size_t)d->n);
    if (d->n) {
      GS_HIP(hipSetDevice(d->device));
      GS_HIP(hipMemcpy(d->h_fhits.data(), d->d_fhits, 4 * (size_t)d->n, hipMemcpyDeviceToHost));
    }
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  *counts = d->h_fhits.data();
  return GS_OK;
}

extern "C" gs_status gs_design_score(gs_index *ix, gs_design *d, const char *alt_pams, uint32_t n_alt, uint32_t mismatches,
                                     uint32_t flags, int64_t threshold, uint64_t batch, void *stream) {
  if (!ix || !d || (n_alt && !alt_pams) || d->device < 0 || mismatches > 7 || threshold > 7 || n_alt > 31) return GS_ERR_ARG;
  if (d->k < 1 || d->k > 31 || d->P > 8 || 2 * d->k + 3 * d->P > 59) {
    gs_set_error("gs_design_score: 2L + 3P > 59, the shape is outside the fast path's key");
    return GS_ERR_UNSUPPORTED;
  }
  if (!batch) batch = 1u << 17;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t sflags = flags & (GS_FLAG_PAM_AT_START | GS_FLAG_NO_NEW_TABLES);
  const gs_genome_structure gs = d->rg->structure();
  struct lock_guard { /* the hit lists and raw counts stay the handle's between the search and the passes that read them */
    gs_index *ix;
    bool held = false;
    ~lock_guard() {
      if (held) gs_index_unlock(ix);
    }
  } lock{ix};
  try {
    GS_HIP(hipSetDevice(d->device));
    GS_TRY(gs_index_lock(ix));
    lock.held = true;
    if (d->rule_annot) {
      if (!d->d_fhits) GS_TRY(gs_ds_array(4 * (size_t)d->n, &d->d_fhits));
      GS_HIP(hipMemsetAsync(d->d_fhits, 0, 4 * (size_t)d->n + 16, st));
      if (threshold < 0) GS_HIP(hipMemsetAsync(d->d_elig, 1, (size_t)d->n + 16, st)); /* the rule alone decides */
    }
    for (uint64_t lo = 0; lo < d->n; lo += batch) {
      const uint64_t nb = std::min<uint64_t>(batch, d->n - lo);
      const char *g = (const char *)d->d_seqs + lo * d->k, *p = (const char *)d->d_pams + lo * d->P;
      const void *d_off = nullptr, *d_hits = nullptr;
      gs_result_view v;
      if (threshold >= 0) { /* the counting pass, as `enumerate -t` runs it: the raw counts are read where the search left them */
        GS_TRY(gs_enumerate_device(ix, g, nb, d->k, p, d->P, alt_pams, n_alt, (uint32_t)threshold, sflags | GS_FLAG_RAW_COUNTS, st, &d_off,
                                   &d_hits, &v));
        if (ix->last_unsupported) {
          gs_set_error("gs_design_score: a record needs the general path");
          return GS_ERR_UNSUPPORTED;
        }
        if (!ix->last_raw_valid) {
          gs_set_error("gs_design_score: the search kept no raw counts");
          return GS_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(k_ds_eligible, dim3((unsigned)((nb + DS_BLOCK - 1) / DS_BLOCK)), dim3(DS_BLOCK), 0, st,
                           (const uint32_t *)ix->w_batch.raw.p, nb, (uint8_t *)d->d_elig + lo);
      }
      GS_TRY(gs_enumerate_device(ix, g, nb, d->k, p, d->P, alt_pams, n_alt, mismatches, sflags, st, &d_off, &d_hits, &v));
      if (ix->last_unsupported) {
        gs_set_error("gs_design_score: a record needs the general path");
        return GS_ERR_UNSUPPORTED;
      }
      /* the CSV rule with no cap on the off-targets, whatever the database is written as */
      GS_TRY(gs_score_device(ix, g, nb, d->k, d->P, sflags & GS_FLAG_PAM_AT_START, -1, &gs, d_off, d_hits, st, nullptr,
                             (float *)d->d_spec + lo));
      if (d->rule_annot) { /* the hit lists are still the handle's: which of them touch a feature */
        const gs_annot_own own{(const uint32_t *)d->d_chr + lo, (const uint32_t *)d->d_pos + lo, (const uint8_t *)d->d_sense + lo,
                               (uint32_t *)d->d_fhits + lo, d->rule_distance};
        const void *fo = nullptr, *ft = nullptr, *gc = nullptr;
        GS_TRY(gs_annotate_device_own(ix, d->rule_annot, &gs, nb, d->k, d->P, mismatches, d_off, d_hits, st, &own, &fo, &ft, &gc));
        hipLaunchKernelGGL(k_ds_feature_rule, dim3((unsigned)((nb + DS_BLOCK - 1) / DS_BLOCK)), dim3(DS_BLOCK), 0, st,
                           (const uint32_t *)d->d_fhits + lo, nb, d->rule_max, (uint8_t *)d->d_elig + lo);
      }
    }
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    d->scored = true;
    d->have_host = false;
    d->have_fhits = d->rule_annot != nullptr;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

/* ---- selection, order and ids ------------------------------------------------------------------------------------- */

struct gs_ds_sel_args {
  const uint32_t *group, *chr, *pos;
  const uint8_t *sense, *elig;
  const float *spec;
  uint64_t *hi, *lo;
  uint32_t *idx;
  uint64_t n;
  uint32_t ranked, per_region, filter;
  float min_spec;
};
__global__ __launch_bounds__(DS_BLOCK) void k_ds_keys(gs_ds_sel_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j >= a.n) return;
  a.hi[j] = gs_rg_key_high(a.group[j], (int)a.ranked, a.spec[j]);
  a.lo[j] = gs_rg_key_low(a.chr[j], a.pos[j], a.sense[j]);
  a.idx[j] = (uint32_t)j;
}
__global__ __launch_bounds__(DS_BLOCK) void k_ds_regather(const uint64_t *hi, const uint32_t *idx, uint64_t n, uint64_t *out) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j < n) out[j] = hi[idx[j]];
}
/* in sorted order: marked = eligible && specificity >= S; one more entry closes the scan */
__global__ __launch_bounds__(DS_BLOCK) void k_ds_mark(gs_ds_sel_args a, const uint32_t *order, uint32_t *mark) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j > a.n) return;
  uint32_t m = 0;
  if (j < a.n) {
    const uint32_t r = order[j];
    m = a.elig[r] && (!a.filter || a.spec[r] >= a.min_spec) ? 1u : 0u;
  }
  mark[j] = m;
}
__global__ __launch_bounds__(DS_BLOCK) void k_ds_heads(const uint64_t *hi_sorted, const uint32_t *rank, uint64_t n, uint32_t *head_rank) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t g = (uint32_t)(hi_sorted[j] >> 32);
  if (j == 0 || (uint32_t)(hi_sorted[j - 1] >> 32) != g) head_rank[g] = rank[j];
}
__global__ __launch_bounds__(DS_BLOCK) void k_ds_cut(const uint64_t *hi_sorted, const uint32_t *mark, const uint32_t *rank,
                                                     const uint32_t *head_rank, uint64_t n, uint32_t per_region, uint32_t *keep,
                                                     uint32_t *kept_of_group) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j > n) return;
  uint32_t kp = 0;
  if (j < n) {
    const uint32_t g = (uint32_t)(hi_sorted[j] >> 32);
    kp = mark[j] && (!per_region || rank[j] - head_rank[g] < per_region) ? 1u : 0u;
    if (kp) atomicAdd(&kept_of_group[g], 1u);
  }
  keep[j] = kp;
}
/* ---- spacing between the picks of a group (gs_select_scan.h) ---------------------------------------------------------- */
/* where every group begins and ends in the sorted order; a group with no record keeps begin == end (both 0) */
__global__ __launch_bounds__(DS_BLOCK) void k_ds_bounds(const uint64_t *hi_sorted, uint64_t n, uint32_t *begin, uint32_t *end) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t g = (uint32_t)(hi_sorted[j] >> 32);
  if (j == 0 || (uint32_t)(hi_sorted[j - 1] >> 32) != g) begin[g] = (uint32_t)j;
  if (j + 1 == n || (uint32_t)(hi_sorted[j + 1] >> 32) != g) end[g] = (uint32_t)(j + 1);
}
struct gs_ds_space_args {
  const uint32_t *chr, *pos;
  const uint8_t *sense;
  const uint32_t *order, *mark, *begin, *end;
  uint32_t *keep, *kept_of_group, *passed_of_group, *marked_of_group;
  uint32_t n_groups, per_region, min_spacing, cut_offset, start, k, P;
};
#define DS_WAVE 64
/* One wave walks one group, 64 records a step, lane i holding record i of the step with its mark and chr << 32 | cut.
 * Phase 1: every lane tests its record against the group's kept list in LDS, all lanes reading the same entry at the same
 * time.  Phase 2: the survivors are resolved in order among themselves - the lowest lane of the ballot is kept and
 * appended to the list, the later lanes within D of it on its chromosome drop out, and the ballot is taken again above
 * it, until it is empty or N is reached.  Control flow is uniform across the wave; the only atomic is the group's final
 * count.  keep[] is written for every record of the group. */
__global__ __launch_bounds__(DS_WAVE) void k_ds_space(gs_ds_space_args a) {
  __shared__ uint64_t list[GS_SL_MAX_PER_REGION];
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= a.n_groups) return;
  const uint32_t b = a.begin[g], e = a.end[g];
  const uint32_t N = a.per_region < GS_SL_MAX_PER_REGION ? a.per_region : GS_SL_MAX_PER_REGION;
  uint32_t kept = 0, passed = 0, marked = 0;
  for (uint32_t base = b; base < e; base += DS_WAVE) {
    const uint32_t j = base + lane;
    const bool valid = j < e;
    if (kept >= N) { /* uniform: the group is full, the rest is cut (its marks are not counted: the group is not short) */
      if (valid) a.keep[j] = 0u;
      continue;
    }
    uint64_t key = 0;
    bool m = false;
    if (valid) {
      const uint32_t r = a.order[j];
      m = a.mark[j] != 0u;
      key = gs_sl_key(a.chr[r], a.pos[r], a.sense[r], a.k, a.P, a.cut_offset, a.start != 0u);
    }
    marked += (uint32_t)__popcll(__ballot(m));
    bool kp = false, alive = m;
    for (uint32_t t = 0; t < kept; t++) alive = alive && !gs_sl_conflict(list[t], key, a.min_spacing);
    unsigned long long cand = __ballot(alive);
    uint32_t stop = DS_WAVE; /* the lane of the N-th pick, where the walk ends */
    while (cand) {
      const uint32_t l = (uint32_t)__ffsll(cand) - 1u;
      const uint64_t picked = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), (int)l) << 32) | (uint32_t)__shfl((int)(uint32_t)key, (int)l);
      if (lane == l) {
        kp = true;
        list[kept] = key;
      }
      kept++;
      if (kept >= N) {
        stop = l;
        break;
      }
      alive = alive && lane > l && !gs_sl_conflict(picked, key, a.min_spacing);
      cand = __ballot(alive);
    }
    passed += (uint32_t)__popcll(__ballot(m && !kp && lane < stop));
    __syncthreads(); /* the list's new entries, before the next step reads them */
    if (valid) a.keep[j] = kp ? 1u : 0u;
  }
  if (lane == 0) {
    if (kept) atomicAdd(&a.kept_of_group[g], kept);
    a.passed_of_group[g] = passed;
    a.marked_of_group[g] = marked;
  }
}

struct gs_ds_gather_args {
  const uint8_t *seqs, *pams, *sense;
  const uint32_t *pos, *group, *chr, *order, *keep, *place;
  uint8_t *o_seqs, *o_pams, *o_sense;
  uint32_t *o_pos, *o_group, *o_chr;
  uint32_t *place_of; /* or null: per record, where it went */
  uint64_t n;
  uint32_t k, P;
};
__global__ __launch_bounds__(DS_BLOCK) void k_ds_gather(gs_ds_gather_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (j >= a.n || !a.keep[j]) return;
  const uint64_t r = a.order[j], o = a.place[j];
  for (uint32_t u = 0; u < a.k; u++) a.o_seqs[o * a.k + u] = a.seqs[r * a.k + u];
  for (uint32_t u = 0; u < a.P; u++) a.o_pams[o * a.P + u] = a.pams[r * a.P + u];
  a.o_pos[o] = a.pos[r];
  a.o_sense[o] = a.sense[r];
  a.o_group[o] = a.group[r];
  a.o_chr[o] = a.chr[r];
  if (a.place_of) a.place_of[r] = (uint32_t)o;
}

/* prefix, group names and chromosome names back to back, and where each begins (gs_km_names, gs_kmers_obj.h) */
static gs_km_names ds_name_table(const gs_regions *rg, const char *prefix) {
  gs_km_names nt;
  nt.names = prefix;
  nt.prefix_len = (uint32_t)nt.names.size();
  for (const std::string &s : rg->group_names) {
    nt.goff.push_back((uint32_t)nt.names.size());
    nt.names += s;
  }
  nt.goff.push_back((uint32_t)nt.names.size());
  for (const std::string &s : rg->chr_names) {
    nt.coff.push_back((uint32_t)nt.names.size());
    nt.names += s;
  }
  nt.coff.push_back((uint32_t)nt.names.size());
  return nt;
}
static void ds_group_tally(gs_design *d, uint64_t kept, const std::vector<uint32_t> &kept_of_group, uint32_t per_region) {
  d->last[0] = d->n;
  d->last[1] = kept;
  d->last[2] = d->last[3] = 0;
  for (uint32_t c : kept_of_group) {
    if (c == 0) d->last[2]++;
    else if (per_region && c < per_region) d->last[3]++;
  }
}

/* the kept records in order as a gs_kmers with ids (rows == false), or their kmers-file rows in HBM (*d_text, the
 * caller's to free); gs_design_obj.h */
gs_status gs_ds_select(gs_design *d, const char *prefix, const gs_ds_select_rule &rule, hipStream_t st, bool rows, gs_kmers **out,
                       void **d_text, uint64_t *text_bytes) {
  const uint32_t per_region = rule.per_region;
  const bool filter = rule.filter;
  const float min_spec = rule.min_spec;
  const uint64_t n = d->n;
  const uint32_t k = d->k, P = d->P;
  const size_t n_groups = d->rg->group_names.size();
  std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new gs_kmers(), km_release);
  gs_kmers *km = own.get();
  km->device = d->device;
  km->k = k;
  km->P = P;
  km->have_ids = km->ids_fixed = true;
  GS_HIP(hipSetDevice(d->device));
  gs_scratch mem;
  gs_prim_tmp tmp;
  uint64_t m = 0;
  uint32_t *o_group = nullptr, *o_chr = nullptr;
  std::vector<uint32_t> kept_of_group(n_groups, 0), space_of_group; /* the latter: passed over, then marked, per group */
  struct marks { /* around k_ds_space, where the rule is set */
    hipEvent_t e[2] = {nullptr, nullptr};
    ~marks() {
      for (hipEvent_t x : e)
        if (x) hipEventDestroy(x);
    }
  } evs;
  hipEvent_t *ev = evs.e;
  if (rule.min_spacing && rule.tally && n)
    for (int i = 0; i < 2; i++) GS_HIP(hipEventCreate(&evs.e[i]));
  if (n) {
    uint32_t *d_space = nullptr;
    uint64_t *hi = nullptr, *lo = nullptr, *key2 = nullptr, *hi_g = nullptr;
    uint32_t *idx = nullptr, *idx1 = nullptr, *idx2 = nullptr, *mark = nullptr, *rank = nullptr, *keep = nullptr, *place = nullptr,
             *head_rank = nullptr, *d_kept = nullptr;
    GS_TRY(mem.get(8 * n, &hi));
    GS_TRY(mem.get(8 * n, &lo));
    GS_TRY(mem.get(8 * n, &key2));
    GS_TRY(mem.get(8 * n, &hi_g));
    GS_TRY(mem.get(4 * n, &idx));
    GS_TRY(mem.get(4 * n, &idx1));
    GS_TRY(mem.get(4 * n, &idx2));
    gs_ds_sel_args a;
    memset(&a, 0, sizeof a);
    a.group = (const uint32_t *)d->d_group;
    a.chr = (const uint32_t *)d->d_chr;
    a.pos = (const uint32_t *)d->d_pos;
    a.sense = (const uint8_t *)d->d_sense;
    a.elig = rule.d_elig;
    a.spec = (const float *)d->d_spec;
    a.hi = hi;
    a.lo = lo;
    a.idx = idx;
    a.n = n;
    a.ranked = per_region ? 1u : 0u;
    a.per_region = per_region;
    a.filter = filter ? 1u : 0u;
    a.min_spec = min_spec;
    const dim3 grid((unsigned)((n + DS_BLOCK - 1) / DS_BLOCK)), grid1((unsigned)((n + 1 + DS_BLOCK - 1) / DS_BLOCK)), block(DS_BLOCK);
    hipLaunchKernelGGL(k_ds_keys, grid, block, 0, st, a);
    GS_TRY(gs_prim("design: sort by the low word", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::radix_sort_pairs(p, b, lo, key2, idx, idx1, (size_t)n, 0u, 64u, st);
    }));
    hipLaunchKernelGGL(k_ds_regather, grid, block, 0, st, (const uint64_t *)hi, (const uint32_t *)idx1, n, hi_g);
    /* stable: records of equal high words keep the order of their low words */
    GS_TRY(gs_prim("design: sort by the high word", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::radix_sort_pairs(p, b, hi_g, key2, idx1, idx2, (size_t)n, 0u, 64u, st);
    }));
    const uint64_t *hi_sorted = key2;
    mem.drop(lo);
    mem.drop(hi);
    GS_TRY(mem.get(4 * (n + 1), &mark));
    GS_TRY(mem.get(4 * (n + 1), &rank));
    GS_TRY(mem.get(4 * (n + 1), &keep));
    GS_TRY(mem.get(4 * (n + 1), &place));
    GS_TRY(mem.get(4 * n_groups, &head_rank));
    GS_TRY(mem.get(4 * n_groups, &d_kept));
    GS_HIP(hipMemsetAsync(head_rank, 0, 4 * n_groups, st));
    GS_HIP(hipMemsetAsync(d_kept, 0, 4 * n_groups, st));
    hipLaunchKernelGGL(k_ds_mark, grid1, block, 0, st, a, (const uint32_t *)idx2, mark);
    GS_TRY(gs_prim("design: ranks of the marked records", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, mark, rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    }));
    if (rule.min_spacing) { /* the walk of every group by one wave in place of the cut by rank */
      uint32_t *bounds = nullptr;
      GS_TRY(mem.get(16 * n_groups, &bounds));
      GS_HIP(hipMemsetAsync(bounds, 0, 16 * n_groups, st));
      GS_HIP(hipMemsetAsync(keep + n, 0, 4, st));
      d_space = bounds + 2 * n_groups;
      hipLaunchKernelGGL(k_ds_bounds, grid, block, 0, st, hi_sorted, n, bounds, bounds + n_groups);
      gs_ds_space_args sa;
      memset(&sa, 0, sizeof sa);
      sa.chr = a.chr;
      sa.pos = a.pos;
      sa.sense = a.sense;
      sa.order = idx2;
      sa.mark = mark;
      sa.begin = bounds;
      sa.end = bounds + n_groups;
      sa.keep = keep;
      sa.kept_of_group = d_kept;
      sa.passed_of_group = d_space;
      sa.marked_of_group = d_space + n_groups;
      sa.n_groups = (uint32_t)n_groups;
      sa.per_region = per_region;
      sa.min_spacing = rule.min_spacing;
      sa.cut_offset = rule.cut_offset;
      sa.start = rule.pam_at_start ? 1u : 0u;
      sa.k = k;
      sa.P = P;
      if (ev[0]) GS_HIP(hipEventRecord(ev[0], st));
      hipLaunchKernelGGL(k_ds_space, dim3((unsigned)n_groups), dim3(DS_WAVE), 0, st, sa);
      if (ev[1]) GS_HIP(hipEventRecord(ev[1], st));
    } else {
      hipLaunchKernelGGL(k_ds_heads, grid, block, 0, st, hi_sorted, (const uint32_t *)rank, n, head_rank);
      hipLaunchKernelGGL(k_ds_cut, grid1, block, 0, st, hi_sorted, (const uint32_t *)mark, (const uint32_t *)rank,
                         (const uint32_t *)head_rank, n, per_region, keep, d_kept);
    }
    GS_TRY(gs_prim("design: places of the kept records", mem, tmp, [&](void *p, size_t &b) {
      return rocprim::exclusive_scan(p, b, keep, place, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    }));
    uint32_t m32 = 0;
    GS_HIP(hipMemcpyAsync(&m32, place + n, 4, hipMemcpyDeviceToHost, st));
    if (n_groups) GS_HIP(hipMemcpyAsync(kept_of_group.data(), d_kept, 4 * n_groups, hipMemcpyDeviceToHost, st));
    if (d_space) {
      space_of_group.resize(2 * n_groups);
      GS_HIP(hipMemcpyAsync(space_of_group.data(), d_space, 8 * n_groups, hipMemcpyDeviceToHost, st));
    }
    GS_HIP(hipStreamSynchronize(st));
    if (ev[0]) {
      float ms = 0;
      GS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      d->space_ms = ms;
    }
    m = m32;
    if (m) {
      GS_TRY(gs_ds_array((size_t)m * k, &km->d_seqs));
      GS_TRY(gs_ds_array((size_t)m * P, &km->d_pams));
      GS_TRY(gs_ds_array(4 * (size_t)m, &km->d_pos));
      GS_TRY(gs_ds_array((size_t)m, &km->d_sense));
      GS_TRY(mem.get(4 * m, &o_group));
      GS_TRY(mem.get(4 * m, &o_chr));
      gs_ds_gather_args ga;
      memset(&ga, 0, sizeof ga);
      ga.seqs = (const uint8_t *)d->d_seqs;
      ga.pams = (const uint8_t *)d->d_pams;
      ga.sense = (const uint8_t *)d->d_sense;
      ga.pos = (const uint32_t *)d->d_pos;
      ga.group = (const uint32_t *)d->d_group;
      ga.chr = (const uint32_t *)d->d_chr;
      ga.order = idx2;
      ga.keep = keep;
      ga.place = place;
      ga.o_seqs = (uint8_t *)km->d_seqs;
      ga.o_pams = (uint8_t *)km->d_pams;
      ga.o_sense = (uint8_t *)km->d_sense;
      ga.o_pos = (uint32_t *)km->d_pos;
      ga.o_group = o_group;
      ga.o_chr = o_chr;
      ga.place_of = rule.d_place;
      ga.n = n;
      ga.k = k;
      ga.P = P;
      hipLaunchKernelGGL(k_ds_gather, grid, block, 0, st, ga);
    }
  }
  if (rule.tally) {
    ds_group_tally(d, m, kept_of_group, per_region);
    d->last_spacing[0] = d->last_spacing[1] = 0;
    for (size_t g = 0; g < n_groups && !space_of_group.empty(); g++) {
      d->last_spacing[0] += space_of_group[g];
      if (kept_of_group[g] < per_region && space_of_group[n_groups + g] >= per_region) d->last_spacing[1]++;
    }
  }
  km->n = m;
  /* the text: ids or rows, by the writer of gs_kmers.hip over the table of all names */
  uint64_t total = 0;
  void *text = nullptr;
  GS_TRY(gs_km_encode_text(km, ds_name_table(d->rg, prefix), o_group, o_chr, rows, "design text: scan of the lengths", st, &text, &total));
  if (rows) {
    *d_text = text;
    *text_bytes = total;
    return GS_OK; /* the object is dropped: the rows are the result */
  }
  *out = own.release();
  return GS_OK;
}

static gs_status ds_select_args(const gs_design *d, const char *prefix, uint32_t per_region, float min_specificity, bool &filter) {
  if (!d || !prefix || strlen(prefix) >= (1u << 20)) return GS_ERR_ARG;
  filter = min_specificity >= 0.0f;
  if (min_specificity != min_specificity || min_specificity > 1.0f) return GS_ERR_ARG;
  if ((per_region || filter) && !d->scored) {
    gs_set_error("a selection by specificity before gs_design_score");
    return GS_ERR_ARG;
  }
  if (d->space_d && (per_region < 1 || per_region > GS_SL_MAX_PER_REGION)) {
    gs_set_error("a minimum spacing needs per_region from 1 to 1024: a group's kept cuts live in LDS");
    return GS_ERR_ARG;
  }
  if (d->space_d && d->space_c > d->k) {
    gs_set_error("the cut offset lies beyond the k-mer length");
    return GS_ERR_ARG;
  }
  return GS_OK;
}
/* the rule of a selection on the design's own eligibility bytes, with the design's spacing */
static gs_ds_select_rule ds_own_rule(const gs_design *d, uint32_t per_region, bool filter, float min_specificity) {
  gs_ds_select_rule rule{(const uint8_t *)d->d_elig, per_region, filter, min_specificity, nullptr, true};
  rule.min_spacing = d->space_d;
  rule.cut_offset = d->space_c;
  rule.pam_at_start = d->space_start;
  return rule;
}

extern "C" gs_status gs_design_set_spacing(gs_design *d, uint32_t min_spacing, uint32_t cut_offset, uint32_t flags) {
  if (!d || (flags & ~GS_FLAG_PAM_AT_START)) return GS_ERR_ARG;
  if (min_spacing && cut_offset > d->k) {
    gs_set_error("gs_design_set_spacing: the cut offset lies beyond the k-mer length");
    return GS_ERR_ARG;
  }
  d->space_d = min_spacing;
  d->space_c = cut_offset;
  d->space_start = (flags & GS_FLAG_PAM_AT_START) != 0;
  return GS_OK;
}

extern "C" gs_status gs_design_last_spacing(const gs_design *d, uint64_t out[2]) {
  if (!d || !out) return GS_ERR_ARG;
  out[0] = d->last_spacing[0];
  out[1] = d->last_spacing[1];
  return GS_OK;
}

extern "C" gs_status gs_debug_design_space_ms(const gs_design *d, double *ms) {
  if (!d || !ms) return GS_ERR_ARG;
  *ms = d->space_ms;
  return GS_OK;
}

extern "C" gs_status gs_debug_design_set_scores(gs_design *d, const float *specificity, const uint8_t *eligible) {
  if (!d || d->device < 0 || (d->n && !specificity)) return GS_ERR_ARG;
  if (d->n) {
    GS_HIP(hipSetDevice(d->device));
    GS_HIP(hipMemcpy(d->d_spec, specificity, 4 * (size_t)d->n, hipMemcpyHostToDevice));
    if (eligible)
      GS_HIP(hipMemcpy(d->d_elig, eligible, (size_t)d->n, hipMemcpyHostToDevice));
    else
      GS_HIP(hipMemset(d->d_elig, 1, (size_t)d->n));
  }
  d->scored = true;
  d->have_host = false;
  return GS_OK;
}

extern "C" gs_status gs_design_select(gs_design *d, const char *prefix, uint32_t per_region, float min_specificity, void *stream,
                                      gs_kmers **out) {
  bool filter = false;
  if (!out) return GS_ERR_ARG;
  GS_TRY(ds_select_args(d, prefix, per_region, min_specificity, filter));
  if (d->device < 0) return GS_ERR_ARG;
  *out = nullptr;
  try {
    const gs_ds_select_rule rule = ds_own_rule(d, per_region, filter, min_specificity);
    return gs_ds_select(d, prefix, rule, (hipStream_t)stream, false, out, nullptr, nullptr);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_design_rows(gs_design *d, const char *prefix, uint32_t per_region, float min_specificity, void *stream,
                                    char **text, uint64_t *len) {
  bool filter = false;
  if (!text || !len) return GS_ERR_ARG;
  GS_TRY(ds_select_args(d, prefix, per_region, min_specificity, filter));
  if (d->device < 0) return GS_ERR_ARG;
  *text = nullptr;
  *len = 0;
  void *d_text = nullptr;
  uint64_t bytes = 0;
  gs_status rc;
  try {
    const gs_ds_select_rule rule = ds_own_rule(d, per_region, filter, min_specificity);
    rc = gs_ds_select(d, prefix, rule, (hipStream_t)stream, true, nullptr, &d_text, &bytes);
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
  if (rc != GS_OK) return rc;
  rc = gs_text_to_host(d_text, bytes, text);
  hipFree(d_text);
  if (rc == GS_OK) *len = bytes;
  return rc;
}

/* ---- the same stages on the host, through the shared header ----------------------------------------------------------- */

static gs_status ds_host_model(const gs_regions *rg, uint32_t n_parts, const uint32_t *chr_index, const uint64_t *n,
                               const uint8_t *const *seqs, const uint32_t *const *positions, const uint8_t *const *senses,
                               const float *const *specificity, const uint8_t *const *eligible, const char *pam, uint32_t k,
                               const char *prefix, uint32_t per_region, float min_specificity, uint32_t min_spacing, uint32_t cut_offset,
                               uint32_t flags, gs_kmers **out, char **rows, uint64_t *rows_len, uint64_t *report) {
  if (!rg || !out || !pam || !prefix || (n_parts && (!chr_index || !n || !seqs || !positions || !senses))) return GS_ERR_ARG;
  if (flags & ~GS_FLAG_PAM_AT_START) return GS_ERR_ARG;
  const uint32_t P = (uint32_t)strlen(pam);
  if (k < 1 || k > 64 || P < 1 || P > 8) return GS_ERR_ARG;
  for (uint32_t i = 0; i < n_parts; i++)
    if (chr_index[i] >= rg->chr.size() || (n[i] && (!seqs[i] || !positions[i] || !senses[i]))) return GS_ERR_ARG;
  *out = nullptr;
  if (rows) *rows = nullptr;
  try {
    gs_design d;
    d.device = -1;
    d.rg = rg;
    d.k = k;
    d.P = P;
    d.scored = specificity != nullptr;
    d.space_d = min_spacing;
    d.space_c = cut_offset;
    d.space_start = (flags & GS_FLAG_PAM_AT_START) != 0;
    bool filter = false;
    GS_TRY(ds_select_args(&d, prefix, per_region, min_specificity, filter));
    /* restrict */
    std::vector<uint32_t> src_part, src_cand;
    for (uint32_t i = 0; i < n_parts; i++) {
      const gs_rg_chr &c = rg->chr[chr_index[i]];
      const gs_rg_table t{c.start.data(), c.end.data(), c.maxend.data(), c.group.data(), (uint32_t)c.start.size()};
      for (uint64_t j = 0; j < n[i]; j++)
        gs_rg_visit(t, positions[i][j] - 1u, k + P, [&](uint32_t iv) {
          d.h_group.push_back(c.group[iv]);
          d.h_chr.push_back(chr_index[i]);
          d.h_pos.push_back(positions[i][j]);
          d.h_sense.push_back(senses[i][j]);
          d.h_spec.push_back(specificity && specificity[i] ? specificity[i][j] : 0.0f);
          d.h_elig.push_back(eligible && eligible[i] ? eligible[i][j] : 1);
          src_part.push_back(i);
          src_cand.push_back((uint32_t)j);
        });
    }
    d.n = d.h_pos.size();
    /* order: the two words */
    std::vector<uint32_t> order(d.n);
    std::vector<uint64_t> hi(d.n), lo(d.n);
    for (uint64_t r = 0; r < d.n; r++) {
      order[r] = (uint32_t)r;
      hi[r] = gs_rg_key_high(d.h_group[r], per_region != 0, d.h_spec[r]);
      lo[r] = gs_rg_key_low(d.h_chr[r], d.h_pos[r], d.h_sense[r]);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lo[a] < lo[b]; });
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hi[a] < hi[b]; });
    /* mark, rank the marked, cut */
    std::vector<uint32_t> kept, kept_of_group(rg->group_names.size(), 0);
    uint32_t rank = 0;
    for (uint64_t j = 0; j < d.n && !min_spacing; j++) {
      const uint32_t r = order[j];
      if (j == 0 || d.h_group[order[j - 1]] != d.h_group[r]) rank = 0;
      const bool marked = d.h_elig[r] && (!filter || d.h_spec[r] >= min_specificity);
      if (marked && (!per_region || rank < per_region)) {
        kept.push_back(r);
        kept_of_group[d.h_group[r]]++;
      }
      if (marked) rank++;
    }
    /* with a minimum spacing: the walk of gs_select_scan.h over every group's stretch of the order */
    for (uint64_t b = 0, e = 0; b < d.n && min_spacing; b = e) {
      const uint32_t g = d.h_group[order[b]];
      for (e = b; e < d.n && d.h_group[order[e]] == g;) e++;
      const uint32_t len = (uint32_t)(e - b);
      std::vector<uint64_t> key(len), list(std::min(len, per_region));
      std::vector<uint8_t> mark(len), keep(len);
      for (uint32_t i = 0; i < len; i++) {
        const uint32_t r = order[b + i];
        key[i] = gs_sl_key(d.h_chr[r], d.h_pos[r], d.h_sense[r], k, P, cut_offset, d.space_start);
        mark[i] = d.h_elig[r] && (!filter || d.h_spec[r] >= min_specificity) ? 1 : 0;
      }
      uint32_t passed = 0, marked = 0;
      kept_of_group[g] = gs_sl_walk(key.data(), mark.data(), len, min_spacing, per_region, list.data(), keep.data(), &passed, &marked);
      for (uint32_t i = 0; i < len; i++)
        if (keep[i]) kept.push_back(order[b + i]);
      d.last_spacing[0] += passed;
      if (kept_of_group[g] < per_region && marked >= per_region) d.last_spacing[1]++;
    }
    if (report) {
      ds_group_tally(&d, kept.size(), kept_of_group, per_region);
      for (int i = 0; i < 4; i++) report[i] = d.last[i];
      report[4] = d.last_spacing[0];
      report[5] = d.last_spacing[1];
    }
    std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new gs_kmers(), km_release);
    gs_kmers *km = own.get();
    km->device = -1;
    km->k = k;
    km->P = P;
    km->n = kept.size();
    km->have_ids = km->ids_fixed = km->have_host = km->have_host_ids = true;
    std::string text;
    km->h_id_off.push_back(0);
    for (uint32_t r : kept) {
      const uint8_t *s = seqs[src_part[r]] + (size_t)src_cand[r] * k;
      km->h_seqs.insert(km->h_seqs.end(), s, s + k);
      km->h_pams.insert(km->h_pams.end(), pam, pam + P);
      km->h_pos.push_back(d.h_pos[r]);
      km->h_sense.push_back(d.h_sense[r]);
      km->h_sense01.push_back(d.h_sense[r] == '+' ? 1 : 0);
      const std::string &chr = rg->chr_names[d.h_chr[r]];
      const std::string id = std::string(prefix) + rg->group_names[d.h_group[r]] + ":" + chr + ":" + std::to_string(d.h_pos[r]) + ":" +
                             (char)d.h_sense[r];
      km->h_ids.insert(km->h_ids.end(), id.begin(), id.end());
      km->h_id_off.push_back(km->h_ids.size());
      if (rows)
        text += id + "," + std::string((const char *)s, k) + "," + pam + "," + chr + "," + std::to_string(d.h_pos[r]) + "," +
                (char)d.h_sense[r] + "\n";
    }
    km->id_bytes = km->h_ids.size();
    if (rows) {
      *rows = (char *)malloc(text.size() + 1);
      if (!*rows) return GS_ERR_NOMEM;
      memcpy(*rows, text.c_str(), text.size() + 1);
      if (rows_len) *rows_len = text.size();
    }
    *out = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_debug_design_host(const gs_regions *rg, uint32_t n_parts, const uint32_t *chr_index, const uint64_t *n,
                                          const uint8_t *const *seqs, const uint32_t *const *positions, const uint8_t *const *senses,
                                          const float *const *specificity, const uint8_t *const *eligible, const char *pam, uint32_t k,
                                          const char *prefix, uint32_t per_region, float min_specificity, gs_kmers **out, char **rows,
                                          uint64_t *rows_len) {
  return ds_host_model(rg, n_parts, chr_index, n, seqs, positions, senses, specificity, eligible, pam, k, prefix, per_region,
                       min_specificity, 0, 0, 0, out, rows, rows_len, nullptr);
}

extern "C" gs_status gs_debug_design_host_spaced(const gs_regions *rg, uint32_t n_parts, const uint32_t *chr_index, const uint64_t *n,
                                                 const uint8_t *const *seqs, const uint32_t *const *positions,
                                                 const uint8_t *const *senses, const float *const *specificity,
                                                 const uint8_t *const *eligible, const char *pam, uint32_t k, const char *prefix,
                                                 uint32_t per_region, float min_specificity, uint32_t min_spacing, uint32_t cut_offset,
                                                 uint32_t flags, gs_kmers **out, char **rows, uint64_t *rows_len, uint64_t *report) {
  return ds_host_model(rg, n_parts, chr_index, n, seqs, positions, senses, specificity, eligible, pam, k, prefix, per_region,
                       min_specificity, min_spacing, cut_offset, flags, out, rows, rows_len, report);
}
