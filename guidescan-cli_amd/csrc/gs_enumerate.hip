/*
 * gs_enumerate.hip -- the batch pipeline on the host: gs_enumerate_device and what it launches, in order, as stages over
 * one batch state (prepare, seeding plan, literal-N windows, arena, search pass, item ordering, overflow redo, ordering of
 * the set, finish), workspace and arena policy, the fall-backs.  Kernels: gs_search.hip, gs_order.hip, gs_bigorder.hip
 * (and its host side), gs_tileorder.hip.
 */
#include "gs_kernels.h"
#include "gs_scratch.h"

/* gs_seed.hip (launched here behind k_prepare; gs_estimate_heavy is its stand-alone form) */
__global__ void k_estimate_heavy(const gs_guide_rec *guides, uint32_t n, const uint4 *ptab0, const uint4 *ptab1, uint32_t k,
                                 uint32_t thresh, uint32_t *out);

#include <cmath>

/* ---- host side of the pipeline ---------------------------------------------- */
/* the batch shape the handle's per-budget memory (gs_index::seen) was measured on */
static uint64_t shape_key(uint32_t L, uint32_t P, uint32_t n_alt, uint32_t flags) {
  return ((uint64_t)L << 32) | ((uint64_t)P << 16) | (n_alt << 8) | (flags & GS_FLAG_PAM_AT_START);
}

/* The switches the pipeline reads (INTEGRATION.md lists them), parsed once per call with their clamps and defaults.
 * (The device-wide ordering's own, GS_BIG2_*, are read in gs_bigorder.hip.) */
struct switches {
  bool debug, no_form_estimate, no_bidir, no_pairtab, no_deep, no_spec, no_cand_buckets, no_tile_order, no_arena;
  bool dbg_share_timeout;
  uint32_t share_min, share_max;
  uint32_t max_pt;                    /* GS_PAIRTABS */
  bool has_deep_symbols;
  uint32_t deep_symbols;
  uint32_t n_astar, astar[8];         /* GS_ASTAR: experiments, "2,2,1,1" */
  double pairtab_reserve;             /* bytes */
  bool has_index_budget;
  double index_budget;                /* bytes */
  uint32_t cand_from;
  bool has_arena_chunks;
  uint64_t arena_chunks;
  bool has_slot_cap;
  double slot_cap;
  uint64_t search_take, share_queue;  /* 0: not set */
  uint32_t max_iter, v_max, dbg_skip, cnt_shift, split_from, seed_sort_from, seed_opt, seed_take, wide_from;
  int heavy, split_share, seed_form;  /* -1: not set */
  bool seed_spaced;                   /* GS_SEED_SPACED: the seeding launches read the spaced tables (0: off) */
  uint32_t spaced_from;               /* GS_SPACED_FROM: recipes of the class from which a spaced table is worth its memory */
};
static switches read_switches(const gs_index *ix) {
  auto has = [&](const char *k) { return gs_opt(ix, k) != nullptr; };
  auto num = [&](const char *k, long dflt) { const char *e = gs_opt(ix, k); return e ? atol(e) : dflt; };
  switches w;
  w.debug = has("GS_DEBUG");
  w.no_form_estimate = has("GS_NO_FORM_ESTIMATE");
  w.no_bidir = has("GS_NO_BIDIR");
  w.no_pairtab = has("GS_NO_PAIRTAB");
  w.no_deep = has("GS_NO_DEEP");
  w.no_spec = has("GS_NO_SPEC");
  w.no_cand_buckets = has("GS_NO_CAND_BUCKETS");
  w.no_tile_order = has("GS_NO_TILE_ORDER");
  w.no_arena = has("GS_NO_ARENA");
  w.dbg_share_timeout = has("GS_DBG_SHARE_TIMEOUT");
  w.share_min = has("GS_SHARE_MIN") ? (uint32_t)std::max(0l, num("GS_SHARE_MIN", 0)) : ix->opt_share_min;
  w.share_max = has("GS_SHARE_MAX") ? (uint32_t)std::max(128l, num("GS_SHARE_MAX", 0)) : ix->opt_share_max;
  w.max_pt = has("GS_PAIRTABS") ? std::min(2u, (uint32_t)num("GS_PAIRTABS", 0)) : 2u;
  w.has_deep_symbols = has("GS_DEEP_SYMBOLS");
  w.deep_symbols = w.has_deep_symbols ? (uint32_t)atoi(gs_opt(ix, "GS_DEEP_SYMBOLS")) : 0u;
  w.n_astar = 0;
  if (const char *e = gs_opt(ix, "GS_ASTAR"))
    for (const char *p = e; *p && w.n_astar < 8; w.n_astar++) {
      w.astar[w.n_astar] = (uint32_t)strtoul(p, (char **)&p, 10);
      if (*p == ',') p++;
    }
  w.pairtab_reserve = has("GS_PAIRTAB_RESERVE_GB") ? atof(gs_opt(ix, "GS_PAIRTAB_RESERVE_GB")) * 1e9 : 64e9;
  w.has_index_budget = has("GS_INDEX_BUDGET_GB");
  w.index_budget = w.has_index_budget ? atof(gs_opt(ix, "GS_INDEX_BUDGET_GB")) * 1e9 : 0.0;
  w.cand_from = (uint32_t)num("GS_CAND_BUCKETS_FROM", 256);
  w.has_arena_chunks = has("GS_ARENA_CHUNKS");
  w.arena_chunks = w.has_arena_chunks ? (uint64_t)atoll(gs_opt(ix, "GS_ARENA_CHUNKS")) : 0u;
  w.has_slot_cap = has("GS_SLOT_CAP");
  w.slot_cap = w.has_slot_cap ? atof(gs_opt(ix, "GS_SLOT_CAP")) : 0.0;
  w.search_take = has("GS_SEARCH_TAKE") ? (uint64_t)std::max(1l, num("GS_SEARCH_TAKE", 0)) : 0u;
  w.share_queue = has("GS_SHARE_QUEUE") ? (uint64_t)std::max(1ll, atoll(gs_opt(ix, "GS_SHARE_QUEUE"))) : 0u;
  w.max_iter = has("GS_SEARCH_MAX_ITER") ? (uint32_t)num("GS_SEARCH_MAX_ITER", 0) : (1u << 26);
  w.v_max = VERIFY_MAX_DEFAULT;
  if (has("GS_VERIFY_MAX")) {
    const long v = num("GS_VERIFY_MAX", 0);
    w.v_max = v < 1 ? 1u : v > 1023 ? 1023u : (uint32_t)v;
  }
  w.dbg_skip = (uint32_t)num("GS_DBG_SKIP", 0);
  w.cnt_shift = has("GS_COUNT_SHIFT") ? (uint32_t)std::min(12l, std::max(4l, num("GS_COUNT_SHIFT", 0))) : 6u;
  w.split_from = has("GS_SPLIT_FROM") ? (uint32_t)num("GS_SPLIT_FROM", 0) : (1u << 19);
  w.seed_sort_from = has("GS_SEED_SORT_FROM") ? (uint32_t)num("GS_SEED_SORT_FROM", 0) : 4096u;
  w.seed_opt = (uint32_t)num("GS_SEED_OPT", 0);
  w.seed_take = has("GS_SEED_TAKE") ? (uint32_t)std::max(1l, num("GS_SEED_TAKE", 0)) : 1u;
  w.wide_from = has("GS_ORDER_WIDE_FROM") ? (uint32_t)num("GS_ORDER_WIDE_FROM", 0) : 1024u;
  w.heavy = has("GS_HEAVY") ? (num("GS_HEAVY", 0) != 0 ? 1 : 0) : -1;
  w.split_share = has("GS_SPLIT_SHARE") ? (int)std::min(3l, std::max(0l, num("GS_SPLIT_SHARE", 0))) : -1;
  w.seed_form = has("GS_SEED_FORM") ? (int)std::min(2l, std::max(0l, num("GS_SEED_FORM", 0))) : -1;
  w.seed_spaced = num("GS_SEED_SPACED", 1) != 0;
  w.spaced_from = has("GS_SPACED_FROM") ? (uint32_t)std::max(1l, num("GS_SPACED_FROM", 0)) : 256u;
  return w;
}

/* slots per (guide, strand) of the first pass.  Up to three mismatches: 64 and the overflow redo
 * takes the tail.  Beyond: from the mean count the previous batch at this budget showed on this
 * index (Poisson-like on a repeat-free genome: mean + 8 sigma), else from the expected count of a
 * uniform genome: sites x sum_k C(L,k) 3^k / 4^L x PAM share.  Whatever does not fit is redone
 * with exact sizes, so a wrong guess costs time, not hits. */
static uint32_t choose_cap(const gs_index *ix, const switches &sw, uint32_t m, uint32_t L, uint32_t P, uint32_t n_alt,
                           uint32_t flags) {
  if (m <= 3) return 64;
  double mean = -1, seen_max = 0;
  if (m < 8 && ix->seen[m].mean >= 0 && ix->seen[m].key == shape_key(L, P, n_alt, flags)) {
    mean = ix->seen[m].mean;
    seen_max = ix->seen[m].max;
  }
  if (mean < 0) {
    double v = 0, c = 1;
    for (uint32_t k = 0; k <= m && k <= L; k++) {
      v += c;
      c = c * 3.0 * (L - k) / (k + 1);
    }
    for (uint32_t i = 0; i < L; i++) v /= 4.0;
    mean = v * (double)ix->strand[0].n * (n_alt + 1) / (P >= 2 ? 16.0 : P == 1 ? 4.0 : 1.0) * 1.3;
  }
  /* counts spread wider than Poisson (base composition of the guide): half again the mean on
   * top, and the largest count the last batch showed unless a repeat-derived guide made it huge */
  double want = 1.5 * mean + 8.0 * sqrt(mean > 1 ? mean : 1) + 64;
  if (seen_max > want) want = seen_max * 1.05 < 3.0 * mean + 64 ? seen_max * 1.05 : 3.0 * mean + 64;
  if (sw.has_slot_cap) want = sw.slot_cap;
  uint32_t cap = 64;
  while (cap < want && cap < 256) cap <<= 1;
  if (want > 256) cap = (uint32_t)((want + 255) / 256) * 256;
  if (cap > (1u << 20)) cap = 1u << 20;
  return cap;
}

int gs_num_cus(int device) {
  /* asked once per device: hipGetDeviceProperties fills a kilobyte-sized struct through the driver every time it is called,
   * and every enumerate and score call wants this one number */
  static std::atomic<int> cached[64];
  if (device >= 0 && device < 64) {
    const int c = cached[device].load(std::memory_order_relaxed);
    if (c > 0) return c;
  }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) {
    (void)hipGetLastError();
    return 256;
  }
  const int n = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  if (device >= 0 && device < 64) cached[device].store(n, std::memory_order_relaxed);
  return n;
}

/* The form estimate's threshold (k_estimate_heavy): a guide whose own k-mer heads an interval of 8 x share_min rows or more
 * sits in a repeat family.  Saturates: a share_min from 2^28 on asks for 2^31 rows, not for a product that wraps. */
static uint32_t estimate_thresh(uint32_t share_min) { return 8u * std::min(share_min, 1u << 28); }

/* ---- the search's form: a pure function of the pass, the estimate and what the last batch showed ---- */
struct form_in {
  uint32_t items, cus, share_min, backoff; /* backoff: the handle's at the pass's start (the main pass counts it down first) */
  bool main, walk, one_chunk, counting, spec;
  uint32_t m;
  uint32_t est[2];                 /* the estimate's words (0 when it did not run) */
  uint64_t last_hpass, last_items; /* the last batch of the same shape (0: none) */
  int heavy, split_share, seed_form; /* switches, -1: not set */
  uint32_t split_from;
};
struct form_out {
  bool want_estimate;
  uint32_t est_thresh;
  bool heavy;
  uint32_t split;     /* 2: the launch without items on a second stream; 1: behind the first; 3: before it (tests) */
  uint32_t seed_form; /* the two-launch seeding form: 0 off, 1 descriptors, 2 descriptors with the guides scheduled */
  uint32_t form;      /* gs_index_last_sharing: 0 plain, 1 heavy, 2 split, 3 two seeding launches */
};
/* Three forms.  Plain: every item with its wave.  Heavy, one launch (GS_HEAVY=1): heavy verification passes are
 * published and the waves that ran out of items run them - the second level of the verification four rows per lane; twice the
 * code, registers in scratch: 32 ms against 22 on 1 M guides of a genome without repeat families.  Split (GS_SPLIT_SHARE=2): the
 * plain form publishes and leaves (+4 % on that batch), the heavy form - no items of its own - runs the packages in a launch
 * of the lowest priority beside it, taking the slots the first launch's waves leave.  By itself a handle picks from what the
 * last batch of the same shape showed (gs_search_args::hpass): no heavy pass - plain; one per sixteen items, or any in a
 * batch of at most 64 items per wave slot - heavy (a repeat-rich batch: 9.3 ms per 20,000 guides against 9.7 split, 16.2
 * plain); fewer - split (1 M light guides + 8 of an Alu-like family, 650,000 hits each: 26.7 ms against 33.6 plain, 32.7 heavy).
 * Which form also comes from THIS batch: the guides whose own k-mer heads an interval of 8 x share_min rows or more in a strand
 * table sit in a repeat family, their items are the ones with heavy passes (k_estimate_heavy: one table read per guide and
 * strand, 20 us); a guide a substitution away from a family's consensus has heavy passes without a heavy k-mer of its own. */
static form_out choose_form(const form_in &in) {
  form_out f;
  /* heavy items shared among waves (gs_search_args::shq): table-seeded kernels with the arena, one PAM pass; a handle whose
   * sharing launch was not resident as a whole backs off for 64 batches (counted down by the main pass), then tries again */
  const uint32_t backoff = in.main && in.backoff != 0 ? in.backoff - 1 : in.backoff;
  const bool share_ok = in.main && !in.walk && in.one_chunk && !in.counting && in.share_min != 0 && backoff == 0;
  f.want_estimate = share_ok;
  f.est_thresh = estimate_thresh(in.share_min);
  /* heavy items expected in this batch (each guide counts for two items; the last batch's count scaled to this batch's size) */
  const double hp_last = in.last_hpass != 0 && in.last_items ? (double)in.last_hpass * (double)in.items / (double)in.last_items : 0.0;
  const double hp = std::max(2.0 * (double)in.est[0], hp_last);
  const bool seen = hp >= 1.0;
  const bool dense = seen && (16.0 * hp >= (double)in.items || (uint64_t)in.items <= 64ull * (uint64_t)in.cus * 32u);
  f.heavy = share_ok && dense;
  /* few heavy items in a large batch: the two launches pay only when an item is too large to hide behind the rest of the
   * batch on one wave - the publishing form runs k_search's one-launch kernel, a quarter slower than the two seeding launches
   * on the light guides (1 M light guides + 8 guides of 650,000 hits, the largest k-mer interval 145,000 rows: every item
   * with its wave 24.9 ms, two launches 29.4, profiles/r06_mixed_batch.txt).  From 2^19 rows under one k-mer on (GS_SPLIT_FROM) */
  f.split = share_ok && seen && !dense && in.est[1] >= in.split_from ? 2u : 0u;
  if (in.heavy >= 0) {
    f.heavy = in.heavy != 0 && share_ok;
    f.split = 0u;
  }
  if (in.split_share >= 0) {
    f.split = share_ok ? (uint32_t)in.split_share : 0u;
    if (f.split) f.heavy = false;
  }
  /* the form of a batch whose every pattern has its tables and that shares no item: 0 - k_search_fast_pd (one launch, every item
   * sets itself up), 1 - two launches from descriptors (gs_seed.hip), 2 - ... with the guides scheduled by their symbols */
  /* (budgets beyond four substitutions stay with the one launch: a hit is no longer rare there - 10^4 per guide at m <= 6 -
   * and rebuilding every hit's path from its recipe costs what the descriptors save: 65.0 against 63.1 ms per 20,000
   * guides at m <= 6, 2.6 against 2.6 at m <= 4, profiles/r06_seed_forms_m6.txt) */
  f.seed_form = (in.spec && !f.heavy && !f.split && in.m <= 4u) ? 2u : 0u;
  if (in.seed_form >= 0) f.seed_form = f.seed_form ? (uint32_t)in.seed_form : 0u;
  f.form = f.heavy ? 1u : f.split ? 2u : f.seed_form ? 3u : 0u;
  return f;
}
extern "C" void gs_debug_search_form(const int64_t in[18], uint32_t out[6]) {
  form_in fi;
  fi.items = (uint32_t)in[0];
  fi.cus = (uint32_t)in[1];
  fi.share_min = (uint32_t)in[2];
  fi.backoff = (uint32_t)in[3];
  fi.main = in[4] != 0;
  fi.walk = in[5] != 0;
  fi.one_chunk = in[6] != 0;
  fi.counting = in[7] != 0;
  fi.spec = in[8] != 0;
  fi.m = (uint32_t)in[9];
  fi.est[0] = (uint32_t)in[10];
  fi.est[1] = (uint32_t)in[11];
  fi.last_hpass = (uint64_t)in[12];
  fi.last_items = (uint64_t)in[13];
  fi.heavy = (int)in[14];
  fi.split_share = (int)in[15];
  fi.split_from = (uint32_t)in[16];
  fi.seed_form = (int)in[17];
  const form_out f = choose_form(fi);
  const uint32_t o[6] = {f.want_estimate ? 1u : 0u, f.est_thresh, f.heavy ? 1u : 0u, f.split, f.seed_form, f.form};
  memcpy(out, o, sizeof(o));
}

/* ---- one batch: what the stages below read and leave ---- */
struct batch {
  gs_index *ix;
  hipStream_t st;
  switches sw;
  /* the shape */
  const void *d_guides, *d_guide_pams;
  uint64_t n;
  uint32_t n32, L, P, m, flags;
  std::string alt_kept;  /* the alt PAMs of the fast path, P symbols each */
  uint32_t n_alt = 0;    /* ... and how many */
  uint32_t n_chunks = 1; /* passes of four PAM patterns */
  uint32_t nb = 0;       /* scan blocks */
  uint32_t cap = 0;      /* slots per item of the main pass */
  bool force_general = false, wide_key = false, table_seeding = false, count_req = false;
  int cus = 0;
  unsigned long long *d_stats = nullptr;
  uint32_t *d_work = nullptr;
  /* k_prepare's readback: PAM-pair histogram (16 = a pattern ends in an N), the form estimate run behind it */
  uint32_t h_pairs[17] = {0};
  uint32_t pre_est[2] = {0, 0};
  bool pre_est_ran = false;
  /* the seeding plan */
  uint32_t v_rem = 0, x_len = 0, deep_kb = 0, n_codes = 0;
  bool bidir = false, deep = false;
  bool spaced_wanted = false; /* the batch's shape allows the spaced lookup: every pattern on pair + deep tables, budget <= 4, the class this strand's and large enough */
  uint32_t astar[8] = {15, 15, 15, 15, 15, 15, 15, 15}, astar_packed = 0xFFFFFFFFu;
  uint32_t n_pt = 0, pt_slot[2] = {0, 0};
  uint32_t n_cand[2] = {0, 0};
  const uint4 *d_cand[2] = {nullptr, nullptr};
  const uint32_t *d_cand_off[2] = {nullptr, nullptr}, *d_cand_ids[2] = {nullptr, nullptr};
  /* the search */
  uint32_t arena_chunks = 0;
  uint64_t arena_fail = 0; /* items of the main pass the arena had no chunk left for */
  uint64_t arena_raw = 0;  /* chunks its waves reserved (theirs, their helpers' partly filled ones, reserves not used up) */
  float ms_search = 0.f;
  unsigned long long h_stats[2] = {0, 0}; /* the main pass: extensions, overflowing items */
  /* the overflow */
  bool big_batch = false;  /* every guide through the device-wide / tile ordering */
  uint32_t n_o = 0, cap2 = 0, n_used = 0;
  bool lds_redo = false;     /* the overflowing guides fit k_order_wg's LDS */
  bool ovf_arena_ok = false; /* their records beyond the slots are in the arena */
  std::vector<uint32_t> ovf_c2; /* exact counts of the overflowing guides' items */
  /* the ordering's outcome (gs_index_last_counters [7]) */
  bool redo_big = false, arena_direct = false; /* arena_direct: the ordering reads the slots and the arena themselves */
  gs_bigorder_out big;
  bool tile_used = false, tile_fell_back = false;
  uint32_t guides_left_out = 0; /* guides with an item beyond the tiles' reach, ordered device-wide by themselves */
  uint64_t total = 0;           /* hits */
};
static const uint32_t LDS_CAP_MAX = 4096; /* k_order_wg: 2 * cap records of 16 bytes in LDS */

/* redo_pos[g] = place of guide g on `list` (0xFFFFFFFF: not on it) */
static gs_status mark_list(batch &b, gs_buffer &redo_pos, const uint32_t *list, uint32_t n_list) {
  GS_TRY(gs_reserve(redo_pos, 4 * ((size_t)b.n + 1)));
  hipLaunchKernelGGL(k_fill_u32, dim3((b.n32 + 255) / 256), dim3(256), 0, b.st, (uint32_t *)redo_pos.p, 0xFFFFFFFFu, b.n32);
  hipLaunchKernelGGL(k_mark_redo, dim3((n_list + 255) / 256), dim3(256), 0, b.st, list, n_list, (uint32_t *)redo_pos.p);
  return GS_OK;
}

/* ---- prepare: the alt-PAM filter, the workspace, k_prepare and the form estimate behind it, one readback ---- */
static gs_status prepare_workspace(batch &b, const char *alt_pams, uint32_t n_alt) {
  gs_index *ix = b.ix;
  b.cap = choose_cap(ix, b.sw, b.m, b.L, b.P, b.P ? n_alt : 0, b.flags);
  GS_TRY(gs_reserve(ix->w_batch.misc, 512));
  /* PAM list = alt PAMs ++ the guide's own (process.hpp:51-56).  An alt PAM with a symbol outside
   * A,C,G,T,N is a literal (index.hpp:130-137): it can only match if the genome holds that symbol -
   * then the whole batch belongs to the general path - and is dropped otherwise. */
  if (b.P)
    for (uint32_t j = 0; j < n_alt; j++) {
      bool plain = true, possible = true;
      for (uint32_t u = 0; u < b.P; u++) {
        const uint8_t c = (uint8_t)alt_pams[j * b.P + u];
        if (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') continue;
        plain = false;
        if (!ix->strand[0].has_sym[c] && !ix->strand[1].has_sym[c]) possible = false;
      }
      if (plain)
        b.alt_kept.append(alt_pams + j * b.P, b.P);
      else if (possible)
        b.force_general = true;
    }
  b.n_alt = b.P ? (uint32_t)(b.alt_kept.size() / b.P) : 0u;
  /* a guide record holds four PAM patterns: longer lists are searched in chunks that append to the
   * same match slots (k_order merges them and drops sequences found twice, as the std::set does) */
  b.n_chunks = (b.n_alt + 1 + 3) / 4;
  const uint64_t n = b.n;
  GS_TRY(gs_reserve(ix->w_batch.grec, sizeof(gs_guide_rec) * (n + 1) * b.n_chunks));
  GS_TRY(gs_reserve(ix->w_batch.flags, n + 16));
  GS_TRY(gs_reserve(ix->w_batch.counts, sizeof(uint32_t) * (2 * n + 2)));
  GS_TRY(gs_reserve(ix->w_batch.nmatch, sizeof(uint32_t) * (n + 1)));
  GS_TRY(gs_reserve(ix->w_batch.nhits, sizeof(uint32_t) * (n + 1)));
  GS_TRY(gs_reserve(ix->w_batch.offsets, sizeof(uint64_t) * (n + 2)));
  b.nb = (b.n32 + SCAN_BLOCK - 1) / SCAN_BLOCK;
  GS_TRY(gs_reserve(ix->w_batch.blocksums, sizeof(uint64_t) * (b.nb + 2)));
  b.d_stats = gs_misc_stats(ix->w_batch.misc.p);
  b.d_work = gs_misc_work(ix->w_batch.misc.p);
  GS_HIP(hipEventRecord(ix->ev[0], b.st));
  GS_HIP(hipMemsetAsync(ix->w_batch.misc.p, 0, 512, b.st));
  return GS_OK;
}
static gs_status launch_prepare(batch &b) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  uint32_t *pair_hist = (uint32_t *)((char *)ix->w_batch.misc.p + MISC_PAIR_HIST);
  for (uint32_t c = 0; c < b.n_chunks; c++) {
    gs_prep_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.guides = (const uint8_t *)b.d_guides;
    pa.guide_pams = (const uint8_t *)b.d_guide_pams;
    for (uint32_t j = 0; j < b.n_alt; j++)
      for (uint32_t u = 0; u < b.P; u++) pa.alt[j][u] = (uint8_t)b.alt_kept[j * b.P + u];
    pa.out = (gs_guide_rec *)ix->w_batch.grec.p + (size_t)c * b.n;
    pa.n_invalid = b.d_work + WK_INVALID;
    pa.flags = (uint8_t *)ix->w_batch.flags.p;
    pa.n = b.n32;
    pa.L = b.L;
    pa.P = b.P;
    pa.n_alt = b.n_alt; /* empty guide PAM drops the alt PAMs: process.hpp:52-53 */
    pa.start = (b.flags & GS_FLAG_PAM_AT_START) ? 1 : 0;
    pa.chunk = c;
    pa.force_invalid = b.force_general ? 1u : 0u;
    pa.pair_hist = pair_hist;
    gs_launch_prepare(pa, st); /* (workgroups of 1,024: one atomic per workgroup and PAM pair) */
  }
  /* the search pass's form estimate (k_estimate_heavy, gs_seed.hip: the guides whose own k-mer heads a giant interval) is
   * launched here, behind the records it reads, so that its two words come back with this stage's readback instead of
   * costing the step a host round trip of their own (25-70 us on this pool's hosts).  Not when the main pass cannot
   * share: the back-off is counted down before it is tested, so from 2 on */
  const uint32_t smin = b.sw.share_min;
  if (b.n_chunks == 1 && smin != 0 && ix->share_backoff <= 1 && ix->pt_k && ix->strand[0].d.ptab && ix->strand[1].d.ptab &&
      !b.sw.no_form_estimate) {
    b.pre_est_ran = true;
    hipLaunchKernelGGL(k_estimate_heavy, dim3((b.n32 + 255) / 256), dim3(256), 0, st, (const gs_guide_rec *)ix->w_batch.grec.p, b.n32,
                       ix->strand[0].d.ptab, ix->strand[1].d.ptab, ix->pt_k, estimate_thresh(smin),
                       b.d_work + WK_SCRATCH2);
  }
  /* guides the fast path does not encode get empty hit lists and a flag; the batch goes on */
  uint32_t h_invalid = 0;
  GS_HIP(hipMemcpyAsync(&h_invalid, b.d_work + WK_INVALID, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(b.h_pairs, pair_hist, sizeof(b.h_pairs), hipMemcpyDeviceToHost, st));
  if (b.pre_est_ran) GS_HIP(hipMemcpyAsync(b.pre_est, b.d_work + WK_SCRATCH2, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  ix->last_unsupported = h_invalid;
  return GS_OK;
}

/* ---- the seeding plan ---- */
/* the slot that holds the PAM-pair tables of `code` at context depth v_rem (-1: none) */
static int pair_slot(const gs_index *ix, uint32_t code, uint32_t v_rem) {
  int s = -1;
  for (int j = 0; j < 2; j++)
    if (ix->pairtab[j].valid && ix->pairtab[j].code == code && ix->pairtab[j].v_rem == v_rem) s = j;
  return s;
}
/* PAM-pair tables for the (at most two) pairs of bases most patterns of this batch end in: b.pt_slot / b.n_pt */
static gs_status place_pair_tables(batch &b, const uint32_t want[2], uint32_t max_pt) {
  gs_index *ix = b.ix;
  gs_status rc;
  const uint32_t n_want = (want[0] < 16 ? 1u : 0u) + (max_pt > 1 && want[1] < 16 ? 1u : 0u);
  const bool frozen = (b.flags & GS_FLAG_NO_NEW_TABLES) != 0; /* use what the handle holds, build nothing */
  /* a pair whose tables did not fit: remembered on the handle, so that later batches do not free and
   * rebuild the first pair's tables every call for nothing (cleared when memory is given back) */
  auto mark_missing = [&]() {
    for (uint32_t i = 0; i < max_pt; i++)
      if (want[i] != 16 && pair_slot(ix, want[i], b.v_rem) < 0) ix->pairtab_nofit |= 1u << want[i];
  };
  for (int round = 0; round < 2; round++) {
    /* round 0: a slot that already holds a pair stays, a missing one takes what is free; when the
     * second pair does not fit next to a first one built with all its copies, round 1 frees both
     * and gives each half of the room (fewer rotated copies each, but both patterns served) */
    b.n_pt = 0;
    bool taken[2] = {false, false};
    uint32_t to_build = 0;
    for (uint32_t i = 0; i < max_pt; i++) {
      if (want[i] == 16) continue;
      const int s = pair_slot(ix, want[i], b.v_rem);
      if (s >= 0) taken[s] = true;
      to_build += s < 0 ? 1u : 0u;
    }
    for (uint32_t i = 0; i < max_pt; i++) {
      if (want[i] == 16) continue;
      int s = pair_slot(ix, want[i], b.v_rem);
      const bool have = s >= 0;
      for (int j = 0; j < 2 && s < 0; j++)
        if (!taken[j]) {
          s = j;
          taken[j] = true;
        }
      if (s < 0) continue;
      if (!have && frozen) continue;
      if ((rc = gs_pairtab_ensure(ix, s, b.v_rem, want[i], frozen ? 31u : ix->rec[ix->rec_cur].a_rot_first,
                                  have ? 1.0 : 1.0 / (double)to_build, b.st)) != GS_OK)
        return rc;
      if (!have && to_build) to_build--;
      if (ix->pairtab[s].valid && b.deep && !(frozen && !ix->pairtab[s].deep) &&
          (rc = gs_pairtab_ensure_deep(ix, s, b.P, b.deep_kb, b.st)) != GS_OK)
        return rc;
      if (ix->pairtab[s].valid) b.pt_slot[b.n_pt++] = s;
    }
    if (b.n_pt == n_want || n_want < 2 || frozen) break;
    if (round == 1) {
      mark_missing();
      break;
    }
    /* round 1 frees a valid first table only when two tables without any rotated copy are known to fit */
    size_t free_b = 0, total_b = 0;
    GS_HIP(hipMemGetInfo(&free_b, &total_b));
    double reserve = b.sw.pairtab_reserve;
    if (reserve > 0.25 * (double)total_b) reserve = 0.25 * (double)total_b;
    double room = (double)free_b + (double)ix->pairtab[0].own.bytes() + (double)ix->pairtab[1].own.bytes() - reserve;
    if (b.sw.has_index_budget) room = std::min(room, b.sw.index_budget - (double)(ix->strand[0].own.bytes() + ix->strand[1].own.bytes()));
    const double one = 2.0 * 8.0 * (double)(1ull << (2 * ix->pt_k)) + 10.0 * 1.5 * ((double)ix->strand[0].n + (double)ix->strand[1].n) / 16.0 +
                       8.0 * (double)(1ull << (2 * ix->pt_k)) + 64e6;
    if (2.0 * one > room) {
      mark_missing();
      break;
    }
    gs_pairtab_free(ix, 0);
    gs_pairtab_free(ix, 1);
  }
  return GS_OK;
}
/* the A* thresholds of two-sided seeding for the current |X| (b.x_len): b.bidir, b.astar, b.astar_packed */
static void plan_thresholds(batch &b, bool pairable) {
  const uint32_t k = b.ix->pt_k, m = b.m;
  const uint32_t nX = b.x_len, nO = k - b.x_len, nR = b.L - k; /* |X|, |O|, |R| */
  /* PAM expansions the other strand enumerates per item (its table holds concrete bases only;
   * a deep table folds the N in: one pass per pattern) */
  double epam = 0;
  const uint32_t np = b.P ? b.n_alt + 1 : 1;
  for (uint32_t j = 0; j < np; j++) {
    double e = 1;
    for (uint32_t u = 0; u < b.P && !b.deep; u++) {
      const char c = j < b.n_alt ? b.alt_kept[j * b.P + u] : 'N'; /* the guides' own PAM: taken as one wildcard pattern */
      if (c == 'N' && (j < b.n_alt || u == 0)) e *= 4;
    }
    epam += e;
  }
  gs_choose_astar(m, nX, nO, nR, epam, b.astar, pairable ? 0.4 : 1.5, b.deep ? 1.6 : 1.9);
  for (uint32_t o = 0; o < b.sw.n_astar; o++) b.astar[o] = b.sw.astar[o];
  bool any_b = false;
  for (uint32_t o = 0; o <= m && o <= nO && o < 8; o++) any_b = any_b || b.astar[o] + o <= m;
  if (any_b) {
    b.bidir = true;
    b.astar_packed = 0;
    for (uint32_t o = 0; o < 8; o++) b.astar_packed |= (b.astar[o] > 15 ? 15u : b.astar[o]) << (4 * o);
  }
}
static gs_status seeding_plan(batch &b) {
  gs_index *ix = b.ix;
  gs_status rc;
  const uint32_t L = b.L, P = b.P;
  /* context verification is possible when what remains after the table depth fits ctx[] */
  if (ix->pt_k >= 4 && ix->pt_k + 1 <= L && !(b.flags & GS_FLAG_FAITHFUL_WALK) && ix->strand[0].d.ctx &&
      ix->strand[1].d.ctx && ix->strand[0].d.ctx16 && ix->strand[1].d.ctx16 && L + P - ix->pt_k <= 16)
    b.v_rem = L + P - ix->pt_k;
  if (b.wide_key && b.v_rem == 0) {
    gs_set_error("match sequences beyond 52 key bits (2L+3P > 52) need the table-seeded search: this index's prefix table is too "
                 "shallow for them (or the reference-order walk was asked for) - gs_enumerate_general carries such sequences as bytes");
    return GS_ERR_UNSUPPORTED;
  }
  /* two-sided seeding (k_search): possible when set X (the first consumed guide symbols, which only
   * this strand's table covers) lies inside the recipes' positions, the PAM fits the table depth and
   * both inverse suffix arrays exist */
  b.table_seeding = ix->pt_k >= 4 && ix->pt_k + 1 <= L && !(b.flags & GS_FLAG_FAITHFUL_WALK);
  const bool two_ok = b.v_rem != 0 && b.m >= 1 && b.v_rem + 1 <= ix->pt_k && P + 1 <= ix->pt_k && ix->pt_k - P <= 21 &&
                      L <= 31 && ix->strand[0].d.isa && ix->strand[1].d.isa && !b.sw.no_bidir;
  /* the pairs of bases the batch's patterns end in (k_prepare's tally), most frequent first */
  uint32_t want[2] = {16, 16};
  for (uint32_t c = 0; c < 16; c++) {
    if (!b.h_pairs[c]) continue;
    b.n_codes++;
    if (ix->pairtab_nofit & (1u << c)) continue; /* its tables did not fit on this handle: not tried again */
    if (want[0] == 16 || b.h_pairs[c] > b.h_pairs[want[0]]) {
      want[1] = want[0];
      want[0] = c;
    } else if (want[1] == 16 || b.h_pairs[c] > b.h_pairs[want[1]]) {
      want[1] = c;
    }
  }
  const uint32_t max_pt = b.sw.max_pt;
  const bool pairable = two_ok && P >= 2 && b.v_rem >= 2 && b.n_codes >= 1 && !ix->pairtab_off && !b.sw.no_pairtab;
  /* deep tables for the other strand's side: every pattern of the batch must have its PAM-pair table */
  b.deep_kb = b.sw.has_deep_symbols ? b.sw.deep_symbols : ix->pt_k - 2; /* guide symbols a deep table is indexed by */
  const uint32_t deep_kb = b.deep_kb;
  bool try_deep = pairable && P == 3 && b.h_pairs[16] == 0 && b.n_codes <= max_pt && deep_kb + P >= ix->pt_k && deep_kb <= 14 &&
                  deep_kb + 2 <= L && L <= deep_kb + 16 && L - deep_kb + 2 <= ix->pt_k && !b.sw.no_deep;
  for (int attempt = 0; attempt < 2; attempt++) {
    b.deep = try_deep;
    b.bidir = false;
    b.n_pt = 0;
    b.x_len = b.deep ? L - deep_kb : b.v_rem;
    if (two_ok) plan_thresholds(b, pairable);
    b.deep = b.deep && b.bidir;
    /* the seed recipes of this (budget, geometry, thresholds): built once per handle and kept */
    if (b.table_seeding && (rc = gs_recipes_for(ix, L, P, b.m, b.x_len, b.bidir ? b.astar : nullptr, b.deep, b.st)) != GS_OK)
      return rc;
    if (b.bidir && pairable && (rc = place_pair_tables(b, want, max_pt)) != GS_OK) return rc;
    if (!try_deep) break;
    bool all_deep = b.deep && b.n_pt == b.n_codes;
    for (uint32_t i = 0; i < b.n_pt; i++) all_deep = all_deep && ix->pairtab[b.pt_slot[i]].deep;
    if (all_deep) break;
    try_deep = false; /* not every pattern has its deep table: plan again with the strand tables on that side */
  }
  /* the spaced tables (gs_pairtab.hip): the class "no substitution in X, all m in O" of this strand's seeds as one lookup per
   * item - for a batch the seeding launches can serve (every pattern on its pair + deep tables, budget <= 4), when the class
   * is this strand's under the thresholds and large enough to be worth a table (540 recipes at k = 14, 108 at k = 13).  Whether
   * the batch may read them is decided here; they are built where the form is known (run_search): a batch that runs the heavy,
   * the split or the one-launch form builds and holds none */
  b.spaced_wanted = false;
  {
    const uint32_t k = ix->pt_k, nO = k > b.x_len ? k - b.x_len : 0u, m = b.m;
    double cls = m <= nO ? 1.0 : 0.0; /* C(|O|, m) 3^m */
    for (uint32_t i = 0; i < m && cls > 0; i++) cls = cls * (nO - i) / (i + 1) * 3.0;
    b.spaced_wanted = b.sw.seed_spaced && b.bidir && b.deep && b.n_pt != 0 && b.n_pt == b.n_codes && b.h_pairs[16] == 0 && m >= 1 &&
                      m <= 4 && b.astar[m] > 0 && b.x_len + 2 <= k && cls >= (double)b.sw.spaced_from;
  }
  /* the strand tables' rotated copies: read by this strand's seeds of items without PAM-pair tables, by the
   * other strand's seeds unless the deep tables take them, by one-sided items - built now if any of that
   * can happen in this batch (a batch whose every pattern has its pair + deep tables reads none) */
  if (b.table_seeding && !(b.bidir && b.deep && b.n_pt != 0 && b.n_pt == b.n_codes && b.h_pairs[16] == 0))
    if ((rc = gs_strand_rot_ensure(ix, b.st)) != GS_OK) return rc;
  return GS_OK;
}

/* ---- literal-N windows ---- */
/* Windows where a literal 'N' of the genome lies under the PAM (index.hpp:139-149) and the guide part is plain A,C,G,T:
 * the other strand's table cannot hold them (its k-mers spell the PAM), so its share of them is reported from this list.
 * Window of strand s, left to right: P PAM symbols (last consumed first), then the guide symbols L-1 .. 0.  Entry = {q lo,
 * q hi, PAM symbols in consumption order (3 bits each, 4 = N), position of the site in the strand's text}. */
static void literal_n_windows(const gs_index *ix, uint32_t L, uint32_t P, std::vector<uint4> cand[2]) {
  const uint32_t W = L + P;
  const uint64_t len = ix->genome_length;
  auto code = [](uint8_t c) -> int { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; };
  for (const gs_nrun &r : ix->nruns_text) {
    auto at = [&](int64_t pos) -> uint8_t { /* forward text around the run */
      if (pos < 0 || (uint64_t)pos >= len) return 0;
      if ((uint64_t)pos < r.start) return r.start - pos <= GS_NRUN_FLANK ? r.left[GS_NRUN_FLANK - (r.start - pos)] : 0;
      if ((uint64_t)pos < r.start + r.len) return 'N';
      const uint64_t o = pos - (r.start + r.len);
      return o < GS_NRUN_FLANK ? r.right[o] : 0;
    };
    const int64_t s0 = (int64_t)r.start, e0 = (int64_t)(r.start + r.len);
    /* forward strand: the run's tail under the window's first P symbols; text offset o < P holds
     * the PAM symbol of consumption step P-1-o */
    for (int64_t i = e0 - (int64_t)P; i < e0; i++) {
      if (i < 0 || (uint64_t)i + W > len) continue;
      bool ok = true;
      uint64_t q = 0;
      uint32_t pc = 0;
      for (uint32_t o = 0; o < W && ok; o++) {
        const uint8_t c = at(i + o);
        if (o < P) {
          ok = c == 'N' || code(c) >= 0;
          if (ok) pc |= (uint32_t)(c == 'N' ? 4 : code(c)) << (3u * (P - 1u - o));
        } else {
          const int cc = code(c);
          ok = cc >= 0;
          if (ok) q |= (uint64_t)cc << (2u * (L - 1u - (o - P)));
        }
      }
      if (ok) cand[0].push_back(make_uint4((uint32_t)q, (uint32_t)(q >> 32), pc, (uint32_t)i));
    }
    /* reverse strand: its window is the forward window read backwards and complemented, so the
     * run's head lies under the forward window's last P symbols; guide symbol t sits at forward
     * offset t, complemented; PAM step u at forward offset L+u, complemented */
    for (int64_t j = s0 + 1 - (int64_t)W; j <= s0 + (int64_t)P - (int64_t)W; j++) {
      if (j < 0 || (uint64_t)j + W > len) continue;
      bool ok = true;
      uint64_t q = 0;
      uint32_t pc = 0;
      for (uint32_t o = 0; o < W && ok; o++) {
        const uint8_t c = at(j + o);
        if (o >= L) {
          ok = c == 'N' || code(c) >= 0;
          if (ok) pc |= (uint32_t)(c == 'N' ? 4 : 3 - code(c)) << (3u * (o - L));
        } else {
          const int cc = code(c);
          ok = cc >= 0;
          if (ok) q |= (uint64_t)(3 - cc) << (2u * o);
        }
      }
      if (ok) cand[1].push_back(make_uint4((uint32_t)q, (uint32_t)(q >> 32), pc, (uint32_t)(len - ((uint64_t)j + W))));
    }
  }
}
/* behind the windows of a strand with many of them: the bucket index by 5-symbol chunks (4 x 1025 offsets, 4 x n places) */
static void window_buckets(const std::vector<uint4> &cand, std::vector<uint32_t> &bidx) {
  const uint32_t nc = (uint32_t)cand.size();
  bidx.assign(4u * 1025u + 4u * (size_t)nc, 0u);
  for (uint32_t c = 0; c < 4; c++) {
    uint32_t *off = bidx.data() + 1025u * c, *ids = bidx.data() + 4u * 1025u + (size_t)c * nc;
    auto val = [&](uint32_t i) { return (uint32_t)((((uint64_t)cand[i].y << 32) | cand[i].x) >> (10u * c)) & 1023u; };
    for (uint32_t i = 0; i < nc; i++) off[val(i) + 1u]++;
    for (uint32_t v = 0; v < 1024; v++) off[v + 1u] += off[v];
    std::vector<uint32_t> cur(off, off + 1024);
    for (uint32_t i = 0; i < nc; i++) ids[cur[val(i)]++] = i;
  }
}
/* The list depends on the text's N runs and on (L, P, whether it is bucketed) only - not on the batch's guides or
 * patterns: the handle keeps the last one it uploaded (a batch of the same shape finds it in place: the host's
 * pass over the runs and three blocking copies were 0.1 ms of every 17 ms step). */
static gs_status upload_windows(batch &b) {
  gs_index *ix = b.ix;
  const bool cand_buckets_ok = !(b.m > 3 || b.L < 20 || b.sw.no_cand_buckets);
  const uint64_t cand_key = (uint64_t)b.L | ((uint64_t)b.P << 8) | ((uint64_t)(cand_buckets_ok ? 1u : 0u) << 16) |
                            ((uint64_t)b.sw.cand_from << 32);
  const bool cand_hit = ix->cand_key == cand_key && ix->w_batch.cand.p != nullptr;
  std::vector<uint4> cand[2];
  std::vector<uint32_t> bidx[2];
  size_t n_bidx[2] = {0, 0};
  if (cand_hit) {
    b.n_cand[0] = ix->cand_n[0];
    b.n_cand[1] = ix->cand_n[1];
    n_bidx[0] = ix->cand_bidx[0];
    n_bidx[1] = ix->cand_bidx[1];
  } else {
    literal_n_windows(ix, b.L, b.P, cand);
    for (uint32_t s = 0; s < 2; s++) {
      b.n_cand[s] = (uint32_t)cand[s].size();
      if (b.n_cand[s] <= b.sw.cand_from || !cand_buckets_ok) continue;
      window_buckets(cand[s], bidx[s]);
      n_bidx[s] = bidx[s].size();
    }
    ix->cand_key = ~0ull; /* (valid again once everything below is in place) */
  }
  if (b.n_cand[0] + b.n_cand[1]) {
    const size_t b_w = 16 * (size_t)(b.n_cand[0] + b.n_cand[1]);
    if (!cand_hit) GS_TRY(gs_reserve(ix->w_batch.cand, b_w + 4 * (n_bidx[0] + n_bidx[1]) + 16));
    uint4 *dc = (uint4 *)ix->w_batch.cand.p;
    if (!cand_hit) {
      if (b.n_cand[0]) GS_HIP(hipMemcpy(dc, cand[0].data(), 16 * (size_t)b.n_cand[0], hipMemcpyHostToDevice));
      if (b.n_cand[1]) GS_HIP(hipMemcpy(dc + b.n_cand[0], cand[1].data(), 16 * (size_t)b.n_cand[1], hipMemcpyHostToDevice));
    }
    b.d_cand[0] = dc;
    b.d_cand[1] = dc + b.n_cand[0];
    uint32_t *di = (uint32_t *)((char *)ix->w_batch.cand.p + b_w);
    for (uint32_t s = 0; s < 2; s++) {
      if (n_bidx[s] == 0) continue;
      if (!cand_hit) GS_HIP(hipMemcpy(di, bidx[s].data(), 4 * n_bidx[s], hipMemcpyHostToDevice));
      b.d_cand_off[s] = di;
      b.d_cand_ids[s] = di + 4u * 1025u; /* chunk c's places: from c * n_cand[s] on */
      di += n_bidx[s];
    }
  }
  if (!cand_hit) {
    ix->cand_n[0] = b.n_cand[0];
    ix->cand_n[1] = b.n_cand[1];
    ix->cand_bidx[0] = n_bidx[0];
    ix->cand_bidx[1] = n_bidx[1];
    ix->cand_key = b.n_cand[0] + b.n_cand[1] ? cand_key : ~0ull; /* (no windows: nothing to keep, nothing to upload) */
  }
  if (b.sw.debug)
    fprintf(stderr, "[gs] two-sided seeding: astar %u,%u,%u,%u,%u,%u,%u,%u over |X|=%u |O|=%u |R|=%u, "
            "literal-N windows %u + %u%s, PAM-pair tables %u%s\n", b.astar[0], b.astar[1], b.astar[2], b.astar[3], b.astar[4],
            b.astar[5], b.astar[6], b.astar[7], b.x_len, ix->pt_k - b.x_len, b.L - ix->pt_k, b.n_cand[0], b.n_cand[1],
            b.d_cand_off[0] || b.d_cand_off[1] ? " (bucketed by 5-symbol chunks)" : "", b.n_pt, b.deep ? " with deep tables" : "");
  return GS_OK;
}

/* ---- overflow arena of the main pass (gs_search_args::arena): sized from what earlier batches on this handle needed;
 * a batch that needs more falls back to the exact-size second pass and leaves a larger arena to the next one ---- */
static void reserve_arena(batch &b) {
  gs_index *ix = b.ix;
  uint64_t want = ix->arena_chunks;
  if (b.sw.has_arena_chunks) want = b.sw.arena_chunks;
  if (b.sw.no_arena) want = 0;
  if (want > (1ull << 21)) want = 1ull << 21; /* 32 GB of records */
  auto reserve = [&]() {
    return gs_reserve(ix->w_batch.arena, sizeof(uint4) * (want << ARENA_SHIFT)) == GS_OK &&
           gs_reserve(ix->w_batch.arena_meta, 16 * want + 64) == GS_OK && gs_reserve(ix->w_batch.nchunk, sizeof(uint2) * (2 * b.n + 2)) == GS_OK &&
           gs_reserve(ix->w_batch.cls, 32 * (2 * b.n + 2)) == GS_OK;
  };
  if (want && !reserve()) {
    /* no room: give back what only the paths without the arena use (the exact-size array of a second
     * pass, the ordered copy that otherwise lives in the arena, the raw-key sort word) and try again */
    (void)hipGetLastError();
    gs_buffer_free(ix->w_batch.slots2);
    gs_buffer_free(ix->w_big.s);
    if (!reserve()) {
      (void)hipGetLastError();
      want = 0; /* the second pass serves the overflowing guides */
    }
  }
  b.arena_chunks = (uint32_t)want;
}

/* ---- the search pass ---- */
struct search_pass {
  const gs_guide_rec *guides;
  uint32_t ng;
  uint4 *slots;
  uint32_t *counts;
  uint32_t cap;
  const uint64_t *slot_off; /* the exact-size redo: the items' places in slots */
  bool with_arena;          /* the main pass */
};
static void fill_search_args(const batch &b, const search_pass &p, gs_search_args &sa) {
  const gs_index *ix = b.ix;
  memset(&sa, 0, sizeof(sa));
  sa.sd[0] = ix->strand[0].d;
  sa.sd[1] = ix->strand[1].d;
  sa.slots = p.slots;
  sa.slot_off = p.slot_off;
  sa.counts = p.counts;
  sa.work = b.d_work;
  sa.stats = b.d_stats;
  sa.n_items = 2 * p.ng;
  sa.L = b.L;
  sa.P = b.P;
  sa.m = b.m;
  sa.cap = p.cap;
  if (p.with_arena) {
    sa.arena = (uint4 *)ix->w_batch.arena.p;
    sa.arena_next = b.d_work + WK_ARENA_NEXT;
    sa.chunk_item = (uint32_t *)ix->w_batch.arena_meta.p;
    sa.chunk_seq = sa.chunk_item + b.arena_chunks;
    sa.nchunk = (uint2 *)ix->w_batch.nchunk.p;
    sa.cls = (uint32_t *)ix->w_batch.cls.p;
    sa.arena_chunks = b.arena_chunks;
    sa.chunk_fill = sa.chunk_item + 2 * (size_t)b.arena_chunks;
  }
  /* items per visit to the work counter: enough to keep the counter far from its ~88 visits per microsecond,
   * few enough that every resident wave still gets several visits (balance at the tail) */
  const uint64_t waves = (uint64_t)b.cus * 32u;
  uint64_t take = (2ull * p.ng) / (waves * 64u); /* 2 M items: 3 (23.8 ms against 26.4 one at a time; 8: 24.4, 64: 26.2) */
  take = take < 1 ? 1 : take > 4 ? 4 : take;
  if (b.sw.search_take) take = b.sw.search_take;
  sa.take = (uint32_t)take;
  sa.max_iter = b.sw.max_iter;
  sa.err = b.d_work + WK_SEARCH_ERR;
  sa.hpass = b.d_work + WK_HPASS;
  sa.v_max = b.sw.v_max;
  sa.dbg_skip = b.sw.dbg_skip;
  sa.cnt_shift = b.sw.cnt_shift;
  sa.astar = 0xFFFFFFFFu;
  if (b.table_seeding) {
    /* seeds = depth-pt_k nodes: variants of the first pt_k-2 query symbols with j <= m
     * substitutions x the two-symbol extensions the remaining budget allows */
    sa.pt_k = ix->pt_k;
    sa.v_rem = b.v_rem;
    sa.x_len = b.x_len;
    sa.bdeep = b.deep ? 1u : 0u;
    const gs_recipe_set &R = ix->rec[ix->rec_cur];
    sa.rec_full = (const uint2 *)R.buf.p;
    sa.n_rec_full = R.n_full;
    if (b.bidir) {
      sa.bidir = 1;
      sa.astar = b.astar_packed;
      sa.rec_a = sa.rec_full + R.n_full;
      sa.n_rec_a = R.n_a;
      sa.rec_b = sa.rec_a + R.n_a;
      sa.n_rec_b = R.n_b;
      sa.rec_a8 = sa.rec_b + R.n_b;
      sa.n_rec_a8 = R.n_a8;
      sa.n_pt = b.n_pt;
      for (uint32_t i = 0; i < b.n_pt; i++) {
        sa.pt[i][0] = ix->pairtab[b.pt_slot[i]].d[0];
        sa.pt[i][1] = ix->pairtab[b.pt_slot[i]].d[1];
      }
      for (uint32_t s = 0; s < 2; s++) {
        sa.cand[s] = b.d_cand[s];
        sa.n_cand[s] = b.n_cand[s];
        sa.cand_off[s] = b.d_cand_off[s];
        sa.cand_ids[s] = b.d_cand_ids[s];
      }
    }
  }
  if (sa.dbg_skip & 4u) sa.n_rec_full = sa.n_rec_a = sa.n_rec_b = sa.n_rec_a8 = 0u; /* (experiments: no recipe at all - what an item costs before its first seed) */
}

/* the launch without items of the split form, and the heavy form's helpers run again */
static void launch_helpers(const gs_search_args &sh, uint32_t sh_grid, bool spec, hipStream_t hs) {
  if (spec)
    hipLaunchKernelGGL(k_search_heavy_pd, dim3(sh_grid), dim3(WAVE * SEARCH_WAVES), 0, hs, sh);
  else
    hipLaunchKernelGGL(k_search_heavy, dim3(sh_grid), dim3(WAVE * SEARCH_WAVES), 0, hs, sh);
}
/* the second stream of the split form, made on first use (false: none to be had - the caller's stream serves) */
static bool helper_stream(gs_index *ix) {
  if (ix->st_help) return true;
  int lo = 0, hi = 0;
  hipStream_t hs = nullptr;
  bool ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hipStreamCreateWithPriority(&hs, hipStreamNonBlocking, lo) == hipSuccess;
  for (hipEvent_t &e : ix->ev_help) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  if (ok) {
    ix->st_help = hs;
    return true;
  }
  (void)hipGetLastError();
  if (hs) (void)hipStreamDestroy(hs);
  for (hipEvent_t &e : ix->ev_help) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  return false;
}
struct search_launch {
  bool walk, spec;
  uint32_t grid, seed_grid, heavy_per_cu;
  form_out f;
  gs_search_args sh_args; /* the launch without items (split) */
  uint32_t sh_grid = 0;
};
/* the kernels of one pass: four PAM patterns per launch, appending to the same slots */
static gs_status launch_search(batch &b, const search_pass &p, gs_search_args &sa, search_launch &k) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  const dim3 blk(WAVE * SEARCH_WAVES);
  for (uint32_t c = 0; c < b.n_chunks; c++) {
    sa.guides = p.guides + (size_t)c * p.ng;
    sa.append = c ? 1u : 0u;
    if (c) GS_HIP(hipMemsetAsync(b.d_work + WK_ITEMS, 0, 4, st));
    if (k.walk)
      hipLaunchKernelGGL(k_search_walk, dim3(k.grid), blk, 0, st, sa);
    else if (k.spec && b.count_req && !k.f.seed_form)
      hipLaunchKernelGGL(k_search_count_pd, dim3(k.grid), blk, 0, st, sa);
    else if (k.f.split && sa.shq != nullptr) {
      /* the launch without items: on a stream of the lowest priority beside the search launch (its workgroups get the
       * slots the search launch's waves leave), or behind it on the same stream */
      k.sh_args = sa;
      k.sh_args.helper_only = 1u;
      k.sh_args.work = b.d_work + WK_HELPER_ITEMS; /* a counter that is past the items from the start */
      k.sh_grid = (uint32_t)b.cus * k.heavy_per_cu;
      const bool side = k.f.split == 2u && helper_stream(ix);
      if (side) { /* the queue's control words are zeroed: the other stream may start */
        GS_HIP(hipEventRecord(ix->ev_help[0], st));
        GS_HIP(hipStreamWaitEvent(ix->st_help, ix->ev_help[0], 0));
      }
      if (k.f.split == 3u) launch_helpers(k.sh_args, k.sh_grid, k.spec, st); /* (tests: a launch that comes too early leaves at once, everything is left for the one behind) */
      if (k.spec)
        hipLaunchKernelGGL(k_search_pub_pd, dim3(k.grid), blk, 0, st, sa);
      else
        hipLaunchKernelGGL(k_search_pub, dim3(k.grid), blk, 0, st, sa);
      if (k.f.split != 3u) launch_helpers(k.sh_args, k.sh_grid, k.spec, side ? ix->st_help : st);
      if (side) {
        GS_HIP(hipEventRecord(ix->ev_help[1], ix->st_help));
        GS_HIP(hipStreamWaitEvent(st, ix->ev_help[1], 0));
      }
    } else if (k.spec && sa.shq != nullptr)
      hipLaunchKernelGGL(k_search_heavy_pd, dim3(k.grid), blk, 0, st, sa);
    else if (sa.shq != nullptr)
      hipLaunchKernelGGL(k_search_heavy, dim3(k.grid), blk, 0, st, sa);
    else if (k.f.seed_form) {
      /* the two-launch form (gs_seed.hip): descriptors per guide, the guides scheduled by their last / first symbols,
       * the other strand's seeds + the window list, then this strand's seeds appending */
      gs_search_args sb;
      gs_status r2 = gs_seed_describe(ix, sa, p.ng, k.f.seed_form >= 2u && p.ng >= b.sw.seed_sort_from, st, &sb);
      /* one item per visit: each XCD has its own counter (a sixteenth of the visits one word took), and the items that share
       * a piece of a table are then in flight together */
      sb.seed_opt = b.sw.seed_opt;
      sb.take = b.sw.seed_take;
      if (r2 == GS_OK) r2 = gs_probes_attach(ix, sb, st); /* the probe lists of the recipes, for the copies sb.pt[] hold */
      if (r2 == GS_OK) r2 = gs_seed_launch(sb, k.seed_grid, b.count_req, st);
      if (r2 != GS_OK) return r2;
    } else if (k.spec)
      hipLaunchKernelGGL(k_search_fast_pd, dim3(k.grid), blk, 0, st, sa);
    else if (b.count_req)
      hipLaunchKernelGGL(k_search_count, dim3(k.grid), blk, 0, st, sa);
    else
      hipLaunchKernelGGL(k_search_fast, dim3(k.grid), blk, 0, st, sa);
  }
  return GS_OK;
}
/* close the gaps the helpers left (k_share_fix), then read the counters again: it may add overflowing items */
static gs_status share_fix(batch &b, const search_pass &p, const gs_search_args &sa, gs_misc_readback &rb) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  gs_share_args fa;
  memset(&fa, 0, sizeof(fa));
  fa.ctl = sa.shq_ctl;
  fa.sh_list = sa.sh_list;
  fa.sh_acc = sa.sh_acc;
  fa.counts = p.counts;
  fa.nchunk = sa.nchunk;
  fa.cls = sa.cls;
  fa.chunk_item = sa.chunk_item;
  fa.chunk_seq = sa.chunk_seq;
  fa.chunk_fill = sa.chunk_fill;
  fa.arena_next = b.d_work + WK_ARENA_NEXT;
  fa.slots = p.slots;
  fa.arena = sa.arena;
  fa.dbase = sa.sh_acc + 16 * (size_t)sa.sh_max;
  fa.dir = sa.chunk_item + 3 * (size_t)b.arena_chunks;
  fa.stats = b.d_stats;
  fa.sh_max = sa.sh_max;
  fa.cap = p.cap;
  fa.arena_chunks = b.arena_chunks;
  const uint32_t n_sh = (uint32_t)ix->last_share[0];
  hipLaunchKernelGGL(k_share_scan, dim3(1), dim3(1024), 0, st, fa);
  hipLaunchKernelGGL(k_share_dir, dim3((b.arena_chunks + 255) / 256), dim3(256), 0, st, fa);
  hipLaunchKernelGGL((k_share_fix<SH_SMALLSEG>), dim3(n_sh), dim3(256), 0, st, fa); /* a workgroup per item */
  hipLaunchKernelGGL((k_share_fix<SH_MAXSEG>), dim3(std::min<uint32_t>(n_sh, (uint32_t)b.cus * 3u)), dim3(256), 0, st, fa);
  GS_HIP(hipEventRecord(ix->ev[2], st));
  GS_HIP(hipMemcpyAsync(&rb, b.d_stats, sizeof(rb), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  return GS_OK;
}
/* the queue of shared verification passes (sa.shq stays nullptr when there is no room) */
static gs_status reserve_share_queue(batch &b, const search_pass &p, gs_search_args &sa, uint32_t grid) {
  gs_index *ix = b.ix;
  uint64_t qcap = b.sw.share_queue ? b.sw.share_queue : ix->shq_packages;
  if (qcap > (1ull << 20)) qcap = 1ull << 20; /* 1.2 GB of packages */
  const uint32_t sh_max = std::min<uint32_t>(2 * p.ng, 1u << 18);
  const size_t meta = 512 + 4 * (size_t)qcap + 4 * (size_t)sh_max + 64 * (size_t)sh_max;
  if (gs_reserve(ix->w_batch.shq, 16 * (size_t)SHQ_PKG * qcap) != GS_OK || gs_reserve(ix->w_batch.sh_meta, meta + 4 * ((size_t)sh_max + 2)) != GS_OK) {
    (void)hipGetLastError(); /* no room for the queue: every item stays with its wave */
    return GS_OK;
  }
  uint32_t *d_shctl = (uint32_t *)ix->w_batch.sh_meta.p;
  sa.shq = (uint4 *)ix->w_batch.shq.p;
  sa.shq_ctl = d_shctl;
  sa.shq_ready = d_shctl + 128;
  sa.sh_list = sa.shq_ready + qcap;
  sa.sh_acc = sa.sh_list + sh_max;
  sa.shq_cap = (uint32_t)qcap;
  sa.sh_max = sh_max;
  sa.share_min = b.sw.share_min;
  sa.share_max = std::max(128u, b.sw.share_max);
  sa.n_waves = grid * SEARCH_WAVES;
  sa.sh_prof = b.sw.debug ? 1u : 0u;
  GS_HIP(hipMemsetAsync(d_shctl, 0, meta, b.st));
  if (sa.sh_prof) GS_HIP(hipMemsetAsync(d_shctl + 104, 0xFF, 8, b.st)); /* the minimum's start value */
  return GS_OK;
}
/* the form of this pass (choose_form), with the estimate run when it is wanted and the prepare stage did not bring it */
static gs_status pick_form(batch &b, const search_pass &p, bool walk, bool spec, form_out &f) {
  gs_index *ix = b.ix;
  const gs_index::seen_t &seen = ix->seen[b.m < 8 ? b.m : 0];
  const bool seen_last = b.m < 8 && seen.key == shape_key(b.L, b.P, b.n_alt, b.flags) && seen.hpass != 0;
  form_in fi;
  fi.items = 2 * p.ng;
  fi.cus = (uint32_t)b.cus;
  fi.share_min = b.sw.share_min;
  fi.backoff = ix->share_backoff;
  fi.main = p.with_arena;
  fi.walk = walk;
  fi.one_chunk = b.n_chunks == 1;
  fi.counting = b.count_req;
  fi.spec = spec;
  fi.m = b.m;
  fi.est[0] = fi.est[1] = 0;
  fi.last_hpass = seen_last ? seen.hpass : 0;
  fi.last_items = seen_last ? seen.items : 0;
  fi.heavy = b.sw.heavy;
  fi.split_share = b.sw.split_share;
  fi.seed_form = b.sw.seed_form;
  fi.split_from = b.sw.split_from;
  if (p.with_arena && ix->share_backoff != 0) ix->share_backoff--;
  f = choose_form(fi);
  if (f.want_estimate && !b.sw.no_form_estimate) {
    if (b.pre_est_ran && p.with_arena) { /* (the main pass: estimated behind k_prepare) */
      fi.est[0] = b.pre_est[0];
      fi.est[1] = b.pre_est[1];
    } else {
      const gs_status er = gs_estimate_heavy(ix, p.guides, p.ng, f.est_thresh, b.d_work + WK_SCRATCH2, b.st, fi.est);
      if (er != GS_OK) return er;
    }
    if (b.sw.debug) fprintf(stderr, "[gs] form estimate: %u guides with a heavy k-mer of their own, the largest interval %u rows\n", fi.est[0], fi.est[1]);
    f = choose_form(fi);
  }
  ix->last_share[7] = fi.est[0]; /* (gs_index_last_sharing: guides of the batch with a heavy k-mer of their own) */
  return GS_OK;
}
static gs_status run_search(batch &b, const search_pass &p, unsigned long long h_stats[2]) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  GS_HIP(hipMemsetAsync(ix->w_batch.misc.p, 0, 16, st));            /* n_ext, overflow items */
  GS_HIP(hipMemsetAsync(b.d_stats + ST_ARENA_FAIL, 0, 8, st)); /* items the arena failed */
  GS_HIP(hipMemsetAsync(b.d_work + WK_ITEMS, 0, 4, st));
  GS_HIP(hipMemsetAsync(b.d_work + WK_SEARCH_ERR, 0, 4, st));
  GS_HIP(hipMemsetAsync(b.d_work + WK_HPASS, 0, 4, st));
  GS_HIP(hipMemsetAsync(b.d_work + WK_HELPER_ITEMS, 0x80, 4, st)); /* (0x80808080: what a launch without items finds in its work counter) */
  if (p.with_arena) {
    GS_HIP(hipMemsetAsync(b.d_work + WK_ARENA_NEXT, 0, 4, st));
    /* every chunk empty until a wave says whose it is: waves reserve several per visit to the counter (k_search) */
    GS_HIP(hipMemsetAsync((uint32_t *)ix->w_batch.arena_meta.p + b.arena_chunks, 0xFF, 4 * (size_t)b.arena_chunks, st));
    GS_HIP(hipMemsetAsync(ix->w_batch.arena_meta.p, 0, 4 * (size_t)b.arena_chunks, st));
    for (int i = 0; i < 7; i++) ix->last_share[i] = 0; /* (of the main pass: a redo shares nothing) */
  }
  gs_search_args sa;
  fill_search_args(b, p, sa);
  search_launch k;
  /* persistent waves pulling (guide, strand) items: as many 4-wave workgroups per CU as their
   * LDS (verification queue 2.5 KiB + substitution table 1.4 KiB per wave, + 3.5 KiB of stacks in
   * the walking variant) and the registers (8 waves per SIMD = 8 workgroups per CU) allow */
  k.walk = sa.pt_k == 0 || sa.v_rem == 0;
  const size_t lds_wg = sizeof(uint4) * (k.walk ? WAVE_LDS_ENTRIES : WAVE_LDS_FAST) * SEARCH_WAVES;
  uint32_t per_cu = (uint32_t)(160u * 1024u / lds_wg);
  /* every item through PAM-pair + deep tables (no pattern ends in an N, each has its tables): the kernel
   * without the strand tables' side of the seeding */
  k.spec = !k.walk && sa.bidir && sa.bdeep && b.n_pt != 0 && b.n_pt == b.n_codes && b.h_pairs[16] == 0 && !b.sw.no_spec;
  sa.share_min = b.sw.share_min ? b.sw.share_min : 0xFFFFFFFFu; /* (every instantiation counts the passes that large: gs_search_args::hpass) */
  gs_status rc;
  if ((rc = pick_form(b, p, k.walk, k.spec, k.f)) != GS_OK) return rc;
  const bool sharing = k.f.heavy || k.f.split;
  const uint32_t weu = k.walk ? GS_WAVES_EU : k.f.heavy ? GS_WAVES_EU_HEAVY : k.spec ? GS_WAVES_EU_PD : GS_WAVES_EU_FAST;
  if (per_cu > weu) per_cu = weu; /* 4 SIMDs x weu waves = weu four-wave workgroups per CU */
  /* The sharing forms need their whole grid on the chip at once (a helper waits for a package only a resident wave can
   * write): never more workgroups than the runtime says the heavy kernel gets per CU - registers, LDS AND its scratch. */
  k.heavy_per_cu = std::min<uint32_t>((uint32_t)(160u * 1024u / lds_wg), GS_WAVES_EU_HEAVY);
  if (sharing) {
    int occ = 0;
    hipError_t oe = k.spec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_search_heavy_pd, WAVE * SEARCH_WAVES, 0)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_search_heavy, WAVE * SEARCH_WAVES, 0);
    if (oe != hipSuccess) (void)hipGetLastError();
    if (oe == hipSuccess && occ > 0 && (uint32_t)occ < k.heavy_per_cu) k.heavy_per_cu = (uint32_t)occ;
    if (k.f.heavy && per_cu > k.heavy_per_cu) per_cu = k.heavy_per_cu;
  }
  k.grid = (uint32_t)b.cus * per_cu;
  const uint32_t need = (2 * p.ng + SEARCH_WAVES - 1) / SEARCH_WAVES;
  if (k.grid > need) k.grid = need;
  if (b.sw.debug) {
    int occ = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.walk ? k_search_walk : k_search_fast, WAVE * SEARCH_WAVES, 0);
    fprintf(stderr, "[gs] k_search (%s): grid %u x %u threads, LDS %zu B per workgroup, %d workgroups per CU resident\n",
            k.walk ? "walk" : "table", k.grid, WAVE * SEARCH_WAVES, lds_wg, occ);
  }
  if (sharing && (rc = reserve_share_queue(b, p, sa, k.grid)) != GS_OK) return rc;
  const uint32_t *d_shctl = sa.shq_ctl;
  k.seed_grid = 0;
  if (k.f.seed_form) {
    const size_t lds_seed = sizeof(uint4) * SEED_LDS * SEARCH_WAVES;
    k.seed_grid = (uint32_t)b.cus * std::min<uint32_t>((uint32_t)(160u * 1024u / lds_seed), GS_WAVES_EU_SEED);
    if (k.seed_grid > need) k.seed_grid = need;
  }
  if (p.with_arena) ix->last_share[6] = sharing && d_shctl == nullptr ? 0u : k.f.form; /* (gs_index_last_sharing: the form of the main pass) */
  if (p.with_arena) { /* (gs_index_last_launch: what the main pass is launched with) */
    const bool seed_launches = k.f.seed_form != 0u && !k.walk && sa.shq == nullptr; /* (launch_search's branch) */
    const unsigned long long ll[8] = {k.walk ? 1u : 0u, k.spec ? 1u : 0u, sa.bdeep, sa.take, seed_launches ? b.sw.seed_take : 0u, sa.n_pt, sa.x_len,
                                      ix->strand[0].d.ptab_rot ? ix->strand[0].rot_plan_n : 0u};
    memcpy(ix->last_launch, ll, sizeof(ll));
  }
  bool spaced = b.spaced_wanted && k.f.seed_form != 0u && !k.walk && sa.shq == nullptr; /* (launch_search's branch: the two seeding launches) */
  if (spaced) { /* the tables of this |X|, |R| on every PAM-pair table of the batch: built here, by the first batch that reads them */
    const bool frozen = (b.flags & GS_FLAG_NO_NEW_TABLES) != 0;
    for (uint32_t i = 0; i < b.n_pt; i++) {
      if (!frozen && !ix->spaced_off && (rc = gs_pairtab_ensure_spaced(ix, b.pt_slot[i], b.x_len, b.L - ix->pt_k, st)) != GS_OK) return rc;
      const gs_pairtab_host &pt = ix->pairtab[b.pt_slot[i]];
      spaced = spaced && pt.spaced && pt.sp_x == b.x_len && pt.sp_g == b.L - ix->pt_k;
      sa.pt[i][0] = pt.d[0];
      sa.pt[i][1] = pt.d[1];
    }
  }
  if (spaced) {
    const gs_recipe_set &R = ix->rec[ix->rec_cur];
    sa.spaced = 1u;
    sa.spaced_ctr = b.d_work + WK_SPACED;
    sa.rec_a8 = sa.rec_a8 + R.n_a8; /* the list without the class the lookup finds */
    sa.n_rec_a8 = (sa.dbg_skip & 4u) ? 0u : R.n_a8s;
  }
  GS_HIP(hipEventRecord(ix->ev[1], st));
  if ((rc = launch_search(b, p, sa, k)) != GS_OK) return rc;
  GS_HIP(hipEventRecord(ix->ev[2], st));
  gs_misc_readback rb; /* the stats and, behind them, the work words */
  uint32_t h_ctl[128] = {0};
  GS_HIP(hipMemcpyAsync(&rb, b.d_stats, sizeof(rb), hipMemcpyDeviceToHost, st));
  if (d_shctl) GS_HIP(hipMemcpyAsync(h_ctl, d_shctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  /* (packages reserved beyond the queue's size were run by their owners: what the helpers could draw is the smaller) */
  if (d_shctl && k.f.split && k.sh_grid != 0u && h_ctl[32] < std::min(h_ctl[0], sa.shq_cap) && rb.work[WK_SEARCH_ERR] == 0u) {
    /* packages nobody ran: the launch without items was on the chip before the one it serves and left (k_search_body's
     * first lines) - again, behind it */
    launch_helpers(k.sh_args, k.sh_grid, k.spec, st);
    GS_HIP(hipEventRecord(ix->ev[2], st));
    GS_HIP(hipMemcpyAsync(&rb, b.d_stats, sizeof(rb), hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(h_ctl, d_shctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_HIP(hipGetLastError());
    ix->last_share[5]++;
  }
  if (d_shctl && sa.sh_prof) {
    const unsigned long long *pr = (const unsigned long long *)(h_ctl + 104);
    const double us = 0.01, nw = (double)sa.n_waves;
    fprintf(stderr, "[gs] heavy launch: %u waves; the last wave left its items after %.0f us, the last exit after %.0f us; per wave: items %.0f us, "
            "helper episodes %.0f us (%.1f episodes), waiting for a package %.0f us; shared items %u, packages %u (queue %u)\n",
            sa.n_waves, us * (double)(pr[1] - pr[0]), us * (double)(pr[2] - pr[0]), us * (double)pr[3] / nw, us * (double)pr[4] / nw,
            (double)pr[6] / nw, us * (double)pr[5] / nw, h_ctl[96], h_ctl[0], sa.shq_cap);
  }
  if (d_shctl) {
    ix->last_share[0] = std::min(h_ctl[96], sa.sh_max); /* shared items */
    ix->last_share[1] = h_ctl[0];                       /* packages reserved */
    ix->last_share[2] = sa.shq_cap;
    ix->last_share[3] = h_ctl[32];                      /* tickets handed out */
    if (!b.sw.share_queue && (uint64_t)h_ctl[0] + h_ctl[0] / 4 + 64 > ix->shq_packages) ix->shq_packages = (uint64_t)h_ctl[0] + h_ctl[0] / 4 + 64;
    if (h_ctl[96] != 0u && rb.work[WK_SEARCH_ERR] == 0u && (rc = share_fix(b, p, sa, rb)) != GS_OK) return rc;
  }
  h_stats[0] = rb.stats[0];
  h_stats[1] = rb.stats[1];
  if (p.with_arena) b.arena_fail = rb.stats[ST_ARENA_FAIL];
  if (p.with_arena) b.arena_raw = rb.work[WK_ARENA_NEXT];
  if (p.with_arena && b.m < 8) { /* the main pass: heavy verification passes per item, for the next batch's choice */
    ix->seen[b.m].hpass = rb.work[WK_HPASS];
    ix->seen[b.m].items = 2 * (uint64_t)p.ng;
  }
  if (sa.shq != nullptr && b.sw.dbg_share_timeout) rb.work[WK_SEARCH_ERR] |= 2u; /* (tests: as if a helping wave had given up) */
  if (rb.work[WK_SEARCH_ERR] != 0u) {
    if ((rb.work[WK_SEARCH_ERR] & 2u) != 0u && sa.shq != nullptr) {
      /* a wave waited ~3 s for a package that was reserved and never written: the launch's waves were not all on the
       * chip together (another process on the device, a profiler holding CUs).  Not a wrong result - none is returned -
       * and not the end of the handle: the caller redoes the batch with every item on its own wave. */
      ix->share_timed_out = true;
      gs_set_error("internal: a wave gave up waiting for a shared verification pass (the launch was not resident as a whole)");
      return GS_ERR_DEVICE;
    }
    gs_set_error("internal: an item of the search passed its iteration bound (GS_SEARCH_MAX_ITER)");
    return GS_ERR_DEVICE;
  }
  float ms = 0.f;
  hipEventElapsedTime(&ms, ix->ev[1], ix->ev[2]);
  b.ms_search += ms;
  return GS_OK;
}

/* ---- k_order / k_locate over one slot array ---- */
static gs_status run_order(const batch &b, uint4 *slots, const uint32_t *counts, uint32_t *nmatch, uint32_t *nhits, uint32_t ng,
                           uint32_t cap_, uint32_t max_item) {
  gs_order_args oa;
  oa.slots = slots;
  oa.counts = counts;
  oa.nmatch = nmatch;
  oa.nhits = nhits;
  oa.stats = b.d_stats;
  oa.n = ng;
  oa.cap = cap_;
  if (cap_ > 128) {
    /* LDS for the largest guide of this pass (2 x the largest item count, as a power of two) */
    uint32_t nmax = 256;
    while (nmax < 2u * max_item && nmax < 2u * cap_) nmax <<= 1;
    const size_t lds = sizeof(uint4) * (size_t)nmax;
    if (lds > 64 * 1024)
      GS_HIP(hipFuncSetAttribute((const void *)k_order_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    uint32_t grid = ng;
    const uint32_t gmax = (uint32_t)b.cus * (uint32_t)(lds > 80 * 1024 ? 1 : lds > 40 * 1024 ? 3 : 6);
    if (grid > gmax) grid = gmax;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_order_wg, dim3(grid), dim3(256), lds, b.st, oa, nmax);
    return GS_OK;
  }
  /* four waves per workgroup (4 KiB per wave at cap 64); eight workgroups per CU resident, twice
   * that many launched so the tail balances */
  const uint32_t ow = ORDER_WAVES;
  const size_t lds = sizeof(uint4) * (2 * (size_t)cap_ + ORDER_SMALL) * ow;
  const uint32_t gsz = gs_lane_group(ng); /* guides a wave takes at a time: a lane each where one record needs no order */
  uint32_t grid = ((ng + gsz - 1) / gsz + ow - 1) / ow;
  const uint32_t gmax = (uint32_t)b.cus * 16u;
  if (grid > gmax) grid = gmax;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(k_order, dim3(grid), dim3(WAVE * ow), lds, b.st, oa);
  return GS_OK;
}
static void run_locate(const batch &b, const uint4 *matches, const uint32_t *nmatch, const uint32_t *gmap, uint32_t ng, uint32_t cap_) {
  const gs_index *ix = b.ix;
  gs_locate_args la;
  la.sd[0] = ix->strand[0].d;
  la.sd[1] = ix->strand[1].d;
  la.matches = matches;
  la.nmatch = nmatch;
  la.offsets = (const uint64_t *)ix->w_batch.offsets.p;
  la.gmap = gmap;
  la.hits = (gs_hit *)ix->w_batch.hits.p;
  la.genome_length = ix->genome_length;
  la.n = ng;
  la.cap = cap_;
  la.v_rem = b.v_rem;
  const size_t lds = sizeof(uint32_t) * (2 * (size_t)cap_ + 1);
  const uint32_t gsz = gs_lane_group(ng);
  hipLaunchKernelGGL(k_locate, dim3((ng + gsz - 1) / gsz), dim3(WAVE), lds, b.st, la);
}

/* ---- main pass, and once more when the arena ran out ---- */
static gs_status main_pass(batch &b) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  gs_status rc;
  GS_TRY(gs_reserve(ix->w_batch.slots, sizeof(uint4) * (size_t)b.cap * 2 * b.n));
  const search_pass p = {(const gs_guide_rec *)ix->w_batch.grec.p, b.n32, (uint4 *)ix->w_batch.slots.p, (uint32_t *)ix->w_batch.counts.p, b.cap,
                         nullptr, b.arena_chunks != 0};
  if ((rc = run_search(b, p, b.h_stats)) != GS_OK) return rc;
  if (b.arena_chunks == 0 || b.arena_fail == 0 || b.sw.has_arena_chunks || b.n_chunks != 1) return GS_OK;
  /* The arena ran out: a handle's first batch on a repeat-rich genome (the arena starts at 64 MB and is sized from
   * what earlier batches needed).  The counts are exact all the same, so the arena this batch needs is known: it is
   * made that large and the main pass runs once more - a second k_search (tens of ms) instead of the exact-size second
   * pass of the overflowing guides and, for them, the device-wide ordering (half a second at 5 x 10^8 records); the
   * per-guide tile ordering then serves this batch like every later one, and allocates its workspace now.  (The second
   * run counts the handle's sharing back-off down once more.) */
  uint32_t *d_need = b.d_work + WK_SCRATCH2, h_need = 0;
  GS_HIP(hipMemsetAsync(d_need, 0, 4, st));
  hipLaunchKernelGGL(k_need_chunks, dim3(std::min<uint32_t>((2 * b.n32 + 255) / 256, 1024u)), dim3(256), 0, st,
                     (const uint32_t *)ix->w_batch.counts.p, 2 * b.n32, b.cap, d_need);
  GS_HIP(hipMemcpyAsync(&h_need, d_need, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  uint64_t want = (uint64_t)h_need + h_need / 4 + (uint64_t)b.cus * 32u * 16u + 64; /* (+ the waves' reserves) */
  if (want > (1ull << 21)) want = 1ull << 21;
  if (want > b.arena_chunks && gs_reserve(ix->w_batch.arena, sizeof(uint4) * (want << ARENA_SHIFT)) == GS_OK &&
      gs_reserve(ix->w_batch.arena_meta, 16 * want + 64) == GS_OK) {
    if (b.sw.debug)
      fprintf(stderr, "[gs] the arena ran out (%u chunks, %u needed): main pass run again with %llu\n", b.arena_chunks, h_need, (unsigned long long)want);
    b.arena_chunks = (uint32_t)want;
    ix->arena_chunks = want;
    b.arena_fail = 0;
    const search_pass p2 = {p.guides, p.ng, p.slots, p.counts, p.cap, nullptr, true};
    return run_search(b, p2, b.h_stats);
  }
  (void)hipGetLastError();
  return GS_OK;
}

/* ---- per-item stats, raw counts, the ordering in LDS of the guides whose records fit their slots ---- */
static gs_status order_items(batch &b) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  GS_HIP(hipMemsetAsync(b.d_stats + ST_MATCHES, 0, 8, st)); /* match counter */
  unsigned long long h_cstat[2] = {0, 0}; /* sum and maximum of this batch's exact per-item counts */
  GS_HIP(hipMemsetAsync(b.d_stats + ST_COUNT_SUM, 0, 16, st));
  hipLaunchKernelGGL(k_count_stats, dim3(std::min<uint32_t>((2 * b.n32 + 1023) / 1024, 256u)), dim3(256), 0, st,
                     (const uint32_t *)ix->w_batch.counts.p, 2 * b.n32, b.d_stats + ST_COUNT_SUM);
  if (b.cap > 128) { /* sizes k_order_wg's LDS; the small-slot path does not wait for it */
    GS_HIP(hipMemcpyAsync(h_cstat, b.d_stats + ST_COUNT_SUM, 16, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
  }
  ix->last_raw_valid = false;
  if (b.flags & GS_FLAG_RAW_COUNTS) { /* before k_order replaces the raw records by the unique ones */
    GS_TRY(gs_reserve(ix->w_batch.raw, 4 * ((size_t)b.n + 1)));
    hipLaunchKernelGGL(k_raw_counts, dim3((b.n32 + 3) / 4), dim3(256), 0, st, (const uint4 *)ix->w_batch.slots.p,
                       (const uint32_t *)ix->w_batch.counts.p, b.n32, b.cap, (uint32_t *)ix->w_batch.raw.p);
    ix->last_raw_valid = true;
  }
  /* every guide through the device-wide sort: slots beyond what LDS orders, and - measured at hg38 size,
   * m <= 5: 96.8 ms per 100 k guides against 105.5 - from 1,024 slots on, where the bitonic network over
   * 16-byte records in LDS costs more than nine radix passes (m <= 4, 512 slots: 32.9 against 35.1, LDS kept) */
  b.big_batch = b.cap > LDS_CAP_MAX || (b.cap >= b.sw.wide_from && (b.wide_key ? gs_tileorder_fits(b.L, b.P, b.m)
                                                                                : gs_bigorder_fits(b.L, b.P, b.m, b.n32)));
  if (b.big_batch) return GS_OK;
  return run_order(b, (uint4 *)ix->w_batch.slots.p, (const uint32_t *)ix->w_batch.counts.p, (uint32_t *)ix->w_batch.nmatch.p, (uint32_t *)ix->w_batch.nhits.p,
                   b.n32, b.cap, (uint32_t)(h_cstat[1] < b.cap ? h_cstat[1] : b.cap));
}

/* ---- the guides whose matches did not fit their slots ---- */
/* the exact-size array of the overflowing guides' items (counts c2): its item offsets go to w_batch.h_off */
static gs_status upload_exact_offsets(batch &b, const std::vector<uint32_t> &c2) {
  gs_index *ix = b.ix;
  std::vector<uint64_t> h_slot_off(2 * (size_t)b.n_o + 1, 0);
  for (size_t i = 0; i < 2 * (size_t)b.n_o; i++) h_slot_off[i + 1] = h_slot_off[i] + c2[i];
  GS_TRY(gs_reserve(ix->w_batch.slots2, sizeof(uint4) * (h_slot_off.back() + 1)));
  GS_TRY(gs_reserve(ix->w_batch.h_off, 8 * h_slot_off.size()));
  GS_HIP(hipMemcpyAsync(ix->w_batch.h_off.p, h_slot_off.data(), 8 * h_slot_off.size(), hipMemcpyHostToDevice, b.st));
  GS_HIP(hipStreamSynchronize(b.st)); /* h_slot_off is a local */
  return GS_OK;
}
/* the overflowing guides' records copied out of the slots and the arena into slots2 (cap2 per item, or exact: dst_off) */
static void arena_gather(const batch &b, const uint64_t *dst_off, uint32_t cap2) {
  const gs_index *ix = b.ix;
  gs_agather_args ga;
  ga.slots = (const uint4 *)ix->w_batch.slots.p;
  ga.arena = (const uint4 *)ix->w_batch.arena.p;
  ga.counts = (const uint32_t *)ix->w_batch.counts.p;
  ga.chunk_item = (const uint32_t *)ix->w_batch.arena_meta.p;
  ga.chunk_seq = ga.chunk_item + b.arena_chunks;
  ga.list = (const uint32_t *)ix->w_batch.ovf_list.p;
  ga.redo_pos = (const uint32_t *)ix->w_big.redo_pos.p;
  ga.dst_off = dst_off;
  ga.dst = (uint4 *)ix->w_batch.slots2.p;
  ga.n_o = b.n_o;
  ga.cap = b.cap;
  ga.cap2 = cap2;
  ga.n_used = b.n_used;
  hipLaunchKernelGGL(k_arena_gather, dim3(2u * b.n_o + b.n_used), dim3(256), 0, b.st, ga);
}
/* exact-size second pass of the guides on the redo list (their counts2 are exact) */
static gs_status redo_exact(batch &b) {
  gs_index *ix = b.ix;
  gs_status rc;
  std::vector<uint32_t> c2(2 * (size_t)b.n_o);
  GS_HIP(hipMemcpy(c2.data(), ix->w_batch.counts2.p, 8 * (size_t)b.n_o, hipMemcpyDeviceToHost));
  if ((rc = upload_exact_offsets(b, c2)) != GS_OK) return rc;
  unsigned long long h2[2] = {0, 0};
  const search_pass p = {(const gs_guide_rec *)ix->w_batch.grec2.p, b.n_o, (uint4 *)ix->w_batch.slots2.p, (uint32_t *)ix->w_batch.counts2.p, 0,
                         (const uint64_t *)ix->w_batch.h_off.p, false};
  if ((rc = run_search(b, p, h2)) != GS_OK) return rc;
  if (h2[1] != 0) {
    gs_set_error("internal: exact-size redo overflowed");
    return GS_ERR_DEVICE;
  }
  return GS_OK;
}
static gs_status overflow_redo(batch &b) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  gs_status rc;
  const uint64_t n = b.n;
  const uint32_t n32 = b.n32, cap = b.cap;
  b.cap2 = cap;
  if (b.h_stats[1] == 0) return GS_OK;
  uint32_t *d_nlist = b.d_work + WK_NLIST;
  GS_TRY(gs_reserve(ix->w_batch.ovf_list, sizeof(uint32_t) * (n + 1)));
  GS_HIP(hipMemsetAsync(d_nlist, 0, 4, st));
  hipLaunchKernelGGL(k_collect_overflow, dim3((n32 + 255) / 256), dim3(256), 0, st,
                     (const uint32_t *)ix->w_batch.counts.p, n32, cap, (uint32_t *)ix->w_batch.ovf_list.p, d_nlist);
  GS_HIP(hipMemcpyAsync(&b.n_o, d_nlist, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  const uint32_t n_o = b.n_o;
  GS_TRY(gs_reserve(ix->w_batch.grec2, sizeof(gs_guide_rec) * (size_t)n_o * b.n_chunks));
  GS_TRY(gs_reserve(ix->w_batch.counts2, sizeof(uint32_t) * 2 * (size_t)n_o));
  GS_TRY(gs_reserve(ix->w_batch.nmatch2, sizeof(uint32_t) * (size_t)n_o));
  GS_TRY(gs_reserve(ix->w_batch.nhits2, sizeof(uint32_t) * (size_t)n_o));
  for (uint32_t c = 0; c < b.n_chunks; c++)
    hipLaunchKernelGGL(k_gather_guides, dim3((n_o + 255) / 256), dim3(256), 0, st,
                       (const gs_guide_rec *)ix->w_batch.grec.p + (size_t)c * n, (const uint32_t *)ix->w_batch.ovf_list.p, n_o,
                       (gs_guide_rec *)ix->w_batch.grec2.p + (size_t)c * n_o);
  /* the main pass counted every item's matches exactly, also beyond its slots */
  hipLaunchKernelGGL(k_gather_counts, dim3((n_o + 255) / 256), dim3(256), 0, st,
                     (const uint32_t *)ix->w_batch.counts.p, (const uint32_t *)ix->w_batch.ovf_list.p, n_o,
                     (uint32_t *)ix->w_batch.counts2.p);
  uint32_t need_cap = 0;
  uint64_t need_chunks = 0;
  std::vector<uint32_t> c2(2 * (size_t)n_o);
  GS_HIP(hipMemcpyAsync(c2.data(), ix->w_batch.counts2.p, 8 * (size_t)n_o, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  for (uint32_t c : c2) {
    need_cap = c > need_cap ? c : need_cap;
    if (c > cap) need_chunks += (c - cap + ARENA_CHUNK - 1u) >> ARENA_SHIFT;
  }
  /* the overflowing items' records beyond their slots are in the arena - unless it ran out (or is off):
   * then these guides are searched once more with slots of the exact sizes, and the next batch gets
   * the arena this one would have needed */
  const bool arena_ok = b.arena_chunks != 0 && b.arena_fail == 0;
  if (b.arena_raw > need_chunks) need_chunks = b.arena_raw; /* (what the waves reserved: a later batch should find as much) */
  if (b.arena_chunks != 0 && !b.sw.has_arena_chunks && need_chunks + need_chunks / 4 + 64 > ix->arena_chunks)
    ix->arena_chunks = need_chunks + need_chunks / 4 + 64;
  if (arena_ok) {
    GS_HIP(hipMemcpyAsync(&b.n_used, b.d_work + WK_ARENA_NEXT, 4, hipMemcpyDeviceToHost, st));
    if ((rc = mark_list(b, ix->w_big.redo_pos, (const uint32_t *)ix->w_batch.ovf_list.p, n_o)) != GS_OK) return rc;
    GS_HIP(hipStreamSynchronize(st));
    if (b.n_used > b.arena_chunks) b.n_used = b.arena_chunks;
  }
  b.lds_redo = !b.big_batch && need_cap <= LDS_CAP_MAX;
  if (b.lds_redo) {
    /* slots every one of these guides fits, ordered in LDS */
    b.cap2 = 128;
    while (b.cap2 < need_cap) b.cap2 <<= 1;
    GS_TRY(gs_reserve(ix->w_batch.slots2, sizeof(uint4) * (size_t)b.cap2 * 2 * n_o));
    if (arena_ok) {
      arena_gather(b, nullptr, b.cap2);
    } else {
      unsigned long long h2[2] = {0, 0};
      const search_pass p = {(const gs_guide_rec *)ix->w_batch.grec2.p, n_o, (uint4 *)ix->w_batch.slots2.p, (uint32_t *)ix->w_batch.counts2.p,
                             b.cap2, nullptr, false};
      if ((rc = run_search(b, p, h2)) != GS_OK) return rc;
      if (h2[1] != 0) {
        gs_set_error("internal: redo pass overflowed slots sized from exact counts");
        return GS_ERR_DEVICE;
      }
    }
    if ((rc = run_order(b, (uint4 *)ix->w_batch.slots2.p, (const uint32_t *)ix->w_batch.counts2.p, (uint32_t *)ix->w_batch.nmatch2.p,
                        (uint32_t *)ix->w_batch.nhits2.p, n_o, b.cap2, need_cap)) != GS_OK)
      return rc;
    hipLaunchKernelGGL(k_patch_overflow, dim3((n_o + 255) / 256), dim3(256), 0, st,
                       (const uint32_t *)ix->w_batch.ovf_list.p, n_o, (const uint32_t *)ix->w_batch.nhits2.p,
                       (uint32_t *)ix->w_batch.nhits.p);
  }
  b.ovf_arena_ok = arena_ok;
  b.ovf_c2.swap(c2);
  return GS_OK;
}

/* ---- the set that LDS does not order: the overflowing guides beyond k_order_wg's reach, or - from 1,024 slots per item
 * on - the whole batch.  Per guide in LDS tiles (gs_tileorder.hip) when k_search counted the classes (arena on) and the
 * sort word fits; the device-wide ordering (gs_bigorder.hip) otherwise, and whenever a tile reports that one of its
 * assumptions did not hold (then everything from the ordering on is done again that way). ---- */
/* (the walking kernel's records are intervals; a batch shape that showed overlapping PAM patterns is remembered) */
static uint64_t tile_key(const batch &b) {
  uint64_t key = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
  mix(b.L);
  mix(b.P);
  mix(b.n_alt);
  mix(b.flags & (GS_FLAG_PAM_AT_START | GS_FLAG_FAITHFUL_WALK));
  for (uint32_t i = 0; i < b.n_alt * b.P; i++) mix((uint8_t)b.alt_kept[i]);
  return key;
}
static gs_status plan_tiles(batch &b, gs_tileorder_in &ti, gs_tileorder_state &ts, bool *usable) {
  gs_index *ix = b.ix;
  gs_status rc;
  if (b.n_o && (rc = mark_list(b, ix->w_big.redo_pos, (const uint32_t *)ix->w_batch.ovf_list.p, b.n_o)) != GS_OK) return rc;
  ti.n_set = b.big_batch ? b.n32 : b.n_o;
  ti.list = b.big_batch ? nullptr : (const uint32_t *)ix->w_batch.ovf_list.p;
  ti.redo_pos = (const uint32_t *)ix->w_big.redo_pos.p;
  ti.counts = (const uint32_t *)ix->w_batch.counts.p;
  ti.cls = (const uint32_t *)ix->w_batch.cls.p;
  ti.slots = (const uint4 *)ix->w_batch.slots.p;
  ti.cap = b.cap;
  ti.arena = (const uint4 *)ix->w_batch.arena.p;
  ti.chunk_item = (const uint32_t *)ix->w_batch.arena_meta.p;
  ti.chunk_seq = ti.chunk_item + b.arena_chunks;
  ti.n_used = b.n_used;
  ti.nhits = (uint32_t *)ix->w_batch.nhits.p;
  ti.L = b.L;
  ti.P = b.P;
  ti.m = b.m;
  ti.v_rem = b.v_rem;
  return gs_tileorder_plan(ix, ti, b.st, ts, usable);
}
static gs_bigorder_in bigorder_in(const batch &b) {
  gs_bigorder_in in;
  memset(&in, 0, sizeof(in));
  in.arena_chunks = b.arena_chunks;
  in.cap = b.cap;
  in.n_used = b.n_used;
  in.L = b.L;
  in.P = b.P;
  in.m = b.m;
  return in;
}
/* the set device-wide: the whole batch (records in the main slots, the redo guides' in the arena or the exact-size
 * array), or the redo list alone */
static gs_status order_device_wide(batch &b) {
  gs_index *ix = b.ix;
  gs_status rc;
  const uint32_t n_set = b.big_batch ? b.n32 : b.n_o;
  const uint32_t *ovf_list = (const uint32_t *)ix->w_batch.ovf_list.p, *redo_pos = nullptr;
  if (b.n_o) {
    if (b.ovf_arena_ok && gs_bigorder_fits(b.L, b.P, b.m, n_set)) {
      b.arena_direct = true; /* no copy at all: the ordering's first kernel reads slots and chunks */
    } else if (b.ovf_arena_ok) {
      /* the exact-size array the second pass would have filled, filled by copies */
      if ((rc = upload_exact_offsets(b, b.ovf_c2)) != GS_OK) return rc;
      arena_gather(b, (const uint64_t *)ix->w_batch.h_off.p, 0u);
    } else if ((rc = redo_exact(b)) != GS_OK) {
      return rc;
    }
    b.redo_big = true;
    if (b.big_batch) {
      if ((rc = mark_list(b, ix->w_big.redo_pos, ovf_list, b.n_o)) != GS_OK) return rc;
      redo_pos = (const uint32_t *)ix->w_big.redo_pos.p;
    }
  }
  gs_bigorder_in in = bigorder_in(b);
  in.n_set = n_set;
  in.counts_main = b.big_batch ? (const uint32_t *)ix->w_batch.counts.p : nullptr;
  in.cap_main = b.big_batch ? b.cap : 0u;
  in.redo_pos = redo_pos;
  in.slot_off2 = (const uint64_t *)ix->w_batch.h_off.p;
  in.counts2 = (const uint32_t *)ix->w_batch.counts2.p;
  in.nmatch = (uint32_t *)(b.big_batch ? ix->w_batch.nmatch.p : ix->w_batch.nmatch2.p);
  in.nhits = (uint32_t *)(b.big_batch ? ix->w_batch.nhits.p : ix->w_batch.nhits2.p);
  in.from_arena = b.arena_direct;
  in.arena_list = b.big_batch ? nullptr : ovf_list;
  if ((rc = gs_bigorder_run(ix, in, b.st, b.big)) != GS_OK) return rc;
  if (!b.big_batch) /* the redo list alone went through the device-wide sort */
    hipLaunchKernelGGL(k_patch_overflow, dim3((b.n_o + 255) / 256), dim3(256), 0, b.st, ovf_list, b.n_o,
                       (const uint32_t *)ix->w_batch.nhits2.p, (uint32_t *)ix->w_batch.nhits.p);
  return GS_OK;
}
/* hit offsets (scan of nhits), the hit array, and the hits of the guides ordered in LDS */
static gs_status scan_and_locate(batch &b) {
  gs_index *ix = b.ix;
  hipStream_t st = b.st;
  hipLaunchKernelGGL(k_scan_partial, dim3(b.nb), dim3(SCAN_BLOCK), 0, st, (const uint32_t *)ix->w_batch.nhits.p,
                     (uint64_t *)ix->w_batch.blocksums.p, b.n32);
  hipLaunchKernelGGL(k_scan_blocksums, dim3(1), dim3(SCAN_BLOCK), 0, st, (uint64_t *)ix->w_batch.blocksums.p, b.nb);
  hipLaunchKernelGGL(k_scan_final, dim3(b.nb), dim3(SCAN_BLOCK), 0, st, (const uint32_t *)ix->w_batch.nhits.p,
                     (const uint64_t *)ix->w_batch.blocksums.p, (uint64_t *)ix->w_batch.offsets.p, b.n32, b.nb);
  b.total = 0;
  GS_HIP(hipMemcpyAsync(&b.total, (uint64_t *)ix->w_batch.offsets.p + b.n, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  GS_TRY(gs_reserve(ix->w_batch.hits, sizeof(gs_hit) * (b.total + 1)));
  if (!b.big_batch) {
    run_locate(b, (const uint4 *)ix->w_batch.slots.p, (const uint32_t *)ix->w_batch.nmatch.p, nullptr, b.n32, b.cap);
    if (b.n_o && b.lds_redo)
      run_locate(b, (const uint4 *)ix->w_batch.slots2.p, (const uint32_t *)ix->w_batch.nmatch2.p, (const uint32_t *)ix->w_batch.ovf_list.p, b.n_o,
                 b.cap2);
  }
  return GS_OK;
}
/* Guides with an item beyond the tiles' reach (10^6 records: a guide inside the largest repeat family of a genome): these
 * alone through the device-wide ordering, their records read where k_search left them; the hit list has their places
 * already (as many hits as records: checked - a difference means one sequence at one row twice, and the batch is then
 * ordered device-wide as a whole, like any batch whose tiles meet that: *viol) */
static gs_status order_left_out(batch &b, const gs_tileorder_state &ts, uint32_t *viol) {
  gs_index *ix = b.ix;
  gs_status rc;
  const uint32_t TO_F_DUP_HOST = 2u; /* (gs_tileorder.hip's TO_F_DUP: one sequence at one row twice) */
  if (b.wide_key || !gs_bigorder_fits(b.L, b.P, b.m, ts.n_excl)) {
    gs_set_error("a guide with more than 10^6 match records per index and a match sequence beyond 52 key bits: the device-wide "
                 "ordering does not carry such keys (gs_enumerate_general does)");
    return GS_ERR_UNSUPPORTED;
  }
  const uint32_t n_x = ts.n_excl;
  const uint32_t *xlist = (const uint32_t *)ix->w_tile.excl.p;
  if ((rc = mark_list(b, ix->w_big.redo_pos2, xlist, n_x)) != GS_OK) return rc;
  GS_TRY(gs_reserve(ix->w_batch.nmatch2, sizeof(uint32_t) * (size_t)std::max(n_x, b.n_o)));
  GS_TRY(gs_reserve(ix->w_batch.nhits2, sizeof(uint32_t) * (size_t)std::max(n_x, b.n_o)));
  if (b.n_used == 0) { /* (the chunks in use, when no earlier step asked for them) */
    GS_HIP(hipMemcpyAsync(&b.n_used, b.d_work + WK_ARENA_NEXT, 4, hipMemcpyDeviceToHost, b.st));
    GS_HIP(hipStreamSynchronize(b.st));
    if (b.n_used > b.arena_chunks) b.n_used = b.arena_chunks;
  }
  gs_bigorder_in in = bigorder_in(b);
  in.n_set = n_x;
  in.nmatch = (uint32_t *)ix->w_batch.nmatch2.p;
  in.nhits = (uint32_t *)ix->w_batch.nhits2.p;
  in.from_arena = true;
  in.arena_list = xlist;
  in.arena_redo_pos = (const uint32_t *)ix->w_big.redo_pos2.p;
  if ((rc = gs_bigorder_run(ix, in, b.st, b.big)) != GS_OK) return rc;
  std::vector<uint32_t> hx(n_x), lx(n_x), cx(2 * (size_t)n_x);
  GS_HIP(hipMemcpy(hx.data(), ix->w_batch.nhits2.p, 4 * (size_t)n_x, hipMemcpyDeviceToHost));
  GS_HIP(hipMemcpy(lx.data(), xlist, 4 * (size_t)n_x, hipMemcpyDeviceToHost));
  bool same = true;
  for (uint32_t j = 0; j < n_x && same; j++) {
    GS_HIP(hipMemcpy(&cx[2 * j], (const uint32_t *)ix->w_batch.counts.p + 2 * (size_t)lx[j], 8, hipMemcpyDeviceToHost));
    same = (uint64_t)hx[j] == (uint64_t)cx[2 * j] + cx[2 * j + 1];
  }
  if (!same) {
    *viol = TO_F_DUP_HOST;
    return GS_OK;
  }
  gs_bigorder_locate(ix, b.big, xlist, b.v_rem, b.st);
  b.guides_left_out = n_x;
  ix->last_share[4] = n_x;
  return GS_OK;
}
static gs_status order_set(batch &b) {
  gs_index *ix = b.ix;
  gs_status rc;
  const bool set_exists = b.big_batch || (b.n_o != 0 && !b.lds_redo);
  const uint64_t key = tile_key(b);
  bool tile = set_exists && b.arena_chunks != 0 && (b.n_o == 0 || b.ovf_arena_ok) && b.v_rem != 0 &&
              gs_tileorder_fits(b.L, b.P, b.m) && !(ix->tile_order_off && ix->tile_order_off_key == key) && !b.sw.no_tile_order;
  for (int attempt = 0; attempt < 2; attempt++) {
    gs_tileorder_in ti;
    gs_tileorder_state ts;
    memset(&ti, 0, sizeof(ti));
    if (set_exists && tile) {
      bool usable = false;
      if ((rc = plan_tiles(b, ti, ts, &usable)) != GS_OK) return rc;
      if (!usable) tile = false;
    }
    if (set_exists && !tile && b.wide_key) {
      gs_set_error("a guide with more matches than LDS orders and a match sequence beyond 52 key bits: the device-wide ordering "
                   "does not carry such keys and the per-guide tile ordering could not take the batch (gs_enumerate_general does)");
      return GS_ERR_UNSUPPORTED;
    }
    if (set_exists && !tile && (rc = order_device_wide(b)) != GS_OK) return rc;
    if ((rc = scan_and_locate(b)) != GS_OK) return rc;
    if (!set_exists) break;
    if (!tile) {
      gs_bigorder_locate(ix, b.big, b.big_batch ? nullptr : (const uint32_t *)ix->w_batch.ovf_list.p, b.v_rem, b.st);
      break;
    }
    ti.offsets = (const uint64_t *)ix->w_batch.offsets.p;
    ti.hits = (gs_hit *)ix->w_batch.hits.p;
    uint32_t viol = 0;
    if ((rc = gs_tileorder_run(ix, ti, ts, b.st, &viol)) != GS_OK) return rc;
    if (!viol && ts.n_excl != 0 && (rc = order_left_out(b, ts, &viol)) != GS_OK) return rc;
    if (!viol) {
      b.tile_used = true;
      return gs_add_matches(ix, ts.n_records); /* these guides were skipped by (or never went through) k_order */
    }
    if (b.sw.debug) fprintf(stderr, "[gs] per-guide tile ordering gave up (flags %u): device-wide ordering instead\n", viol);
    tile = false;
    b.tile_fell_back = true;
    /* overlapping PAM patterns or interval records are a property of the batch's shape: later batches of this handle skip the attempt */
    if (viol & 3u) {
      ix->tile_order_off = true;
      ix->tile_order_off_key = key;
    }
  }
  return GS_OK;
}

/* ---- finish: counters, what the handle remembers of this batch, the outputs ---- */
static gs_status finish(batch &b, const void **d_offsets, const void **d_hits, gs_result_view *stats) {
  gs_index *ix = b.ix;
  GS_HIP(hipEventRecord(ix->ev[3], b.st));
  gs_misc_readback rb; /* the stats and, behind them, the work words: one copy */
  memset(&rb, 0, sizeof(rb));
  unsigned long long *const h_stats3 = rb.stats;
  GS_HIP(hipMemcpyAsync(&rb, b.d_stats, sizeof(rb), hipMemcpyDeviceToHost, b.st));
  GS_HIP(hipStreamSynchronize(b.st));
  for (int i = 0; i < 4; i++) ix->last_spaced[i] = rb.work[WK_SPACED + i];
  if (b.bidir && b.sw.debug)
    fprintf(stderr, "[gs] items: seeded from both strands %llu, one-sided (PAM with more than two N) %llu; slots %u per item, "
            "%u guides redone%s%s\n", h_stats3[4], h_stats3[5], b.cap, b.n_o, b.big_batch ? " (whole batch through the wide ordering)" : "",
            b.tile_used ? " (per guide in LDS tiles)" : "");
  if (b.guides_left_out && b.sw.debug)
    fprintf(stderr, "[gs] %u guide(s) with an item beyond the tiles' reach ordered device-wide by themselves\n", b.guides_left_out);
  h_stats3[6] = b.n_o;
  /* above the flags: items through PAM-pair tables.  Bit 2: the overflowing guides came out of the arena, no second pass;
   * bits 3, 4: ordered by one sort of (word, row bits), runs put right afterwards; bits 5, 6: ordered per guide in LDS
   * tiles, that form gave up and the device-wide one ran */
  h_stats3[7] = (h_stats3[7] << 8) | (b.big_batch ? 1u : 0u) | (b.redo_big ? 2u : 0u) |
                (b.n_o && b.arena_chunks != 0 && b.arena_fail == 0 ? 4u : 0u) | (b.big.comp ? 8u : 0u) | (b.big.fixed ? 16u : 0u) |
                (b.tile_used ? 32u : 0u) | (b.tile_fell_back ? 64u : 0u);
  h_stats3[13] = b.cap;
  memcpy(ix->last_counters, h_stats3, sizeof(rb.stats));
  /* matches per item seen at this budget: sizes the slots of the next batch */
  if (b.m < 8 && b.n32) {
    ix->seen[b.m].mean = (double)h_stats3[14] / (2.0 * b.n32);
    ix->seen[b.m].max = (double)h_stats3[15];
    ix->seen[b.m].key = shape_key(b.L, b.P, b.n_alt, b.flags);
  }
  GS_HIP(hipGetLastError());
  if (d_offsets) *d_offsets = ix->w_batch.offsets.p;
  if (d_hits) *d_hits = ix->w_batch.hits.p;
  if (stats) {
    stats->n_guides = b.n;
    stats->n_ext = b.h_stats[0];
    stats->n_hits = b.total;
    stats->guide_offsets = nullptr;
    stats->hits = nullptr;
    stats->n_matches = h_stats3[ST_MATCHES];
    stats->ms_search = b.ms_search;
    float ms = 0.f;
    hipEventElapsedTime(&ms, ix->ev[0], ix->ev[3]);
    stats->ms_total = ms;
  }
  return GS_OK;
}

static gs_status enumerate_device_impl(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L, const void *d_guide_pams,
                                       uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                       void *stream, const void **d_offsets, const void **d_hits, gs_result_view *stats) {
  if (!ix || (!d_guides && n) || (P && !d_guide_pams && n) || (n_alt && !alt_pams))
    return GS_ERR_ARG;
  if (n >= (1ull << 31)) return GS_ERR_ARG;
  if (L < 1 || L > 31 || P > 8 || 2 * L + 3 * P > 59 || mismatches > 7 || n_alt > 31) {
    gs_set_error("device path supports 1<=L<=31, P<=8, 2L+3P<=59, mismatches<=7, <=31 alt PAMs");
    return GS_ERR_UNSUPPORTED;
  }
  batch b;
  b.ix = ix;
  b.st = (hipStream_t)stream;
  b.sw = read_switches(ix);
  b.d_guides = d_guides;
  b.d_guide_pams = d_guide_pams;
  b.n = n;
  b.n32 = (uint32_t)n;
  b.L = L;
  b.P = P;
  b.m = mismatches;
  b.flags = flags;
  b.wide_key = 2 * L + 3 * P > 52; /* beyond what the walking kernel and the device-wide ordering carry */
  b.count_req = (flags & GS_FLAG_COUNT_REQUESTS) != 0;
  GS_HIP(hipSetDevice(ix->device));
  ix->last_unsupported = 0;
  ix->tx_n = 0; /* the last text and its per-guide offsets do not outlive the next batch */
  for (int i = 0; i < 4; i++)
    if (!ix->ev[i]) GS_HIP(hipEventCreate(&ix->ev[i]));
  gs_status rc;
  if ((rc = prepare_workspace(b, alt_pams, n_alt)) != GS_OK) return rc;
  if (n == 0) {
    GS_HIP(hipMemsetAsync(ix->w_batch.offsets.p, 0, sizeof(uint64_t), b.st));
    GS_HIP(hipStreamSynchronize(b.st));
    if (d_offsets) *d_offsets = ix->w_batch.offsets.p;
    if (d_hits) *d_hits = ix->w_batch.hits.p;
    if (stats) memset(stats, 0, sizeof(*stats));
    return GS_OK;
  }
  if ((rc = launch_prepare(b)) != GS_OK) return rc;
  b.cus = gs_num_cus(ix->device);
  if ((rc = seeding_plan(b)) != GS_OK) return rc;
  if (b.bidir && (rc = upload_windows(b)) != GS_OK) return rc;
  reserve_arena(b);
  if ((rc = main_pass(b)) != GS_OK) return rc;
  if (ix->dbg_nomem != 0) { /* (tests: as if the workspace of the stages below had not fitted - tables placed, copies built, slots grown) */
    ix->dbg_nomem--;
    GS_HIP(hipStreamSynchronize(b.st));
    return GS_ERR_NOMEM;
  }
  if ((rc = order_items(b)) != GS_OK) return rc;
  if ((rc = overflow_redo(b)) != GS_OK) return rc;
  if ((rc = order_set(b)) != GS_OK) return rc;
  return finish(b, d_offsets, d_hits, stats);
}

/* ---- what gs_enumerate_device tries, in order, when a batch fails: each recovery applies when the status calls for it and
 * says whether the batch is redone ---- */
/* the sharing's bounded wait ran out (run_search): this handle shares nothing for a while - whatever kept the launch off the
 * chip may still be there -, whatever the tuning switches say (GS_SHARE_MIN, GS_HEAVY, GS_SPLIT_SHARE): the form is chosen
 * with the back-off after them */
static bool recover_share_timeout(gs_index *ix, gs_status rc) {
  if (rc != GS_ERR_DEVICE || !ix->share_timed_out) return false;
  ix->share_timed_out = false;
  ix->share_backoff = 64;
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] sharing timed out: batch redone with every item on its own wave\n");
  return true;
}
/* the batch's workspace did not fit.  First what earlier batches left on the handle and this one may not need goes - a
 * batch ordered device-wide leaves tens of bytes per record in a dozen arrays that a batch ordered in tiles never touches,
 * and the other way round (10^9 records: 70 GB either way) - and the batch is redone: every workspace buffer grows again
 * on demand.  Then the derived tables, one kind at a time: the strand tables' rotated copies, then the PAM-pair tables. */
static const size_t RELEASE_REDO_MIN = (size_t)1 << 30; /* released bytes from which the same batch is worth another try */
static bool recover_release_workspace(gs_index *ix, gs_status rc) {
  if (rc != GS_ERR_NOMEM) return false;
  (void)hipGetLastError();
  const size_t freed = ix->w_batch.release() + ix->w_big.release() + ix->w_tile.release() + ix->w_score.release() +
                       ix->w_text.release() + ix->w_bgzf.release() + ix->w_annot.release();
  size_t redo_min = RELEASE_REDO_MIN;
  if (const char *e = gs_opt(ix, "GS_DBG_RELEASE_MIN")) redo_min = (size_t)strtoull(e, nullptr, 10); /* (tests: bytes) */
  if (freed <= redo_min) return false;
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] out of device memory: %.1f GB (%zu bytes) of workspace released, batch redone\n", 1e-9 * (double)freed, freed);
  return true;
}
/* the spaced tables go first: without them a batch of the headline's shape takes 17.0 instead of 15.7 ms, without any other table far more */
static bool recover_drop_spaced(gs_index *ix, gs_status rc) {
  if (rc != GS_ERR_NOMEM) return false;
  const bool a = gs_pairtab_free_spaced(ix, 0), b = gs_pairtab_free_spaced(ix, 1);
  if (!a && !b) return false;
  (void)hipGetLastError();
  ix->spaced_off = true;
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] out of device memory: spaced tables dropped, batch redone without them\n");
  return true;
}
static bool recover_drop_rotated(gs_index *ix, gs_status rc) {
  if (rc != GS_ERR_NOMEM || !gs_strand_rot_release(ix)) return false;
  (void)hipGetLastError();
  ix->rot_off = true;
  ix->pairtab_nofit = 0; /* 86 GB came back: a pair that did not fit may now */
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] out of device memory: rotated table copies dropped, batch redone without them\n");
  return true;
}
static bool recover_drop_pairtabs(gs_index *ix, gs_status rc) {
  if (rc != GS_ERR_NOMEM || !(ix->pairtab[0].valid || ix->pairtab[1].valid)) return false;
  (void)hipGetLastError();
  gs_pairtab_free(ix, 0);
  gs_pairtab_free(ix, 1);
  ix->pairtab_off = true;
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] out of device memory: PAM-pair tables dropped, batch redone without them\n");
  return true;
}
extern "C" gs_status gs_enumerate_device(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L,
                                         const void *d_guide_pams, uint32_t P, const char *alt_pams,
                                         uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                         void *stream, const void **d_offsets, const void **d_hits,
                                         gs_result_view *stats) {
  GS_HANDLE_LOCK(ix);
  try { /* the plans and lists built per batch live in std containers: nothing may throw across the C boundary */
    gs_status rc = enumerate_device_impl(ix, d_guides, n, L, d_guide_pams, P, alt_pams, n_alt, mismatches, flags, stream,
                                         d_offsets, d_hits, stats);
    if (ix)
      for (auto recover : {recover_share_timeout, recover_drop_spaced, recover_release_workspace, recover_drop_rotated, recover_drop_pairtabs})
        if (recover(ix, rc))
          rc = enumerate_device_impl(ix, d_guides, n, L, d_guide_pams, P, alt_pams, n_alt, mismatches, flags, stream, d_offsets,
                                     d_hits, stats);
    return rc;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_rank_bwt4(gs_index *ix, int strand, const uint64_t *rows, uint64_t n,
                                  uint64_t *out) {
  GS_HANDLE_LOCK(ix);
  if (!ix || strand < 0 || strand > 1 || (n && (!rows || !out))) return GS_ERR_ARG;
  for (uint64_t j = 0; j < n; j++)
    if (rows[j] > ix->strand[strand].n) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(ix->device));
  uint64_t *d_rows = nullptr, *d_out = nullptr;
  if (n == 0) return GS_OK;
  gs_scratch mem;
  GS_TRY(mem.get(8 * n, &d_rows));
  GS_TRY(mem.get(32 * n, &d_out));
  GS_HIP(hipMemcpy(d_rows, rows, 8 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_rank4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix->strand[strand].d,
                     d_rows, n, d_out);
  GS_HIP(hipMemcpy(out, d_out, 32 * n, hipMemcpyDeviceToHost));
  return GS_OK;
}

extern "C" gs_status gs_resolve(gs_index *ix, int strand, const uint64_t *rows, uint64_t n,
                                uint64_t *out) {
  GS_HANDLE_LOCK(ix);
  if (!ix || strand < 0 || strand > 1 || (n && (!rows || !out))) return GS_ERR_ARG;
  for (uint64_t j = 0; j < n; j++)
    if (rows[j] >= ix->strand[strand].n) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(ix->device));
  uint64_t *d_rows = nullptr, *d_out = nullptr;
  if (n == 0) return GS_OK;
  gs_scratch mem;
  GS_TRY(mem.get(8 * n, &d_rows));
  GS_TRY(mem.get(8 * n, &d_out));
  GS_HIP(hipMemcpy(d_rows, rows, 8 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                     ix->strand[strand].d, d_rows, n, d_out);
  GS_HIP(hipMemcpy(out, d_out, 8 * n, hipMemcpyDeviceToHost));
  return GS_OK;
}

/* ---- gs_index_prepare: the first batch's one-off work ahead of the first job ------------------------------------ */
__global__ void k_prepare_fill(uint8_t *guides, uint8_t *pams, uint64_t n, uint32_t L, uint32_t P, uint4 pat /* <= 8 symbols in x, y */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h = (i + 1u) * 0x9E3779B97F4A7C15ull;
  for (uint32_t t = 0; t < L; ++t) {
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    guides[i * L + t] = "ACGT"[(h >> 61) & 3u];
  }
  for (uint32_t u = 0; u < P; ++u) pams[i * P + u] = (uint8_t)((u < 4u ? pat.x >> (8u * u) : pat.y >> (8u * (u - 4u))) & 0xFFu);
}
extern "C" gs_status gs_index_prepare(gs_index *ix, uint64_t n, uint32_t L, const char *pam, uint32_t P, const char *alt_pams,
                                      uint32_t n_alt, uint32_t mismatches, uint32_t flags) {
  GS_HANDLE_LOCK(ix);
  if (!ix || (P && !pam) || (n_alt && !alt_pams) || L < 1 || L > 31 || P > 8 || n >= (1ull << 31)) return GS_ERR_ARG;
  if (n == 0) return GS_OK;
  GS_HIP(hipSetDevice(ix->device));
  uint8_t *d_g = nullptr, *d_p = nullptr;
  gs_scratch mem;
  GS_TRY(mem.get(n * L, &d_g));
  GS_TRY(mem.get(n * P, &d_p));
  uint4 pat = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t u = 0; u < P; ++u) (u < 4u ? pat.x : pat.y) |= (uint32_t)(uint8_t)pam[u] << (8u * (u & 3u));
  hipLaunchKernelGGL(k_prepare_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_g, d_p, n, L, P, pat);
  const void *off = nullptr, *hits = nullptr;
  gs_result_view v;
  /* what the handle learns from its batches (slot sizing, the search's form, the queue of shared passes) must come from the
   * caller's guides, not from this synthetic few-hit batch: saved and put back.  The call does overwrite the device
   * buffers an earlier gs_enumerate_device left its results in (include/guidescan_amd.h says so). */
  const auto s_seen = ix->seen;
  const uint64_t s_pk = ix->shq_packages;
  const gs_status rc = gs_enumerate_device(ix, d_g, n, L, d_p, P, alt_pams, n_alt, mismatches, flags & ~GS_FLAG_COUNT_REQUESTS, nullptr, &off, &hits, &v);
  ix->seen = s_seen;
  ix->shq_packages = s_pk;
  (void)hipDeviceSynchronize();
  return rc;
}
