/* gs_common.h -- internal declarations shared by the translation units of libgsamd.so */
#ifndef GS_COMMON_H
#define GS_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "guidescan_amd.h"

/* ---- device-resident FM-index of one strand ---------
 * Occ block = 64 bytes covering 128 BWT rows:
 *   uint32 cnt[4]   occurrences of A,C,G,T in BWT[0, 128*b)
 *   uint64 lo[2]    bit j of word w: low  bit of the 2-bit code of row 128*b+64*w+j
 *   uint64 hi[2]    high bit of the code (A=0 C=1 G=2 T=3)
 *   uint64 ex[2]    1 = row holds a non-ACGT symbol ('\0' sentinel, N, IUPAC) or padding
 * One aligned 64-byte read answers Occ(c, i) for all four bases exactly, including
 * rows whose BWT symbol is not a base (no side table on the fast path). */
/* overflow arena of k_search (gs_search.hip): records per chunk (16 KiB): one atomic per 1,024 matches */
#define ARENA_SHIFT 10u
#define ARENA_CHUNK (1u << ARENA_SHIFT)

#define GS_BLOCK_ROWS 128u
#define GS_BLOCK_SHIFT 7u

/* A PAM-pair table (gs_pairtab.hip): the depth-k prefix table restricted to the rows whose left context
 * has the pair `code` (two 2-bit symbols) at offsets v_rem-2, v_rem-1 and only A,C,G,T nearer than
 * that.  Entry = 8 bytes {first of its rows in the table's own row arrays, rows (6 bits) | filter (26 bits)}:
 * the 16 two-symbol extensions of a (k-2)-mer are ONE 128-byte block.  rows = 63: 63 or more - the row
 * arrays then hold a header slot at `first` (rowid[first] = the count) and the rows behind it.  Filter:
 * with one row its nearest 13 context symbols (2 bits each); with more, for each of the nearest 6
 * context positions the set of symbols its rows show there (4 bits each): a query symbol outside the
 * set is a substitution in every row. */
#define GS_PT_BIG 63u
struct gs_pairtab_dev {
  const uint2 *tab;
  const uint2 *rot;      /* rotated copies of consumption steps rot_first .. k-3 */
  const uint16_t *c16;   /* per row of the table: nearest eight context symbols */
  const uint32_t *ctx;   /* all sixteen */
  const uint32_t *rowid; /* its row in the strand's suffix array */
  uint32_t rot_first;
  uint32_t code;
  /* the deep table of the strand seen from the other strand's items (gs_pairtab.hip), or nullptr */
  const uint4 *deep;
  /* the spaced table (gs_pairtab.hip), or nullptr: the table's rows sorted by key = (X symbols of the row's k-mer, its R
   * symbols) - what a site that spent the whole budget inside O shares with its guide.  sp_off: 2^d + 1 offsets into
   * sp_rows over the key's top d bits; sp_rows: {row in the row arrays, O symbols << sp_rem | the key's low sp_rem bits} */
  const uint32_t *sp_off;
  const uint2 *sp_rows;
  uint32_t sp_rem;
};
struct gs_strand_dev {
  const uint4 *blocks;       /* (n >> 7) + 1 blocks of 4 x uint4 */
  const uint32_t *sa;        /* full suffix array, n entries */
  const uint32_t *run_start; /* first row of each maximal run of 'N' in the BWT */
  const uint32_t *run_cum;   /* run_cum[r] = number of N rows in runs < r ; nruns+1 entries */
  uint32_t n;                /* rows = text length + 1 */
  uint32_t nruns;
  uint32_t C[4]; /* first row of the A, C, G, T ranges */
  uint32_t CN;   /* first row of the N range (undefined when has_n == 0) */
  uint32_t has_n;
  /* prefix interval table: one 16-byte entry per k-mer, indexed by the
   * k-mer with its FIRST text symbol in the LOWEST bits, so the 16 two-symbol left extensions of
   * a (k-2)-mer are contiguous.  Entry = {sp, cnt | flag<<31, mask_lo, mask_hi}:
   * cnt==0: k-mer absent; flag: some row of the interval has a non-ACGT symbol (or the text
   * start) within the 16 symbols preceding its suffix, so it must take the Occ walk;
   * mask (64 bits in z, w): four 16-bit sets; bit 16j + v: some row of the interval is preceded by
   * the symbol pair v (two symbols, 2 bits each, nearest first) at distances mask_off[j],
   * mask_off[j]+1 (0 = the symbol right before the suffix); a symbol outside A,C,G,T and a position before the text start
   * read as A there, as in ctx[] (surplus bits cost time, never a hit).  The offsets are 0, 2, 4 and - so that
   * for 20-mers with a 3-symbol PAM whose first symbol is a wildcard the fourth pair is the PAM's two
   * fixed symbols - 21-k (7 at k = 14); any offsets are correct, they only set the filter's power.  A site with at
   * most b substitutions among the symbols a seed still has to match leaves at least (pairs - b)
   * of its query pairs intact, so a seed whose interval shows fewer of them cannot reach a hit. */
  const uint4 *ptab;
  uint32_t mask_off; /* 4 bits per pair position */
  /* rotated copies of the table: copy p (p < k-2) has the symbol of
   * consumption step p moved to the lowest index bits, so the three substitutions at step p
   * of an otherwise fixed k-mer are neighbours in one 64-byte line.  Steps rot_first .. k-2, back to back. */
  const uint4 *ptab_rot;
  uint32_t rot_first; /* first consumption step that has a copy (31: none).  The lowest steps are the
                         other strand's PAM steps, never substituted, and the last substituted step of
                         few one-sided seeds: their copies (4.3 GB each at hg38 size) are not built */
  /* preceding context: ctx[r] = the 16 text symbols before suffix SA[r],
   * nearest first, 2 bits each (A,C,G,T = 0..3).  Lets a small interval at depth k be resolved
   * against the rest of the pattern with one 4-byte read per row instead of an Occ walk. */
  const uint32_t *ctx;
  /* the nearest 8 of them (low 16 bits of ctx[r]): the first level of the verification reads
   * these, 8 rows per 16-byte load, and only the few surviving rows touch ctx[] */
  const uint16_t *ctx16;
  /* inverse suffix array (isa[sa[r]] = r), n entries, or nullptr: turns a text position found
   * through the other strand's index into this strand's row (two-sided seeding) */
  const uint32_t *isa;
  /* exception rows: the rows of valid k-mer intervals whose 16-symbol left
   * context holds a symbol outside A,C,G,T or runs off the text start - ctx[] cannot say so (it
   * stores 2 bits per symbol).  Sorted by row; exc_sym[i] = the 16 symbols as nibbles, nearest
   * first: 0..3 A,C,G,T, 4 'N', 5 any other symbol, 6 before the text start.  A few rows per N run:
   * the verification looks a row up here only when its table entry carries the flag. */
  const uint32_t *exc_row;
  const uint64_t *exc_sym;
  uint32_t n_exc;
  /* every symbol outside A,C,G,T (the general path, gs_general.hip): maximal runs of equal such
   * symbols in the BWT, grouped by symbol.  xr_seg[c] = {first run of symbol c, number of runs};
   * xr_start[i] = first row of run i, xr_cum[i] = rows of the symbol in its earlier runs (one entry
   * more per symbol: its total); C256[c] = csa.C[csa.char2comp[c]] for every byte present. */
  const uint32_t *xr_start;
  const uint32_t *xr_cum;
  const uint2 *xr_seg;
  const uint32_t *C256;
};

/* A device allocation that grows on demand (gs_reserve) and is kept from call to call: a handle's or a decoder's
 * workspace.  Frees itself; moves only.  (The owner sets its device before it lets one go.) */
struct gs_buffer {
  void *p = nullptr;
  size_t cap = 0;
  gs_buffer() = default;
  gs_buffer(gs_buffer &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  gs_buffer &operator=(gs_buffer &&o) noexcept;
  ~gs_buffer();
};
gs_status gs_reserve(gs_buffer &b, size_t bytes);
/* frees the buffer (if any) and leaves it empty; returns the bytes it held */
size_t gs_buffer_free(gs_buffer &b);

/* ---- the handle's per-batch workspace, grown on demand and reused across calls: one group per unit that reserves it.
 * each(f) names the group's buffers, f(buffer, bulk); bulk: sized by the records of a batch, so release() frees it when a
 * batch runs out of device memory (gs_enumerate.hip: recover_release_workspace) and returns the bytes - the rest, a few
 * words per guide or per tile, stays.  Nothing here decides what is freed with the handle: every gs_buffer frees itself. */
template <class G>
static inline size_t gs_ws_release(G &g) {
  size_t freed = 0;
  g.each([&](gs_buffer &b, bool bulk) { freed += bulk ? gs_buffer_free(b) : 0; });
  return freed;
}
/* out[0..2] += buffers held, bytes held, bytes release() would free */
template <class G>
static inline void gs_ws_report(G &g, uint64_t *out) {
  g.each([&](gs_buffer &b, bool bulk) {
    if (!b.p) return;
    out[0]++;
    out[1] += b.cap;
    out[2] += bulk ? b.cap : 0;
  });
}
/* gs_enumerate.hip, the batch pipeline's own (its kernels: gs_search.hip, gs_seed.hip, gs_order.hip) */
struct gs_ws_batch {
  gs_buffer guides, slots, counts, nmatch, nhits, offsets, hits, misc, blocksums, grec, flags, raw, ovf_list, grec2, slots2,
      counts2, nmatch2, nhits2, h_off, h_tmp,
      /* overflow arena of k_search (gs_search.hip): records, chunk owners + sequence numbers, chunks per item */
      arena, arena_meta, nchunk,
      /* heavy items shared among waves (gs_search_args::shq): the package queue; counters, flags, shared-item list, sums, directory bases */
      shq, sh_meta,
      cls,         /* k_search's per-class counts (read by gs_tileorder.hip's plan) */
      desc, sched, /* gs_seed.hip: descriptors per guide; work counters, histograms, the two schedules */
      cand;        /* literal-N candidate windows: kept from batch to batch of one shape */
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&slots, &hits, &slots2, &h_tmp, &arena, &shq}) f(*b, true);
    for (gs_buffer *b : {&guides, &counts, &nmatch, &nhits, &offsets, &misc, &blocksums, &grec, &flags, &raw, &ovf_list, &grec2,
                         &counts2, &nmatch2, &nhits2, &h_off, &arena_meta, &nchunk, &sh_meta, &cls, &desc, &sched, &cand})
      f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_bigorder.hip: device-wide ordering of guides with more matches than an LDS sort holds */
struct gs_ws_big {
  gs_buffer src, cnt, prefix, recs, w0, w0b, idx, idxb, keep, keeps, rows, rowss, s, redo_pos, redo_pos2, tab;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&src, &cnt, &prefix, &recs, &w0, &w0b, &idx, &idxb, &keep, &keeps, &rows, &rowss, &s}) f(*b, true);
    for (gs_buffer *b : {&redo_pos, &redo_pos2, &tab}) f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_tileorder.hip: per-guide ordering in LDS tiles - the plan's scans, tile descriptors, bucket space, chunk index,
 * partitioned items, class starts, rank tables + flags, the guides beyond the tiles' reach, the spill list */
struct gs_ws_tile {
  gs_buffer plan, tiles, buckets, chunkof, big, rel, tab, excl, spill;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&buckets, &tiles, &chunkof, &big}) f(*b, true);
    for (gs_buffer *b : {&plan, &rel, &tab, &excl, &spill}) f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_score.hip: score tables + chromosome prefix sums; host-pointer staging; scratch */
struct gs_ws_score {
  gs_buffer tab, io, tmp;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&tmp, &io}) f(*b, true);
    f(tab, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_textdev.hip: what gs_format_device uploads, its scratch, the of:H: fields, the text it returns; gs_enumerate_text's
 * specificities (gs_host.hip); per-guide text offsets */
struct gs_ws_text {
  gs_buffer in, tmp, hex, text, spec, goff;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&tmp, &hex, &text}) f(*b, true);
    for (gs_buffer *b : {&in, &spec, &goff}) f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_bgzf.hip: what gs_bgzf_compress uploads; token lists, sizes and the pieces' streams; the members it returns */
struct gs_ws_bgzf {
  gs_buffer in, tmp, out;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&in, &tmp, &out}) f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
/* gs_annot.hip: the chromosome prefix sums a call uploads; the counts and the scan's temporary; what gs_annotate_device
 * returns - feature offsets and features per hit, counts per guide and distance; gs_annotate's staging */
struct gs_ws_annot {
  gs_buffer in, cnt, tmp, foff, feats, gcnt, io;
  template <class F>
  void each(F f) {
    for (gs_buffer *b : {&cnt, &foff, &feats, &io}) f(*b, true);
    for (gs_buffer *b : {&in, &tmp, &gcnt}) f(*b, false);
  }
  size_t release() { return gs_ws_release(*this); }
};
#define GS_WS_GROUPS 7

/* The device arrays a handle keeps between calls (a strand's, a PAM-pair slot's): each with the bytes it counts for in
 * gs_index_device_bytes - what the fit estimates reckon with, not the allocation's size.  Frees them when it goes.
 * take(): the array leaves the scratch it was built in (gs_scratch.h), its address goes into `field` of the gs_strand_dev /
 * gs_pairtab_dev; a null array is no entry.  release(): frees the array `field` names, nulls it, returns its bytes. */
struct gs_scratch;
struct gs_resident {
  gs_resident() = default;
  gs_resident(gs_resident &&o) noexcept { v.swap(o.v); } /* (moves only: no copies) */
  gs_resident &operator=(gs_resident &&o) noexcept {
    clear();
    v.swap(o.v);
    return *this;
  }
  ~gs_resident() { clear(); }
  template <class T>
  void take(gs_scratch &from, const T *&field, const void *q, uint64_t bytes) {
    adopt(from, q, bytes);
    field = (const T *)q;
  }
  template <class T>
  uint64_t release(const T *&field) {
    const uint64_t b = drop(field);
    field = nullptr;
    return b;
  }
  void clear();
  uint64_t bytes() const;
  uint64_t bytes_of(const void *q) const; /* 0: not one of its arrays */
  uint64_t count() const { return v.size(); }

 private:
  struct item {
    const void *p;
    uint64_t bytes;
  };
  std::vector<item> v;
  void adopt(gs_scratch &from, const void *q, uint64_t bytes);
  uint64_t drop(const void *q);
};

struct gs_strand {
  gs_strand_dev d{}; /* the one record of the arrays' addresses */
  gs_resident own;   /* ... of who frees them and what they count for */
  bool has_sym[256] = {false}; /* bytes present in this strand's text */
  /* the rotated table copies this strand may hold (gs_strand_rot_ensure builds them on first use): first step, count (0: none), table depth */
  uint32_t rot_plan_first = 31, rot_plan_n = 0, rot_k = 0;
  uint64_t n = 0;
  uint64_t C_acgtn[5] = {0, 0, 0, 0, 0};
  uint64_t xr_entries = 0; /* entries of xr_start / xr_cum: the runs and one closing entry per symbol that has any */
};

/* a maximal run of 'N' bytes in the forward text with the bytes around it (host side; used per
 * batch to list the few windows where a PAM 'N' can meet a literal N, index.hpp:139-149) */
#define GS_NRUN_FLANK 40
struct gs_nrun {
  uint64_t start, len;
  uint8_t left[GS_NRUN_FLANK];  /* text[start-40 .. start), 0 beyond the text */
  uint8_t right[GS_NRUN_FLANK]; /* text[start+len .. start+len+40) */
};

struct gs_pairtab_host {
  bool valid = false;
  uint32_t v_rem = 0, code = 0, rot_first = 31;
  gs_pairtab_dev d[2]{};
  gs_resident own;
  bool deep = false;               /* both strands' deep tables exist (PAM length deep_P) */
  uint32_t deep_P = 0, deep_kb = 0;
  bool spaced = false;             /* both strands' spaced tables exist, keyed by the first sp_x and the last sp_g guide symbols */
  uint32_t sp_x = 0, sp_g = 0;
  uint32_t sp_forced_d = 0;        /* GS_SPACED_BITS when they were built (0: the offsets' bits came from the row count) */
  uint64_t sp_rows[2] = {0, 0};
  uint64_t sp_bytes() const { return own.bytes_of(d[0].sp_off) + own.bytes_of(d[0].sp_rows) + own.bytes_of(d[1].sp_off) + own.bytes_of(d[1].sp_rows); }
  uint64_t n_slots[2] = {0, 0};    /* slots of each strand's row arrays (rows + the big entries' header slots) */
  double sp_build_ms = 0;
  uint64_t used = 0;
};

struct gs_recipe_set {
  gs_buffer buf;
  uint64_t key[2] = {0, 0};
  bool valid = false;
  uint32_t n_full = 0, n_a = 0, n_b = 0, n_a8 = 0; /* full | a | b | a as read through PAM-pair tables */
  uint32_t n_a8s = 0; /* | the same without the class (no substitution in X, the whole budget in O): the spaced tables' share */
  uint32_t a_rot_first = 31; /* lowest consumption step whose rotated copy the PAM-pair list reads (31: none) */
  /* the seeding launches' probe lists (gs_kernels.h: gs_probe_b, gs_probe_a), eight bytes per recipe: prb_b beside the b
   * share; prb_a[] beside both a8 lists, one per value of a PAM-pair table's rot_first the set has met (two table slots:
   * two values at a time).  host_ba: the b | a8 | trimmed a8 words they are built from */
  gs_buffer prb_b;
  struct {
    gs_buffer buf;
    uint32_t rot_first = 31;
    bool valid = false;
  } prb_a[2];
  std::vector<uint64_t> host_ba;
};

struct gs_index {
  /* Switches of the library (tuning experiments, the forms the tests force): the process environment's GS_* variables
   * as they were when the handle was made, then whatever gs_index_set_option changed.  No entry point reads the
   * environment after that (a multithreaded host may setenv at any time): gs_opt() is the only reader. */
  std::map<std::string, std::string> opts;
  /* One batch at a time per handle: the workspace, the lazily built tables and the result buffers belong to the handle,
   * while the reference's seam is called from N host threads on one const index (src/guidescan.cxx:240-247).  Every
   * entry point that takes a handle holds this lock for its whole call (host-pointer entry points copy their
   * results out under it: they are safe from any number of threads); recursive because the host-pointer entry points
   * call the device ones.  gs_index_lock / gs_index_unlock hold it across several device-pointer calls. */
  mutable std::recursive_mutex mtx;
  int device = 0;
  uint64_t genome_length = 0;
  gs_strand strand[2];
  /* per-handle workspace (above), grown on demand, reused across calls */
  gs_ws_batch w_batch;
  gs_ws_big w_big;
  gs_ws_tile w_tile;
  gs_ws_score w_score;
  gs_ws_text w_text;
  gs_ws_bgzf w_bgzf;
  gs_ws_annot w_annot;
  const struct gs_annot *annot = nullptr; /* gs_index_set_annotation: what GS_TEXT_FEATURES looks rows up in; the caller's */
  uint32_t share_backoff = 0; /* batches this handle still runs without sharing after a sharing launch was not resident as a whole */
  bool share_timed_out = false; /* a helping wave gave up waiting for a package (k_search_body): the call fails, gs_enumerate_device redoes the batch without sharing */
  uint32_t opt_share_min = 512, opt_share_max = 2048; /* groups of eight rows: a verification pass of share_min or more is handed out, in packages of at most share_max (0: items are never shared) */
  unsigned long long last_share[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* the last batch: shared items, packages reserved, queue capacity, tickets handed out; [4] guides beyond the tiles' reach, ordered device-wide alone */
  uint64_t shq_packages = 16384; /* packages the next batch's queue holds (1,152 bytes each): grown when a batch reserved more */
  uint64_t arena_chunks = 4096; /* chunks of 1,024 records the next batch's arena holds: grown when a batch needed more */
  /* what the last batch showed, per mismatch budget, and the shape it was measured on (gs_enumerate.hip: shape_key) */
  struct seen_t {
    double mean = -1, max = 0;     /* matches per item (slot sizing) */
    uint64_t hpass = 0, items = 0; /* verification passes of share_min row groups or more, and its items (the search's form) */
    uint64_t key = 0;
  };
  std::array<seen_t, 8> seen;
  bool last_raw_valid = false;   /* w_batch.raw holds the raw hit counts of the last batch (GS_FLAG_RAW_COUNTS) */
  uint64_t last_unsupported = 0; /* guides of the last batch flagged GS_GUIDE_NEEDS_GENERAL (w_batch.flags) */
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_tile = nullptr;  /* gs_tileorder_run: behind the copy of the slow-tile counts */
  hipStream_t st_help = nullptr; /* lowest priority: the launch that runs published packages next to the search launch (run_search) */
  hipEvent_t ev_help[2] = {nullptr, nullptr};
  uint32_t *h_pin = nullptr;     /* 256 bytes of page-locked host memory: small results of asynchronous copies that are read behind an event */
  std::atomic<uint64_t> lock_owner{0}; /* gs_index_lock: the thread that holds the handle (0: none), and how many times */
  uint32_t lock_depth = 0;
  uint32_t pt_k = 0; /* depth of the prefix interval tables (0: none) */
  unsigned long long last_counters[16] = {0}; /* k_search's stats array of the last gs_enumerate_device call */
  /* the main pass's launch of the last batch (gs_index_last_launch): walking kernel, kernel without the strand tables' side,
   * deep tables, items per visit, ... of the two seeding launches (0: not that form), PAM-pair tables, |X|, rotated copies per strand table */
  unsigned long long last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  /* the last call of the general path (gs_debug_general_last): items, workgroups, the first pass's pool, records, search passes,
   * then k_search_general's three counters of the last pass: largest stack, steps the room rule cut, steps with no room at all */
  unsigned long long last_general[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  /* the same call's routing and the seeded form's counters (gs_debug_bulge_last): guides sent to the seeded form, guides that
   * walked, seeds looked up, seeds with an empty interval, row nodes made, interval nodes made, exception-row lookups, largest stack */
  unsigned long long last_bulge[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<gs_nrun> nruns_text; /* 'N' runs of the forward text */
  uint64_t cand_key = ~0ull;       /* (L, P, bucketed or not) w_batch.cand was made for; ~0: nothing kept */
  uint32_t cand_n[2] = {0, 0};     /* windows per strand */
  size_t cand_bidx[2] = {0, 0};    /* words of each strand's bucket index behind them */
  /* seed recipes of the last two (budget, geometry, thresholds) - the CLI's --threshold pass alternates two
   * budgets on one handle: full | a | b per set; rec_cur = the set the last call used */
  gs_recipe_set rec[2];
  uint32_t rec_cur = 0;
  /* PAM pairs whose tables did not fit next to the rest (bit per pair code): not tried again until memory
   * is released (gs_pairtab_forget_nofit) */
  uint32_t pairtab_nofit = 0;
  /* PAM-pair tables (gs_pairtab.hip), built on first use for the pairs a batch's patterns end in */
  gs_pairtab_host pairtab[2];
  bool pairtab_off = false; /* a batch ran out of memory next to them: not built again on this handle */
  bool spaced_off = false;  /* the same for the spaced tables */
  unsigned long long last_spaced[4] = {0, 0, 0, 0}; /* the last batch (gs_index_last_spaced): items looked up, rows read, most rows under one key, rows that matched */
  bool rot_off = false;     /* the same for the strand tables' rotated copies */
  uint32_t dbg_nomem = 0;   /* GS_DBG_NOMEM (tests of those recoveries): passes of a batch that still end as if out of device memory */
  bool tile_order_off = false; /* a batch had interval records or one sequence at one row twice: the per-guide tile ordering is not tried again for that shape */
  uint64_t tile_order_off_key = 0;
  uint64_t tx_n = 0; /* gs_textdev.hip: guides of the last gs_format_device, whose per-guide text offsets w_text.goff holds (0: none) */
  bool big_long_runs = false; /* a batch showed long runs of one sequence (repeat-rich genome): the device-wide ordering sorts by row, then by word (gs_bigorder.hip) */
};

/* make sure slot `slot` holds the tables of pair `code` at context depth v_rem with rotated copies from
 * step rot_first on (fewer when memory is short: they may take `share` of what is free beyond the
 * reserve); valid stays false when they do not fit */
gs_status gs_pairtab_ensure(gs_index *ix, uint32_t slot, uint32_t v_rem, uint32_t code, uint32_t rot_first, double share,
                            hipStream_t st);
/* add the deep tables (the other strand's side, PAM of three symbols) to a valid slot; p.deep stays false when they do not fit */
gs_status gs_pairtab_ensure_deep(gs_index *ix, uint32_t slot, uint32_t P, uint32_t kb, hipStream_t st);
void gs_pairtab_free(gs_index *ix, uint32_t slot);
/* add the spaced tables to a valid slot (keys: the first x_len and the last g guide symbols); p.spaced stays false when they
 * do not fit or the key does not fit the layout */
gs_status gs_pairtab_ensure_spaced(gs_index *ix, uint32_t slot, uint32_t x_len, uint32_t g, hipStream_t st);
/* false: the slot had none */
bool gs_pairtab_free_spaced(gs_index *ix, uint32_t slot);
/* tests (gs_debug_index_layout, gs_debug_index_array): a slot's scalars and arrays (gs_pairtab.hip); bytes of a device array to the host (gs_index.hip) */
gs_status gs_debug_pairtab_layout(const gs_index *ix, uint32_t slot, int strand, uint64_t out[32]);
gs_status gs_debug_pairtab_array(const gs_index *ix, uint32_t slot, int strand, const char *which, uint64_t offset_bytes, void *out,
                                 uint64_t cap_bytes, uint64_t *total_bytes);
gs_status gs_debug_copy_array(const gs_index *ix, const void *p, uint64_t bytes, uint64_t offset_bytes, void *out, uint64_t cap_bytes,
                              uint64_t *total_bytes);
/* gs_index.hip: the strand tables' rotated copies, built by the first batch that reads them */
gs_status gs_strand_rot_ensure(gs_index *ix, hipStream_t st);
bool gs_strand_rot_release(gs_index *ix);

/* ---- gs_tileorder.hip: the per-guide ordering of the guides k_order's LDS does not hold ---- */
struct gs_tileorder_in {
  uint32_t n_set;         /* guides of the set */
  const uint32_t *list;   /* device: set guide -> guide of the batch (nullptr: the whole batch) */
  const uint32_t *redo_pos; /* device: guide of the batch -> set guide (with list) */
  const uint32_t *counts; /* device [2 n]: records per item, exact */
  const uint32_t *cls;    /* device [2 n][8]: records per item and mismatch count */
  const uint4 *slots;     /* the main slot array, `cap` per item */
  uint32_t cap;
  const uint4 *arena;     /* overflow chunks and their owners */
  const uint32_t *chunk_item, *chunk_seq;
  uint32_t n_used;
  uint32_t *nhits;        /* device [n]: set to the set guides' hit counts by the plan */
  const uint64_t *offsets; /* device [n + 1]: valid when gs_tileorder_run is called */
  gs_hit *hits;
  uint32_t L, P, m, v_rem;
};
struct gs_tileorder_state {
  uint32_t n_it = 0, n_tiles = 0, n_btiles = 0, n_chunks = 0, n_big = 0, n_deal = 0;
  uint32_t spill_units = 0, spill_cap = 0; /* bucket units kept for the buckets that outgrow their slots; records the spill list holds */
  uint32_t n_excl = 0; /* guides with an item beyond the tiles' reach (ix->w_tile.excl lists them): ordered device-wide by the caller */
  uint64_t n_records = 0; /* records of the set (set by gs_tileorder_run) */
};
/* does the sort word (class base + rank of the sequence, then the row) fit 64 bits? */
bool gs_tileorder_fits(uint32_t L, uint32_t P, uint32_t m);
/* plan: tiles, bucket space, chunk index, class starts; sets nhits of the set's guides.  *usable = false: an item is
 * too large for this form (nothing else was changed) */
gs_status gs_tileorder_plan(gs_index *ix, const gs_tileorder_in &in, hipStream_t st, gs_tileorder_state &S, bool *usable);
/* partition + order + write the hits; *violations != 0: an assumption did not hold (multi-row records, a sequence at
 * one row twice, a bucket beyond its space) - the hits of the set are then not valid and the caller orders it the other way */
gs_status gs_tileorder_run(gs_index *ix, const gs_tileorder_in &in, gs_tileorder_state &S, hipStream_t st, uint32_t *violations);

#define GS_HANDLE_LOCK(ix)                               \
  std::unique_lock<std::recursive_mutex> handle_lock__; \
  if (ix) handle_lock__ = std::unique_lock<std::recursive_mutex>((ix)->mtx)

#define GS_HIP(expr)                                                              \
  do {                                                                            \
    hipError_t e__ = (expr);                                                      \
    if (e__ != hipSuccess) {                                                      \
      gs_set_error(std::string(#expr) + ": " + hipGetErrorString(e__));           \
      return GS_ERR_DEVICE;                                                       \
    }                                                                             \
  } while (0)

#define GS_TRY(expr)                 \
  do {                               \
    gs_status rc__ = (expr);         \
    if (rc__ != GS_OK) return rc__;  \
  } while (0)

void gs_set_error(const std::string &s);
/* value of switch `key` on this handle, or nullptr (gs_index::opts) */
const char *gs_opt(const gs_index *ix, const char *key);
void gs_opts_from_env(gs_index *ix);
extern std::atomic<int> gs_debug_any; /* some handle has GS_DEBUG set: the allocator reports large growth */
/* gs_host.hip: tl bytes of text in HBM -> *text, malloc'ed and NUL terminated, through page-locked staging */
gs_status gs_text_to_host(const void *d_text, uint64_t tl, char **text);
/* gs_text.hip: a float as the CSV's specificity column prints it, std::to_string(float) */
std::string gs_f2s(float f);

/* GPU suffix array: d_text (n bytes incl. sentinel) -> d_sa (n uint32) */
gs_status gs_device_suffix_array(const uint8_t *d_text, uint64_t n, uint32_t *d_sa, hipStream_t st);
/* build the device layout of one strand from device-resident text and SA; when it succeeds the strand has taken the
 * suffix array out of sa_mem, otherwise the strand holds nothing */
gs_status gs_strand_from_device(const uint8_t *d_text, gs_scratch &sa_mem, uint32_t *d_sa, uint64_t n, gs_strand *out, hipStream_t st);
void gs_strand_free(gs_strand *s);
/* gs_verify.hip: rows of a device-resident suffix array that are out of range or repeat a value */
gs_status gs_count_bad_sa_rows(const uint32_t *d_sa, uint64_t n, hipStream_t st, uint64_t *bad);

/* SDSL importer (gs_sdsl_import.cpp): reads <path> into BWT bytes + SA samples */
gs_status gs_sdsl_read(const char *path, std::vector<uint8_t> &bwt, std::vector<uint64_t> &sa_samples,
                       uint64_t C256[257]);

/* gs_suffix.hip: the same suffix array by doubling over the rows whose groups still have company only */
gs_status gs_device_suffix_array_discarding(const uint8_t *d_text, uint64_t n, uint32_t *d_sa, hipStream_t st, bool debug);

/* k_order / k_locate (gs_order.hip): guides one wave takes at a time, a lane each for the ones that need no wave - as
 * many as still leave every wave of the chip a group (the guides of a group that DO need the wave are served one after
 * the other) */
static inline __host__ __device__ uint32_t gs_lane_group(uint32_t n_guides) {
  uint32_t g = 64;
  while (g > 1 && (n_guides + g - 1) / g < 8192u) g >>= 1;
  return g;
}

#endif
