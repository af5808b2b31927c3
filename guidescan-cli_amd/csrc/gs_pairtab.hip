/*
 * gs_pairtab.hip -- PAM-pair tables: the depth-k prefix table of a strand restricted to the rows that
 * can host a site of a PAM ending in a given pair of bases.
 *
 * This strand's seeds of k_search (gs_search.hip) are depth-k intervals of all rows whose suffix starts
 * with a variant of the guide's first k consumed symbols; what decides a row is the v_rem symbols to
 * its left: the rest of the guide, then the PAM (index.hpp:182-248 walk the same symbols one by
 * one).  The last two consumed PAM symbols of NGG, NAG, TTTN (--start) ... are concrete bases, so
 * only the rows with exactly that pair at context offsets v_rem-2, v_rem-1 can hold a site: one row in
 * sixteen.  Collecting those rows per k-mer gives a table of the same shape whose intervals hold
 * 0.7 rows instead of 11.5 at hg38 size: half the entries are empty (the seed dies with the table
 * read), a third hold one row whose context symbols sit in the entry itself (no second read), the
 * rest are filtered by per-position symbol sets over their few rows.  Entries are 8 bytes
 * (gs_common.h, gs_pairtab_dev): the 16 two-symbol extensions of a variant are one 128-byte block.  Rows with a symbol outside A,C,G,T among
 * the nearest v_rem are left out: k_search reports those sites from the literal-N window list.
 * Derived data, built on the device from the strand's table and ctx[] on first use (~0.1 s at hg38
 * size), 4.3 GB per table copy + 10 bytes per selected row.
 *
 * The spaced table of a pair table (gs_seed.hip reads it): the same rows sorted by what a site that spent its whole
 * budget inside O - the k-mer's symbols behind X - still shares with its guide: X and R.  One lookup keyed on (X, R)
 * answers what C(|O|, m) 3^m seeds of the class (no substitution in X, m in O) ask one table entry each.
 */
#include "gs_device.h"
#include "gs_scratch.h"

#include <algorithm>
#include <rocprim/rocprim.hpp>

struct pt_args {
  const uint4 *tab;
  const uint32_t *ctx;
  const uint32_t *exc_row;
  const uint64_t *exc_sym;
  uint32_t n_exc;
  uint32_t v_rem, code, mask_off;
  uint64_t entries;
  /* outputs */
  uint32_t *count;       /* per k-mer: selected rows */
  const uint32_t *start; /* exclusive sums of count[] */
  uint2 *out;
  uint16_t *c16;
  uint32_t *octx, *rowid;
};

/* does row r (context word w) belong to the pair's table? */
__device__ __forceinline__ bool pt_selected(const pt_args &a, uint32_t r, uint32_t w, bool flagged) {
  if (((w >> (2u * (a.v_rem - 2u))) & 15u) != a.code) return false;
  if (flagged) { /* the k-mer has exception rows: is this one, and is the symbol near enough to matter? */
    uint32_t lo = 0, hi = a.n_exc;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.exc_row[mid] < r)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < a.n_exc && a.exc_row[lo] == r) {
      const uint64_t nb = a.exc_sym[lo];
      for (uint32_t j = 0; j < a.v_rem; j++)
        if (((nb >> (4u * j)) & 15u) > 3u) return false;
    }
  }
  return true;
}

__global__ void k_pt_count(pt_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.entries) return;
  const uint4 e = a.tab[i];
  const uint32_t cnt = e.y & 0x7FFFFFFFu;
  const bool flagged = (e.y >> 31) != 0u;
  uint32_t c = 0;
  for (uint32_t j = 0; j < cnt; j++) c += pt_selected(a, e.x + j, a.ctx[e.x + j], flagged) ? 1u : 0u;
  a.count[i] = c + (c >= GS_PT_BIG ? 1u : 0u); /* slots in the row arrays: a header slot in front of 63 rows and more */
}

__global__ void k_pt_fill(pt_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.entries) return;
  const uint32_t slots = a.count[i];
  uint32_t at = a.start[i];
  uint2 o = make_uint2(at, 0u);
  if (slots) {
    const uint4 e = a.tab[i];
    const uint32_t cnt = e.y & 0x7FFFFFFFu;
    const bool flagged = (e.y >> 31) != 0u;
    const bool big = slots > GS_PT_BIG; /* 63 rows and more: header slot + rows */
    const uint32_t mine = big ? slots - 1u : slots;
    if (big) {
      a.c16[at] = 0;
      a.octx[at] = 0;
      a.rowid[at] = mine;
      at++;
    }
    uint32_t c = 0, sets = 0, lw = 0;
    for (uint32_t j = 0; j < cnt && c < mine; j++) {
      const uint32_t r = e.x + j, w = a.ctx[r];
      if (!pt_selected(a, r, w, flagged)) continue;
      a.c16[at + c] = (uint16_t)w;
      a.octx[at + c] = w;
      a.rowid[at + c] = r;
      for (uint32_t p = 0; p < 6u; p++) sets |= 1u << (4u * p + ((w >> (2u * p)) & 3u));
      lw = w;
      c++;
    }
    o.y = (big ? GS_PT_BIG : mine) | ((mine == 1u ? (lw & 0x3FFFFFFu) : sets) << 6);
  }
  a.out[i] = o;
}

/* rot[slot][perm_p(i)] = tab[i]: the field of consumption step p moves to bits 1:0 (gs_index.hip k_rot_copy) */
__global__ void k_pt_rot(const uint2 *tab, uint2 *rot, uint32_t k, uint32_t p, uint32_t slot) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> (2 * k)) return;
  const uint32_t sh = 2u * (k - 1u - p);
  const uint64_t hi = i >> (sh + 2u), lo = i & ((1ull << sh) - 1ull), f = (i >> sh) & 3ull;
  rot[((uint64_t)slot << (2 * k)) + ((hi << (sh + 2u)) | (lo << 2) | f)] = tab[i];
}

/* ---- the other strand's side: tables deeper by the PAM's free symbol ----------------------------------
 * Under two-sided seeding the sites with many substitutions among a guide's first consumed symbols
 * come from the OTHER strand's table, whose backward search consumes the PAM first: k-mer = P PAM
 * symbols + k-P guide symbols, one lookup per base a PAM 'N' can stand for.  For a PAM of three symbols
 * that ends (as this strand consumes it) in the pair `code`, the deep table is indexed by k-2 guide
 * symbols and, in the lowest two bits, the base under the N: entry = the interval of the rows that
 * start with those k+1 symbols - a quarter of the rows of a depth-k interval - in the strand table's
 * own format {first row, rows | flag << 31, pair masks over these rows (context offsets 0, 2, 4, 6)}.
 * The four entries of one (k-2)-mer are one 64-byte line; with 2.9 rows behind a mask instead of
 * 11.5 few seeds survive it.  The rows are rows of the strand's own suffix array: verification reads
 * the strand's ctx16[] / ctx[] as before.  4^(k-2) x 64 bytes: 1.07 GB per strand at k = 14. */
struct pb_args {
  gs_strand_dev sd;
  uint32_t k, P, code; /* code as this strand's consumption sees the pair: first | second << 2 */
  uint32_t kb;         /* guide symbols of the index: k-P .. 14 */
  uint64_t entries;    /* 4^kb */
  uint4 *out;          /* 4 per entry */
};

__global__ void k_pb_build(pb_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.entries) return;
  const uint32_t k = a.k, P = a.P, kb = a.kb;
  /* the first k consumed symbols: the pair (second consumed PAM symbol of this strand first), the base
   * under the N, then the k-P leading symbols of the entry */
  const uint32_t c0 = a.code & 3u, c1 = (a.code >> 2) & 3u;
  uint32_t head = ((3u - c1) << (2u * (k - 1u))) | ((3u - c0) << (2u * (k - 2u)));
  for (uint32_t y = 0; y < k - P; y++) head |= (uint32_t)((i >> (2u * (kb - 1u - y))) & 3u) << (2u * (k - 1u - P - y));
  for (uint32_t x = 0; x < 4u; x++) {
    const uint4 e = a.sd.ptab[head | (x << (2u * (k - 3u)))];
    uint32_t lo = e.x, cnt = e.y & 0x7FFFFFFFu;
    bool blind = (e.y >> 31) != 0u; /* exception rows somewhere in the depth-k interval: verify, do not filter */
    for (uint32_t y = k - P; y < kb && cnt; y++) { /* the symbols the depth-k table does not reach */
      const uint32_t c = (uint32_t)((i >> (2u * (kb - 1u - y))) & 3u);
      const uint32_t hi = lo + cnt - 1u;
      const uint32_t oa = occ1(a.sd.blocks, lo >> GS_BLOCK_SHIFT, lo & (GS_BLOCK_ROWS - 1u), c);
      const uint32_t ob = occ1(a.sd.blocks, hi >> GS_BLOCK_SHIFT, (hi & (GS_BLOCK_ROWS - 1u)) + 1u, c);
      lo = a.sd.C[c] + oa;
      cnt = ob - oa;
    }
    if (cnt > 4096u) blind = true; /* too many rows to scan here */
    uint32_t mz = 0, mw = 0;
    if (cnt && !blind)
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t w = a.sd.ctx[lo + j];
        mz |= (1u << (w & 15u)) | (1u << (16u + ((w >> 4) & 15u)));
        mw |= (1u << ((w >> 8) & 15u)) | (1u << (16u + ((w >> 12) & 15u)));
      }
    a.out[4 * i + x] = make_uint4(lo, cnt | (blind && cnt ? 0x80000000u : 0u), mz, mw);
  }
}

void gs_pairtab_free(gs_index *ix, uint32_t slot) {
  gs_pairtab_host &p = ix->pairtab[slot];
  p.own.clear();
  p.valid = false;
  p.deep = false;
  p.spaced = false;
  p.d[0] = gs_pairtab_dev{};
  p.d[1] = gs_pairtab_dev{};
}

/* start[] = the exclusive sums of count[] over `entries` entries (the scan's temporary comes from mem and goes back);
 * *total = their sum */
static gs_status scan_counts(gs_scratch &mem, uint32_t *count, uint32_t *start, uint64_t entries, hipStream_t st, uint64_t *total) {
  gs_prim_tmp tmp;
  GS_TRY(gs_prim("scan_counts", mem, tmp, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, count, start, 0u, entries, rocprim::plus<uint32_t>(), st);
  }));
  uint32_t last_start = 0, last_count = 0;
  GS_HIP(hipMemcpyAsync(&last_start, start + entries - 1, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(&last_count, count + entries - 1, 4, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  mem.drop(tmp.p);
  *total = (uint64_t)last_start + last_count;
  return GS_OK;
}

static gs_status build_one(gs_index *ix, gs_pairtab_host &p, int s, uint32_t k, uint32_t rot_from, hipStream_t st) {
  const gs_strand &S = ix->strand[s];
  const uint64_t entries = 1ull << (2 * k);
  pt_args a;
  memset(&a, 0, sizeof(a));
  a.tab = S.d.ptab;
  a.ctx = S.d.ctx;
  a.exc_row = S.d.exc_row;
  a.exc_sym = S.d.exc_sym;
  a.n_exc = S.d.n_exc;
  a.v_rem = p.v_rem;
  a.code = p.code;
  a.mask_off = S.d.mask_off;
  a.entries = entries;
  gs_scratch mem; /* the temporaries, and each array until the slot has it */
  uint32_t *d_count = nullptr, *d_start = nullptr;
  GS_TRY(mem.get(4 * entries, &d_count));
  GS_TRY(mem.get(4 * entries, &d_start));
  a.count = d_count;
  const uint32_t nb = (uint32_t)((entries + 255) / 256);
  hipLaunchKernelGGL(k_pt_count, dim3(nb), dim3(256), 0, st, a);
  uint64_t rows = 0;
  GS_TRY(scan_counts(mem, d_count, d_start, entries, st, &rows));
  const uint32_t nrot = rot_from + 2 < k ? k - 2 - rot_from : 0; /* steps rot_from .. k-3 (step k-2's variants sit in the plain table's 128-byte blocks) */
  uint2 *tab = nullptr, *rot = nullptr;
  uint16_t *c16 = nullptr;
  uint32_t *octx = nullptr, *rowid = nullptr;
  GS_TRY(mem.get(sizeof(uint2) * entries, &tab));
  GS_TRY(mem.get(2 * rows + 64, &c16));
  GS_TRY(mem.get(4 * rows, &octx));
  GS_TRY(mem.get(4 * rows, &rowid));
  if (nrot) GS_TRY(mem.get(sizeof(uint2) * entries * nrot, &rot));
  GS_HIP(hipMemsetAsync(c16, 0, 2 * rows + 64, st)); /* k_search reads whole groups of eight */
  a.start = d_start;
  a.out = tab;
  a.c16 = c16;
  a.octx = octx;
  a.rowid = rowid;
  hipLaunchKernelGGL(k_pt_fill, dim3(nb), dim3(256), 0, st, a);
  for (uint32_t j = 0; j < nrot; j++)
    hipLaunchKernelGGL(k_pt_rot, dim3(nb), dim3(256), 0, st, (const uint2 *)tab, rot, k, rot_from + j, j);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  gs_pairtab_dev &d = p.d[s];
  p.own.take(mem, d.tab, tab, sizeof(uint2) * entries);
  p.own.take(mem, d.rot, rot, sizeof(uint2) * entries * nrot);
  p.own.take(mem, d.c16, c16, 2 * rows);
  p.own.take(mem, d.ctx, octx, 4 * rows);
  p.own.take(mem, d.rowid, rowid, 4 * rows);
  d.rot_first = nrot ? rot_from : 31u;
  d.code = p.code;
  p.n_slots[s] = rows;
  if (gs_opt(ix, "GS_DEBUG"))
    fprintf(stderr, "[gs] PAM-pair table: strand %d, pair %u at context depth %u: %llu of %llu rows, %u rotated copies, %.2f GB\n",
            s, p.code, p.v_rem, (unsigned long long)rows, (unsigned long long)S.n, nrot,
            1e-9 * (double)(sizeof(uint2) * entries * (1 + nrot) + 10 * rows));
  return GS_OK;
}

/* the deep table of strand s for the pair (built after the pair table proper; optional) */
static gs_status build_deep(gs_index *ix, gs_pairtab_host &p, int s, uint32_t k, uint32_t P, uint32_t kb, hipStream_t st) {
  const gs_strand &S = ix->strand[s];
  const uint64_t entries = 1ull << (2 * kb);
  gs_scratch mem;
  uint4 *deep = nullptr;
  GS_TRY(mem.get(64 * entries, &deep));
  pb_args a;
  memset(&a, 0, sizeof(a));
  a.sd = S.d;
  a.k = k;
  a.P = P;
  a.kb = kb;
  a.code = p.code;
  a.entries = entries;
  a.out = deep;
  hipLaunchKernelGGL(k_pb_build, dim3((uint32_t)((entries + 255) / 256)), dim3(256), 0, st, a);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  p.own.take(mem, p.d[s].deep, deep, 64 * entries);
  if (gs_opt(ix, "GS_DEBUG"))
    fprintf(stderr, "[gs] deep table: strand %d, pair %u: %llu lines of four entries, %.2f GB\n", s, p.code,
            (unsigned long long)entries, 1e-9 * (double)(64 * entries));
  return GS_OK;
}

gs_status gs_pairtab_ensure(gs_index *ix, uint32_t slot, uint32_t v_rem, uint32_t code, uint32_t rot_first, double share,
                            hipStream_t st) {
  gs_pairtab_host &p = ix->pairtab[slot];
  const uint32_t k = ix->pt_k;
  if (rot_first > 31) rot_first = 31;
  const uint32_t rot_wanted = rot_first;
  if (p.valid && p.v_rem == v_rem && p.code == code && p.rot_first <= rot_wanted) return GS_OK;
  gs_pairtab_free(ix, slot);
  if (!k || v_rem < 2 || v_rem > 16 || !ix->strand[0].d.ctx || !ix->strand[1].d.ctx) return GS_OK;
  /* fit into what is free, keeping room for the batch workspace: drop rotated copies first */
  size_t free_b = 0, total_b = 0;
  GS_HIP(hipMemGetInfo(&free_b, &total_b));
  const double entry_bytes = 8.0 * (double)(1ull << (2 * k));
  double reserve = 64e9; /* slots, sort buffers and hits of a large batch at a high budget */
  if (const char *e = gs_opt(ix, "GS_PAIRTAB_RESERVE_GB")) reserve = atof(e) * 1e9;
  if (reserve > 0.25 * (double)total_b) reserve = 0.25 * (double)total_b;
  const double rows_bytes = 10.0 * ((double)ix->strand[0].n + (double)ix->strand[1].n) / 16.0 * 1.5;
  const double tmp_bytes = 8.0 * (double)(1ull << (2 * k)) + 64e6;
  double room = (double)free_b - reserve;
  if (const char *e = gs_opt(ix, "GS_INDEX_BUDGET_GB")) { /* the cap on the whole index covers its derived tables too */
    const double left = atof(e) * 1e9 - (double)gs_index_device_bytes(ix);
    if (left < room) room = left;
  }
  for (;;) {
    const uint32_t nrot = rot_first + 2 < k ? k - 2 - rot_first : 0;
    const double need = 2.0 * entry_bytes * (1 + nrot) + rows_bytes + tmp_bytes;
    if (need <= room * share) break; /* share < 1: another pair's tables are still to come */
    if (nrot == 0) {
      if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] PAM-pair table %u: not enough free memory (%.1f GB), skipped\n", code, 1e-9 * (double)free_b);
      return GS_OK;
    }
    rot_first = nrot == 1 ? 31 : rot_first + 1;
  }
  p.v_rem = v_rem;
  p.code = code;
  p.rot_first = rot_wanted;
  for (int s = 0; s < 2; s++) {
    const gs_status rc = build_one(ix, p, s, k, rot_first, st);
    if (rc == GS_ERR_NOMEM) { /* the estimate was off: go on without this table */
      gs_pairtab_free(ix, slot);
      return GS_OK;
    }
    if (rc != GS_OK) {
      gs_pairtab_free(ix, slot);
      return rc;
    }
  }
  p.valid = true;
  return GS_OK;
}

gs_status gs_pairtab_ensure_deep(gs_index *ix, uint32_t slot, uint32_t P, uint32_t kb, hipStream_t st) {
  gs_pairtab_host &p = ix->pairtab[slot];
  const uint32_t k = ix->pt_k;
  if (!p.valid || P != 3 || k < 6 || kb + P < k || kb > 14) return GS_OK;
  if (p.deep && p.deep_P == P && p.deep_kb == kb) return GS_OK;
  auto drop = [&]() {
    for (int s = 0; s < 2; s++) p.own.release(p.d[s].deep);
    p.deep = false;
  };
  drop();
  size_t free_b = 0, total_b = 0;
  GS_HIP(hipMemGetInfo(&free_b, &total_b));
  double reserve = 56e9;
  if (const char *e = gs_opt(ix, "GS_PAIRTAB_RESERVE_GB")) reserve = atof(e) * 1e9;
  if (reserve > 0.25 * (double)total_b) reserve = 0.25 * (double)total_b;
  if (2.0 * 64.0 * (double)(1ull << (2 * kb)) + reserve > (double)free_b) return GS_OK;
  for (int s = 0; s < 2; s++) {
    const gs_status rc = build_deep(ix, p, s, k, P, kb, st);
    if (rc != GS_OK) {
      drop();
      return rc == GS_ERR_NOMEM ? GS_OK : rc;
    }
  }
  p.deep = true;
  p.deep_P = P;
  p.deep_kb = kb;
  return GS_OK;
}

/* ---- the spaced table: the pair table's rows by (X symbols of the k-mer, R symbols of the context) -------------------
 * key = X << 2g | ctx & mask(g), X = the index's highest 2 x_len bits (consumption steps 0 .. x_len-1), g = L - k; payload =
 * {row in the row arrays, O symbols (the index's other bits) << rem | the key's low rem bits}.  Sorted by key; the offsets
 * array is direct-addressed by the key's top d bits, d from the number of rows (2^d >= rows), so the layout serves keys of
 * any width up to 32 bits: the `rem` bits below are stored with the row and compared by the reader. */
struct sp_args {
  const uint2 *tab;
  const uint32_t *ctx, *rowid;
  uint32_t k, x_len, g, rem;
  uint64_t entries;
  uint32_t *count;
  const uint32_t *start;
  uint32_t *keys;
  uint64_t *vals;
};
/* the rows of entry e: where they start and how many (a big entry's header slot is not a row) */
__device__ __forceinline__ uint32_t sp_entry_rows(const sp_args &a, const uint2 e, uint32_t &first) {
  uint32_t cnt = e.y & 63u;
  first = e.x;
  if (cnt == GS_PT_BIG) {
    cnt = a.rowid[first];
    first += 1u;
  }
  return cnt;
}
__global__ void k_sp_count(sp_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.entries) return;
  uint32_t first;
  a.count[i] = sp_entry_rows(a, a.tab[i], first);
}
/* a lane per entry; the rows of a big entry (63 .. 10^5 on a repeat-rich genome) are written by the whole wave, 64 at a time */
__global__ void k_sp_fill(sp_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < a.entries;
  const uint32_t cnt = in ? a.count[i] : 0u;
  uint32_t first = 0;
  if (cnt) (void)sp_entry_rows(a, a.tab[i], first);
  const uint32_t at = cnt ? a.start[i] : 0u;
  const uint32_t obits = 2u * (a.k - a.x_len), gmask = a.g >= 16u ? 0xFFFFFFFFu : ((1u << (2u * a.g)) - 1u);
  const uint32_t remmask = (1u << a.rem) - 1u;
  auto put = [&](uint32_t e, uint32_t e_first, uint32_t e_at, uint32_t j) {
    const uint32_t x = e >> obits, o = e & ((1u << obits) - 1u), r = e_first + j;
    const uint32_t key = (a.g >= 16u ? 0u : x << (2u * a.g)) | (a.ctx[r] & gmask);
    a.keys[e_at + j] = key;
    a.vals[e_at + j] = (uint64_t)r | ((uint64_t)((o << a.rem) | (key & remmask)) << 32);
  };
  const bool big = cnt >= GS_PT_BIG;
  if (!big)
    for (uint32_t j = 0; j < cnt; j++) put((uint32_t)i, first, at, j);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t bb = __ballot(big); bb; bb &= bb - 1ull) {
    const int src = __builtin_ctzll(bb);
    const uint32_t e = (uint32_t)__shfl((int)(uint32_t)i, src), e_first = (uint32_t)__shfl((int)first, src);
    const uint32_t e_at = (uint32_t)__shfl((int)at, src), e_cnt = (uint32_t)__shfl((int)cnt, src);
    for (uint32_t j = lane; j < e_cnt; j += 64u) put(e, e_first, e_at, j);
  }
}
/* off[t] = the first sorted row whose key's top bits are >= t, t = 0 .. 2^d (row `rows` closes the last bucket) */
__global__ void k_sp_offsets(const uint32_t *keys, uint32_t rows, uint32_t rem, uint32_t d, uint32_t *off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > rows) return;
  const uint64_t top = i < rows ? (uint64_t)(keys[i] >> rem) : (1ull << d);
  const uint64_t from = i == 0 ? 0ull : (uint64_t)(keys[i - 1] >> rem) + 1ull;
  for (uint64_t t = from; t <= top; t++) off[t] = (uint32_t)i;
}

bool gs_pairtab_free_spaced(gs_index *ix, uint32_t slot) {
  gs_pairtab_host &p = ix->pairtab[slot];
  bool any = false;
  for (int s = 0; s < 2; s++) {
    any |= p.d[s].sp_off || p.d[s].sp_rows;
    p.own.release(p.d[s].sp_off);
    p.own.release(p.d[s].sp_rows);
    p.d[s].sp_rem = 0;
  }
  p.spaced = false;
  return any;
}

/* the direct part's bits for a table of `rows` rows whose keys have key_bits bits and whose payload keeps obits bits of O:
 * 2^d >= rows, at most 2^28 offsets, and what the payload's second word has to hold (O, the other key bits) fits 32 bits;
 * 0: no such d.  forced != 0 (GS_SPACED_BITS): that d instead of the one the row count gives, under the same three limits - a
 * small genome then gets the key split of a large one (d = the whole key, no key bits with the row) or the smallest legal d */
static uint32_t sp_direct_bits(uint64_t rows, uint32_t key_bits, uint32_t obits, uint32_t forced) {
  uint32_t d = 8;
  while (d < 28 && (1ull << d) < rows) d++;
  if (forced) d = forced < 28u ? forced : 28u;
  if (d > key_bits) d = key_bits;
  if (key_bits - d + obits > 32u) d = key_bits + obits - 32u;
  return d >= 1 && d <= 28 && d <= key_bits ? d : 0u;
}

static gs_status build_spaced(gs_index *ix, gs_pairtab_host &p, int s, uint32_t k, uint32_t x_len, uint32_t g, uint32_t forced_d,
                              hipStream_t st) {
  const uint64_t entries = 1ull << (2 * k);
  const uint32_t key_bits = 2u * (x_len + g), obits = 2u * (k - x_len);
  gs_scratch mem; /* the temporaries, and both arrays until the slot has them */
  uint32_t *d_count = nullptr, *d_start = nullptr, *d_keys = nullptr, *d_keys2 = nullptr, *sp_off = nullptr;
  uint64_t *d_vals = nullptr, *sp_rows = nullptr;
  GS_TRY(mem.get(4 * entries, &d_count));
  GS_TRY(mem.get(4 * entries, &d_start));
  sp_args a;
  memset(&a, 0, sizeof(a));
  a.tab = p.d[s].tab;
  a.ctx = p.d[s].ctx;
  a.rowid = p.d[s].rowid;
  a.k = k;
  a.x_len = x_len;
  a.g = g;
  a.entries = entries;
  a.count = d_count;
  const uint32_t nb = (uint32_t)((entries + 255) / 256);
  hipLaunchKernelGGL(k_sp_count, dim3(nb), dim3(256), 0, st, a);
  /* the rows are the slots of the pair table's row arrays without the header slots: the builder's own count bounds them, so
   * the 32-bit scan cannot have wrapped unseen */
  uint64_t rows = 0;
  GS_TRY(scan_counts(mem, d_count, d_start, entries, st, &rows));
  if (p.n_slots[s] >= 0xFFFFFFFFull || rows > p.n_slots[s]) return GS_ERR_UNSUPPORTED;
  const uint32_t d = sp_direct_bits(rows, key_bits, obits, forced_d);
  if (!d) return GS_ERR_UNSUPPORTED;
  const uint32_t rem = key_bits - d;
  GS_TRY(mem.get(4 * rows, &d_keys));
  GS_TRY(mem.get(4 * rows, &d_keys2));
  GS_TRY(mem.get(8 * rows, &d_vals));
  GS_TRY(mem.get(8 * rows, &sp_rows));
  GS_TRY(mem.get(4 * ((1ull << d) + 1), &sp_off));
  a.start = d_start;
  a.rem = rem;
  a.keys = d_keys;
  a.vals = d_vals;
  hipLaunchKernelGGL(k_sp_fill, dim3(nb), dim3(256), 0, st, a);
  if (rows) {
    gs_prim_tmp tmp;
    GS_TRY(gs_prim("spaced table: sort", mem, tmp, [&](void *t, size_t &tb) {
      return rocprim::radix_sort_pairs(t, tb, d_keys, d_keys2, d_vals, sp_rows, rows, 0, key_bits, st);
    }));
  }
  hipLaunchKernelGGL(k_sp_offsets, dim3((uint32_t)((rows + 1 + 255) / 256)), dim3(256), 0, st, (const uint32_t *)d_keys2, (uint32_t)rows, rem, d,
                     sp_off);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  gs_pairtab_dev &dv = p.d[s];
  p.own.take(mem, dv.sp_off, sp_off, 4 * ((1ull << d) + 1));
  p.own.take(mem, dv.sp_rows, sp_rows, 8 * rows + 16);
  dv.sp_rem = rem;
  p.sp_rows[s] = rows;
  const uint64_t bytes = 8 * rows + 16 + 4 * ((1ull << d) + 1);
  if (gs_opt(ix, "GS_DEBUG"))
    fprintf(stderr, "[gs] spaced table: strand %d, pair %u: %llu rows by %u key bits (|X|=%u, |R|=%u), %u direct, %.2f GB\n", s, p.code,
            (unsigned long long)rows, key_bits, x_len, g, d, 1e-9 * (double)bytes);
  return GS_OK;
}

gs_status gs_pairtab_ensure_spaced(gs_index *ix, uint32_t slot, uint32_t x_len, uint32_t g, hipStream_t st) {
  gs_pairtab_host &p = ix->pairtab[slot];
  const uint32_t k = ix->pt_k;
  if (!p.valid) return GS_OK;
  /* GS_SPACED_BITS: the direct part's bits asked for (0: from the row count); tables built under another value are built anew */
  uint32_t forced_d = 0;
  if (const char *e = gs_opt(ix, "GS_SPACED_BITS")) forced_d = (uint32_t)std::min(32l, std::max(1l, atol(e)));
  if (p.spaced && p.sp_x == x_len && p.sp_g == g && p.sp_forced_d == forced_d) return GS_OK;
  gs_pairtab_free_spaced(ix, slot);
  if (k < 4 || x_len < 1 || x_len + 2 > k || g < 1 || 2 * (x_len + g) > 32 || g > 16) return GS_OK;
  /* what the finished tables take (8 bytes per row and the offsets, both strands) and the sort's buffers while one is built */
  const double rows_est = ((double)ix->strand[0].n + (double)ix->strand[1].n) / 16.0 * 1.5;
  const double keep = 8.0 * rows_est + 2.0 * 4.0 * (double)(1ull << std::min(28u, 2u * (x_len + g)));
  const double tmp = 8.0 * (double)(1ull << (2 * k)) + 24.0 * rows_est / 2.0 + 64e6;
  size_t free_b = 0, total_b = 0;
  GS_HIP(hipMemGetInfo(&free_b, &total_b));
  double reserve = 64e9;
  if (const char *e = gs_opt(ix, "GS_PAIRTAB_RESERVE_GB")) reserve = atof(e) * 1e9;
  if (reserve > 0.25 * (double)total_b) reserve = 0.25 * (double)total_b;
  double room = (double)free_b - reserve;
  if (const char *e = gs_opt(ix, "GS_INDEX_BUDGET_GB")) {
    const double left = atof(e) * 1e9 - (double)gs_index_device_bytes(ix);
    if (left < room) room = left;
  }
  if (keep + tmp > room) {
    if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] spaced table %u: not enough free memory (%.1f GB), skipped\n", p.code, 1e-9 * (double)free_b);
    return GS_OK;
  }
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
  if (timed) (void)hipEventRecord(ev[0], st);
  gs_status rc = GS_OK;
  for (int s = 0; s < 2 && rc == GS_OK; s++) rc = build_spaced(ix, p, s, k, x_len, g, forced_d, st);
  if (timed) {
    float ms = 0.f;
    (void)hipEventRecord(ev[1], st);
    (void)hipEventSynchronize(ev[1]);
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    p.sp_build_ms = ms;
  }
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  (void)hipGetLastError();
  if (rc != GS_OK) {
    gs_pairtab_free_spaced(ix, slot);
    return rc == GS_ERR_NOMEM || rc == GS_ERR_UNSUPPORTED ? GS_OK : rc; /* the batch goes on without them */
  }
  p.spaced = true;
  p.sp_x = x_len;
  p.sp_g = g;
  p.sp_forced_d = forced_d;
  if (gs_opt(ix, "GS_DEBUG")) fprintf(stderr, "[gs] spaced tables of pair %u: %.2f GB, built in %.1f ms\n", p.code, 1e-9 * (double)p.sp_bytes(), p.sp_build_ms);
  return GS_OK;
}

/* tests: the rows under `key` in the spaced table of (slot, strand): four words per row {row in the row arrays, O symbols,
 * row of the strand's suffix array, context word}; info = {built, pair code, context depth, |X|, |R|, table depth k, key bits
 * stored with the row, rows of the table} */
extern "C" gs_status gs_debug_spaced_rows(gs_index *ix, uint32_t slot, int strand, uint32_t key, uint32_t *out, uint64_t cap, uint64_t *n,
                                          uint32_t info[8]) {
  GS_HANDLE_LOCK(ix);
  if (!ix || slot > 1 || strand < 0 || strand > 1 || !n || !info || (cap && !out)) return GS_ERR_ARG;
  const gs_pairtab_host &p = ix->pairtab[slot];
  const gs_pairtab_dev &d = p.d[strand];
  const uint32_t inf[8] = {p.valid && p.spaced ? 1u : 0u, p.code, p.v_rem, p.sp_x, p.sp_g, ix->pt_k, d.sp_rem, (uint32_t)p.sp_rows[strand]};
  memcpy(info, inf, sizeof(inf));
  *n = 0;
  if (!inf[0]) return GS_OK;
  const uint32_t key_bits = 2u * (p.sp_x + p.sp_g);
  if (key_bits < 32u && (key >> key_bits) != 0u) return GS_ERR_ARG;
  GS_HIP(hipSetDevice(ix->device));
  uint32_t off[2] = {0, 0};
  GS_HIP(hipMemcpy(off, d.sp_off + (key >> d.sp_rem), 8, hipMemcpyDeviceToHost));
  if (off[1] < off[0] || off[1] > p.sp_rows[strand]) return GS_ERR_DEVICE;
  std::vector<uint2> rows(off[1] - off[0]);
  if (!rows.empty()) GS_HIP(hipMemcpy(rows.data(), d.sp_rows + off[0], 8 * rows.size(), hipMemcpyDeviceToHost));
  const uint32_t remmask = (1u << d.sp_rem) - 1u;
  for (const uint2 &r : rows) {
    if ((r.y & remmask) != (key & remmask)) continue;
    if (*n < cap) {
      uint32_t w[2] = {0, 0};
      GS_HIP(hipMemcpy(&w[0], d.rowid + r.x, 4, hipMemcpyDeviceToHost));
      GS_HIP(hipMemcpy(&w[1], d.ctx + r.x, 4, hipMemcpyDeviceToHost));
      uint32_t *o = out + 4 * *n;
      o[0] = r.x;
      o[1] = r.y >> d.sp_rem;
      o[2] = w[0];
      o[3] = w[1];
    }
    (*n)++;
  }
  return GS_OK;
}

/* tests (gs_debug_index_layout, gs_debug_index_array): the scalars and the arrays of one slot and strand as they lie in HBM */
gs_status gs_debug_pairtab_layout(const gs_index *ix, uint32_t slot, int strand, uint64_t out[32]) {
  const gs_pairtab_host &p = ix->pairtab[slot];
  const gs_pairtab_dev &d = p.d[strand];
  const uint32_t k = ix->pt_k;
  out[0] = p.valid ? 1 : 0;
  if (!p.valid) return GS_OK;
  out[1] = p.v_rem;
  out[2] = p.code;
  out[3] = d.rot_first;
  out[4] = d.rot && d.rot_first + 2 < k ? k - 2 - d.rot_first : 0;
  out[5] = p.n_slots[strand];
  out[6] = p.deep ? 1 : 0;
  out[7] = p.deep ? p.deep_P : 0;
  out[8] = p.deep ? p.deep_kb : 0;
  out[9] = p.spaced ? 1 : 0;
  if (p.spaced) {
    out[10] = p.sp_x;
    out[11] = p.sp_g;
    out[12] = d.sp_rem;
    out[13] = p.sp_rows[strand];
    out[14] = 2u * (p.sp_x + p.sp_g) - d.sp_rem; /* the offsets array is addressed by the key's top d bits */
  }
  out[15] = k;
  return GS_OK;
}
gs_status gs_debug_pairtab_array(const gs_index *ix, uint32_t slot, int strand, const char *which, uint64_t offset_bytes, void *out,
                                 uint64_t cap_bytes, uint64_t *total_bytes) {
  uint64_t lay[32] = {0};
  GS_TRY(gs_debug_pairtab_layout(ix, slot, strand, lay));
  const gs_pairtab_dev &d = ix->pairtab[slot].d[strand];
  const uint64_t entries = 1ull << (2 * ix->pt_k), slots = lay[5];
  const struct {
    const char *name;
    const void *p;
    uint64_t bytes;
  } arrays[] = {
      {"tab", d.tab, sizeof(uint2) * entries},
      {"rot", d.rot, sizeof(uint2) * entries * lay[4]},
      {"c16", d.c16, 2 * slots + 64}, /* with the zeroed row groups' padding */
      {"ctx", d.ctx, 4 * slots},
      {"rowid", d.rowid, 4 * slots},
      {"deep", lay[6] ? d.deep : nullptr, 64ull << (2 * lay[8])},
      {"sp_off", lay[9] ? d.sp_off : nullptr, 4 * ((1ull << lay[14]) + 1)},
      {"sp_rows", lay[9] ? d.sp_rows : nullptr, 8 * lay[13]},
  };
  for (const auto &a : arrays)
    if (!strcmp(a.name, which)) return gs_debug_copy_array(ix, lay[0] ? a.p : nullptr, a.bytes, offset_bytes, out, cap_bytes, total_bytes);
  return GS_ERR_ARG;
}
