/* gs_bulge_step.h -- what the two forms of the bulge-aware search share: the node and record layouts, the kernels'
 * arguments, and the transition rules of the seeded form (gs_bulge.hip) as ONE __host__ __device__ function, gb_child.
 * The kernel calls it for every child slot of every node; so do the host-only debug entry points
 * (gs_debug_bulge_seeds, gs_debug_bulge_verify), whose CPU tests therefore pin the code the kernel runs. */
#ifndef GS_BULGE_STEP_H
#define GS_BULGE_STEP_H

#include "gs_common.h"

#define GSTACK 1024 /* 48-byte nodes per wave: 48 KB, three single-wave workgroups per CU.  (512 nodes, six per CU: the room a pop of
                        64 nodes needs - 11 children each - is never there, pops shrink to 17 lanes and the batch takes 3 x as long) */
#define GFAN 12     /* children one node can push: 4 DNA-bulge + exact + 4 substitutions + RNA bulge + PAM hop (+1) */

/* state word: t[5:0] mm[8:6] dna[11:9] rna[14:12] bulge_type[16:15] curr[17] slen[23:18] pamid[28:24] inpam[29] hop[30] */
#define GM_T(m) ((m)&63u)
#define GM_MM(m) (((m) >> 6) & 7u)
#define GM_DNA(m) (((m) >> 9) & 7u)
#define GM_RNA(m) (((m) >> 12) & 7u)
#define GM_STATE(m) (((m) >> 15) & 3u)
#define GM_CURR(m) (((m) >> 17) & 1u)
#define GM_SLEN(m) (((m) >> 18) & 63u)
#define GM_PAMID(m) (((m) >> 24) & 31u)
#define GM_INPAM(m) (((m) >> 29) & 1u)
#define GM_HOP(m) (((m) >> 30) & 1u)
__host__ __device__ __forceinline__ uint32_t gm_make(uint32_t t, uint32_t mm, uint32_t dna, uint32_t rna, uint32_t state,
                                                     uint32_t curr, uint32_t slen, uint32_t pamid, uint32_t inpam,
                                                     uint32_t hop) {
  return t | (mm << 6) | (dna << 9) | (rna << 12) | (state << 15) | (curr << 17) | (slen << 18) | (pamid << 24) |
         (inpam << 29) | (hop << 30);
}

struct gs_gen_guide { /* one guide of the general path, prepared on the host */
  uint8_t q[32];      /* query bytes in consumption order (process.hpp:63, index.hpp:218) */
  uint8_t pam[8];     /* the guide's own PAM in consumption order */
};
struct gs_grec { /* one match, 48 bytes */
  uint32_t seq[8]; /* match.sequence, bytes packed big-endian: word order == std::string order */
  uint32_t sp, ep;
  /* mm[2:0] dna[5:3] rna[8:6] index[9] slen[15:10]; the seeded form's row records (sp == ep == the seed's row) add
   * ctx[20:16] = context symbols the match consumed beyond the seed - the match begins that many text symbols before
   * the row's suffix - and rowrec[21] */
  uint32_t meta;
  uint32_t g;
};
#define GREC_CTX(meta) (((meta) >> 16) & 31u)
#define GREC_ROW (1u << 21)

struct gs_gsearch_args {
  gs_strand_dev sd[2];
  const gs_gen_guide *guides;
  gs_grec *recs;             /* item s writes at recs[slot_off[s] ...]; nullptr = count only */
  const uint64_t *slot_off;
  /* slot_off == nullptr with recs: ONE pass - records go to recs[] in emission order through the counter pool_next
   * (the device-wide sort that follows orders by guide first, so an item's records need not be neighbours);
   * records beyond pool_cap are counted, not written: the host then runs the pass again with room for all */
  unsigned long long *pool_next;
  unsigned long long pool_cap;
  uint32_t *counts;
  uint32_t *work;   /* [0] work-queue head, [1] error flag (iteration bound hit), [4..5] pool_next, [8] the largest stack of any
                       item, [9] steps the room rule cut, [10] steps without room for one lane's children (gs_debug_general_last) */
  uint8_t alt[32][8]; /* alt PAM patterns in consumption order */
  uint8_t plen[40];   /* symbols of pattern j (alt PAMs, then the guides' own at n_alt): the reference searches
                         alt PAMs of any length next to the guides' PAM (process.hpp:51-56) */
  uint32_t p_max;     /* the longest of them */
  uint32_t n_items, L, P, m, n_alt, max_rna, max_dna;
  uint32_t max_iter; /* per-item iteration bound */
  uint32_t stack_cap; /* GS_GENERAL_STACK: `limit` is at most this many nodes (it can only lower the stack's use) */
  const uint32_t *glist; /* the guides this launch searches (n_items / 2 of them), or nullptr: every guide of the batch */
};

/* the seeded form's launch (gs_bulge.hip): the walk's arguments - same guides, pool and pattern list, a guide list and a
 * work area of its own - and the table depth.  bwork: [0] work-queue head, [1] error flags (1 the iteration bound, 2 a
 * push beyond the stack), [7] the largest stack; behind these 16 words five 64-bit counters (an item's share of each fits
 * 32 bits, a batch's does not): seeds looked up, seeds with an empty interval, row nodes made, interval nodes made,
 * exception-row lookups (gs_debug_bulge_last) */
struct gs_bsearch_args {
  gs_gsearch_args g;
  uint32_t *bwork;
  uint32_t k;    /* pt_k */
  uint32_t rows; /* GS_BULGE_ROWS: a seed with at most this many rows becomes row nodes */
};
gs_status gs_bulge_launch(const gs_bsearch_args &a, uint32_t grid, hipStream_t st);
/* GS_BULGE_ROWS when it is not set.  At hg38 size (k = 14, 11 rows per k-mer on average) every row of a seed is a node of
 * its own that dies within a step or two, where the interval dies as one node: 0 / 8 / 64 / 512 rows took 1.10 / 1.31 /
 * 3.61 / 3.54 s for 4,096 guides (profiles/bulge_seeded.json).  0 is the fastest there.  The default is 8 all the same, chosen
 * for coverage and not for speed: with 0 the form that is switched on would never read a context, and the form is not the
 * default anywhere, so its own default decides what an opt-in run exercises, not what users pay. */
#define GS_BULGE_ROWS_DEFAULT 8u

/* ---- the seeded form's nodes.  48 bytes as the walk's: {a, b, state word, w, sequence so far}.  w[17:16] says what a, b are:
 *   virtual   fewer than k genome symbols consumed: a = their 2-bit codes as a partial table index (step t at bits
 *             2(k-1-t), as k_estimate_heavy), b unused.  Reads nothing; all four bases are present.
 *   interval  a, b = sp, ep: walked with Occ exactly as k_search_general does.
 *   row       a = one row of the seed's interval; its 16-symbol left context still to be consumed as 3-bit symbols,
 *             nearest first (0..3 A,C,G,T, 4 'N', 5 any other symbol, 6 before the text start, the codes of
 *             gs_strand_dev::exc_sym): the low 32 bits in b, the high 16 in w[15:0].  Reads nothing: the next genome
 *             symbol is the lowest one, and only that one is present.
 *   chain     rows a..b of a seed's interval still to be made row nodes; GB_EXC: the table entry carried the flag,
 *             so the rows are looked up among the exception rows.  The kernel turns a chain node into the row node of
 *             a and the chain a+1..b before it asks for children: fan-out stays bounded whatever the interval holds.
 * GB_SEED marks a child that consumed the k-th genome symbol: a = its table index; the caller looks the entry up and
 * makes the child a chain or an interval node, or drops it when the k-mer is absent. */
#define GB_VIRTUAL 0u
#define GB_INTERVAL 1u
#define GB_ROW 2u
#define GB_CHAIN 3u
#define GB_KIND(w) (((w) >> 16) & 3u)
#define GB_W(kind) ((uint32_t)(kind) << 16)
#define GB_SEED (1u << 18)
#define GB_EXC (1u << 19)
#define GB_CHILDREN 11u /* child slots of gb_child: 0-3 DNA bulge with base c, 4-7 a consumed base c, 8 a literal N under a
                           pattern's N, 9 the hand-over to the PAM stage, 10 RNA bulge; a hop node uses 0 (this pattern's
                           PAM stage), 1 (the hop to the next pattern), 2 (an empty PAM: the match) */

struct gb_node {
  uint32_t a, b, meta, w;
  uint32_t seq[8];
};
struct gb_cfg {
  uint32_t L, P, m, n_alt, max_rna, max_dna, k;
};
/* what an interval node's caller read for it: bit c of present = base c extends the interval to lo[c]..hi[c];
 * c = 4 is a literal N (asked for only when gb_wants_n says so) */
struct gb_env {
  uint32_t present;
  uint32_t lo[5], hi[5];
};

__host__ __device__ __forceinline__ void gseq_append(uint32_t (&s)[8], uint32_t slen, uint32_t byte) {
  if (slen < 32u) s[slen >> 2] |= byte << (8u * (3u - (slen & 3u)));
}
__host__ __device__ __forceinline__ uint32_t glower(uint32_t b) { return b | 0x20u; } /* A,C,G,T -> a,c,g,t */

/* a row node's context from the 16 nibbles of an exception row / from ctx[r] */
__host__ __device__ __forceinline__ uint64_t gb_ctx_from_nibbles(uint64_t nib) {
  uint64_t v = 0;
  for (uint32_t j = 0; j < 16u; ++j) v |= ((nib >> (4u * j)) & 7ull) << (3u * j);
  return v;
}
__host__ __device__ __forceinline__ uint64_t gb_ctx_from_word(uint32_t w) {
  uint64_t v = 0;
  for (uint32_t j = 0; j < 16u; ++j) v |= (uint64_t)((w >> (2u * j)) & 3u) << (3u * j);
  return v;
}
__host__ __device__ __forceinline__ void gb_make_row(gb_node &n, uint32_t row, uint64_t ctx48) {
  n.a = row;
  n.b = (uint32_t)ctx48;
  n.w = GB_W(GB_ROW) | (uint32_t)((ctx48 >> 32) & 0xFFFFu);
}

/* the query symbol of a node's step: a guide byte, a byte of its pattern, or 0 (hop nodes, the finished guide).
 * S gives the batch's symbols: q(t) the guide's, own_pam(u), alt(j, u), plen(j) */
template <class S>
__host__ __device__ __forceinline__ uint32_t gb_query(const gb_cfg &c, const S &src, uint32_t meta) {
  const uint32_t t = GM_T(meta);
  if (GM_HOP(meta)) return 0u;
  if (GM_INPAM(meta)) return GM_PAMID(meta) < c.n_alt ? src.alt(GM_PAMID(meta), t - c.L) : src.own_pam(t - c.L);
  return t < c.L ? src.q(t) : 0u;
}
/* does this node try a literal N (index.hpp:139-149)?  Then an interval node's caller fills lo[4], hi[4] */
template <class S>
__host__ __device__ __forceinline__ bool gb_wants_n(const gb_cfg &c, const S &src, uint32_t meta) {
  return GM_INPAM(meta) && !GM_HOP(meta) && gb_query(c, src, meta) == 'N';
}

/* Child slot i of node n -> ch; live: the child exists; term: it is a match (its a, b, w are the parent's row or the
 * final interval).  The rules are k_search_general's, one by one: the DNA bulge before the terminal check
 * (index.hpp:265-295), the exact step and the substitutions under the budget (:316-356), the RNA bulge (:358-374), the
 * hop chain into the PAM stage (:297-314, process.hpp:51-56), a pattern's N as a literal N and then A,T,C,G at no
 * cost (:139-169).  Only where a consumed symbol leads differs with the node's kind. */
template <class S>
__host__ __device__ __forceinline__ void gb_child(const gb_cfg &c, const S &src, const gb_node &n, const gb_env &e,
                                                  uint32_t i, gb_node &ch, bool &live, bool &term) {
  const uint32_t BASES[5] = {'A', 'C', 'G', 'T', 'N'};
  const uint32_t meta = n.meta;
  const uint32_t t = GM_T(meta), mm = GM_MM(meta), dna = GM_DNA(meta), rna = GM_RNA(meta);
  const uint32_t state = GM_STATE(meta), curr = GM_CURR(meta), slen = GM_SLEN(meta), pamid = GM_PAMID(meta);
  const bool inpam = GM_INPAM(meta) != 0u, hop = GM_HOP(meta) != 0u;
  const uint32_t kind = GB_KIND(n.w);
  const uint32_t L = c.L, npams = c.P ? c.n_alt + 1u : 1u;
  ch = n;
  live = false;
  term = false;
  if (hop) {
    if (i == 0u) {
      live = c.P != 0u;
      ch.meta = gm_make(L, mm, dna, rna, state, curr, slen, pamid, 1u, 0u);
    } else if (i == 1u) {
      live = c.P != 0u && pamid + 1u < npams;
      ch.meta = gm_make(L, mm, dna, rna, state, curr, slen, pamid + 1u, 0u, 1u);
    } else if (i == 2u) {
      live = c.P == 0u; /* empty PAM: the finished guide is a match */
      term = true;
    }
    return;
  }
  const bool guide_node = !inpam;
  if (i == 9u) { /* the guide is consumed: hand over to the PAM stage */
    live = guide_node && t == L;
    ch.meta = gm_make(L, mm, dna, rna, state, curr, slen, 0u, 0u, 1u);
    return;
  }
  if (i == 10u) { /* RNA bulge child: a guide symbol skipped, the genome side unchanged, '.' recorded */
    uint32_t r_rna = rna, r_state = state, r_curr = curr;
    if (c.max_rna > rna && (state != 2u || curr == 1u)) {
      r_state = 2u;
      r_curr = 0u;
      r_rna = rna + 1u;
    }
    live = guide_node && t < L && r_state == 2u && r_curr < 1u && t != 0u;
    gseq_append(ch.seq, slen, '.');
    ch.meta = gm_make(t + 1u, mm, dna, r_rna, 2u, 1u, slen + 1u, 0u, 0u, 0u);
    return;
  }
  if (i > 10u) return;
  /* ---- a child that consumes genome symbol s (0..3 a base, 4 a literal N) */
  const uint32_t s = i < 4u ? i : i < 8u ? i - 4u : 4u;
  const uint32_t next = n.b & 7u; /* row node: the symbol before the text consumed so far */
  const uint32_t present = kind == GB_VIRTUAL ? 0xFu : kind == GB_INTERVAL ? e.present : next < 5u ? 1u << next : 0u;
  const bool here = ((present >> s) & 1u) != 0u;
  const uint32_t qc = gb_query(c, src, meta);
  if (i < 4u) { /* DNA bulge: genome base s consumed, guide position unchanged, lower case; never at the first step */
    uint32_t d_dna = dna, d_state = state, d_curr = curr;
    if (c.max_dna > dna && (state != 1u || curr == 1u)) {
      d_state = 1u;
      d_curr = 0u;
      d_dna = dna + 1u;
    }
    live = guide_node && d_state == 1u && d_curr < 1u && t != 0u && here;
    gseq_append(ch.seq, slen, glower(BASES[s]));
    ch.meta = gm_make(t, mm, d_dna, rna, 1u, 1u, slen + 1u, 0u, 0u, 0u);
  } else if (i < 8u) { /* guide step (exact, or a substitution under the budget) or PAM step (the pattern's base, or any under N) */
    const bool exact = qc == BASES[s];
    const bool wild = inpam && qc == 'N';
    live = inpam ? (here && (exact || wild)) : (t < L && here && (exact || mm < c.m));
    gseq_append(ch.seq, slen, (inpam || exact) ? BASES[s] : glower(BASES[s]));
    ch.meta = inpam ? gm_make(t + 1u, mm, dna, rna, state, curr, slen + 1u, pamid, 1u, 0u)
                    : gm_make(t + 1u, mm + (exact ? 0u : 1u), dna, rna, 0u, curr, slen + 1u, 0u, 0u, 0u);
    term = inpam && t + 1u == L + src.plen(pamid);
  } else { /* the pattern's N against a literal N of the genome */
    live = inpam && qc == 'N' && here;
    gseq_append(ch.seq, slen, 'N');
    ch.meta = gm_make(t + 1u, mm, dna, rna, state, curr, slen + 1u, pamid, 1u, 0u);
    term = t + 1u == L + src.plen(pamid);
  }
  /* ---- where the consumed symbol leads */
  if (kind == GB_VIRTUAL) {
    const uint32_t gcons = slen - rna; /* genome symbols consumed: every sequence byte but the RNA bulges' dots */
    live = live && s < 4u && gcons < c.k;
    ch.a = n.a | ((s & 3u) << (2u * ((c.k - 1u - gcons) & 15u)));
    if (gcons + 1u == c.k) ch.w = n.w | GB_SEED;
  } else if (kind == GB_INTERVAL) {
    ch.a = e.lo[s];
    ch.b = e.hi[s];
  } else {
    /* (beyond the sixteenth symbol nothing is known: "before the text start" moves in and matches nothing) */
    const uint64_t v = ((((uint64_t)(n.w & 0xFFFFu) << 32) | n.b) >> 3) | (6ull << 45);
    ch.b = (uint32_t)v;
    ch.w = (n.w & ~0xFFFFu) | (uint32_t)(v >> 32);
  }
}

#endif
