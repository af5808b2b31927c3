/*
 * gs_bulge.hip -- the seeded form of the bulge-aware search (index.hpp:250-375): k_search_general's machine - one wave
 * per (guide, strand), an LDS stack of 48-byte nodes, one node per lane per step, children placed by ballot - with the
 * children of a node taken from the structures the fast path lives on instead of two Occ-block reads per node from the
 * root down:
 *
 *   - until k = pt_k genome symbols are consumed a node is VIRTUAL: it carries their codes, reads nothing, and all
 *     four bases are present.  The child that consumes the k-th symbol is a SEED: one lookup in the strand's
 *     depth-k interval table (gs_strand_dev::ptab); an absent k-mer ends the path there;
 *   - a seed of at most GS_BULGE_ROWS rows becomes ROW nodes, one per row, each with its 16-symbol left context
 *     (ctx[], or the exception row's nibbles): the next genome symbol is known, so a row node reads nothing either.
 *     The rows are pushed as a chain (row sp, then sp+1..ep), the way the hop nodes chain;
 *   - a larger seed is an INTERVAL node, walked with occ4 exactly as k_search_general walks.
 *
 * The transitions are gb_child (gs_bulge_step.h), shared with the host-only debug entry points at the end of this file.
 * Records are the walk's gs_grec, appended to the same pool; a row node's match has sp == ep == the seed's row and says in
 * its meta word how many context symbols it consumed (k_gen_locate steps back that far).  Eligibility and routing:
 * enumerate_general (gs_general.hip).
 */
#include "gs_device.h"
#include "gs_bulge_step.h"

#include <algorithm>
#include <cstring>
#include <vector>

struct gb_dev_src {
  const gs_gsearch_args &a;
  const gs_gen_guide *gg;
  __device__ __forceinline__ uint32_t q(uint32_t t) const { return gg->q[t & 31u]; }
  __device__ __forceinline__ uint32_t own_pam(uint32_t u) const { return gg->pam[u & 7u]; }
  __device__ __forceinline__ uint32_t alt(uint32_t j, uint32_t u) const { return a.alt[j & 31u][u & 7u]; }
  __device__ __forceinline__ uint32_t plen(uint32_t j) const { return a.plen[j < 40u ? j : 39u]; }
};

__global__ __launch_bounds__(WAVE) void k_search_bulge(gs_bsearch_args b) {
  __shared__ uint4 s_stack[GSTACK * 3];
  const gs_gsearch_args &a = b.g;
  const uint32_t lane = lane_id();
  uint4 *stk = s_stack;
  gb_cfg cfg;
  cfg.L = a.L;
  cfg.P = a.P;
  cfg.m = a.m;
  cfg.n_alt = a.n_alt;
  cfg.max_rna = a.max_rna;
  cfg.max_dna = a.max_dna;
  cfg.k = b.k;
  const uint32_t npams = a.P ? a.n_alt + 1u : 1u;
  /* the walk's room rule; one level more for the chain a row's children sit on */
  const uint32_t reserve = (GFAN - 1) * (a.L + a.p_max + a.max_dna + npams + 5u);
  const uint32_t limit_own = GSTACK > reserve ? GSTACK - reserve : 1u;
  const uint32_t limit = limit_own < a.stack_cap ? limit_own : a.stack_cap;
  const uint32_t n_list = a.n_items >> 1;
  for (;;) {
    uint32_t item = 0;
    if (lane == 0) item = atomicAdd(b.bwork, 1u);
    item = __builtin_amdgcn_readfirstlane(item);
    if (item >= a.n_items) break;
    const uint32_t strand = item >= n_list ? 1u : 0u;
    const uint32_t li = item - strand * n_list;
    const uint32_t guide = a.glist ? a.glist[li] : li;
    const uint32_t slot = 2u * guide + strand;
    const gb_dev_src src{a, a.guides + guide};
    const gs_strand_dev &sd = a.sd[strand];
    const uint4 *__restrict__ blocks = sd.blocks;
    const uint4 *__restrict__ ptab = sd.ptab;
    uint32_t n_match = 0, size = 1;
    /* the root: a virtual node with nothing consumed (the same values from every lane) */
    stk[0] = make_uint4(0u, 0u, 0u, GB_W(GB_VIRTUAL));
    stk[1] = make_uint4(0u, 0u, 0u, 0u);
    stk[2] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    bool ovf = false; /* a push beyond the stack (the room rule keeps it from happening): not written, reported */

    auto route = [&](bool live, bool term, const gb_node &c) __attribute__((always_inline)) {
      const bool pu = live && !term, em = live && term;
      const uint64_t bp = __ballot(pu);
      if (bp) {
        if (pu) {
          const uint32_t at = size + lanes_below(bp);
          if (at < GSTACK) {
            stk[3u * at] = make_uint4(c.a, c.b, c.meta, c.w);
            stk[3u * at + 1u] = make_uint4(c.seq[0], c.seq[1], c.seq[2], c.seq[3]);
            stk[3u * at + 2u] = make_uint4(c.seq[4], c.seq[5], c.seq[6], c.seq[7]);
          } else {
            ovf = true;
          }
        }
        size += __popcll(bp);
      }
      const uint64_t be = __ballot(em);
      if (be) {
        unsigned long long pbase = 0; /* one atomic per emission of the wave */
        if (lane == (uint32_t)__builtin_ctzll(be)) pbase = atomicAdd(a.pool_next, (unsigned long long)__popcll(be));
        pbase = ((unsigned long long)__shfl((int)(pbase >> 32), (int)__builtin_ctzll(be)) << 32) |
                (uint32_t)__shfl((int)(uint32_t)pbase, (int)__builtin_ctzll(be));
        if (em) {
          const unsigned long long idx = pbase + lanes_below(be);
          if (idx < a.pool_cap) {
            const bool row = GB_KIND(c.w) == GB_ROW;
            gs_grec r;
            for (int i = 0; i < 8; i++) r.seq[i] = c.seq[i];
            r.sp = c.a;
            r.ep = row ? c.a : c.b;
            r.meta = GM_MM(c.meta) | (GM_DNA(c.meta) << 3) | (GM_RNA(c.meta) << 6) | (strand << 9) |
                     (GM_SLEN(c.meta) << 10);
            if (row) r.meta |= (((GM_SLEN(c.meta) - GM_RNA(c.meta) - b.k) & 31u) << 16) | GREC_ROW;
            r.g = guide;
            a.recs[idx] = r;
          }
        }
        n_match += __popcll(be);
      }
    };

    /* every wave must drain: past the iteration bound the item gives up loudly (error flag) instead of spinning.  The
     * exit and the tail below are free of lane-conditional blocks (compiler pitfall). */
    uint32_t guard = 0;
    uint32_t tally = lane == 0u ? 1u : 0u; /* lane 0: the stack's high-water mark */
    uint32_t c_seeds = 0, c_empty = 0, c_rows = 0, c_iv = 0, c_exc = 0;
    bool bail = false;
    while (size > 0 && !bail) {
      bail = ++guard > a.max_iter;
      uint32_t w = size < WAVE ? size : WAVE;
      const uint32_t room = size < limit ? limit - size : 0u;
      const uint32_t fit = room / (GFAN - 1);
      if (w > fit) w = fit ? fit : 1u;
      const bool active = lane < w;
      uint4 n0 = make_uint4(0, 0, 0, 0), n1 = n0, n2 = n0;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (active) {
        n0 = stk[3u * (size - 1u - lane)];
        n1 = stk[3u * (size - 1u - lane) + 1u];
        n2 = stk[3u * (size - 1u - lane) + 2u];
      }
      size -= w;
      gb_node n;
      n.a = n0.x;
      n.b = n0.y;
      n.meta = n0.z;
      n.w = n0.w;
      n.seq[0] = n1.x, n.seq[1] = n1.y, n.seq[2] = n1.z, n.seq[3] = n1.w;
      n.seq[4] = n2.x, n.seq[5] = n2.y, n.seq[6] = n2.z, n.seq[7] = n2.w;
      /* ---- a chain node becomes the row node of its first row, and the chain of the rest goes back on the stack */
      {
        const bool chain = active && GB_KIND(n.w) == GB_CHAIN;
        gb_node rest = n;
        rest.a = n.a + 1u;
        const bool more = chain && n.a < n.b;
        if (chain) {
          const uint32_t row = n.a;
          uint64_t c48 = gb_ctx_from_word(sd.ctx[row]);
          if (n.w & GB_EXC) { /* the true symbols of a row whose context holds an N, another symbol or the text start */
            uint32_t el = 0, eh = sd.n_exc;
            while (el < eh) {
              const uint32_t mid = (el + eh) >> 1;
              if (sd.exc_row[mid] < row)
                el = mid + 1;
              else
                eh = mid;
            }
            if (el < sd.n_exc && sd.exc_row[el] == row) c48 = gb_ctx_from_nibbles(sd.exc_sym[el]);
            c_exc++;
          }
          gb_make_row(n, row, c48);
          c_rows++;
        }
        route(more, false, rest);
      }
      /* ---- an interval node reads its two Occ blocks, as the walk does */
      gb_env env;
      env.present = 0u;
      for (int c = 0; c < 5; c++) env.lo[c] = env.hi[c] = 0u;
      if (active && GB_KIND(n.w) == GB_INTERVAL && !GM_HOP(n.meta)) {
        uint32_t oa[4], ob[4];
        occ4(blocks, n.a >> GS_BLOCK_SHIFT, n.a & (GS_BLOCK_ROWS - 1u), oa[0], oa[1], oa[2], oa[3]);
        occ4(blocks, n.b >> GS_BLOCK_SHIFT, (n.b & (GS_BLOCK_ROWS - 1u)) + 1u, ob[0], ob[1], ob[2], ob[3]);
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
          env.lo[c] = sd.C[c] + oa[c];
          env.hi[c] = sd.C[c] + ob[c] - 1u;
          env.present |= ob[c] > oa[c] ? 1u << c : 0u;
        }
        if (gb_wants_n(cfg, src, n.meta)) {
          const uint32_t na = occ_sym(sd, 'N', n.a), nb = occ_sym(sd, 'N', n.b + 1u);
          env.lo[4] = sd.C256['N'] + na;
          env.hi[4] = sd.C256['N'] + nb - 1u;
          env.present |= nb > na ? 16u : 0u;
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < GB_CHILDREN; ++i) {
        gb_node ch;
        bool live, term;
        gb_child(cfg, src, n, env, i, ch, live, term);
        live = live && active;
        if (live && (ch.w & GB_SEED)) { /* the k-th genome symbol: one table lookup says what the path has become */
          const uint4 e = ptab[ch.a];
          const uint32_t cnt = e.y & 0x7FFFFFFFu;
          c_seeds++;
          live = cnt != 0u;
          c_empty += cnt == 0u ? 1u : 0u;
          const bool rows = cnt <= b.rows;
          c_iv += cnt != 0u && !rows ? 1u : 0u;
          ch.a = e.x;
          ch.b = e.x + cnt - 1u;
          ch.w = rows ? GB_W(GB_CHAIN) | ((e.y >> 31) ? GB_EXC : 0u) : GB_W(GB_INTERVAL);
        }
        route(live, term, ch);
      }
      tally = lane == 0u && size > tally ? size : tally;
      bail = bail || __ballot(ovf) != 0ull;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    a.counts[slot] = n_match; /* same address, same value from every lane */
    const uint32_t err = (guard > a.max_iter ? 1u : 0u) | (__ballot(ovf) != 0ull ? 2u : 0u);
    if (err) atomicOr(&b.bwork[1], err);
    /* the item's counters: every lane adds what it counted (most add 0) - no `if (lane == ...)` blocks, which this tail
     * must stay free of.  (A wave sum by DPP under `lane == 63 ? sum : 0` was tried first: the compiler moved the DPP
     * steps behind the select, where only lane 63 runs them, and every counter read 0.) */
    unsigned long long *c64 = (unsigned long long *)(b.bwork + 16); /* 64 bits: one batch at hg38 size makes 3.7e9 row nodes */
    atomicAdd(&c64[0], (unsigned long long)c_seeds);
    atomicAdd(&c64[1], (unsigned long long)c_empty);
    atomicAdd(&c64[2], (unsigned long long)c_rows);
    atomicAdd(&c64[3], (unsigned long long)c_iv);
    atomicAdd(&c64[4], (unsigned long long)c_exc);
    atomicMax(&b.bwork[7], lane == 0u ? tally : 0u);
  }
}

gs_status gs_bulge_launch(const gs_bsearch_args &a, uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(k_search_bulge, dim3(grid), dim3(WAVE), 0, st, a);
  GS_HIP(hipGetLastError());
  return GS_OK;
}

/* ---- host only: the same transitions, from the same function ---------------------------------------------------- */

static uint8_t bulge_comp(uint8_t c) { /* genomics::complement (src/genomics/sequences.cxx:14-26) */
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    default: return c;
  }
}
struct gb_host_src {
  uint8_t qs[32], own[8], alts[32][8], pl[40];
  uint32_t q(uint32_t t) const { return qs[t & 31u]; }
  uint32_t own_pam(uint32_t u) const { return own[u & 7u]; }
  uint32_t alt(uint32_t j, uint32_t u) const { return alts[j & 31u][u & 7u]; }
  uint32_t plen(uint32_t j) const { return pl[j < 40u ? j : 39u]; }
};
static void host_seq_bytes(const gb_node &n, uint8_t out[32]) {
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)((n.seq[i >> 2] >> (8 * (3 - (i & 3)))) & 255u);
}
static bool host_guide(gb_host_src &s, const char *guide, uint32_t L, bool start) {
  memset(&s, 0, sizeof(s));
  for (uint32_t t = 0; t < L; t++) {
    const uint8_t c = (uint8_t)guide[start ? L - 1 - t : t];
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return false;
    s.qs[t] = start ? c : bulge_comp(c);
  }
  return true;
}

extern "C" gs_status gs_debug_bulge_seeds(const char *guide, uint32_t L, uint32_t k, uint32_t mismatches, uint32_t rna_bulges,
                                          uint32_t dna_bulges, uint32_t flags, uint32_t prefix_len, uint32_t prefix,
                                          gs_bulge_seed *out, uint64_t cap, uint64_t *n) {
  if (!guide || !n || (cap && !out) || L < 1 || L > 31 || k < 1 || k > 16 || mismatches > 7 || rna_bulges > 3 ||
      dna_bulges > 3 || L < rna_bulges + k || prefix_len > k || (prefix_len < 16 && (prefix >> (2 * prefix_len)) != 0))
    return GS_ERR_ARG;
  gb_host_src src;
  if (!host_guide(src, guide, L, (flags & GS_FLAG_PAM_AT_START) != 0)) return GS_ERR_ARG;
  const gb_cfg cfg{L, 0u, mismatches, 0u, rna_bulges, dna_bulges, k};
  gb_env env;
  memset(&env, 0, sizeof(env));
  std::vector<gb_node> stack;
  gb_node root;
  memset(&root, 0, sizeof(root));
  root.w = GB_W(GB_VIRTUAL);
  stack.push_back(root);
  uint64_t cnt = 0;
  while (!stack.empty()) {
    const gb_node nd = stack.back();
    stack.pop_back();
    for (uint32_t i = 0; i < GB_CHILDREN; i++) {
      gb_node ch;
      bool live, term;
      gb_child(cfg, src, nd, env, i, ch, live, term);
      if (!live) continue;
      /* the sub-tree asked for: paths whose first prefix_len genome symbols are `prefix` (the top bits of the index) */
      if (prefix_len) {
        const uint32_t have = std::min(GM_SLEN(ch.meta) - GM_RNA(ch.meta), prefix_len); /* symbols of the prefix the child has consumed */
        if (have && (ch.a >> (2u * (k - have))) != (prefix >> (2u * (prefix_len - have)))) continue;
      }
      if (ch.w & GB_SEED) {
        if (cnt < cap) {
          out[cnt].index = ch.a;
          out[cnt].state = ch.meta;
          host_seq_bytes(ch, out[cnt].seq);
        }
        cnt++;
      } else if (!term) {
        stack.push_back(ch);
      }
    }
  }
  *n = cnt;
  return GS_OK;
}

extern "C" gs_status gs_debug_bulge_verify(uint32_t state, const uint8_t seq[32], uint64_t ctx_nibbles, const char *guide,
                                           uint32_t L, const char *guide_pam, uint32_t P, const char *alt_pams,
                                           const uint32_t *alt_lens, uint32_t n_alt, uint32_t k, uint32_t mismatches,
                                           uint32_t rna_bulges, uint32_t dna_bulges, uint32_t flags, gs_bulge_match *out,
                                           uint64_t cap, uint64_t *n) {
  if (!guide || !seq || !n || (cap && !out) || (P && !guide_pam) || (n_alt && (!alt_pams || !alt_lens)) || L < 1 || L > 31 ||
      P > 8 || n_alt > 31 || k < 1 || k > 16 || mismatches > 7 || rna_bulges > 3 || dna_bulges > 3)
    return GS_ERR_ARG;
  const bool start = (flags & GS_FLAG_PAM_AT_START) != 0;
  gb_host_src src;
  if (!host_guide(src, guide, L, start)) return GS_ERR_ARG;
  for (uint32_t u = 0; u < P; u++) src.own[u] = start ? (uint8_t)guide_pam[P - 1 - u] : bulge_comp((uint8_t)guide_pam[u]);
  const uint32_t na = P ? n_alt : 0u; /* an empty guide PAM drops the alt PAMs (process.hpp:52-53) */
  size_t at = 0;
  for (uint32_t j = 0; j < na; j++) {
    const uint32_t pl = alt_lens[j];
    if (pl < 1 || pl > 8) return GS_ERR_ARG;
    for (uint32_t u = 0; u < pl; u++) src.alts[j][u] = start ? (uint8_t)alt_pams[at + pl - 1 - u] : bulge_comp((uint8_t)alt_pams[at + u]);
    src.pl[j] = (uint8_t)pl;
    at += pl;
  }
  src.pl[na] = (uint8_t)P;
  const gb_cfg cfg{L, P, mismatches, na, rna_bulges, dna_bulges, k};
  gb_env env;
  memset(&env, 0, sizeof(env));
  gb_node root;
  memset(&root, 0, sizeof(root));
  root.meta = state;
  for (uint32_t i = 0; i < 32; i++) root.seq[i >> 2] |= (uint32_t)seq[i] << (8u * (3u - (i & 3u)));
  gb_make_row(root, 0u, gb_ctx_from_nibbles(ctx_nibbles));
  std::vector<gb_node> stack{root};
  uint64_t cnt = 0;
  while (!stack.empty()) {
    const gb_node nd = stack.back();
    stack.pop_back();
    for (uint32_t i = 0; i < GB_CHILDREN; i++) {
      gb_node ch;
      bool live, term;
      gb_child(cfg, src, nd, env, i, ch, live, term);
      if (!live) continue;
      if (term) {
        if (cnt < cap) {
          out[cnt].state = ch.meta;
          out[cnt].consumed = GM_SLEN(ch.meta) - GM_RNA(ch.meta) - k;
          host_seq_bytes(ch, out[cnt].seq);
        }
        cnt++;
      } else {
        stack.push_back(ch);
      }
    }
  }
  *n = cnt;
  return GS_OK;
}
