/*
 * gs_sdsl_export.hip -- exporter for the reference's on-disk index: writes
 * <prefix>.forward / <prefix>.reverse exactly as sdsl::csa_wt<wt_huff<>,64,8192>::serialize would for the strand's text
 * (sdsl/include/sdsl/csa_wt.hpp:372-382), from the handle's full suffix arrays.  The counterpart of gs_sdsl_import.hip.
 *
 * What runs where, per strand:
 *   device  BWT bytes text[SA[r]-1] and their 256 counts; per inner node of the Huffman-shaped tree one membership test, one
 *           exclusive scan and one scatter of the node's bits (a byte each) to their place in the concatenated bit vector;
 *           one ballot per 64 bits packs them into m_bv's words; popcounts + scan give the rank_support_v blocks and the
 *           position of every 64th set / unset bit (what select_support_mcl is made of); SA[0], SA[64], ... and the scatter
 *           of the rows whose SA value is a multiple of 8192.
 *   host    the tree and the alphabet (functions of the 256 counts), the select supports' variable-width packing, the
 *           packing of the samples, the file.
 * The format is restated here from the reference's headers (file:line at each part); no SDSL code is part of the product.
 */
#include "gs_common.h"
#include "gs_scratch.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <queue>

#include <unistd.h>

__global__ void k_revcomp(const uint8_t *in, uint8_t *out, uint64_t len); /* gs_index.hip */

namespace {

/* bits::hi (sdsl/include/sdsl/bits.hpp): position of the most significant set bit, 0 for 0 */
uint32_t hi(uint64_t x) { return x ? 63u - (uint32_t)__builtin_clzll(x) : 0u; }

void put_bytes(std::vector<uint8_t> &o, const void *p, size_t n) {
  const uint8_t *q = (const uint8_t *)p;
  o.insert(o.end(), q, q + n);
}
template <class T>
void put(std::vector<uint8_t> &o, T v) {
  put_bytes(o, &v, sizeof(T));
}

/* ---- the tree: a function of the 256 counts ------------------------------------------------------------------------- */
struct exp_node { /* wt_helper.hpp:73-127; size = symbols the node holds (not stored in the file) */
  uint64_t bv_pos = 0, bv_pos_rank = 0;
  uint16_t parent = 0xFFFF, child[2] = {0xFFFF, 0xFFFF};
  uint64_t size = 0;
};
struct exp_tree {
  std::vector<exp_node> nodes;
  uint16_t c_to_leaf[256];
  uint64_t path[256];
  uint64_t bv_size = 0, sigma = 0, n = 0;
};

bool build_tree(const uint64_t counts[256], exp_tree &T) {
  /* the shape: wt_huff.hpp:84-117 - leaves in symbol order, then the two smallest (frequency, node number) pairs joined,
   * the smaller one as child 0, until one node is left */
  struct tmp_node {
    uint64_t freq, sym, parent, child[2];
  };
  const uint64_t undef = ~0ull;
  std::vector<tmp_node> tmp;
  typedef std::pair<uint64_t, uint64_t> pii;
  std::priority_queue<pii, std::vector<pii>, std::greater<pii>> pq;
  T.n = 0;
  for (uint64_t c = 0; c < 256; c++)
    if (counts[c]) {
      pq.push(pii(counts[c], tmp.size()));
      tmp.push_back({counts[c], c, undef, {undef, undef}});
      T.n += counts[c];
    }
  T.sigma = tmp.size();
  if (tmp.empty()) return false;
  while (pq.size() > 1) {
    const pii v1 = pq.top();
    pq.pop();
    const pii v2 = pq.top();
    pq.pop();
    tmp[v1.second].parent = tmp[v2.second].parent = tmp.size();
    pq.push(pii(v1.first + v2.first, tmp.size()));
    tmp.push_back({v1.first + v2.first, 0, undef, {v1.second, v2.second}});
  }
  /* breadth-first renumbering with the root at 0; bv_pos = bits of the inner nodes before (wt_helper.hpp:164-199) */
  auto conv = [&](const tmp_node &t) {
    exp_node e;
    e.size = t.freq;
    e.bv_pos_rank = t.sym;
    e.parent = (uint16_t)t.parent;
    e.child[0] = (uint16_t)t.child[0]; /* (indices into tmp until the node is visited) */
    e.child[1] = (uint16_t)t.child[1];
    return e;
  };
  T.nodes.assign(tmp.size(), exp_node());
  T.nodes[0] = conv(tmp.back());
  T.bv_size = 0;
  size_t node_cnt = 1;
  std::deque<uint16_t> q;
  q.push_back(0);
  while (!q.empty()) {
    const uint16_t idx = q.front();
    q.pop_front();
    exp_node &nd = T.nodes[idx];
    nd.bv_pos = T.bv_size;
    if (nd.child[0] != 0xFFFF) {
      T.bv_size += nd.size;
      for (int k = 0; k < 2; k++) {
        T.nodes[node_cnt] = conv(tmp[nd.child[k]]);
        T.nodes[node_cnt].parent = idx;
        q.push_back((uint16_t)node_cnt);
        nd.child[k] = (uint16_t)node_cnt++;
      }
    }
  }
  /* inner nodes: ones of m_bv before the node's bits (init_node_ranks, wt_helper.hpp:237-242) = the sizes of the
   * right children of the inner nodes before it */
  uint64_t ones = 0;
  for (exp_node &nd : T.nodes)
    if (nd.child[0] != 0xFFFF) {
      nd.bv_pos_rank = ones;
      ones += T.nodes[nd.child[1]].size;
    }
  /* c_to_leaf and path (wt_helper.hpp:200-233): bits 0..55 the code, root's decision lowest, bits 56..63 its length; a
   * symbol that is absent holds the last present symbol below it with length 0 */
  for (int c = 0; c < 256; c++) T.c_to_leaf[c] = 0xFFFF;
  for (size_t v = 0; v < T.nodes.size(); v++)
    if (T.nodes[v].child[0] == 0xFFFF) T.c_to_leaf[(uint8_t)T.nodes[v].bv_pos_rank] = (uint16_t)v;
  uint64_t prev_c = 0;
  for (uint64_t c = 0; c < 256; c++) {
    if (T.c_to_leaf[c] == 0xFFFF) {
      T.path[c] = prev_c;
      continue;
    }
    uint16_t v = T.c_to_leaf[c];
    uint64_t pw = 0, pl = 0;
    while (v != 0) {
      pw <<= 1;
      if (T.nodes[T.nodes[v].parent].child[1] == v) pw |= 1ull;
      ++pl;
      v = T.nodes[v].parent;
    }
    if (pl > 56) return false;
    T.path[c] = pw | (pl << 56);
    prev_c = c;
  }
  return true;
}
/* _byte_tree::serialize, wt_helper.hpp:264-278 */
void serialize_tree(const exp_tree &T, std::vector<uint8_t> &o) {
  put<uint64_t>(o, T.nodes.size());
  for (const exp_node &nd : T.nodes) {
    put<uint64_t>(o, nd.bv_pos);
    put<uint64_t>(o, nd.bv_pos_rank);
    put<uint16_t>(o, nd.parent);
    put<uint16_t>(o, nd.child[0]);
    put<uint16_t>(o, nd.child[1]);
  }
  put_bytes(o, T.c_to_leaf, sizeof(T.c_to_leaf));
  put_bytes(o, T.path, sizeof(T.path));
}
/* byte_alphabet (sdsl/lib/csa_alphabet_strategy.cpp:25-55, 103-113): int_vector<8> char2comp[256], int_vector<8>
 * comp2char[sigma], int_vector<64> C[sigma + 1], u16 sigma */
void serialize_alphabet(const uint64_t counts[256], std::vector<uint8_t> &o) {
  uint8_t char2comp[256] = {0};
  uint8_t comp2char[256 + 8] = {0};
  uint64_t C[257] = {0};
  uint16_t sigma = 0;
  for (int c = 0; c < 256; c++)
    if (counts[c]) {
      char2comp[c] = (uint8_t)sigma;
      comp2char[sigma] = (uint8_t)c;
      C[sigma + 1] = C[sigma] + counts[c];
      ++sigma;
    }
  put<uint64_t>(o, 256 * 8);
  put_bytes(o, char2comp, 256);
  put<uint64_t>(o, (uint64_t)sigma * 8);
  put_bytes(o, comp2char, (((size_t)sigma * 8 + 63) >> 6) * 8);
  put<uint64_t>(o, ((uint64_t)sigma + 1) * 64);
  put_bytes(o, C, ((size_t)sigma + 1) * 8);
  put<uint16_t>(o, sigma);
}

/* ---- int_vector<0>: u64 size in bits, u8 width, ceil(bits / 64) words, entries packed from bit 0 up
 * (int_vector.hpp:416-419, 1545-1560) */
struct ivec0 {
  uint64_t bits = 0;
  uint8_t width = 64;
  std::vector<uint64_t> words;
  ivec0() {}
  ivec0(uint64_t count, uint32_t w) : bits(count * w), width((uint8_t)w), words((count * w + 63) >> 6, 0) {}
  void set(uint64_t i, uint64_t v) { /* (into zeroed words, each entry once) */
    const uint64_t b = i * width, w = b >> 6, o = b & 63;
    words[w] |= v << o;
    if (o + width > 64) words[w + 1] |= v >> (64 - o);
  }
};
struct file_writer {
  FILE *f = nullptr;
  bool ok = true;
  void bytes(const void *p, size_t n) {
    if (ok && n && fwrite(p, 1, n, f) != n) ok = false;
  }
  void u64(uint64_t v) { bytes(&v, 8); }
  void vec(const ivec0 &v) {
    u64(v.bits);
    bytes(&v.width, 1);
    bytes(v.words.data(), 8 * v.words.size());
  }
};

/* ---- select_support_mcl<b> (select_support_mcl.hpp:108-116, 209-343, 425-462) ---------------------------------------
 * Arguments (set bits for b = 1, unset ones for b = 0) in superblocks of 4096; per superblock either every 64th position
 * relative to the first (a miniblock of 64 entries) or, when the superblock spans more than logn4 bits, every position.
 * One restatement of init_slow (vectors under 100,000 bits) and init_fast (the rest).  They differ in what they count:
 * init_fast walks whole words, so for b = 0 the unset padding bits between size and capacity count as arguments where it
 * takes every 64th, and its forward scans (found_arg) see only bits below size; it decides a superblock's span by the
 * first argument of the NEXT superblock (the scan at :297-301 takes 64 steps from the 4033rd argument), stores a last,
 * incomplete superblock always as a long one without setting its superblock entry, and creates the long array - hence
 * a non-empty mini_or_long - even when that incomplete block lies beyond the last superblock that is serialised.
 * S = the position of every 64th argument counted over the capacity (the device made it), n_s of them. */
struct bit_src {
  const uint64_t *w;
  uint64_t W, size; /* words, bits */
  int b;
  uint64_t word(uint64_t i) const { return b ? w[i] : ~w[i]; }
};
/* positions of the arguments in [from, to], at most max of them, over the raw words */
void collect(const bit_src &B, uint64_t from, uint64_t to, uint64_t max, std::vector<uint64_t> &out) {
  out.clear();
  if (from > to || max == 0) return;
  for (uint64_t wi = from >> 6; wi <= (to >> 6) && wi < B.W; wi++) {
    uint64_t x = B.word(wi);
    if (wi == (from >> 6)) x &= ~0ull << (from & 63);
    if (wi == (to >> 6) && (to & 63) != 63) x &= (1ull << ((to & 63) + 1)) - 1ull;
    while (x) {
      out.push_back((wi << 6) + (uint64_t)__builtin_ctzll(x));
      if (out.size() == max) return;
      x &= x - 1;
    }
  }
}
/* the last argument in [from, to]; false: none */
bool find_last(const bit_src &B, uint64_t from, uint64_t to, uint64_t &pos) {
  if (from > to) return false;
  for (uint64_t wi = to >> 6;; wi--) {
    uint64_t x = B.word(wi);
    if (wi == (from >> 6)) x &= ~0ull << (from & 63);
    if (wi == (to >> 6) && (to & 63) != 63) x &= (1ull << ((to & 63) + 1)) - 1ull;
    if (x) {
      pos = (wi << 6) + 63u - (uint64_t)__builtin_clzll(x);
      return true;
    }
    if (wi == (from >> 6)) return false;
  }
}
void write_select(file_writer &fw, const bit_src &B, const uint64_t *S, uint64_t n_s, uint64_t arg_cnt) {
  fw.u64(arg_cnt);
  if (!arg_cnt) return;
  const uint64_t logn = hi(B.W << 6) + 1, logn4 = logn * logn * logn * logn; /* initData, :402-411 */
  const uint64_t sb = (arg_cnt + 4095) >> 12;
  ivec0 superblock(sb, (uint32_t)logn);
  std::vector<ivec0> block(sb);
  std::vector<uint8_t> is_long(sb, 0);
  bool any_long = false;
  std::vector<uint64_t> P;
  auto make_long = [&](uint64_t k, uint32_t width) {
    block[k] = ivec0(4096, width);
    for (size_t j = 0; j < P.size(); j++) block[k].set(j, P[j]);
    is_long[k] = 1;
    any_long = true;
  };
  auto make_mini = [&](uint64_t k, uint64_t diff, uint64_t samples) {
    block[k] = ivec0(64, hi(diff) + 1);
    for (uint64_t j = 0; j < samples; j++) block[k].set(j, S[64 * k + j] - S[64 * k]);
  };
  if (B.size < 100000) { /* init_slow: every argument below size, superblock by superblock */
    for (uint64_t k = 0; k < sb; k++) {
      const uint64_t cnt = std::min<uint64_t>(4096, arg_cnt - 4096 * k), first = S[64 * k];
      collect(B, first, B.size - 1, cnt, P);
      const uint64_t last = P.back();
      superblock.set(k, first);
      if (last - first > logn4)
        make_long(k, hi(last) + 1);
      else
        make_mini(k, last - first, (cnt + 63) / 64);
    }
  } else { /* init_fast */
    const uint64_t full = n_s / 64;
    for (uint64_t k = 0; k < full && k < sb; k++) {
      const uint64_t first = S[64 * k];
      uint64_t last = S[64 * k + 63];
      if (64 * (k + 1) < n_s && S[64 * (k + 1)] < B.size)
        last = S[64 * (k + 1)];
      else
        (void)find_last(B, last + 1, B.size - 1, last);
      superblock.set(k, first);
      if (last - first > logn4) {
        collect(B, first, last, 4096, P);
        make_long(k, hi(last) + 1);
      } else {
        make_mini(k, last - first, 64);
      }
    }
    if (n_s % 64) { /* "handle last block: append long superblock" :332-342 */
      any_long = true;
      if (full < sb) {
        collect(B, S[64 * full], B.size - 1, 4096, P);
        make_long(full, hi(B.size - 1) + 1);
      }
    }
  }
  /* serialize, :425-462 */
  fw.vec(superblock);
  if (any_long) {
    std::vector<uint64_t> mol((sb + 63) >> 6, 0);
    for (uint64_t k = 0; k < sb; k++)
      if (!is_long[k]) mol[k >> 6] |= 1ull << (k & 63);
    fw.u64(sb);
    fw.bytes(mol.data(), 8 * mol.size());
  } else {
    fw.u64(0);
  }
  for (uint64_t k = 0; k < sb; k++) fw.vec(block[k]);
}

}  // namespace

/* ---- device side ----------------------------------------------------------------------------------------------------- */
#define EXP_GRID 8192u /* blocks of 256 of the grid-stride kernels */
struct exp_code {
  uint8_t of[256]; /* per symbol: 0 / 1 = the node's bit for it, 0xFF = not under the node */
};
/* BWT symbols text[SA[r] - 1] (the sentinel row reads the sentinel: text has n bytes, the last is 0) and their counts */
__global__ __launch_bounds__(256) void k_exp_bwt(const uint8_t *text, const uint32_t *sa, uint64_t n, uint8_t *bwt, unsigned long long *hist) {
  __shared__ uint32_t s_h[256];
  s_h[threadIdx.x] = 0u;
  __syncthreads();
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = sa[r];
    const uint8_t c = text[p ? (uint64_t)p - 1u : n - 1u];
    bwt[r] = c;
    atomicAdd(&s_h[c], 1u);
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_h[threadIdx.x]);
}
/* rows of the node per chunk of 64 rows: one wave, one ballot per chunk */
__global__ __launch_bounds__(256) void k_exp_count(const uint8_t *bwt, uint64_t n, exp_code K, uint64_t nb, uint32_t *cnt) {
  __shared__ uint8_t s_of[256];
  s_of[threadIdx.x] = K.of[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t c = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nb; c += waves) {
    const uint64_t r = c * 64u + lane;
    const bool m = r < n && s_of[bwt[r]] != 0xFFu;
    const unsigned long long mask = __ballot(m);
    if (lane == 0u) cnt[c] = (uint32_t)__popcll(mask);
  }
}
/* the node's bits, a byte each, in row order at bits[first of the chunk + members among the lower lanes] */
__global__ __launch_bounds__(256) void k_exp_scatter(const uint8_t *bwt, uint64_t n, exp_code K, uint64_t nb, const uint32_t *excl, uint8_t *bits,
                                                     uint64_t node_size) {
  __shared__ uint8_t s_of[256];
  s_of[threadIdx.x] = K.of[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t c = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nb; c += waves) {
    const uint64_t r = c * 64u + lane;
    const uint8_t b = r < n ? s_of[bwt[r]] : (uint8_t)0xFFu;
    const unsigned long long mask = __ballot(b != 0xFFu);
    if (b != 0xFFu) {
      const uint64_t at = (uint64_t)excl[c] + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (at < node_size) bits[at] = b; /* (always: the counts come from the same test) */
    }
  }
}
/* 64 bit bytes -> one word of m_bv by one ballot, and the word's popcount; words beyond the bits' end: zero padding */
__global__ __launch_bounds__(256) void k_exp_pack(const uint8_t *bits, uint64_t nbits, uint64_t W, uint64_t *words, uint64_t *pc) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < W; w += waves) {
    const uint64_t g = w * 64u + lane;
    const unsigned long long mask = __ballot(g < nbits && bits[g] != 0u);
    if (lane == 0u) {
      words[w] = mask;
      pc[w] = (uint64_t)__popcll(mask);
    }
  }
}
/* rank_support_v (rank_support_v.hpp:75-105): per 512 bits the ones before and, for k = 1..7, the ones of the block's
 * first k words in 9 bits at shift 63 - 9k - up to and including the word count itself in the last block (the tail
 * rules at :97-105: an entry one past the last word, or a block of its own when the words are a multiple of 8).
 * ob[w] = ones before word w, W + 1 entries. */
__global__ __launch_bounds__(256) void k_exp_rank(const uint64_t *ob, uint64_t W, uint64_t nblocks, uint64_t *basic) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t base = ob[8u * b];
  uint64_t second = 0;
  for (uint32_t k = 1; k < 8u; ++k)
    if (8u * b + k <= W) second |= (ob[8u * b + k] - base) << (63u - 9u * k);
  basic[2u * b] = base;
  basic[2u * b + 1u] = second;
}
/* position of every 64th set bit (pos1) and every 64th unset bit counted over whole words (pos0): a word holds at most
 * one of each kind, so every entry has one writer */
__device__ __forceinline__ uint32_t exp_sel(uint64_t x, uint32_t r) { /* position of the set bit of x with r set bits below it */
  for (uint32_t i = 0; i < r; ++i) x &= x - 1ull;
  return (uint32_t)__ffsll((unsigned long long)x) - 1u;
}
__global__ __launch_bounds__(256) void k_exp_every64(const uint64_t *words, const uint64_t *ob, uint64_t W, uint64_t *pos1, uint64_t n1, uint64_t *pos0,
                                                     uint64_t n0) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < W; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t x = words[w], o = ob[w], o2 = ob[w + 1u];
    uint64_t k = (o + 63u) & ~63ull;
    if (k < o2 && (k >> 6) < n1) pos1[k >> 6] = w * 64u + exp_sel(x, (uint32_t)(k - o));
    const uint64_t z = w * 64u - o, z2 = (w + 1u) * 64u - o2;
    k = (z + 63u) & ~63ull;
    if (k < z2 && (k >> 6) < n0) pos0[k >> 6] = w * 64u + exp_sel(~x, (uint32_t)(k - z));
  }
}
/* SA[0], SA[64], ... (csa_sampling_strategy.hpp:85-99) and ISA[0], ISA[8192], ... (:626-642) */
__global__ __launch_bounds__(256) void k_exp_samples(const uint32_t *sa, uint64_t n, uint32_t *sa_s, uint64_t ns, uint32_t *isa_s, uint64_t nis) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = sa[r];
    if ((r & 63u) == 0u && (r >> 6) < ns) sa_s[r >> 6] = v;
    if ((v & 8191u) == 0u && (uint64_t)(v >> 13) < nis) isa_s[v >> 13] = (uint32_t)r;
  }
}

namespace {
uint64_t g_scratch_now = 0, g_scratch_peak = 0; /* device scratch of the export in progress (under the handle's lock) */
struct dbuf {                                   /* a device allocation that frees itself */
  void *p = nullptr;
  size_t bytes = 0;
  ~dbuf() { drop(); }
  hipError_t get(size_t b) {
    const hipError_t e = hipMalloc(&p, b ? b : 16);
    if (e == hipSuccess) {
      bytes = b;
      g_scratch_now += b;
      g_scratch_peak = std::max(g_scratch_peak, g_scratch_now);
    } else {
      p = nullptr;
    }
    return e;
  }
  void drop() {
    if (p) {
      (void)hipFree(p);
      g_scratch_now -= bytes;
    }
    p = nullptr;
    bytes = 0;
  }
};
unsigned grid_for(uint64_t items, uint64_t per_block) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(EXP_GRID, (items + per_block - 1) / per_block)); }
}  // namespace

#define EXP_HIP(expr)                                                   \
  do {                                                                  \
    hipError_t e__ = (expr);                                            \
    if (e__ != hipSuccess) {                                            \
      (void)hipGetLastError();                                          \
      gs_set_error(std::string(#expr) + ": " + hipGetErrorString(e__)); \
      return e__ == hipErrorOutOfMemory ? GS_ERR_NOMEM : GS_ERR_DEVICE; \
    }                                                                   \
  } while (0)

/* what the device hands to the host for one strand's file */
struct exp_parts {
  uint64_t counts[256];
  exp_tree T;
  std::vector<uint64_t> words, basic, pos1, pos0;
  std::vector<uint32_t> sa_s, isa_s;
  uint64_t ones = 0;
};

static gs_status export_strand_device(gs_index *ix, int strand, const uint8_t *text, uint64_t len, exp_parts &X) {
  hipStream_t st = nullptr; /* the stream the handle's builders use */
  const uint64_t n = len + 1;
  const uint32_t *d_sa = ix->strand[strand].d.sa;
  if (!d_sa) {
    gs_set_error("the handle holds no suffix array");
    return GS_ERR_ARG;
  }
  dbuf d_bwt, d_hist;
  EXP_HIP(d_bwt.get(n));
  EXP_HIP(d_hist.get(256 * 8));
  EXP_HIP(hipMemsetAsync(d_hist.p, 0, 256 * 8, st));
  {
    /* the strand's text with its sentinel: forward as given; reverse = its reverse complement, made on the device as the
     * builder makes it (build_common, gs_index.hip) */
    dbuf d_text, d_in;
    EXP_HIP(d_text.get(n));
    if (strand == 0) {
      EXP_HIP(hipMemcpy(d_text.p, text, len, hipMemcpyHostToDevice));
    } else {
      EXP_HIP(d_in.get(len));
      EXP_HIP(hipMemcpy(d_in.p, text, len, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_revcomp, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_in.p, (uint8_t *)d_text.p, len);
      EXP_HIP(hipGetLastError());
    }
    EXP_HIP(hipMemsetAsync((uint8_t *)d_text.p + len, 0, 1, st));
    hipLaunchKernelGGL(k_exp_bwt, dim3(grid_for(n, 256)), dim3(256), 0, st, (const uint8_t *)d_text.p, d_sa, n, (uint8_t *)d_bwt.p,
                       (unsigned long long *)d_hist.p);
    EXP_HIP(hipGetLastError());
    unsigned long long hist[256];
    EXP_HIP(hipMemcpy(hist, d_hist.p, sizeof(hist), hipMemcpyDeviceToHost)); /* (synchronises: the texts are done with) */
    for (int c = 0; c < 256; c++) X.counts[c] = hist[c];
  }
  if (X.counts[0] != 1 || !build_tree(X.counts, X.T) || X.T.n != n || X.T.bv_size == 0) {
    gs_set_error("the strand's BWT does not hold one sentinel and n symbols (is the text the handle's?)");
    return GS_ERR_ARG;
  }
  const exp_tree &T = X.T;
  const uint64_t nbits = T.bv_size, W = (nbits + 63) >> 6, nb = (n + 63) >> 6;
  /* the concatenated node bit vectors (wt_pc.hpp:128-145, 201-253), a byte per bit first */
  dbuf d_words, d_pc;
  EXP_HIP(d_words.get(8 * W));
  EXP_HIP(d_pc.get(8 * (W + 1)));
  {
    dbuf d_bits, d_cnt, d_excl, d_tmp;
    EXP_HIP(d_bits.get(nbits));
    EXP_HIP(d_cnt.get(4 * nb));
    EXP_HIP(d_excl.get(4 * nb));
    auto scan = [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, (uint32_t *)d_cnt.p, (uint32_t *)d_excl.p, 0u, (size_t)nb, rocprim::plus<uint32_t>(), st);
    };
    size_t tb = 0;
    GS_TRY(gs_prim_need("export: scan of the chunk counts", scan, tb));
    EXP_HIP(d_tmp.get(tb + 16));
    for (size_t v = 0; v < T.nodes.size(); v++) {
      const exp_node &nd = T.nodes[v];
      if (nd.child[0] == 0xFFFF) continue;
      /* the symbols under the node and the child each goes to: bit `depth of v` of its path */
      exp_code K;
      memset(K.of, 0xFF, sizeof(K.of));
      for (int c = 0; c < 256; c++) {
        if (T.c_to_leaf[c] == 0xFFFF) continue;
        uint16_t u = 0;
        const uint64_t plen = T.path[c] >> 56;
        for (uint64_t d = 0; d < plen; d++) {
          const uint32_t bit = (uint32_t)((T.path[c] >> d) & 1u);
          if (u == v) {
            K.of[c] = (uint8_t)bit;
            break;
          }
          u = T.nodes[u].child[bit];
        }
      }
      if (nd.bv_pos + nd.size > nbits) return GS_ERR_ARG; /* (never: bv_pos are sums of node sizes) */
      hipLaunchKernelGGL(k_exp_count, dim3(grid_for(nb, 4)), dim3(256), 0, st, (const uint8_t *)d_bwt.p, n, K, nb, (uint32_t *)d_cnt.p);
      EXP_HIP(hipGetLastError());
      GS_TRY(gs_prim_run("export: scan of the chunk counts", d_tmp.p, d_tmp.bytes, tb, scan));
      hipLaunchKernelGGL(k_exp_scatter, dim3(grid_for(nb, 4)), dim3(256), 0, st, (const uint8_t *)d_bwt.p, n, K, nb, (const uint32_t *)d_excl.p,
                         (uint8_t *)d_bits.p + nd.bv_pos, nd.size);
      EXP_HIP(hipGetLastError());
    }
    d_bwt.drop(); /* (frees synchronise) */
    EXP_HIP(hipMemsetAsync((uint64_t *)d_pc.p + W, 0, 8, st));
    hipLaunchKernelGGL(k_exp_pack, dim3(grid_for(W, 4)), dim3(256), 0, st, (const uint8_t *)d_bits.p, nbits, W, (uint64_t *)d_words.p, (uint64_t *)d_pc.p);
    EXP_HIP(hipGetLastError());
    EXP_HIP(hipStreamSynchronize(st));
  }
  /* ones before every word, the rank blocks, every 64th set / unset bit */
  dbuf d_ob;
  EXP_HIP(d_ob.get(8 * (W + 1)));
  {
    dbuf d_tmp;
    auto scan = [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, (uint64_t *)d_pc.p, (uint64_t *)d_ob.p, (uint64_t)0, (size_t)(W + 1), rocprim::plus<uint64_t>(), st);
    };
    size_t tb = 0;
    GS_TRY(gs_prim_need("export: scan of the words' ones", scan, tb));
    EXP_HIP(d_tmp.get(tb + 16));
    GS_TRY(gs_prim_run("export: scan of the words' ones", d_tmp.p, d_tmp.bytes, tb, scan));
    EXP_HIP(hipMemcpy(&X.ones, (uint64_t *)d_ob.p + W, 8, hipMemcpyDeviceToHost));
  }
  d_pc.drop();
  const uint64_t nblocks = (W >> 3) + 1, n1 = (X.ones + 63) >> 6, n0 = (W * 64 - X.ones + 63) >> 6;
  const uint64_t ns = (n + 63) / 64, nis = (n - 1) / 8192 + 1;
  X.words.resize(W);
  X.basic.resize(2 * nblocks);
  X.pos1.resize(n1);
  X.pos0.resize(n0);
  X.sa_s.resize(ns);
  X.isa_s.assign(nis, 0);
  EXP_HIP(hipMemcpy(X.words.data(), d_words.p, 8 * W, hipMemcpyDeviceToHost));
  {
    dbuf d_basic;
    EXP_HIP(d_basic.get(16 * nblocks));
    hipLaunchKernelGGL(k_exp_rank, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, st, (const uint64_t *)d_ob.p, W, nblocks, (uint64_t *)d_basic.p);
    EXP_HIP(hipGetLastError());
    EXP_HIP(hipMemcpy(X.basic.data(), d_basic.p, 16 * nblocks, hipMemcpyDeviceToHost));
  }
  {
    dbuf d_pos1, d_pos0;
    EXP_HIP(d_pos1.get(8 * n1));
    EXP_HIP(d_pos0.get(8 * n0));
    hipLaunchKernelGGL(k_exp_every64, dim3(grid_for(W, 256)), dim3(256), 0, st, (const uint64_t *)d_words.p, (const uint64_t *)d_ob.p, W, (uint64_t *)d_pos1.p,
                       n1, (uint64_t *)d_pos0.p, n0);
    EXP_HIP(hipGetLastError());
    if (n1) EXP_HIP(hipMemcpy(X.pos1.data(), d_pos1.p, 8 * n1, hipMemcpyDeviceToHost));
    if (n0) EXP_HIP(hipMemcpy(X.pos0.data(), d_pos0.p, 8 * n0, hipMemcpyDeviceToHost));
  }
  d_words.drop();
  d_ob.drop();
  {
    dbuf d_sa_s, d_isa_s;
    EXP_HIP(d_sa_s.get(4 * ns));
    EXP_HIP(d_isa_s.get(4 * nis));
    EXP_HIP(hipMemsetAsync(d_isa_s.p, 0, 4 * nis, st));
    hipLaunchKernelGGL(k_exp_samples, dim3(grid_for(n, 256)), dim3(256), 0, st, d_sa, n, (uint32_t *)d_sa_s.p, ns, (uint32_t *)d_isa_s.p, nis);
    EXP_HIP(hipGetLastError());
    EXP_HIP(hipMemcpy(X.sa_s.data(), d_sa_s.p, 4 * ns, hipMemcpyDeviceToHost));
    EXP_HIP(hipMemcpy(X.isa_s.data(), d_isa_s.p, 4 * nis, hipMemcpyDeviceToHost));
  }
  EXP_HIP(hipStreamSynchronize(st));
  return GS_OK;
}

/* csa_wt::serialize (csa_wt.hpp:372-382): wavelet tree (wt_pc.hpp:656-671), sa_samples, isa_samples, alphabet */
static gs_status write_strand_file(const exp_parts &X, const std::string &path) {
  const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
  file_writer fw;
  fw.f = fopen(tmp.c_str(), "wb");
  if (!fw.f) {
    gs_set_error("cannot write " + tmp);
    return GS_ERR_IO;
  }
  setvbuf(fw.f, nullptr, _IOFBF, 1 << 22);
  const exp_tree &T = X.T;
  const uint64_t n = T.n, nbits = T.bv_size, W = X.words.size();
  fw.u64(n);
  fw.u64(T.sigma);
  fw.u64(nbits); /* bit_vector m_bv */
  fw.bytes(X.words.data(), 8 * W);
  fw.u64(64 * (uint64_t)X.basic.size()); /* rank_support_v: int_vector<64> */
  fw.bytes(X.basic.data(), 8 * X.basic.size());
  const bit_src B1{X.words.data(), W, nbits, 1}, B0{X.words.data(), W, nbits, 0};
  write_select(fw, B1, X.pos1.data(), X.pos1.size(), X.ones);
  write_select(fw, B0, X.pos0.data(), X.pos0.size(), nbits - X.ones);
  std::vector<uint8_t> sec;
  serialize_tree(T, sec);
  fw.bytes(sec.data(), sec.size());
  const uint32_t width = hi(n) + 1;
  {
    ivec0 v(X.sa_s.size(), width);
    for (size_t i = 0; i < X.sa_s.size(); i++) v.set(i, X.sa_s[i]);
    fw.vec(v);
  }
  {
    ivec0 v(X.isa_s.size(), width);
    for (size_t i = 0; i < X.isa_s.size(); i++) v.set(i, X.isa_s[i]);
    fw.vec(v);
  }
  sec.clear();
  serialize_alphabet(X.counts, sec);
  fw.bytes(sec.data(), sec.size());
  const bool ok = (fclose(fw.f) == 0) && fw.ok;
  if (!ok || rename(tmp.c_str(), path.c_str()) != 0) {
    (void)remove(tmp.c_str());
    gs_set_error("short write to " + path);
    return GS_ERR_IO;
  }
  return GS_OK;
}

extern "C" gs_status gs_index_save_sdsl(gs_index *ix, const uint8_t *text, uint64_t len, const char *prefix) {
  GS_HANDLE_LOCK(ix);
  if (!ix || !text || !prefix || len != ix->genome_length) return GS_ERR_ARG;
  if (len + 1 >= (1ull << 32)) return GS_ERR_UNSUPPORTED;
  GS_HIP(hipSetDevice(ix->device));
  g_scratch_now = g_scratch_peak = 0;
  try {
    for (int strand = 0; strand < 2; strand++) {
      exp_parts X; /* (the strand's device scratch is released inside, its host parts here, before the next strand) */
      gs_status rc = export_strand_device(ix, strand, text, len, X);
      if (rc == GS_OK) rc = write_strand_file(X, std::string(prefix) + (strand ? ".reverse" : ".forward"));
      if (rc != GS_OK) return rc;
    }
  } catch (const std::bad_alloc &) {
    gs_set_error("out of host memory");
    return GS_ERR_NOMEM;
  }
  return GS_OK;
}

extern "C" uint64_t gs_debug_sdsl_export_scratch(void) { return g_scratch_peak; }

extern "C" gs_status gs_debug_sdsl_sections(const uint64_t counts[256], uint8_t **tree, uint64_t *tree_len, uint8_t **alphabet, uint64_t *alphabet_len) {
  if (!counts || !tree || !tree_len || !alphabet || !alphabet_len) return GS_ERR_ARG;
  try {
    exp_tree T;
    if (!build_tree(counts, T)) return GS_ERR_ARG;
    std::vector<uint8_t> a, b;
    serialize_tree(T, a);
    serialize_alphabet(counts, b);
    uint8_t *pa = (uint8_t *)malloc(a.size()), *pb = (uint8_t *)malloc(b.size());
    if (!pa || !pb) {
      free(pa);
      free(pb);
      return GS_ERR_NOMEM;
    }
    memcpy(pa, a.data(), a.size());
    memcpy(pb, b.data(), b.size());
    *tree = pa;
    *tree_len = a.size();
    *alphabet = pb;
    *alphabet_len = b.size();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}
