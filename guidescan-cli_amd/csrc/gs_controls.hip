/*
 * gs_controls.hip -- non-targeting controls for a library (`guidescan controls`; no counterpart in the reference, whose
 * users draw random protospacers and search each).  The rules are gs_controls_scan.h's: candidates from a counter-based
 * generator, dropped by their own sequence, searched with the existing fast path, kept where the hit list is empty, and
 * thinned by a minimum mutual Hamming distance until N are kept.
 *
 * A round takes up to R consecutive counters (default 2^20) on the handle's device, under the handle's lock:
 *   k_ct_generate     one lane per counter: the word, its letters into the lane's LDS slot, the sequence rule over them
 *                     through gs_select_scan.h -> the charge byte and a 0/1 flag                (no read, 5 B written)
 *   (rocprim 32-bit exclusive scan of the n + 1 flags: the places)
 *   k_ct_gather       the survivors in counter order into the layout gs_enumerate_device takes: letters (from the word,
 *                     computed again: cheaper than storing and reading it), PAM pattern, place in the round, packed word
 *   gs_enumerate_device   the search; its offsets are read where it leaves them in HBM
 *   k_ct_keep         one lane per searched candidate: non-targeting iff off[j + 1] == off[j]; a targeting one is charged
 *   (scan) k_ct_keep_gather   the non-targeting ones in counter order
 *   k_ct_old          one lane per non-targeting candidate against the controls of EARLIER rounds (packed words in HBM,
 *                     every lane reads the same word at the same time: L2 / scalar-like broadcast): order-free
 *   k_ct_walk         ONE wave over the round's non-targeting candidates in counter order, 64 a step: each lane tests its
 *                     candidate against the controls kept earlier in this round (LDS), then the 64 settle among themselves
 *                     by ballots as k_ds_space does; stops at N, and says which candidate was the last one looked at
 *   k_ct_count        the charges of the round's candidates up to that one: one atomic per wave and charge
 * The round's result does not depend on R: a candidate beyond the last one looked at is charged nowhere.
 * At the end k_ct_emit writes the kept controls' arrays, and k_ct_text_len / scan / k_ct_text_write their ids (or, for
 * gs_controls_rows, their kmers-file rows) through gs_ct_row over gs_rowtext.h's sinks.
 */
#include "gs_common.h"
#include "gs_scratch.h"
#include "gs_kmers_obj.h"
#include "gs_controls_scan.h"

#include <rocprim/rocprim.hpp>

#include <atomic>
#include <memory>

#define CT_BLOCK 256
#define CT_WAVE 64
#define CT_SLOT 36u /* bytes of a lane's LDS slot: 31 letters, and 9 dwords apart so that the lanes spread over the banks */

struct gs_ct_gen_args {
  uint64_t seed_mixed, c0; /* c0: the counter of the round's first candidate */
  uint32_t n, L, P, has_rule;
  uint8_t pam[8];
  uint8_t *charge;       /* n */
  uint32_t *flag;        /* n + 1 */
  const uint32_t *place; /* n + 1 */
  uint8_t *o_seqs, *o_pams;
  uint32_t *o_idx;
  uint64_t *o_word;
};
__global__ __launch_bounds__(CT_BLOCK) void k_ct_generate(gs_ct_gen_args a, gs_seq_rule rule) {
  __shared__ uint8_t s_seq[CT_BLOCK * CT_SLOT];
  const uint32_t j = blockIdx.x * CT_BLOCK + threadIdx.x;
  if (j > a.n) return;
  uint32_t ch = GS_SL_PASS;
  if (j < a.n) {
    if (a.has_rule) {
      uint8_t *s = s_seq + threadIdx.x * CT_SLOT; /* the lane's own slot: no barrier */
      gs_ct_ascii(gs_ct_word(a.seed_mixed, a.c0 + j), a.L, s);
      ch = gs_sl_charge(rule, s, a.L);
    }
    a.charge[j] = (uint8_t)ch;
  }
  a.flag[j] = j < a.n && ch == GS_SL_PASS ? 1u : 0u; /* one more entry closes the scan */
}
__global__ __launch_bounds__(CT_BLOCK) void k_ct_gather(gs_ct_gen_args a) {
  const uint32_t j = blockIdx.x * CT_BLOCK + threadIdx.x;
  if (j >= a.n || !a.flag[j]) return;
  const uint64_t o = a.place[j]; /* < the survivors <= n */
  const uint64_t w = gs_ct_word(a.seed_mixed, a.c0 + j);
  gs_ct_ascii(w, a.L, a.o_seqs + o * a.L);
  for (uint32_t u = 0; u < a.P; u++) a.o_pams[o * a.P + u] = a.pam[u];
  a.o_idx[o] = j;
  a.o_word[o] = gs_ct_packed(w, a.L);
}

struct gs_ct_keep_args {
  const uint64_t *off; /* n_s + 1, the search's */
  const uint32_t *idx;
  const uint64_t *word;
  uint32_t n_s;
  uint8_t *charge;
  uint32_t *flag;        /* n_s + 1 */
  const uint32_t *place; /* n_s + 1 */
  uint32_t *nt_idx;
  uint64_t *nt_word;
};
__global__ __launch_bounds__(CT_BLOCK) void k_ct_keep(gs_ct_keep_args a) {
  const uint32_t s = blockIdx.x * CT_BLOCK + threadIdx.x;
  if (s > a.n_s) return;
  uint32_t nt = 0;
  if (s < a.n_s) {
    nt = a.off[s + 1] == a.off[s] ? 1u : 0u;
    if (!nt) a.charge[a.idx[s]] = (uint8_t)GS_CT_TARGETING;
  }
  a.flag[s] = nt;
}
__global__ __launch_bounds__(CT_BLOCK) void k_ct_keep_gather(gs_ct_keep_args a) {
  const uint32_t s = blockIdx.x * CT_BLOCK + threadIdx.x;
  if (s >= a.n_s || !a.flag[s]) return;
  const uint32_t o = a.place[s]; /* < the non-targeting <= n_s */
  a.nt_idx[o] = a.idx[s];
  a.nt_word[o] = a.word[s];
}

struct gs_ct_dist_args {
  const uint32_t *n_nt; /* the non-targeting candidates of the round, where the scan left their number */
  const uint32_t *nt_idx;
  const uint64_t *nt_word;
  uint8_t *dead; /* close to a control of an earlier round */
  uint8_t *charge;
  uint64_t *kept_word, *kept_counter; /* N entries; K0 are filled */
  uint64_t c0;
  uint32_t K0, N, H, n_round;
  uint32_t *state; /* [0] kept in this round, [1] the place in the round of the last candidate looked at */
};
__global__ __launch_bounds__(CT_BLOCK) void k_ct_old(gs_ct_dist_args a) {
  const uint32_t t = blockIdx.x * CT_BLOCK + threadIdx.x;
  if (t >= *a.n_nt) return;
  const uint64_t w = a.nt_word[t];
  bool close = false;
  for (uint32_t u = 0; u < a.K0 && !close; u++) close = gs_ct_close(a.kept_word[u], w, a.H); /* K0 < N <= 16,384 */
  a.dead[t] = close ? 1 : 0;
  if (close) a.charge[a.nt_idx[t]] = (uint8_t)GS_CT_CLOSE;
}
/* One wave.  Lane i of a step holds candidate base + i.  Phase 1: every lane tests its candidate against the controls this
 * round has kept so far, all lanes reading the same entry at the same time.  Phase 2: the survivors settle in order among
 * themselves - the lowest lane of the ballot is kept and appended, the later lanes close to it drop out, the ballot is taken
 * again above it, until it is empty or N is reached.  Control flow is uniform across the wave; no atomics, no spins; the
 * loop is bounded by the round's candidates: at most n / 64 steps of at most N <= GS_CT_MAX_N list entries each.  The round's
 * kept words live in LDS, 8 B each. */
__global__ __launch_bounds__(CT_WAVE) void k_ct_walk(gs_ct_dist_args a) {
  __shared__ uint64_t s_list[GS_CT_MAX_N];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = *a.n_nt, room = a.N - a.K0; /* room >= 1: the driver stops at N */
  uint32_t kept = 0, last = a.n_round - 1u;
  for (uint32_t base = 0; base < n && kept < room; base += CT_WAVE) {
    const uint32_t t = base + lane;
    const bool valid = t < n;
    uint64_t w = 0;
    uint32_t idx = 0;
    bool old = false;
    if (valid) {
      w = a.nt_word[t];
      idx = a.nt_idx[t];
      old = a.dead[t] != 0;
    }
    bool alive = valid && !old, kp = false;
    for (uint32_t u = 0; u < kept; u++) alive = alive && !gs_ct_close(s_list[u], w, a.H);
    unsigned long long cand = __ballot(alive);
    uint32_t stop = CT_WAVE; /* the lane of the N-th control, where the walk ends */
    while (cand) {
      const uint32_t l = (uint32_t)__ffsll((long long)cand) - 1u;
      const uint64_t picked = ((uint64_t)(uint32_t)__shfl((int)(w >> 32), (int)l) << 32) | (uint32_t)__shfl((int)(uint32_t)w, (int)l);
      if (lane == l) {
        kp = true;
        s_list[kept] = w;
        a.kept_word[a.K0 + kept] = w; /* K0 + kept < N */
        a.kept_counter[a.K0 + kept] = a.c0 + idx;
      }
      kept++;
      if (kept >= room) {
        stop = l;
        break;
      }
      alive = alive && lane > l && !gs_ct_close(picked, w, a.H);
      cand = __ballot(alive);
    }
    if (valid && !old && !kp && lane < stop) a.charge[idx] = (uint8_t)GS_CT_CLOSE;
    if (stop < CT_WAVE) last = (uint32_t)__shfl((int)idx, (int)stop);
    __syncthreads(); /* the list's new entries, before the next step reads them */
  }
  if (lane == 0) {
    a.state[0] = kept;
    a.state[1] = last;
  }
}
__global__ __launch_bounds__(CT_BLOCK) void k_ct_count(const uint8_t *charge, uint32_t n, const uint32_t *state, unsigned long long *counts) {
  const uint32_t j = blockIdx.x * CT_BLOCK + threadIdx.x;
  const bool in = j < n && j <= state[1];
  const uint32_t ch = in ? charge[j] : 0u;
  for (uint32_t c = 0; c < GS_CT_CHARGES; c++) {
    const unsigned long long b = __ballot(in && ch == c);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&counts[c], (unsigned long long)__popcll(b));
  }
}

/* ---- the kept controls as an object, their ids and rows -------------------------------------------------------------- */
struct gs_ct_text_args {
  const uint64_t *counter, *word;
  const uint8_t *seqs, *pams, *prefix;
  uint8_t pam[8];
  uint8_t *o_seqs, *o_pams, *o_sense, *o_sense01;
  uint64_t *lens;      /* n + 1 */
  const uint64_t *off; /* n + 1 */
  uint8_t *text;
  uint64_t n;
  uint32_t L, P, prefix_len, rows;
};
__global__ __launch_bounds__(CT_BLOCK) void k_ct_emit(gs_ct_text_args a) {
  const uint64_t t = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (t >= a.n) return;
  gs_ct_ascii(a.word[t], a.L, a.o_seqs + t * a.L); /* the packed word is the word's low 2L bits */
  for (uint32_t u = 0; u < a.P; u++) a.o_pams[t * a.P + u] = a.pam[u];
  a.o_sense[t] = '+';
  a.o_sense01[t] = 1;
}
template <class S>
__device__ __forceinline__ void ct_text_row(S &o, const gs_ct_text_args &a, uint64_t t) {
  gs_ct_row(o, a.prefix, a.prefix_len, a.counter[t], a.seqs + t * a.L, a.L, a.pams + t * a.P, a.P, a.rows != 0u);
}
__global__ __launch_bounds__(CT_BLOCK) void k_ct_text_len(gs_ct_text_args a) {
  const uint64_t t = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (t > a.n) return;
  gs_row_count o;
  if (t < a.n) ct_text_row(o, a, t); /* one more entry closes the scan */
  a.lens[t] = o.n;
}
__global__ __launch_bounds__(CT_BLOCK) void k_ct_text_write(gs_ct_text_args a) {
  const uint64_t t = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (t >= a.n) return;
  gs_row_write o;
  o.p = (char *)a.text + a.off[t];
  ct_text_row(o, a, t);
}

namespace {

std::atomic<uint64_t> g_round{GS_CT_ROUND_DEFAULT};

inline unsigned ct_grid(uint64_t n) { return (unsigned)((n + CT_BLOCK - 1) / CT_BLOCK); }

/* ids (rows == false) or kmers-file rows of n controls: lengths, a 64-bit scan, the write.  a: counter, seqs, pams, n, L, P
 * set.  *d_off / *d_text are allocations of `mem`. */
gs_status ct_text(gs_ct_text_args a, const std::string &prefix, bool rows, hipStream_t st, gs_scratch &mem, void **d_off, void **d_text,
                  uint64_t *bytes) {
  void *d_prefix = nullptr, *d_lens = nullptr;
  gs_prim_tmp tmp;
  GS_TRY(mem.get(prefix.size(), &d_prefix));
  if (!prefix.empty()) GS_HIP(hipMemcpyAsync(d_prefix, prefix.data(), prefix.size(), hipMemcpyHostToDevice, st));
  GS_TRY(mem.get(8 * (a.n + 1), &d_lens));
  GS_TRY(mem.get(8 * (a.n + 1), d_off));
  a.prefix = (const uint8_t *)d_prefix;
  a.prefix_len = (uint32_t)prefix.size();
  a.rows = rows ? 1u : 0u;
  a.lens = (uint64_t *)d_lens;
  a.off = (const uint64_t *)*d_off;
  hipLaunchKernelGGL(k_ct_text_len, dim3(ct_grid(a.n + 1)), dim3(CT_BLOCK), 0, st, a);
  GS_TRY(gs_prim("controls text: scan of the lengths", mem, tmp, [&](void *t, size_t &tb) {
    return rocprim::exclusive_scan(t, tb, (uint64_t *)d_lens, (uint64_t *)*d_off, 0ull, (size_t)a.n + 1, rocprim::plus<uint64_t>(), st);
  }));
  uint64_t total = 0;
  GS_HIP(hipMemcpyAsync(&total, (const uint64_t *)*d_off + a.n, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st)); /* `prefix` may be a temporary of the caller */
  GS_TRY(mem.get(total, d_text));
  a.text = (uint8_t *)*d_text;
  if (a.n) hipLaunchKernelGGL(k_ct_text_write, dim3(ct_grid(a.n)), dim3(CT_BLOCK), 0, st, a);
  GS_HIP(hipStreamSynchronize(st));
  GS_HIP(hipGetLastError());
  mem.drop(d_lens);
  mem.drop(d_prefix);
  if (tmp.p) mem.drop(tmp.p);
  *bytes = total;
  return GS_OK;
}

/* what both the device driver and the host twin refuse */
gs_status ct_rule_args(const gs_controls_rule *r, const char *who, uint32_t *P, uint64_t *C, std::string *prefix) {
  if (!r || !r->pam || (r->n_alt && !r->alt_pams)) return GS_ERR_ARG;
  const size_t pl = strlen(r->pam);
  auto refuse = [&](const std::string &why) {
    gs_set_error(std::string(who) + ": " + why);
    return GS_ERR_ARG;
  };
  if (pl > 8) return refuse("a PAM pattern of more than 8 symbols");
  if (r->n_alt > 31 || r->mismatches > 7) return refuse("at most 31 alt PAMs and 7 mismatches");
  if (r->L < 1 || r->L > GS_CT_MAX_L) return refuse("1 <= L <= 31");
  if (!gs_ct_bounds_ok(r->L, r->min_distance, r->n))
    return refuse("1 <= n <= 16384: the walk keeps a round's controls in LDS");
  if (r->flags & ~(GS_FLAG_PAM_AT_START | GS_FLAG_NO_NEW_TABLES)) return refuse("flags other than GS_FLAG_PAM_AT_START and GS_FLAG_NO_NEW_TABLES");
  if (r->round > GS_CT_ROUND_MAX) return refuse("a round of more than 2^24 counters");
  if (r->seq_rule && !gs_sl_rule_ok(*r->seq_rule))
    return refuse("sequence rule: 0 <= gc_min <= gc_max <= 100, at most 16 motifs of 1 to 32 IUPAC letters");
  *C = r->max_candidates ? r->max_candidates : 1ull << 32;
  if (*C - 1 > ~0ull - r->first) return refuse("first + max_candidates goes beyond 2^64");
  *prefix = r->id_prefix ? r->id_prefix : "control_";
  if (prefix->size() > GS_CT_MAX_PREFIX) return refuse("an id prefix of more than 255 bytes");
  *P = (uint32_t)pl;
  return GS_OK;
}

void ct_report(gs_controls_report *rep, uint64_t first, uint64_t looked, const uint64_t *counts, uint64_t rounds, const double *ms) {
  if (!rep) return;
  memset(rep, 0, sizeof *rep);
  rep->kept = counts[GS_CT_KEPT];
  rep->looked_at = looked;
  rep->gc = counts[GS_SL_GC];
  rep->run = counts[GS_SL_RUN];
  rep->motif = counts[GS_SL_MOTIF];
  rep->targeting = counts[GS_CT_TARGETING];
  rep->close = counts[GS_CT_CLOSE];
  rep->last_counter = looked ? first + looked - 1 : first;
  rep->rounds = rounds;
  for (int i = 0; i < 5 && ms; i++) rep->ms[i] = ms[i];
}

/* The walk cut into rounds the way the device cuts it, on the host: per round the charges of the sequence rule and the
 * search, the non-targeting candidates against the controls of earlier rounds (k_ct_old's part), then the round's own walk
 * (k_ct_walk's part), and the counts up to the last candidate looked at.  Must give what gs_ct_walk gives for any round. */
uint64_t ct_walk_rounds(const gs_controls_rule *rule, const uint8_t *targeting, uint64_t n_candidates, uint64_t *kept_counter, uint64_t *kept_word,
                        uint64_t *counts) {
  const uint64_t sm = gs_ct_mix(rule->seed), R = rule->round, N = rule->n;
  const uint32_t L = rule->L, H = rule->min_distance;
  for (uint32_t c = 0; c < GS_CT_CHARGES; c++) counts[c] = 0;
  uint64_t kept = 0, looked = 0;
  std::vector<uint8_t> charge, dead;
  std::vector<uint64_t> nt_idx, nt_word;
  while (kept < N && looked < n_candidates) {
    const uint64_t n = std::min(R, n_candidates - looked), c0 = rule->first + looked, K0 = kept;
    charge.assign((size_t)n, 0);
    nt_idx.clear(), nt_word.clear();
    for (uint64_t j = 0; j < n; j++) {
      const uint64_t w = gs_ct_word(sm, c0 + j);
      uint8_t seq[GS_CT_MAX_L];
      gs_ct_ascii(w, L, seq);
      uint32_t ch = rule->seq_rule ? gs_sl_charge(*rule->seq_rule, seq, L) : GS_SL_PASS;
      if (ch == GS_SL_PASS && targeting[looked + j]) ch = GS_CT_TARGETING;
      charge[(size_t)j] = (uint8_t)ch;
      if (ch == GS_SL_PASS) nt_idx.push_back(j), nt_word.push_back(gs_ct_packed(w, L));
    }
    dead.assign(nt_idx.size(), 0);
    for (size_t t = 0; t < nt_idx.size(); t++)
      for (uint64_t u = 0; u < K0 && !dead[t]; u++) dead[t] = gs_ct_close(kept_word[u], nt_word[t], H) ? 1 : 0;
    uint64_t last = n - 1;
    for (size_t t = 0; t < nt_idx.size(); t++) {
      bool close = dead[t] != 0;
      for (uint64_t u = K0; u < kept && !close; u++) close = gs_ct_close(kept_word[u], nt_word[t], H);
      if (close) {
        charge[(size_t)nt_idx[t]] = (uint8_t)GS_CT_CLOSE;
        continue;
      }
      kept_counter[kept] = c0 + nt_idx[t];
      kept_word[kept++] = nt_word[t];
      if (kept >= N) {
        last = nt_idx[t];
        break;
      }
    }
    for (uint64_t j = 0; j <= last; j++) counts[charge[(size_t)j]]++;
    looked += last + 1;
  }
  return looked;
}

}  // namespace

extern "C" uint64_t gs_debug_controls_round(uint64_t set) {
  if (set && set <= GS_CT_ROUND_MAX) g_round.store(set);
  return g_round.load();
}

extern "C" gs_status gs_controls_generate(gs_index *ix, const gs_controls_rule *rule, void *stream, gs_kmers **out, gs_controls_report *report) {
  if (!ix || !out) return GS_ERR_ARG;
  *out = nullptr;
  uint32_t P = 0;
  uint64_t C = 0;
  std::string prefix;
  GS_TRY(ct_rule_args(rule, "gs_controls_generate", &P, &C, &prefix));
  const uint32_t L = rule->L, H = rule->min_distance;
  if (2 * L + 3 * P > 59) {
    gs_set_error("gs_controls_generate: 2L + 3P > 59, the shape is outside the fast path's key");
    return GS_ERR_UNSUPPORTED;
  }
  const uint64_t N = rule->n, R = std::min<uint64_t>(rule->round ? rule->round : g_round.load(), C);
  const uint64_t seed_mixed = gs_ct_mix(rule->seed);
  hipStream_t st = (hipStream_t)stream;
  struct lock_guard { /* the offsets stay the handle's between the search and the pass that reads them */
    gs_index *ix;
    bool held = false;
    ~lock_guard() {
      if (held) gs_index_unlock(ix);
    }
  } lock{ix};
  try {
    GS_HIP(hipSetDevice(ix->device));
    GS_TRY(gs_index_lock(ix));
    lock.held = true;
    gs_scratch mem;
    gs_prim_tmp tmp;
    gs_events<7> ev;
    for (hipEvent_t &x : ev.e) GS_HIP(hipEventCreate(&x));
    uint8_t *d_charge = nullptr, *d_seqs = nullptr, *d_pams = nullptr, *d_dead = nullptr;
    uint32_t *d_flag = nullptr, *d_place = nullptr, *d_idx = nullptr, *d_nt_idx = nullptr, *d_state = nullptr;
    uint64_t *d_word = nullptr, *d_nt_word = nullptr, *d_kept_word = nullptr, *d_kept_counter = nullptr;
    unsigned long long *d_counts = nullptr;
    GS_TRY(mem.get(R, &d_charge));
    GS_TRY(mem.get(4 * (R + 1), &d_flag));
    GS_TRY(mem.get(4 * (R + 1), &d_place));
    GS_TRY(mem.get(R * L, &d_seqs));
    GS_TRY(mem.get(R * P, &d_pams));
    GS_TRY(mem.get(4 * R, &d_idx));
    GS_TRY(mem.get(8 * R, &d_word));
    GS_TRY(mem.get(4 * R, &d_nt_idx));
    GS_TRY(mem.get(8 * R, &d_nt_word));
    GS_TRY(mem.get(R, &d_dead));
    GS_TRY(mem.get(8 * N, &d_kept_word));
    GS_TRY(mem.get(8 * N, &d_kept_counter));
    GS_TRY(mem.get(8, &d_state));
    GS_TRY(mem.get(8 * GS_CT_CHARGES, &d_counts));

    gs_ct_gen_args g;
    memset(&g, 0, sizeof g);
    g.seed_mixed = seed_mixed;
    g.L = L;
    g.P = P;
    g.has_rule = rule->seq_rule ? 1u : 0u;
    memcpy(g.pam, rule->pam, P);
    g.charge = d_charge;
    g.flag = d_flag;
    g.place = d_place;
    g.o_seqs = d_seqs;
    g.o_pams = d_pams;
    g.o_idx = d_idx;
    g.o_word = d_word;
    gs_seq_rule seq;
    if (rule->seq_rule)
      seq = *rule->seq_rule;
    else
      gs_seq_rule_init(&seq);
    const uint32_t sflags = rule->flags & (GS_FLAG_PAM_AT_START | GS_FLAG_NO_NEW_TABLES);
    /* The derived tables pay for themselves after 5 searched guides per 1,000 genome bases (guidescan_amd.h): a call builds
     * none before it HAS searched that many - it then pays at most twice what the better choice would have cost, whatever the
     * acceptance turns out to be (estimates of it are off by orders of magnitude).  Tables the handle holds
     * already are used from the first round on. */
    const uint64_t break_even = gs_index_genome_length(ix) / 200;
    uint64_t searched = 0;

    uint64_t counts[GS_CT_CHARGES] = {0, 0, 0, 0, 0, 0}, looked = 0, rounds = 0, kept = 0;
    double ms[5] = {0, 0, 0, 0, 0};
    while (kept < N && looked < C) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(R, C - looked);
      g.c0 = rule->first + looked;
      g.n = n;
      uint32_t n_s = 0, state[2] = {0u, n - 1u};
      GS_HIP(hipMemsetAsync(d_counts, 0, 8 * GS_CT_CHARGES, st));
      GS_HIP(hipEventRecord(ev.e[0], st));
      hipLaunchKernelGGL(k_ct_generate, dim3(ct_grid((uint64_t)n + 1)), dim3(CT_BLOCK), 0, st, g, seq);
      GS_TRY(gs_prim("controls: scan of the sequence rule's flags", mem, tmp, [&](void *t, size_t &tb) {
        return rocprim::exclusive_scan(t, tb, d_flag, d_place, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
      }));
      hipLaunchKernelGGL(k_ct_gather, dim3(ct_grid(n)), dim3(CT_BLOCK), 0, st, g);
      GS_HIP(hipMemcpyAsync(&n_s, d_place + n, 4, hipMemcpyDeviceToHost, st));
      GS_HIP(hipEventRecord(ev.e[1], st));
      GS_HIP(hipStreamSynchronize(st));
      if (n_s > n) {
        gs_set_error("gs_controls_generate: more survivors than candidates");
        return GS_ERR_DEVICE;
      }
      if (n_s) {
        const void *d_off = nullptr, *d_hits = nullptr;
        gs_result_view v;
        GS_TRY(gs_enumerate_device(ix, d_seqs, n_s, L, d_pams, P, rule->alt_pams, rule->n_alt, rule->mismatches,
                                   sflags | (searched < break_even ? GS_FLAG_NO_NEW_TABLES : 0u), st, &d_off, &d_hits, &v));
        searched += n_s;
        if (ix->last_unsupported) {
          gs_set_error("gs_controls_generate: a candidate needs the general path (a PAM symbol outside A,C,G,T,N)");
          return GS_ERR_UNSUPPORTED;
        }
        GS_HIP(hipEventRecord(ev.e[2], st));
        gs_ct_keep_args kp;
        kp.off = (const uint64_t *)d_off;
        kp.idx = d_idx;
        kp.word = d_word;
        kp.n_s = n_s;
        kp.charge = d_charge;
        kp.flag = d_flag; /* the first scan's arrays are free again */
        kp.place = d_place;
        kp.nt_idx = d_nt_idx;
        kp.nt_word = d_nt_word;
        hipLaunchKernelGGL(k_ct_keep, dim3(ct_grid((uint64_t)n_s + 1)), dim3(CT_BLOCK), 0, st, kp);
        GS_TRY(gs_prim("controls: scan of the non-targeting flags", mem, tmp, [&](void *t, size_t &tb) {
          return rocprim::exclusive_scan(t, tb, d_flag, d_place, 0u, (size_t)n_s + 1, rocprim::plus<uint32_t>(), st);
        }));
        hipLaunchKernelGGL(k_ct_keep_gather, dim3(ct_grid(n_s)), dim3(CT_BLOCK), 0, st, kp);
        GS_HIP(hipEventRecord(ev.e[3], st));
        gs_ct_dist_args da;
        da.n_nt = d_place + n_s;
        da.nt_idx = d_nt_idx;
        da.nt_word = d_nt_word;
        da.dead = d_dead;
        da.charge = d_charge;
        da.kept_word = d_kept_word;
        da.kept_counter = d_kept_counter;
        da.c0 = g.c0;
        da.K0 = (uint32_t)kept;
        da.N = (uint32_t)N;
        da.H = H;
        da.n_round = n;
        da.state = d_state;
        hipLaunchKernelGGL(k_ct_old, dim3(ct_grid(n_s)), dim3(CT_BLOCK), 0, st, da);
        hipLaunchKernelGGL(k_ct_walk, dim3(1), dim3(CT_WAVE), 0, st, da);
      } else { /* nothing passed the sequence rule: every candidate of the round was looked at */
        GS_HIP(hipEventRecord(ev.e[2], st));
        GS_HIP(hipEventRecord(ev.e[3], st));
        GS_HIP(hipMemcpyAsync(d_state, state, 8, hipMemcpyHostToDevice, st)); /* `state` lives until the round's wait below */
      }
      hipLaunchKernelGGL(k_ct_count, dim3(ct_grid(n)), dim3(CT_BLOCK), 0, st, (const uint8_t *)d_charge, n, (const uint32_t *)d_state, d_counts);
      GS_HIP(hipEventRecord(ev.e[4], st));
      unsigned long long c[GS_CT_CHARGES];
      GS_HIP(hipMemcpyAsync(state, d_state, 8, hipMemcpyDeviceToHost, st));
      GS_HIP(hipMemcpyAsync(c, d_counts, 8 * GS_CT_CHARGES, hipMemcpyDeviceToHost, st));
      GS_HIP(hipStreamSynchronize(st));
      GS_HIP(hipGetLastError());
      uint64_t sum = 0;
      for (uint32_t i = 0; i < GS_CT_CHARGES; i++) sum += c[i];
      if (state[1] >= n || state[0] > N - kept || sum != (uint64_t)state[1] + 1 || c[GS_CT_KEPT] != state[0]) {
        gs_set_error("gs_controls_generate: the round's counts do not add up");
        return GS_ERR_DEVICE;
      }
      for (uint32_t i = 0; i < GS_CT_CHARGES; i++) counts[i] += c[i];
      kept += state[0];
      looked += (uint64_t)state[1] + 1;
      rounds++;
      static const int from[4] = {0, 1, 2, 3};
      double r_ms[4];
      GS_TRY(ev.elapsed(from, 4, r_ms));
      for (int i = 0; i < 4; i++) ms[i] += r_ms[i];
    }

    /* the object: a parsed one (no positions, ids from the start) with the counters beside it */
    std::unique_ptr<gs_kmers, void (*)(gs_kmers *)> own(new gs_kmers(), km_release);
    gs_kmers *km = own.get();
    km->device = ix->device;
    km->parsed = km->have_ids = km->controls = true;
    km->n = kept;
    km->k = L;
    km->P = P;
    km->ct_prefix = prefix;
    km->h_counters.resize((size_t)kept);
    if (kept) GS_HIP(hipMemcpyAsync(km->h_counters.data(), d_kept_counter, 8 * kept, hipMemcpyDeviceToHost, st));
    void *o_seqs = nullptr, *o_pams = nullptr, *o_sense = nullptr, *o_s01 = nullptr, *d_off = nullptr, *d_text = nullptr;
    GS_TRY(mem.get(kept * L, &o_seqs));
    GS_TRY(mem.get(kept * P, &o_pams));
    GS_TRY(mem.get(kept, &o_sense));
    GS_TRY(mem.get(kept, &o_s01));
    gs_ct_text_args ta;
    memset(&ta, 0, sizeof ta);
    ta.counter = d_kept_counter;
    ta.word = d_kept_word;
    memcpy(ta.pam, rule->pam, P);
    ta.o_seqs = (uint8_t *)o_seqs;
    ta.o_pams = (uint8_t *)o_pams;
    ta.o_sense = (uint8_t *)o_sense;
    ta.o_sense01 = (uint8_t *)o_s01;
    ta.seqs = ta.o_seqs;
    ta.pams = ta.o_pams;
    ta.n = kept;
    ta.L = L;
    ta.P = P;
    GS_HIP(hipEventRecord(ev.e[5], st));
    if (kept) hipLaunchKernelGGL(k_ct_emit, dim3(ct_grid(kept)), dim3(CT_BLOCK), 0, st, ta);
    uint64_t id_bytes = 0;
    GS_TRY(ct_text(ta, prefix, false, st, mem, &d_off, &d_text, &id_bytes));
    GS_HIP(hipEventRecord(ev.e[6], st));
    GS_HIP(hipStreamSynchronize(st));
    static const int from_ids[1] = {5};
    GS_TRY(ev.elapsed(from_ids, 1, ms + 4));
    for (void *q : {o_seqs, o_pams, o_sense, o_s01, d_off, d_text}) mem.keep(q);
    km->d_seqs = o_seqs, km->d_pams = o_pams, km->d_sense = o_sense, km->d_sense01 = o_s01, km->d_id_off = d_off, km->d_ids = d_text;
    km->id_bytes = id_bytes;
    ct_report(report, rule->first, looked, counts, rounds, ms);
    *out = own.release();
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_controls_rows(gs_kmers *km, char **text, uint64_t *len) {
  if (!km || !text || !len) return GS_ERR_ARG;
  if (!km->controls || km->device < 0) {
    gs_set_error("gs_controls_rows takes the object gs_controls_generate made");
    return GS_ERR_ARG;
  }
  *text = nullptr;
  *len = 0;
  try {
    GS_HIP(hipSetDevice(km->device));
    gs_scratch mem;
    void *d_counter = nullptr, *d_off = nullptr, *d_text = nullptr;
    GS_TRY(mem.get(8 * km->n, &d_counter));
    if (km->n) GS_HIP(hipMemcpy(d_counter, km->h_counters.data(), 8 * km->n, hipMemcpyHostToDevice));
    gs_ct_text_args ta;
    memset(&ta, 0, sizeof ta);
    ta.counter = (const uint64_t *)d_counter;
    ta.seqs = (const uint8_t *)km->d_seqs;
    ta.pams = (const uint8_t *)km->d_pams;
    ta.n = km->n;
    ta.L = km->k;
    ta.P = km->P;
    uint64_t bytes = 0;
    GS_TRY(ct_text(ta, km->ct_prefix, true, nullptr, mem, &d_off, &d_text, &bytes));
    GS_TRY(gs_text_to_host(d_text, bytes, text));
    *len = bytes;
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_controls_counters(gs_kmers *km, uint64_t *n, const uint64_t **counters) {
  if (!km || !km->controls) return GS_ERR_ARG;
  if (n) *n = km->n;
  if (counters) *counters = km->h_counters.data();
  return GS_OK;
}

extern "C" gs_status gs_debug_controls_host(const gs_controls_rule *rule, const uint8_t *targeting, uint64_t n_candidates, uint64_t **counters,
                                            char **rows, uint64_t *rows_len, gs_controls_report *report) {
  if (!counters || !rows || !rows_len || (n_candidates && !targeting)) return GS_ERR_ARG;
  *counters = nullptr;
  *rows = nullptr;
  *rows_len = 0;
  uint32_t P = 0;
  uint64_t C = 0;
  std::string prefix;
  GS_TRY(ct_rule_args(rule, "gs_debug_controls_host", &P, &C, &prefix));
  const uint32_t L = rule->L;
  const uint64_t n = std::min(n_candidates, C), room = std::min(rule->n, n);
  try {
    std::vector<uint64_t> kc((size_t)room + 1), kw((size_t)room + 1);
    uint64_t counts[GS_CT_CHARGES];
    const uint64_t looked = rule->round
                                ? ct_walk_rounds(rule, targeting, n, kc.data(), kw.data(), counts)
                                : gs_ct_walk(rule->seed, rule->first, n, L, rule->seq_rule, targeting, rule->min_distance, rule->n, kc.data(), kw.data(), counts);
    const uint64_t kept = counts[GS_CT_KEPT];
    std::vector<uint8_t> seq((size_t)kept * L);
    uint64_t bytes = 0;
    for (uint64_t t = 0; t < kept; t++) {
      gs_ct_ascii(kw[t], L, seq.data() + t * L);
      gs_row_count o;
      gs_ct_row(o, (const uint8_t *)prefix.data(), (uint32_t)prefix.size(), kc[t], seq.data() + t * L, L, (const uint8_t *)rule->pam, P, true);
      bytes += o.n;
    }
    char *text = (char *)malloc((size_t)bytes + 1);
    uint64_t *kout = (uint64_t *)malloc(8 * (size_t)kept + 8);
    if (!text || !kout) {
      free(text);
      free(kout);
      return GS_ERR_NOMEM;
    }
    gs_row_write o;
    o.p = text;
    for (uint64_t t = 0; t < kept; t++) {
      gs_ct_row(o, (const uint8_t *)prefix.data(), (uint32_t)prefix.size(), kc[t], seq.data() + t * L, L, (const uint8_t *)rule->pam, P, true);
      kout[t] = kc[t];
    }
    text[bytes] = '\0';
    *counters = kout;
    *rows = text;
    *rows_len = bytes;
    ct_report(report, rule->first, looked, counts, 0, nullptr);
    return GS_OK;
  } catch (const std::bad_alloc &) {
    return GS_ERR_NOMEM;
  }
}

extern "C" gs_status gs_debug_controls_sequences(uint64_t seed, uint64_t first, uint64_t n, uint32_t L, uint8_t *out) {
  if ((n && !out) || L < 1 || L > GS_CT_MAX_L) return GS_ERR_ARG;
  const uint64_t sm = gs_ct_mix(seed);
  for (uint64_t j = 0; j < n; j++) gs_ct_ascii(gs_ct_word(sm, first + j), L, out + j * L);
  return GS_OK;
}
