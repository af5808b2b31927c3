/*
 * guidescan_amd.h -- C-ABI of the MI355X-native off-target enumerator.
 *
 * This is the drop-in boundary for guidescan's enumerate hot path.  The
 * reference has no FFI: the seam is a C++ template call from the per-guide
 * pipeline into the FM-index.  Each entry point below
 * names the reference interface it replaces (paths relative to the reference
 * tree).  Plain pointers and sizes only; no C++ or torch types; every function
 * returns a gs_status and never throws.
 *
 * Batch-oriented by design: the reference calls inexact_search once per guide
 * per strand from N std::threads (src/guidescan.cxx:240-247); a GPU needs the
 * whole batch, so gs_enumerate takes n guides and returns CSR hit lists in the
 * reference's canonical per-guide order (include/genomics/process.hpp:100-115).
 */
#ifndef GUIDESCAN_AMD_H
#define GUIDESCAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GS_OK = 0,
  GS_ERR_ARG = 1,         /* bad argument (NULL, sizes out of range) */
  GS_ERR_DEVICE = 2,      /* HIP runtime error / no usable device */
  GS_ERR_UNSUPPORTED = 3, /* input outside what the device path implements */
  GS_ERR_NOMEM = 4,
  GS_ERR_IO = 5,
  GS_ERR_FORMAT = 6 /* malformed index file */
} gs_status;

/* Opaque handle: both strand indexes of one genome resident in one GPU's HBM.
 * Replaces the two `genome_index<wt_huff<>,64,8192>` objects built in
 * src/guidescan.cxx:198-211 (include/genomics/index.hpp:23-123).
 * Threads: the reference calls its seam from N std::threads on one const index
 * (src/guidescan.cxx:240-247).  A handle owns its workspace, its lazily built tables and the
 * device buffers its results are left in, so it runs ONE call at a time: every entry point that
 * takes a handle holds the handle's lock for the whole call and other threads' calls wait.  The
 * host-pointer entry points (gs_enumerate, gs_enumerate_general*, gs_score, ...) copy their
 * results out under the lock: any number of threads may call them on one handle and each gets
 * the bytes a single thread would.  The device-pointer entry points leave their results in the
 * handle's buffers "until the next call": a thread that wants to read or score them holds the
 * handle with gs_index_lock ... gs_index_unlock around its calls (the lock is recursive). */
typedef struct gs_index gs_index;

/* One off-target hit, 16 bytes.
 *   pos : signed absolute coordinate exactly as process.hpp:104,111 computes it
 *         (forward-index hit: -SA[row]; reverse-index hit: L-(SA[row]+1)).
 *   key : canonical sort key that also encodes the whole `match` struct
 *         (include/genomics/structures.hpp:33-43):
 *           bits 63..61  match.mismatches
 *           bit  60      0 = found in the forward index, 1 = reverse index
 *           bits 59..1   match.sequence as per-position codes, position 0 first (2L + 3P <= 59 bits,
 *                        from bit 59 down; what a sequence does not use stays zero):
 *                        guide positions (2 bits): 0 = equals the query base
 *                          (upper case), 1..3 = mismatch, the matched base's rank
 *                          among the three other bases in A<C<G<T order (lower case);
 *                        PAM positions (3 bits): A=0 C=1 G=2 N=3 T=4 (upper case).
 *           bit  0       zero
 *         (Sequences of up to 52 bits - 20-mers with a PAM of up to four symbols - leave bits 7..1 zero: the
 *         layout of earlier versions.  23-mers with a four-symbol PAM use 58.)
 *         Ascending key == the reference's order of (distance, index, std::set<match>
 *         ordered by sequence string) because 'A'<'C'<'G'<'N'<'T'<'a'<'c'<'g'<'t'.
 * gs_decode_sequence() rebuilds match.sequence from (guide, key). */
typedef struct {
  int64_t pos;
  uint64_t key;
} gs_hit;

#define GS_KEY_MISMATCHES(key) ((uint32_t)((key) >> 61))
#define GS_KEY_INDEX(key) ((uint32_t)(((key) >> 60) & 1))

/* flags for gs_enumerate */
#define GS_FLAG_PAM_AT_START 1u /* --start, process.hpp:63,84-87 */
/* Walk the whole search tree from the root exactly as the reference does (no prefix-table
 * shortcut).  Same hits; n_ext then equals the reference traversal's node count.  Without it
 * n_ext counts only the extensions actually executed below the table depth. */
#define GS_FLAG_FAITHFUL_WALK 2u
/* Measurement only: run the counting instantiation of the search kernel, which tallies the distinct
 * 64-byte lines each of its load instructions asks for (gs_index_last_counters; with the handle's switch
 * GS_COUNT_SHIFT=7 - gs_index_set_option - 128-byte blocks, what the memory system serves as one random request).
 * Same results, slower; never set in a timed call. */
#define GS_FLAG_COUNT_REQUESTS 4u
/* Also return, per guide, the number of hits BEFORE duplicate sequences are dropped
 * (gs_result_view.raw_hits): the quantity the reference's --threshold filter compares with 1
 * (off_target_counter, process.hpp:25-27 and 66-76 - one count per PAM pattern that matches, so a
 * site two patterns of the list match counts twice).  Saturates at 2^32-1. */
#define GS_FLAG_RAW_COUNTS 8u
/* Do not build new derived tables for this call (the PAM-pair and deep tables, DESIGN.md 4.9-4.10: about
 * 0.3 s and tens of GB at hg38 size, kept on the handle); tables the handle already holds are used.
 * For short jobs: the tables pay for themselves after ~5 guides per 1,000 genome bases (15 M guides
 * at hg38 size).  Same results either way. */
#define GS_FLAG_NO_NEW_TABLES 16u

typedef struct {
  uint64_t n_guides;
  uint64_t n_hits;
  const uint64_t *guide_offsets; /* n_guides+1 entries, host memory owned by the result */
  const gs_hit *hits;            /* n_hits entries, host memory owned by the result */
  /* work counters of SURVEY.md section 8d (properties of the input): */
  uint64_t n_ext;     /* search-tree nodes extended (a3 calls with position>=0 + a4 calls with begin!=end);
                         exact only under GS_FLAG_FAITHFUL_WALK, see there */
  uint64_t n_matches; /* distinct (index, match.sequence) intervals */
  /* device timing of the last call, milliseconds (HIP events on the call's stream) */
  float ms_search;  /* search kernel only */
  float ms_total;   /* prepare + search + order + locate, device side */
  /* Guides outside what the fast path encodes (a guide symbol outside A,C,G,T; a symbol other than
   * A,C,G,T,N in the guide's own PAM; an alt PAM with such a symbol that the genome contains): their
   * hit lists are EMPTY here and guide_flags[i] has bit 0 set - enumerate exactly those guides with
   * gs_enumerate_general (same arguments) and format them with gs_format_guide_ex.  The rest of the
   * batch is unaffected.  guide_flags: n_guides bytes (host memory owned by the result), or NULL
   * when n_unsupported == 0. */
  uint64_t n_unsupported;
  const uint8_t *guide_flags;
  const uint32_t *raw_hits; /* n_guides entries with GS_FLAG_RAW_COUNTS, else NULL */
} gs_result_view;
#define GS_GUIDE_NEEDS_GENERAL 1u

typedef struct gs_result gs_result;

/* ---- index lifecycle ------------------------------------------------------ */

/* Build both strand indexes from the forward genome text (the reference's
 * <fasta>.forward.dna bytes: upper-cased, concatenated, no separators,
 * src/genomics/seq_io.cxx:57-63) and upload them to `device`.
 * Replaces `guidescan index` = sdsl::construct x2 (src/guidescan.cxx:109-179)
 * followed by sdsl::load_from_file x2 (src/guidescan.cxx:198-208).
 * The suffix arrays are built on the GPU. */
gs_status gs_index_build(const uint8_t *text, uint64_t len, int device, gs_index **out);

/* Same, with caller-supplied suffix arrays of text+'\0' and of
 * reverse_complement(text)+'\0' (len+1 uint32 entries each). */
gs_status gs_index_build_with_sa(const uint8_t *text, uint64_t len, const uint32_t *sa_fwd,
                                 const uint32_t *sa_rev, int device, gs_index **out);

/* Import the reference's on-disk index: <prefix>.forward, <prefix>.reverse
 * (sdsl::csa_wt<wt_huff<>,64,8192>::serialize, sdsl/include/sdsl/csa_wt.hpp:372-382).
 * Replaces sdsl::load_from_file (src/guidescan.cxx:198-208).  Both files are turned into text AND suffix array on the
 * device - BWT by wavelet-tree access, LF walks from the SA samples, every step writing text[q - 1] and SA[row] - so no
 * suffix sort runs; .reverse must be the index of reverse_complement(.forward's text) (src/guidescan.cxx:146-157),
 * else GS_ERR_FORMAT.  The arrays come from the files' samples, not from a sort, so they are then checked against the
 * text (gs_index_verify_sa; GS_ERR_FORMAT): every row (GS_VERIFY_ALL_ROWS) where the strand has its inverse suffix array -
 * a damaged file whose arrays are in any wrong order is DETECTED; where it has none (GS_NO_ISA, GS_NO_BIDIR, a memory
 * budget that left it out) 65,536 sampled pairs per strand - values out of range or repeated and damage that changes
 * the text are detected, but sample values exchanged between copies of a repeat (the text stays, a few hundred rows
 * name the other copy) are mostly NOT detected from some 2^22 rows on.  Without a .reverse file (or with more than 16
 * distinct symbols) .forward's text is recovered on the host and both strands are built from it. */
gs_status gs_index_open_sdsl(const char *prefix, int device, gs_index **out);
/* The genome text stored in one reference index file (BWT inverted on the host: the importer's host path).
 * *text is malloc'ed: release with gs_free. */
gs_status gs_sdsl_extract_text(const char *index_file, uint8_t **text, uint64_t *len);

/* Native index file: both suffix arrays of a built index (4 bytes per row and strand, with the text's
 * length and a fingerprint), so that a later gs_index_open_sa skips the suffix sort - the part of
 * `guidescan index` worth storing (src/guidescan.cxx:168-175 stores the whole csa_wt; the device
 * layout here is derived data rebuilt from text + suffix arrays in seconds).  `text` as given to
 * gs_index_build.  gs_index_open_sa returns GS_ERR_FORMAT when the file belongs to another text. */
gs_status gs_index_save_sa(gs_index *ix, const uint8_t *text, uint64_t len, const char *path);
/* The reference's own index files from a handle, however it was made: <prefix>.forward and <prefix>.reverse, byte for
 * byte what sdsl::csa_wt<wt_huff<>,64,8192>::serialize writes for the strand's text - the seam of the reference's `index`
 * command (src/guidescan.cxx:168-175), layout in SURVEY.md App. A.  The reference binary and gs_index_open_sdsl open
 * them.  BWT, wavelet-tree bits, rank blocks, select samples and SA / ISA samples are made on the device from the handle's
 * suffix arrays, strand by strand (scratch: about 3.5 bytes per base; GS_ERR_NOMEM leaves the handle usable); each file
 * is written under a temporary name and renamed.  `text` as given to gs_index_build; GS_ERR_ARG when len is not the
 * handle's.  The handle is left as it was found. */
gs_status gs_index_save_sdsl(gs_index *ix, const uint8_t *text, uint64_t len, const char *prefix);
/* The two parts of such a file that are functions of the 256 symbol counts alone (host only; tests pin them): the
 * serialised _byte_tree (Huffman shape, wt_huff.hpp:84-117; wt_helper.hpp:164-278) and the serialised byte_alphabet
 * (sdsl/lib/csa_alphabet_strategy.cpp:25-55, 103-113).  Both malloc'ed: release with gs_free. */
gs_status gs_debug_sdsl_sections(const uint64_t counts[256], uint8_t **tree, uint64_t *tree_len, uint8_t **alphabet,
                                 uint64_t *alphabet_len);
/* peak device scratch, in bytes, of the last gs_index_save_sdsl of this process */
uint64_t gs_debug_sdsl_export_scratch(void);
gs_status gs_index_open_sa(const uint8_t *text, uint64_t len, const char *path, int device, gs_index **out);

void gs_index_close(gs_index *ix);
/* Work counters of the last gs_enumerate_device call on this handle: [0] extensions executed by the
 * Occ walk, [1] items whose matches overflowed their slots, [2] distinct matches, [4] items seeded
 * from both strands' tables, [5] items seeded one-sided although two-sided seeding was on, [6] guides
 * redone because their matches overflowed the first pass's slots, [7] bit 0: the whole batch was ordered
 * device-wide, bit 1: the redone guides were, bit 2: the overflowing guides' records came out of the arena,
 * bit 3: the device-wide ordering ran as one sort of (sort word, low bits of the first row), bit 4: it had runs
 * to put right afterwards, bit 5: the guides beyond LDS were ordered per guide in tiles (gs_tileorder.hip),
 * bit 6: that form gave up (overlapping PAM patterns, a bucket beyond its slots) and the device-wide one ran
 * (DESIGN.md section 5.3), [13] slots per item of the first pass, [14] / [15] sum and
 * maximum of the per-item match counts; with
 * GS_FLAG_COUNT_REQUESTS also the 64-byte lines requested by the search kernel: [8] prefix-table
 * lines, [9] 16-bit context lines, [10] 32-bit context words, [11] SA/ISA gathers of the search,
 * [12] Occ block lines, [3] lines of the seed recipe lists.  (the bytes the
 * roofline is priced on.)  [7] >> 8: items whose seeds went through PAM-pair tables. */
gs_status gs_index_last_counters(const gs_index *ix, uint64_t out[16]);
/* what the main pass of the last gs_enumerate_device call was launched with: [0] 1 = the walking kernel, [1] 1 = the kernel
 * without the strand tables' side of the seeding (every pattern on PAM-pair + deep tables), [2] 1 = deep tables on the other
 * strand's side, [3] items a wave takes per visit to the work counter, [4] ... in the two seeding launches (0: another form
 * ran), [5] PAM-pair tables in use, [6] |X|, [7] rotated copies per strand table in place */
gs_status gs_index_last_launch(const gs_index *ix, uint64_t out[8]);
/* The spaced tables in the last gs_enumerate_device call (the seeding launches' lookups keyed on a guide's first |X| and last
 * L - k symbols): [0] lookups (one per item and PAM-pair table; 0: the path did not run), [1] rows
 * they read, [2] the most rows one lookup read, [3] rows that matched; and on the handle: [4] bytes of the tables,
 * [5] microseconds their build took. */
gs_status gs_index_last_spaced(const gs_index *ix, uint64_t out[6]);
/* The last batch's heavy items (DESIGN.md sections 5.1, 5.3): [0] items of which at least one verification pass was
 * handed to other waves, [1] packages reserved in the queue, [2] packages the queue holds, [3] tickets the helping waves
 * drew; [4] guides with an item of more than 2^20 match records, which the per-guide tile ordering leaves to the
 * device-wide ordering - alone, the rest of the batch stays in tiles; [5] launches of the package-running form BEHIND the
 * search launch (the one beside it came too early and left); [6] the form the search ran in: 0 every item with its wave,
 * 1 one launch that publishes and helps, 2 two launches (the plain form publishes, the heavy form beside it runs the
 * packages), 3 the two seeding launches of a batch whose every pattern has its PAM-pair + deep tables and that shares no
 * item (gs_seed.hip); [7] guides of the batch whose own k-mer heads an interval of 8 x share_min rows or more in a strand
 * table: what the form is chosen from, together with the last batch's count of heavy passes. */
gs_status gs_index_last_sharing(const gs_index *ix, uint64_t out[8]);
/* Switches of a handle.  The library's tuning and test switches ("GS_NO_BIDIR", "GS_SHARE_MIN", "GS_DEBUG", ... -
 * DESIGN.md names each where it acts) are a per-handle table: filled from the process environment's GS_* variables
 * ONCE, when the handle is made (gs_index_build / _with_sa / _open_sdsl / _open_sa), and changed only through
 * gs_index_set_option (value NULL removes the entry).  No gs_enumerate* / gs_score* / gs_kmers* call reads the
 * environment: a host that calls setenv from another thread cannot change a running batch.  The reference has no
 * counterpart (its behaviour is fixed at compile time, src/guidescan.cxx:24-27).  gs_index_get_option copies the
 * value into out[cap] (GS_ERR_ARG when the switch is not set or does not fit). */
gs_status gs_index_set_option(gs_index *ix, const char *key, const char *value);
gs_status gs_index_get_option(const gs_index *ix, const char *key, char *out, uint64_t cap);
/* Hold / release the handle's lock (see gs_index above): between the two, calls on this handle
 * from other threads wait, and the device buffers a gs_enumerate_device call returned stay as
 * they are.  Stands where the reference needs nothing (its index is const and its per-call state
 * lives on the caller's stack, include/genomics/index.hpp:102-110). */
gs_status gs_index_lock(gs_index *ix);
gs_status gs_index_unlock(gs_index *ix);
uint64_t gs_index_genome_length(const gs_index *ix); /* sum of chromosome lengths (no sentinel) */
uint64_t gs_index_device_bytes(const gs_index *ix);

/* ---- the hot path ---------------------------------------------------------- */

/* Enumerate all off-targets of n guides.
 *   guides     : n*L ASCII bytes (kmer.sequence), no terminators
 *   guide_pams : n*P ASCII bytes (kmer.pam), P may be 0
 *   alt_pams   : n_alt*P ASCII bytes (-a/--alt-pam), searched before the guide's own PAM
 * Replaces, per guide, process.hpp:51-115: query/PAM preparation, the two
 * genome_index::inexact_search calls (index.hpp:377-398 -> 182-248 -> 125-170),
 * the std::set<match> ordering (process.hpp:21-23) and the resolve() expansion
 * (index.hpp:53-55 -> csa_wt.hpp:333-346).  Bulge budgets are 0 (index.hpp:388-391).
 * Host pointers in, host result out (device work and copies inside). */
gs_status gs_enumerate(gs_index *ix, const char *guides, uint64_t n, uint32_t L,
                       const char *guide_pams, uint32_t P, const char *alt_pams, uint32_t n_alt,
                       uint32_t mismatches, uint32_t flags, gs_result **out);

/* Same with the guide/PAM arrays already resident in this device's HBM and the
 * result left in HBM: *d_offsets (n+1 uint64) and *d_hits (gs_hit[]) point into
 * buffers owned by the index handle, valid until the next call on it.
 * `stream` is a hipStream_t (NULL = default stream).  This is what bench.py times. */
gs_status gs_enumerate_device(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L,
                              const void *d_guide_pams, uint32_t P, const char *alt_pams,
                              uint32_t n_alt, uint32_t mismatches, uint32_t flags, void *stream,
                              const void **d_offsets, const void **d_hits, gs_result_view *stats);
/* What the FIRST batch of a shape pays once per handle - the seed recipes, the PAM-pair and deep tables of the PAM patterns
 * (0.3 s and 24-33 GB per strand at hg38 size), the workspace of a batch of n guides - done ahead of the first job: n guides
 * of length L drawn from a generator (not from the genome: few hits), each with the pattern `pam` (P symbols), are enumerated
 * with these alt PAMs, budget and flags and the result is dropped.  Nothing in the reference corresponds (its index is ready
 * when loaded, src/guidescan.cxx:198-211); a service calls this after opening a handle so that a 2,500-guide job
 * (manual/manual.tex:472-475) is not all warm-up.  The batch's own workspace for hits still grows with the first real batch.
 * The call runs a batch on the handle: device results an earlier gs_enumerate_device left in HBM are no longer valid after
 * it; what the handle has learned from the caller's batches (slot sizes, the form of the search) is kept as it was. */
gs_status gs_index_prepare(gs_index *ix, uint64_t n, uint32_t L, const char *pam, uint32_t P, const char *alt_pams,
                           uint32_t n_alt, uint32_t mismatches, uint32_t flags);

/* flags of the last gs_enumerate_device call on this handle (device memory, n bytes, valid until the
 * next call) and how many guides carry GS_GUIDE_NEEDS_GENERAL */
gs_status gs_index_last_guide_flags(const gs_index *ix, const void **d_flags, uint64_t *n_unsupported);
gs_status gs_result_get(const gs_result *r, gs_result_view *view);
void gs_result_free(gs_result *r);

/* Rebuild match.sequence (index.hpp:226,243-244; lower case = mismatch) from the
 * hit key.  `guide`/`L`, `P`, `flags` as passed to gs_enumerate.  out needs L+P+1 bytes. */
gs_status gs_decode_sequence(const char *guide, uint32_t L, uint32_t P, uint32_t flags,
                             uint64_t key, char *out);

/* ---- unit-level entry points (parity tests of SURVEY section 8a rows a6-a8) ---- */

/* Occ(c, i) for c in A,C,G,T at each rows[j] in [0, n]: out[4*j + {0,1,2,3}].
 * Replaces csa_wt::rank_bwt (sdsl/include/sdsl/csa_wt.hpp:270-273). strand 0 = forward index. */
gs_status gs_rank_bwt4(gs_index *ix, int strand, const uint64_t *rows, uint64_t n, uint64_t *out);
/* SA[rows[j]].  Replaces genome_index::resolve (index.hpp:53-55). */
gs_status gs_resolve(gs_index *ix, int strand, const uint64_t *rows, uint64_t n, uint64_t *out);
/* csa.C[csa.char2comp[c]] for c in "ACGT" then 'N' (0 when absent), and csa.size(). */
gs_status gs_index_meta(const gs_index *ix, int strand, uint64_t C_acgtn[5], uint64_t *size);
/* copy the device-resident suffix array back (n = size entries) */
gs_status gs_index_copy_sa(gs_index *ix, int strand, uint32_t *out);
/* The seed plan of k_search as data (host only, no device needed): which depth-k nodes of the
 * reference's search tree (index.hpp:182-248: the variants of a guide's first k consumed symbols with
 * at most m substitutions) a batch shape looks up, and from which strand's table.  Writes the 64-bit
 * recipes (one-sided list | this strand's share | the other strand's share) to out[0..cap) and their
 * counts to counts[3]; astar = NULL: one-sided only.  Recipe: bits 2:0 substitutions n, 5:3 lower bound
 * the other strand's verification applies, 6 reads a rotated copy, 11:7 of which step, then n fields of 7
 * bits from bit 12: step * 4 + digit (the digit-th other base).  n_x = |X|: the leading steps only this
 * strand's table covers; deep: the other strand's recipes index a deep table (steps = guide symbols).
 * gs_debug_choose_thresholds: the cost model's a*(o) for that shape (tests pin both). */
gs_status gs_debug_seed_recipes(uint32_t k, uint32_t L, uint32_t P, uint32_t m, uint32_t n_x, const uint32_t *astar,
                                uint32_t deep, uint64_t *out, uint64_t cap, uint64_t counts[3]);
void gs_debug_choose_thresholds(uint32_t m, uint32_t n_x, uint32_t n_o, uint32_t n_r, double pam_expansions,
                                double verify_a, double verify_b, uint32_t astar[8]);
/* This strand's share as it is read through PAM-pair tables (host only): the whole list, or (trimmed != 0) the list without
 * the class "no substitution in X, all m in O", which a spaced table's lookup finds instead. */
gs_status gs_debug_seed_recipes_a8(uint32_t k, uint32_t m, uint32_t n_x, const uint32_t *astar, uint32_t trimmed, uint64_t *out,
                                   uint64_t cap, uint64_t *count);
/* The probe lists the two seeding launches read beside those recipes (host only), two words per recipe in the recipes' order.
 * side 0: the other strand's share through deep tables - {xor on the item's index, substitutions << 14 | lo << 27 |
 * substitutions}; side 1 / 2: this strand's share, whole / trimmed, through a PAM-pair table whose rotated copies start at
 * step rot_first (31: none) - {xor on the index as the copy it reads holds it, substitutions << 14 | copy << 4 |
 * substitutions}, copy 0 = the plain table, copy c = the copy of step rot_first + c - 1. */
gs_status gs_debug_seed_probes(uint32_t k, uint32_t L, uint32_t P, uint32_t m, uint32_t n_x, const uint32_t *astar, uint32_t side,
                               uint32_t rot_first, uint32_t *out, uint64_t cap, uint64_t *count);
/* What the seeding launches make of one recipe word for the packed guide q (host only): out[0] = the seed's path word
 * (guide symbol t's code at bit 57 - 2 t; on the other strand's side, side_b != 0, sid carries the base under the PAM's N in
 * bits 25:24 and the pattern's number in 27:26), out[1] = the recipe's xor on a table index of nst symbols. */
gs_status gs_debug_seed_path(uint64_t q, const uint32_t pam[4], uint64_t word, uint32_t sid, uint32_t side_b, uint32_t L, uint32_t P,
                             uint32_t nst, uint64_t out[2]);
/* Index pidx of a depth-k table as the copy rotated at consumption step rs holds it (host only). */
gs_status gs_debug_rot_index(uint32_t pidx, uint32_t k, uint32_t rs, uint32_t *out);
/* The device arrays the handle keeps between calls and the bytes they count for in gs_index_device_bytes: [0] arrays and
 * [1] bytes of the two strands (Occ blocks, suffix array, tables, context and inverse arrays, rotated copies), [2] arrays and
 * [3] bytes of the PAM-pair table slots (pair, deep and spaced tables).  [1] + [3] = gs_index_device_bytes.  Tests only. */
gs_status gs_debug_resident(gs_index *ix, uint64_t out[4]);
/* The scalars a reader needs to interpret and size the index's device arrays.  Tests only; takes the handle's lock, changes
 * nothing, launches no kernel.
 * slot = -1, a strand: [0] rows n, [1] Occ blocks, [2] table depth k (0: no table), [3] mask_off, [4] n_exc, [5] nruns,
 *   [6..9] C of A,C,G,T, [10] CN, [11] has_n, [12] rot_first (31: none), [13] rotated copies present, [14] entries of
 *   xr_start / xr_cum.
 * slot = 0, 1, a PAM-pair table slot as `strand` holds it: [0] valid (the rest is 0 if not), [1] v_rem, [2] code, [3] rot_first
 *   (31: none), [4] rotated copies present, [5] slots of the row arrays, [6] deep, [7] deep_P, [8] deep_kb, [9] spaced, [10] sp_x,
 *   [11] sp_g, [12] sp_rem, [13] rows of the spaced table, [14] d = the key bits that address sp_off directly, [15] table depth k. */
gs_status gs_debug_index_layout(gs_index *ix, int slot, int strand, uint64_t out[32]);
/* One of these arrays, device to host: *total_bytes = its size by the layout above (0: the handle does not hold it), and its
 * bytes from offset_bytes on, cap_bytes at most, go to out.  A strand's (slot = -1): blocks, sa, ptab, ptab_rot, ctx, ctx16
 * (without the padding behind it), isa, exc_row, exc_sym, run_start, run_cum, xr_seg, xr_start, xr_cum, C256; a slot's: tab, rot,
 * c16 (with the 64 zero bytes behind it), ctx, rowid, deep, sp_off, sp_rows.  Any other name: GS_ERR_ARG.  Tests only; takes the
 * handle's lock, changes nothing, launches no kernel. */
gs_status gs_debug_index_array(gs_index *ix, int slot, int strand, const char *which, uint64_t offset_bytes, void *out,
                               uint64_t cap_bytes, uint64_t *total_bytes);
/* The workspace buffers (what handles and decoders grow on demand and keep from call to call, and what gs_bgzf_inflate
 * holds for one call) alive in the process: [0] allocations, [1] their bytes.  Tests only. */
gs_status gs_debug_buffers_live(uint64_t out[2]);
/* The handle's per-batch workspace, three words per group, n_groups = 7 groups in the order batch pipeline, device-wide
 * ordering, tile ordering, score, text, BGZF, annotation: buffers held, bytes held, and the bytes of those that an out-of-memory
 * recovery releases.  Tests only. */
gs_status gs_debug_workspace(gs_index *ix, uint64_t *out, uint32_t n_groups);
/* The rows under `key` (X symbols << 2 |R| | R symbols, both in consumption order) in the spaced table of a PAM-pair table
 * slot and strand, four words per row: {row in the table's row arrays, its O symbols, its row in the strand's suffix array,
 * its context word}; *n = rows under the key (out holds the first cap); info = {1 = the slot has spaced tables, pair code,
 * context depth, |X|, |R|, table depth k, key bits stored with a row, rows of the table}.  Tests only. */
gs_status gs_debug_spaced_rows(gs_index *ix, uint32_t slot, int strand, uint32_t key, uint32_t *out, uint64_t cap, uint64_t *n,
                               uint32_t info[8]);
/* What an item of the two seeding launches (gs_seed.hip) starts from: the 64-byte descriptor k_describe derives from a packed
 * guide record - q (2-bit codes in consumption order), four PAM patterns (3 bits per symbol, 4 = N) - for a batch shape
 * (table depth k, |X| = x_len, the PAM-pair codes of the table slots), as sixteen words: q lo, q hi, pam[4], meta, pidx0,
 * pidxg, qrem_b, bsel_z, bsel_w, qhot, key_a, key_b, guide (host only; tests/test_seed_descriptor.py pins every field). */
gs_status gs_debug_guide_descriptor(uint64_t q, const uint32_t pam[4], uint32_t npams, uint32_t valid, uint32_t L, uint32_t P,
                                    uint32_t k, uint32_t x_len, uint32_t n_pt, const uint32_t code[2], uint32_t out[16]);
/* The tile ordering's plan for one (guide, index) item of `records` match records, as data (host only; tests pin it):
 * out = {buckets the item is dealt into (0: the item is one tile), records a bucket's slot holds, sample words per
 * splitter, records one wave orders, buckets an item may have at most (more: the batch is ordered device-wide)}. */
void gs_debug_tile_plan(uint32_t records, uint32_t out[5]);
/* The search's form for a pass, as data (host only; tests/test_search_form.py pins the table).  in = {items (2 x guides),
 * CUs, share_min after the switches, the handle's back-off at the pass's start, main pass, walking kernel, one PAM chunk,
 * counting requests, every item through PAM-pair + deep tables, mismatches, the form estimate's two words (guides with a
 * heavy k-mer of their own, the largest such interval), heavy passes and items of the last batch of the same shape,
 * GS_HEAVY, GS_SPLIT_SHARE, GS_SPLIT_FROM, GS_SEED_FORM (-1: not set)}.  out = {the estimate is wanted, its threshold in
 * rows, heavy, split, seed form, the form gs_index_last_sharing reports: 0 plain, 1 heavy, 2 split, 3 two seeding
 * launches}. */
void gs_debug_search_form(const int64_t in[18], uint32_t out[6]);
/* The last gs_enumerate_general* / gs_enumerate_bulges call on the handle, as data (tests pin what the general path's
 * kernel met): out = {items (2 x guides), workgroups launched, records the first pass's pool held, match records T,
 * search passes run (1, or 2 when the pool was outgrown), then from the kernel, for the last pass: the largest number
 * of nodes any item's stack held after the pushes of a step, steps whose pop the room rule cut below min(nodes, 64)
 * lanes, steps that found no room for one lane's children (the pop is then one node)}.  A call that was refused
 * before its launch leaves the words as they were. */
gs_status gs_debug_general_last(const gs_index *ix, uint64_t out[8]);
/* The same call's routing between the two forms of the search, and what the seeded form's kernel met (tests pin them):
 * out = {guides sent to the seeded form, guides sent to the walk, seeds looked up in the strand tables (the depth-k nodes of
 * index.hpp:250-375's tree that the batch reached), seeds whose interval was empty, row nodes made, interval nodes made,
 * exception-row lookups, the largest number of nodes any item's stack held}; the kernel's words are those of the last pass. */
gs_status gs_debug_bulge_last(const gs_index *ix, uint64_t out[8]);
/* The seeds of one guide as data (host only, no device needed): the depth-k nodes of the bulge-aware recursion
 * (index.hpp:250-375, max_bulge_size = 1) with every base taken as present - each path stops where it has consumed k genome
 * symbols.  One entry per path, duplicates included, in no particular order: the index into the strand table (consumption
 * step t at bits 2(k-1-t)), the state word (t[5:0] mismatches[8:6] dna_bulges[11:9] rna_bulges[14:12] bulge state[16:15]
 * bulge size[17] sequence length[23:18]) and match.sequence so far.  guide: L symbols of A,C,G,T; flags:
 * GS_FLAG_PAM_AT_START.  prefix_len != 0 lists one sub-tree only: the paths whose first prefix_len consumed genome symbols are
 * `prefix` (2 bits each, the first consumed highest - the top bits of the index); at k = 14 a guide has millions of seeds.
 * *n = the seeds there are (out holds the first cap).  The function runs the transition function
 * the seeded kernel runs (gs_bulge_step.h). */
typedef struct gs_bulge_seed {
  uint32_t index, state;
  uint8_t seq[32];
} gs_bulge_seed;
gs_status gs_debug_bulge_seeds(const char *guide, uint32_t L, uint32_t k, uint32_t mismatches, uint32_t rna_bulges,
                               uint32_t dna_bulges, uint32_t flags, uint32_t prefix_len, uint32_t prefix, gs_bulge_seed *out,
                               uint64_t cap, uint64_t *n);
/* The matches one seed reaches in one row, as data (host only): the rest of the same recursion, and the PAM stage
 * (index.hpp:297-314 -> :125-170, alt PAMs first as process.hpp:51-56), run from a seed's state and sequence against the
 * row's 16-symbol left context given as nibbles, nearest first: 0..3 A,C,G,T, 4 'N', 5 any other symbol, 6 before the
 * text start.  One entry per path, duplicates included: the final state word, match.sequence, and the context symbols the
 * match consumed (it begins that many symbols before the row's suffix).  Patterns over A,C,G,T,N; alt_pams: the n_alt
 * patterns back to back, alt_lens[j] symbols each. */
typedef struct gs_bulge_match {
  uint32_t state, consumed;
  uint8_t seq[32];
} gs_bulge_match;
gs_status gs_debug_bulge_verify(uint32_t state, const uint8_t seq[32], uint64_t ctx_nibbles, const char *guide, uint32_t L,
                                const char *guide_pam, uint32_t P, const char *alt_pams, const uint32_t *alt_lens,
                                uint32_t n_alt, uint32_t k, uint32_t mismatches, uint32_t rna_bulges, uint32_t dna_bulges,
                                uint32_t flags, gs_bulge_match *out, uint64_t cap, uint64_t *n);

/* Self-check of a resident index from the genome text alone (no suffix-array builder involved):
 * the suffix array of `strand` is a permutation of [0, n) (all rows), n_samples evenly spread
 * adjacent row pairs are in suffix order by direct comparison of the text, and the BWT symbol
 * each sampled row's Occ block holds is text[SA[row]-1].  `text` = the forward genome text as given
 * to gs_index_build.  Stands where the reference relies on sdsl::construct being right
 * (sdsl/include/sdsl/construct.hpp:121-166); used by the parity tests at n > 2^31.
 * What sampled mode leaves out: sample i looks at the pair (r, r+1) and at row r's BWT symbol for one r in
 * [i*stride, (i+1)*stride), stride = (n-1) / n_samples rounded down - so the BWT symbol of row n-1 is never
 * looked at, and with n_samples < n-1 neither are the trailing (n-1) mod n_samples pairs, which lie beyond the
 * last sample's stride.  n_samples >= n-1 compares every pair once (row n-1's symbol still left out); only
 * GS_VERIFY_ALL_ROWS below looks at every row.  The runs of 'N' that the comparison skips are those of the
 * text the index was built from.  tests/sa_model.py restates both modes in numpy; the reports are held equal to it. */
typedef struct {
  uint64_t rows;            /* n = text length + 1 */
  uint64_t not_permutation; /* rows whose value is out of range or was seen before */
  uint64_t sampled;         /* adjacent pairs compared */
  uint64_t out_of_order;    /* pairs with suffix(SA[r]) >= suffix(SA[r+1]) */
  uint64_t undecided;       /* pairs still equal after 65536 comparison steps (N runs are skipped) */
  uint64_t bwt_mismatch;    /* sampled rows whose block symbol differs from the text */
} gs_sa_report;
gs_status gs_index_verify_sa(gs_index *ix, int strand, const uint8_t *text, uint64_t len,
                             uint64_t n_samples, uint64_t seed, gs_sa_report *report);
/* n_samples = GS_VERIFY_ALL_ROWS: EVERY adjacent pair of rows, by the linear-time rule - text[SA[r]] < text[SA[r+1]], or equal
 * symbols and ISA[SA[r]+1] < ISA[SA[r+1]+1] - with ISA checked to be SA's inverse (counted in not_permutation) and the BWT
 * symbol of every row compared with the text: a complete proof that the resident array is the suffix array of `text`
 * (what csa_wt::operator[] presumes, sdsl/include/sdsl/csa_wt.hpp:333-346), one streaming pass (0.4 s per strand at hg38
 * size); `undecided` is 0 by construction.  Needs the inverse suffix array (GS_ERR_UNSUPPORTED on an index built without). */
#define GS_VERIFY_ALL_ROWS (~0ull)

/* ---- text encoders: the step right after the path (host side) ---------------------------- */

typedef struct {
  const char *const *chr_names; /* genome_structure, include/genomics/structures.hpp:45 */
  const uint64_t *chr_lengths;
  uint32_t n_chr;
} gs_genome_structure;

typedef struct { /* the kmer fields the printers use, include/genomics/structures.hpp:10-17 */
  const char *id;
  const char *sequence;
  const char *pam;
  int sense_positive; /* kmers file `sense` column == "+" */
} gs_kmer;

#define GS_TEXT_SAM 0x100u      /* --format sam (default csv) */
#define GS_TEXT_COMPLETE 0x200u /* --mode complete */
/* gs_format_device / gs_enumerate_text only.  GS_TEXT_BAM: the SAM lines as uncompressed BAM alignment blocks, no header
 * block - what `samtools view -b` (manual/manual.tex:581-582) stores for the lines of printer.hpp:302-360; not together
 * with GS_TEXT_SAM.  GS_TEXT_BGZF (only with GS_TEXT_BAM): those blocks as BGZF members (gs_bgzf_compress_device). */
#define GS_TEXT_BAM 0x800u
#define GS_TEXT_BGZF 0x1000u

/* The database lines of one guide from its hit list (as returned by gs_enumerate, canonical
 * order).  Byte-exact replacement of get_csv_lines / get_sam_lines
 * (include/genomics/printer.hpp:245-300, 302-360) including resolve_absolute
 * (src/genomics/structures.cxx:7-52), CFD and specificity.  `mismatches` and
 * GS_FLAG_PAM_AT_START as passed to gs_enumerate; max_off_targets = -1 for none.
 * *out_text is malloc'ed (NUL terminated); release with gs_free. */
gs_status gs_format_guide(const gs_genome_structure *gs, const gs_kmer *k, const gs_hit *hits,
                          uint64_t n_hits, uint32_t mismatches, uint32_t flags,
                          int64_t max_off_targets, char **out_text, size_t *out_len);
/* Same lines with the guide's specificity supplied by the caller - the float gs_score /
 * gs_score_device computed on the device for the same hits, flags and max_off_targets - so the
 * host formats text only (no CFD arithmetic per hit).  What the C++ host (`guidescan enumerate`)
 * calls. */
gs_status gs_format_guide_scored(const gs_genome_structure *gs, const gs_kmer *k, const gs_hit *hits,
                                 uint64_t n_hits, uint32_t mismatches, uint32_t flags,
                                 int64_t max_off_targets, float specificity, char **out_text,
                                 size_t *out_len);
/* The lines of guides [0, n) of one enumerate result in ONE buffer (same bytes as
 * gs_format_guide_scored guide after guide; rows of guides with skip[g] != 0 left out): what a
 * writer thread calls per contiguous range of a batch.  offsets: n+1 positions into `hits`. */
gs_status gs_format_guides_scored(const gs_genome_structure *gs, const gs_kmer *kmers, uint64_t n,
                                  const uint64_t *offsets, const gs_hit *hits, const float *specificity,
                                  const uint8_t *skip, uint32_t mismatches, uint32_t flags,
                                  int64_t max_off_targets, char **out_text, size_t *out_len);
/* write_sam_header / write_csv_header (include/genomics/printer.hpp:173-187) */
gs_status gs_format_header(const gs_genome_structure *gs, uint32_t flags, char **out_text,
                           size_t *out_len);
void gs_free(void *p);

/* ---- the general path: bulges, symbols outside A,C,G,T, any number of PAMs ---------------------- */

/* One hit of the general path, 48 bytes.  match.sequence can hold '.', lower-case bulge bases, any
 * literal symbol of the guide or of a PAM pattern, and has no fixed length, so it travels as its
 * bytes (byte order == the reference's std::set<match> order). */
typedef struct {
  int64_t pos;
  char seq[32];      /* match.sequence, seq_len bytes, NUL padded */
  uint32_t mismatches;
  uint8_t dna_bulges, rna_bulges;
  uint8_t index;   /* 0 forward index, 1 reverse index */
  uint8_t seq_len;
} gs_hit_ex;

typedef struct gs_result_ex gs_result_ex;

/* Everything genome_index::inexact_search accepts, exactly: replaces both branches of the dispatcher
 * (index.hpp:377-398) - the bulge-aware recursion (:250-375, max_bulge_size = 1 as process.hpp:82-83
 * calls it) when rna_bulges/dna_bulges > 0, else the PAM-aware recursion (:182-248) - for inputs the
 * fast path does not encode: guide symbols outside A,C,G,T (matched literally, else charged a
 * mismatch, :218-247), PAM symbols other than 'N' as literals (:125-170), up to 31 alt PAMs
 * (process.hpp:51-56).  Same set ordering and resolve() expansion; hits per guide in canonical order.
 * A slow path (one node per lane, comparator sort): gs_enumerate reports which guides need it.
 * Two forms of the search, the same result byte for byte.  The walk (the default) descends from the root with two Occ-block
 * reads per node.  The seeded form (the handle's switch GS_BULGE_FORM=1) takes every path's first k = table depth genome
 * symbols without reading anything, looks the k-mer up in the strand's interval table, and resolves a seed of at most
 * GS_BULGE_ROWS rows (default 8; 0: never) row by row against the 16-symbol left context the index keeps per row; a
 * larger seed is walked on.  It serves the guides over A,C,G,T of a batch whose patterns are over A,C,G,T,N, with
 * L - rna_bulges >= k and L + dna_bulges + (longest pattern) - k <= 16; every other guide of the call walks.
 * gs_debug_bulge_last reports the routing. */
gs_status gs_enumerate_general(gs_index *ix, const char *guides, uint64_t n, uint32_t L,
                               const char *guide_pams, uint32_t P, const char *alt_pams, uint32_t n_alt,
                               uint32_t mismatches, uint32_t rna_bulges, uint32_t dna_bulges,
                               uint32_t flags, gs_result_ex **out);
/* The same with alt PAMs of their own lengths: the reference searches every pattern of `-a` next to the
 * guides' PAM whatever its length (process.hpp:51-56 -> index.hpp:182-216: the PAM stage of a pattern ends
 * after its own symbols), so a hit's match.sequence has L + that pattern's length symbols.  alt_pams: the
 * n_alt patterns back to back, alt_lens[j] symbols each (1..8). */
gs_status gs_enumerate_general_pams(gs_index *ix, const char *guides, uint64_t n, uint32_t L,
                                    const char *guide_pams, uint32_t P, const char *alt_pams,
                                    const uint32_t *alt_lens, uint32_t n_alt, uint32_t mismatches,
                                    uint32_t rna_bulges, uint32_t dna_bulges, uint32_t flags, gs_result_ex **out);
/* the same function under the name the bulge options were first served by */
gs_status gs_enumerate_bulges(gs_index *ix, const char *guides, uint64_t n, uint32_t L,
                              const char *guide_pams, uint32_t P, const char *alt_pams, uint32_t n_alt,
                              uint32_t mismatches, uint32_t rna_bulges, uint32_t dna_bulges,
                              uint32_t flags, gs_result_ex **out);
gs_status gs_result_ex_get(const gs_result_ex *r, uint64_t *n_guides, const uint64_t **guide_offsets,
                           const gs_hit_ex **hits);
/* per guide: hits before duplicate sequences are dropped (what --threshold compares, process.hpp:25-27) */
gs_status gs_result_ex_raw_hits(const gs_result_ex *r, const uint32_t **raw_hits);
void gs_result_ex_free(gs_result_ex *r);
/* match.sequence of a general-path hit as a C string; out needs 33 bytes */
gs_status gs_decode_sequence_ex(const gs_hit_ex *hit, char *out);
/* gs_format_guide for general-path hits (rna_bulges / dna_bulges columns filled in) */
gs_status gs_format_guide_ex(const gs_genome_structure *gs, const gs_kmer *k, const gs_hit_ex *hits,
                             uint64_t n_hits, uint32_t mismatches, uint32_t flags,
                             int64_t max_off_targets, char **out_text, size_t *out_len);

/* CFD score of one hit (include/genomics/printer.hpp:98-113), float semantics preserved. */
float gs_calculate_cfd(const char *sgrna, const char *match_sequence, const char *pam);

/* ---- scoring on the device ---------------------------------- */

/* CFD of every hit and specificity of every guide of an enumerate result, computed in HBM.
 * Replaces calculate_cfd (printer.hpp:98-113) and the aggregation loops of get_csv_lines
 * (printer.hpp:251-297; flags without GS_TEXT_SAM) or off_target_fields (printer.hpp:115-170;
 * GS_TEXT_SAM): float sum of the CFDs in canonical hit order, hits dropped by resolve_absolute
 * (structures.cxx:46-48) left out, --max-off-targets applied per distance exactly as each loop
 * does, `+1` unless a perfect hit with an xGG PAM exists, specificity = 1/sum.  Bit-identical
 * to gs_calculate_cfd / gs_format_guide.
 *   d_guides  : n*L ASCII bytes as passed to gs_enumerate_device
 *   d_offsets, d_hits : what gs_enumerate_device returned (or any CSR hit list in that layout)
 *   flags     : GS_FLAG_PAM_AT_START as passed to gs_enumerate, GS_TEXT_SAM selects the SAM rule
 *   d_cfd     : float[n_hits] or NULL;  d_specificity : float[n] */
gs_status gs_score_device(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L, uint32_t P,
                          uint32_t flags, int64_t max_off_targets, const gs_genome_structure *gs,
                          const void *d_offsets, const void *d_hits, void *stream, void *d_cfd,
                          void *d_specificity);
/* Same with host arrays in and out (copies inside). */
gs_status gs_score(gs_index *ix, const char *guides, uint64_t n, uint32_t L, uint32_t P, uint32_t flags,
                   int64_t max_off_targets, const gs_genome_structure *gs, const uint64_t *offsets,
                   const gs_hit *hits, float *cfd, float *specificity);

/* ---- the database text on the device (at scale) ----------------------- */

/* The lines of guides [0, n) of a fast-path batch, encoded in HBM: the same bytes as gs_format_guides_scored, i.e.
 * get_csv_lines / get_sam_lines (include/genomics/printer.hpp:181-300, 115-170 and 302-360) with resolve_absolute
 * (src/genomics/structures.cxx:7-52), the `NA` row of a guide without hits (:189-199), --max-off-targets as each
 * printer applies it (:259 raw index, :129 kept hits) and the specificity printed as std::to_string(float).
 *   d_guides, d_guide_pams : n*L and n*P ASCII bytes in HBM, as passed to gs_enumerate_device
 *   ids, id_offsets        : host; the guides' ids back to back and n+1 offsets into them
 *   senses, skip           : host, n bytes each, either may be NULL: senses[g] != 0 = the kmers file's sense "+"
 *                            (NULL: all "+"); skip[g] != 0 leaves the guide's lines out (NULL: none)
 *   d_offsets, d_hits      : what gs_enumerate_device returned, or any CSR hit list in that layout (d_offsets[0] need
 *                            not be 0: hits are indexed by the offsets' values)
 *   d_specificity          : float[n] of gs_score_device for the same flags and max_off_targets
 *   flags                  : GS_FLAG_PAM_AT_START | GS_TEXT_SAM | GS_TEXT_COMPLETE, or GS_TEXT_BAM [| GS_TEXT_BGZF] in
 *                            place of GS_TEXT_SAM: one BAM alignment block per SAM line, byte for byte the block
 *                            `guidescan sam2bam` makes of that line (refID -1, pos -1, bin 4680 for the reference's
 *                            empty RNAME; MAPQ 100; one CIGAR op; quality 0xFF; k0..km as C, S or I; of:H in
 *                            complete mode; sp:f the float nearest to the six printed decimals), d_specificity under
 *                            the SAM rule; with GS_TEXT_BGZF *d_text holds the blocks' BGZF members instead.  An id of
 *                            more than 254 bytes is GS_ERR_ARG; so are GS_TEXT_BAM with GS_TEXT_SAM, and GS_TEXT_BGZF
 *                            without GS_TEXT_BAM.  gs_index_last_text_offsets gives the guides' places in the blocks.
 * *d_text (device memory owned by the handle, valid until the next call on it) holds *text_len bytes, no terminator.
 * GS_ERR_ARG, reported by the device together with the length: a specificity outside [0, 1] (gs_score_device never
 * produces one), a hit whose distance exceeds `mismatches`, a key that does not decode. */
gs_status gs_format_device(gs_index *ix, const gs_genome_structure *gs, const void *d_guides, uint64_t n, uint32_t L,
                           const void *d_guide_pams, uint32_t P, const char *ids, const uint64_t *id_offsets,
                           const uint8_t *senses, const uint8_t *skip, const void *d_offsets, const void *d_hits,
                           const void *d_specificity, uint32_t mismatches, uint32_t flags, int64_t max_off_targets,
                           void *stream, const void **d_text, uint64_t *text_len);
/* gs_format_device with ids that are in HBM already (gs_kmers_get_ids): d_ids, d_id_offsets (n + 1 uint64 that index d_ids
 * as they stand: d_id_offsets[0] need not be 0) and d_senses (n bytes, != 0 = "+", or NULL) are device pointers; `skip`
 * stays a host array.  The same bytes as gs_format_device on the same inputs; offsets that descend are reported by the
 * device as GS_ERR_ARG. */
gs_status gs_format_device_ids(gs_index *ix, const gs_genome_structure *gs, const void *d_guides, uint64_t n, uint32_t L,
                               const void *d_guide_pams, uint32_t P, const void *d_ids, const void *d_id_offsets,
                               const void *d_senses, const uint8_t *skip, const void *d_offsets, const void *d_hits,
                               const void *d_specificity, uint32_t mismatches, uint32_t flags, int64_t max_off_targets,
                               void *stream, const void **d_text, uint64_t *text_len);
/* Where each guide's lines begin in the text of the last gs_format_device / gs_enumerate_text on this handle: out[g] for
 * g in [0, n], out[n] = the text's length; n as passed to that call (else GS_ERR_ARG, as after any other call on the handle
 * that runs a batch).  Made on the device from the row lengths, with the text.  Stands where the reference's writer has
 * the lines guide by guide anyway (include/genomics/process.hpp:117-158): a host that cuts the text at guide boundaries -
 * `guidescan enumerate --format bam` compresses ranges of guides in parallel - needs no parsing. */
gs_status gs_index_last_text_offsets(gs_index *ix, uint64_t *out, uint64_t n);
/* Guides in, database text out: gs_enumerate_device -> gs_score_device -> gs_format_device inside the library, the text
 * copied back through page-locked staging.  Replaces, for a batch, the per-guide pipeline from the search to the
 * output lines (include/genomics/process.hpp:35-158 with printer.hpp:115-360).  Host pointers in; *text is malloc'ed
 * (NUL terminated, *len bytes before the terminator): release with gs_free.  flags: those of gs_enumerate plus
 * GS_TEXT_SAM / GS_TEXT_COMPLETE, or GS_TEXT_BAM [| GS_TEXT_BGZF] as gs_format_device takes them: *text then holds the
 * batch's BAM alignment blocks, or their BGZF members - search, scoring, records and compressor all inside the library, the
 * step of manual/manual.tex:581-582 over the lines of printer.hpp:302-360.  GS_ERR_UNSUPPORTED and no text when a guide of the batch carries
 * GS_GUIDE_NEEDS_GENERAL: the caller takes gs_enumerate + gs_enumerate_general + the host encoders for that batch.
 * stats (or NULL): the search's counters and timings; its pointers are NULL. */
gs_status gs_enumerate_text(gs_index *ix, const char *guides, uint64_t n, uint32_t L, const char *guide_pams, uint32_t P,
                            const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                            int64_t max_off_targets, const gs_genome_structure *gs, const char *ids,
                            const uint64_t *id_offsets, const uint8_t *senses, const uint8_t *skip, char **text,
                            uint64_t *len, gs_result_view *stats);

/* gs_enumerate_text over guides, ids and senses that are in HBM already (a gs_kmers object's arrays, or a range of them):
 * gs_enumerate_device -> gs_score_device -> gs_format_device_ids; only the text - and `skip`, a host array or NULL -
 * crosses the bus.  GS_ERR_UNSUPPORTED and no text when a guide carries GS_GUIDE_NEEDS_GENERAL or the shape is outside
 * the fast path's key (2L + 3P > 59).
 * With GS_FLAG_RAW_COUNTS in flags the call is the counting pass of --threshold (process.hpp:66-76) instead: the search
 * alone at `mismatches`, its raw hit counts copied to raw_hits (host, n entries, required); no text is made, `text`,
 * `len`, the ids and senses may be NULL.  Without the flag raw_hits must be NULL. */
gs_status gs_enumerate_text_device(gs_index *ix, const void *d_guides, uint64_t n, uint32_t L, const void *d_guide_pams,
                                   uint32_t P, const char *alt_pams, uint32_t n_alt, uint32_t mismatches, uint32_t flags,
                                   int64_t max_off_targets, const gs_genome_structure *gs, const void *d_ids,
                                   const void *d_id_offsets, const void *d_senses, const uint8_t *skip, char **text,
                                   uint64_t *len, gs_result_view *stats, uint32_t *raw_hits);

/* ---- BGZF on the device: the compression step of a BAM database ---------------------------------- */

/* raw_len bytes in HBM -> BGZF members in HBM, back to back, no end-of-file block.  The reference writes SAM text only
 * (include/genomics/printer.hpp:302-360) and its manual sends the user to `samtools view -b` for the BAM database
 * (manual/manual.tex:581-582): this is that step's compressor, for bytes that are on the device already.
 * `raw` is cut every 0xff00 bytes from its start (the last piece may be shorter; raw_len == 0 gives *out_len == 0).  Each
 * piece becomes one gzip member: the 18-byte header 1f 8b 08 04 00000000 00 ff 0600 'B' 'C' 0200 BSIZE, one deflate
 * block, the CRC-32 of the piece and ISIZE.  The block holds LZ77 matches (window 32,768, lengths 3..258) in dynamic
 * Huffman codes; its header gives the code-length code's symbols 0..15 four bits each and writes every length without
 * the repeat symbols.  A piece whose dynamic block would not be smaller is one stored block, so a member is never more
 * than its piece + 31 bytes.  The bytes are a function of `raw` alone: the same on every call, and member k is what
 * piece k gives by itself.  The handle lends its workspace and its lock; the index is not read.  *d_out belongs to the
 * handle until its next gs_bgzf_compress* call; it is not the buffer gs_format_device returns. */
gs_status gs_bgzf_compress_device(gs_index *ix, const void *d_raw, uint64_t raw_len, void *stream, const void **d_out,
                                  uint64_t *out_len);
/* The same with host pointers (manual/manual.tex:581-582, printer.hpp:302-360 as above); *out is malloc'ed: release
 * with gs_free. */
gs_status gs_bgzf_compress(gs_index *ix, const void *raw, uint64_t raw_len, uint8_t **out, uint64_t *out_len);
/* Host only: the code lengths the compressor gives n (<= 288) symbols with counts freq[i] (< 2^23), none above max_len
 * (<= 15): the function its kernel runs between the match search and the bit writer.  A complete code (Kraft sum 1)
 * over the symbols with a count; one such symbol gets length 1, none gives all zeros.  GS_ERR_ARG when the symbols with
 * a count do not fit max_len bits. */
gs_status gs_debug_huffman_lengths(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len);
/* Host only: the float nearest to q / 10^6 (ties to even) for a specificity printed as the integer q of its six
 * decimals, 0 <= q <= 10^6 (larger: 1.0): what the sp:f tag of a BAM record made from the SAM line of
 * printer.hpp:302-360 stores (manual/manual.tex:581-582). */
float gs_debug_sp_float(uint32_t q);

/* ---- candidate-guide generation on the device ------------------- */

typedef struct gs_kmers gs_kmers;

/* Every PAM site of ONE chromosome (one FASTA record, any case) in the reference script's order.
 * Replaces find_all_kmers / find_kmers (scripts/generate_kmers.py:70-118): + strand sites per
 * concrete PAM expansion ('N' -> A,C,T,G), then - strand sites per reverse-complemented
 * expansion, each in position order; protospacers with non-ACGT symbols or cut by the record's
 * ends dropped.  `chr` is a host pointer, or a device pointer when chr_on_device != 0.
 * flags: GS_FLAG_PAM_AT_START (--start). */
gs_status gs_kmers_generate(int device, const uint8_t *chr, uint64_t chr_len, int chr_on_device,
                            const char *pam, uint32_t k, uint32_t flags, void *stream, gs_kmers **out);
/* n records: seqs n*k ASCII, pams n*P ASCII (the pattern), positions uint32 (1-based protospacer
 * or PAM start as the script prints it), senses '+'/'-'.  on_device != 0: pointers into HBM, in
 * the layout gs_enumerate_device takes; else host copies owned by the object. */
gs_status gs_kmers_get(gs_kmers *km, int on_device, uint64_t *n, const void **seqs, const void **pams,
                       const void **positions, const void **senses);
/* The records' ids "{prefix}{chr_name}:{position}:{sense}" (scripts/generate_kmers.py:120-125) encoded in HBM and kept
 * in the object: the bytes back to back, n + 1 uint64 offsets from 0, and the senses as 0 / 1 (1 = "+"), the three
 * arrays gs_format_device_ids / gs_enumerate_text_device take.  A second call replaces them. */
gs_status gs_kmers_encode_ids(gs_kmers *km, const char *prefix, const char *chr_name, void *stream);
/* on_device as in gs_kmers_get; GS_ERR_ARG before gs_kmers_encode_ids */
gs_status gs_kmers_get_ids(gs_kmers *km, int on_device, const void **ids, const void **id_offsets,
                           const void **sense_positive);
/* The records as rows of the kmers file, `id,sequence,pam,chromosome,position,sense\n` (the same lines of the script,
 * `pam` = the pattern): rows only, no header, encoded in HBM and copied back through page-locked staging.  *text is
 * malloc'ed (NUL terminated, *len bytes before the terminator): release with gs_free. */
gs_status gs_kmers_csv(gs_kmers *km, const char *prefix, const char *chr_name, char **text, uint64_t *len);
/* One object holding the records of parts[0], parts[1], ... in that order (same device, k and P), in HBM; ids too when
 * every part has them.  The parts stay valid and are still the caller's to free. */
gs_status gs_kmers_concat(gs_kmers *const *parts, uint32_t n_parts, gs_kmers **out);
void gs_kmers_free(gs_kmers *km);

/* ---- the kmers file read on the device: the guides of `enumerate -f` (src/genomics/kmer.cxx:9-25) ------------- */

/* What a parse found.  bad_kind != 0: the call returned GS_ERR_FORMAT, made no object, and gs_status_string(GS_ERR_FORMAT)
 * reads as cli::read_kmers' message. */
#define GS_KMERS_BAD_FEW 1u      /* "kmers row with too few columns: LINE": bad_text is the line, its '\r' dropped */
#define GS_KMERS_BAD_POSITION 2u /* "kmers position is not an integer: FIELD": bad_text is the trimmed field */
#define GS_KMERS_BAD_EMPTY 3u    /* "empty kmers file" */
#define GS_KMERS_BAD_LACKS 4u    /* "kmers file lacks column NAME": bad_text is NAME */
typedef struct gs_kmers_report {
  uint64_t n, L, P;  /* rows, and the symbols of every row's sequence and PAM */
  uint64_t n_lines;  /* lines of the file, the header and the skipped ones included */
  uint32_t bad_kind, pad;
  /* the first failing row in file order: its line (0 = the header) and its number among the rows, from 0; where bad_text
   * stands in the file and its bytes.  Only these bytes are copied back from the device. */
  uint64_t bad_line, bad_row, bad_off, bad_len;
  char *bad_text;    /* malloc'ed, NUL terminated behind bad_len bytes: release with gs_free.  NULL when bad_kind is 0 */
  /* milliseconds.  Host clocks: the file's reads, waits for its uploads, the device stage (allocations, passes, waits for
   * their results).  Then by events in the stream: tile summaries with their scan, line starts, the line walk, the scan
   * of the rows and id lengths, the emit. */
  double ms[8];
} gs_kmers_report;

/* The rows of a kmers file (src/genomics/kmer.cxx:9-25, under the rules of cli::read_kmers: gs_kmers_scan.h states them)
 * as a gs_kmers object, parsed in HBM: sequences n*L, PAMs n*P, the ids back to back with n + 1 offsets and the senses
 * as 0 / 1, bytes as they stand in the file.  raw: host memory, uploaded whole.  rep may be NULL.
 * GS_ERR_FORMAT: the file fails as it fails on the host (rep->bad_*).  GS_ERR_UNSUPPORTED, no object: rows of several
 * shapes, or a first row without a sequence - read the file on the host.  L > 31 or 2L + 3P > 59 still gives an object.
 * On the object gs_kmers_get gives NULL for the positions and '+' / '-' for the senses; gs_kmers_get_ids, gs_kmers_concat
 * (with other parsed objects) and the host copies work as for scanned ones; gs_kmers_encode_ids and gs_kmers_csv are
 * GS_ERR_ARG.  Device memory at the peak: the raw bytes, the outputs, and 40 bytes per line plus 48 per 4,096 bytes for
 * the passes; the raw bytes and the passes' arrays are freed before the call returns.  Out of it: GS_ERR_NOMEM, nothing
 * stays allocated. */
gs_status gs_kmers_parse(int device, const uint8_t *raw, uint64_t len, gs_kmers **out, gs_kmers_report *rep);
/* The same (src/genomics/kmer.cxx:9-25 opens the file by name too) from a regular file, read in chunks into two
 * page-locked buffers: a chunk is uploaded while the next is read.  GS_ERR_IO when it cannot be read or is no regular file. */
gs_status gs_kmers_parse_file(int device, const char *path, gs_kmers **out, gs_kmers_report *rep);
/* The same (src/genomics/kmer.cxx:9-25) with the raw bytes in HBM already, at any alignment; the kernels run on `stream`,
 * the call returns when they are done.  d_raw is only read and stays the caller's. */
gs_status gs_kmers_parse_device(int device, const void *d_raw, uint64_t len, void *stream, gs_kmers **out, gs_kmers_report *rep);
/* the bytes of a tile of the device passes of gs_kmers_parse* (src/genomics/kmer.cxx:9-25) */
uint64_t gs_debug_kmers_tile_bytes(void);
/* the bytes of a staging chunk of gs_kmers_parse_file (src/genomics/kmer.cxx:9-25 from a file; 32 MB); set != 0 replaces it, for every later call of the process */
uint64_t gs_debug_kmers_chunk_bytes(uint64_t set);
/* Host only: the passes of the device reader (src/genomics/kmer.cxx:9-25 through gs_kmers_scan.h), run one after the other
 * with tiles of `tile_bytes` and windows of min(tile_bytes, 16) bytes: the same arrays and report.  The object has no
 * device side: gs_kmers_get / gs_kmers_get_ids with on_device != 0 are GS_ERR_ARG. */
gs_status gs_debug_kmers_host(const uint8_t *raw, uint64_t len, uint64_t tile_bytes, gs_kmers **out, gs_kmers_report *rep);

/* ---- guides for regions: candidates restricted to the intervals of a BED file, ranked within groups of them ---- */
/* The reference has no counterpart for anything in this section: the pipelines of its manual (manual/manual.tex:321-656)
 * filter the genome-wide table by coordinate and specificity in scripts.  The rules, stated once (gs_regions_scan.h):
 * a candidate printed at 1-based `position` occupies the forward-strand bases [position - 1, position - 1 + k + P) for both
 * senses, with and without --start (scripts/generate_kmers.py:70-100), and belongs to a group iff that footprint lies inside
 * one of the group's intervals on its chromosome, the group's intervals merged first where they overlap or abut.  A
 * candidate inside intervals of several groups gives one record per group.  A record's id is
 * "{prefix}{group}:{chr}:{position}:{sense}".  Records are ordered by group number, then (with per_region: specificity
 * descending first) by chromosome in structure order, position, sense with '+' first. */

typedef struct gs_regions gs_regions;
typedef struct gs_design gs_design;

#define GS_REGIONS_BAD_FEW 1u        /* fewer than three fields */
#define GS_REGIONS_BAD_INTEGER 2u    /* a start or end that is not a non-negative integer (digits only, at most 18) */
#define GS_REGIONS_BAD_ORDER 3u      /* start >= end */
#define GS_REGIONS_BAD_CHROMOSOME 4u /* a chromosome the structure does not have */
#define GS_REGIONS_BAD_BEYOND 5u     /* end beyond the chromosome's length */
#define GS_REGIONS_BAD_COMMA 6u      /* a group name with ',': it would break the CSV id column */
#define GS_REGIONS_BAD_LONG 7u       /* a group name with which an id could pass 254 bytes, the BAM encoder's cap */
#define GS_REGIONS_BAD_EMPTY 8u      /* no interval in the file (bad_line 0) */
typedef struct gs_regions_report { /* in the shape of gs_kmers_report */
  uint64_t n_lines;     /* lines of the file, the skipped ones included */
  uint64_t n_intervals; /* after merging */
  uint64_t n_groups;
  uint32_t bad_kind, pad;
  uint64_t bad_line; /* 1-based, of the first failing line */
  uint64_t bad_len;
  char *bad_text; /* the message, "regions line N: REASON"; malloc'ed, NUL terminated: release with gs_free.  NULL when bad_kind is 0 */
} gs_regions_report;

/* A BED file (no counterpart in the reference) against a genome structure, on the host: a file of every human exon is a
 * few megabytes.  Fields are separated by tabs or blanks; lines that are empty or start with '#', "track" or "browser" are
 * skipped; a trailing '\r' is dropped.  Columns 1-3: chromosome, start, end, 0-based and half-open.  Column 4, if present,
 * names the line's group, otherwise the group is "{chr}:{start}-{end}"; groups are numbered by first appearance and may lie
 * on several chromosomes.  `prefix` (or NULL) is the id prefix the length cap is checked with, against the longest
 * chromosome name and ten position digits.  GS_ERR_FORMAT: rep->bad_* say which line and why, and
 * gs_status_string(GS_ERR_FORMAT) reads as that message.  The object keeps, per chromosome, the merged intervals of all
 * groups sorted by start with the running maximum of their ends, ready to upload. */
gs_status gs_regions_parse(const uint8_t *raw, uint64_t len, const gs_genome_structure *gs, const char *prefix, gs_regions **out,
                           gs_regions_report *rep);
/* the same (no counterpart in the reference) from a file; GS_ERR_IO when it cannot be read */
gs_status gs_regions_parse_file(const char *path, const gs_genome_structure *gs, const char *prefix, gs_regions **out,
                                gs_regions_report *rep);
gs_status gs_regions_info(const gs_regions *regions, uint64_t *n_groups, uint64_t *n_intervals);
void gs_regions_free(gs_regions *regions);

/* The records of one chromosome's scan (gs_kmers_generate on chromosome chr_index of the structure) that lie in a group,
 * made in HBM (no counterpart in the reference): a count per candidate, a scan, and one record per (candidate, group)
 * holding sequence, PAM, position, sense, group and chromosome.  `regions` must outlive every design made from it. */
gs_status gs_design_restrict(const gs_regions *regions, uint32_t chr_index, gs_kmers *scan, void *stream, gs_design **part);
/* one design holding the records of parts[0], parts[1], ... (same device, regions, k and P); the parts stay the caller's */
gs_status gs_design_concat(gs_design *const *parts, uint32_t n_parts, gs_design **out);
/* The specificity of every record, in the design's float[n] in HBM (no counterpart in the reference): the records go in
 * batches of `batch` (0: 2^17) through gs_enumerate_device and gs_score_device under the CSV rule with max_off_targets
 * = -1, whatever the database is written as.  flags: GS_FLAG_PAM_AT_START, GS_FLAG_NO_NEW_TABLES.  threshold >= 0: the
 * counting pass of --threshold (GS_FLAG_RAW_COUNTS, process.hpp:66-76) runs too, its raw counts read in HBM where the
 * search leaves them, and a record it would drop is not eligible for selection.  GS_ERR_UNSUPPORTED where the fast path's key does not fit (2L + 3P > 59) or a record needs
 * the general path. */
gs_status gs_design_score(gs_index *ix, gs_design *design, const char *alt_pams, uint32_t n_alt, uint32_t mismatches,
                          uint32_t flags, int64_t threshold, uint64_t batch, void *stream);
/* The records in order, as a gs_kmers object in HBM with their ids (no counterpart in the reference).  per_region N > 0
 * keeps the first N eligible records of each group with specificity >= min_specificity; min_specificity < 0: no bound;
 * both need gs_design_score first (GS_ERR_ARG).  With neither, every eligible record is ordered and emitted.  The object
 * has ids from the start: gs_kmers_encode_ids on it is GS_ERR_ARG; gs_kmers_get, gs_kmers_get_ids and gs_kmers_concat
 * work as on a scan's. */
gs_status gs_design_select(gs_design *design, const char *prefix, uint32_t per_region, float min_specificity, void *stream,
                           gs_kmers **out);
/* the same selection as rows of the kmers file, `id,sequence,pam,chromosome,position,sense\n` (scripts/generate_kmers.py:120-125
 * with the group in the id), no header; *text is malloc'ed (NUL terminated): release with gs_free */
gs_status gs_design_rows(gs_design *design, const char *prefix, uint32_t per_region, float min_specificity, void *stream,
                         char **text, uint64_t *len);
/* host copies of the records' arrays, owned by the design: groups, chromosomes, positions uint32; senses '+' / '-';
 * specificity float; eligible bytes.  Any pointer may be NULL. */
gs_status gs_design_get(gs_design *design, uint64_t *n, const void **groups, const void **chromosomes, const void **positions,
                        const void **senses, const void **specificity, const void **eligible);
/* the number of records and whether gs_design_score has run; nothing is copied */
gs_status gs_design_info(const gs_design *design, uint64_t *n, int *scored);
/* of the last gs_design_select / gs_design_rows: records, kept records, groups left without a record, groups short of N */
gs_status gs_design_last_select(const gs_design *design, uint64_t out[4]);
void gs_design_free(gs_design *design);
/* Host only: restrict, order, select and ids through gs_regions_scan.h, with no device (no counterpart in the reference).
 * Part i: n[i] candidates of chromosome chr_index[i] as a scan gives them; specificity / eligible (or NULL) are per
 * candidate.  *out has no device side; rows (or NULL): the kmers-file rows, malloc'ed. */
gs_status gs_debug_design_host(const gs_regions *regions, uint32_t n_parts, const uint32_t *chr_index, const uint64_t *n,
                               const uint8_t *const *seqs, const uint32_t *const *positions, const uint8_t *const *senses,
                               const float *const *specificity, const uint8_t *const *eligible, const char *pam, uint32_t k,
                               const char *prefix, uint32_t per_region, float min_specificity, gs_kmers **out, char **rows,
                               uint64_t *rows_len);

/* ---- off-targets annotated with the features of a BED file ------------------------------------------------------------- */
/* The reference has no counterpart for anything in this section: its users join the CSV against a BED file in a script.  The
 * rule, stated once (gs_annot_scan.h): a printed row whose match_position is s (as resolve_absolute returns it) occupies
 * the forward-strand bases [s - 1, s - 1 + L + P) of match_chrm, clipped to [0, chromosome length) - the reference prints
 * rows with s == 0 - with the guide's own L and P for every row.  The row has feature g iff that footprint shares a base
 * with an interval of group g on the chromosome (overlap, not the containment of the regions section).  A row's features
 * are distinct and ascend by group number, the order of first appearance in the file.  A hit that resolve_absolute drops has
 * no row, no features and is counted nowhere. */

typedef struct gs_annot gs_annot;

/* the name of group g of a parsed BED file (no counterpart in the reference); the string is the object's */
gs_status gs_regions_group_name(const gs_regions *regions, uint64_t g, const char **name);
/* The lookup table of a parsed BED file (no counterpart in the reference): per chromosome the sorted distinct interval ends
 * cut it into elementary segments, each with the ascending list of the groups over it (CSR), and the group names as one
 * blob; both are uploaded to `device` (-1: host only, for the host encoders and gs_debug_annotate_host) and kept on the host.
 * The object is independent of `regions` afterwards.  GS_ERR_FORMAT, the message naming the group: a group name with ';',
 * which would break the joined column.  GS_ERR_ARG: a table of more than 2^31 entries (the sum of the segments' depths),
 * refused before it is allocated. */
gs_status gs_annot_build(const gs_regions *regions, int device, gs_annot **out);
/* groups, elementary segments and table entries (no counterpart in the reference); any pointer may be NULL */
gs_status gs_annot_info(const gs_annot *annot, uint64_t *n_groups, uint64_t *n_segments, uint64_t *n_entries);
/* (no counterpart in the reference) a handle the annotation is attached to must be detached first */
void gs_annot_free(gs_annot *annot);
/* the entry cap of gs_annot_build (no counterpart in the reference): set != 0 sets it (at most 2^31); -> the cap.  For tests */
uint64_t gs_debug_annot_entry_cap(uint64_t set);

/* The features of every hit of a CSR hit list, in HBM (no counterpart in the reference): one lane per hit, a count pass, a
 * scan, an emit pass.  d_offsets, d_hits: the layout gs_score_device takes; d_offsets[0] need not be 0.  `gs` must have the
 * chromosome lengths the BED file was parsed against.  With n_hits = d_offsets[n] - d_offsets[0], hit i being
 * d_hits[d_offsets[0] + i]:
 *   *d_feat_offsets : uint64[n_hits + 1], from 0
 *   *d_feats        : uint32 group numbers, hit i's at [feat_offsets[i], feat_offsets[i + 1])
 *   *d_guide_counts : uint32[n * (mismatches + 1)]: the hits of guide g at distance d that have a row and at least one
 *                     feature, at [g * (mismatches + 1) + d]; whatever --max-off-targets is
 * all owned by the handle and valid until the next call on it.  GS_ERR_ARG: a hit at a distance beyond `mismatches`, an
 * annotation of another device. */
gs_status gs_annotate_device(gs_index *ix, const gs_annot *annot, const gs_genome_structure *gs, uint64_t n, uint32_t L,
                             uint32_t P, uint32_t mismatches, const void *d_offsets, const void *d_hits, void *stream,
                             const void **d_feat_offsets, const void **d_feats, const void **d_guide_counts);
/* The same with host arrays in and out, the copies made inside (no counterpart in the reference): feat_offsets
 * (n_hits + 1) and guide_counts (n * (mismatches + 1)) are the caller's, *feats is malloc'ed (*n_feats entries): release
 * with gs_free. */
gs_status gs_annotate(gs_index *ix, const gs_annot *annot, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                      uint32_t mismatches, const uint64_t *offsets, const gs_hit *hits, uint64_t *feat_offsets, uint32_t **feats,
                      uint64_t *n_feats, uint32_t *guide_counts);
/* Host only: the same results through gs_annot_scan.h with no device (no counterpart in the reference) */
gs_status gs_debug_annotate_host(const gs_annot *annot, const gs_genome_structure *gs, uint64_t n, uint32_t L, uint32_t P,
                                 uint32_t mismatches, const uint64_t *offsets, const gs_hit *hits, uint64_t *feat_offsets,
                                 uint32_t **feats, uint64_t *n_feats, uint32_t *guide_counts);

/* The selection rule for guides for regions (no counterpart in the reference), set before gs_design_score: the score phase
 * then also runs gs_annotate_device on each batch and stores, per record, the number of off-target hits at distance <=
 * `distance` that have a feature of `annot`.  The record's own site - the distance-0 hit whose resolved chromosome, position
 * and strand equal the record's chromosome, position and sense - does not count.  A record with more than max_hits is
 * not eligible, exactly as one a --threshold drops.  annot NULL takes the rule off; without a rule gs_design_score is
 * unchanged.  The annotation must outlive the score phase. */
gs_status gs_design_set_feature_rule(gs_design *design, const gs_annot *annot, uint32_t distance, uint32_t max_hits);
/* those counts of the last gs_design_score as uint32[n] on the host, owned by the design (no counterpart in the
 * reference); GS_ERR_ARG when that score phase ran without a rule */
gs_status gs_design_get_feature_hits(gs_design *design, const void **counts);

/* ---- guide pairs for regions ----------------------------------------------------------------------------------------- */
/* The reference has no counterpart for anything in this section.  The rule, stated once (gs_pairs_scan.h): a record of a
 * design with footprint [q, q + k + P), q = position - 1, has its PAM on the right of the protospacer on the forward
 * strand iff (sense == '+') != GS_FLAG_PAM_AT_START.  Its cut is the boundary x - between bases x - 1 and x - that leaves
 * cut_offset protospacer bases between cut and PAM: x = q + k - cut_offset with the PAM on the right, x = q + P + cut_offset
 * otherwise.  A pair is two distinct eligible records a, b of one group and one chromosome, a before b in the order
 * (chromosome, cut, sense with '+' first), with min_span <= x_b - x_a <= max_span; eligible: the design's eligibility byte,
 * and specificity >= min_specificity where that is >= 0.  GS_PAIRS_PAM_OUT: a's PAM on the left and b's on the right (the
 * PAMs face away from each other); GS_PAIRS_PAM_IN: the reverse.  Within a group the pairs are ranked by the smaller of the
 * two specificities descending, then the larger descending, then by a and b in the order above; per_region N > 0 keeps the
 * first N of each group, 0 keeps all.  Pairs never span groups or chromosomes; membership in a group is still by
 * footprint, not by cut. */
typedef struct gs_pairs gs_pairs;
#define GS_PAIRS_ANY 0u
#define GS_PAIRS_PAM_OUT 1u
#define GS_PAIRS_PAM_IN 2u
typedef struct gs_pair_rule {
  uint64_t min_span, max_span;
  uint32_t cut_offset, orientation /* GS_PAIRS_ANY | _PAM_OUT | _PAM_IN */, per_region /* 0: all */, flags /* GS_FLAG_PAM_AT_START */;
  float min_specificity; /* < 0: none */
  uint32_t pad;
} gs_pair_rule;
/* The kept pairs of a scored design and the guides they are made of, in HBM passes of one lane per element (no counterpart
 * in the reference; gs_pairs.hip).  *guides: the records that are a member of at least one kept pair, once per group, in the
 * order and with the ids of gs_design_select(per_region = 0); it behaves as that call's object.  *pairs: the kept pairs,
 * group by group in ranked order.  A design with no pair gives two empty objects.  GS_ERR_ARG: a design gs_design_score has
 * not scored, min_span > max_span, cut_offset > k, an unknown orientation, a bound that is NaN or above 1.
 * GS_ERR_UNSUPPORTED, the message naming the group and its pair count: a group with more pairs than one chunk holds (2^26;
 * gs_debug_pairs_chunk).  The design is unchanged. */
gs_status gs_design_pairs(gs_design *design, const char *prefix, const gs_pair_rule *rule, void *stream, gs_kmers **guides,
                          gs_pairs **pairs);
/* host copies of the kept pairs, the object's (no counterpart in the reference): group, chr, a, b, cut_a, cut_b uint32[n],
 * spec_a, spec_b float[n]; a and b are places in the guides object; cuts are 0-based as defined above.  Any pointer may be
 * NULL. */
gs_status gs_pairs_get(gs_pairs *pairs, uint64_t *n, const void **group, const void **chr, const void **a, const void **b,
                       const void **cut_a, const void **cut_b, const void **spec_a, const void **spec_b);
/* the table, header included (no counterpart in the reference), formatted on the host - it has per_region rows a group:
 * `group,id_a,id_b,chromosome,cut_a,cut_b,span,specificity_a,specificity_b,pair_specificity`, ids exactly those of `guides`
 * (the object gs_design_pairs made with these pairs), the floats as the CSV's specificity column (std::to_string(float)),
 * pair_specificity the smaller one.  *text is malloc'ed (NUL terminated): release with gs_free */
gs_status gs_pairs_rows(gs_pairs *pairs, const gs_kmers *guides, char **text, uint64_t *len);
/* (no counterpart in the reference) eligible records, pairs counted, pairs kept, chunks, groups without a pair, groups
 * short of per_region */
gs_status gs_pairs_last(const gs_pairs *pairs, uint64_t out[6]);
/* the milliseconds of gs_design_pairs' stages between events on its stream (no counterpart in the reference): marking and
 * compacting the eligible records; ordering them (two sorts, the sorted arrays, the prefix counts); the count pass; the
 * offsets and group heads; the emit pass; the ranking sorts; cut, gather and flags; the guides object and the result
 * arrays - the chunked ones summed over the chunks.  Zeros from gs_debug_pairs_host. */
#define GS_PAIRS_STAGES 8
gs_status gs_pairs_ms(const gs_pairs *pairs, double out[GS_PAIRS_STAGES]);
/* (no counterpart in the reference) */
void gs_pairs_free(gs_pairs *pairs);
/* Host only: the same passes through gs_pairs_scan.h on plain arrays of n records, with no device (no counterpart in the
 * reference).  groups are < n_groups.  *out holds what gs_pairs_get gives, a and b as indices of the records given; it has
 * no names, so gs_pairs_rows on it is GS_ERR_ARG. */
gs_status gs_debug_pairs_host(uint64_t n, const uint32_t *group, const uint32_t *chr, const uint32_t *position, const uint8_t *sense,
                              const float *specificity, const uint8_t *eligible, uint32_t k, uint32_t P, uint32_t n_groups,
                              const gs_pair_rule *rule, gs_pairs **out);
/* the most pairs a chunk of gs_design_pairs holds (no counterpart in the reference): set != 0 sets it (below 2^32); -> the
 * value.  For tests */
uint64_t gs_debug_pairs_chunk(uint64_t set);

/* ---- library selection: sequence rules on the candidates, spacing between the picks of a group ------------------------ */
/* The reference has no counterpart for anything in this section: its users filter the genome-wide table in a script.  The
 * rules, stated once (gs_select_scan.h).  Sequence rule: over the k protospacer bytes of a candidate as the kmers file's
 * `sequence` column prints them (guide orientation, both senses, with and without --start; the PAM is not looked at; any
 * case).  With g the number of G and C the candidate passes iff gc_min * k <= 100 * g <= gc_max * k; iff no letter stands
 * more than max_run times in a row (0: no bound); and iff no motif matches at any offset, a position matching when the
 * base is in the IUPAC letter's set.  A failing candidate is charged to the first rule it fails: GC, run, motif. */
#define GS_SEQ_MOTIFS 16u        /* at most, after the expansion of sites */
#define GS_SEQ_MOTIF_LETTERS 32u /* of one motif, at most */
typedef struct gs_seq_rule {
  uint32_t gc_min, gc_max; /* percent, 0 <= gc_min <= gc_max <= 100; 0 and 100: no bound */
  uint32_t max_run;        /* 0: no bound */
  uint32_t n_motifs;
  uint8_t motif_len[GS_SEQ_MOTIFS];
  /* one 4-bit set per position (A = 1, C = 2, G = 4, T = 8), two positions to a byte, the even one in the low half */
  uint8_t motif_set[GS_SEQ_MOTIFS][GS_SEQ_MOTIF_LETTERS / 2];
} gs_seq_rule;
/* the rule that passes everything (no counterpart in the reference): gc 0:100, no run bound, no motif */
gs_status gs_seq_rule_init(gs_seq_rule *rule);
/* One more motif over ACGTRYSWKMBDHVN, either case (no counterpart in the reference); both_strands != 0 adds its reverse
 * complement too, the IUPAC complement letter by letter, unless that is the motif itself.  GS_ERR_FORMAT, and
 * gs_status_string(GS_ERR_FORMAT) reads as one line that names the motif: an empty motif, one of more than
 * GS_SEQ_MOTIF_LETTERS letters, a letter outside the alphabet, or a motif beyond GS_SEQ_MOTIFS; the rule is then unchanged. */
gs_status gs_seq_rule_add_motif(gs_seq_rule *rule, const char *motif, int both_strands);
/* The candidates of a scan that pass the rule, as a fresh object in HBM on the scan's device, in the scan's order (no
 * counterpart in the reference): one lane per candidate evaluates the rule, a 64-bit scan of the flags, a gather.  counts:
 * candidates in, failed by GC, by run, by motif.  Called before gs_kmers_encode_ids: GS_ERR_ARG on an object that has ids,
 * on the rows of a kmers file, and for a rule outside its bounds.  `km` is unchanged and still the caller's. */
gs_status gs_kmers_filter(gs_kmers *km, const gs_seq_rule *rule, void *stream, gs_kmers **out, uint64_t counts[4]);
/* the milliseconds of the three passes that made a gs_kmers_filter's result, between events on its stream (no counterpart
 * in the reference): rule, scan, gather */
gs_status gs_debug_kmers_filter_ms(const gs_kmers *filtered, double out[3]);
/* Host only: the rule through gs_select_scan.h on n sequences of k bytes back to back, with no device (no counterpart in
 * the reference).  charge[i]: 0 where sequence i passes, else 1, 2 or 3 for GC, run, motif; counts as above. */
gs_status gs_debug_kmers_filter_host(const uint8_t *seqs, uint64_t n, uint32_t k, const gs_seq_rule *rule, uint8_t *charge,
                                     uint64_t counts[4]);

/* Spacing (no counterpart in the reference), over the order of gs_design_select: walk a group's marked records (eligible
 * and specificity >= min_specificity) in that order and keep a record iff every record already kept in this group on the
 * same chromosome has its cut at least min_spacing bases away; stop at per_region kept.  The cut is that of the pairs
 * section with cut_offset and flags (GS_FLAG_PAM_AT_START).  min_spacing 0 takes the rule off: the selection is then the
 * code and the bytes it was.  With the rule set gs_design_select and gs_design_rows need 1 <= per_region <= 1024
 * (GS_ERR_ARG otherwise, with a message), and gs_design_pairs is GS_ERR_ARG.  GS_ERR_ARG: cut_offset > k, another flag. */
gs_status gs_design_set_spacing(gs_design *design, uint32_t min_spacing, uint32_t cut_offset, uint32_t flags);
/* of the last gs_design_select / gs_design_rows under the rule (no counterpart in the reference): the marked records the
 * walks passed over for spacing, and the groups left short of per_region that hold at least per_region marked records */
gs_status gs_design_last_spacing(const gs_design *design, uint64_t out[2]);
/* the milliseconds of that selection's walk kernel alone, between events on its stream (no counterpart in the reference) */
gs_status gs_debug_design_space_ms(const gs_design *design, double *ms);
/* Host only: gs_debug_design_host with the rule's three arguments, through gs_select_scan.h (no counterpart in the
 * reference).  report (or NULL): what gs_design_last_select and gs_design_last_spacing would give, six numbers. */
gs_status gs_debug_design_host_spaced(const gs_regions *regions, uint32_t n_parts, const uint32_t *chr_index, const uint64_t *n,
                                      const uint8_t *const *seqs, const uint32_t *const *positions, const uint8_t *const *senses,
                                      const float *const *specificity, const uint8_t *const *eligible, const char *pam, uint32_t k,
                                      const char *prefix, uint32_t per_region, float min_specificity, uint32_t min_spacing,
                                      uint32_t cut_offset, uint32_t flags, gs_kmers **out, char **rows, uint64_t *rows_len,
                                      uint64_t *report);
/* Specificities and eligibility bytes of a design's n records from host arrays, in record order; the design then counts
 * as scored (no counterpart in the reference).  eligible NULL: every record.  For tests: the selection kernels run on
 * chosen ranks and ties without a search. */
gs_status gs_debug_design_set_scores(gs_design *design, const float *specificity, const uint8_t *eligible);

/* ---- non-targeting controls for a library: `guidescan controls` ------------------------------------------------------- */
/* The reference has no counterpart for anything in this section: its manual strips the CTRL guides out of its example
 * library before analysing it (manual/manual.tex:403-411), and the only way to make them is to draw random protospacers
 * and search each.  The rules, stated once (gs_controls_scan.h).  Candidate i is a 64-bit counter from `first`; for seed s
 * its protospacer is a pure function of (s, i, L): with mix(x) the splitmix64 finaliser (x += 0x9E3779B97F4A7C15, two
 * xor-shift-multiplies by 0xBF58476D1CE4E5B9 and 0x94D049BB133111EB, x ^ x >> 31), w = mix(mix(s) ^ i) and base j of the
 * sequence column is "ACGT"[(w >> 2j) & 3]; the PAM column is the pattern.  Candidates are walked in ascending i and each
 * is charged to the first thing it fails: the sequence rule (GC, run, motif, as above), targeting (its hit list on the
 * fast path under `mismatches`, the pattern, the alt PAMs and GS_FLAG_PAM_AT_START is not empty - before positions are
 * resolved, so a site across a chromosome boundary disqualifies too), close (fewer than min_distance mismatches to a
 * control already kept).  Otherwise it is kept.  The walk stops at the candidate that makes n kept or after
 * max_candidates.  The kept list, its order and every count depend on these arguments and the genome only, never on the
 * round size or the device; the controls for n = a are the first a of those for n = b > a. */
typedef struct gs_controls_rule {
  uint64_t seed, first;
  uint64_t n;              /* controls wanted, 1 .. 16,384 (the walk keeps a round's controls in LDS) */
  uint64_t max_candidates; /* 0: 2^32 */
  uint64_t round;          /* counters generated per round, at most 2^24; 0: the default (2^20, gs_debug_controls_round) */
  uint32_t L;              /* 1 .. 31, and 2L + 3P <= 59 where the device searches */
  uint32_t n_alt;
  uint32_t mismatches;
  /* GS_FLAG_PAM_AT_START; GS_FLAG_NO_NEW_TABLES: never build derived tables.  Without it the call still builds none before it
   * has searched 5 candidates per 1,000 genome bases, the tables' break-even; tables the handle holds already are used */
  uint32_t flags;
  uint32_t min_distance;   /* 1 drops exact repeats only, 0 nothing */
  uint32_t pad;
  const char *pam;                /* the pattern, P <= 8 symbols, NUL terminated */
  const char *alt_pams;           /* n_alt * P bytes, or NULL */
  const gs_seq_rule *seq_rule;    /* NULL: none */
  const char *id_prefix;          /* NULL: "control_"; at most 255 bytes */
} gs_controls_rule;
typedef struct gs_controls_report {
  uint64_t kept;         /* controls kept */
  uint64_t looked_at;    /* candidates from `first` to the last one looked at, inclusive */
  uint64_t gc, run, motif; /* of those: charged to the sequence rule */
  uint64_t targeting;    /* charged for a hit list that is not empty */
  uint64_t close;        /* charged to the distance rule */
  uint64_t last_counter; /* counter of the last candidate looked at (`first` when none was) */
  uint64_t rounds;       /* rounds run */
  /* milliseconds between events in the stream, summed over the rounds: generate + rule + compaction, search, keep +
   * compaction, distance (both kernels and the count of the charges), ids */
  double ms[5];
} gs_controls_report;
/* The controls as a gs_kmers object in HBM on the handle's device, ids "{prefix}{i}" (i in decimal) from the start (no
 * counterpart in the reference).  Its positions and ids behave as a parsed object's: gs_kmers_get gives NULL positions and
 * '+' senses, gs_kmers_encode_ids and gs_kmers_csv are GS_ERR_ARG, and its arrays are what gs_enumerate_text_device /
 * gs_format_device_ids take.  Per round: k_ct_generate (one lane per counter: word, sequence rule), a scan and a gather
 * into the layout gs_enumerate_device takes, the search under the handle's lock, k_ct_keep (empty hit list?), a scan and a
 * gather, k_ct_old (against the controls of earlier rounds), k_ct_walk (one wave, in counter order, 64 a step).  Fewer than
 * n kept is still GS_OK and an object: report->kept says so.  GS_ERR_UNSUPPORTED with a message: 2L + 3P > 59, or a
 * candidate the fast path does not take (a PAM symbol outside A,C,G,T,N).  GS_ERR_ARG: a rule outside its bounds,
 * first + max_candidates beyond 2^64. */
gs_status gs_controls_generate(gs_index *ix, const gs_controls_rule *rule, void *stream, gs_kmers **out, gs_controls_report *report);
/* the kmers-file rows "id,sequence,pam,NA,0,+\n" of such an object (no counterpart in the reference; the reference's reader
 * wants the three location columns, src/genomics/kmer.cxx:9-25, its printers never look at them): rows only, no header;
 * *text is malloc'ed (NUL terminated, *len bytes before the terminator): release with gs_free.  GS_ERR_ARG on any other object */
gs_status gs_controls_rows(gs_kmers *controls, char **text, uint64_t *len);
/* the kept counters in order, n entries owned by the object (no counterpart in the reference) */
gs_status gs_controls_counters(gs_kmers *controls, uint64_t *n, const uint64_t **counters);
/* Host only: the walk through gs_controls_scan.h with no device and no search (no counterpart in the reference).
 * targeting[j] != 0: candidate first + j has a hit - the caller says, the tests take it from the oracle; the walk looks at
 * min(n_candidates, max_candidates) candidates at most.  *counters (the kept counters, report->kept of them) and *rows are
 * malloc'ed: release with gs_free.  rule->round != 0: the walk is cut into rounds of that many candidates the way the
 * device cuts it (earlier rounds' controls first, then the round's own walk), which must change nothing.  flags, mismatches
 * and alt PAMs are not looked at; ms stays 0, rounds 0. */
gs_status gs_debug_controls_host(const gs_controls_rule *rule, const uint8_t *targeting, uint64_t n_candidates, uint64_t **counters, char **rows,
                                 uint64_t *rows_len, gs_controls_report *report);
/* Host only: the generator alone (no counterpart in the reference): out gets n * L ASCII bytes, candidates first .. first + n - 1 */
gs_status gs_debug_controls_sequences(uint64_t seed, uint64_t first, uint64_t n, uint32_t L, uint8_t *out);
/* the counters of a round where the rule says 0 (no counterpart in the reference): set != 0 sets it (at most 2^24) for every
 * later call of the process; -> the value.  For tests */
uint64_t gs_debug_controls_round(uint64_t set);

/* The column (no counterpart in the reference).  GS_TEXT_FEATURES: the CSV header ends in ",match_features" and every CSV
 * row ends in ',' and the names of the row's features joined by ';', or "NA" if it has none; the `NA` row of a guide without
 * hits ends in ",NA" too.  Both modes.  Together with GS_TEXT_SAM or GS_TEXT_BAM: GS_ERR_ARG, in every entry point below
 * and in gs_format_header.  The entry points that existed before the flag ignore it: their bytes do not change. */
#define GS_TEXT_FEATURES 0x4000u
/* Attaches an annotation (built for the handle's device) to the handle, NULL detaches it (no counterpart in the reference);
 * the annotation stays the caller's and must outlive its attachment.  With GS_TEXT_FEATURES in their flags, gs_format_device,
 * gs_format_device_ids, gs_enumerate_text and gs_enumerate_text_device run gs_annotate_device between scoring and formatting
 * and append the column on the device; the flag without an attached annotation is GS_ERR_ARG. */
gs_status gs_index_set_annotation(gs_index *ix, const gs_annot *annot);
/* The host encoders' twins (no counterpart in the reference): gs_format_guides_scored, gs_format_guide_scored and
 * gs_format_guide_ex with the rows looked up on the CPU through gs_annot_scan.h when GS_TEXT_FEATURES is set (then `annot`
 * is required); without the flag, the bytes of the entry point each is the twin of. */
gs_status gs_format_guides_features(const gs_genome_structure *gs, const gs_kmer *kmers, uint64_t n, const uint64_t *offsets,
                                    const gs_hit *hits, const float *specificity, const uint8_t *skip, uint32_t mismatches,
                                    uint32_t flags, int64_t max_off_targets, const gs_annot *annot, char **out_text,
                                    size_t *out_len);
gs_status gs_format_guide_features(const gs_genome_structure *gs, const gs_kmer *k, const gs_hit *hits, uint64_t n_hits,
                                   uint32_t mismatches, uint32_t flags, int64_t max_off_targets, float specificity,
                                   const gs_annot *annot, char **out_text, size_t *out_len);
gs_status gs_format_guide_ex_features(const gs_genome_structure *gs, const gs_kmer *k, const gs_hit_ex *hits, uint64_t n_hits,
                                      uint32_t mismatches, uint32_t flags, int64_t max_off_targets, const gs_annot *annot,
                                      char **out_text, size_t *out_len);

/* ---- SAM/BAM databases back to CSV on the device (scripts/decode_database.py) --------------------------------- */

typedef struct gs_decoder gs_decoder;

/* What the script loads once (load_guide_db, :142-146, and SeqIO.to_dict, :223): the @SQ names and LN in header order
 * (sq), and the FASTA records' symbols back to back in `text` (any case; folded to upper case on upload, :59).
 * Chromosome c of sq is the record text[chr_text_off[c], + chr_text_len[c]) - its own length, which may differ from
 * LN; chr_text_len[c] = UINT64_MAX: the FASTA has no record of that name (an off-target on it fails, as fasta_dict[chr]
 * does).  The text, the tables of the CFD (calc_cfd_e, :67-83) and of the double printer stay in HBM until
 * gs_decoder_close.  No index is needed. */
gs_status gs_decoder_open(int device, const uint8_t *text, uint64_t len, const gs_genome_structure *sq,
                          const uint64_t *chr_text_off, const uint64_t *chr_text_len, gs_decoder **out);
void gs_decoder_close(gs_decoder *dec);

/* the fields the script reads of n records (pysam's query_name, query_sequence, is_reverse, reference_name,
 * reference_start, get_tag('of')), each variable-length one as bytes back to back with n + 1 offsets */
typedef struct {
  uint64_t n;
  const char *ids;
  const uint64_t *id_off;
  const char *seqs; /* SEQ as stored, at most 32 symbols each */
  const uint64_t *seq_off;
  const uint8_t *reverse; /* FLAG & 16 */
  const int32_t *chr;     /* index into sq, -1: RNAME is '*' or a name that no @SQ line has (printed as None) */
  const int64_t *pos0;    /* POS - 1 */
  const char *hex;        /* the of:H: digits; an empty span: no field */
  const uint64_t *hex_off;
} gs_decode_batch;

#define GS_DECODE_NO_HEADER 0x400u /* gs_decode_sam: rows only */

/* The rows the script prints for these records, no header line: output_succinct (:156-187; flags 0) or output_complete
 * (:148-154; GS_TEXT_COMPLETE) over decode_off_targets (:106-140), byte for byte, floats as Python's repr.  *n_rows
 * (may be NULL): rows written.  Where the script would raise - hex digits that are no multiple of 16 or no hex digits,
 * |word| >= sum of LN, a PAM pair outside the 16 keys, in succinct mode a distance outside 0..3 (negative ones too),
 * a chromosome the FASTA lacks - GS_ERR_FORMAT, no text, and gs_status_string(GS_ERR_FORMAT) names record `first_record` + its index
 * in the batch, its id and the reason; the first such record of the batch.  The result does not depend on how the
 * records are cut into batches.  *text is malloc'ed (NUL terminated, *len bytes before the terminator): gs_free. */
gs_status gs_decode_records(gs_decoder *dec, const gs_decode_batch *batch, uint32_t flags, uint64_t first_record, char **text,
                            uint64_t *len, uint64_t *n_rows);
/* the same with the text left in HBM: *d_text belongs to the decoder and is valid until its next call */
gs_status gs_decode_records_device(gs_decoder *dec, const gs_decode_batch *batch, uint32_t flags, uint64_t first_record,
                                   const void **d_text, uint64_t *len, uint64_t *n_rows);
/* SAM text (whole lines; header lines are skipped: the @SQ lines went into gs_decoder_open) split into records on the
 * host, then gs_decode_records; the script's header line first (:213-217) unless GS_DECODE_NO_HEADER.  A line with
 * fewer than eleven fields or a FLAG or POS that is no number: GS_ERR_FORMAT. */
gs_status gs_decode_sam(gs_decoder *dec, const char *sam, uint64_t sam_len, uint32_t flags, uint64_t first_record, char **text,
                        uint64_t *len, uint64_t *n_records);

/* A decoded database annotated with the features of a BED file, in the pass that decodes it (no counterpart in the
 * reference: its users join the decoded CSV against the BED file in a script; the database keeps the reference's format, no
 * tag is added, so any database is annotatable).  The rule, stated once (gs_annot_scan.h: gs_an_decoded_footprint): an
 * off-target of a record whose stored SEQ has n symbols, decoded to chromosome c (LN bases by its @SQ line), coordinate x (as
 * map_int_to_coord, :38-50, gives it) and a strand, occupies the forward-strand bases the script slices: [x + 1 - n, x + 1)
 * on '+', [x, x + n) on '-', clipped to [0, LN) - by LN, not by the FASTA record's length, and without Python's wrap of a
 * negative slice start: a row whose printed sequence is short or wrapped is annotated by where it lies.  The row has
 * feature g iff that footprint shares a base with an interval of group g on c (overlap, as for GS_TEXT_FEATURES above);
 * features are distinct and ascend by group number; an empty footprint has none.
 * gs_decoder_set_annotation attaches an annotation, NULL detaches it; the annotation stays the caller's and must outlive
 * its attachment.  GS_ERR_ARG: an annotation built for another device or for the host only, or one whose chromosome count
 * or lengths differ from the decoder's @SQ table.
 * GS_TEXT_FEATURES is then valid in the flags of gs_decode_records, gs_decode_records_device, gs_decode_sam, gs_decode_bam
 * and gs_decode_bam_device; without an attached annotation it is GS_ERR_ARG; without the flag every byte is what it was.
 *   complete mode: the header (gs_decode_sam) ends in ",match_features", every row in ',' and the group names joined by
 *     ';', or NA.
 *   succinct mode: the header ends in ",distance_0_feature_matches,...,distance_3_feature_matches", every row in those four
 *     counts: the record's off-targets at that distance that have at least one feature, counted exactly as
 *     distance_k_matches counts - every off-target of the list, the record's own site included.
 * GS_DECODE_FEATURES_ONLY (only with GS_TEXT_FEATURES | GS_TEXT_COMPLETE, else GS_ERR_ARG): rows without a feature are left
 * out; match_number stays the rank among all of the record's off-targets, so the table joins against the full one; *n_rows
 * counts the rows written.
 * The script's failures stay GS_ERR_FORMAT with the same record and reason as without the flag, and win over anything the
 * annotation does (a row of 32 MB or more, GS_ERR_UNSUPPORTED, is looked for only in a batch that has none). */
#define GS_DECODE_FEATURES_ONLY 0x8000u
gs_status gs_decoder_set_annotation(gs_decoder *dec, const gs_annot *annot);
/* the milliseconds of the annotation pass in the decoder's last batch that ran one, between two stream events (no
 * counterpart in the reference) */
gs_status gs_debug_decode_annot_ms(gs_decoder *dec, double *ms);
/* Host only: Python's repr() of n doubles, 32 bytes each, NUL padded - the routine the decoder's kernels print with. */
gs_status gs_debug_repr_doubles(const double *v, uint64_t n, char *out);
/* Host only: the CFD tables the decoder uploads: mm[(r * 4 + d) * 20 + i] for the key r{ACGU}:d{ACGT},i+1 (320), pam[16] */
gs_status gs_debug_decode_tables(double *mm, double *pam);

/* ---- BGZF on the device, the other way: the inflate step of reading a BAM database ---------------------------- */

/* BGZF members (SAMv1 section 4.1: gzip members with the BC subfield, what `samtools view -b` of manual/manual.tex:581-582
 * and gs_bgzf_compress write; SAMv1 section 4.2 is what they hold), back to back in host memory -> their bytes, inflated
 * on the device: the mirror of gs_bgzf_compress, and the first step of scripts/decode_database.py's pysam.AlignmentFile on
 * a BAM database.  Any writer's members are taken: several deflate blocks, stored, fixed and dynamic ones.  A zero-length
 * member (the end-of-file block) gives no bytes.  The host walks the members (1f 8b 08 04, XLEN, the BC subfield among
 * any others, BSIZE; CRC-32 and ISIZE from the trailer); a wave inflates a member and checks its CRC-32.  GS_ERR_FORMAT:
 * gs_status_string names the first failing member's index, its byte offset in `bgzf` and the reason (a BSIZE that runs
 * past the data, no BC subfield, ISIZE above 65,536, a damaged deflate stream, a wrong CRC-32 or ISIZE); no bytes then.
 * *out is malloc'ed: release with gs_free. */
gs_status gs_bgzf_inflate(int device, const void *bgzf, uint64_t len, uint8_t **out, uint64_t *out_len);
/* The same (SAMv1 sections 4.1 and 4.2, scripts/decode_database.py as above) with the result left in the decoder's
 * workspace: *d_out holds the last `keep` bytes of what the call before left (the tail of a BAM record cut by the end of
 * that group of members; keep <= its length), then the bytes of these members; *out_len counts both.  *d_out belongs to
 * the decoder until the call after the next one.  *n_members (may be NULL): members inflated.  A failed call leaves
 * what the call before left. */
gs_status gs_bgzf_inflate_device(gs_decoder *dec, const void *bgzf, uint64_t len, uint64_t keep, const void **d_out,
                                 uint64_t *out_len, uint64_t *n_members);
/* Where the bytes of the decoder's next gs_bgzf_inflate_device / gs_decode_bam* calls lie in their file (SAMv1 section 4.1; a
 * file that scripts/decode_database.py would read whole is handed over in groups of members): the members and the bytes in
 * front of them.  They are added to the index and the offset in the message of a member that fails, which then names
 * the member in the file.  They stay until set again; 0, 0 at first. */
gs_status gs_bgzf_inflate_base(gs_decoder *dec, uint64_t members_before, uint64_t bytes_before);
/* Host only: one whole member (header, deflate stream, trailer; SAMv1 section 4.1, as pysam reads it for
 * scripts/decode_database.py) through the function the kernel's lane runs (gs_bgzf_inflate.h).  out[cap] takes ISIZE
 * bytes (GS_ERR_ARG when cap is smaller).  *reason: 0, or why the member fails (then GS_ERR_FORMAT); *out_len: the bytes
 * made up to there. */
gs_status gs_debug_inflate_member(const void *member, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint32_t *reason);
/* Host only: the member table's walk over bgzf[0, len) (SAMv1 section 4.1; scripts/decode_database.py reads such files
 * through pysam): *n members, the first `cap` of them with their offsets and ISIZE (either array may be NULL).
 * GS_ERR_FORMAT and *reason when a member is refused; *n is then its index. */
gs_status gs_debug_bgzf_members(const void *bgzf, uint64_t len, uint64_t *member_off, uint32_t *isize, uint64_t cap, uint64_t *n,
                                uint32_t *reason);

#define GS_DECODE_BAM_END 0x2000u /* gs_decode_bam: the data ends with these members */

/* A BAM database's records, still compressed, to the rows scripts/decode_database.py prints for them, on the device all
 * the way: the BGZF members (SAMv1 section 4.1) are inflated as by gs_bgzf_inflate_device, the alignment records (SAMv1
 * section 4.2) are found by following their block_size fields and split into the arrays of gs_decode_batch in HBM
 * (read_name without its NUL, SEQ as =ACMGRSVTWYHKDBN letters, FLAG & 16, refID through ref_to_sq, pos, the last of:H:
 * tag), then the kernels of gs_decode_records run.  bgzf: whole members.  skip: the inflated bytes of these members that
 * belong to the BAM header (magic, text, reference list); a call with skip != 0 begins a file, and a file's header lies
 * within its first call.  ref_to_sq[n_ref]: the binary reference list's entries as indices of the decoder's
 * chromosomes, negative: no @SQ line (such a record, like one with a negative refID, prints None).  Rows only, no header
 * line; flags: GS_TEXT_COMPLETE, GS_DECODE_BAM_END, GS_TEXT_FEATURES [| GS_DECODE_FEATURES_ONLY] as gs_decode_records takes
 * them (checked before anything is inflated).  *n_records: the complete records of this call (the next call's
 * first_record grows by it); *tail: the bytes of a record cut by the end of these members.  The decoder keeps them
 * and the next call's records begin with them, so a file streams in groups of members and the output does not depend
 * on where the groups are cut.  With GS_DECODE_BAM_END a tail is an error.  GS_ERR_FORMAT names the first record in
 * file order that is malformed, by index and with decode_bam_file's words - "a record shorter than its fixed part",
 * "a record's fields outrun it", "a record's reference is beyond the list", "a text tag without its end", "an array
 * tag", "a tag of unknown type", "a tag outruns its record", "a record is cut", "a record's size" - or the member
 * that does not inflate, or what gs_decode_records reports.  *text is malloc'ed (NUL terminated): gs_free. */
gs_status gs_decode_bam(gs_decoder *dec, const void *bgzf, uint64_t len, uint64_t skip, const int32_t *ref_to_sq, uint32_t n_ref,
                        uint32_t flags, uint64_t first_record, char **text, uint64_t *text_len, uint64_t *n_records, uint64_t *tail);
/* the same (SAMv1 sections 4.1 and 4.2, scripts/decode_database.py) with the text left in HBM: *d_text belongs to the
 * decoder and is valid until its next call */
gs_status gs_decode_bam_device(gs_decoder *dec, const void *bgzf, uint64_t len, uint64_t skip, const int32_t *ref_to_sq,
                               uint32_t n_ref, uint32_t flags, uint64_t first_record, const void **d_text, uint64_t *text_len,
                               uint64_t *n_records, uint64_t *tail);
/* The last gs_decode_bam* call of this decoder: counts[4] = members, compressed bytes, inflated bytes, records;
 * ms[4] = milliseconds of inflate (with the upload), record starts, fields, the decoder's kernels. */
gs_status gs_debug_decode_bam_last(gs_decoder *dec, uint64_t *counts, double *ms);

/* ---- FASTA read on the device: the first step of `index` and of `decode` ------------------------------------ */

typedef struct gs_fasta gs_fasta;

/* Both rule sets split the file at '\n' only (a last line without a newline is a line; a newline at the end of the file
 * starts none); a line is a title iff its first byte is '>'; blank = C-locale isspace.
 * GS_FASTA_INDEX_RULES: what the reference's `index` reads (src/genomics/seq_io.cxx:47-63 the sequence, :74-110 the
 *   structure).  A non-title line adds its bytes with the blanks at both ends removed (blanks inside stay), a-z folded to
 *   upper case and every other byte as it is; lines ahead of the first title add to the text but to no record; a record's
 *   line_len is the sum of its lines' untrimmed lengths (seq_io.cxx:100-104; a '\r' counts, the '\n' does not); the name
 *   is the title without its '>' up to the first ' '.
 * GS_FASTA_RECORD_RULES: Bio.SeqIO.to_dict as scripts/decode_database.py:223 calls it.  Lines ahead of the first title are
 *   dropped; every blank of a non-title line is removed; case is left alone; the name is the first run of non-blank bytes
 *   behind '>', leading blanks skipped; a name that occurs twice is GS_ERR_FORMAT, and gs_status_string(GS_ERR_FORMAT)
 *   then reads "FASTA record 'NAME' occurs twice" (the first such title of the file). */
#define GS_FASTA_INDEX_RULES 0u
#define GS_FASTA_RECORD_RULES 1u

/* A FASTA file's bytes -> the text and the record table, parsed in HBM (seq_io.cxx:47-63, :74-110 or SeqIO.to_dict, by
 * `rules`).  raw: host memory, uploaded whole.  The object holds the text in HBM until gs_fasta_free.  Device memory that
 * runs out: GS_ERR_NOMEM, nothing stays allocated. */
gs_status gs_fasta_parse(int device, const uint8_t *raw, uint64_t len, uint32_t rules, gs_fasta **out);
/* The same (seq_io.cxx:57-63 opens the file by name too) from a regular file, read in chunks into two page-locked
 * buffers: a chunk is uploaded while the next is read.  GS_ERR_IO ("cannot read PATH") when it cannot be read - and for
 * anything that is no regular file (a pipe, a process substitution): the device buffer is sized from the file's length. */
gs_status gs_fasta_parse_file(int device, const char *path, uint32_t rules, gs_fasta **out);
/* The same (seq_io.cxx:47-63, :74-110) with the raw bytes in HBM already; the kernels run on `stream`, the call returns
 * when they are done.  d_raw is only read and stays the caller's. */
gs_status gs_fasta_parse_device(int device, const void *d_raw, uint64_t len, uint32_t rules, void *stream, gs_fasta **out);
/* records (title lines), bytes of the text, bytes of all names (genome_structure of seq_io.cxx:74-110) */
gs_status gs_fasta_info(const gs_fasta *fa, uint64_t *n_records, uint64_t *text_len, uint64_t *names_bytes);
/* Per record (any array may be NULL): where its title line begins in the file and its length without the newline; its
 * symbols text[text_off, + text_len); line_len (seq_io.cxx:100-104, both rule sets); its name names[name_off[r],
 * name_off[r + 1]) - name_off has n + 1 entries, names is not NUL terminated (a name may hold any byte). */
gs_status gs_fasta_records(const gs_fasta *fa, uint64_t *title_off, uint64_t *title_len, uint64_t *text_off, uint64_t *text_len,
                           uint64_t *line_len, uint64_t *name_off, char *names);
/* The text (seq_io.cxx:57-63: the <fasta>.forward.dna bytes under the index rules): on_device as in gs_kmers_get - a
 * pointer into HBM, or a host copy that the object makes on the first such call (under a lock of its own: any number of
 * threads may ask) and owns (NUL terminated). */
gs_status gs_fasta_text(const gs_fasta *fa, int on_device, const void **text);
void gs_fasta_free(gs_fasta *fa);
/* gs_decoder_open (scripts/decode_database.py:142-146, :223) from a GS_FASTA_RECORD_RULES object of the same device: sq's
 * names are matched to the records, the text goes from the object to the decoder inside HBM, and the decoder is in the
 * state gs_decoder_open reaches from the host reader's output.  A name without a record: chr_text_len = UINT64_MAX.
 * The object is still the caller's to free, at any time afterwards. */
gs_status gs_decoder_open_fasta(int device, const gs_fasta *fa, const gs_genome_structure *sq, gs_decoder **out);
/* the bytes of a tile of the device passes */
uint64_t gs_debug_fasta_tile_bytes(void);
/* Host only: the summaries, their composition and the walk of the device passes (gs_fasta_scan.h), run one tile after the
 * other with tiles of `tile_bytes` (any size from 1 up): the same text and table (seq_io.cxx:47-63, :74-110 / SeqIO.to_dict).
 * The object has no device side: gs_fasta_text(.., 1, ..) is GS_ERR_ARG. */
gs_status gs_debug_fasta_host(const uint8_t *raw, uint64_t len, uint32_t rules, uint64_t tile_bytes, gs_fasta **out);
/* the bytes of a staging chunk of gs_fasta_parse_file (32 MB); set != 0 replaces it, for every later call of the process */
uint64_t gs_debug_fasta_chunk_bytes(uint64_t set);
/* ms[9] of the object's making.  Host clocks: the file's reads, waits for its uploads, the device stage (its allocations,
 * the five passes and the waits for their results), the title gather with the names.  Then the passes alone, by events
 * in the stream: tile summaries, their two scans, tile counts, the counts' scan, emit. */
gs_status gs_debug_fasta_ms(const gs_fasta *fa, double *ms);

const char *gs_status_string(gs_status s);
const char *gs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GUIDESCAN_AMD_H */
