/* rowtext_check.cpp -- the host/device part of gs_rowtext.h as a host program (make -C guidescan-cli_amd/csrc rowtext-check,
 * under the address and undefined-behaviour sanitizers; no GPU and no library).  For gs_guide_row and for the sinks' u64,
 * each case is run over the counting sink and over the writing sink, into a buffer of exactly the counted length between
 * guard bytes:
 *   1. the counting sink's total is the number of bytes the writing sink wrote;
 *   2. nothing outside them was touched (the guards on both sides; the buffer is exact, so the sanitizer sees a longer store);
 *   3. the bytes are those of an snprintf restatement.
 * Cases: positions of every digit count from 1 to 10 at both ends of the count; for u64 0, 9, 10, every power of ten up to
 * 10^19 with its predecessor, 2^32 - 1, 2^32, 2^64 - 1; an empty prefix, no group, an empty group name, names that bring
 * the id to the 254-byte limit of a BAM record; both senses; ids and rows.  One more case runs `lit`, `put` with a 64-bit
 * length and, over gs_row_write_span, a recorded `span`: the sink advances by its length, leaves the bytes to the copy that
 * follows and records where, from where and how many. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gs_rowtext.h"

namespace {

const unsigned GUARD = 32;
const char GUARD_BYTE = (char)0xA5;
uint64_t checked = 0;

int fail(const std::string &what, const std::string &got, const std::string &want) {
  fprintf(stderr, "rowtext-check: %s\n  got  %s\n  want %s\n", what.c_str(), got.c_str(), want.c_str());
  return 1;
}

/* `emit` over both sinks against `want` */
template <class F>
int check(const std::string &what, const std::string &want, F emit) {
  gs_row_count c;
  emit(c);
  if (c.n != want.size()) return fail(what + ": counted " + std::to_string(c.n) + " bytes", "", want);
  std::vector<char> buf(GUARD + (size_t)c.n + GUARD, GUARD_BYTE);
  gs_row_write w;
  w.p = buf.data() + GUARD;
  emit(w);
  const std::string got(buf.data() + GUARD, (size_t)c.n);
  if (w.p != buf.data() + GUARD + c.n) return fail(what + ": wrote " + std::to_string(w.p - (buf.data() + GUARD)) + " bytes", got, want);
  for (unsigned i = 0; i < GUARD; i++)
    if (buf[i] != GUARD_BYTE || buf[GUARD + (size_t)c.n + i] != GUARD_BYTE) return fail(what + ": a guard byte was overwritten", got, want);
  if (got != want) return fail(what, got, want);
  checked++;
  return 0;
}

int check_u64(uint64_t v) {
  char want[32];
  snprintf(want, sizeof want, "%" PRIu64, v);
  if (gs_dec_digits(v) != strlen(want)) return fail("gs_dec_digits", std::to_string(gs_dec_digits(v)), want);
  return check(std::string("u64 ") + want, want, [&](auto &o) { o.u64(v); });
}

int check_guide(const std::string &prefix, const std::string *group, const std::string &chr, uint32_t pos, char sense, const std::string &seq,
                const std::string &pam) {
  /* the name table as the writers lay it out: prefix, group, chromosome */
  const std::string names = prefix + (group ? *group : std::string()) + chr;
  const uint8_t *nm = (const uint8_t *)names.data();
  const gs_rt_span g{group ? nm + prefix.size() : nullptr, group ? (uint32_t)group->size() : 0u};
  const gs_rt_span c{nm + prefix.size() + (group ? group->size() : 0), (uint32_t)chr.size()};
  std::vector<char> id(names.size() + 32), row(2 * names.size() + seq.size() + pam.size() + 64);
  if (group)
    snprintf(id.data(), id.size(), "%s%s:%s:%u:%c", prefix.c_str(), group->c_str(), chr.c_str(), pos, sense);
  else
    snprintf(id.data(), id.size(), "%s%s:%u:%c", prefix.c_str(), chr.c_str(), pos, sense);
  snprintf(row.data(), row.size(), "%s,%s,%s,%s,%u,%c\n", id.data(), seq.c_str(), pam.c_str(), chr.c_str(), pos, sense);
  for (int rows = 0; rows < 2; rows++) {
    const std::string what = std::string(rows ? "row " : "id ") + id.data();
    if (check(what, rows ? row.data() : id.data(), [&](auto &o) {
          gs_guide_row(o, nm, (uint32_t)prefix.size(), g, c, pos, (uint8_t)sense, (const uint8_t *)seq.data(), (const uint8_t *)pam.data(),
                       (uint32_t)seq.size(), (uint32_t)pam.size(), rows != 0);
        }))
      return 1;
  }
  return 0;
}

/* the members gs_guide_row does not reach: lit, put with a 64-bit length, and span over the third sink, which records the
 * copy (the wave does it afterwards on the device; here the check does it) and advances by its length */
int check_other_members() {
  const uint8_t bytes[] = "0123456789abcdef";
  const char field[] = "ffeeddccbbaa0011";
  if (check("lit and put with a 64-bit length", "k0:i:0123456789abcdef\t", [&](auto &o) {
        GS_ROW_LIT(o, "k0:i:");
        o.put(bytes, (uint64_t)16);
        o.put(bytes, (uint64_t)0);
        o.ch('\t');
      }))
    return 1;
  auto emit = [&](auto &o) {
    GS_ROW_LIT(o, "of:H:");
    o.span(field, 16);
    o.ch('\n');
  };
  gs_row_count c;
  emit(c);
  std::vector<char> buf(GUARD + (size_t)c.n + GUARD, GUARD_BYTE);
  gs_row_write_span w;
  w.p = buf.data() + GUARD;
  emit(w);
  if (c.n != 22 || w.p != buf.data() + GUARD + 22 || w.sp_dst != buf.data() + GUARD + 5 || w.sp_src != field || w.sp_n != 16)
    return fail("span: what the sink recorded", std::to_string(w.sp_n), "16 bytes at offset 5");
  if (std::string(w.sp_dst, 16) != std::string(16, GUARD_BYTE)) return fail("span: the sink itself wrote into the span", "", "");
  memcpy(w.sp_dst, w.sp_src, (size_t)w.sp_n);
  const std::string got(buf.data(), buf.size()), want = std::string(GUARD, GUARD_BYTE) + "of:H:" + field + "\n" + std::string(GUARD, GUARD_BYTE);
  if (got != want) return fail("span", got, want);
  gs_row_write_span none; /* a row without a span leaves nothing for the wave */
  if (none.sp_n != 0 || none.sp_dst || none.sp_src) return fail("span: a fresh sink", "", "");
  checked++;
  return 0;
}

}  // namespace

int main() {
  if (check_other_members()) return 1;
  /* u64 */
  std::vector<uint64_t> values = {0, 9, 10, 0xFFFFFFFFull, 1ull << 32, ~0ull};
  for (uint64_t p = 10;; p *= 10) { /* 10 .. 10^19, with the number before each */
    values.push_back(p);
    values.push_back(p - 1);
    values.push_back(p + 1);
    if (p == 10000000000000000000ull) break;
  }
  for (uint64_t v : values)
    if (check_u64(v)) return 1;

  /* positions: the first and the last of every digit count 1 .. 10 */
  std::vector<uint32_t> positions;
  for (uint64_t lo = 1; lo <= 1000000000ull; lo *= 10) {
    positions.push_back((uint32_t)lo);
    positions.push_back((uint32_t)(lo * 10 - 1 > 0xFFFFFFFFull ? 0xFFFFFFFFull : lo * 10 - 1));
  }
  const std::string empty, g1 = "g", seq = "ACGTACGTACGTACGTACGT", pam = "NGG";
  const std::string prefixes[] = {empty, "chr_", std::string(200, 'p')};
  const std::string chrs[] = {"1", "chrUn_KI270302v1"};
  for (const std::string &prefix : prefixes)
    for (const std::string &chr : chrs)
      for (uint32_t pos : positions)
        for (char sense : {'+', '-'}) {
          /* the longest group name with which this id still has 254 bytes */
          const size_t rest = prefix.size() + 1 + chr.size() + 1 + std::to_string(pos).size() + 2;
          const std::string glong(254 - rest, 'G');
          const std::string *groups[] = {nullptr, &empty, &g1, &glong};
          for (const std::string *group : groups)
            if (check_guide(prefix, group, chr, pos, sense, seq, pam)) return 1;
        }
  /* no group: the chromosome name brings the id to 254 bytes; kmer and PAM lengths at their limits */
  if (check_guide(empty, nullptr, std::string(254 - 1 - 10 - 2, 'c'), 0xFFFFFFFFu, '-', std::string(64, 'T'), std::string(8, 'N'))) return 1;
  if (check_guide(empty, nullptr, "c", 1, '+', "A", "G")) return 1;
  printf("rowtext-check: %llu cases ok\n", (unsigned long long)checked);
  return 0;
}
