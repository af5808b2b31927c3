/* bgzf_huff_check.cpp -- the host/device header of the BGZF compressor (csrc/gs_bgzf_huff.h) as a stand-alone host
 * program, meant to be built with -fsanitize=address,undefined (make -C guidescan-cli_amd/csrc huff-check): the
 * code-length builder over the histograms of tests/test_bgzf_model.py with exactly sized heap arrays, the canonical codes,
 * the symbol maps over every length and distance, the CRC arithmetic against the bytewise loop, and the sp:f conversion
 * over every q against strtof of the printed decimals.  Exit status 0: every check held. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gs_bgzf_huff.h"

static int fails = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
      fails++;                                             \
    }                                                      \
  } while (0)

static void run(const std::vector<uint32_t> &freq, uint32_t max_len) {
  const uint32_t n = (uint32_t)freq.size();
  std::vector<uint8_t> len(n);
  std::vector<uint32_t> work(n); /* n words exactly: an access beyond them is reported */
  std::vector<uint16_t> code(n);
  uint32_t used = 0;
  for (uint32_t f : freq) used += f != 0;
  const int rc = gb_huffman_lengths(freq.data(), n, max_len, len.data(), work.data());
  if (used > (1u << max_len)) {
    CHECK(rc == 1);
    return;
  }
  CHECK(rc == 0);
  unsigned long long kraft = 0;
  for (uint32_t i = 0; i < n; i++) {
    CHECK((len[i] != 0) == (freq[i] != 0));
    CHECK(len[i] <= max_len);
    if (len[i]) kraft += 1ull << (max_len - len[i]);
  }
  if (used == 1) CHECK(kraft == 1ull << (max_len - 1));
  if (used > 1) CHECK(kraft == 1ull << max_len);
  gb_codes(len.data(), n, code.data());
  for (uint32_t i = 0; i < n; i++) CHECK(len[i] == 0 ? code[i] == 0 : code[i] < (1u << len[i]));
}

int main() {
  std::vector<uint32_t> one(286, 0), two(286, 0), equal(286, 100), but_one(286, 0), fib(286, 0);
  one[65] = 1000;
  two[0] = 7;
  two[256] = 1;
  but_one[285] = 3;
  fib[0] = 1;
  fib[1] = 2;
  for (int i = 2; i < 20; i++) fib[i] = fib[i - 1] + fib[i - 2] + 1;
  fib[256] = 1;
  for (uint32_t max_len : {15u, 7u})
    for (const auto *h : {&one, &two, &equal, &but_one, &fib}) run(*h, max_len);
  run(std::vector<uint32_t>(30, 0), 15); /* no distance code at all */
  run(std::vector<uint32_t>(288, 1), 15);

  /* a whole plan */
  {
    std::vector<uint32_t> ll(GB_NLL, 3), d(GB_ND, 0), work(GB_MAX_SYMS);
    d[7] = 5;
    gb_plan *p = new gb_plan;
    gb_make_plan(ll.data(), d.data(), p, work.data());
    CHECK(p->hlit == 286 && p->hdist == 8 && p->d_len[7] == 1 && p->bits > 0);
    delete p;
  }
  /* symbol maps: every length and distance lands in its code's range */
  {
    static const uint32_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    for (uint32_t l = 3; l <= 258; l++) {
      uint32_t eb, ev;
      const uint32_t s = gb_len_sym(l, &eb, &ev);
      CHECK(s >= 257 && s <= 285 && eb == gb_len_extra(s) && lbase[s - 257] + ev == l && ev < (1u << eb));
    }
    uint32_t dbase[30];
    for (uint32_t s = 0, b = 1; s < 30; s++) {
      dbase[s] = b;
      b += 1u << gb_dist_extra(s);
    }
    for (uint32_t dist = 1; dist <= 32768; dist++) {
      uint32_t eb, ev;
      const uint32_t s = gb_dist_sym(dist, &eb, &ev);
      CHECK(s < 30 && eb == gb_dist_extra(s) && dbase[s] + ev == dist && ev < (1u << eb));
    }
    for (uint32_t i = 0; i < 19; i++) CHECK(gb_clc_order(i) < 19);
  }
  /* CRC-32 of a || b from the parts */
  {
    std::vector<uint8_t> m(1000);
    for (size_t i = 0; i < m.size(); i++) m[i] = (uint8_t)(i * 131u + 7u);
    auto raw = [&](uint32_t c, size_t b, size_t e) {
      for (size_t i = b; i < e; i++) {
        c ^= m[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
      }
      return c;
    };
    const uint32_t whole = raw(0xFFFFFFFFu, 0, 1000);
    for (size_t cut : {(size_t)0, (size_t)1, (size_t)333, (size_t)999, (size_t)1000})
      CHECK((gb_crc_mul(gb_crc_shift((uint32_t)(1000 - cut)), raw(0xFFFFFFFFu, 0, cut)) ^ raw(0u, cut, 1000)) == whole);
  }
  /* sp:f: every q against strtof of the text a SAM line prints */
  for (uint32_t q = 0; q <= 1000000u; q++) {
    char txt[16];
    snprintf(txt, sizeof txt, "%u.%06u", q / 1000000u, q % 1000000u);
    const float f = strtof(txt, nullptr);
    uint32_t bits;
    memcpy(&bits, &f, 4);
    if (gb_sp_float_bits(q) != bits) {
      CHECK(gb_sp_float_bits(q) == bits);
      break;
    }
  }
  printf(fails ? "FAILED: %d checks\n" : "ok%.0d\n", fails);
  return fails ? 1 : 0;
}
