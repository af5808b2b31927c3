/* bgzf_inflate_check.cpp -- the host/device header of the BGZF inflater (csrc/gs_bgzf_inflate.h) as a stand-alone host
 * program, meant to be built with -fsanitize=address,undefined (make -C guidescan-cli_amd/csrc inflate-check) and linked
 * with host zlib.  Members made by deflate at levels 0, 1, 6 and 9, with Z_FIXED, and with a Z_FULL_FLUSH in the middle,
 * of text, zeros, a byte pattern of period 32,768 + 1 and random bytes: the header's output must equal inflate's.  Three
 * members of at most 300 bytes (stored, fixed, dynamic) with every single-byte replacement and every truncation, and
 * the fixed list of damaged members that tests/test_gpu_bgzf_inflate.py runs on the device: each must end in a reason
 * code or in output, in exactly sized heap arrays, so that a read or write outside them is reported.  Every member goes
 * through twice: with the whole stream as the window, and with the kernel's 1 KiB windows at every alignment (same
 * reason, same bytes, never GBI_ERR_WINDOW).  Exit status 0: every check held. */
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gs_bgzf_inflate.h"

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      fails++;                                        \
    }                                                 \
  } while (0)

typedef std::vector<uint8_t> bytes;

/* one BGZF member around the raw deflate stream of `raw` */
static bytes member_of(const bytes &raw, int level, int strategy, bool flush_mid) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) abort();
  bytes c(deflateBound(&zs, (uLong)raw.size()) + 64);
  zs.next_out = c.data();
  zs.avail_out = (uInt)c.size();
  static uint8_t none = 0;
  zs.next_in = raw.empty() ? &none : const_cast<uint8_t *>(raw.data());
  if (flush_mid) {
    zs.avail_in = (uInt)(raw.size() / 2);
    if (deflate(&zs, Z_FULL_FLUSH) != Z_OK) abort();
    zs.avail_in = (uInt)(raw.size() - raw.size() / 2);
  } else {
    zs.avail_in = (uInt)raw.size();
  }
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  const size_t clen = zs.total_out;
  deflateEnd(&zs);
  const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), raw.data() ? raw.data() : &none, (uInt)raw.size());
  const uint32_t size = (uint32_t)(18 + clen + 8), isize = (uint32_t)raw.size();
  if (size > 65536u) abort(); /* BSIZE has 16 bits */
  bytes m = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)((size - 1) & 255), (uint8_t)((size - 1) >> 8)};
  m.insert(m.end(), c.begin(), c.begin() + (long)clen);
  for (int k = 0; k < 4; k++) m.push_back((uint8_t)(crc >> (8 * k)));
  for (int k = 0; k < 4; k++) m.push_back((uint8_t)(isize >> (8 * k)));
  return m;
}

/* The stream through gbi_step the way k_bgzf_inflate drives it: before every step a window of 1,024 bytes, copied
 * into a heap array of exactly that size, that begins at the 16-byte boundary at or before the next bits' byte when the
 * stream itself lies `mis` bytes behind such a boundary (so lo may be negative); what the window holds outside the stream
 * is other data (0xA5 here).  A read outside the window would be GBI_ERR_WINDOW, one outside the array is the sanitizer's. */
static uint32_t windowed_member(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t isize, gbi_work *w, uint32_t mis, uint32_t *out_len) {
  const int32_t WIN = 1024;
  gbi_state s;
  gbi_state_init(&s);
  uint32_t tok[GBI_TOKENS], ntok = 0;
  *out_len = 0;
  for (uint64_t guard = 0; guard < 8ull * len + 8ull && s.mode != GBI_MODE_DONE; guard++) {
    const int32_t bytepos = (int32_t)(s.bitpos >> 3);
    const int32_t lo = bytepos - (int32_t)((mis + (uint32_t)bytepos) & 15u);
    uint8_t *win = (uint8_t *)malloc((size_t)WIN);
    for (int32_t i = 0; i < WIN; i++) win[i] = lo + i >= 0 && lo + i < (int32_t)len ? in[lo + i] : 0xA5;
    const uint32_t at = s.outpos;
    const uint32_t rc = gbi_step(&s, w, win, lo, (uint32_t)WIN, len, isize, tok, &ntok);
    free(win);
    if (rc) return rc;
    gbi_apply(out, at, in, &s, tok, ntok);
    *out_len = s.outpos;
  }
  return s.mode == GBI_MODE_DONE ? GBI_OK : GBI_ERR_WINDOW;
}

static uint32_t g_mis = 0; /* the next stream's place behind a 16-byte boundary: every member takes another */

/* a member through the header, every array sized exactly -> the reason; out: what it made */
static uint32_t run_member(const bytes &member, bytes &out) {
  out.clear();
  uint8_t *copy = (uint8_t *)malloc(member.size() ? member.size() : 1); /* exactly the member: no slack behind it */
  if (!member.empty()) memcpy(copy, member.data(), member.size());
  gbi_member gm;
  uint32_t rc = gbi_walk_member(copy, member.size(), &gm);
  if (rc == GBI_OK) {
    uint8_t *stream = (uint8_t *)malloc(gm.clen ? gm.clen : 1);
    memcpy(stream, copy + gm.cdata_off, gm.clen);
    uint8_t *o = (uint8_t *)malloc(gm.isize ? gm.isize : 1);
    gbi_work *w = (gbi_work *)malloc(sizeof(gbi_work));
    uint32_t n = 0;
    rc = gbi_inflate_member(stream, gm.clen, o, gm.isize, w, &n);
    CHECK(n <= gm.isize);
    { /* the kernel's windows give the same reason and the same bytes */
      uint8_t *o2 = (uint8_t *)malloc(gm.isize ? gm.isize : 1);
      uint32_t n2 = 0;
      const uint32_t rc2 = windowed_member(stream, gm.clen, o2, gm.isize, w, g_mis++ & 15u, &n2);
      CHECK(rc2 != GBI_ERR_WINDOW);
      CHECK(rc2 == rc && n2 == n && (n == 0 || !memcmp(o, o2, n)));
      free(o2);
    }
    if (rc == GBI_OK) {
      CHECK(n == gm.isize);
      out.assign(o, o + n);
      if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), o, n) != gm.crc) rc = GBI_ERR_CRC;
    }
    free(w);
    free(o);
    free(stream);
  }
  free(copy);
  CHECK(rc < GBI_N_REASONS);
  CHECK(rc != GBI_ERR_WINDOW); /* the host's window is the whole stream */
  return rc;
}

/* the same member through host zlib (gzip wrapper) */
static bool zlib_member(const bytes &member, bytes &out) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 15 + 16) != Z_OK) abort();
  out.assign(GBI_MAX_OUT + 1, 0);
  zs.next_in = const_cast<uint8_t *>(member.data());
  zs.avail_in = (uInt)member.size();
  zs.next_out = out.data();
  zs.avail_out = (uInt)out.size();
  const int rc = inflate(&zs, Z_FINISH);
  out.resize(zs.total_out);
  inflateEnd(&zs);
  return rc == Z_STREAM_END;
}

static void equal_to_zlib(const bytes &raw, int level, int strategy, bool flush_mid) {
  const bytes m = member_of(raw, level, strategy, flush_mid);
  bytes mine, theirs;
  const uint32_t rc = run_member(m, mine);
  if (rc != GBI_OK) fprintf(stderr, "%zu bytes, level %d, strategy %d, flush %d: reason %u (%s)\n", raw.size(), level, strategy, (int)flush_mid, rc, gbi_reason_string(rc));
  CHECK(rc == GBI_OK);
  CHECK(zlib_member(m, theirs));
  CHECK(mine == theirs);
  CHECK(mine == raw);
}

static void damage(const bytes &m, const char *what, unsigned want_type) {
  CHECK(m.size() <= 300 + 26);
  CHECK(((m[18] >> 1) & 3u) == want_type);
  bytes out;
  CHECK(run_member(m, out) == GBI_OK);
  unsigned long refused = 0, taken = 0;
  for (size_t i = 0; i < m.size(); i++)
    for (unsigned v = 0; v < 256; v++) {
      if (v == m[i]) continue;
      bytes d = m;
      d[i] = (uint8_t)v;
      (run_member(d, out) == GBI_OK ? taken : refused)++;
    }
  for (size_t n = 0; n < m.size(); n++) {
    bytes d(m.begin(), m.begin() + (long)n);
    CHECK(run_member(d, out) != GBI_OK);
    refused++;
  }
  printf("%s member of %zu bytes: %lu damaged forms refused, %lu still a sound member\n", what, m.size(), refused, taken);
}

static bytes from_hex(const char *h) {
  bytes b;
  for (; h[0] && h[1]; h += 2) {
    char t[3] = {h[0], h[1], 0};
    b.push_back((uint8_t)strtoul(t, nullptr, 16));
  }
  return b;
}

int main(int argc, char **argv) {
  uint32_t seed = 12345;
  auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u, seed >> 8; };
  std::vector<bytes> inputs;
  {
    bytes text;
    const char *words[] = {"guide", "scan", "off-target", "ACGTTGCA", "NGG", "0123456789abcdef", "\t", "\n"};
    while (text.size() < 60000) {
      const char *w = words[rnd() % 8];
      text.insert(text.end(), w, w + strlen(w));
    }
    inputs.push_back(text);
    inputs.push_back(bytes(65536, 0));
    bytes period(65536);
    for (size_t i = 0; i < 32769 && i < period.size(); i++) period[i] = (uint8_t)"0123456789abcdef"[rnd() & 15]; /* (bytes of any value would not fit a member) */
    for (size_t i = 32769; i < period.size(); i++) period[i] = period[i - 32769];
    inputs.push_back(period);
    bytes random(0xff00);
    for (auto &b : random) b = (uint8_t)(rnd() & 255);
    inputs.push_back(random);
    inputs.push_back(bytes());
    inputs.push_back(bytes(1, 'x'));
    bytes skew; /* Fibonacci-like counts (each the two before it and one more): codes of 15 bits */
    uint32_t a = 1, b = 2;
    for (int s = 0; s < 17; s++) {
      skew.insert(skew.end(), a, (uint8_t)('A' + s));
      const uint32_t c = a + b + 1;
      a = b;
      b = c;
    }
    for (size_t i = skew.size(); i > 1; i--) std::swap(skew[i - 1], skew[rnd() % i]);
    inputs.push_back(skew);
  }
  for (const bytes &raw : inputs) {
    const bytes fits(raw.begin(), raw.begin() + (long)std::min<size_t>(raw.size(), 0xff00)); /* what a stored member holds */
    equal_to_zlib(fits, 0, Z_DEFAULT_STRATEGY, false);
    equal_to_zlib(fits, 0, Z_DEFAULT_STRATEGY, true);
    for (int level : {1, 6, 9}) equal_to_zlib(raw, level, Z_DEFAULT_STRATEGY, false);
    equal_to_zlib(raw, 6, Z_FIXED, false);
    equal_to_zlib(raw, 6, Z_DEFAULT_STRATEGY, true);
    equal_to_zlib(bytes(fits.begin(), fits.begin() + (long)std::min<size_t>(fits.size(), 0x8000)), 6, Z_HUFFMAN_ONLY, true); /* no matches */
  }

  bytes small_text, small_acgt;
  for (const char *p = "the quick brown fox jumps over the lazy dog; the lazy dog sleeps, the quick fox jumps again and again"; *p; p++)
    small_text.push_back((uint8_t)*p);
  for (int i = 0; i < 800; i++) small_acgt.push_back((uint8_t)"ACGT"[rnd() & 3]);
  damage(member_of(small_text, 0, Z_DEFAULT_STRATEGY, false), "stored", 0);
  damage(member_of(small_text, 6, Z_FIXED, false), "fixed", 1);
  damage(member_of(small_acgt, 6, Z_DEFAULT_STRATEGY, false), "dynamic", 2);

  /* the damaged members the device test runs (tests/test_gpu_bgzf_inflate.py), with the reason each must give: lines of
   * `reason hex-bytes name` */
  unsigned listed = 0;
  if (FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr) {
    char line[4096], hex[4096], name[256];
    unsigned reason;
    while (fgets(line, sizeof line, f)) {
      if (line[0] == '#' || sscanf(line, "%u %4095s %255s", &reason, hex, name) != 3) continue;
      bytes out;
      const uint32_t rc = run_member(from_hex(hex), out);
      if (rc != reason) fprintf(stderr, "listed member %s: reason %u, expected %u\n", name, rc, reason);
      CHECK(rc == reason);
      listed++;
    }
    fclose(f);
  }
  CHECK(argc < 2 || listed >= 6);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("bgzf_inflate_check: ok (%u listed damaged members)\n", listed);
  return 0;
}
