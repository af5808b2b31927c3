/* gs_bgzf_crc.h -- the CRC-32 of a BGZF member's bytes by one wave, shared by the compressor (gs_bgzf.hip) and the
 * inflater (gs_bgzf_inflate.hip): every lane folds a slice byte by byte, multiplies by x^(8 * bytes behind the slice)
 * (gb_crc_mul / gb_crc_shift of gs_bgzf_huff.h) and the wave XORs. */
#ifndef GS_BGZF_CRC_H
#define GS_BGZF_CRC_H

#include "gs_device.h"
#include "gs_bgzf_huff.h"

/* the byte table of the reflected polynomial into 256 words of LDS; the caller synchronises before gb_crc_wave */
__device__ __forceinline__ void gb_crc_table(uint32_t *s_crc) {
  for (uint32_t i = lane_id(); i < 256u; i += WAVE) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    s_crc[i] = c;
  }
}
/* CRC-32 of d[0, n), the same value in every lane */
__device__ __forceinline__ uint32_t gb_crc_wave(const uint8_t *d, uint32_t n, const uint32_t *s_crc) {
  const uint32_t lane = lane_id();
  const uint32_t slice = ((n + WAVE - 1u) / WAVE + 3u) & ~3u;
  const uint32_t b0 = lane * slice < n ? lane * slice : n, b1 = b0 + slice < n ? b0 + slice : n;
  uint32_t crc = lane == 0u ? 0xFFFFFFFFu : 0u;
  for (uint32_t i = b0; i < b1; i++) crc = s_crc[(crc ^ d[i]) & 255u] ^ (crc >> 8);
  crc = gb_crc_mul(gb_crc_shift(n - b1), crc);
  for (int o = 32; o >= 1; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o);
  return crc ^ 0xFFFFFFFFu;
}

#endif
