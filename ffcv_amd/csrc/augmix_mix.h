// augmix_mix.h -- AugMix's mix, the one statement of its
// arithmetic for the host twin and the three kernels, and the 16-byte chunks
// the streaming kernels mix by.  Include it under the no-packed-fp32-ops
// attribute of its users.
#pragma once
#include "blur_common.h"
#include "lds_stage.h"

#define AM_MAX_WIDTH 4  // chains per image
#define AM_MAX_DEPTH 3  // steps per chain: chain i owns slots 3 i .. 3 i + 2 of RandAugment's arrays

// Per byte, in float32 with every product and sum rounded on its own:
// acc = w_0 x, then acc += w_{i+1} y_i chain after chain, then the byte.
FFCV_HD float augmix_first(float w, float x) { return blur_mul(w, x); }
FFCV_HD float augmix_add(float acc, float w, float y) { return blur_add(acc, blur_mul(w, y)); }
FFCV_HD uint32_t augmix_byte(float acc) { return (uint32_t)sat_u8i(ffcv_f2i_rn(acc)); }  // half to even, capped

// The 16 bytes from address a on, of which bytes [jlo, jhi) are wanted, from
// the one or two ALIGNED 16-byte chunks that hold a wanted byte (a chunk that
// holds none is not touched: it may lie in a page that is not ours).
FFCV_DEV lds_x4_t am_load16(uint64_t a, int jlo, int jhi) {
  const uint64_t a0 = a & ~(uint64_t)15;
  const glb_x4_t *p = (const glb_x4_t *)(uintptr_t)a0;
  lds_x4_t lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
  if (a + (uint64_t)jlo < a0 + 16u) lo = p[0];
  if (a + (uint64_t)jhi > a0 + 16u) hi = p[1];
  const uint32_t sh = (uint32_t)(a & 15), d = sh >> 2, r = sh & 3u;
  uint32_t w[9] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w, 0u};
  // by whole dwords (two selects), then by bytes
  if (d & 2u) {
#pragma unroll
    for (int i = 0; i < 7; i++) w[i] = w[i + 2];
  }
  if (d & 1u) {
#pragma unroll
    for (int i = 0; i < 5; i++) w[i] = w[i + 1];
  }
  lds_x4_t v;
  v.x = __builtin_amdgcn_alignbyte(w[1], w[0], r);
  v.y = __builtin_amdgcn_alignbyte(w[2], w[1], r);
  v.z = __builtin_amdgcn_alignbyte(w[3], w[2], r);
  v.w = __builtin_amdgcn_alignbyte(w[4], w[3], r);
  return v;
}

// 16 bytes of the original (first) or of a chain's result into the chunk's
// accumulators at weight w
FFCV_DEV void am_mix16(float (&acc)[16], bool first, float w, lds_x4_t v) {
  const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const float y = (float)((word[e >> 2] >> (8 * (e & 3))) & 0xffu);
    acc[e] = first ? augmix_first(w, y) : augmix_add(acc[e], w, y);
  }
}

// The chunk's rounded bytes [jlo, jhi) to the aligned chunk at gb: one 16-byte
// store when all are wanted, else byte by byte (the others are not ours).
FFCV_DEV void am_store16(uint8_t *gb, const float (&acc)[16], int jlo, int jhi) {
  if (jlo == 0 && jhi == 16) {
    lds_x4_t o;
    uint32_t word[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
      word[e] = augmix_byte(acc[4 * e]) | augmix_byte(acc[4 * e + 1]) << 8 | augmix_byte(acc[4 * e + 2]) << 16 |
                augmix_byte(acc[4 * e + 3]) << 24;
    o.x = word[0];
    o.y = word[1];
    o.z = word[2];
    o.w = word[3];
    *(glb_x4_t *)gb = o;
  } else {
#pragma unroll
    for (int e = 0; e < 16; e++)
      if (e >= jlo && e < jhi) gb[e] = (uint8_t)augmix_byte(acc[e]);
  }
}
