// jpeg_idct.h -- K1b of ffcv_jpeg.hip: the ifast IDCT and jpeg_idct_kernel.
#pragma once
#include "jpeg_defs.h"

// libjpeg post-IDCT range limit: table[x & 1023] (jdmaster.c)
FFCV_DEV uint8_t idct_rl(int x) {
  // table[x & 1023] = x+128 (x & 1023 < 128), 255 (< 512), 0 (< 896), x-896:
  // with u = (x + 128) & 1023 that is min(u, 255) below 640, else 0
  const uint32_t u = (uint32_t)(x + 128) & 1023u;
  return (uint8_t)(u >= 640u ? 0u : min(u, 255u));
}
// jidctfst.c MULTIPLY: DESCALE(var * const, CONST_BITS = 8) with a JLONG
// (64-bit) product.  The 32-bit form is identical whenever the product fits.
// Interval bounds through jpeg_idct_ifast with every dequantised input
// |d| <= M: pass-1 outputs <= 35.83 M (+ 5 from truncation), and the largest
// product is pass 2's (z10 + z12) * 473 <= 67,787 M, below 2^31 for
// M <= 31,680 (tools/idct_bound.py); the 32-bit form is used for M <= 30,000
// and WIDE keeps the exact 64-bit form for the rest.
template <bool WIDE>
FFCV_DEV int fmul8(int v, int c) {
  return WIDE ? (int)(((int64_t)v * c) >> 8) : (v * c) >> 8;
}

// jidctfst.c jpeg_idct_ifast on one dequantised block d (natural order),
// straight-line: the reference's all-zero-AC shortcuts produce the same
// values, so they are not taken (they would only diverge the wave).
template <bool WIDE>
FFCV_DEV void idct_ifast_block(int d[64], uint8_t *out, int stride) {
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int tmp0 = d[c], tmp1 = d[16 + c], tmp2 = d[32 + c], tmp3 = d[48 + c];
    int tmp10 = tmp0 + tmp2, tmp11 = tmp0 - tmp2;
    int tmp13 = tmp1 + tmp3, tmp12 = fmul8<WIDE>(tmp1 - tmp3, 362) - tmp13;
    tmp0 = tmp10 + tmp13;
    tmp3 = tmp10 - tmp13;
    tmp1 = tmp11 + tmp12;
    tmp2 = tmp11 - tmp12;
    int tmp4 = d[8 + c], tmp5 = d[24 + c], tmp6 = d[40 + c], tmp7 = d[56 + c];
    int z13 = tmp6 + tmp5, z10 = tmp6 - tmp5, z11 = tmp4 + tmp7, z12 = tmp4 - tmp7;
    tmp7 = z11 + z13;
    tmp11 = fmul8<WIDE>(z11 - z13, 362);
    int z5 = fmul8<WIDE>(z10 + z12, 473);
    tmp10 = fmul8<WIDE>(z12, 277) - z5;
    tmp12 = fmul8<WIDE>(z10, -669) + z5;
    tmp6 = tmp12 - tmp7;
    tmp5 = tmp11 - tmp6;
    tmp4 = tmp10 + tmp5;
    d[c] = tmp0 + tmp7;
    d[56 + c] = tmp0 - tmp7;
    d[8 + c] = tmp1 + tmp6;
    d[48 + c] = tmp1 - tmp6;
    d[16 + c] = tmp2 + tmp5;
    d[40 + c] = tmp2 - tmp5;
    d[32 + c] = tmp3 + tmp4;
    d[24 + c] = tmp3 - tmp4;
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int *w = d + 8 * r;
    int tmp10 = w[0] + w[4], tmp11 = w[0] - w[4];
    int tmp13 = w[2] + w[6], tmp12 = fmul8<WIDE>(w[2] - w[6], 362) - tmp13;
    int tmp0 = tmp10 + tmp13, tmp3 = tmp10 - tmp13, tmp1 = tmp11 + tmp12, tmp2 = tmp11 - tmp12;
    int z13 = w[5] + w[3], z10 = w[5] - w[3], z11 = w[1] + w[7], z12 = w[1] - w[7];
    int tmp7 = z11 + z13;
    tmp11 = fmul8<WIDE>(z11 - z13, 362);
    int z5 = fmul8<WIDE>(z10 + z12, 473);
    tmp10 = fmul8<WIDE>(z12, 277) - z5;
    tmp12 = fmul8<WIDE>(z10, -669) + z5;
    int tmp6 = tmp12 - tmp7, tmp5 = tmp11 - tmp6, tmp4 = tmp10 + tmp5;
    uint32_t o0 = idct_rl((tmp0 + tmp7) >> 5), o7 = idct_rl((tmp0 - tmp7) >> 5);
    uint32_t o1 = idct_rl((tmp1 + tmp6) >> 5), o6 = idct_rl((tmp1 - tmp6) >> 5);
    uint32_t o2 = idct_rl((tmp2 + tmp5) >> 5), o5 = idct_rl((tmp2 - tmp5) >> 5);
    uint32_t o4 = idct_rl((tmp3 + tmp4) >> 5), o3 = idct_rl((tmp3 - tmp4) >> 5);
    uint2 v;
    v.x = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
    v.y = o4 | (o5 << 8) | (o6 << 16) | (o7 << 24);
    *(uint2 *)(out + (uint64_t)r * stride) = v;
  }
}

// One block: load the zigzag coefficients at cp, de-zigzag +
// jidctfst.c DEQUANTIZE (int16 x int16 -> int) with the multipliers qm, and
// the ifast IDCT into out (stride bytes per row).
typedef int16_t s16x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// dc_add: added to the DC coefficient (slot 0) before dequantisation
FFCV_DEV void idct_block(const int16_t *cp, const int16_t *qm, int qmax, uint8_t *out, int stride, int dc_add) {
  int16_t zz[64];
  int d[64];
#pragma unroll
  for (int p8 = 0; p8 < 8; p8++) *(uint4 *)(zz + p8 * 8) = ((const uint4 *)cp)[p8];
  zz[0] = (int16_t)(zz[0] + dc_add);
  // max |AC coefficient| on packed halves (|-32768| reads as 32768
  // unsigned); max(|DC| * |qmul[0]|, max|AC| * max|AC qmul|) bounds every
  // dequantised input (the DC term is the large one: a bright block's DC
  // times the small DC multiplier), which selects the 32-bit IDCT products
  // when they are exact (see fmul8)
  u16x2 mu = {0, 0};
#pragma unroll
  for (int w = 0; w < 32; w++) {
    s16x2 v = *(const s16x2 *)(zz + 2 * w);
    if (w == 0) v.x = 0;  // the DC coefficient
    const s16x2 av = __builtin_elementwise_max(v, (s16x2){0, 0} - v);
    mu = __builtin_elementwise_max(mu, __builtin_bit_cast(u16x2, av));
  }
  const int cmax = max((int)mu.x, (int)mu.y);
  const int dc = zz[0], qdc = qm[0];
  const int bound = max(abs(dc) * abs(qdc), cmax * qmax);
#pragma unroll
  for (int n = 0; n < 64; n++) d[n] = (int)zz[kZigzagOfNatural[n]] * (int)qm[n];
  if (bound <= 30000)
    idct_ifast_block<false>(d, out, stride);
  else
    idct_ifast_block<true>(d, out, stride);
}

// ======================================================================= //
// K1b: DC prediction + de-zigzag + dequantise + ifast IDCT (jidctfst.c)   //
// ======================================================================= //
// One 256-thread workgroup per image; every thread IDCTs window blocks
// i = t, t + 256, ... into the window planes K2 reads.  The DC prediction
// (jdhuff.c last_dc_val) is done by K1's write pass as running sums per lane:
// the absolute DC of a block is its slot 0 plus the offset of the lane that
// started it (a 6-step search over the lanes' start blocks).
constexpr int K1B_T = 256;

__global__ void __launch_bounds__(K1B_T) jpeg_idct_kernel(JpegArgs a) {
  __shared__ ImgInfo L;  // this image's record (per-thread component lookups read LDS)
  const int k = blockIdx.x, t = threadIdx.x;
  const ImgInfo &G = a.info[k];
  if (G.status != FFCV_SAMPLE_OK) return;  // failed (K2 zero-fills) or raw (-1)
  static_assert(sizeof(ImgInfo) % 4 == 0, "ImgInfo copies as dwords");
  for (int i = t; i < (int)(sizeof(ImgInfo) / 4); i += K1B_T) ((uint32_t *)&L)[i] = ((const uint32_t *)&G)[i];
  __syncthreads();
  // K2's band records (RRC launches: brec_bands > 0), one thread per band,
  // from the record in LDS
  for (int b = t; b < a.brec_bands; b += K1B_T)
    k2_write_band_rec(a.brec + ((uint64_t)k * a.brec_bands + b), InfoGeom{L}, L.plan, a.p.out_w, a.p.out_h, b,
                      a.p.lut ? 1536 : 0, L.taps);
  int16_t *coef = (int16_t *)(a.arena + L.cf_off);
  uint8_t *planes = a.arena;
  int nbw[3];
#pragma unroll
  for (int c = 0; c < 3; c++) nbw[c] = c < L.ncomp ? (L.wx1[c] - L.wx0[c] + 1) * (L.wy1[c] - L.wy0[c] + 1) : 0;
  const int ntot = nbw[0] + nbw[1] + nbw[2];
  for (int i = t; i < ntot; i += K1B_T) {
    int c = 0, j = i;
    if (j >= nbw[0]) {
      j -= nbw[0];
      c = 1;
      if (j >= nbw[1]) {
        j -= nbw[1];
        c = 2;
      }
    }
    const int wbw = L.wx1[c] - L.wx0[c] + 1;
    const int by = L.wy0[c] + j / wbw, bx = L.wx0[c] + j % wbw;
    const int stride = wbw * 8;
    // block (c, bx, by) in MCU order, then the lane that started it: its
    // running DC sum in slot 0 plus that lane's offset is the absolute DC
    const int hs = L.hs[c], vs = L.vs[c];
    const int mx = bx / hs, my = by / vs, dx = bx - mx * hs, dy = by - my * vs;
    int ph = 0;
    for (int q = 0; q < L.bpm; q++)
      if (L.blk_comp[q] == c && L.blk_dx[q] == dx && L.blk_dy[q] == dy) ph = q;
    const uint32_t b = (uint32_t)((my * L.mcux + mx) * L.bpm + ph);
    int lane = 0;  // K1 wrote lane_blk0 / lane_off for its JT lanes only
#pragma unroll
    for (int st = JT / 2; st >= 1; st >>= 1)
      if (lane + st < JT && L.lane_blk0[lane + st] <= b) lane += st;
    idct_block(coef + (L.coff[c] + (uint64_t)j) * 64, L.qmul[c], L.qmax[c],
               planes + L.poff[c] + (uint64_t)by * 8 * stride + bx * 8, stride, L.lane_off[c][lane]);
  }
}
