// elastic_common.h -- the ElasticTransform arithmetic, single-source: the
// gfx950 kernel (ffcv_elastic.hip) and the host twin of the C ABI run the very
// same functions.  Everything behind the weight table is
// integer arithmetic.
#pragma once
#include <math.h>

#include "affine_common.h"

#define ELASTIC_OP 27         // seeding contract: the noise key
#define ELASTIC_MAX_R 64      // largest blur radius
#define ELASTIC_MAX_ALPHA 4096

// A sample's noise key: the contract's hash of op id 27, all 64 bits.
FFCV_HD uint64_t elastic_key(uint64_t loader_seed, uint64_t epoch, uint64_t sample) {
  uint64_t h = splitmix64(loader_seed ^ ((uint64_t)ELASTIC_OP << 56));
  h = splitmix64(h ^ epoch);
  return splitmix64(h ^ sample);
}

// The hash word of pixels 2 q and 2 q + 1 (index inside the image, r W + c):
// element e = 2 (r W + c) + axis takes bits [16 (e & 3), 16 (e & 3) + 16) of
// splitmix64(key ^ (e >> 2)), less 32768: Q15 of [-1, 1).
FFCV_HD uint64_t elastic_word(uint64_t key, uint64_t q) { return splitmix64(key ^ q); }
FFCV_HD int elastic_noise(uint64_t word, uint32_t pixel, int axis) {
  return (int)((word >> (16 * (2 * (pixel & 1u) + axis))) & 0xFFFFu) - 32768;
}

// torch's `reflect` border for -n < i < 2 n - 1
FFCV_HD int elastic_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// Q16 of a horizontal sum; the displacement, Q16 pixels, of a vertical one
FFCV_HD int elastic_h16(int h) { return (h + 32768) >> 16; }
FFCV_HD int elastic_disp(int amp, int v) { return (int)(((int64_t)amp * v + ((int64_t)1 << 22)) >> 23); }

// The blur of one launch: R, amp = round(128 alpha), the weights w[0 .. R] of
// |offset|, and the same weights as the int16 pairs the packed dot product
// takes.  Tap k = 0 .. 2 R (offset k - R) of an output at an EVEN position of
// the pair grid is half k & 1 of pair k >> 1; at an ODD position, the same
// pairs serve with the taps moved up by one: even[m] = (W[2m], W[2m+1]),
// odd[m] = (W[2m-1], W[2m]), W outside 0 .. 2 R being 0.
struct ElasticBlur {
  int R, amp;
  uint32_t even[ELASTIC_MAX_R + 1], odd[ELASTIC_MAX_R + 1];
  FFCV_HD int w(int k) const {  // tap k of 0 .. 2 R
    const uint32_t p = even[k >> 1];
    return (int)((k & 1) ? p >> 16 : p & 0xFFFFu);
  }
};

// false: sigma or alpha outside what the arithmetic carries
static inline bool elastic_blur(double alpha, double sigma, ElasticBlur *b) {
  if (!(sigma >= 1.0) || !(sigma <= (2 * ELASTIC_MAX_R + 1) / 8.0) || !(alpha >= 0.0 && alpha <= ELASTIC_MAX_ALPHA))
    return false;
  int k = (int)(8.0 * sigma + 1.0);
  k += (k % 2 == 0);
  const int R = (k - 1) / 2;
  if (R > ELASTIC_MAX_R) return false;
  double g[ELASTIC_MAX_R + 1], sum = 0.0;
  for (int i = 0; i <= R; i++) {
    const double x = (double)i / sigma;
    g[i] = exp(-0.5 * (x * x));
  }
  for (int i = -R; i <= R; i++) sum += g[i < 0 ? -i : i];
  int64_t w[ELASTIC_MAX_R + 1], total = 0;
  for (int i = 0; i <= R; i++) {
    w[i] = (int64_t)floor(65536.0 * g[i] / sum + 0.5);
    total += i ? 2 * w[i] : w[i];
  }
  w[0] += 65536 - total;  // sigma >= 1: at most 26,145, an int16 like the others
  b->R = R;
  b->amp = (int)floor(alpha * 128.0 + 0.5);
  for (int m = 0; m <= R; m++) {
    const auto W = [&](int t) -> uint32_t { return t < 0 || t > 2 * R ? 0u : (uint32_t)w[t < R ? R - t : t - R]; };
    b->even[m] = W(2 * m) | (W(2 * m + 1) << 16);
    b->odd[m] = W(2 * m - 1) | (W(2 * m) << 16);
  }
  return true;
}

// The tap a pixel's footprint is measured by: the column (row) of the first
// tap of coordinate X, held to [-1, n]: beyond that every tap takes fill.
FFCV_HD int elastic_tap(int mode, int64_t X, int n) {
  const int64_t i = (X + (mode == FFCV_AFFINE_NEAREST ? 32768 : 0)) >> 16;
  return (int)(i < -1 ? -1 : (i > n ? n : i));
}

// The source box of a tile from the extremes of elastic_tap over its pixels:
// widened by bilinear's row and column, clipped to the image.
FFCV_HD AffineBox elastic_box(int mode, int H, int W, int ixmin, int ixmax, int iymin, int iymax) {
  const int wide = mode == FFCV_AFFINE_NEAREST ? 1 : 2;
  AffineBox b;
  b.cl = ixmin < 0 ? 0 : ixmin;
  b.ch = ixmax + wide > W ? W : ixmax + wide;
  b.lo = iymin < 0 ? 0 : iymin;
  b.hi = iymax + wide > H ? H : iymax + wide;
  b.fits32 = true;
  b.X0 = b.Y0 = 0;
  return b;
}
