// blur_common.h -- the GaussianBlur arithmetic, single-source: the gfx950
// kernels (ffcv_blur.hip) and the host twins of the C ABI run the very same
// functions.
//
// Weights are float64 until the last step; pixels are float32 with every
// product and every sum rounded on its own, taps added in ascending order.
// A fused multiply-add or another order changes a handful of bytes per
// megapixel, so each product and each sum below is a statement of its own
// under `#pragma clang fp contract(off)` (the build also passes
// -ffp-contract=off).
#pragma once
#include <math.h>

#include "color_common.h"

#define FFCV_BLUR_MAX_K 31
#define FFCV_BLUR_WROW 32  // floats per sample in the weights array

FFCV_HD float blur_mul(float a, float b) {
#pragma clang fp contract(off)
  const float r = a * b;
  return r;
}
FFCV_HD float blur_add(float a, float b) {
#pragma clang fp contract(off)
  const float r = a + b;
  return r;
}

// reflect-101 of index i on an axis of n elements (-1 -> 1, n -> n - 2);
// |i| < n and i < 2 n - 1 here, so one reflection lands inside
FFCV_HD int blur_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

// uint8(clip(rint(acc), 0, 255)), rint rounding half to even
FFCV_HD uint32_t blur_round_u8(float acc) { return (uint32_t)sat_u8i(ffcv_f2i_rn(acc)); }

// e_j = exp(-0.5 (t t)), t = (j - (k - 1) / 2) / sigma, all float64
FFCV_HD double blur_e(int j, int ksize, double sigma) {
#pragma clang fp contract(off)
  const double x = (double)j - (double)(ksize - 1) / 2.0;
  const double t = x / sigma;
  const double tt = t * t;
  const double a = -0.5 * tt;
  return exp(a);
}

// The k float32 weights of one sample into w[0 .. 31] (entries from k on are
// 0).  e_j is computed twice, for the sum and for the quotient, so that no
// per-lane array is needed; both evaluations give the same value.  A weight
// whose float32 value would lie below 2^-126 is stored as +0: the double
// quotient is compared against 2^-126 - 2^-150, the smallest value that
// rounds (half to even) to 2^-126, so the conversion never meets a subnormal
// and the result does not depend on the denormal mode.
FFCV_HD void blur_weights(int ksize, double sigma, float *w) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int j = 0; j < ksize; j++) s = s + blur_e(j, ksize, sigma);
  for (int j = 0; j < FFCV_BLUR_WROW; j++) {
    float v = 0.f;
    if (j < ksize) {
      const double q = blur_e(j, ksize, sigma) / s;
      if (q >= 0x1p-126 - 0x1p-150) v = (float)q;
    }
    w[j] = v;
  }
}

// One sample's decision, sigma and weights (op id 11), drawn like colour
// jitter.  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_blur(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, double lo, double hi,
                       int ksize, uint8_t *apply, double *sigma, float *weights) {
  const int err = draw_color_jitter(k, id, loader_seed, epoch, 11, p, lo, hi, apply, sigma);
  blur_weights(ksize, sigma[k], weights + (uint64_t)k * FFCV_BLUR_WROW);
  return err;
}
