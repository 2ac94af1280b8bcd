// color_common.h -- the colour-jitter pixel arithmetic, single-source: the
// gfx950 kernels (ffcv_color.hip) and the host twin of the C ABI run the very
// same functions.
//
// The reference (color_jitter.py) computes in float64 through numpy, which
// rounds every multiply and every add on its own.  A fused multiply-add
// changes the truncated gray value of 276 of the 2^24 RGB triples, so each
// product and each sum below is a statement of its own under
// `#pragma clang fp contract(off)` (the build also passes -ffp-contract=off).
#pragma once
#include "device_common.h"

FFCV_HD double cj_mul(double a, double b) {
#pragma clang fp contract(off)
  const double r = a * b;
  return r;
}
FFCV_HD double cj_add(double a, double b) {
#pragma clang fp contract(off)
  const double r = a + b;
  return r;
}

// color_jitter.py:85 / :127: (0.2989 * r + 0.587 * g + 0.114 * b).astype(uint8), left to right
FFCV_HD uint32_t cj_gray(uint32_t r, uint32_t g, uint32_t b) {
  const double pr = cj_mul(0.2989, (double)r);
  const double pg = cj_mul(0.587, (double)g);
  const double pb = cj_mul(0.114, (double)b);
  const double rg = cj_add(pr, pg);
  const double s = cj_add(rg, pb);
  return (uint32_t)(int32_t)s;  // 0 <= s < 255: truncation
}

// color_jitter.py:38 blend: (ratio * v + (1 - ratio) * other).clip(0, 255).astype(uint8);
// omr = 1 - ratio (cj_one_minus), computed once per image like numpy's scalar
FFCV_HD double cj_one_minus(double ratio) {
#pragma clang fp contract(off)
  const double r = 1.0 - ratio;
  return r;
}
FFCV_HD uint32_t cj_blend(double ratio, double omr, uint32_t v, double other) {
  const double a = cj_mul(ratio, (double)v);
  const double b = cj_mul(omr, other);
  double z = cj_add(a, b);
  z = z < 0.0 ? 0.0 : z;
  z = z > 255.0 ? 255.0 : z;
  return (uint32_t)(int32_t)z;
}

// RandomSolarization's table entry: v >= threshold ? 255 - v : v, the integer
// threshold in [0, 256] carried as the step's float64 ratio
FFCV_HD uint32_t cj_solarize(double threshold, uint32_t v) { return (double)v >= threshold ? 255u - v : v; }

// color_jitter.py:86: l_img.mean() = float64(sum of the uint8 gray image) / float64(H * W);
// the sum is an integer below 2^53, exact in any order
FFCV_HD double cj_mean(uint64_t gray_sum, uint64_t pixels) { return (double)gray_sum / (double)pixels; }

// One sample's decisions (color_jitter.py:40-41 and twins): rand() < p, then
// uniform(lo, hi), from the sample's own stream (op id 5 brightness, 6
// contrast, 7 saturation).  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_color_jitter(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, uint32_t op_id, double p,
                               double lo, double hi, uint8_t *apply, double *ratio) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, op_id));
  apply[k] = (uint8_t)(mt_double(m) < p);
  ratio[k] = mt_uniform(m, lo, hi);
  return m.err;
}
