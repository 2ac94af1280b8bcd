// sharpness_common.h -- the RandomAdjustSharpness arithmetic, single-source:
// the gfx950 kernel (ffcv_sharpness.hip) and the host twins of the C ABI run
// the very same functions.
//
// Pillow's ImageEnhance.Sharpness: blend(smooth(image), image, factor), all in
// float32 with every product, difference and sum rounded on its own (the
// helpers of blur_common.h, which do not depend on -ffp-contract).
#pragma once
#include "blur_common.h"

// ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13, the quotients in float32
#define SHARP_W1 (1.0f / 13.0f)
#define SHARP_W5 (5.0f / 13.0f)

FFCV_HD float sharp_sub(float a, float b) {
#pragma clang fp contract(off)
  const float r = a - b;
  return r;
}

// the sum of one row's three products, left to right
FFCV_HD float sharp_row(float p0, float p1, float p2) { return blur_add(blur_add(p0, p1), p2); }

// The smoothed byte, as a float, from the three row sums, top row first:
// 0.5 + top + centre + bottom, clamped to [0, 255], truncated.
FFCV_HD float sharp_smooth(float top, float mid, float bot) {
  float s = blur_add(0.5f, top);
  s = blur_add(s, mid);
  s = blur_add(s, bot);
  s = s < 0.f ? 0.f : s;
  s = s > 255.f ? 255.f : s;
  return (float)(int32_t)s;
}

// Image.blend(smooth, image, factor) of one byte: d + a (i - d), clamped to
// [0, 255], truncated.  For 0 <= a <= 1 the sum lies between d and i, so the
// clamp is Pillow's plain conversion there.  A border byte has d == i and
// comes out as i at every finite a.  (A NaN gives 0.)
FFCV_HD uint32_t sharp_blend(float a, float d, float i) {
  float t = blur_add(d, blur_mul(a, sharp_sub(i, d)));
  t = !(t > 0.f) ? 0.f : t;
  t = t > 255.f ? 255.f : t;
  return (uint32_t)(int32_t)t;
}

// One sample's decision (op id 19): rand() < p; the factor is the constant.
// Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_sharpness(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, float factor,
                            uint8_t *apply, float *factor_out) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, 19));
  apply[k] = (uint8_t)(mt_double(m) < p);
  factor_out[k] = factor;
  return m.err;
}
