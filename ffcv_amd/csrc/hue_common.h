// hue_common.h -- the hue shift of one pixel and the draws of RandomHue and
// RandomColorJitter, single-source: the gfx950 kernels
// (ffcv_hue.hip) and the host twin of the C ABI run the very same functions.
//
// The contract is float32 arithmetic that numpy reproduces bit for bit: every
// product, sum and quotient is rounded on its own.  A fused multiply-add in
// 1 - s * f or 1 - s * (1 - f) changes 87,959 of the 2^24 RGB triples at
// d = 0.05, so each operation below is a statement of its own under
// `#pragma clang fp contract(off)` (the build also passes -ffp-contract=off),
// and the two divisions are the plain `/`: correctly rounded IEEE under the
// build's -fno-fast-math, never a reciprocal multiply.
#pragma once
#include "device_common.h"

// D of an image from its drawn d: float32(float64(6) * d)
FFCV_HD float hue_shift6(double d) {
#pragma clang fp contract(off)
  const double d6 = 6.0 * d;
  return (float)d6;
}

// r, g, b in 0..255, D = hue_shift6(d) with |d| <= 0.5.  Returns R | G << 8 | B << 16.
FFCV_HD uint32_t hue_pixel(uint32_t r, uint32_t g, uint32_t b, float D) {
#pragma clang fp contract(off)
  const uint32_t mx = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const uint32_t mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const int c = (int)(mx - mn);
  if (c == 0) return r | (g << 8) | (b << 16);  // gray: no hue to turn
  const float C = (float)c;
  const float V = (float)mx;
  const int ri = (int)r, gi = (int)g, bi = (int)b;
  int num = ri - gi;
  float base = 4.0f;
  if (mx == r) {
    num = gi - bi;
    base = 0.0f;
  } else if (mx == g) {
    num = bi - ri;
    base = 2.0f;
  }
  const float h = (float)num / C;
  float x = base + h;
  x = x + D;
  const float xp = x + 6.0f;
  x = x < 0.0f ? xp : x;
  const float xm = x - 6.0f;
  x = x >= 6.0f ? xm : x;  // after the wrap up: a tiny negative x became 6.0 there
  const int i = (int)x;    // 0 <= x < 6: truncation is floor
  const float f = x - (float)i;
  const float s = C / V;
  const float oms = 1.0f - s;
  const float P = V * oms;
  const float sf = s * f;
  const float omsf = 1.0f - sf;
  const float Q = V * omsf;
  const float omf = 1.0f - f;
  const float somf = s * omf;
  const float omsomf = 1.0f - somf;
  const float T = V * omsomf;
  // (R, G, B) of sector i: (V,T,P) (Q,V,P) (P,V,T) (P,Q,V) (T,P,V) (V,P,Q)
  const float R = i == 0 || i >= 5 ? V : (i == 1 ? Q : (i == 4 ? T : P));
  const float G = i == 1 || i == 2 ? V : (i == 0 ? T : (i == 3 ? Q : P));
  const float B = i == 3 || i == 4 ? V : (i == 2 ? T : (i >= 5 ? Q : P));
  // values in [0, mx]: rint (half to even), no clip
  return (uint32_t)ffcv_f2i_rn(R) | ((uint32_t)ffcv_f2i_rn(G) << 8) | ((uint32_t)ffcv_f2i_rn(B) << 16);
}

// RandomHue's decisions of one sample (op id 12): rand() < p, then
// uniform(-magnitude, magnitude).  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_hue(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, double magnitude,
                     uint8_t *apply, double *shift) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, 12));
  apply[k] = (uint8_t)(mt_double(m) < p);
  shift[k] = mt_uniform(m, -magnitude, magnitude);
  return m.err;
}

// RandomColorJitter's five draws of one sample from one stream (op id 13):
// rand() < p, then uniform(lo[j], hi[j]) for brightness, contrast, saturation
// and hue, always all five.  Component j lands in row row[j] of apply / ratio
// ([rows][B]; row[j] < 0: drawn and dropped); the apply rows all carry the one
// decision.
struct JointDraw {
  double lo[4], hi[4];
  int row[4];
};
FFCV_HD int draw_color_jitter_joint(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p,
                                    const JointDraw &jd, uint8_t *apply, double *ratio) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, 13));
  const uint8_t a = (uint8_t)(mt_double(m) < p);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double v = mt_uniform(m, jd.lo[j], jd.hi[j]);
    if (jd.row[j] >= 0) {
      apply[(uint64_t)jd.row[j] * B + k] = a;
      ratio[(uint64_t)jd.row[j] * B + k] = v;
    }
  }
  return m.err;
}
