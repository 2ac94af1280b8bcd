// tone_common.h -- the table steps RandomPosterize / RandomAutocontrast /
// RandomEqualize / RandomInvert, single-source: the gfx950
// kernels (ffcv_tone.hip) and the host twin of the C ABI run the very same
// functions.
//
// Every step is a 256-entry byte table per channel, out = T[in].  Invert and
// posterize are fixed tables; autocontrast's depends on the channel's first and
// last occupied bin, equalize's on the channel's histogram (Pillow's
// ImageOps.autocontrast with cutoff 0 and ImageOps.equalize without a mask).
// All of it is integer arithmetic but autocontrast's float64 scale: an IEEE
// division, then a product and a sum each rounded on its own (cj_mul / cj_add)
// and a truncation toward zero, like Python's int(ix * scale + offset).
#pragma once
#include "color_common.h"

// ImageOps.invert
FFCV_HD uint32_t tone_invert(uint32_t v) { return 255u - v; }

// ImageOps.posterize: v & ~(2 ** (8 - bits) - 1), bits in [1, 8]
FFCV_HD uint32_t tone_posterize(int bits, uint32_t v) { return v & (0xffu & ~((1u << (8 - bits)) - 1u)); }

// ImageOps.autocontrast: lo / hi the first / last occupied bin of the channel
FFCV_HD uint32_t tone_autocontrast(uint32_t lo, uint32_t hi, uint32_t v) {
  if (hi <= lo) return v;
  const double scale = 255.0 / (double)(int32_t)(hi - lo);
  const double offset = cj_mul(-(double)(int32_t)lo, scale);
  const double z = cj_add(cj_mul((double)(int32_t)v, scale), offset);  // |z| <= 255 * 255
  const int32_t i = (int32_t)z;                                        // toward zero
  return (uint32_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

// ImageOps.equalize: step = (sum(h) - h[last occupied bin]) // 255, or 0 (the
// identity) when fewer than two bins are occupied.  Every channel's
// histogram sums to the image's pixels, before and after any table step.
FFCV_HD uint32_t tone_equalize_step(uint32_t pixels, uint32_t lo, uint32_t hi, uint32_t h_hi) {
  return hi <= lo ? 0u : (pixels - h_hi) / 255u;
}
// below = sum(h[:v]); pixels < 2^30, so step / 2 + below fits 32 bits
FFCV_HD uint32_t tone_equalize(uint32_t step, uint32_t below, uint32_t v) {
  if (step == 0) return v;
  const uint32_t e = (step / 2u + below) / step;
  return e > 255u ? 255u : e;
}

// the steps whose table needs the channel's histogram
FFCV_HD bool tone_needs_stats(int kind) { return kind == FFCV_TONE_AUTOCONTRAST || kind == FFCV_TONE_EQUALIZE; }

// Entry v of step `kind` for a channel with first / last occupied bin lo / hi,
// h[hi] = h_hi and sum(h[:v]) = below (the last three are read by the
// statistics steps only).
FFCV_HD uint32_t tone_entry(int kind, int bits, uint32_t pixels, uint32_t lo, uint32_t hi, uint32_t h_hi,
                            uint32_t below, uint32_t v) {
  if (kind == FFCV_TONE_POSTERIZE) return tone_posterize(bits, v);
  if (kind == FFCV_TONE_INVERT) return tone_invert(v);
  if (kind == FFCV_TONE_AUTOCONTRAST) return tone_autocontrast(lo, hi, v);
  return tone_equalize(tone_equalize_step(pixels, lo, hi, h_hi), below, v);
}

// The decisions of one sample: for each of the n (op id, p) pairs one draw,
// rand() < p, from the sample's own stream of that op id -> apply[i * B + k].
// Returns 1 when an MT19937 stream ran out.
struct ToneDraw {
  int n;
  uint32_t op[4];
  double p[4];
};
FFCV_HD int draw_tone(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, const ToneDraw &d,
                      uint8_t *apply) {
  int err = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= d.n) break;
    DevMT m;
    mt_init(m, sample_seed(loader_seed, epoch, id, d.op[i]));
    apply[(uint64_t)i * B + k] = (uint8_t)(mt_double(m) < d.p[i]);
    err |= m.err;
  }
  return err;
}
