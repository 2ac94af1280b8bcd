// erase_common.h -- what the RandomErasing kernels and their host twins share
// (ffcv_erase.hip): the draws of a sample, the box in the units
// of the fill, and the noise index of an element.
#pragma once
#include <cmath>

#include "device_common.h"

#define ERASE_OP_DRAW 21    // seeding contract: the box draws
#define ERASE_OP_NOISE 22   // and the noise key
#define ERASE_TABLE 4096    // entries of the noise table
#define ERASE_TRIES 10

// A sample's noise key: the contract's hash of op id 22, all 64 bits.
FFCV_HD uint64_t erase_key(uint64_t loader_seed, uint64_t epoch, uint64_t sample) {
  uint64_t h = splitmix64(loader_seed ^ ((uint64_t)ERASE_OP_NOISE << 56));
  h = splitmix64(h ^ epoch);
  return splitmix64(h ^ sample);
}

// The table entry of element e (its index inside its sample, storage order)
// out of the word splitmix64(key ^ (e >> 2)): 12 of the word's 16 bits of e.
FFCV_HD uint32_t erase_index(uint64_t word, uint32_t e) { return (uint32_t)(word >> (16 * (e & 3) + 4)) & 0xFFFu; }

// DevMT's first 227 words, which come from the initial state alone: without
// the out-of-line path for the words behind them, whose call frame would cost
// the draw kernel scratch (as CropMT, ffcv_rrc_images.hip).  The draws take 2 +
// 40 + a few words; word 227 and later set err (FFCV_SAMPLE_RNG).
FFCV_HD uint32_t erase_u32(DevMT &m) {
  uint32_t v = 0;
  if (m.n < 227) {
    v = mt_twist1(m.a0, m.a1, m.b);
    m.a0 = m.a1;
    m.a1 = mt_chain(m.a1, (uint32_t)(m.n + 2));
    m.b = mt_chain(m.b, (uint32_t)(m.n + 398));
  } else {
    m.err = 1;
  }
  m.n++;
  return mt_temper(v);
}
FFCV_HD double erase_uniform(DevMT &m, double lo, double hi) {  // mt_uniform
  const int32_t a = (int32_t)(erase_u32(m) >> 5);
  const int32_t b = (int32_t)(erase_u32(m) >> 6);
  return lo + (hi - lo) * ((a * 67108864.0 + b) / 9007199254740992.0);
}
FFCV_HD int32_t erase_randint(DevMT &m, uint32_t high) {        // mt_randint, high >= 1
  const uint32_t rng = high - 1;
  if (rng == 0) return 0;
  uint32_t mask = rng;
  mask |= mask >> 1;
  mask |= mask >> 2;
  mask |= mask >> 4;
  mask |= mask >> 8;
  mask |= mask >> 16;
  uint32_t v;
  do {
    v = erase_u32(m) & mask;
  } while (v > rng && !m.err);
  return (int32_t)v;
}

// torchvision's RandomErasing.get_params on the sample's own stream: apply
// first, then up to ten tries, drawn whether or not the sample applies (the
// words consumed do not depend on p).  h rows by w columns, both strictly
// inside the image.  box: (y, x, h, w), h = w = 0 when nothing is erased.
FFCV_HD int draw_erase(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, double s0, double s1,
                       double r0, double r1, int H, int W, int32_t *boxes, uint64_t *keys) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, ERASE_OP_DRAW));
  const bool apply = erase_uniform(m, 0.0, 1.0) < p;
  const double area = (double)(H * W), lr0 = log(r0), lr1 = log(r1);
  int32_t y = 0, x = 0, bh = 0, bw = 0;
#pragma unroll 1
  for (int t = 0; t < ERASE_TRIES; t++) {
    const double ea = area * erase_uniform(m, s0, s1);
    const double ar = exp(erase_uniform(m, lr0, lr1));
    const int64_t h = (int64_t)rint(sqrt(ea * ar));
    const int64_t w = (int64_t)rint(sqrt(ea / ar));
    if (0 < h && h < H && 0 < w && w < W) {
      y = erase_randint(m, (uint32_t)(H - h + 1));
      x = erase_randint(m, (uint32_t)(W - w + 1));
      bh = (int32_t)h;
      bw = (int32_t)w;
      break;
    }
  }
  if (!apply) y = x = bh = bw = 0;
  boxes[4 * k] = y;
  boxes[4 * k + 1] = x;
  boxes[4 * k + 2] = bh;
  boxes[4 * k + 3] = bw;
  if (keys) keys[k] = erase_key(loader_seed, epoch, id);
  return m.err;
}

// A box in the units of the fill: rows [y1, y2) of every plane, `len` bytes
// from byte xb1 of a row; clamped to the image.
struct EraseBox {
  uint32_t y1, y2, xb1, len;
};

FFCV_HD uint32_t erase_clamp(int64_t v, uint32_t hi) { return v < 0 ? 0u : (v > (int64_t)hi ? hi : (uint32_t)v); }

// false: nothing to erase (h <= 0, w <= 0 or a box wholly outside the image)
FFCV_HD bool erase_box(int32_t y, int32_t x, int32_t h, int32_t w, uint32_t height, uint32_t width,
                       uint32_t pixel_bytes, EraseBox *o) {
  if (h <= 0 || w <= 0) return false;
  o->y1 = erase_clamp(y, height);
  o->y2 = erase_clamp((int64_t)y + h, height);
  const uint32_t x1 = erase_clamp(x, width), x2 = erase_clamp((int64_t)x + w, width);
  o->xb1 = x1 * pixel_bytes;
  o->len = (x2 > x1 ? x2 - x1 : 0u) * pixel_bytes;
  return o->y1 < o->y2 && o->len > 0;
}
