// affine_common.h -- the RandomAffine / RandomRotation arithmetic,
// single-source: the gfx950 kernels (ffcv_affine.hip) and the host twins of
// the C ABI run the very same functions.
//
// The draws and the matrix are float64 with every operation a statement of
// its own under `#pragma clang fp contract(off)`; sin, cos and tan are the one
// part not pinned bit for bit.  The six coefficients are quantised to Q16
// integers, and from there on every pixel is integer arithmetic.
#pragma once
#include <math.h>

#include "device_common.h"
#include "lds_stage.h"  // lds_chunks

#define FFCV_AFFINE_OP 14
#define FFCV_AFFINE_M_MAX ((int64_t)1 << 23)  // |q0|, |q1|, |q3|, |q4| at most
#define FFCV_AFFINE_B_MAX ((int64_t)1 << 40)  // |q2|, |q5| at most
#define FFCV_AFFINE_MAX_DIM 32767             // largest supported height and width

// int64(rint(v * 65536)), rint rounding half to even
FFCV_HD int64_t affine_q16(double v) {
#pragma clang fp contract(off)
  const double s = v * 65536.0;
  return (int64_t)rint(s);
}

// The matrix of one sample: angle, shx, shy in degrees, tx, ty
// whole pixels, s the scale; q = (m00, m01, b0, m10, m11, b1) in Q16.
FFCV_HD void affine_matrix(double angle, double tx, double ty, double s, double shx, double shy, int H, int W,
                            int64_t *q) {
#pragma clang fp contract(off)
  const double K = 0.017453292519943295;
  const double rot = angle * K;
  const double sx = shx * K;
  const double sy = shy * K;
  const double rs = rot - sy;
  const double crs = cos(rs), srs = sin(rs), csy = cos(sy), tsx = tan(sx);
  const double a = crs / csy;
  const double bt = crs * tsx;
  const double bq = bt / csy;
  const double b = -bq - sin(rot);
  const double c = srs / csy;
  const double dt = srs * tsx;
  const double dq = dt / csy;
  const double d = -dq + cos(rot);
  const double m00 = d / s;
  const double m01 = -b / s;
  const double m10 = -c / s;
  const double m11 = a / s;
  const double cx = (double)(W - 1) / 2.0;
  const double cy = (double)(H - 1) / 2.0;
  const double ux = -cx - tx;
  const double uy = -cy - ty;
  const double p00 = m00 * ux;
  const double p01 = m01 * uy;
  const double s0 = p00 + p01;
  const double b0 = s0 + cx;
  const double p10 = m10 * ux;
  const double p11 = m11 * uy;
  const double s1 = p10 + p11;
  const double b1 = s1 + cy;
  q[0] = affine_q16(m00);
  q[1] = affine_q16(m01);
  q[2] = affine_q16(b0);
  q[3] = affine_q16(m10);
  q[4] = affine_q16(m11);
  q[5] = affine_q16(b1);
}

// One sample's seven draws (op id 14), always all seven, and its coefficients.
// rg: six (lo, hi) pairs in draw order: angle, tx, ty, scale, shear x, shear y.
// Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_affine(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, const double *rg, int H,
                         int W, uint8_t *apply, int64_t *coef) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_AFFINE_OP));
  apply[k] = (uint8_t)(mt_double(m) < p);
  const double angle = mt_uniform(m, rg[0], rg[1]);
  const double tx = rint(mt_uniform(m, rg[2], rg[3]));
  const double ty = rint(mt_uniform(m, rg[4], rg[5]));
  const double s = mt_uniform(m, rg[6], rg[7]);
  const double shx = mt_uniform(m, rg[8], rg[9]);
  const double shy = mt_uniform(m, rg[10], rg[11]);
  affine_matrix(angle, tx, ty, s, shx, shy, H, W, coef + 6 * (uint64_t)k);
  return m.err;
}

// coefficients the pixel pass accepts; any other set gives an image of fill
FFCV_HD bool affine_coef_ok(const int64_t *q) {
  const int64_t M = FFCV_AFFINE_M_MAX, Bm = FFCV_AFFINE_B_MAX;
  return q[0] >= -M && q[0] <= M && q[1] >= -M && q[1] <= M && q[3] >= -M && q[3] <= M && q[4] >= -M && q[4] <= M &&
         q[2] >= -Bm && q[2] <= Bm && q[5] >= -Bm && q[5] <= Bm;
}

// Source coordinates of output pixel (r, c), Q16: no overflow under
// affine_coef_ok and r, c <= 32767 (below 2^41 in magnitude).
FFCV_HD int64_t affine_x(const int64_t *q, int c, int r) { return q[0] * c + q[1] * r + q[2]; }
FFCV_HD int64_t affine_y(const int64_t *q, int c, int r) { return q[3] * c + q[4] * r + q[5]; }

// The bilinear blend of four packed taps with weights fx, fy in 0 .. 255, per
// channel: top = (256 - fx) t0 + fx t1, bot alike, out = ((256 - fy) top + fy
// bot + 32768) >> 16.  top and bot are at most 255 * 256, the last sum is at
// most 255 * 65536 + 32768: nothing clips.
FFCV_HD uint32_t affine_blend(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1, uint32_t fx, uint32_t fy) {
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const uint32_t sh = 8u * ch;
    const uint32_t top = (256u - fx) * ((t0 >> sh) & 0xffu) + fx * ((t1 >> sh) & 0xffu);
    const uint32_t bot = (256u - fx) * ((b0 >> sh) & 0xffu) + fx * ((b1 >> sh) & 0xffu);
    out |= (((256u - fy) * top + fy * bot + 32768u) >> 16) << sh;  // at most 255
  }
  return out;
}

// One output pixel, R | G << 8 | B << 16, from Q16 source coordinates (X, Y)
// in the frame of `tap`: tap.one(iy, ix) is the packed pixel at (iy, ix) or
// the packed fill outside the image; tap.pair gives (iy, ix) and (iy, ix + 1),
// each tested on its own.  T is int64_t, or int32_t where the caller has shown
// the coordinates to fit (shifts are arithmetic, so they floor).
template <class T, class Tap>
FFCV_HD uint32_t affine_sample(int mode, T X, T Y, const Tap &tap) {
  if (mode == FFCV_AFFINE_NEAREST) {
    const T ix = (X + 32768) >> 16, iy = (Y + 32768) >> 16;
    return tap.one(iy, ix);
  }
  const T ix = X >> 16, iy = Y >> 16;
  const uint32_t fx = ((uint32_t)X & 0xFFFFu) >> 8, fy = ((uint32_t)Y & 0xFFFFu) >> 8;
  uint32_t t0, t1, b0, b1;
  tap.pair(iy, ix, &t0, &t1);
  tap.pair(iy + 1, ix, &b0, &b1);
  return affine_blend(t0, t1, b0, b1, fx, fy);
}

// Taps from memory (the host twin; the kernel's direct regime): `img` is one
// H x W x 3 image, coordinates are the image's own.
struct AffineMemTap {
  const uint8_t *img;
  int H, W;
  uint32_t fill;
  FFCV_HD uint32_t one(int64_t iy, int64_t ix) const {
    if (iy < 0 || iy >= H || ix < 0 || ix >= W) return fill;
    const uint8_t *p = img + ((uint64_t)iy * (uint32_t)W + (uint64_t)ix) * 3u;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
  FFCV_HD void pair(int64_t iy, int64_t ix, uint32_t *a, uint32_t *b) const {
    *a = one(iy, ix);
    *b = one(iy, ix + 1);
  }
};

// The source footprint of output rows [y0, y1) x columns [x0, x1) under q:
// the bounding box of the four corners' (iy, ix) -- X and Y are linear in (c,
// r), so their extremes over the rectangle are at its corners, and the shifts
// are monotone -- widened by a row and a column for bilinear and clipped to
// the image: rows [lo, hi) x columns [cl, ch), empty when hi <= lo or ch <=
// cl.  fits32: every pixel's coordinates relative to (org_y, org_x) -- the
// box's corner, or the image's (whole = true: the box, when not empty, is the
// image) -- lie in [-2^30, 2^30), so 32-bit arithmetic on them is exact.
struct AffineBox {
  int lo, hi, cl, ch;
  bool fits32;
  int64_t X0, Y0;  // coordinates of (y0, x0), less the origin
  FFCV_HD bool empty() const { return hi <= lo || ch <= cl; }
  // the bytes a workgroup stages for it: rows that span the width are one byte
  // range, else a range per row in whole chunks
  FFCV_HD uint32_t staged_bytes(int W) const {
    if (empty()) return 0;
    const uint32_t nrows = (uint32_t)(hi - lo), cw = (uint32_t)(ch - cl);
    return cw == (uint32_t)W ? lds_chunks(nrows * 3u * cw) * 16u : nrows * lds_chunks(3u * cw) * 16u;
  }
};

FFCV_HD int64_t affine_min4(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t x = a < b ? a : b, y = c < d ? c : d;
  return x < y ? x : y;
}
FFCV_HD int64_t affine_max4(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t x = a > b ? a : b, y = c > d ? c : d;
  return x > y ? x : y;
}

FFCV_HD AffineBox affine_box(const int64_t *q, int mode, int H, int W, int x0, int y0, int x1, int y1, bool whole) {
  const int64_t off = mode == FFCV_AFFINE_NEAREST ? 32768 : 0;
  const int64_t Xa = affine_x(q, x0, y0), Xb = affine_x(q, x1 - 1, y0), Xc = affine_x(q, x0, y1 - 1),
                Xd = affine_x(q, x1 - 1, y1 - 1);
  const int64_t Ya = affine_y(q, x0, y0), Yb = affine_y(q, x1 - 1, y0), Yc = affine_y(q, x0, y1 - 1),
                Yd = affine_y(q, x1 - 1, y1 - 1);
  const int64_t Xmin = affine_min4(Xa, Xb, Xc, Xd), Xmax = affine_max4(Xa, Xb, Xc, Xd);
  const int64_t Ymin = affine_min4(Ya, Yb, Yc, Yd), Ymax = affine_max4(Ya, Yb, Yc, Yd);
  const int64_t wide = mode == FFCV_AFFINE_NEAREST ? 0 : 1;
  const int64_t ix0 = (Xmin + off) >> 16, ix1 = ((Xmax + off) >> 16) + wide;
  const int64_t iy0 = (Ymin + off) >> 16, iy1 = ((Ymax + off) >> 16) + wide;
  AffineBox b;
  b.cl = (int)(ix0 < 0 ? 0 : (ix0 > W ? W : ix0));
  b.ch = (int)(ix1 + 1 > W ? W : (ix1 + 1 < 0 ? 0 : ix1 + 1));
  b.lo = (int)(iy0 < 0 ? 0 : (iy0 > H ? H : iy0));
  b.hi = (int)(iy1 + 1 > H ? H : (iy1 + 1 < 0 ? 0 : iy1 + 1));
  if (whole && !b.empty()) {
    b.cl = 0;
    b.ch = W;
    b.lo = 0;
    b.hi = H;
  }
  const int64_t ox = (int64_t)b.cl << 16, oy = (int64_t)b.lo << 16, L = (int64_t)1 << 30;
  b.fits32 = Xmin - ox >= -L && Xmax - ox < L && Ymin - oy >= -L && Ymax - oy < L;
  b.X0 = Xa - ox;
  b.Y0 = Ya - oy;
  return b;
}
