// perspective_common.h -- the RandomPerspective arithmetic, single-source: the
// gfx950 kernels (ffcv_perspective.hip) and the host twins of the C ABI run
// the very same functions.
//
// The draws, the nine coefficients and a pixel's source coordinates are
// float64 with every operation a statement of its own under `#pragma clang fp
// contract(off)`: products, sums, quotients and floor only, no library solve
// and no transcendental function, so numpy (tests/perspective_ref.py), the
// host twin and the device agree bit for bit.  From the Q16 coordinates on a
// pixel is s21's integer sample (affine_common.h: affine_sample).
#pragma once
#include <math.h>

#include "affine_common.h"

#define FFCV_PERSPECTIVE_OP 26
#define FFCV_PERSPECTIVE_MIN_DIM 2  // a side of 1 has no quadrilateral

// lo + min(int(floor(rand() * (hi - lo + 1))), hi - lo)
FFCV_HD int persp_randint(DevMT &m, int lo, int hi) {
#pragma clang fp contract(off)
  const double n = (double)(hi - lo + 1);
  const double v = mt_double(m) * n;
  const int64_t i = (int64_t)floor(v);
  return lo + (int)(i > hi - lo ? hi - lo : i);
}

// The four corner cross-products of the quadrilateral tl, tr, br, bl (p: x0,
// y0 .. x3, y3), in exact integers: all > 0 where it is strictly convex with
// the image's orientation.
FFCV_HD bool persp_convex(const int *p) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) & 3, l = (i + 2) & 3;
    const int64_t ax = p[2 * j] - p[2 * i], ay = p[2 * j + 1] - p[2 * i + 1];
    const int64_t bx = p[2 * l] - p[2 * j], by = p[2 * l + 1] - p[2 * j + 1];
    ok &= ax * by - ay * bx > 0;
  }
  return ok;
}

// The homography of one sample: q[9] = A B C / D E F / G Hh I sends output
// pixel (c, r) inside the quadrilateral p to the source rectangle [0, W - 1] x
// [0, H - 1].  Heckbert's unit-square-to-quadrilateral matrix (a b c / d e f /
// g h 1), its adjugate, the first row scaled by W - 1 and the second by H - 1,
// everything divided by the matrix's determinant: p = the image's own corners
// gives the identity exactly.  The sums of the eight integers are exact in
// int64 (below 2^33).  Returns false, and the identity, where the determinant
// is not a positive finite number (never for a convex quadrilateral in exact
// arithmetic: the map keeps the orientation).
FFCV_HD bool persp_matrix(const int *p, int H, int W, double *q) {
#pragma clang fp contract(off)
  const int64_t x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3], x2 = p[4], y2 = p[5], x3 = p[6], y3 = p[7];
  const int64_t dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
  const int64_t dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
  const double gn = (double)(sy * dx2 - sx * dy2);  // both signs turned, so that dn > 0
  const double hn = (double)(dy1 * sx - dx1 * sy);
  const double dn = (double)(dx2 * dy1 - dx1 * dy2);  // the cross-product at br
  const double g = gn / dn;
  const double h = hn / dn;
  const double gx = g * (double)x1;
  const double a = (double)(x1 - x0) + gx;
  const double hx = h * (double)x3;
  const double b = (double)(x3 - x0) + hx;
  const double c = (double)x0;
  const double gy = g * (double)y1;
  const double d = (double)(y1 - y0) + gy;
  const double hy = h * (double)y3;
  const double e = (double)(y3 - y0) + hy;
  const double f = (double)y0;
  // the adjugate (i = 1)
  const double fh = f * h;
  const double A = e - fh;
  const double ch = c * h;
  const double B = ch - b;
  const double bf = b * f;
  const double ce = c * e;
  const double C = bf - ce;
  const double fg = f * g;
  const double D = fg - d;
  const double cg = c * g;
  const double E = a - cg;
  const double cd = c * d;
  const double af = a * f;
  const double F = cd - af;
  const double dh = d * h;
  const double eg = e * g;
  const double G = dh - eg;
  const double bg = b * g;
  const double ah = a * h;
  const double Hh = bg - ah;
  const double ae = a * e;
  const double bd = b * d;
  const double I = ae - bd;
  const double aA = a * A;
  const double bD = b * D;
  const double cG = c * G;
  const double s0 = aA + bD;
  const double det = s0 + cG;
  if (!(det > 0.0) || !(det <= 1.7976931348623157e308)) {
    for (int i = 0; i < 9; i++) q[i] = i % 4 == 0 ? 1.0 : 0.0;
    return false;
  }
  const double w1 = (double)(W - 1), h1 = (double)(H - 1);
  const double Aw = A * w1;
  const double Bw = B * w1;
  const double Cw = C * w1;
  const double Dh = D * h1;
  const double Eh = E * h1;
  const double Fh = F * h1;
  q[0] = Aw / det;
  q[1] = Bw / det;
  q[2] = Cw / det;
  q[3] = Dh / det;
  q[4] = Eh / det;
  q[5] = Fh / det;
  q[6] = G / det;
  q[7] = Hh / det;
  q[8] = I / det;
  return true;
}

// One sample's nine draws (op id 26), always all nine, its decision and its
// coefficients; d: the distortion scale.  A quadrilateral that is not strictly
// convex is not applied and takes the identity.  Returns 1 when the MT19937
// stream ran out.
FFCV_HD int draw_perspective(int k, uint64_t id, uint64_t loader_seed, uint64_t epoch, double p, double d, int H, int W,
                              uint8_t *apply, double *coef) {
#pragma clang fp contract(off)
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_PERSPECTIVE_OP));
  bool on = mt_double(m) < p;
  const double dw = d * (double)(W / 2);
  const double dh = d * (double)(H / 2);
  const int bw = (int)floor(dw), bh = (int)floor(dh);
  int q[8];
  q[0] = persp_randint(m, 0, bw);
  q[1] = persp_randint(m, 0, bh);
  q[2] = persp_randint(m, W - 1 - bw, W - 1);
  q[3] = persp_randint(m, 0, bh);
  q[4] = persp_randint(m, W - 1 - bw, W - 1);
  q[5] = persp_randint(m, H - 1 - bh, H - 1);
  q[6] = persp_randint(m, 0, bw);
  q[7] = persp_randint(m, H - 1 - bh, H - 1);
  if (!persp_convex(q)) {
    q[0] = q[1] = q[3] = q[6] = 0;
    q[2] = q[4] = W - 1;
    q[5] = q[7] = H - 1;
    on = false;
  }
  on &= persp_matrix(q, H, W, coef + 9 * (uint64_t)k);
  apply[k] = (uint8_t)on;
  return m.err;
}

// Source coordinates of output pixel (c, r) in Q16, or false where the pixel
// takes fill: den not > 0 (on or behind the horizon), or X or Y not finite or
// of magnitude >= 65536.  One division.
FFCV_HD bool persp_coords(const double *q, int c, int r, int64_t *Xq, int64_t *Yq) {
#pragma clang fp contract(off)
  const double fc = (double)c, fr = (double)r;
  const double ac = q[0] * fc;
  const double br = q[1] * fr;
  const double sx = ac + br;
  const double nx = sx + q[2];
  const double dc = q[3] * fc;
  const double er = q[4] * fr;
  const double sy = dc + er;
  const double ny = sy + q[5];
  const double gc = q[6] * fc;
  const double hr = q[7] * fr;
  const double sd = gc + hr;
  const double den = sd + q[8];
  const double w = 1.0 / den;
  const double X = nx * w;
  const double Y = ny * w;
  // (NaN fails every comparison)
  if (!(den > 0.0) || !(X > -65536.0 && X < 65536.0) || !(Y > -65536.0 && Y < 65536.0)) return false;
  const double xs = X * 65536.0;
  const double ys = Y * 65536.0;
  *Xq = (int64_t)floor(xs);
  *Yq = (int64_t)floor(ys);
  return true;
}

// One output pixel, R | G << 8 | B << 16, with taps in the image's own frame
template <class Tap>
FFCV_HD uint32_t persp_pixel(const double *q, int mode, int c, int r, uint32_t fill, const Tap &tap) {
  int64_t Xq, Yq;
  if (!persp_coords(q, c, r, &Xq, &Yq)) return fill;
  return affine_sample<int64_t>(mode, Xq, Yq, tap);
}

// The source footprint of output rows [y0, y1) x columns [x0, x1).  Where den
// > 0 on the four corner pixels it is > 0 on the whole tile (den is linear),
// and X and Y, quotients of linear functions, take their extremes over the
// tile at its corners (they are monotone along every segment on which den
// keeps its sign): the footprint is the corners' bounding box, widened by a
// pixel on each side for the rounding of the float64 statements, by a row and
// a column for bilinear, and clipped to the image: rows [lo, hi) x columns
// [cl, ch).  The kernel stages it, but tests every tap against it (a tap
// outside the staged box that lies inside the image is read from memory), so
// the argument above serves speed only.
//   direct: a corner has den <= 0 or coordinates of magnitude >= 65536:
//           nothing is said about the footprint
//   empty():  the box misses the image
struct PerspBox {
  int lo, hi, cl, ch;
  bool direct;
  FFCV_HD bool empty() const { return hi <= lo || ch <= cl; }
  FFCV_HD uint32_t staged_bytes(int W) const {
    if (empty()) return 0;
    const uint32_t nrows = (uint32_t)(hi - lo), cw = (uint32_t)(ch - cl);
    return cw == (uint32_t)W ? lds_chunks(nrows * 3u * cw) * 16u : nrows * lds_chunks(3u * cw) * 16u;
  }
};

FFCV_HD PerspBox persp_box(const double *q, int mode, int H, int W, int x0, int y0, int x1, int y1, bool whole) {
  PerspBox b;
  b.lo = b.cl = 0;
  b.hi = H;
  b.ch = W;
  b.direct = false;
  if (whole) return b;  // the image itself: every tap inside the image is staged
  const int64_t L = (int64_t)1 << 40;
  int64_t Xmin = L, Xmax = -L, Ymin = L, Ymax = -L;
  for (int i = 0; i < 4; i++) {
    int64_t X, Y;
    if (!persp_coords(q, (i & 1) ? x1 - 1 : x0, (i & 2) ? y1 - 1 : y0, &X, &Y)) {
      b.direct = true;
      return b;
    }
    Xmin = X < Xmin ? X : Xmin;
    Xmax = X > Xmax ? X : Xmax;
    Ymin = Y < Ymin ? Y : Ymin;
    Ymax = Y > Ymax ? Y : Ymax;
  }
  const int64_t off = mode == FFCV_AFFINE_NEAREST ? 32768 : 0, wide = mode == FFCV_AFFINE_NEAREST ? 0 : 1;
  const int64_t ix0 = ((Xmin + off) >> 16) - 1, ix1 = ((Xmax + off) >> 16) + wide + 1;
  const int64_t iy0 = ((Ymin + off) >> 16) - 1, iy1 = ((Ymax + off) >> 16) + wide + 1;
  b.cl = (int)(ix0 < 0 ? 0 : (ix0 > W ? W : ix0));
  b.ch = (int)(ix1 + 1 > W ? W : (ix1 + 1 < 0 ? 0 : ix1 + 1));
  b.lo = (int)(iy0 < 0 ? 0 : (iy0 > H ? H : iy0));
  b.hi = (int)(iy1 + 1 > H ? H : (iy1 + 1 < 0 ? 0 : iy1 + 1));
  return b;
}
