// jpeg_color_resize.h -- K2 of ffcv_jpeg.hip: planes, upsampling and colour, the band
// records' readers, the linear / area walks and the general path;
// jpeg_color_resize_kernel and k2_rec_kernel.
#pragma once
#include "jpeg_defs.h"
#include "jpeg_idct.h"  // u16x2

// ======================================================================= //
// K2: fancy upsampling + colour conversion into LDS, INTER_AREA + epilogue //
// ======================================================================= //

// Plane accessors: a component plane in HBM (GPlane) or a tile of it staged
// in LDS (TPlane, rows [r0, ..] x cols [c0, ..] of the plane).
struct GPlane {
  const uint8_t *p;
  int stride;
  FFCV_DEV int at(int r, int c) const { return p[(uint64_t)r * stride + c]; }
};
struct TPlane {
  const uint8_t *p;
  int r0, c0, pitch;
  FFCV_DEV int at(int r, int c) const { return p[__mul24(r - r0, pitch) + (c - c0)]; }  // tiles < 2^24 B
};

// jdsample.c upsampling of one component at full-resolution sample (y, x),
// with libjpeg's context-row edge replication.
template <class PL>
FFCV_DEV int upsample_at(const PL &P, int cw, int ch, int he, int ve, int y, int x) {
  auto clampr = [&](int r) { return r < 0 ? 0 : (r >= ch ? ch - 1 : r); };
  if (he == 1 && ve == 1) return P.at(y, x);
  if (he == 2 && ve == 1) {
    int col = x >> 1;
    if (cw <= 2) return P.at(y, col);
    int cur = P.at(y, col) * 3;
    if (x & 1) {
      if (col + 1 >= cw) return P.at(y, col);
      return (cur + P.at(y, col + 1) + 2) >> 2;
    }
    if (col == 0) return P.at(y, 0);
    return (cur + P.at(y, col - 1) + 1) >> 2;
  }
  if (he == 1 && ve == 2) {
    int r = y >> 1, other = (y & 1) ? r + 1 : r - 1;
    int sum = P.at(clampr(r), x) * 3 + P.at(clampr(other), x);
    return (sum + ((y & 1) ? 2 : 1)) >> 2;
  }
  if (he == 2 && ve == 2) {
    int r = y >> 1, col = x >> 1;
    if (cw <= 2) return P.at(r, col);
    int other = (y & 1) ? r + 1 : r - 1;
    int rc = clampr(r), oc = clampr(other);
    int thiss = P.at(rc, col) * 3 + P.at(oc, col);
    if (x & 1) {
      int nxt = col + 1 < cw ? P.at(rc, col + 1) * 3 + P.at(oc, col + 1) : thiss;
      return (thiss * 3 + nxt + 7) >> 4;
    }
    int last = col > 0 ? P.at(rc, col - 1) * 3 + P.at(oc, col - 1) : thiss;
    return (thiss * 3 + last + 8) >> 4;
  }
  return P.at(y / ve, x / he);  // int_upsample
}

// jdcolor.c ycc_rgb_convert with build_ycc_rgb_table's fixed point
FFCV_DEV void ycc_rgb(int y, int cb, int cr, int out[3]) {
  int x_cb = cb - 128, x_cr = cr - 128;
  out[0] = sat_u8i(y + ((91881 * x_cr + 32768) >> 16));
  out[1] = sat_u8i(y + ((-22554 * x_cb + 32768 + -46802 * x_cr) >> 16));
  out[2] = sat_u8i(y + ((116130 * x_cb + 32768) >> 16));
}

// The per-image fields the colour pass needs, held in registers.
struct ColorGeom {
  int ncomp, color_rgb;
  int he[3], ve[3], cw[3], ch[3];
};
// The part of an image record K2 reads (ImgInfo up to and including `taps`),
// read through the scalar cache (s_load) at the top of the kernel.  Reading
// the fields from the global record where they are used issued them in ~6
// dependent round trips (the compiler may not hoist loads above the status /
// mode branches), which was most of K2's per-workgroup fixed cost.  (Until
// round 5 the head was one vector load per lane, broadcast with v_readlane
// per field: 49 VALU per wave.  That arm last existed in commit 356ba29.)
struct K2Rec {
  const __attribute__((address_space(4))) uint32_t *p;  // the record (written by K1: a previous kernel)
  FFCV_DEV void load(const ImgInfo *rec, int) { p = (const __attribute__((address_space(4))) uint32_t *)rec; }
  FFCV_DEV uint32_t u(int i) const { return p[i]; }
  FFCV_DEV int32_t s(int i) const { return (int32_t)u(i); }
  FFCV_DEV uint64_t u64(int i) const { return (uint64_t)u(i) | ((uint64_t)u(i + 1) << 32); }
  FFCV_DEV double f64(int i) const { return __builtin_bit_cast(double, u64(i)); }
};
#define K2F(f) ((int)(offsetof(ImgInfo, f) / 4))
// This band's K2BandRec (written by K1b: a previous kernel), read through the
// scalar cache in the same round trip: 32 dwords, no lane broadcast.  The
// phases below pick their few fields from it.
struct K2Band {
  const __attribute__((address_space(4))) uint32_t *p;
  FFCV_DEV void load(const K2BandRec *rec) { p = (const __attribute__((address_space(4))) uint32_t *)rec; }
  // A new phase reads its fields again (scalar cache hits) instead of
  // holding them in registers from the top: the compiler must not merge
  // these loads with the earlier phase's
  FFCV_DEV void phase() { asm volatile("" : "+s"(p)); }
  FFCV_DEV uint32_t u(int i) const { return p[i]; }
  FFCV_DEV int32_t s(int i) const { return (int32_t)p[i]; }
  FFCV_DEV uint64_t u64(int i) const { return (uint64_t)p[i] | ((uint64_t)p[i + 1] << 32); }
  FFCV_DEV double f64(int i) const { return __builtin_bit_cast(double, u64(i)); }
};
#define K2BF(f) ((int)(offsetof(K2BandRec, f) / 4))
FFCV_DEV ImgInfo k2_head(const K2Rec &R) {
  ImgInfo I;  // only the head fields are set (SROA keeps them in registers)
  I.status = R.s(K2F(status));
  I.W = R.s(K2F(W));
  I.H = R.s(K2F(H));
  I.ncomp = R.s(K2F(ncomp));
  I.color_rgb = R.s(K2F(color_rgb));
#pragma unroll
  for (int c = 0; c < 3; c++) {
    I.he[c] = R.s(K2F(he) + c);
    I.ve[c] = R.s(K2F(ve) + c);
    I.cw[c] = R.s(K2F(cw) + c);
    I.ch[c] = R.s(K2F(ch) + c);
    I.stride[c] = R.s(K2F(stride) + c);
    I.poff[c] = R.u64(K2F(poff) + 2 * c);
  }
  I.ri = R.s(K2F(ri));
  I.rj = R.s(K2F(rj));
  I.rh = R.s(K2F(rh));
  I.rw = R.s(K2F(rw));
  I.rgb_off = R.u64(K2F(rgb_off));
  I.plan.sw = R.s(K2F(plan.sw));
  I.plan.sh = R.s(K2F(plan.sh));
  I.plan.dw = R.s(K2F(plan.dw));
  I.plan.dh = R.s(K2F(plan.dh));
  I.plan.kind = R.s(K2F(plan.kind));
  I.plan.isx = R.s(K2F(plan.isx));
  I.plan.isy = R.s(K2F(plan.isy));
  I.plan.vec_end = R.s(K2F(plan.vec_end));
  I.plan.scale_x = R.f64(K2F(plan.scale_x));
  I.plan.scale_y = R.f64(K2F(plan.scale_y));
  I.plan.inv_x = R.f64(K2F(plan.inv_x));
  I.plan.inv_y = R.f64(K2F(plan.inv_y));
  I.taps = R.s(K2F(taps));
  return I;
}

FFCV_DEV ColorGeom color_geom(const ImgInfo &I) {
  ColorGeom g;
  g.ncomp = I.ncomp;
  g.color_rgb = I.color_rgb;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    g.he[c] = I.he[c];
    g.ve[c] = I.ve[c];
    g.cw[c] = I.cw[c];
    g.ch[c] = I.ch[c];
  }
  return g;
}

// The wave-uniform format fields pass through an empty asm per call: the
// upsampling-mode tests of upsample_at are then scalar compares beside their
// branches.  Without it the compiler hoists every (he == a && ve == b)
// combination of three components out of the caller's per-pixel loop as
// 64-bit masks, ~20 SGPR pairs that spilled and were reloaded per iteration.
template <class PL>
FFCV_DEV void pixel_rgb(const ColorGeom &G, const PL *pl, int Y, int X, int v[3]) {
  ColorGeom I = G;
  asm volatile("" : "+s"(I.ncomp), "+s"(I.color_rgb));
#pragma unroll
  for (int c = 0; c < 3; c++) asm volatile("" : "+s"(I.he[c]), "+s"(I.ve[c]), "+s"(I.cw[c]));
  if (I.ncomp == 1) {
    v[0] = v[1] = v[2] = pl[0].at(Y, X);
    return;
  }
  int s0 = upsample_at(pl[0], I.cw[0], I.ch[0], I.he[0], I.ve[0], Y, X);
  int s1 = upsample_at(pl[1], I.cw[1], I.ch[1], I.he[1], I.ve[1], Y, X);
  int s2 = upsample_at(pl[2], I.cw[2], I.ch[2], I.he[2], I.ve[2], Y, X);
  if (I.color_rgb) {
    v[0] = s0;
    v[1] = s1;
    v[2] = s2;
  } else {
    ycc_rgb(s0, s1, s2, v);
  }
}

// h2v2 fancy upsampling (jdsample.c h2v2_fancy_upsample) of the 2x2 output
// quad that chroma sample (R, C) expands to: q[0..3] = (2R,2C), (2R,2C+1),
// (2R+1,2C), (2R+1,2C+1).  Same arithmetic as upsample_at(he=ve=2, cw>2),
// with the 3x3 neighbourhood read once.
template <class PL>
FFCV_DEV void upsample_quad_h2v2(const PL &P, int cw, int ch, int R, int C, int q[4]) {
  const int ru = max(R - 1, 0), rd = min(R + 1, ch - 1);
  const int cl = max(C - 1, 0), cr = min(C + 1, cw - 1);
  const int ml = P.at(R, cl), mc = P.at(R, C), mr = P.at(R, cr);
  const int tl = 3 * ml + P.at(ru, cl), tc = 3 * mc + P.at(ru, C), tr = 3 * mr + P.at(ru, cr);
  const int bl = 3 * ml + P.at(rd, cl), bc = 3 * mc + P.at(rd, C), br = 3 * mr + P.at(rd, cr);
  const bool first = C == 0, last = C + 1 >= cw;
  q[0] = (3 * tc + (first ? tc : tl) + 8) >> 4;
  q[1] = (3 * tc + (last ? tc : tr) + 7) >> 4;
  q[2] = (3 * bc + (first ? bc : bl) + 8) >> 4;
  q[3] = (3 * bc + (last ? bc : br) + 7) >> 4;
}

struct LdsRoi {  // crop rows [row0, row0 + nrows), staged as RGB in LDS
  const uint8_t *p;
  int row0;
  int step;
  FFCV_DEV int at(int y, int x, int c) const { return p[__mul24(y - row0, step) + x * 3 + c]; }
  FFCV_DEV const uint8_t *pix(int y, int x) const { return p + __mul24(y - row0, step) + x * 3; }
};

// K2's FP16 LUT in LDS is channel-major, [c][256] halves (a.p.lut is [v][c]):
// entry (v, c) is v shifted plus the ds_read's immediate offset c * 512,
// where the interleaved v * 3 + c compiled to a 64-bit multiply-add per read
typedef __attribute__((address_space(3))) uint16_t lds_u16_t;
FFCV_DEV uint32_t lut_at(const lds_u16_t *L, int v, int c) { return L[(uint32_t)v + 256u * (uint32_t)c]; }
FFCV_DEV uint16_t lut_src(const uint16_t *lut, int d) { return lut[(d & 255) * 3 + (d >> 8)]; }  // LDS entry d
// The linear walk's last step, VResizeLinearVec's (m0 + m1 + 2) >> 2 of the
// vertical sum x = m0 + m1: the u8 value, or (FP16) the LDS byte address of
// its channel-0 LUT entry, base + 2 * ((x + 2) >> 2) = (x + lq) >> 1 & ~1 with
// lq = 2 + 2 * base (base even): an add3, a shift and an and, where indexing
// the value cost a 4-cycle shift-add more (tools/op_rate); lut_ld reads the
// channel-c entry at that address (channel c's table: + 512 c bytes)
template <bool FP16>
FFCV_DEV uint32_t lut_q(uint32_t x, uint32_t lq) { return FP16 ? ((x + lq) >> 1) & ~1u : (x + 2u) >> 2; }
FFCV_DEV uint32_t lut_base(const lds_u16_t *L) { return (uint32_t)(uintptr_t)L; }
FFCV_DEV uint32_t lut_ld(uint32_t q, int c) { return ((const lds_u16_t *)(uintptr_t)q)[256 * c]; }

#ifndef K2_WPE
#define K2_WPE 6  // waves per SIMD K2 is compiled for (6 WGs per CU at K2_LDS)
#endif

// K2's area walk: ResizeArea_Invoker (resize.cpp, INTER_AREA with both scales
// in [1, 2)) for output columns dx0, dx0 + 1 over this thread's row group, from
// the band's packed RGB rows in LDS (crop column x at byte xoff3 + 3 x of LDS
// row r - r0).  Same arithmetic and order as resize_area: per source row the
// horizontal sums buf = S[lo] a0 + S[lo + 1] a1 + S[lo + 2] a2 (a fixed
// 3-tap body: a destination index at a scale < 2 covers at most 3 source
// indices, and a tap past hi has weight 0, so x + S * 0 == x for these
// non-negative sums), then sum = beta(lo) buf(lo), sum += beta(r) buf(r).
// Consecutive output rows share at most their boundary source row, so one
// cached row of sums covers the reuse.  The two columns' values of a channel
// form one float2 (v_pk_mul_f32 / v_pk_add_f32: each lane is an ordinary
// IEEE multiply or add, contraction off).  A row group is two whole waves: the
// row loops and the cache test are scalar.
typedef float k2f2 __attribute__((ext_vector_type(2)));
template <bool FP16>
FFCV_DEV void k2_area_walk(const Epilogue &ep, int psw, double pscale_x, const AreaTaps *atab, const uint8_t *rgb,
                           int pitch3, int xoff3, int r0, int oy0, int oy1, int sub, int dx0, uint32_t lutb,
                           char *ob) {
  const int half = (BAND + K2T / K2_COLS - 1) / (K2T / K2_COLS);  // rows per row group
  const int ya = __builtin_amdgcn_readfirstlane(oy0 + sub * half);
  const int yb = __builtin_amdgcn_readfirstlane(min(oy1, ya + half));
  const int out_w = ep.out_w;
  uint32_t xa[2], sh[2];  // a column's first tap: aligned byte offset in the row, byte shift
  k2f2 wk[3];             // tap k's weight for (dx0, dx0 + 1)
  {
    const AreaTaps t0 = area_taps(psw, pscale_x, ep.src_x(dx0)), t1 = area_taps(psw, pscale_x, ep.src_x(dx0 + 1));
    const uint32_t o0 = (uint32_t)(xoff3 + 3 * t0.lo), o1 = (uint32_t)(xoff3 + 3 * t1.lo);
    xa[0] = o0 & ~3u;
    sh[0] = o0 & 3u;
    xa[1] = o1 & ~3u;
    sh[1] = o1 & 3u;
#pragma unroll
    for (int k = 0; k < 3; k++)
      wk[k] = (k2f2){t0.lo + k <= t0.hi ? t0.w(t0.lo + k) : 0.f, t1.lo + k <= t1.hi ? t1.w(t1.lo + k) : 0.f};
  }
  // a column's three tap pixels are 9 consecutive bytes: three aligned dword
  // reads and v_alignbyte (misaligned LDS reads are several times slower)
  auto hsum = [&](int r, k2f2 B[3]) {
    const uint8_t *row = rgb + __mul24(r - r0, pitch3);
    uint32_t e[2][3];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t *qa = (const uint32_t *)(row + xa[j]);
      const uint32_t d0 = qa[0], d1 = qa[1], d2 = qa[2];
      e[j][0] = __builtin_amdgcn_alignbyte(d1, d0, sh[j]);
      e[j][1] = __builtin_amdgcn_alignbyte(d2, d1, sh[j]);
      e[j][2] = d2 >> (8 * sh[j]);
    }
    auto bx = [&](int i) {
      return (k2f2){(float)((e[0][i >> 2] >> (8 * (i & 3))) & 0xffu), (float)((e[1][i >> 2] >> (8 * (i & 3))) & 0xffu)};
    };
#pragma unroll
    for (int c = 0; c < 3; c++) {
      k2f2 b = bx(c) * wk[0];  // (0 + x == x for x >= 0: the reference's zeroed buf)
      b = b + bx(3 + c) * wk[1];
      b = b + bx(6 + c) * wk[2];
      B[c] = b;
    }
  };
  const bool cut0 = ep.in_cut(ep.cut_y, dx0), cut1 = ep.in_cut(ep.cut_y, dx0 + 1);
  int cr = -1;
  k2f2 Hc[3];
#pragma unroll
  for (int c = 0; c < 3; c++) Hc[c] = (k2f2){0.f, 0.f};
  for (int dy = ya; dy < yb; dy++) {
    const AreaTaps ty = atab[dy - oy0];
    k2f2 S[3];
    for (int r = ty.lo; r <= ty.hi; r++) {
      k2f2 H[3];
      if (r == cr) {
#pragma unroll
        for (int c = 0; c < 3; c++) H[c] = Hc[c];
      } else {
        hsum(r, H);
      }
      const k2f2 w = (k2f2){ty.w(r), ty.w(r)};
      if (r == ty.lo) {
#pragma unroll
        for (int c = 0; c < 3; c++) S[c] = w * H[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++) S[c] = S[c] + w * H[c];
      }
      if (r == ty.hi) {
#pragma unroll
        for (int c = 0; c < 3; c++) Hc[c] = H[c];
        cr = r;
      }
    }
    // cvRound + saturate_cast<uchar> of sums in [0, 255.5) (bytes times
    // weights summing to 1 up to a few float roundings): S + 1.5 * 2^23
    // rounds half-to-even into the float's low byte, one packed add per
    // column pair (the saturation never acts); only that byte is used
    uint32_t o[6];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const k2f2 m = S[c] + (k2f2){12582912.0f, 12582912.0f};
      o[c] = ffcv_f2u_bits(m.x);
      o[3 + c] = ffcv_f2u_bits(m.y);
    }
    if ((cut0 || cut1) && dy >= ep.cut_y && dy < ep.cut_y + ep.cut_size) {
      if (cut0) {
        o[0] = ep.fill[0];
        o[1] = ep.fill[1];
        o[2] = ep.fill[2];
      }
      if (cut1) {
        o[3] = ep.fill[0];
        o[4] = ep.fill[1];
        o[5] = ep.fill[2];
      }
    }
    // the row's address is wave-uniform: scalar base + this thread's offset
    typedef __attribute__((address_space(1))) uint8_t gbyte_t;
    const uint64_t rb64 = (uint64_t)(uintptr_t)ob + (uint64_t)(uint32_t)dy * (uint32_t)((FP16 ? 6 : 3) * out_w);
    gbyte_t *orow = (gbyte_t *)(uintptr_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(rb64 >> 32)) << 32) |
                                           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)rb64));
    const uint32_t xoff = (uint32_t)((FP16 ? 6 : 3) * dx0);
    if (FP16) {  // LUT entry (v, c) at lutb + 2 v + 512 c (lut_ld)
      auto la = [&](uint32_t b) { return lutb + 2u * (b & 0xffu); };
      const uint32_t h0 = lut_ld(la(o[0]), 0), h1 = lut_ld(la(o[1]), 1), h2 = lut_ld(la(o[2]), 2);
      const uint32_t h3 = lut_ld(la(o[3]), 0), h4 = lut_ld(la(o[4]), 1), h5 = lut_ld(la(o[5]), 2);
      typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
      u32x3 w;
      w.x = h0 | (h1 << 16);
      w.y = h2 | (h3 << 16);
      w.z = h4 | (h5 << 16);
      __builtin_nontemporal_store(w, (__attribute__((address_space(1))) u32x3 *)(orow + xoff));
    } else {
      __attribute__((address_space(1))) uint16_t *o16 =
          (__attribute__((address_space(1))) uint16_t *)(orow + xoff);  // low bytes of two values: v_perm
      o16[0] = (uint16_t)__builtin_amdgcn_perm(o[1], o[0], 0x0c0c0400u);
      o16[1] = (uint16_t)__builtin_amdgcn_perm(o[3], o[2], 0x0c0c0400u);
      o16[2] = (uint16_t)__builtin_amdgcn_perm(o[5], o[4], 0x0c0c0400u);
    }
  }
}
// One band of BAND output rows of image k (one per K2 workgroup; the
// band-loop form of round 4 was deleted in round 6: slower at the driver's
// launch sizes, equal at 400 steps).  Every barrier inside is reached by all threads;
// the only thread-level return follows the last one.
template <int MODE, bool FP16>
FFCV_DEV void k2_band(const JpegArgs &a, const int k, const int band, uint8_t *lds) {
  lds_u16_t *s_lut = (lds_u16_t *)lds;  // 768 entries (FP16), channel-major
  const int t = threadIdx.x;
  // ---- one round trip for everything that depends only on (k, band, t):
  // the record head, the LUT, this band's row taps, this thread's column
  // taps and the epilogue draws (see K2Rec)
  K2Rec R;
  R.load(a.info + k, t);
  constexpr int LU = (768 + K2T - 1) / K2T;
  uint16_t lv[LU];
  if (FP16) {
#pragma unroll
    for (int u = 0; u < LU; u++) lv[u] = u * K2T + t < 768 ? lut_src(a.p.lut, u * K2T + t) : (uint16_t)0;
  }
  const int band_rows_n = MODE == JM_RRC ? min(a.p.out_h - band * BAND, BAND) : 0;
  // K1 writes an image's tap table only when out_w + out_h fits K2_TAPS: a
  // larger output never reads it (and past the last image the index would
  // leave the allocation)
  const uint2 *ktaps = MODE == JM_RRC && a.taps && a.p.out_w + a.p.out_h <= K2_TAPS
                           ? a.taps + (uint64_t)k * K2_TAPS
                           : nullptr;
  uint2 rt_pre = make_uint2(0, 0);
  uint4 ct_pre = make_uint4(0, 0, 0, 0);
  if (ktaps) {
    if (t < band_rows_n) rt_pre = ktaps[a.p.out_w + band * BAND + t];
    if (2 * (t % K2_COLS) + 1 < a.p.out_w) ct_pre = *(const uint4 *)(ktaps + 2 * (t % K2_COLS));
  }
  // (the band record: its selector and what the first phase, the tile
  // staging, reads)
  K2Band B;
  uint32_t b_fmt = 0, b_trp[3] = {0, 0, 0}, b_tos[3] = {0, 0, 0};
  uint64_t b_pbase[3] = {0, 0, 0};
  if (MODE == JM_RRC) {
    B.load(a.brec + ((uint64_t)k * a.brec_bands + band));
    b_fmt = B.u(K2BF(fmt));
#pragma unroll
    for (int c = 0; c < 3; c++) {
      b_trp[c] = B.u(K2BF(trp) + c);
      b_tos[c] = B.u(K2BF(tos) + c);
      b_pbase[c] = B.u64(K2BF(pbase) + 2 * c);
    }
  }
  const int cut_y0 = a.cut ? a.cut[2 * k] : 0, cut_x0 = a.cut ? a.cut[2 * k + 1] : 0;
  const int flip0 = a.flips ? a.flips[k] : 0;
  if (k == 0 && band == 0 && t == 0) {  // K1 is done: close its arena (see arena_before_k1)
    const unsigned long long top = a.arena_top[0];
    if (top) {
      a.arena_top[1] = top;
      a.arena_top[0] = 0;
    }
  }
  const int status = R.s(K2F(status));
  if (status == -1) return;  // raw sample (handled by the raw kernel)
  const int out_h = MODE == JM_FULL ? (int)a.samples[k].height : a.p.out_h;
  const int out_w = MODE == JM_FULL ? (int)a.samples[k].width : a.p.out_w;
  const int oy0 = band * BAND, oy1 = min(out_h, oy0 + BAND);
  if (oy0 >= out_h) return;
  char *ob = (char *)a.out + a.out_stride * k;
  const int esz = FP16 ? 2 : 1;
  if (status != FFCV_SAMPLE_OK) {  // zero-fill this band
    if (MODE == JM_RRC) {
      uint64_t row = (uint64_t)out_w * 3 * esz;
      for (uint64_t i = t; i < row * (oy1 - oy0); i += K2T) ob[row * oy0 + i] = 0;
    }
    return;
  }
  if (MODE == JM_FULL) {
    const ImgInfo I = k2_head(R);
    const ColorGeom G = color_geom(I);
    GPlane gp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) gp[c] = GPlane{a.arena + I.poff[c], I.stride[c]};
    uint8_t *o = (uint8_t *)ob;
    for (int i = t; i < (oy1 - oy0) * out_w; i += K2T) {
      int y = oy0 + i / out_w, x = i % out_w;
      int v[3];
      pixel_rgb(G, gp, y, x, v);
      uint8_t *d = o + ((uint64_t)y * out_w + x) * 3;
      d[0] = (uint8_t)v[0];
      d[1] = (uint8_t)v[1];
      d[2] = (uint8_t)v[2];
    }
    return;
  }
  if (FP16) {  // (loaded at the top)
#pragma unroll
    for (int u = 0; u < LU; u++)
      if (u * K2T + t < 768) s_lut[u * K2T + t] = lv[u];
  }
  // Epilogue parameters (flip, cutout) of this image
  Epilogue ep;
  ep.out_h = out_h;
  ep.out_w = out_w;
  ep.cut_size = a.cut ? a.p.cutout_size : 0;
  ep.cut_y = cut_y0;
  ep.cut_x = cut_x0;
  ep.flip = flip0;
  ep.cut_before_flip = a.p.cutout_fill[3];
  ep.fill[0] = a.p.cutout_fill[0];
  ep.fill[1] = a.p.cutout_fill[1];
  ep.fill[2] = a.p.cutout_fill[2];

  // ---- fast paths, selected per band by K1b (k2_write_band_rec).
  // Linear (kind 3 with the SSE2 vertical body on every element: every RRC
  // crop that is upscaled along some axis at out_w 224).
  // LDS: [LUT][row taps][component tiles, dword rows][crop rows as RGBx
  // words].  Each thread owns one output column pair and walks its half of
  // the band's rows, keeping the two source rows' horizontal sums in
  // registers (resize.cpp HResizeLinear -> VResizeLinearVec_32s8u).
  // Area (round 6): INTER_AREA crops with both scales in [1, 2) (every RRC
  // crop larger than the output on both axes, up to 2x) of 4:2:0 images: the
  // same tiles and colour pass, the crop rows kept as packed RGB (3 bytes per
  // pixel: 4-byte words would not fit a band's ~20 rows of up to 256 px), then
  // a column-pair walk with one cached row of horizontal sums (as
  // rrc_raw_kernel's area walk).  These bands took the general per-pixel
  // path before, ~3x the time of a linear band (r5z2_c3_k2_by_crop_perband.log).
  if (MODE == JM_RRC && (b_fmt & 3u) != K2B_GENERAL) {
    const uint32_t fmt = b_fmt;
    const bool area_fast = (fmt & 3u) == K2B_AREA;
    const int lut_b = FP16 ? 1536 : 0;
    LinTap *rtab = (LinTap *)(lds + lut_b);
    AreaTaps *atab = (AreaTaps *)(lds + lut_b);
    const uint2 *taps = (fmt & K2B_TAPS) ? ktaps : nullptr;
    {
      K2_STOP_AT(1, a.out_stride != 77);  // diagnostics: the band's set-up (record, LUT, taps)
      // ---- phase 1: row taps and tile staging
      if (!area_fast && t < oy1 - oy0) {  // weights stored as the walk's multiplier operands, c << 8 (see hrow)
        // (no table: out_w + out_h > K2_TAPS; the f64 scales come from the image record)
        LinTap lt = taps ? tap_unpack(rt_pre)
                         : lin_tap(R.f64(K2F(plan.scale_y)), R.f64(K2F(plan.inv_y)), B.s(K2BF(sh)), oy0 + t);
        lt.c0 = (lt.c0 & 0xfff) << 8;
        lt.c1 = (lt.c1 & 0xfff) << 8;
        rtab[t] = lt;
      }
      // tile staging: the first SU dwords per thread of every component are
      // loaded before any LDS write (one memory round trip, not one per
      // dword); row = i / wpr by a float reciprocal: exact while the +0.5
      // margin, 0.5 / (i + 0.5) relative, exceeds v_rcp_f32's 1 ulp plus the
      // product's rounding (i < 2^20; tiles here hold < 2^13 dwords)
      // Round 6: (float)i + 0.5 as t's float plus a constant, and the dword's
      // address as a 32-bit offset (24-bit multiply-add: tile offsets stay
      // below 2^24) from the component's scalar base (the saddr form) instead
      // of 64-bit address arithmetic per dword
      constexpr int SU = 4;
      uint32_t sv[3][SU];
      const float ft = (float)t + 0.5f;
      typedef const __attribute__((address_space(1))) uint8_t gu8_t;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int trows = (int)(b_trp[c] & 0xffffu), tpitch = (int)(b_trp[c] >> 16);
        const int wpr = max(tpitch >> 2, 1), n = trows * (tpitch >> 2);
        const float rwp = __builtin_amdgcn_rcpf((float)wpr);  // (1 ulp: far inside the +0.5 margin)
        gu8_t *src = (gu8_t *)(uintptr_t)(a.arena + b_pbase[c]);
        const uint32_t st = (b_tos[c] >> 16) << 3;
#pragma unroll
        for (int u = 0; u < SU; u++) {
          const int i = u * K2T + t;
          const int rr = (int)((ft + (float)(u * K2T)) * rwp), q = i - __mul24(rr, wpr);
          sv[c][u] = i < n ? *(const __attribute__((address_space(1))) uint32_t *)(src + (__umul24((uint32_t)rr, st) + 4u * (uint32_t)q)) : 0u;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int trows = (int)(b_trp[c] & 0xffffu), tpitch = (int)(b_trp[c] >> 16);
        uint32_t *tl = (uint32_t *)(lds + (b_tos[c] & 0xffffu));
        const int wpr = max(tpitch >> 2, 1), n = trows * (tpitch >> 2);
#pragma unroll
        for (int u = 0; u < SU; u++)
          if (u * K2T + t < n) tl[u * K2T + t] = sv[c][u];
        const uint8_t *src = a.arena + b_pbase[c];
        const uint32_t st = (b_tos[c] >> 16) << 3;
        const float rwp = __builtin_amdgcn_rcpf((float)wpr);
        for (int i = SU * K2T + t; i < n; i += K2T) {  // big tiles
          const int rr = (int)(((float)i + 0.5f) * rwp), q = i - __mul24(rr, wpr);
          tl[i] = *(const uint32_t *)(src + (uint64_t)rr * st + 4 * q);
        }
      }
      // (after the tiles: its f64 arithmetic would raise the register peak
      // while the tile loads are in flight)
      if (area_fast && t < oy1 - oy0) atab[t] = area_taps(B.s(K2BF(sh)), B.f64(K2BF(scale_y)), oy0 + t);
      __syncthreads();
      K2_STOP_AT(2, a.out_stride != 77);  // diagnostics: + the plane tiles
      // ---- phase 2: the colour pass, on its own fields of the record
      B.phase();
      TPlane tp[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint32_t tyx = B.u(K2BF(tyx) + c);
        tp[c] = TPlane{lds + (B.u(K2BF(tos) + c) & 0xffffu), (int)(tyx & 0xffffu), (int)(tyx >> 16),
                       (int)(B.u(K2BF(trp) + c) >> 16)};
      }
      const int r0c = B.s(K2BF(r0)), nrows = B.s(K2BF(nrows)), rw = B.s(K2BF(rw));
      const int Y0 = B.s(K2BF(ri)) + r0c, Y1 = Y0 + nrows - 1, X0 = B.s(K2BF(rj)), X1 = X0 + rw - 1;
      uint32_t *rgbx = (uint32_t *)(lds + (B.u(K2BF(rgbp)) & 0xffffu));
      const int pitch3 = (int)(B.u(K2BF(rgbp)) >> 16);
      if (fmt & K2B_Q420) {  // (every area_fast band)
        // 4:2:0 (jdsample.c h2v2_fancy_upsample, as upsample_quad_h2v2): each
        // thread owns a pair of adjacent chroma columns (C, C + 1) and walks
        // every ng-th chroma row of the band.  Column clamps, edge terms and
        // offsets are computed once per thread; per row the 3 x 4 chroma
        // neighbourhood of the two quads is read once per plane and its
        // vertical sums (3 * centre + above / below) are shared by both quads.
        // Pixels outside the crop go to a dummy LDS word (branch-free).
        const int R0 = Y0 >> 1, R1 = Y1 >> 1, C0 = X0 >> 1, C1 = X1 >> 1;
        const int npairs = (C1 - C0 + 2) >> 1;
        const int ps = min(npairs, K2T);  // pairs per sweep of the workgroup
        const float rp = __builtin_amdgcn_rcpf((float)ps);
        // ng row groups; t = g * ps + pair (quotients by a float reciprocal:
        // exact for these small operands, as in the tile staging)
        const int ng = (int)(((float)K2T + 0.5f) * rp);
        const int g = (int)(((float)t + 0.5f) * rp);
        if (g < ng)
        for (int pr = t - __mul24(g, ps); pr < npairs; pr += ps) {
          const int C = C0 + 2 * pr;
          // plane columns of the two quads' neighbourhoods (clamped like
          // upsample_quad_h2v2; the fourth is unused without a second quad)
          const int cw = (int)(B.u(K2BF(cwh) + 1) & 0xffffu), ch = (int)(B.u(K2BF(cwh) + 1) >> 16);
          const int xm = max(C - 1, 0) - tp[1].c0, x0 = C - tp[1].c0;
          const int x1 = min(C + 1, cw - 1) - tp[1].c0, x2 = min(C + 2, min(C1 + 1, cw - 1)) - tp[1].c0;
          // luma columns 2C .. 2C + 3: inside the crop?  (reads clamped into it)
          const int X = 2 * C;
          bool vx[4];
          int lx[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            vx[j] = X + j >= X0 && X + j <= X1;
            lx[j] = min(max(X + j, X0), X1) - tp[0].c0;
          }
          uint32_t *dummy = rgbx + nrows * rw;
          for (int R = R0 + g; R <= R1; R += ng) {
            const int ru = max(R - 1, 0), rd = min(R + 1, ch - 1);
            int qb[2][8];  // [plane][quad u: C's q0..q3, then C + 1's]
#pragma unroll
            for (int pl = 0; pl < 2; pl++) {
              const uint8_t *b = tp[1 + pl].p;
              const int pitch = tp[1 + pl].pitch, ty = tp[1 + pl].r0;
              const uint8_t *rm = b + __mul24(R - ty, pitch), *ra = b + __mul24(ru - ty, pitch),
                            *rb = b + __mul24(rd - ty, pitch);
              const int mm = rm[xm], m0 = rm[x0], m1 = rm[x1], m2 = rm[x2];
              // vertical sums above (T) and below (B) for columns xm, x0, x1, x2
              const int Tm = 3 * mm + ra[xm], T0 = 3 * m0 + ra[x0], T1 = 3 * m1 + ra[x1], T2 = 3 * m2 + ra[x2];
              const int Bm = 3 * mm + rb[xm], B0 = 3 * m0 + rb[x0], B1 = 3 * m1 + rb[x1], B2 = 3 * m2 + rb[x2];
              qb[pl][0] = (3 * T0 + Tm + 8) >> 4;
              qb[pl][1] = (3 * T0 + T1 + 7) >> 4;
              qb[pl][2] = (3 * B0 + Bm + 8) >> 4;
              qb[pl][3] = (3 * B0 + B1 + 7) >> 4;
              qb[pl][4] = (3 * T1 + T0 + 8) >> 4;
              qb[pl][5] = (3 * T1 + T2 + 7) >> 4;
              qb[pl][6] = (3 * B1 + B0 + 8) >> 4;
              qb[pl][7] = (3 * B1 + B2 + 7) >> 4;
            }
            if (area_fast) {  // four packed RGB pixels per row: 3 words at byte 12 * pr of the row
#pragma unroll
              for (int dy = 0; dy < 2; dy++) {
                const int Y = 2 * R + dy;
                const uint8_t *ly = tp[0].p + __mul24(min(max(Y, Y0), Y1) - tp[0].r0, tp[0].pitch);
                uint32_t px[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                  const int u = (j >> 1) * 4 + dy * 2 + (j & 1);
                  int v[3];
                  ycc_rgb(ly[lx[j]], qb[0][u], qb[1][u], v);
                  px[j] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
                }
                if (Y >= Y0 && Y <= Y1) {
                  uint32_t *d = rgbx + __mul24(Y - Y0, pitch3 >> 2) + 3 * pr;
                  d[0] = px[0] | (px[1] << 24);
                  d[1] = (px[1] >> 8) | (px[2] << 16);
                  d[2] = (px[2] >> 16) | (px[3] << 8);
                }
              }
              continue;
            }
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
              const int Y = 2 * R + dy;
              const bool vy = Y >= Y0 && Y <= Y1;
              const uint8_t *ly = tp[0].p + __mul24(min(max(Y, Y0), Y1) - tp[0].r0, tp[0].pitch);
              uint32_t *orow = rgbx + __mul24(Y - Y0, rw) - X0;
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int u = (j >> 1) * 4 + dy * 2 + (j & 1);  // quad, then its q index
                int v[3];
                ycc_rgb(ly[lx[j]], qb[0][u], qb[1][u], v);
                uint32_t *d = vy && vx[j] ? orow + X + j : dummy;
                *d = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
              }
            }
          }
        }
      } else {
        ColorGeom G;  // (the record's packed format)
        G.ncomp = (int)((fmt >> K2B_NCOMP_SH) & 3u);
        G.color_rgb = (fmt & K2B_RGB) != 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          G.he[c] = 1 << ((fmt >> (K2B_EXP_SH + 4 * c)) & 3u);
          G.ve[c] = 1 << ((fmt >> (K2B_EXP_SH + 4 * c + 2)) & 3u);
          G.cw[c] = (int)(B.u(K2BF(cwh) + c) & 0xffffu);
          G.ch[c] = (int)(B.u(K2BF(cwh) + c) >> 16);
        }
        for (int i = t; i < nrows * rw; i += K2T) {
          const int yy = i / rw, x = i - yy * rw;
          int v[3];
          pixel_rgb(G, tp, Y0 + yy, X0 + x, v);
          rgbx[i] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
        }
      }
      __syncthreads();
      K2_STOP_AT(3, a.out_stride != 77);  // diagnostics: + the colour pass
      const int tx = t % K2_COLS, sub = t / K2_COLS;
      if (tx >= out_w / 2) return;
      const int dx0 = 2 * tx;
      // ---- phase 3: the walk, on its own fields of the record
      B.phase();
      const int r0 = B.s(K2BF(r0)), psh = B.s(K2BF(sh));
      const uint32_t *wrgb = (const uint32_t *)(lds + (B.u(K2BF(rgbp)) & 0xffffu));
      if (area_fast) {
        const int rj = B.s(K2BF(rj));
        k2_area_walk<FP16>(ep, B.s(K2BF(sw)), B.f64(K2BF(scale_x)), atab, (const uint8_t *)wrgb,
                           (int)(B.u(K2BF(rgbp)) >> 16), 3 * (rj - 2 * (rj >> 1)), r0, oy0, oy1, sub, dx0,
                           lut_base(s_lut), ob);
        return;
      }
      const int wrw = B.s(K2BF(rw));
      LinTap l0, l1;
      if (taps) {  // K1's table (flip applied): both columns in one 16-byte load (at the top)
        const uint4 q = ct_pre;
        l0 = tap_unpack(make_uint2(q.x, q.y));
        l1 = tap_unpack(make_uint2(q.z, q.w));
      } else {
        const double sx = R.f64(K2F(plan.scale_x)), ix = R.f64(K2F(plan.inv_x));
        l0 = lin_tap(sx, ix, B.s(K2BF(sw)), ep.src_x(dx0));
        l1 = lin_tap(sx, ix, B.s(K2BF(sw)), ep.src_x(dx0 + 1));
      }
      // a border tap (src[s] * 2048) as the same two-tap form with weights
      // (2048, 0) on (s, s + 1): branch-free, identical sums
      const int a0w = l0.border ? 2048 : l0.c0, b0w = l0.border ? 0 : l0.c1;
      const int a1w = l1.border ? 2048 : l1.c0, b1w = l1.border ? 0 : l1.c1;
      // horizontal pass of crop row r for both columns: sat_s16(h >> 4) per
      // channel.  The saturations of this walk never act (so they are not
      // computed): weights are in [0, 2048] with c0 + c1 <= 2049 (linear_coef
      // rounds each), so 0 <= h >> 4 <= 255 * 2049 >> 4 = 32655 and the
      // vertical sum m0 + m1 <= 32655 * 2049 >> 16 = 1020, (1020 + 2) >> 2 = 255.
      // The rows keep (h >> 4) << 8 (< 2^23), so VResizeLinearVec's
      // (h * c) >> 16 is one 24-bit high multiply by c << 8 (< 2^20):
      // mulhi_u24(h << 8, c << 8) = (h * c * 2^16) >> 32.
      // On gfx950 every multiply, bit-field extract and 3-operand integer
      // form issues in 4 cycles per wave against 2 for add / shift / and
      // (tools/op_rate), so the pair of a channel's two source samples is
      // gathered by one v_perm_b32 as u16 halves and weighted by one
      // v_dot2_u32_u16 with the weights pre-scaled by 16: dot = 16 h, and
      // (h >> 4) << 8 = dot & 0x7fff00 (10 cycles per value instead of 22).
      const uint32_t w0 = ((uint32_t)a0w << 4) | ((uint32_t)b0w << 20), w1 = ((uint32_t)a1w << 4) | ((uint32_t)b1w << 20);
      const uint32_t so0 = 4u * (uint32_t)l0.s, so1 = 4u * (uint32_t)l1.s;  // byte offsets in a row
      auto hrow = [&](int r, uint32_t H[6]) {
        const uint32_t *row = wrgb + __mul24(r - r0, wrw);
        // words s and s + 1 as one ds_read2 per column (a border tap's second
        // word has weight 0: at the crop's right edge it is the next row's
        // first word or, in the last row, the dummy word)
        const uint32_t *e0 = (const uint32_t *)((const uint8_t *)row + so0), *e1 = (const uint32_t *)((const uint8_t *)row + so1);
        const uint32_t p0 = e0[0], q0 = e0[1];
        const uint32_t p1 = e1[0], q1 = e1[1];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          // bytes [p.c, 0, q.c, 0]: v_perm_b32 selector c | 0x0c << 8 | (4 + c) << 16 | 0x0c << 24
          const uint32_t sel = (uint32_t)c | 0x0c00u | ((uint32_t)(4 + c) << 16) | 0x0c000000u;
          H[c] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, __builtin_amdgcn_perm(q0, p0, sel)),
                                        __builtin_bit_cast(u16x2_t, w0), 0u, false) & 0x7fff00u;
          H[3 + c] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, __builtin_amdgcn_perm(q1, p1, sel)),
                                            __builtin_bit_cast(u16x2_t, w1), 0u, false) & 0x7fff00u;
        }
      };
      auto mulhi24 = [](uint32_t x, uint32_t y) -> uint32_t {  // x, y < 2^24: v_mul_hi_u32_u24
        return (uint32_t)(((uint64_t)(x & 0xffffffu) * (y & 0xffffffu)) >> 32);
      };
      // cutout: which of this thread's two columns lie in the square (tested
      // once; a row tests its own range)
      const bool cut0 = ep.in_cut(ep.cut_y, dx0), cut1 = ep.in_cut(ep.cut_y, dx0 + 1);
      const uint32_t lq = FP16 ? 2u + 2u * lut_base(s_lut) : 2u;  // (lut_q)
      uint32_t qfill[3];  // the cutout fill as lut_q's result
      for (int c = 0; c < 3; c++) qfill[c] = FP16 ? lut_base(s_lut) + 2u * ep.fill[c] : ep.fill[c];
      const int half = (BAND + K2T / K2_COLS - 1) / (K2T / K2_COLS);  // rows per row group
      // (a row group is two whole waves: its rows are wave-uniform, so the
      // per-row tap read, cutout test and row changes are scalar)
      const int ya = __builtin_amdgcn_readfirstlane(oy0 + sub * half);
      const int yb = __builtin_amdgcn_readfirstlane(min(oy1, ya + half));
      int ca = -1, cb = -1;
      uint32_t HA[6], HB[6];
      for (int dy = ya; dy < yb; dy++) {
        const LinTap ly = rtab[dy - oy0];
        const int ra = min(max(ly.s, 0), psh - 1), rb = min(max(ly.s + 1, 0), psh - 1);
        if (ra != ca) {
          if (ra == cb) {
#pragma unroll
            for (int i = 0; i < 6; i++) HA[i] = HB[i];
          } else {
            hrow(ra, HA);
          }
          ca = ra;
        }
        if (rb != cb) {
          hrow(rb, HB);
          cb = rb;
        }
        uint32_t o[6];
        const uint32_t c0 = ly.c0, c1 = ly.c1;  // (pre-scaled in rtab)
#pragma unroll
        for (int i = 0; i < 6; i++)  // (sat_s16(m0 + m1) + 2) >> 2, no saturation (see hrow); FP16: its LUT address
          o[i] = lut_q<FP16>(mulhi24(HA[i], c0) + mulhi24(HB[i], c1), lq);
        if ((cut0 || cut1) && dy >= ep.cut_y && dy < ep.cut_y + ep.cut_size) {
          if (cut0) {
            o[0] = qfill[0];
            o[1] = qfill[1];
            o[2] = qfill[2];
          }
          if (cut1) {
            o[3] = qfill[0];
            o[4] = qfill[1];
            o[5] = qfill[2];
          }
        }
        // (round 6) the row's address is wave-uniform (dy is): scalar base +
        // this thread's fixed 32-bit offset (the store's saddr form), no
        // 64-bit address arithmetic per row
        typedef __attribute__((address_space(1))) uint8_t gbyte_t;
        const uint64_t rb64 = (uint64_t)(uintptr_t)ob + (uint64_t)(uint32_t)dy * (uint32_t)(3 * esz * out_w);
        gbyte_t *orow = (gbyte_t *)(uintptr_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(rb64 >> 32)) << 32) |
                                               (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)rb64));
        const uint32_t xoff = (uint32_t)(3 * esz * dx0);
        if (FP16) {
          const uint32_t h0 = lut_ld(o[0], 0), h1 = lut_ld(o[1], 1), h2 = lut_ld(o[2], 2);
          const uint32_t h3 = lut_ld(o[3], 0), h4 = lut_ld(o[4], 1), h5 = lut_ld(o[5], 2);
          typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));  // 12-byte group, 4-byte aligned
          u32x3 w;
          w.x = h0 | (h1 << 16);
          w.y = h2 | (h3 << 16);
          w.z = h4 | (h5 << 16);
          // streaming output: non-temporal (measured +2.7% C3 over plain stores)
          __builtin_nontemporal_store(w, (__attribute__((address_space(1))) u32x3 *)(orow + xoff));
        } else {
          __attribute__((address_space(1))) uint16_t *o16 = (__attribute__((address_space(1))) uint16_t *)(orow + xoff);
          o16[0] = (uint16_t)(o[0] | (o[1] << 8));
          o16[1] = (uint16_t)(o[2] | (o[3] << 8));
          o16[2] = (uint16_t)(o[4] | (o[5] << 8));
        }
      }
      return;
    }
  }
  // ---- general path: the image record's head (as every band before the
  // band records), its own set-up
  const ImgInfo I = k2_head(R);
  const ColorGeom G = color_geom(I);
  const int ncomp = G.ncomp;
  GPlane gp[3];
#pragma unroll
  for (int c = 0; c < 3; c++) gp[c] = GPlane{a.arena + I.poff[c], I.stride[c]};
  const int ri = I.ri, rj = I.rj, rw = I.rw;
  const ResizePlan P = I.plan;  // K1's plan
  int r0, r1;
  band_rows(P, oy0, oy1, &r0, &r1);
  const int nrows = r1 - r0 + 1;
  const int step = rw * 3;
  // diagnostics (K1's stamp buffer, slot 11): bands of this image that take
  // the general path below
  if (a.dbg && t == 0) atomicAdd((unsigned long long *)(a.dbg + (uint64_t)k * 16 + 11), 1ull);
  // LDS: [LUT][column + row taps][component tiles][RGB rows].  The taps of
  // the band's rows and of every output column are computed once per
  // workgroup; the tiles cover every plane sample the band's upsampling
  // reads, so the colour pass runs from LDS.
  const int tap_b = (P.kind == 2 ? (int)sizeof(AreaTaps) : (P.kind == 3 ? (int)sizeof(LinTap) : 0)) * (out_w + BAND);
  const int lut_b = (FP16 ? 1536 : 0) + ((tap_b + 15) & ~15);
  AreaTaps *atab = (AreaTaps *)(lds + (FP16 ? 1536 : 0));
  LinTap *ltab = (LinTap *)atab;
  int ty0[3], tx0[3], trows[3], tcols[3], toff[3];
  int need = lut_b;
#pragma unroll
  for (int c = 0; c < 3; c++) {  // (unrolled: no dynamically indexed arrays)
    if (c >= ncomp) {
      ty0[c] = tx0[c] = trows[c] = tcols[c] = toff[c] = 0;
      continue;
    }
    const int he = G.he[c], ve = G.ve[c];
    int y0 = (ri + r0) / ve - (ve == 2 ? 1 : 0), y1 = (ri + r1) / ve + (ve == 2 ? 1 : 0);
    int x0 = rj / he - (he == 2 ? 1 : 0), x1 = (rj + rw - 1) / he + (he == 2 ? 1 : 0);
    y0 = max(y0, 0);
    x0 = max(x0, 0);
    y1 = min(y1, G.ch[c] - 1);
    x1 = min(x1, G.cw[c] - 1);
    ty0[c] = y0;
    tx0[c] = x0;
    trows[c] = y1 - y0 + 1;
    tcols[c] = x1 - x0 + 1;
    toff[c] = need;
    need += (trows[c] * tcols[c] + 15) & ~15;
  }
  const int roi_off = need;
  need += nrows * step;
  const bool tiled = need <= K2_LDS;
  const bool staged = tiled || lut_b + nrows * step <= K2_LDS;  // (tap tables fit: see tabs)
  uint8_t *roi = lds + (tiled ? roi_off : lut_b);
  // Bands too wide for LDS stage their rows in the image's rgb slot at their
  // absolute crop-row position; rows shared with a neighbouring band are
  // written with identical bytes by both.
  uint8_t *groi = a.arena + I.rgb_off;
  uint8_t *dst = staged ? roi : groi + (uint64_t)r0 * step;
  const bool tabs = tap_b > 0 && lut_b <= K2_LDS / 2;
  if (tabs) {  // [0, out_w): columns, [out_w, out_w + rows): the band's rows
    for (int i = t; i < out_w + (oy1 - oy0); i += K2T) {
      if (P.kind == 2)
        atab[i] = i < out_w ? area_taps(P.sw, P.scale_x, i) : area_taps(P.sh, P.scale_y, oy0 + i - out_w);
      else
        ltab[i] = i < out_w ? lin_tap(P.scale_x, P.inv_x, P.sw, i) : lin_tap(P.scale_y, P.inv_y, P.sh, oy0 + i - out_w);
    }
  }
  if (tiled) {
    TPlane tp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      uint8_t *tl = lds + toff[c];
      const int cols = tcols[c], n = trows[c] * cols;
      const uint8_t *src = gp[c].p + (uint64_t)ty0[c] * gp[c].stride + tx0[c];
      for (int i = t; i < n; i += K2T) {
        const int rr = i / cols, cc = i - rr * cols;
        tl[rr * cols + cc] = src[(uint64_t)rr * gp[c].stride + cc];
      }
      tp[c] = TPlane{tl, ty0[c], tx0[c], cols};
    }
    __syncthreads();
    const bool q420 = ncomp == 3 && !G.color_rgb && G.he[0] == 1 && G.ve[0] == 1 && G.he[1] == 2 &&
                      G.ve[1] == 2 && G.he[2] == 2 && G.ve[2] == 2 && G.cw[1] > 2 && G.cw[2] > 2;
    if (q420) {  // one thread per chroma sample: a 2x2 quad of pixels
      const int Y0 = ri + r0, Y1 = ri + r1, X0 = rj, X1 = rj + rw - 1;
      const int R0 = Y0 >> 1, C0 = X0 >> 1, qcols = (X1 >> 1) - C0 + 1;
      const int nq = ((Y1 >> 1) - R0 + 1) * qcols;
      for (int i = t; i < nq; i += K2T) {
        const int qr = i / qcols, R = R0 + qr, C = C0 + (i - qr * qcols);
        int cb[4], cr[4];
        upsample_quad_h2v2(tp[1], G.cw[1], G.ch[1], R, C, cb);
        upsample_quad_h2v2(tp[2], G.cw[2], G.ch[2], R, C, cr);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int Y = 2 * R + (u >> 1), X = 2 * C + (u & 1);
          if (Y < Y0 || Y > Y1 || X < X0 || X > X1) continue;
          int v[3];
          ycc_rgb(tp[0].at(Y, X), cb[u], cr[u], v);
          uint8_t *d = dst + (Y - Y0) * step + (X - X0) * 3;
          d[0] = (uint8_t)v[0];
          d[1] = (uint8_t)v[1];
          d[2] = (uint8_t)v[2];
        }
      }
    } else {
      for (int i = t; i < nrows * rw; i += K2T) {
        int yy = i / rw, x = i - yy * rw;
        int v[3];
        pixel_rgb(G, tp, ri + r0 + yy, rj + x, v);
        uint8_t *d = dst + yy * step + x * 3;
        d[0] = (uint8_t)v[0];
        d[1] = (uint8_t)v[1];
        d[2] = (uint8_t)v[2];
      }
    }
  } else {
    for (int i = t; i < nrows * rw; i += K2T) {
      int yy = i / rw, x = i - yy * rw;
      int v[3];
      pixel_rgb(G, gp, ri + r0 + yy, rj + x, v);
      uint8_t *d = dst + (uint64_t)yy * step + x * 3;
      d[0] = (uint8_t)v[0];
      d[1] = (uint8_t)v[1];
      d[2] = (uint8_t)v[2];
    }
  }
  // Separable linear (kind 3): OpenCV's horizontal pass depends only on the
  // source row, so each (row, column) tap pair is computed once per band and
  // kept as the saturated int16 (h >> 4) the vertical SIMD body consumes
  // (resize.cpp VResizeLinearVec_32s8u).  Columns in the scalar tail
  // (>= vec_end) keep the per-pixel path.
  const int hoff = (((tiled ? roi_off : lut_b) + nrows * step) + 15) & ~15;
  const bool sep = P.kind == 3 && staged && tabs && hoff + nrows * out_w * 8 <= K2_LDS;
  uint2 *H = (uint2 *)(lds + hoff);
  __syncthreads();
  if (sep) {
    for (int i = t; i < nrows * out_w; i += K2T) {
      const int rr = i / out_w, cx = i - rr * out_w;
      const LinTap lx = ltab[cx];
      const uint8_t *q = roi + rr * step + lx.s * 3;
      int hv[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int h = lx.border ? q[c] * 2048 : q[c] * lx.c0 + q[c + 3] * lx.c1;
        hv[c] = sat_s16i(h >> 4);
      }
      H[i] = make_uint2((uint32_t)(hv[0] & 0xffff) | ((uint32_t)hv[1] << 16), (uint32_t)(hv[2] & 0xffff));
    }
    __syncthreads();
  }
  LdsRoi lr{roi, r0, step};
  // resize_area_lds reads up to 5 bytes past the staged rows
  const bool pad8 = (int)(roi - lds) + nrows * step + 8 <= K2_LDS;
  RoiSrc gr{groi, (uint64_t)step};
  auto px = [&](int dy, int dx, int v[3]) {
    if (ep.in_cut(dy, dx)) {
      v[0] = ep.fill[0];
      v[1] = ep.fill[1];
      v[2] = ep.fill[2];
    } else if (sep && ep.src_x(dx) * 3 + 2 < P.vec_end) {
      const int cx = ep.src_x(dx);
      const LinTap ly = ltab[out_w + dy - oy0];
      const int ra = min(max(ly.s, 0), P.sh - 1) - r0, rb = min(max(ly.s + 1, 0), P.sh - 1) - r0;
      const uint2 A = H[ra * out_w + cx], Bv = H[rb * out_w + cx];
      const int a0[3] = {(int16_t)(A.x & 0xffff), (int16_t)(A.x >> 16), (int16_t)(A.y & 0xffff)};
      const int b0[3] = {(int16_t)(Bv.x & 0xffff), (int16_t)(Bv.x >> 16), (int16_t)(Bv.y & 0xffff)};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int m0 = __mul24(a0[c], ly.c0) >> 16, m1 = __mul24(b0[c], ly.c1) >> 16;
        v[c] = sat_u8i((sat_s16i(m0 + m1) + 2) >> 2);
      }
    } else if (staged && tabs) {
      const int cx = ep.src_x(dx);
      if (P.kind == 2 && pad8)  // (aligned reads: see resize_area_lds)
        resize_area_lds(lr, atab[cx], atab[out_w + dy - oy0], v);
      else if (P.kind == 2)
        resize_area(lr, atab[cx], atab[out_w + dy - oy0], v);
      else
        resize_linear(P, lr, cx, ltab[cx], ltab[out_w + dy - oy0], v);
    } else if (staged) {
      resize_pixel(P, lr, dy, ep.src_x(dx), v);
    } else {
      resize_pixel(P, gr, dy, ep.src_x(dx), v);
    }
  };
  // pixel pairs: 12 bytes (fp16) / 6 bytes (u8) per thread, 4-/2-byte
  // aligned when rows and samples start aligned; single pixels otherwise
  const bool pairs = (out_w & 1) == 0 && (a.out_stride & 3) == 0;
  const int per = pairs ? 2 : 1;
  const int hw = out_w / per;
  const int npx = (oy1 - oy0) * hw;
  for (int i = t; i < npx; i += K2T) {
    const int dy = oy0 + i / hw, dx = per * (i % hw);
    const bool two = pairs;
    int v[3], u[3];
    px(dy, dx, v);
    if (two) px(dy, dx + 1, u);
    const uint64_t p0 = (uint64_t)dy * out_w + dx;
    if (FP16) {
      uint16_t h0 = lut_at(s_lut, v[0], 0), h1 = lut_at(s_lut, v[1], 1), h2 = lut_at(s_lut, v[2], 2);
      uint16_t *o = (uint16_t *)ob + p0 * 3;
      if (two) {
        uint16_t h3 = lut_at(s_lut, u[0], 0), h4 = lut_at(s_lut, u[1], 1), h5 = lut_at(s_lut, u[2], 2);
        uint32_t *o32 = (uint32_t *)o;  // p0 even -> 12-byte aligned group
        o32[0] = h0 | ((uint32_t)h1 << 16);
        o32[1] = h2 | ((uint32_t)h3 << 16);
        o32[2] = h4 | ((uint32_t)h5 << 16);
      } else {
        o[0] = h0;
        o[1] = h1;
        o[2] = h2;
      }
    } else {
      uint8_t *o = (uint8_t *)ob + p0 * 3;
      if (two) {
        uint16_t *o16 = (uint16_t *)o;
        o16[0] = (uint16_t)(v[0] | (v[1] << 8));
        o16[1] = (uint16_t)(v[2] | (u[0] << 8));
        o16[2] = (uint16_t)(u[1] | (u[2] << 8));
      } else {
        o[0] = (uint8_t)v[0];
        o[1] = (uint8_t)v[1];
        o[2] = (uint8_t)v[2];
      }
    }
  }
}

template <int MODE, bool FP16>
__global__ void __launch_bounds__(K2T) __attribute__((amdgpu_waves_per_eu(K2_WPE))) jpeg_color_resize_kernel(JpegArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  k2_band<MODE, FP16>(a, (int)blockIdx.y, (int)blockIdx.x, lds);
}

// Diagnostics only (ffcv_jpeg_set_diag): a launch that runs K2 without K1b
// re-runs it on the previous launch's scratch, whose band records may be for
// another output size; this kernel rewrites them from the image records, one
// thread per (image, band), so K2 never reads records its own launch did not
// write.  The product path has no such launch: K1b writes them.
__global__ void __launch_bounds__(256) k2_rec_kernel(JpegArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = i / a.brec_bands, b = i - k * a.brec_bands;
  if (k >= a.batch) return;
  const ImgInfo &I = a.info[k];
  if (I.status != FFCV_SAMPLE_OK) return;
  // (the image record's plan and tap table: what such a launch's K2 used before)
  k2_write_band_rec(a.brec + i, InfoGeom{I}, I.plan, a.p.out_w, a.p.out_h, b, a.p.lut ? 1536 : 0, I.taps);
}
