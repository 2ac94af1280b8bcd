// ffcv_rrc.hip -- device random draws of the decoders and the raw-mode
// crop + INTER_AREA resize with a fused flip / cutout / LUT-normalize epilogue.
//
// Reference path (raw mode): rgb_image.py:202-208 takes a
// zero-copy view of the mmap'd sample, get_random_crop draws the window and
// libffcv.cpp:33-42 cv::resize(INTER_AREA) writes the output; Cutout
// (cutout.py:36-47) and NormalizeImage (normalize.py:65) follow as separate
// passes.  Here the .beton bytes are already resident in HBM, so one launch
// reads each crop ROI once and writes the final (u8 or fp16) pixels once.
#include "api_internal.h"
#include "device_common.h"
#include "diag_hooks.h"
#include "resize_out.h"

// ------------------------------------------------------------ draws -------
__global__ void __launch_bounds__(64) draw_kernel(const uint64_t *__restrict__ ids,
                                                  const ffcv_sample *__restrict__ samples, int B,
                                                  ffcv_draw_params p, int32_t *__restrict__ crops,
                                                  int32_t *__restrict__ cut, uint8_t *__restrict__ flips,
                                                  int32_t *__restrict__ status) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const uint64_t id = ids[k];
  const uint32_t H = crops ? samples[k].height : 0, W = crops ? samples[k].width : 0;
  int err = 0;
  for (int part = 0; part < 3; part++) err |= draw_part(part, k, id, H, W, p, crops, cut, flips);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// ------------------------------------------------ raw crop + resize -------
struct GlobalSrc {
  const uint8_t *p;
  uint64_t step;
  FFCV_DEV int at(int y, int x, int c) const { return p[(uint64_t)y * step + (uint64_t)x * 3 + c]; }
};

#define RRC_THREADS 256
static_assert(RRC_THREADS == 256, "rrc_band's row staging and walk assume four waves per workgroup");
#define RRC_BAND 16        // output rows per workgroup
#define RRC_STAGE_ROWS 5   // rows a wave stages per batch of loads in flight (2 x 16 B per lane each)
#define RRC_LDS_BYTES 30464  // source-row stage: the most that keeps 5 workgroups per CU with the LUT and tap tables (28 KB: 1% slower, 24 KB: 15% slower)
static_assert(RRC_LDS_BYTES % 16 == 0, "the stage is an array of 16-byte chunks");

// the band's staged crop rows (resize_out.h); the per-pixel functions read single bytes
typedef StagedRows<false> LdsSrc;

// One workgroup per band of RRC_BAND output rows of one image.
//   Staging: the band's source rows of the crop (band_rows) are copied into
//   LDS with 16-byte aligned global loads (an aligned chunk holding at least
//   one byte of the row never crosses a page, so the aligned-down/up edges
//   are safe), so each source byte is read from HBM once per band and every
//   tap after that is an LDS read.  Bands whose rows do not fit
//   RRC_LDS_BYTES read their taps from global memory instead.
//   Linear fast path (every crop upscaled along some axis, OpenCV's
//   "area-mode" linear with the SSE2 vertical body on every element): each
//   thread owns four adjacent output columns and walks a slice of the band's
//   rows, keeping the two source rows' horizontal sums in registers; the four
//   pixels leave as one 12-byte (u8) or three 8-byte (fp16) stores, so a wave
//   writes one contiguous run of the output row.
//   Otherwise (area downscale, copy, widths not a multiple of 4): the
//   per-pixel restatement, over the staged rows when they fit.
// rrc_taps_kernel's table: entries per image (even: 16-byte quads stay
// aligned): linear plans use out_w + out_h (columns, then rows), area plans at
// scales < 2 two per column (a 16-byte record: first tap, three weights)
#define RAW_TAPS(p) ((max((p).out_w + (p).out_h, 2 * (p).out_w) + 1) & ~1)
// an area plan whose column records rrc_taps_kernel writes: both scales < 2
// (scale_x = 1 / (dw / sw) < 2 exactly when sw < 2 dw)
FFCV_HD bool area_walk_plan(const ResizePlan &P) { return P.kind == 2 && P.sw < 2 * P.dw && P.sh < 2 * P.dh; }
#define RRC_WPE 5  // waves per SIMD the raw kernel is compiled for (5 workgroups per CU by LDS)
// LDS of one band
template <bool FP16>
struct RrcLds {
  uint16_t lut[FP16 ? 768 : 1];
  uint4 src[RRC_LDS_BYTES / 16];
  uint4 rt[RRC_BAND];  // linear row taps: {ra, rb, c0 << 8, c1 << 8}
  AreaTaps at[RRC_BAND];
};
// five workgroups per CU (160 KB of LDS): at most 32 KB each
static_assert(sizeof(RrcLds<false>) == 31184 && sizeof(RrcLds<true>) == 32704, "RrcLds: five workgroups per CU");

// What the parts of rrc_band share: one band (output rows [oy0, oy1)) of one image.
template <bool FP16>
struct Band {
  ResizePlan P;
  Epilogue ep;
  LdsSrc L;             // the staged source rows
  RrcLds<FP16> &S;      // LUT and row taps
  const uint2 *itaps;   // the image's table from rrc_taps_kernel, or null
  char *o;              // the image's output
  int oy0, oy1;
};

// A thread's share of a quad walk: columns dx0 .. dx0 + 3 of rows [gy0, gy1)
// (wave-uniform), and the quad's cutout.
struct QuadRows {
  int dx0, gy0, gy1;
  QuadCut cut;
};

// ---- stage the band's source rows into LDS: nrows rows of sw pixels, `step`
// bytes apart from address row0 on, nch chunks of s_src each
FFCV_DEV void stage_band(uint4 *s_src, uint64_t row0, uint64_t step, int sw, int nrows, int nch, int t) {
  // wave w copies rows w, w + 4, ...; lane l the row's 16-byte chunks l and
  // l + 64: the row address and its chunk count are wave-uniform (scalar),
  // a lane's chunk offset is fixed, and a wave has up to RRC_STAGE_ROWS
  // rows' loads in flight before its LDS writes
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;  // (wv scalar: row addresses in SGPRs)
  // (a lane that loads nothing keeps the registers' previous contents: its
  // LDS write is skipped too; zeroing them cost 8 moves per row)
  typedef uint32_t sx4_t __attribute__((ext_vector_type(4)));
  sx4_t v[RRC_STAGE_ROWS][2] = {};
  for (int cg = 0; cg < nch; cg += 128)  // (one pass for rows up to 2 KB: crops up to 677 px wide)
    for (int rb0 = wv; rb0 < nrows; rb0 += (RRC_THREADS / 64) * RRC_STAGE_ROWS) {
#pragma unroll
      for (int q = 0; q < RRC_STAGE_ROWS; q++) {
        const int r = rb0 + (RRC_THREADS / 64) * q;
        const uint64_t ra = row0 + (uint64_t)r * step;
        // chunks holding bytes of this row (none past the dataset's end)
        const int lim = r < nrows ? (int)(((ra & 15) + 3 * (uint64_t)sw + 15) >> 4) - cg : 0;
        // (a global-address-space pointer: global_load, not flat_load --
        // a flat load also counts in lgkmcnt, so every LDS wait would wait
        // for it too)
        typedef const __attribute__((address_space(1))) uint32_t gu32_t;
        gu32_t *rp = (gu32_t *)(uintptr_t)(ra & ~(uint64_t)15) + 4 * cg;
        if (ln < lim) v[q][0] = (sx4_t){rp[4 * ln], rp[4 * ln + 1], rp[4 * ln + 2], rp[4 * ln + 3]};
        if (ln + 64 < lim) v[q][1] = (sx4_t){rp[4 * ln + 256], rp[4 * ln + 257], rp[4 * ln + 258], rp[4 * ln + 259]};
      }
#pragma unroll
      for (int q = 0; q < RRC_STAGE_ROWS; q++) {
        const int r = rb0 + (RRC_THREADS / 64) * q;
        const uint64_t ra = row0 + (uint64_t)r * step;
        const int lim = r < nrows ? (int)(((ra & 15) + 3 * (uint64_t)sw + 15) >> 4) - cg : 0;
        if (ln < lim) s_src[r * nch + cg + ln] = __builtin_bit_cast(uint4, v[q][0]);
        if (ln + 64 < lim) s_src[r * nch + cg + ln + 64] = __builtin_bit_cast(uint4, v[q][1]);
      }
    }
}

// row dy of the quad, cutout applied: one 12-byte (u8) or three 8-byte (fp16) stores
template <bool FP16>
FFCV_DEV void put_quad(const Band<FP16> &B, const QuadRows &Q, int dy, int v[12]) {
  Q.cut.patch<0>(dy, v);
  store_quad<FP16>(B.o, (uint64_t)dy * B.ep.out_w + Q.dx0, v, B.S.lut);
}

// A column's three tap pixels lo, lo + 1, lo + 2 are 9 consecutive
// bytes: three ALIGNED 4-byte LDS reads cover them at any alignment
// and v_alignbyte shifts them into place (bytes at fixed positions,
// converted by v_cvt_f32_ubyte0-3).  Misaligned LDS reads (the 2- and
// 4-byte reads the compiler forms from adjacent byte reads) made this
// walk ~5x slower per pixel than the linear one.  A tap past hi has
// weight 0 and reads a byte of the staged rows or the LDS that
// follows them (finite: 0 * x == 0).
FFCV_DEV void area_hsum(const uint8_t *row, const int xo[4], const float wx[4][3], float B[12]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint8_t *q = row + xo[j];
    const uint32_t *qa = (const uint32_t *)__builtin_align_down(q, 4);
    const uint32_t sh = (uint32_t)(q - (const uint8_t *)qa);  // 0..3
    const uint32_t d0 = qa[0], d1 = qa[1], d2 = qa[2];
    uint32_t e[3];
    e[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
    e[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    e[2] = d2 >> (8 * sh);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float b = 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int i = 3 * k + c;
        b = b + (float)((e[i >> 2] >> (8 * (i & 3))) & 0xffu) * wx[j][k];
      }
      B[3 * j + c] = b;
    }
  }
}

// The area walk (ResizeArea_Invoker, column taps once per thread, row taps
// from LDS) for scales in [1, 2): a destination index takes at most 3
// consecutive source indices, so a fixed 3-tap horizontal body with zero
// weights past `hi` is exact (x + S * 0.f == x for the non-negative sums
// here).  buf of a source row (the horizontal sums)
// does not depend on the destination row: each destination row dy
// sums its source rows lo..hi in ascending order (sum = w(lo) * B(lo),
// then sum += w(r) * B(r): the reference's order), and consecutive
// rows share at most their boundary source row, so one cached row of
// sums (Hc, source row cr) covers the reuse (any other reuse
// recomputes, exactly).  The rows are wave-uniform (a row group is
// whole waves): the loop bounds and the cache test are scalar.
template <bool FP16>
FFCV_DEV void area_walk(const Band<FP16> &B, const QuadRows &Q) {
  const ResizePlan &P = B.P;
  int xo[4];  // the first tap pixel's byte offset in a row
  float wx[4][3];
  if (B.itaps) {  // rrc_taps_kernel's column records (flip applied): one 16-byte load per column
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint4 e = *(const uint4 *)(B.itaps + 2 * (Q.dx0 + j));
      xo[j] = 3 * (int)e.x;
      wx[j][0] = ffcv_u2f_bits(e.y);
      wx[j][1] = ffcv_u2f_bits(e.z);
      wx[j][2] = ffcv_u2f_bits(e.w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const AreaTaps tx = area_taps(P.sw, P.scale_x, B.ep.src_x(Q.dx0 + j));
      xo[j] = 3 * tx.lo;
#pragma unroll
      for (int k = 0; k < 3; k++) wx[j][k] = tx.lo + k <= tx.hi ? tx.w(tx.lo + k) : 0.f;
    }
  }
  RRC_STOP_AT(4, B.ep.cut_before_flip != 77);  // diagnostics: + the area walk's column taps
  int cr = -1;
  float Hc[12];
#pragma unroll
  for (int i = 0; i < 12; i++) Hc[i] = 0.f;
  for (int dy = Q.gy0; dy < Q.gy1; dy++) {
    const AreaTaps ty = B.S.at[dy - B.oy0];
    float S[12];
    for (int r = ty.lo; r <= ty.hi; r++) {
      float H[12];
      if (r == cr) {
#pragma unroll
        for (int i = 0; i < 12; i++) H[i] = Hc[i];
      } else {
        area_hsum(B.L.row(r), xo, wx, H);
      }
      const float w = ty.w(r);
      if (r == ty.lo) {
#pragma unroll
        for (int i = 0; i < 12; i++) S[i] = w * H[i];
      } else {
#pragma unroll
        for (int i = 0; i < 12; i++) S[i] = S[i] + w * H[i];
      }
      if (r == ty.hi) {
#pragma unroll
        for (int i = 0; i < 12; i++) Hc[i] = H[i];
        cr = r;
      }
    }
    // cvRound + saturate_cast<uchar>: the sums lie in [0, 255.5) (bytes
    // times weights that sum to 1 up to a few float roundings), so
    // S + 1.5 * 2^23 rounds S half-to-even into the float's low byte and
    // the saturation never acts: one (packed) add per value instead of
    // v_rndne + v_cvt + v_med3, and the u8 bytes packed by v_perm (the
    // v_rndne form was a build switch until commit 356ba29)
    uint32_t bz[12];
#pragma unroll
    for (int i = 0; i < 12; i++) bz[i] = ffcv_f2u_bits(S[i] + 12582912.0f);
    Q.cut.patch<0>(dy, bz);
    const uint64_t px = (uint64_t)dy * B.ep.out_w + Q.dx0;
    if (FP16) {
      int v[12];
#pragma unroll
      for (int i = 0; i < 12; i++) v[i] = (int)(bz[i] & 0xffu);
      store_quad<true>(B.o, px, v, B.S.lut);
    } else {
      typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
      uint32_t wd[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {  // low bytes of four values: [a, b, 0, 0], [c, d, 0, 0] -> [a, b, c, d]
        const uint32_t lo = __builtin_amdgcn_perm(bz[4 * d + 1], bz[4 * d], 0x0c0c0400u);
        const uint32_t hi = __builtin_amdgcn_perm(bz[4 * d + 3], bz[4 * d + 2], 0x0c0c0400u);
        wd[d] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
      }
      u32x3 w;
      w.x = wd[0];
      w.y = wd[1];
      w.z = wd[2];
      __builtin_nontemporal_store(w, (u32x3 *)((uint8_t *)B.o + px * 3));
    }
  }
}

// The general-area quad loop (scales of 2 and more): each pixel by resize_area_lds
template <bool FP16>
FFCV_DEV void area_quads(const Band<FP16> &B, const QuadRows &Q) {
  AreaTaps tx[4];
#pragma unroll
  for (int j = 0; j < 4; j++) tx[j] = area_taps(B.P.sw, B.P.scale_x, B.ep.src_x(Q.dx0 + j));
  for (int dy = Q.gy0; dy < Q.gy1; dy++) {
    const AreaTaps ty = B.S.at[dy - B.oy0];
    int v[12];
#pragma unroll
    for (int j = 0; j < 4; j++) resize_area_lds(B.L, tx[j], ty, v + 3 * j);  // (s_src is followed by s_rt: in LDS)
    put_quad(B, Q, dy, v);
  }
}

FFCV_DEV uint32_t mulhi24(uint32_t a, uint32_t b) {  // a, b < 2^24: v_mul_hi_u32_u24
  return (uint32_t)(((uint64_t)(a & 0xffffffu) * (b & 0xffffffu)) >> 32);
}

// row dy of the linear walk's quad from its two source rows' sums A (upper,
// weight c0) and Bl (lower, weight c1)
template <bool FP16>
FFCV_DEV void linear_emit(const Band<FP16> &B, const QuadRows &Q, int dy, const uint32_t (&A)[12],
                          const uint32_t (&Bl)[12], uint32_t c0, uint32_t c1) {
  if (FP16) {
    int v[12];
#pragma unroll
    for (int i = 0; i < 12; i++)  // VResizeLinearVec_32s8u: (m0 + 2 + m1) >> 2, no saturation (see linear_walk)
      v[i] = (int)((mulhi24(A[i], c0) + mulhi24(Bl[i], c1) + 2u) >> 2);
    put_quad(B, Q, dy, v);
  } else {
    // u8: t = m0 + m1 + 2 (<= 1022) per value, two values per dword in
    // 16-bit lanes, one packed shift (v_pk_lshrrev_b16) per pair and the
    // low bytes picked by one v_perm per output dword: 5 instructions per
    // dword instead of 8 (a cutout value is fill << 2: exact after >> 2)
    uint32_t tv[12];
#pragma unroll
    for (int i = 0; i < 12; i++) tv[i] = mulhi24(A[i], c0) + mulhi24(Bl[i], c1) + 2u;
    Q.cut.patch<2>(dy, tv);
    auto shr2 = [](uint32_t x) -> uint32_t {  // both 16-bit halves >> 2
      return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, x) >> (u16x2_t){2, 2});
    };
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    uint32_t wd[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const uint32_t lo = shr2(tv[4 * d] | (tv[4 * d + 1] << 16)), hi = shr2(tv[4 * d + 2] | (tv[4 * d + 3] << 16));
      wd[d] = __builtin_amdgcn_perm(hi, lo, 0x06040200u);  // bytes lo.0, lo.2, hi.0, hi.2
    }
    u32x3 w;
    w.x = wd[0];
    w.y = wd[1];
    w.z = wd[2];
    // uniform row address (scalar) + this lane's 32-bit offset: the
    // store's saddr form, no 64-bit address arithmetic per row
    typedef __attribute__((address_space(1))) uint8_t gbyte_t;
    typedef __attribute__((address_space(1))) u32x3 gu32x3_t;
    const uint64_t ra64 = (uint64_t)(uintptr_t)B.o + (uint64_t)(uint32_t)dy * (uint32_t)(3 * B.ep.out_w);
    gbyte_t *orow = (gbyte_t *)(uintptr_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(ra64 >> 32)) << 32) |
                                           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ra64));
    __builtin_nontemporal_store(w, (gu32x3_t *)(orow + (uint32_t)(3 * Q.dx0)));
  }
}

// The linear walk.  tq0 / tq1: the quad's four column taps of the image's
// table (flip applied), loaded by the caller before the staging.
template <bool FP16>
FFCV_DEV void linear_walk(const Band<FP16> &B, const QuadRows &Q, const uint4 &tq0, const uint4 &tq1) {
  const ResizePlan &P = B.P;
  const uint2 *itaps = B.itaps;
  const int out_w = B.ep.out_w;
  int xa[4], xb[4], wa[4], wb[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint4 &tq = j < 2 ? tq0 : tq1;
    const LinTap l = itaps ? tap_unpack((j & 1) ? make_uint2(tq.z, tq.w) : make_uint2(tq.x, tq.y))
                           : lin_tap(P.scale_x, P.inv_x, P.sw, B.ep.src_x(Q.dx0 + j));
    // a border tap (src[s] * 2048) as the two-tap form with weights (2048, 0)
    xa[j] = 3 * l.s;
    xb[j] = 3 * (l.border ? l.s : l.s + 1);
    wa[j] = l.border ? 2048 : l.c0;
    wb[j] = l.border ? 0 : l.c1;
  }
  // resize.cpp HResizeLinear of crop row r: sat_s16(h >> 4).  The
  // saturations of this walk never act (so they are not computed): weights
  // are in [0, 2048] with wa + wb <= 2049 (linear_coef rounds each), so
  // 0 <= h >> 4 <= 255 * 2049 >> 4 = 32655 and the vertical sum
  // m0 + m1 <= 32655 * 2049 >> 16 = 1020, (1020 + 2) >> 2 = 255.
  // The row keeps (h >> 4) << 8 (< 2^23), so VResizeLinearVec's
  // (h * c) >> 16 is one 24-bit high multiply by c << 8 (< 2^20):
  // mulhi_u24(h << 8, c << 8) = (h * c * 2^16) >> 32.
  auto hrow = [&](int r, uint32_t H[12]) {
    const uint8_t *row = B.L.row(r);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        H[3 * j + c] = (((uint32_t)(row[xa[j] + c] * wa[j] + row[xb[j] + c] * wb[j]) >> 4) & 0x7fffu) << 8;
  };
  RRC_STOP_AT(3, B.ep.cut_before_flip != 77);  // diagnostics: + the linear walk's column taps
  // row taps: from the image's table through the scalar cache (the rows of a
  // row group are wave-uniform) when there is one, else the band's LDS records
  const __attribute__((address_space(4))) uint32_t *rtp =
      itaps ? (const __attribute__((address_space(4))) uint32_t *)(itaps + out_w) : nullptr;
  auto row_taps = [&](int dy, int &ra, int &rb, uint32_t &c0, uint32_t &c1) {
    if (rtp) {
      const uint32_t tx = rtp[2 * dy], ty = rtp[2 * dy + 1];
      const int sr = (int)(tx & 0x7fffffffu);
      ra = min(max(sr, 0), P.sh - 1);
      rb = min(max(sr + 1, 0), P.sh - 1);
      c0 = (ty & 0xfffu) << 8;
      c1 = ((ty >> 16) & 0xfffu) << 8;
    } else {
      const uint4 ly = B.S.rt[dy - B.oy0];
      ra = (int)ly.x;
      rb = (int)ly.y;
      c0 = ly.z;
      c1 = ly.w;
    }
  };
  // the two source rows' horizontal sums live in register sets X and Y;
  // which one is the upper row (A) flips when the walk moves down one
  // source row, instead of copying B into A (12 moves per such row): the
  // flag is wave-uniform, so both orders are separate straight-line code
  uint32_t HX[12], HY[12];
  int cx = -1, cy = -1;  // source rows held by X / Y
  // two loops, one per role assignment (a single loop with a role flag was
  // compiled into one shared epilogue fed by 24 register moves per row)
  int dy = Q.gy0;
  while (dy < Q.gy1) {
    for (; dy < Q.gy1; dy++) {  // A = X, B = Y
      int ra, rb;
      uint32_t c0, c1;
      row_taps(dy, ra, rb, c0, c1);
      if (ra != cx && ra == cy) break;  // down one source row: continue with A = Y
      if (ra != cx) {
        hrow(ra, HX);
        cx = ra;
      }
      if (rb != cy) {
        hrow(rb, HY);
        cy = rb;
      }
      linear_emit(B, Q, dy, HX, HY, c0, c1);
    }
    for (; dy < Q.gy1; dy++) {  // A = Y, B = X
      int ra, rb;
      uint32_t c0, c1;
      row_taps(dy, ra, rb, c0, c1);
      if (ra != cy && ra == cx) break;  // down one source row: continue with A = X
      if (ra != cy) {
        hrow(ra, HY);
        cy = ra;
      }
      if (rb != cx) {
        hrow(rb, HX);
        cx = rb;
      }
      linear_emit(B, Q, dy, HY, HX, c0, c1);
    }
  }
}

// The per-pixel restatement of the band, over the staged rows when they fit
template <bool FP16>
FFCV_DEV void pixel_tail(const Band<FP16> &B, const GlobalSrc &src, bool staged, int t) {
  const int out_w = B.ep.out_w;
  const int npx = (B.oy1 - B.oy0) * out_w;
  for (int i = t; i < npx; i += RRC_THREADS) {
    const int dy = B.oy0 + i / out_w, dx = i % out_w;
    int v[3];
    if (B.ep.in_cut(dy, dx)) {
      v[0] = B.ep.fill[0];
      v[1] = B.ep.fill[1];
      v[2] = B.ep.fill[2];
    } else if (staged) {
      resize_pixel(B.P, B.L, dy, B.ep.src_x(dx), v);
    } else {
      resize_pixel(B.P, src, dy, B.ep.src_x(dx), v);
    }
    store_px<FP16>(B.o, (uint64_t)dy * out_w + dx, v, B.S.lut);
  }
}

// One band of RRC_BAND output rows of image k.  Every barrier is reached by
// all threads; thread-level returns follow the last one.
template <bool FP16>
FFCV_DEV void rrc_band(const uint8_t *__restrict__ base, const ffcv_sample *__restrict__ samples,
                       const int32_t *__restrict__ crops, const int32_t *__restrict__ cut,
                       const uint8_t *__restrict__ flips, const ffcv_rrc_params &p, uint64_t stride,
                       void *__restrict__ out, const int k, const int band, RrcLds<FP16> &S,
                       const ResizePlan *__restrict__ plans, const uint2 *__restrict__ taps) {
  const int t = threadIdx.x;
  const ffcv_sample s = samples[k];
  if (FP16) {
    for (int i = t; i < 768; i += RRC_THREADS) S.lut[i] = p.lut[i];
  }
  if (s.mode != 1) return;
  const int oy0 = band * RRC_BAND, oy1 = min(p.out_h, oy0 + RRC_BAND);
  if (oy0 >= p.out_h) return;
  const int ci = crops[4 * k], cj = crops[4 * k + 1], chh = crops[4 * k + 2], cww = crops[4 * k + 3];
  GlobalSrc src{base + s.offset + ((uint64_t)ci * s.width + cj) * 3, (uint64_t)s.width * 3};
  // the image's plan and linear taps from rrc_taps_kernel when the caller gave
  // a workspace (computed once per image, not in each of its band workgroups:
  // the f64 plan and four column taps per thread were a third of this
  // kernel's instructions, profiles/r5c_c5parts.txt)
  const uint2 *itaps = taps ? taps + (uint64_t)k * RAW_TAPS(p) : nullptr;
  const ResizePlan P = plans ? plans[k] : make_plan(cww, chh, p.out_w, p.out_h);
  const Epilogue ep = make_epilogue(p, cut, flips, k);
  const int out_w = p.out_w;
  // The linear walk's column taps (flip applied, 32 bytes per thread quad),
  // loaded before the band's staging so their latency hides under it (after
  // it, every workgroup waited ~1 us for them: 28 ns per image)
  uint4 tq0 = make_uint4(0, 0, 0, 0), tq1 = tq0;
  {
    int tpg = 64;
    while (tpg < (out_w >> 2)) tpg <<= 1;
    const int qq = t & (tpg - 1);
    // (rrc_taps_kernel writes these entries for linear plans only: an area
    // crop's table holds the area walk's column records, read there)
    if (itaps && P.kind == 3 && qq < (out_w >> 2)) {
      tq0 = *(const uint4 *)(itaps + 4 * qq);
      tq1 = *(const uint4 *)(itaps + 4 * qq + 2);
    }
  }

  RRC_STOP_AT(1, p.cutout_fill[3] != 77);  // diagnostics: the band's set-up only
  int r0, r1;
  band_rows(P, oy0, oy1, &r0, &r1);
  const uint64_t row0 = (uint64_t)(uintptr_t)src.p + (uint64_t)r0 * src.step;
  const int nrows = r1 - r0 + 1;
  const int nch = (15 + P.sw * 3 + 15) >> 4;  // 16-byte chunks per LDS row (any alignment)
  const bool staged = nrows * nch * 16 <= RRC_LDS_BYTES;
  const LdsSrc L{(const uint8_t *)S.src, nch * 16, (int)(row0 & 15), (int)(src.step & 15), r0};
  const Band<FP16> B{P, ep, L, S, itaps, (char *)out + stride * k, oy0, oy1};
  if (staged) stage_band(S.src, row0, src.step, P.sw, nrows, nch, t);
  if (P.kind == 3 && !itaps && t < oy1 - oy0) {  // clamped source rows, weights << 8: no per-row clamps in the walk
    const LinTap l = lin_tap(P.scale_y, P.inv_y, P.sh, oy0 + t);
    S.rt[t] = make_uint4((uint32_t)min(max(l.s, 0), P.sh - 1), (uint32_t)min(max(l.s + 1, 0), P.sh - 1),
                         ((uint32_t)l.c0 & 0xfffu) << 8, ((uint32_t)l.c1 & 0xfffu) << 8);
  }
  if (P.kind == 2 && t < oy1 - oy0) S.at[t] = area_taps(P.sh, P.scale_y, oy0 + t);
  __syncthreads();
  RRC_STOP_AT(2, p.cutout_fill[3] != 77);  // diagnostics: set-up + staging

  const bool aligned4 = ((((uintptr_t)out) | stride) & 3) == 0;
  const int nq = out_w >> 2;  // column quads
  if (staged && (out_w & 3) == 0 && nq <= RRC_THREADS && aligned4 &&
      ((P.kind == 3 && P.vec_end == 3 * out_w) || P.kind == 2)) {
    // row groups: tpg threads (a power of two >= nq, >= 64) per group, each
    // group walks its own slice of the band's rows
    int tpg = 64;
    while (tpg < nq) tpg <<= 1;
    const int groups = RRC_THREADS / tpg;
    const int per = (oy1 - oy0 + groups - 1) / groups;
    const int g = t / tpg, q = t - g * tpg;
    // (a row group is whole waves, tpg >= 64: its rows are wave-uniform, so
    // the per-row cutout range test is scalar)
    const int gy0 = __builtin_amdgcn_readfirstlane(oy0 + g * per);
    const int gy1 = __builtin_amdgcn_readfirstlane(min(oy1, gy0 + per));
    if (q >= nq || gy0 >= gy1) return;
    const QuadRows Q{4 * q, gy0, gy1, QuadCut(ep, 4 * q)};
    // (each walk returns here: an RRC_STOP build's hook inside it ends the band)
    if (P.kind == 2) {
      if (area_walk_plan(P)) return area_walk(B, Q);
      return area_quads(B, Q);
    }
    return linear_walk(B, Q, tq0, tq1);
  }
  pixel_tail(B, src, staged, t);
}

template <bool FP16>
__global__ void __launch_bounds__(RRC_THREADS) __attribute__((amdgpu_waves_per_eu(RRC_WPE)))
    rrc_raw_kernel(const uint8_t *__restrict__ base, const ffcv_sample *__restrict__ samples,
                   const int32_t *__restrict__ crops, const int32_t *__restrict__ cut,
                   const uint8_t *__restrict__ flips, ffcv_rrc_params p, uint64_t stride,
                   void *__restrict__ out, const ResizePlan *__restrict__ plans, const uint2 *__restrict__ taps) {
  __shared__ RrcLds<FP16> S;
  rrc_band<FP16>(base, samples, crops, cut, flips, p, stride, out, (int)blockIdx.y, (int)blockIdx.x, S, plans,
                 taps);
}

// Per-image resize plan + linear tap table for rrc_raw_kernel (one thread per
// tap: columns [0, out_w) with the image's flip applied, then rows [out_w,
// out_w + out_h)), the same functions the band workgroups would evaluate
// (resize.cpp linear coefficients, make_plan), so the output is unchanged.
__global__ void __launch_bounds__(256) rrc_taps_kernel(const int32_t *__restrict__ crops,
                                                       const uint8_t *__restrict__ flips, ffcv_rrc_params p,
                                                       ResizePlan *__restrict__ plans, uint2 *__restrict__ taps) {
  const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const ResizePlan P = make_plan(crops[4 * k + 3], crops[4 * k + 2], p.out_w, p.out_h);
  if (i == 0) plans[k] = P;
  if (area_walk_plan(P)) {  // column records of the area walk: {lo, w(lo), w(lo + 1), w(lo + 2)}, 0 past hi
    if (i >= p.out_w) return;
    const int flip = flips ? flips[k] : 0;
    const AreaTaps a = area_taps(P.sw, P.scale_x, flip ? p.out_w - 1 - i : i);
    uint32_t w[3];
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = ffcv_f2u_bits(a.lo + j <= a.hi ? a.w(a.lo + j) : 0.f);
    *(uint4 *)(taps + (uint64_t)k * RAW_TAPS(p) + 2 * i) = make_uint4((uint32_t)a.lo, w[0], w[1], w[2]);
    return;
  }
  if (P.kind != 3 || i >= p.out_w + p.out_h) return;
  LinTap l;
  if (i < p.out_w) {
    const int flip = flips ? flips[k] : 0;
    l = lin_tap(P.scale_x, P.inv_x, P.sw, flip ? p.out_w - 1 - i : i);
  } else {
    l = lin_tap(P.scale_y, P.inv_y, P.sh, i - p.out_w);
  }
  taps[(uint64_t)k * RAW_TAPS(p) + i] = tap_pack(l);
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_draw_batch(void *stream, const uint64_t *sample_ids, const ffcv_sample *samples, int batch,
                    const ffcv_draw_params *p, int32_t *crops, int32_t *cutout_yx, uint8_t *flips,
                    int32_t *status) {
  if (batch < 0 || !p || !sample_ids || (crops && !samples)) {
    ffcv::set_error("ffcv_draw_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  if (p->cutout_size > 0 && (p->cutout_size > p->out_h || p->cutout_size > p->out_w)) {
    ffcv::set_error("ffcv_draw_batch: cutout_size %d exceeds output %dx%d", p->cutout_size, p->out_h,
                    p->out_w);
    return FFCV_EINVAL;
  }
  return ffcv::launch_draw("draw_kernel", draw_kernel, stream, batch, sample_ids, samples, batch, *p, crops,
                           cutout_yx, flips, status);
}

static uint64_t raw_plans_bytes(int batch) { return ((uint64_t)batch * sizeof(ResizePlan) + 255) & ~(uint64_t)255; }

uint64_t ffcv_rrc_raw_workspace_bytes(int batch, int out_h, int out_w) {
  if (batch <= 0 || out_h <= 0 || out_w <= 0) return 0;
  ffcv_rrc_params q{};
  q.out_h = out_h;
  q.out_w = out_w;
  return raw_plans_bytes(batch) + (uint64_t)batch * RAW_TAPS(q) * sizeof(uint2);
}

int ffcv_rrc_raw_batch_ws(void *stream, const uint8_t *base, const ffcv_sample *samples, int batch,
                          const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                          const ffcv_rrc_params *p, void *out, void *workspace, uint64_t workspace_bytes) {
  if (batch < 0 || !p || !base || !samples || !crops || !out || p->out_h <= 0 || p->out_w <= 0) {
    ffcv::set_error("ffcv_rrc_raw_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  const ResizePlan *plans = nullptr;
  const uint2 *taps = nullptr;
  if (workspace) {
    const uint64_t need = ffcv_rrc_raw_workspace_bytes(batch, p->out_h, p->out_w);
    if (workspace_bytes < need || ((uintptr_t)workspace & 15)) {
      ffcv::set_error("ffcv_rrc_raw_batch_ws: workspace of %llu bytes (16-byte aligned) needed, got %llu",
                      (unsigned long long)need, (unsigned long long)workspace_bytes);
      return FFCV_EINVAL;
    }
    ResizePlan *wp = (ResizePlan *)workspace;
    uint2 *wt = (uint2 *)((uint8_t *)workspace + raw_plans_bytes(batch));
    hipLaunchKernelGGL(rrc_taps_kernel, dim3((p->out_w + p->out_h + 255) / 256, batch), dim3(256), 0,
                       ffcv::as_stream(stream), crops, flips, *p, wp, wt);
    FFCV_LAUNCH_CHECK("rrc_taps_kernel");
    plans = wp;
    taps = wt;
  }
  const bool fp16 = p->lut != nullptr;
  uint64_t dense = (uint64_t)p->out_h * p->out_w * 3 * (fp16 ? 2 : 1);
  uint64_t stride = p->out_stride ? p->out_stride : dense;
  dim3 grid((p->out_h + RRC_BAND - 1) / RRC_BAND, batch);
  if (fp16)
    hipLaunchKernelGGL(rrc_raw_kernel<true>, grid, dim3(RRC_THREADS), 0, ffcv::as_stream(stream), base,
                       samples, crops, cutout_yx, flips, *p, stride, out, plans, taps);
  else
    hipLaunchKernelGGL(rrc_raw_kernel<false>, grid, dim3(RRC_THREADS), 0, ffcv::as_stream(stream), base,
                       samples, crops, cutout_yx, flips, *p, stride, out, plans, taps);
  FFCV_LAUNCH_CHECK("rrc_raw_kernel");
  return FFCV_OK;
}

int ffcv_rrc_raw_batch(void *stream, const uint8_t *base, const ffcv_sample *samples, int batch,
                       const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                       const ffcv_rrc_params *p, void *out) {
  return ffcv_rrc_raw_batch_ws(stream, base, samples, batch, crops, cutout_yx, flips, p, out, nullptr, 0);
}

}  // extern "C"
