// ffcv_affine.hip -- RandomAffine / RandomRotation on a dense uint8 batch
// [B][H][W][3] (one launch behind its draw launch), the draws (op id 14), and
// the host twins.
//
// One kernel serves every regime.  A 256-thread workgroup owns a tile of
// output rows [y0, y1) x columns [x0, x1) of one image, and decides, the same
// for all its threads, how the tile's taps are read:
//
//   fill:   the coefficients lie outside the bounds, or the tile's source
//           footprint (affine_box) misses the image: nothing is read.
//   LDS:    the footprint's rows are staged as uint8 in LDS, a tile of rows
//           (lds_stage.h): one byte range per row, one for all when they span
//           the image's width.  Taps are lds_pixel reads; the two horizontal
//           taps of a bilinear sample are six contiguous bytes, three dwords.
//           Coordinates are 32-bit, relative to the footprint's corner, which
//           affine_box has shown exact.
//   direct: the footprint exceeds the tile's LDS budget (strong minification,
//           a sheared tile of a wide image) or its relative coordinates leave
//           32 bits: taps come from global memory, coordinates are 64-bit.
//
// Every thread computes four adjacent pixels at a time, twelve bytes, into an
// LDS copy of the tile's output, dense, walking the coordinates by one add
// per pixel; those bytes leave by the row tile's write-back at any alignment
// of dst.  An image whose apply flag is 0 is the identity under nearest: its
// footprint is the tile itself, and the staged bytes leave as they came: a
// copy.
//
//   whole image: 3 H W <= AFFINE_WHOLE_BYTES -- one tile per image, the image
//     staged once as one byte range.
//   tiles: AFFINE_TILE_ROWS x AFFINE_TILE_COLS outputs; the staged footprint
//     takes at most AFFINE_TILE_LDS bytes.
//
// The entries' argument check, the launch and the host twin's claim loop are
// those of every out-of-place operator (api_internal.h: out_of_place_ok,
// launch_tiles, host_images).
#include <cmath>
#include <cstring>

#include "affine_common.h"
#include "api_internal.h"

#define AFFINE_THREADS 256
#ifndef AFFINE_WHOLE_BYTES
#define AFFINE_WHOLE_BYTES 16384  // whole-image regime: 3 H W at most this
#endif
#ifndef AFFINE_TILE_ROWS
#define AFFINE_TILE_ROWS 32
#endif
#ifndef AFFINE_TILE_COLS
#define AFFINE_TILE_COLS 32
#endif
#ifndef AFFINE_TILE_LDS
#define AFFINE_TILE_LDS 16384  // staged footprint of a tile, at most
#endif

struct AffineRanges {
  double v[12];
};

__global__ void __launch_bounds__(64) affine_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed,
                                                         uint64_t epoch, double p, AffineRanges rg, int H, int W,
                                                         uint8_t *__restrict__ apply, int64_t *__restrict__ coef,
                                                         int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_affine(k, ids[k], loader_seed, epoch, p, rg.v, H, W, apply, coef);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// How a launch cuts an image into tiles, and the LDS a workgroup takes:
// 16 bytes | staged source | 16 bytes | output bytes | 32 bytes
struct AffinePlan {
  int th, tw, nty, ntx, whole;
  uint32_t budget;   // staged bytes a tile may take
  uint32_t out_off;  // byte offset of the output region, a multiple of 16
  uint32_t lds;
};

static AffinePlan affine_plan(int H, int W) {
  AffinePlan P;
  P.whole = (uint64_t)H * W * 3u <= AFFINE_WHOLE_BYTES;
  P.th = P.whole ? H : std::min(H, AFFINE_TILE_ROWS);
  P.tw = P.whole ? W : std::min(W, AFFINE_TILE_COLS);
  P.nty = (H + P.th - 1) / P.th;
  P.ntx = (W + P.tw - 1) / P.tw;
  P.budget = P.whole ? lds_chunks(3u * H * W) * 16u : AFFINE_TILE_LDS;
  P.out_off = 16u + P.budget + 16u;
  P.lds = P.out_off + ((3u * P.th * P.tw + 15u) & ~15u) + 32u;
  return P;
}

// Taps from the staged footprint (a tile of rows, lds_stage.h); coordinates
// relative to its corner.
struct AffineLdsTap : LdsRows<true> {
  int nrows, cw;
  uint32_t fill;
  // v where ok, else fill, as masks: a select whose operands are both computed
  // keeps the LDS reads out of branches, so the reads of a thread's four
  // pixels can be in flight together
  FFCV_DEV uint32_t pick(bool ok, uint32_t v) const {
    const uint32_t m = 0u - (uint32_t)ok;
    return (v & 0xffffffu & m) | (fill & ~m);
  }
  FFCV_DEV uint32_t one(int iy, int ix) const {
    const bool ok = (uint32_t)iy < (uint32_t)nrows && (uint32_t)ix < (uint32_t)cw;
    return pick(ok, lds_pixel(row(ok ? iy : 0) + 3 * (ok ? ix : 0)));
  }
  // (iy, ix) and (iy, ix + 1): six contiguous bytes from three aligned dwords.
  // The column is clamped to [-1, cw - 1] for the address only (16 bytes lie in
  // front of the first row and 16 behind the last), each tap is tested on its own.
  FFCV_DEV void pair(int iy, int ix, uint32_t *t0, uint32_t *t1) const {
    const bool rok = (uint32_t)iy < (uint32_t)nrows;
    const int xc = max(-1, min(ix, cw - 1));
    const uint8_t *a = row(rok ? iy : 0) + 3 * xc;
    const uint32_t *qa = (const uint32_t *)__builtin_align_down(a, 4);
    const uint32_t sh = (uint32_t)(a - (const uint8_t *)qa);
    const uint32_t q0 = qa[0], q1 = qa[1], q2 = qa[2];
    const uint32_t lo = __builtin_amdgcn_alignbyte(q1, q0, sh), hi = __builtin_amdgcn_alignbyte(q2, q1, sh);
    *t0 = pick(rok & ((uint32_t)ix < (uint32_t)cw), lo);
    *t1 = pick(rok & ((uint32_t)(ix + 1) < (uint32_t)cw), (lo >> 24) | (hi << 8));
  }
};

// Coordinates walk with the pixels: one multiply-add per group start, then a
// step per pixel (`wrap`: the step from a row's last pixel to the next row's
// first).  C is uint32_t, wrapping, where the caller has shown the true values
// to fit 32 bits, else int64_t.
template <class C>
struct AffineWalk {
  C X, Y, x0, y0, dxc, dyc, dxr, dyr, dxw, dyw;
  FFCV_DEV void init(C X0, C Y0, C q0, C q1, C q3, C q4, int tc) {
    x0 = X0, y0 = Y0, dxc = q0, dyc = q3, dxr = q1, dyr = q4;
    dxw = q1 - q0 * (C)(tc - 1);
    dyw = q4 - q3 * (C)(tc - 1);
  }
  FFCV_DEV void start(int r, int c) {
    X = x0 + dxc * (C)c + dxr * (C)r;
    Y = y0 + dyc * (C)c + dyr * (C)r;
  }
  FFCV_DEV void step(bool wrap) {
    X += wrap ? dxw : dxc;
    Y += wrap ? dyw : dyc;
  }
};

// f / tc for 0 <= f < 2^22, 0 < tc < 2^15 with inv = 1.0f / tc: the float
// quotient is off by less than one, so one correction either way settles it
FFCV_DEV int affine_div(int f, int tc, float inv) {
  int r = (int)((float)f * inv);
  r -= (int)(__mul24(r, tc) > f);
  r += (int)(__mul24(r + 1, tc) <= f);
  return r;
}

// The tile's pixels, four adjacent ones (in row-major order of the tile) per
// thread and step, as three aligned dwords into the dense output bytes.
// pix(r, c, first): the pixel at tile row r, column c; `first` where it opens
// a thread's group, else it follows the previous call's pixel in that order.
// The last group may run up to three pixels past the tile: they are computed
// like any other (every tap is bounds-checked, coordinates past the tile only
// miss), land in the bytes behind the tile's and are never stored; so the four
// pixels are straight-line code.
template <class F>
FFCV_DEV void affine_groups(int t, int npix, int tc, uint32_t *s_out, F pix) {
  const float inv = 1.0f / (float)tc;
  for (int g = t; 4 * g < npix; g += AFFINE_THREADS) {
    int r = affine_div(4 * g, tc, inv), c = 4 * g - __mul24(r, tc);
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      v[e] = pix(r, c, e == 0);
      c++;
      if (c == tc) {
        c = 0;
        r++;
      }
    }
    s_out[3 * g + 0] = v[0] | (v[1] << 24);
    s_out[3 * g + 1] = (v[1] >> 8) | (v[2] << 16);
    s_out[3 * g + 2] = (v[2] >> 16) | (v[3] << 8);
  }
}

__global__ void __launch_bounds__(AFFINE_THREADS)
    affine_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_stride, int H, int W,
                       int mode, uint32_t fill, const uint8_t *__restrict__ apply, const int64_t *__restrict__ coef,
                       AffinePlan P) {
  extern __shared__ uint4 affine_smem[];
  lds_x4_t *s_u8 = (lds_x4_t *)affine_smem + 1;  // staged chunks, behind 16 bytes a tap at column -1 may read
  uint32_t *s_out = (uint32_t *)((uint8_t *)affine_smem + P.out_off);
  const int t = threadIdx.x;
  const uint32_t per = (uint32_t)P.nty * P.ntx;
  const uint32_t k = blockIdx.x / per, rem = blockIdx.x - k * per;
  const int ty = rem / P.ntx, tx = rem - ty * P.ntx;
  const int y0 = ty * P.th, y1 = min(H, y0 + P.th), x0 = tx * P.tw, x1 = min(W, x0 + P.tw);
  const int rows = y1 - y0, tc = x1 - x0;

  // the image's decision and coefficients (the same for the whole workgroup;
  // both loads leave together); an image that is not applied is the identity
  // under nearest: its footprint is the tile itself, and the staged bytes leave
  // as they came
  // (a byte load lands in a vector register: readfirstlane tells the compiler
  // that the flag, and with it the footprint's 64-bit arithmetic, is scalar)
  const bool on = __builtin_amdgcn_readfirstlane((int)apply[k]) != 0;
  int64_t q[6];
#pragma unroll
  for (int i = 0; i < 6; i++) q[i] = coef[(uint64_t)k * 6 + i];
  if (!on) {
#pragma unroll
    for (int i = 0; i < 6; i++) q[i] = i == 0 || i == 4 ? 65536 : 0;
  }
  const int md = on ? mode : FFCV_AFFINE_NEAREST;
  const bool ok = affine_coef_ok(q);
  if (!ok) {  // keep the footprint's arithmetic inside 64 bits
#pragma unroll
    for (int i = 0; i < 6; i++) q[i] = 0;
  }
  const AffineBox box = affine_box(q, md, H, W, x0, y0, x1, y1, P.whole != 0);
  const int regime = !ok || box.empty() ? 0 : (!box.fits32 || box.staged_bytes(W) > P.budget ? 2 : 1);

  const uint64_t step = (uint64_t)W * 3u;
  const uint8_t *img = src + (uint64_t)k * H * step;
  const int npix = rows * tc;
  // where the write-back finds range y: the tile's dense output bytes
  LdsRows<> wb = {(const uint8_t *)s_out, 3 * tc, 0, 0};
  if (regime == 1) {
    // ---- stage source rows [lo, hi) x columns [cl, ch) as a tile of rows (lds_stage.h)
    const int nrows = box.hi - box.lo, cw = box.ch - box.cl;
    const uint64_t src0 = (uint64_t)(uintptr_t)img + ((uint64_t)box.lo * W + box.cl) * 3u;
    const bool span = cw == W;
    const int n_srows = span ? 1 : nrows;
    const uint32_t srow_bytes = span ? (uint32_t)nrows * 3u * W : 3u * cw;
    const int nchr = (int)lds_chunks(srow_bytes);
    stage_rows<AFFINE_THREADS>(t, src0, step, n_srows, srow_bytes, nchr, s_u8);
    __syncthreads();
    const AffineLdsTap tap{lds_rows<true>(s_u8, src0, step, span, nchr), nrows, cw, fill};
    if (on) {
      // 32-bit coordinates relative to the footprint's corner: the true values
      // fit (box.fits32), so wrapping arithmetic gives them exactly
      AffineWalk<uint32_t> w;
      w.init((uint32_t)box.X0, (uint32_t)box.Y0, (uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[3], (uint32_t)q[4], tc);
      affine_groups(t, npix, tc, s_out, [&](int r, int c, bool first) -> uint32_t {
        if (first)
          w.start(r, c);
        else
          w.step(c == 0);
        return affine_sample<int32_t>(md, (int32_t)w.X, (int32_t)w.Y, tap);
      });
    } else {
      wb = {tap.base, tap.pitch, tap.lead0, tap.stepmod};  // a copy: the staged rows
    }
  } else if (regime == 2) {
    AffineMemTap tap;
    tap.img = img;
    tap.H = H;
    tap.W = W;
    tap.fill = fill;
    AffineWalk<int64_t> w;
    w.init(affine_x(q, x0, y0), affine_y(q, x0, y0), q[0], q[1], q[3], q[4], tc);
    affine_groups(t, npix, tc, s_out, [&](int r, int c, bool first) -> uint32_t {
      if (first)
        w.start(r, c);
      else
        w.step(c == 0);
      return affine_sample<int64_t>(md, w.X, w.Y, tap);
    });
  } else {
    affine_groups(t, npix, tc, s_out, [&](int, int, bool) -> uint32_t { return fill; });
  }
  __syncthreads();

  // ---- write back: the tile's bytes are in LDS, dense (warped) or as staged
  // (a copy).  Rows that span the width leave as one byte range.
  const bool ospan = tc == W;
  const int n_orows = ospan ? 1 : rows;
  const uint32_t orow_bytes = ospan ? (uint32_t)rows * 3u * W : 3u * tc;
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * dst_stride + ((uint64_t)y0 * W + x0) * 3u;
  write_back_rows<AFFINE_THREADS>(t, dst0, step, n_orows, orow_bytes, [&](int y) { return wb.row(y); });
}

namespace {

bool affine_draw_args_ok(const char *who, const void *ids, int batch, double p, const double *rg, int height,
                         int width, const void *apply, const void *coef) {
  if (batch < 0 || !ids || !rg || !apply || !coef || height < 1 || width < 1 || height > FFCV_AFFINE_MAX_DIM ||
      width > FFCV_AFFINE_MAX_DIM || !(p >= 0.0 && p <= 1.0)) {
    ffcv::set_error("%s: invalid arguments (p %g, %dx%d images)", who, p, height, width);
    return false;
  }
  // (lo, hi) pairs: angle, tx, ty, scale, shear x, shear y
  const double lim_lo[6] = {-360.0, -(double)width, -(double)height, 1.0 / 16, -60.0, -60.0};
  const double lim_hi[6] = {360.0, (double)width, (double)height, 16.0, 60.0, 60.0};
  for (int i = 0; i < 6; i++) {
    const double lo = rg[2 * i], hi = rg[2 * i + 1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi) || !(lo >= lim_lo[i]) || !(hi <= lim_hi[i])) {
      ffcv::set_error("%s: range %d is %g .. %g (finite, low <= high, within %g .. %g)", who, i, lo, hi, lim_lo[i],
                      lim_hi[i]);
      return false;
    }
  }
  return true;
}

// the checks of both pixel entries; *stride: the resolved dst stride
bool affine_args_ok(const char *who, const uint8_t *src, const uint8_t *dst, int batch, int height, int width,
                    int mode, const uint8_t *fill, const void *apply, const void *coef, uint64_t dst_stride,
                    uint64_t *stride) {
  if (!ffcv::out_of_place_ok(who, fill && apply && coef, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM,
                             dst_stride, stride))
    return false;
  if ((uint64_t)height * width * 3u > 0x7fffffffull) {
    ffcv::set_error("%s: images of %dx%d exceed the supported 2^31 - 1 bytes", who, height, width);
    return false;
  }
  if (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) {
    ffcv::set_error("%s: mode %d is neither FFCV_AFFINE_BILINEAR nor FFCV_AFFINE_NEAREST", who, mode);
    return false;
  }
  return true;
}

uint32_t pack_fill(const uint8_t *fill) {
  return (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
}

// One image on the host: the kernel's pixel function on 64-bit coordinates.
void affine_image_host(const uint8_t *in, uint8_t *out, int H, int W, int mode, uint32_t fill, const int64_t *q) {
  const bool ok = affine_coef_ok(q);
  AffineMemTap tap;
  tap.img = in;
  tap.H = H;
  tap.W = W;
  tap.fill = fill;
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) {
      const uint32_t v = ok ? affine_sample<int64_t>(mode, affine_x(q, c, r), affine_y(q, c, r), tap) : fill;
      uint8_t *o = out + ((size_t)r * W + c) * 3;
      o[0] = (uint8_t)v;
      o[1] = (uint8_t)(v >> 8);
      o[2] = (uint8_t)(v >> 16);
    }
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_affine_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                           double p, const double *ranges, int height, int width, uint8_t *apply, int64_t *coef,
                           int32_t *status) {
  if (!affine_draw_args_ok("ffcv_affine_draw_batch", sample_ids, batch, p, ranges, height, width, apply, coef))
    return FFCV_EINVAL;
  AffineRanges rg;
  std::memcpy(rg.v, ranges, sizeof(rg.v));
  return ffcv::launch_draw("affine_draw_kernel", affine_draw_kernel, stream, batch, sample_ids, batch, loader_seed,
                           epoch, p, rg, height, width, apply, coef, status);
}

int ffcv_affine_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, double p,
                                const double *ranges, int height, int width, uint8_t *apply, int64_t *coef) {
  if (!affine_draw_args_ok("ffcv_affine_draw_batch_host", sample_ids, batch, p, ranges, height, width, apply, coef))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_affine_draw_batch_host", batch, [&](int k) {
    return draw_affine(k, sample_ids[k], loader_seed, epoch, p, ranges, height, width, apply, coef);
  });
}

uint64_t ffcv_affine_whole_bytes(void) { return AFFINE_WHOLE_BYTES; }
uint64_t ffcv_affine_tile_rows(void) { return AFFINE_TILE_ROWS; }
uint64_t ffcv_affine_tile_cols(void) { return AFFINE_TILE_COLS; }
uint64_t ffcv_affine_tile_lds(void) { return AFFINE_TILE_LDS; }

uint64_t ffcv_affine_tile_bytes(int height, int width, int mode, const int64_t *coef, int tile_row, int tile_col) {
  if (!coef || height < 1 || width < 1 || height > FFCV_AFFINE_MAX_DIM || width > FFCV_AFFINE_MAX_DIM ||
      (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) || !affine_coef_ok(coef))
    return 0;
  const AffinePlan P = affine_plan(height, width);
  if (tile_row < 0 || tile_row >= P.nty || tile_col < 0 || tile_col >= P.ntx) return 0;
  const int y0 = tile_row * P.th, y1 = std::min(height, y0 + P.th), x0 = tile_col * P.tw,
            x1 = std::min(width, x0 + P.tw);
  const AffineBox box = affine_box(coef, mode, height, width, x0, y0, x1, y1, P.whole != 0);
  if (box.empty()) return 0;
  return box.fits32 ? box.staged_bytes(width) : ~(uint64_t)0;
}

int ffcv_affine_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                      const uint8_t *fill, const uint8_t *apply, const int64_t *coef, uint64_t dst_stride_bytes) {
  uint64_t stride;
  if (!affine_args_ok("ffcv_affine_batch", src, dst, batch, height, width, mode, fill, apply, coef, dst_stride_bytes,
                      &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const AffinePlan P = affine_plan(height, width);
  return ffcv::launch_tiles("ffcv_affine_batch", "affine_warp_kernel", affine_warp_kernel, stream,
                            (uint64_t)batch * P.nty * P.ntx, AFFINE_THREADS, P.lds, src, dst, stride, height, width,
                            mode, pack_fill(fill), apply, coef, P);
}

int ffcv_affine_batch_host(const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                           const uint8_t *fill, const uint8_t *apply, const int64_t *coef, uint64_t dst_stride_bytes,
                           int nthreads) {
  uint64_t stride;
  if (!affine_args_ok("ffcv_affine_batch_host", src, dst, batch, height, width, mode, fill, apply, coef,
                      dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const uint32_t f = pack_fill(fill);
  ffcv::host_images(nthreads, batch, src, dst, (uint64_t)height * width * 3, stride,
                    [&](uint64_t k, const uint8_t *in, uint8_t *out, int &) {
                      if (apply[k]) affine_image_host(in, out, height, width, mode, f, coef + k * 6);
                      return apply[k] != 0;
                    });
  return FFCV_OK;
}

}  // extern "C"
