// ffcv_perspective.hip -- RandomPerspective on a dense uint8 batch
// [B][H][W][3] (one launch behind its draw launch), the draws (op id 26), and
// the host twins.
//
// A projective map is not linear in the output position: a pixel's source
// coordinates are two quotients with a common denominator, so nothing of s21's
// walk by integer increments carries over.  Every pixel evaluates the float64
// statement (perspective_common.h: persp_coords: six products, six sums, ONE
// division, two products) on its own -- a running sum along a row would round
// differently from the statement's products -- and hands the Q16 coordinates
// to s21's integer sample.
//
// One kernel serves every regime.  A 256-thread workgroup owns a tile of
// output rows [y0, y1) x columns [x0, x1) of one image, and decides, the same
// for all its threads, how the tile's taps are read:
//
//   staged: den > 0 on the tile's four corner pixels and the source footprint
//           (persp_box: the corners' bounding box, widened) takes at most the
//           tile's LDS budget: its rows are staged as uint8 in LDS, a tile of
//           rows (lds_stage.h).  Coordinates are 32-bit, relative to the box's
//           corner.  Every tap is tested against the box: one outside it and
//           inside the image is read from global memory, one outside the image
//           is fill.  So the result never rests on the footprint argument.
//   direct: a corner on or behind the horizon, or a footprint beyond the
//           budget (the far edge of a strong quadrilateral): taps come from
//           global memory, coordinates are 64-bit.
//   empty:  the box misses the image.  The direct code runs; every tap is
//           tested on its own and misses, so nothing is read and fill is stored.
//
// Every thread computes four adjacent pixels at a time, twelve bytes, into an
// LDS copy of the tile's output, dense; those bytes leave by the row tile's
// write-back at any alignment of dst, aligned 16-byte stores where a chunk
// lies inside the range.  An image whose apply flag is 0 stages its tile and
// the staged bytes leave as they came: a copy.
//
//   whole image: 3 H W <= PERSP_WHOLE_BYTES -- one tile per image, the image
//     staged once as one byte range, every tap from LDS.
//   tiles: PERSP_TILE_ROWS x PERSP_TILE_COLS outputs; the staged footprint
//     takes at most PERSP_TILE_LDS bytes.
#include <cmath>
#include <cstring>

#include "api_internal.h"
#include "perspective_common.h"

#define PERSP_THREADS 256
#ifndef PERSP_WHOLE_BYTES
#define PERSP_WHOLE_BYTES 16384  // whole-image regime: 3 H W at most this
#endif
#ifndef PERSP_TILE_ROWS
#define PERSP_TILE_ROWS 32
#endif
#ifndef PERSP_TILE_COLS
#define PERSP_TILE_COLS 32
#endif
#ifndef PERSP_TILE_LDS
#define PERSP_TILE_LDS 16384  // staged footprint of a tile, at most
#endif
// a tile that is copied stages its own pixels, a range per row
static_assert(PERSP_TILE_ROWS * (((3 * PERSP_TILE_COLS + 30) >> 4) * 16) <= PERSP_TILE_LDS, "a copied tile must fit");

__global__ void __launch_bounds__(64) perspective_draw_kernel(const uint64_t *__restrict__ ids, int B,
                                                              uint64_t loader_seed, uint64_t epoch, double p, double d,
                                                              int H, int W, uint8_t *__restrict__ apply,
                                                              double *__restrict__ coef, int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_perspective(k, ids[k], loader_seed, epoch, p, d, H, W, apply, coef);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// How a launch cuts an image into tiles, and the LDS a workgroup takes:
// 16 bytes | staged source | 16 bytes | output bytes | 32 bytes
struct PerspPlan {
  int th, tw, nty, ntx, whole;
  uint32_t budget;   // staged bytes a tile may take
  uint32_t out_off;  // byte offset of the output region, a multiple of 16
  uint32_t lds;
};

static PerspPlan persp_plan(int H, int W) {
  PerspPlan P;
  P.whole = (uint64_t)H * W * 3u <= PERSP_WHOLE_BYTES;
  P.th = P.whole ? H : std::min(H, PERSP_TILE_ROWS);
  P.tw = P.whole ? W : std::min(W, PERSP_TILE_COLS);
  P.nty = (H + P.th - 1) / P.th;
  P.ntx = (W + P.tw - 1) / P.tw;
  P.budget = P.whole ? lds_chunks(3u * H * W) * 16u : PERSP_TILE_LDS;
  P.out_off = 16u + P.budget + 16u;
  P.lds = P.out_off + ((3u * P.th * P.tw + 15u) & ~15u) + 32u;
  return P;
}

// Taps from the staged box (a tile of rows, lds_stage.h): coordinates relative
// to its corner (lo, cl).  A tap outside the box is the image's own tap: from
// global memory inside the image, fill outside it.
struct PerspLdsTap : LdsRows<true> {
  int nrows, cw, lo, cl;
  AffineMemTap mem;
  // the LDS read is outside the branch, at a clamped address, so that the reads
  // of a thread's four pixels can be in flight together; the branch is taken by
  // taps at the image's border (no load) and, rarely, by a tap the box missed
  FFCV_DEV uint32_t one(int iy, int ix) const {
    const bool ok = (uint32_t)iy < (uint32_t)nrows && (uint32_t)ix < (uint32_t)cw;
    uint32_t v = lds_pixel(row(ok ? iy : 0) + 3 * (ok ? ix : 0)) & 0xffffffu;
    if (!ok) v = mem.one((int64_t)iy + lo, (int64_t)ix + cl);
    return v;
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
    const uint32_t lo4 = __builtin_amdgcn_alignbyte(q1, q0, sh), hi4 = __builtin_amdgcn_alignbyte(q2, q1, sh);
    uint32_t v0 = lo4 & 0xffffffu, v1 = ((lo4 >> 24) | (hi4 << 8)) & 0xffffffu;
    if (!(rok & ((uint32_t)ix < (uint32_t)cw))) v0 = mem.one((int64_t)iy + lo, (int64_t)ix + cl);
    if (!(rok & ((uint32_t)(ix + 1) < (uint32_t)cw))) v1 = mem.one((int64_t)iy + lo, (int64_t)ix + cl + 1);
    *t0 = v0;
    *t1 = v1;
  }
};

// f / tc for 0 <= f < 2^22, 0 < tc < 2^15 with inv = 1.0f / tc: the float
// quotient is off by less than one, so one correction either way settles it
FFCV_DEV int persp_div(int f, int tc, float inv) {
  int r = (int)((float)f * inv);
  r -= (int)(__mul24(r, tc) > f);
  r += (int)(__mul24(r + 1, tc) <= f);
  return r;
}

// The tile's pixels, four adjacent ones (in row-major order of the tile) per
// thread and step, as three aligned dwords into the dense output bytes.
// pix(r, c): the pixel at tile row r, column c.  The last group may run up to
// three pixels past the tile: they are computed like any other (every tap is
// bounds-checked), land in the bytes behind the tile's and are never stored.
template <class F>
FFCV_DEV void persp_groups(int t, int npix, int tc, uint32_t *s_out, F pix) {
  const float inv = 1.0f / (float)tc;
  for (int g = t; 4 * g < npix; g += PERSP_THREADS) {
    int r = persp_div(4 * g, tc, inv), c = 4 * g - __mul24(r, tc);
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      v[e] = pix(r, c);
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

__global__ void __launch_bounds__(PERSP_THREADS)
    perspective_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_stride, int H,
                            int W, int mode, uint32_t fill, const uint8_t *__restrict__ apply,
                            const double *__restrict__ coef, PerspPlan P) {
  extern __shared__ uint4 persp_smem[];
  lds_x4_t *s_u8 = (lds_x4_t *)persp_smem + 1;  // staged chunks, behind 16 bytes a tap at column -1 may read
  uint32_t *s_out = (uint32_t *)((uint8_t *)persp_smem + P.out_off);
  const int t = threadIdx.x;
  const uint32_t per = (uint32_t)P.nty * P.ntx;
  const uint32_t k = blockIdx.x / per, rem = blockIdx.x - k * per;
  const int ty = rem / P.ntx, tx = rem - ty * P.ntx;
  const int y0 = ty * P.th, y1 = min(H, y0 + P.th), x0 = tx * P.tw, x1 = min(W, x0 + P.tw);
  const int rows = y1 - y0, tc = x1 - x0;

  // the image's decision and coefficients, the same for the whole workgroup
  // (a byte load lands in a vector register: readfirstlane tells the compiler
  // that the flag is scalar)
  const bool on = __builtin_amdgcn_readfirstlane((int)apply[k]) != 0;
  double q[9];
#pragma unroll
  for (int i = 0; i < 9; i++) q[i] = coef[(uint64_t)k * 9 + i];
  if (!on) {  // the identity under nearest, should a copied tile ever not be staged
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = i % 4 == 0 ? 1.0 : 0.0;
  }
  const int md = on ? mode : FFCV_AFFINE_NEAREST;

  // the staged box: the footprint, or the tile itself for a copy; float64 has
  // no scalar unit, so the box is computed by every lane and then declared
  // uniform
  PerspBox box = persp_box(q, md, H, W, x0, y0, x1, y1, P.whole != 0);
  if (!on && !P.whole) {
    box.lo = y0, box.hi = y1, box.cl = x0, box.ch = x1;
    box.direct = false;
  }
  box.lo = __builtin_amdgcn_readfirstlane(box.lo);
  box.hi = __builtin_amdgcn_readfirstlane(box.hi);
  box.cl = __builtin_amdgcn_readfirstlane(box.cl);
  box.ch = __builtin_amdgcn_readfirstlane(box.ch);
  const bool staged =
      __builtin_amdgcn_readfirstlane((int)(!box.direct && !box.empty() && box.staged_bytes(W) <= P.budget)) != 0;

  const uint64_t step = (uint64_t)W * 3u;
  const uint8_t *img = src + (uint64_t)k * H * step;
  const int npix = rows * tc;
  AffineMemTap mem;
  mem.img = img;
  mem.H = H;
  mem.W = W;
  mem.fill = fill;
  // where the write-back finds range y: the tile's dense output bytes
  LdsRows<> wb = {(const uint8_t *)s_out, 3 * tc, 0, 0};
  if (staged) {
    // ---- stage source rows [lo, hi) x columns [cl, ch) as a tile of rows (lds_stage.h)
    const int nrows = box.hi - box.lo, cw = box.ch - box.cl;
    const uint64_t src0 = (uint64_t)(uintptr_t)img + ((uint64_t)box.lo * W + box.cl) * 3u;
    const bool span = cw == W;
    const int n_srows = span ? 1 : nrows;
    const uint32_t srow_bytes = span ? (uint32_t)nrows * 3u * W : 3u * cw;
    const int nchr = (int)lds_chunks(srow_bytes);
    stage_rows<PERSP_THREADS>(t, src0, step, n_srows, srow_bytes, nchr, s_u8);
    __syncthreads();
    const PerspLdsTap tap{lds_rows<true>(s_u8, src0, step, span, nchr), nrows, cw, box.lo, box.cl, mem};
    if (on) {
      // A pixel with X outside [-1, W) or Y outside [-1, H) has every tap
      // outside the image: fill.  The others' coordinates less the box's corner
      // lie within (-2^31, 2^31): 32-bit arithmetic on them is exact.
      const int64_t Wq = (int64_t)W << 16, Hq = (int64_t)H << 16;
      const int64_t ox = (int64_t)box.cl << 16, oy = (int64_t)box.lo << 16;
      persp_groups(t, npix, tc, s_out, [&](int r, int c) -> uint32_t {
        int64_t Xq, Yq;
        const bool in = persp_coords(q, x0 + c, y0 + r, &Xq, &Yq) && Xq >= -65536 && Xq < Wq && Yq >= -65536 && Yq < Hq;
        if (!in) return fill;
        return affine_sample<int32_t>(md, (int32_t)(Xq - ox), (int32_t)(Yq - oy), tap);
      });
    } else {
      wb = {tap.base, tap.pitch, tap.lead0, tap.stepmod};  // a copy: the staged rows
    }
  } else {
    persp_groups(t, npix, tc, s_out,
                 [&](int r, int c) -> uint32_t { return persp_pixel(q, md, x0 + c, y0 + r, fill, mem); });
  }
  __syncthreads();

  // ---- write back: the tile's bytes are in LDS, dense (warped) or as staged
  // (a copy).  Rows that span the width leave as one byte range.
  const bool ospan = tc == W;
  const int n_orows = ospan ? 1 : rows;
  const uint32_t orow_bytes = ospan ? (uint32_t)rows * 3u * W : 3u * tc;
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * dst_stride + ((uint64_t)y0 * W + x0) * 3u;
  write_back_rows<PERSP_THREADS>(t, dst0, step, n_orows, orow_bytes, [&](int y) { return wb.row(y); });
}

namespace {

bool persp_draw_args_ok(const char *who, const void *ids, int batch, double p, double d, int height, int width,
                        const void *apply, const void *coef) {
  if (batch < 0 || !ids || !apply || !coef || height < FFCV_PERSPECTIVE_MIN_DIM || width < FFCV_PERSPECTIVE_MIN_DIM ||
      height > FFCV_AFFINE_MAX_DIM || width > FFCV_AFFINE_MAX_DIM || !(p >= 0.0 && p <= 1.0) ||
      !(d >= 0.0 && d <= 1.0)) {
    ffcv::set_error("%s: invalid arguments (p %g, distortion scale %g, %dx%d images)", who, p, d, height, width);
    return false;
  }
  return true;
}

// the checks of both pixel entries; *stride: the resolved dst stride
bool persp_args_ok(const char *who, const uint8_t *src, const uint8_t *dst, int batch, int height, int width, int mode,
                   const uint8_t *fill, const void *apply, const void *coef, uint64_t dst_stride, uint64_t *stride) {
  if (!ffcv::out_of_place_ok(who, fill && apply && coef, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM,
                             dst_stride, stride))
    return false;
  if (height < FFCV_PERSPECTIVE_MIN_DIM || width < FFCV_PERSPECTIVE_MIN_DIM) {
    ffcv::set_error("%s: images of %dx%d have a side below 2", who, height, width);
    return false;
  }
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

uint32_t persp_pack_fill(const uint8_t *fill) {
  return (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_perspective_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                uint64_t epoch, double p, double distortion_scale, int height, int width,
                                uint8_t *apply, double *coef, int32_t *status) {
  if (!persp_draw_args_ok("ffcv_perspective_draw_batch", sample_ids, batch, p, distortion_scale, height, width, apply,
                          coef))
    return FFCV_EINVAL;
  return ffcv::launch_draw("perspective_draw_kernel", perspective_draw_kernel, stream, batch, sample_ids, batch,
                           loader_seed, epoch, p, distortion_scale, height, width, apply, coef, status);
}

int ffcv_perspective_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                     double p, double distortion_scale, int height, int width, uint8_t *apply,
                                     double *coef) {
  if (!persp_draw_args_ok("ffcv_perspective_draw_batch_host", sample_ids, batch, p, distortion_scale, height, width,
                          apply, coef))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_perspective_draw_batch_host", batch, [&](int k) {
    return draw_perspective(k, sample_ids[k], loader_seed, epoch, p, distortion_scale, height, width, apply, coef);
  });
}

uint64_t ffcv_perspective_whole_bytes(void) { return PERSP_WHOLE_BYTES; }
uint64_t ffcv_perspective_tile_rows(void) { return PERSP_TILE_ROWS; }
uint64_t ffcv_perspective_tile_cols(void) { return PERSP_TILE_COLS; }
uint64_t ffcv_perspective_tile_lds(void) { return PERSP_TILE_LDS; }

uint64_t ffcv_perspective_tile_bytes(int height, int width, int mode, const double *coef, int tile_row, int tile_col) {
  if (!coef || height < FFCV_PERSPECTIVE_MIN_DIM || width < FFCV_PERSPECTIVE_MIN_DIM ||
      height > FFCV_AFFINE_MAX_DIM || width > FFCV_AFFINE_MAX_DIM ||
      (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST))
    return 0;
  const PerspPlan P = persp_plan(height, width);
  if (tile_row < 0 || tile_row >= P.nty || tile_col < 0 || tile_col >= P.ntx) return 0;
  const int y0 = tile_row * P.th, y1 = std::min(height, y0 + P.th), x0 = tile_col * P.tw,
            x1 = std::min(width, x0 + P.tw);
  const PerspBox box = persp_box(coef, mode, height, width, x0, y0, x1, y1, P.whole != 0);
  return box.direct ? ~(uint64_t)0 : box.staged_bytes(width);
}

int ffcv_perspective_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                           const uint8_t *fill, const uint8_t *apply, const double *coef, uint64_t dst_stride_bytes) {
  uint64_t stride;
  if (!persp_args_ok("ffcv_perspective_batch", src, dst, batch, height, width, mode, fill, apply, coef,
                     dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const PerspPlan P = persp_plan(height, width);
  return ffcv::launch_tiles("ffcv_perspective_batch", "perspective_warp_kernel", perspective_warp_kernel, stream,
                            (uint64_t)batch * P.nty * P.ntx, PERSP_THREADS, P.lds, src, dst, stride, height, width,
                            mode, persp_pack_fill(fill), apply, coef, P);
}

int ffcv_perspective_batch_host(const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                                const uint8_t *fill, const uint8_t *apply, const double *coef,
                                uint64_t dst_stride_bytes, int nthreads) {
  uint64_t stride;
  if (!persp_args_ok("ffcv_perspective_batch_host", src, dst, batch, height, width, mode, fill, apply, coef,
                     dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const uint32_t f = persp_pack_fill(fill);
  ffcv::host_images(nthreads, batch, src, dst, (uint64_t)height * width * 3, stride,
                    [&](uint64_t k, const uint8_t *in, uint8_t *out, int &) {
                      if (!apply[k]) return false;
                      AffineMemTap tap;
                      tap.img = in;
                      tap.H = height;
                      tap.W = width;
                      tap.fill = f;
                      for (int r = 0; r < height; r++)
                        for (int c = 0; c < width; c++) {
                          const uint32_t v = persp_pixel(coef + k * 9, mode, c, r, f, tap);
                          uint8_t *o = out + ((size_t)r * width + c) * 3;
                          o[0] = (uint8_t)v;
                          o[1] = (uint8_t)(v >> 8);
                          o[2] = (uint8_t)(v >> 16);
                        }
                      return true;
                    });
  return FFCV_OK;
}

}  // extern "C"
