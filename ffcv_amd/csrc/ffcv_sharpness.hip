// ffcv_sharpness.hip -- RandomAdjustSharpness on a dense uint8 batch
// [B][H][W][3] (one launch behind its draw launch), its draw (op id 19), and
// the host twins.
//
// A 256-thread workgroup owns a tile of output rows [y0, y1) x columns
// [x0, x1) of one image:
//
//   1. it stages the tile's source, rows [y0 - 1, y1 + 1) x columns
//      [x0 - 1, x1 + 1) clipped to the image, as uint8 in LDS (the row-tile
//      scheme of lds_stage.h; rows that span the width are one range);
//   2. a thread takes four adjacent BYTES of one output row.  An HWC row is a
//      run of 3 W bytes whose horizontal neighbours lie 3 bytes apart, so the
//      four outputs need the ten bytes [b - 3, b + 7) of three rows: four
//      aligned LDS dwords per row joined by v_alignbyte, each byte converted
//      and multiplied by 1/13 once and shared by the outputs it serves.  The
//      smoothed value and the blend are computed straight from them (no float
//      plane); a byte on the image's outermost ring takes d = i through the
//      same code.  The four bytes go to a second, dense LDS region;
//   3. the bytes leave as 16-byte aligned stores at any alignment of dst;
//      chunks cut by a row's (or the tile's) ends are stored byte by byte.
//
// An image whose apply code is 2 is left alone: its workgroups exit at once.
// One whose code is neither 1 nor 2 runs steps 1 and 3 only (a copy).  The
// tiles, and a copy's pieces, are the band tiles of band_tiles.h at halo 1,
// with this kernel's constants:
//
//   whole image: 6 H W <= SHARP_LDS_BYTES (64 x 64).
//   bands: SHARP_BAND_ROWS rows, in strips where the staged rows and the
//     output bytes exceed SHARP_TILE_LDS.
// A workgroup takes at most SHARP_TILE_LDS = 25 KiB, so six of them (24 waves)
// share a CU's 160 KiB; a 32 x 32 image takes 6.1 KiB and the CU holds the
// eight workgroups (32 waves) that are its wave limit.
#include <cmath>

#include "api_internal.h"
#include "band_tiles.h"
#include "sharpness_common.h"

#define SHARP_THREADS 256
#define SHARP_LDS_BYTES 24576  // whole-image regime: 6 H W at most this
#define SHARP_BAND_ROWS 16
#define SHARP_TILE_LDS 25600  // dynamic LDS of one workgroup, at most
#define SHARP_MAX_DIM 65535   // largest supported height and width
#define SHARP_LDS_LEAD 16     // bytes in front of the staged source: the left taps of a row's first bytes

__global__ void __launch_bounds__(64) sharpness_draw_kernel(const uint64_t *__restrict__ ids, int B,
                                                            uint64_t loader_seed, uint64_t epoch, double p,
                                                            float factor, uint8_t *__restrict__ apply,
                                                            float *__restrict__ factor_out,
                                                            int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_sharpness(k, ids[k], loader_seed, epoch, p, factor, apply, factor_out);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// The plan of a launch (band_tiles.h); dynamic LDS: lead | uint8 region (the
// staged source) | the output bytes, dense, + the look-ahead of the chunks
// assembled from them
static BandPlan sharp_plan(int H, int W) {
  const int band = std::min(H, SHARP_BAND_ROWS), nr = std::min(H, band + 2);  // a band's rows, and its staged rows
  // the first guess, per strip column: 3 bytes per staged row and per output row; fixed: the halo columns, a row's
  // chunk slack, the lead and the look-aheads
  return band_plan(
      H, W, (uint64_t)H * W * 6u <= SHARP_LDS_BYTES, SHARP_BAND_ROWS, SHARP_TILE_LDS, 1,
      [](uint32_t, uint32_t rows, uint32_t cols) { return SHARP_LDS_LEAD + ((rows * 3u * cols + 15u) & ~15u) + 32u; },
      (SHARP_TILE_LDS - 96 - nr * 38) / (3 * (nr + band)));
}

// the ten bytes from LDS address p on (any alignment) as three dwords: four aligned reads joined by v_alignbyte
struct SharpTen {
  uint32_t w0, w1, w2;
  FFCV_DEV explicit SharpTen(const uint8_t *p) {
    const uint32_t *q = (const uint32_t *)__builtin_align_down(p, 4);
    const uint32_t sh = (uint32_t)(p - (const uint8_t *)q);
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    w0 = __builtin_amdgcn_alignbyte(q1, q0, sh);
    w1 = __builtin_amdgcn_alignbyte(q2, q1, sh);
    w2 = __builtin_amdgcn_alignbyte(q3, q2, sh);
  }
  FFCV_DEV float f(int e) const {  // byte e of the ten as a float (e is a constant after unrolling)
    const uint32_t w = e < 4 ? w0 : (e < 8 ? w1 : w2);
    return (float)((w >> (8 * (e & 3))) & 0xffu);
  }
};

__global__ void __launch_bounds__(SHARP_THREADS)
    sharpness_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_stride, int H, int W,
                     const uint8_t *__restrict__ apply, const float *__restrict__ factor, BandPlan P) {
  extern __shared__ uint4 sharp_smem[];
  lds_x4_t *s_u8 = (lds_x4_t *)((uint8_t *)sharp_smem + SHARP_LDS_LEAD);
  uint8_t *s_out = (uint8_t *)s_u8 + P.u8_bytes;
  const int t = threadIdx.x;

  // the image's code (the same for the whole workgroup), and the tile
  const uint32_t k = band_image(blockIdx.x, P);
  const uint32_t code = apply[k];
  if (code == 2) return;
  const bool on = code == 1;
  const float a = on ? factor[k] : 0.f;
  const BandTile T(blockIdx.x, P, H, W, 1);
  if (!on && T.cp_len == 0) return;
  const int y0 = T.y0, x0 = T.x0, lo = T.lo, cl = T.cl, nrows = T.nrows, rows = T.rows, tc = T.tc;

  // ---- stage the tile's source, or the copy's piece
  const BandRows S = T.source(!on, H, W, src);
  const int nchr = (int)lds_chunks(S.bytes);
  stage_rows<SHARP_THREADS>(t, S.a0, T.step, S.n, S.bytes, nchr, s_u8);
  __syncthreads();

  const int rowb = 3 * tc;  // output bytes per tile row
  if (on) {
    const LdsRows<> R = lds_rows(s_u8, S.a0, T.step, S.span, nchr);
    const int ng = (rowb + 3) >> 2;
    const int left = 3 * (x0 - cl) - 3;  // from a staged row's first byte to the left tap of the tile's byte 0
    const int gb0 = 3 * x0, gb_last = 3 * W - 3;
    for (int i = t; i < rows * ng; i += SHARP_THREADS) {
      const int yr = i / ng, b0 = 4 * (i - yr * ng);
      const int y = y0 + yr, rc = y - lo;
      // the rows above and below, kept inside the staged rows: where they are not the neighbours the row is a
      // border row and only its own bytes count
      const SharpTen up(R.row(max(rc - 1, 0)) + left + b0);
      const SharpTen ce(R.row(rc) + left + b0);
      const SharpTen dn(R.row(min(rc + 1, nrows - 1)) + left + b0);
      float pu[10], pc[10], pd[10];
#pragma unroll
      for (int e = 0; e < 10; e++) {
        pu[e] = blur_mul(up.f(e), SHARP_W1);
        pc[e] = blur_mul(ce.f(e), SHARP_W1);
        pd[e] = blur_mul(dn.f(e), SHARP_W1);
      }
      const bool edge_row = y == 0 || y == H - 1;
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float v = ce.f(j + 3);
        const float top = sharp_row(pu[j], pu[j + 3], pu[j + 6]);
        const float mid = sharp_row(pc[j], blur_mul(v, SHARP_W5), pc[j + 6]);
        const float bot = sharp_row(pd[j], pd[j + 3], pd[j + 6]);
        const int gb = gb0 + b0 + j;
        const bool border = edge_row || gb < 3 || gb >= gb_last;
        o[j] = sharp_blend(a, border ? v : sharp_smooth(top, mid, bot), v);
      }
      const int ob = yr * rowb + b0;
      if (!(ob & 3) && b0 + 4 <= rowb) {
        *(uint32_t *)(s_out + ob) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (b0 + j < rowb) s_out[ob + j] = (uint8_t)o[j];
      }
    }
    __syncthreads();
  }

  // ---- write back: the tile's bytes, dense, or the copy's piece as staged.
  // Rows that span the width leave as one byte range.
  const BandRows D = T.dest(!on, W, dst, dst_stride);
  const uint8_t *s_from = on ? s_out : (const uint8_t *)s_u8 + (int)(S.a0 & 15);
  write_back_rows<SHARP_THREADS>(t, D.a0, T.step, D.n, D.bytes, [&](int y) { return s_from + y * rowb; });
}

namespace {

bool sharp_draw_args_ok(const char *who, const void *ids, int batch, double p, double factor, const void *apply,
                        const void *factor_out) {
  if (batch < 0 || !ids || !apply || !factor_out || !(p >= 0.0 && p <= 1.0) || !(factor >= 0.0 && factor <= 16.0)) {
    ffcv::set_error("%s: invalid arguments (p %g, factor %g)", who, p, factor);
    return false;
  }
  return true;
}

// One image on the host: the kernel's arithmetic in the kernel's order.
void sharp_image_host(const uint8_t *in, uint8_t *out, int H, int W, float a) {
  const int pitch = 3 * W;
  for (int y = 0; y < H; y++)
    for (int b = 0; b < pitch; b++) {
      const uint8_t *c = in + (size_t)y * pitch + b;
      const float v = (float)c[0];
      float d = v;
      if (y > 0 && y < H - 1 && b >= 3 && b < pitch - 3) {
        const uint8_t *u = c - pitch, *n = c + pitch;
        const float top = sharp_row(blur_mul((float)u[-3], SHARP_W1), blur_mul((float)u[0], SHARP_W1),
                                    blur_mul((float)u[3], SHARP_W1));
        const float mid = sharp_row(blur_mul((float)c[-3], SHARP_W1), blur_mul(v, SHARP_W5),
                                    blur_mul((float)c[3], SHARP_W1));
        const float bot = sharp_row(blur_mul((float)n[-3], SHARP_W1), blur_mul((float)n[0], SHARP_W1),
                                    blur_mul((float)n[3], SHARP_W1));
        d = sharp_smooth(top, mid, bot);
      }
      out[(size_t)y * pitch + b] = (uint8_t)sharp_blend(a, d, v);
    }
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_sharpness_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                              uint64_t epoch, double p, double factor, uint8_t *apply, float *factor_out,
                              int32_t *status) {
  if (!sharp_draw_args_ok("ffcv_sharpness_draw_batch", sample_ids, batch, p, factor, apply, factor_out))
    return FFCV_EINVAL;
  return ffcv::launch_draw("sharpness_draw_kernel", sharpness_draw_kernel, stream, batch, sample_ids, batch,
                           loader_seed, epoch, p, (float)factor, apply, factor_out, status);
}

int ffcv_sharpness_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                   double p, double factor, uint8_t *apply, float *factor_out) {
  if (!sharp_draw_args_ok("ffcv_sharpness_draw_batch_host", sample_ids, batch, p, factor, apply, factor_out))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_sharpness_draw_batch_host", batch, [&](int k) {
    return draw_sharpness(k, sample_ids[k], loader_seed, epoch, p, (float)factor, apply, factor_out);
  });
}

uint64_t ffcv_sharpness_lds_bytes(void) { return SHARP_LDS_BYTES; }
uint64_t ffcv_sharpness_band_rows(void) { return SHARP_BAND_ROWS; }

uint64_t ffcv_sharpness_strip_cols(int height, int width) {
  if (height <= 0 || width <= 0 || height > SHARP_MAX_DIM || width > SHARP_MAX_DIM) return 0;
  return (uint64_t)sharp_plan(height, width).strip_cols;
}

int ffcv_sharpness_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                         const uint8_t *apply, const float *factor, uint64_t dst_stride_bytes) {
  uint64_t stride;
  if (!ffcv::out_of_place_ok("ffcv_sharpness_batch", apply && factor, src, dst, batch, height, width, SHARP_MAX_DIM,
                             dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const BandPlan P = sharp_plan(height, width);
  return ffcv::launch_tiles("ffcv_sharpness_batch", "sharpness_kernel", sharpness_kernel, stream,
                            (uint64_t)batch * P.nbands * P.nstrips, SHARP_THREADS, P.lds, src, dst, stride, height,
                            width, apply, factor, P);
}

int ffcv_sharpness_batch_host(const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                              const uint8_t *apply, const float *factor, uint64_t dst_stride_bytes, int nthreads) {
  uint64_t stride;
  if (!ffcv::out_of_place_ok("ffcv_sharpness_batch_host", apply && factor, src, dst, batch, height, width,
                             SHARP_MAX_DIM, dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  ffcv::host_images(nthreads, batch, src, dst, (uint64_t)height * width * 3, stride,
                    [&](uint64_t k, const uint8_t *in, uint8_t *out, int &) {
                      if (apply[k] == 1) sharp_image_host(in, out, height, width, factor[k]);
                      return apply[k] == 1 || apply[k] == 2;  // 2: dst is left alone
                    });
  return FFCV_OK;
}

}  // extern "C"
