// ffcv_blur.hip -- GaussianBlur on a dense uint8 batch [B][H][W][3] (one
// launch behind its draw launch), its draw (op id 11), and the host twins.
//
// One kernel serves both regimes.  A 256-thread workgroup owns a tile of
// output rows [y0, y1) x columns [x0, x1) of one image:
//
//   1. it stages the tile's source, rows [y0 - r, y1 + r) x columns
//      [x0 - r, x1 + r) clipped to the image, as uint8 in LDS: a tile of rows
//      (the scheme of lds_stage.h; rows that span the width are one range);
//   2. horizontal pass: one float32 per staged row and tile column and
//      channel into an LDS plane, border columns reflected at read time, a
//      thread per four adjacent columns;
//   3. vertical pass over that plane, border rows reflected at read time (a
//      reflected row is always one of the staged rows), a thread per column
//      and four adjacent rows, rounded to uint8 into the LDS bytes the source
//      no longer needs;
//   4. the bytes leave as 16-byte aligned stores at any alignment of dst;
//      chunks cut by a row's (or the tile's) ends are stored byte by byte.
//
// The float32 intermediate never touches global memory.  An image whose
// apply flag is 0 runs steps 1 and 4 only (a copy).  The tiles, and a copy's
// pieces, are the band tiles of band_tiles.h, with this kernel's constants:
//
//   whole image: 15 H W <= BLUR_LDS_BYTES.  At the bound a workgroup takes
//     32.2 KiB of LDS, so four of them (16 waves, four per SIMD) share a CU's
//     160 KiB; a 32 x 32 image takes 15.2 KiB and the CU holds the eight
//     workgroups (32 waves) that are its wave limit.
//   bands: BLUR_BAND_ROWS rows, in strips where the staged rows and the float
//     plane exceed BLUR_TILE_LDS (40 KiB: four workgroups per CU again).
#include <cmath>

#include "api_internal.h"
#include "band_tiles.h"
#include "blur_common.h"

#define BLUR_THREADS 256
#define BLUR_LDS_BYTES 32768  // whole-image regime: 15 H W at most this
#define BLUR_BAND_ROWS 32
#define BLUR_TILE_LDS 40960  // dynamic LDS of one band-regime workgroup, at most
#define BLUR_MAX_DIM 65535   // largest supported height and width
// the weights in LDS: up to 31 and the +0 padding of a four-output walk (34 floats in all), in whole chunks
#define BLUR_W_LDS 144

__global__ void __launch_bounds__(64) blur_draw_kernel(const uint64_t *__restrict__ ids, int B,
                                                       uint64_t loader_seed, uint64_t epoch, double p, double lo,
                                                       double hi, int ksize, uint8_t *__restrict__ apply,
                                                       double *__restrict__ sigma, float *__restrict__ weights,
                                                       int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_blur(k, ids[k], loader_seed, epoch, p, lo, hi, ksize, apply, sigma, weights);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// The plan of a launch (band_tiles.h); dynamic LDS: weights | uint8 region
// (staged source, later the output bytes) | float plane
static BandPlan blur_plan(int H, int W, int ksize) {
  const int r = (ksize - 1) / 2, nr = std::min(H, std::min(H, BLUR_BAND_ROWS) + 2 * r);  // a band's staged rows
  // the first guess, per strip column: 15 bytes per staged row; fixed: the halo columns, a row's chunk slack, the
  // weights
  return band_plan(
      H, W, (uint64_t)H * W * 15u <= BLUR_LDS_BYTES, BLUR_BAND_ROWS, BLUR_TILE_LDS, r,
      [](uint32_t nrows, uint32_t, uint32_t cols) { return BLUR_W_LDS + nrows * cols * 12u; },
      (BLUR_TILE_LDS - 176 - nr * (6 * r + 32)) / (15 * nr));
}

__global__ void __launch_bounds__(BLUR_THREADS)
    gaussian_blur_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_stride, int H, int W,
                         int ksize, const uint8_t *__restrict__ apply, const float *__restrict__ weights,
                         BandPlan P) {
  extern __shared__ uint4 blur_smem[];
  typedef uint32_t bx4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(1))) bx4_t gx4_t;
  float *s_w = (float *)blur_smem;
  bx4_t *s_u8 = (bx4_t *)((uint8_t *)blur_smem + BLUR_W_LDS);
  float *s_h = (float *)((uint8_t *)blur_smem + BLUR_W_LDS + P.u8_bytes);
  const int t = threadIdx.x;
  // the workgroup's tile: BandTile (band_tiles.h) written out, like the staging and the write back below (on the
  // struct the 32 x 32 launches measured slower, profiles/band_tiles_ab.txt)
  const uint32_t per = (uint32_t)P.nbands * P.nstrips;
  const uint32_t k = blockIdx.x / per, rem = blockIdx.x - k * per;
  const int band = rem / P.nstrips, strip = rem - band * P.nstrips;

  // the image's decision (the same for the whole workgroup)
  const bool on = apply[k] != 0;
  const int r = (ksize - 1) / 2;
  const int y0 = band * P.band_rows, y1 = min(H, y0 + P.band_rows);
  const int x0 = strip * P.strip_cols, x1 = min(W, x0 + P.strip_cols);
  const int lo = max(0, y0 - r), hi = min(H, y1 + r), cl = max(0, x0 - r), ch = min(W, x1 + r);
  const int nrows = hi - lo, cw = ch - cl, rows = y1 - y0, tc = x1 - x0;

  // ---- stage source rows [lo, hi) x columns [cl, ch).  This and the write
  // back are the row-tile scheme of lds_stage.h written out: on the helpers
  // the copy path measured slower (profiles/lds_stage_ab.txt).  One contiguous
  // byte range when the rows span the width, else a range per row in whole
  // chunks.  A copy needs no halo and no columns: the band's rows
  // are one byte range of the image, and the band's workgroups (one per
  // strip) take an equal piece of it each, never more than a tile's bytes.
  const uint64_t step = (uint64_t)W * 3u;
  const uint32_t band_bytes = (uint32_t)rows * 3u * W, piece = (band_bytes + P.nstrips - 1) / P.nstrips;
  const uint32_t cp0 = min(band_bytes, (uint32_t)strip * piece), cp_len = min(piece, band_bytes - cp0);
  if (!on && cp_len == 0) return;
  const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * H * step +
                        (on ? ((uint64_t)lo * W + cl) * 3u : (uint64_t)y0 * step + cp0);
  const bool span = !on || cw == W;
  const int n_srows = span ? 1 : nrows;
  const uint32_t srow_bytes = !on ? cp_len : (span ? (uint32_t)nrows * 3u * W : 3u * cw);
  const int nchr = (int)lds_chunks(srow_bytes);
  const int pitch = span ? 3 * W : nchr * 16;  // LDS bytes from a staged row to the next
  const int lead0 = (int)(src0 & 15), stepmod = span ? 0 : (int)(step & 15);
  for (int i = t; i < n_srows * nchr; i += BLUR_THREADS) {
    const int rr = i / nchr, c = i - rr * nchr;
    const uint64_t ra = src0 + (uint64_t)rr * step;
    if (c < (int)(((ra & 15) + srow_bytes + 15) >> 4)) s_u8[i] = ((gx4_t *)(uintptr_t)(ra & ~(uint64_t)15))[c];
  }
  if (t < BLUR_W_LDS / 4) s_w[t] = on && t < ksize ? weights[(uint64_t)k * FFCV_BLUR_WROW + t] : 0.f;  // padded with +0
  __syncthreads();
  const uint8_t *s_bytes = (const uint8_t *)s_u8;
  // first byte of staged row `row` (column cl)
  auto rowoff = [&](int row) -> int { return row * pitch + ((lead0 + row * stepmod) & 15); };
  // a pixel's R | G << 8 | B << 16 from two ALIGNED 4-byte LDS reads joined by
  // v_alignbyte (misaligned LDS reads are several times slower); reads up to
  // 7 bytes past the pixel's first, inside the region's look-ahead
  auto pixel = [&](const uint8_t *a) -> uint32_t {
    const uint32_t *qa = (const uint32_t *)__builtin_align_down(a, 4);
    return __builtin_amdgcn_alignbyte(qa[1], qa[0], (uint32_t)(a - (const uint8_t *)qa));
  };

  const int pitchf = 3 * tc;  // floats per row of the plane
  uint8_t *s_out = (uint8_t *)s_u8;
  if (on) {
    // Both passes give a thread four adjacent outputs along the pass's axis
    // and walk the k + 3 source values under them once: each value is read
    // and converted once and meets the four outputs' weights (w_m, w_m-1,
    // w_m-2, w_m-3, kept in registers as the walk moves on).  Every output
    // still adds its taps in ascending order.  Taps outside 0 .. k - 1 have
    // weight +0 (s_w is padded): their products are zeros, which leave a sum
    // as it is, and an accumulator that starts at +0 takes its first product
    // exactly.
    // ---- horizontal pass: a thread per staged row and four tile columns
    const int ngx = (tc + 3) >> 2;
    for (int i = t; i < nrows * ngx; i += BLUR_THREADS) {
      const int row = i / ngx, xg = 4 * (i - row * ngx);
      const int last = ksize + min(4, tc - xg) - 2;  // the walk's last step: no column past the tile's halo
      const uint8_t *base = s_bytes + rowoff(row) - 3 * cl;
      const int xs = x0 + xg - r;
      float a[12];
#pragma unroll
      for (int e = 0; e < 12; e++) a[e] = 0.f;
      float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3;
      for (int m = 0; m <= last; m++) {
        w3 = w2;
        w2 = w1;
        w1 = w0;
        w0 = s_w[m];
        const uint32_t v = pixel(base + 3 * blur_reflect(xs + m, W));
        const float f[3] = {(float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu)};
#pragma unroll
        for (int c = 0; c < 3; c++) {
          a[c] = blur_add(a[c], blur_mul(w0, f[c]));
          a[3 + c] = blur_add(a[3 + c], blur_mul(w1, f[c]));
          a[6 + c] = blur_add(a[6 + c], blur_mul(w2, f[c]));
          a[9 + c] = blur_add(a[9 + c], blur_mul(w3, f[c]));
        }
      }
      float *o = s_h + row * pitchf + 3 * xg;
#pragma unroll
      for (int e = 0; e < 12; e++)
        if (e < 3 * (tc - xg)) o[e] = a[e];
    }
    __syncthreads();
    // ---- vertical pass: a thread per float column and four output rows;
    // the rounded bytes go, dense, where the staged source was
    const int ngy = (rows + 3) >> 2;
    for (int i = t; i < ngy * pitchf; i += BLUR_THREADS) {
      const int g = i / pitchf, c = i - g * pitchf, yg = 4 * g;
      const int nv = min(4, rows - yg);
      const float *col = s_h + c - lo * pitchf;
      const int ys = y0 + yg - r;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f, w3;
      for (int m = 0; m <= ksize + nv - 2; m++) {  // no row past the tile's halo
        w3 = w2;
        w2 = w1;
        w1 = w0;
        w0 = s_w[m];
        const float h = col[blur_reflect(ys + m, H) * pitchf];
        a0 = blur_add(a0, blur_mul(w0, h));
        a1 = blur_add(a1, blur_mul(w1, h));
        a2 = blur_add(a2, blur_mul(w2, h));
        a3 = blur_add(a3, blur_mul(w3, h));
      }
      uint8_t *o = s_out + yg * pitchf + c;
      o[0] = (uint8_t)blur_round_u8(a0);
      if (nv > 1) o[pitchf] = (uint8_t)blur_round_u8(a1);
      if (nv > 2) o[2 * pitchf] = (uint8_t)blur_round_u8(a2);
      if (nv > 3) o[3 * pitchf] = (uint8_t)blur_round_u8(a3);
    }
    __syncthreads();
  }

  // ---- write back: the bytes are in LDS, the tile's, dense (blurred), or
  // the copy's piece as staged.  Rows that span the width leave as one byte
  // range.  Whole 16-byte chunks of dst inside a range are one store,
  // assembled from five aligned LDS dwords; the chunks cut by its ends go
  // byte by byte.
  const bool ospan = !on || tc == W;
  const int n_orows = ospan ? 1 : rows;
  const uint32_t orow_bytes = !on ? cp_len : (ospan ? band_bytes : 3u * tc);
  const int onch = (int)lds_chunks(orow_bytes);
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * dst_stride +
                        (on ? ((uint64_t)y0 * W + x0) * 3u : (uint64_t)y0 * step + cp0);
  for (int i = t; i < n_orows * onch; i += BLUR_THREADS) {
    const int y = i / onch, c = i - y * onch;
    const uint64_t da = dst0 + (uint64_t)y * step;
    const int dl = (int)(da & 15), c0 = 16 * c;  // the range is bytes [dl, dl + orow_bytes) of the aligned row
    if (c0 >= dl + (int)orow_bytes) continue;
    const uint8_t *sp = s_bytes + (on ? y * pitchf : lead0) + (c0 - dl);
    uint8_t *gb = (uint8_t *)(uintptr_t)(da & ~(uint64_t)15) + c0;
    if (c0 >= dl && c0 + 16 <= dl + (int)orow_bytes) {
      const uint32_t *q = (const uint32_t *)__builtin_align_down(sp, 4);
      const uint32_t sh = (uint32_t)(sp - (const uint8_t *)q);
      const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
      bx4_t o;
      o.x = __builtin_amdgcn_alignbyte(q1, q0, sh);
      o.y = __builtin_amdgcn_alignbyte(q2, q1, sh);
      o.z = __builtin_amdgcn_alignbyte(q3, q2, sh);
      o.w = __builtin_amdgcn_alignbyte(q4, q3, sh);
      *(gx4_t *)gb = o;
    } else {
      for (int j = 0; j < 16; j++) {
        const int b = c0 + j - dl;
        if (b >= 0 && b < (int)orow_bytes) gb[j] = sp[j];
      }
    }
  }
}

namespace {

bool blur_draw_args_ok(const char *who, const void *ids, int batch, double p, double lo, double hi, int ksize,
                       const void *apply, const void *sigma, const void *weights) {
  if (batch < 0 || !ids || !apply || !sigma || !weights || !(p >= 0.0 && p <= 1.0) || !std::isfinite(lo) ||
      !std::isfinite(hi) || !(lo > 0.0) || !(lo <= hi) || ksize < 1 || ksize > FFCV_BLUR_MAX_K || !(ksize & 1)) {
    ffcv::set_error("%s: invalid arguments (p %g, sigma %g .. %g, ksize %d)", who, p, lo, hi, ksize);
    return false;
  }
  return true;
}

// the checks of both pixel entries; *stride: the resolved dst stride
bool blur_args_ok(const char *who, const uint8_t *src, const uint8_t *dst, int batch, int height, int width,
                  int ksize, const void *apply, const void *weights, uint64_t dst_stride, uint64_t *stride) {
  if (!ffcv::out_of_place_ok(who, apply && weights, src, dst, batch, height, width, BLUR_MAX_DIM, dst_stride, stride))
    return false;
  if (ksize < 1 || ksize > FFCV_BLUR_MAX_K || !(ksize & 1) || (ksize - 1) / 2 >= std::min(height, width)) {
    ffcv::set_error("%s: ksize %d on %dx%d images (odd, 1 .. %d, (ksize - 1) / 2 < min(height, width))", who, ksize,
                    height, width, FFCV_BLUR_MAX_K);
    return false;
  }
  return true;
}

// One image on the host: the kernel's arithmetic in the kernel's order.
void blur_image_host(const uint8_t *in, uint8_t *out, int H, int W, int ksize, const float *w,
                     std::vector<float> &plane) {
  const int r = (ksize - 1) / 2, pitchf = 3 * W;
  plane.resize((size_t)H * pitchf);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++)
      for (int c = 0; c < 3; c++) {
        const uint8_t *row = in + (size_t)y * pitchf + c;
        float acc = blur_mul(w[0], (float)row[3 * blur_reflect(x - r, W)]);
        for (int j = 1; j < ksize; j++) acc = blur_add(acc, blur_mul(w[j], (float)row[3 * blur_reflect(x - r + j, W)]));
        plane[(size_t)y * pitchf + 3 * x + c] = acc;
      }
  for (int y = 0; y < H; y++)
    for (int c = 0; c < pitchf; c++) {
      const float *col = plane.data() + c;
      float acc = blur_mul(w[0], col[(size_t)blur_reflect(y - r, H) * pitchf]);
      for (int j = 1; j < ksize; j++)
        acc = blur_add(acc, blur_mul(w[j], col[(size_t)blur_reflect(y - r + j, H) * pitchf]));
      out[(size_t)y * pitchf + c] = (uint8_t)blur_round_u8(acc);
    }
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_blur_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                         double p, double sigma_lo, double sigma_hi, int ksize, uint8_t *apply, double *sigma,
                         float *weights, int32_t *status) {
  if (!blur_draw_args_ok("ffcv_blur_draw_batch", sample_ids, batch, p, sigma_lo, sigma_hi, ksize, apply, sigma,
                         weights))
    return FFCV_EINVAL;
  return ffcv::launch_draw("blur_draw_kernel", blur_draw_kernel, stream, batch, sample_ids, batch, loader_seed, epoch,
                           p, sigma_lo, sigma_hi, ksize, apply, sigma, weights, status);
}

int ffcv_blur_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, double p,
                              double sigma_lo, double sigma_hi, int ksize, uint8_t *apply, double *sigma,
                              float *weights) {
  if (!blur_draw_args_ok("ffcv_blur_draw_batch_host", sample_ids, batch, p, sigma_lo, sigma_hi, ksize, apply, sigma,
                         weights))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_blur_draw_batch_host", batch, [&](int k) {
    return draw_blur(k, sample_ids[k], loader_seed, epoch, p, sigma_lo, sigma_hi, ksize, apply, sigma, weights);
  });
}

uint64_t ffcv_gaussian_blur_lds_bytes(void) { return BLUR_LDS_BYTES; }
uint64_t ffcv_gaussian_blur_band_rows(void) { return BLUR_BAND_ROWS; }

uint64_t ffcv_gaussian_blur_strip_cols(int height, int width, int ksize) {
  if (height <= 0 || width <= 0 || height > BLUR_MAX_DIM || width > BLUR_MAX_DIM || ksize < 1 ||
      ksize > FFCV_BLUR_MAX_K || !(ksize & 1))
    return 0;
  return (uint64_t)blur_plan(height, width, ksize).strip_cols;
}

int ffcv_gaussian_blur_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                             int ksize, const uint8_t *apply, const float *weights, uint64_t dst_stride_bytes) {
  uint64_t stride;
  if (!blur_args_ok("ffcv_gaussian_blur_batch", src, dst, batch, height, width, ksize, apply, weights,
                    dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const BandPlan P = blur_plan(height, width, ksize);
  return ffcv::launch_tiles("ffcv_gaussian_blur_batch", "gaussian_blur_kernel", gaussian_blur_kernel, stream,
                            (uint64_t)batch * P.nbands * P.nstrips, BLUR_THREADS, P.lds, src, dst, stride, height,
                            width, ksize, apply, weights, P);
}

int ffcv_gaussian_blur_batch_host(const uint8_t *src, uint8_t *dst, int batch, int height, int width, int ksize,
                                  const uint8_t *apply, const float *weights, uint64_t dst_stride_bytes,
                                  int nthreads) {
  uint64_t stride;
  if (!blur_args_ok("ffcv_gaussian_blur_batch_host", src, dst, batch, height, width, ksize, apply, weights,
                    dst_stride_bytes, &stride))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  ffcv::host_images<std::vector<float>>(
      nthreads, batch, src, dst, (uint64_t)height * width * 3, stride,
      [&](uint64_t k, const uint8_t *in, uint8_t *out, std::vector<float> &plane) {
        if (apply[k]) blur_image_host(in, out, height, width, ksize, weights + k * FFCV_BLUR_WROW, plane);
        return apply[k] != 0;
      });
  return FFCV_OK;
}

}  // extern "C"
