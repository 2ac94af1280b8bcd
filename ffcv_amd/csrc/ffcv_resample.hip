// ffcv_resample.hip -- RandomResizedCrop's 'bilinear' and 'bicubic' modes:
// Pillow's antialiased separable resampling (ImagingResample for 8-bit
// images: img.crop(window).resize(size, BILINEAR | BICUBIC)) of a crop window
// of each image of a dense uint8 batch [B][H][W][3].
//
// The filter's support grows with the downscale, so a window of 224 x 224 and
// its intermediate do not fit a workgroup's LDS the way rrc_images_kernel
// keeps a crop.  Here a workgroup owns a BAND of output rows of one image and
// the two passes roll over the window's rows:
//   records    the out_w column records and the band's row records (first
//              sample, count, 22-bit taps: resample_common.h) are built in LDS
//              by the workgroup, one lane per record in float64, while the
//              first chunk's loads are in flight: no taps kernel, no workspace;
//   staging    the window rows the band needs arrive once, a chunk of rows at
//              a time, as the aligned 16-byte words that hold a byte of them;
//              the next chunk's words wait in registers during the passes;
//   horizontal a work item is (staged row, output column): its taps are
//              contiguous bytes of the row, read four taps (three aligned
//              dwords) at a time, three int32 sums, three bytes into a RING of
//              intermediate rows;
//   vertical   a work item is (output row, four adjacent bytes of it): one
//              aligned dword of each of the row's ring rows, four sums; it
//              runs as soon as the ring holds the row's last source row, and
//              its bytes leave as one dword where the address allows.
// The ring holds the longest record plus a chunk, which is all a row that
// has just become ready can still need.
#include "api_internal.h"
#include "device_common.h"
#include "lds_stage.h"
#include "resample_common.h"

FFCV_HD bool resample_crop_ok(int i, int j, int h, int w, int H, int W) {
  return h > 0 && w > 0 && i >= 0 && j >= 0 && (int64_t)i + h <= H && (int64_t)j + w <= W;
}

// byte b of w times k, added to acc: one v_mad_i32_i24 (|k| <= RESAMPLE_KMAX)
FFCV_DEV int tap_mad(uint32_t w, int b, int k, int acc) { return ffcv_mul24((int)((w >> (8 * b)) & 0xffu), k) + acc; }

__global__ void __launch_bounds__(RESAMPLE_THREADS)
    resample_images_kernel(const uint8_t *__restrict__ in, uint64_t in_stride, int H, int W,
                           const int32_t *__restrict__ crops, int mode, int out_h, int out_w,
                           uint8_t *__restrict__ out, uint64_t out_stride, int32_t *__restrict__ status,
                           ResamplePlan P) {
  extern __shared__ uint4 smem[];
  typedef const __attribute__((address_space(1))) lds_x4_t gx4_t;
  const int t = threadIdx.x;
  const uint32_t k = blockIdx.x / (uint32_t)P.bands, band = blockIdx.x - k * (uint32_t)P.bands;
  const int y0 = (int)band * P.band_rows, y1 = min(out_h, y0 + P.band_rows);
  const int orb = 3 * out_w;  // bytes of an output row
  uint8_t *o = out + (uint64_t)k * out_stride;
  const int ci = crops[4 * (size_t)k], cj = crops[4 * (size_t)k + 1], chh = crops[4 * (size_t)k + 2],
            cww = crops[4 * (size_t)k + 3];
  if (!resample_crop_ok(ci, cj, chh, cww, H, W)) {  // (the same for the whole workgroup)
    uint8_t *ob = o + (uint64_t)y0 * orb;
    for (int i = t; i < (y1 - y0) * orb; i += RESAMPLE_THREADS) ob[i] = 0;
    if (status && band == 0 && t == 0) status[k] = FFCV_SAMPLE_RANGE;
    return;
  }
  if (status && band == 0 && t == 0) status[k] = FFCV_SAMPLE_OK;

  const int KX = RESAMPLE_HEAD + P.kx, KY = RESAMPLE_HEAD + P.ky;
  int32_t *s_col = (int32_t *)smem;
  int32_t *s_row = (int32_t *)((uint8_t *)smem + P.off_rows);
  lds_x4_t *s_src = (lds_x4_t *)((uint8_t *)smem + P.off_src);
  uint32_t *s_ring = (uint32_t *)((uint8_t *)smem + P.off_ring);
  const int ring_rows = P.ring_rows, ndw = P.ring_pitch >> 2, CH = P.chunk_rows;

  // window rows [r_lo, r_hi) feed the band (a record's first and end sample never decrease along a pass)
  const ResampleSpan sp0 = resample_span(chh, out_h, mode, y0), sp1 = resample_span(chh, out_h, mode, y1 - 1);
  const int r_lo = sp0.first, r_hi = sp1.first + sp1.count;

  const uint64_t step = (uint64_t)W * 3;
  const uint64_t src0 = (uint64_t)(uintptr_t)in + (uint64_t)k * in_stride + ((uint64_t)ci * W + cj) * 3;
  const int lead0 = (int)(src0 & 15), stepmod = (int)(step & 15);
  const int nch = (int)lds_chunks(3 * cww), pitch = nch * 16;  // nch <= P.src_pitch / 16: cww <= W

  lds_x4_t v[RESAMPLE_CHUNK_LOADS];
  int di[RESAMPLE_CHUNK_LOADS];
  // the aligned words of window rows [cs, cs + nr) into registers (nr * nch <= CHUNK_LOADS * THREADS: the plan)
  auto load = [&](int cs, int nr) {
#pragma unroll
    for (int q = 0; q < RESAMPLE_CHUNK_LOADS; q++) {
      const int idx = t + q * RESAMPLE_THREADS;
      di[q] = -1;
      if (idx < nr * nch) {
        const int r = idx / nch, c = idx - r * nch;
        const uint64_t ra = src0 + (uint64_t)(cs + r) * step;
        // words holding bytes of this row (none past the batch's last byte)
        if (c < (int)(((ra & 15) + 3 * (uint64_t)cww + 15) >> 4)) {
          v[q] = ((gx4_t *)(uintptr_t)(ra & ~(uint64_t)15))[c];
          di[q] = idx;
        }
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int q = 0; q < RESAMPLE_CHUNK_LOADS; q++)
      if (di[q] >= 0) s_src[di[q]] = v[q];
  };

  int c0 = r_lo, rows = min(CH, r_hi - r_lo);
  load(c0, rows);
  for (int i = t; i < out_w + (y1 - y0); i += RESAMPLE_THREADS) {  // the records, under the loads
    if (i < out_w)
      resample_record(cww, out_w, mode, i, P.kx, s_col + i * KX);
    else
      resample_record(chh, out_h, mode, y0 + (i - out_w), P.ky, s_row + (i - out_w) * KY);
  }
  store();
  __syncthreads();

  int ydone = y0;
  for (;;) {
    const int c1 = c0 + rows, next_rows = min(CH, r_hi - c1);
    if (next_rows > 0) load(c1, next_rows);

    // ---- horizontal: staged rows [c0, c1) -> ring rows
    for (int i = t; i < rows * out_w; i += RESAMPLE_THREADS) {
      const int r = i / out_w, xo = i - r * out_w;
      const int32_t *rec = s_col + xo * KX;
      const int first = rec[0], n = rec[1];
      const uint8_t *a = (const uint8_t *)s_src + r * pitch + ((lead0 + (c0 + r) * stepmod) & 15) + 3 * first;
      const uint32_t *q = (const uint32_t *)__builtin_align_down(a, 4);
      const uint32_t sh = (uint32_t)(a - (const uint8_t *)q);
      uint32_t w0 = q[0];
      int a0 = 1 << (RESAMPLE_BITS - 1), a1 = a0, a2 = a0;
      // four taps are twelve bytes; the taps behind n are zero and meet whatever bytes follow
      for (int x = 0; x < n; x += 4) {
        const int4 kk = *(const int4 *)(rec + RESAMPLE_HEAD + x);
        const uint32_t w1 = q[1], w2 = q[2], w3 = q[3];
        const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                       d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
        w0 = w3;
        q += 3;
        a0 = tap_mad(d0, 0, kk.x, a0);
        a1 = tap_mad(d0, 1, kk.x, a1);
        a2 = tap_mad(d0, 2, kk.x, a2);
        a0 = tap_mad(d0, 3, kk.y, a0);
        a1 = tap_mad(d1, 0, kk.y, a1);
        a2 = tap_mad(d1, 1, kk.y, a2);
        a0 = tap_mad(d1, 2, kk.z, a0);
        a1 = tap_mad(d1, 3, kk.z, a1);
        a2 = tap_mad(d2, 0, kk.z, a2);
        a0 = tap_mad(d2, 1, kk.w, a0);
        a1 = tap_mad(d2, 2, kk.w, a1);
        a2 = tap_mad(d2, 3, kk.w, a2);
      }
      uint8_t *dst = (uint8_t *)(s_ring + ((uint32_t)(c0 + r) % (uint32_t)ring_rows) * ndw) + 3 * xo;
      dst[0] = (uint8_t)resample_clip8(a0);
      dst[1] = (uint8_t)resample_clip8(a1);
      dst[2] = (uint8_t)resample_clip8(a2);
    }
    __syncthreads();

    // ---- vertical: the output rows whose last source row is now in the ring
    int yr = ydone;
    while (yr < y1) {
      const int32_t *rr = s_row + (yr - y0) * KY;
      if (rr[0] + rr[1] > c1) break;
      yr++;
    }
    for (int i = t; i < (yr - ydone) * ndw; i += RESAMPLE_THREADS) {
      const int yy = i / ndw, d = i - yy * ndw, y = ydone + yy;
      const int32_t *rec = s_row + (y - y0) * KY;
      const int n = rec[1];
      int j = (int)((uint32_t)rec[0] % (uint32_t)ring_rows);
      int a0 = 1 << (RESAMPLE_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int x = 0; x < n; x++) {
        const int kk = rec[RESAMPLE_HEAD + x];
        const uint32_t w = s_ring[j * ndw + d];
        a0 = tap_mad(w, 0, kk, a0);
        a1 = tap_mad(w, 1, kk, a1);
        a2 = tap_mad(w, 2, kk, a2);
        a3 = tap_mad(w, 3, kk, a3);
        j = j + 1 == ring_rows ? 0 : j + 1;
      }
      const uint32_t b0 = (uint32_t)resample_clip8(a0), b1 = (uint32_t)resample_clip8(a1),
                     b2 = (uint32_t)resample_clip8(a2), b3 = (uint32_t)resample_clip8(a3);
      const uint32_t packed = b0 | b1 << 8 | b2 << 16 | b3 << 24;
      uint8_t *g = o + (uint64_t)y * orb + 4 * d;
      const int valid = min(4, orb - 4 * d);  // the row's last dword may hold fewer than four bytes
      if (valid == 4 && ((uintptr_t)g & 3) == 0) {
        *(uint32_t *)g = packed;
      } else {
        for (int b = 0; b < valid; b++) g[b] = (uint8_t)(packed >> (8 * b));
      }
    }
    ydone = yr;
    if (next_rows <= 0) break;
    store();
    __syncthreads();
    c0 = c1;
    rows = next_rows;
  }
}

namespace {

// one image on the host: the same records, a uint8 intermediate of h x out_w pixels
struct HostScratch {
  std::vector<int32_t> col, row;
  std::vector<uint8_t> mid;
};

void resample_one_host(const uint8_t *img, int W, const int32_t *c, int mode, int out_h, int out_w, uint8_t *dst,
                       HostScratch &s) {
  const int ci = c[0], cj = c[1], chh = c[2], cww = c[3];
  const int kx = resample_taps_cap(cww, out_w, mode), ky = resample_taps_cap(chh, out_h, mode);
  const int KX = RESAMPLE_HEAD + kx, KY = RESAMPLE_HEAD + ky;
  s.col.resize((size_t)out_w * KX);
  s.row.resize((size_t)out_h * KY);
  s.mid.resize((size_t)chh * out_w * 3);
  for (int x = 0; x < out_w; x++) resample_record(cww, out_w, mode, x, kx, s.col.data() + (size_t)x * KX);
  for (int y = 0; y < out_h; y++) resample_record(chh, out_h, mode, y, ky, s.row.data() + (size_t)y * KY);
  for (int r = 0; r < chh; r++) {
    const uint8_t *src = img + ((uint64_t)(ci + r) * W + cj) * 3;
    uint8_t *m = s.mid.data() + (size_t)r * out_w * 3;
    for (int x = 0; x < out_w; x++) {
      const int32_t *rec = s.col.data() + (size_t)x * KX;
      for (int ch = 0; ch < 3; ch++) {
        int32_t acc = 1 << (RESAMPLE_BITS - 1);
        for (int i = 0; i < rec[1]; i++) acc += (int32_t)src[3 * (rec[0] + i) + ch] * rec[RESAMPLE_HEAD + i];
        m[3 * x + ch] = (uint8_t)resample_clip8(acc);
      }
    }
  }
  const size_t orb = (size_t)out_w * 3;
  for (int y = 0; y < out_h; y++) {
    const int32_t *rec = s.row.data() + (size_t)y * KY;
    for (size_t e = 0; e < orb; e++) {
      int32_t acc = 1 << (RESAMPLE_BITS - 1);
      for (int i = 0; i < rec[1]; i++) acc += (int32_t)s.mid[(size_t)(rec[0] + i) * orb + e] * rec[RESAMPLE_HEAD + i];
      dst[(size_t)y * orb + e] = (uint8_t)resample_clip8(acc);
    }
  }
}

// the guards both entries share; *stride: the resolved out_stride
bool resample_args_ok(const char *who, const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                      const int32_t *crops, int mode, int out_h, int out_w, const uint8_t *out, uint64_t out_stride,
                      uint64_t *stride) {
  if (!in || !crops || !out || batch < 0 || height <= 0 || width <= 0 || height > 65535 || width > 65535 ||
      out_h <= 0 || out_w <= 0 || out_h > 65535 || out_w > 65535) {
    ffcv::set_error("%s: invalid arguments", who);
    return false;
  }
  if (mode != FFCV_RESAMPLE_BILINEAR && mode != FFCV_RESAMPLE_BICUBIC) {
    ffcv::set_error("%s: mode %d (FFCV_RESAMPLE_BILINEAR or FFCV_RESAMPLE_BICUBIC)", who, mode);
    return false;
  }
  const uint64_t img = (uint64_t)height * width * 3, dense = (uint64_t)out_h * out_w * 3;
  *stride = out_stride ? out_stride : dense;
  if (in_stride < img || *stride < dense) {
    ffcv::set_error("%s: in_stride %llu / out_stride %llu for images of %llu / %llu bytes", who,
                    (unsigned long long)in_stride, (unsigned long long)*stride, (unsigned long long)img,
                    (unsigned long long)dense);
    return false;
  }
  if (batch > 0) {  // the two ranges must not overlap
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uint64_t)(batch - 1) * in_stride + img;
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uint64_t)(batch - 1) * *stride + dense;
    if (a0 < b1 && b0 < a1) {
      ffcv::set_error("%s: in and out overlap", who);
      return false;
    }
  }
  return true;
}

int resample_launch(const char *who, void *stream, const uint8_t *in, uint64_t in_stride, int batch, int height,
                    int width, const int32_t *crops, int mode, int out_h, int out_w, uint8_t *out,
                    uint64_t out_stride, int32_t *status, int band_rows, int chunk_rows) {
  uint64_t stride;
  if (!resample_args_ok(who, in, in_stride, batch, height, width, crops, mode, out_h, out_w, out, out_stride,
                        &stride))
    return FFCV_EINVAL;
  ResamplePlan P;
  if (!resample_plan(height, width, out_h, out_w, mode, band_rows, chunk_rows, &P)) {
    ffcv::set_error("%s: %dx%d -> %dx%d does not fit the %d bytes of LDS a workgroup may use (ffcv_resample_fits)",
                    who, height, width, out_h, out_w, RESAMPLE_LDS_MAX);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  return ffcv::launch_tiles(who, "resample_images_kernel", resample_images_kernel, stream,
                            (uint64_t)batch * (uint64_t)P.bands, RESAMPLE_THREADS, P.lds, in, in_stride, height,
                            width, crops, mode, out_h, out_w, out, stride, status, P);
}

}  // namespace

extern "C" {

int ffcv_resample_fits(int height, int width, int out_h, int out_w, int mode) {
  ResamplePlan P;
  return resample_plan(height, width, out_h, out_w, mode, 0, 0, &P) ? 1 : 0;
}

int ffcv_resample_images_batch(const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                               const int32_t *crops, int mode, int out_h, int out_w, uint8_t *out,
                               uint64_t out_stride, int32_t *status, void *stream) {
  return resample_launch("ffcv_resample_images_batch", stream, in, in_stride, batch, height, width, crops, mode,
                         out_h, out_w, out, out_stride, status, 0, 0);
}

// Measurement hook (not in ffcv_hip.h): the launch with a given number of
// output rows per band and source rows per chunk (0: the default of each).
int ffcv_resample_images_batch_plan(const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                                    const int32_t *crops, int mode, int out_h, int out_w, uint8_t *out,
                                    uint64_t out_stride, int32_t *status, void *stream, int band_rows,
                                    int chunk_rows) {
  if (band_rows < 0 || chunk_rows < 0) {
    ffcv::set_error("ffcv_resample_images_batch_plan: band_rows %d, chunk_rows %d", band_rows, chunk_rows);
    return FFCV_EINVAL;
  }
  return resample_launch("ffcv_resample_images_batch_plan", stream, in, in_stride, batch, height, width, crops, mode,
                         out_h, out_w, out, out_stride, status, band_rows, chunk_rows);
}

int ffcv_resample_images_batch_host(const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                                    const int32_t *crops, int mode, int out_h, int out_w, uint8_t *out,
                                    uint64_t out_stride, int32_t *status, int nthreads) {
  const char *who = "ffcv_resample_images_batch_host";
  uint64_t stride;
  if (!resample_args_ok(who, in, in_stride, batch, height, width, crops, mode, out_h, out_w, out, out_stride,
                        &stride))
    return FFCV_EINVAL;
  if (!ffcv_resample_fits(height, width, out_h, out_w, mode)) {  // the twin serves what the device serves
    ffcv::set_error("%s: %dx%d -> %dx%d is outside ffcv_resample_fits", who, height, width, out_h, out_w);
    return FFCV_EINVAL;
  }
  const uint64_t dense = (uint64_t)out_h * out_w * 3;
  ffcv::host_threads(nthreads, batch, [&](std::atomic<uint64_t> &next, int, int) {
    HostScratch s;
    for (uint64_t k = next.fetch_add(1); k < (uint64_t)batch; k = next.fetch_add(1)) {
      const int32_t *c = crops + 4 * (size_t)k;
      uint8_t *dst = out + k * stride;
      if (!resample_crop_ok(c[0], c[1], c[2], c[3], height, width)) {
        std::fill(dst, dst + dense, (uint8_t)0);
        if (status) status[k] = FFCV_SAMPLE_RANGE;
        continue;
      }
      resample_one_host(in + k * in_stride, width, c, mode, out_h, out_w, dst, s);
      if (status) status[k] = FFCV_SAMPLE_OK;
    }
  });
  return FFCV_OK;
}

}  // extern "C"
