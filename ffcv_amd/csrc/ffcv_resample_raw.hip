// ffcv_resample_raw.hip -- the raw samples of a crop decoder's batch in the
// 'bilinear' / 'bicubic' modes: Pillow's antialiased
// img.crop(window).resize(size, filter) of each raw sample's stored bytes,
// whatever its size, in one launch.  The band kernel of resample_passes.h with
// ffcv_resample.hip's row loader: every image's address, height and width come
// from its ffcv_sample, a workgroup owns a band of output rows of one image,
// and the window's rows arrive a chunk at a time as the aligned 16-byte words
// that hold a byte of them, the next chunk's words waiting in registers during
// the passes.  Samples of the other mode are skipped (ffcv_jpeg_resample_batch
// serves them), as the area kernels do.
#include "api_internal.h"
#include "device_common.h"
#include "lds_stage.h"
#include "resample_passes.h"

__global__ void __launch_bounds__(RESAMPLE_THREADS)
    resample_raw_kernel(const uint8_t *__restrict__ base, const ffcv_sample *__restrict__ samples,
                        const int32_t *__restrict__ crops, int mode, int out_h, int out_w, uint8_t *__restrict__ out,
                        uint64_t out_stride, int max_h, int max_w, BandResamplePlan P) {
  extern __shared__ uint4 smem[];
  typedef const __attribute__((address_space(1))) lds_x4_t gx4_t;
  const int t = threadIdx.x;
  const uint32_t k = blockIdx.x / (uint32_t)P.bands, band = blockIdx.x - k * (uint32_t)P.bands;
  const ffcv_sample s = samples[k];
  if (s.mode != 1) return;  // (the same for the whole workgroup)
  const int y0 = (int)band * P.band_rows, y1 = min(out_h, y0 + P.band_rows);
  const int orb = 3 * out_w;  // bytes of an output row
  uint8_t *o = out + (uint64_t)k * out_stride;
  const int H = (int)s.height, W = (int)s.width;
  const int ci = crops[4 * (size_t)k], cj = crops[4 * (size_t)k + 1], chh = crops[4 * (size_t)k + 2],
            cww = crops[4 * (size_t)k + 3];
  // (the plan's LDS is sized for max_h x max_w: a larger sample yields zeros)
  if ((uint32_t)s.height > (uint32_t)max_h || (uint32_t)s.width > (uint32_t)max_w ||
      !resample_window_ok(ci, cj, chh, cww, H, W)) {
    resample_zero_band(t, o, y0, y1, orb);
    return;
  }

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
  const uint64_t src0 = (uint64_t)(uintptr_t)base + s.offset + ((uint64_t)ci * W + cj) * 3;
  const int lead0 = (int)(src0 & 15), stepmod = (int)(step & 15);
  const int nch = (int)lds_chunks(3 * cww), pitch = nch * 16;  // nch <= P.src_pitch / 16: cww <= max_w

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
        // words holding bytes of this row (none past the sample's last byte)
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
  resample_band_records(t, cww, chh, out_w, out_h, mode, y0, y1, P.kx, P.ky, s_col, s_row);  // under the loads
  store();
  __syncthreads();

  int ydone = y0;
  for (;;) {
    const int c1 = c0 + rows, next_rows = min(CH, r_hi - c1);
    if (next_rows > 0) load(c1, next_rows);
    resample_h_pass(
        t, rows, c0, out_w, s_col, KX,
        [&](int r) { return (const uint8_t *)s_src + r * pitch + ((lead0 + (c0 + r) * stepmod) & 15); }, s_ring,
        ring_rows, ndw);
    __syncthreads();
    ydone = resample_v_pass(t, ydone, y0, y1, c1, s_row, KY, s_ring, ring_rows, ndw, o, orb);
    if (next_rows <= 0) break;
    store();
    __syncthreads();
    c0 = c1;
    rows = next_rows;
  }
}

extern "C" {

int ffcv_resample_raw_batch(const uint8_t *base, const ffcv_sample *samples, int batch, const int32_t *crops, int mode,
                            int out_h, int out_w, uint8_t *out, uint64_t out_stride, int max_h, int max_w,
                            void *stream) {
  const char *who = "ffcv_resample_raw_batch";
  if (!base || !samples || !crops || !out || batch < 0 || out_h <= 0 || out_w <= 0 || max_h <= 0 || max_w <= 0) {
    ffcv::set_error("%s: invalid arguments", who);
    return FFCV_EINVAL;
  }
  if (mode != FFCV_RESAMPLE_BILINEAR && mode != FFCV_RESAMPLE_BICUBIC) {
    ffcv::set_error("%s: mode %d (FFCV_RESAMPLE_BILINEAR or FFCV_RESAMPLE_BICUBIC)", who, mode);
    return FFCV_EINVAL;
  }
  const uint64_t dense = (uint64_t)out_h * out_w * 3, stride = out_stride ? out_stride : dense;
  if (stride < dense) {
    ffcv::set_error("%s: out_stride %llu for images of %llu bytes", who, (unsigned long long)stride,
                    (unsigned long long)dense);
    return FFCV_EINVAL;
  }
  BandResamplePlan P;
  if (!band_resample_plan(max_h, max_w, out_h, out_w, mode, 0, 0, &P)) {
    ffcv::set_error("%s: images of up to %dx%d -> %dx%d do not fit the %d bytes of LDS a workgroup may use "
                    "(ffcv_jpeg_resample_fits)", who, max_h, max_w, out_h, out_w, RESAMPLE_LDS_MAX);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  // (the plane tiles behind the ring are the JPEG kernel's: not allocated here)
  return ffcv::launch_tiles(who, "resample_raw_kernel", resample_raw_kernel, stream, (uint64_t)batch * (uint64_t)P.bands,
                            RESAMPLE_THREADS, P.off_tiles, base, samples, crops, mode, out_h, out_w, out, stride, max_h,
                            max_w, P);
}

}  // extern "C"
