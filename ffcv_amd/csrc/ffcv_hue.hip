// ffcv_hue.hip -- RandomHue and the jointly gated RandomColorJitter
// (DESIGN.md s20): their draws, and the hue shift of a uint8 HWC batch in one
// launch, with the host twins.
//
// The hue kernel needs neither the image's mean nor a table, so it is a kernel
// of its own beside color_jitter_kernel and borrows only its staging scheme: a
// 256-thread workgroup takes one image's contiguous run of whole pixels (the
// whole image up to HUE_LDS_BYTES, else a tile of HUE_TILE_PX pixels), stages
// it in LDS with 16-byte aligned loads whatever the run's byte offset, turns
// every pixel there (hue_pixel, hue_common.h) and writes the bytes back once.
// An image whose decision is 0 is neither read nor written.
//
// LDS budget: 16 KiB of pixels + 32 B staging slack, so eight workgroups (all
// 32 waves of a CU) fit the 160 KiB of a CU and LDS never limits occupancy.
#include "api_internal.h"
#include "hue_common.h"

#define HUE_THREADS 256
#define HUE_LDS_BYTES 16384
#define HUE_TILE_PX 4096  // 12 KiB of pixels per workgroup beyond the whole-image regime

__global__ void __launch_bounds__(64) hue_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed,
                                                      uint64_t epoch, double p, double magnitude,
                                                      uint8_t *__restrict__ apply, double *__restrict__ shift,
                                                      int32_t *__restrict__ status) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_hue(k, ids[k], loader_seed, epoch, p, magnitude, apply, shift);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

__global__ void __launch_bounds__(64)
    color_jitter_joint_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed, uint64_t epoch,
                                   double p, JointDraw jd, uint8_t *__restrict__ apply, double *__restrict__ ratio,
                                   int32_t *__restrict__ status) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_color_jitter_joint(k, B, ids[k], loader_seed, epoch, p, jd, apply, ratio);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// img: bytes of one image; tile_px pixels per workgroup (tile_px * 3 <=
// HUE_LDS_BYTES), ntiles workgroups per image.
__global__ void __launch_bounds__(HUE_THREADS)
    hue_kernel(uint8_t *__restrict__ images, uint64_t img, const uint8_t *__restrict__ apply,
               const double *__restrict__ shift, uint32_t tile_px, uint32_t ntiles) {
  typedef uint32_t hx4_t __attribute__((ext_vector_type(4)));
  __shared__ hx4_t s_img[HUE_LDS_BYTES / 16 + 2];  // + the range's lead bytes and the pixel read-ahead
  const int t = threadIdx.x;
  const uint32_t k = blockIdx.x / ntiles, tile = blockIdx.x - k * ntiles;
  if (!apply[k]) return;  // the same for the whole workgroup: the image is neither read nor written
  const float D = hue_shift6(shift[k]);

  // ---- stage pixels [tile * tile_px, ...) of image k: one contiguous byte
  // range, copied with 16-byte aligned loads whatever its byte offset (an
  // aligned chunk holding a byte of the range never crosses a page)
  const uint64_t b0 = (uint64_t)tile * tile_px * 3u;
  const uint32_t nbytes = (uint32_t)(img - b0 < (uint64_t)tile_px * 3u ? img - b0 : (uint64_t)tile_px * 3u);
  const uint32_t npix = nbytes / 3u;
  uint8_t *src = images + (uint64_t)k * img + b0;
  const uint32_t lead = (uint32_t)((uintptr_t)src & 15);
  typedef __attribute__((address_space(1))) hx4_t gx4_t;
  gx4_t *gp = (gx4_t *)((uintptr_t)src & ~(uintptr_t)15);
  const int nch = (int)((lead + nbytes + 15) >> 4);  // <= HUE_LDS_BYTES / 16 + 1
  for (int i = t; i < nch; i += HUE_THREADS) s_img[i] = gp[i];
  __syncthreads();
  uint8_t *s_bytes = (uint8_t *)s_img + lead;  // byte 0 of the staged pixels

  // pixel q's R | G << 8 | B << 16 from two ALIGNED 4-byte LDS reads joined by
  // v_alignbyte; reads up to 7 bytes past the pixel's first, inside s_img.  A
  // thread writes the three bytes of its own pixels only.
  for (uint32_t q = t; q < npix; q += HUE_THREADS) {
    uint8_t *a = s_bytes + 3u * q;
    const uint32_t *qa = (const uint32_t *)__builtin_align_down(a, 4);
    const uint32_t v = __builtin_amdgcn_alignbyte(qa[1], qa[0], (uint32_t)(a - (const uint8_t *)qa));
    const uint32_t o = hue_pixel(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu, D);
    a[0] = (uint8_t)o;
    a[1] = (uint8_t)(o >> 8);
    a[2] = (uint8_t)(o >> 16);
  }
  __syncthreads();

  // ---- write back: whole 16-byte chunks inside the range as one store, the
  // two cut by its ends byte by byte (their other bytes belong to a neighbour)
  for (int i = t; i < nch; i += HUE_THREADS) {
    const uint32_t c0 = 16u * (uint32_t)i;
    if (c0 >= lead && c0 + 16u <= lead + nbytes) {
      gp[i] = s_img[i];
    } else {
      const uint8_t *sb = (const uint8_t *)s_img;
      uint8_t *gb = (uint8_t *)((uintptr_t)src & ~(uintptr_t)15);
      for (uint32_t j = c0; j < c0 + 16u; j++)
        if (j >= lead && j < lead + nbytes) gb[j] = sb[j];
    }
  }
}

static int hue_check_draw(const char *who, const void *ids, int batch, double p, double magnitude, const void *apply,
                          const void *shift) {
  if (batch < 0 || !ids || !apply || !shift || !(p >= 0.0 && p <= 1.0) || !(magnitude >= 0.0 && magnitude <= 0.5)) {
    ffcv::set_error("%s: invalid arguments (batch %d, p %g, magnitude %g in [0, 0.5])", who, batch, p, magnitude);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

// The ranges and the compacted rows of the joint draw: b, c, s follow
// color_jitter.py:41 (uniform(max(0, 1 - m), 1 + m)), hue is uniform(-m, m).
static int joint_check_draw(const char *who, const void *ids, int batch, double p, const double *magnitude,
                            const void *apply, const void *ratio, JointDraw *jd) {
  if (batch < 0 || !ids || !magnitude || !apply || !ratio || !(p >= 0.0 && p <= 1.0)) {
    ffcv::set_error("%s: invalid arguments (batch %d, p %g)", who, batch, p);
    return FFCV_EINVAL;
  }
  int rows = 0;
  for (int j = 0; j < 4; j++) {
    const double m = magnitude[j];
    if (!(m >= 0.0) || m > (j == 3 ? 0.5 : 1.7e308)) {
      ffcv::set_error("%s: magnitude[%d] = %g must be finite and %s", who, j, m, j == 3 ? "in [0, 0.5]" : ">= 0");
      return FFCV_EINVAL;
    }
    if (j == 3) {
      jd->lo[j] = -m;
      jd->hi[j] = m;
    } else {
      const double l = 1.0 - m;
      jd->lo[j] = l < 0.0 ? 0.0 : l;
      jd->hi[j] = 1.0 + m;
    }
    jd->row[j] = m != 0.0 ? rows++ : -1;
  }
  return FFCV_OK;
}

static int hue_check_batch(const char *who, const void *images, int batch, int height, int width, const void *apply,
                           const void *shift) {
  if (batch < 0 || !images || !apply || !shift || height <= 0 || width <= 0 ||
      (uint64_t)height * (uint64_t)width * 3 > 0x7fffffffull) {
    ffcv::set_error("%s: invalid arguments (batch %d, %dx%d)", who, batch, height, width);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_hue_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                        double p, double magnitude, uint8_t *apply, double *shift, int32_t *status) {
  if (hue_check_draw("ffcv_hue_draw_batch", sample_ids, batch, p, magnitude, apply, shift)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  hipLaunchKernelGGL(hue_draw_kernel, dim3((batch + 63) / 64), dim3(64), 0, ffcv::as_stream(stream), sample_ids,
                     batch, loader_seed, epoch, p, magnitude, apply, shift, status);
  FFCV_LAUNCH_CHECK("hue_draw_kernel");
  return FFCV_OK;
}

int ffcv_hue_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, double p,
                             double magnitude, uint8_t *apply, double *shift) {
  if (hue_check_draw("ffcv_hue_draw_batch_host", sample_ids, batch, p, magnitude, apply, shift)) return FFCV_EINVAL;
  int err = 0;
  for (int k = 0; k < batch; k++) err |= draw_hue(k, sample_ids[k], loader_seed, epoch, p, magnitude, apply, shift);
  if (err) {
    ffcv::set_error("ffcv_hue_draw_batch_host: MT19937 stream exhausted");
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

int ffcv_color_jitter_joint_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                       uint64_t epoch, double p, const double *magnitude, uint8_t *apply,
                                       double *ratio, int32_t *status) {
  JointDraw jd;
  if (joint_check_draw("ffcv_color_jitter_joint_draw_batch", sample_ids, batch, p, magnitude, apply, ratio, &jd))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  hipLaunchKernelGGL(color_jitter_joint_draw_kernel, dim3((batch + 63) / 64), dim3(64), 0, ffcv::as_stream(stream),
                     sample_ids, batch, loader_seed, epoch, p, jd, apply, ratio, status);
  FFCV_LAUNCH_CHECK("color_jitter_joint_draw_kernel");
  return FFCV_OK;
}

int ffcv_color_jitter_joint_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                            uint64_t epoch, double p, const double *magnitude, uint8_t *apply,
                                            double *ratio) {
  JointDraw jd;
  if (joint_check_draw("ffcv_color_jitter_joint_draw_batch_host", sample_ids, batch, p, magnitude, apply, ratio, &jd))
    return FFCV_EINVAL;
  int err = 0;
  for (int k = 0; k < batch; k++)
    err |= draw_color_jitter_joint(k, batch, sample_ids[k], loader_seed, epoch, p, jd, apply, ratio);
  if (err) {
    ffcv::set_error("ffcv_color_jitter_joint_draw_batch_host: MT19937 stream exhausted");
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

int ffcv_hue_batch(void *stream, uint8_t *images, int batch, int height, int width, const uint8_t *apply,
                   const double *shift) {
  if (hue_check_batch("ffcv_hue_batch", images, batch, height, width, apply, shift)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const uint64_t npx = (uint64_t)height * width, img = npx * 3;
  const uint32_t tile_px = img <= HUE_LDS_BYTES ? (uint32_t)npx : HUE_TILE_PX;
  const uint64_t ntiles = (npx + tile_px - 1) / tile_px;
  const uint64_t blocks = (uint64_t)batch * ntiles;
  if (blocks > 0x7fffffffull) {
    ffcv::set_error("ffcv_hue_batch: %llu workgroups exceed one launch", (unsigned long long)blocks);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL(hue_kernel, dim3((unsigned)blocks), dim3(HUE_THREADS), 0, ffcv::as_stream(stream), images, img,
                     apply, shift, tile_px, (uint32_t)ntiles);
  FFCV_LAUNCH_CHECK("hue_kernel");
  return FFCV_OK;
}

int ffcv_hue_batch_host(uint8_t *images, int batch, int height, int width, const uint8_t *apply,
                        const double *shift) {
  if (hue_check_batch("ffcv_hue_batch_host", images, batch, height, width, apply, shift)) return FFCV_EINVAL;
  const uint64_t npx = (uint64_t)height * width;
  for (int k = 0; k < batch; k++) {
    if (!apply[k]) continue;
    const float D = hue_shift6(shift[k]);
    uint8_t *im = images + (uint64_t)k * npx * 3;
    for (uint64_t q = 0; q < npx; q++) {
      uint8_t *o = im + 3 * q;
      const uint32_t v = hue_pixel(o[0], o[1], o[2], D);
      o[0] = (uint8_t)v;
      o[1] = (uint8_t)(v >> 8);
      o[2] = (uint8_t)(v >> 16);
    }
  }
  return FFCV_OK;
}

}  // extern "C"
