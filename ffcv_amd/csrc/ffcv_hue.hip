// ffcv_hue.hip -- RandomHue and the jointly gated RandomColorJitter
// (DESIGN.md s20): their draws, and the hue shift of a uint8 HWC batch in one
// launch, with the host twins.
//
// The hue kernel needs neither the image's mean nor a table, so it is a kernel
// of its own beside color_jitter_kernel and shares only its staging scheme
// (PixelRun, lds_stage.h): a 256-thread workgroup takes one image's contiguous
// run of whole pixels (the whole image up to HUE_LDS_BYTES, else a tile of
// HUE_TILE_PX pixels), stages it in LDS, turns every pixel there (hue_pixel,
// hue_common.h) and writes the bytes back once.
// An image whose decision is 0 is neither read nor written.
//
// LDS budget: 16 KiB of pixels + 32 B staging slack, so eight workgroups (all
// 32 waves of a CU) fit the 160 KiB of a CU and LDS never limits occupancy.
#include "api_internal.h"
#include "hue_common.h"
#include "lds_stage.h"

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
// HUE_LDS_BYTES), ntiles workgroups per image.  Staging: lds_stage.h.
__global__ void __launch_bounds__(HUE_THREADS)
    hue_kernel(uint8_t *__restrict__ images, uint64_t img, const uint8_t *__restrict__ apply,
               const double *__restrict__ shift, uint32_t tile_px, uint32_t ntiles) {
  __shared__ lds_x4_t s_img[HUE_LDS_BYTES / 16 + 2];
  const int t = threadIdx.x;
  const uint32_t k = blockIdx.x / ntiles, tile = blockIdx.x - k * ntiles;
  if (!apply[k]) return;  // the same for the whole workgroup: the image is neither read nor written
  const float D = hue_shift6(shift[k]);

  const PixelRun<HUE_THREADS> run(images, img, k, tile, tile_px, s_img);
  run.stage(t);
  __syncthreads();
  // a thread writes the three bytes of its own pixels only
  for (uint32_t q = t; q < run.npix(); q += HUE_THREADS) {
    uint8_t *a = run.bytes() + 3u * q;
    const uint32_t v = lds_pixel(a);
    const uint32_t o = hue_pixel(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu, D);
    a[0] = (uint8_t)o;
    a[1] = (uint8_t)(o >> 8);
    a[2] = (uint8_t)(o >> 16);
  }
  __syncthreads();
  run.write_back(t);
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

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_hue_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                        double p, double magnitude, uint8_t *apply, double *shift, int32_t *status) {
  if (hue_check_draw("ffcv_hue_draw_batch", sample_ids, batch, p, magnitude, apply, shift)) return FFCV_EINVAL;
  return ffcv::launch_draw("hue_draw_kernel", hue_draw_kernel, stream, batch, sample_ids, batch, loader_seed, epoch, p,
                           magnitude, apply, shift, status);
}

int ffcv_hue_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, double p,
                             double magnitude, uint8_t *apply, double *shift) {
  if (hue_check_draw("ffcv_hue_draw_batch_host", sample_ids, batch, p, magnitude, apply, shift)) return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_hue_draw_batch_host", batch, [&](int k) {
    return draw_hue(k, sample_ids[k], loader_seed, epoch, p, magnitude, apply, shift);
  });
}

int ffcv_color_jitter_joint_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                       uint64_t epoch, double p, const double *magnitude, uint8_t *apply,
                                       double *ratio, int32_t *status) {
  JointDraw jd;
  if (joint_check_draw("ffcv_color_jitter_joint_draw_batch", sample_ids, batch, p, magnitude, apply, ratio, &jd))
    return FFCV_EINVAL;
  return ffcv::launch_draw("color_jitter_joint_draw_kernel", color_jitter_joint_draw_kernel, stream, batch, sample_ids,
                           batch, loader_seed, epoch, p, jd, apply, ratio, status);
}

int ffcv_color_jitter_joint_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                            uint64_t epoch, double p, const double *magnitude, uint8_t *apply,
                                            double *ratio) {
  JointDraw jd;
  if (joint_check_draw("ffcv_color_jitter_joint_draw_batch_host", sample_ids, batch, p, magnitude, apply, ratio, &jd))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_color_jitter_joint_draw_batch_host", batch, [&](int k) {
    return draw_color_jitter_joint(k, batch, sample_ids[k], loader_seed, epoch, p, jd, apply, ratio);
  });
}

int ffcv_hue_batch(void *stream, uint8_t *images, int batch, int height, int width, const uint8_t *apply,
                   const double *shift) {
  if (!ffcv::u8_images_ok("ffcv_hue_batch", images && apply && shift, batch, height, width)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const uint64_t npx = (uint64_t)height * width;
  uint32_t tile_px, ntiles;
  unsigned blocks;
  if (!ffcv::run_tiling("ffcv_hue_batch", batch, npx, HUE_LDS_BYTES, HUE_TILE_PX, &tile_px, &ntiles, &blocks))
    return FFCV_EINVAL;
  hipLaunchKernelGGL(hue_kernel, dim3(blocks), dim3(HUE_THREADS), 0, ffcv::as_stream(stream), images, npx * 3, apply,
                     shift, tile_px, ntiles);
  FFCV_LAUNCH_CHECK("hue_kernel");
  return FFCV_OK;
}

int ffcv_hue_batch_host(uint8_t *images, int batch, int height, int width, const uint8_t *apply,
                        const double *shift) {
  if (!ffcv::u8_images_ok("ffcv_hue_batch_host", images && apply && shift, batch, height, width)) return FFCV_EINVAL;
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
