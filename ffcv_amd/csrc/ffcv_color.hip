// ffcv_color.hip -- RandomBrightness / RandomContrast / RandomSaturation
// (color_jitter.py) as one-launch device colour jitter, with the host twin;
// RandomGrayscale and RandomSolarization are two more steps
// of the same launch.  The uniform draw (ffcv_uniform_draw_batch: grayscale,
// solarization, blur's gate) is the colour steps' draw and lives here too.
//
// One kernel serves both regimes.  A workgroup stages a run of whole pixels
// of one image in LDS (the whole image when it fits CJ_LDS_BYTES, else a tile
// of CJ_TILE_PX pixels), runs the program's steps on it there, each step on
// the previous step's uint8 result, and writes the bytes back once.
//
//   whole image (mode CJ_WHOLE): contrast's gray sum is reduced inside the
//     workgroup (integer: wave shuffle, then an LDS combine), so any program
//     is one launch with one HBM read and one HBM write per image.
//   tiles: a program without contrast is one pointwise launch (CJ_POINT).  A
//     program with contrast is two: pass A (CJ_SUM) runs the steps before
//     contrast, and adds the tile's gray sum of what it wrote to the image's
//     uint64 in the workspace (one integer atomic per workgroup: order does
//     not matter, the result is deterministic); pass B (CJ_POINT) builds the
//     contrast table from that sum and runs contrast and the steps after it.
//
// LDS budget: 16 KiB of pixels + 32 B staging slack + a 256 B table: under
// 20 KiB, so eight 256-thread workgroups (all 32 waves of a CU) fit the
// 160 KiB of a CU and LDS never limits occupancy.  A 32x32 image is 3 KiB.
#include <cmath>

#include "api_internal.h"
#include "color_common.h"
#include "lds_stage.h"

#define CJ_THREADS 256
#define CJ_LDS_BYTES 16384
#define CJ_TILE_PX 4096  // 12 KiB of pixels per workgroup beyond the whole-image regime
enum { CJ_WHOLE = 0, CJ_SUM = 1, CJ_POINT = 2 };

// apply[k] with probability p and value[k] uniform in [lo, hi): the draw of the
// colour jitter steps (op ids 5-7) and of ffcv_uniform_draw_batch (9-11)
__global__ void __launch_bounds__(64) uniform_draw_kernel(const uint64_t *__restrict__ ids, int B,
                                                          uint64_t loader_seed, uint64_t epoch, uint32_t op_id,
                                                          double p, double lo, double hi,
                                                          uint8_t *__restrict__ apply, double *__restrict__ value,
                                                          int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_color_jitter(k, ids[k], loader_seed, epoch, op_id, p, lo, hi, apply, value);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// prog: steps[i] in byte i.  Steps [s0, s1) run; in mode CJ_SUM the gray sum
// of the result is then added to ws[k] when step s1 (contrast) applies.
// img / npx: bytes / pixels of one image; tile_px pixels per workgroup
// (tile_px * 3 <= CJ_LDS_BYTES), ntiles workgroups per image.
__global__ void __launch_bounds__(CJ_THREADS)
    color_jitter_kernel(uint8_t *__restrict__ images, int B, uint64_t img, uint64_t npx, uint32_t prog, int s0, int s1,
                        const uint8_t *__restrict__ apply, const double *__restrict__ ratio,
                        unsigned long long *__restrict__ ws, int mode, uint32_t tile_px, uint32_t ntiles) {
  __shared__ lds_x4_t s_img[CJ_LDS_BYTES / 16 + 2];
  __shared__ uint8_t s_tab[256];
  __shared__ uint32_t s_part[CJ_THREADS / 64];
  const int t = threadIdx.x;
  const uint32_t k = blockIdx.x / ntiles, tile = blockIdx.x - k * ntiles;

  // the image's decisions (the same for the whole workgroup)
  bool any = false;
  for (int i = s0; i < s1; i++) any |= apply[(uint64_t)i * B + k] != 0;
  const bool add_sum = mode == CJ_SUM && apply[(uint64_t)s1 * B + k] != 0;
  if (!any && !add_sum) return;  // an image no step touches is neither read nor written

  const PixelRun<CJ_THREADS> run(images, img, k, tile, tile_px, s_img);  // staging: lds_stage.h
  run.stage(t);
  __syncthreads();
  uint8_t *s_bytes = run.bytes();
  const uint32_t npix = run.npix();
  auto pixel = [&](uint32_t q) -> uint32_t { return lds_pixel(s_bytes + 3u * q) & 0xffffffu; };
  // the staged pixels' gray sum (fits 32 bits: <= 5461 * 254), in every thread
  auto gray_sum = [&]() -> uint32_t {
    uint32_t s = 0;
    for (uint32_t q = t; q < npix; q += CJ_THREADS) {
      const uint32_t v = pixel(q);
      s += cj_gray(v & 0xffu, (v >> 8) & 0xffu, v >> 16);
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((t & 63) == 0) s_part[t >> 6] = s;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < CJ_THREADS / 64; w++) total += s_part[w];
    return total;
  };

  for (int i = s0; i < s1; i++) {
    if (!apply[(uint64_t)i * B + k]) continue;
    const uint32_t st = (prog >> (8 * i)) & 0xffu;
    // grayscale is saturation at ratio 0 (0 v + 1 gray is exact)
    const double r = st == FFCV_CJ_GRAYSCALE ? 0.0 : ratio[(uint64_t)i * B + k];
    const double omr = cj_one_minus(r);
    if (st == FFCV_CJ_SATURATION || st == FFCV_CJ_GRAYSCALE) {
      for (uint32_t q = t; q < npix; q += CJ_THREADS) {
        const uint32_t v = pixel(q);
        const uint32_t c0 = v & 0xffu, c1 = (v >> 8) & 0xffu, c2 = v >> 16;
        const double g = (double)cj_gray(c0, c1, c2);
        uint8_t *o = s_bytes + 3u * q;
        o[0] = (uint8_t)cj_blend(r, omr, c0, g);
        o[1] = (uint8_t)cj_blend(r, omr, c1, g);
        o[2] = (uint8_t)cj_blend(r, omr, c2, g);
      }
      __syncthreads();
      continue;
    }
    // brightness / contrast / solarize: a 256-entry table of the image, then a byte map
    double other = 0.0;
    if (st == FFCV_CJ_CONTRAST) {
      const uint64_t total = mode == CJ_WHOLE ? (uint64_t)gray_sum() : (uint64_t)ws[k];
      other = cj_mean(total, npx);
    }
    s_tab[t] = (uint8_t)(st == FFCV_CJ_SOLARIZE ? cj_solarize(r, (uint32_t)t)
                                                : cj_blend(r, omr, (uint32_t)t, other));  // CJ_THREADS == 256
    __syncthreads();
    run.map_words(t, [&](uint32_t v) -> uint32_t {
      return (uint32_t)s_tab[v & 0xffu] | ((uint32_t)s_tab[(v >> 8) & 0xffu] << 8) |
             ((uint32_t)s_tab[(v >> 16) & 0xffu] << 16) | ((uint32_t)s_tab[v >> 24] << 24);
    });
    __syncthreads();
  }

  if (add_sum) {
    const uint32_t total = gray_sum();
    if (t == 0) atomicAdd(&ws[k], (unsigned long long)total);
  }
  if (any) run.write_back(t);
}

static int cj_check_program(const char *who, const ffcv_color_jitter_params *p, int *contrast_at) {
  if (p->n_steps < 1 || p->n_steps > 3) {
    ffcv::set_error("%s: a program has 1 to 3 steps, got %d", who, p->n_steps);
    return FFCV_EINVAL;
  }
  unsigned seen = 0;
  *contrast_at = -1;
  for (int i = 0; i < p->n_steps; i++) {
    const int st = p->steps[i];
    if (st < FFCV_CJ_BRIGHTNESS || st > FFCV_CJ_SOLARIZE) {
      ffcv::set_error("%s: unknown step %d at position %d", who, st, i);
      return FFCV_EINVAL;
    }
    if (seen & (1u << st)) {
      ffcv::set_error("%s: step %d repeated at position %d", who, st, i);
      return FFCV_EINVAL;
    }
    seen |= 1u << st;
    if (st == FFCV_CJ_CONTRAST) *contrast_at = i;
  }
  return FFCV_OK;
}

static int cj_check_draw(const char *who, const void *ids, int batch, int op_id, double p, double magnitude,
                         const void *apply, const void *ratio) {
  if (batch < 0 || !ids || !apply || !ratio || op_id < 5 || op_id > 7 || !(p >= 0.0 && p <= 1.0) ||
      !(magnitude >= 0.0) || magnitude > 1.7e308) {
    ffcv::set_error("%s: invalid arguments (op_id %d, p %g, magnitude %g)", who, op_id, p, magnitude);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

static bool uniform_args_ok(const char *who, const void *ids, int batch, int op_id, double p, double lo, double hi,
                            const void *apply, const void *value) {
  if (batch < 0 || !ids || !apply || !value || op_id < 9 || op_id > 11 || !(p >= 0.0 && p <= 1.0) ||
      !std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi)) {
    ffcv::set_error("%s: invalid arguments (op_id %d, p %g, range %g .. %g)", who, op_id, p, lo, hi);
    return false;
  }
  return true;
}

// color_jitter.py:41: uniform(max(0, 1 - magnitude), 1 + magnitude)
static void cj_range(double magnitude, double *lo, double *hi) {
  const double l = 1.0 - magnitude;
  *lo = l < 0.0 ? 0.0 : l;
  *hi = 1.0 + magnitude;
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_color_jitter_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                 uint64_t epoch, int op_id, double p, double magnitude, uint8_t *apply,
                                 double *ratio, int32_t *status) {
  if (cj_check_draw("ffcv_color_jitter_draw_batch", sample_ids, batch, op_id, p, magnitude, apply, ratio))
    return FFCV_EINVAL;
  double lo, hi;
  cj_range(magnitude, &lo, &hi);
  return ffcv::launch_draw("uniform_draw_kernel", uniform_draw_kernel, stream, batch, sample_ids, batch, loader_seed,
                           epoch, (uint32_t)op_id, p, lo, hi, apply, ratio, status);
}

int ffcv_color_jitter_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                      int op_id, double p, double magnitude, uint8_t *apply, double *ratio) {
  if (cj_check_draw("ffcv_color_jitter_draw_batch_host", sample_ids, batch, op_id, p, magnitude, apply, ratio))
    return FFCV_EINVAL;
  double lo, hi;
  cj_range(magnitude, &lo, &hi);
  return ffcv::host_draw("ffcv_color_jitter_draw_batch_host", batch, [&](int k) {
    return draw_color_jitter(k, sample_ids[k], loader_seed, epoch, (uint32_t)op_id, p, lo, hi, apply, ratio);
  });
}

int ffcv_uniform_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                            uint64_t epoch, int op_id, double p, double lo, double hi, uint8_t *apply,
                            double *value, int32_t *status) {
  if (!uniform_args_ok("ffcv_uniform_draw_batch", sample_ids, batch, op_id, p, lo, hi, apply, value))
    return FFCV_EINVAL;
  return ffcv::launch_draw("uniform_draw_kernel", uniform_draw_kernel, stream, batch, sample_ids, batch, loader_seed,
                           epoch, (uint32_t)op_id, p, lo, hi, apply, value, status);
}

int ffcv_uniform_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                 int op_id, double p, double lo, double hi, uint8_t *apply, double *value) {
  if (!uniform_args_ok("ffcv_uniform_draw_batch_host", sample_ids, batch, op_id, p, lo, hi, apply, value))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_uniform_draw_batch_host", batch, [&](int k) {
    return draw_color_jitter(k, sample_ids[k], loader_seed, epoch, (uint32_t)op_id, p, lo, hi, apply, value);
  });
}

uint64_t ffcv_color_jitter_workspace_bytes(int batch) { return batch > 0 ? 8ull * (uint64_t)batch : 0; }
uint64_t ffcv_color_jitter_lds_bytes(void) { return CJ_LDS_BYTES; }

int ffcv_color_jitter_batch(void *stream, uint8_t *images, int batch, int height, int width,
                            const ffcv_color_jitter_params *params, const uint8_t *apply, const double *ratio,
                            void *workspace, uint64_t workspace_bytes) {
  if (!ffcv::u8_images_ok("ffcv_color_jitter_batch", images && params && apply && ratio, batch, height, width))
    return FFCV_EINVAL;
  int c = -1;
  if (cj_check_program("ffcv_color_jitter_batch", params, &c)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const int n = params->n_steps;
  const uint32_t prog =
      (uint32_t)params->steps[0] | ((uint32_t)params->steps[1] << 8) | ((uint32_t)params->steps[2] << 16);
  const uint64_t npx = (uint64_t)height * width, img = npx * 3;
  const bool whole = img <= CJ_LDS_BYTES;
  uint32_t tile_px, ntiles;
  unsigned blocks;
  if (!ffcv::run_tiling("ffcv_color_jitter_batch", batch, npx, CJ_LDS_BYTES, CJ_TILE_PX, &tile_px, &ntiles, &blocks))
    return FFCV_EINVAL;
  hipStream_t s = ffcv::as_stream(stream);
  unsigned long long *ws = (unsigned long long *)workspace;
  if (whole || c < 0) {
    hipLaunchKernelGGL(color_jitter_kernel, dim3(blocks), dim3(CJ_THREADS), 0, s, images, batch, img, npx, prog, 0, n,
                       apply, ratio, ws, whole ? CJ_WHOLE : CJ_POINT, tile_px, ntiles);
    FFCV_LAUNCH_CHECK("color_jitter_kernel");
    return FFCV_OK;
  }
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < ffcv_color_jitter_workspace_bytes(batch)) {
    ffcv::set_error("ffcv_color_jitter_batch: a contrast step on %dx%d images needs an 8-byte aligned workspace of "
                    "%llu bytes, got %llu",
                    height, width, (unsigned long long)ffcv_color_jitter_workspace_bytes(batch),
                    (unsigned long long)workspace_bytes);
    return FFCV_EINVAL;
  }
  FFCV_HIP_CHECK(hipMemsetAsync(workspace, 0, 8ull * (uint64_t)batch, s));
  hipLaunchKernelGGL(color_jitter_kernel, dim3(blocks), dim3(CJ_THREADS), 0, s, images, batch, img, npx, prog, 0, c,
                     apply, ratio, ws, CJ_SUM, tile_px, ntiles);
  FFCV_LAUNCH_CHECK("color_jitter_kernel (pass A)");
  hipLaunchKernelGGL(color_jitter_kernel, dim3(blocks), dim3(CJ_THREADS), 0, s, images, batch, img, npx, prog, c, n,
                     apply, ratio, ws, CJ_POINT, tile_px, ntiles);
  FFCV_LAUNCH_CHECK("color_jitter_kernel (pass B)");
  return FFCV_OK;
}

int ffcv_color_jitter_batch_host(uint8_t *images, int batch, int height, int width,
                                 const ffcv_color_jitter_params *params, const uint8_t *apply, const double *ratio) {
  if (!ffcv::u8_images_ok("ffcv_color_jitter_batch_host", images && params && apply && ratio, batch, height, width))
    return FFCV_EINVAL;
  int c = -1;
  if (cj_check_program("ffcv_color_jitter_batch_host", params, &c)) return FFCV_EINVAL;
  const uint64_t npx = (uint64_t)height * width;
  for (int k = 0; k < batch; k++) {
    uint8_t *im = images + (uint64_t)k * npx * 3;
    for (int i = 0; i < params->n_steps; i++) {
      if (!apply[(uint64_t)i * batch + k]) continue;
      const int st = params->steps[i];
      const double r = st == FFCV_CJ_GRAYSCALE ? 0.0 : ratio[(uint64_t)i * batch + k];
      const double omr = cj_one_minus(r);
      if (st == FFCV_CJ_SATURATION || st == FFCV_CJ_GRAYSCALE) {
        for (uint64_t q = 0; q < npx; q++) {
          uint8_t *o = im + 3 * q;
          const uint32_t c0 = o[0], c1 = o[1], c2 = o[2];
          const double g = (double)cj_gray(c0, c1, c2);
          o[0] = (uint8_t)cj_blend(r, omr, c0, g);
          o[1] = (uint8_t)cj_blend(r, omr, c1, g);
          o[2] = (uint8_t)cj_blend(r, omr, c2, g);
        }
        continue;
      }
      double other = 0.0;
      if (st == FFCV_CJ_CONTRAST) {
        uint64_t total = 0;
        for (uint64_t q = 0; q < npx; q++) total += cj_gray(im[3 * q], im[3 * q + 1], im[3 * q + 2]);
        other = cj_mean(total, npx);
      }
      uint8_t tab[256];
      for (uint32_t v = 0; v < 256; v++)
        tab[v] = (uint8_t)(st == FFCV_CJ_SOLARIZE ? cj_solarize(r, v) : cj_blend(r, omr, v, other));
      for (uint64_t j = 0; j < npx * 3; j++) im[j] = tab[im[j]];
    }
  }
  return FFCV_OK;
}

}  // extern "C"
