// ffcv_randaugment_large.hip -- RandAugment's fused pixel pass for images
// beyond 64 x 64, up to 224 x 224: the bytes of
// ffcv_randaugment_batch, from ONE image buffer in LDS.
//
//   randaugment_large_kernel: one workgroup per image.  The image is staged as
//     bytes in LDS once and leaves once, as in randaugment_kernel
//     (lds_stage.h).  An operation that works in place runs as in ra_slot.h,
//     with every thread on the pixel passes and threads 0..255 on the 256
//     table entries and histogram bins.  An operation that moves pixels
//     (shear / translate / rotate, the sharpness stencil) has no second buffer
//     to write into: a thread computes its share of the result into registers
//     (the loop over its steps is unrolled to a compile-time bound, a
//     predicate per step), all threads meet at a barrier, and the registers
//     are stored over the image, dense from byte 16 on.  (The slot code is
//     ral_slot.h, which AugMix's kernel for these shapes shares.)
//
// 1024 threads, an image of 150,528 bytes (224 x 224 x 3): 13 warp steps of
// three dwords or 37 stencil dwords per thread, 114 VGPRs (four waves per
// SIMD), 154,720 B of LDS, one workgroup per CU.  (A second instance of 512
// threads and 76,800 bytes, two workgroups per CU, was slower at 128 x 128 and
// 160 x 160 than this one and is not built.)
//
// LDS: the image + 64 B (16 in front for a tap left of column 0, 16 for the
// staged range's lead, 32 of read-ahead), the counters 3,072, the tables 768,
// scan partials 12 B per wave, occupancy words 96.
#if defined(__HIP_DEVICE_COMPILE__)
// every float32 product and sum of the stencil is an instruction of its own
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "api_internal.h"
#include "ral_slot.h"

#define RAL_MAX_SLOTS 8
#define RAL_MIN_BYTES 40960

template <class T>
__global__ void __launch_bounds__(T::THREADS)
    randaugment_large_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int B, int H0, int W0,
                             int num_ops, int mode, uint32_t fill0, RaIn A) {
  __shared__ lds_x4_t s_buf[T::CHUNKS];  // the image
  __shared__ uint32_t s_hist[3 * 256];   // the channel histograms
  __shared__ uint8_t s_tab[3 * 256];     // the slot's table: one, or one per channel
  __shared__ uint32_t s_part[3][T::WAVES];
  __shared__ uint64_t s_occ[3][4];
  const int t0 = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const uint32_t nbytes0 = 3u * (uint32_t)H0 * (uint32_t)W0;  // <= T::IMG_BYTES
  uint8_t *const s_mem = (uint8_t *)s_buf;
  const RalScratch<T> lds = {s_hist, s_tab, s_part, s_occ};

  // ---- stage the image: one byte range, behind the buffer's 16 front bytes
  const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * nbytes0;
  stage_rows<T::THREADS>(t0, src0, 0, 1, nbytes0, (int)lds_chunks(nbytes0), s_buf + 1);
  uint32_t cur_off = 16u + (uint32_t)(src0 & 15);  // where in s_mem the image's first byte is
  __syncthreads();

  for (int s = 0; s < num_ops; s++) ral_slot<T>(t0, H0, W0, fill0, mode, B, k, s, A, s_mem, cur_off, lds);

  // ---- write out once, at any alignment of dst
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * nbytes0;
  const uint8_t *out = s_mem + cur_off;
  write_back_rows<T::THREADS>(t0, dst0, 0, 1, nbytes0, [&](int) { return out; });
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

// Every shape of 3 H W <= 150,528 bytes (H, W <= 224 among them) whose step
// counts stay inside the unrolled bounds: 13 x 1024 groups of four pixels and
// 37 x 1024 groups of four row bytes.  The second bound leaves out tall thin
// shapes whose rows each end in a partial group (3 W no multiple of 4): 3
// pixels wide from 12,630 rows on, 6 wide from 7,578, 7 wide from 6,315.
int ffcv_randaugment_large_fits(int height, int width) { return RalTop::fits(height, width) ? 1 : 0; }

uint64_t ffcv_randaugment_large_min_bytes(void) { return RAL_MIN_BYTES; }

int ffcv_randaugment_large_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                                 int num_ops, int mode, const uint8_t *fill, const uint8_t *op,
                                 const uint8_t *cj_apply, const double *cj_ratio, const uint8_t *tone_apply,
                                 const uint8_t *tone_bits, const uint8_t *aff_apply, const int64_t *aff_coef,
                                 const uint8_t *sharp_apply, const float *sharp_factor) {
  const char *who = "ffcv_randaugment_large_batch";
  const bool pointers = fill && op && cj_apply && cj_ratio && tone_apply && tone_bits && aff_apply && aff_coef &&
                        sharp_apply && sharp_factor;
  uint64_t stride;
  if (!ffcv::out_of_place_ok(who, pointers, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM, 0, &stride))
    return FFCV_EINVAL;
  if (num_ops < 1 || num_ops > RAL_MAX_SLOTS) {
    ffcv::set_error("%s: %d operations per sample, outside 1 to %d", who, num_ops, RAL_MAX_SLOTS);
    return FFCV_EINVAL;
  }
  if (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) {
    ffcv::set_error("%s: mode %d is neither FFCV_AFFINE_BILINEAR nor FFCV_AFFINE_NEAREST", who, mode);
    return FFCV_EINVAL;
  }
  if (!ffcv_randaugment_large_fits(height, width)) {
    ffcv::set_error("%s: images of %dx%d are outside the kernel's regime (3 H W <= %d, see "
                    "ffcv_randaugment_large_fits): run the slots' launches instead",
                    who, height, width, RalTop::IMG_BYTES);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  const RaIn A = {op, cj_ratio, tone_bits, aff_coef, sharp_factor};
  const uint32_t f = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
  return ffcv::launch_tiles(who, "randaugment_large_kernel", randaugment_large_kernel<RalTop>, stream,
                            (uint64_t)batch, RalTop::THREADS, 0, src, dst, batch, height, width, num_ops, mode, f, A);
}

}  // extern "C"
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
