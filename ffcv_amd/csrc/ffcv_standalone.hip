// ffcv_standalone.hip -- the first-generation standalone transforms, one pass over a dense batch
// each: Cutout (cutout.py:36-47), the table lookup, flip and RandomTranslate with its draw.
#include "api_internal.h"
#include "device_common.h"

__global__ void __launch_bounds__(256) cutout_kernel(uint8_t *__restrict__ img, int H, int W,
                                                     const int32_t *__restrict__ yx, int c, uint8_t f0,
                                                     uint8_t f1, uint8_t f2) {
  const int k = blockIdx.x;
  const int y0 = yx[2 * k], x0 = yx[2 * k + 1];
  uint8_t *base = img + (uint64_t)k * H * W * 3;
  for (int i = threadIdx.x; i < c * c; i += 256) {
    int y = y0 + i / c, x = x0 + i % c;
    if (y < H && x < W) {
      uint8_t *p = base + ((uint64_t)y * W + x) * 3;
      p[0] = f0;
      p[1] = f1;
      p[2] = f2;
    }
  }
}

// normalize.py:64-65: output = table[input * 3 + i % 3] for any table dtype
// (the cupy kernel is templated on T); T is the element's bit pattern, so
// one instantiation per element size serves every dtype of that size.  The
// 768-entry table lives in LDS; 12 elements (4 RGB pixels) per lane, input
// read as three dwords when 4-byte aligned.
template <class T>
__global__ void __launch_bounds__(256) lut_kernel(const uint8_t *__restrict__ in, uint64_t n,
                                                  const T *__restrict__ lut, T *__restrict__ out) {
  __shared__ T s_lut[768];
  for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = lut[i];
  __syncthreads();
  const uint64_t groups = n / 12;
  const bool aligned = ((uintptr_t)in & 3) == 0;
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256) {
    const uint8_t *ip = in + g * 12;
    uint8_t v[12];
    if (aligned) {
      const uint32_t *w = (const uint32_t *)ip;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        uint32_t x = w[q];
#pragma unroll
        for (int b = 0; b < 4; b++) v[4 * q + b] = (uint8_t)(x >> (8 * b));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 12; e++) v[e] = ip[e];
    }
    T *op = out + g * 12;
#pragma unroll
    for (int e = 0; e < 12; e++) op[e] = s_lut[v[e] * 3 + (e % 3)];
  }
  if (blockIdx.x == 0) {
    for (uint64_t i = groups * 12 + threadIdx.x; i < n; i += 256) out[i] = s_lut[in[i] * 3 + (i % 3)];
  }
}

__global__ void __launch_bounds__(256) flip_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                   int H, int W, int cb, const uint8_t *__restrict__ flips) {
  const int k = blockIdx.y;
  const uint64_t img = (uint64_t)H * W * cb;
  const bool f = flips[k] != 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < img; i += (uint64_t)gridDim.x * 256) {
    uint64_t px = i / cb;
    int b = (int)(i - px * cb);
    int y = (int)(px / W), x = (int)(px - (uint64_t)y * W);
    int sx = f ? W - 1 - x : x;
    out[k * img + i] = in[k * img + ((uint64_t)y * W + sx) * cb + b];
  }
}

// ------------------------------------------------ RandomTranslate -------
__global__ void __launch_bounds__(64) translate_draw_kernel(const uint64_t *__restrict__ ids, int B,
                                                            uint64_t loader_seed, uint64_t epoch, int padding,
                                                            int32_t *__restrict__ yx, int32_t *__restrict__ status) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_translate(k, ids[k], loader_seed, epoch, padding, yx);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// translate.py:35-44: out[r, c] = in[r + y - p, c + x - p] inside the image, else fill
__global__ void __launch_bounds__(256) translate_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                        int H, int W, const int32_t *__restrict__ yx, int pad,
                                                        uint8_t f0, uint8_t f1, uint8_t f2) {
  const int k = blockIdx.y;
  const uint64_t img = (uint64_t)H * W * 3;
  const int64_t dy = (int64_t)yx[2 * k] - pad, dx = (int64_t)yx[2 * k + 1] - pad;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < img; i += (uint64_t)gridDim.x * 256) {
    const uint64_t px = i / 3;
    const int b = (int)(i - px * 3);
    const int y = (int)(px / W), x = (int)(px - (uint64_t)y * W);
    const int64_t sy = y + dy, sx = x + dx;
    uint8_t v = b == 0 ? f0 : (b == 1 ? f1 : f2);
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = in[k * img + ((uint64_t)sy * W + (uint64_t)sx) * 3 + b];
    out[k * img + i] = v;
  }
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

// flip_kernel and translate_kernel take the image from blockIdx.y, and a grid
// has at most 65,535 rows: their entries launch a larger batch in slices of
// that many images, with the per-image pointers advanced.
#define MAX_GRID_Y 65535
static inline unsigned slice_of(int batch, int64_t k0) {
  return (unsigned)(batch - k0 < MAX_GRID_Y ? batch - k0 : MAX_GRID_Y);
}

int ffcv_cutout_batch(void *stream, uint8_t *images, int batch, int height, int width,
                      const int32_t *cutout_yx, int crop_size, const uint8_t fill[3]) {
  if (batch < 0 || !images || !cutout_yx || crop_size <= 0 || crop_size > height || crop_size > width) {
    ffcv::set_error("ffcv_cutout_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  hipLaunchKernelGGL(cutout_kernel, dim3(batch), dim3(256), 0, ffcv::as_stream(stream), images, height,
                     width, cutout_yx, crop_size, fill[0], fill[1], fill[2]);
  FFCV_LAUNCH_CHECK("cutout_kernel");
  return FFCV_OK;
}

int ffcv_lut_batch(void *stream, const uint8_t *in, uint64_t n, const void *lut, int elem_bytes, void *out) {
  if (!in || !lut || !out || !(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8)) {
    ffcv::set_error("ffcv_lut_batch: invalid arguments (element size %d)", elem_bytes);
    return FFCV_EINVAL;
  }
  if (n == 0) return FFCV_OK;
  uint64_t groups = n / 12 + 1;
  unsigned gx = (unsigned)((groups + 255) / 256);
  if (gx > 8192) gx = 8192;
  hipStream_t s = ffcv::as_stream(stream);
  switch (elem_bytes) {
    case 1:
      hipLaunchKernelGGL(lut_kernel<uint8_t>, dim3(gx), dim3(256), 0, s, in, n, (const uint8_t *)lut, (uint8_t *)out);
      break;
    case 2:
      hipLaunchKernelGGL(lut_kernel<uint16_t>, dim3(gx), dim3(256), 0, s, in, n, (const uint16_t *)lut,
                         (uint16_t *)out);
      break;
    case 4:
      hipLaunchKernelGGL(lut_kernel<uint32_t>, dim3(gx), dim3(256), 0, s, in, n, (const uint32_t *)lut,
                         (uint32_t *)out);
      break;
    default:
      hipLaunchKernelGGL(lut_kernel<uint64_t>, dim3(gx), dim3(256), 0, s, in, n, (const uint64_t *)lut,
                         (uint64_t *)out);
      break;
  }
  FFCV_LAUNCH_CHECK("lut_kernel");
  return FFCV_OK;
}

int ffcv_normalize_batch(void *stream, const uint8_t *in, uint64_t n, const uint16_t *lut, uint16_t *out) {
  return ffcv_lut_batch(stream, in, n, lut, 2, out);
}

int ffcv_flip_batch(void *stream, const uint8_t *in, uint8_t *out, int batch, int height, int width,
                    int channels_bytes, const uint8_t *flips) {
  if (batch < 0 || !in || !out || !flips || in == out || height <= 0 || width <= 0 || channels_bytes <= 0) {
    ffcv::set_error("ffcv_flip_batch: invalid arguments (in-place flip unsupported)");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  uint64_t img = (uint64_t)height * width * channels_bytes;
  unsigned gx = (unsigned)((img + 255) / 256);
  if (gx > 256) gx = 256;
  for (int64_t k0 = 0; k0 < batch; k0 += MAX_GRID_Y) {
    hipLaunchKernelGGL(flip_kernel, dim3(gx, slice_of(batch, k0)), dim3(256), 0, ffcv::as_stream(stream),
                       in + img * k0, out + img * k0, height, width, channels_bytes, flips + k0);
    FFCV_LAUNCH_CHECK("flip_kernel");
  }
  return FFCV_OK;
}

int ffcv_translate_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                              uint64_t epoch, int padding, int32_t *yx, int32_t *status) {
  if (batch < 0 || !sample_ids || !yx || padding < 0 || padding >= (1 << 30)) {
    ffcv::set_error("ffcv_translate_draw_batch: invalid arguments (padding %d)", padding);
    return FFCV_EINVAL;
  }
  return ffcv::launch_draw("translate_draw_kernel", translate_draw_kernel, stream, batch, sample_ids, batch,
                           loader_seed, epoch, padding, yx, status);
}

int ffcv_translate_batch(void *stream, const uint8_t *in, uint8_t *out, int batch, int height, int width,
                         const int32_t *yx, int padding, const uint8_t fill[3]) {
  if (batch < 0 || !in || !out || !yx || !fill || in == out || height <= 0 || width <= 0 || padding < 0 ||
      padding >= (1 << 30)) {
    ffcv::set_error("ffcv_translate_batch: invalid arguments (in-place translate unsupported)");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  uint64_t img = (uint64_t)height * width * 3;
  unsigned gx = (unsigned)((img + 255) / 256);
  if (gx > 256) gx = 256;
  for (int64_t k0 = 0; k0 < batch; k0 += MAX_GRID_Y) {
    hipLaunchKernelGGL(translate_kernel, dim3(gx, slice_of(batch, k0)), dim3(256), 0, ffcv::as_stream(stream),
                       in + img * k0, out + img * k0, height, width, yx + 2 * (uint64_t)k0, padding, fill[0], fill[1],
                       fill[2]);
    FFCV_LAUNCH_CHECK("translate_kernel");
  }
  return FFCV_OK;
}

}  // extern "C"
