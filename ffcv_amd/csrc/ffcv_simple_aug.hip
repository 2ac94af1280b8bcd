// ffcv_simple_aug.hip -- the fused small-image augmentation (pull): translate, flip and cutout in
// any order plus the LUT normalize of raw samples of one size, one launch, each source byte read once.
#include "api_internal.h"
#include "device_common.h"

#define AUG_THREADS 256
#define AUG_STAGE_BYTES 16384  // source rows one workgroup stages (a 32x32 image is 3 KB)

// One workgroup per band of output rows of one raw sample (a whole 32x32
// image; `band` rows of a larger one, chosen by the host so that the rows fit
// AUG_STAGE_BYTES).
//   Staging: only a translate step moves rows, so the band reads source rows
//   [oy0 + y - p, oy1 + y - p) clipped to the image: one contiguous byte range
//   of the sample, copied to LDS with 16-byte aligned global loads whatever
//   the sample's byte offset (an aligned chunk holding a byte of the range
//   never crosses a page).  Rows wider than the stage are read from global
//   memory instead.
//   Pull: output elements are taken in groups of four that are 4-byte (u8) or
//   8-byte (fp16) aligned IN MEMORY, so a whole group leaves as one store; the
//   groups cut by the band's ends store their elements one by one.  Each pixel
//   of a group walks the program backwards (pull_px) to a fill colour or to
//   the source pixel it shows.
template <bool FP16>
__global__ void __launch_bounds__(AUG_THREADS)
    simple_aug_kernel(const uint8_t *__restrict__ base, const ffcv_sample *__restrict__ samples, int H, int W,
                      ffcv_simple_aug_params p, const uint8_t *__restrict__ flips, const int32_t *__restrict__ cut,
                      const int32_t *__restrict__ tyx, const uint16_t *__restrict__ lut, void *__restrict__ out,
                      uint64_t stride, int band, int nbands) {
  typedef uint32_t sx4_t __attribute__((ext_vector_type(4)));
  __shared__ uint16_t s_lut[FP16 ? 768 : 1];
  __shared__ sx4_t s_src[AUG_STAGE_BYTES / 16 + 2];  // + the range's lead bytes and pull_px's read-ahead
  const int t = threadIdx.x;
  const int k = blockIdx.x / nbands, bi = blockIdx.x - k * nbands;
  const ffcv_sample s = samples[k];
  const uint32_t row = 3u * (uint32_t)W;  // bytes per image row (height * row < 2^31, checked by the host)
  if (s.mode != 1 || s.size < (uint64_t)H * row) return;  // (the same for the whole workgroup)
  const int oy0 = bi * band, oy1 = min(H, oy0 + band);

  // the sample's decisions; steps[0] is the first operation of the pipeline
  const int n = p.n_steps;
  const uint32_t prog = (uint32_t)p.steps[0] | ((uint32_t)p.steps[1] << 8) | ((uint32_t)p.steps[2] << 16);
  int dy = 0, dx = 0, cy = 0, cx = 0;
  bool flip = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const uint32_t st = i < n ? (prog >> (8 * i)) & 0xffu : 0u;
    if (st == FFCV_AUG_TRANSLATE) {
      dy = tyx[2 * k] - p.padding;
      dx = tyx[2 * k + 1] - p.padding;
    }
    if (st == FFCV_AUG_FLIP) flip = flips[k] != 0;
    if (st == FFCV_AUG_CUTOUT) {
      cy = cut[2 * k];
      cx = cut[2 * k + 1];
    }
  }
  const int cs = p.cutout_size;
  const uint32_t tfill = p.translate_fill[0] | ((uint32_t)p.translate_fill[1] << 8) | ((uint32_t)p.translate_fill[2] << 16);
  const uint32_t cfill = p.cutout_fill[0] | ((uint32_t)p.cutout_fill[1] << 8) | ((uint32_t)p.cutout_fill[2] << 16);

  // ---- stage the band's source rows
  const int sr0 = min(max(oy0 + dy, 0), H), sr1 = min(max(oy1 + dy, 0), H);
  const uint32_t nbytes = (uint32_t)(sr1 - sr0) * row;
  const bool staged = (uint32_t)band * row <= AUG_STAGE_BYTES;
  const uint8_t *src = base + s.offset + (uint64_t)sr0 * row;  // source row sr0
  const uint32_t lead = (uint32_t)((uintptr_t)src & 15);
  if (staged && nbytes) {
    // (a global-address-space pointer: global_load_dwordx4, not a flat load)
    typedef const __attribute__((address_space(1))) sx4_t gx4_t;
    gx4_t *gp = (gx4_t *)((uintptr_t)src & ~(uintptr_t)15);
    const int nch = (int)((lead + nbytes + 15) >> 4);  // <= AUG_STAGE_BYTES / 16 + 1
    for (int i = t; i < nch; i += AUG_THREADS) s_src[i] = gp[i];
  }
  if (FP16) {
    for (int i = t; i < 768; i += AUG_THREADS) s_lut[i] = lut[i];
  }
  __syncthreads();

  // The source pixel (R | G << 8 | B << 16) that output pixel (r, c) shows.
  // A pixel that met a fill keeps walking with its colour set (no divergent
  // early return); a pixel that met none ends inside rows [sr0, sr1).
  auto pull_px = [&](int r, int c) -> uint32_t {
    uint32_t fillv = 0;
    bool filled = false;
    for (int i = n - 1; i >= 0; i--) {
      const uint32_t st = (prog >> (8 * i)) & 0xffu;  // wave-uniform
      if (st == FFCV_AUG_CUTOUT) {
        if (!filled && r >= cy && r < cy + cs && c >= cx && c < cx + cs) {
          filled = true;
          fillv = cfill;
        }
      } else if (st == FFCV_AUG_TRANSLATE) {
        r += dy;
        c += dx;
        if (!filled && (r < 0 || r >= H || c < 0 || c >= W)) {
          filled = true;
          fillv = tfill;
        }
      } else {
        c = flip ? W - 1 - c : c;
      }
    }
    if (filled) return fillv;
    const uint32_t off = ((uint32_t)(r - sr0) * (uint32_t)W + (uint32_t)c) * 3u;
    if (staged) {
      // the pixel's three bytes from two ALIGNED 4-byte LDS reads joined by
      // v_alignbyte (misaligned LDS reads are several times slower); reads up
      // to 4 bytes past the pixel, inside s_src
      const uint8_t *q = (const uint8_t *)s_src + lead + off;
      const uint32_t *qa = (const uint32_t *)__builtin_align_down(q, 4);
      return __builtin_amdgcn_alignbyte(qa[1], qa[0], (uint32_t)(q - (const uint8_t *)qa)) & 0xffffffu;
    }
    const uint8_t *q = src + off;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  };

  // ---- pull
  char *o = (char *)out + stride * k;
  const uint32_t e_lo = (uint32_t)oy0 * row, e_hi = (uint32_t)oy1 * row;  // the band's elements of the image
  const uint32_t mis = (uint32_t)(((uintptr_t)o / (FP16 ? 2 : 1)) & 3);   // elements past a group boundary at o
  // group g holds elements 4 g - mis .. 4 g - mis + 3
  const uint32_t g0 = (e_lo + mis) >> 2, g1 = (e_hi + mis + 3) >> 2;
  for (uint32_t g = g0 + t; g < g1; g += AUG_THREADS) {
    const int64_t e0 = (int64_t)4 * g - mis;
    if (e0 >= (int64_t)e_lo && e0 + 4 <= (int64_t)e_hi) {
      const uint32_t e = (uint32_t)e0, px = e / 3u;
      int ch = (int)(e - 3u * px);
      int r = (int)(px / (uint32_t)W), c = (int)(px - (uint32_t)r * (uint32_t)W);
      uint32_t v = pull_px(r, c);
      uint32_t val[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        val[j] = (v >> (8 * ch)) & 0xffu;
        if (FP16) val[j] = s_lut[val[j] * 3 + ch];
        if (++ch == 3) {
          ch = 0;
          if (++c == W) {
            c = 0;
            r++;
          }
          if (j < 3) v = pull_px(r, c);
        }
      }
      if (FP16)
        *(uint2 *)((uint16_t *)o + e) = make_uint2(val[0] | (val[1] << 16), val[2] | (val[3] << 16));
      else
        *(uint32_t *)((uint8_t *)o + e) = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
    } else {
      for (int j = 0; j < 4; j++) {
        const int64_t ej = e0 + j;
        if (ej < (int64_t)e_lo || ej >= (int64_t)e_hi) continue;
        const uint32_t e = (uint32_t)ej, px = e / 3u;
        const int ch = (int)(e - 3u * px);
        const int r = (int)(px / (uint32_t)W), c = (int)(px - (uint32_t)r * (uint32_t)W);
        const uint32_t b = (pull_px(r, c) >> (8 * ch)) & 0xffu;
        if (FP16)
          ((uint16_t *)o)[e] = s_lut[b * 3 + ch];
        else
          ((uint8_t *)o)[e] = (uint8_t)b;
      }
    }
  }
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_simple_aug_batch(void *stream, const uint8_t *base, const ffcv_sample *samples, int batch, int height,
                          int width, const ffcv_simple_aug_params *p, const uint8_t *flips,
                          const int32_t *cutout_yx, const int32_t *translate_yx, const uint16_t *lut, void *out,
                          uint64_t out_stride) {
  if (batch < 0 || !base || !samples || !p || !out || height <= 0 || width <= 0 ||
      (uint64_t)height * width * 3 > 0x7fffffffull) {
    ffcv::set_error("ffcv_simple_aug_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (p->n_steps < 1 || p->n_steps > 3) {
    ffcv::set_error("ffcv_simple_aug_batch: a program has 1 to 3 steps, got %d", p->n_steps);
    return FFCV_EINVAL;
  }
  unsigned seen = 0;
  for (int i = 0; i < p->n_steps; i++) {
    const int st = p->steps[i];
    if (st != FFCV_AUG_FLIP && st != FFCV_AUG_TRANSLATE && st != FFCV_AUG_CUTOUT) {
      ffcv::set_error("ffcv_simple_aug_batch: unknown step %d at position %d", st, i);
      return FFCV_EINVAL;
    }
    if (seen & (1u << st)) {
      ffcv::set_error("ffcv_simple_aug_batch: step %d repeated at position %d", st, i);
      return FFCV_EINVAL;
    }
    seen |= 1u << st;
    if ((st == FFCV_AUG_FLIP && !flips) || (st == FFCV_AUG_TRANSLATE && !translate_yx) ||
        (st == FFCV_AUG_CUTOUT && !cutout_yx)) {
      ffcv::set_error("ffcv_simple_aug_batch: step %d has no decision array", st);
      return FFCV_EINVAL;
    }
  }
  if ((seen & (1u << FFCV_AUG_TRANSLATE)) && (p->padding < 0 || p->padding >= (1 << 30))) {
    ffcv::set_error("ffcv_simple_aug_batch: padding %d out of range", p->padding);
    return FFCV_EINVAL;
  }
  if ((seen & (1u << FFCV_AUG_CUTOUT)) &&
      (p->cutout_size <= 0 || p->cutout_size > height || p->cutout_size > width)) {
    ffcv::set_error("ffcv_simple_aug_batch: cutout_size %d does not fit %dx%d", p->cutout_size, height, width);
    return FFCV_EINVAL;
  }
  const bool fp16 = lut != nullptr;
  const uint64_t dense = (uint64_t)height * width * 3 * (fp16 ? 2 : 1);
  const uint64_t stride = out_stride ? out_stride : dense;
  if (stride < dense || (fp16 && ((((uintptr_t)out) | stride) & 1))) {
    ffcv::set_error("ffcv_simple_aug_batch: out_stride %llu for samples of %llu bytes (fp16: 2-byte aligned)",
                    (unsigned long long)stride, (unsigned long long)dense);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  // rows per workgroup: what fits the stage (a row wider than it: one row, read from global memory)
  const uint64_t row = (uint64_t)width * 3;
  int band = 1;
  if (row <= AUG_STAGE_BYTES) band = AUG_STAGE_BYTES / row < (uint64_t)height ? (int)(AUG_STAGE_BYTES / row) : height;
  const int nbands = (height + band - 1) / band;
  const uint64_t blocks = (uint64_t)batch * nbands;
  if (blocks > 0x7fffffffull) {
    ffcv::set_error("ffcv_simple_aug_batch: %llu workgroups exceed one launch", (unsigned long long)blocks);
    return FFCV_EINVAL;
  }
  if (fp16)
    hipLaunchKernelGGL(simple_aug_kernel<true>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0,
                       ffcv::as_stream(stream), base, samples, height, width, *p, flips, cutout_yx, translate_yx, lut,
                       out, stride, band, nbands);
  else
    hipLaunchKernelGGL(simple_aug_kernel<false>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0,
                       ffcv::as_stream(stream), base, samples, height, width, *p, flips, cutout_yx, translate_yx, lut,
                       out, stride, band, nbands);
  FFCV_LAUNCH_CHECK("simple_aug_kernel");
  return FFCV_OK;
}

}  // extern "C"
