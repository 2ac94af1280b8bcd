// ffcv_rrc_images.hip -- the RandomResizedCrop TRANSFORM
// (ffcv/transforms/random_resized_crop.py: fast_crop.py get_random_crop, then
// resize_crop = cv::resize INTER_AREA) on a dense batch [B][H][W][3] of
// equal-size images, with the decoder path's flip / cutout / LUT epilogue.
//
// The raw decoder's kernel (ffcv_rrc.hip) is shaped for .beton samples of any
// size: a descriptor per sample, a taps kernel into a workspace and a
// workgroup per band of 16 output rows.  A CIFAR or 64 px image fits a
// fraction of a CU's LDS, so here ONE workgroup owns an image: it stages the
// crop's rows once, builds the out_w + out_h taps in LDS itself and writes the
// final pixels (rrc_images_kernel).  Images too large for that run the band
// kernel behind a small descriptor kernel (rrc_images_desc_kernel).
#include <cmath>

#include "api_internal.h"
#include "device_common.h"
#include "lds_stage.h"
#include "resize_out.h"

#define RRCI_THREADS 256
// The largest staged source (rows of whole 16-byte chunks, see lds_src_bytes)
// a launch runs in the LDS regime: 64 x 64 fits, 96 x 96 does not.  Set from
// the measurement in profiles/rrc_transform_bench.txt: the
// LDS kernel is 1.9-3.5x faster than the band kernel up to a 64 x 64 source
// and slower from 96 x 96 on.
#define RRCI_LDS_BYTES 16384
#define RRCI_LDS_MAX 65536  // LDS one workgroup may allocate
#define RRCI_TAP_BYTES 32   // one LDS tap record (AreaTaps: 28 bytes, LinTap: 16)

// Crop window of one sample from its own MT19937, op id 8 ("crop transform":
// id 1 is the decoder's, so a pipeline with both draws two streams).
// A crop takes at most 44 words of its stream (ten tries of two doubles, then
// two more), all of them among the first 227, which need only the generator's
// initial state (device_common.h): this generator is DevMT without the
// out-of-line path for the words behind them, whose call frame would cost the
// draw kernel scratch.  Word 227 and later set err (FFCV_SAMPLE_RNG).
struct CropMT {
  DevMT m;
};
FFCV_HD double mt_uniform(CropMT &g, double lo, double hi) {
  uint32_t w[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    DevMT &m = g.m;
    uint32_t v = 0;
    if (m.n < 227) {
      v = mt_twist1(m.a0, m.a1, m.b);
      m.a0 = m.a1;
      m.a1 = mt_chain(m.a1, (uint32_t)(m.n + 2));
      m.b = mt_chain(m.b, (uint32_t)(m.n + 398));
    } else {
      m.err = 1;
    }
    m.n++;
    w[i] = mt_temper(v);
  }
  const int32_t a = (int32_t)(w[0] >> 5), b = (int32_t)(w[1] >> 6);
  const double range = hi - lo;
  return lo + range * ((a * 67108864.0 + b) / 9007199254740992.0);
}

FFCV_HD int draw_crop_transform(int k, uint64_t id, uint32_t H, uint32_t W, const double *scale,
                                const double *ratio, uint64_t loader_seed, uint64_t epoch, int32_t *crops) {
  CropMT g;
  DevMT &m = g.m;
  mt_init(m, sample_seed(loader_seed, epoch, id, 8));
  random_crop(g, H, W, scale, ratio, crops + 4 * k);
  return m.err;
}

struct CropRanges {  // a kernel argument: read in place (local arrays of them went to scratch)
  double scale[2], ratio[2];
};

__global__ void __launch_bounds__(64) crop_draw_kernel(const uint64_t *__restrict__ ids, int B, uint32_t H,
                                                       uint32_t W, CropRanges rg, uint64_t loader_seed,
                                                       uint64_t epoch, int32_t *__restrict__ crops,
                                                       int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_crop_transform(k, ids[k], H, W, rg.scale, rg.ratio, loader_seed, epoch, crops);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

FFCV_HD bool crop_ok(int i, int j, int h, int w, int H, int W) {
  return h > 0 && w > 0 && i >= 0 && j >= 0 && (int64_t)i + h <= H && (int64_t)j + w <= W;
}

// 16-byte chunks of one LDS row: the aligned chunks that can hold bytes of a
// crop row of w pixels at any alignment
FFCV_HD int row_chunks(int w) { return lds_chunks(3 * w); }
// LDS bytes of the staged source of an H x W image (any crop of it), plus the
// pixel reads' look-ahead (two aligned dwords per pixel: up to 5 bytes past it)
static uint64_t lds_src_bytes(int H, int W) { return (uint64_t)H * row_chunks(W) * 16 + 16; }

// the whole crop's staged rows (resize_out.h, r0 = 0); every read is a pixel's two aligned dwords
typedef StagedRows<true> ImgLds;

// One workgroup per image.  Dynamic LDS: [staged rows | taps | LUT].
//   Validation: an invalid crop's image is not read; its output row is
//   zero-filled and its status FFCV_SAMPLE_RANGE.
//   Staging: the crop's rows with 16-byte aligned global loads (only aligned
//   words holding a byte of a crop row), four loads in flight per thread; the
//   out_w column and out_h row taps are computed while the first loads fly.
//   Pixels: the shared per-pixel functions (device_common.h) over the LDS
//   rows, four adjacent pixels per thread leaving as one 12-byte (u8) or three
//   8-byte (fp16) stores where out_w and the output's alignment allow; linear
//   crops (some axis upscaled: most crops of a small image) walk rows with
//   the two source rows' horizontal sums in registers, bit-exact with
//   resize_linear.
template <bool FP16>
__global__ void __launch_bounds__(RRCI_THREADS)
    rrc_images_kernel(const uint8_t *__restrict__ in, uint64_t in_stride, int H, int W,
                      const int32_t *__restrict__ crops, const int32_t *__restrict__ cut,
                      const uint8_t *__restrict__ flips, ffcv_rrc_params p, uint64_t stride, void *__restrict__ out,
                      int32_t *__restrict__ status, int src_cap) {
  extern __shared__ uint4 smem[];
  typedef uint32_t sx4_t __attribute__((ext_vector_type(4)));
  const int t = threadIdx.x, k = blockIdx.x;
  const int out_w = p.out_w, out_h = p.out_h;
  sx4_t *s_src = (sx4_t *)smem;
  uint8_t *s_tap = (uint8_t *)smem + src_cap;
  uint16_t *s_lut = (uint16_t *)(s_tap + (out_w + out_h) * RRCI_TAP_BYTES);
  const int ci = crops[4 * k], cj = crops[4 * k + 1], chh = crops[4 * k + 2], cww = crops[4 * k + 3];
  char *o = (char *)out + stride * k;
  if (!crop_ok(ci, cj, chh, cww, H, W)) {  // (the same for the whole workgroup)
    const uint32_t dense = (uint32_t)out_h * out_w * 3 * (FP16 ? 2 : 1);
    for (uint32_t i = t; i < dense; i += RRCI_THREADS) o[i] = 0;
    if (status && t == 0) status[k] = FFCV_SAMPLE_RANGE;
    return;
  }
  if (status && t == 0) status[k] = FFCV_SAMPLE_OK;

  // ---- stage the crop's rows
  const uint64_t step = (uint64_t)W * 3;
  const uint64_t src0 = (uint64_t)(uintptr_t)in + (uint64_t)k * in_stride + ((uint64_t)ci * W + cj) * 3;
  const int nch = row_chunks(cww);
  const int total = chh * nch;  // <= H * row_chunks(W): inside src_cap
  ImgLds L{(const uint8_t *)s_src, nch * 16, (int)(src0 & 15), (int)(step & 15), 0};
  const ResizePlan P = make_plan(cww, chh, out_w, out_h);
  bool first = true;
  for (int b0 = t; b0 < total || first; b0 += 4 * RRCI_THREADS) {
    sx4_t v[4] = {};
    int di[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int idx = b0 + q * RRCI_THREADS;
      di[q] = -1;
      if (idx < total) {
        const int r = idx / nch, c = idx - r * nch;
        const uint64_t ra = src0 + (uint64_t)r * step;
        // chunks holding bytes of this row (none past the batch's last byte)
        const int lim = (int)(((ra & 15) + 3 * (uint64_t)cww + 15) >> 4);
        if (c < lim) {
          // (a global-address-space pointer: global_load_dwordx4, not a flat load)
          typedef const __attribute__((address_space(1))) sx4_t gx4_t;
          v[q] = ((gx4_t *)(uintptr_t)(ra & ~(uint64_t)15))[c];
          di[q] = idx;
        }
      }
    }
    if (first) {  // the image's taps, under the loads
      first = false;
      for (int i = t; i < out_w + out_h; i += RRCI_THREADS) {
        const bool col = i < out_w;
        const int d = col ? i : i - out_w;
        if (P.kind == 2)
          *(AreaTaps *)(s_tap + i * RRCI_TAP_BYTES) =
              area_taps(col ? P.sw : P.sh, col ? P.scale_x : P.scale_y, d);
        else if (P.kind == 3)
          *(LinTap *)(s_tap + i * RRCI_TAP_BYTES) =
              lin_tap(col ? P.scale_x : P.scale_y, col ? P.inv_x : P.inv_y, col ? P.sw : P.sh, d);
      }
      if (FP16) {
        for (int i = t; i < 768; i += RRCI_THREADS) s_lut[i] = p.lut[i];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (di[q] >= 0) s_src[di[q]] = v[q];
  }
  __syncthreads();

  // (in place: through make_epilogue this kernel grew by ten scalar instructions and its large
  // LDS-regime cases measured up to 0.7 % slower, profiles/rrc_split_ab.txt)
  Epilogue ep;
  ep.out_h = out_h;
  ep.out_w = out_w;
  ep.cut_size = cut ? p.cutout_size : 0;
  ep.cut_y = cut ? cut[2 * k] : 0;
  ep.cut_x = cut ? cut[2 * k + 1] : 0;
  ep.flip = flips ? flips[k] : 0;
  ep.cut_before_flip = p.cutout_fill[3];
  ep.fill[0] = p.cutout_fill[0];
  ep.fill[1] = p.cutout_fill[1];
  ep.fill[2] = p.cutout_fill[2];

  // output pixel (dy, dx): flip, cutout, then the resize of source column sx
  auto pixel = [&](int dy, int dx, int v[3]) {
    if (ep.in_cut(dy, dx)) {
      v[0] = ep.fill[0];
      v[1] = ep.fill[1];
      v[2] = ep.fill[2];
      return;
    }
    const int sx = ep.src_x(dx);
    if (P.kind == 3) {
      resize_linear(P, L, sx, *(const LinTap *)(s_tap + sx * RRCI_TAP_BYTES),
                    *(const LinTap *)(s_tap + (out_w + dy) * RRCI_TAP_BYTES), v);
    } else if (P.kind == 2) {
      resize_area_lds(L, *(const AreaTaps *)(s_tap + sx * RRCI_TAP_BYTES),
                      *(const AreaTaps *)(s_tap + (out_w + dy) * RRCI_TAP_BYTES), v);
    } else if (P.kind == 1) {  // resizeAreaFast: integer sums, one float multiply
      const int sy0 = dy * P.isy, sx0 = sx * P.isx;
      const float sc = 1.f / (float)(P.isx * P.isy);
      int s0 = 0, s1 = 0, s2 = 0;
      for (int yy = 0; yy < P.isy; yy++)
        for (int xx = 0; xx < P.isx; xx++) {
          const uint32_t w = L.px(sy0 + yy, sx0 + xx);
          s0 += (int)(w & 0xffu);
          s1 += (int)((w >> 8) & 0xffu);
          s2 += (int)((w >> 16) & 0xffu);
        }
      v[0] = sat_u8i(ffcv_f2i_rn((float)s0 * sc));
      v[1] = sat_u8i(ffcv_f2i_rn((float)s1 * sc));
      v[2] = sat_u8i(ffcv_f2i_rn((float)s2 * sc));
    } else {
      const uint32_t w = L.px(dy, sx);
      v[0] = (int)(w & 0xffu);
      v[1] = (int)((w >> 8) & 0xffu);
      v[2] = (int)((w >> 16) & 0xffu);
    }
  };

  const bool wide = (out_w & 3) == 0 && ((((uintptr_t)out) | stride) & (FP16 ? 7 : 3)) == 0;
  if (wide) {
    // four adjacent pixels as one 12-byte (u8) or three 8-byte (fp16) stores (store_quad)
    const int nq = out_w >> 2;
    if (P.kind == 3 && nq <= RRCI_THREADS) {
      // Linear walk (resize_linear in its separable form, as resize.cpp runs
      // it): a thread owns four adjacent columns and a run of consecutive
      // rows.  Its column taps stay in registers; the horizontal sums of the
      // two source rows of an output row (HA: the upper, HB: the lower) are
      // kept while the walk moves down, so most rows of an upscale compute one
      // new source row or none.
      const int groups = RRCI_THREADS / nq;
      const int per = (out_h + groups - 1) / groups;
      const int g = t / nq, q = t - g * nq;
      const int gy0 = g * per, gy1 = min(out_h, gy0 + per);
      if (g >= groups || gy0 >= gy1) return;
      const int dx0 = 4 * q;
      int xa[4], xb[4], wa[4], wb[4], e0[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int sx = ep.src_x(dx0 + j);
        const LinTap l = *(const LinTap *)(s_tap + sx * RRCI_TAP_BYTES);
        // a border tap (src[s] * 2048) as the two-tap form with weights (2048, 0)
        xa[j] = l.s;
        xb[j] = l.border ? l.s : l.s + 1;
        wa[j] = l.border ? 2048 : l.c0;
        wb[j] = l.border ? 0 : l.c1;
        e0[j] = 3 * sx;  // the element's index in the resized row: the vector body ends at vec_end
      }
      auto hrow = [&](int r, int Hh[12]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t pa = L.px(r, xa[j]), pb = L.px(r, xb[j]);
#pragma unroll
          for (int c = 0; c < 3; c++)
            Hh[3 * j + c] = (int)((pa >> (8 * c)) & 0xffu) * wa[j] + (int)((pb >> (8 * c)) & 0xffu) * wb[j];
        }
      };
      int HA[12], HB[12];
      int ca = -1, cb = -1;
      for (int dy = gy0; dy < gy1; dy++) {
        const LinTap ly = *(const LinTap *)(s_tap + (out_w + dy) * RRCI_TAP_BYTES);
        const int r0 = min(max(ly.s, 0), P.sh - 1), r1 = min(max(ly.s + 1, 0), P.sh - 1);
        if (r0 != ca) {
          if (r0 == cb) {
#pragma unroll
            for (int i = 0; i < 12; i++) HA[i] = HB[i];
          } else {
            hrow(r0, HA);
          }
          ca = r0;
        }
        if (r1 != cb) {
          hrow(r1, HB);
          cb = r1;
        }
        int v[12];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bool cutpx = ep.in_cut(dy, dx0 + j);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const int h0 = HA[3 * j + c], h1 = HB[3 * j + c];
            int r;
            if (e0[j] + c < P.vec_end) {  // VResizeLinearVec_32s8u (resize_linear's vector body)
              const int s0 = sat_s16i(h0 >> 4), s1 = sat_s16i(h1 >> 4);
              const int m0 = ffcv_mul24(s0, ly.c0) >> 16, m1 = ffcv_mul24(s1, ly.c1) >> 16;
              r = sat_u8i((sat_s16i(m0 + m1) + 2) >> 2);
            } else {  // its scalar tail
              r = sat_u8i((h0 * ly.c0 + h1 * ly.c1 + (1 << 21)) >> 22);
            }
            v[3 * j + c] = cutpx ? (int)ep.fill[c] : r;
          }
        }
        store_quad<FP16>(o, (uint64_t)dy * out_w + dx0, v, s_lut);
      }
      return;
    }
    const int nquads = out_h * nq;
    for (int i = t; i < nquads; i += RRCI_THREADS) {
      const int dy = i / nq, dx0 = 4 * (i - dy * nq);
      int v[12];
#pragma unroll
      for (int j = 0; j < 4; j++) pixel(dy, dx0 + j, v + 3 * j);
      store_quad<FP16>(o, (uint64_t)dy * out_w + dx0, v, s_lut);
    }
    return;
  }
  const int npx = out_h * out_w;
  for (int i = t; i < npx; i += RRCI_THREADS) {
    const int dy = i / out_w, dx = i - dy * out_w;
    int v[3];
    pixel(dy, dx, v);
    store_px<FP16>(o, (uint64_t)i, v, s_lut);
  }
}

// Band regime front end, one workgroup per image: the raw kernel's descriptor
// of image k (offset k * in_stride from `in`, raw mode) and a copy of its
// crop.  An invalid crop gets mode 0 (the band kernel skips the sample), the
// window (0, 0, 1, 1) for the taps kernel, a zero-filled output row and
// FFCV_SAMPLE_RANGE: the band kernel never sees it.
__global__ void __launch_bounds__(RRCI_THREADS)
    rrc_images_desc_kernel(uint64_t in_stride, int H, int W, const int32_t *__restrict__ crops,
                           ffcv_sample *__restrict__ samples, int32_t *__restrict__ crops_out, uint64_t stride,
                           uint32_t dense, void *__restrict__ out, int32_t *__restrict__ status) {
  const int t = threadIdx.x, k = blockIdx.x;
  const int ci = crops[4 * k], cj = crops[4 * k + 1], chh = crops[4 * k + 2], cww = crops[4 * k + 3];
  const bool ok = crop_ok(ci, cj, chh, cww, H, W);
  if (t == 0) {
    ffcv_sample s;
    s.offset = (uint64_t)k * in_stride;
    s.size = (uint64_t)H * W * 3;
    s.height = (uint32_t)H;
    s.width = (uint32_t)W;
    s.mode = ok ? 1u : 0u;
    s.reserved = 0;
    samples[k] = s;
    crops_out[4 * k + 0] = ok ? ci : 0;
    crops_out[4 * k + 1] = ok ? cj : 0;
    crops_out[4 * k + 2] = ok ? chh : 1;
    crops_out[4 * k + 3] = ok ? cww : 1;
    if (status) status[k] = ok ? FFCV_SAMPLE_OK : FFCV_SAMPLE_RANGE;
  }
  if (!ok) {
    char *o = (char *)out + stride * k;
    for (uint32_t i = t; i < dense; i += RRCI_THREADS) o[i] = 0;
  }
}

namespace {

uint64_t a256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

// dynamic LDS of an LDS-regime launch, or 0 when the launch runs the band regime
uint64_t lds_launch_bytes(int H, int W, int out_h, int out_w, bool fp16) {
  const uint64_t src = lds_src_bytes(H, W);
  if (src > RRCI_LDS_BYTES) return 0;
  const uint64_t all = src + ((uint64_t)out_h + out_w) * RRCI_TAP_BYTES + (fp16 ? 1536 : 0);
  return all <= RRCI_LDS_MAX ? all : 0;  // (an output of ~1,500 rows + columns or more: its taps do not fit)
}

bool draw_args_ok(const void *ids, int batch, int height, int width, const double *scale, const double *ratio,
                  const void *crops) {
  if (!ids || !crops || !scale || !ratio || batch < 0 || height <= 0 || width <= 0 || height > 65535 ||
      width > 65535)
    return false;
  for (int i = 0; i < 2; i++)
    if (!std::isfinite(scale[i]) || !std::isfinite(ratio[i]) || scale[i] < 0 || ratio[i] <= 0) return false;
  return true;
}

}  // namespace

extern "C" {

uint64_t ffcv_rrc_images_lds_bytes(void) { return RRCI_LDS_BYTES; }

int ffcv_crop_draw_batch(void *stream, const uint64_t *sample_ids, int batch, int height, int width,
                         const double scale[2], const double ratio[2], uint64_t loader_seed, uint64_t epoch,
                         int32_t *crops, int32_t *status) {
  if (!draw_args_ok(sample_ids, batch, height, width, scale, ratio, crops)) {
    ffcv::set_error("ffcv_crop_draw_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  const CropRanges rg{{scale[0], scale[1]}, {ratio[0], ratio[1]}};
  return ffcv::launch_draw("crop_draw_kernel", crop_draw_kernel, stream, batch, sample_ids, batch, (uint32_t)height,
                           (uint32_t)width, rg, loader_seed, epoch, crops, status);
}

int ffcv_crop_draw_batch_host(const uint64_t *sample_ids, int batch, int height, int width, const double scale[2],
                              const double ratio[2], uint64_t loader_seed, uint64_t epoch, int32_t *crops,
                              int32_t *status) {
  if (!draw_args_ok(sample_ids, batch, height, width, scale, ratio, crops)) {
    ffcv::set_error("ffcv_crop_draw_batch_host: invalid arguments");
    return FFCV_EINVAL;
  }
  for (int k = 0; k < batch; k++) {
    const int err = draw_crop_transform(k, sample_ids[k], (uint32_t)height, (uint32_t)width, scale, ratio,
                                        loader_seed, epoch, crops);
    if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
  }
  return FFCV_OK;
}

static uint64_t band_workspace_bytes(int batch, int out_h, int out_w) {
  return a256((uint64_t)batch * sizeof(ffcv_sample)) + a256((uint64_t)batch * 16) +
         ffcv_rrc_raw_workspace_bytes(batch, out_h, out_w);
}

uint64_t ffcv_rrc_images_workspace_bytes(int batch, int height, int width, int out_h, int out_w) {
  if (batch <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0) return 0;
  if (lds_launch_bytes(height, width, out_h, out_w, true)) return 0;
  return band_workspace_bytes(batch, out_h, out_w);
}

// regime 0: chosen from the sizes; 1 / 2: the LDS / the band regime whatever
// the cutover says (measurement: tools/rrc_transform_bench.py)
static int rrc_images_launch(void *stream, const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                             const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                             const ffcv_rrc_params *p, void *out, int32_t *status, void *workspace,
                             uint64_t workspace_bytes, int regime) {
  if (!in || !crops || !p || !out || batch < 0 || height <= 0 || width <= 0 || height > 65535 || width > 65535) {
    ffcv::set_error("ffcv_rrc_images_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (p->out_h <= 0 || p->out_w <= 0 || p->out_h > 65535 || p->out_w > 65535) {
    ffcv::set_error("ffcv_rrc_images_batch: output size %dx%d", p->out_h, p->out_w);
    return FFCV_EINVAL;
  }
  const uint64_t img = (uint64_t)height * width * 3;
  if (in_stride < img) {
    ffcv::set_error("ffcv_rrc_images_batch: in_stride %llu for images of %llu bytes", (unsigned long long)in_stride,
                    (unsigned long long)img);
    return FFCV_EINVAL;
  }
  if (cutout_yx && p->cutout_size > 0 && (p->cutout_size > p->out_h || p->cutout_size > p->out_w)) {
    ffcv::set_error("ffcv_rrc_images_batch: cutout_size %d exceeds output %dx%d", p->cutout_size, p->out_h,
                    p->out_w);
    return FFCV_EINVAL;
  }
  const bool fp16 = p->lut != nullptr;
  const uint64_t dense = (uint64_t)p->out_h * p->out_w * 3 * (fp16 ? 2 : 1);
  const uint64_t stride = p->out_stride ? p->out_stride : dense;
  if (stride < dense || (fp16 && ((((uintptr_t)out) | stride) & 1))) {
    ffcv::set_error("ffcv_rrc_images_batch: out_stride %llu for images of %llu bytes (fp16: 2-byte aligned)",
                    (unsigned long long)stride, (unsigned long long)dense);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  {  // the two ranges must not overlap
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uint64_t)(batch - 1) * in_stride + img;
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uint64_t)(batch - 1) * stride + dense;
    if (a0 < b1 && b0 < a1) {
      ffcv::set_error("ffcv_rrc_images_batch: in and out overlap");
      return FFCV_EINVAL;
    }
  }
  uint64_t lds = regime == 2 ? 0 : lds_launch_bytes(height, width, p->out_h, p->out_w, fp16);
  if (regime == 1) {
    lds = lds_src_bytes(height, width) + ((uint64_t)p->out_h + p->out_w) * RRCI_TAP_BYTES + (fp16 ? 1536 : 0);
    if (lds > RRCI_LDS_MAX) {
      ffcv::set_error("ffcv_rrc_images_batch_regime: %llu bytes of LDS needed", (unsigned long long)lds);
      return FFCV_EINVAL;
    }
  }
  const uint64_t need = lds ? 0 : band_workspace_bytes(batch, p->out_h, p->out_w);
  if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) {
    ffcv::set_error("ffcv_rrc_images_batch: workspace of %llu bytes (16-byte aligned) needed, got %llu",
                    (unsigned long long)need, (unsigned long long)(workspace ? workspace_bytes : 0));
    return FFCV_EINVAL;
  }
  hipStream_t s = ffcv::as_stream(stream);
  if (lds) {
    const int src_cap = (int)lds_src_bytes(height, width);
    if (fp16)
      hipLaunchKernelGGL(rrc_images_kernel<true>, dim3(batch), dim3(RRCI_THREADS), (size_t)lds, s, in, in_stride,
                         height, width, crops, cutout_yx, flips, *p, stride, out, status, src_cap);
    else
      hipLaunchKernelGGL(rrc_images_kernel<false>, dim3(batch), dim3(RRCI_THREADS), (size_t)lds, s, in, in_stride,
                         height, width, crops, cutout_yx, flips, *p, stride, out, status, src_cap);
    FFCV_LAUNCH_CHECK("rrc_images_kernel");
    return FFCV_OK;
  }
  ffcv_sample *samples = (ffcv_sample *)workspace;
  int32_t *wcrops = (int32_t *)((uint8_t *)workspace + a256((uint64_t)batch * sizeof(ffcv_sample)));
  uint8_t *raw_ws = (uint8_t *)wcrops + a256((uint64_t)batch * 16);
  hipLaunchKernelGGL(rrc_images_desc_kernel, dim3(batch), dim3(RRCI_THREADS), 0, s, in_stride, height, width, crops,
                     samples, wcrops, stride, (uint32_t)dense, out, status);
  FFCV_LAUNCH_CHECK("rrc_images_desc_kernel");
  ffcv_rrc_params q = *p;
  q.out_stride = stride;
  if (!cutout_yx) q.cutout_size = 0;
  return ffcv_rrc_raw_batch_ws(stream, in, samples, batch, wcrops, cutout_yx, flips, &q, out, raw_ws,
                               ffcv_rrc_raw_workspace_bytes(batch, p->out_h, p->out_w));
}

int ffcv_rrc_images_batch(void *stream, const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                          const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                          const ffcv_rrc_params *p, void *out, int32_t *status, void *workspace,
                          uint64_t workspace_bytes) {
  return rrc_images_launch(stream, in, in_stride, batch, height, width, crops, cutout_yx, flips, p, out, status,
                           workspace, workspace_bytes, 0);
}

// Measurement hook (not in ffcv_hip.h): ffcv_rrc_images_batch in a given
// regime (1: LDS, 2: band with a workspace of a band launch's size).
int ffcv_rrc_images_batch_regime(void *stream, const uint8_t *in, uint64_t in_stride, int batch, int height,
                                 int width, const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                                 const ffcv_rrc_params *p, void *out, int32_t *status, void *workspace,
                                 uint64_t workspace_bytes, int regime) {
  if (regime < 0 || regime > 2) {
    ffcv::set_error("ffcv_rrc_images_batch_regime: regime %d", regime);
    return FFCV_EINVAL;
  }
  return rrc_images_launch(stream, in, in_stride, batch, height, width, crops, cutout_yx, flips, p, out, status,
                           workspace, workspace_bytes, regime);
}

int ffcv_rrc_images_batch_host(const uint8_t *in, uint64_t in_stride, int batch, int height, int width,
                               const int32_t *crops, int out_h, int out_w, uint8_t *out, uint64_t out_stride,
                               int32_t *status, int nthreads) {
  if (!in || !crops || !out || batch < 0 || height <= 0 || width <= 0 || height > 65535 || width > 65535 ||
      out_h <= 0 || out_w <= 0 || out_h > 65535 || out_w > 65535) {
    ffcv::set_error("ffcv_rrc_images_batch_host: invalid arguments");
    return FFCV_EINVAL;
  }
  const uint64_t img = (uint64_t)height * width * 3, dense = (uint64_t)out_h * out_w * 3;
  const uint64_t stride = out_stride ? out_stride : dense;
  if (in_stride < img || stride < dense) {
    ffcv::set_error("ffcv_rrc_images_batch_host: in_stride %llu / out_stride %llu for images of %llu / %llu bytes",
                    (unsigned long long)in_stride, (unsigned long long)stride, (unsigned long long)img,
                    (unsigned long long)dense);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  {
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uint64_t)(batch - 1) * in_stride + img;
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uint64_t)(batch - 1) * stride + dense;
    if (a0 < b1 && b0 < a1) {
      ffcv::set_error("ffcv_rrc_images_batch_host: in and out overlap");
      return FFCV_EINVAL;
    }
  }
  ffcv::host_threads(nthreads, batch, [&](std::atomic<uint64_t> &next, int, int) {
    for (int k = (int)next.fetch_add(1); k < batch; k = (int)next.fetch_add(1)) {
      const int32_t *c = crops + 4 * k;
      uint8_t *dst = out + (uint64_t)k * stride;
      if (!crop_ok(c[0], c[1], c[2], c[3], height, width)) {
        std::fill(dst, dst + dense, (uint8_t)0);
        if (status) status[k] = FFCV_SAMPLE_RANGE;
        continue;
      }
      resize(0, (int64_t)(uintptr_t)(in + (uint64_t)k * in_stride), height, width, c[0], (int64_t)c[0] + c[2], c[1],
             (int64_t)c[1] + c[3], (int64_t)(uintptr_t)dst, out_h, out_w);
      if (status) status[k] = FFCV_SAMPLE_OK;
    }
  });
  return FFCV_OK;
}

}  // extern "C"
