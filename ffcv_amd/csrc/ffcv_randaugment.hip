// ffcv_randaugment.hip -- RandAugment: the draws (op id 23)
// and the fused pixel pass for images up to 64 x 64, with the draws' host twin.
//
// A sample runs num_ops operations of the 14 of s24 in sequence, each on the
// uint8 result of the one before, all at one fixed strength bin.
//
//   draws: one lane per sample; slot s of a sample draws (op, neg), always
//     both, and fills slot s's slice of every array exactly as
//     ffcv_policy_draw_batch fills the whole array, so the pixel entries of s24
//     take a slot's slices unchanged (the rounds path, and the host path).
//
//   randaugment_kernel: one 256-thread workgroup per image.  The image is
//     staged as bytes in LDS once (16-byte aligned loads at any alignment of
//     src, lds_stage.h), every slot's operation runs there, and the result
//     leaves once (16-byte aligned stores at any alignment of dst).  A slot's
//     operation is read once per workgroup (a uniform branch):
//       brightness / contrast / solarize / posterize: a 256-entry table of the
//         image, then a byte map over whole words; contrast's gray sum is
//         reduced in the workgroup;
//       colour (saturation): per pixel;
//       autocontrast / equalize: the three channels' histograms in 768 LDS
//         counters, their tables, a byte map by channel;
//       shear / translate / rotate, sharpness: from the current image buffer
//         into the second one, which becomes the current.
//     The arithmetic is that of color_common.h, tone_common.h, affine_common.h
//     and sharpness_common.h: the bytes equal those of the s24 launches, slot
//     after slot.
//
// LDS: two image buffers of 12,288 B + 64 B (16 in front for a tap left of
// column 0, 16 for the staged range's lead, 32 of read-ahead) = 24,704, the
// counters 3,072, the tables 768, scan partials 144: 28,688 bytes, five
// workgroups per CU.
#include "affine_common.h"
#include "api_internal.h"
#include "color_common.h"
#include "lds_stage.h"
#include "sharpness_common.h"
#include "tone_common.h"

#define FFCV_RANDAUG_OP 23
#define RA_NOPS 14
#define RA_MAX_SLOTS 8
#define RA_THREADS 256
#define RA_LDS_BYTES 24576                 // the fused regime: 6 H W at most this
#define RA_IMG_BYTES (RA_LDS_BYTES / 2)    // one image, at most
#define RA_BUF_CHUNKS (1 + RA_IMG_BYTES / 16 + 1 + 2)
#define RA_BUF_BYTES (16 * RA_BUF_CHUNKS)

// the 14 operations, in the order of the value table's rows
enum {
  RA_IDENTITY = 0, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y, RA_ROTATE, RA_BRIGHTNESS, RA_COLOR,
  RA_CONTRAST, RA_SHARPNESS, RA_POSTERIZE, RA_SOLARIZE, RA_AUTOCONTRAST, RA_EQUALIZE
};

// the arrays of ffcv_policy_draw_batch, each with a leading slot dimension
struct RaArrays {
  uint8_t *op, *cj_apply;
  double *cj_ratio;
  uint8_t *tone_apply, *tone_bits, *aff_apply;
  int64_t *aff_coef;
  uint8_t *sharp_apply;
  float *sharp_factor;
  bool complete() const {
    return op && cj_apply && cj_ratio && tone_apply && tone_bits && aff_apply && aff_coef && sharp_apply &&
           sharp_factor;
  }
};

// One sample's draws, two per slot and always both, and every launch's
// arguments for every slot.  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_randaugment(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, int num_ops, int nbins,
                              int magnitude, const double *table, int H, int W, const RaArrays &o) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_RANDAUG_OP));
  const uint64_t uk = (uint64_t)k, uB = (uint64_t)B;
  // the draws first, unrolled: the stream's position is then a constant at every
  // draw, and its slow path (beyond 227 words) is never compiled in.  Slot s's
  // (op, neg) in byte s.
  uint64_t drawn = 0;
#pragma unroll
  for (int s = 0; s < RA_MAX_SLOTS; s++) {
    if (s >= num_ops) break;
    const double u0 = mt_double(m), u1 = mt_double(m);
    const uint32_t op = (uint32_t)min(RA_NOPS - 1, (int)cj_mul(u0, (double)RA_NOPS));
    drawn |= (uint64_t)(op | (u1 < 0.5 ? 16u : 0u)) << (8 * s);
  }
  for (int s = 0; s < num_ops; s++) {
    const int op = (int)((drawn >> (8 * s)) & 15u);
    const bool neg = ((drawn >> (8 * s)) & 16u) != 0;
    const double v = table[op * nbins + magnitude];
    const double sv = neg && op >= RA_SHEAR_X && op <= RA_SHARPNESS ? -v : v;
    const double ratio = cj_add(1.0, sv);
    const uint64_t sk = (uint64_t)s * uB + uk;  // the sample in slot s's slice of a [B] array
    o.op[sk] = (uint8_t)op;

    // colour programs: brightness, saturation, contrast | solarize
    const int cj_op[4] = {RA_BRIGHTNESS, RA_COLOR, RA_CONTRAST, RA_SOLARIZE};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool on = op == cj_op[i];
      const uint64_t at = (4u * (uint64_t)s + i) * uB + uk;
      o.cj_apply[at] = (uint8_t)on;
      o.cj_ratio[at] = i == 3 ? (on ? v : 256.0) : (on ? ratio : 1.0);
    }
    // tone program: posterize, autocontrast, equalize
    o.tone_apply[(3u * (uint64_t)s + 0) * uB + uk] = (uint8_t)(op == RA_POSTERIZE);
    o.tone_apply[(3u * (uint64_t)s + 1) * uB + uk] = (uint8_t)(op == RA_AUTOCONTRAST);
    o.tone_apply[(3u * (uint64_t)s + 2) * uB + uk] = (uint8_t)(op == RA_EQUALIZE);
    o.tone_bits[sk] = op == RA_POSTERIZE ? (uint8_t)(v < 1.0 ? 1.0 : (v > 8.0 ? 8.0 : v)) : (uint8_t)8;
    // affine: the one non-zero argument, scale 1
    o.aff_apply[sk] = (uint8_t)(op >= RA_SHEAR_X && op <= RA_ROTATE);
    affine_matrix(op == RA_ROTATE ? sv : 0.0, op == RA_TRANSLATE_X ? sv : 0.0, op == RA_TRANSLATE_Y ? sv : 0.0, 1.0,
                  op == RA_SHEAR_X ? sv : 0.0, op == RA_SHEAR_Y ? sv : 0.0, H, W, o.aff_coef + 6 * sk);
    // sharpness: every other image is left to the launches before it
    o.sharp_apply[sk] = op == RA_SHARPNESS ? (uint8_t)1 : (uint8_t)2;
    o.sharp_factor[sk] = op == RA_SHARPNESS ? (float)ratio : 1.0f;
  }
  return m.err;
}

__global__ void __launch_bounds__(64)
    randaugment_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed, uint64_t epoch, int num_ops,
                            int nbins, int magnitude, const double *__restrict__ table, int H, int W, RaArrays o,
                            int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  // (the nine pointers are live across the slots' loop, whose trigonometry is
  // full of scalar constants: kept in scalar registers they spill; vector
  // registers are plentiful here)
  asm volatile(""
               : "+v"(o.op), "+v"(o.cj_apply), "+v"(o.cj_ratio), "+v"(o.tone_apply), "+v"(o.tone_bits),
                 "+v"(o.aff_apply), "+v"(o.aff_coef), "+v"(o.sharp_apply), "+v"(o.sharp_factor));
  const int err = draw_randaugment(k, B, ids[k], loader_seed, epoch, num_ops, nbins, magnitude, table, H, W, o);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// Taps from the image in LDS, H x W x 3 dense from `img` on (any alignment;
// the buffer keeps the read-ahead of lds_pixel); T: the coordinates' type.
struct RaTap {
  const uint8_t *img;
  int H, W;
  uint32_t fill;
  template <class T>
  FFCV_DEV uint32_t one(T iy, T ix) const {
    const bool ok = iy >= 0 && iy < (T)H && ix >= 0 && ix < (T)W;
    const uint32_t at = ok ? 3u * ((uint32_t)iy * (uint32_t)W + (uint32_t)ix) : 0u;
    const uint32_t v = lds_pixel(img + at) & 0xffffffu;  // read either way: no LDS read inside a branch
    return ok ? v : fill;
  }
  template <class T>
  FFCV_DEV void pair(T iy, T ix, uint32_t *a, uint32_t *b) const {
    *a = one(iy, ix);
    *b = one(iy, (T)(ix + 1));
  }
};

// The image's pixels, four adjacent ones per thread and step, as three aligned
// dwords into dense output bytes (s_out is 4-byte aligned).  The last group may
// run up to three pixels past the image: pix(r, c) is safe at any (r, c), and
// their bytes land in the buffer's slack.
template <class F>
FFCV_DEV void ra_groups(int t, int npix, int W, uint32_t *s_out, F pix) {
  for (int g = t; 4 * g < npix; g += RA_THREADS) {
    int r = (4 * g) / W, c = 4 * g - r * W;
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      v[e] = pix(r, c);
      c++;
      if (c == W) {
        c = 0;
        r++;
      }
    }
    s_out[3 * g + 0] = v[0] | (v[1] << 24);
    s_out[3 * g + 1] = (v[1] >> 8) | (v[2] << 16);
    s_out[3 * g + 2] = (v[2] >> 16) | (v[3] << 8);
  }
}

// the ten bytes from LDS address p on (any alignment) as three dwords
struct RaTen {
  uint32_t w0, w1, w2;
  FFCV_DEV explicit RaTen(const uint8_t *p) {
    const uint32_t *q = (const uint32_t *)__builtin_align_down(p, 4);
    const uint32_t sh = (uint32_t)(p - (const uint8_t *)q);
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    w0 = __builtin_amdgcn_alignbyte(q1, q0, sh);
    w1 = __builtin_amdgcn_alignbyte(q2, q1, sh);
    w2 = __builtin_amdgcn_alignbyte(q3, q2, sh);
  }
  FFCV_DEV float f(int e) const {  // byte e as a float (e is a constant after unrolling)
    const uint32_t w = e < 4 ? w0 : (e < 8 ? w1 : w2);
    return (float)((w >> (8 * (e & 3))) & 0xffu);
  }
};

// the kernel's view of the draws' arrays
struct RaIn {
  const uint8_t *op;
  const double *cj_ratio;
  const uint8_t *tone_bits;
  const int64_t *aff_coef;
  const float *sharp_factor;
};

__global__ void __launch_bounds__(RA_THREADS)
    randaugment_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int B, int H0, int W0, int num_ops,
                       int mode, uint32_t fill0, RaIn A) {
  __shared__ lds_x4_t s_buf[2 * RA_BUF_CHUNKS];  // two image buffers
  __shared__ uint32_t s_hist[3 * 256];           // the channel histograms
  __shared__ uint8_t s_tab[3 * 256];             // the slot's table: one, or one per channel
  __shared__ uint32_t s_part[3][RA_THREADS / 64];
  __shared__ uint64_t s_occ[3][RA_THREADS / 64];
  const int t0 = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const uint32_t nbytes0 = 3u * (uint32_t)H0 * (uint32_t)W0;  // <= RA_IMG_BYTES
  uint8_t *const s_mem = (uint8_t *)s_buf;

  // ---- stage the image: one byte range, behind buffer 0's 16 front bytes
  const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * nbytes0;
  stage_rows<RA_THREADS>(t0, src0, 0, 1, nbytes0, (int)lds_chunks(nbytes0), s_buf + 1);
  uint32_t cb = 0;                                // the buffer that holds the current image ...
  uint32_t cur_off = 16u + (uint32_t)(src0 & 15);  // ... and where in s_mem its first byte is
  __syncthreads();

  for (int s = 0; s < num_ops; s++) {
    // (the thread index, the sizes and fill pass through an empty asm in every
    // slot: what all the branches below derive from them -- per-thread
    // predicates, addresses, reciprocals -- would otherwise be hoisted out of
    // this loop, live across it in scalar registers, and spill)
    int t = t0, H = H0, W = W0;
    uint32_t fill = fill0;
    asm volatile("" : "+v"(t), "+s"(H), "+s"(W), "+s"(fill));
    const int lane = t & 63, wave = t >> 6, rowb = 3 * W;
    const uint32_t npix = (uint32_t)H * (uint32_t)W, nbytes = 3u * npix;
    // the gray sum of the image at `img` (fits 32 bits: 4096 * 254), in every thread
    auto gray_sum = [&](const uint8_t *img) -> uint32_t {
      uint32_t s = 0;
      for (uint32_t q = t; q < npix; q += RA_THREADS) {
        const uint32_t v = lds_pixel(img + 3u * q);
        s += cj_gray(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu);
      }
      for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
      if (lane == 0) s_part[0][wave] = s;
      __syncthreads();
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < RA_THREADS / 64; w++) total += s_part[0][w];
      return total;
    };
    // every whole word that covers the image's bytes through s_tab: one table, or
    // one per channel (the channel of a byte is its offset in the image % 3).
    // The bytes around the image in those words are slack.
    auto map_words = [&](uint8_t *img, bool by_channel) {
      uint32_t *w0 = (uint32_t *)__builtin_align_down(img, 4);
      const uint32_t lead = (uint32_t)(img - (uint8_t *)w0), nw = (lead + nbytes + 3u) >> 2;
      for (uint32_t w = t; w < nw; w += RA_THREADS) {
        const uint32_t v = w0[w];
        const uint32_t c = by_channel ? (4u * w + 3u - lead) % 3u : 0u;  // the channel of the word's first byte
        const uint32_t o0 = by_channel ? c * 256u : 0u, o1 = by_channel ? (c == 2u ? 0u : c + 1u) * 256u : 0u,
                       o2 = by_channel ? (c == 0u ? 2u : c - 1u) * 256u : 0u;
        w0[w] = (uint32_t)s_tab[o0 + (v & 0xffu)] | ((uint32_t)s_tab[o1 + ((v >> 8) & 0xffu)] << 8) |
                ((uint32_t)s_tab[o2 + ((v >> 16) & 0xffu)] << 16) | ((uint32_t)s_tab[o0 + (v >> 24)] << 24);
      }
    };
    const uint64_t sk = (uint64_t)s * (uint32_t)B + k;
    // (a byte load lands in a vector register: readfirstlane makes the branch scalar)
    const int op = __builtin_amdgcn_readfirstlane((int)A.op[sk]);
    uint8_t *cur = s_mem + cur_off;
    const uint32_t nxt_off = (1u - cb) * RA_BUF_BYTES + 16u;  // dense, 16-byte aligned, in the other buffer
    uint8_t *nxt = s_mem + nxt_off;

    if (op >= RA_SHEAR_X && op <= RA_ROTATE) {
      // ---- the warp of ffcv_affine_batch on a whole image: coefficients out of
      // bounds or a footprint that misses the image give an image of fill
      int64_t q[6];
#pragma unroll
      for (int i = 0; i < 6; i++) q[i] = A.aff_coef[sk * 6 + i];
      const bool ok = affine_coef_ok(q);
      if (!ok) {  // keep the footprint's arithmetic inside 64 bits
#pragma unroll
        for (int i = 0; i < 6; i++) q[i] = 0;
      }
      const AffineBox box = affine_box(q, mode, H, W, 0, 0, W, H, true);
      const RaTap tap{cur, H, W, fill};
      if (!ok || box.empty()) {
        ra_groups(t, (int)npix, W, (uint32_t *)nxt, [&](int, int) -> uint32_t { return fill; });
      } else if (box.fits32) {
        // 32-bit coordinates relative to the image's corner: the true values fit
        // (box.fits32), so wrapping arithmetic gives them exactly
        const uint32_t X0 = (uint32_t)box.X0, Y0 = (uint32_t)box.Y0, q0 = (uint32_t)q[0], q1 = (uint32_t)q[1],
                       q3 = (uint32_t)q[3], q4 = (uint32_t)q[4];
        ra_groups(t, (int)npix, W, (uint32_t *)nxt, [&](int r, int c) -> uint32_t {
          const uint32_t X = X0 + q0 * (uint32_t)c + q1 * (uint32_t)r, Y = Y0 + q3 * (uint32_t)c + q4 * (uint32_t)r;
          return affine_sample<int32_t>(mode, (int32_t)X, (int32_t)Y, tap);
        });
      } else {
        ra_groups(t, (int)npix, W, (uint32_t *)nxt, [&](int r, int c) -> uint32_t {
          return affine_sample<int64_t>(mode, affine_x(q, c, r), affine_y(q, c, r), tap);
        });
      }
      cb = 1u - cb;
      cur_off = nxt_off;
      __syncthreads();
    } else if (op == RA_SHARPNESS) {
      // ---- ffcv_sharpness_batch's stencil: four adjacent bytes of a row per
      // thread and step, from the ten bytes [b - 3, b + 7) of three rows; a byte
      // on the image's outermost ring takes d = i through the same code
      const float a = A.sharp_factor[sk];
      const int ng = (rowb + 3) >> 2;
      for (int i = t; i < H * ng; i += RA_THREADS) {
        const int y = i / ng, b0 = 4 * (i - y * ng);
        const RaTen up(cur + max(y - 1, 0) * rowb + b0 - 3);
        const RaTen ce(cur + y * rowb + b0 - 3);
        const RaTen dn(cur + min(y + 1, H - 1) * rowb + b0 - 3);
        float pu[10], pc[10], pd[10];
#pragma unroll
        for (int e = 0; e < 10; e++) {
          pu[e] = blur_mul(up.f(e), SHARP_W1);
          pc[e] = blur_mul(ce.f(e), SHARP_W1);
          pd[e] = blur_mul(dn.f(e), SHARP_W1);
        }
        const bool edge_row = y == 0 || y == H - 1;
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float v = ce.f(j + 3);
          const float top = sharp_row(pu[j], pu[j + 3], pu[j + 6]);
          const float mid = sharp_row(pc[j], blur_mul(v, SHARP_W5), pc[j + 6]);
          const float bot = sharp_row(pd[j], pd[j + 3], pd[j + 6]);
          const bool border = edge_row || b0 + j < 3 || b0 + j >= rowb - 3;
          o[j] = sharp_blend(a, border ? v : sharp_smooth(top, mid, bot), v);
        }
        const int ob = y * rowb + b0;
        if (!(ob & 3) && b0 + 4 <= rowb) {
          *(uint32_t *)(nxt + ob) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (b0 + j < rowb) nxt[ob + j] = (uint8_t)o[j];
        }
      }
      cb = 1u - cb;
      cur_off = nxt_off;
      __syncthreads();
    } else if (op == RA_COLOR) {
      // ---- saturation, per pixel
      const double r = A.cj_ratio[(4u * (uint64_t)s + 1u) * (uint32_t)B + k];
      const double omr = cj_one_minus(r);
      for (uint32_t p = t; p < npix; p += RA_THREADS) {
        uint8_t *o = cur + 3u * p;
        const uint32_t v = lds_pixel(o);
        const uint32_t c0 = v & 0xffu, c1 = (v >> 8) & 0xffu, c2 = (v >> 16) & 0xffu;
        const double g = (double)cj_gray(c0, c1, c2);
        o[0] = (uint8_t)cj_blend(r, omr, c0, g);
        o[1] = (uint8_t)cj_blend(r, omr, c1, g);
        o[2] = (uint8_t)cj_blend(r, omr, c2, g);
      }
      __syncthreads();
    } else if (op == RA_BRIGHTNESS || op == RA_CONTRAST || op == RA_SOLARIZE || op == RA_POSTERIZE) {
      // ---- one 256-entry table of the image (RA_THREADS == 256), then a byte map
      if (op == RA_POSTERIZE) {
        const int bits = min(8, max(1, __builtin_amdgcn_readfirstlane((int)A.tone_bits[sk])));
        s_tab[t] = (uint8_t)tone_posterize(bits, (uint32_t)t);
      } else {
        const uint32_t row = op == RA_BRIGHTNESS ? 0u : (op == RA_CONTRAST ? 2u : 3u);
        const double r = A.cj_ratio[(4u * (uint64_t)s + row) * (uint32_t)B + k];
        const double omr = cj_one_minus(r);
        double other = 0.0;
        if (op == RA_CONTRAST) other = cj_mean((uint64_t)gray_sum(cur), (uint64_t)npix);
        s_tab[t] = (uint8_t)(op == RA_SOLARIZE ? cj_solarize(r, (uint32_t)t) : cj_blend(r, omr, (uint32_t)t, other));
      }
      __syncthreads();
      map_words(cur, false);
      __syncthreads();
    } else if (op == RA_AUTOCONTRAST || op == RA_EQUALIZE) {
      // ---- the channels' histograms, their tables (thread t owns bin t of the
      // three channels), a byte map by channel
      const int kind = op == RA_AUTOCONTRAST ? FFCV_TONE_AUTOCONTRAST : FFCV_TONE_EQUALIZE;
#pragma unroll
      for (int c = 0; c < 3; c++) s_hist[c * 256 + t] = 0u;
      __syncthreads();
      for (uint32_t p = t; p < npix; p += RA_THREADS) {
        const uint32_t v = lds_pixel(cur + 3u * p);
        atomicAdd(&s_hist[v & 0xffu], 1u);
        atomicAdd(&s_hist[256u + ((v >> 8) & 0xffu)], 1u);
        atomicAdd(&s_hist[512u + ((v >> 16) & 0xffu)], 1u);
      }
      __syncthreads();
      uint32_t h[3], incl[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        h[c] = s_hist[c * 256 + t];
        // per wave: which bins are occupied (ballot) and the inclusive sum (scan)
        const uint64_t occ = __ballot(h[c] != 0u);
        uint32_t sum = h[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = __shfl_up(sum, d, 64);
          if (lane >= d) sum += o;
        }
        incl[c] = sum;
        if (lane == 63) s_part[c][wave] = sum;
        if (lane == 0) s_occ[c][wave] = occ;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; c++) {
        uint32_t below = incl[c] - h[c], lo = 0u, hi = 0u;
#pragma unroll
        for (int w = 0; w < RA_THREADS / 64; w++) below += w < wave ? s_part[c][w] : 0u;
#pragma unroll
        for (int w = RA_THREADS / 64 - 1; w >= 0; w--) {
          const uint64_t occ = s_occ[c][w];
          if (occ) lo = 64u * w + (uint32_t)__builtin_ctzll(occ);
        }
#pragma unroll
        for (int w = 0; w < RA_THREADS / 64; w++) {
          const uint64_t occ = s_occ[c][w];
          if (occ) hi = 64u * w + 63u - (uint32_t)__builtin_clzll(occ);
        }
        s_tab[c * 256 + t] = (uint8_t)tone_entry(kind, 8, npix, lo, hi, s_hist[c * 256 + hi], below, (uint32_t)t);
      }
      __syncthreads();
      map_words(cur, true);
      __syncthreads();
    }
    // identity, or a code outside the 14: the image stays
  }

  // ---- write out once: the current image, at any alignment of dst
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * nbytes0;
  const uint8_t *out = s_mem + cur_off;
  write_back_rows<RA_THREADS>(t0, dst0, 0, 1, nbytes0, [&](int) { return out; });
}

namespace {

bool ra_draw_args_ok(const char *who, const void *ids, int batch, int num_ops, int nbins, int magnitude,
                     const void *table, int H, int W, const RaArrays &o) {
  if (batch < 0 || !ids || !table || !o.complete() || num_ops < 1 || num_ops > RA_MAX_SLOTS || nbins < 2 ||
      nbins > 256 || magnitude < 0 || magnitude >= nbins || H <= 0 || W <= 0 || H > FFCV_AFFINE_MAX_DIM ||
      W > FFCV_AFFINE_MAX_DIM) {
    ffcv::set_error("%s: invalid arguments (batch %d, %d operations of 1 to %d, bin %d of %d, %dx%d)", who, batch,
                    num_ops, RA_MAX_SLOTS, magnitude, nbins, H, W);
    return false;
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_randaugment_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed,
                                uint64_t epoch, int num_ops, int nbins, int magnitude, const double *table, int height,
                                int width, uint8_t *op, uint8_t *cj_apply, double *cj_ratio, uint8_t *tone_apply,
                                uint8_t *tone_bits, uint8_t *aff_apply, int64_t *aff_coef, uint8_t *sharp_apply,
                                float *sharp_factor, int32_t *status) {
  const RaArrays o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!ra_draw_args_ok("ffcv_randaugment_draw_batch", sample_ids, batch, num_ops, nbins, magnitude, table, height,
                       width, o))
    return FFCV_EINVAL;
  return ffcv::launch_draw("randaugment_draw_kernel", randaugment_draw_kernel, stream, batch, sample_ids, batch,
                           loader_seed, epoch, num_ops, nbins, magnitude, table, height, width, o, status);
}

int ffcv_randaugment_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                     int num_ops, int nbins, int magnitude, const double *table, int height,
                                     int width, uint8_t *op, uint8_t *cj_apply, double *cj_ratio, uint8_t *tone_apply,
                                     uint8_t *tone_bits, uint8_t *aff_apply, int64_t *aff_coef, uint8_t *sharp_apply,
                                     float *sharp_factor) {
  const RaArrays o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!ra_draw_args_ok("ffcv_randaugment_draw_batch_host", sample_ids, batch, num_ops, nbins, magnitude, table,
                       height, width, o))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_randaugment_draw_batch_host", batch, [&](int k) {
    return draw_randaugment(k, batch, sample_ids[k], loader_seed, epoch, num_ops, nbins, magnitude, table, height,
                            width, o);
  });
}

uint64_t ffcv_randaugment_lds_bytes(void) { return RA_LDS_BYTES; }

int ffcv_randaugment_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                           int num_ops, int mode, const uint8_t *fill, const uint8_t *op, const uint8_t *cj_apply,
                           const double *cj_ratio, const uint8_t *tone_apply, const uint8_t *tone_bits,
                           const uint8_t *aff_apply, const int64_t *aff_coef, const uint8_t *sharp_apply,
                           const float *sharp_factor) {
  const char *who = "ffcv_randaugment_batch";
  const bool pointers = fill && op && cj_apply && cj_ratio && tone_apply && tone_bits && aff_apply && aff_coef &&
                        sharp_apply && sharp_factor;
  uint64_t stride;
  if (!ffcv::out_of_place_ok(who, pointers, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM, 0, &stride))
    return FFCV_EINVAL;
  if (num_ops < 1 || num_ops > RA_MAX_SLOTS) {
    ffcv::set_error("%s: %d operations per sample, outside 1 to %d", who, num_ops, RA_MAX_SLOTS);
    return FFCV_EINVAL;
  }
  if (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) {
    ffcv::set_error("%s: mode %d is neither FFCV_AFFINE_BILINEAR nor FFCV_AFFINE_NEAREST", who, mode);
    return FFCV_EINVAL;
  }
  if ((uint64_t)height * width * 6u > RA_LDS_BYTES) {
    ffcv::set_error("%s: images of %dx%d exceed the fused regime (6 H W <= %d): run the slots' launches instead", who,
                    height, width, RA_LDS_BYTES);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  const RaIn A = {op, cj_ratio, tone_bits, aff_coef, sharp_factor};
  const uint32_t f = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
  return ffcv::launch_tiles(who, "randaugment_kernel", randaugment_kernel, stream, (uint64_t)batch, RA_THREADS, 0, src,
                            dst, batch, height, width, num_ops, mode, f, A);
}

}  // extern "C"
