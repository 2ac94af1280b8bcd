// ral_slot.h -- one slot of RandAugment on an image held in ONE LDS buffer
// (DESIGN.md s27): the sizes of the 1024-thread kernel, the LDS a slot works
// in beside the image, and ral_slot itself, shared by
// ffcv_randaugment_large.hip and ffcv_augmix_large.hip.  Device code, all
// inlined; include it under the no-packed-fp32-ops attribute of its users.
#pragma once
#include "ra_slot.h"

#define RAL_OUT_OFF 16u  // where a moving operation's dense result starts in the buffer

// The kernel's sizes.  A thread's steps: groups of four pixels (12 bytes)
// for the warp, of four row bytes for the stencil, whose rows may each end in
// a partial group (H more groups at most: fits() holds a shape to the bound).
template <int THREADS_, int IMG_BYTES_>
struct RalTier {
  static constexpr int THREADS = THREADS_, IMG_BYTES = IMG_BYTES_, WAVES = THREADS_ / 64;
  static constexpr int CHUNKS = 1 + IMG_BYTES_ / 16 + 1 + 2;
  static constexpr int WARP_STEPS = (IMG_BYTES_ / 12 + THREADS_ - 1) / THREADS_;
  static constexpr int STEN_STEPS = (IMG_BYTES_ / 4 + THREADS_ - 1) / THREADS_;
  static bool fits(int H, int W) {
    if (H <= 0 || W <= 0 || H > FFCV_AFFINE_MAX_DIM || W > FFCV_AFFINE_MAX_DIM) return false;
    const uint64_t npix = (uint64_t)H * W, ng = (3u * (uint64_t)W + 3u) >> 2;
    return 3u * npix <= (uint64_t)IMG_BYTES && (npix + 3u) / 4u <= (uint64_t)WARP_STEPS * THREADS &&
           (uint64_t)H * ng <= (uint64_t)STEN_STEPS * THREADS;
  }
};
typedef RalTier<1024, 224 * 224 * 3> RalTop;

// the LDS a slot works in beside the image
template <class T>
struct RalScratch {
  uint32_t *hist;              // [3 * 256] the channel histograms
  uint8_t *tab;                // [3 * 256] the slot's table: one, or one per channel
  uint32_t (*part)[T::WAVES];  // [3] scan partials; [0]: the gray sum's
  uint64_t (*occ)[4];          // [3] occupied bins per wave of the 256 bins
};

// Slot s's operation of image k of B on the H0 x W0 image at s_mem + cur_off,
// in place, or over it as the dense image at s_mem + RAL_OUT_OFF, which
// cur_off then names.  Every path that changes the image ends with a
// __syncthreads().
template <class T>
FFCV_DEV void ral_slot(int t0, int H0, int W0, uint32_t fill0, int mode, int B, uint32_t k, int s, const RaIn &A,
                       uint8_t *s_mem, uint32_t &cur_off, const RalScratch<T> &L) {
  constexpr int THREADS = T::THREADS;
  // (pinned as in ra_slot: what the branches derive from these would otherwise
  // be hoisted out of the slots' loop, live across it in scalar registers, and spill)
  int t = t0, H = H0, W = W0;
  uint32_t fill = fill0;
  asm volatile("" : "+v"(t), "+s"(H), "+s"(W), "+s"(fill));
  const int lane = t & 63, wave = t >> 6, rowb = 3 * W;
  const uint32_t npix = (uint32_t)H * (uint32_t)W, nbytes = 3u * npix;
  const uint64_t sk = (uint64_t)s * (uint32_t)B + k;
  const int op = ra_op(A, B, k, s);
  uint8_t *cur = s_mem + cur_off;
  uint32_t *const out = (uint32_t *)(s_mem + RAL_OUT_OFF);

  // the gray sum of the image (fits 32 bits: 50,176 * 255), in every thread
  auto gray_sum = [&]() -> uint32_t {
    uint32_t sum = 0;
    for (uint32_t q = t; q < npix; q += THREADS) {
      const uint32_t v = lds_pixel(cur + 3u * q);
      sum += cj_gray(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu);
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) L.part[0][wave] = sum;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < T::WAVES; w++) total += L.part[0][w];
    return total;
  };
  // every whole word that covers the image's bytes through the table: one, or
  // one per channel (the channel of a byte is its offset in the image % 3)
  auto map_words = [&](bool by_channel) {
    uint32_t *w0 = (uint32_t *)__builtin_align_down(cur, 4);
    const uint32_t lead = (uint32_t)(cur - (uint8_t *)w0), nw = (lead + nbytes + 3u) >> 2;
    for (uint32_t w = t; w < nw; w += THREADS) {
      const uint32_t v = w0[w];
      const uint32_t c = by_channel ? (4u * w + 3u - lead) % 3u : 0u;  // the channel of the word's first byte
      const uint32_t o0 = by_channel ? c * 256u : 0u, o1 = by_channel ? (c == 2u ? 0u : c + 1u) * 256u : 0u,
                     o2 = by_channel ? (c == 0u ? 2u : c - 1u) * 256u : 0u;
      w0[w] = (uint32_t)L.tab[o0 + (v & 0xffu)] | ((uint32_t)L.tab[o1 + ((v >> 8) & 0xffu)] << 8) |
              ((uint32_t)L.tab[o2 + ((v >> 16) & 0xffu)] << 16) | ((uint32_t)L.tab[o0 + (v >> 24)] << 24);
    }
  };
  // The warp: group g = t + j * THREADS of four adjacent pixels is step j's,
  // three dwords of registers; all are stored after the barrier.  The group's
  // first pixel (r, c) advances by 4 * THREADS pixels per step without a
  // division.  The last group may run up to three pixels past the image:
  // pix(r, c) is safe at any (r, c), and their bytes land in the buffer's slack.
  auto warp = [&](auto pix) {
    const int dr = (4 * THREADS) / W, dc = (4 * THREADS) - dr * W;
    int r = (4 * t) / W, c = 4 * t - r * W;
    uint32_t R[3 * T::WARP_STEPS];
#pragma unroll
    for (int j = 0; j < T::WARP_STEPS; j++) {
      R[3 * j] = R[3 * j + 1] = R[3 * j + 2] = 0u;
      if (4u * (uint32_t)(t + j * THREADS) < npix) {
        int rr = r, cc = c;
        uint32_t v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          v[e] = pix(rr, cc);
          cc++;
          if (cc == W) {
            cc = 0;
            rr++;
          }
        }
        R[3 * j + 0] = v[0] | (v[1] << 24);
        R[3 * j + 1] = (v[1] >> 8) | (v[2] << 16);
        R[3 * j + 2] = (v[2] >> 16) | (v[3] << 8);
      }
      r += dr;
      c += dc;
      if (c >= W) {
        c -= W;
        r++;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T::WARP_STEPS; j++) {
      const uint32_t g = (uint32_t)(t + j * THREADS);
      if (4u * g < npix) {
        out[3u * g + 0] = R[3 * j + 0];
        out[3u * g + 1] = R[3 * j + 1];
        out[3u * g + 2] = R[3 * j + 2];
      }
    }
  };

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
      // nothing of the image is read: no registers, no barrier in front
      const uint32_t f0 = fill | (fill << 24), f1 = (fill >> 8) | (fill << 16), f2 = (fill >> 16) | (fill << 8);
      for (uint32_t g = t; 4u * g < npix; g += THREADS) {
        out[3u * g + 0] = f0;
        out[3u * g + 1] = f1;
        out[3u * g + 2] = f2;
      }
    } else if (box.fits32) {
      // 32-bit coordinates relative to the image's corner: the true values fit
      // (box.fits32), so wrapping arithmetic gives them exactly
      const uint32_t X0 = (uint32_t)box.X0, Y0 = (uint32_t)box.Y0, q0 = (uint32_t)q[0], q1 = (uint32_t)q[1],
                     q3 = (uint32_t)q[3], q4 = (uint32_t)q[4];
      warp([&](int r, int c) -> uint32_t {
        const uint32_t X = X0 + q0 * (uint32_t)c + q1 * (uint32_t)r, Y = Y0 + q3 * (uint32_t)c + q4 * (uint32_t)r;
        return affine_sample<int32_t>(mode, (int32_t)X, (int32_t)Y, tap);
      });
    } else {
      warp([&](int r, int c) -> uint32_t {
        return affine_sample<int64_t>(mode, affine_x(q, c, r), affine_y(q, c, r), tap);
      });
    }
    cur_off = RAL_OUT_OFF;
    __syncthreads();
  } else if (op == RA_SHARPNESS) {
    // ---- ffcv_sharpness_batch's stencil: four adjacent bytes of a row per
    // thread and step, from the ten bytes [b - 3, b + 7) of three rows, as one
    // dword of registers; a byte on the image's outermost ring takes d = i
    // through the same code.  Item i = t + j * THREADS is group i % ng of row
    // i / ng, advanced without a division.
    const float a = A.sharp_factor[sk];
    const int ng = (rowb + 3) >> 2, items = H * ng;
    const int dy = THREADS / ng, dg = THREADS - dy * ng;
    const int y0 = t / ng, g0 = t - y0 * ng;
    uint32_t R[T::STEN_STEPS];
    int y = y0, g = g0;
#pragma unroll
    for (int j = 0; j < T::STEN_STEPS; j++) {
      R[j] = 0u;
      if (t + j * THREADS < items) {
        const int b0 = 4 * g;
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
        for (int e = 0; e < 4; e++) {
          const float v = ce.f(e + 3);
          const float top = sharp_row(pu[e], pu[e + 3], pu[e + 6]);
          const float mid = sharp_row(pc[e], blur_mul(v, SHARP_W5), pc[e + 6]);
          const float bot = sharp_row(pd[e], pd[e + 3], pd[e + 6]);
          const bool border = edge_row || b0 + e < 3 || b0 + e >= rowb - 3;
          o[e] = sharp_blend(a, border ? v : sharp_smooth(top, mid, bot), v);
        }
        R[j] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
      }
      y += dy;
      g += dg;
      if (g >= ng) {
        g -= ng;
        y++;
      }
    }
    __syncthreads();
    // (the stores' rows and groups are computed afresh from an opaque copy:
    // shared with the pass above, every step's pair would stay live across it)
    uint8_t *const ob8 = (uint8_t *)out;
    int ts = t;
    y = y0, g = g0;
    asm volatile("" : "+v"(ts), "+v"(y), "+v"(g));
#pragma unroll
    for (int j = 0; j < T::STEN_STEPS; j++) {
      if (ts + j * THREADS < items) {
        const int b0 = 4 * g, ob = y * rowb + b0;
        if (!(ob & 3) && b0 + 4 <= rowb) {
          *(uint32_t *)(ob8 + ob) = R[j];
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (b0 + e < rowb) ob8[ob + e] = (uint8_t)(R[j] >> (8 * e));
        }
      }
      y += dy;
      g += dg;
      if (g >= ng) {
        g -= ng;
        y++;
      }
    }
    cur_off = RAL_OUT_OFF;
    __syncthreads();
  } else if (op == RA_COLOR) {
    // ---- saturation, per pixel
    const double r = A.cj_ratio[(4u * (uint64_t)s + 1u) * (uint32_t)B + k];
    const double omr = cj_one_minus(r);
    for (uint32_t p = t; p < npix; p += THREADS) {
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
    // ---- one 256-entry table of the image (threads 0..255 own an entry
    // each), then a byte map by every thread
    if (op == RA_POSTERIZE) {
      const int bits = min(8, max(1, __builtin_amdgcn_readfirstlane((int)A.tone_bits[sk])));
      if (t < 256) L.tab[t] = (uint8_t)tone_posterize(bits, (uint32_t)t);
    } else {
      const uint32_t row = op == RA_BRIGHTNESS ? 0u : (op == RA_CONTRAST ? 2u : 3u);
      const double r = A.cj_ratio[(4u * (uint64_t)s + row) * (uint32_t)B + k];
      const double omr = cj_one_minus(r);
      double other = 0.0;
      if (op == RA_CONTRAST) other = cj_mean((uint64_t)gray_sum(), (uint64_t)npix);
      if (t < 256)
        L.tab[t] = (uint8_t)(op == RA_SOLARIZE ? cj_solarize(r, (uint32_t)t) : cj_blend(r, omr, (uint32_t)t, other));
    }
    __syncthreads();
    map_words(false);
    __syncthreads();
  } else if (op == RA_AUTOCONTRAST || op == RA_EQUALIZE) {
    // ---- the channels' histograms by every thread, their tables (thread t <
    // 256 owns bin t of the three channels: waves 0..3, whole), a byte map by
    // channel by every thread
    const int kind = op == RA_AUTOCONTRAST ? FFCV_TONE_AUTOCONTRAST : FFCV_TONE_EQUALIZE;
    if (t < 768) L.hist[t] = 0u;
    if (THREADS < 768 && t < 768 - THREADS) L.hist[THREADS + t] = 0u;
    __syncthreads();
    for (uint32_t p = t; p < npix; p += THREADS) {
      const uint32_t v = lds_pixel(cur + 3u * p);
      atomicAdd(&L.hist[v & 0xffu], 1u);
      atomicAdd(&L.hist[256u + ((v >> 8) & 0xffu)], 1u);
      atomicAdd(&L.hist[512u + ((v >> 16) & 0xffu)], 1u);
    }
    __syncthreads();
    uint32_t h[3] = {0u, 0u, 0u}, incl[3] = {0u, 0u, 0u};
    if (t < 256) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        h[c] = L.hist[c * 256 + t];
        // per wave: which bins are occupied (ballot) and the inclusive sum (scan)
        const uint64_t occ = __ballot(h[c] != 0u);
        uint32_t sum = h[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = __shfl_up(sum, d, 64);
          if (lane >= d) sum += o;
        }
        incl[c] = sum;
        if (lane == 63) L.part[c][wave] = sum;
        if (lane == 0) L.occ[c][wave] = occ;
      }
    }
    __syncthreads();
    if (t < 256) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        uint32_t below = incl[c] - h[c], lo = 0u, hi = 0u;
#pragma unroll
        for (int w = 0; w < 4; w++) below += w < wave ? L.part[c][w] : 0u;
#pragma unroll
        for (int w = 3; w >= 0; w--) {
          const uint64_t occ = L.occ[c][w];
          if (occ) lo = 64u * w + (uint32_t)__builtin_ctzll(occ);
        }
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const uint64_t occ = L.occ[c][w];
          if (occ) hi = 64u * w + 63u - (uint32_t)__builtin_clzll(occ);
        }
        L.tab[c * 256 + t] = (uint8_t)tone_entry(kind, 8, npix, lo, hi, L.hist[c * 256 + hi], below, (uint32_t)t);
      }
    }
    __syncthreads();
    map_words(true);
    __syncthreads();
  }
}
