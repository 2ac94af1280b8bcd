// ffcv_augmix.hip -- AugMix: the draws (op ids 24 and 25), the
// fused pixel pass for images up to 64 x 64, the streaming mix of the rounds
// path beyond, and the host twins of the draws and of the mix.  (The mix's
// arithmetic is augmix_mix.h; the pixel pass for images up to 224 x 224 is
// ffcv_augmix_large.hip.)
//
// A sample runs `width` (1..4) independent chains of 1..3 operations of s24,
// each chain from the ORIGINAL image, and leaves as the float32 convex
// combination  w_0 x + w_1 y_0 + ... + w_width y_{width-1}  of the original and
// the chains' results, rounded half to even.
//
//   draws: one lane per sample, two MT19937 streams.  Stream 24 draws ten
//     values per chain, always all ten (depth; then op, bin, neg per step), and
//     fills slot 3 i + j of RandAugment's arrays (ra_slot.h) for step j of chain
//     i -- Identity beyond the chain's depth -- so the pixel entries of s24 take
//     a slot's slices unchanged.  Stream 25, whose length varies, draws the
//     gammas a, b, g_0 .. g_{width-1} as numpy's legacy RandomState does, and
//     from them the weights, in float64, each rounded once to float32.
//
//   augmix_kernel: one 256-thread workgroup per image, three image buffers in
//     LDS.  Buffer 0 takes the staged original and is never written again;
//     buffers 1 and 2 are a chain's ping-pong, running the slot code of
//     ra_slot.h.  A chain's first step that moves the image reads the original
//     in place; one that works in place gets an LDS-to-LDS copy first.  The mix
//     never exists as an image: thread t owns the image's bytes 4 (t + 256 j)
//     .. + 3, j = 0 .. 11, as 48 float32 accumulators in registers, adds every
//     chain's result to them as the chain ends, and packs the rounded bytes into
//     the buffer the last chain did not end in, from where they leave once.
//     Chain i + 1 starts in the buffer chain i did NOT end in, so a thread that
//     still adds chain i's result is never overtaken: the barrier that ends a
//     step is the only one there is.
//
//   augmix_mix_kernel: the same mix, streaming, for images beyond the fused
//     regime: 16 output bytes per thread from the aligned 16-byte chunks of the
//     original and of the chains' result batches, at any alignment of each.
//
// LDS of augmix_kernel: three image buffers of 12,352 B, the counters 3,072,
// the tables 768, scan partials 144: 41,040 bytes, three workgroups per CU.
#if defined(__HIP_DEVICE_COMPILE__)
// every float32 product and sum of the mix is an instruction of its own, never
// half of a packed one
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "api_internal.h"
#include "augmix_mix.h"
#include "ra_slot.h"

#define FFCV_AUGMIX_OP 24
#define FFCV_AUGMIX_WEIGHT_OP 25
#define AM_NBINS 10
#define AM_LDS_BYTES (3 * RA_IMG_BYTES)  // the fused regime: 9 H W at most this
#define AM_OWN (RA_IMG_BYTES / (4 * RA_THREADS))  // words of the image a thread owns

// ----------------------------------------------------------- the draws --
// Stream 24 of one sample.  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_augmix_chains(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, int severity,
                               int width, int chain_depth, int all_ops, const double *table, int H, int W,
                               const RaArrays &o, uint8_t *depth) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_AUGMIX_OP));
  const uint64_t uk = (uint64_t)k, uB = (uint64_t)B;
  const int n = all_ops ? 13 : 9;
  // the draws first, unrolled (constant stream positions, as in RandAugment's):
  // chain i in 32 bits, step j's op | bin << 4 | neg << 8 in bits 10 j on, the
  // depth in bits 30 and 31
  uint64_t drawn[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < AM_MAX_WIDTH; i++) {
    if (i >= width) break;
    const double ud = mt_double(m);
    uint32_t word = (uint32_t)(chain_depth > 0 ? chain_depth : min(AM_MAX_DEPTH, 1 + (int)cj_mul(ud, 3.0))) << 30;
#pragma unroll
    for (int j = 0; j < AM_MAX_DEPTH; j++) {
      const double u0 = mt_double(m), u1 = mt_double(m), u2 = mt_double(m);
      const int at = min(n - 1, (int)cj_mul(u0, (double)n));
      // all 13, or ShearX .. Rotate and Posterize .. Equalize
      const uint32_t op = (uint32_t)(all_ops || at < 5 ? at + 1 : at + 5);
      const uint32_t bin = (uint32_t)min(severity - 1, (int)cj_mul(u1, (double)severity));
      word |= (op | (bin << 4) | (u2 < 0.5 ? 256u : 0u)) << (10 * j);
    }
    drawn[i >> 1] |= (uint64_t)word << (32 * (i & 1));
  }
  for (int i = 0; i < width; i++) {
    const uint32_t word = (uint32_t)((i < 2 ? drawn[0] : drawn[1]) >> (32 * (i & 1)));
    const int d = (int)(word >> 30);
    depth[(uint64_t)i * uB + uk] = (uint8_t)d;
    for (int j = 0; j < AM_MAX_DEPTH; j++) {
      const uint32_t step = (word >> (10 * j)) & 1023u;
      const int op = j < d ? (int)(step & 15u) : RA_IDENTITY;
      ra_fill_slot(AM_MAX_DEPTH * i + j, uk, uB, op, (step & 256u) != 0, table[op * AM_NBINS + (int)((step >> 4) & 15u)],
                   H, W, o);
    }
  }
  return m.err;
}

// The weights' stream is as long as its rejections make it, so words 227 ..
// 623 of the MT19937 (device_common.h) are reachable.  mt_u32 computes those
// by a recursion that is kept out of line; a kernel that calls it pays for the
// call in scratch and in scalar registers saved around it.  Here the same
// words come from loops, inlined: new[m], m < 623, is a twist of old[m],
// old[m + 1] and old[m + 397] (m < 227) or new[m - 227], which is at most two
// steps from a word below 227; new[623] twists old[623], new[0] and new[396].
FFCV_HD void am_old_pair(uint32_t seed, int k, uint32_t &a0, uint32_t &a1) {  // old[k], old[k + 1]
  uint32_t x = seed;
  for (int i = 1; i <= k; i++) x = mt_chain(x, (uint32_t)i);
  a0 = x;
  a1 = mt_chain(x, (uint32_t)(k + 1));
}
FFCV_HD uint32_t am_new_at(uint32_t seed, int m) {  // m < 623
  const int levels = m / 227;
  int mm = m - 227 * levels;
  uint32_t a0, a1;
  am_old_pair(seed, mm, a0, a1);
  uint32_t far = a1;
  for (int i = mm + 2; i <= mm + 397; i++) far = mt_chain(far, (uint32_t)i);
  uint32_t v = mt_twist1(a0, a1, far);
  for (int l = 0; l < levels; l++) {
    mm += 227;
    am_old_pair(seed, mm, a0, a1);
    v = mt_twist1(a0, a1, v);
  }
  return v;
}
FFCV_HD uint32_t am_u32(DevMT &m) {
  uint32_t v = 0;
  if (m.n < 227) {
    v = mt_twist1(m.a0, m.a1, m.b);
    m.a0 = m.a1;
    m.a1 = mt_chain(m.a1, (uint32_t)(m.n + 2));
    m.b = mt_chain(m.b, (uint32_t)(m.n + 398));
  } else if (m.n < 623) {
    v = am_new_at(m.seed, m.n);
  } else if (m.n == 623) {
    uint32_t a0, a1;
    am_old_pair(m.seed, 623, a0, a1);
    v = mt_twist1(a0, am_new_at(m.seed, 0), am_new_at(m.seed, 396));
  } else {
    m.err = 1;
  }
  m.n++;
  return mt_temper(v);
}
// genrand_res53, as mt_double; one copy of am_u32's code
FFCV_HD double am_double(DevMT &m) {
  int32_t a = 0, b = 0;
#pragma unroll 1
  for (int i = 0; i < 2; i++) {
    const uint32_t u = am_u32(m);
    a = i == 0 ? (int32_t)(u >> 5) : a;
    b = i == 1 ? (int32_t)(u >> 6) : b;
  }
  return (a * 67108864.0 + b) / 9007199254740992.0;
}

// numpy's legacy RandomState on that stream: standard_exponential, gauss
// (polar, the second value kept for the next call) and standard_gamma.  Every
// loop ends when the stream runs out.
struct AmGauss {
  double g;
  int has;
};
FFCV_HD double am_exponential(DevMT &m) {
#pragma clang fp contract(off)
  return -log(1.0 - am_double(m));
}
FFCV_HD double am_gauss(DevMT &m, AmGauss &c) {
#pragma clang fp contract(off)
  if (c.has) {
    c.has = 0;
    return c.g;
  }
  double x1, x2, r2;
  do {
    x1 = 2.0 * am_double(m) - 1.0;
    x2 = 2.0 * am_double(m) - 1.0;
    r2 = x1 * x1 + x2 * x2;
  } while ((r2 >= 1.0 || r2 == 0.0) && !m.err);
  if (m.err) return 0.0;
  const double f = sqrt(-2.0 * log(r2) / r2);
  c.g = f * x1;
  c.has = 1;
  return f * x2;
}
// KIND: shape == 1 (0), < 1 (1), > 1 (2), the same for a whole batch
template <int KIND>
FFCV_HD double am_gamma(DevMT &m, AmGauss &c, double shape) {
#pragma clang fp contract(off)
  if (KIND == 0) return am_exponential(m);
  if (KIND == 1) {  // Ahrens-Dieter
    while (!m.err) {
      const double U = am_double(m), V = am_exponential(m);
      if (U <= 1.0 - shape) {
        const double X = pow(U, 1.0 / shape);
        if (X <= V) return X;
      } else {
        const double Y = -log((1.0 - U) / shape);
        const double X = pow(1.0 - shape + shape * Y, 1.0 / shape);
        if (X <= V + Y) return X;
      }
    }
    return 0.0;
  }
  const double b = shape - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * b);  // Marsaglia-Tsang
  while (!m.err) {
    double X, V;
    do {
      X = am_gauss(m, c);
      V = 1.0 + cc * X;
    } while (V <= 0.0 && !m.err);
    V = V * V * V;
    const double U = am_double(m);
    if (U < 1.0 - 0.0331 * (X * X) * (X * X)) return b * V;
    if (log(U) < 0.5 * X * X + b * (1.0 - V + log(V))) return b * V;
  }
  return 0.0;
}

// Stream 25 of one sample: weights[0 .. width][B].  Returns 1 when the stream
// ran out or a sum is 0 or not finite: the weights are then (1, 0, .., 0).
template <int KIND>
FFCV_HD int draw_augmix_weights(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, int width,
                                double alpha, float *weights) {
#pragma clang fp contract(off)
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_AUGMIX_WEIGHT_OP));
  AmGauss c = {0.0, 0};
  // a, b, g_0 .. g_{width-1}, in this order (one copy of the gamma's code)
  double a = 0.0, b = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
  for (int i = 0; i < 2 + width; i++) {
    const double x = am_gamma<KIND>(m, c, alpha);
    a = i == 0 ? x : a;
    b = i == 1 ? x : b;
    g0 = i == 2 ? x : g0;
    g1 = i == 3 ? x : g1;
    g2 = i == 4 ? x : g2;
    g3 = i == 5 ? x : g3;
  }
  const double g[AM_MAX_WIDTH] = {g0, g1, g2, g3};
  const double ab = a + b, gs = ((g0 + g1) + g2) + g3;
  const bool bad = m.err || !(ab > 0.0) || !(gs > 0.0) || !__builtin_isfinite(ab) || !__builtin_isfinite(gs);
  const double rest = bad ? 0.0 : b / ab;
  weights[k] = bad ? 1.0f : (float)(a / ab);
#pragma unroll
  for (int i = 0; i < AM_MAX_WIDTH; i++)
    if (i < width) weights[(uint64_t)(i + 1) * (uint64_t)B + (uint64_t)k] = bad ? 0.0f : (float)(rest * (g[i] / gs));
  return bad;
}

// Two kernels, one lane per sample each: the chains' draw is RandAugment's in
// registers and more, the gammas' loops are long and diverge.  status: the
// chains' kernel writes it, the weights' kernel, launched behind it, raises it.
__global__ void __launch_bounds__(64)
    augmix_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed, uint64_t epoch, int severity,
                       int width, int chain_depth, int all_ops, const double *__restrict__ table, int H, int W,
                       RaArrays o, uint8_t *__restrict__ depth, int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  // (the pointers in vector registers, as in randaugment_draw_kernel)
  asm volatile(""
               : "+v"(o.op), "+v"(o.cj_apply), "+v"(o.cj_ratio), "+v"(o.tone_apply), "+v"(o.tone_bits),
                 "+v"(o.aff_apply), "+v"(o.aff_coef), "+v"(o.sharp_apply), "+v"(o.sharp_factor), "+v"(depth),
                 "+v"(table), "+v"(status));
  const int err = draw_augmix_chains(k, B, ids[k], loader_seed, epoch, severity, width, chain_depth, all_ops, table, H,
                                     W, o, depth);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

template <int KIND>
__global__ void __launch_bounds__(64)
    augmix_weight_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed, uint64_t epoch, int width,
                         double alpha, float *__restrict__ weights, int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_augmix_weights<KIND>(k, B, ids[k], loader_seed, epoch, width, alpha, weights);
  if (status && err) status[k] = FFCV_SAMPLE_RNG;
}

// ---------------------------------------------------- the fused kernel --
// The image at `img` (LDS, any alignment) into the thread's accumulators at
// weight w: word j of the thread is the image's bytes 4 (t + 256 j) .. + 3,
// read as two aligned LDS words.  A word wholly past the image is skipped (by
// all threads of a block of 256 words: a scalar branch) or read at word 0, its
// accumulators never leaving.
template <bool FIRST>
FFCV_DEV void am_accumulate(float (&acc)[4 * AM_OWN], const uint8_t *img, uint32_t nbytes, int t, float w) {
  const uint32_t *q = (const uint32_t *)__builtin_align_down(img, 4);
  const uint32_t sh = (uint32_t)(img - (const uint8_t *)q);
#pragma unroll
  for (int j = 0; j < AM_OWN; j++) {
    if (4u * RA_THREADS * (uint32_t)j < nbytes) {
      const uint32_t idx = (uint32_t)t + RA_THREADS * (uint32_t)j;
      const uint32_t at = 4u * idx < nbytes ? idx : 0u;
      const uint32_t v = __builtin_amdgcn_alignbyte(q[at + 1], q[at], sh);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float y = (float)((v >> (8 * e)) & 0xffu);
        acc[4 * j + e] = FIRST ? augmix_first(w, y) : augmix_add(acc[4 * j + e], w, y);
      }
    }
  }
}

__global__ void __launch_bounds__(RA_THREADS)
    augmix_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int B, int H0, int W0, int width, int mode,
                  uint32_t fill0, RaIn A, const uint8_t *__restrict__ depth, const float *__restrict__ weights) {
  __shared__ lds_x4_t s_buf[3 * RA_BUF_CHUNKS];  // the original, and a chain's two buffers
  __shared__ uint32_t s_hist[3 * 256];
  __shared__ uint8_t s_tab[3 * 256];
  __shared__ uint32_t s_part[3][RA_THREADS / 64];
  __shared__ uint64_t s_occ[3][RA_THREADS / 64];
  const int t0 = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const uint32_t nbytes0 = 3u * (uint32_t)H0 * (uint32_t)W0;  // <= RA_IMG_BYTES
  uint8_t *const s_mem = (uint8_t *)s_buf;
  const RaScratch lds = {s_hist, s_tab, s_part, s_occ};
  // (these pointers are live across the chains' loop, beside everything the
  // slot code keeps in scalar registers: there they spill)
  asm volatile(""
               : "+v"(dst), "+v"(depth), "+v"(weights), "+v"(A.op), "+v"(A.cj_ratio), "+v"(A.tone_bits), "+v"(A.aff_coef),
                 "+v"(A.sharp_factor));
  // weight i of the image, in a scalar register
  auto weight = [&](int i) -> float {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(weights[(uint64_t)i * (uint32_t)B + k])));
  };

  // ---- stage the original behind buffer 0's 16 front bytes; it stays
  const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * nbytes0;
  stage_rows<RA_THREADS>(t0, src0, 0, 1, nbytes0, (int)lds_chunks(nbytes0), s_buf + 1);
  uint32_t orig_off = 16u + (uint32_t)(src0 & 15);
  __syncthreads();
  // (what the slot code wants in scalar registers waits in vector registers
  // between the slots, for the same reason)
  int Hv = H0, Wv = W0, modev = mode, Bv = B;
  uint32_t fillv = fill0, nbytesv = nbytes0;
  asm volatile("" : "+v"(Hv), "+v"(Wv), "+v"(modev), "+v"(Bv), "+v"(fillv), "+v"(nbytesv), "+v"(orig_off));
  float acc[4 * AM_OWN];
  am_accumulate<true>(acc, s_mem + orig_off, nbytes0, t0, weight(0));

  uint32_t last = 0;  // the buffer the chain before ended in (0: the original)
  for (int i = 0; i < width; i++) {
    const int d = min(AM_MAX_DEPTH, max(1, __builtin_amdgcn_readfirstlane((int)depth[(uint64_t)i * (uint32_t)B + k])));
    const uint32_t first = last == 1u ? 2u : 1u;
    uint32_t cur_off = orig_off;
    for (int j = 0; j < d; j++) {
      const int s = AM_MAX_DEPTH * i + j;
      const uint32_t cb = cur_off / RA_BUF_BYTES;
      const uint32_t nxt_off = (cb == 0u ? first : 3u - cb) * RA_BUF_BYTES + 16u;  // dense, 16-byte aligned
      const int op = ra_op(A, B, k, s);
      if (cb == 0u && op >= RA_BRIGHTNESS && op <= RA_EQUALIZE && op != RA_SHARPNESS) {
        // an operation in place, on the original: on a copy of it
        const uint32_t *q = (const uint32_t *)__builtin_align_down(s_mem + orig_off, 4);
        const uint32_t sh = orig_off & 3u;
        uint32_t *o = (uint32_t *)(s_mem + nxt_off);
        for (uint32_t w = t0; 4u * w < nbytesv; w += RA_THREADS) o[w] = __builtin_amdgcn_alignbyte(q[w + 1], q[w], sh);
        cur_off = nxt_off;
        __syncthreads();
      }
      ra_slot(t0, __builtin_amdgcn_readfirstlane(Hv), __builtin_amdgcn_readfirstlane(Wv),
              (uint32_t)__builtin_amdgcn_readfirstlane((int)fillv), __builtin_amdgcn_readfirstlane(modev),
              __builtin_amdgcn_readfirstlane(Bv), k, s, A, s_mem, cur_off, nxt_off, lds);
    }
    am_accumulate<false>(acc, s_mem + cur_off, (uint32_t)__builtin_amdgcn_readfirstlane((int)nbytesv), t0, weight(i + 1));
    last = cur_off / RA_BUF_BYTES;
  }

  // ---- the rounded bytes, dense, into the buffer the last chain did not end
  // in; they leave once, at any alignment of dst
  const uint32_t out_off = (last == 1u ? 2u : 1u) * RA_BUF_BYTES + 16u;
  uint32_t *o = (uint32_t *)(s_mem + out_off);
#pragma unroll
  for (int j = 0; j < AM_OWN; j++) {
    const uint32_t idx = (uint32_t)t0 + RA_THREADS * (uint32_t)j;
    if (4u * idx < nbytesv)
      o[idx] = augmix_byte(acc[4 * j]) | augmix_byte(acc[4 * j + 1]) << 8 | augmix_byte(acc[4 * j + 2]) << 16 |
               augmix_byte(acc[4 * j + 3]) << 24;
  }
  __syncthreads();
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * nbytes0;
  const uint8_t *out = s_mem + out_off;
  write_back_rows<RA_THREADS>(t0, dst0, 0, 1, nbytes0, [&](int) { return out; });
}

// ------------------------------------------------ the streaming kernel --
struct AmMixIn {
  const uint8_t *img[1 + AM_MAX_WIDTH];  // the original, then the chains' results
};

// One thread per aligned 16-byte chunk of `out` that holds a byte of image k.
__global__ void __launch_bounds__(256)
    augmix_mix_kernel(AmMixIn in, int width, const float *__restrict__ weights, uint8_t *__restrict__ out, uint32_t B,
                      uint32_t img, uint32_t blocks_per_img) {
  const uint32_t k = blockIdx.x / blocks_per_img;
  const uint32_t c = (blockIdx.x - k * blocks_per_img) * 256u + threadIdx.x;
  const uint64_t da = (uint64_t)(uintptr_t)out + (uint64_t)k * img;
  const int dl = (int)(da & 15);
  const int64_t b0 = 16 * (int64_t)c - dl;  // the chunk's first byte, as a byte of the image
  if (b0 >= (int64_t)img) return;
  const int jlo = b0 < 0 ? (int)-b0 : 0, jhi = (int64_t)img - b0 < 16 ? (int)((int64_t)img - b0) : 16;
  float acc[16];
#pragma unroll
  for (int i = 0; i <= AM_MAX_WIDTH; i++) {
    if (i > width) break;
    const float w = weights[(uint64_t)i * B + k];
    const lds_x4_t v = am_load16((uint64_t)(uintptr_t)in.img[i] + (uint64_t)k * img + (uint64_t)b0, jlo, jhi);
    am_mix16(acc, i == 0, w, v);
  }
  uint8_t *gb = (uint8_t *)(uintptr_t)((da & ~(uint64_t)15) + 16u * (uint64_t)c);
  am_store16(gb, acc, jlo, jhi);
}

namespace {

bool am_draw_args_ok(const char *who, const void *ids, int batch, int severity, int width, int chain_depth, double alpha,
                     const void *table, int H, int W, const RaArrays &o, const void *depth, const void *weights) {
  if (batch < 0 || !ids || !table || !o.complete() || !depth || !weights || severity < 1 || severity > AM_NBINS ||
      width < 1 || width > AM_MAX_WIDTH || !(chain_depth == -1 || (chain_depth >= 1 && chain_depth <= AM_MAX_DEPTH)) ||
      !(alpha >= 0.01 && alpha <= 100.0) || H <= 0 || W <= 0 || H > FFCV_AFFINE_MAX_DIM || W > FFCV_AFFINE_MAX_DIM) {
    ffcv::set_error("%s: invalid arguments (batch %d, severity %d of 1 to %d, width %d of 1 to %d, depth %d, alpha %g, "
                    "%dx%d)", who, batch, severity, AM_NBINS, width, AM_MAX_WIDTH, chain_depth, alpha, H, W);
    return false;
  }
  return true;
}

// the mix entries' arguments; *img: an image's bytes
bool am_mix_args_ok(const char *who, const uint8_t *orig, const uint8_t *const r[AM_MAX_WIDTH], int width,
                    const float *weights, const uint8_t *out, int batch, int height, int width_px, uint64_t *img) {
  if (width < 1 || width > AM_MAX_WIDTH) {
    ffcv::set_error("%s: mixture width %d, outside 1 to %d", who, width, AM_MAX_WIDTH);
    return false;
  }
  bool pointers = orig && weights && out;
  for (int i = 0; i < width; i++) pointers = pointers && r[i];
  if (!ffcv::u8_images_ok(who, pointers, batch, height, width_px)) return false;
  *img = (uint64_t)height * width_px * 3;
  const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uint64_t)batch * *img;
  for (int i = 0; i <= width && batch > 0; i++) {
    const uintptr_t a0 = (uintptr_t)(i == 0 ? orig : r[i - 1]), a1 = a0 + (uint64_t)batch * *img;
    if (a0 < b1 && b0 < a1) {
      ffcv::set_error("%s: out overlaps an input (the mix is out of place)", who);
      return false;
    }
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_augmix_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                           int severity, int mixture_width, int chain_depth, double alpha, int all_ops,
                           const double *table, int height, int width, uint8_t *op, uint8_t *cj_apply, double *cj_ratio,
                           uint8_t *tone_apply, uint8_t *tone_bits, uint8_t *aff_apply, int64_t *aff_coef,
                           uint8_t *sharp_apply, float *sharp_factor, uint8_t *depth, float *weights, int32_t *status) {
  const RaArrays o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!am_draw_args_ok("ffcv_augmix_draw_batch", sample_ids, batch, severity, mixture_width, chain_depth, alpha, table,
                       height, width, o, depth, weights))
    return FFCV_EINVAL;
  const int rc = ffcv::launch_draw("augmix_draw_kernel", augmix_draw_kernel, stream, batch, sample_ids, batch,
                                   loader_seed, epoch, severity, mixture_width, chain_depth, (int)(all_ops != 0), table,
                                   height, width, o, depth, status);
  if (rc != FFCV_OK) return rc;
  const auto kernel = alpha == 1.0 ? augmix_weight_kernel<0> : (alpha < 1.0 ? augmix_weight_kernel<1>
                                                                              : augmix_weight_kernel<2>);
  return ffcv::launch_draw("augmix_weight_kernel", kernel, stream, batch, sample_ids, batch, loader_seed, epoch,
                           mixture_width, alpha, weights, status);
}

int ffcv_augmix_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                                int severity, int mixture_width, int chain_depth, double alpha, int all_ops,
                                const double *table, int height, int width, uint8_t *op, uint8_t *cj_apply,
                                double *cj_ratio, uint8_t *tone_apply, uint8_t *tone_bits, uint8_t *aff_apply,
                                int64_t *aff_coef, uint8_t *sharp_apply, float *sharp_factor, uint8_t *depth,
                                float *weights) {
  const RaArrays o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!am_draw_args_ok("ffcv_augmix_draw_batch_host", sample_ids, batch, severity, mixture_width, chain_depth, alpha,
                       table, height, width, o, depth, weights))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_augmix_draw_batch_host", batch, [&](int k) {
    return draw_augmix_chains(k, batch, sample_ids[k], loader_seed, epoch, severity, mixture_width, chain_depth,
                              all_ops != 0, table, height, width, o, depth) |
           (alpha == 1.0   ? draw_augmix_weights<0>(k, batch, sample_ids[k], loader_seed, epoch, mixture_width, alpha, weights)
            : alpha < 1.0 ? draw_augmix_weights<1>(k, batch, sample_ids[k], loader_seed, epoch, mixture_width, alpha, weights)
                          : draw_augmix_weights<2>(k, batch, sample_ids[k], loader_seed, epoch, mixture_width, alpha,
                                                   weights));
  });
}

uint64_t ffcv_augmix_lds_bytes(void) { return AM_LDS_BYTES; }

int ffcv_augmix_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                      int mixture_width, int mode, const uint8_t *fill, const uint8_t *op, const uint8_t *cj_apply,
                      const double *cj_ratio, const uint8_t *tone_apply, const uint8_t *tone_bits,
                      const uint8_t *aff_apply, const int64_t *aff_coef, const uint8_t *sharp_apply,
                      const float *sharp_factor, const uint8_t *depth, const float *weights) {
  const char *who = "ffcv_augmix_batch";
  const bool pointers = fill && op && cj_apply && cj_ratio && tone_apply && tone_bits && aff_apply && aff_coef &&
                        sharp_apply && sharp_factor && depth && weights;
  uint64_t stride;
  if (!ffcv::out_of_place_ok(who, pointers, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM, 0, &stride))
    return FFCV_EINVAL;
  if (mixture_width < 1 || mixture_width > AM_MAX_WIDTH) {
    ffcv::set_error("%s: mixture width %d, outside 1 to %d", who, mixture_width, AM_MAX_WIDTH);
    return FFCV_EINVAL;
  }
  if (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) {
    ffcv::set_error("%s: mode %d is neither FFCV_AFFINE_BILINEAR nor FFCV_AFFINE_NEAREST", who, mode);
    return FFCV_EINVAL;
  }
  if ((uint64_t)height * width * 9u > AM_LDS_BYTES) {
    ffcv::set_error("%s: images of %dx%d exceed the fused regime (9 H W <= %d): run the chains' launches instead", who,
                    height, width, AM_LDS_BYTES);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  const RaIn A = {op, cj_ratio, tone_bits, aff_coef, sharp_factor};
  const uint32_t f = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
  return ffcv::launch_tiles(who, "augmix_kernel", augmix_kernel, stream, (uint64_t)batch, RA_THREADS, 0, src, dst,
                            batch, height, width, mixture_width, mode, f, A, depth, weights);
}

int ffcv_augmix_mix_batch(void *stream, const uint8_t *orig, const uint8_t *r0, const uint8_t *r1, const uint8_t *r2,
                          const uint8_t *r3, int mixture_width, const float *weights, uint8_t *out, int batch,
                          int height, int width) {
  const char *who = "ffcv_augmix_mix_batch";
  const uint8_t *const r[AM_MAX_WIDTH] = {r0, r1, r2, r3};
  uint64_t img;
  if (!am_mix_args_ok(who, orig, r, mixture_width, weights, out, batch, height, width, &img)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  AmMixIn in = {{orig, r0, r1, r2, r3}};
  for (int i = mixture_width + 1; i <= AM_MAX_WIDTH; i++) in.img[i] = nullptr;
  const uint64_t blocks_per_img = (((img + 30) >> 4) + 255) / 256;
  return ffcv::launch_tiles(who, "augmix_mix_kernel", augmix_mix_kernel, stream, (uint64_t)batch * blocks_per_img, 256, 0,
                            in, mixture_width, weights, out, (uint32_t)batch, (uint32_t)img, (uint32_t)blocks_per_img);
}

int ffcv_augmix_mix_batch_host(const uint8_t *orig, const uint8_t *r0, const uint8_t *r1, const uint8_t *r2,
                               const uint8_t *r3, int mixture_width, const float *weights, uint8_t *out, int batch,
                               int height, int width, int nthreads) {
  const uint8_t *const r[AM_MAX_WIDTH] = {r0, r1, r2, r3};
  uint64_t img;
  if (!am_mix_args_ok("ffcv_augmix_mix_batch_host", orig, r, mixture_width, weights, out, batch, height, width, &img))
    return FFCV_EINVAL;
  ffcv::host_threads(nthreads, batch, [&](std::atomic<uint64_t> &next, int, int) {
    for (uint64_t k = next.fetch_add(1); k < (uint64_t)batch; k = next.fetch_add(1)) {
      for (uint64_t b = k * img; b < (k + 1) * img; b++) {
        float acc = augmix_first(weights[k], (float)orig[b]);
        for (int i = 0; i < mixture_width; i++)
          acc = augmix_add(acc, weights[(uint64_t)(i + 1) * (uint64_t)batch + k], (float)r[i][b]);
        out[b] = (uint8_t)augmix_byte(acc);
      }
    }
  });
  return FFCV_OK;
}

}  // extern "C"
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
