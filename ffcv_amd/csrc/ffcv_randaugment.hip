// ffcv_randaugment.hip -- RandAugment: the draws (op id 23)
// and the fused pixel pass for images up to 64 x 64, with the draws' host twin.
// (The fused pass for larger images, up to 224 x 224, from a single LDS buffer:
// ffcv_randaugment_large.hip.)
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
//     src, lds_stage.h), every slot's operation runs there (ra_slot.h, shared
//     with AugMix's kernel), and the result leaves once (16-byte aligned stores
//     at any alignment of dst).  The bytes equal those of the s24 launches,
//     slot after slot.
//
// LDS: two image buffers of 12,288 B + 64 B (16 in front for a tap left of
// column 0, 16 for the staged range's lead, 32 of read-ahead) = 24,704, the
// counters 3,072, the tables 768, scan partials 144: 28,688 bytes, five
// workgroups per CU.
#include "api_internal.h"
#include "ra_slot.h"

#define FFCV_RANDAUG_OP 23
#define RA_MAX_SLOTS 8

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
    ra_fill_slot(s, uk, uB, op, ((drawn >> (8 * s)) & 16u) != 0, table[op * nbins + magnitude], H, W, o);
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
  const RaScratch lds = {s_hist, s_tab, s_part, s_occ};

  // ---- stage the image: one byte range, behind buffer 0's 16 front bytes
  const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * nbytes0;
  stage_rows<RA_THREADS>(t0, src0, 0, 1, nbytes0, (int)lds_chunks(nbytes0), s_buf + 1);
  uint32_t cur_off = 16u + (uint32_t)(src0 & 15);  // where in s_mem the current image's first byte is
  __syncthreads();

  for (int s = 0; s < num_ops; s++) {
    // dense, 16-byte aligned, in the buffer that does not hold the current image
    const uint32_t nxt_off = (cur_off < RA_BUF_BYTES ? RA_BUF_BYTES : 0u) + 16u;
    ra_slot(t0, H0, W0, fill0, mode, B, k, s, A, s_mem, cur_off, nxt_off, lds);
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
