// ffcv_augmix_large.hip -- AugMix's fused pixel pass for images beyond
// 64 x 64, up to 224 x 224: the bytes of ffcv_augmix_batch
// from ONE image buffer in LDS.
//
//   augmix_large_kernel: persistent workgroups of 1024 threads, one per CU
//     (the image buffer and the slot scratch of ral_slot.h fill its LDS);
//     workgroup g takes images g, g + grid, ...  Such an image fits in LDS
//     once, not three times, and its 150,528 float32 accumulators fit in no
//     register file, so a chain's result leaves the CU as BYTES:
//       - chain i stages the original again (any alignment, as
//         randaugment_large_kernel does) and runs its slots 3 i .. 3 i +
//         depth - 1 in the buffer through ral_slot;
//       - the results of chains 0 .. width - 2 go to the workgroup's own slab
//         of the workspace, result i in 16-byte stores, laid out in the phase
//         of the image's place in dst: byte b of the image is byte
//         (dst0 & 15) + b of the result;
//       - the last chain's result stays in LDS;
//       - the mix follows in the same launch: a thread owns aligned 16-byte
//         chunks of the output, takes x from memory at any alignment
//         (am_load16), y_0 .. y_{width-2} from the slab as aligned chunks,
//         y_{width-1} from LDS, runs the arithmetic of augmix_mix.h in chain
//         order, and stores the chunk once.
//     The slab is the workgroup's alone, so what orders its writes before the
//     mix's reads, and those before the next image's writes, is the
//     __syncthreads() that the LDS buffer needs at the same places anyway.
//
// The workspace is one slab per workgroup, whatever the batch: the grid is
// min(batch, slabs).  Per image at width 3 the original is read four times
// (three stagings and the mix), two results are written and read back, and
// the output is written once.
//
// 122 VGPRs (four waves per SIMD may use 128), no scratch; LDS as
// randaugment_large_kernel and the loops' own state: 154,848 bytes.
#if defined(__HIP_DEVICE_COMPILE__)
// every float32 product and sum of the stencil and of the mix is an
// instruction of its own
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "api_internal.h"
#include "augmix_mix.h"
#include "ral_slot.h"

// 16 bytes of LDS from byte address sp on, at any alignment, from five aligned
// dwords (the image buffer keeps the look-ahead, as for write_back_rows)
FFCV_DEV lds_x4_t aml_lds16(const uint8_t *sp) {
  const uint32_t *q = (const uint32_t *)__builtin_align_down(sp, 4);
  const uint32_t sh = (uint32_t)(sp - (const uint8_t *)q);
  const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
  lds_x4_t o;
  o.x = __builtin_amdgcn_alignbyte(q1, q0, sh);
  o.y = __builtin_amdgcn_alignbyte(q2, q1, sh);
  o.z = __builtin_amdgcn_alignbyte(q3, q2, sh);
  o.w = __builtin_amdgcn_alignbyte(q4, q3, sh);
  return o;
}

// What the loops over images and chains need between two slots.  It waits in
// LDS: the slot code fills the scalar registers (ral_slot.h), and what is live
// across it there or in vector registers spills.
struct AmlArgs {
  uint64_t src, dst;  // addresses
  const uint8_t *depth;
  const float *weights;
  glb_x4_t *slab;  // the workgroup's slab: result i at slab + i * res_chunks
  RaIn A;
  int B, H, W, width, mode;
  uint32_t fill, nbytes, res_chunks, grid;
};
FFCV_DEV uint32_t aml_s(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
FFCV_DEV uint64_t aml_s(uint64_t v) { return (uint64_t)aml_s((uint32_t)v) | (uint64_t)aml_s((uint32_t)(v >> 32)) << 32; }
FFCV_DEV int aml_s(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <class P>
FFCV_DEV P *aml_s(P *p) {
  return (P *)(uintptr_t)aml_s((uint64_t)(uintptr_t)p);
}

// ws: 16-byte aligned, gridDim.x slabs of max(width - 1, 1) results of
// res_bytes = 16 * lds_chunks(3 H0 W0) bytes each
template <class T>
__global__ void __launch_bounds__(T::THREADS)
    augmix_large_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int B, int H0, int W0, int width,
                        int mode, uint32_t fill0, RaIn A0, const uint8_t *__restrict__ depth,
                        const float *__restrict__ weights, uint8_t *ws, uint32_t res_bytes) {
  __shared__ lds_x4_t s_buf[T::CHUNKS];  // the image
  __shared__ uint32_t s_hist[3 * 256];   // the channel histograms
  __shared__ uint8_t s_tab[3 * 256];     // the slot's table: one, or one per channel
  __shared__ uint32_t s_part[3][T::WAVES];
  __shared__ uint64_t s_occ[3][4];
  __shared__ AmlArgs s_args;
  const int t0 = threadIdx.x;
  uint8_t *const s_mem = (uint8_t *)s_buf;
  const RalScratch<T> lds = {s_hist, s_tab, s_part, s_occ};
  if (t0 == 0)
    s_args = {(uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst, depth, weights,
              (glb_x4_t *)(ws + (uint64_t)blockIdx.x * (uint32_t)max(width - 1, 1) * res_bytes), A0, B, H0, W0, width, mode,
              fill0, 3u * (uint32_t)H0 * (uint32_t)W0, res_bytes >> 4, gridDim.x};
  __syncthreads();
  const AmlArgs &P = s_args;

  for (uint32_t k = blockIdx.x; k < (uint32_t)aml_s(P.B); k += aml_s(P.grid)) {
    const int nchains = aml_s(P.width);
    uint32_t cur_off = 0;
    for (int i = 0; i < nchains; i++) {
      // ---- stage the original behind the buffer's 16 front bytes.  (The
      // barrier behind the passes that read the buffer is in front of this.)
      {
        const uint32_t nbytes = aml_s(P.nbytes);  // <= T::IMG_BYTES
        const uint64_t src0 = aml_s(P.src) + (uint64_t)k * nbytes;
        stage_rows<T::THREADS>(t0, src0, 0, 1, nbytes, (int)lds_chunks(nbytes), s_buf + 1);
        cur_off = 16u + (uint32_t)(src0 & 15);
      }
      __syncthreads();
      const int d = min(AM_MAX_DEPTH, max(1, aml_s((int)aml_s(P.depth)[(uint64_t)i * (uint32_t)aml_s(P.B) + k])));
      for (int j = 0; j < d; j++) {
        const RaIn A = {aml_s(P.A.op), aml_s(P.A.cj_ratio), aml_s(P.A.tone_bits), aml_s(P.A.aff_coef),
                        aml_s(P.A.sharp_factor)};
        ral_slot<T>(t0, aml_s(P.H), aml_s(P.W), aml_s(P.fill), aml_s(P.mode), aml_s(P.B), k, AM_MAX_DEPTH * i + j, A,
                    s_mem, cur_off, lds);
      }
      if (i == nchains - 1) break;
      // ---- the result to the slab, whole chunks in the output's phase (the
      // bytes of the end chunks that are not the image's are never mixed)
      const uint32_t nbytes = aml_s(P.nbytes);
      const uint32_t dl = (uint32_t)((aml_s(P.dst) + (uint64_t)k * nbytes) & 15);
      const uint32_t nch = (dl + nbytes + 15u) >> 4;
      glb_x4_t *const res = aml_s(P.slab) + (uint64_t)i * aml_s(P.res_chunks);
      const uint8_t *const sp = s_mem + cur_off - dl;
      for (uint32_t c = t0; c < nch; c += T::THREADS) res[c] = aml_lds16(sp + 16u * c);
      __syncthreads();
    }

    // ---- the mix: chunk c of the output is bytes [b0, b0 + 16) of the image
    const uint32_t nbytes = aml_s(P.nbytes), B0 = (uint32_t)aml_s(P.B), res_chunks = aml_s(P.res_chunks);
    const uint64_t src0 = aml_s(P.src) + (uint64_t)k * nbytes, dst0 = aml_s(P.dst) + (uint64_t)k * nbytes;
    const uint32_t dl = (uint32_t)(dst0 & 15);      // the output's phase
    const uint32_t nch = (dl + nbytes + 15u) >> 4;  // aligned chunks of dst that hold a byte of the image
    const float *const weights_k = aml_s(P.weights) + k;
    const glb_x4_t *const slab = aml_s(P.slab);
    float w[1 + AM_MAX_WIDTH];
#pragma unroll
    for (int i = 0; i <= AM_MAX_WIDTH; i++) w[i] = i <= nchains ? weights_k[(uint64_t)i * B0] : 0.0f;
    // (w[nchains], by selects: a register array takes no runtime index)
    float wl = w[1];
#pragma unroll
    for (int i = 2; i <= AM_MAX_WIDTH; i++) wl = i == nchains ? w[i] : wl;
    const uint8_t *const sp = s_mem + cur_off - dl;
    for (uint32_t c = t0; c < nch; c += T::THREADS) {
      const int b0 = 16 * (int)c - (int)dl;
      const int jlo = b0 < 0 ? -b0 : 0, jhi = (int)nbytes - b0 < 16 ? (int)nbytes - b0 : 16;
      float acc[16];
      am_mix16(acc, true, w[0], am_load16(src0 + (uint64_t)(int64_t)b0, jlo, jhi));
#pragma unroll
      for (int i = 0; i < AM_MAX_WIDTH - 1; i++) {
        if (i >= nchains - 1) break;
        am_mix16(acc, false, w[i + 1], slab[(uint64_t)i * res_chunks + c]);
      }
      am_mix16(acc, false, wl, aml_lds16(sp + 16u * c));
      am_store16((uint8_t *)(uintptr_t)((dst0 & ~(uint64_t)15) + 16u * (uint64_t)c), acc, jlo, jhi);
    }
    // the next image's staging and slab stores wait for this one's reads
    __syncthreads();
  }
}

// ---------------------------------------------------------- C ABI -------
namespace {

uint64_t aml_result_bytes(int height, int width) { return 16u * lds_chunks((uint64_t)height * width * 3u); }

bool aml_shape_ok(int height, int width, int mixture_width) {
  return RalTop::fits(height, width) && mixture_width >= 1 && mixture_width <= AM_MAX_WIDTH;
}

}  // namespace

extern "C" {

uint64_t ffcv_augmix_large_slab_bytes(int height, int width, int mixture_width) {
  if (!aml_shape_ok(height, width, mixture_width)) return 0;
  return (uint64_t)std::max(mixture_width - 1, 1) * aml_result_bytes(height, width);
}

uint64_t ffcv_augmix_large_workspace_bytes(int height, int width, int mixture_width) {
  const uint64_t slab = ffcv_augmix_large_slab_bytes(height, width, mixture_width);
  if (!slab) {
    ffcv::set_error("ffcv_augmix_large_workspace_bytes: %dx%d at mixture width %d is outside the kernel's regime", height,
                    width, mixture_width);
    return 0;
  }
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) {
    ffcv::check_hip(e, "ffcv_augmix_large_workspace_bytes: the device's compute units");
    return 0;
  }
  return (uint64_t)std::max(cus, 1) * slab + 16u;
}

int ffcv_augmix_large_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width,
                            int mixture_width, int mode, const uint8_t *fill, const uint8_t *op,
                            const uint8_t *cj_apply, const double *cj_ratio, const uint8_t *tone_apply,
                            const uint8_t *tone_bits, const uint8_t *aff_apply, const int64_t *aff_coef,
                            const uint8_t *sharp_apply, const float *sharp_factor, const uint8_t *depth,
                            const float *weights, void *workspace, uint64_t workspace_bytes) {
  const char *who = "ffcv_augmix_large_batch";
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
  if (!RalTop::fits(height, width)) {
    ffcv::set_error("%s: images of %dx%d are outside the kernel's regime (3 H W <= %d, see "
                    "ffcv_randaugment_large_fits): run the chains' launches instead",
                    who, height, width, RalTop::IMG_BYTES);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  // whole slabs from the workspace's first 16-byte boundary on
  const uint64_t slab = ffcv_augmix_large_slab_bytes(height, width, mixture_width);
  const uintptr_t w0 = (uintptr_t)workspace, w1 = (w0 + 15u) & ~(uintptr_t)15;
  const uint64_t slabs = workspace && workspace_bytes >= w1 - w0 ? (workspace_bytes - (w1 - w0)) / slab : 0;
  if (!slabs) {
    ffcv::set_error("%s: a workspace of %llu bytes holds no slab of %llu bytes (ffcv_augmix_large_slab_bytes)", who,
                    (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)slab);
    return FFCV_EINVAL;
  }
  const uint64_t grid = std::min<uint64_t>((uint64_t)batch, slabs);
  const uintptr_t a0 = (uintptr_t)src, a1 = a0 + (uint64_t)batch * stride, b0 = (uintptr_t)dst;
  if ((w1 < a1 && a0 < w1 + grid * slab) || (w1 < b0 + (uint64_t)batch * stride && b0 < w1 + grid * slab)) {
    ffcv::set_error("%s: the workspace overlaps src or dst", who);
    return FFCV_EINVAL;
  }
  const RaIn A = {op, cj_ratio, tone_bits, aff_coef, sharp_factor};
  const uint32_t f = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
  return ffcv::launch_tiles(who, "augmix_large_kernel", augmix_large_kernel<RalTop>, stream, grid, RalTop::THREADS, 0,
                            src, dst, batch, height, width, mixture_width, mode, f, A, depth, weights,
                            (uint8_t *)w1, (uint32_t)aml_result_bytes(height, width));
}

}  // extern "C"
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
