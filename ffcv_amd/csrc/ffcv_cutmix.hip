// ffcv_cutmix.hip -- ImageCutMix (CutMix: https://arxiv.org/abs/1905.04899)
// on the device, with its host twin.
//
//   out[i] = in[i];  out[i][y1:y2, x1:x2, :] = in[i - 1][y1:y2, x1:x2, :]
//
// A sample is planes x height rows of width * pixel_bytes bytes, dense, the
// samples outermost: NHWC of any dtype is planes = 1, pixel_bytes = C *
// itemsize; contiguous NCHW is planes = C, pixel_bytes = itemsize.  The box
// applies to every plane.  Sample i's neighbour is i - 1, or the LAST sample
// of i's own batch when i is the batch's first; batches are runs of batch_size
// samples (the last may be shorter), so a launch group of several batches is
// one call (as in ffcv_mixup.hip).  Boxes are (y1, x1, y2, x2) in pixels, one
// per batch (same_box) or one per sample, and are clamped to the image here:
// whatever the device buffer holds, no access leaves the batch.
//
// Kernel form.  The operation is a select, so the kernel moves bytes and never
// interprets them.  A thread owns 16 bytes of byte offsets of a sample (a
// piece) and walks a run of up to CUT_RUN consecutive samples of one batch; it
// locates its piece's row once (the only integer divisions).  For each sample
// a piece that lies in one row and wholly on one side of the box is ONE
// 16-byte load, from in[i] outside the box or from in[i - 1] inside it, and
// one 16-byte store: every output byte is written once and costs one read.
// All of a run's loads are issued before the first store.  A piece that
// straddles a box edge or a row end, and the last, partial piece of a sample,
// is resolved byte by byte with a running (column, row) pair: a full piece as
// 16 byte loads, each from its own side, then the stores (these
// pieces are what the kernel costs over a copy).  The 16-byte
// accesses sit at the data's own addresses, whatever their alignment (gfx950
// takes unaligned dwordx4 accesses; in and out may be aligned differently).
// No byte outside [in, in + n * sample_bytes) is read and none outside the
// same range of out written.

#include "api_internal.h"

#define CUT_THREADS 256
#define CUT_RUN 4  // as mixup_kernel

namespace {

typedef uint32_t CutChunk __attribute__((ext_vector_type(4)));  // 16 bytes, moved whole

__device__ inline CutChunk cut_load(const uint8_t *p) {
  CutChunk c;
  __builtin_memcpy(&c, p, 16);
  return c;
}

__device__ inline void cut_store(uint8_t *p, CutChunk c) { __builtin_memcpy(p, &c, 16); }

// A box in the units of the copy: rows [y1, y2) of every plane, bytes
// [xb1, xb2) of a row; clamped to the image, empty when y1 >= y2 or xb1 >= xb2.
struct CutBox {
  uint32_t y1, y2, xb1, xb2;
};

__host__ __device__ inline uint32_t cut_clamp(int32_t v, uint32_t hi) {
  return v < 0 ? 0u : ((uint32_t)v > hi ? hi : (uint32_t)v);
}

__host__ __device__ inline CutBox cut_box(const int32_t *b, uint32_t height, uint32_t width, uint32_t pixel_bytes) {
  CutBox x;
  x.y1 = cut_clamp(b[0], height);
  x.y2 = cut_clamp(b[2], height);
  x.xb1 = cut_clamp(b[1], width) * pixel_bytes;
  x.xb2 = cut_clamp(b[3], width) * pixel_bytes;
  return x;
}

// Where the 16 bytes from column byte col of row y come from: 0 the sample
// itself (wholly outside the box), 1 its neighbour (wholly inside), 2 both.
__device__ inline int cut_side(const CutBox &bx, uint32_t y, uint32_t col) {
  const bool rows = y >= bx.y1 && y < bx.y2 && bx.xb1 < bx.xb2;
  if (!rows || col + 16 <= bx.xb1 || col >= bx.xb2) return 0;
  return col >= bx.xb1 && col + 16 <= bx.xb2 ? 1 : 2;
}

// blockIdx.x = run * chunk_blocks + chunk block.  Run r of the launch is run
// r % runs_per_batch of batch r / runs_per_batch: samples [i0, i0 + cnt).
template <int R>
__global__ void __launch_bounds__(CUT_THREADS)
    cutmix_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t n, uint32_t sample_bytes,
                  uint32_t row_bytes, uint32_t height, uint32_t width, uint32_t pixel_bytes, uint32_t planes,
                  uint64_t batch_size, const int32_t *__restrict__ boxes, int same_box, uint32_t chunk_blocks,
                  uint32_t runs_per_batch) {
  const uint32_t run = blockIdx.x / chunk_blocks, cb = blockIdx.x - run * chunk_blocks;
  const uint64_t s = run / runs_per_batch, k0 = (uint64_t)(run - s * runs_per_batch) * R;
  const uint64_t b0 = s * batch_size;                                    // the batch's first sample
  const uint64_t len = n - b0 < batch_size ? n - b0 : batch_size;        // its length
  if (k0 >= len) return;
  const uint64_t i0 = b0 + k0;
  const int cnt = (int)(len - k0 < (uint64_t)R ? len - k0 : (uint64_t)R);
  const uint64_t c64 = ((uint64_t)cb * CUT_THREADS + threadIdx.x) * 16;  // this thread's first byte
  if (c64 >= sample_bytes) return;
  const uint32_t c = (uint32_t)c64;
  const uint64_t ip = k0 == 0 ? b0 + len - 1 : i0 - 1;                   // the run's first neighbour

  // the piece's place in the sample: row r of planes * height, column byte col
  const uint32_t r = c / row_bytes, col = c - r * row_bytes;
  const uint32_t y = planes == 1 ? r : r % height;
  const uint32_t left = sample_bytes - c;                                // bytes from c to the sample's end
  const bool one_row = left >= 16 && col + 16 <= row_bytes;

  // The whole pieces of the run: one 16-byte load each, all issued before the
  // first store.  Bit k of `mixed`: sample k's piece crosses a box edge, a row
  // end or the sample's end.
  static_assert(R == 4, "the run's pieces are four named registers");
  uint32_t mixed = 0;
  CutChunk v0, v1, v2, v3;
  // (a macro, not an array: each piece stays a value of its own, so that a
  // lane that skips a load costs the others no copy and no wait)
#define CUT_LOAD(k, v)                                                                               \
  if (k < cnt) {                                                                                     \
    const CutBox bx = cut_box(boxes + 4 * (same_box ? s : i0 + k), height, width, pixel_bytes);      \
    const int side = one_row ? cut_side(bx, y, col) : 2;                                             \
    if (side == 2)                                                                                   \
      mixed |= 1u << k;                                                                              \
    else                                                                                             \
      v = cut_load(in + (side == 0 ? i0 + k : (k == 0 ? ip : i0 + k - 1)) * sample_bytes + c);       \
  }
#define CUT_STORE(k, v) \
  if (k < cnt && !(mixed >> k & 1)) cut_store(out + (i0 + k) * sample_bytes + c, v);
  CUT_LOAD(0, v0) CUT_LOAD(1, v1) CUT_LOAD(2, v2) CUT_LOAD(3, v3)
  if (!mixed && cnt == R) {  // nearly every lane: four stores behind one wait
    cut_store(out + i0 * sample_bytes + c, v0);
    cut_store(out + (i0 + 1) * sample_bytes + c, v1);
    cut_store(out + (i0 + 2) * sample_bytes + c, v2);
    cut_store(out + (i0 + 3) * sample_bytes + c, v3);
    return;
  }
  CUT_STORE(0, v0) CUT_STORE(1, v1) CUT_STORE(2, v2) CUT_STORE(3, v3)
#undef CUT_LOAD
#undef CUT_STORE
  if (!mixed) return;

  // The mixed pieces, byte by byte, (cc, yy) following the byte's column and
  // row: a full piece as 16 loads, then 16 stores; a sample's last, shorter
  // piece one byte after the other.
#pragma unroll 1
  for (int k = 0; k < cnt; k++) {
    if (!(mixed >> k & 1)) continue;
    const CutBox bx = cut_box(boxes + 4 * (same_box ? s : i0 + k), height, width, pixel_bytes);
    const uint8_t *a = in + (i0 + k) * sample_bytes + c;
    const uint8_t *b = in + (k == 0 ? ip : i0 + k - 1) * sample_bytes + c;
    uint8_t *o = out + (i0 + k) * sample_bytes + c;
    uint32_t cc = col, yy = y;
    if (left >= 16) {
      uint8_t t[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const bool inside = yy >= bx.y1 && yy < bx.y2 && cc >= bx.xb1 && cc < bx.xb2;
        const uint8_t *p = inside ? b : a;
        t[j] = p[j];
        if (++cc == row_bytes) {
          cc = 0;
          if (++yy == height) yy = 0;
        }
      }
#pragma unroll
      for (int j = 0; j < 16; j++) o[j] = t[j];
      continue;
    }
#pragma unroll 1
    for (uint32_t j = 0; j < left; j++) {
      const bool inside = yy >= bx.y1 && yy < bx.y2 && cc >= bx.xb1 && cc < bx.xb2;
      const uint8_t *p = inside ? b : a;
      o[j] = p[j];
      if (++cc == row_bytes) {
        cc = 0;
        if (++yy == height) yy = 0;
      }
    }
  }
}

struct CutDims {
  uint64_t n, bs;
  uint32_t planes, height, width, pixel_bytes, row_bytes, sample_bytes;
};

int cut_check(const char *who, const void *in, const void *out, int64_t n, int32_t planes, int32_t height,
              int32_t width, int32_t pixel_bytes, int64_t batch_size, const int32_t *boxes, CutDims *d) {
  if (!in || !out || !boxes) {
    ffcv::set_error("%s: null pointer (in %p, out %p, boxes %p)", who, in, out, (const void *)boxes);
    return FFCV_EINVAL;
  }
  if (n <= 0 || planes <= 0 || height <= 0 || width <= 0 || batch_size <= 0) {
    ffcv::set_error("%s: n_samples %lld, planes %d, height %d, width %d and batch_size %lld must be > 0", who,
                    (long long)n, planes, height, width, (long long)batch_size);
    return FFCV_EINVAL;
  }
  if (pixel_bytes < 1 || pixel_bytes > 64) {
    ffcv::set_error("%s: pixel_bytes %d is outside 1..64", who, pixel_bytes);
    return FFCV_EINVAL;
  }
  const uint64_t row = (uint64_t)width * (uint64_t)pixel_bytes;           // < 2^37
  const uint64_t rows = (uint64_t)planes * (uint64_t)height;              // < 2^62
  if (rows > 0x7fffffffull / row || (uint64_t)n > (1ull << 62) / (rows * row)) {
    ffcv::set_error("%s: %lld samples of %d x %d x %d pixels of %d bytes overflow (a sample holds at most 2^31 - 1 "
                    "bytes)", who, (long long)n, planes, height, width, pixel_bytes);
    return FFCV_EINVAL;
  }
  const uint64_t bytes = (uint64_t)n * rows * row;
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
  if (a < b + bytes && b < a + bytes) {
    ffcv::set_error("%s: in and out overlap (a sample's neighbour is read after it may have been written)", who);
    return FFCV_EINVAL;
  }
  d->n = (uint64_t)n;
  d->bs = (uint64_t)batch_size < d->n ? (uint64_t)batch_size : d->n;
  d->planes = (uint32_t)planes;
  d->height = (uint32_t)height;
  d->width = (uint32_t)width;
  d->pixel_bytes = (uint32_t)pixel_bytes;
  d->row_bytes = (uint32_t)row;
  d->sample_bytes = (uint32_t)(rows * row);
  return FFCV_OK;
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_cutmix_batch(void *stream, const void *in, void *out, int64_t n_samples, int32_t planes, int32_t height,
                      int32_t width, int32_t pixel_bytes, int64_t batch_size, const int32_t *boxes, int same_box) {
  CutDims d;
  if (cut_check("ffcv_cutmix_batch", in, out, n_samples, planes, height, width, pixel_bytes, batch_size, boxes, &d))
    return FFCV_EINVAL;
  constexpr uint64_t per_block = (uint64_t)CUT_THREADS * 16;
  const uint64_t chunk_blocks = (d.sample_bytes + per_block - 1) / per_block;
  const uint64_t runs_per_batch = (d.bs + CUT_RUN - 1) / CUT_RUN;
  const uint64_t runs = ((d.n + d.bs - 1) / d.bs) * runs_per_batch;
  if (runs > 0x7fffffffull || chunk_blocks * runs > 0x7fffffffull) {
    ffcv::set_error("ffcv_cutmix_batch: %llu x %llu workgroups exceed one launch", (unsigned long long)chunk_blocks,
                    (unsigned long long)runs);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL((cutmix_kernel<CUT_RUN>), dim3((unsigned)(chunk_blocks * runs)), dim3(CUT_THREADS), 0,
                     ffcv::as_stream(stream), (const uint8_t *)in, (uint8_t *)out, d.n, d.sample_bytes, d.row_bytes,
                     d.height, d.width, d.pixel_bytes, d.planes, d.bs, boxes, same_box != 0, (uint32_t)chunk_blocks,
                     (uint32_t)runs_per_batch);
  FFCV_LAUNCH_CHECK("cutmix_kernel");
  return FFCV_OK;
}

int ffcv_cutmix_batch_host(const void *in, void *out, int64_t n_samples, int32_t planes, int32_t height, int32_t width,
                           int32_t pixel_bytes, int64_t batch_size, const int32_t *boxes, int same_box, int nthreads) {
  CutDims d;
  if (cut_check("ffcv_cutmix_batch_host", in, out, n_samples, planes, height, width, pixel_bytes, batch_size, boxes,
                &d))
    return FFCV_EINVAL;
  const uint8_t *src = (const uint8_t *)in;
  uint8_t *dst = (uint8_t *)out;
  const uint64_t bs = (uint64_t)batch_size;
  ffcv::host_threads(nthreads, n_samples, [&](std::atomic<uint64_t> &next, int, int) {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= d.n) return;
      const uint64_t s = i / bs, b0 = s * bs, len = d.n - b0 < bs ? d.n - b0 : bs;
      const uint64_t nb = i == b0 ? b0 + len - 1 : i - 1;
      const CutBox bx = cut_box(boxes + 4 * (same_box ? s : i), d.height, d.width, d.pixel_bytes);
      const uint8_t *a = src + i * d.sample_bytes, *b = src + nb * d.sample_bytes;
      uint8_t *o = dst + i * d.sample_bytes;
      if (bx.y1 >= bx.y2 || bx.xb1 >= bx.xb2) {
        std::memcpy(o, a, d.sample_bytes);
        continue;
      }
      const uint64_t plane = (uint64_t)d.height * d.row_bytes;
      for (uint32_t p = 0; p < d.planes; p++) {
        const uint64_t at = p * plane, top = (uint64_t)bx.y1 * d.row_bytes, bot = (uint64_t)bx.y2 * d.row_bytes;
        std::memcpy(o + at, a + at, top);                                 // the rows above the box
        for (uint64_t q = at + top; q < at + bot; q += d.row_bytes) {
          std::memcpy(o + q, a + q, bx.xb1);
          std::memcpy(o + q + bx.xb1, b + q + bx.xb1, bx.xb2 - bx.xb1);
          std::memcpy(o + q + bx.xb2, a + q + bx.xb2, d.row_bytes - bx.xb2);
        }
        std::memcpy(o + at + bot, a + at + bot, plane - bot);             // and below it
      }
    }
  });
  return FFCV_OK;
}

}  // extern "C"
