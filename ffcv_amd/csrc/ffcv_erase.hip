// ffcv_erase.hip -- RandomErasing (https://arxiv.org/abs/1708.04896, with
// torchvision's get_params and timm's per-pixel noise) on the device, with its
// host twins: the draw (op id 21, one lane per sample) and the fill, in place.
//
// A sample is planes x height rows of width * pixel_bytes bytes, dense, the
// samples outermost (the geometry of ffcv_cutmix.hip).  The box (y, x, h, w)
// of a sample, clamped to the image here, is filled in every plane, with one
// pixel pattern per plane (constant mode) or with a table entry chosen by a
// hash of the element's index in its sample (noise mode, erase_common.h).
// The kernels move bytes and table entries and never interpret them, so one
// kernel family serves uint8, float16 and float32.
//
// Kernel form.  The grid is sized for the largest box: a
// workgroup is (sample, plane, band) with blockIdx.x the sample, and takes the
// band's share of the box's rows in its plane.  It loads its sample's box
// through the scalar cache and leaves at once when nothing is erased.  Its
// threads walk the 16-byte pieces of the box's row segments, pieces cut at
// 16-byte-aligned ADDRESSES: a piece wholly inside a row's segment is one
// 16-byte store, a row's first and last piece go element by element.  A thread
// finds its first (row, piece) with one division and steps through the rest
// with a running pair.
//   constant: the workgroup expands its plane's pixel to 96 bytes of LDS
//     (pattern[i % pixel_bytes]); a piece is the 16 bytes from its phase, read
//     as five aligned words and shifted (one modulo per piece, none per byte).
//   noise: a piece of 16 / itemsize elements takes the splitmix64 words of its
//     4-element groups once (one more when the piece does not start on a
//     group), funnel-shifted so that element j reads bits of word j / 4; the
//     workgroup stages the table (4, 8 or 16 KiB) in LDS once.  The form that
//     reads it through the cache instead is kept for tools/erase_bench.py: it
//     takes 1.5 to 2 times as long on ImageNet-shape batches.
// No byte outside the box is written: the pieces' stores are either whole
// inside a row's segment or predicated per element.

#include "api_internal.h"
#include "erase_common.h"

#define ERASE_THREADS 256
// Workgroups per (sample, plane), DESIGN.md s26: 4 in a launch group of many
// batches, 8 while the launch has at most ERASE_SMALL (sample, plane) pairs
// (one batch), where 4 leave the chip short of workgroups.
#define ERASE_BANDS 4
#define ERASE_BANDS_SMALL 8
#define ERASE_SMALL 2048
#define ERASE_EXT_BYTES 96 // the expanded pixel: phase < 64, + 16 bytes, + the shift's look-ahead

namespace {

typedef uint32_t EraseChunk __attribute__((ext_vector_type(4)));  // 16 bytes, stored whole

template <int ITEM> struct EraseItem;
template <> struct EraseItem<1> { typedef uint8_t type; };
template <> struct EraseItem<2> { typedef uint16_t type; };
template <> struct EraseItem<4> { typedef uint32_t type; };

// Elements [lo, hi) (byte bounds, multiples of ITEM) of the piece at q.
template <int ITEM>
__device__ __forceinline__ void erase_store_part(uint8_t *q, EraseChunk c, int lo, int hi) {
  typedef typename EraseItem<ITEM>::type T;
#pragma unroll
  for (int j = 0; j < 16; j += ITEM)
    if (j >= lo && j < hi) *(T *)(q + j) = (T)(c[j >> 2] >> (8 * (j & 3)));
}

// The pieces of rows [0, nrows) of a workgroup: row r's segment is the `len`
// bytes from sample + first + r * row_bytes.  piece(off, rel): the 16 bytes of
// the piece that starts at byte off of the sample (negative in front of it),
// rel bytes from its row segment's start (-15..).
template <int ITEM, class Piece>
__device__ __forceinline__ void erase_rows(uint8_t *sample, uint32_t first, uint32_t row_bytes, uint32_t nrows,
                                           uint32_t len, Piece piece) {
  const uint32_t ppr = (len + 15) / 16 + 1;              // pieces of a row, at most
  uint32_t r = threadIdx.x / ppr, k = threadIdx.x - r * ppr;
  const uint32_t dr = ERASE_THREADS / ppr, dk = ERASE_THREADS - dr * ppr;
  while (r < nrows) {
    const uint32_t off = first + r * row_bytes;
    uint8_t *p = sample + off;
    const int32_t rel = (int32_t)(16 * k) - (int32_t)((uint32_t)(uintptr_t)p & 15u);
    const int32_t end = (int32_t)len - rel;               // from the piece's start to the segment's end
    if (end > 0) {
      const EraseChunk c = piece((int32_t)off + rel, rel);
      uint8_t *q = p + rel;
      if (rel >= 0 && end >= 16)
        *(EraseChunk *)q = c;
      else
        erase_store_part<ITEM>(q, c, rel < 0 ? -rel : 0, end < 16 ? end : 16);
    }
    k += dk;
    r += dr;
    if (k >= ppr) {
      k -= ppr;
      ++r;
    }
  }
}

// What a workgroup does: sample blockIdx.x, plane and band from blockIdx.y.
struct EraseWork {
  uint8_t *sample;
  uint32_t plane, first, nrows, len;
};

__device__ __forceinline__ bool erase_work(uint8_t *images, const int32_t *__restrict__ boxes, uint32_t sample_bytes,
                                           uint32_t row_bytes, uint32_t height, uint32_t width, uint32_t pixel_bytes,
                                           uint32_t bands, EraseWork *w) {
  const int32_t *b = boxes + 4 * (uint64_t)blockIdx.x;   // uniform: one scalar load
  const int32_t bh = b[2], bw = b[3];
  if (bh <= 0 || bw <= 0) return false;
  EraseBox bx;
  if (!erase_box(b[0], b[1], bh, bw, height, width, pixel_bytes, &bx)) return false;
  const uint32_t plane = blockIdx.y / bands, band = blockIdx.y - plane * bands;
  const uint32_t per = (bx.y2 - bx.y1 + bands - 1) / bands;
  const uint32_t r0 = bx.y1 + band * per;
  if (r0 >= bx.y2) return false;
  w->sample = images + (uint64_t)blockIdx.x * sample_bytes;
  w->plane = plane;
  w->first = (plane * height + r0) * row_bytes + bx.xb1;
  w->nrows = bx.y2 - r0 < per ? bx.y2 - r0 : per;
  w->len = bx.len;
  return true;
}

__global__ void __launch_bounds__(ERASE_THREADS)
    erase_constant_kernel(uint8_t *images, uint32_t sample_bytes, uint32_t row_bytes, uint32_t height, uint32_t width,
                          uint32_t pixel_bytes, uint32_t bands, const int32_t *__restrict__ boxes,
                          const uint8_t *__restrict__ pattern) {
  EraseWork w;
  if (!erase_work(images, boxes, sample_bytes, row_bytes, height, width, pixel_bytes, bands, &w)) return;
  __shared__ uint32_t ext[ERASE_EXT_BYTES / 4];
  if (threadIdx.x < ERASE_EXT_BYTES)
    ((uint8_t *)ext)[threadIdx.x] = pattern[w.plane * pixel_bytes + threadIdx.x % pixel_bytes];
  __syncthreads();
  const uint32_t bias = 16 * pixel_bytes;                // a multiple of the pixel, >= 15
  erase_rows<1>(w.sample, w.first, row_bytes, w.nrows, w.len, [&](int32_t, int32_t rel) {
    const uint32_t ph = (uint32_t)(rel + (int32_t)bias) % pixel_bytes;
    const uint32_t *d = ext + (ph >> 2);
    const uint32_t s = 8 * (ph & 3);
    EraseChunk c;
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> s);
    return c;
  });
}

// The 16 / ITEM elements from element e (negative in front of the sample:
// those are never stored).
template <int ITEM, class Lookup>
__device__ __forceinline__ EraseChunk erase_noise_piece(uint64_t key, int32_t e, Lookup table) {
  constexpr int E = 16 / ITEM, NW = E / 4;
  const uint32_t ph = (uint32_t)e & 3u, sh = 16 * ph;
  const int64_t w0 = (int64_t)(e >> 2);
  uint64_t W[NW + 1];
#pragma unroll
  for (int i = 0; i < NW; i++) W[i] = splitmix64(key ^ (uint64_t)(w0 + i));
  W[NW] = ph ? splitmix64(key ^ (uint64_t)(w0 + NW)) : 0;
  EraseChunk c = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < NW; i++) {
    // elements 4 i .. 4 i + 3 of the piece, 16 bits each
    const uint64_t v = (W[i] >> sh) | ((W[i + 1] << 1) << (63 - sh));
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t val = (uint32_t)table((uint32_t)(v >> (16 * j + 4)) & 0xFFFu);
      const int at = (4 * i + j) * ITEM;                  // the element's byte in the piece
      c[at >> 2] |= val << (8 * (at & 3));
    }
  }
  return c;
}

template <int ITEM, bool STAGE>
__global__ void __launch_bounds__(ERASE_THREADS)
    erase_noise_kernel(uint8_t *images, uint32_t sample_bytes, uint32_t row_bytes, uint32_t height, uint32_t width,
                       uint32_t pixel_bytes, uint32_t bands, const int32_t *__restrict__ boxes,
                       const void *__restrict__ table, const uint64_t *__restrict__ keys) {
  typedef typename EraseItem<ITEM>::type T;
  EraseWork w;
  if (!erase_work(images, boxes, sample_bytes, row_bytes, height, width, pixel_bytes, bands, &w)) return;
  const uint64_t key = keys[blockIdx.x];
  constexpr int shift = ITEM == 1 ? 0 : (ITEM == 2 ? 1 : 2);
  if constexpr (STAGE) {
    __shared__ __attribute__((aligned(16))) T lds[ERASE_TABLE];
    const EraseChunk *src = (const EraseChunk *)table;
#pragma unroll
    for (int i = 0; i < ITEM; i++) ((EraseChunk *)lds)[i * ERASE_THREADS + threadIdx.x] = src[i * ERASE_THREADS + threadIdx.x];
    __syncthreads();
    erase_rows<ITEM>(w.sample, w.first, row_bytes, w.nrows, w.len, [&](int32_t off, int32_t) {
      return erase_noise_piece<ITEM>(key, off >> shift, [&](uint32_t i) { return lds[i]; });
    });
  } else {
    const T *tab = (const T *)table;
    erase_rows<ITEM>(w.sample, w.first, row_bytes, w.nrows, w.len, [&](int32_t off, int32_t) {
      return erase_noise_piece<ITEM>(key, off >> shift, [&](uint32_t i) { return tab[i]; });
    });
  }
}

__global__ void __launch_bounds__(64) erase_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed,
                                                        uint64_t epoch, double p, double s0, double s1, double r0,
                                                        double r1, int H, int W, int32_t *__restrict__ boxes,
                                                        uint64_t *__restrict__ keys, int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_erase(k, ids[k], loader_seed, epoch, p, s0, s1, r0, r1, H, W, boxes, keys);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

bool erase_draw_args_ok(const char *who, const void *ids, int batch, double p, const double *scale,
                        const double *ratio, int height, int width, const void *boxes) {
  if (!ids || !boxes || !scale || !ratio || batch < 0) {
    ffcv::set_error("%s: null pointer or batch %d < 0", who, batch);
    return false;
  }
  if (!(p >= 0.0 && p <= 1.0) || !(scale[0] >= 0.0 && scale[0] <= scale[1] && scale[1] <= 1.0) ||
      !(ratio[0] > 0.0 && ratio[0] <= ratio[1] && std::isfinite(ratio[1]))) {
    ffcv::set_error("%s: p %g, scale (%g, %g) or ratio (%g, %g) out of range", who, p, scale[0], scale[1], ratio[0],
                    ratio[1]);
    return false;
  }
  if (height < 1 || height > 32767 || width < 1 || width > 32767) {
    ffcv::set_error("%s: height %d and width %d must lie in 1..32767", who, height, width);
    return false;
  }
  return true;
}

struct EraseDims {
  uint64_t n;
  uint32_t planes, height, width, pixel_bytes, row_bytes, sample_bytes;
};

int erase_check(const char *who, const void *images, int64_t n, int32_t planes, int32_t height, int32_t width,
                int32_t pixel_bytes, const int32_t *boxes, int mode, int32_t itemsize, const void *fill,
                const uint64_t *keys, EraseDims *d) {
  if (mode != FFCV_ERASE_CONSTANT && mode != FFCV_ERASE_NOISE) {
    ffcv::set_error("%s: mode %d is neither FFCV_ERASE_CONSTANT nor FFCV_ERASE_NOISE", who, mode);
    return FFCV_EINVAL;
  }
  if (!images || !boxes || !fill || (mode == FFCV_ERASE_NOISE && !keys)) {
    ffcv::set_error("%s: null pointer (images %p, boxes %p, fill %p, keys %p)", who, images, (const void *)boxes,
                    fill, (const void *)keys);
    return FFCV_EINVAL;
  }
  if (n <= 0 || planes <= 0 || height <= 0 || width <= 0) {
    ffcv::set_error("%s: n_samples %lld, planes %d, height %d and width %d must be > 0", who, (long long)n, planes,
                    height, width);
    return FFCV_EINVAL;
  }
  if (pixel_bytes < 1 || pixel_bytes > 64) {
    ffcv::set_error("%s: pixel_bytes %d is outside 1..64", who, pixel_bytes);
    return FFCV_EINVAL;
  }
  if (mode == FFCV_ERASE_NOISE) {
    if (itemsize != 1 && itemsize != 2 && itemsize != 4) {
      ffcv::set_error("%s: itemsize %d is not 1, 2 or 4", who, itemsize);
      return FFCV_EINVAL;
    }
    if (pixel_bytes % itemsize) {
      ffcv::set_error("%s: pixel_bytes %d is no multiple of itemsize %d", who, pixel_bytes, itemsize);
      return FFCV_EINVAL;
    }
    if ((uintptr_t)images % (uintptr_t)itemsize) {
      ffcv::set_error("%s: images %p are not aligned to itemsize %d", who, images, itemsize);
      return FFCV_EINVAL;
    }
  }
  const uint64_t row = (uint64_t)width * (uint64_t)pixel_bytes;           // < 2^37
  const uint64_t rows = (uint64_t)planes * (uint64_t)height;              // < 2^62
  if (rows > 0x7fffffffull / row || (uint64_t)n > (1ull << 62) / (rows * row)) {
    ffcv::set_error("%s: %lld samples of %d x %d x %d pixels of %d bytes overflow (a sample holds at most 2^31 - 1 "
                    "bytes)", who, (long long)n, planes, height, width, pixel_bytes);
    return FFCV_EINVAL;
  }
  d->n = (uint64_t)n;
  d->planes = (uint32_t)planes;
  d->height = (uint32_t)height;
  d->width = (uint32_t)width;
  d->pixel_bytes = (uint32_t)pixel_bytes;
  d->row_bytes = (uint32_t)row;
  d->sample_bytes = (uint32_t)(rows * row);
  return FFCV_OK;
}

template <int ITEM>
void erase_noise_launch(bool stage, dim3 grid, hipStream_t s, uint8_t *images, const EraseDims &d, uint32_t bands,
                        const int32_t *boxes, const void *table, const uint64_t *keys) {
  if (stage)
    hipLaunchKernelGGL((erase_noise_kernel<ITEM, true>), grid, dim3(ERASE_THREADS), 0, s, images, d.sample_bytes,
                       d.row_bytes, d.height, d.width, d.pixel_bytes, bands, boxes, table, keys);
  else
    hipLaunchKernelGGL((erase_noise_kernel<ITEM, false>), grid, dim3(ERASE_THREADS), 0, s, images, d.sample_bytes,
                       d.row_bytes, d.height, d.width, d.pixel_bytes, bands, boxes, table, keys);
}

int erase_launch(const char *who, void *stream, void *images, int64_t n_samples, int32_t planes, int32_t height,
                 int32_t width, int32_t pixel_bytes, const int32_t *boxes, int mode, int32_t itemsize,
                 const void *fill, const uint64_t *keys, int bands, int stage) {
  EraseDims d;
  if (erase_check(who, images, n_samples, planes, height, width, pixel_bytes, boxes, mode, itemsize, fill, keys, &d))
    return FFCV_EINVAL;
  if (mode == FFCV_ERASE_NOISE && (uintptr_t)fill % 16) {
    ffcv::set_error("%s: the noise table %p is not aligned to 16 bytes", who, fill);
    return FFCV_EINVAL;
  }
  if (bands == 0) bands = d.n * d.planes <= ERASE_SMALL ? ERASE_BANDS_SMALL : ERASE_BANDS;
  if (d.n > 0x7fffffffull || d.planes > 65535u || bands < 1) {
    ffcv::set_error("%s: %llu samples of %u planes in %d bands exceed one launch (2^31 - 1 samples, 65,535 planes)",
                    who, (unsigned long long)d.n, d.planes, bands);
    return FFCV_EINVAL;
  }
  uint32_t nb = std::min<uint32_t>((uint32_t)bands, std::min<uint32_t>(d.height, 65535u / d.planes));
  const dim3 grid((unsigned)d.n, d.planes * nb);
  hipStream_t s = ffcv::as_stream(stream);
  uint8_t *im = (uint8_t *)images;
  if (mode == FFCV_ERASE_CONSTANT) {
    hipLaunchKernelGGL(erase_constant_kernel, grid, dim3(ERASE_THREADS), 0, s, im, d.sample_bytes, d.row_bytes,
                       d.height, d.width, d.pixel_bytes, nb, boxes, (const uint8_t *)fill);
    FFCV_LAUNCH_CHECK("erase_constant_kernel");
    return FFCV_OK;
  }
  if (itemsize == 1)
    erase_noise_launch<1>(stage != 0, grid, s, im, d, nb, boxes, fill, keys);
  else if (itemsize == 2)
    erase_noise_launch<2>(stage != 0, grid, s, im, d, nb, boxes, fill, keys);
  else
    erase_noise_launch<4>(stage != 0, grid, s, im, d, nb, boxes, fill, keys);
  FFCV_LAUNCH_CHECK("erase_noise_kernel");
  return FFCV_OK;
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_erase_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                          double p, const double scale[2], const double ratio[2], int height, int width,
                          int32_t *boxes, uint64_t *keys, int32_t *status) {
  if (!erase_draw_args_ok("ffcv_erase_draw_batch", sample_ids, batch, p, scale, ratio, height, width, boxes))
    return FFCV_EINVAL;
  return ffcv::launch_draw("erase_draw_kernel", erase_draw_kernel, stream, batch, sample_ids, batch, loader_seed,
                           epoch, p, scale[0], scale[1], ratio[0], ratio[1], height, width, boxes, keys, status);
}

int ffcv_erase_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, double p,
                               const double scale[2], const double ratio[2], int height, int width, int32_t *boxes,
                               uint64_t *keys) {
  if (!erase_draw_args_ok("ffcv_erase_draw_batch_host", sample_ids, batch, p, scale, ratio, height, width, boxes))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_erase_draw_batch_host", batch, [&](int k) {
    return draw_erase(k, sample_ids[k], loader_seed, epoch, p, scale[0], scale[1], ratio[0], ratio[1], height, width,
                      boxes, keys);
  });
}

int ffcv_erase_batch(void *stream, void *images, int64_t n_samples, int32_t planes, int32_t height, int32_t width,
                     int32_t pixel_bytes, const int32_t *boxes, int mode, int32_t itemsize, const void *fill,
                     const uint64_t *keys) {
  return erase_launch("ffcv_erase_batch", stream, images, n_samples, planes, height, width, pixel_bytes, boxes, mode,
                      itemsize, fill, keys, 0, 1);
}

// Diagnostics (tools/erase_bench.py; not in ffcv_hip.h): the same launch with
// `bands` workgroups per (sample, plane) (0: the product's choice) and, without
// `stage`, the noise table read through the cache.
int ffcv_erase_batch_form(void *stream, void *images, int64_t n_samples, int32_t planes, int32_t height, int32_t width,
                          int32_t pixel_bytes, const int32_t *boxes, int mode, int32_t itemsize, const void *fill,
                          const uint64_t *keys, int bands, int stage) {
  return erase_launch("ffcv_erase_batch_form", stream, images, n_samples, planes, height, width, pixel_bytes, boxes,
                      mode, itemsize, fill, keys, bands, stage);
}

int ffcv_erase_batch_host(void *images, int64_t n_samples, int32_t planes, int32_t height, int32_t width,
                          int32_t pixel_bytes, const int32_t *boxes, int mode, int32_t itemsize, const void *fill,
                          const uint64_t *keys, int nthreads) {
  EraseDims d;
  if (erase_check("ffcv_erase_batch_host", images, n_samples, planes, height, width, pixel_bytes, boxes, mode,
                  itemsize, fill, keys, &d))
    return FFCV_EINVAL;
  uint8_t *im = (uint8_t *)images;
  const uint8_t *f = (const uint8_t *)fill;
  ffcv::host_threads(nthreads, n_samples, [&](std::atomic<uint64_t> &next, int, int) {
    for (uint64_t i = next.fetch_add(1); i < d.n; i = next.fetch_add(1)) {
      const int32_t *b = boxes + 4 * i;
      EraseBox bx;
      if (!erase_box(b[0], b[1], b[2], b[3], d.height, d.width, d.pixel_bytes, &bx)) continue;
      uint8_t *sample = im + i * d.sample_bytes;
      for (uint32_t p = 0; p < d.planes; p++)
        for (uint32_t y = bx.y1; y < bx.y2; y++) {
          const uint32_t off = (p * d.height + y) * d.row_bytes + bx.xb1;
          if (mode == FFCV_ERASE_CONSTANT) {
            for (uint32_t q = 0; q < bx.len; q += d.pixel_bytes)
              std::memcpy(sample + off + q, f + p * d.pixel_bytes, d.pixel_bytes);
            continue;
          }
          const uint32_t isz = (uint32_t)itemsize;
          for (uint32_t q = 0; q < bx.len; q += isz) {
            const uint32_t e = (off + q) / isz;
            const uint32_t idx = erase_index(splitmix64(keys[i] ^ (uint64_t)(e >> 2)), e);
            std::memcpy(sample + off + q, f + (uint64_t)idx * isz, isz);
          }
        }
    }
  });
  return FFCV_OK;
}

}  // extern "C"
