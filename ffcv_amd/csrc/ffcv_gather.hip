// ffcv_gather.hip -- fixed-size row gather out of the resident .beton bytes
// (NDArrayDecoder on the device: ndarray.py:19-45, one my_memcpy per sample
// there, one launch per launch group here).
//
//   out[k * out_stride : + row_bytes] = base[row_off[ids[k]] : + row_bytes]
//
// bit for bit, the id -> offset lookup inside the kernel.  The writer's
// allocator does not align regions, so a row starts at any byte offset and
// source and destination disagree in every residue mod 16.
//
// Row copy.  The destination row is cut into a head of fewer than 16 bytes up
// to the first 16-byte boundary, a body of whole 16-byte vectors, and a tail
// of fewer than 16 bytes.  Every body vector is one aligned dwordx4 store.
// Its 16 source bytes start at byte b = source address mod 4 (the same b for
// every vector of the row) of an aligned dword: the lane loads the four
// aligned dwords from there as one dwordx4 and, when b != 0, the dword behind
// them, and funnels neighbouring pairs together with v_alignbyte_b32, so the
// copy is as wide for every value of (source - destination) mod 16.  Head and
// tail bytes go one per lane (byte load, byte store): they are the only
// accesses narrower than a vector, and a row shorter than 16 bytes is all
// head and tail.
//
// Bounds.  Loads touch the bytes of the row and, in the body, the aligned
// dwords that hold at least one of them; `base` is 16-byte aligned, so every
// byte read lies in an aligned 16-byte word that holds a byte of a valid row,
// below the next multiple of 16 past base_bytes.  Stores touch the row_bytes
// bytes of each output row and status[k].  A row whose id is >= n_rows, or
// whose bytes do not lie inside [0, base_bytes) (compared without forming
// off + row_bytes), is not read at all: its output is zero-filled by the same
// stores and status[k] = FFCV_SAMPLE_RANGE.
//
// Dispatch (by row_bytes, on the host):
//   row_bytes <= GATHER_SUBWAVE_BYTES  16 lanes per row, 16 rows per workgroup
//   row_bytes <  GATHER_LARGE_BYTES    one wave per row, 4 rows per workgroup
//   otherwise                          grid (chunks of 16 KiB, rows): each
//                                      workgroup keeps four vectors per lane
//                                      in flight; rows beyond 65535 and chunks
//                                      beyond the grid are looped over
// GATHER_LARGE_BYTES was measured.
// The decoders' two simple gathers (sample descriptors, raw sample bytes) live here too.
#include "api_internal.h"

#define GATHER_THREADS 256
#define GATHER_SUBWAVE_BYTES 256    // 16 lanes x 16 bytes: one pass of a quarter wave
#define GATHER_LARGE_BYTES 12288    // measured cut-over to the 2-D grid
#define GATHER_UNROLL 4             // vectors per lane in flight in the 2-D kernel
#define GATHER_CHUNK_VECS (GATHER_THREADS * GATHER_UNROLL)
#define GATHER_MAX_GRID_X 4096
#define GATHER_MAX_GRID_Y 65535

// --------------------------------------------- simple (raw) gather -------
__global__ void __launch_bounds__(256) gather_raw_kernel(const uint8_t *__restrict__ base,
                                                         const ffcv_sample *__restrict__ samples,
                                                         uint8_t *__restrict__ out, uint64_t stride) {
  const int k = blockIdx.y;
  const ffcv_sample s = samples[k];
  if (s.mode != 1) return;
  const uint8_t *src = base + s.offset;
  uint8_t *dst = out + stride * k;
  uint64_t n = s.size;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    dst[i] = src[i];
}

__global__ void __launch_bounds__(256) gather_samples_kernel(const ffcv_sample *__restrict__ table, uint64_t n,
                                                             const uint64_t *__restrict__ ids, int B,
                                                             ffcv_sample *__restrict__ out) {
  int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= B) return;
  uint64_t i = ids[k];
  ffcv_sample s;
  if (i < n) {
    s = table[i];
  } else {  // out-of-range index: an empty jpg sample -> BAD_MARKER status
    s.offset = 0;
    s.size = 0;
    s.height = s.width = 1;
    s.mode = 0;
    s.reserved = 0;
  }
  out[k] = s;
}

namespace {

// a dwordx4 load at a dword-aligned (not 16-byte-aligned) address
struct __attribute__((packed, aligned(4))) Dwords4 {
  uint32_t x, y, z, w;
};

// One row of the launch, resolved: where it is read and written and how its
// destination splits into head / body / tail.
struct Row {
  const uint8_t *src;  // first source byte (unused when bad)
  uint8_t *dst;
  uint32_t head, tail, b;  // b: (source address of the first body vector) mod 4
  uint64_t nvec;
  bool bad;
};

__device__ __forceinline__ Row resolve_row(const uint8_t *base, uint64_t base_bytes, const uint64_t *row_off,
                                           uint64_t n_rows, const uint64_t *ids, uint64_t k, uint64_t row_bytes,
                                           uint8_t *out, uint64_t out_stride) {
  Row R;
  const uint64_t id = ids[k];
  uint64_t off = 0;
  R.bad = id >= n_rows;
  if (!R.bad) {
    off = row_off[id];
    R.bad = off > base_bytes || row_bytes > base_bytes - off;
  }
  if (R.bad) off = 0;
  R.src = base + off;
  R.dst = out + k * out_stride;
  const uint64_t to_boundary = (16 - ((uintptr_t)R.dst & 15)) & 15;
  R.head = (uint32_t)(to_boundary < row_bytes ? to_boundary : row_bytes);
  const uint64_t rest = row_bytes - R.head;
  R.nvec = rest >> 4;
  R.tail = (uint32_t)(rest & 15);
  R.b = (uint32_t)((uintptr_t)(R.src + R.head) & 3);
  return R;
}

// body vector i of the row as loaded: the four aligned dwords that hold its
// first 13 bytes and, when b != 0, the dword behind them (when b == 0 the
// fourth again: no branch, and no byte beyond the vector)
struct Raw {
  Dwords4 lo;
  uint32_t x4;
};

__device__ __forceinline__ Raw load_raw(const Row &R, uint64_t i) {
  Raw w = {{0, 0, 0, 0}, 0};
  if (R.bad) return w;
  const uint32_t *p = (const uint32_t *)(R.src + R.head - R.b) + 4 * i;
  w.lo = *(const Dwords4 *)p;
  w.x4 = p[R.b ? 4 : 3];
  return w;
}

// ... funnelled together: the vector's 16 bytes
__device__ __forceinline__ uint4 realign(const Row &R, const Raw &w) {
  return make_uint4(__builtin_amdgcn_alignbyte(w.lo.y, w.lo.x, R.b), __builtin_amdgcn_alignbyte(w.lo.z, w.lo.y, R.b),
                    __builtin_amdgcn_alignbyte(w.lo.w, w.lo.z, R.b), __builtin_amdgcn_alignbyte(w.x4, w.lo.w, R.b));
}

__device__ __forceinline__ uint4 load_body(const Row &R, uint64_t i) { return realign(R, load_raw(R, i)); }

__device__ __forceinline__ void store_body(const Row &R, uint64_t i, uint4 v) {
  *((uint4 *)(R.dst + R.head) + i) = v;
}

// head and tail, one byte per lane: lanes [0, 16) of the caller's group
__device__ __forceinline__ void copy_peels(const Row &R, uint64_t row_bytes, uint32_t lane) {
  if (lane < R.head) R.dst[lane] = R.bad ? (uint8_t)0 : R.src[lane];
  if (lane < R.tail) {
    const uint64_t at = row_bytes - R.tail + lane;
    R.dst[at] = R.bad ? (uint8_t)0 : R.src[at];
  }
}

// LANES lanes per row, GATHER_THREADS / LANES rows per workgroup
template <int LANES>
__global__ void __launch_bounds__(GATHER_THREADS)
    gather_rows_kernel(const uint8_t *__restrict__ base, uint64_t base_bytes, const uint64_t *__restrict__ row_off,
                       uint64_t n_rows, const uint64_t *__restrict__ ids, uint32_t batch, uint64_t row_bytes,
                       uint8_t *__restrict__ out, uint64_t out_stride, int32_t *__restrict__ status) {
  constexpr uint32_t ROWS = GATHER_THREADS / LANES;
  const uint32_t lane = threadIdx.x % LANES;
  const uint64_t k = (uint64_t)blockIdx.x * ROWS + threadIdx.x / LANES;
  if (k >= batch) return;
  const Row R = resolve_row(base, base_bytes, row_off, n_rows, ids, k, row_bytes, out, out_stride);
  if (lane == 0) status[k] = R.bad ? FFCV_SAMPLE_RANGE : FFCV_SAMPLE_OK;
  copy_peels(R, row_bytes, lane);
  for (uint64_t i = lane; i < R.nvec; i += LANES) store_body(R, i, load_body(R, i));
}

// grid (chunks, rows): workgroup (x, y) copies chunks x, x + gridDim.x, ... of
// rows y, y + gridDim.y, ...; the workgroups with x == 0 also do the peels
__global__ void __launch_bounds__(GATHER_THREADS)
    gather_rows_grid_kernel(const uint8_t *__restrict__ base, uint64_t base_bytes,
                            const uint64_t *__restrict__ row_off, uint64_t n_rows, const uint64_t *__restrict__ ids,
                            uint32_t batch, uint64_t row_bytes, uint8_t *__restrict__ out, uint64_t out_stride,
                            int32_t *__restrict__ status) {
  for (uint64_t k = blockIdx.y; k < batch; k += gridDim.y) {
    const Row R = resolve_row(base, base_bytes, row_off, n_rows, ids, k, row_bytes, out, out_stride);
    if (blockIdx.x == 0) {
      if (threadIdx.x == 0) status[k] = R.bad ? FFCV_SAMPLE_RANGE : FFCV_SAMPLE_OK;
      if (threadIdx.x < 16) copy_peels(R, row_bytes, threadIdx.x);
    }
    for (uint64_t v0 = (uint64_t)blockIdx.x * GATHER_CHUNK_VECS; v0 < R.nvec;
         v0 += (uint64_t)gridDim.x * GATHER_CHUNK_VECS) {
      // all loads of the chunk are issued before the first is used; a whole
      // chunk (every one but a row's last) runs without per-lane bounds
      Raw w[GATHER_UNROLL];
      if (v0 + GATHER_CHUNK_VECS <= R.nvec) {
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++) w[u] = load_raw(R, v0 + (uint64_t)u * GATHER_THREADS + threadIdx.x);
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++)
          store_body(R, v0 + (uint64_t)u * GATHER_THREADS + threadIdx.x, realign(R, w[u]));
      } else {
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++) {
          const uint64_t i = v0 + (uint64_t)u * GATHER_THREADS + threadIdx.x;
          if (i < R.nvec) w[u] = load_raw(R, i);
        }
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; u++) {
          const uint64_t i = v0 + (uint64_t)u * GATHER_THREADS + threadIdx.x;
          if (i < R.nvec) store_body(R, i, realign(R, w[u]));
        }
      }
    }
  }
}

enum { SHAPE_AUTO = 0, SHAPE_SUBWAVE = 1, SHAPE_WAVE = 2, SHAPE_GRID = 3 };

}  // namespace

extern "C" {

int ffcv_gather_samples(void *stream, const ffcv_sample *table, uint64_t n_table, const uint64_t *ids,
                        int batch, ffcv_sample *out) {
  if (!table || !ids || !out || batch < 0) {
    ffcv::set_error("ffcv_gather_samples: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  hipLaunchKernelGGL(gather_samples_kernel, dim3((batch + 255) / 256), dim3(256), 0, ffcv::as_stream(stream),
                     table, n_table, ids, batch, out);
  FFCV_LAUNCH_CHECK("gather_samples_kernel");
  return FFCV_OK;
}

// gather_raw_kernel takes the image from blockIdx.y, and a grid has at most
// 65,535 rows: a larger batch is launched in slices of that many images, with
// the per-image pointers advanced.
int ffcv_gather_raw_batch(void *stream, const uint8_t *base, const ffcv_sample *samples, int batch,
                          uint8_t *out, uint64_t out_stride) {
  if (batch < 0 || !base || !samples || !out || !out_stride) {
    ffcv::set_error("ffcv_gather_raw_batch: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  unsigned gx = (unsigned)((out_stride + 255) / 256);
  if (gx > 64) gx = 64;
  for (int64_t k0 = 0; k0 < batch; k0 += GATHER_MAX_GRID_Y) {
    const unsigned slice = (unsigned)(batch - k0 < GATHER_MAX_GRID_Y ? batch - k0 : GATHER_MAX_GRID_Y);
    hipLaunchKernelGGL(gather_raw_kernel, dim3(gx, slice), dim3(256), 0, ffcv::as_stream(stream), base,
                       samples + k0, out + out_stride * k0, out_stride);
    FFCV_LAUNCH_CHECK("gather_raw_kernel");
  }
  return FFCV_OK;
}

uint64_t ffcv_gather_rows_cutover(void) { return GATHER_LARGE_BYTES; }
uint64_t ffcv_gather_rows_subwave(void) { return GATHER_SUBWAVE_BYTES; }

// Diagnostics (not in ffcv_hip.h): ffcv_gather_rows with the dispatch shape
// forced (1: 16 lanes per row, 2: a wave per row, 3: the 2-D grid; 0: by
// row_bytes), for the sweep that chose GATHER_LARGE_BYTES.
int ffcv_gather_rows_shape(void *stream, const uint8_t *base, uint64_t base_bytes, const uint64_t *row_off,
                           uint64_t n_rows, const uint64_t *ids, int batch, uint64_t row_bytes, uint8_t *out,
                           uint64_t out_stride, int32_t *status, int shape) {
  if (!base || !row_off || !ids || !out || !status || batch < 0) {
    ffcv::set_error("ffcv_gather_rows: invalid arguments (null pointer or negative batch)");
    return FFCV_EINVAL;
  }
  if (row_bytes == 0 || out_stride < row_bytes) {
    ffcv::set_error("ffcv_gather_rows: invalid row_bytes %llu / out_stride %llu", (unsigned long long)row_bytes,
                    (unsigned long long)out_stride);
    return FFCV_EINVAL;
  }
  if ((uintptr_t)base & 15) {
    ffcv::set_error("ffcv_gather_rows: invalid base, not 16-byte aligned");
    return FFCV_EINVAL;
  }
  if (shape < SHAPE_AUTO || shape > SHAPE_GRID) {
    ffcv::set_error("ffcv_gather_rows_shape: invalid shape %d", shape);
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  if (shape == SHAPE_AUTO)
    shape = row_bytes <= GATHER_SUBWAVE_BYTES ? SHAPE_SUBWAVE : row_bytes < GATHER_LARGE_BYTES ? SHAPE_WAVE : SHAPE_GRID;
  hipStream_t s = ffcv::as_stream(stream);
  const uint32_t b = (uint32_t)batch;
  if (shape == SHAPE_SUBWAVE) {
    hipLaunchKernelGGL(gather_rows_kernel<16>, dim3((b + 15) / 16), dim3(GATHER_THREADS), 0, s, base, base_bytes,
                       row_off, n_rows, ids, b, row_bytes, out, out_stride, status);
  } else if (shape == SHAPE_WAVE) {
    hipLaunchKernelGGL(gather_rows_kernel<64>, dim3((b + 3) / 4), dim3(GATHER_THREADS), 0, s, base, base_bytes,
                       row_off, n_rows, ids, b, row_bytes, out, out_stride, status);
  } else {
    uint64_t gx = ((row_bytes >> 4) + GATHER_CHUNK_VECS - 1) / GATHER_CHUNK_VECS;
    gx = gx < 1 ? 1 : gx > GATHER_MAX_GRID_X ? GATHER_MAX_GRID_X : gx;
    const uint32_t gy = b > GATHER_MAX_GRID_Y ? GATHER_MAX_GRID_Y : b;
    hipLaunchKernelGGL(gather_rows_grid_kernel, dim3((uint32_t)gx, gy), dim3(GATHER_THREADS), 0, s, base, base_bytes,
                       row_off, n_rows, ids, b, row_bytes, out, out_stride, status);
  }
  FFCV_LAUNCH_CHECK("gather_rows_kernel");
  return FFCV_OK;
}

int ffcv_gather_rows(void *stream, const uint8_t *base, uint64_t base_bytes, const uint64_t *row_off,
                     uint64_t n_rows, const uint64_t *ids, int batch, uint64_t row_bytes, uint8_t *out,
                     uint64_t out_stride, int32_t *status) {
  return ffcv_gather_rows_shape(stream, base, base_bytes, row_off, n_rows, ids, batch, row_bytes, out, out_stride,
                                status, SHAPE_AUTO);
}

}  // extern "C"
