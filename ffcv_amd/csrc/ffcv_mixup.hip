// ffcv_mixup.hip -- ImageMixup (mixup.py:39-48) and MixupToOneHot
// (mixup.py:102-109) on the device, with the image mix's host twin.
//
//   out[i] = cast(l_i * double(in[i]) + (1 - l_i) * double(in[i - 1]))
//
// every multiply and add rounded on its own in float64 (never fused), the
// cast truncating for uint8 and rounding to nearest even for float32.  Sample
// i's neighbour is i - 1, or the LAST sample of i's own batch when i is the
// batch's first; batches are runs of batch_size samples (the last may be
// shorter), so a launch group of several batches is one call.
//
// Kernel form.  A thread owns 16 bytes of element offsets of a sample and
// walks a run of up to MIX_RUN consecutive samples of one batch, keeping the
// previous sample's 16 bytes in registers: one extra read per run instead of
// one per sample.  All of a run's loads are issued before the first is used.
// The 16-byte accesses sit at the elements' own addresses, whatever their
// alignment (a uint8 batch may start at any byte, and sample_elems need not be
// a multiple of 16; gfx950 takes unaligned dwordx4 accesses); the last,
// partial 16 bytes of a sample are read and written element by element.  No
// byte outside [in, in + n * elems) is read and none outside the same range
// of out written.  Runs of 4 measured best.

#include "api_internal.h"

#define MIX_THREADS 256
#define MIX_RUN 4  // measured: DESIGN.md s15 (runs of 4 beat 8, 2 and 1 at every shape)

namespace {

// the one pixel function of both the kernels and the host twin
template <typename T>
__host__ __device__ inline T mix_value(double l, double oml, double a, double b);
template <>
__host__ __device__ inline uint8_t mix_value<uint8_t>(double l, double oml, double a, double b) {
  const double m = l * a;
  const double n = oml * b;
  return (uint8_t)(int)(m + n);  // in [0, 255 + 3e-14]: truncation, no clip
}
template <>
__host__ __device__ inline float mix_value<float>(double l, double oml, double a, double b) {
  const double m = l * a;
  const double n = oml * b;
  return (float)(m + n);
}

template <typename T>
struct MixChunk {
  static constexpr int V = 16 / (int)sizeof(T);
  T e[V];
};

// 16 bytes at p, which is aligned to T only
template <typename T>
__device__ inline MixChunk<T> mix_load(const T *p) {
  MixChunk<T> c;
  __builtin_memcpy(&c, p, 16);
  return c;
}

template <typename T>
__device__ inline void mix_store(T *p, const MixChunk<T> &c) {
  __builtin_memcpy(p, &c, 16);
}

// blockIdx.x = run * chunk_blocks + chunk block.  Run r of the launch is run
// r % runs_per_batch of batch r / runs_per_batch: samples [i0, i0 + cnt).
template <typename T, int R>
__global__ void __launch_bounds__(MIX_THREADS)
    mixup_kernel(const T *__restrict__ in, T *__restrict__ out, uint64_t n, uint64_t elems, uint64_t batch_size,
                 const double *__restrict__ lam, int same_lambda, uint32_t chunk_blocks, uint32_t runs_per_batch) {
  constexpr int V = MixChunk<T>::V;
  const uint32_t run = blockIdx.x / chunk_blocks, cb = blockIdx.x - run * chunk_blocks;
  const uint64_t s = run / runs_per_batch, k0 = (uint64_t)(run - s * runs_per_batch) * R;
  const uint64_t b0 = s * batch_size;                                    // the batch's first sample
  const uint64_t len = n - b0 < batch_size ? n - b0 : batch_size;        // its length
  if (k0 >= len) return;
  const uint64_t i0 = b0 + k0;
  const int cnt = (int)(len - k0 < (uint64_t)R ? len - k0 : (uint64_t)R);
  const uint64_t c = ((uint64_t)cb * MIX_THREADS + threadIdx.x) * V;     // this thread's first element
  if (c >= elems) return;
  const uint64_t ip = k0 == 0 ? b0 + len - 1 : i0 - 1;                   // the run's first neighbour
  if (c + V > elems) {
    // the sample's last, partial 16 bytes: element by element (one thread per run)
#pragma unroll 1
    for (int k = 0; k < cnt; k++) {
      const double l = lam[same_lambda ? s : i0 + k];
      const double oml = 1.0 - l;
      const T *a = in + (i0 + k) * elems, *b = in + (k == 0 ? ip : i0 + k - 1) * elems;
      T *o = out + (i0 + k) * elems;
#pragma unroll 1
      for (uint64_t j = c; j < elems; j++) o[j] = mix_value<T>(l, oml, (double)a[j], (double)b[j]);
    }
    return;
  }

  MixChunk<T> prev = mix_load(in + ip * elems + c);
  MixChunk<T> cur[R];
#pragma unroll
  for (int k = 0; k < R; k++)  // past a short run's end: its last sample again, unused
    cur[k] = mix_load(in + (i0 + (k < cnt ? k : cnt - 1)) * elems + c);

#pragma unroll
  for (int k = 0; k < R; k++) {
    if (k >= cnt) break;
    const double l = lam[same_lambda ? s : i0 + k];
    const double oml = 1.0 - l;
    MixChunk<T> o;
#pragma unroll
    for (int j = 0; j < V; j++) o.e[j] = mix_value<T>(l, oml, (double)cur[k].e[j], (double)prev.e[j]);
    mix_store(out + (i0 + k) * elems + c, o);
    prev = cur[k];
    // keep the scheduler from converting every sample's bytes to float64 up
    // front (32 registers per sample; runs of 8 would leave one wave per SIMD)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// out[i][c] = 0, then [a_i] = lam_i, then [b_i] = float(1) - lam_i (the second
// store wins when a_i == b_i).  A row with a label outside [0, classes)
// stays zero and sets status[i].
__global__ void __launch_bounds__(MIX_THREADS)
    mixup_onehot_kernel(const float *__restrict__ labels3, float *__restrict__ out, uint64_t n, uint64_t classes,
                        int32_t *__restrict__ status) {
  const uint64_t j = (uint64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
  if (j >= n * classes) return;
  const uint64_t i = j / classes, c = j - i * classes;
  const float la = labels3[3 * i], lb = labels3[3 * i + 1], lam = labels3[3 * i + 2];
  const float fc = (float)classes;
  const bool ok = la > -1.0f && la < fc && lb > -1.0f && lb < fc;  // false for a NaN
  float v = 0.0f;
  if (ok) {
    const uint64_t a = (uint64_t)(long long)la, b = (uint64_t)(long long)lb;
    if (c == b)
      v = 1.0f - lam;
    else if (c == a)
      v = lam;
  }
  out[j] = v;
  if (c == 0) status[i] = ok ? FFCV_SAMPLE_OK : FFCV_SAMPLE_LABEL;
}

int mix_check(const char *who, const void *in, const void *out, int64_t n, int64_t elems, int dtype, int64_t batch_size,
              const double *lam, uint64_t *bytes) {
  if (!in || !out || !lam) {
    ffcv::set_error("%s: null pointer (in %p, out %p, lam %p)", who, in, out, (const void *)lam);
    return FFCV_EINVAL;
  }
  if (n <= 0 || elems <= 0 || batch_size <= 0) {
    ffcv::set_error("%s: n_samples %lld, sample_elems %lld and batch_size %lld must be > 0", who, (long long)n,
                    (long long)elems, (long long)batch_size);
    return FFCV_EINVAL;
  }
  if (dtype != FFCV_MIXUP_U8 && dtype != FFCV_MIXUP_F32) {
    ffcv::set_error("%s: unknown dtype %d (FFCV_MIXUP_U8 or FFCV_MIXUP_F32)", who, dtype);
    return FFCV_EINVAL;
  }
  const uint64_t sz = dtype == FFCV_MIXUP_F32 ? 4 : 1;
  if ((uint64_t)n > (1ull << 62) / ((uint64_t)elems * sz)) {
    ffcv::set_error("%s: %lld samples of %lld elements overflow", who, (long long)n, (long long)elems);
    return FFCV_EINVAL;
  }
  *bytes = (uint64_t)n * (uint64_t)elems * sz;
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
  if (((a | b) & (sz - 1)) != 0) {
    ffcv::set_error("%s: in and out must be aligned to the element size %llu", who, (unsigned long long)sz);
    return FFCV_EINVAL;
  }
  if (a < b + *bytes && b < a + *bytes) {
    ffcv::set_error("%s: in and out overlap (a sample's neighbour is read after it may have been written)", who);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

template <typename T, int R>
int mix_launch(hipStream_t s, const void *in, void *out, uint64_t n, uint64_t elems, uint64_t batch_size,
               const double *lam, int same_lambda) {
  constexpr uint64_t per_block = (uint64_t)MIX_THREADS * MixChunk<T>::V;
  const uint64_t chunk_blocks = (elems + per_block - 1) / per_block;
  const uint64_t bs = batch_size < n ? batch_size : n;
  const uint64_t runs_per_batch = (bs + R - 1) / R;
  const uint64_t runs = ((n + bs - 1) / bs) * runs_per_batch;
  if (chunk_blocks > 0x7fffffffull || runs > 0x7fffffffull || chunk_blocks * runs > 0x7fffffffull) {
    ffcv::set_error("ffcv_mixup_batch: %llu x %llu workgroups exceed one launch", (unsigned long long)chunk_blocks,
                    (unsigned long long)runs);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL((mixup_kernel<T, R>), dim3((unsigned)(chunk_blocks * runs)), dim3(MIX_THREADS), 0, s,
                     (const T *)in, (T *)out, n, elems, bs, lam, same_lambda, (uint32_t)chunk_blocks,
                     (uint32_t)runs_per_batch);
  FFCV_LAUNCH_CHECK("mixup_kernel");
  return FFCV_OK;
}

template <typename T>
int mix_launch_run(int run, hipStream_t s, const void *in, void *out, uint64_t n, uint64_t elems, uint64_t bs,
                   const double *lam, int same_lambda) {
  switch (run) {
    case 1: return mix_launch<T, 1>(s, in, out, n, elems, bs, lam, same_lambda);
    case 2: return mix_launch<T, 2>(s, in, out, n, elems, bs, lam, same_lambda);
    case 4: return mix_launch<T, 4>(s, in, out, n, elems, bs, lam, same_lambda);
    case 8: return mix_launch<T, 8>(s, in, out, n, elems, bs, lam, same_lambda);
  }
  ffcv::set_error("ffcv_mixup_batch_run: run length %d is not one of 1, 2, 4, 8", run);
  return FFCV_EINVAL;
}

template <typename T>
void mix_host_sample(const T *in, T *out, uint64_t elems, uint64_t i, uint64_t nb, double l) {
  const T *a = in + i * elems, *b = in + nb * elems;
  T *o = out + i * elems;
  const double oml = 1.0 - l;
  for (uint64_t j = 0; j < elems; j++) o[j] = mix_value<T>(l, oml, (double)a[j], (double)b[j]);
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

// Diagnostics (tools/mixup_bench.py; not in ffcv_hip.h): the same kernel
// with an explicit run length.  run == 1 is the plain form in which every
// sample's workgroup reads the sample and its neighbour.
int ffcv_mixup_batch_run(void *stream, const void *in, void *out, int64_t n_samples, int64_t sample_elems, int dtype,
                         int64_t batch_size, const double *lam, int same_lambda, int run) {
  uint64_t bytes = 0;
  if (mix_check("ffcv_mixup_batch", in, out, n_samples, sample_elems, dtype, batch_size, lam, &bytes))
    return FFCV_EINVAL;
  hipStream_t s = ffcv::as_stream(stream);
  if (dtype == FFCV_MIXUP_U8)
    return mix_launch_run<uint8_t>(run, s, in, out, (uint64_t)n_samples, (uint64_t)sample_elems,
                                   (uint64_t)batch_size, lam, same_lambda != 0);
  return mix_launch_run<float>(run, s, in, out, (uint64_t)n_samples, (uint64_t)sample_elems, (uint64_t)batch_size,
                               lam, same_lambda != 0);
}

int ffcv_mixup_batch(void *stream, const void *in, void *out, int64_t n_samples, int64_t sample_elems, int dtype,
                     int64_t batch_size, const double *lam, int same_lambda) {
  return ffcv_mixup_batch_run(stream, in, out, n_samples, sample_elems, dtype, batch_size, lam, same_lambda, MIX_RUN);
}

int ffcv_mixup_batch_host(const void *in, void *out, int64_t n_samples, int64_t sample_elems, int dtype,
                          int64_t batch_size, const double *lam, int same_lambda, int nthreads) {
  uint64_t bytes = 0;
  if (mix_check("ffcv_mixup_batch_host", in, out, n_samples, sample_elems, dtype, batch_size, lam, &bytes))
    return FFCV_EINVAL;
  const uint64_t n = (uint64_t)n_samples, elems = (uint64_t)sample_elems, bs = (uint64_t)batch_size;
  ffcv::host_threads(nthreads, n_samples, [&](std::atomic<uint64_t> &next, int, int) {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= n) return;
      const uint64_t s = i / bs, b0 = s * bs, len = n - b0 < bs ? n - b0 : bs;
      const uint64_t nb = i == b0 ? b0 + len - 1 : i - 1;
      const double l = lam[same_lambda ? s : i];
      if (dtype == FFCV_MIXUP_U8)
        mix_host_sample<uint8_t>((const uint8_t *)in, (uint8_t *)out, elems, i, nb, l);
      else
        mix_host_sample<float>((const float *)in, (float *)out, elems, i, nb, l);
    }
  });
  return FFCV_OK;
}

int ffcv_mixup_onehot_batch(void *stream, const float *labels3, float *out, int64_t n, int64_t num_classes,
                            int32_t *status) {
  if (!labels3 || !out || !status || n <= 0 || num_classes <= 0 || num_classes > (1 << 24) ||
      (uint64_t)n * (uint64_t)num_classes > 0x7fffffffull * MIX_THREADS) {
    ffcv::set_error("ffcv_mixup_onehot_batch: invalid arguments (labels3 %p, out %p, status %p, n %lld, "
                    "num_classes %lld)",
                    (const void *)labels3, (void *)out, (void *)status, (long long)n, (long long)num_classes);
    return FFCV_EINVAL;
  }
  const uint64_t total = (uint64_t)n * (uint64_t)num_classes;
  hipLaunchKernelGGL(mixup_onehot_kernel, dim3((unsigned)((total + MIX_THREADS - 1) / MIX_THREADS)), dim3(MIX_THREADS),
                     0, ffcv::as_stream(stream), labels3, out, (uint64_t)n, (uint64_t)num_classes, status);
  FFCV_LAUNCH_CHECK("mixup_onehot_kernel");
  return FFCV_OK;
}

}  // extern "C"
