// ffcv_poison.hip -- Poison (poisoning.py:46-59) and ReplaceLabel
// (replace_label.py:36-42) on the device, with Poison's host twin.
//
// For every sample whose dataset index is in the sorted set `poison_ids`
//
//   image[e] = uint8(clip(float32(float64(float32(float64(image[e]) * keep[e])) + add[e]), lo, hi))
//
// (poison_common.h), in place; every other sample is neither read nor
// written.  keep = float64(1 - alpha) and add = float64(mask) * alpha are
// float64 tables of one sample's size, the same for every sample.
//
// Kernel form.  A thread owns PSN_BYTES of element offsets of a sample, and a
// workgroup covers a run of up to 64 consecutive samples.  Each wave first
// decides the run's memberships, lane k searching for sample k of the run, and
// a ballot makes the result wave-uniform; a run with no poisoned sample ends
// there, before any table or image load.  Otherwise the thread loads its keep
// / add values once into registers and walks the set bits of the ballot, the
// loads of four poisoned samples in flight together, blending and storing them
// one by one.  The accesses sit at the
// elements' own addresses, whatever their alignment (gfx950 takes unaligned
// dwordx2 / dwordx4 accesses); the last, partial span of a sample goes element
// by element.  No byte outside [images, images + n * elems) is touched.
// 8 bytes per thread and runs of 64 (shorter on small launches) measured best
// (DESIGN.md s16).

#include "api_internal.h"
#include "poison_common.h"

#define PSN_THREADS 256
#define PSN_BYTES 8  // measured: DESIGN.md s16
#define PSN_RUN 64
#define PSN_MIN_RUN 8
#define PSN_MIN_BLOCKS 1024  // halve the run while the launch has fewer workgroups

namespace {

using ffcv::poison_member;
using ffcv::poison_value;

template <int V>
struct PsnChunk {
  uint8_t e[V];
};

#define PSN_GROUP 4  // poisoned samples whose loads are in flight together

// Run r of the launch is samples [r * run, r * run + cnt), run <= 64.
// blockIdx.x = r * chunk_blocks + chunk block, or with chunk_major
// chunk block * runs + r (neighbouring workgroups then share the table chunk).
template <int V>
__global__ void __launch_bounds__(PSN_THREADS)
    poison_kernel(uint8_t *images, uint64_t n, uint64_t elems, const int64_t *__restrict__ sample_ids,
                  const uint64_t *__restrict__ poison_ids, uint64_t n_poison, const double *__restrict__ keep,
                  const double *__restrict__ add, float lo, float hi, uint32_t chunk_blocks, uint32_t runs,
                  uint32_t run_len, int chunk_major) {
  const uint32_t run = chunk_major ? blockIdx.x % runs : blockIdx.x / chunk_blocks;
  const uint32_t cb = chunk_major ? blockIdx.x / runs : blockIdx.x - run * chunk_blocks;
  const uint64_t i0 = (uint64_t)run * run_len;
  const uint32_t cnt = (uint32_t)(n - i0 < (uint64_t)run_len ? n - i0 : (uint64_t)run_len);
  const uint32_t lane = threadIdx.x & 63u;
  bool mine = false;
  if (lane < cnt) mine = poison_member(poison_ids, n_poison, sample_ids[i0 + lane]);
  uint64_t hit = __ballot(mine);  // bit k: sample i0 + k is poisoned (the same in every wave)
  if (hit == 0) return;
  const uint64_t c = ((uint64_t)cb * PSN_THREADS + threadIdx.x) * V;  // this thread's first element
  if (c >= elems) return;
  if (c + V > elems) {
    // the sample's last, partial span: element by element (one thread per run)
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
      if (!((hit >> k) & 1)) continue;
      uint8_t *p = images + (i0 + k) * elems;
#pragma unroll 1
      for (uint64_t j = c; j < elems; j++) p[j] = poison_value(p[j], keep[j], add[j], lo, hi);
    }
    return;
  }

  double kp[V], ad[V];
  __builtin_memcpy(kp, keep + c, V * sizeof(double));
  __builtin_memcpy(ad, add + c, V * sizeof(double));
  uint8_t *base = images + i0 * elems + c;
  // the poisoned samples of the run, PSN_GROUP at a time: hit is wave-uniform,
  // so the walk over its set bits is scalar code
#pragma unroll 1
  while (hit) {
    uint64_t off[PSN_GROUP];  // wave-uniform, like ok
    bool ok[PSN_GROUP];
    PsnChunk<V> cur[PSN_GROUP];
#pragma unroll
    for (int u = 0; u < PSN_GROUP; u++) {
      ok[u] = hit != 0;
      off[u] = 0;
      if (ok[u]) {
        off[u] = (uint64_t)__builtin_ctzll(hit) * elems;
        hit &= hit - 1;
        __builtin_memcpy(&cur[u], base + off[u], V);
      }
    }
#pragma unroll
    for (int u = 0; u < PSN_GROUP; u++) {
      if (ok[u]) {
        PsnChunk<V> o;
#pragma unroll
        for (int j = 0; j < V; j++) o.e[j] = poison_value(cur[u].e[j], kp[j], ad[j], lo, hi);
        __builtin_memcpy(base + off[u], &o, V);
      }
      // keep the scheduler from converting every sample's bytes up front
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// one thread per row of row_elems labels
__global__ void __launch_bounds__(PSN_THREADS)
    replace_label_kernel(int64_t *labels, uint64_t n, uint64_t row_elems, const int64_t *__restrict__ sample_ids,
                         const uint64_t *__restrict__ poison_ids, uint64_t n_poison, int64_t new_label) {
  const uint64_t i = (uint64_t)blockIdx.x * PSN_THREADS + threadIdx.x;
  if (i >= n || !poison_member(poison_ids, n_poison, sample_ids[i])) return;
  for (uint64_t e = 0; e < row_elems; e++) labels[i * row_elems + e] = new_label;
}

int ids_check(const char *who, const void *data, int64_t n, int64_t elems, uint64_t elem_size, const void *sample_ids,
              const void *poison_ids, int64_t n_poison) {
  if (!data || !sample_ids || (n_poison > 0 && !poison_ids)) {
    ffcv::set_error("%s: null pointer (data %p, sample_ids %p, poison_ids %p)", who, data, sample_ids, poison_ids);
    return FFCV_EINVAL;
  }
  if (n <= 0 || elems <= 0 || n_poison < 0) {
    ffcv::set_error("%s: n %lld and elements per sample %lld must be > 0, n_poison %lld >= 0", who, (long long)n,
                    (long long)elems, (long long)n_poison);
    return FFCV_EINVAL;
  }
  if ((uint64_t)n > (1ull << 62) / ((uint64_t)elems * elem_size)) {
    ffcv::set_error("%s: %lld samples of %lld elements overflow", who, (long long)n, (long long)elems);
    return FFCV_EINVAL;
  }
  if ((((uintptr_t)sample_ids | (uintptr_t)poison_ids) & 7) != 0 || ((uintptr_t)data & (elem_size - 1)) != 0) {
    ffcv::set_error("%s: sample_ids and poison_ids must be aligned to 8 bytes, the data to its element size", who);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

int psn_check(const char *who, const void *images, int64_t n, int64_t elems, const void *sample_ids,
              const void *poison_ids, int64_t n_poison, const double *keep, const double *add, float lo, float hi) {
  if (ids_check(who, images, n, elems, 1, sample_ids, poison_ids, n_poison)) return FFCV_EINVAL;
  if (!keep || !add) {
    ffcv::set_error("%s: null pointer (keep %p, add %p)", who, (const void *)keep, (const void *)add);
    return FFCV_EINVAL;
  }
  if ((((uintptr_t)keep | (uintptr_t)add) & 7) != 0) {
    ffcv::set_error("%s: keep and add must be aligned to 8 bytes", who);
    return FFCV_EINVAL;
  }
  if (!(0.0f <= lo && lo <= hi && hi <= 255.0f)) {  // false for a NaN
    ffcv::set_error("%s: clamp (%g, %g) must satisfy 0 <= lo <= hi <= 255", who, (double)lo, (double)hi);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

template <int V>
int psn_launch(hipStream_t s, uint8_t *images, uint64_t n, uint64_t elems, const int64_t *sample_ids,
               const uint64_t *poison_ids, uint64_t n_poison, const double *keep, const double *add, float lo,
               float hi, int run, int chunk_major) {
  if (run < 1 || run > 64) {
    ffcv::set_error("ffcv_poison_batch_form: run length %d is not in [1, 64] (one lane of a wave per sample)", run);
    return FFCV_EINVAL;
  }
  constexpr uint64_t per_block = (uint64_t)PSN_THREADS * V;
  const uint64_t chunk_blocks = (elems + per_block - 1) / per_block;
  const uint64_t runs = (n + (uint64_t)run - 1) / (uint64_t)run;
  if (chunk_blocks > 0x7fffffffull || runs > 0x7fffffffull || chunk_blocks * runs > 0x7fffffffull) {
    ffcv::set_error("ffcv_poison_batch: %llu x %llu workgroups exceed one launch", (unsigned long long)chunk_blocks,
                    (unsigned long long)runs);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL((poison_kernel<V>), dim3((unsigned)(chunk_blocks * runs)), dim3(PSN_THREADS), 0, s, images, n,
                     elems, sample_ids, poison_ids, n_poison, keep, add, lo, hi, (uint32_t)chunk_blocks,
                     (uint32_t)runs, (uint32_t)run, chunk_major);
  FFCV_LAUNCH_CHECK("poison_kernel");
  return FFCV_OK;
}

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

// Diagnostics (tools/poison_bench.py; not in ffcv_hip.h): the same kernel with
// explicit bytes per thread (4, 8 or 16), run length (1 to 64) and workgroup
// order (chunk_major: workgroups that share a table chunk are neighbours).
int ffcv_poison_batch_form(void *stream, uint8_t *images, int64_t n_samples, int64_t sample_elems,
                           const int64_t *sample_ids, const uint64_t *poison_ids, int64_t n_poison, const double *keep,
                           const double *add, float clamp_lo, float clamp_hi, int bytes_per_thread, int run,
                           int chunk_major) {
  if (psn_check("ffcv_poison_batch", images, n_samples, sample_elems, sample_ids, poison_ids, n_poison, keep, add,
                clamp_lo, clamp_hi))
    return FFCV_EINVAL;
  if (n_poison == 0) return FFCV_OK;
  hipStream_t s = ffcv::as_stream(stream);
  const uint64_t n = (uint64_t)n_samples, e = (uint64_t)sample_elems, np = (uint64_t)n_poison;
  const int cm = chunk_major != 0;
  switch (bytes_per_thread) {
    case 4: return psn_launch<4>(s, images, n, e, sample_ids, poison_ids, np, keep, add, clamp_lo, clamp_hi, run, cm);
    case 8: return psn_launch<8>(s, images, n, e, sample_ids, poison_ids, np, keep, add, clamp_lo, clamp_hi, run, cm);
    case 16:
      return psn_launch<16>(s, images, n, e, sample_ids, poison_ids, np, keep, add, clamp_lo, clamp_hi, run, cm);
  }
  ffcv::set_error("ffcv_poison_batch_form: %d bytes per thread is not one of 4, 8, 16", bytes_per_thread);
  return FFCV_EINVAL;
}

int ffcv_poison_batch(void *stream, uint8_t *images, int64_t n_samples, int64_t sample_elems,
                      const int64_t *sample_ids, const uint64_t *poison_ids, int64_t n_poison, const double *keep,
                      const double *add, float clamp_lo, float clamp_hi) {
  // runs of 64 samples amortise the search and the table best, but a small
  // launch needs shorter runs to fill the chip (measured: DESIGN.md s16)
  int run = PSN_RUN;
  if (n_samples > 0 && sample_elems > 0) {
    const uint64_t chunk_blocks = ((uint64_t)sample_elems + PSN_THREADS * PSN_BYTES - 1) / (PSN_THREADS * PSN_BYTES);
    while (run > PSN_MIN_RUN && chunk_blocks * (((uint64_t)n_samples + run - 1) / run) < PSN_MIN_BLOCKS) run >>= 1;
  }
  return ffcv_poison_batch_form(stream, images, n_samples, sample_elems, sample_ids, poison_ids, n_poison, keep, add,
                                clamp_lo, clamp_hi, PSN_BYTES, run, 0);
}

int ffcv_poison_batch_host(uint8_t *images, int64_t n_samples, int64_t sample_elems, const int64_t *sample_ids,
                           const uint64_t *poison_ids, int64_t n_poison, const double *keep, const double *add,
                           float clamp_lo, float clamp_hi, int nthreads) {
  if (psn_check("ffcv_poison_batch_host", images, n_samples, sample_elems, sample_ids, poison_ids, n_poison, keep, add,
                clamp_lo, clamp_hi))
    return FFCV_EINVAL;
  if (n_poison == 0) return FFCV_OK;
  const uint64_t n = (uint64_t)n_samples, elems = (uint64_t)sample_elems;
  ffcv::host_threads(nthreads, n_samples, [&](std::atomic<uint64_t> &next, int, int) {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= n) return;
      if (!poison_member(poison_ids, (uint64_t)n_poison, sample_ids[i])) continue;
      uint8_t *p = images + i * elems;
      for (uint64_t j = 0; j < elems; j++) p[j] = poison_value(p[j], keep[j], add[j], clamp_lo, clamp_hi);
    }
  });
  return FFCV_OK;
}

int ffcv_replace_label_batch(void *stream, int64_t *labels, int64_t n, int64_t row_elems, const int64_t *sample_ids,
                             const uint64_t *poison_ids, int64_t n_poison, int64_t new_label) {
  if (ids_check("ffcv_replace_label_batch", labels, n, row_elems, 8, sample_ids, poison_ids, n_poison))
    return FFCV_EINVAL;
  if (n_poison == 0) return FFCV_OK;
  const uint64_t blocks = ((uint64_t)n + PSN_THREADS - 1) / PSN_THREADS;
  if (blocks > 0x7fffffffull) {
    ffcv::set_error("ffcv_replace_label_batch: %lld rows exceed one launch", (long long)n);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL(replace_label_kernel, dim3((unsigned)blocks), dim3(PSN_THREADS), 0, ffcv::as_stream(stream),
                     labels, (uint64_t)n, (uint64_t)row_elems, sample_ids, poison_ids, (uint64_t)n_poison, new_label);
  FFCV_LAUNCH_CHECK("replace_label_kernel");
  return FFCV_OK;
}

}  // extern "C"
