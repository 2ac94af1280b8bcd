// api_internal.h -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/ffcv_hip.h"

namespace ffcv {
void set_error(const char *fmt, ...);
int check_hip(hipError_t e, const char *what);
inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace ffcv

#define FFCV_HIP_CHECK(expr)                                        \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) return ffcv::check_hip(_e, #expr);        \
  } while (0)

#define FFCV_LAUNCH_CHECK(what)                                      \
  do {                                                               \
    hipError_t _e = hipGetLastError();                               \
    if (_e != hipSuccess) return ffcv::check_hip(_e, what);          \
  } while (0)

// ---- shared by the entries of the uint8 HWC image transforms --------------
namespace ffcv {

// The argument check of an entry that takes a batch of dense uint8
// [batch][height][width][3] images of at most 2^31 - 1 bytes each; pointers:
// every pointer argument the entry needs is there.
inline bool u8_images_ok(const char *who, bool pointers, int batch, int height, int width) {
  if (batch < 0 || !pointers || height <= 0 || width <= 0 || (uint64_t)height * (uint64_t)width * 3 > 0x7fffffffull) {
    set_error("%s: invalid arguments (batch %d, %dx%d)", who, batch, height, width);
    return false;
  }
  return true;
}

// The argument check of both entries (device and host twin) of an operator
// that writes a dense uint8 [batch][height][width][3] batch into another:
// pointers (every pointer argument the entry needs is there), the sizes, sides
// of at most max_dim, the dst stride (0: dense), resolved into *stride, and
// that the batches do not overlap.
inline bool out_of_place_ok(const char *who, bool pointers, const uint8_t *src, const uint8_t *dst, int batch,
                            int height, int width, int max_dim, uint64_t dst_stride, uint64_t *stride) {
  if (!src || !dst || !pointers || batch < 0 || height <= 0 || width <= 0) {
    set_error("%s: invalid arguments", who);
    return false;
  }
  if (height > max_dim || width > max_dim) {
    set_error("%s: images of %dx%d exceed the supported %d per side", who, height, width, max_dim);
    return false;
  }
  const uint64_t img = (uint64_t)height * width * 3;
  *stride = dst_stride ? dst_stride : img;
  if (*stride < img) {
    set_error("%s: dst_stride %llu for images of %llu bytes", who, (unsigned long long)dst_stride,
              (unsigned long long)img);
    return false;
  }
  if (batch > 0) {
    const uintptr_t a0 = (uintptr_t)src, a1 = a0 + (uint64_t)batch * img;
    const uintptr_t b0 = (uintptr_t)dst, b1 = b0 + (uint64_t)(batch - 1) * *stride + img;
    if (a0 < b1 && b0 < a1) {
      set_error("%s: src and dst overlap (the operation is out of place)", who);
      return false;
    }
  }
  return true;
}

// How a pixel-run launch (lds_stage.h) cuts images of npx pixels: the whole
// image per workgroup when its bytes fit lds_bytes, else tiles of tile_px.
inline bool run_tiling(const char *who, int batch, uint64_t npx, uint32_t lds_bytes, uint32_t tile_px,
                       uint32_t *tile_px_out, uint32_t *ntiles, unsigned *blocks) {
  *tile_px_out = npx * 3 <= lds_bytes ? (uint32_t)npx : tile_px;
  const uint64_t nt = (npx + *tile_px_out - 1) / *tile_px_out, nb = (uint64_t)batch * nt;
  if (nb > 0x7fffffffull) {
    set_error("%s: %llu workgroups exceed one launch", who, (unsigned long long)nb);
    return false;
  }
  *ntiles = (uint32_t)nt;
  *blocks = (unsigned)nb;
  return true;
}

// A draw kernel, one lane per sample: kernel(args...) over `batch` samples.
template <class K, class... A>
int launch_draw(const char *name, K kernel, void *stream, int batch, A... args) {
  if (batch == 0) return FFCV_OK;
  hipLaunchKernelGGL(kernel, dim3((batch + 63) / 64), dim3(64), 0, as_stream(stream), args...);
  FFCV_LAUNCH_CHECK(name);
  return FFCV_OK;
}

// A kernel of one workgroup per tile: kernel(args...) on `blocks` workgroups
// of `threads` threads and `lds` bytes of dynamic LDS, for the entry `who`.
template <class K, class... A>
int launch_tiles(const char *who, const char *name, K kernel, void *stream, uint64_t blocks, int threads, uint32_t lds,
                 A... args) {
  if (blocks > 0x7fffffffull) {
    set_error("%s: %llu workgroups exceed one launch", who, (unsigned long long)blocks);
    return FFCV_EINVAL;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), (size_t)lds, as_stream(stream), args...);
  FFCV_LAUNCH_CHECK(name);
  return FFCV_OK;
}

// The host twin of a draw: draw_one(k) for every sample, non-zero when the
// sample's random stream ran out.
template <class F>
int host_draw(const char *who, int batch, F draw_one) {
  int err = 0;
  for (int k = 0; k < batch; k++) err |= draw_one(k);
  if (err) {
    set_error("%s: MT19937 stream exhausted", who);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

// The threads of a host twin over n items: body(next, tid, T) runs on
// T = min(max(nthreads, 1), n) threads (at least one), the caller among them
// as tid 0, and all are joined before this returns.  next: a counter from 0
// that the bodies share to claim items one at a time (fetch_add); tid and T
// serve a static split instead.  A thread's scratch lives at the top of body.
template <class F>
void host_threads(int nthreads, int64_t n, F body) {
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, n));
  std::atomic<uint64_t> next{0};
  std::vector<std::thread> th;
  th.reserve(T - 1);
  for (int t = 1; t < T; t++) th.emplace_back([&body, &next, t, T] { body(next, t, T); });
  body(next, 0, T);
  for (auto &x : th) x.join();
}

// The host twin of an out-of-place operator over the images of a batch (img
// bytes each, those of dst `stride` bytes apart), claimed one at a time:
// one(k, in, out, scratch) says whether it has dealt with image k, which is
// copied if not.  scratch: an S of the thread's own.
template <class S = int, class F>
void host_images(int nthreads, int batch, const uint8_t *src, uint8_t *dst, uint64_t img, uint64_t stride, F one) {
  host_threads(nthreads, batch, [&](std::atomic<uint64_t> &next, int, int) {
    S scratch{};
    for (uint64_t k = next.fetch_add(1); k < (uint64_t)batch; k = next.fetch_add(1))
      if (!one(k, src + k * img, dst + k * stride, scratch)) std::memcpy(dst + k * stride, src + k * img, img);
  });
}

}  // namespace ffcv
