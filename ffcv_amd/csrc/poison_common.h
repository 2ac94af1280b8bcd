// poison_common.h -- what the Poison / ReplaceLabel kernels and their host
// twins share: the membership test and the pixel function.
#pragma once
#include <cmath>
#include <cstdint>

namespace ffcv {

// poisoning.py:51-52: np.searchsorted(to_poison, id), then the equality test.
// `ids` holds n sorted unique values; a negative sample id is in no set.
__host__ __device__ inline bool poison_member(const uint64_t *ids, uint64_t n, int64_t id) {
  if (id < 0) return false;
  const uint64_t key = (uint64_t)id;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && ids[lo] == key;
}

// poisoning.py:54-58 on one uint8 value, as numpy evaluates it on a float32
// temp: keep = float64(1 - alpha), add = float64(mask) * alpha.
//   temp *= 1 - alpha   float32(float64(v) * keep)   (for a float32 alpha the
//                       float32 multiply: that product is exact in float64)
//   temp += mask        float32(float64(t1) + add)
//   clip, then the truncating cast
// Two separate float32 roundings; the build keeps -ffp-contract=off.
__host__ __device__ inline uint8_t poison_value(uint8_t v, double keep, double add, float lo, float hi) {
  const float t1 = (float)((double)v * keep);
  const float t2 = (float)((double)t1 + add);
  const float t3 = fminf(fmaxf(t2, lo), hi);
  return (uint8_t)(int)t3;
}

}  // namespace ffcv
