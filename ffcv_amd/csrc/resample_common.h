// resample_common.h -- what the device kernel and the host twin of
// ffcv_resample_images_batch share: Pillow's ImagingResample
// for 8-bit images, restated.  A 1-D pass from n_in to n_out samples is a
// table of records, one per output sample: the first source sample, the tap
// count and the taps as 22-bit fixed point.  Every product and every sum of
// the float64 arithmetic is rounded on its own (the library is built with
// -ffp-contract=off), so host and device records are equal as bits.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/ffcv_hip.h"
#include "device_common.h"
#include "lds_stage.h"

#define RESAMPLE_BITS 22
// |k| of a coefficient: 2^22 |w|, and the largest normalised |w| met is about
// 1.125, so the bound never acts
// (tests/test_resample.py) and a tap is one 24-bit multiply-add
#define RESAMPLE_KMAX ((1 << 23) - 1)
#define RESAMPLE_HEAD 4  // int32 words in front of a record's taps: first, count, 0, 0

// support of the filter at scale 1: FFCV_RESAMPLE_BILINEAR 1, FFCV_RESAMPLE_BICUBIC 2
FFCV_HD double resample_support(int mode) { return mode == FFCV_RESAMPLE_BICUBIC ? 2.0 : 1.0; }

FFCV_HD double resample_filter(int mode, double x) {
  if (x < 0.0) x = -x;
  if (mode != FFCV_RESAMPLE_BICUBIC) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// The most taps a record of a pass from at most n_in samples can have
// (Pillow's ksize, and never more than the samples there are), rounded up to
// whole groups of four: the passes read taps four at a time.
FFCV_HD int resample_taps_cap(int n_in, int n_out, int mode) {
  const double scale = (double)n_in / (double)n_out;
  const double support = resample_support(mode) * (scale < 1.0 ? 1.0 : scale);
  const int64_t ks = (int64_t)ceil(support) * 2 + 1;
  return (int)(((ks < n_in ? ks : (int64_t)n_in) + 3) & ~(int64_t)3);
}

struct ResampleSpan {
  int first, count;  // source samples [first, first + count)
  double center, inv_fs;
};

FFCV_HD ResampleSpan resample_span(int n_in, int n_out, int mode, int xx) {
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = resample_support(mode) * fs;
  ResampleSpan s;
  s.center = ((double)xx + 0.5) * scale;
  s.inv_fs = 1.0 / fs;
  int lo = (int)(s.center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(s.center + support + 0.5);
  if (hi > n_in) hi = n_in;
  s.first = lo;
  s.count = hi - lo;
  return s;
}

// Record xx of the pass n_in -> n_out into rec[0 .. RESAMPLE_HEAD + cap): the
// taps behind the count are zero up to cap.  The weights are evaluated twice
// (once for their sum, left to right, once to scale them) instead of being
// kept: a lane has no array to keep them in.
FFCV_HD void resample_record(int n_in, int n_out, int mode, int xx, int cap, int32_t *rec) {
  const ResampleSpan s = resample_span(n_in, n_out, mode, xx);
  const int n = s.count < cap ? s.count : cap;  // (count <= cap: resample_taps_cap)
  double ww = 0.0;
  for (int x = 0; x < n; x++) ww += resample_filter(mode, ((double)(x + s.first) - s.center + 0.5) * s.inv_fs);
  rec[0] = s.first;
  rec[1] = n;
  rec[2] = rec[3] = 0;
  for (int x = 0; x < cap; x++) {
    int32_t k = 0;
    if (x < n) {
      double w = resample_filter(mode, ((double)(x + s.first) - s.center + 0.5) * s.inv_fs);
      if (ww != 0.0) w = w / ww;
      const double f = w * (double)(1 << RESAMPLE_BITS);
      k = w < 0.0 ? (int32_t)(-0.5 + f) : (int32_t)(0.5 + f);
      k = k > RESAMPLE_KMAX ? RESAMPLE_KMAX : (k < -RESAMPLE_KMAX ? -RESAMPLE_KMAX : k);
    }
    rec[RESAMPLE_HEAD + x] = k;
  }
}

// (sum + half) >> 22 (arithmetic) clamped to a byte, written as the clamp of
// the sum to [0, 2^30) followed by the shift: the same value.  With the shift
// first, the vertical pass's packing of two results into a dword was compiled
// to v_ashr_pk_u8_i32 and the third byte of each output dword came out with
// bits of the register's earlier contents on the MI355X (DESIGN.md s30, step 7
// has the instructions); in this order the instruction is not selected.
FFCV_HD int resample_clip8(int32_t acc) {
  const int32_t top = (256 << RESAMPLE_BITS) - 1;
  const int32_t v = acc < 0 ? 0 : (acc > top ? top : acc);
  return v >> RESAMPLE_BITS;
}

// ---- the launch plan: host arithmetic, shared with the predicate ----------
#define RESAMPLE_THREADS 256
#define RESAMPLE_LDS_MAX 65536   // LDS one workgroup may allocate
#define RESAMPLE_CHUNK_LOADS 4   // 16-byte loads a thread keeps in flight for the next chunk
#define RESAMPLE_BAND_ROWS 32    // output rows of a band (default plan)
// source rows of a chunk (default plan): 16 for sources of up to 128 rows, 8 above
#define RESAMPLE_CHUNK_ROWS(H) ((H) <= 128 ? 16 : 8)

struct ResamplePlan {
  int bands, band_rows, chunk_rows;  // workgroups per image, output rows each, source rows staged at once
  int kx, ky;                        // taps a column / row record holds
  int src_pitch, ring_pitch, ring_rows;
  uint32_t off_rows, off_src, off_ring, lds;  // byte offsets behind the column records; the total
};

// band_rows / chunk_rows 0: the defaults.  false: the shape does not fit.
static inline bool resample_plan(int H, int W, int out_h, int out_w, int mode, int band_rows, int chunk_rows,
                                 ResamplePlan *p) {
  if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || H > 65535 || W > 65535 || out_h > 65535 || out_w > 65535)
    return false;
  if (mode != FFCV_RESAMPLE_BILINEAR && mode != FFCV_RESAMPLE_BICUBIC) return false;
  p->band_rows = std::min(out_h, band_rows > 0 ? band_rows : RESAMPLE_BAND_ROWS);
  p->bands = (out_h + p->band_rows - 1) / p->band_rows;
  p->kx = resample_taps_cap(W, out_w, mode);
  p->ky = resample_taps_cap(H, out_h, mode);
  const int nch = (int)lds_chunks(3 * W);
  p->src_pitch = nch * 16;
  const int fit = RESAMPLE_CHUNK_LOADS * RESAMPLE_THREADS / nch;  // rows whose chunks the threads hold at once
  if (fit < 1) return false;
  p->chunk_rows = std::min(std::min(H, fit), chunk_rows > 0 ? chunk_rows : RESAMPLE_CHUNK_ROWS(H));
  p->ring_pitch = (3 * out_w + 3) & ~3;
  p->ring_rows = p->ky + p->chunk_rows;
  const uint64_t cols = (uint64_t)out_w * (RESAMPLE_HEAD + p->kx) * 4;
  const uint64_t rows = (uint64_t)p->band_rows * (RESAMPLE_HEAD + p->ky) * 4;
  const uint64_t src = (uint64_t)p->chunk_rows * p->src_pitch + 32;  // + the tap groups' look-ahead
  const uint64_t ring = (uint64_t)p->ring_rows * p->ring_pitch;
  const uint64_t all = cols + rows + src + ring;
  if (all > RESAMPLE_LDS_MAX) return false;
  p->off_rows = (uint32_t)cols;
  p->off_src = (uint32_t)(cols + rows);
  p->off_ring = (uint32_t)(cols + rows + src);
  p->lds = (uint32_t)all;
  return true;
}
