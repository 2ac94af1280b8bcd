// lds_stage.h -- how the image-transform kernels move uint8 HWC bytes between
// global memory and LDS.  Device code, all inlined;
// lds_chunks alone is also the host plans' arithmetic.
//
// A byte range of an image starts at any byte offset, so it is moved in the
// 16-byte ALIGNED chunks that hold a byte of it:
//   - loads: an aligned chunk holding a byte of the range lies in that byte's
//     page, so the load never touches a page the range does not, whatever
//     bytes of a neighbour it also brings;
//   - LDS reads: a pixel's three bytes sit at any offset; they come from two
//     ALIGNED dwords joined by v_alignbyte (adjacent byte reads are merged
//     into misaligned reads, several times slower), which reads up to 7 bytes
//     past the pixel's first: every staging array keeps that look-ahead;
//   - stores: a chunk wholly inside the range is one 16-byte store; the chunks
//     cut by the range's ends go byte by byte, since their other bytes belong
//     to a neighbouring image, row or allocation and are not ours to rewrite.
#pragma once
#include "device_common.h"

typedef uint32_t lds_x4_t __attribute__((ext_vector_type(4)));
// (a global-address-space pointer: global_load / global_store_dwordx4, not flat)
typedef __attribute__((address_space(1))) lds_x4_t glb_x4_t;

// 16-byte chunks that can hold `bytes` contiguous bytes at any alignment
template <class T>
FFCV_HD T lds_chunks(T bytes) {
  return (bytes + 30) >> 4;
}

// The pixel at LDS byte address a: R | G << 8 | B << 16 | the next byte << 24
FFCV_DEV uint32_t lds_pixel(const uint8_t *a) {
  const uint32_t *qa = (const uint32_t *)__builtin_align_down(a, 4);
  return __builtin_amdgcn_alignbyte(qa[1], qa[0], (uint32_t)(a - (const uint8_t *)qa));
}

// ---------------------------------------------------------------------------
// A run of whole pixels: tile `tile` of image k, tile_px pixels (the last tile
// of an image fewer), one contiguous byte range, staged in s_img as the chunks
// [0, nch) that cover it.  s_img holds the range's bytes / 16 + 2 chunks: the
// lead bytes and the pixel read-ahead.  Staged byte j is byte j - lead of the
// range.  The caller puts a __syncthreads() between stage, its own passes and
// write_back.
template <int THREADS>
struct PixelRun {
  lds_x4_t *s_img;
  uintptr_t ga;  // address of the aligned chunk holding the range's first byte
  uint32_t lead, nbytes;
  int nch;

  FFCV_DEV PixelRun(uint8_t *images, uint64_t img, uint32_t k, uint32_t tile, uint32_t tile_px, lds_x4_t *s)
      : s_img(s) {
    const uint64_t b0 = (uint64_t)tile * tile_px * 3u;
    nbytes = (uint32_t)(img - b0 < (uint64_t)tile_px * 3u ? img - b0 : (uint64_t)tile_px * 3u);
    uint8_t *src = images + (uint64_t)k * img + b0;
    lead = (uint32_t)((uintptr_t)src & 15);
    ga = (uintptr_t)src & ~(uintptr_t)15;
    nch = (int)((lead + nbytes + 15) >> 4);
  }
  FFCV_DEV uint32_t npix() const { return nbytes / 3u; }
  FFCV_DEV glb_x4_t *chunks() const { return (glb_x4_t *)ga; }  // the run's nch chunks in memory
  FFCV_DEV uint8_t *bytes() const { return (uint8_t *)s_img + lead; }  // byte 0 of the staged pixels

  FFCV_DEV void stage(int t) const {
    for (int i = t; i < nch; i += THREADS) s_img[i] = chunks()[i];
  }

  // every whole word of s_img that covers staged bytes becomes f(word) (the
  // bytes around the range are not written back)
  template <class F>
  FFCV_DEV void map_words(int t, F f) const {
    uint32_t *s_words = (uint32_t *)s_img;
    const uint32_t w1 = (lead + nbytes + 3) >> 2;
    for (uint32_t w = (lead >> 2) + t; w < w1; w += THREADS) s_words[w] = f(s_words[w]);
  }

  FFCV_DEV void write_back(int t) const {
    for (int i = t; i < nch; i += THREADS) {
      const uint32_t c0 = 16u * (uint32_t)i;
      if (c0 >= lead && c0 + 16u <= lead + nbytes) {
        chunks()[i] = s_img[i];
      } else {
        const uint8_t *sb = (const uint8_t *)s_img;
        uint8_t *gb = (uint8_t *)ga;
        for (uint32_t j = c0; j < c0 + 16u; j++)
          if (j >= lead && j < lead + nbytes) gb[j] = sb[j];
      }
    }
  }
};

// ---------------------------------------------------------------------------
// A tile of rows: n byte ranges of the same length, `step` bytes apart in
// memory.  Rows that span the image's width are one range (n = 1).  Range r is
// staged as its own lds_chunks(bytes) chunks, so its first byte sits at its
// alignment offset behind r * pitch.
template <bool MUL24 = false>  // r < 2^15, pitch < 2^17, the product inside LDS: 24-bit multiplies (full rate)
struct LdsRows {
  const uint8_t *base;  // first staged chunk
  int pitch, lead0, stepmod;
  FFCV_DEV const uint8_t *row(int r) const {
    if (MUL24)
      return base + __umul24((uint32_t)r, (uint32_t)pitch) +
             ((lead0 + __umul24((uint32_t)r, (uint32_t)stepmod)) & 15);
    return base + r * pitch + ((lead0 + r * stepmod) & 15);
  }
};

// where stage_rows puts the ranges; span: they are one range, rows `step` bytes apart in LDS too
template <bool MUL24 = false>
FFCV_DEV LdsRows<MUL24> lds_rows(const lds_x4_t *s_u8, uint64_t src0, uint64_t step, bool span, int nchr) {
  return {(const uint8_t *)s_u8, span ? (int)step : nchr * 16, (int)(src0 & 15), span ? 0 : (int)(step & 15)};
}

// n_srows ranges of srow_bytes bytes from address src0 on, nchr = lds_chunks(srow_bytes) chunks each
template <int THREADS>
FFCV_DEV void stage_rows(int t, uint64_t src0, uint64_t step, int n_srows, uint32_t srow_bytes, int nchr,
                         lds_x4_t *s_u8) {
  for (int i = t; i < n_srows * nchr; i += THREADS) {
    const int rr = i / nchr, c = i - rr * nchr;
    const uint64_t ra = src0 + (uint64_t)rr * step;
    if (c < (int)(((ra & 15) + srow_bytes + 15) >> 4)) s_u8[i] = ((glb_x4_t *)(uintptr_t)(ra & ~(uint64_t)15))[c];
  }
}

// n_orows ranges of orow_bytes bytes to address dst0 on, from LDS: range y's
// bytes start at row_ptr(y), at any offset.  A whole chunk of dst is assembled
// from five aligned LDS dwords (row_ptr's array keeps 32 bytes of look-ahead).
template <int THREADS, class F>
FFCV_DEV void write_back_rows(int t, uint64_t dst0, uint64_t step, int n_orows, uint32_t orow_bytes, F row_ptr) {
  const int onch = (int)lds_chunks(orow_bytes);
  for (int i = t; i < n_orows * onch; i += THREADS) {
    const int y = i / onch, c = i - y * onch;
    const uint64_t da = dst0 + (uint64_t)y * step;
    const int dl = (int)(da & 15), c0 = 16 * c;  // the range is bytes [dl, dl + orow_bytes) of the aligned row
    if (c0 >= dl + (int)orow_bytes) continue;
    const uint8_t *sp = row_ptr(y) + (c0 - dl);
    uint8_t *gb = (uint8_t *)(uintptr_t)(da & ~(uint64_t)15) + c0;
    if (c0 >= dl && c0 + 16 <= dl + (int)orow_bytes) {
      const uint32_t *q = (const uint32_t *)__builtin_align_down(sp, 4);
      const uint32_t sh = (uint32_t)(sp - (const uint8_t *)q);
      const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
      lds_x4_t o;
      o.x = __builtin_amdgcn_alignbyte(q1, q0, sh);
      o.y = __builtin_amdgcn_alignbyte(q2, q1, sh);
      o.z = __builtin_amdgcn_alignbyte(q3, q2, sh);
      o.w = __builtin_amdgcn_alignbyte(q4, q3, sh);
      *(glb_x4_t *)gb = o;
    } else {
      for (int j = 0; j < 16; j++) {
        const int b = c0 + j - dl;
        if (b >= 0 && b < (int)orow_bytes) gb[j] = sp[j];
      }
    }
  }
}
