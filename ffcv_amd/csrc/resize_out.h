// resize_out.h -- what the two crop + resize kernels (ffcv_rrc.hip: a band of
// a .beton sample per workgroup; ffcv_rrc_images.hip: an image per workgroup)
// share: the epilogue's set-up, the staged source rows, and how a pixel or a
// quad of four adjacent pixels, cutout applied, leaves for memory.
#pragma once
#include "device_common.h"
#include "lds_stage.h"

// The flip / cutout decisions of image k (cut, flips: null when the step is off)
FFCV_DEV Epilogue make_epilogue(const ffcv_rrc_params &p, const int32_t *__restrict__ cut,
                                const uint8_t *__restrict__ flips, int k) {
  Epilogue ep;
  ep.out_h = p.out_h;
  ep.out_w = p.out_w;
  ep.cut_size = ep.cut_y = ep.cut_x = 0;
  if (cut) {  // (one test: the origin is one 8-byte load)
    ep.cut_size = p.cutout_size;
    ep.cut_y = cut[2 * k];
    ep.cut_x = cut[2 * k + 1];
  }
  ep.flip = flips ? flips[k] : 0;
  ep.cut_before_flip = p.cutout_fill[3];
  ep.fill[0] = p.cutout_fill[0];
  ep.fill[1] = p.cutout_fill[1];
  ep.fill[2] = p.cutout_fill[2];
  return ep;
}

// Crop rows staged in LDS.  LDS row y - r0 holds the 16-byte aligned chunks
// covering crop row y, so the row's first byte sits at its alignment
// offset ((lead + (y - r0) * step) & 15) inside the LDS row (lds_stage.h).
// at(): a channel of a pixel for the shared per-pixel functions; ALIGNED_AT
// takes it from the pixel's two aligned dwords (px: up to 7 bytes of
// look-ahead), else it is one byte read.
template <bool ALIGNED_AT>
struct StagedRows {
  const uint8_t *p;
  int pitch, lead, stepmod, r0;
  FFCV_DEV const uint8_t *row(int y) const {
    const int r = y - r0;
    return p + r * pitch + ((lead + r * stepmod) & 15);
  }
  FFCV_DEV const uint8_t *pix(int y, int x) const { return row(y) + x * 3; }
  FFCV_DEV uint32_t px(int y, int x) const { return lds_pixel(pix(y, x)); }
  FFCV_DEV int at(int y, int x, int c) const {
    return ALIGNED_AT ? (int)((px(y, x) >> (8 * c)) & 0xffu) : (int)row(y)[x * 3 + c];
  }
};

// pixel idx of the image at `out`: three bytes, or three LUT entries
template <bool FP16>
FFCV_DEV void store_px(void *out, uint64_t idx, const int v[3], const uint16_t *lut) {
  if (FP16) {
    uint16_t *o = (uint16_t *)out + idx * 3;
    o[0] = lut[v[0] * 3 + 0];
    o[1] = lut[v[1] * 3 + 1];
    o[2] = lut[v[2] * 3 + 2];
  } else {
    uint8_t *o = (uint8_t *)out + idx * 3;
    o[0] = (uint8_t)v[0];
    o[1] = (uint8_t)v[1];
    o[2] = (uint8_t)v[2];
  }
}

// pixels px .. px + 3 (px % 4 == 0, `out` 4-byte aligned; fp16: 8-byte) as one
// 12-byte (u8) or three 8-byte (fp16) stores
template <bool FP16>
FFCV_DEV void store_quad(void *out, uint64_t px, const int v[12], const uint16_t *lut) {
  if (FP16) {  // 24-byte group, 8-byte aligned
    uint32_t h[12];
#pragma unroll
    for (int i = 0; i < 12; i++) h[i] = lut[v[i] * 3 + i % 3];
    uint2 *o64 = (uint2 *)((uint16_t *)out + px * 3);
    o64[0] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    o64[1] = make_uint2(h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    o64[2] = make_uint2(h[8] | (h[9] << 16), h[10] | (h[11] << 16));
  } else {  // 12-byte group, 4-byte aligned
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    u32x3 w;
    w.x = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    w.y = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
    w.z = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
    // streaming output: non-temporal (measured +2% over plain stores; 16-byte
    // aligned stores of 4-lane groups exchanged by DPP measured the same)
    __builtin_nontemporal_store(w, (u32x3 *)((uint8_t *)out + px * 3));
  }
}

// The cutout of the quad of columns dx0 .. dx0 + 3: the columns inside the
// square (bit j = column dx0 + j; flip-aware), tested once; rows test their
// own range.
struct QuadCut {
  uint32_t mask;
  int y0, y1;  // the square's rows
  uint8_t fill[3];
  FFCV_DEV QuadCut(const Epilogue &ep, int dx0) : mask(0), y0(ep.cut_y), y1(ep.cut_y + ep.cut_size) {
#pragma unroll
    for (int j = 0; j < 4; j++) mask |= ep.in_cut(ep.cut_y, dx0 + j) ? 1u << j : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) fill[c] = ep.fill[c];
  }
  // row dy of the quad: the fill, << SHIFT, into the columns inside the square
  template <int SHIFT, class T>
  FFCV_DEV void patch(int dy, T vals[12]) const {
    if (mask && dy >= y0 && dy < y1) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if ((mask >> j) & 1) {
          vals[3 * j] = (T)fill[0] << SHIFT;
          vals[3 * j + 1] = (T)fill[1] << SHIFT;
          vals[3 * j + 2] = (T)fill[2] << SHIFT;
        }
    }
  }
};
