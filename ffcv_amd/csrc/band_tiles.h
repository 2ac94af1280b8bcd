// band_tiles.h -- how the stencil kernels on dense uint8 [B][H][W][3] batches
// (gaussian_blur_kernel, sharpness_kernel) cut an image into tiles, on the host
// (the plan of a launch) and in the kernel (a workgroup's tile: BandTile, which
// gaussian_blur_kernel keeps written out), DESIGN.md s23.
//
// A workgroup owns output rows [y0, y1) x columns [x0, x1) of one image and
// stages their source with a halo of r, rows [y0 - r, y1 + r) x columns
// [x0 - r, x1 + r) clipped to the image, as a tile of rows (lds_stage.h).
//
//   whole image: it fits the kernel's limit -- one tile per image.
//   bands: tiles of band_rows rows; a band whose tile exceeds the kernel's LDS
//     cap at the image's width is split into column strips of the widest width
//     that fits.
//
// An image that is not applied is copied: no halo and no columns.  A band's
// rows are one byte range of the image, and the band's workgroups (one per
// strip) take an equal piece of it each, never more than a tile's bytes.
#pragma once
#include <algorithm>

#include "lds_stage.h"

// How a launch cuts an image into tiles, and the LDS a workgroup takes.
struct BandPlan {
  int band_rows, strip_cols, nbands, nstrips;
  uint32_t u8_bytes;  // the staged source with its look-ahead, a multiple of 16
  uint32_t lds;       // dynamic LDS: the kernel's regions in front of, with and behind u8_bytes
};

// The uint8 region of a tile of `rows` x `cols` outputs at halo r in an H x W image
inline uint32_t band_u8_bytes(int H, int W, int rows, int cols, int r) {
  const uint32_t nrows = (uint32_t)std::min(H, rows + 2 * r), cw = (uint32_t)std::min(W, cols + 2 * r);
  // one range when every tile spans the width, else a range per row (a tile
  // at the image's edge may still span it and stage one range: never more
  // chunks than its rows take apart, from two rows on; one row is the same
  // either way).  A copy stages one range of at most rows x cols pixels:
  // never more than this.
  const uint32_t one = lds_chunks(nrows * 3u * cw) * 16u, apart = nrows * lds_chunks(3u * cw) * 16u;
  const uint32_t staged = cols >= W ? one : std::max(one, apart);
  return staged + 32u;  // + the look-ahead of the pixel reads and of the chunks assembled for dst
}

// The plan of H x W images.  whole: an image is one tile; else bands of
// band_rows rows, in strips where a band exceeds `cap` bytes of LDS.
// rest(nrows, rows, cols): the LDS a tile of rows x cols outputs and nrows
// staged rows takes beside its uint8 region.  guess: the strip width from
// which the search counts down to the first that fits (a closed form of the
// kernel's own, so that the search takes a few steps).
template <class F>
BandPlan band_plan(int H, int W, bool whole, int band_rows, uint32_t cap, int r, F rest, int guess) {
  BandPlan P;
  P.band_rows = whole ? H : std::min(H, band_rows);
  P.strip_cols = W;
  auto tile = [&](int cols) {
    P.u8_bytes = band_u8_bytes(H, W, P.band_rows, cols, r);
    P.lds = P.u8_bytes + rest((uint32_t)std::min(H, P.band_rows + 2 * r), (uint32_t)P.band_rows, (uint32_t)cols);
  };
  tile(W);
  if (!whole && P.lds > cap) {
    int c = std::max(1, std::min(guess, W));
    for (;; c--) {
      tile(c);
      if (P.lds <= cap || c == 1) break;
    }
    P.strip_cols = c;
  }
  P.nbands = (H + P.band_rows - 1) / P.band_rows;
  P.nstrips = (W + P.strip_cols - 1) / P.strip_cols;
  return P;
}

// n byte ranges of `bytes` bytes from address a0 on, `step` bytes apart: what
// stage_rows and write_back_rows move.  span: rows that span the image's
// width, which are one range.
struct BandRows {
  uint64_t a0;
  bool span;
  int n;
  uint32_t bytes;
};

// the image a workgroup works on: BandTile's k, for a kernel that reads the image's decision first
FFCV_DEV uint32_t band_image(uint32_t block, const BandPlan &P) { return block / ((uint32_t)P.nbands * P.nstrips); }

// A workgroup's tile: the image k it belongs to and its place in it.  With the
// image's decision `on` it is computed, rows x tc outputs from nrows x cw
// staged pixels, else copied: piece [cp0, cp0 + cp_len) of the band's bytes
// (nothing to do where cp_len is 0).
struct BandTile {
  uint32_t k;
  int strip;
  int y0, y1, x0, x1, lo, hi, cl, ch, nrows, cw, rows, tc;
  uint64_t step;  // bytes from an image row to the next
  uint32_t band_bytes, cp0, cp_len;

  FFCV_DEV BandTile(uint32_t block, const BandPlan &P, int H, int W, int r) {
    const uint32_t per = (uint32_t)P.nbands * P.nstrips;
    k = block / per;
    const uint32_t rem = block - k * per;
    const int band = rem / P.nstrips;
    strip = rem - band * P.nstrips;
    y0 = band * P.band_rows, y1 = min(H, y0 + P.band_rows);
    x0 = strip * P.strip_cols, x1 = min(W, x0 + P.strip_cols);
    lo = max(0, y0 - r), hi = min(H, y1 + r), cl = max(0, x0 - r), ch = min(W, x1 + r);
    nrows = hi - lo, cw = ch - cl, rows = y1 - y0, tc = x1 - x0;

    step = (uint64_t)W * 3u;
    band_bytes = (uint32_t)rows * 3u * W;
    const uint32_t piece = (band_bytes + P.nstrips - 1) / P.nstrips;
    cp0 = min(band_bytes, (uint32_t)strip * piece), cp_len = min(piece, band_bytes - cp0);
  }

  // what is staged: source rows [lo, hi) x columns [cl, ch), or the copy's piece
  FFCV_DEV BandRows source(bool copy, int H, int W, const uint8_t *src) const {
    const uint64_t src0 = (uint64_t)(uintptr_t)src + (uint64_t)k * H * step +
                          (!copy ? ((uint64_t)lo * W + cl) * 3u : (uint64_t)y0 * step + cp0);
    const bool span = copy || cw == W;
    return {src0, span, span ? 1 : nrows, copy ? cp_len : (span ? (uint32_t)nrows * 3u * W : 3u * cw)};
  }

  // what is written: rows [y0, y1) x columns [x0, x1) of dst, or the copy's piece
  FFCV_DEV BandRows dest(bool copy, int W, uint8_t *dst, uint64_t dst_stride) const {
    const bool ospan = copy || tc == W;
    const uint32_t orow_bytes = copy ? cp_len : (ospan ? band_bytes : 3u * tc);
    const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * dst_stride +
                          (!copy ? ((uint64_t)y0 * W + x0) * 3u : (uint64_t)y0 * step + cp0);
    return {dst0, ospan, ospan ? 1 : rows, orow_bytes};
  }
};
