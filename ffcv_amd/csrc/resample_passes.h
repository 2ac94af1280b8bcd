// resample_passes.h -- the rolling two-pass of the crop decoders' 'bilinear'
// and 'bicubic' modes, shared by jpeg_color_resample_kernel
// (ffcv_jpeg.hip), resample_raw_kernel (ffcv_resample_raw.hip) and the host
// decoder (ffcv_cpu_jpeg.hip): the band plan and its predicate, the horizontal
// pass from staged packed-RGB rows into a ring of uint8 intermediate rows, the
// vertical pass from the ring to memory, and both passes on the host.  The
// records and the clip are resample_common.h's; the passes follow
// ffcv_resample.hip (four taps per step from aligned dwords, v_mad_i32_i24).
#pragma once
#include <vector>

#include "resample_common.h"

FFCV_HD bool resample_window_ok(int i, int j, int h, int w, int H, int W) {
  return h > 0 && w > 0 && i >= 0 && j >= 0 && (int64_t)i + h <= H && (int64_t)j + w <= W;
}

// ---- the plan: host arithmetic, shared with ffcv_jpeg_resample_fits --------
// LDS of a band workgroup, sized for the worst window of a context (the whole
// image of max_h x max_w):
//   [column records][row records][staged rows][ring][plane tiles x 3]
// staged rows: chunk_rows rows of packed RGB (the JPEG kernel writes them from
// its colour stage at pitch src_pitch; the raw kernel stages the aligned
// 16-byte words of the file's rows there).  Plane tiles: per component the
// chunk's plane rows with their chroma context, at most tile_rows x tile_pitch
// bytes (three full-resolution components: 4:4:4 and RGB-coded files).
struct BandResamplePlan {
  int bands, band_rows, chunk_rows;  // workgroups per image, output rows each, window rows staged at once
  int kx, ky;                        // taps a column / row record holds
  int src_pitch, ring_pitch, ring_rows;
  int tile_rows, tile_pitch;  // a component tile's most rows and bytes per row
  uint32_t off_rows, off_src, off_ring, off_tiles, lds;  // byte offsets behind the column records; the total
};

// window rows of a chunk (default plan): 16 for contexts of up to 256 rows, 8
// above (measured; the transform's rule changes at 128 rows)
#define BAND_RESAMPLE_CHUNK_ROWS(H) ((H) <= 256 ? 16 : 8)

// band_rows / chunk_rows 0: the defaults (32 output rows; 16 / 8 window rows).
// The default chunk is halved until the layout fits; a chunk given by the
// caller is taken as it is.  false: the shape does not fit 64 KiB.
static inline bool band_resample_plan(int max_h, int max_w, int out_h, int out_w, int mode, int band_rows,
                                      int chunk_rows, BandResamplePlan *p) {
  if (max_h <= 0 || max_w <= 0 || out_h <= 0 || out_w <= 0 || max_h > 65535 || max_w > 65535 || out_h > 65535 ||
      out_w > 65535)
    return false;
  if (mode != FFCV_RESAMPLE_BILINEAR && mode != FFCV_RESAMPLE_BICUBIC) return false;
  p->band_rows = std::min(out_h, band_rows > 0 ? band_rows : RESAMPLE_BAND_ROWS);
  p->bands = (out_h + p->band_rows - 1) / p->band_rows;
  p->kx = resample_taps_cap(max_w, out_w, mode);
  p->ky = resample_taps_cap(max_h, out_h, mode);
  const int nch = (int)lds_chunks(3 * max_w);
  p->src_pitch = nch * 16;
  p->ring_pitch = (3 * out_w + 3) & ~3;
  p->tile_pitch = ((max_w + 3) & ~3) + 8;  // a row's dwords, from the dword under its first sample
  const int fit = RESAMPLE_CHUNK_LOADS * RESAMPLE_THREADS / nch;  // raw rows whose words the threads hold at once
  if (fit < 1) return false;
  const uint64_t cols = (uint64_t)out_w * (RESAMPLE_HEAD + p->kx) * 4;
  const uint64_t rows = (uint64_t)p->band_rows * (RESAMPLE_HEAD + p->ky) * 4;
  for (int ch = std::min(std::min(max_h, fit), chunk_rows > 0 ? chunk_rows : BAND_RESAMPLE_CHUNK_ROWS(max_h));; ch >>= 1) {
    if (ch < 1) return false;
    p->chunk_rows = ch;
    p->ring_rows = p->ky + ch;
    p->tile_rows = std::max(ch, ch / 2 + 3);  // ve = 2: the rows' chroma rows and one of context either side
    const uint64_t src = (uint64_t)ch * p->src_pitch + 32;  // + the tap groups' look-ahead
    const uint64_t ring = (uint64_t)p->ring_rows * p->ring_pitch;
    const uint64_t tiles = 3 * (uint64_t)p->tile_rows * p->tile_pitch;
    const uint64_t all = cols + rows + src + ring + tiles;
    if (all <= RESAMPLE_LDS_MAX) {
      p->off_rows = (uint32_t)cols;
      p->off_src = (uint32_t)(cols + rows);
      p->off_ring = (uint32_t)(cols + rows + src);
      p->off_tiles = (uint32_t)(cols + rows + src + ring);
      p->lds = (uint32_t)all;
      return true;
    }
    if (chunk_rows > 0) return false;
  }
}

// byte b of w times k, added to acc: one v_mad_i32_i24 (|k| <= RESAMPLE_KMAX)
FFCV_DEV int resample_mad(uint32_t w, int b, int k, int acc) {
  return ffcv_mul24((int)((w >> (8 * b)) & 0xffu), k) + acc;
}

// The records of a band: the out_w column records of the window's width and
// the row records of output rows [y0, y1), one lane per record.
FFCV_DEV void resample_band_records(int t, int cww, int chh, int out_w, int out_h, int mode, int y0, int y1, int kx,
                                    int ky, int32_t *s_col, int32_t *s_row) {
  const int KX = RESAMPLE_HEAD + kx, KY = RESAMPLE_HEAD + ky;
  for (int i = t; i < out_w + (y1 - y0); i += RESAMPLE_THREADS) {
    if (i < out_w)
      resample_record(cww, out_w, mode, i, kx, s_col + i * KX);
    else
      resample_record(chh, out_h, mode, y0 + (i - out_w), ky, s_row + (i - out_w) * KY);
  }
}

// Horizontal: staged window rows [c0, c0 + rows) -> their ring rows.  A work
// item is (row, output column): its taps are contiguous bytes of the row
// (row_ptr(r): the first byte of staged row r, at any alignment), read four
// taps (three aligned dwords) at a time; the taps behind a record's count are
// zero and meet whatever bytes follow, inside the staging area's look-ahead.
template <class RowPtr>
FFCV_DEV void resample_h_pass(int t, int rows, int c0, int out_w, const int32_t *s_col, int KX, RowPtr row_ptr,
                              uint32_t *s_ring, int ring_rows, int ndw) {
  for (int i = t; i < rows * out_w; i += RESAMPLE_THREADS) {
    const int r = i / out_w, xo = i - r * out_w;
    const int32_t *rec = s_col + xo * KX;
    const int first = rec[0], n = rec[1];
    const uint8_t *a = row_ptr(r) + 3 * first;
    const uint32_t *q = (const uint32_t *)__builtin_align_down(a, 4);
    const uint32_t sh = (uint32_t)(a - (const uint8_t *)q);
    uint32_t w0 = q[0];
    int a0 = 1 << (RESAMPLE_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; x += 4) {  // four taps are twelve bytes
      const int4 kk = *(const int4 *)(rec + RESAMPLE_HEAD + x);
      const uint32_t w1 = q[1], w2 = q[2], w3 = q[3];
      const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                     d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
      w0 = w3;
      q += 3;
      a0 = resample_mad(d0, 0, kk.x, a0);
      a1 = resample_mad(d0, 1, kk.x, a1);
      a2 = resample_mad(d0, 2, kk.x, a2);
      a0 = resample_mad(d0, 3, kk.y, a0);
      a1 = resample_mad(d1, 0, kk.y, a1);
      a2 = resample_mad(d1, 1, kk.y, a2);
      a0 = resample_mad(d1, 2, kk.z, a0);
      a1 = resample_mad(d1, 3, kk.z, a1);
      a2 = resample_mad(d2, 0, kk.z, a2);
      a0 = resample_mad(d2, 1, kk.w, a0);
      a1 = resample_mad(d2, 2, kk.w, a1);
      a2 = resample_mad(d2, 3, kk.w, a2);
    }
    uint8_t *dst = (uint8_t *)(s_ring + ((uint32_t)(c0 + r) % (uint32_t)ring_rows) * ndw) + 3 * xo;
    dst[0] = (uint8_t)resample_clip8(a0);
    dst[1] = (uint8_t)resample_clip8(a1);
    dst[2] = (uint8_t)resample_clip8(a2);
  }
}

// Vertical: the output rows from ydone on whose last window row is below c1
// (the ring holds it).  A work item is (output row, four adjacent bytes): one
// aligned dword of each of the row's ring rows, four sums, one dword store
// where the address allows.  o: the image's first output byte, rows of orb
// bytes.  Returns the first row not done.
FFCV_DEV int resample_v_pass(int t, int ydone, int y0, int y1, int c1, const int32_t *s_row, int KY,
                             const uint32_t *s_ring, int ring_rows, int ndw, uint8_t *o, int orb) {
  int yr = ydone;
  while (yr < y1) {
    const int32_t *rr = s_row + (yr - y0) * KY;
    if (rr[0] + rr[1] > c1) break;
    yr++;
  }
  for (int i = t; i < (yr - ydone) * ndw; i += RESAMPLE_THREADS) {
    const int yy = i / ndw, d = i - yy * ndw, y = ydone + yy;
    const int32_t *rec = s_row + (y - y0) * KY;
    const int n = rec[1];
    int j = (int)((uint32_t)rec[0] % (uint32_t)ring_rows);
    int a0 = 1 << (RESAMPLE_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int x = 0; x < n; x++) {
      const int kk = rec[RESAMPLE_HEAD + x];
      const uint32_t w = s_ring[j * ndw + d];
      a0 = resample_mad(w, 0, kk, a0);
      a1 = resample_mad(w, 1, kk, a1);
      a2 = resample_mad(w, 2, kk, a2);
      a3 = resample_mad(w, 3, kk, a3);
      j = j + 1 == ring_rows ? 0 : j + 1;
    }
    const uint32_t b0 = (uint32_t)resample_clip8(a0), b1 = (uint32_t)resample_clip8(a1),
                   b2 = (uint32_t)resample_clip8(a2), b3 = (uint32_t)resample_clip8(a3);
    const uint32_t packed = b0 | b1 << 8 | b2 << 16 | b3 << 24;
    uint8_t *g = o + (uint64_t)y * orb + 4 * d;
    const int valid = min(4, orb - 4 * d);  // the row's last dword may hold fewer than four bytes
    if (valid == 4 && ((uintptr_t)g & 3) == 0) {
      *(uint32_t *)g = packed;
    } else {
      for (int b = 0; b < valid; b++) g[b] = (uint8_t)(packed >> (8 * b));
    }
  }
  return yr;
}

// A band of a sample that yields no picture: zeros.
FFCV_DEV void resample_zero_band(int t, uint8_t *o, int y0, int y1, int orb) {
  uint8_t *ob = o + (uint64_t)y0 * orb;
  for (int i = t; i < (y1 - y0) * orb; i += RESAMPLE_THREADS) ob[i] = 0;
}

// ---- both passes on the host: one window, a uint8 intermediate of h x out_w
struct ResampleHostScratch {
  std::vector<int32_t> col, row;
  std::vector<uint8_t> mid;
};

static inline void resample_window_host(const uint8_t *img, int W, const int32_t *c, int mode, int out_h, int out_w,
                                        uint8_t *dst, ResampleHostScratch &s) {
  const int ci = c[0], cj = c[1], chh = c[2], cww = c[3];
  const int kx = resample_taps_cap(cww, out_w, mode), ky = resample_taps_cap(chh, out_h, mode);
  const int KX = RESAMPLE_HEAD + kx, KY = RESAMPLE_HEAD + ky;
  s.col.resize((size_t)out_w * KX);
  s.row.resize((size_t)out_h * KY);
  s.mid.resize((size_t)chh * out_w * 3);
  for (int x = 0; x < out_w; x++) resample_record(cww, out_w, mode, x, kx, s.col.data() + (size_t)x * KX);
  for (int y = 0; y < out_h; y++) resample_record(chh, out_h, mode, y, ky, s.row.data() + (size_t)y * KY);
  for (int r = 0; r < chh; r++) {
    const uint8_t *src = img + ((uint64_t)(ci + r) * W + cj) * 3;
    uint8_t *m = s.mid.data() + (size_t)r * out_w * 3;
    for (int x = 0; x < out_w; x++) {
      const int32_t *rec = s.col.data() + (size_t)x * KX;
      for (int ch = 0; ch < 3; ch++) {
        int32_t acc = 1 << (RESAMPLE_BITS - 1);
        for (int i = 0; i < rec[1]; i++) acc += (int32_t)src[3 * (rec[0] + i) + ch] * rec[RESAMPLE_HEAD + i];
        m[3 * x + ch] = (uint8_t)resample_clip8(acc);
      }
    }
  }
  const size_t orb = (size_t)out_w * 3;
  for (int y = 0; y < out_h; y++) {
    const int32_t *rec = s.row.data() + (size_t)y * KY;
    for (size_t e = 0; e < orb; e++) {
      int32_t acc = 1 << (RESAMPLE_BITS - 1);
      for (int i = 0; i < rec[1]; i++) acc += (int32_t)s.mid[(size_t)(rec[0] + i) * orb + e] * rec[RESAMPLE_HEAD + i];
      dst[(size_t)y * orb + e] = (uint8_t)resample_clip8(acc);
    }
  }
}
