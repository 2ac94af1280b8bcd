// jpeg_color_resample.h -- the crop decoders' 'bilinear' and 'bicubic' modes
// (DESIGN.md s31): jpeg_color_resample_kernel, launched in K2's place behind
// K1 and K1b.  Output = Pillow's img.crop(window).resize(size, filter) of the
// decoded image, byte for byte, as uint8 with no epilogue.
//
// One workgroup per (image, band of output rows).  The window's rows the band
// needs roll through LDS a chunk at a time:
//   records    the out_w column records and the band's row records, from the
//              image's own window size, one lane per record, while the first
//              chunk's plane loads are in flight;
//   staging    the chunk's tiles of K1b's component planes, chroma context
//              rows and columns included, as aligned dwords; the next chunk's
//              first dwords wait in registers during the passes;
//   colour     K2's arithmetic on the tiles (upsample_quad_h2v2 / pixel_rgb /
//              ycc_rgb on TPlane, plane coordinates absolute, so the chroma
//              phase and libjpeg's edge replication are the image's whatever
//              row the chunk starts on) into packed RGB rows;
//   passes     resample_passes.h: horizontal into a ring of uint8 rows, vertical
//              as soon as the ring holds an output row's last window row.
#pragma once
#include "jpeg_color_resize.h"
#include "resample_passes.h"

struct JpegResampleArgs {
  int mode;
  BandResamplePlan P;
};

#define JR_SU 4  // dwords of each component's next tile a thread holds in registers

// x / d for the expansion factors a frame can have (1, 2 and 4 by shifts)
FFCV_DEV int jr_div(int x, int d) { return d == 1 ? x : (d == 2 ? x >> 1 : (d == 4 ? x >> 2 : x / d)); }

__global__ void __launch_bounds__(RESAMPLE_THREADS) jpeg_color_resample_kernel(JpegArgs a, JpegResampleArgs ra) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = threadIdx.x, k = (int)blockIdx.y, band = (int)blockIdx.x;
  const BandResamplePlan &P = ra.P;
  const int mode = ra.mode;
  K2Rec R;
  R.load(a.info + k, t);
  if (k == 0 && band == 0 && t == 0) {  // K1 is done: close its arena (see arena_before_k1)
    const unsigned long long top = a.arena_top[0];
    if (top) {
      a.arena_top[1] = top;
      a.arena_top[0] = 0;
    }
  }
  const int status = R.s(K2F(status));
  if (status == -1) return;  // raw sample (ffcv_resample_raw_batch)
  const int out_h = a.p.out_h, out_w = a.p.out_w;
  const int y0 = band * P.band_rows, y1 = min(out_h, y0 + P.band_rows);
  const int orb = 3 * out_w;  // bytes of an output row
  uint8_t *o = (uint8_t *)a.out + a.out_stride * (uint64_t)k;
  if (status != FFCV_SAMPLE_OK) {
    resample_zero_band(t, o, y0, y1, orb);
    return;
  }
  const ImgInfo I = k2_head(R);
  const ColorGeom G = color_geom(I);
  const int ncomp = G.ncomp;
  const int ri = I.ri, rj = I.rj, chh = I.rh, cww = I.rw;

  const int KX = RESAMPLE_HEAD + P.kx, KY = RESAMPLE_HEAD + P.ky;
  int32_t *s_col = (int32_t *)lds;
  int32_t *s_row = (int32_t *)(lds + P.off_rows);
  uint8_t *s_rgb = lds + P.off_src;
  uint32_t *s_ring = (uint32_t *)(lds + P.off_ring);
  const int ring_rows = P.ring_rows, ndw = P.ring_pitch >> 2, CH = P.chunk_rows, pitch = P.src_pitch;
  const int tile_cap = P.tile_rows * P.tile_pitch;

  // window rows [r_lo, r_hi) feed the band (a record's first and end sample never decrease along a pass)
  const ResampleSpan sp0 = resample_span(chh, out_h, mode, y0), sp1 = resample_span(chh, out_h, mode, y1 - 1);
  const int r_lo = sp0.first, r_hi = sp1.first + sp1.count;

  // the columns of every chunk's tiles: plane columns [tx0, tx0 + tpitch) hold
  // the window's samples and their context, from an aligned dword on (plane
  // rows are 8-byte aligned and as wide as K1's window of 8 x 8 blocks)
  const int X0 = rj, X1 = rj + cww - 1;
  int tx0[3], tpitch[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int he = G.he[c];
    const int x0 = max(jr_div(X0, he) - (he == 2 ? 1 : 0), 0);
    const int x1 = min(jr_div(X1, he) + (he == 2 ? 1 : 0), G.cw[c] - 1);
    tx0[c] = x0 & ~3;
    tpitch[c] = c < ncomp ? ((x1 + 4) & ~3) - tx0[c] : 0;
  }
  // the rows of the tiles of window rows [cs, cs + nr)
  auto tile_rows = [&](int c, int cs, int nr, int *ty0) {
    const int ve = G.ve[c];
    const int ya = max(jr_div(ri + cs, ve) - (ve == 2 ? 1 : 0), 0);
    const int yb = min(jr_div(ri + cs + nr - 1, ve) + (ve == 2 ? 1 : 0), G.ch[c] - 1);
    *ty0 = ya;
    return c < ncomp ? yb - ya + 1 : 0;
  };
  typedef const __attribute__((address_space(1))) uint32_t gu32_t;
  uint32_t sv[3][JR_SU];
  // the first JR_SU dwords per thread of each component's tile into registers
  auto load = [&](int cs, int nr) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      int ty0;
      const int trows = tile_rows(c, cs, nr, &ty0), wpr = max(tpitch[c] >> 2, 1), n = trows * (tpitch[c] >> 2);
      const uint8_t *src = a.arena + (I.poff[c] + (uint64_t)ty0 * (uint64_t)I.stride[c] + (uint64_t)tx0[c]);
#pragma unroll
      for (int u = 0; u < JR_SU; u++) {
        const int i = u * RESAMPLE_THREADS + t, rr = i / wpr, q = i - rr * wpr;
        sv[c][u] = i < n ? *(gu32_t *)(uintptr_t)(src + (uint64_t)rr * (uint64_t)I.stride[c] + 4 * q) : 0u;
      }
    }
  };
  // the registers into the LDS tiles, and whatever a tile holds beyond them
  auto store = [&](int cs, int nr) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      int ty0;
      const int trows = tile_rows(c, cs, nr, &ty0), wpr = max(tpitch[c] >> 2, 1), n = trows * (tpitch[c] >> 2);
      uint32_t *tl = (uint32_t *)(lds + P.off_tiles + c * tile_cap);
#pragma unroll
      for (int u = 0; u < JR_SU; u++)
        if (u * RESAMPLE_THREADS + t < n) tl[u * RESAMPLE_THREADS + t] = sv[c][u];
      const uint8_t *src = a.arena + (I.poff[c] + (uint64_t)ty0 * (uint64_t)I.stride[c] + (uint64_t)tx0[c]);
      for (int i = JR_SU * RESAMPLE_THREADS + t; i < n; i += RESAMPLE_THREADS) {
        const int rr = i / wpr, q = i - rr * wpr;
        tl[i] = *(gu32_t *)(uintptr_t)(src + (uint64_t)rr * (uint64_t)I.stride[c] + 4 * q);
      }
    }
  };
  // the tiles of window rows [cs, cs + nr) -> packed RGB rows 0 .. nr - 1
  const bool q420 = ncomp == 3 && !G.color_rgb && G.he[0] == 1 && G.ve[0] == 1 && G.he[1] == 2 && G.ve[1] == 2 &&
                    G.he[2] == 2 && G.ve[2] == 2 && G.cw[1] > 2 && G.cw[2] > 2;
  auto colour = [&](int cs, int nr) {
    TPlane tp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      int ty0;
      (void)tile_rows(c, cs, nr, &ty0);
      tp[c] = TPlane{lds + P.off_tiles + c * tile_cap, ty0, tx0[c], tpitch[c]};
    }
    const int Y0 = ri + cs, Y1 = Y0 + nr - 1;
    if (q420) {  // one thread per chroma sample: a 2 x 2 quad of pixels (as K2's general path)
      const int R0 = Y0 >> 1, C0 = X0 >> 1, qcols = (X1 >> 1) - C0 + 1;
      const int nq = ((Y1 >> 1) - R0 + 1) * qcols;
      for (int i = t; i < nq; i += RESAMPLE_THREADS) {
        const int qr = i / qcols, Rr = R0 + qr, C = C0 + (i - qr * qcols);
        int cb[4], cr[4];
        upsample_quad_h2v2(tp[1], G.cw[1], G.ch[1], Rr, C, cb);
        upsample_quad_h2v2(tp[2], G.cw[2], G.ch[2], Rr, C, cr);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int Y = 2 * Rr + (u >> 1), X = 2 * C + (u & 1);
          if (Y < Y0 || Y > Y1 || X < X0 || X > X1) continue;
          int v[3];
          ycc_rgb(tp[0].at(Y, X), cb[u], cr[u], v);
          uint8_t *d = s_rgb + (Y - Y0) * pitch + (X - X0) * 3;
          d[0] = (uint8_t)v[0];
          d[1] = (uint8_t)v[1];
          d[2] = (uint8_t)v[2];
        }
      }
    } else {
      for (int i = t; i < nr * cww; i += RESAMPLE_THREADS) {
        const int yy = i / cww, x = i - yy * cww;
        int v[3];
        pixel_rgb(G, tp, Y0 + yy, X0 + x, v);
        uint8_t *d = s_rgb + yy * pitch + x * 3;
        d[0] = (uint8_t)v[0];
        d[1] = (uint8_t)v[1];
        d[2] = (uint8_t)v[2];
      }
    }
  };

  int c0 = r_lo, rows = min(CH, r_hi - r_lo);
  load(c0, rows);
  resample_band_records(t, cww, chh, out_w, out_h, mode, y0, y1, P.kx, P.ky, s_col, s_row);  // under the loads
  store(c0, rows);
  __syncthreads();

  int ydone = y0;
  for (;;) {
    const int c1 = c0 + rows, next_rows = min(CH, r_hi - c1);
    if (next_rows > 0) load(c1, next_rows);
    colour(c0, rows);
    __syncthreads();
    resample_h_pass(t, rows, c0, out_w, s_col, KX, [&](int r) { return (const uint8_t *)s_rgb + r * pitch; }, s_ring,
                    ring_rows, ndw);
    __syncthreads();
    ydone = resample_v_pass(t, ydone, y0, y1, c1, s_row, KY, s_ring, ring_rows, ndw, o, orb);
    if (next_rows <= 0) break;
    store(c1, next_rows);  // (the colour stage has read this chunk's tiles: two barriers ago)
    __syncthreads();
    c0 = c1;
    rows = next_rows;
  }
}
