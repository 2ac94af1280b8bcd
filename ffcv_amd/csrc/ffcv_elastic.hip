// ffcv_elastic.hip -- ElasticTransform on a dense uint8 batch [B][H][W][3]:
// noise, blur, warp and write-back in ONE launch, and the host twin
// (DESIGN.md s33).
//
// Every pixel has a displacement of its own: a per-pixel hash noise (op id
// 27), blurred by a separable Gaussian of radius R with torch's `reflect`
// border, scaled by alpha.  Nothing of it is stored in memory: a 256-thread
// workgroup owns a tile of ELASTIC_TILE x ELASTIC_TILE outputs of one image
// and rebuilds the field of its tile from the hash.
//
//   (a) noise: the source rectangle the tile's blur reaches (the tile and R
//       around it, clipped to the image) is hashed once, a splitmix64 word per
//       two pixels x two axes, and every value is written to the one to nine
//       places of the tile's (rows + 2R) x (cols + 2R) int16 plane that reflect
//       onto its pixel.  So the passes below see a plain halo and no
//       neighbour workgroup is needed.
//   (b) blur: adjacent int16 pairs of a plane row are one dword, weights are
//       int16 too, so a tap pair is one v_dot2_i32_i16.  A work item of the
//       horizontal pass makes two adjacent outputs from the same R + 1 dwords
//       (the weight pairs of the even and of the odd output, elastic_common.h)
//       and stores them as int16 so that rows 2m and 2m + 1 of a column share
//       a dword.  The vertical pass then runs the same way down the columns:
//       a thread owns a 2 x 2 block of pixels, two axes, eight sums in
//       registers, from one 8-byte LDS read per axis and step.
//   (c) footprint: the extremes of the first tap's column and row over the
//       tile's pixels, by a wave reduction and four LDS atomics per wave.
//       The box they span (a few pixels around the tile at the default alpha)
//       is staged as uint8 rows (lds_stage.h) over the noise planes, which
//       are dead by then, if it takes at most ELASTIC_TILE_LDS bytes.
//   (d) sample: s21's integer sample, every tap tested against the box, into
//       the tile's dense output bytes (over the blur's planes), which leave
//       by the row tile's write-back.  A tile whose box is beyond the budget
//       reads its taps from global memory (the direct regime).
#include <climits>
#include <cmath>
#include <cstring>

#include "api_internal.h"
#include "elastic_common.h"

#define ELASTIC_THREADS 256
#define ELASTIC_TILE 32       // outputs per tile side; a thread owns 2 x 2 of them
#ifndef ELASTIC_TILE_LDS
#define ELASTIC_TILE_LDS 16384  // staged footprint of a tile, at most
#endif
#define ELASTIC_OUT_PITCH (3 * ELASTIC_TILE)  // bytes per row of the tile's output
static_assert(ELASTIC_THREADS * 4 == ELASTIC_TILE * ELASTIC_TILE, "a thread owns 2 x 2 pixels");

typedef short elastic_s2_t __attribute__((ext_vector_type(2)));

// a.lo b.lo + a.hi b.hi + c on int16 halves (v_dot2_i32_i16); the sums of the
// blur stay inside int32 (elastic_common.h), so nothing clamps
FFCV_DEV int elastic_dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(elastic_s2_t, a), __builtin_bit_cast(elastic_s2_t, b), c, false);
}

// How a launch cuts an image into tiles, and the LDS of a workgroup:
//   16 bytes: the footprint's extremes
//   A: the noise planes, two axes of nrows x npd dwords; later 16 bytes |
//      staged source | 16 bytes
//   B: the horizontal pass's planes, two axes of prow x ELASTIC_TILE dwords
//      (a dword: rows 2m and 2m + 1 of a column); later the output bytes
struct ElasticPlan {
  int th, tw, nty, ntx;
  int nrows, npd, prow;
  uint32_t b_off, lds;
};

static ElasticPlan elastic_plan(int H, int W, int R) {
  ElasticPlan P;
  P.th = std::min(H, ELASTIC_TILE);
  P.tw = std::min(W, ELASTIC_TILE);
  P.nty = (H + P.th - 1) / P.th;
  P.ntx = (W + P.tw - 1) / P.tw;
  P.nrows = P.th + 2 * R;
  P.npd = ((P.tw + 1) >> 1) + R;
  P.prow = ((P.th + 1) >> 1) + R;
  const uint32_t a = std::max<uint32_t>(2u * P.nrows * P.npd * 4u, 16u + ELASTIC_TILE_LDS + 16u);
  const uint32_t b = std::max<uint32_t>(2u * P.prow * ELASTIC_TILE * 4u, (uint32_t)P.th * ELASTIC_OUT_PITCH + 32u);
  P.b_off = 16u + ((a + 15u) & ~15u);
  P.lds = P.b_off + ((b + 15u) & ~15u);
  return P;
}

// Taps from the staged box, coordinates relative to its corner.  The box holds
// every tap of the tile that lies inside the image, so a tap outside the box is
// fill.  The LDS read is outside the test, at a clamped address.
struct ElasticLdsTap : LdsRows<true> {
  int nrows, cw;
  uint32_t fill;
  FFCV_DEV uint32_t one(int iy, int ix) const {
    const bool ok = (uint32_t)iy < (uint32_t)nrows && (uint32_t)ix < (uint32_t)cw;
    const uint32_t v = lds_pixel(row(ok ? iy : 0) + 3 * (ok ? ix : 0)) & 0xffffffu;
    return ok ? v : fill;
  }
  // (iy, ix) and (iy, ix + 1): six contiguous bytes from three aligned dwords;
  // the column is clamped to [-1, cw - 1] for the address only (16 bytes lie in
  // front of the first row and 16 behind the last)
  FFCV_DEV void pair(int iy, int ix, uint32_t *t0, uint32_t *t1) const {
    const bool rok = (uint32_t)iy < (uint32_t)nrows;
    const int xc = max(-1, min(ix, cw - 1));
    const uint8_t *a = row(rok ? iy : 0) + 3 * xc;
    const uint32_t *qa = (const uint32_t *)__builtin_align_down(a, 4);
    const uint32_t sh = (uint32_t)(a - (const uint8_t *)qa);
    const uint32_t q0 = qa[0], q1 = qa[1], q2 = qa[2];
    const uint32_t lo4 = __builtin_amdgcn_alignbyte(q1, q0, sh), hi4 = __builtin_amdgcn_alignbyte(q2, q1, sh);
    *t0 = (rok && (uint32_t)ix < (uint32_t)cw) ? lo4 & 0xffffffu : fill;
    *t1 = (rok && (uint32_t)(ix + 1) < (uint32_t)cw) ? ((lo4 >> 24) | (hi4 << 8)) & 0xffffffu : fill;
  }
};

FFCV_DEV int elastic_wave_min(int v) {
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
FFCV_DEV int elastic_wave_max(int v) {
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ void __launch_bounds__(ELASTIC_THREADS)
    elastic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_stride, int H, int W,
                   int mode, uint32_t fill, const uint64_t *__restrict__ ids, uint64_t loader_seed, uint64_t epoch,
                   ElasticBlur bl, ElasticPlan P) {
  extern __shared__ uint4 elastic_smem[];
  int *s_box = (int *)elastic_smem;
  uint8_t *s_a = (uint8_t *)elastic_smem + 16;
  uint8_t *s_b = (uint8_t *)elastic_smem + P.b_off;
  const int t = threadIdx.x;
  const uint32_t per = (uint32_t)P.nty * P.ntx;
  const uint32_t k = blockIdx.x / per, rem = blockIdx.x - k * per;
  const int ty = rem / P.ntx, tx = rem - ty * P.ntx;
  const int y0 = ty * P.th, y1 = min(H, y0 + P.th), x0 = tx * P.tw, x1 = min(W, x0 + P.tw);
  const int rows = y1 - y0, tc = x1 - x0, R = bl.R;
  const uint64_t key = elastic_key(loader_seed, epoch, ids[k]);
  if (t == 0) {
    s_box[0] = s_box[2] = INT_MAX;
    s_box[1] = s_box[3] = INT_MIN;
  }

  // ---- (a) the noise of source rows [rl, rh] x columns [cl, ch], a hash word
  // per two pixels, to every place of the planes that reflects onto it
  {
    const int rl = max(0, y0 - R), rh = min(H - 1, y1 - 1 + R), cl = max(0, x0 - R), ch = min(W - 1, x1 - 1 + R);
    const uint32_t nwr = (uint32_t)((ch - cl + 1) >> 1) + 1u, nitems = (uint32_t)(rh - rl + 1) * nwr;
    int16_t *nz = (int16_t *)s_a;
    const int pitch = 2 * P.npd, plane = P.nrows * pitch, nj = rows + 2 * R, ni = tc + 2 * R;
    for (uint32_t it = t; it < nitems; it += ELASTIC_THREADS) {
      const uint32_t ri = it / nwr, wi = it - ri * nwr;
      const int rr = rl + (int)ri;
      const uint32_t rowp = (uint32_t)rr * (uint32_t)W, q = ((rowp + (uint32_t)cl) >> 1) + wi;
      const uint64_t word = elastic_word(key, q);
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const uint32_t p = 2u * q + e;
        const int cc = (int)(p - rowp);
        if (cc < cl || cc > ch) continue;
        const int16_t ux = (int16_t)elastic_noise(word, p, 0), uy = (int16_t)elastic_noise(word, p, 1);
#pragma unroll
        for (int a = 0; a < 3; a++) {  // the row itself, its mirror at the top edge, at the bottom edge
          const int j = (a == 0 ? rr : (a == 1 ? -rr : 2 * (H - 1) - rr)) - (y0 - R);
          if ((a == 1 && rr == 0) || (a == 2 && rr == H - 1) || j < 0 || j >= nj) continue;
#pragma unroll
          for (int b = 0; b < 3; b++) {
            const int i = (b == 0 ? cc : (b == 1 ? -cc : 2 * (W - 1) - cc)) - (x0 - R);
            if ((b == 1 && cc == 0) || (b == 2 && cc == W - 1) || i < 0 || i >= ni) continue;
            nz[j * pitch + i] = ux;
            nz[plane + j * pitch + i] = uy;
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- (b) horizontal: plane row j, axis a, outputs 2m and 2m + 1
  {
    const uint32_t *nzw = (const uint32_t *)s_a;
    int16_t *hp = (int16_t *)s_b;
    const int nj = rows + 2 * R, nm = (tc + 1) >> 1;
    for (int it = t; it < nj * 32; it += ELASTIC_THREADS) {
      const int m = it & 15, a = (it >> 4) & 1, j = it >> 5;
      if (m >= nm) continue;
      const uint32_t *row = nzw + (a * P.nrows + j) * P.npd + m;
      int he = 0, ho = 0;
      for (int mm = 0; mm <= R; mm++) {
        const uint32_t v = row[mm];
        he = elastic_dot2(v, bl.even[mm], he);
        ho = elastic_dot2(v, bl.odd[mm], ho);
      }
      int16_t *o = hp + ((a * P.prow + (j >> 1)) * ELASTIC_TILE + 2 * m) * 2 + (j & 1);
      o[0] = (int16_t)elastic_h16(he);
      o[2] = (int16_t)elastic_h16(ho);
    }
  }
  __syncthreads();

  // ---- vertical, into registers: rows 2 br, 2 br + 1 x columns 2 bc, 2 bc + 1
  const int br = t >> 4, bc = t & 15;
  int64_t X[4], Y[4];  // pixel e: row 2 br + (e >> 1), column 2 bc + (e & 1)
  {
    int vx[4] = {0, 0, 0, 0}, vy[4] = {0, 0, 0, 0};
    if (2 * br < rows) {
      const uint2 *hx = (const uint2 *)s_b + br * (ELASTIC_TILE / 2) + bc;
      const uint2 *hy = hx + P.prow * (ELASTIC_TILE / 2);
      for (int mm = 0; mm <= R; mm++) {
        const uint2 a = hx[mm * (ELASTIC_TILE / 2)], b = hy[mm * (ELASTIC_TILE / 2)];
        const uint32_t we = bl.even[mm], wo = bl.odd[mm];
        vx[0] = elastic_dot2(a.x, we, vx[0]);
        vx[1] = elastic_dot2(a.y, we, vx[1]);
        vx[2] = elastic_dot2(a.x, wo, vx[2]);
        vx[3] = elastic_dot2(a.y, wo, vx[3]);
        vy[0] = elastic_dot2(b.x, we, vy[0]);
        vy[1] = elastic_dot2(b.y, we, vy[1]);
        vy[2] = elastic_dot2(b.x, wo, vy[2]);
        vy[3] = elastic_dot2(b.y, wo, vy[3]);
      }
    }
    // ---- (c) the tile's footprint
    int ixmin = INT_MAX, ixmax = INT_MIN, iymin = INT_MAX, iymax = INT_MIN;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int r = 2 * br + (e >> 1), c = 2 * bc + (e & 1);
      X[e] = ((int64_t)(x0 + c) << 16) + elastic_disp(bl.amp, vx[e]);
      Y[e] = ((int64_t)(y0 + r) << 16) + elastic_disp(bl.amp, vy[e]);
      if (r < rows && c < tc) {
        const int ix = elastic_tap(mode, X[e], W), iy = elastic_tap(mode, Y[e], H);
        ixmin = min(ixmin, ix), ixmax = max(ixmax, ix), iymin = min(iymin, iy), iymax = max(iymax, iy);
      }
    }
    ixmin = elastic_wave_min(ixmin), ixmax = elastic_wave_max(ixmax);
    iymin = elastic_wave_min(iymin), iymax = elastic_wave_max(iymax);
    if ((t & 63) == 0) {
      atomicMin(&s_box[0], ixmin);
      atomicMax(&s_box[1], ixmax);
      atomicMin(&s_box[2], iymin);
      atomicMax(&s_box[3], iymax);
    }
  }
  __syncthreads();
  AffineBox box = elastic_box(mode, H, W, __builtin_amdgcn_readfirstlane(s_box[0]),
                              __builtin_amdgcn_readfirstlane(s_box[1]), __builtin_amdgcn_readfirstlane(s_box[2]),
                              __builtin_amdgcn_readfirstlane(s_box[3]));
  const bool staged = !box.empty() && box.staged_bytes(W) <= ELASTIC_TILE_LDS;

  // ---- (d) sample into the tile's output bytes
  const uint64_t step = (uint64_t)W * 3u;
  const uint8_t *img = src + (uint64_t)k * H * step;
  uint8_t *s_out = s_b;
  uint32_t v[4];
  if (staged) {
    lds_x4_t *s_u8 = (lds_x4_t *)s_a + 1;  // behind 16 bytes a tap at column -1 may read
    const int nrows = box.hi - box.lo, cw = box.ch - box.cl;
    const uint64_t src0 = (uint64_t)(uintptr_t)img + ((uint64_t)box.lo * W + box.cl) * 3u;
    const bool span = cw == W;
    const int n_srows = span ? 1 : nrows;
    const uint32_t srow_bytes = span ? (uint32_t)nrows * 3u * W : 3u * cw;
    const int nchr = (int)lds_chunks(srow_bytes);
    stage_rows<ELASTIC_THREADS>(t, src0, step, n_srows, srow_bytes, nchr, s_u8);
    __syncthreads();
    const ElasticLdsTap tap{lds_rows<true>(s_u8, src0, step, span, nchr), nrows, cw, fill};
    // A pixel with X outside [-1, W) or Y outside [-1, H) has every tap outside
    // the image: fill.  The others' coordinates less the box's corner lie
    // within (-2^31, 2^31).
    const int64_t Wq = (int64_t)W << 16, Hq = (int64_t)H << 16;
    const int64_t ox = (int64_t)box.cl << 16, oy = (int64_t)box.lo << 16;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const bool in = X[e] >= -65536 && X[e] < Wq && Y[e] >= -65536 && Y[e] < Hq;
      v[e] = fill;
      if (in) v[e] = affine_sample<int32_t>(mode, (int32_t)(X[e] - ox), (int32_t)(Y[e] - oy), tap);
    }
  } else {
    AffineMemTap mem;
    mem.img = img;
    mem.H = H;
    mem.W = W;
    mem.fill = fill;
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = affine_sample<int64_t>(mode, X[e], Y[e], mem);
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {  // two pixels, six bytes at an even offset
    const int r = 2 * br + h;
    if (r < rows) {
      uint16_t *o = (uint16_t *)(s_out + r * ELASTIC_OUT_PITCH + 6 * bc);
      const uint32_t v0 = v[2 * h], v1 = v[2 * h + 1];
      o[0] = (uint16_t)v0;
      o[1] = (uint16_t)((v0 >> 16) | (v1 << 8));
      o[2] = (uint16_t)(v1 >> 8);
    }
  }
  __syncthreads();

  // ---- write back; rows that span the width at the output's pitch are one range
  const bool ospan = tc == W && 3 * W == ELASTIC_OUT_PITCH;
  const uint64_t dst0 = (uint64_t)(uintptr_t)dst + (uint64_t)k * dst_stride + ((uint64_t)y0 * W + x0) * 3u;
  write_back_rows<ELASTIC_THREADS>(t, dst0, step, ospan ? 1 : rows, ospan ? (uint32_t)rows * 3u * W : 3u * tc,
                                   [&](int y) { return (const uint8_t *)s_out + y * ELASTIC_OUT_PITCH; });
}

namespace {

// the checks of every entry; *bl: the blur of (alpha, sigma)
bool elastic_shape_ok(const char *who, int height, int width, int mode, double alpha, double sigma, ElasticBlur *bl) {
  if (height < 2 || width < 2 || height > FFCV_AFFINE_MAX_DIM || width > FFCV_AFFINE_MAX_DIM) {
    ffcv::set_error("%s: images of %dx%d have a side outside 2 .. %d", who, height, width, FFCV_AFFINE_MAX_DIM);
    return false;
  }
  if ((uint64_t)height * width * 3u > 0x7fffffffull) {
    ffcv::set_error("%s: images of %dx%d exceed the supported 2^31 - 1 bytes", who, height, width);
    return false;
  }
  if (mode != FFCV_AFFINE_BILINEAR && mode != FFCV_AFFINE_NEAREST) {
    ffcv::set_error("%s: mode %d is neither FFCV_AFFINE_BILINEAR nor FFCV_AFFINE_NEAREST", who, mode);
    return false;
  }
  if (!elastic_blur(alpha, sigma, bl)) {
    ffcv::set_error("%s: alpha %g outside [0, %d] or sigma %g outside [1, %g]", who, alpha, ELASTIC_MAX_ALPHA, sigma,
                    (2 * ELASTIC_MAX_R) / 8.0);
    return false;
  }
  if (bl->R > std::min(height, width) - 1) {
    ffcv::set_error("%s: sigma %g blurs over %d pixels a side, images of %dx%d carry %d", who, sigma, bl->R, height,
                    width, std::min(height, width) - 1);
    return false;
  }
  return true;
}

bool elastic_args_ok(const char *who, const uint8_t *src, const uint8_t *dst, int batch, int height, int width,
                     int mode, const uint8_t *fill, const uint64_t *ids, double alpha, double sigma,
                     uint64_t dst_stride, uint64_t *stride, ElasticBlur *bl) {
  return ffcv::out_of_place_ok(who, fill && ids, src, dst, batch, height, width, FFCV_AFFINE_MAX_DIM, dst_stride,
                               stride) &&
         elastic_shape_ok(who, height, width, mode, alpha, sigma, bl);
}

uint32_t elastic_pack_fill(const uint8_t *fill) {
  return (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
}

// The host twin's field: the Q16 coordinates of every pixel of one image, the
// statement's loops over whole planes.
struct ElasticField {
  std::vector<int16_t> u, h;
  std::vector<int64_t> X, Y;
  void make(uint64_t key, int H, int W, const ElasticBlur &bl) {
    const size_t n = (size_t)H * W;
    const int R = bl.R;
    u.resize(2 * n), h.resize(2 * n), X.resize(n), Y.resize(n);
    for (size_t p = 0; p < n; p++) {
      const uint64_t word = elastic_word(key, p >> 1);
      u[p] = (int16_t)elastic_noise(word, (uint32_t)p, 0);
      u[n + p] = (int16_t)elastic_noise(word, (uint32_t)p, 1);
    }
    for (int a = 0; a < 2; a++)
      for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
          int s = 0;
          for (int i = -R; i <= R; i++) s += bl.w(i + R) * u[a * n + (size_t)r * W + elastic_reflect(c + i, W)];
          h[a * n + (size_t)r * W + c] = (int16_t)elastic_h16(s);
        }
    for (int r = 0; r < H; r++)
      for (int c = 0; c < W; c++) {
        int sx = 0, sy = 0;
        for (int j = -R; j <= R; j++) {
          const size_t at = (size_t)elastic_reflect(r + j, H) * W + c;
          sx += bl.w(j + R) * h[at];
          sy += bl.w(j + R) * h[n + at];
        }
        X[(size_t)r * W + c] = ((int64_t)c << 16) + elastic_disp(bl.amp, sx);
        Y[(size_t)r * W + c] = ((int64_t)r << 16) + elastic_disp(bl.amp, sy);
      }
  }
};

}  // namespace

// ---------------------------------------------------------- C ABI -------
extern "C" {

uint64_t ffcv_elastic_tile_rows(void) { return ELASTIC_TILE; }
uint64_t ffcv_elastic_tile_cols(void) { return ELASTIC_TILE; }
uint64_t ffcv_elastic_tile_lds(void) { return ELASTIC_TILE_LDS; }

uint64_t ffcv_elastic_lds_bytes(int height, int width, double sigma) {
  ElasticBlur bl;
  if (!elastic_shape_ok("ffcv_elastic_lds_bytes", height, width, FFCV_AFFINE_BILINEAR, 0.0, sigma, &bl)) return 0;
  return elastic_plan(height, width, bl.R).lds;
}

uint64_t ffcv_elastic_tile_bytes(int height, int width, int mode, uint64_t sample_id, uint64_t loader_seed,
                                 uint64_t epoch, double alpha, double sigma, int tile_row, int tile_col) {
  ElasticBlur bl;
  if (!elastic_shape_ok("ffcv_elastic_tile_bytes", height, width, mode, alpha, sigma, &bl)) return 0;
  const ElasticPlan P = elastic_plan(height, width, bl.R);
  if (tile_row < 0 || tile_row >= P.nty || tile_col < 0 || tile_col >= P.ntx) return 0;
  ElasticField f;
  f.make(elastic_key(loader_seed, epoch, sample_id), height, width, bl);
  const int y0 = tile_row * P.th, y1 = std::min(height, y0 + P.th), x0 = tile_col * P.tw,
            x1 = std::min(width, x0 + P.tw);
  int ixmin = INT_MAX, ixmax = INT_MIN, iymin = INT_MAX, iymax = INT_MIN;
  for (int r = y0; r < y1; r++)
    for (int c = x0; c < x1; c++) {
      const int ix = elastic_tap(mode, f.X[(size_t)r * width + c], width),
                iy = elastic_tap(mode, f.Y[(size_t)r * width + c], height);
      ixmin = std::min(ixmin, ix), ixmax = std::max(ixmax, ix);
      iymin = std::min(iymin, iy), iymax = std::max(iymax, iy);
    }
  return elastic_box(mode, height, width, ixmin, ixmax, iymin, iymax).staged_bytes(width);
}

int ffcv_elastic_batch(void *stream, const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                       const uint8_t *fill, const uint64_t *sample_ids, uint64_t loader_seed, uint64_t epoch,
                       double alpha, double sigma, uint64_t dst_stride_bytes) {
  uint64_t stride;
  ElasticBlur bl;
  if (!elastic_args_ok("ffcv_elastic_batch", src, dst, batch, height, width, mode, fill, sample_ids, alpha, sigma,
                       dst_stride_bytes, &stride, &bl))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const ElasticPlan P = elastic_plan(height, width, bl.R);
  return ffcv::launch_tiles("ffcv_elastic_batch", "elastic_kernel", elastic_kernel, stream,
                            (uint64_t)batch * P.nty * P.ntx, ELASTIC_THREADS, P.lds, src, dst, stride, height, width,
                            mode, elastic_pack_fill(fill), sample_ids, loader_seed, epoch, bl, P);
}

int ffcv_elastic_batch_host(const uint8_t *src, uint8_t *dst, int batch, int height, int width, int mode,
                            const uint8_t *fill, const uint64_t *sample_ids, uint64_t loader_seed, uint64_t epoch,
                            double alpha, double sigma, uint64_t dst_stride_bytes, int nthreads) {
  uint64_t stride;
  ElasticBlur bl;
  if (!elastic_args_ok("ffcv_elastic_batch_host", src, dst, batch, height, width, mode, fill, sample_ids, alpha, sigma,
                       dst_stride_bytes, &stride, &bl))
    return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const uint32_t f = elastic_pack_fill(fill);
  ffcv::host_images<ElasticField>(nthreads, batch, src, dst, (uint64_t)height * width * 3, stride,
                                  [&](uint64_t k, const uint8_t *in, uint8_t *out, ElasticField &field) {
                                    field.make(elastic_key(loader_seed, epoch, sample_ids[k]), height, width, bl);
                                    AffineMemTap tap;
                                    tap.img = in;
                                    tap.H = height;
                                    tap.W = width;
                                    tap.fill = f;
                                    for (size_t p = 0; p < (size_t)height * width; p++) {
                                      const uint32_t v = affine_sample<int64_t>(mode, field.X[p], field.Y[p], tap);
                                      out[3 * p] = (uint8_t)v;
                                      out[3 * p + 1] = (uint8_t)(v >> 8);
                                      out[3 * p + 2] = (uint8_t)(v >> 16);
                                    }
                                    return true;
                                  });
  return FFCV_OK;
}

}  // extern "C"
