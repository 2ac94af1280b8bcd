// ffcv_tone.hip -- RandomPosterize / RandomAutocontrast / RandomEqualize /
// RandomInvert: their draws, and a program of one to four of
// them on a uint8 HWC batch, with the host twins.
//
// Every step is a 256-entry byte table per image and channel (tone_common.h).
// A step's table needs at most the channel's histogram as the step finds it,
// and the histogram behind a table step is the one before it pushed through
// the table, h'[T[v]] += h[v].  So a program needs ONE histogram of the image
// as it arrives: the applied steps' tables are built and composed on 3 x 256
// counters, and the pixels are mapped once through the composed tables.
//
// One kernel serves both regimes, like color_jitter_kernel.  A workgroup takes
// a run of whole pixels of one image (the whole image when it fits
// TONE_LDS_BYTES, else a tile of TONE_TILE_PX pixels).
//
//   whole image (TONE_WHOLE): stage the bytes in LDS with 16-byte aligned
//     loads, counting them on the way (LDS atomics, one histogram per
//     workgroup) when an applied step needs statistics; build and compose the
//     tables; map whole words; write back once.  One HBM read, one write.
//   tiles: a program without autocontrast / equalize is one launch (TONE_MAP).
//     With one it is two over a zeroed workspace of 3 x 256 uint32 per image:
//     pass A (TONE_HIST) counts each tile in LDS and adds its non-zero bins
//     to the image's counters (integer atomics: order does not matter, the
//     result is deterministic); in pass B (TONE_MAP) every workgroup rebuilds
//     the image's composed tables from the counters and maps its tile.
//
// The channel of a byte is its offset in the image % 3; tiles start on whole
// pixels, so the channel of staged byte j is (j - lead) % 3, from arithmetic on
// the word index (4 = 16 = 1 mod 3).
//
// LDS: 16 KiB of pixels + 32 B staging slack + 3 KiB counters + the composed
// and the step's tables (768 B each) + 144 B scan partials = 21,168 bytes:
// seven 256-thread workgroups per CU (28 of its 32 waves).  The histogram is
// not privatised per wave (four copies would cost 12 KiB and two workgroups
// per CU); a flat image serialises its LDS atomics on one bin.
#include "api_internal.h"
#include "tone_common.h"

#define TONE_THREADS 256
#define TONE_LDS_BYTES 16384
#define TONE_TILE_PX 4096  // 12 KiB of pixels per workgroup beyond the whole-image regime
enum { TONE_WHOLE = 0, TONE_HIST = 1, TONE_MAP = 2 };

__global__ void __launch_bounds__(64) tone_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed,
                                                       uint64_t epoch, ToneDraw d, uint8_t *__restrict__ apply,
                                                       int32_t *__restrict__ status) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_tone(k, B, ids[k], loader_seed, epoch, d, apply);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

// prog: steps[i] in byte i, n of them; bits_k: posterize's bits per image, or
// NULL for bits_all.  img / npx: bytes / pixels of one image;
// tile_px pixels per workgroup (tile_px * 3 <= TONE_LDS_BYTES), ntiles
// workgroups per image.  ws: 3 x 256 counters per image (tiles with statistics).
__global__ void __launch_bounds__(TONE_THREADS)
    tone_kernel(uint8_t *__restrict__ images, int B, uint64_t img, uint32_t npx, uint32_t prog, int n, int bits_all,
                const uint8_t *__restrict__ bits_k, const uint8_t *__restrict__ apply, uint32_t *__restrict__ ws,
                int mode, uint32_t tile_px, uint32_t ntiles) {
  typedef uint32_t tx4_t __attribute__((ext_vector_type(4)));
  __shared__ tx4_t s_img[TONE_LDS_BYTES / 16 + 2];  // + the range's lead bytes
  __shared__ uint32_t s_hist[3 * 256];              // the channel histograms as the current step finds them
  __shared__ uint8_t s_comp[3 * 256];               // the applied steps so far, composed
  __shared__ uint8_t s_tab[3 * 256];                // the current step
  __shared__ uint32_t s_part[3][TONE_THREADS / 64];
  __shared__ uint64_t s_occ[3][TONE_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t k = blockIdx.x / ntiles, tile = blockIdx.x - k * ntiles;

  // the image's decisions (the same for the whole workgroup)
  uint32_t applied = 0;
  int last_stat = -1;  // the last applied step that needs the histogram
  for (int i = 0; i < n; i++) {
    if (!apply[(uint64_t)i * B + k]) continue;
    applied |= 1u << i;
    if (tone_needs_stats((int)((prog >> (8 * i)) & 0xffu))) last_stat = i;
  }
  if (!applied) return;  // an image no step touches is neither read nor written
  // posterize's bits: the image's own (one scalar load, kept inside 1 .. 8) or the program's
  const int bits = bits_k ? min(8, max(1, (int)bits_k[k])) : bits_all;
  const bool hist = last_stat >= 0;
  if (mode == TONE_HIST && !hist) return;
  uint32_t *wsk = ws + (uint64_t)k * 768u;

  if (hist) {
#pragma unroll
    for (int c = 0; c < 3; c++) s_hist[c * 256 + t] = mode == TONE_MAP ? wsk[c * 256 + t] : 0u;
    __syncthreads();
  }

  // ---- stage pixels [tile * tile_px, ...) of image k, counted from the
  // registers on the way.  This is PixelRun's scheme (lds_stage.h) written out:
  // on the helper this kernel measured slower at 512 x 32 x 32
  // (profiles/lds_stage_ab.txt).
  const uint64_t b0 = (uint64_t)tile * tile_px * 3u;
  const uint32_t nbytes = (uint32_t)(img - b0 < (uint64_t)tile_px * 3u ? img - b0 : (uint64_t)tile_px * 3u);
  uint8_t *src = images + (uint64_t)k * img + b0;
  const uint32_t lead = (uint32_t)((uintptr_t)src & 15);
  typedef __attribute__((address_space(1))) tx4_t gx4_t;
  gx4_t *gp = (gx4_t *)((uintptr_t)src & ~(uintptr_t)15);
  const int nch = (int)((lead + nbytes + 15) >> 4);  // <= TONE_LDS_BYTES / 16 + 1
  const bool count = hist && mode != TONE_MAP;
  for (int i = t; i < nch; i += TONE_THREADS) {
    const tx4_t x = gp[i];
    if (mode != TONE_HIST) s_img[i] = x;
    if (count) {
      const uint32_t j0 = 16u * (uint32_t)i;  // staged byte j is byte j - lead of the range
      uint32_t c = (j0 + 15u - lead) % 3u;    // the channel of byte j0 (15 = 0 mod 3 keeps it positive)
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int wi = 0; wi < 4; wi++) {
#pragma unroll
        for (int bi = 0; bi < 4; bi++) {
          const uint32_t j = j0 + 4u * wi + bi;
          if (j - lead < nbytes) atomicAdd(&s_hist[c * 256u + ((xs[wi] >> (8 * bi)) & 0xffu)], 1u);
          c = c == 2u ? 0u : c + 1u;
        }
      }
    }
  }
  __syncthreads();

  if (mode == TONE_HIST) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const uint32_t v = s_hist[c * 256 + t];
      if (v) atomicAdd(&wsk[c * 256 + t], v);
    }
    return;
  }

  // ---- build and compose the applied steps' tables: thread t owns bin t of
  // the three channels (TONE_THREADS == 256)
#pragma unroll
  for (int c = 0; c < 3; c++) s_comp[c * 256 + t] = (uint8_t)t;
  for (int i = 0; i < n; i++) {
    if (!((applied >> i) & 1u)) continue;
    const int kind = (int)((prog >> (8 * i)) & 0xffu);
    const bool stats = tone_needs_stats(kind), push = i < last_stat;
    uint32_t h[3] = {0u, 0u, 0u}, T[3];
    if (stats || push) {
#pragma unroll
      for (int c = 0; c < 3; c++) h[c] = s_hist[c * 256 + t];
    }
    if (stats) {
      // per wave: which bins are occupied (ballot) and the inclusive sum (scan)
      uint32_t incl[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint64_t occ = __ballot(h[c] != 0u);
        uint32_t s = h[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = __shfl_up(s, d, 64);
          if (lane >= d) s += o;
        }
        incl[c] = s;
        if (lane == 63) s_part[c][wave] = s;
        if (lane == 0) s_occ[c][wave] = occ;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; c++) {
        uint32_t below = incl[c] - h[c], lo = 0u, hi = 0u;
#pragma unroll
        for (int w = 0; w < TONE_THREADS / 64; w++) below += w < wave ? s_part[c][w] : 0u;
#pragma unroll
        for (int w = TONE_THREADS / 64 - 1; w >= 0; w--) {
          const uint64_t occ = s_occ[c][w];
          if (occ) lo = 64u * w + (uint32_t)__builtin_ctzll(occ);
        }
#pragma unroll
        for (int w = 0; w < TONE_THREADS / 64; w++) {
          const uint64_t occ = s_occ[c][w];
          if (occ) hi = 64u * w + 63u - (uint32_t)__builtin_clzll(occ);
        }
        T[c] = tone_entry(kind, bits, npx, lo, hi, s_hist[c * 256 + hi], below, (uint32_t)t);
      }
    } else {
      T[0] = T[1] = T[2] = tone_entry(kind, bits, 0u, 0u, 0u, 0u, 0u, (uint32_t)t);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) s_tab[c * 256 + t] = (uint8_t)T[c];
    __syncthreads();  // s_tab complete; every read of s_hist, s_part and s_occ is behind us
#pragma unroll
    for (int c = 0; c < 3; c++) s_comp[c * 256 + t] = s_tab[c * 256 + s_comp[c * 256 + t]];
    if (push) {  // a later applied step needs the histogram behind this one
#pragma unroll
      for (int c = 0; c < 3; c++) s_hist[c * 256 + t] = 0u;
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (h[c]) atomicAdd(&s_hist[c * 256 + T[c]], h[c]);
    }
    __syncthreads();
  }

  // ---- map the whole words covering the staged bytes (the bytes around them
  // are not written back); word w's first byte is byte 4 w - lead of the range
  uint32_t *s_words = (uint32_t *)s_img;
  const uint32_t w1 = (lead + nbytes + 3) >> 2;
  for (uint32_t w = (lead >> 2) + t; w < w1; w += TONE_THREADS) {
    const uint32_t v = s_words[w];
    const uint32_t c = (w + 15u - lead) % 3u;
    const uint32_t o0 = c * 256u, o1 = (c == 2u ? 0u : c + 1u) * 256u, o2 = (c == 0u ? 2u : c - 1u) * 256u;
    s_words[w] = (uint32_t)s_comp[o0 + (v & 0xffu)] | ((uint32_t)s_comp[o1 + ((v >> 8) & 0xffu)] << 8) |
                 ((uint32_t)s_comp[o2 + ((v >> 16) & 0xffu)] << 16) | ((uint32_t)s_comp[o0 + (v >> 24)] << 24);
  }
  __syncthreads();

  // ---- write back: whole 16-byte chunks inside the range as one store, the
  // two cut by its ends byte by byte (their other bytes belong to a neighbour)
  for (int i = t; i < nch; i += TONE_THREADS) {
    const uint32_t c0 = 16u * (uint32_t)i;
    if (c0 >= lead && c0 + 16u <= lead + nbytes) {
      gp[i] = s_img[i];
    } else {
      const uint8_t *sb = (const uint8_t *)s_img;
      uint8_t *gb = (uint8_t *)((uintptr_t)src & ~(uintptr_t)15);
      for (uint32_t j = c0; j < c0 + 16u; j++)
        if (j >= lead && j < lead + nbytes) gb[j] = sb[j];
    }
  }
}

static int tone_check_program(const char *who, const ffcv_tone_params *p, bool *stats) {
  if (p->n_steps < 1 || p->n_steps > 4) {
    ffcv::set_error("%s: a program has 1 to 4 steps, got %d", who, p->n_steps);
    return FFCV_EINVAL;
  }
  unsigned seen = 0;
  *stats = false;
  for (int i = 0; i < p->n_steps; i++) {
    const int st = p->steps[i];
    if (st < FFCV_TONE_POSTERIZE || st > FFCV_TONE_INVERT) {
      ffcv::set_error("%s: unknown step %d at position %d", who, st, i);
      return FFCV_EINVAL;
    }
    if (seen & (1u << st)) {
      ffcv::set_error("%s: step %d repeated at position %d", who, st, i);
      return FFCV_EINVAL;
    }
    seen |= 1u << st;
    if (st == FFCV_TONE_POSTERIZE && (p->bits < 1 || p->bits > 8)) {
      ffcv::set_error("%s: posterize keeps 1 to 8 bits, got %d", who, p->bits);
      return FFCV_EINVAL;
    }
    *stats |= tone_needs_stats(st);
  }
  return FFCV_OK;
}

static int tone_check_draw(const char *who, const void *ids, int batch, int n, const int32_t *op_ids, const double *p,
                           const void *apply, ToneDraw *d) {
  if (batch < 0 || !ids || !op_ids || !p || !apply || n < 1 || n > 4) {
    ffcv::set_error("%s: invalid arguments (batch %d, %d operations of 1 to 4)", who, batch, n);
    return FFCV_EINVAL;
  }
  d->n = n;
  for (int i = 0; i < 4; i++) {
    d->op[i] = 0;
    d->p[i] = 0.0;
  }
  for (int i = 0; i < n; i++) {
    if (op_ids[i] < 15 || op_ids[i] > 18 || !(p[i] >= 0.0 && p[i] <= 1.0)) {
      ffcv::set_error("%s: invalid arguments (op_id %d in 15..18, p %g) at position %d", who, op_ids[i], p[i], i);
      return FFCV_EINVAL;
    }
    d->op[i] = (uint32_t)op_ids[i];
    d->p[i] = p[i];
  }
  return FFCV_OK;
}

// One channel's table of step `kind` from its histogram, on the host.
static void tone_table_host(int kind, int bits, uint32_t pixels, const uint32_t *h, uint8_t *T) {
  uint32_t lo = 0, hi = 0;
  for (uint32_t v = 0; v < 256; v++)
    if (h[v]) {
      lo = v;
      break;
    }
  for (uint32_t v = 256; v-- > 0;)
    if (h[v]) {
      hi = v;
      break;
    }
  uint32_t below = 0;
  for (uint32_t v = 0; v < 256; v++) {
    T[v] = (uint8_t)tone_entry(kind, bits, pixels, lo, hi, h[hi], below, v);
    below += h[v];
  }
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_tone_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                         int n, const int32_t *op_ids, const double *p, uint8_t *apply, int32_t *status) {
  ToneDraw d;
  if (tone_check_draw("ffcv_tone_draw_batch", sample_ids, batch, n, op_ids, p, apply, &d)) return FFCV_EINVAL;
  return ffcv::launch_draw("tone_draw_kernel", tone_draw_kernel, stream, batch, sample_ids, batch, loader_seed, epoch,
                           d, apply, status);
}

int ffcv_tone_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, int n,
                              const int32_t *op_ids, const double *p, uint8_t *apply) {
  ToneDraw d;
  if (tone_check_draw("ffcv_tone_draw_batch_host", sample_ids, batch, n, op_ids, p, apply, &d)) return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_tone_draw_batch_host", batch,
                         [&](int k) { return draw_tone(k, batch, sample_ids[k], loader_seed, epoch, d, apply); });
}

uint64_t ffcv_tone_workspace_bytes(int batch) { return batch > 0 ? 3072ull * (uint64_t)batch : 0; }
uint64_t ffcv_tone_lds_bytes(void) { return TONE_LDS_BYTES; }

// both device entries; bits: per image or NULL
static int tone_batch(const char *who, void *stream, uint8_t *images, int batch, int height, int width,
                      const ffcv_tone_params *params, const uint8_t *apply, void *workspace,
                      uint64_t workspace_bytes, const uint8_t *bits) {
  if (!ffcv::u8_images_ok(who, images && params && apply, batch, height, width)) return FFCV_EINVAL;
  bool stats = false;
  if (tone_check_program(who, params, &stats)) return FFCV_EINVAL;
  if (batch == 0) return FFCV_OK;
  const int n = params->n_steps;
  uint32_t prog = 0;
  for (int i = 0; i < n; i++) prog |= (uint32_t)params->steps[i] << (8 * i);
  const uint64_t npx = (uint64_t)height * width, img = npx * 3;
  const bool whole = img <= TONE_LDS_BYTES;
  uint32_t tile_px, ntiles;
  unsigned blocks;
  if (!ffcv::run_tiling(who, batch, npx, TONE_LDS_BYTES, TONE_TILE_PX, &tile_px, &ntiles, &blocks))
    return FFCV_EINVAL;
  hipStream_t s = ffcv::as_stream(stream);
  uint32_t *ws = (uint32_t *)workspace;
  if (whole || !stats) {
    hipLaunchKernelGGL(tone_kernel, dim3(blocks), dim3(TONE_THREADS), 0, s, images, batch, img, (uint32_t)npx, prog, n,
                       (int)params->bits, bits, apply, ws, whole ? TONE_WHOLE : TONE_MAP, tile_px, ntiles);
    FFCV_LAUNCH_CHECK("tone_kernel");
    return FFCV_OK;
  }
  if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < ffcv_tone_workspace_bytes(batch)) {
    ffcv::set_error("%s: an autocontrast or equalize step on %dx%d images needs a 4-byte aligned "
                    "workspace of %llu bytes, got %llu",
                    who, height, width, (unsigned long long)ffcv_tone_workspace_bytes(batch),
                    (unsigned long long)workspace_bytes);
    return FFCV_EINVAL;
  }
  FFCV_HIP_CHECK(hipMemsetAsync(workspace, 0, ffcv_tone_workspace_bytes(batch), s));
  hipLaunchKernelGGL(tone_kernel, dim3(blocks), dim3(TONE_THREADS), 0, s, images, batch, img, (uint32_t)npx, prog, n,
                     (int)params->bits, bits, apply, ws, TONE_HIST, tile_px, ntiles);
  FFCV_LAUNCH_CHECK("tone_kernel (pass A)");
  hipLaunchKernelGGL(tone_kernel, dim3(blocks), dim3(TONE_THREADS), 0, s, images, batch, img, (uint32_t)npx, prog, n,
                     (int)params->bits, bits, apply, ws, TONE_MAP, tile_px, ntiles);
  FFCV_LAUNCH_CHECK("tone_kernel (pass B)");
  return FFCV_OK;
}

int ffcv_tone_batch(void *stream, uint8_t *images, int batch, int height, int width, const ffcv_tone_params *params,
                    const uint8_t *apply, void *workspace, uint64_t workspace_bytes) {
  return tone_batch("ffcv_tone_batch", stream, images, batch, height, width, params, apply, workspace,
                    workspace_bytes, NULL);
}

int ffcv_tone_batch_bits(void *stream, uint8_t *images, int batch, int height, int width,
                         const ffcv_tone_params *params, const uint8_t *apply, void *workspace,
                         uint64_t workspace_bytes, const uint8_t *bits) {
  return tone_batch("ffcv_tone_batch_bits", stream, images, batch, height, width, params, apply, workspace,
                    workspace_bytes, bits);
}

// both host entries; bits: per image (each in 1 .. 8 where the program posterizes) or NULL
static int tone_batch_host(const char *who, uint8_t *images, int batch, int height, int width,
                           const ffcv_tone_params *params, const uint8_t *apply, const uint8_t *bits) {
  if (!ffcv::u8_images_ok(who, images && params && apply, batch, height, width)) return FFCV_EINVAL;
  bool stats = false;
  if (tone_check_program(who, params, &stats)) return FFCV_EINVAL;
  if (bits)
    for (int i = 0; i < params->n_steps; i++)
      for (int k = 0; params->steps[i] == FFCV_TONE_POSTERIZE && k < batch; k++)
        if (bits[k] < 1 || bits[k] > 8) {
          ffcv::set_error("%s: posterize keeps 1 to 8 bits, got %d for image %d", who, (int)bits[k], k);
          return FFCV_EINVAL;
        }
  const uint64_t npx = (uint64_t)height * width;
  const int n = params->n_steps;
  for (int k = 0; k < batch; k++) {
    uint8_t *im = images + (uint64_t)k * npx * 3;
    int last = -1, last_stat = -1;
    for (int i = 0; i < n; i++) {
      if (!apply[(uint64_t)i * batch + k]) continue;
      last = i;
      if (tone_needs_stats(params->steps[i])) last_stat = i;
    }
    if (last < 0) continue;
    // the kernel's scheme: one histogram of the image as it arrives, the
    // applied steps' tables built and composed on it, the bytes mapped once
    uint32_t h[3][256], h2[3][256];
    uint8_t comp[3][256], T[256];
    for (int c = 0; c < 3; c++)
      for (int v = 0; v < 256; v++) {
        h[c][v] = 0;
        comp[c][v] = (uint8_t)v;
      }
    if (last_stat >= 0)
      for (uint64_t q = 0; q < npx; q++)
        for (int c = 0; c < 3; c++) h[c][im[3 * q + c]]++;
    for (int i = 0; i <= last; i++) {
      if (!apply[(uint64_t)i * batch + k]) continue;
      for (int c = 0; c < 3; c++) {
        tone_table_host(params->steps[i], bits ? (int)bits[k] : (int)params->bits, (uint32_t)npx, h[c], T);
        for (int v = 0; v < 256; v++) comp[c][v] = T[comp[c][v]];
        if (i < last_stat) {
          for (int v = 0; v < 256; v++) h2[c][v] = 0;
          for (int v = 0; v < 256; v++) h2[c][T[v]] += h[c][v];
          for (int v = 0; v < 256; v++) h[c][v] = h2[c][v];
        }
      }
    }
    for (uint64_t q = 0; q < npx; q++)
      for (int c = 0; c < 3; c++) im[3 * q + c] = comp[c][im[3 * q + c]];
  }
  return FFCV_OK;
}

int ffcv_tone_batch_host(uint8_t *images, int batch, int height, int width, const ffcv_tone_params *params,
                         const uint8_t *apply) {
  return tone_batch_host("ffcv_tone_batch_host", images, batch, height, width, params, apply, NULL);
}

int ffcv_tone_batch_bits_host(uint8_t *images, int batch, int height, int width, const ffcv_tone_params *params,
                              const uint8_t *apply, const uint8_t *bits) {
  return tone_batch_host("ffcv_tone_batch_bits_host", images, batch, height, width, params, apply, bits);
}

int ffcv_tone_tables_host(int kind, int bits, const uint32_t *hists, uint8_t *tables, int n) {
  if (!hists || !tables || n < 0 || kind < FFCV_TONE_POSTERIZE || kind > FFCV_TONE_INVERT ||
      (kind == FFCV_TONE_POSTERIZE && (bits < 1 || bits > 8))) {
    ffcv::set_error("ffcv_tone_tables_host: invalid arguments (kind %d, bits %d, n %d)", kind, bits, n);
    return FFCV_EINVAL;
  }
  for (int j = 0; j < n; j++) {
    const uint32_t *h = hists + 256 * (uint64_t)j;
    uint64_t pixels = 0;
    for (int v = 0; v < 256; v++) pixels += h[v];
    if (pixels > 0x3fffffffull) {
      ffcv::set_error("ffcv_tone_tables_host: histogram %d counts %llu pixels, over 2^30 - 1", j,
                      (unsigned long long)pixels);
      return FFCV_EINVAL;
    }
    tone_table_host(kind, bits, (uint32_t)pixels, h, tables + 256 * (uint64_t)j);
  }
  return FFCV_OK;
}

}  // extern "C"
