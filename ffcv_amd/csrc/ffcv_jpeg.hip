// ffcv_jpeg.hip -- baseline JPEG decode on gfx950, fused with the RRC crop,
// INTER_AREA resize and the flip / cutout / normalize epilogue.
//
// Reference: rgb_image.py:194-208 decodes every JPEG in full with
// libjpeg-turbo (libffcv.cpp:104-106: tjDecompress2(TJPF_RGB,
// TJFLAG_FASTDCT) = ifast IDCT + fancy upsampling + fixed-point YCbCr->RGB)
// into a temp buffer, then crops and resizes on the CPU.
//
// Launches per batch (launch_rrc): k1_order_kernel (size-sorted image order),
// then three kernels on the launch's stream:
//
// K1 jpeg_entropy_kernel -- ONE WAVE (64 lanes) per image, four images per
// 256-thread workgroup sharing one LDS table set (38.8 KB: 16 images per CU).
// (A self-synchronising Huffman decode costs about the same latency at 64 or
// 256 lanes per image -- the latency is the resynchronisation distance -- but
// a third of the lane-steps at 64, so the wave-per-image shape triples
// throughput.  A wave once could also decode two images side by side, 32
// lanes each: slower and in the end no longer exact, DESIGN.md s6 "What was
// tried"; the lanes-per-image parameter and its segmented wave helpers last
// existed in commit 356ba29.)
//   P0  gather (table[ids[k]]) and the RRC / cutout / flip draws (wave 0 for
//       the workgroup); the first 2 KB of the file staged in LDS; the whole
//       wave walks the markers (SOF/DHT/DQT/DRI/SOS) on wave-uniform values,
//       validates geometry and tables, and hands out Huffman table slots
//   P1  Huffman decode tables (jdhuff.c jpeg_make_d_derived_tbl, with its
//       checks): per slot an 11-bit (luma AC), 10-bit (chroma AC) or 8-bit
//       (DC) first-level LUT with two-symbol pair entries, a 5-bit second
//       level for longer codes, canonical limits for the rest; ifast
//       dequantisation multipliers (jddctmgr.c); built once per workgroup when
//       its images' tables agree, else per image in global scratch
//   P2  de-stuffing (0xFF00 -> 0xFF) of the entropy-coded segment in stream
//       order, one coalesced dword per lane per step with a wave scan of the
//       kept-byte counts, into an L2-resident scratch stream (zero-padded:
//       libjpeg fills zeros after a marker)
//   P3  self-synchronising parallel Huffman decode.  The stream is cut into
//       one bit range per lane; a lane decodes its range from a guessed state
//       (bit position, coefficient index z, block-in-MCU), records where its
//       blocks start, and the state at which it leaves the range.  Each
//       further round gives lane t the exit state of lane t-1; a lane whose
//       guess changed re-decodes only until it reaches a block start it
//       recorded before (same bit position and MCU phase: from there its old
//       trajectory is exact).  Lane 0 is exact, so round r fixes lanes 0..r
//       at worst; rounds end when no guess changes.  (The entropy index skips
//       these rounds for a sample decoded before.)
//   P4  wave scan of blocks-started -> each lane's first block index
//   P5  write pass: DC differences summed per lane, quantised AC coefficients
//       (zigzag order) of the blocks the crop window needs, into a zeroed
//       window; K2's resize plan and linear tap table
//
// K1b jpeg_idct_kernel -- one workgroup per image: DC prediction from the
//   per-lane sums, de-zigzag + dequantise + ifast IDCT (jidctfst.c) of the
//   window's blocks -> component planes in scratch; K2's per-band records
//   (K2BandRec: one thread per band).
//
// K2 jpeg_color_resize_kernel -- one workgroup per band of 16 output rows:
//   reads the band's record (path, source rows, tiles, LDS layout), stages
//   the band's plane tiles and then its source rows of the crop as RGB
//   in LDS (jdsample.c fancy upsampling + jdcolor.c fixed-point YCbCr->RGB,
//   once per source pixel), then computes the band's output pixels with the
//   OpenCV 4.5.4 resize restatement (linear walk, area walk, or the general
//   per-pixel path) + flip / cutout / LUT epilogue.
//
// Every integer step matches libjpeg-turbo bit for bit
// (tests/test_kernels_gpu.py); float steps use -ffp-contract=off.
//
// This file is the one translation unit of all of it: the context, the C ABI
// and the launches are below; the kernels are in the headers it includes, in
// this order (jpeg_defs.h: tunables, the records between the kernels, wave
// helpers; jpeg_entropy.h: K1 and k1_order_kernel; jpeg_idct.h: K1b;
// jpeg_color_resize.h: K2 and k2_rec_kernel).
#include <climits>

#include "api_internal.h"
#include "jpeg_defs.h"
#include "jpeg_entropy.h"
#include "jpeg_idct.h"
#include "jpeg_color_resize.h"

// ---------------------------------------------------------------- ctx -----
struct ffcv_jpeg_ctx {
  uint64_t *dbg;
  int diag_only;    // diagnostics (ffcv_jpeg_set_diag): kernels a launch runs
  int max_batch;
  uint32_t max_h, max_w;
  uint64_t max_bytes;
  uint8_t *arena;  // per-launch scratch, bump-allocated per image by K1
  uint64_t arena_bytes;
  unsigned long long *arena_top;  // [0] bump counter, [1] high water of the last launch K2 closed
  bool arena_zero;  // [0] is 0 at the stream's tail: the last launch ran K2, which zeroes it
  ImgInfo *info;
  uint2 *taps;
  K2BandRec *brec;  // K2's band records: max_batch x brec_cap (launch_rrc grows it for taller outputs)
  int brec_cap;
  uint8_t *gtab;
  uint32_t *k1_order;  // max_batch slots (k1_order_kernel); used when k1_sorted
  bool k1_sorted;
  uint64_t gtab_slot;
  uint32_t *eidx;  // entropy index (caller-owned), or NULL
  uint64_t eidx_n;
  // per-kernel timing (ffcv_jpeg_set_timing): 4 events per launch recorded on
  // the launch's stream before K1, after K1, after K1b and after K2
  hipEvent_t *tev;
  int tev_cap, tev_n;
};

static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

static void free_timing(ffcv_jpeg_ctx *c) {
  for (int i = 0; i < 4 * c->tev_cap; i++) (void)hipEventDestroy(c->tev[i]);
  delete[] c->tev;
  c->tev = nullptr;
  c->tev_cap = c->tev_n = 0;
}

static void free_ctx(ffcv_jpeg_ctx *c) {
  free_timing(c);
  (void)hipFree(c->arena);
  (void)hipFree(c->arena_top);
  (void)hipFree(c->info);
  (void)hipFree(c->taps);
  (void)hipFree(c->brec);
  (void)hipFree(c->gtab);
  (void)hipFree(c->k1_order);
  delete c;
}

extern "C" {

uint64_t ffcv_jpeg_scratch_bound(uint32_t height, uint32_t width, uint64_t nbytes) {
  // every region alloc_scratch can take for an image of this size, whatever
  // its crop, sampling and MCU padding (hmax, vmax <= 4; <= 10 blocks per MCU)
  const uint64_t blocks = 3 * ((uint64_t)(width + 7) / 8 + 4) * ((uint64_t)(height + 7) / 8 + 4);
  return align_up(nbytes + 64, 256) + align_up(blocks * 128, 256) + align_up(blocks * 2, 256) +
         align_up(blocks * 64, 256) + align_up((uint64_t)height * width * 3, 256);
}

int ffcv_jpeg_create_arena(ffcv_jpeg_ctx **out, int max_batch, uint32_t max_height, uint32_t max_width,
                           uint64_t max_bytes, uint64_t arena_bytes) {
  if (!out || max_batch <= 0 || max_height == 0 || max_width == 0 || max_height > 65535 ||
      max_width > 65535 || max_bytes == 0) {
    ffcv::set_error("ffcv_jpeg_create: invalid arguments");
    return FFCV_EINVAL;
  }
  ffcv_jpeg_ctx *c = new ffcv_jpeg_ctx();
  c->max_batch = max_batch;
  c->diag_only = 7;
  {
    const char *o = getenv("FFCV_K1_ORDER");  // size-grouped K1 workgroups (A/B knob: 0 turns it off)
    c->k1_sorted = !o || atoi(o) != 0;
  }
  c->max_h = max_height;
  c->max_w = max_width;
  c->max_bytes = max_bytes;
  // default: room for max_batch images of the maximum size (never exhausted)
  c->arena_bytes = arena_bytes ? arena_bytes
                               : (uint64_t)max_batch * ffcv_jpeg_scratch_bound(max_height, max_width, max_bytes);
  c->gtab_slot = align_up(sizeof(JTables), 256);
  hipError_t e;
  if ((e = hipMalloc(&c->arena, c->arena_bytes)) != hipSuccess ||
      (e = hipMalloc(&c->arena_top, 2 * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMemset(c->arena_top, 0, 2 * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMalloc(&c->info, sizeof(ImgInfo) * max_batch)) != hipSuccess ||
      (e = hipMalloc(&c->taps, sizeof(uint2) * K2_TAPS * max_batch)) != hipSuccess ||
      (e = hipMalloc(&c->brec, sizeof(K2BandRec) * K2_REC_BANDS * max_batch)) != hipSuccess ||
      (e = hipMalloc(&c->gtab, c->gtab_slot * max_batch)) != hipSuccess ||
      (e = hipMalloc(&c->k1_order, sizeof(uint32_t) * max_batch)) != hipSuccess ||
      // the memset above runs on the null stream, which the caller's
      // non-blocking streams do not wait for: finish it here (a first launch
      // on another stream read a stale counter left in reused memory and
      // failed every image TOO_LARGE)
      (e = hipStreamSynchronize(nullptr)) != hipSuccess) {
    int rc = ffcv::check_hip(e, "ffcv_jpeg_create: hipMalloc");
    free_ctx(c);
    return rc;
  }
  c->brec_cap = K2_REC_BANDS;
  c->arena_zero = false;  // the first launch also zeroes the counter, on its own stream
  *out = c;
  return FFCV_OK;
}

int ffcv_jpeg_create(ffcv_jpeg_ctx **out, int max_batch, uint32_t max_height, uint32_t max_width,
                     uint64_t max_bytes) {
  return ffcv_jpeg_create_arena(out, max_batch, max_height, max_width, max_bytes, 0);
}

// Diagnostic hook (not in the public header): per-image phase stamps
// (wall_clock64, 100 MHz) into dbg[B][16]; NULL disables.
int ffcv_jpeg_set_debug(ffcv_jpeg_ctx *c, uint64_t *dbg) {
  if (!c) return FFCV_EINVAL;
  c->dbg = dbg;
  return FFCV_OK;
}

// Diagnostic hook (not in the public header): which kernels a decode launch
// runs (bit 0 = K1, bit 1 = the IDCT kernel, bit 2 = K2; timing of one kernel
// re-run on the previous launch's scratch) and K2 timing-only flags.  Set once per context, never
// read from the environment on the launch path.
int ffcv_jpeg_set_diag(ffcv_jpeg_ctx *c, int only, int k2flags) {
  // (k2flags: the K2 timing-only switches of rounds 1-4 are gone from the
  // product kernels; only 0 is accepted)
  if (!c || k2flags != 0) return FFCV_EINVAL;
  c->diag_only = only ? only : 7;
  return FFCV_OK;
}

int ffcv_jpeg_set_timing(ffcv_jpeg_ctx *c, int max_launches) {
  if (!c || max_launches < 0) {
    ffcv::set_error("ffcv_jpeg_set_timing: invalid arguments");
    return FFCV_EINVAL;
  }
  free_timing(c);
  if (!max_launches) return FFCV_OK;
  c->tev = new hipEvent_t[4 * (size_t)max_launches]();
  for (int i = 0; i < 4 * max_launches; i++) {
    hipError_t e = hipEventCreate(&c->tev[i]);
    if (e != hipSuccess) {
      c->tev_cap = i / 4;  // destroy what was made (whole sets, then the partial one)
      for (int j = 4 * c->tev_cap; j < i; j++) (void)hipEventDestroy(c->tev[j]);
      free_timing(c);
      return ffcv::check_hip(e, "ffcv_jpeg_set_timing: hipEventCreate");
    }
  }
  c->tev_cap = max_launches;
  c->tev_n = 0;
  return FFCV_OK;
}

int ffcv_jpeg_timing_read(ffcv_jpeg_ctx *c, float *ms, int max_launches, int *n_launches) {
  if (!c || !n_launches || (max_launches && !ms)) {
    ffcv::set_error("ffcv_jpeg_timing_read: invalid arguments");
    return FFCV_EINVAL;
  }
  const int n = c->tev_n < max_launches ? c->tev_n : max_launches;
  for (int i = 0; i < n; i++) {
    FFCV_HIP_CHECK(hipEventSynchronize(c->tev[4 * i + 3]));
    for (int q = 0; q < 3; q++) FFCV_HIP_CHECK(hipEventElapsedTime(&ms[3 * i + q], c->tev[4 * i + q], c->tev[4 * i + q + 1]));
  }
  *n_launches = n;
  c->tev_n = 0;
  return FFCV_OK;
}

// Diagnostic hook (not in the public header): the DC lane table the last
// RRC / FULL launch's entropy kernel wrote for images [0, n): lane_blk0[64]
// (first block each lane started, non-decreasing), lane_off[3][64] (the
// lanes' exclusive DC offsets per component) and the image status.
int ffcv_jpeg_lane_table(ffcv_jpeg_ctx *c, void *stream, int n, uint32_t *blk0, int32_t *off, int32_t *status) {
  if (!c || n < 0 || n > c->max_batch || !blk0 || !off || !status) {
    ffcv::set_error("ffcv_jpeg_lane_table: invalid arguments");
    return FFCV_EINVAL;
  }
  hipStream_t s = ffcv::as_stream(stream);
  ImgInfo *h = new ImgInfo[n > 0 ? n : 1];
  hipError_t e = hipMemcpyAsync(h, c->info, sizeof(ImgInfo) * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    delete[] h;
    return ffcv::check_hip(e, "ffcv_jpeg_lane_table");
  }
  for (int k = 0; k < n; k++) {
    status[k] = h[k].status;
    for (int l = 0; l < 64; l++) {
      blk0[64 * k + l] = h[k].lane_blk0[l];
      for (int q = 0; q < 3; q++) off[192 * k + 64 * q + l] = h[k].lane_off[q][l];
    }
  }
  delete[] h;
  return FFCV_OK;
}

// Diagnostic hook (not in the public header): the arena reservation the last
// launch's entropy kernel made for images [0, n) -- base offset and size in
// bytes (size 0: the image reserved nothing; K1 clears it for every image
// before the parse) -- and the arena's capacity.  Statuses come from the
// launch's own status array.
int ffcv_jpeg_arena_regions(ffcv_jpeg_ctx *c, void *stream, int n, uint64_t *base, uint64_t *size,
                            uint64_t *capacity) {
  if (!c || n < 0 || n > c->max_batch || !base || !size) {
    ffcv::set_error("ffcv_jpeg_arena_regions: invalid arguments");
    return FFCV_EINVAL;
  }
  hipStream_t s = ffcv::as_stream(stream);
  ImgInfo *h = new ImgInfo[n > 0 ? n : 1];
  hipError_t e = hipMemcpyAsync(h, c->info, sizeof(ImgInfo) * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    delete[] h;
    return ffcv::check_hip(e, "ffcv_jpeg_arena_regions");
  }
  for (int k = 0; k < n; k++) {
    base[k] = h[k].arena_base;
    size[k] = h[k].arena_need;
  }
  if (capacity) *capacity = c->arena_bytes;
  delete[] h;
  return FFCV_OK;
}

int ffcv_jpeg_set_entropy_index(ffcv_jpeg_ctx *c, uint32_t *index, uint64_t n_samples) {
  if (!c || (!index && n_samples)) {
    ffcv::set_error("ffcv_jpeg_set_entropy_index: invalid arguments");
    return FFCV_EINVAL;
  }
  c->eidx = index;
  c->eidx_n = index ? n_samples : 0;
  return FFCV_OK;
}

int ffcv_jpeg_arena_used(ffcv_jpeg_ctx *c, void *stream, uint64_t *used, uint64_t *capacity) {
  if (!c || !used) {
    ffcv::set_error("ffcv_jpeg_arena_used: invalid arguments");
    return FFCV_EINVAL;
  }
  unsigned long long v[2] = {0, 0};
  hipStream_t s = ffcv::as_stream(stream);
  FFCV_HIP_CHECK(hipMemcpyAsync(v, c->arena_top, sizeof(v), hipMemcpyDeviceToHost, s));
  FFCV_HIP_CHECK(hipStreamSynchronize(s));
  *used = c->arena_zero ? v[1] : v[0];
  if (capacity) *capacity = c->arena_bytes;
  return FFCV_OK;
}

int ffcv_jpeg_destroy(ffcv_jpeg_ctx *c) {
  if (c) free_ctx(c);
  return FFCV_OK;
}

static JpegArgs make_args(ffcv_jpeg_ctx *c, const uint8_t *base, const ffcv_sample *samples, int batch,
                          int32_t *status) {
  JpegArgs a = {};
  a.batch = batch;
  a.base = base;
  a.samples = samples;
  a.status = status;
  a.arena = c->arena;
  a.arena_bytes = c->arena_bytes;
  a.arena_top = c->arena_top;
  a.info = c->info;
  a.taps = c->taps;
  a.eidx = c->eidx;
  a.eidx_n = c->eidx_n;
  a.gtab = c->gtab;
  a.gtab_slot = c->gtab_slot;
  a.max_h = c->max_h;
  a.max_w = c->max_w;
  a.dbg = c->dbg;
  a.diag_only = c->diag_only;
  return a;
}

static int check_common(const char *fn, ffcv_jpeg_ctx *c, const uint8_t *base, const ffcv_sample *samples,
                        int batch, const void *out, const int32_t *status) {
  if (!c || !base || !samples || !out || !status || batch < 0) {
    ffcv::set_error("%s: invalid arguments", fn);
    return FFCV_EINVAL;
  }
  if (batch > c->max_batch) {
    ffcv::set_error("%s: batch %d exceeds ctx max_batch %d", fn, batch, c->max_batch);
    return FFCV_EINVAL;
  }
  return FFCV_OK;
}

// The bump counter must be 0 when K1 starts.  K2 zeroes it (its first
// workgroup, after K1 has finished on the stream), so a launch that follows
// one with K2 needs no memset: a memset is a kernel, and queued behind another
// stream's K1 it held this stream's K1 back by ~0.7 ms (rocprofv3 trace).
static int arena_before_k1(ffcv_jpeg_ctx *c, JpegArgs &a, hipStream_t s) {
  if (!c->arena_zero) FFCV_HIP_CHECK(hipMemsetAsync(a.arena_top, 0, sizeof(unsigned long long), s));
  c->arena_zero = false;
  return FFCV_OK;
}

static int launch_rrc(ffcv_jpeg_ctx *c, JpegArgs &a, hipStream_t s, const ffcv_rrc_params *p, void *out) {
  const int batch = a.batch;
  a.p = *p;
  a.out = out;
  const bool fp16 = p->lut != nullptr;
  uint64_t dense = (uint64_t)p->out_h * p->out_w * 3 * (fp16 ? 2 : 1);
  a.out_stride = p->out_stride ? p->out_stride : dense;
  const int only = a.diag_only;
  // K2's band records: ceil(out_h / BAND) per image.  The buffer holds
  // K2_REC_BANDS per image (out_h <= 256); a taller output grows it once, a
  // cold path that synchronises the device (include/ffcv_hip.h says so) and
  // fails under stream capture, where hipMalloc is refused, before anything
  // is freed.  Records do not outlive their launch (K1b rewrites them), so
  // nothing is copied over; earlier launches on any stream may still read
  // the old buffer, and hipFree returns only after they have finished.  This
  // launch's kernels are enqueued after the swap and only see the new one.
  const int nb = (p->out_h + BAND - 1) / BAND;
  if (nb > c->brec_cap) {
    K2BandRec *nbuf = nullptr;
    FFCV_HIP_CHECK(hipMalloc(&nbuf, sizeof(K2BandRec) * (size_t)nb * c->max_batch));
    (void)hipFree(c->brec);
    c->brec = nbuf;
    c->brec_cap = nb;
  }
  a.brec = c->brec;
  a.brec_bands = nb;
  if (only & 1) {
    if (int rc = arena_before_k1(c, a, s)) return rc;
  }
  // per-kernel timing: events around each kernel on this stream
  hipEvent_t *ev = c->tev_n < c->tev_cap ? c->tev + 4 * c->tev_n++ : nullptr;
  if (ev) FFCV_HIP_CHECK(hipEventRecord(ev[0], s));
  if (only & 1) {
    if (c->k1_sorted && batch > JW) {
      hipLaunchKernelGGL(k1_order_kernel, dim3(1), dim3(K1O_T), 0, s, a, c->k1_order);
      FFCV_LAUNCH_CHECK("k1_order_kernel");
      a.k1_order = c->k1_order;
    }
    hipLaunchKernelGGL((jpeg_entropy_kernel<JM_RRC>), dim3((batch + JW - 1) / JW), dim3(JW * JT), 0,
                       s, a);
    a.k1_order = nullptr;
    FFCV_LAUNCH_CHECK("jpeg_entropy_kernel<RRC>");
  }
  if (ev) FFCV_HIP_CHECK(hipEventRecord(ev[1], s));
  if (only & 2) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(batch), dim3(K1B_T), 0, s, a);
    FFCV_LAUNCH_CHECK("jpeg_idct_kernel");
  }
  if ((only & 4) && !(only & 2)) {  // diagnostics: K2 without K1b (see k2_rec_kernel)
    hipLaunchKernelGGL(k2_rec_kernel, dim3((unsigned)(((uint64_t)batch * nb + 255) / 256)), dim3(256), 0, s, a);
    FFCV_LAUNCH_CHECK("k2_rec_kernel");
  }
  if (ev) FFCV_HIP_CHECK(hipEventRecord(ev[2], s));
  dim3 g2(nb, batch);
  if (!(only & 4)) {
  } else if (fp16)
    hipLaunchKernelGGL((jpeg_color_resize_kernel<JM_RRC, true>), g2, dim3(K2T), K2_LDS, s, a);
  else
    hipLaunchKernelGGL((jpeg_color_resize_kernel<JM_RRC, false>), g2, dim3(K2T), K2_LDS, s, a);
  FFCV_LAUNCH_CHECK("jpeg_color_resize_kernel<RRC>");
  if (ev) FFCV_HIP_CHECK(hipEventRecord(ev[3], s));
  if (only & 4) c->arena_zero = true;
  return FFCV_OK;
}

int ffcv_jpeg_rrc_batch(ffcv_jpeg_ctx *c, void *stream, const uint8_t *base, const ffcv_sample *samples,
                        int batch, const int32_t *crops, const int32_t *cutout_yx, const uint8_t *flips,
                        const ffcv_rrc_params *p, void *out, int32_t *status) {
  int rc = check_common("ffcv_jpeg_rrc_batch", c, base, samples, batch, out, status);
  if (rc) return rc;
  if (!p || !crops || p->out_h <= 0 || p->out_w <= 0) {
    ffcv::set_error("ffcv_jpeg_rrc_batch: invalid params");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  JpegArgs a = make_args(c, base, samples, batch, status);
  a.crops = crops;
  a.cut = cutout_yx;
  a.flips = flips;
  return launch_rrc(c, a, ffcv::as_stream(stream), p, out);
}

int ffcv_jpeg_rrc_fused(ffcv_jpeg_ctx *c, void *stream, const uint8_t *base, const ffcv_sample *table,
                        uint64_t n_table, const uint64_t *ids, int batch, const ffcv_draw_params *dp,
                        int32_t *crops, int32_t *cutout_yx, uint8_t *flips, ffcv_sample *samples_out,
                        const ffcv_rrc_params *p, void *out, int32_t *status) {
  if (!c || !base || !table || !ids || !dp || !crops || !out || !status || batch < 0 || !p || p->out_h <= 0 ||
      p->out_w <= 0) {
    ffcv::set_error("ffcv_jpeg_rrc_fused: invalid arguments");
    return FFCV_EINVAL;
  }
  if (batch > c->max_batch) {
    ffcv::set_error("ffcv_jpeg_rrc_fused: batch %d exceeds ctx max_batch %d", batch, c->max_batch);
    return FFCV_EINVAL;
  }
  if (dp->out_h != p->out_h || dp->out_w != p->out_w || (cutout_yx && dp->cutout_size != p->cutout_size)) {
    ffcv::set_error("ffcv_jpeg_rrc_fused: draw and resize parameters disagree");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  JpegArgs a = make_args(c, base, nullptr, batch, status);
  a.table = table;
  a.n_table = n_table;
  a.ids = ids;
  a.samples_out = samples_out;
  a.dp = *dp;
  a.do_draw = 1;
  a.crops = a.crops_w = crops;
  a.cut = a.cut_w = cutout_yx;
  a.flips = a.flips_w = flips;
  return launch_rrc(c, a, ffcv::as_stream(stream), p, out);
}

int ffcv_jpeg_decode_batch(ffcv_jpeg_ctx *c, void *stream, const uint8_t *base, const ffcv_sample *samples,
                           int batch, uint8_t *out, uint64_t out_stride, int32_t *status) {
  int rc = check_common("ffcv_jpeg_decode_batch", c, base, samples, batch, out, status);
  if (rc) return rc;
  if (!out_stride) {
    ffcv::set_error("ffcv_jpeg_decode_batch: out_stride must be > 0");
    return FFCV_EINVAL;
  }
  if (batch == 0) return FFCV_OK;
  JpegArgs a = make_args(c, base, samples, batch, status);
  a.out = out;
  a.out_stride = out_stride;
  hipStream_t s = ffcv::as_stream(stream);
  if (int rc = arena_before_k1(c, a, s)) return rc;
  hipLaunchKernelGGL((jpeg_entropy_kernel<JM_FULL>), dim3((batch + JW - 1) / JW), dim3(JW * JT), 0, s, a);
  FFCV_LAUNCH_CHECK("jpeg_entropy_kernel<FULL>");
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(batch), dim3(K1B_T), 0, s, a);
  FFCV_LAUNCH_CHECK("jpeg_idct_kernel");
  dim3 g2((c->max_h + BAND - 1) / BAND, batch);
  hipLaunchKernelGGL((jpeg_color_resize_kernel<JM_FULL, false>), g2, dim3(K2T), 0, s, a);
  FFCV_LAUNCH_CHECK("jpeg_color_resize_kernel<FULL>");
  c->arena_zero = true;
  return FFCV_OK;
}

int ffcv_jpeg_coefficients_batch(ffcv_jpeg_ctx *c, void *stream, const uint8_t *base,
                                 const ffcv_sample *samples, int batch, int16_t *coefs, uint64_t max_blocks,
                                 int32_t *status) {
  int rc = check_common("ffcv_jpeg_coefficients_batch", c, base, samples, batch, coefs, status);
  if (rc) return rc;
  if (batch == 0) return FFCV_OK;
  JpegArgs a = make_args(c, base, samples, batch, status);
  a.out = coefs;
  a.out_stride = max_blocks * 64 * 2;
  a.max_blocks = max_blocks;
  if (int rc2 = arena_before_k1(c, a, ffcv::as_stream(stream))) return rc2;
  hipLaunchKernelGGL((jpeg_entropy_kernel<JM_COEF>), dim3((batch + JW - 1) / JW), dim3(JW * JT), 0,
                     ffcv::as_stream(stream), a);
  FFCV_LAUNCH_CHECK("jpeg_entropy_kernel<COEF>");
  return FFCV_OK;
}

}  // extern "C"
