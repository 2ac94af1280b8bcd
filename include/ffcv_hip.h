/*
 * ffcv_hip.h -- C ABI of libffcv_hip.so, the MI355X (gfx950) replacement for
 * the reference's native shim.
 *
 * Reference boundary being replaced:
 *   /root/reference/libffcv/libffcv.cpp   (exports resize / my_memcpy /
 *                                          my_fread / imdecode, :33-112)
 *   /root/reference/ffcv/libffcv.py       (ctypes binding, :8-55)
 * The reference binds ONE sample per call from numba prange workers.  This
 * ABI is batch- and device-first: every compute entry point takes a device
 * base pointer to the .beton bytes resident in HBM, a device array of
 * per-sample descriptors, and a hipStream_t (passed as void*) on which all
 * work is enqueued asynchronously.  No torch types, no hidden hipMalloc in a
 * launch, no host synchronisation in a launch (graph-capturable).
 *
 * Ownership: the caller owns every input/output buffer.  The library owns
 * only the scratch inside an ffcv_jpeg_ctx (allocated once at create time).
 *
 * Errors: every function returns an int status (FFCV_OK == 0).  On failure a
 * thread-local message is available from ffcv_last_error().  Per-sample
 * decode failures (corrupt / unsupported JPEG) are reported in a device
 * int32 status array and the sample's output is zero-filled; the reference
 * ignores imdecode's return code (rgb_image.py:131,196) and yields garbage.
 */
#ifndef FFCV_HIP_H
#define FFCV_HIP_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFCV_HIP_ABI_VERSION 1

enum {
  FFCV_OK = 0,
  FFCV_EINVAL = -1,      /* bad argument */
  FFCV_EHIP = -2,        /* HIP runtime error */
  FFCV_ENOMEM = -3,      /* allocation failed */
  FFCV_EUNSUPPORTED = -4 /* feature not on this path */
};

/* Per-sample status codes written by the device (int32). */
enum {
  FFCV_SAMPLE_OK = 0,
  FFCV_SAMPLE_BAD_MARKER = 1,      /* not a JPEG / truncated header */
  FFCV_SAMPLE_UNSUPPORTED = 2,     /* progressive, arithmetic, 12-bit, DRI, CMYK */
  FFCV_SAMPLE_TOO_LARGE = 3,       /* exceeds the ctx's max size or scratch arena */
  FFCV_SAMPLE_CORRUPT = 4,         /* entropy stream inconsistent, or ends before its last block */
  FFCV_SAMPLE_GEOMETRY = 5,        /* SOF size != .beton metadata */
  FFCV_SAMPLE_RNG = 6,             /* > 623 MT19937 draws for one stream */
  FFCV_SAMPLE_LABEL = 7,           /* MixupToOneHot: label outside [0, num_classes) */
  FFCV_SAMPLE_RANGE = 8            /* ffcv_gather_rows: id outside the table, or row outside the bytes */
};

/* One sample of a batch, as resolved from the .beton metadata + allocation
 * table (rgb_image.py:302-308 metadata; memory_managers/os_cache.py:55-60
 * read).  32 bytes, device-resident array. */
typedef struct ffcv_sample {
  uint64_t offset; /* byte offset of the sample's data from the base pointer */
  uint64_t size;   /* byte count (allocation table 'size') */
  uint32_t height; /* metadata 'height' */
  uint32_t width;  /* metadata 'width' */
  uint32_t mode;   /* 0 = jpg, 1 = raw (rgb_image.py:21-23) */
  uint32_t reserved;
} ffcv_sample;

/* Parameters of a fused decode -> crop -> resize -> cutout -> normalize
 * launch (rgb_image.py:168-212, cutout.py:31-52, normalize.py:58-87). */
typedef struct ffcv_rrc_params {
  int32_t out_h, out_w;    /* output_size (rgb_image.py:145-149) */
  int32_t cutout_size;     /* 0: no cutout; else crop_size (cutout.py:26) */
  uint8_t cutout_fill[4];  /* fill RGB (cutout.py:29); [3] = 1 when the
                              pipeline runs Cutout BEFORE RandomHorizontalFlip
                              (0: flip first, then cutout) */
  const uint16_t *lut;     /* device [256][3] fp16 bits (normalize.py:42-49), or
                              NULL for uint8 output */
  uint64_t out_stride;     /* bytes between samples in the output; 0 = dense */
} ffcv_rrc_params;

/* Crop-draw parameters (rgb_image.py:48-81) + seeding contract
 * (DESIGN.md "RNG contract": one MT19937 per (op, sample, epoch) seeded
 * with low32(splitmix64 chain of loader_seed, epoch, sample index, op id)). */
typedef struct ffcv_draw_params {
  int32_t crop_kind;       /* 0 = get_random_crop, 1 = get_center_crop */
  int32_t out_h, out_w;    /* needed for cutout bounds */
  int32_t cutout_size;     /* 0 = no cutout draw */
  double scale[2];         /* RandomResizedCrop scale (rgb_image.py:234) */
  double ratio[2];         /* RandomResizedCrop ratio */
  double center_ratio;     /* CenterCrop ratio (rgb_image.py:259) */
  uint64_t loader_seed;
  uint64_t epoch;
  double flip_prob;        /* RandomHorizontalFlip probability (flip.py:33) */
} ffcv_draw_params;

/* ---------------------------------------------------------------- misc -- */
int ffcv_abi_version(void);
const char *ffcv_last_error(void);
int ffcv_device_count(int *count);
int ffcv_set_device(int device);
int ffcv_stream_synchronize(void *stream);

/* Device memory helpers (for callers without torch; the Python package uses
 * torch allocations instead). */
int ffcv_malloc(void **dptr, uint64_t bytes);
int ffcv_free(void *dptr);
int ffcv_memcpy_h2d_async(void *dst, const void *src, uint64_t bytes, void *stream);
int ffcv_memcpy_d2h_async(void *dst, const void *src, uint64_t bytes, void *stream);

/* libffcv.cpp:44-46 my_memcpy (host plumbing; SimpleRGBImageDecoder raw on a
 * CPU-only Loader, C1).  Same argument order as the reference. */
void my_memcpy(void *source, void *dst, uint64_t size);

/* libffcv.cpp:48-51 my_fread: fseek((FILE *)fp, offset, SEEK_SET) then
 * fread(destination, 1, size, fp) (host plumbing; exported by the reference,
 * never bound by its Python).  Same arguments; like the reference it returns
 * nothing, and a short read leaves the rest of destination untouched. */
void my_fread(int64_t fp, int64_t offset, void *destination, int64_t size);

/* libffcv.cpp:33-42 resize: cv::resize(src[start_row:end_row,
 * start_col:end_col], dst, (tx rows, ty cols), INTER_AREA) where src is an
 * sx x sy x 3 uint8 image and dst a tx x ty x 3 uint8 buffer, both in host
 * memory (bound as resize_crop, ffcv/libffcv.py:22-31; cresizer unused).
 * Computed on the CPU by the kernels' own INTER_AREA functions.  On an
 * invalid ROI nothing is written and ffcv_last_error() says why. */
void resize(int64_t cresizer, int64_t source_p, int64_t sx, int64_t sy,
            int64_t start_row, int64_t end_row, int64_t start_col,
            int64_t end_col, int64_t dest_p, int64_t tx, int64_t ty);

/* libffcv.cpp:53-112 imdecode (bound at ffcv/libffcv.py:34-48): decode the
 * JPEG input_buffer[input_size] to crop_height x crop_width x 3 RGB in host
 * output_buffer, tjDecompress2(TJPF_RGB, TJFLAG_FASTDCT) semantics (ifast
 * IDCT, fancy upsampling), on the CPU of the calling thread like the
 * reference (ffcv_cpu_jpeg.hip; thread-safe, per-thread scratch).  Baseline
 * / extended sequential Huffman, 8-bit, 1 or 3 components, restart
 * intervals.  With enable_crop or hflip, the reference's tjTransform
 * (TJXOPT_CROP at offset_x, offset_y, crop_width x crop_height, plus
 * TJXOP_HFLIP) is applied to the coefficients first (lossless: the crop origin
 * must be on an iMCU boundary, the size is clamped to the image, the crop is
 * taken in the mirrored frame, the partial iMCU column at the right edge is
 * not mirrored).  As tjDecompress2 does, the decode runs at the largest
 * TurboJPEG scaling factor whose output fits the requested size (scaled by
 * scale_num / scale_denom), rows packed at the decoded width; the factors
 * 1/1, 1/2, 1/4 and 1/8 are restated (libjpeg's reduced IDCTs, bit-exact
 * with libjpeg-turbo).  Returns 0, or -1 on a decode error, an unsupported
 * stream (progressive, arithmetic, multi-scan, CMYK), a misaligned crop, or
 * a request TurboJPEG would decode at another factor -- see
 * ffcv_last_error().  ffcv itself passes the image's size, 0, 0, 1, 1,
 * False, False. */
int imdecode(unsigned char *input_buffer, uint64_t input_size,
             uint32_t source_height, uint32_t source_width,
             unsigned char *output_buffer, uint32_t crop_height,
             uint32_t crop_width, uint32_t offset_x, uint32_t offset_y,
             uint32_t scale_num, uint32_t scale_denom, bool enable_crop,
             bool hflip);

/* The reference's per-sample CPU decode loop (rgb_image.py:123-136 Simple,
 * :185-210 ResizedCrop, under numba prange) as one call over nthreads host
 * threads: sample k (data[k], sizes[k] bytes, heights[k] x widths[k], modes[k]
 * 0 = jpg through imdecode, 1 = raw, other = skipped) is written whole at
 * out + k * out_stride, or, with crops (batch x 4: i, j, h, w), cut and resized
 * by resize() to out_h x out_w there.  status[k] = 0, or -1 when its decode
 * failed.  Returns FFCV_OK or FFCV_EINVAL. */
int ffcv_cpu_decode_batch(const uint8_t *const *data, const uint64_t *sizes,
                          const uint32_t *heights, const uint32_t *widths,
                          const uint32_t *modes, int batch, const int32_t *crops,
                          int out_h, int out_w, uint8_t *out, uint64_t out_stride,
                          int nthreads, int32_t *status);

/* Measurement helper (new; no reference counterpart): per image k of n,
 * stats[3k] = Huffman symbols of its scan (DC + AC, EOB / ZRL included),
 * stats[3k+1] = blocks, stats[3k+2] = entropy-coded bytes (host decode by the
 * CPU decoder's Huffman loop).  bench.py's K1 lane-instructions per symbol.
 * Returns FFCV_OK, -1 when an image does not parse (its stats are 0), or
 * FFCV_EINVAL. */
int ffcv_jpeg_scan_stats(const uint8_t *const *data, const uint64_t *sizes, int n, uint64_t *stats);

/* imdecode's signature and semantics, executed by the gfx950 JPEG kernels
 * (per-thread stream and decoder context; host buffers in and out). */
int ffcv_imdecode_device(unsigned char *input_buffer, uint64_t input_size,
                         uint32_t source_height, uint32_t source_width,
                         unsigned char *output_buffer, uint32_t crop_height,
                         uint32_t crop_width, uint32_t offset_x,
                         uint32_t offset_y, uint32_t scale_num,
                         uint32_t scale_denom, bool enable_crop, bool hflip);

/* Host gather of n byte ranges src + src_off[i] (sizes[i] bytes) to
 * dst + dst_off[i], split over nthreads threads by bytes: the PCIe path's
 * per-batch staging of compressed samples from the mmap'd .beton
 * (memory_managers/os_cache.py:55-60 read, batched). */
int ffcv_host_gather(const uint8_t *src, const uint64_t *src_off, const uint64_t *sizes,
                     const uint64_t *dst_off, int n, uint8_t *dst, int nthreads);

/* ------------------------------------------------------- random draws -- */
/* rgb_image.py:48-81 crop windows (+ cutout.py:38-42 origins, + flip.py:35
 * decisions) for B samples, on the device.
 *   sample_ids : device uint64[B] dataset indices (batch_indices)
 *   samples    : device ffcv_sample[B] (height/width used; may be NULL when
 *                crops is NULL)
 *   crops      : device int32[B][4] (i, j, h, w) out
 *   cutout_yx  : device int32[B][2] out, or NULL
 *   flips      : device uint8[B] out, or NULL
 *   status     : device int32[B] out, or NULL */
int ffcv_draw_batch(void *stream, const uint64_t *sample_ids,
                    const ffcv_sample *samples, int batch,
                    const ffcv_draw_params *p, int32_t *crops,
                    int32_t *cutout_yx, uint8_t *flips, int32_t *status);

/* The same draws on the host (the CPU-device Loader's decoders): heights /
 * widths / sample_ids are host arrays, outputs host arrays. */
int ffcv_draw_batch_host(const uint64_t *sample_ids, const uint32_t *heights,
                         const uint32_t *widths, int batch,
                         const ffcv_draw_params *p, int32_t *crops,
                         int32_t *cutout_yx, uint8_t *flips);

/* ------------------------------------------- raw-mode crop + resize ---- */
/* rgb_image.py:202-208 (raw branch) + libffcv.cpp:33-42 cv::resize
 * INTER_AREA, fused with Cutout (cutout.py:44) and the NormalizeImage LUT
 * (normalize.py:65).  Samples with mode != raw are skipped.
 *   base  : device pointer to the .beton bytes (file offset 0)
 *   out   : device [B][out_h][out_w][3] uint8 (lut==NULL) or fp16 bits */
int ffcv_rrc_raw_batch(void *stream, const uint8_t *base,
                       const ffcv_sample *samples, int batch,
                       const int32_t *crops, const int32_t *cutout_yx,
                       const uint8_t *flips, const ffcv_rrc_params *p,
                       void *out);

/* The same with a caller-provided device workspace (16-byte aligned, at
 * least ffcv_rrc_raw_workspace_bytes(batch, out_h, out_w) bytes; NULL runs
 * ffcv_rrc_raw_batch): each image's resize plan and its linear tap table
 * (or, for INTER_AREA crops at scales < 2, its column records) are computed
 * once (one small kernel, one thread per tap) instead of in every band
 * workgroup of the image.  Output is identical.  The workspace is
 * overwritten by the launch and must not be shared by launches in flight
 * on different streams. */
int ffcv_rrc_raw_batch_ws(void *stream, const uint8_t *base,
                          const ffcv_sample *samples, int batch,
                          const int32_t *crops, const int32_t *cutout_yx,
                          const uint8_t *flips, const ffcv_rrc_params *p,
                          void *out, void *workspace, uint64_t workspace_bytes);
uint64_t ffcv_rrc_raw_workspace_bytes(int batch, int out_h, int out_w);

/* Per-batch descriptor gather: out[k] = table[ids[k]] (the reference reads
 * metadata[source_ix] per sample, rgb_image.py:188-189).  table: device
 * ffcv_sample[N] built once per dataset; ids: device uint64[B]. */
int ffcv_gather_samples(void *stream, const ffcv_sample *table, uint64_t n_table,
                        const uint64_t *ids, int batch, ffcv_sample *out);

/* rgb_image.py:123-136 SimpleRGBImageDecoder raw branch (my_memcpy per
 * sample) as a device gather into [B][H][W][3]: row k of `out` receives the
 * `size` bytes of a mode-1 (raw) sample; the rest of the row, and the row of
 * a sample of another mode, are not written.  Any batch >= 0 (more than
 * 65,535 samples go out as several launches). */
int ffcv_gather_raw_batch(void *stream, const uint8_t *base,
                          const ffcv_sample *samples, int batch, uint8_t *out,
                          uint64_t out_stride);

/* ndarray.py:19-45 NDArrayDecoder (one my_memcpy per sample) as ONE device
 * gather of fixed-size rows out of the resident .beton bytes, the id -> offset
 * lookup inside the kernel (no descriptor gather in front):
 *
 *   out[k * out_stride : + row_bytes] = base[row_off[ids[k]] : + row_bytes]
 *
 * bit for bit, for k in [0, batch).
 *   base       : device bytes, 16-byte aligned; base_bytes of them are valid.
 *                The ALLOCATION must extend to the next multiple of 16 past
 *                base_bytes: rows may start at any byte offset and are read
 *                with aligned dword loads, so the aligned dword that holds a
 *                row's last byte is read whole (nothing further is: only
 *                aligned 16-byte words holding at least one byte of a valid
 *                row are touched).  The 64 bytes of padding behind the
 *                HBM-resident file and the staging buffers satisfy this.
 *   row_off    : device uint64[n_rows], byte offset of every sample's row
 *   ids        : device uint64[batch] sample indices
 *   out        : device bytes, any alignment; out_stride >= row_bytes, and
 *                only the row_bytes bytes of each output row are written
 *   status     : device int32[batch] out, required
 * A row with ids[k] >= n_rows, or whose bytes do not lie inside
 * [0, base_bytes) (checked without wrap-around), is not read: its output row
 * is zero-filled and status[k] = FFCV_SAMPLE_RANGE; every other status[k] is
 * FFCV_SAMPLE_OK.  Rows shorter than ffcv_gather_rows_cutover() bytes take a
 * wave (up to ffcv_gather_rows_subwave() bytes: 16 lanes) each, several rows
 * per workgroup; longer rows a 2-D grid of 16 KiB chunks by rows.
 * batch == 0 returns FFCV_OK without a launch.  FFCV_EINVAL, before any
 * launch, for a null pointer, batch < 0, row_bytes == 0, out_stride <
 * row_bytes or a base that is not 16-byte aligned. */
int ffcv_gather_rows(void *stream, const uint8_t *base, uint64_t base_bytes,
                     const uint64_t *row_off, uint64_t n_rows,
                     const uint64_t *ids, int batch, uint64_t row_bytes,
                     uint8_t *out, uint64_t out_stride, int32_t *status);
uint64_t ffcv_gather_rows_cutover(void);
uint64_t ffcv_gather_rows_subwave(void);

/* ------------------------------------------------------- JPEG decode -- */
/* Baseline-sequential Huffman JPEG, 8-bit, 1 or 3 components, any 1x/2x
 * sampling, bit-exact with libjpeg-turbo tjDecompress2(TJPF_RGB,
 * TJFLAG_FASTDCT) (libffcv.cpp:104-106): ifast IDCT, fancy upsampling,
 * fixed-point YCbCr->RGB.  One context holds the scratch for up to
 * max_batch images of at most max_height x max_width pixels and max_bytes
 * compressed bytes each. */
typedef struct ffcv_jpeg_ctx ffcv_jpeg_ctx;
int ffcv_jpeg_create(ffcv_jpeg_ctx **ctx, int max_batch, uint32_t max_height,
                     uint32_t max_width, uint64_t max_bytes);
/* Scratch is one arena per context, bump-allocated per image by the entropy
 * kernel from the image's own size and crop window (not dataset-max x
 * batch).  ffcv_jpeg_create sizes it for max_batch images of the maximum
 * size; ffcv_jpeg_create_arena takes the size from the caller, e.g. the sum
 * of ffcv_jpeg_scratch_bound over the largest max_batch images of a dataset
 * (a launch can then never exhaust it).  An image that does not fit in what
 * is left of the arena gets FFCV_SAMPLE_TOO_LARGE. */
int ffcv_jpeg_create_arena(ffcv_jpeg_ctx **ctx, int max_batch,
                           uint32_t max_height, uint32_t max_width,
                           uint64_t max_bytes, uint64_t arena_bytes);
/* Upper bound of the arena bytes one image of this size (and compressed
 * size) can take, for any crop (host function, no device access). */
uint64_t ffcv_jpeg_scratch_bound(uint32_t height, uint32_t width,
                                 uint64_t nbytes);
int ffcv_jpeg_destroy(ffcv_jpeg_ctx *ctx);

/* Arena bytes the last entropy launch on `stream` bump-allocated (waits for
 * the stream), and the arena's capacity (may be NULL): the high-water mark
 * for sizing arenas. */
int ffcv_jpeg_arena_used(ffcv_jpeg_ctx *ctx, void *stream, uint64_t *used,
                         uint64_t *capacity);

/* rgb_image.py:185-210 jpg branch fused end to end: decode only the MCUs the
 * crop needs -> crop -> INTER_AREA -> cutout -> LUT.  Samples with mode !=
 * jpg are skipped (call ffcv_rrc_raw_batch for them).  status: device
 * int32[B] (FFCV_SAMPLE_*), required.
 * A context is created with per-band scratch for outputs of up to 256 rows.
 * The first launch on it (this call or ffcv_jpeg_rrc_fused) whose out_h is
 * larger re-allocates that scratch for the new height: that one call
 * synchronises the whole device (hipMalloc + hipFree) and must not be made
 * under stream capture; it fails with the HIP error there.  Launch once at
 * the largest out_h before capturing or before timing. */
int ffcv_jpeg_rrc_batch(ffcv_jpeg_ctx *ctx, void *stream, const uint8_t *base,
                        const ffcv_sample *samples, int batch,
                        const int32_t *crops, const int32_t *cutout_yx,
                        const uint8_t *flips, const ffcv_rrc_params *p,
                        void *out, int32_t *status);

/* ffcv_gather_samples + ffcv_draw_batch + ffcv_jpeg_rrc_batch in one launch
 * sequence: the entropy kernel reads sample ids[k] of table[n_table] and
 * draws its crop / cutout origin / flip under the seeding contract itself
 * (two fewer small kernels on the slot's stream).  crops (int32[B,4]) is
 * required; cutout_yx (int32[B,2]) and flips (uint8[B]) may be NULL; all
 * three are written for the caller, like ffcv_draw_batch.  samples_out
 * (ffcv_sample[B], may be NULL) receives the gathered descriptors, e.g. for
 * ffcv_rrc_raw_batch on the raw samples of a mixed field.  An RNG overrun
 * sets that sample's status to FFCV_SAMPLE_RNG. */
int ffcv_jpeg_rrc_fused(ffcv_jpeg_ctx *ctx, void *stream, const uint8_t *base,
                        const ffcv_sample *table, uint64_t n_table,
                        const uint64_t *ids, int batch, const ffcv_draw_params *dp,
                        int32_t *crops, int32_t *cutout_yx, uint8_t *flips,
                        ffcv_sample *samples_out, const ffcv_rrc_params *p,
                        void *out, int32_t *status);

/* Entropy index: index[n_samples][64][3] uint32, zero-initialised and owned
 * by the caller (768 B per dataset sample).  With it attached, a
 * ffcv_jpeg_rrc_fused decode of dataset sample ids[k] that finds no record
 * runs the self-synchronising Huffman sync and publishes the converged start
 * state of each lane range; a later decode of the same sample (the next
 * epoch) reads it and skips the sync rounds.  Output is bit-identical either
 * way.  NULL detaches.  Records are written and read with plain memory
 * operations and carry a 64-bit hash of their words, so a launch on another
 * stream that reads a record while it is being published sees a torn record
 * fail the hash and decodes that sample in full. */
int ffcv_jpeg_set_entropy_index(ffcv_jpeg_ctx *ctx, uint32_t *index,
                                uint64_t n_samples);

/* Measurement (no reference counterpart; bench.py's per-kernel roofline):
 * with max_launches > 0 the next max_launches RRC launches on this context
 * record HIP events on their own stream before the entropy kernel, after
 * it, after the IDCT kernel and after the colour/resize kernel; 0 turns it
 * off.  ffcv_jpeg_timing_read waits for the recorded launches and writes
 * ms[3*i + {0,1,2}] = the three kernels' durations of launch i (in launch
 * order, at most max_launches), then starts a new recording. */
int ffcv_jpeg_set_timing(ffcv_jpeg_ctx *ctx, int max_launches);
int ffcv_jpeg_timing_read(ffcv_jpeg_ctx *ctx, float *ms, int max_launches,
                          int *n_launches);

/* rgb_image.py:123-136 SimpleRGBImageDecoder jpg branch (imdecode into the
 * destination, full image) -> device [B][H][W][3] with out_stride bytes per
 * sample. */
int ffcv_jpeg_decode_batch(ffcv_jpeg_ctx *ctx, void *stream,
                           const uint8_t *base, const ffcv_sample *samples,
                           int batch, uint8_t *out, uint64_t out_stride,
                           int32_t *status);

/* Test hook: quantised coefficients (DC predicted, natural order) of every
 * block in MCU order, [B][max_blocks][64] int16, for checking the entropy
 * stage against the oracle on its own. */
int ffcv_jpeg_coefficients_batch(ffcv_jpeg_ctx *ctx, void *stream,
                                 const uint8_t *base,
                                 const ffcv_sample *samples, int batch,
                                 int16_t *coefs, uint64_t max_blocks,
                                 int32_t *status);

/* ---------------------------------------------- standalone transforms -- */
/* cutout.py:36-47 in place on a device [B][H][W][3] uint8 batch.  Each
 * origin cutout_yx[k] = (y, x) must be >= 0 in both coordinates; the part of
 * the square past the bottom or right edge of the image is dropped. */
int ffcv_cutout_batch(void *stream, uint8_t *images, int batch, int height,
                      int width, const int32_t *cutout_yx, int crop_size,
                      const uint8_t fill[3]);
/* normalize.py:64-65 cupy ElementwiseKernel 'output = table[input*3 + i%3]'
 * (templated on the output type T there): out[i] = lut[in[i]*3 + i%3] over n
 * elements of a channels-last uint8 batch.  lut: device [256][3] table of
 * elem_bytes-wide elements (1, 2, 4 or 8: u8/int16/fp16/fp32/f64 ...). */
int ffcv_lut_batch(void *stream, const uint8_t *in, uint64_t n,
                   const void *lut, int elem_bytes, void *out);
/* ffcv_lut_batch with a fp16 (int16 bits) table (normalize.py:45-48). */
int ffcv_normalize_batch(void *stream, const uint8_t *in, uint64_t n,
                         const uint16_t *lut, uint16_t *out);
/* flip.py:35-40: dst[i] = images[i, :, ::-1] where flips[i] != 0, a copy
 * otherwise, for pixels of channels_bytes bytes (in == out is FFCV_EINVAL).
 * Any batch >= 0 (more than 65,535 images go out as several launches). */
int ffcv_flip_batch(void *stream, const uint8_t *in, uint8_t *out, int batch,
                    int height, int width, int channels_bytes,
                    const uint8_t *flips);

/* ------------------------------------------------- RandomTranslate ---- */
/* translate.py:35-44: the image sits at offset `padding` in a canvas of
 * `fill` sized (H + 2p, W + 2p); y = randint(0, 2p + 1) is drawn first,
 * then x, and the output is the H x W window at (y, x):
 *   out[r, c] = in[r + y - p, c + x - p] inside the image, else fill.
 * Draws under the seeding contract with op id 4 (one lane per sample):
 *   sample_ids : device uint64[B]
 *   yx         : device int32[B][2] out (y, x)
 *   status     : device int32[B] out (FFCV_SAMPLE_RNG when the sample's
 *                MT19937 stream ran out), or NULL */
int ffcv_translate_draw_batch(void *stream, const uint64_t *sample_ids,
                              int batch, uint64_t loader_seed, uint64_t epoch,
                              int padding, int32_t *yx, int32_t *status);
/* The same draws on host arrays (the CPU-device Loader). */
int ffcv_translate_draw_batch_host(const uint64_t *sample_ids, int batch,
                                   uint64_t loader_seed, uint64_t epoch,
                                   int padding, int32_t *yx);
/* Standalone translate of a device [B][H][W][3] uint8 batch into `out`
 * (same shape; in == out is FFCV_EINVAL: shifted reads overlap the writes).
 * Any batch >= 0 (more than 65,535 images go out as several launches). */
int ffcv_translate_batch(void *stream, const uint8_t *in, uint8_t *out,
                         int batch, int height, int width, const int32_t *yx,
                         int padding, const uint8_t fill[3]);

/* ------------------------------------- RandomResizedCrop transform ---- */
/* random_resized_crop.py: fast_crop.py get_random_crop on a batch of images
 * of one common height x width, then cv::resize(INTER_AREA) of each window.
 * Draws under the seeding contract with op id 8 ("crop transform"; id 1 is
 * the crop DECODER's, so a pipeline with both draws two different streams),
 * one lane per sample:
 *   sample_ids : device uint64[B]
 *   scale, ratio : host double[2] each (finite, scale >= 0, ratio > 0)
 *   crops      : device int32[B][4] out (i, j, h, w)
 *   status     : device int32[B] out (FFCV_SAMPLE_RNG when the sample's
 *                MT19937 stream ran out), or NULL */
int ffcv_crop_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                         int height, int width, const double scale[2],
                         const double ratio[2], uint64_t loader_seed,
                         uint64_t epoch, int32_t *crops, int32_t *status);
/* The same draws on host arrays (the CPU-device Loader). */
int ffcv_crop_draw_batch_host(const uint64_t *sample_ids, int batch,
                              int height, int width, const double scale[2],
                              const double ratio[2], uint64_t loader_seed,
                              uint64_t epoch, int32_t *crops, int32_t *status);

/* Image k of `out` = cv::resize(in_k[i:i+h, j:j+w], (out_h, out_w),
 * INTER_AREA) with crops[k] = (i, j, h, w), then the epilogue of
 * ffcv_rrc_raw_batch, bit for bit: flip where flips[k], cutout at
 * cutout_yx[k] (p->cutout_size, p->cutout_fill, [3] = cutout before flip),
 * the fp16 LUT when p->lut is set; p->out_stride bytes between output images
 * (0 = dense), only each image's own bytes are written.
 *   in    : device uint8, image k at in + k * in_stride, height x width x 3
 *           with dense rows, at ANY byte alignment.  Rows are read with
 *           aligned 16-byte loads: only aligned 16-byte words that hold at
 *           least one byte of a crop row are touched, so the allocation must
 *           extend to the 16-byte boundaries around
 *           [in, in + batch * in_stride) (the rule of ffcv_gather_rows).
 *   crops : device int32[B][4], validated on the device: with h <= 0, w <= 0,
 *           i < 0, j < 0, i + h > height or j + w > width the image is not
 *           read, its output is zero-filled and status[k] =
 *           FFCV_SAMPLE_RANGE; every other status[k] is FFCV_SAMPLE_OK.
 *   cutout_yx, flips, status : device, each may be NULL
 *   out   : device, must not overlap `in`
 * Two regimes, chosen from height and width: while the staged source
 * (height rows of whole 16-byte chunks) is at most
 * ffcv_rrc_images_lds_bytes(), ONE launch, a workgroup per image that stages
 * the crop in LDS, builds its taps there and writes the final pixels (no
 * workspace; an output so large that its out_h + out_w taps do not fit the
 * workgroup's LDS beside the source takes the other regime).  Larger images
 * run the band kernel of ffcv_rrc_raw_batch_ws behind a small descriptor
 * kernel and need a 16-byte aligned workspace of
 * ffcv_rrc_images_workspace_bytes() (0 in the LDS regime), overwritten by the
 * launch.  batch == 0 returns FFCV_OK without a launch.  FFCV_EINVAL, before
 * any launch, for a null in / crops / p / out, batch < 0, sizes <= 0,
 * in_stride < height * width * 3, an out_stride smaller than an image, a
 * cutout larger than the output, overlapping in and out, or a workspace
 * that is too small or misaligned. */
int ffcv_rrc_images_batch(void *stream, const uint8_t *in, uint64_t in_stride,
                          int batch, int height, int width,
                          const int32_t *crops, const int32_t *cutout_yx,
                          const uint8_t *flips, const ffcv_rrc_params *p,
                          void *out, int32_t *status, void *workspace,
                          uint64_t workspace_bytes);
uint64_t ffcv_rrc_images_workspace_bytes(int batch, int height, int width,
                                         int out_h, int out_w);
uint64_t ffcv_rrc_images_lds_bytes(void);
/* The resize on host memory: resize() per image over nthreads threads, the
 * same crop validation (status may be NULL), no epilogue (the host Cutout /
 * flip / NormalizeImage are separate operations).  out_stride 0 = dense. */
int ffcv_rrc_images_batch_host(const uint8_t *in, uint64_t in_stride,
                               int batch, int height, int width,
                               const int32_t *crops, int out_h, int out_w,
                               uint8_t *out, uint64_t out_stride,
                               int32_t *status, int nthreads);

/* ------------------------------- fused small-image augmentation ------- */
/* Geometric steps of ffcv_simple_aug_batch's program. */
enum {
  FFCV_AUG_FLIP = 1,      /* flip.py:35-40, decided by flips[k] */
  FFCV_AUG_TRANSLATE = 2, /* translate.py:35-44, window translate_yx[k] */
  FFCV_AUG_CUTOUT = 3     /* cutout.py:36-47, square at cutout_yx[k] */
};

typedef struct ffcv_simple_aug_params {
  int32_t n_steps;           /* 1..3 */
  uint8_t steps[4];          /* FFCV_AUG_* in pipeline order, each at most once */
  int32_t padding;           /* RandomTranslate padding */
  int32_t cutout_size;       /* Cutout crop_size */
  uint8_t translate_fill[4]; /* RGB ([3] unused) */
  uint8_t cutout_fill[4];    /* RGB ([3] unused) */
} ffcv_simple_aug_params;

/* SimpleRGBImageDecoder raw branch (rgb_image.py:123-136) fused with
 * RandomHorizontalFlip / RandomTranslate / Cutout in any order and the
 * NormalizeImage LUT (normalize.py:65): one read of each raw sample, one
 * write of the final pixels.  Every sample is height x width x 3 raw bytes
 * at base + samples[k].offset (any byte alignment); samples of another mode
 * or with fewer bytes are skipped.  Each output pixel walks the program
 * backwards to the source pixel it shows (or to a fill colour), so every
 * ordering of the steps gives what the separate operations give.
 *   flips        : device uint8[B]      (required by a FLIP step, else NULL)
 *   cutout_yx    : device int32[B][2]   (required by a CUTOUT step)
 *   translate_yx : device int32[B][2]   (required by a TRANSLATE step)
 *   lut          : device [256][3] fp16 bits, or NULL for uint8 output
 *   out          : device [B][height][width][3] uint8 or fp16 bits,
 *                  out_stride bytes per sample (0 = dense) */
int ffcv_simple_aug_batch(void *stream, const uint8_t *base,
                          const ffcv_sample *samples, int batch, int height,
                          int width, const ffcv_simple_aug_params *p,
                          const uint8_t *flips, const int32_t *cutout_yx,
                          const int32_t *translate_yx, const uint16_t *lut,
                          void *out, uint64_t out_stride);

/* ------------------------------------------------- colour jitter ------ */
/* color_jitter.py: RandomBrightness / RandomContrast / RandomSaturation on
 * uint8 HWC RGB images.  All arithmetic is float64, every multiply and add
 * rounded on its own (never fused):
 *   gray(r, g, b) = uint8(trunc((0.2989 r + 0.587 g) + 0.114 b))
 *   blend(v, o)   = uint8(trunc(clip(ratio v + (1 - ratio) o, 0, 255)))
 *   brightness: o = 0;  contrast: o = (sum of gray over the image) / (H W),
 *   the same for the three channels;  saturation: o = gray(pixel).
 * Draws under the seeding contract, one lane per sample, op_id 5 brightness,
 * 6 contrast, 7 saturation: apply = rand() < p, then ratio = uniform(max(0,
 * 1 - magnitude), 1 + magnitude); both are always drawn, in that order.
 *   sample_ids : device uint64[B]
 *   apply      : device uint8[B] out
 *   ratio      : device float64[B] out
 *   status     : device int32[B] out (FFCV_SAMPLE_RNG when the sample's
 *                MT19937 stream ran out), or NULL */
int ffcv_color_jitter_draw_batch(void *stream, const uint64_t *sample_ids,
                                 int batch, uint64_t loader_seed,
                                 uint64_t epoch, int op_id, double p,
                                 double magnitude, uint8_t *apply,
                                 double *ratio, int32_t *status);
/* The same draws on host arrays (the CPU-device Loader). */
int ffcv_color_jitter_draw_batch_host(const uint64_t *sample_ids, int batch,
                                      uint64_t loader_seed, uint64_t epoch,
                                      int op_id, double p, double magnitude,
                                      uint8_t *apply, double *ratio);

enum {
  FFCV_CJ_BRIGHTNESS = 1,
  FFCV_CJ_CONTRAST = 2,
  FFCV_CJ_SATURATION = 3,
  FFCV_CJ_GRAYSCALE = 4, /* every channel = gray(pixel): saturation at ratio 0
                            (the step's ratio is not read) */
  FFCV_CJ_SOLARIZE = 5   /* v >= threshold ? 255 - v : v per byte, the integer
                            threshold in [0, 256] passed as the step's ratio */
};

typedef struct ffcv_color_jitter_params {
  int32_t n_steps;  /* 1..3 */
  uint8_t steps[4]; /* FFCV_CJ_* in pipeline order, each at most once */
} ffcv_color_jitter_params;

/* Bytes of workspace ffcv_color_jitter_batch needs for `batch` images of any
 * size and any program (one uint64 gray sum per image; only a program with a
 * CONTRAST step on images beyond the one-workgroup regime uses it, every
 * other call may pass NULL / 0). */
uint64_t ffcv_color_jitter_workspace_bytes(int batch);
/* The largest image (height * width * 3 bytes) one workgroup keeps in LDS:
 * up to this size a program is ONE launch, beyond it one launch without and
 * two launches with a CONTRAST step. */
uint64_t ffcv_color_jitter_lds_bytes(void);
/* The program in place on a device [B][height][width][3] uint8 batch; step
 * i of image k runs when apply[i * batch + k] != 0, with ratio[i * batch +
 * k], on the previous step's uint8 result, exactly as the separate
 * operations would.  An image none of whose steps applies is not written.
 *   apply : device uint8[n_steps][B];  ratio : device float64[n_steps][B]
 *   workspace : device, 8-byte aligned, >= ffcv_color_jitter_workspace_bytes
 *               (zeroed on the stream by the call), or NULL where unused */
int ffcv_color_jitter_batch(void *stream, uint8_t *images, int batch,
                            int height, int width,
                            const ffcv_color_jitter_params *params,
                            const uint8_t *apply, const double *ratio,
                            void *workspace, uint64_t workspace_bytes);
/* The same program on host memory, compiled from the same pixel functions
 * as the kernels (gray, table entry, blend). */
int ffcv_color_jitter_batch_host(uint8_t *images, int batch, int height,
                                 int width,
                                 const ffcv_color_jitter_params *params,
                                 const uint8_t *apply, const double *ratio);

/* ------------------------- grayscale / solarization / Gaussian blur --- */
/* RandomGrayscale, RandomSolarization and GaussianBlur (the
 * reference has none of them, the semantics are this project's own).  Seeding
 * contract op ids: 9 grayscale, 10 solarization, 11 blur.  All three draw
 * like colour jitter: apply = rand() < p, then value = uniform(lo, hi), both
 * always drawn, in that order.
 *
 * The draws of grayscale (lo = hi = 0) and solarization (lo = hi =
 * threshold); their pixels are steps FFCV_CJ_GRAYSCALE / FFCV_CJ_SOLARIZE of
 * ffcv_color_jitter_batch.  op_id must be 9, 10 or 11, p in [0, 1], lo <= hi
 * finite; apply / value / status as in ffcv_color_jitter_draw_batch. */
int ffcv_uniform_draw_batch(void *stream, const uint64_t *sample_ids,
                            int batch, uint64_t loader_seed, uint64_t epoch,
                            int op_id, double p, double lo, double hi,
                            uint8_t *apply, double *value, int32_t *status);
int ffcv_uniform_draw_batch_host(const uint64_t *sample_ids, int batch,
                                 uint64_t loader_seed, uint64_t epoch,
                                 int op_id, double p, double lo, double hi,
                                 uint8_t *apply, double *value);

/* The blur's draws (op id 11) in one launch: the decision, sigma =
 * uniform(sigma_lo, sigma_hi) and the sample's float32 weights, a row of 32
 * floats per sample with entries [ksize, 32) zero.  In float64, with k =
 * ksize: e_j = exp(-0.5 (t_j t_j)), t_j = (j - (k - 1) / 2) / sigma; s = the
 * sum of e_j in ascending j; w_j = float32(e_j / s), stored as +0 where it
 * lies below 2^-126.  exp is the one function not pinned bit for bit.
 *   ksize : odd, 1 .. 31;  0 < sigma_lo <= sigma_hi, finite
 *   apply : uint8[B];  sigma : float64[B];  weights : float32[B][32]
 *   status : int32[B] or NULL (device entry only) */
int ffcv_blur_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                         uint64_t loader_seed, uint64_t epoch, double p,
                         double sigma_lo, double sigma_hi, int ksize,
                         uint8_t *apply, double *sigma, float *weights,
                         int32_t *status);
int ffcv_blur_draw_batch_host(const uint64_t *sample_ids, int batch,
                              uint64_t loader_seed, uint64_t epoch, double p,
                              double sigma_lo, double sigma_hi, int ksize,
                              uint8_t *apply, double *sigma, float *weights);

/* Separable blur of a dense device [B][height][width][3] uint8 batch, out of
 * place, in ONE launch; image k is written at dst + k * dst_stride_bytes (0 =
 * dense).  Image k is blurred with weights[k][0 .. ksize) where apply[k] != 0
 * and copied otherwise.  All pixel arithmetic is float32, every product and
 * sum rounded on its own (never fused), border reflect-101:
 *   h(y, x) = w_0 v(y, x - r) + w_1 v(y, x - r + 1) + ...   (ascending j)
 *   out     = uint8(clip(rint(w_0 h(y - r, x) + w_1 h(y - r + 1, x) + ...)))
 * with r = (ksize - 1) / 2 and rint rounding half to even; the weights must
 * be finite (the kernel also multiplies pixels by padding weights of +0, which
 * changes no finite sum).  Any byte
 * alignment of src and dst; loads are 16-byte aligned chunks holding at
 * least one byte of an image, so the allocation of src must extend to the
 * 16-byte boundaries around it (the rule of ffcv_gather_rows).
 * Two regimes: while 15 * height * width <= ffcv_gaussian_blur_lds_bytes()
 * a workgroup owns an image; larger images are cut into bands of
 * ffcv_gaussian_blur_band_rows() rows, and a band too wide for a workgroup's
 * LDS into column strips of ffcv_gaussian_blur_strip_cols(height, width,
 * ksize) columns (== width while one strip serves).  Supported sizes: height
 * and width up to 65535.
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, sizes <= 0 or
 * beyond 65535, an even ksize or one outside 1 .. 31, (ksize - 1) / 2 >=
 * min(height, width), a dst_stride_bytes smaller than an image, or src and dst
 * ranges that overlap (dst == src included). */
int ffcv_gaussian_blur_batch(void *stream, const uint8_t *src, uint8_t *dst,
                             int batch, int height, int width, int ksize,
                             const uint8_t *apply, const float *weights,
                             uint64_t dst_stride_bytes);
/* The same on host memory over nthreads threads, compiled from the kernel's
 * pixel functions. */
int ffcv_gaussian_blur_batch_host(const uint8_t *src, uint8_t *dst, int batch,
                                  int height, int width, int ksize,
                                  const uint8_t *apply, const float *weights,
                                  uint64_t dst_stride_bytes, int nthreads);
uint64_t ffcv_gaussian_blur_lds_bytes(void);
uint64_t ffcv_gaussian_blur_band_rows(void);
uint64_t ffcv_gaussian_blur_strip_cols(int height, int width, int ksize);

/* ------------------------------------------- RandomAdjustSharpness ----- */
/* RandomAdjustSharpness (the reference has none, the semantics
 * are Pillow's ImageEnhance.Sharpness restated in float32).  Seeding contract
 * op id 19: one draw per sample, apply = rand() < p.
 *   p in [0, 1];  factor finite in [0, 16]
 *   apply : uint8[B], 0 or 1;  factor_out : float32[B], float32(factor)
 *   status : int32[B] or NULL (device entry only) */
int ffcv_sharpness_draw_batch(void *stream, const uint64_t *sample_ids,
                              int batch, uint64_t loader_seed, uint64_t epoch,
                              double p, double factor, uint8_t *apply,
                              float *factor_out, int32_t *status);
int ffcv_sharpness_draw_batch_host(const uint64_t *sample_ids, int batch,
                                   uint64_t loader_seed, uint64_t epoch,
                                   double p, double factor, uint8_t *apply,
                                   float *factor_out);

/* Sharpness of a dense device [B][height][width][3] uint8 batch, out of
 * place, in ONE launch; image k is written at dst + k * dst_stride_bytes (0 =
 * dense).  apply[k] selects per image:
 *   1 : sharpen with a = factor[k];
 *   2 : leave dst alone (nothing of image k is read or written);
 *   0 and every other value : copy src to dst.
 * All arithmetic is float32, every product, difference and sum rounded on its
 * own (never fused).  With w = 1/13, w5 = 5/13 (float32 quotients) and v the
 * bytes of a channel, for a byte i = v(y, x) inside the outermost ring of an
 * image of at least 3 x 3:
 *   row(y') = (w v(y', x - 1) + wc v(y', x)) + w v(y', x + 1)
 *             (wc = w5 on the centre row, w elsewhere)
 *   s = ((0.5 + row(y - 1)) + row(y)) + row(y + 1)
 *   d = float(int(clamp(s, 0, 255)))
 *   out = uint8(clamp(d + a (i - d), 0, 255))         (truncation)
 * and d = i on the outermost ring and in images below 3 x 3, which therefore
 * come out unchanged.  factor[k] must be finite where apply[k] == 1.
 * Any byte alignment of src and dst; loads are 16-byte aligned chunks holding
 * at least one byte of an image (the rule of ffcv_gather_rows).
 * Two regimes: while 6 * height * width <= ffcv_sharpness_lds_bytes() a
 * workgroup owns an image; larger images are cut into bands of
 * ffcv_sharpness_band_rows() rows, and a band too wide for a workgroup's LDS
 * into column strips of ffcv_sharpness_strip_cols(height, width) columns (==
 * width while one strip serves).  Supported sizes: height and width up to
 * 65535.
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, sizes <= 0 or
 * beyond 65535, a dst_stride_bytes smaller than an image, src and dst ranges
 * that overlap (dst == src included), or more workgroups than one launch
 * takes. */
int ffcv_sharpness_batch(void *stream, const uint8_t *src, uint8_t *dst,
                         int batch, int height, int width,
                         const uint8_t *apply, const float *factor,
                         uint64_t dst_stride_bytes);
/* The same on host memory over nthreads threads, compiled from the kernel's
 * pixel functions (csrc/sharpness_common.h). */
int ffcv_sharpness_batch_host(const uint8_t *src, uint8_t *dst, int batch,
                              int height, int width, const uint8_t *apply,
                              const float *factor, uint64_t dst_stride_bytes,
                              int nthreads);
uint64_t ffcv_sharpness_lds_bytes(void);
uint64_t ffcv_sharpness_band_rows(void);
uint64_t ffcv_sharpness_strip_cols(int height, int width);

/* ------------------------------- hue, jointly gated colour jitter ----- */
/* RandomHue and RandomColorJitter (the reference has neither,
 * the semantics are this project's own).  Seeding contract op ids: 12 hue,
 * 13 joint colour jitter.
 *
 * Hue's draws: apply = rand() < p, then shift = uniform(-magnitude,
 * magnitude), both always drawn, in that order.  p in [0, 1], magnitude
 * finite in [0, 0.5]; sample_ids / apply / shift / status as in
 * ffcv_color_jitter_draw_batch. */
int ffcv_hue_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                        uint64_t loader_seed, uint64_t epoch, double p,
                        double magnitude, uint8_t *apply, double *shift,
                        int32_t *status);
int ffcv_hue_draw_batch_host(const uint64_t *sample_ids, int batch,
                             uint64_t loader_seed, uint64_t epoch, double p,
                             double magnitude, uint8_t *apply, double *shift);

/* The joint draws: five values from ONE stream per sample, always all five:
 * rand() < p, then uniform(max(0, 1 - m), 1 + m) for m = magnitude[0]
 * (brightness), [1] (contrast), [2] (saturation), then uniform(-magnitude[3],
 * magnitude[3]) (hue).  magnitude is a HOST array of four: the first three
 * finite and >= 0, the fourth finite in [0, 0.5].  One row of apply / ratio is
 * written per component with a non-zero magnitude, compacted in the order
 * brightness, contrast, saturation, hue; every apply row carries the one
 * decision.  The brightness / contrast / saturation rows are thus the
 * [n_steps][B] arrays ffcv_color_jitter_batch takes for the program of the
 * active components, and the hue row, the last, is what ffcv_hue_batch takes.
 *   apply : uint8[rows][B];  ratio : float64[rows][B], rows <= 4
 *   status : int32[B] or NULL (device entry only) */
int ffcv_color_jitter_joint_draw_batch(void *stream,
                                       const uint64_t *sample_ids, int batch,
                                       uint64_t loader_seed, uint64_t epoch,
                                       double p, const double *magnitude,
                                       uint8_t *apply, double *ratio,
                                       int32_t *status);
int ffcv_color_jitter_joint_draw_batch_host(const uint64_t *sample_ids,
                                            int batch, uint64_t loader_seed,
                                            uint64_t epoch, double p,
                                            const double *magnitude,
                                            uint8_t *apply, double *ratio);

/* The hue shift in place on a device [B][height][width][3] uint8 batch, in ONE
 * launch; image k is turned by shift[k] (|shift[k]| <= 0.5) where apply[k] !=
 * 0 and is neither read nor written otherwise.  Per pixel, with integers r, g,
 * b and D = float32(float64(6) * shift[k]), all else float32 with every
 * operation rounded on its own (never fused), `/` the correctly rounded IEEE
 * division:
 *   mx, mn = max, min of (r, g, b);  c = mx - mn;  c == 0: unchanged
 *   C = float32(c);  V = float32(mx)
 *   (num, base) = (g - b, 0) if mx == r, else (b - r, 2) if mx == g, else
 *                 (r - g, 4)
 *   x = base + float32(num) / C;  x = x + D
 *   x = x < 0 ? x + 6 : x;  then  x = x >= 6 ? x - 6 : x
 *   i = floor(x);  f = x - i;  s = C / V
 *   P = V * (1 - s);  Q = V * (1 - s * f);  T = V * (1 - s * (1 - f))
 *   (R, G, B) for i = 0 .. 5: (V,T,P) (Q,V,P) (P,V,T) (P,Q,V) (T,P,V) (V,P,Q)
 *   out = uint8(rint(value)), rint rounding half to even
 * Any byte alignment of images; loads are 16-byte aligned chunks holding at
 * least one byte of an applied image (the rule of ffcv_gather_rows), and no
 * byte outside an applied image is written.
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, sizes <= 0 or
 * 3 * height * width > 2^31 - 1. */
int ffcv_hue_batch(void *stream, uint8_t *images, int batch, int height,
                   int width, const uint8_t *apply, const double *shift);
/* The same on host memory, compiled from the kernel's pixel function. */
int ffcv_hue_batch_host(uint8_t *images, int batch, int height, int width,
                        const uint8_t *apply, const double *shift);

/* ------------------------------------- affine warp (rotation, shear) -- */
/* RandomAffine and RandomRotation (the reference has neither,
 * the semantics are this project's own).  Seeding contract op id: 14.
 *
 * The draws: seven values from one stream per sample, always all seven:
 * apply = rand() < p, angle = uniform(r0, r1) in degrees, tx =
 * rint(uniform(r2, r3)), ty = rint(uniform(r4, r5)), s = uniform(r6, r7),
 * shx = uniform(r8, r9), shy = uniform(r10, r11) in degrees, with r = ranges,
 * a HOST array of six (low, high) pairs; uniform is lo + (hi - lo) * rand(),
 * rint rounds half to even.  The matrix, in float64, every operation rounded
 * on its own, K = 0.017453292519943295, for height x width images:
 *   rot = angle K;  sx = shx K;  sy = shy K
 *   a = cos(rot - sy) / cos(sy)
 *   b = -(cos(rot - sy) tan(sx) / cos(sy)) - sin(rot)
 *   c = sin(rot - sy) / cos(sy)
 *   d = -(sin(rot - sy) tan(sx) / cos(sy)) + cos(rot)
 *   m00 = d / s;  m01 = -b / s;  m10 = -c / s;  m11 = a / s
 *   cx = (width - 1) / 2;  cy = (height - 1) / 2
 *   b0 = (m00 (-cx - tx) + m01 (-cy - ty)) + cx
 *   b1 = (m10 (-cx - tx) + m11 (-cy - ty)) + cy
 * and coef[k] = int64(rint(v * 65536)) of (m00, m01, b0, m10, m11, b1).  sin,
 * cos and tan are the functions not pinned bit for bit.
 *   ranges : finite, low <= high; angle within -360 .. 360, tx within -width
 *            .. width, ty within -height .. height, scale within 1/16 .. 16,
 *            both shears within -60 .. 60
 *   height, width : 1 .. 32767;  p in [0, 1]
 *   apply : uint8[B] (written even where p == 1);  coef : int64[B][6]
 *   status : int32[B] or NULL (device entry only) */
#define FFCV_AFFINE_BILINEAR 0
#define FFCV_AFFINE_NEAREST 1
int ffcv_affine_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                           uint64_t loader_seed, uint64_t epoch, double p,
                           const double *ranges, int height, int width,
                           uint8_t *apply, int64_t *coef, int32_t *status);
int ffcv_affine_draw_batch_host(const uint64_t *sample_ids, int batch,
                                uint64_t loader_seed, uint64_t epoch, double p,
                                const double *ranges, int height, int width,
                                uint8_t *apply, int64_t *coef);

/* The warp of a dense device [B][height][width][3] uint8 batch, out of place,
 * in ONE launch; image k is written at dst + k * dst_stride_bytes (0 = dense),
 * warped by q = coef[k] where apply[k] != 0 and copied otherwise.  Integers
 * only, in int64, for output column c and row r:
 *   X = q0 c + q1 r + q2;  Y = q3 c + q4 r + q5
 * a tap outside 0 <= iy < height, 0 <= ix < width takes the channel's fill
 * (a HOST array of three), each tap tested on its own; shifts are arithmetic.
 *   nearest:  out = tap((Y + 32768) >> 16, (X + 32768) >> 16)
 *   bilinear: ix = X >> 16, iy = Y >> 16, fx = (X & 0xFFFF) >> 8, fy alike
 *             top = (256 - fx) tap(iy, ix) + fx tap(iy, ix + 1)
 *             bot = the same on row iy + 1
 *             out = ((256 - fy) top + fy bot + 32768) >> 16
 * An image whose coefficients have |q0|, |q1|, |q3| or |q4| above 2^23, or
 * |q2| or |q5| above 2^40, comes out all fill.  Any byte alignment of src and
 * dst; loads are 16-byte aligned chunks holding at least one byte of an image
 * (the rule of ffcv_gather_rows); no byte outside dst's image ranges is
 * written.  While 3 * height * width <= ffcv_affine_whole_bytes() a workgroup
 * owns an image and stages it in LDS; larger images are cut into tiles of
 * ffcv_affine_tile_rows() x ffcv_affine_tile_cols() outputs, and a tile stages
 * its source footprint while that takes at most ffcv_affine_tile_lds() bytes
 * and reads its taps from global memory otherwise.
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, sizes outside
 * 1 .. 32767, 3 * height * width > 2^31 - 1, a mode other than the two, a
 * dst_stride_bytes smaller than an image, or src and dst ranges that overlap
 * (dst == src included). */
int ffcv_affine_batch(void *stream, const uint8_t *src, uint8_t *dst,
                      int batch, int height, int width, int mode,
                      const uint8_t *fill, const uint8_t *apply,
                      const int64_t *coef, uint64_t dst_stride_bytes);
/* The same on host memory over nthreads threads, compiled from the kernel's
 * pixel function. */
int ffcv_affine_batch_host(const uint8_t *src, uint8_t *dst, int batch,
                           int height, int width, int mode,
                           const uint8_t *fill, const uint8_t *apply,
                           const int64_t *coef, uint64_t dst_stride_bytes,
                           int nthreads);
uint64_t ffcv_affine_whole_bytes(void);
uint64_t ffcv_affine_tile_rows(void);
uint64_t ffcv_affine_tile_cols(void);
uint64_t ffcv_affine_tile_lds(void);
/* The bytes the kernel stages for tile (tile_row, tile_col) of a height x
 * width image under coef (a HOST array of six) and mode, from the kernel's own
 * footprint code: 0 for a tile that reads nothing (its footprint misses the
 * image; coefficients outside the bounds; invalid arguments), 2^64 - 1 for a
 * footprint whose relative coordinates leave 32 bits.  The tile reads global
 * memory directly when the value exceeds ffcv_affine_tile_lds() (beyond the
 * whole-image regime, where the value is the image's chunks). */
uint64_t ffcv_affine_tile_bytes(int height, int width, int mode,
                                const int64_t *coef, int tile_row,
                                int tile_col);

/* --------------------------------------------------------- mixup ------ */
/* mixup.py: ImageMixup.  Sample i of a dense [n_samples][sample_elems] array
 * belongs to batch s = i / batch_size, of length min(batch_size, n_samples -
 * s * batch_size); its neighbour is sample i - 1, or the LAST sample of its
 * own batch when i is the batch's first (a batch of one mixes a sample with
 * itself).  With l = lam[s] when same_lambda, else lam[i]:
 *   out[i][j] = cast(l * double(in[i][j]) + (1 - l) * double(in[nb][j]))
 * in float64, every multiply and add rounded on its own (never fused); the
 * cast truncates for uint8 (the value lies in [0, 255 + 3e-14]) and rounds to
 * nearest even for float32.  A launch of several batches is one call.
 *   in, out : device, aligned to the element size only (a uint8 batch may
 *             start at any byte); the two ranges must not overlap
 *   lam     : device float64, one per sample, or one per batch when
 *             same_lambda
 * FFCV_EINVAL, before any launch, for a null pointer, a count <= 0, an
 * unknown dtype or overlapping ranges. */
enum {
  FFCV_MIXUP_U8 = 1,
  FFCV_MIXUP_F32 = 2
};
int ffcv_mixup_batch(void *stream, const void *in, void *out,
                     int64_t n_samples, int64_t sample_elems, int dtype,
                     int64_t batch_size, const double *lam, int same_lambda);
/* The same on host memory (lam on the host too), compiled from the same
 * pixel function as the kernel, over nthreads threads (one sample at a
 * time each). */
int ffcv_mixup_batch_host(const void *in, void *out, int64_t n_samples,
                          int64_t sample_elems, int dtype, int64_t batch_size,
                          const double *lam, int same_lambda, int nthreads);
/* mixup.py: MixupToOneHot in one launch.  labels3 is device float32 [n][3]
 * of (label a, label b, lam) as LabelMixup writes it and is not changed;
 * out is device float32 [n][num_classes]: zeros, then out[i][a] = lam, then
 * out[i][b] = float(1) - lam (the second store wins when a == b).  A row
 * with a label outside [0, num_classes) stays zero and gets status[i] =
 * FFCV_SAMPLE_LABEL; every other status[i] is FFCV_SAMPLE_OK.
 *   status : device int32[n], required */
int ffcv_mixup_onehot_batch(void *stream, const float *labels3, float *out,
                            int64_t n, int64_t num_classes, int32_t *status);

/* -------------------------------------------------------- cutmix ------ */
/* ImageCutMix.  A sample is planes x height rows of width * pixel_bytes
 * bytes, dense, the samples outermost: NHWC of any dtype is planes = 1,
 * pixel_bytes = C * itemsize; contiguous NCHW is planes = C, pixel_bytes =
 * itemsize.  Batches and neighbours are those of ffcv_mixup_batch.  With the
 * box (y1, x1, y2, x2) = boxes[4 * s ..] when same_box, else boxes[4 * i ..],
 * each bound clamped to the image here:
 *   out[i] = in[i];  out[i][p][y1:y2][x1:x2] = in[nb][p][y1:y2][x1:x2]
 * for every plane p; a box with y1 >= y2 or x1 >= x2 is empty.  The bytes are
 * moved, never interpreted, so any dtype is served.  A launch of several
 * batches is one call.
 *   in, out : device, at any byte alignment; the two ranges must not overlap
 *   boxes   : device int32, aligned to 4 bytes, one box per sample, or one
 *             per batch when same_box
 * FFCV_EINVAL, before any launch, for a null pointer, a count <= 0,
 * pixel_bytes outside 1..64, a sample of more than 2^31 - 1 bytes or a batch
 * of more than 2^62, or overlapping ranges. */
int ffcv_cutmix_batch(void *stream, const void *in, void *out,
                      int64_t n_samples, int32_t planes, int32_t height,
                      int32_t width, int32_t pixel_bytes, int64_t batch_size,
                      const int32_t *boxes, int same_box);
/* The same on host memory (boxes on the host too) with memcpy of row
 * segments, over nthreads threads (one sample at a time each). */
int ffcv_cutmix_batch_host(const void *in, void *out, int64_t n_samples,
                           int32_t planes, int32_t height, int32_t width,
                           int32_t pixel_bytes, int64_t batch_size,
                           const int32_t *boxes, int same_box, int nthreads);

/* -------------------------------------------- poison, replace label ---- */
/* poisoning.py: Poison.  Every sample i of a dense uint8
 * [n_samples][sample_elems] array whose dataset index sample_ids[i] is in
 * the sorted set poison_ids is changed in place, element e to
 *   t1 = float32(float64(v) * keep[e])
 *   t2 = float32(float64(t1) + add[e])
 *   uint8(int(min(max(t2, clamp_lo), clamp_hi)))
 * which is numpy's `temp *= 1 - alpha; temp += mask * alpha; clip` on a
 * float32 temp with keep = float64(1 - alpha), add = float64(mask) * alpha.
 * Every other sample is neither read nor written.  Membership is decided on
 * the device: no host work and no copy per call.
 *   images     : device uint8 at any byte alignment
 *   sample_ids : device int64[n_samples] (a negative id is in no set)
 *   poison_ids : device uint64[n_poison], sorted, unique
 *   keep, add  : device float64[sample_elems] each, finite
 * n_poison == 0 returns FFCV_OK without a launch.  FFCV_EINVAL, before any
 * launch, for a null pointer, n_samples or sample_elems <= 0, n_poison < 0,
 * sizes that overflow, ids or tables not aligned to 8 bytes, a clamp outside
 * 0 <= clamp_lo <= clamp_hi <= 255 and a launch of more than 2^31 - 1
 * workgroups. */
int ffcv_poison_batch(void *stream, uint8_t *images, int64_t n_samples,
                      int64_t sample_elems, const int64_t *sample_ids,
                      const uint64_t *poison_ids, int64_t n_poison,
                      const double *keep, const double *add, float clamp_lo,
                      float clamp_hi);
/* The same on host memory (ids and tables on the host too), compiled from
 * the same membership and pixel functions as the kernel, over nthreads
 * threads (one sample at a time each). */
int ffcv_poison_batch_host(uint8_t *images, int64_t n_samples,
                           int64_t sample_elems, const int64_t *sample_ids,
                           const uint64_t *poison_ids, int64_t n_poison,
                           const double *keep, const double *add,
                           float clamp_lo, float clamp_hi, int nthreads);
/* replace_label.py: ReplaceLabel.  Row i of the device int64
 * [n][row_elems] labels becomes new_label where sample_ids[i] is in
 * poison_ids (ids as above); the other rows are not touched. */
int ffcv_replace_label_batch(void *stream, int64_t *labels, int64_t n,
                             int64_t row_elems, const int64_t *sample_ids,
                             const uint64_t *poison_ids, int64_t n_poison,
                             int64_t new_label);

/* ------------------- posterize / autocontrast / equalize / invert ------ */
/* RandomPosterize, RandomAutocontrast, RandomEqualize and RandomInvert
 * (the reference has none of them, the semantics are Pillow's
 * ImageOps).  Each is a 256-entry byte table per image and channel, applied
 * in place to a uint8 [H][W][3] image; autocontrast's table depends on the
 * channel's first and last occupied value, equalize's on its histogram.
 * Seeding contract op ids: 15 posterize, 16 autocontrast, 17 equalize,
 * 18 invert; each operation makes ONE draw per sample, rand() < p. */
enum {
  FFCV_TONE_POSTERIZE = 1,    /* v & ~(2 ** (8 - bits) - 1) */
  FFCV_TONE_AUTOCONTRAST = 2, /* ImageOps.autocontrast, cutoff 0 */
  FFCV_TONE_EQUALIZE = 3,     /* ImageOps.equalize, no mask */
  FFCV_TONE_INVERT = 4        /* 255 - v */
};

typedef struct ffcv_tone_params {
  int32_t n_steps;  /* 1..4 */
  uint8_t steps[4]; /* FFCV_TONE_* in pipeline order, each at most once */
  int32_t bits;     /* posterize's bits, 1..8 (read when the program has a
                       POSTERIZE step) */
} ffcv_tone_params;

/* The decisions of n operations (1..4) in one launch: apply[i * batch + k] =
 * rand() < p[i] from sample k's own stream of op id op_ids[i] (15..18).
 * op_ids and p are HOST arrays of n.
 *   sample_ids : device uint64[B];  apply : device uint8[n][B] out
 *   status     : device int32[B] out (FFCV_SAMPLE_RNG when a stream ran out),
 *                or NULL */
int ffcv_tone_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                         uint64_t loader_seed, uint64_t epoch, int n,
                         const int32_t *op_ids, const double *p,
                         uint8_t *apply, int32_t *status);
/* The same draws on host arrays (the CPU-device Loader). */
int ffcv_tone_draw_batch_host(const uint64_t *sample_ids, int batch,
                              uint64_t loader_seed, uint64_t epoch, int n,
                              const int32_t *op_ids, const double *p,
                              uint8_t *apply);

/* Bytes of workspace ffcv_tone_batch needs for `batch` images of any size
 * (3 x 256 uint32 counters per image; only a program with an AUTOCONTRAST or
 * EQUALIZE step on images beyond the one-workgroup regime uses it, every
 * other call may pass NULL / 0). */
uint64_t ffcv_tone_workspace_bytes(int batch);
/* The largest image (height * width * 3 bytes) one workgroup keeps in LDS:
 * up to this size a program is ONE launch, beyond it one launch without and
 * two launches with an AUTOCONTRAST or EQUALIZE step. */
uint64_t ffcv_tone_lds_bytes(void);
/* The program in place on a device [B][height][width][3] uint8 batch at any
 * byte alignment; step i of image k runs when apply[i * batch + k] != 0, on
 * the previous step's result, exactly as the separate operations would (the
 * launch composes the applied steps' tables on the image's histogram and
 * touches the pixels once).  An image none of whose steps applies is neither
 * read nor written.
 *   apply     : device uint8[n_steps][B]
 *   workspace : device, 4-byte aligned, >= ffcv_tone_workspace_bytes (zeroed
 *               on the stream by the call), or NULL where unused
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, a
 * non-positive shape, an image over 2^31 - 1 bytes, n_steps outside 1..4, an
 * unknown or repeated step, bits outside 1..8 with a POSTERIZE step, and a
 * missing, misaligned or short workspace where it is used.  batch == 0
 * returns FFCV_OK. */
int ffcv_tone_batch(void *stream, uint8_t *images, int batch, int height,
                    int width, const ffcv_tone_params *params,
                    const uint8_t *apply, void *workspace,
                    uint64_t workspace_bytes);
/* The same program on host memory, compiled from the same table functions as
 * the kernels (csrc/tone_common.h) and composed the same way. */
int ffcv_tone_batch_host(uint8_t *images, int batch, int height, int width,
                         const ffcv_tone_params *params, const uint8_t *apply);
/* ffcv_tone_batch with posterize's bits per image: bits is a device uint8[B]
 * read where a POSTERIZE step applies to image k (values outside 1..8 are
 * taken as the nearest of 1 and 8), or NULL for params->bits, which is
 * ffcv_tone_batch itself.  Everything else, errors included, as there. */
int ffcv_tone_batch_bits(void *stream, uint8_t *images, int batch, int height,
                         int width, const ffcv_tone_params *params,
                         const uint8_t *apply, void *workspace,
                         uint64_t workspace_bytes, const uint8_t *bits);
/* The same on host memory; with a POSTERIZE step, a bits[k] outside 1..8 is
 * FFCV_EINVAL before any image is touched. */
int ffcv_tone_batch_bits_host(uint8_t *images, int batch, int height,
                              int width, const ffcv_tone_params *params,
                              const uint8_t *apply, const uint8_t *bits);
/* The host twin's table builder: tables[j][v] of step `kind` (bits read by
 * POSTERIZE) for a channel whose 256-bin histogram is hists[j], j < n. */
int ffcv_tone_tables_host(int kind, int bits, const uint32_t *hists,
                          uint8_t *tables, int n);


/* ------------------------------------------ TrivialAugmentWide --------- */
/* The draws of the TrivialAugmentWide policy: every sample
 * runs exactly ONE of 14 operations at a random strength.  Seeding contract
 * op id 20; three draws per sample, always all three:
 *   op  = min(13, int(rand() * 14))
 *   bin = min(nbins - 1, int(rand() * nbins))
 *   neg = rand() < 0.5
 * v = table[op * nbins + bin], negated where neg and 1 <= op <= 9.  The table
 * (float64 [14][nbins], built by the caller; device memory for the device
 * entry) holds per operation:
 *    0 identity            -
 *    1 / 2 shear x / y     degrees
 *    3 / 4 translate x / y whole pixels
 *    5 rotate              degrees
 *    6 / 7 / 8 brightness / saturation ("color") / contrast: ratio = 1 + v
 *    9 sharpness           factor = float32(1 + v)
 *   10 posterize           bits (1..8)
 *   11 solarize            threshold (0..256)
 *   12 / 13 autocontrast / equalize   -
 * One lane per sample fills the arguments of the pixel launches:
 *   op           : uint8[B]
 *   cj_apply     : uint8[4][B], cj_ratio : float64[4][B] -- rows 0 .. 2 the
 *                  program BRIGHTNESS, SATURATION, CONTRAST of
 *                  ffcv_color_jitter_batch, row 3 the program SOLARIZE (a
 *                  program has at most three steps); ratio 1 and threshold
 *                  256 where the step does not apply
 *   tone_apply   : uint8[3][B], tone_bits : uint8[B] -- the program POSTERIZE,
 *                  AUTOCONTRAST, EQUALIZE of ffcv_tone_batch_bits (bits 8
 *                  where posterize does not apply)
 *   aff_apply    : uint8[B], aff_coef : int64[B][6] -- ffcv_affine_batch; the
 *                  coefficients of affine_matrix (scale 1, the one non-zero
 *                  argument v) for height x width images, the identity's
 *                  where the operation is not geometric
 *   sharp_apply  : uint8[B], 1 where op == 9 and 2 elsewhere, sharp_factor :
 *                  float32[B] -- ffcv_sharpness_batch
 *   status       : int32[B] or NULL (device entry only)
 * FFCV_EINVAL for a null pointer, batch < 0, nbins outside 2..256, or a
 * height or width outside 1..32767. */
int ffcv_policy_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                           uint64_t loader_seed, uint64_t epoch, int nbins,
                           const double *table, int height, int width,
                           uint8_t *op, uint8_t *cj_apply, double *cj_ratio,
                           uint8_t *tone_apply, uint8_t *tone_bits,
                           uint8_t *aff_apply, int64_t *aff_coef,
                           uint8_t *sharp_apply, float *sharp_factor,
                           int32_t *status);
int ffcv_policy_draw_batch_host(const uint64_t *sample_ids, int batch,
                                uint64_t loader_seed, uint64_t epoch,
                                int nbins, const double *table, int height,
                                int width, uint8_t *op, uint8_t *cj_apply,
                                double *cj_ratio, uint8_t *tone_apply,
                                uint8_t *tone_bits, uint8_t *aff_apply,
                                int64_t *aff_coef, uint8_t *sharp_apply,
                                float *sharp_factor);

/* ------------------------------------------------- RandAugment --------- */
/* RandAugment: every sample runs num_ops (1..8) of the 14
 * operations above in sequence, each on the uint8 result of the one before,
 * all at the strength of one bin, `magnitude` (0 .. nbins - 1).  Seeding
 * contract op id 23; one stream per sample, two draws per slot s = 0 ..
 * num_ops - 1, always both:
 *   op_s  = min(13, int(rand() * 14))
 *   neg_s = rand() < 0.5
 * v = table[op * nbins + magnitude], negated where neg and 1 <= op <= 9; the
 * table is float64 [14][nbins] as above (device memory for the device entry).
 * The output arrays are those of ffcv_policy_draw_batch, each with a leading
 * slot dimension: op uint8[S][B], cj_apply uint8[S][4][B], cj_ratio
 * float64[S][4][B], tone_apply uint8[S][3][B], tone_bits uint8[S][B],
 * aff_apply uint8[S][B], aff_coef int64[S][B][6], sharp_apply uint8[S][B],
 * sharp_factor float32[S][B].  Slot s's slice of each is contiguous and holds
 * what ffcv_policy_draw_batch would write for that slot's operation, so the
 * pixel entries above take a slot's slices unchanged.  status: int32[B] or
 * NULL, per sample (device entry only).
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, num_ops
 * outside 1..8, nbins outside 2..256, magnitude outside 0..nbins-1, or a
 * height or width outside 1..32767. */
int ffcv_randaugment_draw_batch(void *stream, const uint64_t *sample_ids,
                                int batch, uint64_t loader_seed,
                                uint64_t epoch, int num_ops, int nbins,
                                int magnitude, const double *table, int height,
                                int width, uint8_t *op, uint8_t *cj_apply,
                                double *cj_ratio, uint8_t *tone_apply,
                                uint8_t *tone_bits, uint8_t *aff_apply,
                                int64_t *aff_coef, uint8_t *sharp_apply,
                                float *sharp_factor, int32_t *status);
int ffcv_randaugment_draw_batch_host(const uint64_t *sample_ids, int batch,
                                     uint64_t loader_seed, uint64_t epoch,
                                     int num_ops, int nbins, int magnitude,
                                     const double *table, int height,
                                     int width, uint8_t *op, uint8_t *cj_apply,
                                     double *cj_ratio, uint8_t *tone_apply,
                                     uint8_t *tone_bits, uint8_t *aff_apply,
                                     int64_t *aff_coef, uint8_t *sharp_apply,
                                     float *sharp_factor);
/* 6 * height * width of the largest image ffcv_randaugment_batch takes. */
uint64_t ffcv_randaugment_lds_bytes(void);
/* The fused pixel pass: every slot of every sample in ONE launch, one
 * workgroup per image, the image in LDS from the first slot to the last.
 * src, dst: dense device uint8 [B][height][width][3], out of place (any
 * overlap is FFCV_EINVAL); src is not written.  mode, fill: as
 * ffcv_affine_batch.  The arrays are the draw's (device memory).  The kernel
 * reads slot s's op[s][k] and that operation's argument -- cj_ratio (rows 0,
 * 1, 2, 3 for brightness, saturation, contrast, solarize), tone_bits,
 * aff_coef, sharp_factor -- so `op` and the apply arrays must agree, as the
 * draw writes them; an op code outside 0..13 leaves the image as it is.  The
 * bytes equal those of the launches above run slot after slot on the slot's
 * slices; coefficients ffcv_affine_batch refuses give an image of fill here
 * too, and tone_bits is kept inside 1..8.
 * FFCV_EINVAL, before any launch, for a null pointer, batch < 0, sizes <= 0,
 * num_ops outside 1..8, an unknown mode, or 6 * height * width above
 * ffcv_randaugment_lds_bytes() (the caller runs the slots' launches then). */
int ffcv_randaugment_batch(void *stream, const uint8_t *src, uint8_t *dst,
                           int batch, int height, int width, int num_ops,
                           int mode, const uint8_t *fill, const uint8_t *op,
                           const uint8_t *cj_apply, const double *cj_ratio,
                           const uint8_t *tone_apply, const uint8_t *tone_bits,
                           const uint8_t *aff_apply, const int64_t *aff_coef,
                           const uint8_t *sharp_apply,
                           const float *sharp_factor);

/* ------------------------------------------------- random erasing ------ */
/* RandomErasing.  The draws of sample k, from its own MT19937
 * under the seeding contract with op id 21: rand() < p first, then up to ten
 * tries of (area, aspect ratio) for a box of h rows and w columns with
 * 0 < h < height and 0 < w < width, and the box's origin; the tries are drawn
 * whether or not the sample applies.
 *   sample_ids : device uint64[B]
 *   scale, ratio : host double[2] each (0 <= scale <= 1, ratio > 0, finite)
 *   boxes      : device int32[B][4] out, (y, x, h, w); h = w = 0: not erased
 *   keys       : device uint64[B] out, the noise keys (op id 22), or NULL
 *   status     : device int32[B] out (FFCV_SAMPLE_RNG when the sample's
 *                MT19937 stream ran out), or NULL
 * FFCV_EINVAL, before any launch, for a null sample_ids / boxes, batch < 0,
 * p outside [0, 1], a scale or ratio outside the above, or a height or width
 * outside 1..32767. */
int ffcv_erase_draw_batch(void *stream, const uint64_t *sample_ids, int batch,
                          uint64_t loader_seed, uint64_t epoch, double p,
                          const double scale[2], const double ratio[2],
                          int height, int width, int32_t *boxes,
                          uint64_t *keys, int32_t *status);
int ffcv_erase_draw_batch_host(const uint64_t *sample_ids, int batch,
                               uint64_t loader_seed, uint64_t epoch, double p,
                               const double scale[2], const double ratio[2],
                               int height, int width, int32_t *boxes,
                               uint64_t *keys);
/* The fill, in place, one launch.  The geometry is ffcv_cutmix_batch's: a
 * sample is planes x height rows of width * pixel_bytes bytes.  The box
 * (y, x, h, w) of sample i, clamped to the image here, is filled in every
 * plane; h <= 0 or w <= 0 leaves the sample alone.  No byte outside
 * [images, images + n_samples * sample bytes) is written and none outside the
 * box changes.
 *   FFCV_ERASE_CONSTANT: fill = planes x pixel_bytes bytes, one pixel of every
 *     plane, already in the tensor's dtype; itemsize and keys are not used.
 *   FFCV_ERASE_NOISE: element e of sample i (e: its index in storage order,
 *     in elements of itemsize bytes) becomes entry
 *     (splitmix64(keys[i] ^ (e >> 2)) >> (16 * (e & 3) + 4)) & 0xFFF
 *     of fill, a table of 4096 entries of itemsize (1, 2 or 4) bytes.
 *   images : device, aligned to itemsize in noise mode, any byte otherwise
 *   boxes  : device int32[n_samples][4];  keys : device uint64[n_samples]
 *   fill   : device; the noise table 16-byte aligned
 * FFCV_EINVAL, before any launch, for a null pointer, a count <= 0,
 * pixel_bytes outside 1..64 or (noise) no multiple of itemsize, an itemsize
 * other than 1, 2 or 4, a sample of more than 2^31 - 1 bytes, a mode other
 * than the two, a misaligned images or table, or more than 2^31 - 1 samples
 * or 65,535 planes in one launch. */
enum { FFCV_ERASE_CONSTANT = 0, FFCV_ERASE_NOISE = 1 };
int ffcv_erase_batch(void *stream, void *images, int64_t n_samples,
                     int32_t planes, int32_t height, int32_t width,
                     int32_t pixel_bytes, const int32_t *boxes, int mode,
                     int32_t itemsize, const void *fill, const uint64_t *keys);
/* The same on host memory, compiled from the kernel's box and noise
 * functions, over nthreads threads (one sample at a time each). */
int ffcv_erase_batch_host(void *images, int64_t n_samples, int32_t planes,
                          int32_t height, int32_t width, int32_t pixel_bytes,
                          const int32_t *boxes, int mode, int32_t itemsize,
                          const void *fill, const uint64_t *keys,
                          int nthreads);

#ifdef __cplusplus
}
#endif
#endif
