// jpeg_defs.h -- what the JPEG kernels of ffcv_jpeg.hip share: the tunables, the
// records K1, K1b and K2 pass to each other, K2's band-record writer, K1's
// LDS state, the launch arguments and the wave helpers.  Included by
// ffcv_jpeg.hip only (one translation unit).
#pragma once
#include "device_common.h"
#include "diag_hooks.h"

#define JT 64           // lanes per wave = lanes per image (K1 decodes one image per wave)
#define HDR_BYTES 2048  // header bytes staged in LDS (aliased by the LUT pool)
#ifndef FB_AC
#define FB_AC 11        // first-level bits, the scan's first AC table (luma)
#endif
static_assert(FB_AC <= 11, "FB_AC > 11 is not supported: a 12-bit build failed the bench parity check (DESIGN.md s6, r6j)");
#define FB_AC2 10       // first-level bits, further AC tables (chroma)
#ifndef FB_DC
#define FB_DC 8         // first-level bits, DC tables
#endif
// first-level LUT words shared by the slots (+ two zero words): one table of
// each AC size and two DC tables, the 4:2:0 / 4:2:2 / 4:4:4 norm
#define LUT_POOL ((1 << FB_AC) + (1 << FB_AC2) + 2 * (1 << FB_DC) + 2)
#define SUBB 5          // second-level bits
#ifndef NSUB
#define NSUB 8          // second-level tables per slot
#endif
#define NSLOT 6         // Huffman tables a scan can reference (3 DC + 3 AC)
#define NLUTSLOT 4      // slots that can get a first-level LUT from the pool
#define NTAB 8
#ifndef NEV
#define NEV 6
#endif
#define DS_FLUSH 8      // de-stuff steps per LDS -> HBM flush
#define DS_DEPTH 8      // de-stuff loads in flight per lane
#define STAGE_BYTES (DS_FLUSH * JT * 4 + 64)  // a flush's bytes + the carried tail + pad
#define STAGE_DUMMY (STAGE_BYTES - 4)
#define STREAM_PAD 32   // zero bytes after the de-stuffed stream
#ifndef ACS_Z
#define ACS_Z 24        // zigzag positions of a block the write pass stages in LDS
#endif
#define ACS_BYTES (ACS_Z * 2)
// AC steps per chunk of the write pass (write_range): the per-block work runs
// once per chunk.  2, 3 and 4 were measured.
#ifndef K1_WCHUNK
#define K1_WCHUNK 4
#endif
static_assert(K1_WCHUNK >= 1 && K1_WCHUNK <= 8, "K1_WCHUNK outside 1..8 is not supported: past 8 a flat block idles through most of its chunk (tools/sync_sim.c chunks)");
// K1 decode extent (entropy_passes): the entropy decode stops at the linear
// estimate of where the crop window's last MCU row ends, plus a margin of
// K1_EXT_REL / 256 of the stream and K1_EXT_ABS bits (chosen with the host
// model, tools/k1_extent_model.py; K1_EXT_REL >= 256 always decodes in full).
#ifndef K1_EXT_REL
#define K1_EXT_REL 8
#endif
#ifndef K1_EXT_ABS
#define K1_EXT_ABS 2048
#endif
#ifndef BAND
#define BAND 16  // K2 output rows per workgroup
#endif
#ifndef K2T
#define K2T 256  // K2 threads per workgroup
#endif
#define K2_COLS 128  // K2 fast path: output column-pair slots (out_w <= 256); K2T / K2_COLS row groups
#ifndef K2_LDS
#define K2_LDS 26624  // K2 dynamic LDS: the most that keeps 6 workgroups per CU (6 x 26 KB of 160 KB; 512 B granules); bigger bands take the general path (24 KB: 1% slower at C3, 32 KB: 3% slower)
#endif
#ifndef JW
#define JW 4  // waves per K1 workgroup
#endif

enum JMode { JM_RRC = 0, JM_FULL = 1, JM_COEF = 2 };

// Per-image geometry written by K1 for K2.
struct ImgInfo {
  int32_t status;
  int32_t W, H, ncomp, color_rgb;
  int32_t he[3], ve[3];  // expansion factors hmax/h, vmax/v
  int32_t cw[3], ch[3], stride[3];
  int32_t ri, rj, rh, rw;
  // arena offset of each component's window plane, minus (wy0 * 8 * stride +
  // wx0 * 8): plane sample (row, col) in absolute coordinates is at
  // arena + poff + row * stride + col (stride = window width in samples)
  uint64_t poff[3];
  uint64_t rgb_off;  // K2 band staging (crop rows as RGB) for bands wider than LDS
  // RRC: the crop's resize plan, and whether K1 wrote the image's linear tap
  // table (JpegArgs::taps: out_w column taps, flip applied, then out_h row
  // taps), computed once per image instead of once per K2 workgroup
  ResizePlan plan;
  int32_t taps;
  // K1 -> jpeg_idct_kernel: what the DC prediction and the IDCT need
  uint64_t cf_off;   // arena offset of the window coefficients
  uint64_t coff[3];  // first window block of each component in the coefficient region
  int32_t nblocks, bpm, mcux;
  int32_t hs[3], vs[3], wx0[3], wx1[3], wy0[3], wy1[3], qmax[3];
  int32_t blk_comp[10], blk_dx[10], blk_dy[10];
  // DC prediction (RRC / FULL): slot 0 of a window block holds the running sum,
  // per component, of the DC differences its decoding lane had read up to and
  // including it; the absolute DC adds that lane's offset (the sums of the
  // lanes before it).  lane_blk0[l]: first block lane l started (non-decreasing)
  uint32_t lane_blk0[64];
  int32_t lane_off[3][64];
  int16_t qmul[3][64] __attribute__((aligned(16)));
  // this image's launch-arena reservation [arena_base, arena_base +
  // arena_need) (need 0: none); read only by ffcv_jpeg_arena_regions
  uint64_t arena_base, arena_need;
};

#define K2_TAPS 512  // tap table entries per image: out_w + out_h <= 512 (tap_pack format)


// K2's per-band record (RRC): everything a band workgroup of an OK image
// needs once it has checked the image's status, written once per image by K1b
// (one thread per band, from the image record it holds in LDS; JpegArgs::brec,
// ceil(out_h / BAND) records per image)
// instead of being rebuilt from ImgInfo by each of the image's band
// workgroups (band_rows in f64, three components' tile bounds, the LDS layout
// and the path selection: ~100 live scalars that spilled).  A band whose
// selector is K2B_GENERAL reads nothing else of it: the general path keeps
// the ImgInfo head.  Tile fields are packed in halves: a fast band's tile
// rows, pitches and LDS offsets are below K2_LDS, plane and image dimensions
// below 2^16 (ffcv_jpeg_create), strides multiples of 8 below 2^19.
enum { K2B_GENERAL = 0, K2B_LINEAR = 1, K2B_AREA = 2 };  // fmt bits 0-1
#define K2B_Q420 4u    // the 4:2:0 colour pass applies (every K2B_AREA band)
#define K2B_TAPS 8u    // K1 wrote the image's linear tap table (ImgInfo::taps)
#define K2B_NCOMP_SH 4     // bits 4-5: ncomp
#define K2B_RGB 64u        // color_rgb
#define K2B_EXP_SH 8       // from bit 8, per component c: log2 he at 4 c, log2 ve at 4 c + 2
struct __attribute__((aligned(128))) K2BandRec {
  uint32_t fmt;
  int32_t r0, nrows;  // band_rows: crop rows [r0, r0 + nrows) feed this band
  int32_t need;       // LDS bytes of the fast layout (fast selectors: <= K2_LDS)
  uint64_t pbase[3];  // arena offset of tile sample (ty0, tx0): poff + ty0 * stride + tx0
  uint32_t tyx[3];    // tile origin in the plane: ty0 | tx0 << 16
  uint32_t trp[3];    // tile rows | tile pitch << 16
  uint32_t tos[3];    // tile's LDS offset | (plane stride >> 3) << 16
  uint32_t cwh[3];    // plane size: cw | ch << 16
  uint32_t rgbp;      // LDS offset of the RGB rows | the area rows' pitch << 16
  int32_t ri, rj, rw;
  int32_t sw, sh;            // the plan's source size (the crop's)
  double scale_x, scale_y;   // the plan's scales (the area walk's taps)
};
static_assert(sizeof(K2BandRec) == 128, "K2BandRec is 32 dwords");
#define K2_REC_BANDS 16  // bands per image a context's record buffer starts with (out_h <= 256; grown on demand)

// One band's record.  The expressions are the ones K2's set-up evaluated per
// workgroup before (band_rows, the tile clamps and the LDS layout decide
// which plane samples a band reads).  GS: the image's geometry (K1's LDS
// state, or the image record), read where it is used and every field stored
// as soon as it is known, so the writer adds nothing to its kernel's register
// peak; the selector goes last (the layout's size decides it).  lut_b: bytes
// of the FP16 LUT ahead of the layout.
template <class GS>
FFCV_DEV void k2_write_band_rec(K2BandRec *o, const GS &g, const ResizePlan &P, int out_w, int out_h, int band,
                                int lut_b, int taps) {
  // expansion factors 1 / 2 / 4 (every common subsampling): the tile bounds
  // below divide by shifts; 3 takes the general path
  auto p2 = [](int x) { return x == 1 || x == 2 || x == 4; };
  const bool pow2 = p2(g.he(0)) && p2(g.ve(0)) && p2(g.he(1)) && p2(g.ve(1)) && p2(g.he(2)) && p2(g.ve(2));
  const int ncomp = g.ncomp();
  const bool q420 = ncomp == 3 && !g.color_rgb() && g.he(0) == 1 && g.ve(0) == 1 && g.he(1) == 2 && g.ve(1) == 2 &&
                    g.he(2) == 2 && g.ve(2) == 2 && g.cw(1) > 2 && g.cw(2) > 2;
  // area fast path (round 6): INTER_AREA crops with both scales in [1, 2)
  // (every RRC crop larger than the output on both axes, up to 2x) of 4:2:0
  // images.  (scale_x = 1 / (dw / sw) < 2 exactly when sw < 2 dw: integer
  // tests keep the f64 scales out of this condition)
  const bool area_fast = P.kind == 2 && P.sw < 2 * P.dw && P.sh < 2 * P.dh && q420;
  // linear fast path: kind 3 with the SSE2 vertical body on every element
  // (every RRC crop that is upscaled along some axis at out_w 224)
  if (!(((P.kind == 3 && P.vec_end == 3 * out_w) || area_fast) && (out_w & 1) == 0 && out_w <= 2 * K2_COLS && pow2)) {
    o->fmt = K2B_GENERAL;  // (nothing else is read)
    return;
  }
  const int oy0 = band * BAND, oy1 = min(out_h, oy0 + BAND);
  int r0, r1;
  band_rows(P, oy0, oy1, &r0, &r1);
  const int nrows = r1 - r0 + 1;
  o->r0 = r0;
  o->nrows = nrows;
  const int ri = g.ri(), rj = g.rj(), rw = g.rw();
  o->ri = ri;
  o->rj = rj;
  o->rw = rw;
  o->sw = P.sw;
  o->sh = P.sh;
  o->scale_x = P.scale_x;
  o->scale_y = P.scale_y;
  // LDS: [LUT][row taps][component tiles, dword rows][crop rows]
  int need = lut_b + (area_fast ? (int)sizeof(AreaTaps) : (int)sizeof(LinTap)) * BAND;
  uint32_t fmt = area_fast ? K2B_AREA : K2B_LINEAR;
  fmt |= (q420 ? K2B_Q420 : 0u) | (taps ? K2B_TAPS : 0u) | ((uint32_t)ncomp << K2B_NCOMP_SH) | (g.color_rgb() ? K2B_RGB : 0u);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c >= ncomp) {
      o->pbase[c] = 0;
      o->tyx[c] = o->trp[c] = o->tos[c] = o->cwh[c] = 0;
      continue;
    }
    const int he = g.he(c), ve = g.ve(c), hsh = he >> 1, vsh = ve >> 1;  // 1 / 2 / 4 -> 0 / 1 / 2
    const int cw = g.cw(c), ch = g.ch(c), stride = g.stride(c);
    fmt |= ((uint32_t)hsh | ((uint32_t)vsh << 2)) << (K2B_EXP_SH + 4 * c);
    int y0 = ((ri + r0) >> vsh) - (ve == 2 ? 1 : 0), y1 = ((ri + r1) >> vsh) + (ve == 2 ? 1 : 0);
    int x0 = (rj >> hsh) - (he == 2 ? 1 : 0), x1 = ((rj + rw - 1) >> hsh) + (he == 2 ? 1 : 0);
    y0 = max(y0, 0);
    x0 = max(x0, 0);
    y1 = min(y1, ch - 1);
    x1 = min(x1, cw - 1);
    const int tx0 = x0 & ~3;  // whole dwords of the plane row (rows are 8-byte aligned)
    const int trows = y1 - y0 + 1, tpitch = ((x1 + 4) & ~3) - tx0;
    o->pbase[c] = g.poff(c) + (uint64_t)y0 * stride + tx0;
    o->tyx[c] = (uint32_t)y0 | ((uint32_t)tx0 << 16);
    o->trp[c] = ((uint32_t)trows & 0xffffu) | ((uint32_t)tpitch << 16);
    o->tos[c] = ((uint32_t)need & 0xffffu) | ((uint32_t)(stride >> 3) << 16);
    o->cwh[c] = (uint32_t)cw | ((uint32_t)ch << 16);
    need += trows * tpitch;
  }
  const int rgb_off = need;
  // area: RGB rows from luma column Xb = 2 * (rj >> 1) (the colour pass's
  // first quad column), 12 bytes per chroma column pair, 4-byte aligned;
  // + 16 bytes for the walk's aligned reads past the last row's end
  const int pitch3 = 12 * (((((rj + rw - 1) >> 1) - (rj >> 1)) + 2) >> 1);
  need += area_fast ? nrows * pitch3 + 16 : nrows * rw * 4 + 4;  // linear: + a dummy word for off-crop pixels
  o->rgbp = ((uint32_t)rgb_off & 0xffffu) | ((uint32_t)pitch3 << 16);
  o->need = need;
  // (a fast band's packed halves fit, see K2BandRec; a band that turns out
  // general here has low halves cut to 16 bits and high halves that may have
  // lost bits: K2 reads none of them under K2B_GENERAL)
  o->fmt = need <= K2_LDS ? fmt : (uint32_t)K2B_GENERAL;
}

// The geometry k2_write_band_rec reads, from an image record.
struct InfoGeom {
  const ImgInfo &I;
  FFCV_DEV int ncomp() const { return I.ncomp; }
  FFCV_DEV int color_rgb() const { return I.color_rgb; }
  FFCV_DEV int he(int c) const { return I.he[c]; }
  FFCV_DEV int ve(int c) const { return I.ve[c]; }
  FFCV_DEV int cw(int c) const { return I.cw[c]; }
  FFCV_DEV int ch(int c) const { return I.ch[c]; }
  FFCV_DEV int stride(int c) const { return I.stride[c]; }
  FFCV_DEV uint64_t poff(int c) const { return I.poff[c]; }
  FFCV_DEV int ri() const { return I.ri; }
  FFCV_DEV int rj() const { return I.rj; }
  FFCV_DEV int rw() const { return I.rw; }
};

// Huffman decode tables built from one image's DHT segments.  K1 runs JW
// images per workgroup; images whose tables (and table slots) are byte-
// identical to the workgroup's first valid image share ONE LDS copy -- the
// usual case, every encoder of a dataset writes the same tables -- and any
// other image builds its own copy in global scratch (L1/L2-resident).
struct JTables {
  uint32_t lim[NSLOT][17];  // left-justified end of length-l codes
  int32_t valoff[NSLOT][17];
  uint8_t vals[NSLOT][256];
  int nsub[NSLOT];
  int nvals[NSLOT];
  int bad;
  uint16_t sub_prefix[NSLOT][NSUB];
  // second-level tables (codes longer than the first level; make_entry format)
  uint16_t lut2[NLUTSLOT][NSUB][1 << SUBB];
  uint32_t lut[LUT_POOL];  // first-level LUT pool (single or pair entries, see make_pair)
};

// Per-image (per-wave) state.
struct JShared {
  int status;
  const uint8_t *src;  // the image's bytes (read by the workgroup's table build)
  int W, H, ncomp, hmax, vmax;
  int hs[3], vs[3], tq[3], td[3], ta[3], cid[3];
  int color_rgb;
  int mcux, mcuy, bpm, nblocks;
  int cw[3], ch[3], bw[3], bh[3];
  int blk_comp[10], blk_dx[10], blk_dy[10];
  // Huffman table slots referenced by the scan (AC first); per block-in-MCU
  // slot numbers packed 3 bits per phase; per slot LUT base and bits
  int nslots;
  int slot_tab[NSLOT];  // class * 4 + id
  uint32_t sinfo[NSLOT];  // see SI_* below
  uint32_t dcpack, acpack, acmask;
  uint32_t scan_off;
  uint32_t dqt_off[4];
  int dqt_prec[4], dqt_ok[4];
  uint32_t dht_off[NTAB];
  int dht_ok[NTAB];
  int saw_jfif, saw_adobe, adobe_transform;
  int restart;
  int ri, rj, rh, rw;
  int wx0[3], wx1[3], wy0[3], wy1[3];
  uint64_t coff[3];  // first window block of each component in the coefficient region
  uint64_t poff[3];  // see ImgInfo::poff
  uint32_t nwin;     // window blocks (all components)
  // this image's regions of the launch arena (bump-allocated after the parse)
  uint64_t ds_off, cf_off, dc_off, rgb_off;
  uint32_t ds_bytes, cf_bytes, dc_bytes;
  uint32_t dlen;
  int any;
  // per block-in-MCU (phase) record, read by the decode loops for the phase
  // that follows the current one: its DC / AC table sinfo, its own successor
  // (so the loops carry the next phase index instead of computing ph + 1 mod
  // bpm and its address every step), and the write pass's descriptor: block
  // index of MCU (0,0) in the component's window, blocks per MCU row step,
  // hs, and the window as MCU ranges [mx_lo, mx_hi] x [my_lo, my_hi]
  // (64 bytes: the record address is one shift-add from the phase index)
  struct __attribute__((aligned(16))) PhaseRec {
    uint32_t dinf, ainf;
    int next, pad;
    int4 pd0, pd1, pad2;
  } phr[10];
  int qmax[3];  // max |qmul| of the AC multipliers per component (the IDCT's 32-bit-product test)
  union __attribute__((aligned(16))) {
    uint8_t hdr[HDR_BYTES];       // P0-P1: the first header bytes
    uint32_t ev[2][NEV + 1][JT];  // P3: block-start events (pos << 4 | phase), double-buffered
    uint8_t stage[STAGE_BYTES];   // P2: de-stuffed bytes awaiting a flush
    uint4 acs[JT][ACS_BYTES / 16];  // P5: each lane's block of low-frequency AC coefficients
  };
};

struct K1Shared {
  JTables tab;
  JShared w[JW];
};

// zigzag index of each natural (row-major) coefficient position; the entropy
// pass stores coefficients in zigzag order
constexpr uint8_t kZigzagOfNatural[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__constant__ uint8_t c_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__constant__ int32_t c_aanscales[64] = {
    16384, 22725, 21407, 19266, 16384, 12873, 8867,  4520,  22725, 31521, 29692, 26722, 22725,
    17855, 12299, 6270,  21407, 29692, 27969, 25172, 21407, 16819, 11585, 5906,  19266, 26722,
    25172, 22654, 19266, 15137, 10426, 5315,  16384, 22725, 21407, 19266, 16384, 12873, 8867,
    4520,  12873, 17855, 16819, 15137, 12873, 10114, 6967,  3552,  8867,  12299, 11585, 10426,
    8867,  6967,  4799,  2446,  4520,  6270,  5906,  5315,  4520,  3552,  2446,  1247};

struct JpegArgs {
  const uint8_t *base;
  const ffcv_sample *samples;
  const int32_t *crops;
  const int32_t *cut;
  const uint8_t *flips;
  int32_t *crops_w;  // the same arrays, written by the fused draws
  int32_t *cut_w;
  uint8_t *flips_w;
  ffcv_rrc_params p;
  void *out;
  uint64_t out_stride;
  int32_t *status;
  // Per-launch scratch arena: K1 bump-allocates each image's regions (de-
  // stuffed stream, window coefficients, DC differences, window planes, K2
  // band staging) sized by that image's own geometry and crop window, so
  // scratch follows the content instead of dataset-max x batch.
  uint8_t *arena;
  uint64_t arena_bytes;
  unsigned long long *arena_top;  // [0] bump counter (0 when K1 starts), [1] last launch's high water
  ImgInfo *info;
  uint2 *taps;    // K2_TAPS packed linear taps per image (RRC), written by K1
  uint8_t *gtab;  // per-image JTables for images that cannot share the workgroup's
  uint64_t gtab_slot;
  int batch;
  // fused gather + draws (ffcv_jpeg_rrc_fused): samples = table[ids[k]],
  // crop / cutout / flip drawn in K1 (lanes 1-3) into crops / cut / flips
  const ffcv_sample *table;
  uint64_t n_table;
  const uint64_t *ids;
  const uint32_t *k1_order;  // K1's image of (workgroup, wave) slot i (null: i itself); see k1_order_kernel
  ffcv_sample *samples_out;
  ffcv_draw_params dp;
  int do_draw;
  uint32_t max_h, max_w;
  uint64_t max_blocks;
  uint64_t *dbg;
  int diag_only;  // host side only: kernels the launch runs (ffcv_jpeg_set_diag)
  // Entropy index (ffcv_jpeg_set_entropy_index): per dataset sample, the
  // converged start state of every lane range of the sync pass.  A sample
  // decoded once with the index attached records it; later decodes of the
  // same sample (later epochs) skip the sync rounds.  Fused launches only
  // (the sample id comes from ids[k]).
  uint32_t *eidx;
  uint64_t eidx_n;
  // RRC: brec_bands = ceil(out_h / BAND) K2 band records per image, written by K1b
  K2BandRec *brec;
  int brec_bands;
};

// Diagnostic stamps: lane 0 records wall_clock64 at phase boundaries into
// dbg[image*16 + slot] (never read by the kernel; off when dbg == nullptr).
#define STAMP(slot)                                                          \
  do {                                                                       \
    if (a.dbg && t == 0) a.dbg[(uint64_t)k * 16 + (slot)] = wall_clock64();  \
  } while (0)

// p as a wave-uniform (scalar-register) pointer: every lane of the wave
// holds the same value when one image maps to one wave.
template <class P>
FFCV_DEV P *wave_uniform(P *p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (P *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// A wave-uniform value in a scalar register (one image per wave).
FFCV_DEV uint32_t wuni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Cross-lane helpers on DPP (no LDS round trip, unlike __shfl's
// ds_bpermute).  All lanes of the wave must be active.
//   wave_exscan: exclusive prefix sum (row_shr 1/2/4/8, row_bcast 15/31)
//   lane_prev / lane_next: value of lane t-1 / t+1 (0 past the ends)
FFCV_DEV uint32_t wave_exscan(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
  return (uint32_t)x - v;
}
FFCV_DEV uint32_t lane_prev(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }
FFCV_DEV uint32_t lane_next(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false); }
FFCV_DEV uint32_t lane_read(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
FFCV_DEV int32_t wave_exscan_i(int32_t v) { return (int32_t)wave_exscan((uint32_t)v); }
// lane_prev with lane 0's zero as an explicit select on the lane index t (the
// DPP move already leaves 0 there; the select is part of K1's compiled code)
FFCV_DEV uint32_t lane_prev0(uint32_t v, int t) {
  const uint32_t p = lane_prev(v);
  return t == 0 ? 0u : p;
}

// Wave-level syncs: K1's waves decode independent images, so after the
// workgroup's shared table build each wave orders only its own lanes.
FFCV_DEV void wsync_lds() {  // LDS writes of this wave visible to its lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
FFCV_DEV void wsync_mem() {  // LDS and global writes of this wave visible to its lanes
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
}
