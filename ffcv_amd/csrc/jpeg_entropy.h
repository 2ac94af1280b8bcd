// jpeg_entropy.h -- K1 of ffcv_jpeg.hip: the bit readers and decode tables, the
// header parse, scratch allocation, de-stuffing, the sync rounds, the write
// pass and the entropy index; k1_order_kernel and jpeg_entropy_kernel.
#pragma once
#include "jpeg_defs.h"

// ------------------------------------------------------------ bit reader --
// The de-stuffed stream: big-endian bytes read as 32-bit words from the
// image's scratch slot (L2-resident: written in P2, re-read every round),
// zero-padded by STREAM_PAD bytes so no read needs a bounds check.  The
// reader holds 33..64 valid bits plus the next word, loaded right after a
// refill and consumed at the following one (~5 symbols later), so a symbol
// (code <= 16 bits + <= 15 extra bits) never waits on memory.
typedef const __attribute__((address_space(1))) uint8_t gbytes_t;  // global memory
// Non-temporal loads of file bytes through the global address space: a
// generic pointer compiles to flat loads, which count in both vmcnt and
// lgkmcnt and defeat the compiler's per-load waits (every prefetch waited).
FFCV_DEV uint8_t gld_u8(const uint8_t *p) { return __builtin_nontemporal_load((gbytes_t *)p); }
FFCV_DEV uint32_t gld_u32(const uint32_t *p) {
  return __builtin_nontemporal_load((const __attribute__((address_space(1))) uint32_t *)p);
}
struct BitReader {
  gbytes_t *w;
  uint64_t acc;
  int nb;
  uint32_t wo;   // byte offset of the word in nxt (32-bit: scalar base + vector offset loads)
  uint32_t nxt;  // raw (little-endian) next word: swapped only when used, so
                 // its load is waited for at the next refill, not here
  FFCV_DEV uint32_t word(uint32_t off) const { return *(const __attribute__((address_space(1))) uint32_t *)(w + off); }
  FFCV_DEV void init(const uint32_t *words, uint32_t p) {
    w = (gbytes_t *)words;
    wo = (p >> 5) * 4;
    uint32_t w0 = __builtin_bswap32(word(wo)), w1 = __builtin_bswap32(word(wo + 4));
    wo += 8;
    nxt = word(wo);
    acc = (((uint64_t)w0 << 32) | (uint64_t)w1) << (p & 31);
    nb = 64 - (int)(p & 31);
  }
  FFCV_DEV void consume(int n) {
    acc <<= n;
    nb -= n;
    if (nb <= 32) {
      acc |= (uint64_t)__builtin_bswap32(nxt) << (32 - nb);
      nb += 32;
      wo += 4;
      nxt = word(wo);
    }
  }
};



struct DecState {
  uint32_t pos;
  int z;   // 0: next symbol is a DC; else index of the next AC coefficient
  int ph;  // block index inside the MCU
};

// Symbol -> decode entry: bits consumed (code + extra bits, 1..31) | extra
// bits << 5 | coefficient advance << 9.  DC: size = symbol, z 0 -> 1.  AC:
// size = low nibble; z advances by run+1, by 16 for ZRL, past the block for
// EOB.  A LUT word with bits-consumed 0 is not an entry: 0 sends the decode
// to the canonical fallback, (n + 1) << 5 to second-level table n.
FFCV_DEV uint32_t make_entry(bool ac, int len, int sym) {
  int size, zinc;
  if (!ac) {
    size = sym;
    zinc = 1;
  } else {
    size = sym & 15;
    int r = sym >> 4;
    zinc = size ? r + 1 : (r == 15 ? 16 : 127);
  }
  return (uint32_t)(len + size) | ((uint32_t)size << 5) | ((uint32_t)zinc << 9);
}

// Canonical decode of a 16-bit lookahead (jdhuff.c jpeg_huff_decode): the
// code length is the first l with look < lim[l]; past lim[16] the code is
// invalid and, like libjpeg, yields symbol 0 after 16 bits.
template <class TB>
FFCV_DEV uint32_t slow_entry(const TB &T, uint32_t acmask, int slot, uint32_t look) {
  int len = 1;
#pragma unroll
  for (int l = 1; l < 16; l++) len += look >= T.lim[slot][l];
  int sym = 0;
  if (look < T.lim[slot][16]) sym = T.vals[slot][(T.valoff[slot][len] + (int)(look >> (16 - len))) & 0xff];
  else len = 16;
  return make_entry((acmask >> slot) & 1, len, sym);
}

// Two AC symbols per first-level lookup.  When a first-level AC entry's
// symbol (code + extra bits, t1 bits) is not EOB and the next symbol's code
// and extra bits also fit in the first-level window, the entry carries both:
//   [0:5) total bits  [5:9) size1  [9:16) z advance of both (clamped 127)
//   [16:21) t1  [21:25) size2  [25:32) z advance of the first (1..16)
// A single entry has bits 16.. zero.  A pair never crosses a block end:
// the decoder takes only the first symbol when it alone reaches z = 64.
// Then e >> 16 is the first symbol's entry for the sync pass (bits t1 in
// [0:5), advance in [9:16)), so both passes select with one shift.  The
// symbol sequence and every bit position are the same as decoding one
// symbol per step.
template <class TB>
FFCV_DEV uint32_t make_pair(const TB &T, int slot, int bits, const uint32_t *L, uint32_t look, uint32_t e1) {
  // L[l] = T.lim[slot][l] for l <= FB_AC, in registers
  const int t1 = (int)(e1 & 31), size1 = (int)(e1 >> 5) & 15, zinc1 = (int)(e1 >> 9);
  if (zinc1 > 16 || t1 >= bits) return e1;  // EOB, or no room for a second code
  const uint32_t look2 = (look << t1) & 0xffffu;
  const int room = bits - t1;
  int len = 1;  // the canonical length if it is at most room (limits are non-decreasing)
#pragma unroll
  for (int l = 1; l < FB_AC; l++) len += (l < room && look2 >= L[l]) ? 1 : 0;
  if (look2 >= T.lim[slot][len]) return e1;  // a longer code
  const int sym = T.vals[slot][(T.valoff[slot][len] + (int)(look2 >> (16 - len))) & 0xff];
  const uint32_t e2 = make_entry(true, len, sym);
  const int t2 = (int)(e2 & 31), size2 = (int)(e2 >> 5) & 15, zinc2 = (int)(e2 >> 9);
  if (t2 > room) return e1;
  return (uint32_t)(t1 + t2) | ((uint32_t)size1 << 5) | ((uint32_t)min(zinc1 + zinc2, 127) << 9) |
         ((uint32_t)t1 << 16) | ((uint32_t)size2 << 21) | ((uint32_t)zinc1 << 25);
}

// inf = sinfo of the table: [0:5) 32 - first-level bits, [5:21) LUT byte
// offset, [21:24) slot, [24:27) second-level set, [27:31) first-level bits.
// The first-level index is the top bits of the reader's high word, one
// shift by the low field (the shifter reads 5 bits).  A slot without a
// first-level LUT (bits 0) has shift 31 onto two reserved zero words.
// Write-pass reader: every AC step and every chunk part (write_range) issues
// exactly one buffer load (a lane that does not refill reads out of range: no
// access, returns 0) and then a fixed set of buffer stores (two 2-byte stores
// in a step; the DC store and three 16-byte stores in a chunk part; out of
// range when a lane has nothing to store).  vmcnt counts loads and stores in
// issue order, so with these static counts the next step waits for its load
// with a counted vmcnt instead of draining the previous steps' coefficient
// stores (vmcnt(0), which the conditional global stores forced).
// (BUF_OOR / BUF_CFG: device_common.h)
struct BufReader {
  __amdgpu_buffer_rsrc_t rs;
  uint64_t acc;
  int nb;
  uint32_t wo;  // byte offset of the word in nxt
  uint32_t nxt, ld;
  bool rp;  // the previous step refilled: its load (ld) is the next word
  FFCV_DEV uint32_t word(uint32_t off) const { return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0); }
  FFCV_DEV void init(const uint32_t *words, uint32_t nbytes, uint32_t p) {
    rs = __builtin_amdgcn_make_buffer_rsrc((void *)words, 0, (int)nbytes, BUF_CFG);
    wo = (p >> 5) * 4;
    const uint32_t w0 = __builtin_bswap32(word(wo)), w1 = __builtin_bswap32(word(wo + 4));
    wo += 8;
    nxt = word(wo);
    ld = 0;
    rp = false;
    acc = (((uint64_t)w0 << 32) | (uint64_t)w1) << (p & 31);
    nb = 64 - (int)(p & 31);
  }
  FFCV_DEV void begin() { nxt = rp ? ld : nxt; }
  FFCV_DEV void consume(int n) {
    acc <<= n;
    nb -= n;
    const bool r = nb <= 32;
    acc |= r ? (uint64_t)__builtin_bswap32(nxt) << (r ? 32 - nb : 0) : 0ull;
    nb += r ? 32 : 0;
    wo += r ? 4u : 0u;
    ld = word(r ? wo : BUF_OOR);
    rp = r;
  }
};

FFCV_DEV uint32_t si_pack(uint32_t base, uint32_t bits, uint32_t slot, uint32_t set) {
  return (bits ? 32 - bits : 31) | (base * 4) << 5 | slot << 21 | set << 24 | bits << 27;
}
FFCV_DEV uint32_t si_base(uint32_t inf) { return ((inf >> 5) & 0xffff) >> 2; }
FFCV_DEV int si_bits(uint32_t inf) { return (int)(inf >> 27) & 15; }
FFCV_DEV int si_set(uint32_t inf) { return (int)(inf >> 24) & 7; }

template <class TB>
FFCV_DEV uint32_t decode_entry(const TB &T, uint32_t acmask, uint32_t inf, uint64_t acc, bool live = true) {
  const uint32_t hi = (uint32_t)(acc >> 32);
  uint32_t e = *(const uint32_t *)((const uint8_t *)T.lut + ((inf >> 5) & 0xffff) + ((hi >> (inf & 31)) << 2));
  if ((e & 31) == 0 && live) {  // (a finished lane of a wave-uniform loop skips the rare paths)
    const uint32_t look = hi >> 16;
    const int bits = si_bits(inf), slot = (int)(inf >> 21) & 7;
    if (e) e = T.lut2[si_set(inf)][(e >> 5) - 1][(look >> (16 - bits - SUBB)) & ((1 << SUBB) - 1)];
    if ((e & 31) == 0) e = slow_entry(T, acmask, slot, look);
  }
  return e;
}

FFCV_DEV int slot_of(uint32_t pack, int ph) { return (int)((pack >> (3 * ph)) & 7); }

// SYNC decode of a lane's range [st.pos, end_bit): counts the blocks started
// in it and records their start events (the first NEV; row NEV is a dummy
// that absorbs every non-recording store).  With use_old (a later round) it
// stops at a block start that matches an event of the lane's previous
// trajectory and splices onto it: from an identical state the old trajectory
// is exact, so its remaining count and exit state are reused.  A splice off
// the new trajectory's slot grid keeps the old events from the hit on, on a
// grid based at the hit's block count (eb), when they outnumber the new ones:
// a lane re-run again in a later round then still finds them (the sync
// rounds' wave-iterations fell 808 -> 774 per image, round 4).  The old-event
// cursor advances one event per symbol (old events behind the decode
// position can never match); lagging only delays a splice, never makes a
// wrong one.  Events are double-buffered: buffer cb holds the previous
// trajectory's, cb ^ 1 receives the new one.
//
// The loop body is straight-line except the refill, the second-level lookup
// and the canonical fallback: with 64 lanes some lane starts or ends a block
// on almost every step, so those updates are selects fed by loads issued at
// the top of the step (next phase's table infos, next old event).
template <bool use_old, class TB>
FFCV_DEV DecState sync_range(JShared &S, const TB &T, const uint32_t *words, DecState st,
                             uint32_t end_bit, int lane, uint32_t &cnt, int &nev, int &cb, int &eb,
                             DecState old_exit, int sh, uint32_t &iters) {
  const int smask = (1 << sh) - 1;  // events: every 2^sh-th block start (slot q = block eb + (q << sh))
  BitReader br;
  br.init(words, st.pos);
  uint32_t pos = st.pos;
  int z = st.z, ph = st.ph;
  uint32_t dinf = S.phr[ph].dinf, ainf = S.phr[ph].ainf;
  int nph = S.phr[ph].next;
  const int ob = cb, nbuf = cb ^ 1;
  const int onev = use_old ? nev : 0;
  const uint32_t *evo = &S.ev[ob][0][lane];
  uint32_t *evn = &S.ev[nbuf][0][lane];
  int j = 0;
  uint32_t ocur = onev > 0 ? evo[0] : 0xFFFFFFFFu;
  int n = 0;
  bool hit = false;
  while (pos < end_bit && !hit) {
    K1_DIAG(iters++);
    const uint32_t ndinf = S.phr[nph].dinf, nainf = S.phr[nph].ainf;
    const int nnph = S.phr[nph].next;
    const bool isblk = z == 0;
    const uint32_t key = (pos << 4) | (uint32_t)ph;
    if constexpr (use_old) {
      const uint32_t onext = evo[min(j + 1, NEV) * JT];
      hit = isblk && ocur == key;
      const bool adv = ocur < key;
      j += adv ? 1 : 0;
      ocur = adv ? (j < onev ? onext : 0xFFFFFFFFu) : ocur;
    }
    const bool rec = isblk && !hit;
    // slot n >> sh at a block start on the slot grid, else the dummy row NEV:
    // nz is 0 exactly then, and any non-zero nz pushes the index past NEV.
    // (A hit step may write its key: the splice below copies that same old
    // event into that slot.)
    const uint32_t nz = ((uint32_t)n & (uint32_t)smask) | (uint32_t)z;
    evn[min((n >> sh) + (int)(nz << 8), NEV) * JT] = key;
    n += rec ? 1 : 0;
    const uint32_t e = decode_entry(T, S.acmask, isblk ? dinf : ainf, br.acc);
    // a pair whose first symbol ends the block decodes that symbol alone
    // (e >> 16: its bits and advance); a hit leaves the loop, its step unused
    const uint32_t v = z + (int)(e >> 25) >= 64 ? e >> 16 : e;
    const int nbits = (int)(v & 31);
    br.consume(nbits);
    pos += nbits;
    z += (int)(v >> 9) & 127;
    const bool bend = z >= 64;
    z = bend ? 0 : z;
    ph = bend ? nph : ph;
    nph = bend ? nnph : nph;
    dinf = bend ? ndinf : dinf;
    ainf = bend ? nainf : ainf;
  }
  if (hit) {  // at the previous trajectory's event j = its block start eb + (j << sh)
    const uint32_t ocnt = (uint32_t)eb + ((uint32_t)j << sh);
    int m = min((n + smask) >> sh, NEV);  // slots written so far
    if ((n & smask) == 0 && m < NEV) {     // the old events stay on the slot grid: keep them
      const int keep = min(onev - j, NEV - m);
      for (int q = 0; q < keep; q++) evn[(m + q) * JT] = evo[(j + q) * JT];
      m += keep;
      eb = 0;
    } else if (onev - j > m) {  // off the grid: the old events from j on, on a grid based at n
      const int keep = min(onev - j, NEV);
      for (int q = 0; q < keep; q++) evn[q * JT] = evo[(j + q) * JT];
      m = keep;
      eb = n;
    } else {
      eb = 0;
    }
    nev = m;
    cnt = (uint32_t)n + (cnt - ocnt);
    cb = nbuf;
    return old_exit;
  }
  nev = min((n + smask) >> sh, NEV);
  cnt = (uint32_t)n;
  eb = 0;
  cb = nbuf;
  DecState out;
  out.pos = pos;
  out.z = z;
  out.ph = ph;
  return out;
}

// WRITE decode: DC differences of every block and the AC coefficients (in
// zigzag order; the IDCT de-zigzags in registers) of the blocks inside the
// window.  blk = index of the block in progress (z > 0) or of the next block
// to start (z == 0).  The loop runs in chunks: a per-chunk part that does
// everything a block boundary needs (flush of the block that ended in the
// last chunk, the next block's destination and window test from the next
// phase's descriptor, the DC symbol), then K1_WCHUNK AC-only steps.  A lane
// that ends its block or its range inside a chunk idles through the chunk's
// remaining steps (no bits, out-of-range stores), so the per-block work costs
// one chunk part per block instead of a share of every step.
FFCV_DEV void locate_block(const int4 pd0, const int4 pd1, uint32_t blk, uint32_t nblocks, int mx, int my,
                           uint32_t &boff, bool &inwin) {
  // pd0 = {base block, blocks per MCU row, hs, mx_lo}, pd1 = {mx_hi, my_lo, my_hi, component}
  inwin = blk < nblocks && mx >= pd0.w && mx <= pd1.x && my >= pd1.y && my <= pd1.z;
  boff = ((uint32_t)pd0.x + __umul24((uint32_t)my, (uint32_t)pd0.y) + __umul24((uint32_t)mx, (uint32_t)pd0.z)) * 64u;
}

// jdhuff.c HUFF_EXTEND of the s extra bits at bit offset off of w (from
// the LSB): branch-free, 0 for s = 0.
FFCV_DEV int huff_value(uint32_t w, uint32_t off, uint32_t s) {
  const uint32_t raw = __builtin_amdgcn_ubfe(w, off, s), msb = __builtin_amdgcn_ubfe(w, off + s - 1, 1);
  return (int)(msb ? raw : raw - ((1u << s) - 1u));
}

typedef __attribute__((address_space(1))) int16_t gshort_t;  // global memory
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// Coefficient stores.  A 2-byte store per non-zero coefficient, scattered
// over the window's blocks, cost ~23% of this kernel (measured without them),
// about in proportion to the lanes that store.  So the AC coefficients at
// zigzag positions below ACS_Z (most of a block's non-zero ones) collect in
// the lane's LDS slot (the event area, dead after the sync pass) and leave as
// three 16-byte stores when the block ends; the rest, and the blocks a lane
// shares with its neighbour (the one it starts inside, the one it stops
// inside: their positions below the split belong to one lane each), are
// stored directly.  The window coefficients were zeroed before this pass, so
// unwritten positions read as zero either way.  Every step issues the same
// vector memory instructions (out-of-range offsets where a lane has nothing
// to store), so the refill waits on a static vmcnt.
template <class TB>
FFCV_DEV void write_range(JShared &S, const TB &T, const uint32_t *words, uint32_t words_bytes, DecState st,
                          uint32_t end_bit, uint32_t blk, gshort_t *coef, uint32_t coef_bytes, gshort_t *dcd,
                          uint32_t dcd_bytes, uint32_t &iters, bool dc_diffs, int &rs0, int &rs1, int &rs2) {
  uint4 *acs = S.acs[threadIdx.x % JT];
  int16_t *acs16 = (int16_t *)acs;
#pragma unroll
  for (int q = 0; q < ACS_BYTES / 16; q++) acs[q] = make_uint4(0, 0, 0, 0);
  bool stg = st.z == 0;  // a block entered part-way is the previous lane's to stage
  BufReader br;
  br.init(words, words_bytes, st.pos);
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void *)coef, 0, (int)coef_bytes, BUF_CFG);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void *)dcd, 0, (int)dcd_bytes, BUF_CFG);
  uint32_t pos = st.pos;
  int z = st.z, ph = st.ph;
  const int bpm = S.bpm, mcux = S.mcux;
  const uint32_t nblocks = (uint32_t)S.nblocks;
  uint32_t dinf = S.phr[ph].dinf, ainf = S.phr[ph].ainf;
  int nph = S.phr[ph].next;
  int m = (int)(blk / bpm);
  int my = m / mcux, mx = m - my * mcux;
  uint32_t boff;
  bool inwin;
  locate_block(S.phr[ph].pd0, S.phr[ph].pd1, blk, nblocks, mx, my, boff, inwin);
  int cc = S.phr[ph].pd1.w;  // component of the block in progress
  int r0 = 0, r1 = 0, r2 = 0;  // running DC sums of the blocks this lane started
  for (;;) {
    K1_DIAG(iters++);
    // ---- chunk part: block boundaries (z >= 64: ended in the last chunk; z == 0: a DC is next)
    br.begin();
    const uint32_t ndinf = S.phr[nph].dinf, nainf = S.phr[nph].ainf;
    const int nnph = S.phr[nph].next;
    const int4 npd0 = S.phr[nph].pd0, npd1 = S.phr[nph].pd1;
    const bool bend = z >= 64;
    {  // a staged block that ended leaves as three 16-byte stores
      const bool fl = bend && stg && inwin;
      // left undefined where the lane does not flush (its stores go out of
      // range): zeroing it cost 12 moves per step
      uint4 c[ACS_BYTES / 16];
      if (fl) {
#pragma unroll
        for (int q = 0; q < ACS_BYTES / 16; q++) {
          c[q] = acs[q];
          acs[q] = make_uint4(0, 0, 0, 0);
        }
      }
      const uint32_t fo = fl ? boff * 2 : BUF_OOR;
#pragma unroll
      for (int q = 0; q < ACS_BYTES / 16; q++)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, c[q]), crs, fo + 16 * q, 0, 0);
    }
    stg = stg || bend;
    // the next block: (blk + 1, nph, mx', my')
    const bool wrap = nph == 0;
    const int nmx = wrap ? (mx + 1 == mcux ? 0 : mx + 1) : mx;
    const int nmy = wrap && mx + 1 == mcux ? my + 1 : my;
    uint32_t nboff;
    bool ninwin;
    locate_block(npd0, npd1, blk + 1, nblocks, nmx, nmy, nboff, ninwin);
    z = bend ? 0 : z;
    blk += bend ? 1 : 0;
    ph = bend ? nph : ph;
    nph = bend ? nnph : nph;
    mx = bend ? nmx : mx;
    my = bend ? nmy : my;
    dinf = bend ? ndinf : dinf;
    ainf = bend ? nainf : ainf;
    boff = bend ? nboff : boff;
    inwin = bend ? ninwin : inwin;
    cc = bend ? npd1.w : cc;
    {  // DC: the difference itself (coefficient output) or this lane's running sum
      const bool isblk = z == 0 && pos < end_bit && blk < nblocks;
      const uint32_t e = decode_entry(T, S.acmask, dinf, br.acc, isblk);
      const int nbits = isblk ? (int)(e & 31) : 0;
      const int v = huff_value((uint32_t)(br.acc >> 32), 32 - nbits, (e >> 5) & 15);
      br.consume(nbits);
      pos += nbits;
      const int rsum = (cc == 0 ? r0 : (cc == 1 ? r1 : r2)) + v;
      r0 = isblk && cc == 0 ? rsum : r0;
      r1 = isblk && cc == 1 ? rsum : r1;
      r2 = isblk && cc == 2 ? rsum : r2;
      if (dc_diffs)
        __builtin_amdgcn_raw_buffer_store_b16((short)v, drs, isblk ? blk * 2 : BUF_OOR, 0, 0);
      else if (isblk && inwin)
        acs16[0] = (int16_t)rsum;  // a DC step starts the block: this lane stages it
      z = isblk ? 1 : z;
    }
    if (!(z > 0 && pos < end_bit)) break;  // nothing left in this lane's range
    // ---- K1_WCHUNK AC-only steps: one refill load and two 2-byte stores each
    // (see BufReader); no block-end work, the lane idles once z >= 64
#pragma unroll
    for (int s = 0; s < K1_WCHUNK; s++) {
      br.begin();
      const bool live = z < 64 && pos < end_bit;
      uint32_t e = decode_entry(T, S.acmask, ainf, br.acc, live);
      e = live ? e : 0u;  // an idle lane: no bits, no advance, sizes 0
      // see make_pair: vs = this step's bits and z advance
      const int zi1 = (int)(e >> 25);
      const bool one = z + zi1 >= 64, pair = zi1 != 0;
      const uint32_t vs = one ? e >> 16 : e;
      const int nbits = (int)(vs & 31), zadd = (int)(vs >> 9) & 127;
      const int t1 = pair ? (int)(e >> 16) & 31 : nbits, zinc = pair ? zi1 : zadd;
      const uint32_t size = (e >> 5) & 15, size2 = pair && !one ? (e >> 21) & 15 : 0u;
      // the extra bits sit in the reader's high word (t1, nbits <= 31)
      const uint32_t hi = (uint32_t)(br.acc >> 32);
      const int v = huff_value(hi, 32 - t1, size), v2 = huff_value(hi, 32 - nbits, size2);
      br.consume(nbits);
      pos += nbits;
      const int p1 = min(z + zinc - 1, 63), p2 = min(z + zadd - 1, 63);
      const uint32_t o1 = (boff + (uint32_t)p1) * 2, o2 = (boff + (uint32_t)p2) * 2;
      const bool a1 = size && inwin, a2 = size2 && inwin;
      const bool l1 = a1 && stg && p1 < ACS_Z, l2 = a2 && stg && p2 < ACS_Z;
      if (l1) acs16[p1] = (int16_t)v;
      if (l2) acs16[p2] = (int16_t)v2;
      // (issuing these under exec masks instead measured 0.6-2% slower: K1's
      // refill would then wait for every pending store, see BufReader)
      __builtin_amdgcn_raw_buffer_store_b16((short)v, crs, a1 && !l1 ? o1 : BUF_OOR, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b16((short)v2, crs, a2 && !l2 ? o2 : BUF_OOR, 0, 0);
      z += zadd;
    }
  }
  rs0 = r0;
  rs1 = r1;
  rs2 = r2;
  if (stg && z > 0 && inwin) {  // stopped inside a staged block: its positions below z are this lane's
    for (int q = 0; q < ACS_Z; q++) {
      const int c = acs16[q];
      if (q < z && c != 0) __builtin_amdgcn_raw_buffer_store_b16((short)c, crs, (boff + (uint32_t)q) * 2, 0, 0);
    }
  }
}

// P0: marker walk over the LDS copy of the header bytes.  With one image per
// wave every lane runs it on wave-uniform (scalar) values: each byte read is
// broadcast to a scalar register, so the walk's branches and arithmetic are
// scalar instead of one lane under an exec mask.
// x / d for x >= 0 and a sampling factor or ratio d in 1..4 (the parse
// rejects anything else): shifts, or a multiply-high for 3, instead of a
// ~25-instruction VALU division sequence (the operands are wave-uniform, so
// these stay on the scalar unit)
FFCV_DEV int dsmall(int x, int d) {
  return d == 3 ? (int)(((uint64_t)(uint32_t)x * 0xAAAAAAABull) >> 33) : x >> (d >> 1);
}

FFCV_DEV int parse_header(JShared &S, const uint8_t *src, uint32_t nbytes, const ffcv_sample &smp_in,
                          const JpegArgs &a, int k_in, int MODE) {
  nbytes = wuni(nbytes);
  const int k = (int)wuni((uint32_t)k_in);
  ffcv_sample smp = smp_in;
  smp.width = wuni(smp_in.width);
  smp.height = wuni(smp_in.height);
  // (p through readfirstlane: the compiler kept the walk's position in a
  // 64-bit vector register pair and branched on it under exec masks, ~20
  // VALU per byte read; uniform, the branch and the address are scalar)
  auto B = [&](uint32_t p) -> int {
    p = wuni(p);
    int v;
    if (p < HDR_BYTES)
      v = S.hdr[p];
    else
      v = gld_u8(src + p);
    return (int)wuni((uint32_t)v);
  };
  auto R16 = [&](uint32_t p) -> int { return (B(p) << 8) | B(p + 1); };
  for (int i = 0; i < 4; i++) S.dqt_ok[i] = 0;
  for (int i = 0; i < NTAB; i++) S.dht_ok[i] = 0;
  S.saw_jfif = S.saw_adobe = 0;
  S.adobe_transform = 1;
  S.restart = 0;
  S.ncomp = 0;
  int have_sof = 0, have_sos = 0;
  if (nbytes < 4 || B(0) != 0xFF || B(1) != 0xD8) return FFCV_SAMPLE_BAD_MARKER;
  uint32_t p = 2;
  while (!have_sos) {
    p = wuni(p);
    if (p + 4 > nbytes || B(p) != 0xFF) return FFCV_SAMPLE_BAD_MARKER;
    while (p < nbytes && B(p) == 0xFF) p++;
    if (p >= nbytes) return FFCV_SAMPLE_BAD_MARKER;
    int m = B(p++);
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (m == 0xD9 || p + 2 > nbytes) return FFCV_SAMPLE_BAD_MARKER;
    int len = R16(p);
    if (len < 2 || p + (uint32_t)len > nbytes) return FFCV_SAMPLE_BAD_MARKER;
    uint32_t s = p + 2;
    int sl = len - 2;
    if (m == 0xDB) {
      int o = 0;
      while (o < sl) {
        int pq = B(s + o) >> 4, tq = B(s + o) & 15;
        // (a table must end inside its segment: jdmarker.c get_dqt's JERR_BAD_LENGTH)
        if (tq > 3 || o + 1 + (pq ? 128 : 64) > sl) return FFCV_SAMPLE_BAD_MARKER;
        S.dqt_off[tq] = s + o + 1;
        S.dqt_prec[tq] = pq;
        S.dqt_ok[tq] = 1;
        o += 1 + (pq ? 128 : 64);
      }
    } else if (m == 0xC4) {
      int o = 0;
      while (o < sl) {
        int tc = B(s + o) >> 4, th = B(s + o) & 15;
        // (the counts, then the symbols, must end inside the segment: get_dht)
        if (th > 3 || tc > 1 || o + 17 > sl) return FFCV_SAMPLE_BAD_MARKER;
        int total = 0;
        for (int l = 0; l < 16; l++) total += B(s + o + 1 + l);
        if (total > 256 || o + 17 + total > sl) return FFCV_SAMPLE_BAD_MARKER;
        S.dht_off[tc * 4 + th] = s + o + 1;
        S.dht_ok[tc * 4 + th] = 1;
        o += 17 + total;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      if (sl < 6) return FFCV_SAMPLE_BAD_MARKER;
      if (B(s) != 8) return FFCV_SAMPLE_UNSUPPORTED;
      S.H = R16(s + 1);
      S.W = R16(s + 3);
      S.ncomp = B(s + 5);
      if (S.ncomp != 1 && S.ncomp != 3) return FFCV_SAMPLE_UNSUPPORTED;
      if (sl < 6 + 3 * S.ncomp) return FFCV_SAMPLE_BAD_MARKER;
      S.hmax = S.vmax = 1;
      for (int c = 0; c < S.ncomp; c++) {
        S.cid[c] = B(s + 6 + 3 * c);
        S.hs[c] = B(s + 7 + 3 * c) >> 4;
        S.vs[c] = B(s + 7 + 3 * c) & 15;
        if (B(s + 8 + 3 * c) > 3) return FFCV_SAMPLE_BAD_MARKER;  // no such table (JERR_NO_QUANT_TABLE)
        S.tq[c] = B(s + 8 + 3 * c);
        if (S.hs[c] < 1 || S.hs[c] > 4 || S.vs[c] < 1 || S.vs[c] > 4) return FFCV_SAMPLE_UNSUPPORTED;
        S.hmax = max(S.hmax, S.hs[c]);
        S.vmax = max(S.vmax, S.vs[c]);
      }
      have_sof = 1;
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return FFCV_SAMPLE_UNSUPPORTED;  // progressive / lossless / arithmetic
    } else if (m == 0xDD) {
      if (sl < 2) return FFCV_SAMPLE_BAD_MARKER;
      S.restart = R16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && B(s) == 'J' && B(s + 1) == 'F' && B(s + 2) == 'I' && B(s + 3) == 'F' && B(s + 4) == 0)
        S.saw_jfif = 1;
    } else if (m == 0xEE) {
      if (sl >= 12 && B(s) == 'A' && B(s + 1) == 'd' && B(s + 2) == 'o' && B(s + 3) == 'b' && B(s + 4) == 'e') {
        S.saw_adobe = 1;
        S.adobe_transform = B(s + 11);
      }
    } else if (m == 0xDA) {
      if (!have_sof) return FFCV_SAMPLE_BAD_MARKER;
      if (sl < 1) return FFCV_SAMPLE_BAD_MARKER;
      int ns = B(s);
      if (ns != S.ncomp) return FFCV_SAMPLE_UNSUPPORTED;  // multi-scan sequential
      if (sl < 1 + 2 * ns) return FFCV_SAMPLE_BAD_MARKER;
      int order[3];
      for (int i = 0; i < ns; i++) {
        int c = -1;
        for (int q = 0; q < S.ncomp; q++)
          if (S.cid[q] == B(s + 1 + 2 * i)) c = q;
        if (c < 0) return FFCV_SAMPLE_BAD_MARKER;
        order[i] = c;
        S.td[c] = B(s + 2 + 2 * i) >> 4;
        S.ta[c] = B(s + 2 + 2 * i) & 15;
        if (S.td[c] > 3 || S.ta[c] > 3) return FFCV_SAMPLE_BAD_MARKER;
      }
      int nb = 0;
      if (S.ncomp == 1) {
        S.blk_comp[0] = order[0];
        S.blk_dx[0] = S.blk_dy[0] = 0;
        nb = 1;
      } else {
        for (int i = 0; i < ns; i++) {
          int c = order[i];
          for (int yy = 0; yy < S.vs[c]; yy++)
            for (int xx = 0; xx < S.hs[c]; xx++) {
              if (nb < 10) {
                S.blk_comp[nb] = c;
                S.blk_dx[nb] = xx;
                S.blk_dy[nb] = yy;
              }
              nb++;
            }
        }
      }
      if (nb > 10) return FFCV_SAMPLE_UNSUPPORTED;
      S.bpm = nb;
      // table slots: AC tables first (they decode most symbols), so they
      // always get a fast LUT
      S.nslots = 0;
      S.dcpack = S.acpack = S.acmask = 0;
      for (int pass = 0; pass < 2; pass++) {
        for (int b = 0; b < nb; b++) {
          int c = S.blk_comp[b];
          int tab = pass == 0 ? 4 + S.ta[c] : S.td[c];
          int sl = -1;
          for (int q = 0; q < S.nslots; q++)
            if (S.slot_tab[q] == tab) sl = q;
          if (sl < 0) {
            sl = S.nslots++;
            S.slot_tab[sl] = tab;
            if (pass == 0) S.acmask |= 1u << sl;
          }
          if (pass == 0)
            S.acpack |= (uint32_t)sl << (3 * b);
          else
            S.dcpack |= (uint32_t)sl << (3 * b);
        }
      }
      // first-level LUT space from the pool, in slot order (AC slots first)
      uint32_t used = 0, nset = 0, nac = 0;
      for (int q = 0; q < S.nslots; q++) {
        uint32_t bits = S.slot_tab[q] >= 4 ? (nac++ ? FB_AC2 : FB_AC) : FB_DC;
        if (used + (1u << bits) > LUT_POOL - 2 || nset == NLUTSLOT) bits = 0;  // canonical decode only
        S.sinfo[q] = si_pack(bits ? used : (uint32_t)(LUT_POOL - 2), bits, (uint32_t)q, bits ? nset : 0u);
        used += bits ? (1u << bits) : 0u;
        nset += bits ? 1u : 0u;
      }
      for (int b = 0; b < nb; b++) {
        S.phr[b].dinf = S.sinfo[slot_of(S.dcpack, b)];
        S.phr[b].ainf = S.sinfo[slot_of(S.acpack, b)];
        S.phr[b].next = b + 1 == nb ? 0 : b + 1;
      }
      S.scan_off = p + (uint32_t)len;
      have_sos = 1;
    }
    p += (uint32_t)len;
  }
  if (S.restart) return FFCV_SAMPLE_UNSUPPORTED;
  if (S.W != (int)smp.width || S.H != (int)smp.height) return FFCV_SAMPLE_GEOMETRY;
  if ((uint32_t)S.W > a.max_w || (uint32_t)S.H > a.max_h) return FFCV_SAMPLE_TOO_LARGE;
  for (int c = 0; c < S.ncomp; c++) {
    if (!S.dqt_ok[S.tq[c]] || !S.dht_ok[S.td[c]] || !S.dht_ok[4 + S.ta[c]]) return FFCV_SAMPLE_BAD_MARKER;
    if (S.hmax % S.hs[c] || S.vmax % S.vs[c]) return FFCV_SAMPLE_UNSUPPORTED;
  }
  if (S.ncomp == 3) {  // jdapimin.c default_decompress_parms colour-space rule
    if (S.saw_jfif)
      S.color_rgb = 0;
    else if (S.saw_adobe)
      S.color_rgb = S.adobe_transform == 0;
    else
      S.color_rgb = S.cid[0] == 82 && S.cid[1] == 71 && S.cid[2] == 66;
  } else {
    S.color_rgb = 0;
  }
  if (S.ncomp == 1) {
    S.cw[0] = dsmall(S.W * S.hs[0] + S.hmax - 1, S.hmax);
    S.ch[0] = dsmall(S.H * S.vs[0] + S.vmax - 1, S.vmax);
    S.mcux = (S.cw[0] + 7) / 8;
    S.mcuy = (S.ch[0] + 7) / 8;
    S.bw[0] = S.mcux;
    S.bh[0] = S.mcuy;
    S.hs[0] = S.vs[0] = 1;  // non-interleaved scan: one block per MCU
    S.hmax = S.vmax = 1;
  } else {
    S.mcux = dsmall((S.W + 8 * S.hmax - 1) >> 3, S.hmax);
    S.mcuy = dsmall((S.H + 8 * S.vmax - 1) >> 3, S.vmax);
    for (int c = 0; c < S.ncomp; c++) {
      S.cw[c] = dsmall(S.W * S.hs[c] + S.hmax - 1, S.hmax);
      S.ch[c] = dsmall(S.H * S.vs[c] + S.vmax - 1, S.vmax);
      S.bw[c] = S.mcux * S.hs[c];
      S.bh[c] = S.mcuy * S.vs[c];
    }
  }
  S.nblocks = S.mcux * S.mcuy * S.bpm;
  if (MODE == JM_COEF && (uint64_t)S.nblocks > a.max_blocks) return FFCV_SAMPLE_TOO_LARGE;
  if (MODE == JM_RRC) {
    // vector loads (the fused draws wrote the crop with vector stores in this
    // kernel; a scalar load at this uniform address could hit a stale K$ line)
    auto crop = [&](int i) {
      return (int)wuni((uint32_t)__builtin_nontemporal_load((const __attribute__((address_space(1))) int32_t *)a.crops + 4 * k + i));
    };
    S.ri = crop(0);
    S.rj = crop(1);
    S.rh = crop(2);
    S.rw = crop(3);
    if (S.rh <= 0 || S.rw <= 0 || S.ri < 0 || S.rj < 0 || S.ri + S.rh > S.H || S.rj + S.rw > S.W)
      return FFCV_SAMPLE_GEOMETRY;
  } else {
    S.ri = 0;
    S.rj = 0;
    S.rh = S.H;
    S.rw = S.W;
  }
  for (int c = 0; c < S.ncomp; c++) {  // blocks the crop reads (+1 sample of fancy context)
    int he = dsmall(S.hmax, S.hs[c]), ve = dsmall(S.vmax, S.vs[c]);
    int y0 = dsmall(S.ri, ve) - (ve == 2 ? 1 : 0), y1 = dsmall(S.ri + S.rh - 1, ve) + (ve == 2 ? 1 : 0);
    int x0 = dsmall(S.rj, he) - (he == 2 ? 1 : 0), x1 = dsmall(S.rj + S.rw - 1, he) + (he == 2 ? 1 : 0);
    y0 = max(y0, 0);
    x0 = max(x0, 0);
    y1 = min(y1, S.ch[c] - 1);
    x1 = min(x1, S.cw[c] - 1);
    if (MODE == JM_COEF) {
      y0 = x0 = 0;
      y1 = S.bh[c] * 8 - 1;
      x1 = S.bw[c] * 8 - 1;
    }
    S.wy0[c] = y0 >> 3;
    S.wy1[c] = y1 >> 3;
    S.wx0[c] = x0 >> 3;
    S.wx1[c] = x1 >> 3;
  }
  uint32_t nwin = 0;  // coefficients / planes are stored for the window only
  for (int c = 0; c < S.ncomp; c++) {
    S.coff[c] = nwin;
    nwin += (uint32_t)((S.wx1[c] - S.wx0[c] + 1) * (S.wy1[c] - S.wy0[c] + 1));
  }
  S.nwin = nwin;
  for (int b = 0; b < S.bpm; b++) {
    int c = S.blk_comp[b], dx = S.blk_dx[b], dy = S.blk_dy[b], hs = S.hs[c], vs = S.vs[c];
    // bx = mx * hs + dx in [wx0, wx1]  <=>  mx in [mx_lo, mx_hi]
    int mxl = S.wx0[c] - dx <= 0 ? 0 : dsmall(S.wx0[c] - dx + hs - 1, hs);
    int mxh = S.wx1[c] - dx < 0 ? -1 : dsmall(S.wx1[c] - dx, hs);
    int myl = S.wy0[c] - dy <= 0 ? 0 : dsmall(S.wy0[c] - dy + vs - 1, vs);
    int myh = S.wy1[c] - dy < 0 ? -1 : dsmall(S.wy1[c] - dy, vs);
    // window-relative index of block (mx * hs + dx, my * vs + dy) is
    // base + my * (vs * wbw) + mx * hs (base may be negative: only window
    // blocks are ever addressed, and the sum wraps back in 32 bits)
    const int wbw = S.wx1[c] - S.wx0[c] + 1;
    S.phr[b].pd0 = make_int4((int)S.coff[c] + (dy - S.wy0[c]) * wbw + (dx - S.wx0[c]), vs * wbw, hs, mxl);
    S.phr[b].pd1 = make_int4(mxh, myl, myh, c);  // .w: the phase's component (write pass DC sums)
  }
  return FFCV_SAMPLE_OK;
}

// P1: Huffman decode tables for the table slots of image R (jdhuff.c
// jpeg_make_d_derived_tbl, including its table checks), by NT threads: the
// workgroup into its shared LDS copy, or one wave into its own global copy.
template <int NT, class TB, class HBF>
FFCV_DEV void build_tables(TB &T, const JShared &R, const HBF &HB, int tid) {
  auto bar = [&]() {
    if constexpr (NT == JT)
      wsync_mem();
    else
      __syncthreads();
  };
  const int nslots = R.nslots;
  if (tid == 0) T.bad = 0;
  bar();
  if (tid < nslots) {
    const int tab = R.slot_tab[tid];
    const uint32_t d = R.dht_off[tab];
    uint32_t code = 0;
    int kk = 0;
    bool bad = false;
    for (int l = 1; l <= 16; l++) {
      int nl = HB(d + l - 1);
      T.valoff[tid][l] = kk - (int)code;
      code += nl;
      kk += nl;
      if (code >= (1u << l)) bad = true;  // over-subscribed (or all-ones) code space
      T.lim[tid][l] = code << (16 - l);
      code <<= 1;
    }
    T.nvals[tid] = kk;
    if (bad) T.bad = 1;
    T.nsub[tid] = 0;
  }
  bar();
  for (int s2 = 0; s2 < nslots; s2++) {
    const int tab = R.slot_tab[s2];
    const uint32_t d = R.dht_off[tab];
    for (int i = tid; i < T.nvals[s2]; i += NT) {
      int v = HB(d + 16 + i);
      if (tab < 4 && v > 15) T.bad = 1;  // DC sizes are 0..15
      T.vals[s2][i] = (uint8_t)v;
    }
  }
  if (tid < 2) T.lut[LUT_POOL - 2 + tid] = 0;  // the zero words of LUT-less slots
  bar();
  for (int s = 0; s < nslots; s++) {
    const uint32_t inf = R.sinfo[s];
    const int bits = si_bits(inf);
    if (!bits) continue;
    const bool ac = (R.acmask >> s) & 1;
    uint32_t L[FB_AC + 1];
#pragma unroll
    for (int l = 1; l <= FB_AC; l++) L[l] = T.lim[s][l];
    for (int v = tid; v < (1 << bits); v += NT) {
      const uint32_t look = (uint32_t)v << (16 - bits);
      int len = 1;
#pragma unroll
      for (int l = 1; l < FB_AC; l++) len += (l < bits && look >= L[l]) ? 1 : 0;
      uint32_t e = 0;
      if (look < T.lim[s][len]) {
        int sym = T.vals[s][(T.valoff[s][len] + (int)(look >> (16 - len))) & 0xff];
        e = make_entry(ac, len, sym);
      } else if (look < T.lim[s][16]) {  // codes longer than `bits` under this prefix
        int n = atomicAdd(&T.nsub[s], 1);
        if (n < NSUB) {
          T.sub_prefix[s][n] = (uint16_t)v;
          e = (uint32_t)(n + 1) << 5;
        }
      }
      if (ac && e) e = make_pair(T, s, bits, L, look, e);
      T.lut[si_base(inf) + v] = e;
    }
  }
  bar();
  for (int i = tid; i < NSLOT * NSUB * (1 << SUBB); i += NT) {
    const int s = i / (NSUB << SUBB), n = (i >> SUBB) % NSUB, x = i & ((1 << SUBB) - 1);
    if (s >= nslots || n >= min(T.nsub[s], NSUB)) continue;
    const int bits = si_bits(R.sinfo[s]);
    const uint32_t look = ((uint32_t)T.sub_prefix[s][n] << (16 - bits)) | ((uint32_t)x << (16 - bits - SUBB));
    int len = 1;
    for (int l = 1; l < 16; l++) len += look >= T.lim[s][l];
    T.lut2[si_set(R.sinfo[s])][n][x] = len <= bits + SUBB ? (uint16_t)slow_entry(T, R.acmask, s, look) : (uint16_t)0;
  }
  bar();
}

// P3-P5 with table set T (the workgroup's LDS copy or the image's global
// copy; separate instantiations so each reads its own address space).
// Entropy index record of one sample: EIDX_WORDS words per lane range t >= 1,
// [pos, z | ph << 8, first block].  Lane 0's range always starts at (0, 0, 0),
// so its words carry [hash high, EIDX_VALID | nthr << 16, hash low]: a 64-bit
// hash of the other lanes' words.  Records are written and read with plain
// memory operations and no fences (an agent-scope release / acquire writes
// back / invalidates the whole L2 of the XCD): a record is used only when its
// hash matches, so a reader that sees part of a record being published by a
// concurrent launch on another XCD (lines not yet written back) decodes the
// sample in full instead.  A record's content is a pure function of the
// sample, so every publish writes the same words.
#define EIDX_LANES 64
static_assert(EIDX_LANES == JT, "an entropy index record holds one state per lane of K1's wave");
#define EIDX_WORDS 3
#define EIDX_VALID 0x80000000u
FFCV_DEV uint64_t eidx_hash(uint32_t w0, uint32_t w1, uint32_t w2, int t) {
  // per lane mix, then an xor over the wave (wave-uniform result)
  uint64_t h = ((uint64_t)w0 << 32 | w1) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)w2 << 32 | (uint32_t)t) * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 29;
  uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    lo ^= (uint32_t)__shfl_xor((int)lo, m);
    hi ^= (uint32_t)__shfl_xor((int)hi, m);
  }
  return ((uint64_t)hi << 32) | lo;
}
// Zero the image's window coefficients right before the write pass stores
// its non-zero ones: the lines are then still in L2 when the scattered 2-byte
// stores and the IDCT's block reads reach them (zeroed at allocation, ~300 us
// earlier, they had been written back and the stores missed).
FFCV_DEV void zero_window_coefs(const JShared &S, int16_t *coef, int t) {
  K1_SKIP_ZEROING;  // diagnostics (wrong pixels): the zeroing's share of K1's traffic and time
  // (buffer stores: no flat_store, which would also count in lgkmcnt)
  const __amdgpu_buffer_rsrc_t zrs =
      __builtin_amdgcn_make_buffer_rsrc(wave_uniform((void *)coef), 0, (int)wuni(S.cf_bytes), BUF_CFG);
  const uint32_t n = wuni((uint32_t)(S.nwin * 8));
  for (uint32_t i = (uint32_t)t; i < n; i += JT)
    __builtin_amdgcn_raw_buffer_store_b128((u32x4_t){0u, 0u, 0u, 0u}, zrs, 16 * i, 0, 0);
  wsync_mem();
}

template <class TB>
FFCV_DEV bool entropy_passes(JShared &S, const TB &T, const JpegArgs &a, int k, int t, const uint32_t *words,
                             uint32_t total_bits, int16_t *coef, int16_t *dcd, uint64_t sample_id, bool dc_diffs) {
  int rs0 = 0, rs1 = 0, rs2 = 0;
  uint32_t start_blk = 0;  // first block this lane starts
  // each lane's DC offsets and start block for jpeg_idct_kernel (non-coefficient modes)
  auto publish_dc = [&]() {
    if (dc_diffs) return;
    const int o0 = wave_exscan_i(rs0), o1 = wave_exscan_i(rs1), o2 = wave_exscan_i(rs2);
    ImgInfo *info = a.info + k;
    info->lane_blk0[t] = start_blk;
    info->lane_off[0][t] = o0;
    info->lane_off[1][t] = o1;
    info->lane_off[2][t] = o2;
  };
  // ---------------------------------------------------- decode extent ----
  // A baseline stream is sequential: the blocks up to the end of the last MCU
  // row that holds a window block are needed (block boundaries, DC sums), the
  // rest of the scan is not.  need_blocks is that prefix in MCU order; the
  // lane ranges are laid over [0, ext), the linear estimate of its end plus a
  // margin (K1_EXT_*), instead of the whole stream.  The estimate is checked
  // once the rounds have converged (P4), and a prefix that fell short is
  // decoded again over the full extent.  A sample with an entropy index
  // record is always decoded in full: a record holds the lane states of the
  // full partition and later epochs skip the sync rounds with it.
  uint32_t *rec = nullptr;
  if (a.eidx && sample_id < a.eidx_n) rec = a.eidx + sample_id * (EIDX_LANES * EIDX_WORDS);
  const uint32_t nblocks = wuni((uint32_t)S.nblocks);
  int my_last = 0;  // last MCU row with a window block
  for (int c = 0; c < S.ncomp; c++) my_last = max(my_last, dsmall(S.wy1[c], S.vs[c]));
  const uint32_t need_rows = wuni((uint32_t)my_last + 1u);
  const uint32_t need_blocks = min(nblocks, need_rows * wuni((uint32_t)(S.mcux * S.bpm)));
  uint32_t ext = total_bits;
  if (need_blocks < nblocks && !rec && K1_EXT_REL < 256) {
    const uint32_t est = total_bits / wuni((uint32_t)S.mcuy) * need_rows;
    ext = min(total_bits, est + (total_bits >> 8) * K1_EXT_REL + K1_EXT_ABS);
  }
  bool fell_back = false;
  uint32_t nthr, cbits, my_end;
  bool active;
  auto lay_ranges = [&]() {  // up to JT lane ranges of >= 192 bits over [0, ext)
    nthr = (ext + 191) / 192;
    nthr = max(1u, min(nthr, (uint32_t)JT));
    cbits = (ext + nthr - 1) / nthr;
    active = t < (int)nthr;
    my_end = active ? (t == (int)nthr - 1 ? ext : min(ext, (t + 1) * cbits)) : 0;
  };
  lay_ranges();
  // ---------------------------------------------------- entropy index ----
  if (rec) {
    const uint32_t w0 = __builtin_nontemporal_load(rec + EIDX_WORDS * t);
    const uint32_t w1 = __builtin_nontemporal_load(rec + EIDX_WORDS * t + 1);
    const uint32_t w2 = __builtin_nontemporal_load(rec + EIDX_WORDS * t + 2);
    const uint32_t head = __builtin_amdgcn_readfirstlane(w1);
    const uint64_t want = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(w0) << 32) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(w2);
    const uint64_t got = eidx_hash(t ? w0 : 0u, t ? w1 : 0u, t ? w2 : 0u, t);
    if ((head & EIDX_VALID) && ((head >> 16) & 0xff) == nthr && wuni((uint32_t)(got == want))) {
      // published by an earlier decode of this sample: every lane starts
      // from its exact state (no sync rounds, no block scan)
      STAMP(3);
      STAMP(4);
      STAMP(5);
      if (a.dbg && t == 0) a.dbg[(uint64_t)k * 16 + 12] = ~0ull;  // index hit: no sync rounds
      zero_window_coefs(S, coef, t);
      if (active) {
        DecState g;
        g.pos = t ? w0 : 0u;
        g.z = t ? (int)(w1 & 0xff) : 0;
        g.ph = t ? (int)((w1 >> 8) & 0xff) : 0;
        const uint32_t cur = t ? w2 : 0u;
        start_blk = g.z == 0 ? cur : cur + 1;
        uint32_t it_lane2 = 0;
        if (g.pos < my_end)
          write_range(S, T, words, wuni(S.ds_bytes), g, my_end, cur, wave_uniform((gshort_t *)coef),
                      wuni(S.cf_bytes), wave_uniform((gshort_t *)dcd), wuni(S.dc_bytes), it_lane2, dc_diffs, rs0,
                      rs1, rs2);
      } else {
        start_blk = (uint32_t)S.nblocks;
      }
      publish_dc();
      return false;
    }
  }
  // ------------------------------------------------------------- P3 ----
  STAMP(3);
  DecState g, e;
  uint32_t my_cnt, blk_base;
  int my_nev, my_cb, my_eb;  // events: count, buffer, block count of slot 0
  uint32_t it_lane = 0, it_wave = 0;  // diagnostics: loop iterations (max over lanes per round)
  int rounds = 0;
  bool any_bad;
  // (a loop: run once, and once more over the whole stream when [0, ext) held
  // fewer than need_blocks blocks; the rounds write only LDS events and
  // registers, the write pass starts after the coverage check)
  for (;;) {
    g.pos = active ? t * cbits : 0;
    g.z = 0;
    g.ph = 0;
    my_cnt = 0;
    my_nev = my_cb = my_eb = 0;
    e = g;
    // event stride: NEV events spread over a lane's expected block count
    const uint32_t exp_blocks = ext == total_bits ? nblocks : min(nblocks, ext / max(1u, total_bits / nblocks));
    const uint32_t evq = (exp_blocks / nthr + NEV) / NEV;
    const int esh = evq <= 1 ? 0 : 32 - __clz((int)(evq - 1));
    if (active) e = sync_range<false>(S, T, words, g, my_end, t, my_cnt, my_nev, my_cb, my_eb, g, esh, it_lane);
    if (a.dbg) it_wave += __reduce_max_sync(~0ull, it_lane);
    for (;;) {
      DecState ng;
      ng.pos = lane_prev0(e.pos, t);
      ng.z = (int)lane_prev0((uint32_t)e.z, t);
      ng.ph = (int)lane_prev0((uint32_t)e.ph, t);
      const bool changed = active && t > 0 && (ng.pos != g.pos || ng.z != g.z || ng.ph != g.ph);
      if (!__any(changed)) break;
      rounds++;
      if (changed) {
        g = ng;
        if (g.pos >= my_end) {
          e = g;
          my_cnt = 0;
          my_nev = 0;
          my_eb = 0;
        } else {
          it_lane = 0;
          e = sync_range<true>(S, T, words, g, my_end, t, my_cnt, my_nev, my_cb, my_eb, e, esh, it_lane);
        }
      }
      if (a.dbg) it_wave += __reduce_max_sync(~0ull, changed ? it_lane : 0u);
    }
    if (!active) my_cnt = 0;

    // ----------------------------------------------------------- P4 ----
    STAMP(4);
    blk_base = wave_exscan(my_cnt);
    bool bad_lane = false;
    if (active) {
      int64_t cur = g.z == 0 ? (int64_t)blk_base : (int64_t)blk_base - 1;
      bad_lane = cur < 0 || (cur % S.bpm) != g.ph;  // inconsistent stream
    }
    // Blocks completed in [0, ext): those started, less the one the last lane
    // range left unfinished (the pad bits of a whole stream may start one
    // block more).  Fewer than need_blocks over a shortened extent: the
    // estimate fell short, decode the whole stream.  Fewer over the whole
    // stream (truncated data, an early marker) is a corrupt stream: libjpeg
    // pads it with zero bits and leaves the remaining MCUs grey, this path
    // reports it.
    const uint32_t nstarted = lane_read(blk_base + my_cnt, JT - 1);
    const uint32_t zlast = lane_read((uint32_t)e.z, (int)wuni(nthr - 1));
    const bool is_short = nstarted - (zlast != 0 ? 1u : 0u) < need_blocks;
    any_bad = __ballot(bad_lane) != 0 || is_short;
    if (!is_short || ext == total_bits) break;
    ext = total_bits;
    fell_back = true;
    lay_ranges();
  }
  if (a.dbg && t == 0) {
    a.dbg[(uint64_t)k * 16 + 12] = (uint64_t)rounds;
    // nthr, whether the full-extent pass had to follow, the extent decoded
    a.dbg[(uint64_t)k * 16 + 13] = (uint64_t)nthr | (fell_back ? 0x100ull : 0ull) | (uint64_t)ext << 32;
    a.dbg[(uint64_t)k * 16 + 14] = (uint64_t)it_wave;
  }
  if (rec && !any_bad) {  // publish this sample's converged lane states
    const int64_t cur = g.z == 0 ? (int64_t)blk_base : (int64_t)blk_base - 1;
    uint32_t w0 = active ? g.pos : 0u, w1 = active ? (uint32_t)g.z | ((uint32_t)g.ph << 8) : 0u,
             w2 = active ? (uint32_t)cur : 0u;
    const uint64_t h = eidx_hash(t ? w0 : 0u, t ? w1 : 0u, t ? w2 : 0u, t);
    if (t == 0) {  // lane 0's state is (0, 0, 0): its words carry the header and hash
      w0 = (uint32_t)(h >> 32);
      w1 = EIDX_VALID | (nthr << 16);
      w2 = (uint32_t)h;
    }
    rec[EIDX_WORDS * t] = w0;
    rec[EIDX_WORDS * t + 1] = w1;
    rec[EIDX_WORDS * t + 2] = w2;
  }

  // ------------------------------------------------------------- P5 ----
  STAMP(5);
  K1_STOP_AT(4, nthr != 0x7fffffffu, any_bad);  // diagnostics: K1 up to the sync pass (no write pass)
  zero_window_coefs(S, coef, t);
  uint32_t it_lane2 = 0;
  start_blk = blk_base;
  if (active && g.pos < my_end) {
    int64_t cur = g.z == 0 ? (int64_t)blk_base : (int64_t)blk_base - 1;
    if (cur >= 0)
      write_range(S, T, words, wuni(S.ds_bytes), g, my_end, (uint32_t)cur, wave_uniform((gshort_t *)coef),
                  wuni(S.cf_bytes), wave_uniform((gshort_t *)dcd), wuni(S.dc_bytes), it_lane2, dc_diffs, rs0, rs1,
                  rs2);
  }
  publish_dc();
  if (a.dbg) {
    const uint32_t wmax = __reduce_max_sync(~0ull, it_lane2);
    if (t == 0) a.dbg[(uint64_t)k * 16 + 15] = (uint64_t)wmax;
  }

  return any_bad;
}

// Bump-allocate this image's regions of the launch arena (wave-uniform; lane
// 0 does the atomic) and zero its window coefficients (the write pass stores
// only non-zero coefficients).  Region sizes: de-stuffed stream + padding,
// window coefficients (int16 x 64 per block), DC differences (int16 per
// block, coefficient output only), window planes (64 B per block), K2 band
// staging (crop RGB).
FFCV_DEV uint64_t align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
FFCV_DEV int alloc_scratch(JShared &S, const JpegArgs &a, uint32_t nbytes, int t, int MODE, int k) {
  const uint64_t ds = align256((uint64_t)nbytes + 64), cf = align256((uint64_t)S.nwin * 128);
  // DC differences are stored only for the coefficient output (the other
  // modes predict DC from the write pass's per-lane running sums)
  const uint64_t dc = MODE == JM_COEF ? align256((uint64_t)S.nblocks * 2) : 0, pl = align256((uint64_t)S.nwin * 64);
  const uint64_t rgb = MODE == JM_RRC ? align256((uint64_t)S.rh * S.rw * 3) : 0;
  const uint64_t need = ds + cf + dc + pl + rgb;
  // An image larger than the whole arena reserves nothing (a 2400x1800 image
  // decoded first, largest-first, would otherwise hold the arena whenever its
  // give-back below loses the race, failing every image of the launch).  A
  // check against the live counter measured -1.5% (one more memory round
  // trip before the workgroup barrier).
  if (need > a.arena_bytes) {
    if (t == 0) a.info[k].arena_need = 0;
    return FFCV_SAMPLE_TOO_LARGE;
  }
  unsigned long long base = 0;
  if (t == 0) base = atomicAdd(a.arena_top, (unsigned long long)need);
  // readfirstlane returns int: widen through uint32_t (an offset at or past
  // 2^31 would otherwise sign-extend and read as TOO_LARGE)
  base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)base);
  if (base + need > a.arena_bytes) {
    // Arena exhausted.  Give the space back only if no reservation was made
    // after this one (the counter still ends at this image's region): a
    // compare-and-swap from base + need to base.  A plain subtract (round 3)
    // lowered the counter below a later image's live region whenever two
    // failures interleaved with a success, and the next image was handed
    // overlapping scratch.  When the swap fails the region stays reserved
    // (unused): the counter never goes below a live region.
    if (t == 0) {
      atomicCAS(a.arena_top, (unsigned long long)(base + need), (unsigned long long)base);
      a.info[k].arena_need = 0;
    }
    return FFCV_SAMPLE_TOO_LARGE;
  }
  if (t == 0) {
    a.info[k].arena_base = base;
    a.info[k].arena_need = need;
  }
  S.ds_off = base;
  S.ds_bytes = (uint32_t)ds;
  S.cf_off = base + ds;
  S.cf_bytes = (uint32_t)cf;
  S.dc_off = S.cf_off + cf;
  S.dc_bytes = (uint32_t)dc;
  const uint64_t pl_off = S.dc_off + dc;
  S.rgb_off = pl_off + pl;
  uint64_t o = pl_off;
  for (int c = 0; c < S.ncomp; c++) {
    const uint64_t wstride = (uint64_t)(S.wx1[c] - S.wx0[c] + 1) * 8;
    S.poff[c] = o - ((uint64_t)S.wy0[c] * 8 * wstride + (uint64_t)S.wx0[c] * 8);  // wraps: see ImgInfo
    o += wstride * (uint64_t)(S.wy1[c] - S.wy0[c] + 1) * 8;
  }
  return FFCV_SAMPLE_OK;
}

// K1 workgroup order: a workgroup's waves decode JW images and its LDS is
// held until the slowest one is done, so images of similar stream length
// (the best predictor of an image's K1 time) are grouped together: a
// one-workgroup counting sort of the batch by compressed size in 1 KB
// buckets, largest first, so the launch's last workgroups (its tail, which
// K1b and K2 wait for) hold its smallest images.  Only which wave decodes
// which image changes: every image is decoded the same way, and its outputs
// stay at its own index.
#define K1O_NB 128
#define K1O_T 1024
#define K1O_PER 16  // images per thread held in registers: launches up to 16,384 images in one pass
__global__ void __launch_bounds__(K1O_T) k1_order_kernel(JpegArgs a, uint32_t *order) {
  __shared__ uint32_t cnt[K1O_NB];
  const int t = threadIdx.x;
  if (t < K1O_NB) cnt[t] = 0;
  auto bucket_of = [](uint64_t size) -> int {
    return K1O_NB - 1 - (int)min<uint64_t>(size >> 10, K1O_NB - 1);
  };
  auto size_of = [&](int k) -> uint64_t {
    if (a.table) {
      const uint64_t id = a.ids[k];
      return id < a.n_table ? a.table[id].size : 0;
    }
    return a.samples[k].size;
  };
  // (round 4) every image's sample id, then its size, loaded with all of a
  // thread's images in flight, the buckets kept in registers for both passes:
  // the round-3 loop issued two dependent loads per image per pass in series
  // (~50-70 us per 12,288-image launch, ahead of every K1)
  uint64_t ids[K1O_PER];
#pragma unroll
  for (int i = 0; i < K1O_PER; i++) {
    const int k = t + i * K1O_T;
    ids[i] = a.table && k < a.batch ? a.ids[k] : 0;
  }
  int bk[K1O_PER];
#pragma unroll
  for (int i = 0; i < K1O_PER; i++) {
    const int k = t + i * K1O_T;
    uint64_t size = 0;
    if (k < a.batch) size = a.table ? (ids[i] < a.n_table ? a.table[ids[i]].size : 0) : a.samples[k].size;
    bk[i] = bucket_of(size);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K1O_PER; i++)
    if (t + i * K1O_T < a.batch) atomicAdd(&cnt[bk[i]], 1u);
  for (int k = t + K1O_PER * K1O_T; k < a.batch; k += K1O_T) atomicAdd(&cnt[bucket_of(size_of(k))], 1u);
  __syncthreads();
  if (t < 64) {  // exclusive scan of the 128 bucket counts: one wave, two counts per lane
    const uint32_t c0 = cnt[2 * t], c1 = cnt[2 * t + 1];
    uint32_t x = c0 + c1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (t >= d) x += y;
    }
    const uint32_t ex = x - c0 - c1;
    cnt[2 * t] = ex;
    cnt[2 * t + 1] = ex + c0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K1O_PER; i++) {
    const int k = t + i * K1O_T;
    if (k < a.batch) order[atomicAdd(&cnt[bk[i]], 1u)] = (uint32_t)k;
  }
  for (int k = t + K1O_PER * K1O_T; k < a.batch; k += K1O_T) order[atomicAdd(&cnt[bucket_of(size_of(k))], 1u)] = (uint32_t)k;
}

template <int MODE>
// Waves per SIMD K1 is compiled for: 4 (= the LDS limit, 16 images per CU)
// caps it at 128 VGPRs (a few spill, outside the decode loops); measured
// 1-2% faster than 3 (143 VGPRs) in the full pipeline.
#ifndef K1_WPE
#define K1_WPE 4
#endif
__global__ void __launch_bounds__(JW * JT) __attribute__((amdgpu_waves_per_eu(K1_WPE))) jpeg_entropy_kernel(JpegArgs a) {
  __shared__ K1Shared KS;
  const int wi = threadIdx.x / JT;  // image within the workgroup
  const int t = threadIdx.x % JT;   // lane within the image's wave
  const int slot = blockIdx.x * JW + wi;
  const int k = a.k1_order && slot < a.batch ? (int)wuni(a.k1_order[slot]) : slot;
  JShared &S = KS.w[wi];
  const bool have = k < a.batch;
  ffcv_sample smp = {};
  int rng_err = 0;
  // The workgroup's draws (draw_kernel fused): all in wave 0, lane 3 w + part
  // for image w, so the MT19937 seeding chain runs once per workgroup instead
  // of once per wave; the crops are read by every wave's parse after the
  // barrier that follows the header staging (a workgroup fence: same CU)
  __shared__ int s_rngerr[JW];
  if (a.table && a.do_draw) {
    if (threadIdx.x < JT) {
      int err = 0;
      if (threadIdx.x < 3 * JW) {
        const int w = threadIdx.x / 3, part = threadIdx.x % 3;
        const int sw = blockIdx.x * JW + w;
        const int kw = a.k1_order && sw < a.batch ? (int)a.k1_order[sw] : sw;
        if (kw < a.batch) {
          const uint64_t idw = a.ids[kw];
          const uint32_t hw = idw < a.n_table ? a.table[idw].height : 1u, ww = idw < a.n_table ? a.table[idw].width : 1u;
          err = draw_part(part, kw, idw, hw, ww, a.dp, a.crops_w, a.cut_w, a.flips_w);
        }
      }
      const uint64_t eb = __ballot(err != 0);
      if (threadIdx.x < JW) s_rngerr[threadIdx.x] = ((eb >> (3 * threadIdx.x)) & 7ull) != 0;
    }
  }
  if (have) {
    if (a.table) {  // fused gather (gather_samples_kernel)
      const uint64_t id = a.ids[k];
      if (id < a.n_table) {
        smp = a.table[id];
      } else {  // out-of-range index: an empty jpg sample -> BAD_MARKER status
        smp.height = smp.width = 1;
      }
      if (t == 0 && a.samples_out) a.samples_out[k] = smp;
    } else {
      smp = a.samples[k];
    }
  }
  ImgInfo *info = a.info + k;
  const bool live = have && smp.mode == 0;
  if (have && smp.mode != 0 && t == 0) {  // raw samples are handled by rrc_raw_kernel / gather
    a.status[k] = FFCV_SAMPLE_OK;
    info->status = -1;  // K2 skips
  }
  K1_STOP_ONLY(if (have && t == 0) info->status = -1);  // diagnostics: K1b / K2 skip (K1 stops before writing the record)
  // no reservation until alloc_scratch makes one: an image that fails before
  // it (draws, parse, raw) must not report the previous launch's region
  // (ffcv_jpeg_arena_regions)
  if (have && t == 0) info->arena_need = 0;
  const uint8_t *src = wave_uniform(a.base + smp.offset);
  const uint32_t nbytes = wuni((uint32_t)smp.size);  // uniform: sizes buffer resources
  auto fail = [&]() {
    if (t == 0) {
      a.status[k] = S.status;
      info->status = S.status;
    }
    if (MODE == JM_FULL) {  // zero-fill (K2 does it for RRC)
      uint64_t bytes = (uint64_t)smp.height * smp.width * 3;
      uint8_t *o = (uint8_t *)a.out + a.out_stride * k;
      for (uint64_t i = t; i < bytes && i < a.out_stride; i += JT) o[i] = 0;
    }
    if (MODE == JM_COEF) {  // the image's whole row of blocks
      uint4 *o = (uint4 *)((uint8_t *)a.out + a.out_stride * k);
      for (uint64_t i = t; i < a.out_stride / 16; i += JT) o[i] = make_uint4(0, 0, 0, 0);
    }
  };

  // ------------------------------------------------------------- P0 ----
  STAMP(0);
  if (live) {
    // aligned dword loads (one batch per lane), bytes scattered into LDS
    const uint32_t nh = min(nbytes, (uint32_t)HDR_BYTES);
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3);
    const uint32_t *aw = (const uint32_t *)(src - mis);
    constexpr int NW = (HDR_BYTES + 4) / 4;
#pragma unroll
    for (int r = 0; r < (NW + JT - 1) / JT; r++) {
      const int i = r * JT + t;
      const int b0 = 4 * i - (int)mis;
      const uint32_t w = i < NW && b0 < (int)nh ? gld_u32(aw + i) : 0u;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int idx = b0 + j;
        if (idx >= 0 && idx < HDR_BYTES) S.hdr[idx] = idx < (int)nh ? (uint8_t)(w >> (8 * j)) : 0;
      }
    }
  }
  if (a.table && a.do_draw) {  // the draws (wave 0) are done; waves 1.. staged their headers meanwhile
    __syncthreads();
    rng_err = s_rngerr[wi];
  } else {
    wsync_lds();
  }
  STAMP(10);
  K1_STOP_AT(7, smp.size != 0x7fffffffffffull);  // diagnostics: gather, draws and header staging
  if (t == 0) S.src = src;
  {  // the whole wave runs the (scalar) parse; see parse_header
    int st = live ? (rng_err ? FFCV_SAMPLE_RNG : parse_header(S, wave_uniform(src), nbytes, smp, a, k, MODE)) : -1;
    if (st == FFCV_SAMPLE_OK) st = alloc_scratch(S, a, nbytes, t, MODE, k);
    if (t == 0) S.status = st;
  }
  __syncthreads();

  K1_STOP_AT(8, smp.size != 0x7fffffffffffull);  // diagnostics: up to the parse and the scratch allocation
  // ------------------------------------------------------------- P1 ----
  // The workgroup's first valid image provides the shared tables; every
  // image whose table slots and DHT bytes equal that image's uses them.
  STAMP(1);
  int ref = -1;
#pragma unroll
  for (int w = JW - 1; w >= 0; w--)
    if (KS.w[w].status == FFCV_SAMPLE_OK) ref = w;
  bool match = false;
  if (ref >= 0 && S.status == FFCV_SAMPLE_OK) {
    const JShared &R = KS.w[ref];
    const uint8_t *rsrc = R.src;
    match = R.nslots == S.nslots;
    for (int q = 0; q < NSLOT; q++)
      if (q < R.nslots && R.slot_tab[q] != S.slot_tab[q]) match = false;
    if (match && ref != wi) {
      bool diff = false;
      for (int q = 0; q < R.nslots; q++) {
        const uint32_t dr = R.dht_off[R.slot_tab[q]], ds = S.dht_off[S.slot_tab[q]];
        auto hb = [](const JShared &X, const uint8_t *xs, uint32_t p) -> int {
          return p < HDR_BYTES ? X.hdr[p] : gld_u8(xs + p);
        };
        int total = 0;
        for (int l = 0; l < 16; l++) total += hb(S, src, ds + l);
        for (int i = t; i < 16 + total; i += JT) diff |= hb(S, src, ds + i) != hb(R, rsrc, dr + i);
      }
      match = __ballot(diff) == 0;
    }
  }
  if (ref >= 0) {
    const JShared &R = KS.w[ref];
    const uint8_t *rsrc = R.src;
    auto HBR = [&](uint32_t p) -> int { return p < HDR_BYTES ? (int)R.hdr[p] : (int)gld_u8(rsrc + p); };
    build_tables<JW * JT>(KS.tab, R, HBR, (int)threadIdx.x);
  }
  // (no workgroup barrier below this point: each wave runs on its own)
  if (!live) return;
  if (S.status != FFCV_SAMPLE_OK) {
    fail();
    return;
  }
  auto HB = [&](uint32_t p) -> int {
    int v;
    if (p < HDR_BYTES)
      v = S.hdr[p];
    else
      v = gld_u8(src + p);
    return v;
  };
  JTables *gt = (JTables *)(a.gtab + a.gtab_slot * k);
  if (!match) build_tables<JT>(*gt, S, HB, t);
  if (t < 3) S.qmax[t] = 0;
  wsync_lds();
  for (int i = t; i < S.ncomp * 64; i += JT) {
    int c = i >> 6, zz = i & 63;
    int tq = S.tq[c];
    uint32_t q = S.dqt_off[tq];
    int qv = S.dqt_prec[tq] ? ((HB(q + 2 * zz) << 8) | HB(q + 2 * zz + 1)) : HB(q + zz);
    int n = c_natural[zz];
    const int16_t qmv = (int16_t)(((int64_t)qv * c_aanscales[n] + (1 << 11)) >> 12);
    info->qmul[c][n] = qmv;  // read by jpeg_idct_kernel only
    if (n != 0) atomicMax(&S.qmax[c], qmv < 0 ? -(int)qmv : (int)qmv);
  }
  wsync_lds();  // header bytes are dead from here (P2 stages into the same LDS)
  if (match ? KS.tab.bad : gt->bad) {
    if (t == 0) S.status = FFCV_SAMPLE_BAD_MARKER;
    wsync_lds();
    fail();
    return;
  }
  // the window coefficients were zeroed by alloc_scratch
  // arena offsets are wave-uniform: keep them in scalar registers
  const uint64_t cf_off = ((uint64_t)wuni((uint32_t)(S.cf_off >> 32)) << 32) | wuni((uint32_t)S.cf_off);
  int16_t *coef = (int16_t *)(a.arena + cf_off);

  K1_STOP_AT(1, cf_off != 0x7fffffffffffull);  // diagnostics: K1 up to the tables (no de-stuff)
  // ------------------------------------------------------------- P2 ----
  // De-stuffing in stream order: each step the wave reads 64 consecutive
  // aligned dwords of the segment (one per lane), keeps every byte except a
  // 0x00 after 0xFF, stops at the first marker (0xFF + non-zero), and
  // writes the kept bytes at offsets from a wave scan of their counts.
  STAMP(2);
  uint8_t *gds = a.arena + (((uint64_t)wuni((uint32_t)(S.ds_off >> 32)) << 32) | wuni((uint32_t)S.ds_off));
  uint32_t dlen = 0;
  {
    const uint32_t seg0 = wuni(S.scan_off);  // uniform: sizes the buffer resource below
    const uint32_t seglen = nbytes > seg0 ? nbytes - seg0 : 0;
    const uintptr_t sb = (uintptr_t)(src + seg0);
    const uint32_t mis = (uint32_t)(sb & 3);
    const uint32_t *aw = (const uint32_t *)(sb - mis);
    const uint32_t ndw = (seglen + mis + 3) / 4;
    uint32_t carry = 0;  // byte before this step's first byte (0: none / not 0xFF)
    // Kept bytes are staged in LDS and flushed to HBM as aligned dwords every
    // DS_FLUSH steps: a byte store per kept byte would make every prefetch
    // wait behind the stores (gfx9 counts loads and stores in one vmcnt).
    uint32_t fbase = 0;  // stream offset of stage[0] (a multiple of 4)
    // The flush issues a fixed number of buffer stores per lane (out of range
    // past the staged bytes), so the prefetched loads issued before it are
    // waited for with a static vmcnt, not behind a dynamic store count.
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(wave_uniform(gds), 0, (int)wuni(S.ds_bytes), BUF_CFG);
    constexpr int FL_N = (STAGE_BYTES / 4 + JT - 1) / JT;  // stores per lane per flush
    auto flush = [&](uint32_t upto) {  // write stage bytes [fbase, upto), upto % 4 == 0
      wsync_lds();
      const uint32_t nd = (upto - fbase) / 4;
#pragma unroll
      for (int f = 0; f < FL_N; f++) {
        const uint32_t q = (uint32_t)(f * JT + t);
        const uint32_t v = ((const uint32_t *)S.stage)[min(q, (uint32_t)(STAGE_BYTES / 4 - 1))];
        __builtin_amdgcn_raw_buffer_store_b32(v, drs, q < nd ? fbase + 4 * q : BUF_OOR, 0, 0);
      }
      wsync_lds();
    };
    // DS_DEPTH-deep prefetch ring, unrolled so every ring register is consumed in
    // place (a rotating copy would make the compiler wait for all loads)
    // segment dwords through a buffer resource: past the segment the load is
    // out of range and returns 0 with no access, so every step issues its
    // load unconditionally and the compiler can count vmcnt statically
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void *)wave_uniform(aw), 0, (int)(ndw * 4), BUF_CFG);
    auto ld = [&](uint32_t d) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(srs, d * 4, 0, 0); };
    // Each lane takes two consecutive dwords per step (8 bytes): the step's
    // fixed work -- the wave scan of the kept counts, the neighbour bytes,
    // the marker ballot, the ring bookkeeping -- is shared by twice the bytes.
    // Byte masks stay in 0x80-per-byte form (zm), so no multiply gathers bits.
    constexpr int D2 = DS_DEPTH / 2;  // ring depth in two-dword lane steps
    static_assert(DS_FLUSH == DS_DEPTH, "one flush per ring cycle");
    uint32_t r0[D2], r1[D2];
#pragma unroll
    for (int u = 0; u < D2; u++) {
      r0[u] = ld(2 * (u * JT + t));
      r1[u] = ld(2 * (u * JT + t) + 1);
    }
    bool done = false;
    auto zm = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };
    // kept / marker bytes of one dword (0x80 per byte) at stream index rel0 of its byte 0
    auto scan_dw = [&](uint32_t w, uint32_t prevb, uint32_t nextb, int rel0, uint32_t &keep, uint32_t &mark) {
      const uint32_t pw = (w << 8) | prevb;          // previous byte of each byte
      const uint32_t nw = (w >> 8) | (nextb << 24);  // next byte of each byte
      const int lo = max(0, -rel0), hi = min(4, (int)seglen - rel0);  // valid bytes [lo, hi)
      const uint32_t vhi = hi >= 4 ? 0x80808080u : (hi <= 0 ? 0u : 0x80808080u >> (32 - 8 * hi));
      const uint32_t valid = vhi & (0x80808080u << (8 * lo));
      const uint32_t ff = zm(~w);
      // a 0x00 after 0xFF is stuffing, except the segment's first byte
      const uint32_t head = rel0 <= 0 ? 0x80808080u >> (24 - 8 * min(3, -rel0)) : 0u;  // bytes with rel <= 0
      const uint32_t removed = zm(w) & zm(~pw) & ~head;
      // a marker is 0xFF followed by a non-zero byte; end of data acts as one
      const uint32_t lastm = (hi >= 1 && rel0 + hi == (int)seglen) ? 0x80u << (8 * (hi - 1)) : 0u;
      mark = ((ff & ~zm(nw)) | (ff & lastm)) & valid;
      keep = valid & ~removed;
    };
    for (uint32_t base2 = 0; !done; base2 += D2 * JT) {
#pragma unroll
      for (int u = 0; u < D2; u++) {
        const uint32_t base = base2 + u * JT;  // two-dword lane step of lane 0
        const uint32_t w0 = r0[u], w1 = r1[u];
        const uint32_t nd = 2 * (base + D2 * JT + t);
        r0[u] = ld(nd);  // issued on every step (see srs)
        r1[u] = ld(nd + 1);
        if (done || 2 * base >= ndw) {
          done = true;
          continue;
        }
        const uint32_t d0 = 2 * (base + t);
        const uint32_t w1prev = lane_prev(w1);
        const uint32_t w0next = lane_next(w0);
        const uint32_t nfirst = lane_read(r0[(u + 1) % D2], 0);  // next step's first dword
        const uint32_t prevb = t == 0 ? carry : (w1prev >> 24);
        const uint32_t next1 = (t == JT - 1 ? nfirst : w0next) & 0xff;
        const int rel0 = (int)(4 * d0) - (int)mis;  // stream index of w0's byte 0
        uint32_t k0, m0, k1, m1;
        scan_dw(w0, prevb, w1 & 0xff, rel0, k0, m0);
        scan_dw(w1, w0 >> 24, next1, rel0 + 4, k1, m1);
        // the first marker of the step ends the segment: keep the bytes before it
        const uint32_t b0 = m0 ? (m0 & (0u - m0)) - 1u : 0xffffffffu;
        const uint32_t b1 = m0 ? 0u : (m1 ? (m1 & (0u - m1)) - 1u : 0xffffffffu);
        k0 &= b0;
        k1 &= b1;
        const uint64_t mk = __ballot((m0 | m1) != 0);
        if (mk) {
          const int ml = __ffsll((unsigned long long)mk) - 1;
          if (t > ml) k0 = k1 = 0;
          done = true;
        }
        const uint32_t c0 = __popc(k0), cnt = c0 + __popc(k1);
        const uint32_t off = dlen + wave_exscan(cnt) - fbase;
#pragma unroll
        for (int j = 0; j < 8; j++) {  // branch-free: dropped bytes go to a dummy byte
          const uint32_t km = j < 4 ? k0 : k1, w = j < 4 ? w0 : w1;
          const int jj = j & 3;
          const bool kj = (km >> (8 * jj + 7)) & 1;
          const uint32_t before = (j < 4 ? 0u : c0) + (jj ? __popc(km & ((1u << (8 * jj)) - 1u)) : 0u);
          S.stage[kj ? off + before : STAGE_DUMMY] = (uint8_t)(w >> (8 * jj));
        }
        dlen = lane_read(off + cnt, JT - 1) + fbase;
        carry = lane_read(w1, JT - 1) >> 24;
      }
      if (!done) {  // flush whole dwords, keep the 0..3-byte tail
        const uint32_t upto = dlen & ~3u;
        flush(upto);
        if (t < (int)(dlen - upto)) S.stage[t] = S.stage[upto - fbase + t];
        fbase = upto;
        wsync_lds();
      }
    }
    // tail + zero padding (libjpeg fills zeros after a marker)
    wsync_lds();
    for (uint32_t i = dlen - fbase + t; i < dlen - fbase + STREAM_PAD + 4; i += JT) S.stage[i] = 0;
    flush((dlen + STREAM_PAD + 3) & ~3u);
  }
  wsync_mem();
  K1_STOP_AT(2, dlen != 0x7fffffffu);  // diagnostics: K1 up to the de-stuffed stream
  // one image per wave: its stream base is wave-uniform (scalar registers,
  // so the refill loads use the scalar-base + 32-bit offset form)
  const uint32_t *words = wave_uniform((const uint32_t *)gds);
  const uint32_t total_bits = dlen * 8;


  int16_t *dcd = (int16_t *)(a.arena + (((uint64_t)wuni((uint32_t)(S.dc_off >> 32)) << 32) | wuni((uint32_t)S.dc_off)));
  const uint64_t sid = a.ids && a.eidx ? a.ids[k] : ~0ull;
  const bool any_bad = match ? entropy_passes(S, KS.tab, a, k, t, words, total_bits, coef, dcd, sid, MODE == JM_COEF)
                             : entropy_passes(S, *gt, a, k, t, words, total_bits, coef, dcd, sid, MODE == JM_COEF);
  wsync_mem();
  K1_STOP_AT(5, !any_bad);  // diagnostics: K1 up to the write pass
  if (any_bad) {  // a failed sample like any other: its status, zero output, no K1b / K2 work
    if (t == 0) S.status = FFCV_SAMPLE_CORRUPT;
    wsync_lds();
    fail();
    return;
  }

  // ------------------------------------------------------------- P6 ----
  // DC prediction (jdhuff.c last_dc_val) for the coefficient output (JM_COEF;
  // the other modes run it in jpeg_idct_kernel): per-component running sum of
  // DC differences in MCU block order, as a wave scan over block ranges of a
  // multiple of 8 blocks read as 16-byte buffer loads, DCP_U in flight.
  STAMP(6);
  if (MODE == JM_COEF) {
    constexpr int DCP_U = 4;
    const int nb = S.nblocks, bpm = S.bpm;
    const int per_b = ((nb + JT - 1) / JT + 7) & ~7;
    const int b0 = min(nb, per_b * t), b1 = min(nb, per_b * (t + 1));
    const __amdgpu_buffer_rsrc_t drs =
        __builtin_amdgcn_make_buffer_rsrc(wave_uniform((void *)dcd), 0, (int)wuni(S.dc_bytes), BUF_CFG);
    auto load8 = [&](int q) -> uint4 {  // blocks b0 + 8q .. b0 + 8q + 7
      const int b = b0 + 8 * q;
      return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                           drs, b < b1 ? (uint32_t)b * 2 : BUF_OOR, 0, 0));
    };
    auto diff = [](const uint4 &w, int e) -> int {
      const uint32_t x = e < 2 ? w.x : e < 4 ? w.y : e < 6 ? w.z : w.w;
      return (int)(int16_t)(x >> (16 * (e & 1)));
    };
    int32_t s0 = 0, s1 = 0, s2 = 0;  // (registers: no dynamically indexed arrays)
    int ph = b0 % bpm;
    for (int q0 = 0; q0 * 8 < per_b; q0 += DCP_U) {
      uint4 w[DCP_U];
#pragma unroll
      for (int u = 0; u < DCP_U; u++) w[u] = load8(q0 + u);
#pragma unroll
      for (int u = 0; u < DCP_U; u++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          if (b0 + 8 * (q0 + u) + e < b1) {
            const int c = S.blk_comp[ph], d = diff(w[u], e);
            s0 += c == 0 ? d : 0;
            s1 += c == 1 ? d : 0;
            s2 += c == 2 ? d : 0;
            if (++ph == bpm) ph = 0;
          }
        }
    }
    int32_t p0 = wave_exscan_i(s0), p1 = wave_exscan_i(s1), p2 = wave_exscan_i(s2);
    ph = b0 % bpm;
    int m = b0 / bpm;
    int my = m / S.mcux, mx = m - my * S.mcux;
    for (int q0 = 0; q0 * 8 < per_b; q0 += DCP_U) {
      uint4 w[DCP_U];
#pragma unroll
      for (int u = 0; u < DCP_U; u++) w[u] = load8(q0 + u);
#pragma unroll
      for (int u = 0; u < DCP_U; u++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          if (b0 + 8 * (q0 + u) + e < b1) {
            const int c = S.blk_comp[ph], d = diff(w[u], e);
            p0 += c == 0 ? d : 0;
            p1 += c == 1 ? d : 0;
            p2 += c == 2 ? d : 0;
            const int pv = c == 0 ? p0 : (c == 1 ? p1 : p2);
            const int bx = mx * S.hs[c] + S.blk_dx[ph], by = my * S.vs[c] + S.blk_dy[ph];
            if (bx >= S.wx0[c] && bx <= S.wx1[c] && by >= S.wy0[c] && by <= S.wy1[c])
              coef[(S.coff[c] + (uint64_t)(by - S.wy0[c]) * (S.wx1[c] - S.wx0[c] + 1) + (bx - S.wx0[c])) * 64] =
                  (int16_t)pv;
            if (++ph == bpm) {
              ph = 0;
              if (++mx == S.mcux) {
                mx = 0;
                my++;
              }
            }
          }
        }
    }
  }
  wsync_mem();
  K1_STOP_AT(6, !any_bad);  // diagnostics: K1 up to the DC prediction

  if (MODE == JM_COEF) {
    int16_t *o = (int16_t *)a.out + a.out_stride / 2 * k;
    for (int64_t b = t; b < S.nblocks; b += JT) {
      int64_t m = b / S.bpm;
      int ph = (int)(b - m * S.bpm);
      int my = (int)(m / S.mcux), mx = (int)(m - (int64_t)my * S.mcux);
      int c = S.blk_comp[ph];
      int bx = mx * S.hs[c] + S.blk_dx[ph], by = my * S.vs[c] + S.blk_dy[ph];
      const int16_t *cp = coef + (S.coff[c] + (uint64_t)by * (S.wx1[c] - S.wx0[c] + 1) + bx) * 64;  // window = image
      int16_t zz[64], nb[64];
#pragma unroll
      for (int p8 = 0; p8 < 8; p8++) *(uint4 *)(zz + p8 * 8) = ((const uint4 *)cp)[p8];
#pragma unroll
      for (int n = 0; n < 64; n++) nb[n] = zz[kZigzagOfNatural[n]];
      uint4 *dp = (uint4 *)(o + b * 64);
#pragma unroll
      for (int p8 = 0; p8 < 8; p8++) dp[p8] = *(const uint4 *)(nb + p8 * 8);
    }
    if (t == 0) a.status[k] = any_bad ? FFCV_SAMPLE_CORRUPT : FFCV_SAMPLE_OK;
    return;
  }

  // ------------------------------------------------------------- P7 ----
  // geometry + crop window for K2
  STAMP(7);
  if (t == 0) {
    info->status = FFCV_SAMPLE_OK;
    info->W = S.W;
    info->H = S.H;
    info->ncomp = S.ncomp;
    info->color_rgb = S.color_rgb;
    for (int c = 0; c < 3; c++) {
      bool v = c < S.ncomp;
      info->he[c] = v ? S.hmax / S.hs[c] : 1;
      info->ve[c] = v ? S.vmax / S.vs[c] : 1;
      info->cw[c] = v ? S.cw[c] : 0;
      info->ch[c] = v ? S.ch[c] : 0;
      info->stride[c] = v ? (S.wx1[c] - S.wx0[c] + 1) * 8 : 0;
      info->poff[c] = v ? S.poff[c] : 0;
    }
    info->rgb_off = S.rgb_off;
    info->cf_off = S.cf_off;
    info->nblocks = S.nblocks;
    info->bpm = S.bpm;
    info->mcux = S.mcux;
    for (int c = 0; c < 3; c++) {
      info->coff[c] = S.coff[c];
      info->hs[c] = S.hs[c];
      info->vs[c] = S.vs[c];
      info->wx0[c] = S.wx0[c];
      info->wx1[c] = S.wx1[c];
      info->wy0[c] = S.wy0[c];
      info->wy1[c] = S.wy1[c];
      info->qmax[c] = S.qmax[c];
    }
    for (int b = 0; b < 10; b++) {
      info->blk_comp[b] = S.blk_comp[b];
      info->blk_dx[b] = S.blk_dx[b];
      info->blk_dy[b] = S.blk_dy[b];
    }
    info->ri = S.ri;
    info->rj = S.rj;
    info->rh = S.rh;
    info->rw = S.rw;
    a.status[k] = any_bad ? FFCV_SAMPLE_CORRUPT : FFCV_SAMPLE_OK;
  }
  if (MODE == JM_RRC) {  // the resize plan and linear taps K2's workgroups share
    const int out_h = a.p.out_h, out_w = a.p.out_w;
    const ResizePlan P = make_plan(S.rw, S.rh, out_w, out_h);
    const bool tabs = a.taps && P.kind == 3 && out_w + out_h <= K2_TAPS;
    if (tabs) {
      const int flip = a.flips ? a.flips[k] : 0;
      uint2 *tp = a.taps + (uint64_t)k * K2_TAPS;
      for (int i = t; i < out_w + out_h; i += JT)
        tp[i] = tap_pack(i < out_w ? lin_tap(P.scale_x, P.inv_x, P.sw, flip ? out_w - 1 - i : i)
                                   : lin_tap(P.scale_y, P.inv_y, P.sh, i - out_w));
    }
    if (t == 0) {
      info->plan = P;
      info->taps = tabs;
    }
  }

  // (P8, the DC prediction and the IDCT of the window's blocks, is
  // jpeg_idct_kernel: a launch of its own runs it at VALU throughput instead of
  // behind this kernel's latency-bound waves, ~25% of K1's time per image)
  STAMP(9);
}
