// Huffman stage of the JPEG encoder on the device (include/danhip.h, "JPEG encode: Huffman stage on the device"): the staging buffer that
// danhip_jpeg_encode_scan_prepare fills, and the per-lane routines of every phase - block length, block write, FF count, stuffing scatter,
// file finish - as __host__ __device__ templates over a context C.  The kernels of jpeg_encode_huffman_exact.hip instantiate them over
// device memory, danhip_jpeg_encode_entropy_emulate_batch (jpeg_encode.cpp) over checked host arrays: one body of code encodes on both sides.
// What they write is what jpeg_encode.cpp's write_file writes (jchuff.c encode_one_block, flush_bits, emit_byte's FF 00).
//
// A context C supplies
//   void load_block(int64_t el, int16_t v[64])     the 64 coefficients (column-major) that start at element el of the coefficient buffer
//   int dc(int64_t el)                             the one coefficient at el (a block's DC value)
//   uint32_t tab(int t, int sym)                   code | length << 16 of table t (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma)
//   void or_word(const DhJencImage&, int64_t w, uint32_t v)   v OR-ed into 32-bit word w of the image's unstuffed buffer; the word's most
//                                                  significant byte is byte 4 w of the stream.  Refused at and beyond im.bits_bytes / 4
//   uint32_t ubyte(const DhJencImage&, int64_t i)  byte i of the unstuffed buffer, i < im.bits_bytes
//   void file_store(const DhJencImage&, int64_t i, uint32_t b)   byte i of the image's file slot; refused at and beyond im.file_capacity
//   uint32_t header_byte(const DhJencImage&, int i)   byte i of the image's staged markers, i < im.header_len
#pragma once
#include <stdint.h>

#include "../../include/danhip.h"

#if defined(__HIPCC__)
#define DH_JHUF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DH_JHUF_HD inline
#endif
#if defined(__clang__)
#define DH_JHUF_UNROLL _Pragma("unroll")
#else
#define DH_JHUF_UNROLL
#endif

#define DH_JHUF_MAGIC 0x4655484a
#define DH_JHUF_GROUP 256                                            /* lanes of every workgroup */
#define DH_JHUF_BLOCK_BITS 1658                                      /* (9 + 11) + 63 * (16 + 10): the longest block */
#define DH_JHUF_BLOCK_BYTES 208                                      /* ... in whole bytes, a multiple of 4 */
#define DH_JHUF_LANE_BYTES DANHIP_JPEG_ENCODE_STUFF_LANE_BYTES       /* unstuffed bytes a lane of the stuffing launches takes */
#define DH_JHUF_CHUNK_BYTES (DH_JHUF_GROUP * DH_JHUF_LANE_BYTES)     /* ... and a workgroup */
#define DH_JHUF_HEADER_SLOT 640                                      /* staged bytes per image's markers (623 are used) */
#define DH_JHUF_MAX_FILE ((int64_t)1 << 30)                          /* an image whose file bound reaches this stays with the host stage */
#define DH_JHUF_INVALID ((uint64_t)1 << 63)                          /* flag on a workgroup's bit sum: a value without a baseline code */

// optimize (DANHIP_JPEG_ENC_OPTIMIZE): image i owns the first bytes of the device workspace, DH_JHUF_OPT_STRIDE of them from i * stride
#define DH_JHUF_OPT_COUNTS 0                                         /* uint32 [4][257]: the symbol statistics, table order as C::tab */
#define DH_JHUF_OPT_TABS 4128                                        /* uint32 [4][256]: code | length << 16, what the walk reads */
#define DH_JHUF_OPT_BITSVALS 8224                                    /* per table uint8 bits[17], vals[256] */
#define DH_JHUF_OPT_WORDS 9328                                       /* int32 [4]: the length of the markers below, 3 spare */
#define DH_JHUF_OPT_HEADER 9344                                      /* the image's markers with its own DHT segments */
#define DH_JHUF_OPT_HEADER_MAX (DH_JHUF_HEADER_PRE + 4 * (21 + 256) + DH_JHUF_HEADER_SOS)
#define DH_JHUF_OPT_STRIDE 10656
#define DH_JHUF_HEADER_PRE 177                                       /* SOI, APP0, two DQT, SOF0: the staged markers in front of the DHTs */
#define DH_JHUF_HEADER_SOS 14                                        /* ... and behind them */
#define DH_JHUF_HIST_ROUNDS 4                                        /* blocks a lane of the histogram launch counts */
#define DH_JHUF_HIST_BLOCKS (DH_JHUF_HIST_ROUNDS * DH_JHUF_GROUP)    /* ... and a workgroup: its work item */
static_assert(DH_JHUF_OPT_HEADER + DH_JHUF_OPT_HEADER_MAX <= DH_JHUF_OPT_STRIDE && DH_JHUF_OPT_STRIDE % 16 == 0, "the regions fit the stride");
static_assert(DH_JHUF_OPT_BITSVALS + 4 * 273 <= DH_JHUF_OPT_WORDS && DH_JHUF_OPT_TABS + 4096 <= DH_JHUF_OPT_BITSVALS, "the regions do not overlap");

struct DhJencHeader {              // first bytes of the staging buffer; every off_* counts bytes from the buffer's start, 16-byte aligned
  int32_t magic, B, nprepared, max_len_groups, max_stuff_groups, optimize, reserved[2];   // optimize: 0 | 1, per-image tables in the workspace
  int64_t off_images, off_tabs, off_headers, used_bytes, workspace_bytes, coef_count, file_bytes, reserved2;
};

struct DhJencImage {               // one per image of the batch; prepared = 0: left to the host stage, every count below is 0
  int32_t prepared, hs, nl, bpm;   // luma blocks per MCU row of the MCU (1 | 2), luma blocks per MCU (1 | 4), blocks per MCU (3 | 6)
  int32_t mcus_x, mcus_y, bw0, header_len;
  int32_t len_groups, stuff_groups, reserved[2];       // workgroups of the length / write launches and (worst case) of the stuffing launches
  int64_t nblocks;                 // blocks in scan order = mcus_x * mcus_y * bpm
  int64_t plane[3];                // first element of each component in the coefficient BUFFER (coef_offset included)
  int64_t coef_offset, coef_count; // the image's slot, int16 elements
  int64_t file_offset, file_capacity;
  int64_t header_off;              // the staged markers, bytes from the staging buffer's start
  int64_t ws_gsum;                 // workspace, bytes: uint64 [len_groups] bit sum of a workgroup's blocks | DH_JHUF_INVALID
  int64_t ws_goff;                 //   uint64 [len_groups + 1] bit offset of a workgroup's first block; the last entry is the scan's bits
  int64_t ws_bits;                 //   the unstuffed scan, bits_bytes bytes = len_groups * DH_JHUF_GROUP * DH_JHUF_BLOCK_BYTES
  int64_t bits_bytes;
  int64_t ws_ff;                   //   uint32 [stuff_groups] FF bytes of a chunk
  int64_t ws_ffoff;                //   uint32 [stuff_groups] FF bytes in front of a chunk
};

// k-th coded coefficient -> column * 8 + row: the zig-zag order in the decoder's column-major layout
DH_JHUF_HD int dh_jhuf_zig(int k) {
  constexpr uint8_t z[64] = {0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,
                             13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58,
                             51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};
  return z[k];
}

DH_JHUF_HD int dh_jhuf_bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// where block s of the scan lies: its first coefficient's element in the buffer, and the same of the block whose DC value it is coded
// against (-1: the component's first block, predicted from 0).  One interleaved scan: per MCU nl luma blocks (row by row), then Cb, then Cr.
DH_JHUF_HD void dh_jhuf_locate(const DhJencImage& im, int64_t s, int64_t* el, int64_t* pred_el, int* comp) {
  const int64_t mcu = s / im.bpm;
  const int bi = (int)(s - mcu * im.bpm);
  const int c = bi < im.nl ? 0 : bi - im.nl + 1;
  const int64_t my = mcu / im.mcus_x, mx = mcu - my * im.mcus_x;
  *comp = c;
  if (c == 0) {
    const int vs = im.nl / im.hs;
    const int v = bi / im.hs, h = bi - v * im.hs;
    *el = im.plane[0] + ((my * vs + v) * im.bw0 + mx * im.hs + h) * 64;
    if (bi > 0) {
      const int pv = (bi - 1) / im.hs, ph = (bi - 1) - pv * im.hs;
      *pred_el = im.plane[0] + ((my * vs + pv) * im.bw0 + mx * im.hs + ph) * 64;
    } else if (mcu > 0) {
      const int64_t py = (mcu - 1) / im.mcus_x, px = (mcu - 1) - py * im.mcus_x;
      *pred_el = im.plane[0] + ((py * vs + (vs - 1)) * im.bw0 + px * im.hs + (im.hs - 1)) * 64;
    } else {
      *pred_el = -1;
    }
  } else {
    const int64_t base = c == 1 ? im.plane[1] : im.plane[2];
    *el = base + mcu * 64;
    *pred_el = mcu > 0 ? base + (mcu - 1) * 64 : -1;
  }
}

// jchuff.c encode_one_block over a sink E { void put(unsigned code, int len); }.  false: a value the baseline tables do not carry (a DC
// difference of more than 11 bits, an AC value of more than 10); the sink has then taken a prefix of the block.
template <class C, class E>
DH_JHUF_HD bool dh_jhuf_walk(C& c, const int16_t v[64], int pred, int comp, E& e) {
  const int tdc = comp == 0 ? 0 : 2, tac = tdc + 1;
  const int diff = (int)v[0] - pred;
  int nb = dh_jhuf_bit_length((unsigned)(diff < 0 ? -diff : diff));
  if (nb > 11) return false;
  uint32_t t = c.tab(tdc, nb);
  if ((t >> 16) == 0) return false;
  e.put(t & 0xffff, (int)(t >> 16));
  if (nb) e.put((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);      // a negative value: the low bits of its one's complement
  int run = 0;
  const uint32_t zrl = c.tab(tac, 0xf0);
  DH_JHUF_UNROLL
  for (int k = 1; k < 64; ++k) {
    const int a = v[dh_jhuf_zig(k)];
    if (a == 0) { ++run; continue; }
    while (run > 15) { e.put(zrl & 0xffff, (int)(zrl >> 16)); run -= 16; }
    nb = dh_jhuf_bit_length((unsigned)(a < 0 ? -a : a));
    if (nb > 10) return false;
    t = c.tab(tac, (run << 4) | nb);
    e.put(t & 0xffff, (int)(t >> 16));
    e.put((unsigned)(a < 0 ? a - 1 : a) & ((1u << nb) - 1), nb);
    run = 0;
  }
  if (run > 0) {
    t = c.tab(tac, 0);
    e.put(t & 0xffff, (int)(t >> 16));
  }
  return true;
}

// The symbols of the same walk without a table (jchuff.c htest_one_block, the gather pass of optimize=True) over a sink
// S { void add(int t, int sym); }: table t as C::tab numbers them, sym the DC category or the AC run / size byte, ZRL 0xF0 and EOB 0x00
// among them.  false at the same values as dh_jhuf_walk; the sink has then taken a prefix of the block.
template <class S>
DH_JHUF_HD bool dh_jhuf_symbols(const int16_t v[64], int pred, int comp, S& s) {
  const int tdc = comp == 0 ? 0 : 2, tac = tdc + 1;
  const int diff = (int)v[0] - pred;
  int nb = dh_jhuf_bit_length((unsigned)(diff < 0 ? -diff : diff));
  if (nb > 11) return false;
  s.add(tdc, nb);
  int run = 0;
  DH_JHUF_UNROLL
  for (int k = 1; k < 64; ++k) {
    const int a = v[dh_jhuf_zig(k)];
    if (a == 0) { ++run; continue; }
    while (run > 15) { s.add(tac, 0xf0); run -= 16; }
    nb = dh_jhuf_bit_length((unsigned)(a < 0 ? -a : a));
    if (nb > 10) return false;
    s.add(tac, (run << 4) | nb);
    run = 0;
  }
  if (run > 0) s.add(tac, 0);
  return true;
}

struct DhJhufCount {               // the sink of the length phase
  uint32_t bits = 0;
  DH_JHUF_HD void put(unsigned, int len) { bits += (uint32_t)len; }
};

template <class C>
struct DhJhufEmit {                // the sink of the write phase: MSB first from a bit offset, whole 32-bit words OR-ed into the buffer
  C& c;
  const DhJencImage& im;
  int64_t w;                       // the word that the next flush goes to
  uint64_t acc;
  int n;                           // bits of acc that belong to word w (the bits in front of the block's first one count, as zeros)
  DH_JHUF_HD DhJhufEmit(C& c_, const DhJencImage& im_, uint64_t bit) : c(c_), im(im_), w((int64_t)(bit >> 5)), acc(0), n((int)(bit & 31)) {}
  DH_JHUF_HD void put(unsigned code, int len) {                      // len <= 16, code < 2^len
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      c.or_word(im, w++, (uint32_t)(acc >> (n - 32)));
      n -= 32;
      acc &= ((uint64_t)1 << n) - 1;
    }
  }
  DH_JHUF_HD void finish() {
    if (n > 0) c.or_word(im, w, (uint32_t)(acc << (32 - n)));
  }
};

// Phase 1, one lane per block s < im.nblocks: the block's bits, at most DH_JHUF_BLOCK_BITS, or DH_JHUF_INVALID
template <class C>
DH_JHUF_HD uint64_t dh_jhuf_lane_length(C& c, const DhJencImage& im, int64_t s) {
  int64_t el, pred_el;
  int comp;
  dh_jhuf_locate(im, s, &el, &pred_el, &comp);
  int16_t v[64];
  c.load_block(el, v);
  const int pred = pred_el >= 0 ? c.dc(pred_el) : 0;
  DhJhufCount e;
  if (!dh_jhuf_walk(c, v, pred, comp, e)) return DH_JHUF_INVALID;
  // The standard tables never exceed the bound.  An image's own tables (optimize) can give one block 16-bit codes throughout, (16 + 11) +
  // 63 * (16 + 10) = 1665 bits: such a block is flagged like a value without a code, and the image goes to the host stage.
  return e.bits <= DH_JHUF_BLOCK_BITS ? e.bits : DH_JHUF_INVALID;
}

// The histogram launch of optimize, one lane per block s < im.nblocks: the block's symbols into the sink; false as dh_jhuf_lane_length
// gives DH_JHUF_INVALID for a value (the image is flagged there; its statistics are then of no use)
template <class C, class S>
DH_JHUF_HD bool dh_jhuf_lane_symbols(C& c, const DhJencImage& im, int64_t s, S& sink) {
  int64_t el, pred_el;
  int comp;
  dh_jhuf_locate(im, s, &el, &pred_el, &comp);
  int16_t v[64];
  c.load_block(el, v);
  const int pred = pred_el >= 0 ? c.dc(pred_el) : 0;
  return dh_jhuf_symbols(v, pred, comp, sink);
}

// Phase 3, the same walk: the block's codes from bit `bit` of the unstuffed buffer.  len: what phase 1 gave for the block; a block it
// found invalid writes nothing.  The scan's last block also pads its last byte with 1 bits (flush_bits).
template <class C>
DH_JHUF_HD void dh_jhuf_lane_write(C& c, const DhJencImage& im, int64_t s, uint64_t bit, uint64_t len) {
  if (len & DH_JHUF_INVALID) return;
  int64_t el, pred_el;
  int comp;
  dh_jhuf_locate(im, s, &el, &pred_el, &comp);
  int16_t v[64];
  c.load_block(el, v);
  const int pred = pred_el >= 0 ? c.dc(pred_el) : 0;
  DhJhufEmit<C> e(c, im, bit);
  dh_jhuf_walk(c, v, pred, comp, e);
  if (s == im.nblocks - 1) {
    const int pad = (int)((8 - ((bit + len) & 7)) & 7);
    if (pad) e.put((1u << pad) - 1, pad);
  }
  e.finish();
}

// bytes of the unstuffed scan: the bits of the scan in whole bytes, never more than the buffer holds
DH_JHUF_HD int64_t dh_jhuf_scan_bytes(const DhJencImage& im, uint64_t total_bits) {
  const uint64_t n = (total_bits + 7) >> 3;
  return n < (uint64_t)im.bits_bytes ? (int64_t)n : im.bits_bytes;
}

// Phase 4, one lane per DH_JHUF_LANE_BYTES bytes from byte0: the FF bytes among them
template <class C>
DH_JHUF_HD uint32_t dh_jhuf_lane_ffcount(C& c, const DhJencImage& im, int64_t scan_bytes, int64_t byte0) {
  uint32_t n = 0;
  for (int k = 0; k < DH_JHUF_LANE_BYTES; ++k)
    if (byte0 + k < scan_bytes && c.ubyte(im, byte0 + k) == 0xff) ++n;
  return n;
}

// Phase 6, the same lanes: every byte to its place behind the markers, 00 behind every FF.  ff_before: the FF bytes of the scan in front of byte0
template <class C>
DH_JHUF_HD void dh_jhuf_lane_scatter(C& c, const DhJencImage& im, int64_t scan_bytes, int64_t byte0, uint32_t ff_before) {
  int64_t out = (int64_t)im.header_len + byte0 + ff_before;
  for (int k = 0; k < DH_JHUF_LANE_BYTES; ++k) {
    if (byte0 + k >= scan_bytes) return;
    const uint32_t b = c.ubyte(im, byte0 + k);
    c.file_store(im, out++, b);
    if (b == 0xff) c.file_store(im, out++, 0);
  }
}

// Phase 5, `lanes` lanes of one workgroup per image: the markers in front, EOI behind.  Returns the file's size; a size above the
// slot's capacity is the caller's to flag (the stores are refused there).
template <class C>
DH_JHUF_HD int64_t dh_jhuf_lane_finish(C& c, const DhJencImage& im, int64_t scan_bytes, uint32_t total_ff, int lane, int lanes) {
  for (int i = lane; i < im.header_len; i += lanes) c.file_store(im, i, c.header_byte(im, i));
  const int64_t end = (int64_t)im.header_len + scan_bytes + total_ff;
  if (lane == 0) {
    c.file_store(im, end, 0xff);
    c.file_store(im, end + 1, 0xd9);
  }
  return end + 2;
}
