// Huffman stage of the JPEG decoder as a self-synchronising parallel decoder (include/danhip.h, "Huffman decoding on the device"): the tables
// danhip_jpeg_scan_prepare_batch packs into the staging buffer, and the per-subsequence routines - bit reader with FF00 stuffing, symbol
// decode, one subsequence from an entry state, block addressing - as __host__ __device__ templates over a context C.  The kernels of
// jpeg_huffman_exact.hip instantiate them over LDS, danhip_jpeg_entropy_emulate_batch (jpeg_entropy.cpp) over checked host arrays: one
// body of code decodes on both sides.
//
// A context C supplies
//   uint32_t byte(int32_t i)               byte i of the lane's SEGMENT; 0 at and beyond the segment's data length or outside the staged window
//   uint32_t look(int t, uint32_t i) ...   fields of table t of the image (t = 2 * component + (AC ? 1 : 0))
//   uint32_t zig(int k)                    column-major element of the k-th coded coefficient
//   void store(int64_t block, int el, int v)   one coefficient of the image (write phase only)
// Inside a segment's data every FF is followed by its stuffed 00 (the prepare pass ends the data at the first FF that is not), so the
// reader skips the byte after an FF without looking at it.
#pragma once
#include <stdint.h>

#include "../../include/danhip.h"

#if defined(__HIPCC__)
#define DH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DH_HD inline
#endif

#define DH_HUFF_S DANHIP_JPEG_SUBSEQ_BYTES
#define DH_HUFF_G DANHIP_JPEG_SUBSEQ_PER_GROUP
#define DH_HUFF_TAIL 32                                              /* bytes a group's last lane may read past its subsequence */
#define DH_HUFF_WINDOW (DH_HUFF_G * DH_HUFF_S + 16 + DH_HUFF_TAIL)   /* a group's window starts on the 16-byte boundary at or before its first item */
#define DH_HUFF_MAX_OFF (DH_HUFF_S * 8 + 64)                         /* an entry offset (bits into the subsequence) never leaves [0, this] */
#define DH_HUFF_MAX_SYMBOLS (DH_HUFF_S * 8 + 8)                      /* a symbol takes at least one bit */
#define DH_HUFF_DC_CHUNK 256                                         /* MCUs per workgroup of the DC prefix sum */
#define DH_HUFF_MAGIC 0x46465548
#define DH_HUFF_MAX_SCAN (1 << 30)                                   /* a longer scan stays with the host stage */

struct DhHuffTab {                 // Huff of jpeg_entropy.cpp without its flag: 1424 bytes
  uint16_t look[512];
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t sym[256];
};

struct DhScanHeader {              // first bytes of the staging buffer; every off_* counts bytes from the buffer's start, 16-byte aligned
  int32_t magic, B, nseg, nitems, ngroups, nchunks, ntabs, reserved;
  int64_t off_images, off_segs, off_items, off_groups, off_chunks, off_tabs, off_scan, scan_bytes, used_bytes, coef_capacity;
};

struct DhScanImage {               // one per image of the batch; prepared = 0: every count below is 0
  int32_t prepared, ncomp, hs, vs, bpm, mcus_x, mcus, restart;
  int32_t blocks_w[3], tab_first;
  int32_t first_seg, nseg, first_item, nitems, first_group, ngroups, first_chunk, nchunks;
  int64_t plane[3];                // first block of each component in the image's coefficient slot
  int64_t total_blocks, coef_offset, scan_offset, scan_len;       // scan_offset: bytes from off_scan, a multiple of 16
};

struct DhScanSeg {                 // one restart interval (the whole scan without DRI)
  int32_t offset, len;             // bytes from the image's scan start up to the FF of the marker that ends it; segment + 2-byte marker tile the scan
  int32_t data_len;                // up to the first FF that no 00 follows (fill bytes before the marker are no data)
  int32_t first_mcu, mcu_count, first_item, nitems, final;
};

struct DhScanItem { int32_t seg, sub; };                             // subsequence sub of segment seg: bytes [sub * S, min(sub * S + S, data_len))

struct DhScanGroup {               // one workgroup of the Huffman launches: items [first_item, first_item + nitems), nitems <= G
  int32_t image, first_item, nitems, carry_from;                     // carry_from: first group that holds items of this group's first segment
  int64_t win_base;                // bytes from off_scan, a multiple of 16: the group's LDS window is [win_base, win_base + DH_HUFF_WINDOW)
  int64_t reserved;
};

struct DhDcChunk {                 // one workgroup of the DC launches: MCUs [mcu0, mcu0 + n) of segment seg, n <= DH_HUFF_DC_CHUNK
  int32_t image, seg, mcu0, n, chain_from, reserved;                 // chain_from: the segment's first chunk
};

struct DhExit { int32_t off, state, n, entry; };                     // where a lane left its subsequence: bits into the next one, bi | k << 8,
                                                                     // blocks completed, and the entry (off << 16 | state) it started from

DH_HD int32_t dh_huff_pack(int32_t off, int32_t state) { return (off << 16) | (state & 0xffff); }

template <class C>
struct DhBits {                    // MSB-first reader; acc holds cnt unread bits, stuffed one flag per loaded byte (1: a 00 was skipped after it)
  int32_t p;
  uint64_t acc;
  int32_t cnt;
  uint32_t stuffed;
  DH_HD void fill(C& c) {
    while (cnt <= 56) {
      const uint32_t b = c.byte(p);
      const uint32_t st = b == 0xFF ? 1u : 0u;
      p += 1 + (int32_t)st;
      acc = (acc << 8) | b;
      cnt += 8;
      stuffed = (stuffed << 1) | st;
    }
  }
  DH_HD void init(C& c, int32_t byte, int bit) { p = byte; acc = 0; cnt = 0; stuffed = 0; fill(c); cnt -= bit; }
  DH_HD uint32_t peek(int k) const { return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1); }
  DH_HD void skip(int k) { cnt -= k; }
  // the next unread bit: byte index in the segment and bit within it; never the 00 of an FF00 pair that this reader skipped
  DH_HD void pos(int32_t* byte, int32_t* bit) const {
    const int nb = (cnt + 7) >> 3;
    uint32_t m = stuffed & ((1u << nb) - 1), skipped = 0;
    for (int i = 0; i < 8; ++i) skipped += (m >> i) & 1u;
    *byte = p - nb - (int32_t)skipped;
    *bit = nb * 8 - cnt;
  }
};

template <class C>
DH_HD int dh_huff_sym(DhBits<C>& b, C& c, int t) {                   // decode_sym of jpeg_entropy.cpp; -1: no such code (16 bits are dropped)
  const uint32_t look = c.look(t, b.peek(9));
  if (look) { b.skip((int)(look >> 8)); return (int)(look & 255); }
  int l = 10;
  int32_t code = (int32_t)b.peek(10);
  while (code > c.maxcode(t, l)) {
    ++l;
    if (l > 16) { b.skip(16); return -1; }
    code = (int32_t)b.peek(l);
  }
  b.skip(l);
  const int idx = code + c.valoff(t, l);
  return (idx < 0 || idx > 255) ? -1 : (int)c.sym(t, idx);
}

DH_HD int dh_huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct DhBlockGeom {               // what decode_scan derives from the header
  int32_t bpm, nl, hs, mcus_x, bw0, bw1, bw2;                        // scalars, not arrays: a select between registers needs no indexing
  int64_t plane0, plane1, plane2, total_blocks;
};

// scan-order block index of the image -> block of the coefficient slot (decode_scan's MCU, component, v, h order); -1: outside the image
DH_HD int64_t dh_huff_block(const DhBlockGeom& g, int64_t scan_index) {
  const int64_t mcu = scan_index / g.bpm;
  const int bi = (int)(scan_index - mcu * g.bpm);
  const int c = bi < g.nl ? 0 : bi - g.nl + 1;
  const int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.nl / g.hs : 1;
  const int v = c == 0 ? bi / g.hs : 0, h = c == 0 ? bi - v * g.hs : 0;
  const int64_t my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
  const int64_t m0 = -(int64_t)(c == 0), m1 = -(int64_t)(c == 1), m2 = -(int64_t)(c == 2);      // masks, not selects: the compiler turns a select
  const int64_t plane = (g.plane0 & m0) | (g.plane1 & m1) | (g.plane2 & m2);                    // of fields into an indexed load from scratch
  const int64_t bw = ((int64_t)g.bw0 & m0) | ((int64_t)g.bw1 & m1) | ((int64_t)g.bw2 & m2);
  const int64_t blk = plane + (my * cv + v) * bw + mx * ch + h;
  return (scan_index < 0 || blk < 0 || blk >= g.total_blocks) ? -1 : blk;
}

struct DhSub {                     // one subsequence of one segment
  int32_t start, end, data_len;    // bytes of the segment: [start, end), end <= data_len
  int32_t bpm, nl;
};

struct DhWrite {                   // write phase: the segment's blocks and what the lane found
  int64_t cur;                     // in: blocks of the segment completed before the lane's entry
  int64_t seg_blocks, first_block; // blocks of the segment; scan-order index of its first block in the image
  int32_t final;                   // the scan's last segment: nothing is asked of the bytes behind its last block
  int32_t error, capped;           // out: a code no table holds, a run past 63, a DC category above 11, bits beyond the data; stopped at seg_blocks
};

// Decodes every symbol that starts in [entry, end) of the subsequence.  An impossible code, run or category restarts the block and goes on
// (speculation meets those all the time); with WRITE it is an error of the image, coefficients are stored, and the lane stops at the segment's
// block count.  Every loop is bounded by constants: DH_HUFF_MAX_SYMBOLS symbols, 8 bytes per refill, 7 steps of the long-code walk.
template <class C, bool WRITE>
DH_HD DhExit dh_huff_decode_sub(C& c, const DhSub& a, int32_t entry, const DhBlockGeom* g, DhWrite* w) {
  int32_t eoff = (entry >> 16) & 0xffff;
  if (eoff > DH_HUFF_MAX_OFF) eoff = DH_HUFF_MAX_OFF;
  int bi = entry & 255, k = (entry >> 8) & 255;
  if (bi >= a.bpm) bi = 0;
  if (k > 63) k = 0;
  DhBits<C> b;
  b.init(c, a.start + (eoff >> 3), eoff & 7);
  int32_t n = 0, b0 = 0, bit = 0;
  int64_t blk = -1;
  if (WRITE) {
    w->error = 0; w->capped = 0;
    if (w->cur < w->seg_blocks) blk = dh_huff_block(*g, w->first_block + w->cur);
  }
  for (int it = 0; it < DH_HUFF_MAX_SYMBOLS; ++it) {
    b.pos(&b0, &bit);
    if (b0 >= a.end) break;
    if (WRITE && w->cur >= w->seg_blocks) { w->capped = 1; break; }
    if (b.cnt < 32) b.fill(c);                                       // a symbol and its value take at most 16 + 15 bits
    const int comp = bi < a.nl ? 0 : bi - a.nl + 1;
    const int s = dh_huff_sym(b, c, comp * 2 + (k ? 1 : 0));
    bool done = false, bad = false;
    if (k == 0) {
      if (s < 0 || s > 11) {
        bad = true;
      } else {
        const int diff = s ? dh_huff_extend((int)b.peek(s), s) : 0;
        b.skip(s);
        if (WRITE && blk >= 0) c.store(blk, 0, diff);                // the DC DIFFERENCE; the DC launches turn it into the value
        k = 1;
      }
    } else if (s < 0) {
      bad = true;
    } else {
      const int r = s >> 4, z = s & 15;
      if (z) {
        k += r;
        if (k > 63) {
          bad = true;
        } else {
          const int val = dh_huff_extend((int)b.peek(z), z);
          b.skip(z);
          if (WRITE && blk >= 0) c.store(blk, (int)c.zig(k), val);
          ++k;
          done = k > 63;
        }
      } else if (r == 15) {
        k += 16;
        done = k > 63;
      } else {
        done = true;
      }
    }
    if (bad) {
      k = 0;                                                         // the block starts over
      if (WRITE) w->error = 1;
    }
    if (done) {
      k = 0;
      bi = bi + 1 == a.bpm ? 0 : bi + 1;
      ++n;
      if (WRITE) {
        b.pos(&b0, &bit);
        if (blk < 0 || b0 > a.data_len || (b0 == a.data_len && bit > 0)) w->error = 1;      // bits from beyond the segment's data
        ++w->cur;
        if (w->cur < w->seg_blocks) {
          blk = dh_huff_block(*g, w->first_block + w->cur);
        } else if (!w->final) {                                      // a restart marker follows: less than one whole byte may be left over
          const int32_t used = bit ? b0 + 1 + (c.byte(b0) == 0xFF ? 1 : 0) : b0;
          if (used != a.data_len) w->error = 1;
        }
      }
    }
  }
  b.pos(&b0, &bit);
  DhExit e;
  e.off = (b0 - a.end) * 8 + bit;
  if (e.off < 0) e.off = 0;
  if (e.off > DH_HUFF_MAX_OFF) e.off = DH_HUFF_MAX_OFF;
  e.state = bi | (k << 8);
  e.n = n;
  e.entry = entry;
  return e;
}

// ---- DC and range: one MCU of a segment.  C adds  int load(int64_t block, int el)  and  uint32_t quant(int comp, int nat).
template <class C>
DH_HD void dh_dc_mcu_sum(C& c, const DhBlockGeom& g, int64_t mcu, int64_t s[3]) {
  s[0] = s[1] = s[2] = 0;
  for (int bi = 0; bi < g.bpm; ++bi) {
    const int64_t blk = dh_huff_block(g, mcu * g.bpm + bi);
    if (blk < 0) continue;
    const int comp = bi < g.nl ? 0 : bi - g.nl + 1;
    const int64_t d = c.load(blk, 0);
    s[0] += comp == 0 ? d : 0; s[1] += comp == 1 ? d : 0; s[2] += comp == 2 ? d : 0;
  }
}

// pred: the components' DC values before this MCU.  Returns non-zero when a DC value leaves int16 or a block's energy the bound.
template <class C>
DH_HD int dh_dc_mcu_apply(C& c, const DhBlockGeom& g, int64_t mcu, int64_t pred[3]) {
  int flag = 0;
  for (int bi = 0; bi < g.bpm; ++bi) {
    const int64_t blk = dh_huff_block(g, mcu * g.bpm + bi);
    if (blk < 0) { flag = 1; continue; }
    const int comp = bi < g.nl ? 0 : bi - g.nl + 1;
    const int64_t dc = (comp == 0 ? pred[0] : (comp == 1 ? pred[1] : pred[2])) + c.load(blk, 0);
    pred[0] = comp == 0 ? dc : pred[0]; pred[1] = comp == 1 ? dc : pred[1]; pred[2] = comp == 2 ? dc : pred[2];
    if (dc < -32768 || dc > 32767) { flag = 1; continue; }
    c.store(blk, 0, (int)dc);
    int64_t energy = 0;
    for (int el = 0; el < 64; ++el) {                                // el = col * 8 + row; the tables are row-major
      const int64_t dq = (int64_t)(el ? c.load(blk, el) : (int)dc) * (int64_t)c.quant(comp, (el & 7) * 8 + (el >> 3));
      energy += dq * dq;
    }
    if (energy > DANHIP_JPEG_MAX_BLOCK_ENERGY) flag = 1;
  }
  return flag;
}
