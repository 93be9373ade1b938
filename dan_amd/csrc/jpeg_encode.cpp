// Host half of the JPEG encoder (include/danhip.h, "Baseline JPEG encode"): descriptors, the Huffman stage, the file writer, and the pixel
// stage once more on the host through the arithmetic of jpeg_encode.h.  Plain C++: no HIP call, usable in a process without a GPU.
// The file is what libjpeg-turbo's jcmarker.c / jchuff.c write for Pillow's save(quality=q, subsampling=0 | 2): see jpeg_encode.h for the
// places where that is not the textbook.
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "jpeg_encode.h"
#include "jpeg_encode_huffman.h"
#include "jpeg_layout.h"

void danhip_set_error(const char* fmt, ...);

namespace {

const uint8_t kZigColMajor[64] = {0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,
                                  13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58,
                                  51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};   // k-th coded -> col * 8 + row
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};        // k-th coded -> row * 8 + col

// T.81 K.1 / K.2, row-major
const uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 K.3 - K.6: code counts per length 1 .. 16, then the symbols.  Order: DC luma, AC luma, DC chroma, AC chroma (the order of the DHT segments)
const uint8_t kBitsDcLuma[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kBitsDcChroma[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kValDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kBitsAcLuma[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kValAcLuma[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kBitsAcChroma[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kValAcChroma[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

struct EncTable {
  uint16_t code[256];
  uint8_t len[256];                                       // 0: the table has no code for the symbol
};

struct StdTables {
  EncTable dc[2], ac[2];
  StdTables() {
    build(kBitsDcLuma, kValDc, &dc[0]);
    build(kBitsAcLuma, kValAcLuma, &ac[0]);
    build(kBitsDcChroma, kValDc, &dc[1]);
    build(kBitsAcChroma, kValAcChroma, &ac[1]);
  }
  static void build(const uint8_t* bits, const uint8_t* vals, EncTable* t) {
    memset(t, 0, sizeof(*t));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
        t->code[vals[k]] = (uint16_t)code;
        t->len[vals[k]] = (uint8_t)l;
      }
      code <<= 1;
    }
  }
};

const StdTables& std_tables() {
  static const StdTables t;
  return t;
}

struct HuffSpec {                                         // one DHT segment's content: bits[l] codes of length l (bits[0] = 0), then the symbols
  uint8_t bits[17], vals[256];
};

// the four tables of one image in DHT order (DC luma, AC luma, DC chroma, AC chroma): what the markers carry and what the scan is coded with
struct ImageTables {
  HuffSpec spec[4];
  EncTable enc[4];
};

const int64_t kHeaderBound = 1024;                        // the markers in front of the scan take 623 bytes
const int64_t kBlockBound = 416;                          // (9 + 11) + 63 * (16 + 10) bits = 208 bytes, every one stuffed

bool enc_mode_ok(int32_t mode) { return mode == DANHIP_JPEG_420 || mode == DANHIP_JPEG_444; }

// everything of a descriptor that follows from (width, height, mode, quality); the offsets stay as they are
bool derive_desc(int32_t width, int32_t height, int32_t mode, int32_t quality, danhip_jpeg_enc_desc* d) {
  DhJpegGeom g;
  if (!enc_mode_ok(mode) || quality < 1 || quality > 100 || !dh_jpeg_geometry(width, height, mode, &g)) return false;
  d->width = width; d->height = height; d->mode = mode; d->quality = quality;
  for (int c = 0; c < 3; ++c) {
    d->blocks_w[c] = g.blocks_w[c]; d->blocks_h[c] = g.blocks_h[c]; d->comp_w[c] = g.comp_w[c]; d->comp_h[c] = g.comp_h[c];
  }
  d->real_bw = (width + 7) / 8;
  d->real_bh = (height + 7) / 8;
  const int64_t items = (int64_t)(g.blocks_h[0] * 8 / g.vs) * g.blocks_w[0];
  d->color_groups = (int32_t)((items + 255) / 256);
  d->fdct_groups = (int32_t)((g.blocks + DH_JPEG_IDCT_BLOCKS_PER_GROUP - 1) / DH_JPEG_IDCT_BLOCKS_PER_GROUP);
  d->coef_count = g.coef_count;
  d->file_capacity = kHeaderBound + g.blocks * kBlockBound;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;          // jpeg_quality_scaling
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      int q = (kStdQuant[t][k] * scale + 50) / 100;                             // jpeg_add_quant_table, force_baseline
      q = q < 1 ? 1 : (q > 255 ? 255 : q);
      d->qtable[t][k] = (uint8_t)q;
      dh_jenc_reciprocal((unsigned)q * 8, &d->recip[t][k], &d->corr[t][k], &d->shift[t][k]);
    }
  return true;
}

// NULL = the descriptor is what derive_desc gives and its offsets lie inside the buffers, else what is wrong
const char* check_desc(const danhip_jpeg_enc_desc* d, int64_t coef_count, int64_t workspace_bytes, int64_t file_bytes) {
  danhip_jpeg_enc_desc w;
  memset(&w, 0, sizeof(w));
  if (!derive_desc(d->width, d->height, d->mode, d->quality, &w)) return "size, mode or quality outside the accepted range";
  w.src = d->src; w.coef_offset = d->coef_offset; w.file_offset = d->file_offset;
  for (int c = 0; c < 3; ++c) w.plane_offset[c] = d->plane_offset[c];
  if (memcmp(&w, d, sizeof(w)) != 0) return "fields do not fit (width, height, mode, quality)";
  if (d->coef_offset < 0 || d->coef_offset % 64 || d->coef_offset > coef_count || d->coef_count > coef_count - d->coef_offset)
    return "coefficients leave the buffer";
  if (workspace_bytes >= 0)
    for (int c = 0; c < 3; ++c) {
      const int64_t bytes = (int64_t)d->blocks_w[c] * d->blocks_h[c] * 64;
      if (d->plane_offset[c] < 0 || d->plane_offset[c] % 256 || d->plane_offset[c] > workspace_bytes || bytes > workspace_bytes - d->plane_offset[c])
        return "component plane leaves the workspace";
    }
  if (file_bytes >= 0 && (d->file_offset < 0 || d->file_offset > file_bytes || d->file_capacity > file_bytes - d->file_offset))
    return "file leaves the file buffer";
  return nullptr;
}

struct BitWriter {
  uint8_t* p;
  uint8_t* end;
  uint64_t acc = 0;
  int n = 0;                                              // bits held in acc
  bool overflow = false;
  void byte(unsigned b) {
    if (p < end) *p++ = (uint8_t)b; else overflow = true;
  }
  void put(unsigned code, int len) {                      // len <= 27
    acc = (acc << len) | (code & ((1u << len) - 1));
    n += len;
    while (n >= 8) {
      const unsigned b = (unsigned)(acc >> (n - 8)) & 255;
      byte(b);
      if (b == 255) byte(0);
      n -= 8;
    }
  }
  void flush() {                                          // jchuff.c flush_bits: fill the last byte with ones
    if (n > 0) put(0x7f, 8 - n);
    acc = 0; n = 0;
  }
};

int bit_length(unsigned v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}

// one block (column-major, de-zigzagged) as jchuff.c encode_one_block codes it.  false: a value the baseline tables cannot carry
bool encode_block(const int16_t* blk, int* last_dc, const EncTable& dc, const EncTable& ac, BitWriter* w) {
  int diff = blk[0] - *last_dc;
  *last_dc = blk[0];
  int bits = diff < 0 ? diff - 1 : diff;                  // the low bits of the one's complement for a negative value
  int nb = bit_length((unsigned)(diff < 0 ? -diff : diff));
  if (nb > 11 || !dc.len[nb]) return false;
  w->put(dc.code[nb], dc.len[nb]);
  if (nb) w->put((unsigned)bits, nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kZigColMajor[k]];
    if (v == 0) { ++run; continue; }
    while (run > 15) { w->put(ac.code[0xf0], ac.len[0xf0]); run -= 16; }
    bits = v < 0 ? v - 1 : v;
    nb = bit_length((unsigned)(v < 0 ? -v : v));
    if (nb > 10) return false;
    const int sym = (run << 4) | nb;
    w->put(ac.code[sym], ac.len[sym]);
    w->put((unsigned)bits, nb);
    run = 0;
  }
  if (run > 0) w->put(ac.code[0], ac.len[0]);
  return true;
}

void put16(uint8_t*& p, unsigned v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; }

uint8_t* write_dht(uint8_t* p, int index, const uint8_t* bits, const uint8_t* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  put16(p, 0xffc4); put16(p, (unsigned)(2 + 1 + 16 + n));
  *p++ = (uint8_t)index;
  memcpy(p, bits, 16); p += 16;
  memcpy(p, vals, (size_t)n); p += n;
  return p;
}

// jcmarker.c: write_file_header, write_frame_header, write_scan_header for three components, tables 0 (Y) and 1 (Cb, Cr).
// own: the image's own tables (optimize), NULL: the standard ones.  The DHT segments keep their place and order either way.
uint8_t* write_header(uint8_t* p, const danhip_jpeg_enc_desc& d, const ImageTables* own = nullptr) {
  put16(p, 0xffd8);
  put16(p, 0xffe0); put16(p, 16);
  memcpy(p, "JFIF", 5); p += 5;
  *p++ = 1; *p++ = 1;                                     // version 1.01
  *p++ = 0; put16(p, 1); put16(p, 1);                     // density: unit 0, 1 : 1
  *p++ = 0; *p++ = 0;                                     // no thumbnail
  for (int t = 0; t < 2; ++t) {
    put16(p, 0xffdb); put16(p, 67);
    *p++ = (uint8_t)t;
    for (int k = 0; k < 64; ++k) *p++ = d.qtable[t][kZigzag[k]];
  }
  put16(p, 0xffc0); put16(p, 17);
  *p++ = 8; put16(p, (unsigned)d.height); put16(p, (unsigned)d.width); *p++ = 3;
  *p++ = 1; *p++ = d.mode == DANHIP_JPEG_420 ? 0x22 : 0x11; *p++ = 0;
  *p++ = 2; *p++ = 0x11; *p++ = 1;
  *p++ = 3; *p++ = 0x11; *p++ = 1;
  if (own) {
    for (int t = 0; t < 4; ++t) p = write_dht(p, ((t & 1) << 4) | (t >> 1), own->spec[t].bits + 1, own->spec[t].vals);
  } else {
    p = write_dht(p, 0x00, kBitsDcLuma, kValDc);
    p = write_dht(p, 0x10, kBitsAcLuma, kValAcLuma);
    p = write_dht(p, 0x01, kBitsDcChroma, kValDc);
    p = write_dht(p, 0x11, kBitsAcChroma, kValAcChroma);
  }
  put16(p, 0xffda); put16(p, 12);
  *p++ = 3; *p++ = 1; *p++ = 0x00; *p++ = 2; *p++ = 0x11; *p++ = 3; *p++ = 0x11;
  *p++ = 0; *p++ = 63; *p++ = 0;
  return p;
}

// every block of the image's one interleaved scan in the order it is written, dummy blocks included: f(block, component) until it is false
template <class F>
bool for_each_scan_block(const danhip_jpeg_enc_desc& d, const int16_t* coef, F f) {
  const int hs = d.mode == DANHIP_JPEG_420 ? 2 : 1, vs = hs;
  const int mcus_x = d.blocks_w[1], mcus_y = d.blocks_h[1];
  const int16_t* plane[3];
  plane[0] = coef;
  plane[1] = plane[0] + (int64_t)d.blocks_w[0] * d.blocks_h[0] * 64;
  plane[2] = plane[1] + (int64_t)d.blocks_w[1] * d.blocks_h[1] * 64;
  for (int my = 0; my < mcus_y; ++my)
    for (int mx = 0; mx < mcus_x; ++mx) {
      for (int v = 0; v < vs; ++v)
        for (int h = 0; h < hs; ++h) {
          const int64_t b = (int64_t)(my * vs + v) * d.blocks_w[0] + (mx * hs + h);
          if (!f(plane[0] + b * 64, 0)) return false;
        }
      for (int c = 1; c < 3; ++c)
        if (!f(plane[c] + ((int64_t)my * mcus_x + mx) * 64, c)) return false;
    }
  return true;
}

struct CountSink {                                        // dh_jhuf_symbols' sink over counts[4][257]
  int32_t (*counts)[257];
  void add(int t, int sym) { ++counts[t][sym]; }
};

// the gather pass of optimize: the statistics of the scan as it will be written.  false: a coefficient no baseline code carries
bool count_symbols(const danhip_jpeg_enc_desc& d, const int16_t* coef, int32_t counts[4][257]) {
  memset(counts, 0, sizeof(int32_t) * 4 * 257);
  CountSink sink{counts};
  int last_dc[3] = {0, 0, 0};
  return for_each_scan_block(d, coef, [&](const int16_t* blk, int c) {
    const int pred = last_dc[c];
    last_dc[c] = blk[0];
    return dh_jhuf_symbols(blk, pred, c, sink);
  });
}

// false: a merge chain longer than libjpeg takes (it fails there as well)
bool optimal_tables(const int32_t counts[4][257], ImageTables* T) {
  int32_t work[DH_JENC_TABLE_WORK];
  for (int t = 0; t < 4; ++t) {
    if (!dh_jenc_optimal_table(counts[t], T->spec[t].bits, T->spec[t].vals, work)) return false;
    StdTables::build(T->spec[t].bits + 1, T->spec[t].vals, &T->enc[t]);
  }
  return true;
}

// the file of one image from its coefficient slot; -1: capacity, -2: a coefficient the tables cannot carry, -3: no optimal table.
// optimize: the image's own tables from two passes over its coefficients (jchuff.c's gather pass, then the scan), else the standard ones.
// The capacity is checked, not assumed, in both forms.  The bound of danhip_jpeg_encode_file_bound covers the standard tables by
// construction; own tables carry at most as many symbols (12 DC, 162 AC), so their markers are no longer, and their scan is shorter.
int64_t write_file(const danhip_jpeg_enc_desc& d, const int16_t* coef, uint8_t* out, int64_t capacity, bool optimize = false) {
  if (capacity < kHeaderBound) return -1;
  const StdTables& S = std_tables();
  const EncTable* dc[2] = {&S.dc[0], &S.dc[1]};
  const EncTable* ac[2] = {&S.ac[0], &S.ac[1]};
  ImageTables own;
  if (optimize) {
    int32_t counts[4][257];
    if (!count_symbols(d, coef, counts)) return -2;
    if (!optimal_tables(counts, &own)) return -3;
    dc[0] = &own.enc[0]; ac[0] = &own.enc[1]; dc[1] = &own.enc[2]; ac[1] = &own.enc[3];
  }
  uint8_t* p = write_header(out, d, optimize ? &own : nullptr);
  BitWriter w;
  w.p = p; w.end = out + capacity - 2;
  int last_dc[3] = {0, 0, 0};
  const bool coded = for_each_scan_block(d, coef, [&](const int16_t* blk, int c) {
    const int t = c == 0 ? 0 : 1;
    return encode_block(blk, &last_dc[c], *dc[t], *ac[t], &w);
  });
  if (!coded) return -2;
  w.flush();
  if (w.overflow) return -1;
  p = w.p;
  put16(p, 0xffd9);
  return p - out;
}

// the pixel stage of one image on the host: planes as the device makes them, then block by block
void pixels_host(const danhip_jpeg_enc_desc& d, int16_t* coef) {
  const int W = d.width, H = d.height;
  const bool sub = d.mode == DANHIP_JPEG_420;
  std::vector<uint8_t> planes[3];
  int pitch[3];
  for (int c = 0; c < 3; ++c) {
    pitch[c] = d.blocks_w[c] * 8;
    planes[c].resize((size_t)pitch[c] * d.blocks_h[c] * 8);
  }
  auto ycc = [&](int y, int x, int* yy, int* cb, int* cr) {
    const uint8_t* px = d.src + ((int64_t)(y < H ? y : H - 1) * W + (x < W ? x : W - 1)) * 3;
    dh_jenc_ycc(px[0], px[1], px[2], yy, cb, cr);
  };
  for (int y = 0; y < d.blocks_h[0] * 8; ++y)
    for (int x = 0; x < pitch[0]; ++x) {
      int yy, cb, cr;
      ycc(y, x, &yy, &cb, &cr);
      planes[0].at((size_t)y * pitch[0] + x) = (uint8_t)yy;
      if (!sub) {
        planes[1].at((size_t)y * pitch[1] + x) = (uint8_t)cb;
        planes[2].at((size_t)y * pitch[2] + x) = (uint8_t)cr;
      }
    }
  if (sub)
    for (int cy = 0; cy < d.blocks_h[1] * 8; ++cy)
      for (int cx = 0; cx < pitch[1]; ++cx) {
        const int ry = cy < d.comp_h[1] ? cy : d.comp_h[1] - 1;                 // the component's last row, repeated
        int yy, cb[4], cr[4];
        for (int k = 0; k < 4; ++k) ycc(2 * ry + (k >> 1), 2 * cx + (k & 1), &yy, &cb[k], &cr[k]);
        planes[1].at((size_t)cy * pitch[1] + cx) = (uint8_t)dh_jenc_h2v2(cb[0], cb[1], cb[2], cb[3], cx);
        planes[2].at((size_t)cy * pitch[2] + cx) = (uint8_t)dh_jenc_h2v2(cr[0], cr[1], cr[2], cr[3], cx);
      }
  int16_t* out = coef;
  for (int c = 0; c < 3; ++c) {
    const int t = c == 0 ? 0 : 1;
    for (int by = 0; by < d.blocks_h[c]; ++by)
      for (int bx = 0; bx < d.blocks_w[c]; ++bx, out += 64) {
        int sy = by, sx = bx;
        const int dummy = c == 0 ? dh_jenc_block_source(by, bx, d.real_bw, d.real_bh, &sy, &sx) : 0;
        int m[8][8];
        for (int r = 0; r < 8; ++r) {
          for (int k = 0; k < 8; ++k) m[r][k] = (int)planes[c].at((size_t)(sy * 8 + r) * pitch[c] + sx * 8 + k) - 128;
          dh_jenc_fdct_1d(m[r], 1);
        }
        for (int j = 0; j < 8; ++j) {
          int col[8];
          for (int r = 0; r < 8; ++r) col[r] = m[r][j];
          dh_jenc_fdct_1d(col, 0);
          for (int r = 0; r < 8; ++r) {
            const int k = r * 8 + j;
            const int q = dh_jenc_quant(col[r], d.recip[t][k], d.corr[t][k], d.shift[t][k]);
            out[j * 8 + r] = (int16_t)((dummy && k != 0) ? 0 : q);
          }
        }
      }
  }
}


// ---- Huffman stage on the device: the staging buffer (jpeg_encode_huffman.h) and the phases on the host ----

int64_t align16(int64_t v) { return dh_jpeg_align(v, 16); }

size_t scan_staging_bytes(int32_t B) {
  return (size_t)(align16(sizeof(DhJencHeader)) + align16((int64_t)B * (int64_t)sizeof(DhJencImage)) + 4 * 256 * 4 + (int64_t)B * DH_JHUF_HEADER_SLOT);
}

// fills `staging` (scan_staging_bytes(B) bytes) from checked descriptors; status may be NULL.  optimize (0 | 1) changes two things: the
// header's word, and the workspace, whose first B * DH_JHUF_OPT_STRIDE bytes then hold the images' statistics, tables and markers (the
// staged standard tables and markers stay: the table launch takes the markers around the DHT segments from them).
void fill_staging(const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count, int64_t file_bytes, uint8_t* staging, int32_t* status,
                  int32_t optimize = 0) {
  const size_t bytes = scan_staging_bytes(B);
  memset(staging, 0, bytes);
  DhJencHeader* H = (DhJencHeader*)staging;
  H->magic = DH_JHUF_MAGIC;
  H->B = B;
  H->optimize = optimize;
  H->off_images = align16(sizeof(DhJencHeader));
  H->off_tabs = H->off_images + align16((int64_t)B * (int64_t)sizeof(DhJencImage));
  H->off_headers = H->off_tabs + 4 * 256 * 4;
  H->used_bytes = (int64_t)bytes;
  H->coef_count = coef_count;
  H->file_bytes = file_bytes;
  const StdTables& T = std_tables();
  const EncTable* tabs[4] = {&T.dc[0], &T.ac[0], &T.dc[1], &T.ac[1]};
  uint32_t* tab = (uint32_t*)(staging + H->off_tabs);
  for (int t = 0; t < 4; ++t)
    for (int k = 0; k < 256; ++k) tab[t * 256 + k] = (uint32_t)tabs[t]->code[k] | ((uint32_t)tabs[t]->len[k] << 16);
  DhJencImage* images = (DhJencImage*)(staging + H->off_images);
  int64_t ws = optimize ? (int64_t)B * DH_JHUF_OPT_STRIDE : 0;
  for (int32_t i = 0; i < B; ++i) {
    const danhip_jpeg_enc_desc& d = descs[i];
    DhJencImage& im = images[i];
    im.coef_offset = d.coef_offset; im.coef_count = d.coef_count;
    im.file_offset = d.file_offset; im.file_capacity = d.file_capacity;
    if (d.file_capacity >= DH_JHUF_MAX_FILE) {
      if (status) status[i] = DANHIP_JPEG_HOSTONLY;
      continue;
    }
    if (status) status[i] = 0;
    im.prepared = 1;
    im.hs = d.mode == DANHIP_JPEG_420 ? 2 : 1;
    im.nl = im.hs * im.hs;
    im.bpm = im.nl + 2;
    im.mcus_x = d.blocks_w[1]; im.mcus_y = d.blocks_h[1];
    im.bw0 = d.blocks_w[0];
    im.nblocks = (int64_t)im.mcus_x * im.mcus_y * im.bpm;
    im.plane[0] = d.coef_offset;
    im.plane[1] = im.plane[0] + (int64_t)d.blocks_w[0] * d.blocks_h[0] * 64;
    im.plane[2] = im.plane[1] + (int64_t)d.blocks_w[1] * d.blocks_h[1] * 64;
    im.header_off = H->off_headers + (int64_t)i * DH_JHUF_HEADER_SLOT;
    im.header_len = (int32_t)(write_header(staging + im.header_off, d) - (staging + im.header_off));
    im.len_groups = (int32_t)((im.nblocks + DH_JHUF_GROUP - 1) / DH_JHUF_GROUP);
    im.bits_bytes = (int64_t)im.len_groups * DH_JHUF_GROUP * DH_JHUF_BLOCK_BYTES;
    im.stuff_groups = (int32_t)((im.bits_bytes + DH_JHUF_CHUNK_BYTES - 1) / DH_JHUF_CHUNK_BYTES);
    im.ws_gsum = ws; ws += align16((int64_t)im.len_groups * 8);
    im.ws_goff = ws; ws += align16(((int64_t)im.len_groups + 1) * 8);
    im.ws_bits = ws; ws += align16(im.bits_bytes);
    im.ws_ff = ws; ws += align16((int64_t)im.stuff_groups * 4);
    im.ws_ffoff = ws; ws += align16((int64_t)im.stuff_groups * 4);
    H->nprepared += 1;
    H->max_len_groups = im.len_groups > H->max_len_groups ? im.len_groups : H->max_len_groups;
    H->max_stuff_groups = im.stuff_groups > H->max_stuff_groups ? im.stuff_groups : H->max_stuff_groups;
  }
  H->workspace_bytes = ws;
}

static_assert(623 <= DH_JHUF_HEADER_SLOT, "the markers fit their staged slot");
static_assert(DH_JHUF_HEADER_PRE + 2 * (21 + 12) + 2 * (21 + 162) + DH_JHUF_HEADER_SOS == 623, "the markers around the DHT segments");

// NULL = staging is what fill_staging makes of these descriptors and buffer sizes, else what is wrong
const char* check_staging(const void* staging, size_t staging_bytes, const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count,
                          int64_t file_bytes) {
  if (staging_bytes < scan_staging_bytes(B)) return "staging buffer shorter than danhip_jpeg_encode_scan_staging_bytes(B)";
  for (int32_t i = 0; i < B; ++i) {
    const char* why = check_desc(&descs[i], coef_count, -1, file_bytes);
    if (why) return why;
  }
  const int32_t optimize = ((const DhJencHeader*)staging)->optimize;
  if (optimize != 0 && optimize != 1) return "staging buffer is not what danhip_jpeg_encode_scan_prepare makes of the descriptors";
  std::vector<uint8_t> again(scan_staging_bytes(B));
  fill_staging(descs, B, coef_count, file_bytes, again.data(), nullptr, optimize);
  if (memcmp(again.data(), staging, again.size()) != 0) return "staging buffer is not what danhip_jpeg_encode_scan_prepare makes of the descriptors";
  return nullptr;
}

// the context of jpeg_encode_huffman.h over host arrays: every index checked, a refused one counted
struct EmuCtx {
  const uint8_t* staging;
  const DhJencHeader* H;
  const int16_t* coef;
  std::vector<uint8_t>* ws;
  uint8_t* files;
  int64_t errors = 0;
  void load_block(int64_t el, int16_t v[64]) {
    if (el < 0 || el + 64 > H->coef_count) { ++errors; memset(v, 0, 128); return; }
    memcpy(v, coef + el, 128);
  }
  int dc(int64_t el) {
    if (el < 0 || el >= H->coef_count) { ++errors; return 0; }
    return coef[el];
  }
  uint32_t tab(int t, int sym) {
    if (t < 0 || t > 3 || sym < 0 || sym > 255) { ++errors; return 0; }
    return ((const uint32_t*)(staging + H->off_tabs))[t * 256 + sym];
  }
  void or_word(const DhJencImage& im, int64_t w, uint32_t v) {
    if (w < 0 || w >= im.bits_bytes / 4) { ++errors; return; }
    uint8_t* p = &ws->at((size_t)(im.ws_bits + w * 4));
    p[0] |= (uint8_t)(v >> 24); p[1] |= (uint8_t)(v >> 16); p[2] |= (uint8_t)(v >> 8); p[3] |= (uint8_t)v;
  }
  uint32_t ubyte(const DhJencImage& im, int64_t i) {
    if (i < 0 || i >= im.bits_bytes) { ++errors; return 0; }
    return ws->at((size_t)(im.ws_bits + i));
  }
  void file_store(const DhJencImage& im, int64_t i, uint32_t b) {
    if (i < 0 || i >= im.file_capacity || im.file_offset + i >= H->file_bytes) { ++errors; return; }
    files[im.file_offset + i] = (uint8_t)b;
  }
  uint32_t header_byte(const DhJencImage& im, int i) {
    if (i < 0 || i >= im.header_len) { ++errors; return 0; }
    return staging[im.header_off + i];
  }
  template <class T>
  T* array(int64_t off, int64_t n) {                      // n elements of the workspace at byte off; NULL and an error when they leave it
    if (off < 0 || n < 0 || off % (int64_t)sizeof(T) || off + n * (int64_t)sizeof(T) > (int64_t)ws->size()) { ++errors; return nullptr; }
    return (T*)(ws->data() + off);
  }
};

// the six launches of jpeg_encode_huffman_exact.hip for one image, workgroup by workgroup and lane by lane
void emulate_image(EmuCtx& c, const DhJencImage& im, int64_t* size_out, int32_t* status_out) {
  uint64_t* gsum = c.array<uint64_t>(im.ws_gsum, im.len_groups);
  uint64_t* goff = c.array<uint64_t>(im.ws_goff, (int64_t)im.len_groups + 1);
  uint32_t* ff = c.array<uint32_t>(im.ws_ff, im.stuff_groups);
  uint32_t* ffoff = c.array<uint32_t>(im.ws_ffoff, im.stuff_groups);
  uint8_t* bits = c.array<uint8_t>(im.ws_bits, im.bits_bytes);
  if (!gsum || !goff || !ff || !ffoff || !bits) { *size_out = 0; *status_out = DANHIP_JPEG_ENC_DEV_CAPACITY; return; }
  // 1 length (and the zero fill)
  memset(bits, 0, (size_t)im.bits_bytes);
  for (int32_t g = 0; g < im.len_groups; ++g) {
    uint64_t sum = 0;
    for (int lane = 0; lane < DH_JHUF_GROUP; ++lane) {
      const int64_t s = (int64_t)g * DH_JHUF_GROUP + lane;
      if (s >= im.nblocks) break;
      const uint64_t len = dh_jhuf_lane_length(c, im, s);
      if (len & DH_JHUF_INVALID) sum |= DH_JHUF_INVALID;             // the flag is OR-ed, the bits (0 for such a block) are added
      else sum += len;
    }
    gsum[g] = sum;
  }
  // 2 offsets
  uint64_t at = 0;
  int32_t status = 0;
  for (int32_t g = 0; g < im.len_groups; ++g) {
    goff[g] = at;
    if (gsum[g] & DH_JHUF_INVALID) status |= DANHIP_JPEG_ENC_DEV_RANGE;
    at += gsum[g] & ~DH_JHUF_INVALID;
  }
  goff[im.len_groups] = at;
  // 3 write
  for (int32_t g = 0; g < im.len_groups; ++g) {
    uint64_t bit = goff[g];
    for (int lane = 0; lane < DH_JHUF_GROUP; ++lane) {
      const int64_t s = (int64_t)g * DH_JHUF_GROUP + lane;
      if (s >= im.nblocks) break;
      const uint64_t len = dh_jhuf_lane_length(c, im, s);
      dh_jhuf_lane_write(c, im, s, bit, len);
      bit += len & ~DH_JHUF_INVALID;
    }
  }
  // 4 count
  const int64_t scan_bytes = dh_jhuf_scan_bytes(im, goff[im.len_groups]);
  const int32_t chunks = (int32_t)((scan_bytes + DH_JHUF_CHUNK_BYTES - 1) / DH_JHUF_CHUNK_BYTES);
  for (int32_t g = 0; g < chunks && g < im.stuff_groups; ++g) {
    uint32_t n = 0;
    for (int lane = 0; lane < DH_JHUF_GROUP; ++lane)
      n += dh_jhuf_lane_ffcount(c, im, scan_bytes, (int64_t)g * DH_JHUF_CHUNK_BYTES + (int64_t)lane * DH_JHUF_LANE_BYTES);
    ff[g] = n;
  }
  // 5 finish
  uint32_t total_ff = 0;
  for (int32_t g = 0; g < chunks && g < im.stuff_groups; ++g) { ffoff[g] = total_ff; total_ff += ff[g]; }
  int64_t size = 0;
  const bool fits = (int64_t)im.header_len + scan_bytes + total_ff + 2 <= im.file_capacity;
  if (!fits) status |= DANHIP_JPEG_ENC_DEV_CAPACITY;
  else
    for (int lane = 0; lane < DH_JHUF_GROUP; ++lane) size = dh_jhuf_lane_finish(c, im, scan_bytes, total_ff, lane, DH_JHUF_GROUP);
  // 6 stuff
  if (fits)
    for (int32_t g = 0; g < chunks && g < im.stuff_groups; ++g) {
      uint32_t before = ffoff[g];
      for (int lane = 0; lane < DH_JHUF_GROUP; ++lane) {
        const int64_t byte0 = (int64_t)g * DH_JHUF_CHUNK_BYTES + (int64_t)lane * DH_JHUF_LANE_BYTES;
        dh_jhuf_lane_scatter(c, im, scan_bytes, byte0, before);
        before += dh_jhuf_lane_ffcount(c, im, scan_bytes, byte0);
      }
    }
  *status_out = status;
  *size_out = status ? 0 : size;
}

}  // namespace

extern "C" size_t danhip_jpeg_enc_desc_bytes(void) { return sizeof(danhip_jpeg_enc_desc); }

extern "C" int64_t danhip_jpeg_encode_file_bound(int32_t width, int32_t height, int32_t mode) {
  DhJpegGeom g;
  if (!enc_mode_ok(mode) || !dh_jpeg_geometry(width, height, mode, &g)) return 0;
  return kHeaderBound + g.blocks * kBlockBound;
}

extern "C" int danhip_jpeg_encode_prepare(const int32_t* widths, const int32_t* heights, const void* const* srcs, int32_t B, int32_t mode,
                                          int32_t quality, danhip_jpeg_enc_desc* descs_out, int64_t* totals_out) {
  if (!widths || !heights || !descs_out || !totals_out || B < 1 || B > 65535) {
    danhip_set_error("jpeg_encode_prepare: bad arguments (1 <= B <= 65535, no NULL table)");
    return DANHIP_EINVAL;
  }
  if (!enc_mode_ok(mode) || quality < 1 || quality > 100) {
    danhip_set_error("jpeg_encode_prepare: mode %d / quality %d (DANHIP_JPEG_444 or DANHIP_JPEG_420, quality 1 .. 100)", mode, quality);
    return DANHIP_EINVAL;
  }
  int64_t coef = 0, ws = 0, file = 0;
  for (int32_t i = 0; i < B; ++i) {
    danhip_jpeg_enc_desc* d = &descs_out[i];
    memset(d, 0, sizeof(*d));
    if (!derive_desc(widths[i], heights[i], mode, quality, d)) {
      danhip_set_error("jpeg_encode_prepare: image %d is %d x %d (sides 1 .. %d)", i, widths[i], heights[i], DANHIP_JPEG_MAX_DIM);
      return DANHIP_EINVAL;
    }
    d->src = srcs ? (const uint8_t*)srcs[i] : nullptr;
    d->coef_offset = coef;
    coef += d->coef_count;
    for (int c = 0; c < 3; ++c) {
      d->plane_offset[c] = ws;
      ws += dh_jpeg_align((int64_t)d->blocks_w[c] * d->blocks_h[c] * 64, 256);
    }
    d->file_offset = file;
    file += d->file_capacity;
  }
  totals_out[0] = coef; totals_out[1] = ws; totals_out[2] = file;
  return DANHIP_OK;
}

// the check of the device launcher (jpeg_encode_exact.hip), here because the derivation is
extern "C" const char* danhip_jpeg_enc_desc_check(const danhip_jpeg_enc_desc* d, int64_t coef_count, int64_t workspace_bytes, int64_t file_bytes) {
  return check_desc(d, coef_count, workspace_bytes, file_bytes);
}

extern "C" int danhip_jpeg_encode_pixels_host(const danhip_jpeg_enc_desc* descs, int32_t B, int16_t* coef_out, int64_t coef_count) {
  if (!descs || !coef_out || B < 1 || B > 65535 || coef_count < 0) {
    danhip_set_error("jpeg_encode_pixels_host: bad arguments");
    return DANHIP_EINVAL;
  }
  for (int32_t i = 0; i < B; ++i) {
    const char* why = check_desc(&descs[i], coef_count, -1, -1);
    if (!why && !descs[i].src) why = "src is NULL";
    if (why) {
      danhip_set_error("jpeg_encode_pixels_host: descriptor %d: %s", i, why);
      return DANHIP_EINVAL;
    }
  }
  for (int32_t i = 0; i < B; ++i) pixels_host(descs[i], coef_out + descs[i].coef_offset);
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_optimal_table_host(const int32_t counts[257], uint8_t bits_out[17], uint8_t vals_out[256]) {
  if (!counts || !bits_out || !vals_out) {
    danhip_set_error("jpeg_optimal_table_host: NULL table");
    return DANHIP_EINVAL;
  }
  int64_t sum = 0;
  for (int i = 0; i < 256; ++i) sum += counts[i] > 0 ? counts[i] : 0;
  int32_t work[DH_JENC_TABLE_WORK];
  if (sum >= 0x7fffffff || !dh_jenc_optimal_table(counts, bits_out, vals_out, work)) {
    danhip_set_error("jpeg_optimal_table_host: the counts sum to 2^31 - 1 or more, or give a code of more than 32 bits before the cut to 16");
    return DANHIP_EINVAL;
  }
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_encode_optimize_layout(int32_t out[8]) {
  if (!out) return DH_JHUF_OPT_STRIDE;
  out[0] = DH_JHUF_OPT_STRIDE; out[1] = DH_JHUF_OPT_COUNTS; out[2] = DH_JHUF_OPT_TABS; out[3] = DH_JHUF_OPT_BITSVALS;
  out[4] = DH_JHUF_OPT_WORDS; out[5] = DH_JHUF_OPT_HEADER; out[6] = DH_JHUF_HIST_BLOCKS; out[7] = DH_JHUF_OPT_HEADER_MAX;
  return DH_JHUF_OPT_STRIDE;
}

extern "C" int danhip_jpeg_encode_entropy_batch(const int16_t* coef, int64_t coef_count, const danhip_jpeg_enc_desc* descs, int32_t B,
                                                int32_t threads, uint8_t* files_out, int64_t files_capacity, int64_t* sizes_out) {
  return danhip_jpeg_encode_entropy_batch_ex(coef, coef_count, descs, B, threads, 0, files_out, files_capacity, sizes_out);
}

extern "C" int danhip_jpeg_encode_entropy_batch_ex(const int16_t* coef, int64_t coef_count, const danhip_jpeg_enc_desc* descs, int32_t B,
                                                   int32_t threads, int32_t flags, uint8_t* files_out, int64_t files_capacity,
                                                   int64_t* sizes_out) {
  if (!coef || !descs || !files_out || !sizes_out || B < 1 || B > 65535 || coef_count < 0 || files_capacity < 0) {
    danhip_set_error("jpeg_encode_entropy_batch: bad arguments (1 <= B <= 65535, no NULL buffer)");
    return DANHIP_EINVAL;
  }
  if (flags & ~DANHIP_JPEG_ENC_OPTIMIZE) {
    danhip_set_error("jpeg_encode_entropy_batch_ex: flags %d (DANHIP_JPEG_ENC_OPTIMIZE or 0)", flags);
    return DANHIP_EINVAL;
  }
  const bool optimize = (flags & DANHIP_JPEG_ENC_OPTIMIZE) != 0;
  for (int32_t i = 0; i < B; ++i) {
    const char* why = check_desc(&descs[i], coef_count, -1, files_capacity);
    if (why) {
      danhip_set_error("jpeg_encode_entropy_batch: descriptor %d: %s", i, why);
      return DANHIP_EINVAL;
    }
  }
  int T = threads < 1 ? 1 : threads;
  if (T > DANHIP_JPEG_MAX_THREADS) T = DANHIP_JPEG_MAX_THREADS;
  if (T > B) T = B;
  std::atomic<int32_t> cursor(0);
  auto work = [&]() {
    for (;;) {
      const int32_t i = cursor.fetch_add(1);
      if (i >= B) return;
      sizes_out[i] = write_file(descs[i], coef + descs[i].coef_offset, files_out + descs[i].file_offset, descs[i].file_capacity, optimize);
    }
  };
  if (T == 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
  }
  for (int32_t i = 0; i < B; ++i)
    if (sizes_out[i] < 0) {
      danhip_set_error("jpeg_encode_entropy_batch: image %d: %s", i,
                       sizes_out[i] == -2   ? "a coefficient outside what the baseline tables carry (DC difference 11 bits, AC 10 bits)"
                       : sizes_out[i] == -3 ? "symbol statistics without an optimal table (a code of more than 32 bits before the cut to 16)"
                                            : "file capacity");
      return DANHIP_EINVAL;
    }
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_encode_host(const uint8_t* rgb, int32_t width, int32_t height, int32_t mode, int32_t quality, uint8_t* out,
                                       int64_t capacity, int64_t* size_out) {
  if (!rgb || !out || !size_out || capacity < 0) {
    danhip_set_error("jpeg_encode_host: NULL buffer");
    return DANHIP_EINVAL;
  }
  danhip_jpeg_enc_desc d;
  int64_t totals[3];
  const void* src = rgb;
  const int rc = danhip_jpeg_encode_prepare(&width, &height, &src, 1, mode, quality, &d, totals);
  if (rc) return rc;
  std::vector<int16_t> coef((size_t)totals[0]);
  pixels_host(d, coef.data());
  std::vector<uint8_t> file((size_t)d.file_capacity);
  const int64_t n = write_file(d, coef.data(), file.data(), d.file_capacity);
  if (n < 0) {
    danhip_set_error("jpeg_encode_host: internal: the scan left its bound");
    return DANHIP_EINVAL;
  }
  *size_out = n;
  if (n > capacity) {
    danhip_set_error("jpeg_encode_host: the file takes %lld bytes, capacity is %lld", (long long)n, (long long)capacity);
    return DANHIP_EWORKSPACE;
  }
  memcpy(out, file.data(), (size_t)n);
  return DANHIP_OK;
}

extern "C" size_t danhip_jpeg_encode_scan_staging_bytes(int32_t B) { return B < 1 || B > 65535 ? 0 : scan_staging_bytes(B); }

extern "C" int danhip_jpeg_encode_scan_prepare(const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count, int64_t file_bytes, void* staging,
                                               size_t staging_bytes, int32_t* status_out) {
  return danhip_jpeg_encode_scan_prepare_ex(descs, B, coef_count, file_bytes, 0, staging, staging_bytes, status_out);
}

extern "C" int danhip_jpeg_encode_scan_prepare_ex(const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count, int64_t file_bytes,
                                                  int32_t flags, void* staging, size_t staging_bytes, int32_t* status_out) {
  if (flags & ~DANHIP_JPEG_ENC_OPTIMIZE) {
    danhip_set_error("jpeg_encode_scan_prepare_ex: flags %d (DANHIP_JPEG_ENC_OPTIMIZE or 0)", flags);
    return DANHIP_EINVAL;
  }
  if (!descs || !staging || !status_out || B < 1 || B > 65535 || coef_count < 0 || file_bytes < 0 || ((uintptr_t)staging & 15) ||
      staging_bytes < scan_staging_bytes(B)) {
    danhip_set_error("jpeg_encode_scan_prepare: bad arguments (1 <= B <= 65535, no NULL table, staging 16-byte aligned and at least "
                     "danhip_jpeg_encode_scan_staging_bytes(B) bytes)");
    return DANHIP_EINVAL;
  }
  for (int32_t i = 0; i < B; ++i) {
    const char* why = check_desc(&descs[i], coef_count, -1, file_bytes);
    if (why) {
      danhip_set_error("jpeg_encode_scan_prepare: descriptor %d: %s", i, why);
      return DANHIP_EINVAL;
    }
  }
  fill_staging(descs, B, coef_count, file_bytes, (uint8_t*)staging, status_out, (flags & DANHIP_JPEG_ENC_OPTIMIZE) ? 1 : 0);
  return DANHIP_OK;
}

extern "C" size_t danhip_jpeg_encode_scan_workspace_bytes(const void* staging) {
  const DhJencHeader* H = (const DhJencHeader*)staging;
  if (!H || H->magic != DH_JHUF_MAGIC || H->workspace_bytes < 0) return 0;
  return (size_t)H->workspace_bytes;
}

// the check of the device launcher (jpeg_encode_huffman_exact.hip), here because the derivation is
extern "C" const char* danhip_jpeg_encode_scan_check(const void* staging, size_t staging_bytes, const danhip_jpeg_enc_desc* descs, int32_t B,
                                                     int64_t coef_count, int64_t file_bytes) {
  return check_staging(staging, staging_bytes, descs, B, coef_count, file_bytes);
}

extern "C" int danhip_jpeg_encode_entropy_emulate_batch(const void* staging, size_t staging_bytes, const danhip_jpeg_enc_desc* descs, int32_t B,
                                                        const int16_t* coef, int64_t coef_count, uint8_t* files_out, int64_t file_bytes,
                                                        int64_t* sizes_out, int32_t* status_out, int64_t* range_errors) {
  if (range_errors) *range_errors = 0;
  if (!staging || !descs || !coef || !files_out || !sizes_out || !status_out || B < 1 || B > 65535 || coef_count < 0 || file_bytes < 0 ||
      ((uintptr_t)staging & 15)) {
    danhip_set_error("jpeg_encode_entropy_emulate_batch: bad arguments (1 <= B <= 65535, no NULL buffer, staging 16-byte aligned)");
    return DANHIP_EINVAL;
  }
  const char* why = check_staging(staging, staging_bytes, descs, B, coef_count, file_bytes);
  if (why) {
    danhip_set_error("jpeg_encode_entropy_emulate_batch: %s", why);
    return DANHIP_EINVAL;
  }
  const DhJencHeader* H = (const DhJencHeader*)staging;
  if (H->optimize) {
    danhip_set_error("jpeg_encode_entropy_emulate_batch: a staging buffer prepared with DANHIP_JPEG_ENC_OPTIMIZE is not emulated (the "
                     "statistics and the table rule have host entry points of their own)");
    return DANHIP_EINVAL;
  }
  const DhJencImage* images = (const DhJencImage*)((const uint8_t*)staging + H->off_images);
  std::vector<uint8_t> ws((size_t)H->workspace_bytes, (uint8_t)0xa5);       // exactly the queried size, not zeroed: the phases own every byte they read
  EmuCtx c;
  c.staging = (const uint8_t*)staging; c.H = H; c.coef = coef; c.ws = &ws; c.files = files_out;
  for (int32_t i = 0; i < B; ++i) {
    if (!images[i].prepared) { sizes_out[i] = 0; status_out[i] = DANHIP_JPEG_HOSTONLY; continue; }
    emulate_image(c, images[i], &sizes_out[i], &status_out[i]);
  }
  if (range_errors) *range_errors = c.errors;
  return DANHIP_OK;
}
