// Host half of the JPEG decoder (include/danhip.h, "Baseline JPEG decode"): marker parsing, validation and Huffman decoding of baseline
// streams - and, where the caller allows them, of complete progressive streams ("Progressive streams") - into de-zigzagged, column-major
// int16 coefficient blocks plus one descriptor per image for the two device launches of jpeg_exact.hip.  Plain C++: no HIP call, usable
// in a process without a GPU.  A malformed stream ends here as a reason code; nothing
// read from a file becomes an index on the device - the descriptors carry geometry derived from (width, height, mode) by jpeg_layout.h.
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "jpeg_layout.h"

void danhip_set_error(const char* fmt, ...);

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};   // k-th coded -> row * 8 + col
const uint8_t kZigColMajor[64] = {0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,
                                  13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58,
                                  51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};   // (kZigzag[k] & 7) * 8 + (kZigzag[k] >> 3)

struct Huff {
  bool defined = false;
  uint16_t look[512];        // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits
  int32_t maxcode[18];       // largest code of each length, -1 = none
  int32_t valoff[17];        // symbol index of a length's first code minus that code
  uint8_t sym[256];
};

struct Header {
  int32_t width = 0, height = 0, ncomp = 0, mode = 0;
  int32_t tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  int32_t restart = 0;
  uint16_t quant[4][64];
  bool quant_defined[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int64_t scan = 0;          // first byte of the entropy-coded segment; of a progressive frame: the FF of its first SOS marker
  bool progressive = false;  // SOF2 (only with DANHIP_JPEG_ALLOW_PROGRESSIVE): dc / ac / restart are the state at the first SOS
  int32_t ids[3] = {0, 0, 0};
};

bool build_huff(const uint8_t* counts, const uint8_t* syms, int n, bool is_dc, Huff* h) {
  int32_t code = 0, k = 0;
  memset(h->look, 0, sizeof(h->look));
  for (int l = 1; l <= 16; ++l) {
    h->valoff[l] = k - code;
    for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
      if (code >= (1 << l)) return false;                       // the counts do not describe a prefix code
      if (is_dc && syms[k] > 11) return false;                  // an 8-bit DC difference has at most 11 bits
      if (l <= 9)
        for (int f = 0; f < (1 << (9 - l)); ++f) h->look[(code << (9 - l)) | f] = (uint16_t)((l << 8) | syms[k]);
    }
    h->maxcode[l] = counts[l - 1] ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[17] = 0x7fffffff;
  memcpy(h->sym, syms, n);
  h->defined = true;
  return true;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

int parse_dht(const uint8_t* s, int L, Header* H) {
  int q = 0;
  while (q < L) {
    if (q + 17 > L) return DANHIP_JPEG_ETABLE;
    const int tc = s[q] >> 4, t = s[q] & 15;
    int cnt = 0;
    for (int i = 0; i < 16; ++i) cnt += s[q + 1 + i];
    if (tc > 1 || t > 3 || cnt > 256 || q + 17 + cnt > L) return DANHIP_JPEG_ETABLE;
    if (!build_huff(s + q + 1, s + q + 17, cnt, tc == 0, tc ? &H->ac[t] : &H->dc[t])) return DANHIP_JPEG_ETABLE;
    q += 17 + cnt;
  }
  return 0;
}

// Markers up to and including SOS (of a progressive frame: up to its first SOS; prog_walk goes on from there).  0 = a stream the device
// path decodes.  flags: DANHIP_JPEG_ALLOW_PROGRESSIVE or 0.
int parse_header(const uint8_t* d, int64_t n, Header* H, uint32_t flags = 0) {
  if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return DANHIP_JPEG_ENOTJPEG;
  int64_t p = 2;
  bool have_sof = false;
  int adobe_transform = -1, hv[3] = {0, 0, 0};
  int32_t* ids = H->ids;
  for (;;) {
    if (p >= n) return DANHIP_JPEG_ETRUNCATED;
    if (d[p] != 0xFF) return DANHIP_JPEG_ENOTJPEG;
    const int64_t mark = p;
    while (p < n && d[p] == 0xFF) ++p;                          // fill bytes
    if (p >= n) return DANHIP_JPEG_ETRUNCATED;
    const int m = d[p++];
    if (m == 0x00) return DANHIP_JPEG_ENOTJPEG;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;         // TEM / stray RSTn: no payload
    if (m == 0xD8) return DANHIP_JPEG_ENOTJPEG;
    if (m == 0xD9) return DANHIP_JPEG_ETRUNCATED;               // EOI before any scan
    if (p + 2 > n) return DANHIP_JPEG_ETRUNCATED;
    const int len = be16(d + p);
    if (len < 2) return DANHIP_JPEG_ETABLE;
    if (p + len > n) return DANHIP_JPEG_ETRUNCATED;
    const uint8_t* s = d + p + 2;
    const int L = len - 2;
    p += len;
    if (m == 0xC2 && !(flags & DANHIP_JPEG_ALLOW_PROGRESSIVE)) return DANHIP_JPEG_EPROGRESSIVE;
    if (m >= 0xC9 && m <= 0xCF) return DANHIP_JPEG_EARITHMETIC;
    if (m == 0xC3 || (m >= 0xC5 && m <= 0xC8) || m == 0xDC || m == 0xDE || m == 0xDF) return DANHIP_JPEG_EUNSUPPORTED;
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      if (have_sof) return DANHIP_JPEG_EUNSUPPORTED;
      if (L < 6) return DANHIP_JPEG_ETABLE;
      if (s[0] != 8) return DANHIP_JPEG_EPRECISION;
      const int h = be16(s + 1), w = be16(s + 3), nc = s[5];
      if (h == 0) return DANHIP_JPEG_EUNSUPPORTED;               // height left to a DNL marker
      if (w == 0) return DANHIP_JPEG_ETABLE;
      if (h > DANHIP_JPEG_MAX_DIM || w > DANHIP_JPEG_MAX_DIM) return DANHIP_JPEG_ETOOLARGE;
      if (nc != 1 && nc != 3) return DANHIP_JPEG_ECOMPONENTS;
      if (L != 6 + 3 * nc) return DANHIP_JPEG_ETABLE;
      for (int c = 0; c < nc; ++c) {
        ids[c] = s[6 + 3 * c];
        hv[c] = s[7 + 3 * c];
        H->tq[c] = s[8 + 3 * c];
        if (H->tq[c] > 3) return DANHIP_JPEG_ETABLE;
      }
      if (nc == 3 && ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B') return DANHIP_JPEG_ERGBIDS;
      if (nc == 3 && (ids[0] == ids[1] || ids[0] == ids[2] || ids[1] == ids[2])) return DANHIP_JPEG_ETABLE;
      if (nc == 1) {
        if (hv[0] != 0x11) return DANHIP_JPEG_ESAMPLING;
        H->mode = DANHIP_JPEG_GREY;
      } else {
        if (hv[1] != 0x11 || hv[2] != 0x11) return DANHIP_JPEG_ESAMPLING;
        if (hv[0] == 0x11) H->mode = DANHIP_JPEG_444;
        else if (hv[0] == 0x21) H->mode = DANHIP_JPEG_422;
        else if (hv[0] == 0x22) H->mode = DANHIP_JPEG_420;
        else return DANHIP_JPEG_ESAMPLING;
      }
      H->width = w; H->height = h; H->ncomp = nc;
      H->progressive = m == 0xC2;
      have_sof = true;
    } else if (m == 0xDB) {
      int q = 0;
      while (q < L) {
        const int pq = s[q] >> 4, t = s[q] & 15;
        if (pq > 1 || t > 3 || q + 1 + 64 * (pq + 1) > L) return DANHIP_JPEG_ETABLE;
        for (int k = 0; k < 64; ++k) {
          const int v = pq ? be16(s + q + 1 + 2 * k) : s[q + 1 + k];
          if (v == 0) return DANHIP_JPEG_ETABLE;
          H->quant[t][kZigzag[k]] = (uint16_t)v;
        }
        H->quant_defined[t] = true;
        q += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xC4) {
      const int rc = parse_dht(s, L, H);
      if (rc) return rc;
    } else if (m == 0xDD) {
      if (L != 2) return DANHIP_JPEG_ETABLE;
      H->restart = be16(s);
    } else if (m == 0xEE) {
      if (L >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
    } else if (m == 0xDA) {
      if (!have_sof) return DANHIP_JPEG_ETABLE;
      if (H->progressive) {                                       // the scans themselves: prog_walk
        for (int c = 0; c < H->ncomp; ++c)
          if (!H->quant_defined[H->tq[c]]) return DANHIP_JPEG_ETABLE;
        if (adobe_transform >= 0 && adobe_transform != 1) return DANHIP_JPEG_EADOBE;
        H->scan = mark;
        return 0;
      }
      if (L < 1) return DANHIP_JPEG_ETABLE;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || L != 4 + 2 * ns) return DANHIP_JPEG_ETABLE;
      if (ns != H->ncomp) return DANHIP_JPEG_EMULTISCAN;
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != ids[c]) return DANHIP_JPEG_EUNSUPPORTED;        // components in another order than the frame's
        H->td[c] = s[2 + 2 * c] >> 4;
        H->ta[c] = s[2 + 2 * c] & 15;
        if (H->td[c] > 3 || H->ta[c] > 3 || !H->dc[H->td[c]].defined || !H->ac[H->ta[c]].defined) return DANHIP_JPEG_ETABLE;
        if (!H->quant_defined[H->tq[c]]) return DANHIP_JPEG_ETABLE;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return DANHIP_JPEG_ETABLE;
      if (adobe_transform >= 0 && adobe_transform != 1) return DANHIP_JPEG_EADOBE;
      H->scan = p;
      return 0;
    }
    // APPn, COM and the remaining markers with a length: skipped
  }
}

// MSB-first bit reader over the entropy-coded segment: FF00 unstuffed; at a marker or the end of the data it supplies zero bits and counts
// them, and the decoder refuses the image as soon as one of those has been consumed.
struct Bits {
  const uint8_t* d;
  int64_t n, p;
  uint64_t acc = 0;
  int cnt = 0;               // bits in acc (the low cnt bits)
  int64_t fake = 0;          // zero bits supplied beyond the data, still in acc or consumed
  Bits(const uint8_t* d_, int64_t n_, int64_t p_) : d(d_), n(n_), p(p_) {}
  void fill() {
    while (cnt <= 56) {
      uint32_t b = 0;
      if (p < n && d[p] != 0xFF) b = d[p++];
      else if (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0x00) { b = 0xFF; p += 2; }
      else fake += 8;                                           // a marker, or the end: stay there
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  inline uint32_t peek(int k) { return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1); }
  inline void skip(int k) { cnt -= k; }
  inline bool overrun() const { return cnt < fake; }
  // restart: drop the bits of the current byte, then expect FF Dn exactly here
  bool restart(int expect) {
    if (overrun()) return false;
    // fill() never reads past a marker, so what is left in acc belongs to this interval: an encoder pads its last byte, at most 7 bits
    // are legitimate; anything more is data that belongs to nobody
    const int real = cnt - (int)fake;
    if (real >= 8) return false;
    acc = 0; cnt = 0; fake = 0;
    while (p < n && d[p] == 0xFF && p + 1 < n && d[p + 1] == 0xFF) ++p;       // fill bytes before the marker
    if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + expect) return false;
    p += 2;
    return true;
  }
};

inline int decode_sym(Bits& b, const Huff& h) {
  const uint32_t look = h.look[b.peek(9)];
  if (look) { b.skip(look >> 8); return look & 255; }
  int l = 10;
  int32_t code = (int32_t)b.peek(10);
  while (code > h.maxcode[l]) { ++l; if (l > 16) return -1; code = (int32_t)b.peek(l); }
  b.skip(l);
  const int idx = code + h.valoff[l];
  return (idx < 0 || idx > 255) ? -1 : h.sym[idx];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

int decode_scan(const uint8_t* d, int64_t n, const Header& H, const DhJpegGeom& g, int16_t* coef) {
  Bits b(d, n, H.scan);
  const int32_t mcus_x = g.blocks_w[0] / g.hs, mcus_y = g.blocks_h[0] / g.vs;
  int64_t plane[3] = {0, 0, 0};
  for (int c = 1; c < g.ncomp; ++c) plane[c] = plane[c - 1] + (int64_t)g.blocks_w[c - 1] * g.blocks_h[c - 1];
  int pred[3] = {0, 0, 0};
  int64_t mcu = 0;
  int next_rst = 0;
  for (int32_t my = 0; my < mcus_y; ++my) {
    for (int32_t mx = 0; mx < mcus_x; ++mx, ++mcu) {
      if (H.restart && mcu && mcu % H.restart == 0) {
        if (!b.restart(next_rst)) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_ERESTART;
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < g.ncomp; ++c) {
        const int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.vs : 1;
        const Huff& hd = H.dc[H.td[c]];
        const Huff& ha = H.ac[H.ta[c]];
        const uint16_t* q = H.quant[H.tq[c]];
        for (int v = 0; v < cv; ++v) {
          for (int h = 0; h < ch; ++h) {
            int16_t* blk = coef + 64 * (plane[c] + (int64_t)(my * cv + v) * g.blocks_w[c] + (mx * ch + h));
            memset(blk, 0, 128);
            b.fill();
            int s = decode_sym(b, hd);
            if (s < 0 || s > 11) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
            if (s) { const int r = (int)b.peek(s); b.skip(s); pred[c] += extend(r, s); }
            if (pred[c] < -32768 || pred[c] > 32767) return DANHIP_JPEG_EHUFFMAN;
            blk[0] = (int16_t)pred[c];
            int64_t dq = (int64_t)pred[c] * q[0];
            int64_t energy = dq * dq;
            for (int k = 1; k < 64; ++k) {
              if (b.cnt < 32) b.fill();                                     // a symbol and its value take at most 16 + 15 bits
              const int rs = decode_sym(b, ha);
              if (rs < 0) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
              const int r = rs >> 4;
              s = rs & 15;
              if (s) {
                k += r;
                if (k > 63) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
                const int val = extend((int)b.peek(s), s);
                b.skip(s);
                const int nat = kZigzag[k];
                blk[(nat & 7) * 8 + (nat >> 3)] = (int16_t)val;            // column-major: col * 8 + row
                dq = (int64_t)val * q[nat];
                energy += dq * dq;
              } else if (r == 15) {
                k += 15;
              } else {
                break;
              }
            }
            if (b.overrun()) return DANHIP_JPEG_ETRUNCATED;
            if (energy > DANHIP_JPEG_MAX_BLOCK_ENERGY) return DANHIP_JPEG_ECOEFRANGE;
          }
        }
      }
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Progressive frames (include/danhip.h, "Progressive streams"): the scans of T.81 G.2 as jdphuff.c decodes them, into the same coefficient
// layout.  One walk over the markers behind the frame header does both jobs: without a coefficient buffer it validates the scan script
// (every SOS against G.1.1.1.1, completeness at EOI) and finds where each scan's data end - this is the "header" of a progressive stream,
// and a stream refused here owns no slot; with one it decodes every scan on the way.
struct ProgScan {
  int32_t ns, comp[3], td[3], ta, ss, se, ah, al;
};

enum { PROG_DC_FIRST, PROG_DC_REFINE, PROG_AC_FIRST, PROG_AC_REFINE };

// one SOS of a progressive frame against the tables and the progression state so far; on success bits[c][k] (the Al a coefficient has
// been sent down to, -1 = never) has advanced for every coefficient of the scan
int prog_scan_header(const uint8_t* s, int L, const Header& H, int8_t bits[3][64], ProgScan* S) {
  if (L < 1) return DANHIP_JPEG_ETABLE;
  const int ns = s[0];
  if (ns < 1 || ns > 4 || L != 4 + 2 * ns || ns > H.ncomp) return DANHIP_JPEG_ETABLE;
  S->ns = ns;
  int prev = -1;
  for (int i = 0; i < ns; ++i) {
    int c = -1;
    for (int k = 0; k < H.ncomp; ++k)
      if (H.ids[k] == s[1 + 2 * i]) c = k;
    if (c < 0) return DANHIP_JPEG_ETABLE;
    if (c <= prev) return DANHIP_JPEG_EUNSUPPORTED;             // components in another order than the frame's
    prev = c;
    S->comp[i] = c;
    S->td[i] = s[2 + 2 * i] >> 4;
    if (S->td[i] > 3 || (s[2 + 2 * i] & 15) > 3) return DANHIP_JPEG_ETABLE;
  }
  S->ta = s[2] & 15;
  S->ss = s[1 + 2 * ns]; S->se = s[2 + 2 * ns]; S->ah = s[3 + 2 * ns] >> 4; S->al = s[3 + 2 * ns] & 15;
  if (S->ss == 0) {
    if (S->se != 0) return DANHIP_JPEG_EPROGRESSION;
  } else if (ns != 1 || S->ss > S->se || S->se > 63) {
    return DANHIP_JPEG_EPROGRESSION;
  }
  if (S->al > 13 || (S->ah != 0 && S->al != S->ah - 1)) return DANHIP_JPEG_EPROGRESSION;
  for (int i = 0; i < ns; ++i) {
    const int8_t* b = bits[S->comp[i]];
    if (S->ss > 0 && b[0] < 0) return DANHIP_JPEG_EPROGRESSION;                 // a component's DC comes before its AC bands
    for (int k = S->ss; k <= S->se; ++k) {
      if (b[k] < 0 ? S->ah != 0 : (S->ah == 0 || S->ah != b[k])) return DANHIP_JPEG_EPROGRESSION;   // first scan: Ah = 0; later: Ah = previous Al, never twice
    }
  }
  if (S->ss == 0) {
    if (S->ah == 0)
      for (int i = 0; i < ns; ++i)
        if (!H.dc[S->td[i]].defined) return DANHIP_JPEG_ETABLE;
  } else if (!H.ac[S->ta].defined) {
    return DANHIP_JPEG_ETABLE;
  }
  for (int i = 0; i < ns; ++i)
    for (int k = S->ss; k <= S->se; ++k) bits[S->comp[i]][k] = (int8_t)S->al;
  return 0;
}

inline int prog_bit(Bits& b) {
  if (b.cnt < 1) b.fill();
  const int v = (int)b.peek(1);
  b.skip(1);
  return v;
}

// a correction bit for a coefficient that is already non-zero (G.1.2.3): the bit of this scan is added away from zero
inline void prog_correct(Bits& b, int16_t* c, int p1) {
  if (prog_bit(b) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c - p1);
}

// The entropy-coded data d[begin, end) of one scan.  An interleaved scan walks the frame's MCUs; a single-component scan walks that
// component's own ceil(comp_w / 8) x ceil(comp_h / 8) blocks (not the padded grid), and there the restart interval counts those blocks.
template <int KIND>
int prog_decode_scan(const uint8_t* d, int64_t begin, int64_t end, const Header& H, const DhJpegGeom& g, const ProgScan& S, int16_t* coef) {
  Bits b(d, end, begin);
  int64_t plane[3] = {0, 0, 0};
  for (int c = 1; c < g.ncomp; ++c) plane[c] = plane[c - 1] + (int64_t)g.blocks_w[c - 1] * g.blocks_h[c - 1];
  const bool inter = S.ns > 1;
  const int c0 = S.comp[0];
  const int32_t ux = inter ? g.blocks_w[0] / g.hs : (g.comp_w[c0] + 7) / 8, uy = inter ? g.blocks_h[0] / g.vs : (g.comp_h[c0] + 7) / 8;
  const int p1 = 1 << S.al;
  const Huff& ha = H.ac[S.ta];
  int pred[3] = {0, 0, 0};
  int32_t eobrun = 0;
  int64_t unit = 0;
  int next_rst = 0;
  for (int32_t y = 0; y < uy; ++y) {
    for (int32_t x = 0; x < ux; ++x, ++unit) {
      if (H.restart && unit && unit % H.restart == 0) {
        if (!b.restart(next_rst)) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_ERESTART;
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        eobrun = 0;
      }
      for (int i = 0; i < S.ns; ++i) {
        const int c = S.comp[i];
        const int ch = inter && c == 0 ? g.hs : 1, cv = inter && c == 0 ? g.vs : 1;
        for (int v = 0; v < cv; ++v) {
          for (int h = 0; h < ch; ++h) {
            int16_t* blk = coef + 64 * (plane[c] + (int64_t)(y * cv + v) * g.blocks_w[c] + (x * ch + h));
            if (KIND == PROG_DC_FIRST) {
              b.fill();
              const int s = decode_sym(b, H.dc[S.td[i]]);
              if (s < 0 || s > 11) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
              if (s) { const int r = (int)b.peek(s); b.skip(s); pred[i] += extend(r, s); }
              const int64_t val = (int64_t)pred[i] * p1;
              if (val < -32768 || val > 32767) return DANHIP_JPEG_EHUFFMAN;
              blk[0] = (int16_t)val;
            } else if (KIND == PROG_DC_REFINE) {
              if (prog_bit(b)) blk[0] = (int16_t)(blk[0] | p1);
            } else if (KIND == PROG_AC_FIRST) {
              if (eobrun > 0) {
                --eobrun;
              } else {
                for (int k = S.ss; k <= S.se; ++k) {
                  if (b.cnt < 32) b.fill();                                   // a symbol and its value take at most 16 + 15 bits
                  const int rs = decode_sym(b, ha);
                  if (rs < 0) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
                  const int r = rs >> 4, s = rs & 15;
                  if (s) {
                    k += r;
                    if (k > S.se) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
                    const int64_t val = (int64_t)extend((int)b.peek(s), s) * p1;
                    b.skip(s);
                    if (val < -32768 || val > 32767) return DANHIP_JPEG_EHUFFMAN;
                    blk[kZigColMajor[k]] = (int16_t)val;
                  } else if (r == 15) {
                    k += 15;
                  } else {                                                    // EOBr: this band of this block and of the next run - 1 is over
                    eobrun = 1 << r;
                    if (r) { eobrun += (int32_t)b.peek(r); b.skip(r); }
                    --eobrun;
                    break;
                  }
                }
              }
            } else {
              int k = S.ss;
              if (eobrun == 0) {
                for (; k <= S.se; ++k) {
                  if (b.cnt < 32) b.fill();
                  const int rs = decode_sym(b, ha);
                  if (rs < 0) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;
                  int r = rs >> 4, s = rs & 15;
                  if (s) {
                    if (s != 1) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;      // a new coefficient is +-1 at this precision
                    s = prog_bit(b) ? p1 : -p1;
                  } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) { eobrun += (int32_t)b.peek(r); b.skip(r); }
                    break;                                                    // the rest of the band: correction bits only, below
                  }
                  // over r coefficients that are still zero, and every non-zero one on the way takes a correction bit
                  do {
                    int16_t* cf = blk + kZigColMajor[k];
                    if (*cf != 0) prog_correct(b, cf, p1);
                    else if (--r < 0) break;
                    ++k;
                  } while (k <= S.se);
                  if (s) {
                    if (k > S.se) return b.overrun() ? DANHIP_JPEG_ETRUNCATED : DANHIP_JPEG_EHUFFMAN;    // the run leaves the band
                    blk[kZigColMajor[k]] = (int16_t)s;
                  }
                }
              }
              if (eobrun > 0) {
                for (; k <= S.se; ++k) {
                  int16_t* cf = blk + kZigColMajor[k];
                  if (*cf != 0) prog_correct(b, cf, p1);
                }
                --eobrun;
              }
            }
            if (b.overrun()) return DANHIP_JPEG_ETRUNCATED;
          }
        }
      }
    }
  }
  return 0;
}

// The DC value and every first AC value are range-checked where they are written; the +-p1 corrections of the refinement scans are not (on
// a hostile stream one may wrap in the int16 it is stored in), so AC magnitudes are bounded here, by the block energy of the finished
// coefficients as the baseline path checks it: a block that passes has every dequantised coefficient within +-1440.
int prog_post_check(const Header& H, const DhJpegGeom& g, const int16_t* coef) {
  const int16_t* blk = coef;
  for (int c = 0; c < g.ncomp; ++c) {
    const uint16_t* q = H.quant[H.tq[c]];
    const int64_t nb = (int64_t)g.blocks_w[c] * g.blocks_h[c];
    for (int64_t i = 0; i < nb; ++i, blk += 64) {
      int64_t energy = 0;
      for (int e = 0; e < 64; ++e) {
        const int64_t dq = (int64_t)blk[e] * q[(e & 7) * 8 + (e >> 3)];
        energy += dq * dq;
      }
      if (energy > DANHIP_JPEG_MAX_BLOCK_ENERGY) return DANHIP_JPEG_ECOEFRANGE;
    }
  }
  return 0;
}

// The markers of a progressive frame from its first SOS to EOI.  coef == nullptr: validation alone (what the header phase runs);
// else the slot is zeroed first - padding blocks that no single-component scan visits must read as zero - and every scan decoded.
int prog_walk(const uint8_t* d, int64_t n, const Header& H0, const DhJpegGeom& g, int16_t* coef) {
  Header H = H0;                                                 // DHT and DRI between scans change the copy
  int8_t bits[3][64];
  memset(bits, -1, sizeof(bits));
  if (coef) memset(coef, 0, (size_t)g.coef_count * 2);
  int64_t p = H0.scan;
  for (;;) {
    if (p >= n) return DANHIP_JPEG_ETRUNCATED;
    if (d[p] != 0xFF) return DANHIP_JPEG_ENOTJPEG;
    while (p < n && d[p] == 0xFF) ++p;                          // fill bytes
    if (p >= n) return DANHIP_JPEG_ETRUNCATED;
    const int m = d[p++];
    if (m == 0x00) return DANHIP_JPEG_ENOTJPEG;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD8) return DANHIP_JPEG_ENOTJPEG;
    if (m == 0xD9) break;
    if (p + 2 > n) return DANHIP_JPEG_ETRUNCATED;
    const int len = be16(d + p);
    if (len < 2) return DANHIP_JPEG_ETABLE;
    if (p + len > n) return DANHIP_JPEG_ETRUNCATED;
    const uint8_t* s = d + p + 2;
    const int L = len - 2;
    p += len;
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) return DANHIP_JPEG_EUNSUPPORTED;           // a second frame
    if (m >= 0xC9 && m <= 0xCF) return DANHIP_JPEG_EARITHMETIC;
    if (m == 0xC3 || (m >= 0xC5 && m <= 0xC8) || m == 0xDC || m == 0xDE || m == 0xDF) return DANHIP_JPEG_EUNSUPPORTED;
    if (m == 0xDB) return DANHIP_JPEG_ETABLE;                   // libjpeg latched the quantisation tables at a component's first scan
    if (m == 0xC4) {
      const int rc = parse_dht(s, L, &H);
      if (rc) return rc;
    } else if (m == 0xDD) {
      if (L != 2) return DANHIP_JPEG_ETABLE;
      H.restart = be16(s);
    } else if (m == 0xDA) {
      ProgScan S;
      int rc = prog_scan_header(s, L, H, bits, &S);
      if (rc) return rc;
      int64_t q = p;                                             // the data end at the first marker that is no RSTn
      for (;;) {
        const void* f = q < n ? memchr(d + q, 0xFF, (size_t)(n - q)) : nullptr;
        if (!f) return DANHIP_JPEG_ETRUNCATED;                  // no EOI
        q = (const uint8_t*)f - d;
        if (q + 1 >= n) return DANHIP_JPEG_ETRUNCATED;
        const int x = d[q + 1];
        if (x == 0x00 || (x >= 0xD0 && x <= 0xD7)) { q += 2; continue; }
        if (x == 0xFF) { q += 1; continue; }
        break;
      }
      if (coef) {
        if (S.ss == 0) rc = S.ah == 0 ? prog_decode_scan<PROG_DC_FIRST>(d, p, q, H, g, S, coef) : prog_decode_scan<PROG_DC_REFINE>(d, p, q, H, g, S, coef);
        else rc = S.ah == 0 ? prog_decode_scan<PROG_AC_FIRST>(d, p, q, H, g, S, coef) : prog_decode_scan<PROG_AC_REFINE>(d, p, q, H, g, S, coef);
        if (rc) return rc;
      }
      p = q;
    }
    // APPn, COM and the remaining markers with a length: skipped
  }
  for (int c = 0; c < H.ncomp; ++c)                             // complete: every coefficient of every component down to Al = 0
    for (int k = 0; k < 64; ++k)
      if (bits[c][k] != 0) return DANHIP_JPEG_EPROGRESSION;
  return coef ? prog_post_check(H, g, coef) : 0;
}

// header and geometry of one stream; for a progressive frame the header is the whole scan script
int accept_stream(const uint8_t* d, int64_t n, uint32_t flags, Header* H, DhJpegGeom* g) {
  int rc = parse_header(d, n, H, flags);
  if (rc == 0 && !dh_jpeg_geometry(H->width, H->height, H->mode, g)) rc = DANHIP_JPEG_ETOOLARGE;
  if (rc == 0 && H->progressive) rc = prog_walk(d, n, *H, *g, nullptr);
  return rc;
}

bool bad_flags(const char* who, uint32_t flags) {
  if (!(flags & ~(uint32_t)DANHIP_JPEG_ALLOW_PROGRESSIVE)) return false;
  danhip_set_error("%s: unknown bits in flags 0x%x (DANHIP_JPEG_ALLOW_PROGRESSIVE is the one flag)", who, flags);
  return true;
}

void clear_desc(danhip_jpeg_desc* d, int status) {
  memset(d, 0, sizeof(*d));
  d->status = status;
}

// geometry, quantisation tables and the device offsets (planes, output) of one image that goes to the device
void fill_device_fields(danhip_jpeg_desc* d, const Header& H, const DhJpegGeom& g, int64_t* ws, int64_t* out) {
  d->width = H.width; d->height = H.height; d->ncomp = H.ncomp; d->mode = H.mode;
  for (int c = 0; c < 3; ++c) {
    d->blocks_w[c] = g.blocks_w[c]; d->blocks_h[c] = g.blocks_h[c]; d->comp_w[c] = g.comp_w[c]; d->comp_h[c] = g.comp_h[c];
    d->quant_index[c] = c < g.ncomp ? H.tq[c] : 0;
    d->plane_offset[c] = 0;
    if (c < g.ncomp) { d->plane_offset[c] = *ws; *ws += dh_jpeg_align(g.plane_bytes[c], 256); }
  }
  d->idct_groups = g.idct_groups; d->rgb_groups = g.rgb_groups;
  d->out_offset = *out;
  *out += dh_jpeg_align(g.out_bytes, 256);
  for (int t = 0; t < 4; ++t)
    for (int k = 0; k < 64; ++k) d->quant[t][k] = H.quant_defined[t] ? H.quant[t][k] : 1;
  d->reserved[0] = H.progressive ? 1 : 0;                        // informational: the launcher does not look at it
}

}  // namespace

extern "C" int danhip_jpeg_inspect_ex(const uint8_t* data, int64_t n, uint32_t flags, danhip_jpeg_info* info) {
  if (!info) { danhip_set_error("jpeg_inspect: info is NULL"); return DANHIP_EINVAL; }
  memset(info, 0, sizeof(*info));
  if (bad_flags("jpeg_inspect_ex", flags)) return DANHIP_EINVAL;
  Header* H = new Header();
  DhJpegGeom g;
  const int rc = accept_stream(data, n, flags, H, &g);
  info->reason = rc;
  if (rc == 0) {
    info->width = H->width; info->height = H->height; info->ncomp = H->ncomp; info->mode = H->mode;
    info->reserved = H->progressive ? 1 : 0;
    info->coef_count = g.coef_count;
  }
  delete H;
  return rc;
}

extern "C" int danhip_jpeg_inspect(const uint8_t* data, int64_t n, danhip_jpeg_info* info) { return danhip_jpeg_inspect_ex(data, n, 0, info); }

extern "C" int danhip_jpeg_entropy_decode_batch_ex(const uint8_t* const* datas, const int64_t* sizes, int32_t B, int32_t threads, uint32_t flags,
                                                   int16_t* coef_out, int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out) {
  if (!datas || !sizes || B < 1 || B > 65535 || !descs_out || !status_out || coef_capacity < 0 || (coef_capacity > 0 && !coef_out)) {
    danhip_set_error("jpeg_entropy_decode_batch: bad arguments (1 <= B <= 65535, no NULL table)");
    return DANHIP_EINVAL;
  }
  if (bad_flags("jpeg_entropy_decode_batch_ex", flags)) return DANHIP_EINVAL;
  std::vector<Header> hdr((size_t)B);
  std::vector<DhJpegGeom> geom((size_t)B);
  int64_t next = 0;
  for (int32_t i = 0; i < B; ++i) {                              // headers in order: the coefficient slots
    int rc = accept_stream(datas[i], sizes[i], flags, &hdr[i], &geom[i]);
    if (rc == 0 && geom[i].coef_count > coef_capacity - next) rc = DANHIP_JPEG_ECAPACITY;
    clear_desc(&descs_out[i], rc);
    status_out[i] = rc;
    if (rc) continue;
    descs_out[i].coef_offset = next;
    descs_out[i].coef_count = geom[i].coef_count;
    next += geom[i].coef_count;
  }
  int T = threads < 1 ? 1 : threads;
  if (T > DANHIP_JPEG_MAX_THREADS) T = DANHIP_JPEG_MAX_THREADS;
  if (T > B) T = B;
  std::atomic<int32_t> cursor(0);
  auto work = [&]() {
    for (;;) {
      const int32_t i = cursor.fetch_add(1);
      if (i >= B) return;
      if (status_out[i]) continue;
      int16_t* slot = coef_out + descs_out[i].coef_offset;
      status_out[i] = hdr[i].progressive ? prog_walk(datas[i], sizes[i], hdr[i], geom[i], slot) : decode_scan(datas[i], sizes[i], hdr[i], geom[i], slot);
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
  int64_t ws = 0, out = 0;
  for (int32_t i = 0; i < B; ++i) {                              // device offsets: to the decoded images alone
    danhip_jpeg_desc* d = &descs_out[i];
    if (status_out[i]) { clear_desc(d, status_out[i]); continue; }
    fill_device_fields(d, hdr[i], geom[i], &ws, &out);
  }
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_entropy_decode_batch(const uint8_t* const* datas, const int64_t* sizes, int32_t B, int32_t threads, int16_t* coef_out,
                                                int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out) {
  return danhip_jpeg_entropy_decode_batch_ex(datas, sizes, B, threads, 0, coef_out, coef_capacity, descs_out, status_out);
}

namespace {
// total bytes of the workspace (which = 0) or of the output (which = 1) that the decodable descriptors need; -1: one is malformed
int64_t jpeg_extent(const danhip_jpeg_desc* descs, int32_t B, int which) {
  if (!descs || B < 1) return -1;
  int64_t end = 0;
  for (int32_t i = 0; i < B; ++i) {
    const danhip_jpeg_desc* d = &descs[i];
    if (d->status) continue;
    DhJpegGeom g;
    if (!dh_jpeg_geometry(d->width, d->height, d->mode, &g)) return -1;
    if (which == 0) {
      for (int c = 0; c < g.ncomp; ++c) {
        if (d->plane_offset[c] < 0 || d->plane_offset[c] > ((int64_t)1 << 46)) return -1;
        const int64_t e = d->plane_offset[c] + dh_jpeg_align(g.plane_bytes[c], 256);
        if (e > end) end = e;
      }
    } else {
      if (d->out_offset < 0 || d->out_offset > ((int64_t)1 << 46)) return -1;
      const int64_t e = d->out_offset + dh_jpeg_align(g.out_bytes, 256);
      if (e > end) end = e;
    }
  }
  return end;
}
}  // namespace

extern "C" size_t danhip_jpeg_workspace_bytes(const danhip_jpeg_desc* descs, int32_t B) {
  const int64_t e = jpeg_extent(descs, B, 0);
  return e < 0 ? 0 : (size_t)e;
}

extern "C" int64_t danhip_jpeg_output_bytes(const danhip_jpeg_desc* descs, int32_t B) {
  const int64_t e = jpeg_extent(descs, B, 1);
  return e < 0 ? 0 : e;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Host half of the device Huffman stage (include/danhip.h, "Huffman decoding on the device"): segments, work items, workgroups, tables and
// the stuffed scan bytes packed into one staging buffer; the check of such a buffer that the launcher runs before a launch; and the same
// phases as the kernels on the host, through the routines of jpeg_huffman.h with checked indexing.
#include "jpeg_huffman.h"

namespace {

inline int64_t a16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct ScanPlan {                  // what the prepare pass collects before it packs
  std::vector<DhScanImage> images;
  std::vector<DhScanSeg> segs;
  std::vector<DhScanItem> items;
  std::vector<DhScanGroup> groups;
  std::vector<DhDcChunk> chunks;
  std::vector<DhHuffTab> tabs;
  int64_t scan_bytes = 0;
};

void pack_tab(const Huff& h, DhHuffTab* t) {
  memcpy(t->look, h.look, sizeof(t->look));
  memcpy(t->maxcode, h.maxcode, sizeof(t->maxcode));
  t->valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) t->valoff[l] = h.valoff[l];
  t->valoff[17] = 0;
  t->maxcode[0] = -1;
  memcpy(t->sym, h.sym, sizeof(t->sym));
}

// One pass over the scan that looks for FF alone.  0: the segments are in plan; 1: an RSTn is missing or out of sequence (the host decoder
// refuses such a stream; with which code depends on the bits in front of the place, so the caller asks it).
int scan_segments(const uint8_t* d, int64_t n, const Header& H, const DhJpegGeom& g, int32_t image, ScanPlan* plan, DhScanImage* im) {
  const int64_t mcus = (int64_t)(g.blocks_w[0] / g.hs) * (g.blocks_h[0] / g.vs);
  const int64_t nseg = H.restart ? (mcus + H.restart - 1) / H.restart : 1;
  if (nseg - 1 > (n - H.scan) / 2) return 1;                    // every marker takes two bytes
  const size_t seg0 = plan->segs.size();
  int64_t start = H.scan;
  for (int64_t s = 0; s < nseg; ++s) {
    int64_t q = start;
    for (;;) {                                                   // the first FF that no 00 follows, or the end
      const void* f = q < n ? memchr(d + q, 0xFF, (size_t)(n - q)) : nullptr;
      if (!f) { q = n; break; }
      q = (const uint8_t*)f - d;
      if (q + 1 < n && d[q + 1] == 0x00) { q += 2; continue; }
      break;
    }
    const int64_t data_end = q;
    while (q + 1 < n && d[q] == 0xFF && d[q + 1] == 0xFF) ++q;   // fill bytes before a marker
    const bool final = s == nseg - 1;
    if (!final && (q + 1 >= n || d[q] != 0xFF || d[q + 1] != 0xD0 + (int)(s & 7))) {
      plan->segs.resize(seg0);
      return 1;
    }
    DhScanSeg sg;
    sg.offset = (int32_t)(start - H.scan);
    sg.len = (int32_t)(q - start);
    sg.data_len = (int32_t)(data_end - start);
    sg.first_mcu = (int32_t)(s * (H.restart ? H.restart : 0));
    sg.mcu_count = (int32_t)(final ? mcus - sg.first_mcu : H.restart);
    sg.first_item = 0; sg.nitems = 0;
    sg.final = final ? 1 : 0;
    plan->segs.push_back(sg);
    start = q + 2;
  }
  const DhScanSeg& last = plan->segs.back();
  im->scan_len = (int64_t)last.offset + last.len;
  im->first_seg = (int32_t)seg0;
  im->nseg = (int32_t)nseg;
  (void)image;
  return 0;
}

// items, workgroups and DC chunks of one image whose segments are in plan
void plan_work(int32_t image, ScanPlan* plan, DhScanImage* im) {
  im->first_item = (int32_t)plan->items.size();
  im->first_chunk = (int32_t)plan->chunks.size();
  for (int32_t s = im->first_seg; s < im->first_seg + im->nseg; ++s) {
    DhScanSeg& sg = plan->segs[(size_t)s];
    sg.first_item = (int32_t)plan->items.size();
    sg.nitems = sg.data_len > 0 ? (sg.data_len + DH_HUFF_S - 1) / DH_HUFF_S : 1;
    for (int32_t j = 0; j < sg.nitems; ++j) plan->items.push_back(DhScanItem{s, j});
    const int32_t chain = (int32_t)plan->chunks.size();
    for (int32_t m = 0; m < sg.mcu_count; m += DH_HUFF_DC_CHUNK) {
      const int32_t left = sg.mcu_count - m;
      plan->chunks.push_back(DhDcChunk{image, s, m, left < DH_HUFF_DC_CHUNK ? left : DH_HUFF_DC_CHUNK, chain, 0});
    }
  }
  im->nitems = (int32_t)plan->items.size() - im->first_item;
  im->nchunks = (int32_t)plan->chunks.size() - im->first_chunk;
  im->first_group = (int32_t)plan->groups.size();
  int32_t seg_group = im->first_group;                           // the group that holds the current segment's first item
  for (int32_t it = im->first_item; it < im->first_item + im->nitems;) {
    DhScanGroup gr;
    memset(&gr, 0, sizeof(gr));
    gr.image = image;
    gr.first_item = it;
    const int32_t g_index = (int32_t)plan->groups.size();
    const DhScanItem& first = plan->items[(size_t)it];
    gr.win_base = (im->scan_offset + plan->segs[(size_t)first.seg].offset + (int64_t)first.sub * DH_HUFF_S) & ~(int64_t)15;
    gr.carry_from = first.sub == 0 ? g_index : seg_group;
    while (it < im->first_item + im->nitems && gr.nitems < DH_HUFF_G) {
      const DhScanItem& x = plan->items[(size_t)it];
      const DhScanSeg& sg = plan->segs[(size_t)x.seg];
      const int64_t a = im->scan_offset + sg.offset + (int64_t)x.sub * DH_HUFF_S;
      int64_t e = a + DH_HUFF_S;
      if (e > im->scan_offset + sg.offset + sg.data_len) e = im->scan_offset + sg.offset + sg.data_len;
      if (e < a) e = a;
      if (gr.nitems && e - gr.win_base > (int64_t)DH_HUFF_G * DH_HUFF_S + 16) break;
      if (x.sub == 0) seg_group = g_index;
      ++gr.nitems;
      ++it;
    }
    plan->groups.push_back(gr);
  }
  im->ngroups = (int32_t)plan->groups.size() - im->first_group;
}

struct ScanView {                  // a staging buffer taken apart
  const DhScanHeader* h;
  const DhScanImage* images;
  const DhScanSeg* segs;
  const DhScanItem* items;
  const DhScanGroup* groups;
  const DhDcChunk* chunks;
  const DhHuffTab* tabs;
  const uint8_t* scan;
};

DhBlockGeom block_geom(const DhScanImage& im) {
  DhBlockGeom g;
  g.bpm = im.bpm; g.nl = im.hs * im.vs; g.hs = im.hs; g.mcus_x = im.mcus_x;
  g.bw0 = im.blocks_w[0]; g.bw1 = im.blocks_w[1]; g.bw2 = im.blocks_w[2];
  g.plane0 = im.plane[0]; g.plane1 = im.plane[1]; g.plane2 = im.plane[2];
  g.total_blocks = im.total_blocks;
  return g;
}

}  // namespace

// Every offset, count and index of a staging buffer against the buffer's size, the descriptors and the coefficient buffer.  NULL = fine.
// Shared with the launcher (jpeg_huffman_exact.hip), which runs it on the host copy before a kernel sees the device copy.
const char* dh_jpeg_scan_check(const void* staging, size_t staging_bytes, int32_t B, const danhip_jpeg_desc* descs, int64_t coef_count) {
  if (!staging || ((uintptr_t)staging & 15) || staging_bytes < sizeof(DhScanHeader)) return "no staging buffer, or one not 16-byte aligned";
  const DhScanHeader* h = (const DhScanHeader*)staging;
  if (h->magic != DH_HUFF_MAGIC || h->B != B || B < 1 || B > 65535) return "not a prepared staging buffer of this batch";
  if (h->nseg < 0 || h->nitems < 0 || h->ngroups < 0 || h->nchunks < 0 || h->ntabs < 0 || h->scan_bytes < 0) return "negative count";
  if (h->used_bytes < 0 || (uint64_t)h->used_bytes > staging_bytes) return "the tables leave the staging buffer";
  struct { int64_t off; int64_t bytes; } part[7] = {
      {h->off_images, (int64_t)B * (int64_t)sizeof(DhScanImage)},      {h->off_segs, (int64_t)h->nseg * (int64_t)sizeof(DhScanSeg)},
      {h->off_items, (int64_t)h->nitems * (int64_t)sizeof(DhScanItem)}, {h->off_groups, (int64_t)h->ngroups * (int64_t)sizeof(DhScanGroup)},
      {h->off_chunks, (int64_t)h->nchunks * (int64_t)sizeof(DhDcChunk)}, {h->off_tabs, (int64_t)h->ntabs * (int64_t)sizeof(DhHuffTab)},
      {h->off_scan, h->scan_bytes}};
  int64_t at = (int64_t)sizeof(DhScanHeader);
  for (int i = 0; i < 7; ++i) {
    if (part[i].off < at || (part[i].off & 15) || part[i].bytes > h->used_bytes - part[i].off) return "a table leaves the staging buffer";
    at = part[i].off + part[i].bytes;
  }
  const uint8_t* base = (const uint8_t*)staging;
  const DhScanImage* images = (const DhScanImage*)(base + h->off_images);
  const DhScanSeg* segs = (const DhScanSeg*)(base + h->off_segs);
  const DhScanItem* items = (const DhScanItem*)(base + h->off_items);
  const DhScanGroup* groups = (const DhScanGroup*)(base + h->off_groups);
  const DhDcChunk* chunks = (const DhDcChunk*)(base + h->off_chunks);
  const DhHuffTab* tabs = (const DhHuffTab*)(base + h->off_tabs);
  for (int32_t t = 0; t < h->ntabs; ++t)
    for (int i = 0; i < 512; ++i) {
      const int len = tabs[t].look[i] >> 8;
      if (tabs[t].look[i] && (len < 1 || len > 9)) return "a code length of a lookup table outside [1, 9]";
    }
  int32_t seg_at = 0, item_at = 0, group_at = 0, chunk_at = 0, tab_at = 0;
  for (int32_t i = 0; i < B; ++i) {
    const DhScanImage& im = images[i];
    if (!im.prepared) {
      if (im.nseg || im.nitems || im.ngroups || im.nchunks) return "an image that is not prepared asks for work";
      continue;
    }
    if (!descs || descs[i].status) return "a prepared image without a decodable descriptor";
    const danhip_jpeg_desc& d = descs[i];
    DhJpegGeom g;
    if (!dh_jpeg_geometry(d.width, d.height, d.mode, &g)) return "size or mode outside the accepted range";
    const int32_t mcus_x = g.blocks_w[0] / g.hs, mcus = mcus_x * (g.blocks_h[0] / g.vs);
    if (im.ncomp != g.ncomp || im.hs != g.hs || im.vs != g.vs || im.bpm != g.hs * g.vs + (g.ncomp - 1) || im.mcus_x != mcus_x || im.mcus != mcus)
      return "MCU geometry does not fit the size";
    int64_t plane = 0;
    for (int c = 0; c < 3; ++c) {
      if (im.blocks_w[c] != g.blocks_w[c] || d.blocks_w[c] != g.blocks_w[c] || d.blocks_h[c] != g.blocks_h[c]) return "block grid does not fit the size";
      if (im.plane[c] != (c < g.ncomp ? plane : 0)) return "component planes do not fit the size";
      plane += (int64_t)g.blocks_w[c] * g.blocks_h[c];
      if (d.quant_index[c] < 0 || d.quant_index[c] > 3) return "quantisation table index outside [0, 3]";
    }
    if (im.total_blocks != g.blocks || d.coef_count != g.coef_count || im.coef_offset != d.coef_offset || d.coef_offset < 0 || d.coef_offset % 64 ||
        d.coef_offset > coef_count || g.coef_count > coef_count - d.coef_offset)
      return "coefficients leave the buffer";
    if (im.tab_first != tab_at || im.tab_first + 2 * g.ncomp > h->ntabs) return "Huffman tables leave their array";
    tab_at += 2 * g.ncomp;
    if (im.scan_offset < 0 || (im.scan_offset & 15) || im.scan_len < 0 || im.scan_len >= DH_HUFF_MAX_SCAN || im.scan_offset > h->scan_bytes ||
        im.scan_len > h->scan_bytes - im.scan_offset)
      return "scan bytes leave the staging buffer";
    if (im.first_seg != seg_at || im.nseg < 1 || im.nseg > h->nseg - seg_at || im.first_item != item_at || im.first_group != group_at ||
        im.first_chunk != chunk_at)
      return "tables of the images are not consecutive";
    int32_t mcu_at = 0;
    int64_t byte_at = 0;
    for (int32_t s = seg_at; s < seg_at + im.nseg; ++s) {
      const DhScanSeg& sg = segs[s];
      if (sg.offset != byte_at || sg.len < 0 || sg.data_len < 0 || sg.data_len > sg.len || sg.len > im.scan_len - sg.offset) return "a segment leaves its scan";
      byte_at = (int64_t)sg.offset + sg.len + 2;
      if (sg.first_mcu != mcu_at || sg.mcu_count < 1 || sg.mcu_count > mcus - mcu_at || sg.final != (s == seg_at + im.nseg - 1)) return "segments do not tile the MCUs";
      mcu_at += sg.mcu_count;
      const int32_t want = sg.data_len > 0 ? (sg.data_len + DH_HUFF_S - 1) / DH_HUFF_S : 1;
      if (sg.first_item != item_at || sg.nitems != want || want > h->nitems - item_at) return "work items do not tile a segment";
      for (int32_t j = 0; j < want; ++j)
        if (items[item_at + j].seg != s || items[item_at + j].sub != j) return "a work item names another subsequence";
      item_at += want;
      int32_t m = 0;
      const int32_t chain = chunk_at;
      while (m < sg.mcu_count) {
        if (chunk_at >= h->nchunks) return "DC chunks leave their array";
        const DhDcChunk& ck = chunks[chunk_at];
        if (ck.image != i || ck.seg != s || ck.mcu0 != m || ck.n < 1 || ck.n > DH_HUFF_DC_CHUNK || ck.n > sg.mcu_count - m || ck.chain_from != chain)
          return "DC chunks do not tile a segment";
        m += ck.n;
        ++chunk_at;
      }
    }
    if (mcu_at != mcus) return "segments do not tile the MCUs";
    if (im.nitems != item_at - im.first_item || im.nchunks != chunk_at - im.first_chunk) return "counts of an image do not fit its tables";
    seg_at += im.nseg;
    int32_t it = im.first_item;
    while (it < item_at) {
      if (group_at >= h->ngroups) return "workgroups leave their array";
      const DhScanGroup& gr = groups[group_at];
      if (gr.image != i || gr.first_item != it || gr.nitems < 1 || gr.nitems > DH_HUFF_G || gr.nitems > item_at - it || gr.win_base < 0 || (gr.win_base & 15))
        return "workgroups do not tile the work items";
      for (int32_t j = 0; j < gr.nitems; ++j) {
        const DhScanSeg& sg = segs[items[it + j].seg];
        const int64_t a = im.scan_offset + sg.offset + (int64_t)items[it + j].sub * DH_HUFF_S;
        int64_t e = a + DH_HUFF_S;
        if (e > im.scan_offset + sg.offset + sg.data_len) e = im.scan_offset + sg.offset + sg.data_len;
        if (a < gr.win_base || (j > 0 && e - gr.win_base > (int64_t)DH_HUFF_G * DH_HUFF_S + 16) || (j == 0 && a - gr.win_base > 15))
          return "a work item leaves its group's window";
      }
      const int32_t head = segs[items[it].seg].first_item;       // the carry chain starts at the group that holds the segment's first item
      if (gr.carry_from < im.first_group || gr.carry_from > group_at || groups[gr.carry_from].first_item > head ||
          head >= groups[gr.carry_from].first_item + groups[gr.carry_from].nitems)
        return "a workgroup's carry chain starts at the wrong group";
      it += gr.nitems;
      ++group_at;
    }
    if (im.ngroups != group_at - im.first_group) return "counts of an image do not fit its tables";
  }
  if (seg_at != h->nseg || item_at != h->nitems || group_at != h->ngroups || chunk_at != h->nchunks || tab_at != h->ntabs) return "tables hold entries no image owns";
  return nullptr;
}

extern "C" size_t danhip_jpeg_scan_staging_bytes(const uint8_t* const* datas, const int64_t* sizes, int32_t B) {
  if (!datas || !sizes || B < 1 || B > 65535) return 0;
  int64_t total = a16(sizeof(DhScanHeader)) + a16((int64_t)B * (int64_t)sizeof(DhScanImage)) + 7 * 16 + 64;
  Header* H = new Header();
  for (int32_t i = 0; i < B; ++i) {
    DhJpegGeom g;
    if (parse_header(datas[i], sizes[i], H) != 0 || !dh_jpeg_geometry(H->width, H->height, H->mode, &g)) continue;
    const int64_t scanb = sizes[i] - H->scan;
    if (scanb >= DH_HUFF_MAX_SCAN) continue;
    const int64_t mcus = (int64_t)(g.blocks_w[0] / g.hs) * (g.blocks_h[0] / g.vs);
    int64_t nseg = H->restart ? (mcus + H->restart - 1) / H->restart : 1;
    if (nseg > scanb / 2 + 1) nseg = scanb / 2 + 1;
    const int64_t nitems = nseg + scanb / DH_HUFF_S + 1;
    const int64_t nchunks = nseg + mcus / DH_HUFF_DC_CHUNK + 1;
    total += nseg * (int64_t)sizeof(DhScanSeg) + nitems * (int64_t)(sizeof(DhScanItem) + sizeof(DhScanGroup)) + nchunks * (int64_t)sizeof(DhDcChunk) +
             6 * (int64_t)sizeof(DhHuffTab) + a16(scanb);
  }
  delete H;
  return (size_t)total;
}

extern "C" int danhip_jpeg_scan_prepare_batch_ex(const uint8_t* const* datas, const int64_t* sizes, int32_t B, uint32_t flags, void* staging,
                                                 size_t staging_bytes, int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out) {
  if (!datas || !sizes || B < 1 || B > 65535 || !descs_out || !status_out || coef_capacity < 0 || !staging || ((uintptr_t)staging & 15) ||
      staging_bytes < sizeof(DhScanHeader)) {
    danhip_set_error("jpeg_scan_prepare_batch: bad arguments (1 <= B <= 65535, no NULL table, staging 16-byte aligned)");
    return DANHIP_EINVAL;
  }
  if (bad_flags("jpeg_scan_prepare_batch_ex", flags)) return DANHIP_EINVAL;
  std::vector<Header> hdr((size_t)B);
  std::vector<DhJpegGeom> geom((size_t)B);
  ScanPlan plan;
  plan.images.resize((size_t)B);
  int64_t next = 0, ws = 0, out = 0;
  std::vector<int16_t> scratch;
  for (int32_t i = 0; i < B; ++i) {
    DhScanImage& im = plan.images[(size_t)i];
    memset(&im, 0, sizeof(im));
    int rc = accept_stream(datas[i], sizes[i], flags, &hdr[i], &geom[i]);
    if (rc == 0 && geom[i].coef_count > coef_capacity - next) rc = DANHIP_JPEG_ECAPACITY;
    clear_desc(&descs_out[i], rc);
    status_out[i] = rc;
    if (rc) continue;
    const Header& H = hdr[i];
    const DhJpegGeom& g = geom[i];
    const int64_t coef_offset = next;                            // the slot belongs to the image whatever happens to it below
    next += g.coef_count;
    if (H.progressive || sizes[i] - H.scan >= DH_HUFF_MAX_SCAN) {   // the device stage decodes one interleaved baseline scan
      rc = DANHIP_JPEG_HOSTONLY;
    } else {
      im.scan_offset = a16(plan.scan_bytes);
      if (scan_segments(datas[i], sizes[i], H, g, i, &plan, &im)) {
        scratch.resize((size_t)g.coef_count);                    // refused: the host decoder names the reason
        rc = decode_scan(datas[i], sizes[i], H, g, scratch.data());
        if (rc == 0) rc = DANHIP_JPEG_ERESTART;                   // (it cannot: it needs the marker that is not there)
      }
    }
    if (rc) {
      clear_desc(&descs_out[i], rc);
      status_out[i] = rc;
      memset(&im, 0, sizeof(im));
      continue;
    }
    im.prepared = 1;
    im.ncomp = g.ncomp; im.hs = g.hs; im.vs = g.vs; im.bpm = g.hs * g.vs + (g.ncomp - 1);
    im.mcus_x = g.blocks_w[0] / g.hs; im.mcus = im.mcus_x * (g.blocks_h[0] / g.vs);
    im.restart = H.restart;
    int64_t plane = 0;
    for (int c = 0; c < 3; ++c) {
      im.blocks_w[c] = g.blocks_w[c];
      im.plane[c] = c < g.ncomp ? plane : 0;
      plane += (int64_t)g.blocks_w[c] * g.blocks_h[c];
    }
    im.total_blocks = g.blocks;
    im.coef_offset = coef_offset;
    im.tab_first = (int32_t)plan.tabs.size();
    for (int c = 0; c < g.ncomp; ++c) {
      plan.tabs.resize(plan.tabs.size() + 2);
      pack_tab(H.dc[H.td[c]], &plan.tabs[plan.tabs.size() - 2]);
      pack_tab(H.ac[H.ta[c]], &plan.tabs[plan.tabs.size() - 1]);
    }
    plan_work(i, &plan, &im);
    plan.scan_bytes = im.scan_offset + im.scan_len;
    danhip_jpeg_desc* d = &descs_out[i];
    d->coef_offset = coef_offset;
    d->coef_count = g.coef_count;
    fill_device_fields(d, H, g, &ws, &out);
  }
  DhScanHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = DH_HUFF_MAGIC; h.B = B;
  h.nseg = (int32_t)plan.segs.size(); h.nitems = (int32_t)plan.items.size(); h.ngroups = (int32_t)plan.groups.size();
  h.nchunks = (int32_t)plan.chunks.size(); h.ntabs = (int32_t)plan.tabs.size();
  h.coef_capacity = coef_capacity;
  int64_t at = a16(sizeof(DhScanHeader));
  h.off_images = at; at = a16(at + (int64_t)B * (int64_t)sizeof(DhScanImage));
  h.off_segs = at; at = a16(at + (int64_t)plan.segs.size() * (int64_t)sizeof(DhScanSeg));
  h.off_items = at; at = a16(at + (int64_t)plan.items.size() * (int64_t)sizeof(DhScanItem));
  h.off_groups = at; at = a16(at + (int64_t)plan.groups.size() * (int64_t)sizeof(DhScanGroup));
  h.off_chunks = at; at = a16(at + (int64_t)plan.chunks.size() * (int64_t)sizeof(DhDcChunk));
  h.off_tabs = at; at = a16(at + (int64_t)plan.tabs.size() * (int64_t)sizeof(DhHuffTab));
  h.off_scan = at;
  h.scan_bytes = a16(plan.scan_bytes);
  h.used_bytes = at + h.scan_bytes;
  if ((uint64_t)h.used_bytes > staging_bytes) {
    danhip_set_error("jpeg_scan_prepare_batch: the staging buffer holds %zu bytes, the batch needs %lld (danhip_jpeg_scan_staging_bytes)", staging_bytes,
                     (long long)h.used_bytes);
    return DANHIP_EWORKSPACE;
  }
  uint8_t* base = (uint8_t*)staging;
  memset(base, 0, (size_t)h.off_scan);
  memcpy(base, &h, sizeof(h));
  memcpy(base + h.off_images, plan.images.data(), plan.images.size() * sizeof(DhScanImage));
  if (!plan.segs.empty()) memcpy(base + h.off_segs, plan.segs.data(), plan.segs.size() * sizeof(DhScanSeg));
  if (!plan.items.empty()) memcpy(base + h.off_items, plan.items.data(), plan.items.size() * sizeof(DhScanItem));
  if (!plan.groups.empty()) memcpy(base + h.off_groups, plan.groups.data(), plan.groups.size() * sizeof(DhScanGroup));
  if (!plan.chunks.empty()) memcpy(base + h.off_chunks, plan.chunks.data(), plan.chunks.size() * sizeof(DhDcChunk));
  if (!plan.tabs.empty()) memcpy(base + h.off_tabs, plan.tabs.data(), plan.tabs.size() * sizeof(DhHuffTab));
  for (int32_t i = 0; i < B; ++i) {                              // the scan bytes, left stuffed; the gaps up to the next 16-byte boundary are zero
    const DhScanImage& im = plan.images[(size_t)i];
    if (!im.prepared) continue;
    uint8_t* dst = base + h.off_scan + im.scan_offset;
    memcpy(dst, datas[i] + hdr[i].scan, (size_t)im.scan_len);
    memset(dst + im.scan_len, 0, (size_t)(a16(im.scan_offset + im.scan_len) - (im.scan_offset + im.scan_len)));
  }
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_scan_prepare_batch(const uint8_t* const* datas, const int64_t* sizes, int32_t B, void* staging, size_t staging_bytes,
                                              int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out) {
  return danhip_jpeg_scan_prepare_batch_ex(datas, sizes, B, 0, staging, staging_bytes, coef_capacity, descs_out, status_out);
}

extern "C" size_t danhip_jpeg_scan_device_bytes(const void* staging) {
  const DhScanHeader* h = (const DhScanHeader*)staging;
  return (!h || h->magic != DH_HUFF_MAGIC || h->used_bytes < 0) ? 0 : (size_t)h->used_bytes;
}

// workspace of the launches: exits [nitems] | seam entries int32 [2][ngroups] | group tails int64 [ngroups] | DC chunk sums int64 [nchunks][3]
extern "C" size_t danhip_jpeg_scan_workspace_bytes(const void* staging) {
  const DhScanHeader* h = (const DhScanHeader*)staging;
  if (!h || h->magic != DH_HUFF_MAGIC || h->nitems < 0 || h->ngroups < 0 || h->nchunks < 0) return 0;
  return (size_t)(a16((int64_t)h->nitems * 16) + a16((int64_t)h->ngroups * 8) + a16((int64_t)h->ngroups * 8) + a16((int64_t)h->nchunks * 24) + 16);
}

namespace {

struct EmuCtx {                    // the context of jpeg_huffman.h with every index checked: a refused one is counted and reads as 0
  const uint8_t* scan; int64_t scan_bytes;
  int64_t win_base; int32_t base, data_len;
  const DhHuffTab* tabs; int32_t ntabs;
  int16_t* coef; int64_t coef_n;
  const danhip_jpeg_desc* desc;
  int64_t* errors;
  bool ok(int64_t i, int64_t n) { if (i < 0 || i >= n) { ++*errors; return false; } return true; }
  uint32_t byte(int32_t i) {
    if ((uint32_t)i >= (uint32_t)data_len) return 0;
    const uint32_t o = (uint32_t)(base + i);
    if (o >= (uint32_t)DH_HUFF_WINDOW) return 0;
    return ok(win_base + o, scan_bytes) ? scan[win_base + o] : 0;
  }
  uint32_t look(int t, uint32_t i) { return ok(t, ntabs) && ok(i, 512) ? tabs[t].look[i] : 0; }
  int32_t maxcode(int t, int l) { return ok(t, ntabs) && ok(l, 18) ? tabs[t].maxcode[l] : 0x7fffffff; }
  int32_t valoff(int t, int l) { return ok(t, ntabs) && ok(l, 18) ? tabs[t].valoff[l] : 0; }
  uint32_t sym(int t, int i) { return ok(t, ntabs) && ok(i, 256) ? tabs[t].sym[i] : 0; }
  uint32_t zig(int k) { return ok(k, 64) ? kZigColMajor[k] : 0; }
  void store(int64_t blk, int el, int v) { if (ok(el, 64) && ok(blk * 64 + el, coef_n)) coef[blk * 64 + el] = (int16_t)v; }
  int load(int64_t blk, int el) { return ok(el, 64) && ok(blk * 64 + el, coef_n) ? coef[blk * 64 + el] : 0; }
  uint32_t quant(int comp, int nat) { return ok(comp, 3) && ok(nat, 64) ? desc->quant[desc->quant_index[comp]][nat] : 1; }
};

}  // namespace

extern "C" int danhip_jpeg_entropy_emulate_batch(const void* staging, size_t staging_bytes, int32_t B, const danhip_jpeg_desc* descs, int16_t* coef_out,
                                                 int64_t coef_count, int32_t sync_rounds, int32_t* status_out, int64_t* range_errors) {
  if (range_errors) *range_errors = 0;
  if (!status_out || coef_count < 0 || (coef_count > 0 && !coef_out)) {
    danhip_set_error("jpeg_entropy_emulate_batch: bad arguments");
    return DANHIP_EINVAL;
  }
  const char* why = dh_jpeg_scan_check(staging, staging_bytes, B, descs, coef_count);
  if (why) {
    danhip_set_error("jpeg_entropy_emulate_batch: %s", why);
    return DANHIP_EINVAL;
  }
  const uint8_t* base = (const uint8_t*)staging;
  const DhScanHeader* h = (const DhScanHeader*)staging;
  ScanView v{h, (const DhScanImage*)(base + h->off_images), (const DhScanSeg*)(base + h->off_segs), (const DhScanItem*)(base + h->off_items),
             (const DhScanGroup*)(base + h->off_groups), (const DhDcChunk*)(base + h->off_chunks), (const DhHuffTab*)(base + h->off_tabs),
             base + h->off_scan};
  const int rounds = sync_rounds < 0 ? DANHIP_JPEG_SYNC_ROUNDS : sync_rounds;
  int64_t errors = 0;
  for (int32_t i = 0; i < B; ++i) {
    status_out[i] = 0;
    if (v.images[i].prepared) memset(coef_out + v.images[i].coef_offset, 0, (size_t)descs[i].coef_count * 2);        // launch 1: zero
  }
  std::vector<DhExit> ex((size_t)h->nitems);
  std::vector<int32_t> seam[2] = {std::vector<int32_t>((size_t)h->ngroups), std::vector<int32_t>((size_t)h->ngroups)};
  std::vector<int64_t> tail((size_t)h->ngroups);

  auto context = [&](const DhScanGroup& gr, const DhScanSeg& sg) {
    const DhScanImage& im = v.images[gr.image];
    EmuCtx c;
    c.scan = v.scan; c.scan_bytes = h->scan_bytes;
    c.win_base = gr.win_base; c.base = (int32_t)(im.scan_offset + sg.offset - gr.win_base); c.data_len = sg.data_len;
    c.tabs = v.tabs + im.tab_first; c.ntabs = 2 * im.ncomp;
    c.coef = coef_out + im.coef_offset; c.coef_n = descs[gr.image].coef_count;
    c.desc = &descs[gr.image];
    c.errors = &errors;
    return c;
  };
  auto sub_of = [&](const DhScanImage& im, const DhScanSeg& sg, const DhScanItem& x) {
    DhSub a;
    a.start = x.sub * DH_HUFF_S;
    a.end = a.start + DH_HUFF_S < sg.data_len ? a.start + DH_HUFF_S : sg.data_len;
    a.data_len = sg.data_len; a.bpm = im.bpm; a.nl = im.hs * im.vs;
    return a;
  };

  for (int r = 0; r <= rounds; ++r) {                            // launches 2 .. 2 + rounds: speculate, then the synchronisation rounds
    for (int32_t g = 0; g < h->ngroups; ++g) {
      const DhScanGroup& gr = v.groups[g];
      const DhScanImage& im = v.images[gr.image];
      const int32_t n = gr.nitems;
      std::vector<DhExit> cur((size_t)n), nxt((size_t)n);
      for (int32_t t = 0; t < n; ++t) {
        const DhScanItem& x = v.items[gr.first_item + t];
        if (r == 0) {
          EmuCtx c = context(gr, v.segs[x.seg]);
          cur[(size_t)t] = dh_huff_decode_sub<EmuCtx, false>(c, sub_of(im, v.segs[x.seg], x), 0, nullptr, nullptr);
        } else {
          cur[(size_t)t] = ex[(size_t)(gr.first_item + t)];
        }
      }
      for (int32_t iter = 0; iter < n; ++iter) {                 // the loop around __syncthreads(): until no lane has changed anything
        bool any = false;
        for (int32_t t = 0; t < n; ++t) {
          const DhScanItem& x = v.items[gr.first_item + t];
          int32_t entry;
          if (x.sub == 0) entry = 0;
          else if (t > 0) entry = dh_huff_pack(cur[(size_t)t - 1].off, cur[(size_t)t - 1].state);
          else entry = r == 0 ? 0 : seam[(r - 1) & 1][(size_t)g - 1];
          nxt[(size_t)t] = cur[(size_t)t];
          if (entry == cur[(size_t)t].entry) continue;
          EmuCtx c = context(gr, v.segs[x.seg]);
          nxt[(size_t)t] = dh_huff_decode_sub<EmuCtx, false>(c, sub_of(im, v.segs[x.seg], x), entry, nullptr, nullptr);
          any = true;
        }
        cur.swap(nxt);
        if (!any) break;
      }
      int64_t run = 0;
      for (int32_t t = 0; t < n; ++t) {
        if (v.items[gr.first_item + t].sub == 0) run = 0;
        run += cur[(size_t)t].n;
        ex[(size_t)(gr.first_item + t)] = cur[(size_t)t];
      }
      tail[(size_t)g] = run;
      seam[r & 1][(size_t)g] = dh_huff_pack(cur[(size_t)n - 1].off, cur[(size_t)n - 1].state);
    }
  }

  for (int32_t g = 0; g < h->ngroups; ++g) {                     // write and verify
    const DhScanGroup& gr = v.groups[g];
    const DhScanImage& im = v.images[gr.image];
    const DhBlockGeom geom = block_geom(im);
    int64_t run = 0;
    for (int32_t k = gr.carry_from; k < g; ++k) run += tail[(size_t)k];
    for (int32_t t = 0; t < gr.nitems; ++t) {
      const int32_t item = gr.first_item + t;
      const DhScanItem& x = v.items[item];
      const DhScanSeg& sg = v.segs[x.seg];
      if (x.sub == 0) run = 0;
      const int32_t entry = x.sub == 0 ? 0 : dh_huff_pack(ex[(size_t)item - 1].off, ex[(size_t)item - 1].state);
      DhWrite w;
      w.cur = run; w.seg_blocks = (int64_t)sg.mcu_count * im.bpm; w.first_block = (int64_t)sg.first_mcu * im.bpm; w.final = sg.final;
      EmuCtx c = context(gr, sg);
      const DhExit e = dh_huff_decode_sub<EmuCtx, true>(c, sub_of(im, sg, x), entry, &geom, &w);
      const DhExit& st = ex[(size_t)item];
      if (!w.capped && (e.off != st.off || e.state != st.state || e.n != st.n)) status_out[gr.image] |= DANHIP_JPEG_DEV_NOTSYNC;
      if (w.error) status_out[gr.image] |= DANHIP_JPEG_DEV_ERROR;
      if (x.sub == sg.nitems - 1 && run + st.n < w.seg_blocks) status_out[gr.image] |= DANHIP_JPEG_DEV_ERROR;      // the data end before the blocks do
      run += st.n;
    }
  }

  std::vector<int64_t> sums((size_t)h->nchunks * 3);             // DC prefix sum, int16 range, block energy
  for (int pass = 0; pass < 2; ++pass) {
    for (int32_t k = 0; k < h->nchunks; ++k) {
      const DhDcChunk& ck = v.chunks[k];
      const DhScanImage& im = v.images[ck.image];
      const DhBlockGeom geom = block_geom(im);
      EmuCtx c = context(v.groups[im.first_group], v.segs[ck.seg]);
      int64_t pred[3] = {0, 0, 0};
      if (pass == 1)
        for (int32_t j = ck.chain_from; j < k; ++j)
          for (int q = 0; q < 3; ++q) pred[q] += sums[(size_t)j * 3 + q];
      for (int32_t m = 0; m < ck.n; ++m) {
        const int64_t mcu = (int64_t)v.segs[ck.seg].first_mcu + ck.mcu0 + m;
        if (pass == 0) {
          int64_t s[3];
          dh_dc_mcu_sum(c, geom, mcu, s);
          for (int q = 0; q < 3; ++q) sums[(size_t)k * 3 + q] += s[q];
        } else if (dh_dc_mcu_apply(c, geom, mcu, pred)) {
          status_out[ck.image] |= DANHIP_JPEG_DEV_ERROR;
        }
      }
    }
  }
  if (range_errors) *range_errors = errors;
  return DANHIP_OK;
}
