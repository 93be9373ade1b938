// Host half of the JPEG decoder (include/danhip.h, "Baseline JPEG decode"): marker parsing, validation and Huffman decoding of baseline
// streams into de-zigzagged, column-major int16 coefficient blocks plus one descriptor per image for the two device launches of
// jpeg_exact.hip.  Plain C++: no HIP call, usable in a process without a GPU.  A malformed stream ends here as a reason code; nothing
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
  int64_t scan = 0;          // first byte of the entropy-coded segment
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

// Markers up to and including SOS.  0 = a stream the device path decodes.
int parse_header(const uint8_t* d, int64_t n, Header* H) {
  if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return DANHIP_JPEG_ENOTJPEG;
  int64_t p = 2;
  bool have_sof = false;
  int adobe_transform = -1, ids[3] = {0, 0, 0}, hv[3] = {0, 0, 0};
  for (;;) {
    if (p >= n) return DANHIP_JPEG_ETRUNCATED;
    if (d[p] != 0xFF) return DANHIP_JPEG_ENOTJPEG;
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
    if (m == 0xC2) return DANHIP_JPEG_EPROGRESSIVE;
    if (m >= 0xC9 && m <= 0xCF) return DANHIP_JPEG_EARITHMETIC;
    if (m == 0xC3 || (m >= 0xC5 && m <= 0xC8) || m == 0xDC || m == 0xDE || m == 0xDF) return DANHIP_JPEG_EUNSUPPORTED;
    if (m == 0xC0 || m == 0xC1) {
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
    } else if (m == 0xDD) {
      if (L != 2) return DANHIP_JPEG_ETABLE;
      H->restart = be16(s);
    } else if (m == 0xEE) {
      if (L >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
    } else if (m == 0xDA) {
      if (!have_sof) return DANHIP_JPEG_ETABLE;
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

void clear_desc(danhip_jpeg_desc* d, int status) {
  memset(d, 0, sizeof(*d));
  d->status = status;
}

}  // namespace

extern "C" int danhip_jpeg_inspect(const uint8_t* data, int64_t n, danhip_jpeg_info* info) {
  if (!info) { danhip_set_error("jpeg_inspect: info is NULL"); return DANHIP_EINVAL; }
  memset(info, 0, sizeof(*info));
  Header* H = new Header();
  int rc = parse_header(data, n, H);
  DhJpegGeom g;
  if (rc == 0 && !dh_jpeg_geometry(H->width, H->height, H->mode, &g)) rc = DANHIP_JPEG_ETOOLARGE;
  info->reason = rc;
  if (rc == 0) {
    info->width = H->width; info->height = H->height; info->ncomp = H->ncomp; info->mode = H->mode;
    info->coef_count = g.coef_count;
  }
  delete H;
  return rc;
}

extern "C" int danhip_jpeg_entropy_decode_batch(const uint8_t* const* datas, const int64_t* sizes, int32_t B, int32_t threads, int16_t* coef_out,
                                                int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out) {
  if (!datas || !sizes || B < 1 || B > 65535 || !descs_out || !status_out || coef_capacity < 0 || (coef_capacity > 0 && !coef_out)) {
    danhip_set_error("jpeg_entropy_decode_batch: bad arguments (1 <= B <= 65535, no NULL table)");
    return DANHIP_EINVAL;
  }
  std::vector<Header> hdr((size_t)B);
  std::vector<DhJpegGeom> geom((size_t)B);
  int64_t next = 0;
  for (int32_t i = 0; i < B; ++i) {                              // headers in order: the coefficient slots
    int rc = parse_header(datas[i], sizes[i], &hdr[i]);
    if (rc == 0 && !dh_jpeg_geometry(hdr[i].width, hdr[i].height, hdr[i].mode, &geom[i])) rc = DANHIP_JPEG_ETOOLARGE;
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
      status_out[i] = decode_scan(datas[i], sizes[i], hdr[i], geom[i], coef_out + descs_out[i].coef_offset);
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
    const Header& H = hdr[i];
    const DhJpegGeom& g = geom[i];
    d->width = H.width; d->height = H.height; d->ncomp = H.ncomp; d->mode = H.mode;
    for (int c = 0; c < 3; ++c) {
      d->blocks_w[c] = g.blocks_w[c]; d->blocks_h[c] = g.blocks_h[c]; d->comp_w[c] = g.comp_w[c]; d->comp_h[c] = g.comp_h[c];
      d->quant_index[c] = c < g.ncomp ? H.tq[c] : 0;
      d->plane_offset[c] = 0;
      if (c < g.ncomp) { d->plane_offset[c] = ws; ws += dh_jpeg_align(g.plane_bytes[c], 256); }
    }
    d->idct_groups = g.idct_groups; d->rgb_groups = g.rgb_groups;
    d->out_offset = out;
    out += dh_jpeg_align(g.out_bytes, 256);
    for (int t = 0; t < 4; ++t)
      for (int k = 0; k < 64; ++k) d->quant[t][k] = H.quant_defined[t] ? H.quant[t][k] : 1;
  }
  return DANHIP_OK;
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
