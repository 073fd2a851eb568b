// The host half of the JPEG decode (include/fastvim_hip.h at fv_jpeg_probe): marker parser and Huffman decoder of baseline
// JPEG files, plain C++ with nothing from HIP -- the file also compiles on its own with the host compiler
// (tools/jpeg_host_check.cpp runs it under the address and undefined-behaviour sanitizers).  No global state: any number
// of loader threads may decode at once.  Every read is checked against [data, data + nbytes), every write against
// coef_out[0 : coef_capacity]; an anomaly is an error code, never a partial result.
//
// The decoder is the shape of libjpeg's jdhuff.c: a 64-bit bit buffer filled a byte at a time (0xFF 0x00 unstuffed, fill
// 0xFF bytes skipped, a marker stops the fill and zero bits follow), and a lookahead table of LOOK bits that gives
// length and symbol of every code that short in one probe; longer codes walk maxcode[].
#include <stdint.h>
#include <string.h>

#include "../../include/fastvim_hip.h"

namespace {

constexpr int LOOK = 9;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool present = false;
  uint16_t look[1 << LOOK];      // length << 8 | symbol of a code of at most LOOK bits, 0: longer
  int32_t maxcode[18];           // largest code of each length, -1: none
  int32_t valoff[17];            // index of the first symbol of each length minus its first code
  uint8_t vals[256];
  int nvals = 0;
};

struct Frame {
  int H = 0, W = 0, ncomp = 0, cls = -1, reason = FV_JPEG_R_MALFORMED;
  int hmax = 1, vmax = 1, mcus_x = 0, mcus_y = 0, ri = 0;
  int ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, ctq[3] = {0, 0, 0}, cid[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  uint16_t qt[4][64];            // natural order
  bool qt_present[4] = {false, false, false, false}, qt16[4] = {false, false, false, false};
  Huff huff[2][4];
  long long scan = 0;            // offset of the first entropy-coded byte
};

bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
  memset(h.look, 0, sizeof(h.look));
  memcpy(h.vals, vals, (size_t)nvals);
  h.nvals = nvals;
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int n = counts[len - 1];
    h.valoff[len] = k - code;
    if (n) {
      if (code + n > (1 << len)) return false;
      if (len <= LOOK)
        for (int i = 0; i < n; ++i) {
          const int first = (code + i) << (LOOK - len);
          for (int j = 0; j < (1 << (LOOK - len)); ++j) h.look[first + j] = (uint16_t)(len << 8 | vals[k + i]);
        }
      code += n;
      k += n;
      h.maxcode[len] = code - 1;
    } else {
      h.maxcode[len] = -1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  h.present = true;
  return true;
}

// Markers up to and including the first SOS; f.reason says whether the file is served.
void parse(const uint8_t* d, long long n, Frame& f) {
  f.reason = FV_JPEG_R_MALFORMED;
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return;
  long long pos = 2;
  int frame = -1, precision = 0, adobe = -1;
  bool jfif = false;
  for (;;) {
    if (pos + 4 > n || d[pos] != 0xFF) return;
    while (pos + 1 < n && d[pos + 1] == 0xFF) ++pos;
    if (pos + 1 >= n) return;
    const int m = d[pos + 1];
    pos += 2;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || pos + 2 > n) return;
    const long long ln = (d[pos] << 8) | d[pos + 1];
    if (ln < 2 || pos + ln > n) return;
    const uint8_t* seg = d + pos + 2;
    const int sl = (int)ln - 2;
    pos += ln;
    if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        if (tq > 3 || pq > 1 || q + 1 + 64 * (pq + 1) > sl) return;
        for (int k = 0; k < 64; ++k)
          f.qt[tq][kZigzag[k]] = pq ? (uint16_t)((seg[q + 1 + 2 * k] << 8) | seg[q + 2 + 2 * k]) : seg[q + 1 + k];
        f.qt_present[tq] = true;
        f.qt16[tq] = pq != 0;
        q += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return;
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        int nv = 0;
        for (int k = 0; k < 16; ++k) nv += seg[q + 1 + k];
        if (tc > 1 || th > 3 || nv > 256 || q + 17 + nv > sl) return;
        if (!build_huff(f.huff[tc][th], seg + q + 1, seg + q + 17, nv)) return;
        q += 17 + nv;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return;
      f.ri = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0 && sl >= 14 && memcmp(seg, "JFIF\0", 5) == 0) {
      jfif = true;
    } else if (m == 0xEE && sl >= 12 && memcmp(seg, "Adobe", 5) == 0) {
      adobe = seg[11];
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (frame >= 0 || sl < 6) return;
      frame = m;
      precision = seg[0];
      f.H = (seg[1] << 8) | seg[2];
      f.W = (seg[3] << 8) | seg[4];
      f.ncomp = seg[5];
      if (sl != 6 + 3 * f.ncomp || f.H == 0 || f.W == 0 || f.ncomp == 0) {
        f.H = f.W = f.ncomp = 0;
        return;
      }
      for (int c = 0; c < f.ncomp && c < 3; ++c) {
        f.cid[c] = seg[6 + 3 * c];
        f.ch[c] = seg[7 + 3 * c] >> 4;
        f.cv[c] = seg[7 + 3 * c] & 15;
        f.ctq[c] = seg[8 + 3 * c];
      }
    } else if (m == 0xDA) {
      if (frame < 0) return;
      const int nc = f.ncomp;
      if (frame == 0xC2 || frame == 0xC6 || frame == 0xCA || frame == 0xCE) { f.reason = FV_JPEG_R_PROGRESSIVE; return; }
      if (frame >= 0xC9) { f.reason = FV_JPEG_R_ARITHMETIC; return; }
      if (frame != 0xC0) { f.reason = FV_JPEG_R_FRAME; return; }
      if (precision != 8) { f.reason = FV_JPEG_R_PRECISION; return; }
      if (nc != 1 && nc != 3) { f.reason = FV_JPEG_R_COMPONENTS; return; }
      if (nc == 3) {
        if (adobe >= 0) {
          if (adobe != 1) { f.reason = FV_JPEG_R_COLOUR; return; }
        } else if (!jfif && f.cid[0] == 'R' && f.cid[1] == 'G' && f.cid[2] == 'B') {
          f.reason = FV_JPEG_R_COLOUR;
          return;
        }
      }
      for (int c = 0; c < nc; ++c)
        if (f.ch[c] < 1 || f.ch[c] > 4 || f.cv[c] < 1 || f.cv[c] > 4) return;
      if (nc == 1) {
        if (f.ch[0] != 1 || f.cv[0] != 1) { f.reason = FV_JPEG_R_SAMPLING; return; }
        f.cls = FV_JPEG_GRAY;
      } else {
        const int h = f.ch[0], v = f.cv[0];
        if (f.ch[1] != 1 || f.cv[1] != 1 || f.ch[2] != 1 || f.cv[2] != 1 || !((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) {
          f.reason = FV_JPEG_R_SAMPLING;
          return;
        }
        f.cls = h == 1 ? FV_JPEG_444 : v == 1 ? FV_JPEG_422 : FV_JPEG_420;
      }
      f.reason = FV_JPEG_R_MALFORMED;
      const int cls = f.cls;
      f.cls = -1;
      if (sl < 1 || sl != 4 + 2 * seg[0]) return;
      if (seg[0] != nc) { f.reason = FV_JPEG_R_SCANS; return; }
      for (int c = 0; c < nc; ++c) {
        if (seg[1 + 2 * c] != f.cid[c]) { f.reason = FV_JPEG_R_SCANS; return; }
        f.td[c] = seg[2 + 2 * c] >> 4;
        f.ta[c] = seg[2 + 2 * c] & 15;
        if (f.td[c] > 3 || f.ta[c] > 3 || !f.huff[0][f.td[c]].present || !f.huff[1][f.ta[c]].present) return;
        if (f.ctq[c] > 3 || !f.qt_present[f.ctq[c]]) return;
        if (f.qt16[f.ctq[c]]) { f.reason = FV_JPEG_R_TABLES16; return; }
      }
      if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0) return;
      f.cls = cls;
      f.hmax = f.ch[0];
      f.vmax = f.cv[0];
      f.mcus_x = (f.W + 8 * f.hmax - 1) / (8 * f.hmax);
      f.mcus_y = (f.H + 8 * f.vmax - 1) / (8 * f.vmax);
      f.scan = pos;
      f.reason = FV_JPEG_R_OK;
      return;
    }
  }
}

struct Bits {
  const uint8_t* d;
  long long n, pos;
  uint64_t buf = 0;
  int bits = 0;        // bits in buf, zero padding included
  int real = 0;        // of them, bits that came from the file; negative: padding was consumed
  bool stopped = false;  // at a marker or at the end of the data

  void fill() {
    while (bits <= 56) {
      int b = 0;
      if (!stopped) {
        if (pos >= n) {
          stopped = true;
        } else {
          b = d[pos];
          if (b == 0xFF) {
            long long p = pos;
            while (p + 1 < n && d[p + 1] == 0xFF) ++p;      // fill bytes
            if (p + 1 >= n || d[p + 1] != 0) {
              pos = p;                                      // at the 0xFF of a marker (or the last byte)
              stopped = true;
              b = 0;
            } else {
              pos = p + 2;
            }
          } else {
            ++pos;
          }
        }
      }
      buf = (buf << 8) | (uint64_t)b;
      bits += 8;
      if (!stopped) real += 8;
    }
  }
  inline uint32_t peek(int k) const { return (uint32_t)(buf >> (bits - k)) & ((1u << k) - 1u); }
  inline void skip(int k) { bits -= k; real -= k; }
  inline uint32_t get(int k) { const uint32_t v = peek(k); skip(k); return v; }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one symbol; -1: no such code.  Needs 16 bits in the buffer.
inline int symbol(Bits& b, const Huff& h) {
  const uint16_t e = h.look[b.peek(LOOK)];
  if (e) {
    b.skip(e >> 8);
    return e & 255;
  }
  int len = LOOK + 1;
  int32_t code = (int32_t)b.peek(len);
  while (len <= 16 && code > h.maxcode[len]) {
    ++len;
    if (len <= 16) code = (int32_t)b.peek(len);
  }
  if (len > 16) return -1;
  const int idx = h.valoff[len] + code;
  if (idx < 0 || idx >= h.nvals) return -1;
  b.skip(len);
  return h.vals[idx];
}

}  // namespace

extern "C" int fv_jpeg_probe(const void* data, long long nbytes, int* info) {
  if (!data || !info || nbytes < 0) return FV_ERR_INVALID;
  Frame f;
  parse((const uint8_t*)data, nbytes, f);
  const bool ok = f.reason == FV_JPEG_R_OK;
  info[0] = f.H;
  info[1] = f.W;
  info[2] = f.ncomp;
  info[3] = ok ? f.cls : -1;
  info[4] = ok ? 1 : 0;
  info[5] = f.reason;
  info[6] = ok ? f.mcus_x : 0;
  info[7] = ok ? f.mcus_y : 0;
  return FV_OK;
}

extern "C" int fv_jpeg_entropy_decode(const void* data, long long nbytes, const int* window, int16_t* coef_out,
                                      long long coef_capacity, int* record) {
  if (!data || !window || !coef_out || !record || nbytes < 0 || coef_capacity < 0) return FV_ERR_INVALID;
  Frame f;
  parse((const uint8_t*)data, nbytes, f);
  if (f.reason != FV_JPEG_R_OK) return FV_JPEG_E_UNSERVED;
  const int x0 = window[0], y0 = window[1], mw = window[2], mh = window[3];
  if (x0 < 0 || y0 < 0 || mw < 1 || mh < 1 || x0 > f.mcus_x - mw || y0 > f.mcus_y - mh) return FV_JPEG_E_WINDOW;
  const int nc = f.ncomp;
  long long off[3] = {0, 0, 0}, total = 0, blocks = 0;
  for (int c = 0; c < nc; ++c) {
    off[c] = total;
    const long long nb = (long long)mw * f.ch[c] * mh * f.cv[c];
    blocks += nb;
    total += nb * 64;
  }
  if (total > coef_capacity || blocks > 0x7fffffff) return FV_JPEG_E_CAPACITY;

  Bits b{(const uint8_t*)data, nbytes, f.scan};
  int pred[3] = {0, 0, 0};
  const long long last = (long long)(y0 + mh - 1) * f.mcus_x + x0 + mw - 1;
  int mx = 0, my = 0, to_restart = f.ri, rst = 0;
  int16_t skipped[64];
  for (long long m = 0; m <= last; ++m) {
    if (f.ri && m && to_restart == 0) {
      // byte-align; a whole data byte left over is not what an encoder writes
      if (b.real < 0) return FV_JPEG_E_TRUNCATED;
      if (b.real >= 8) return FV_JPEG_E_RESTART;
      b.fill();                                             // runs the fill up to the marker if it has not got there
      if (b.real >= 8 || !b.stopped) return FV_JPEG_E_RESTART;
      long long p = b.pos;
      if (p + 1 >= nbytes) return FV_JPEG_E_TRUNCATED;
      if (b.d[p] != 0xFF) return FV_JPEG_E_RESTART;
      while (p + 1 < nbytes && b.d[p + 1] == 0xFF) ++p;
      if (p + 1 >= nbytes) return FV_JPEG_E_TRUNCATED;
      if (b.d[p + 1] != 0xD0 + (rst & 7)) return FV_JPEG_E_RESTART;
      b.pos = p + 2;
      b.buf = 0;
      b.bits = b.real = 0;
      b.stopped = false;
      rst++;
      pred[0] = pred[1] = pred[2] = 0;
      to_restart = f.ri;
    }
    --to_restart;
    const bool inside = my >= y0 && my < y0 + mh && mx >= x0 && mx < x0 + mw;
    for (int c = 0; c < nc; ++c) {
      const Huff& dc = f.huff[0][f.td[c]];
      const Huff& ac = f.huff[1][f.ta[c]];
      const int h = f.ch[c], v = f.cv[c];
      for (int by = 0; by < v; ++by)
        for (int bx = 0; bx < h; ++bx) {
          int16_t* blk = skipped;
          if (inside) {
            const long long e = off[c] + (((long long)(my - y0) * v + by) * ((long long)mw * h) + (long long)(mx - x0) * h + bx) * 64;
            if (e < 0 || e + 64 > coef_capacity) return FV_JPEG_E_CAPACITY;
            blk = coef_out + e;
          }
          memset(blk, 0, 128);
          if (b.bits < 32) b.fill();
          int s = symbol(b, dc);
          if (s < 0 || s > 15) return FV_JPEG_E_CODE;
          if (s) pred[c] = (int16_t)(pred[c] + extend((int)b.get(s), s));
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            if (b.bits < 32) b.fill();
            const int rs = symbol(b, ac);
            if (rs < 0) return FV_JPEG_E_CODE;
            const int r = rs >> 4;
            s = rs & 15;
            if (s) {
              k += r;
              if (k > 63) return FV_JPEG_E_RUN;
              blk[kZigzag[k]] = (int16_t)extend((int)b.get(s), s);
              ++k;
            } else if (r == 15) {
              k += 16;
              if (k > 64) return FV_JPEG_E_RUN;
            } else {
              break;
            }
          }
          if (b.real < 0) return FV_JPEG_E_TRUNCATED;
        }
    }
    if (++mx == f.mcus_x) { mx = 0; ++my; }
  }

  memset(record, 0, sizeof(int) * FV_JPEG_REC_INTS);
  record[0] = 1;
  record[1] = f.H;
  record[2] = f.W;
  record[3] = nc;
  record[4] = f.cls;
  record[5] = x0; record[6] = y0; record[7] = mw; record[8] = mh;
  for (int c = 0; c < nc; ++c) {
    record[9 + 2 * c] = (int)(uint32_t)(off[c] & 0xffffffffll);
    record[10 + 2 * c] = (int)(off[c] >> 32);
    for (int k = 0; k < 64; ++k) record[32 + 64 * c + k] = f.qt[f.ctq[c]][k];
  }
  record[15] = (int)(uint32_t)(total & 0xffffffffll);
  record[16] = (int)(total >> 32);
  record[17] = (int)blocks;
  record[18] = (int)(last + 1 > 0x7fffffff ? 0x7fffffff : last + 1);
  return FV_OK;
}
