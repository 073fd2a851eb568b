// The host half of the JPEG decode (include/fastvim_hip.h at fv_jpeg_probe): marker parser and Huffman decoder of baseline
// JPEG files, plain C++ with nothing from HIP -- the file also compiles on its own with the host compiler
// (tools/jpeg_host_check.cpp, tools/jpeg_packed_check.cpp, tools/jpeg_index_check.cpp and tools/jpeg_sync_check.cpp run it under the address and
// undefined-behaviour sanitizers).  No shared state -- the packed entry point keeps a scratch buffer per thread: any number of loader threads
// may decode at once.  Every read is checked against [data, data + nbytes), every write against
// coef_out[0 : coef_capacity]; an anomaly is an error code, never a partial result.
//
// The decoder is the shape of libjpeg's jdhuff.c: a 64-bit bit buffer filled a byte at a time (0xFF 0x00 unstuffed, fill
// 0xFF bytes skipped, a marker stops the fill and zero bits follow), and a lookahead table of LOOK bits that gives
// length and symbol of every code that short in one probe; longer codes walk maxcode[].
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/fastvim_hip.h"
#include "jpeg_huff_core.h"
#include "jpeg_sync_core.h"

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

// The window's geometry: the offset of each component's first block (in blocks) and the blocks of the window.
struct Window {
  int x0, y0, mw, mh;
  long long first[3] = {0, 0, 0}, blocks = 0;
};

int window_of(const Frame& f, const int* window, Window& w) {
  w.x0 = window[0]; w.y0 = window[1]; w.mw = window[2]; w.mh = window[3];
  if (w.x0 < 0 || w.y0 < 0 || w.mw < 1 || w.mh < 1 || w.x0 > f.mcus_x - w.mw || w.y0 > f.mcus_y - w.mh) return FV_JPEG_E_WINDOW;
  for (int c = 0; c < f.ncomp; ++c) {
    w.first[c] = w.blocks;
    w.blocks += (long long)w.mw * f.ch[c] * w.mh * f.cv[c];
  }
  return w.blocks > 0x7fffffff ? FV_JPEG_E_CAPACITY : FV_OK;
}

// The MCU loop of both entry points: MCUs in file order up to the last one the window needs; the 64 coefficients of a
// block inside the window go, natural order, to coef_out + 64 * (its number), every other block to a scratch block.
// With `masks` (one word per block of the window, or null) the block's word gets bit k set for every AC term k written --
// an AC term that is coded is never 0 -- and bit 0 when one of them lies outside -128 .. 127.  `mcus` is the count decoded.
int decode_mcus(const Frame& f, const uint8_t* data, long long nbytes, const Window& w, int16_t* coef_out,
                long long coef_capacity, uint64_t* masks, long long* mcus) {
  const int x0 = w.x0, y0 = w.y0, mw = w.mw, mh = w.mh, nc = f.ncomp;
  Bits b{data, nbytes, f.scan};
  int pred[3] = {0, 0, 0};
  const long long last = (long long)(y0 + mh - 1) * f.mcus_x + x0 + mw - 1;
  int mx = 0, my = 0, to_restart = f.ri, rst = 0;
  int16_t skipped[64];
  uint64_t skipped_mask;
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
          uint64_t* bits = &skipped_mask;
          if (inside) {
            const long long e = (w.first[c] + ((long long)(my - y0) * v + by) * ((long long)mw * h) + (long long)(mx - x0) * h + bx) * 64;
            if (e < 0 || e + 64 > coef_capacity) return FV_JPEG_E_CAPACITY;
            blk = coef_out + e;
            if (masks) bits = masks + e / 64;
          }
          uint64_t mask = 0;
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
              const int at = kZigzag[k], v = extend((int)b.get(s), s);
              blk[at] = (int16_t)v;
              mask |= (uint64_t)1 << at | (uint64_t)((unsigned)(v + 128) > 255u);
              ++k;
            } else if (r == 15) {
              k += 16;
              if (k > 64) return FV_JPEG_E_RUN;
            } else {
              break;
            }
          }
          if (b.real < 0) return FV_JPEG_E_TRUNCATED;
          *bits = mask;
        }
    }
    if (++mx == f.mcus_x) { mx = 0; ++my; }
  }
  *mcus = last + 1;
  return FV_OK;
}

// the words of the record both forms share
void common_record(const Frame& f, const Window& w, long long mcus, int kind, int* record) {
  memset(record, 0, sizeof(int) * FV_JPEG_REC_INTS);
  record[0] = kind;
  record[1] = f.H;
  record[2] = f.W;
  record[3] = f.ncomp;
  record[4] = f.cls;
  record[5] = w.x0; record[6] = w.y0; record[7] = w.mw; record[8] = w.mh;
  for (int c = 0; c < f.ncomp; ++c) {
    const long long off = w.first[c] * 64;       // dense: elements of the coefficients; both: bytes of the plane
    record[9 + 2 * c] = (int)(uint32_t)(off & 0xffffffffll);
    record[10 + 2 * c] = (int)(off >> 32);
    for (int k = 0; k < 64; ++k) record[32 + 64 * c + k] = f.qt[f.ctq[c]][k];
  }
  record[17] = (int)w.blocks;
  record[18] = (int)(mcus > 0x7fffffff ? 0x7fffffff : mcus);
}

// the packed entry point's dense window: kept per thread from call to call unless a single file made it large
struct Scratch {
  void* p = nullptr;
  size_t n = 0;
  ~Scratch() { free(p); }
  void* get(size_t need) {
    if (need > n) {
      free(p);
      p = malloc(need);
      n = p ? need : 0;
    }
    return p;
  }
  void trim() {
    if (n > ((size_t)16 << 20)) { free(p); p = nullptr; n = 0; }
  }
};
thread_local Scratch scratch;

inline void put_i64(int* record, int at, long long v) {
  record[at] = (int)(uint32_t)(v & 0xffffffffll);
  record[at + 1] = (int)(v >> 32);
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
  Window w;
  int rc = window_of(f, window, w);
  if (rc != FV_OK) return rc;
  const long long total = w.blocks * 64;
  if (total > coef_capacity) return FV_JPEG_E_CAPACITY;
  long long mcus = 0;
  rc = decode_mcus(f, (const uint8_t*)data, nbytes, w, coef_out, coef_capacity, nullptr, &mcus);
  if (rc != FV_OK) return rc;
  common_record(f, w, mcus, 1, record);
  put_i64(record, 15, total);
  return FV_OK;
}

extern "C" long long fv_jpeg_packed_bound(long long blocks) { return blocks > 0 ? blocks * (16 + 126) : 0; }

// The packed form (include/fastvim_hip.h): the MCU loop above decodes into a dense scratch of the window and notes each
// block's mask -- the file interleaves the components, the packed values are in block order -- and one pass over the
// masks writes headers and values.
extern "C" int fv_jpeg_entropy_decode_packed(const void* data, long long nbytes, const int* window, void* out,
                                             long long out_capacity_bytes, int* record) {
  if (!data || !window || !out || !record || nbytes < 0 || out_capacity_bytes < 0 || ((uintptr_t)out & 15)) return FV_ERR_INVALID;
  Frame f;
  parse((const uint8_t*)data, nbytes, f);
  if (f.reason != FV_JPEG_R_OK) return FV_JPEG_E_UNSERVED;
  Window w;
  int rc = window_of(f, window, w);
  if (rc != FV_OK) return rc;
  const long long vbase = 16 * w.blocks;
  if (vbase > out_capacity_bytes) return FV_JPEG_E_CAPACITY;      // also bounds the scratch: 8 x the capacity
  uint64_t* masks = (uint64_t*)scratch.get((size_t)w.blocks * (8 + 128));
  if (!masks) return FV_JPEG_E_CAPACITY;
  const int16_t* dense = (const int16_t*)(masks + w.blocks);
  long long mcus = 0;
  rc = decode_mcus(f, (const uint8_t*)data, nbytes, w, (int16_t*)(masks + w.blocks), w.blocks * 64, masks, &mcus);
  uint8_t* const o = (uint8_t*)out;
  long long cur = vbase;                                           // where the next block's values go; cur - vbase is even
  for (long long blk = 0; rc == FV_OK && blk < w.blocks; ++blk) {
    const int16_t* t = dense + blk * 64;
    const uint64_t mask = masks[blk] & ~(uint64_t)1;
    const bool wide = masks[blk] & 1;
    const int n = __builtin_popcountll(mask), bytes = wide ? 2 * n : n;
    if (cur - vbase > 0x7fffffff || cur + bytes + (bytes & 1) > out_capacity_bytes) { rc = FV_JPEG_E_CAPACITY; break; }
    const uint32_t hdr[4] = {(uint32_t)mask, (uint32_t)(mask >> 32), (uint32_t)(cur - vbase) | (wide ? 0x80000000u : 0u),
                             (uint32_t)(uint16_t)t[0]};
    memcpy(o + 16 * blk, hdr, 16);                                 // little-endian host, as the device
    uint8_t* v8 = o + cur;
    if (wide) {
      for (uint64_t m = mask; m; m &= m - 1, v8 += 2) memcpy(v8, t + __builtin_ctzll(m), 2);
    } else {
      for (uint64_t m = mask; m; m &= m - 1) *v8++ = (uint8_t)(int8_t)t[__builtin_ctzll(m)];
    }
    if (bytes & 1) *v8++ = 0;
    cur = v8 - o;
  }
  scratch.trim();
  if (rc != FV_OK) return rc;
  common_record(f, w, mcus, 2, record);
  put_i64(record, 15, cur);
  put_i64(record, 25, 0);
  put_i64(record, 27, vbase);
  return FV_OK;
}

// ---------------------------------------------------------------------------------------------------------- THE INDEX
// include/fastvim_hip.h at THE INDEX.  The builder decodes every group with the core the device runs (jpeg_huff_core.h),
// each from its own entry with a fresh reader -- an entry is by construction what a lane starts from -- and moves a
// (byte, bit) cursor over the stuffed stream by the bits the group consumed.
namespace {

constexpr uint32_t IDX_MAGIC = FV_JPEG_INDEX_MAGIC;
constexpr int IDX_HEAD_WORDS = FV_JPEG_REC_INTS;                                        // the tables sit where the record's do
constexpr int IDX_TABLE_WORDS = fvhuff::TABLES * fvhuff::TABLE_WORDS;
constexpr long long IDX_ENTRIES = 4ll * (IDX_HEAD_WORDS + IDX_TABLE_WORDS);             // byte offset of the first entry
constexpr int IDX_MAX_S = 65536;
static_assert(IDX_ENTRIES == FV_JPEG_INDEX_HEAD_BYTES && IDX_ENTRIES % 16 == 0, "the header's size");
static_assert(FV_JPEG_STREAM_REC_INTS == 32, "the stream record");

inline uint32_t rd32(const void* p, long long word) {
  uint32_t v;
  memcpy(&v, (const uint8_t*)p + 4 * word, 4);
  return v;
}

uint64_t fnv1a(const uint8_t* d, long long n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (long long i = 0; i < n; ++i) h = (h ^ d[i]) * 0x100000001b3ull;
  return h;
}

void pack_table(const Huff& h, uint32_t* t) {
  memset(t, 0, sizeof(uint32_t) * fvhuff::TABLE_WORDS);
  memcpy(t, h.look, sizeof(h.look));
  t[fvhuff::T_MAXCODE] = (uint32_t)-1;
  for (int l = 1; l <= 17; ++l) t[fvhuff::T_MAXCODE + l] = (uint32_t)h.maxcode[l];
  for (int l = 1; l <= 16; ++l) t[fvhuff::T_VALOFF + l] = (uint32_t)h.valoff[l];
  t[fvhuff::T_NVALS] = (uint32_t)h.nvals;
  memcpy(t + fvhuff::T_VALS, h.vals, (size_t)h.nvals);
}

// the four tables of a file in the order the device reads them
void pack_tables(const Frame& f, uint32_t* tables) {
  const int cc = f.ncomp == 3 ? 1 : 0;
  pack_table(f.huff[0][f.td[0]], tables);
  pack_table(f.huff[0][f.td[cc]], tables + fvhuff::TABLE_WORDS);
  pack_table(f.huff[1][f.ta[0]], tables + 2 * fvhuff::TABLE_WORDS);
  pack_table(f.huff[1][f.ta[cc]], tables + 3 * fvhuff::TABLE_WORDS);
}

// why a parsed file gets no entries (index or sync), or FV_JPEG_R_OK
int indexed_reason(const Frame& f) {
  if (f.reason != FV_JPEG_R_OK) return f.reason;
  if (f.ri) return FV_JPEG_R_RESTART;
  if (f.ncomp == 3 && (f.td[1] != f.td[2] || f.ta[1] != f.ta[2])) return FV_JPEG_R_CHROMA_TABLES;
  return FV_JPEG_R_OK;
}

struct Index {
  const uint8_t* p;
  int H, W, cls, ncomp, mcus_x, mcus_y, S, gpr;
  long long groups, scan;
  void entry(long long g, uint32_t* e) const { memcpy(e, p + IDX_ENTRIES + 16 * g, 16); }
};

// the header of an index against the file's size; nothing of it is trusted
int open_index(const void* index, long long index_bytes, long long nbytes, Index& ix) {
  if (index_bytes < IDX_ENTRIES + 16) return FV_JPEG_E_INDEX_FORMAT;
  ix.p = (const uint8_t*)index;
  if (rd32(index, 0) != IDX_MAGIC || rd32(index, 1) != FV_JPEG_INDEX_VERSION) return FV_JPEG_E_INDEX_FORMAT;
  const long long nb = (long long)(((uint64_t)rd32(index, 3) << 32) | rd32(index, 2));
  if (nb != nbytes || nbytes > 0x7fffffff) return FV_JPEG_E_INDEX_FILE;
  ix.H = (int)rd32(index, 6); ix.W = (int)rd32(index, 7); ix.cls = (int)rd32(index, 8); ix.ncomp = (int)rd32(index, 9);
  ix.mcus_x = (int)rd32(index, 10); ix.mcus_y = (int)rd32(index, 11); ix.S = (int)rd32(index, 12); ix.gpr = (int)rd32(index, 13);
  ix.groups = (long long)rd32(index, 14);
  ix.scan = (long long)(((uint64_t)rd32(index, 17) << 32) | rd32(index, 16));
  if (ix.cls < 0 || ix.cls > 3 || ix.ncomp != (ix.cls == FV_JPEG_GRAY ? 1 : 3)) return FV_JPEG_E_INDEX_FORMAT;
  if (ix.H < 1 || ix.H > 65535 || ix.W < 1 || ix.W > 65535 || ix.S < 1 || ix.S > IDX_MAX_S) return FV_JPEG_E_INDEX_FORMAT;
  const int hmax = (ix.cls == FV_JPEG_422 || ix.cls == FV_JPEG_420) ? 2 : 1, vmax = ix.cls == FV_JPEG_420 ? 2 : 1;
  if (ix.mcus_x != (ix.W + 8 * hmax - 1) / (8 * hmax) || ix.mcus_y != (ix.H + 8 * vmax - 1) / (8 * vmax)) return FV_JPEG_E_INDEX_FORMAT;
  if (ix.gpr != (ix.mcus_x + ix.S - 1) / ix.S || ix.groups != (long long)ix.gpr * ix.mcus_y) return FV_JPEG_E_INDEX_FORMAT;
  if (index_bytes < IDX_ENTRIES + 16 * (ix.groups + 1)) return FV_JPEG_E_INDEX_FORMAT;
  if (ix.scan < 0 || ix.scan > nbytes) return FV_JPEG_E_INDEX_FORMAT;
  return FV_OK;
}

}  // namespace

extern "C" long long fv_jpeg_index_bound(int mcus_x, int mcus_y, int segment_mcus) {
  if (mcus_x < 1 || mcus_y < 1 || mcus_x > 8192 || mcus_y > 8192 || segment_mcus < 1 || segment_mcus > IDX_MAX_S) return 0;
  return IDX_ENTRIES + 16 * ((long long)((mcus_x + segment_mcus - 1) / segment_mcus) * mcus_y + 1);
}

extern "C" long long fv_jpeg_build_index(const void* data, long long nbytes, int segment_mcus, void* out,
                                         long long out_capacity_bytes) {
  if (!data || !out || nbytes < 0 || out_capacity_bytes < 0 || segment_mcus < 1 || segment_mcus > IDX_MAX_S) return FV_ERR_INVALID;
  Frame f;
  const uint8_t* d = (const uint8_t*)data;
  parse(d, nbytes, f);
  const int reason = indexed_reason(f);
  if (reason != FV_JPEG_R_OK) {
    if (out_capacity_bytes >= 4) memcpy(out, &reason, 4);
    return FV_JPEG_E_UNSERVED;
  }
  if (nbytes > 0x7fffffff) return FV_JPEG_E_CAPACITY;
  const int S = segment_mcus, gpr = (f.mcus_x + S - 1) / S;
  const long long groups = (long long)gpr * f.mcus_y, total = IDX_ENTRIES + 16 * (groups + 1);
  if (total > out_capacity_bytes) return FV_JPEG_E_CAPACITY;
  uint32_t head[IDX_HEAD_WORDS];
  memset(head, 0, sizeof(head));
  const uint64_t hash = fnv1a(d, nbytes);
  head[0] = IDX_MAGIC; head[1] = FV_JPEG_INDEX_VERSION;
  head[2] = (uint32_t)nbytes; head[3] = (uint32_t)((uint64_t)nbytes >> 32);
  head[4] = (uint32_t)hash; head[5] = (uint32_t)(hash >> 32);
  head[6] = (uint32_t)f.H; head[7] = (uint32_t)f.W; head[8] = (uint32_t)f.cls; head[9] = (uint32_t)f.ncomp;
  head[10] = (uint32_t)f.mcus_x; head[11] = (uint32_t)f.mcus_y; head[12] = (uint32_t)S; head[13] = (uint32_t)gpr;
  head[14] = (uint32_t)groups;
  head[16] = (uint32_t)f.scan; head[17] = (uint32_t)((uint64_t)f.scan >> 32);
  for (int c = 0; c < f.ncomp; ++c)
    for (int k = 0; k < 64; ++k) head[32 + 64 * c + k] = f.qt[f.ctq[c]][k];
  // the tables the walk below reads are the ones that go into the index
  uint32_t* tables = (uint32_t*)malloc(sizeof(uint32_t) * IDX_TABLE_WORDS);
  if (!tables) return FV_JPEG_E_CAPACITY;
  pack_tables(f, tables);
  uint8_t* o = (uint8_t*)out;
  memcpy(o, head, sizeof(head));
  memcpy(o + sizeof(head), tables, sizeof(uint32_t) * IDX_TABLE_WORDS);
  fvhuff::Place nowhere{f.cls, 0, 0, 0, 0, {0, 0, 0}};             // an empty window: every block is dropped
  uint32_t byte = (uint32_t)f.scan, bit = 0;
  int pred[3] = {0, 0, 0};
  int rc = FV_OK;
  long long g = 0;
  for (int my = 0; my < f.mcus_y && rc == FV_OK; ++my)
    for (int gx = 0; gx < gpr && rc == FV_OK; ++gx, ++g) {
      const uint32_t e[4] = {byte, bit, (uint32_t)(uint16_t)pred[0] | (uint32_t)(uint16_t)pred[1] << 16, (uint32_t)(uint16_t)pred[2]};
      memcpy(o + IDX_ENTRIES + 16 * g, e, 16);
      const int count = f.mcus_x - gx * S < S ? f.mcus_x - gx * S : S;
      fvhuff::Reader end;
      const int st = fvhuff::decode_group(d, (uint32_t)nbytes, byte, (int)bit, pred[0], pred[1], pred[2], tables, nowhere, my,
                                          gx * S, count, nullptr, 0, &end);
      if (st != fvhuff::ST_OK) { rc = st == fvhuff::ST_RUN ? FV_JPEG_E_RUN : FV_JPEG_E_CODE; break; }
      if (fvhuff::past_end(end)) { rc = FV_JPEG_E_TRUNCATED; break; }
      // the cursor moves over whole stuffed bytes: it never rests on a stuffed 0x00
      uint32_t left = fvhuff::consumed(end);
      while (left >= 8) {
        if ((long long)byte >= nbytes) { rc = FV_JPEG_E_TRUNCATED; break; }
        byte += d[byte] == 0xFF ? 2 : 1;
        left -= 8;
      }
      bit = left;
    }
  free(tables);
  if (rc != FV_OK) return rc;
  const uint32_t e[4] = {byte, bit, (uint32_t)(uint16_t)pred[0] | (uint32_t)(uint16_t)pred[1] << 16, (uint32_t)(uint16_t)pred[2]};
  memcpy(o + IDX_ENTRIES + 16 * groups, e, 16);                   // the end sentinel
  return total;
}

extern "C" int fv_jpeg_index_stage(const void* data, long long nbytes, const void* index, long long index_bytes,
                                   const int* window, int verify, void* pool, long long pool_capacity_bytes,
                                   long long* pool_used, long long coef_base, int* record, int* stream_record) {
  if (!data || !index || !window || !pool || !pool_used || !record || !stream_record || nbytes < 0 || index_bytes < 0 ||
      pool_capacity_bytes < 0 || *pool_used < 0 || coef_base < 0 || (coef_base & 7) || ((uintptr_t)pool & 15))
    return FV_ERR_INVALID;
  Index ix;
  int rc = open_index(index, index_bytes, nbytes, ix);
  if (rc != FV_OK) return rc;
  const uint8_t* d = (const uint8_t*)data;
  if (verify) {
    const uint64_t hash = fnv1a(d, nbytes);
    if (rd32(index, 4) != (uint32_t)hash || rd32(index, 5) != (uint32_t)(hash >> 32)) return FV_JPEG_E_INDEX_FILE;
  }
  Frame geo;                                                      // only what window_of reads
  geo.ncomp = ix.ncomp; geo.mcus_x = ix.mcus_x; geo.mcus_y = ix.mcus_y;
  geo.ch[0] = (ix.cls == FV_JPEG_422 || ix.cls == FV_JPEG_420) ? 2 : 1;
  geo.cv[0] = ix.cls == FV_JPEG_420 ? 2 : 1;
  Window w;
  rc = window_of(geo, window, w);
  if (rc != FV_OK) return rc;
  const int gx0 = w.x0 / ix.S, gx1 = (w.x0 + w.mw - 1) / ix.S, gw = gx1 - gx0 + 1;
  const long long lanes = (long long)gw * w.mh;
  // every entry a lane starts from, and the one behind each row's last group, inside the scan and in file order
  uint32_t e[4];
  long long before = ix.scan * 8;
  for (int y = w.y0; y < w.y0 + w.mh; ++y)
    for (int gx = gx0; gx <= gx1 + 1; ++gx) {
      ix.entry((long long)y * ix.gpr + gx, e);
      const long long at = (long long)e[0] * 8 + e[1];
      if (e[1] > 7 || (long long)e[0] > nbytes || at < before) return FV_JPEG_E_INDEX_ENTRY;
      before = at;
    }
  ix.entry((long long)w.y0 * ix.gpr + gx0, e);
  const long long first = e[0];
  ix.entry((long long)(w.y0 + w.mh - 1) * ix.gpr + gx1 + 1, e);
  // the byte the next group starts in belongs to this one up to its bit; a 0xFF there is read with its stuffed 0x00
  const long long end = (long long)e[0] + 2 < nbytes ? (long long)e[0] + 2 : nbytes;
  const long long len = end - first, len16 = (len + 15) / 16 * 16;
  const long long base = (*pool_used + 15) / 16 * 16, tbytes = 4ll * IDX_TABLE_WORDS;
  if (len < 0 || base + tbytes + 16 * lanes + len16 > pool_capacity_bytes) return FV_JPEG_E_CAPACITY;
  uint8_t* o = (uint8_t*)pool + base;
  memcpy(o, ix.p + 4 * IDX_HEAD_WORDS, (size_t)tbytes);
  for (int y = 0; y < w.mh; ++y)
    memcpy(o + tbytes + 16ll * y * gw, ix.p + IDX_ENTRIES + 16 * ((long long)(w.y0 + y) * ix.gpr + gx0), 16 * (size_t)gw);
  memcpy(o + tbytes + 16 * lanes, d + first, (size_t)len);
  memset(o + tbytes + 16 * lanes + len, 0, (size_t)(len16 - len));
  *pool_used = base + tbytes + 16 * lanes + len16;

  memset(record, 0, sizeof(int) * FV_JPEG_REC_INTS);
  record[0] = 1;
  record[1] = ix.H; record[2] = ix.W; record[3] = ix.ncomp; record[4] = ix.cls;
  record[5] = w.x0; record[6] = w.y0; record[7] = w.mw; record[8] = w.mh;
  memset(stream_record, 0, sizeof(int) * FV_JPEG_STREAM_REC_INTS);
  for (int c = 0; c < ix.ncomp; ++c) {
    put_i64(record, 9 + 2 * c, coef_base + w.first[c] * 64);
    put_i64(stream_record, 10 + 2 * c, coef_base + w.first[c] * 64);
  }
  put_i64(record, 15, w.blocks * 64);
  record[17] = (int)w.blocks;
  record[18] = (int)((long long)(w.y0 + w.mh - 1) * ix.mcus_x + w.x0 + w.mw);
  memcpy(record + 32, ix.p + 4 * 32, sizeof(int) * 192);
  stream_record[0] = 1;
  stream_record[1] = ix.cls;
  stream_record[2] = w.x0; stream_record[3] = w.y0; stream_record[4] = w.mw; stream_record[5] = w.mh;
  stream_record[6] = ix.mcus_x;
  stream_record[7] = ix.S;
  stream_record[8] = gx0; stream_record[9] = gw;
  put_i64(stream_record, 16, base);
  put_i64(stream_record, 18, base + tbytes);
  put_i64(stream_record, 20, base + tbytes + 16 * lanes);
  stream_record[22] = (int)len;
  stream_record[23] = (int)first;
  return FV_OK;
}

// --------------------------------------------------------------------------------------- ENTRIES MADE ON THE DEVICE
// include/fastvim_hip.h at ENTRIES MADE ON THE DEVICE.  The host parses markers and copies; the entries are found by the
// passes of jpeg_sync_core.h -- on the device by fv_jpeg_sync (jpeg_sync.hip), here serially by fv_jpeg_sync_host.
static_assert(FV_JPEG_SYNC_JOB_INTS == fvsync::JOB_INTS && FV_JPEG_ST_SYNC_JOB == fvsync::ST_JOB && FV_JPEG_ST_SYNC_LOST == fvsync::ST_LOST &&
              FV_JPEG_SYNC_REC_BYTES == 4 * fvsync::REC_WORDS && FV_JPEG_SYNC_MAX_SUBSEQS == fvsync::MAX_SUBSEQS,
              "the sync core and the header agree");

extern "C" int fv_jpeg_sync_stage(const void* data, long long nbytes, const int* window, int segment_mcus, int subseq_bytes,
                                  long long max_scan_bytes, void* pool, long long pool_capacity_bytes, long long* pool_used,
                                  long long scratch_capacity_records, long long* scratch_used, long long coef_base, int* record,
                                  int* stream_record, int* job) {
  if (!data || !window || !pool || !pool_used || !scratch_used || !record || !stream_record || !job || nbytes < 0 ||
      pool_capacity_bytes < 0 || *pool_used < 0 || scratch_capacity_records < 0 || *scratch_used < 0 || coef_base < 0 ||
      (coef_base & 7) || ((uintptr_t)pool & 15) || segment_mcus < 1 || segment_mcus > IDX_MAX_S || subseq_bytes < fvsync::MIN_SUBSEQ ||
      subseq_bytes > fvsync::MAX_SUBSEQ || (subseq_bytes & (subseq_bytes - 1)) || max_scan_bytes < 0)
    return FV_ERR_INVALID;
  Frame f;
  const uint8_t* d = (const uint8_t*)data;
  parse(d, nbytes, f);
  const int reason = indexed_reason(f);
  if (reason != FV_JPEG_R_OK) {
    job[0] = 0;
    job[1] = reason;
    return FV_JPEG_E_UNSERVED;
  }
  if (nbytes > 0x7fffffff) return FV_JPEG_E_CAPACITY;
  Window w;
  int rc = window_of(f, window, w);
  if (rc != FV_OK) return rc;
  // the scan ends in front of the first 0xFF that no 0x00 follows.  Fill bytes in front of a stuffed 0x00 or a restart
  // marker continue it in a way the device reader does not follow: the index builder gives such a file up as well
  long long end = f.scan;
  while (end < nbytes && !(d[end] == 0xFF && (end + 1 >= nbytes || d[end + 1] != 0))) end += d[end] == 0xFF ? 2 : 1;
  if (end > nbytes) end = nbytes;
  if (end < nbytes) {
    long long p = end;
    while (p + 1 < nbytes && d[p + 1] == 0xFF) ++p;
    if (p > end && p + 1 < nbytes && (d[p + 1] == 0 || (d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7))) return FV_JPEG_E_TRUNCATED;
  }
  const long long len = end - f.scan;
  if (len < 1) return FV_JPEG_E_TRUNCATED;
  const long long cap = max_scan_bytes < fvsync::MAX_SCAN ? max_scan_bytes : fvsync::MAX_SCAN;
  if (len > cap || (len + subseq_bytes - 1) / subseq_bytes > fvsync::MAX_SUBSEQS) return FV_JPEG_E_SCAN_SIZE;
  const int S = segment_mcus, L = subseq_bytes;
  const int gx0 = w.x0 / S, gx1 = (w.x0 + w.mw - 1) / S, gw = gx1 - gx0 + 1;
  const long long lanes = (long long)gw * w.mh, len16 = (len + 15) / 16 * 16, nsub = (len + L - 1) / L;
  const long long base = (*pool_used + 15) / 16 * 16, tbytes = 4ll * IDX_TABLE_WORDS;
  if (base + tbytes + 16 * lanes + len16 > pool_capacity_bytes || *scratch_used + nsub > scratch_capacity_records) return FV_JPEG_E_CAPACITY;
  uint8_t* o = (uint8_t*)pool + base;
  pack_tables(f, (uint32_t*)o);
  memset(o + tbytes, 0xFF, (size_t)(16 * lanes));      // an entry nobody wrote: bit > 7, fv_jpeg_huff's lane gives ST_RECORD
  memcpy(o + tbytes + 16 * lanes, d + f.scan, (size_t)len);
  memset(o + tbytes + 16 * lanes + len, 0, (size_t)(len16 - len));
  const long long roff = *scratch_used;
  *pool_used = base + tbytes + 16 * lanes + len16;
  *scratch_used = roff + nsub;

  const long long mcus = (long long)(w.y0 + w.mh - 1) * f.mcus_x + w.x0 + w.mw;
  common_record(f, w, mcus, 1, record);
  memset(stream_record, 0, sizeof(int) * FV_JPEG_STREAM_REC_INTS);
  for (int c = 0; c < f.ncomp; ++c) {
    put_i64(record, 9 + 2 * c, coef_base + w.first[c] * 64);
    put_i64(stream_record, 10 + 2 * c, coef_base + w.first[c] * 64);
  }
  put_i64(record, 15, w.blocks * 64);
  stream_record[0] = 1;
  stream_record[1] = f.cls;
  stream_record[2] = w.x0; stream_record[3] = w.y0; stream_record[4] = w.mw; stream_record[5] = w.mh;
  stream_record[6] = f.mcus_x;
  stream_record[7] = S;
  stream_record[8] = gx0; stream_record[9] = gw;
  put_i64(stream_record, 16, base);
  put_i64(stream_record, 18, base + tbytes);
  put_i64(stream_record, 20, base + tbytes + 16 * lanes);
  stream_record[22] = (int)len;
  stream_record[23] = (int)f.scan;
  memset(job, 0, sizeof(int) * FV_JPEG_SYNC_JOB_INTS);
  job[0] = 1;
  job[1] = f.cls;
  job[2] = w.x0; job[3] = w.y0; job[4] = w.mw; job[5] = w.mh;
  job[6] = f.mcus_x;
  job[7] = S;
  job[8] = gx0; job[9] = gw;
  put_i64(job, 10, base + tbytes + 16 * lanes);
  job[12] = (int)len;
  job[13] = (int)f.scan;
  job[14] = 0;
  job[15] = L;
  job[16] = (int)nsub;
  put_i64(job, 17, base + tbytes);
  put_i64(job, 19, base);
  put_i64(job, 21, roff);
  job[23] = f.mcus_y;
  return FV_OK;
}

extern "C" int fv_jpeg_sync_host(void* pool, long long pool_bytes, int* job, void* scratch, long long scratch_records) {
  if (!pool || !job || !scratch || pool_bytes < 0 || scratch_records < 0 || ((uintptr_t)pool & 15) || ((uintptr_t)scratch & 3))
    return FV_ERR_INVALID;
  if (job[0] != 1) return FV_OK;
  fvsync::Job J;
  if (!fvsync::open_job(job, pool_bytes, scratch_records, J)) {
    job[fvsync::JOB_STATUS] = fvsync::ST_JOB;
    return FV_OK;
  }
  uint8_t* p = (uint8_t*)pool;
  const uint8_t* d = p + J.soff;
  const uint32_t* tables = (const uint32_t*)(p + J.toff);
  uint32_t* recs = (uint32_t*)scratch + J.roff * fvsync::REC_WORDS;
  for (uint32_t i = 0; i < J.nsub; ++i) fvsync::pass_speculate(J, d, tables, recs, i);
  // what speculation was worth (words [26..28], this function only): the speculative exit states are kept for that
  uint32_t* spec = (uint32_t*)malloc(sizeof(uint32_t) * 2 * (size_t)J.nsub);
  for (uint32_t i = 0; spec && i < J.nsub; ++i) memcpy(spec + 2 * i, recs + (size_t)i * fvsync::REC_WORDS, 8);
  int rounds = 0;
  for (uint32_t r = 0; r < J.nsub; ++r) {
    bool any = false;
    for (uint32_t i = 0; i < J.nsub; ++i) any |= fvsync::round_take(recs, i);
    if (!any) break;
    for (uint32_t i = 0; i < J.nsub; ++i) fvsync::round_decode(J, d, tables, recs, i);
    ++rounds;
  }
  if (spec) {
    int dead = 0, wrong = 0, run = 0, longest = 0;
    for (uint32_t i = 0; i + 1 < J.nsub; ++i) {                   // the last exit state lies behind the last MCU
      const uint32_t* rec = recs + (size_t)i * fvsync::REC_WORDS;
      const bool inv = spec[2 * i] == fvsync::INVALID && rec[0] != fvsync::INVALID;
      dead += inv;
      wrong += !inv && (spec[2 * i] != rec[0] || spec[2 * i + 1] != rec[1]);
      run = inv ? run + 1 : 0;
      longest = run > longest ? run : longest;
    }
    job[26] = dead; job[27] = wrong; job[28] = longest;
    free(spec);
  }
  // the scan: counts and sums become the first MCU start and the predictors at each subsequence's entry; the MCU starts
  // that count are those in front of the first INVALID exit state
  fvsync::Prefix valid{0u, 0u};
  uint32_t first = 0, dc[3] = {0, 0, 0};
  for (uint32_t i = 0; i < J.nsub; ++i) {
    uint32_t* rec = recs + (size_t)i * fvsync::REC_WORDS;
    const uint32_t n = rec[4], s01 = rec[5], s2 = rec[6];
    valid = fvsync::join(valid, fvsync::prefix_of(rec));
    rec[4] = first;
    rec[5] = (dc[0] & 0xffffu) | (dc[1] & 0xffffu) << 16;
    rec[6] = dc[2] & 0xffffu;
    first += n;
    dc[0] += s01 & 0xffffu; dc[1] += s01 >> 16; dc[2] += s2 & 0xffffu;
  }
  job[fvsync::JOB_ROUNDS] = rounds;
  if ((long long)valid.n <= fvsync::last_needed(J)) {
    job[fvsync::JOB_STATUS] = fvsync::ST_LOST;
    return FV_OK;
  }
  for (uint32_t i = 0; i < J.nsub; ++i)
    fvsync::pass_emit(J, d, tables, recs, i, i + 1 < J.nsub ? recs[(size_t)(i + 1) * fvsync::REC_WORDS + 4] : first, p);
  job[fvsync::JOB_STATUS] = 0;
  return FV_OK;
}
