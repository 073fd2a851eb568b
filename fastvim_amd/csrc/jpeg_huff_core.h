// The Huffman decode core of the INDEXED JPEG path (include/fastvim_hip.h at THE INDEX): bit reader, symbol lookup, extend
// and the block loop, as functions that hipcc compiles for host and device and the host compiler compiles as they stand
// (the qualifier macro is empty there).  jpeg.hip runs decode_group once per lane; jpeg_host.cpp builds the index with it;
// tools/jpeg_index_check.cpp runs it under the address and undefined-behaviour sanitizers.
//
// Nothing here trusts the stream or the tables.  Every loop has a bound that does not depend on them: 8 bytes per fill,
// 16 - LOOK steps per code-length walk, 63 AC iterations per block, 6 blocks per MCU, `count` MCUs per group.  Every read
// of the stream is checked against [d, d + n) -- beyond it, and from a marker on, the reader delivers zero bits -- every
// table word lies inside TABLE_WORDS, and every coefficient store is checked against `coef_elems`.  A bad code or a run
// past 63 ends the group with a status; what was written up to there stays.
#ifndef FASTVIM_JPEG_HUFF_CORE_H
#define FASTVIM_JPEG_HUFF_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define FVH_FN __host__ __device__ inline
#else
#define FVH_FN inline
#endif

namespace fvhuff {

constexpr int LOOK = 9;
// One Huffman table as the device reads it, 32-bit words:
//   [0, 256)    look: 512 uint16, index = the next LOOK bits; length << 8 | symbol of a code of at most LOOK bits, 0: longer
//   [256, 274)  maxcode[0..17]: the largest code of each length, -1: none
//   [274, 291)  valoff[0..16]: index of the first symbol of each length minus its first code
//   [291]       the number of symbols
//   [292, 356)  the symbols, 256 bytes
constexpr int T_MAXCODE = 256, T_VALOFF = 274, T_NVALS = 291, T_VALS = 292, TABLE_WORDS = 356;
constexpr int TABLES = 4;      // DC of component 0, DC of the chroma components, AC of component 0, AC of chroma

constexpr int ST_OK = 0, ST_CODE = 1, ST_RUN = 2, ST_CAPACITY = 3, ST_RECORD = 4;      // the status of a group

struct Reader {
  const uint8_t* d;
  uint32_t n, pos;       // bytes of the range, the next one to load
  uint64_t buf;
  int bits;              // bits in buf, zero padding included
  uint32_t loaded;       // bytes shifted into buf since the start, padding included
  int pad;               // of them, padding bytes: those loaded last
  bool stopped;          // at a marker or at the end of the range
};

// at most 8 bytes; afterwards bits > 56
FVH_FN void fill(Reader& r) {
  for (int i = 0; i < 8 && r.bits <= 56; ++i) {
    uint32_t b = 0;
    if (!r.stopped) {
      if (r.pos >= r.n) {
        r.stopped = true;
      } else {
        b = r.d[r.pos];
        if (b == 0xFF) {
          // a data 0xFF is followed by a stuffed 0x00; anything else there is a marker (or the end of the range)
          if (r.pos + 1 < r.n && r.d[r.pos + 1] == 0) {
            r.pos += 2;
          } else {
            r.stopped = true;
            b = 0;
          }
        } else {
          ++r.pos;
        }
      }
    }
    r.buf = (r.buf << 8) | (uint64_t)b;
    r.bits += 8;
    ++r.loaded;
    if (r.stopped) ++r.pad;
  }
}

FVH_FN void start(Reader& r, const uint8_t* d, uint32_t n, uint32_t byte, int bit) {
  r.d = d; r.n = n; r.pos = byte < n ? byte : n;
  r.buf = 0; r.bits = 0; r.loaded = 0; r.pad = 0; r.stopped = false;
  fill(r);
  r.bits -= bit & 7;
}

FVH_FN uint32_t peek(const Reader& r, int k) { return (uint32_t)(r.buf >> (r.bits - k)) & ((1u << k) - 1u); }
FVH_FN uint32_t consumed(const Reader& r) { return 8u * r.loaded - (uint32_t)r.bits; }      // bits, from the first byte's bit 0
FVH_FN bool past_end(const Reader& r) { return r.bits < 8 * r.pad; }                        // padding was consumed

FVH_FN int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one symbol; -1: no such code.  Needs 16 bits in the buffer.
FVH_FN int symbol(Reader& r, const uint32_t* t) {
  const uint32_t e = reinterpret_cast<const uint16_t*>(t)[peek(r, LOOK)];
  if (e) {
    const int len = (int)(e >> 8);
    if (len > LOOK) return -1;
    r.bits -= len;
    return (int)(e & 255u);
  }
  const int32_t* maxcode = reinterpret_cast<const int32_t*>(t) + T_MAXCODE;
  int len = 0;
  int32_t code = 0;
  for (int l = LOOK + 1; l <= 16; ++l) {
    code = (int32_t)peek(r, l);
    if (code <= maxcode[l]) { len = l; break; }
  }
  if (!len) return -1;
  const int idx = reinterpret_cast<const int32_t*>(t)[T_VALOFF + len] + code;
  int nvals = (int)t[T_NVALS];
  if (nvals > 256) nvals = 256;
  if (idx < 0 || idx >= nvals) return -1;
  r.bits -= len;
  return reinterpret_cast<const uint8_t*>(t + T_VALS)[idx];
}

FVH_FN int zigzag(int k) {
  constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// One block: the DC difference onto `pred`, then the AC terms.  With `blk` (128 bytes, 16-byte aligned, or null) all 64
// coefficients are written, natural order: zeros first, then every coded term at its place.
FVH_FN int decode_block(Reader& r, const uint32_t* dc, const uint32_t* ac, int& pred, int16_t* blk) {
  if (blk) __builtin_memset(__builtin_assume_aligned(blk, 16), 0, 128);
  if (r.bits < 32) fill(r);
  int s = symbol(r, dc);
  if (s < 0 || s > 15) return ST_CODE;
  if (s) {
    const int v = (int)peek(r, s);
    r.bits -= s;
    pred = (int16_t)(pred + extend(v, s));
  }
  if (blk) blk[0] = (int16_t)pred;
  int k = 1;
  for (int it = 0; it < 63 && k < 64; ++it) {
    if (r.bits < 32) fill(r);
    const int rs = symbol(r, ac);
    if (rs < 0) return ST_CODE;
    const int run = rs >> 4;
    s = rs & 15;
    if (s) {
      k += run;
      if (k > 63) return ST_RUN;
      const int v = (int)peek(r, s);
      r.bits -= s;
      if (blk) blk[zigzag(k)] = (int16_t)extend(v, s);
      ++k;
    } else if (run == 15) {
      k += 16;
      if (k > 64) return ST_RUN;
    } else {
      break;
    }
  }
  return ST_OK;
}

// What a group's blocks are placed by: the sampling class, the MCU window and where each component's coefficients start
// (int16 elements, multiples of 8) -- the layout fv_jpeg_entropy_decode writes.
struct Place {
  int cls, x0, y0, mw, mh;
  long long off[3];
};

// `count` MCUs of MCU row `my` from MCU column `mx` on, read from bit `bit` of d[byte]; the DC predictors go in and come
// out.  Blocks inside the window go to coef[0 : coef_elems], the others are decoded and dropped.  `tables`: TABLES tables.
// With `end`, the reader is left there for the caller (the index builder reads its position).
FVH_FN int decode_group(const uint8_t* d, uint32_t n, uint32_t byte, int bit, int& pred0, int& pred1, int& pred2,
                        const uint32_t* tables, const Place& p, int my, int mx, int count, int16_t* coef,
                        long long coef_elems, Reader* end = nullptr) {
  Reader r;
  start(r, d, n, byte, bit);
  const int gray = p.cls == 3;
  const int hmax = (p.cls == 1 || p.cls == 2) ? 2 : 1, vmax = p.cls == 2 ? 2 : 1;
  const bool row_in = my >= p.y0 && my < p.y0 + p.mh;
  const int nl = hmax * vmax, nb = gray ? 1 : nl + 2;            // blocks of an MCU: luma first, then one per chroma component
  int status = ST_OK;
  for (int m = 0; m < count && status == ST_OK; ++m, ++mx) {
    const bool inside = row_in && mx >= p.x0 && mx < p.x0 + p.mw;
    for (int b = 0; b < 6 && b < nb && status == ST_OK; ++b) {
      const int c = b < nl ? 0 : b - nl + 1;
      int16_t* blk = nullptr;
      if (inside) {
        long long e;
        if (c == 0) {
          const int by = hmax == 2 ? b >> 1 : b, bx = hmax == 2 ? b & 1 : 0;
          e = p.off[0] + (((long long)(my - p.y0) * vmax + by) * ((long long)p.mw * hmax) + (long long)(mx - p.x0) * hmax + bx) * 64;
        } else {
          e = (c == 1 ? p.off[1] : p.off[2]) + ((long long)(my - p.y0) * p.mw + (mx - p.x0)) * 64;
        }
        if (e < 0 || (e & 7) || e > coef_elems - 64) { status = ST_CAPACITY; break; }
        blk = coef + e;
      }
      int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
      const int t = c ? 1 : 0;
      status = decode_block(r, tables + t * TABLE_WORDS, tables + (2 + t) * TABLE_WORDS, pred, blk);
      if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
    }
  }
  if (end) *end = r;
  return status;
}

constexpr int MAX_MCUS = 8192, MAX_S = 65536;      // MCUs per axis (65535 / 8 rounded up), MCUs per group
constexpr int SREC_INTS = 32, SREC_STATUS = 24;    // the stream record (include/fastvim_hip.h)

FVH_FN long long rec64(const int* r, int i) {
  return (long long)(((unsigned long long)(unsigned)r[i + 1] << 32) | (unsigned long long)(unsigned)r[i]);
}

// What one lane does: group `lane` of the indexed sample whose stream record is `r`, out of the stream pool
// pool[0 : pool_bytes) (16-byte aligned) into coef[0 : coef_elems).  Nothing of the record, the entry or the tables is
// trusted: whatever does not fit is ST_RECORD without an access.
FVH_FN int run_lane(const uint8_t* pool, long long pool_bytes, const int* r, long long lane, int16_t* coef, long long coef_elems) {
  Place p;
  p.cls = r[1]; p.x0 = r[2]; p.y0 = r[3]; p.mw = r[4]; p.mh = r[5];
  const int mcus_x = r[6], S = r[7], gx0 = r[8], gw = r[9];
  const long long toff = rec64(r, 16), eoff = rec64(r, 18), soff = rec64(r, 20);
  const int len = r[22], file0 = r[23];
  bool ok = r[0] == 1 && p.cls >= 0 && p.cls <= 3 && p.x0 >= 0 && p.y0 >= 0 && p.mw >= 1 && p.mh >= 1 && mcus_x >= 1 &&
            mcus_x <= MAX_MCUS && p.x0 <= mcus_x - p.mw && p.y0 <= MAX_MCUS - p.mh && S >= 1 && S <= MAX_S && gx0 >= 0 && gw >= 1 &&
            gw <= MAX_MCUS && gx0 <= MAX_MCUS - gw && lane >= 0 && lane < (long long)gw * p.mh;
  ok = ok && toff >= 0 && (toff & 15) == 0 && toff <= pool_bytes - 4ll * TABLES * TABLE_WORDS;
  ok = ok && eoff >= 0 && (eoff & 15) == 0 && eoff <= pool_bytes - 16 * (lane + 1);
  ok = ok && soff >= 0 && len >= 0 && file0 >= 0 && soff <= pool_bytes - len;
  if (!ok) return ST_RECORD;
  p.off[0] = rec64(r, 10); p.off[1] = rec64(r, 12); p.off[2] = rec64(r, 14);
  const int row = (int)(lane / gw), gx = gx0 + (int)(lane - (long long)row * gw);
  const long long mx = (long long)gx * S;                       // at most 8192 * 65536
  const uint32_t* e = reinterpret_cast<const uint32_t*>(pool + eoff + 16 * lane);
  const uint32_t e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
  const long long at = (long long)e0 - file0;
  if (mx >= mcus_x || at < 0 || at > len || e1 > 7u) return ST_RECORD;
  const int count = mcus_x - (int)mx < S ? mcus_x - (int)mx : S;
  int pred0 = (int16_t)(e2 & 0xffffu), pred1 = (int16_t)(e2 >> 16), pred2 = (int16_t)(e3 & 0xffffu);
  return decode_group(pool + soff, (uint32_t)len, (uint32_t)at, (int)e1, pred0, pred1, pred2,
                      reinterpret_cast<const uint32_t*>(pool + toff), p, p.y0 + row, (int)mx, count, coef, coef_elems);
}

}  // namespace fvhuff
#endif
