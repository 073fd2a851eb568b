// hipcc-flags: -fwrapv
// The device half of the JPEG decode (include/fastvim_hip.h at fv_jpeg_probe): the host's entropy decoder
// (jpeg_host.cpp) leaves quantised coefficients and one record per sample; two launches turn them into the RGB bytes
// libjpeg-turbo would have written, in the pixel pool fv_resample_u8 reads.  All arithmetic is integer and exact; signed
// overflow wraps (-fwrapv), which only coefficient values no encoder writes can reach.
//
//   jpeg_idct_kernel  8 lanes per 8 x 8 block, 32 blocks per workgroup pass.  Lane r loads coefficient row r (one 16-byte
//                     load) and its table row, multiplies, and the block goes through LDS twice: columns are read for
//                     pass 1 and written back, rows are read for pass 2 (row stride 9 words: the column reads of the four
//                     blocks of a 32-lane half fall on 32 distinct banks).  Lane r stores pixel row r as one 8-byte
//                     store.  A block whose AC terms are all zero -- most blocks of a photograph -- skips LDS and both
//                     passes: pass 1 gives 4 dc exactly, pass 2 (dc + 4) >> 3.
//                     Two forms of the coefficients, one kernel body (PACKED): the dense form above, and the packed form
//                     -- a 16-byte header per block (64-bit mask of the non-zero AC terms, value offset, `wide`, DC) and
//                     the non-zero values as int8 or int16.  Lane r owns mask byte r: its values start at number
//                     popcount(mask below bit 8 r) of the block; it loads the aligned words around them without a
//                     branch and shifts the values out; DC-only is mask == 0.
//   jpeg_rgb_kernel   a thread per QUAD of four consecutive pixels of a crop (12 bytes: three aligned 4-byte stores).
// Both split the table's prefix sums into one contiguous share per workgroup: the grid depends on capacities only, so a
// captured launch serves whatever batch the table describes when it runs.
//
//   jpeg_huff_kernel  the indexed path (include/fastvim_hip.h at THE INDEX), in front of jpeg_idct_kernel: a LANE per group
//                     of S MCUs, decoded from its index entry by jpeg_huff_core.h.  Serial, divergent work with dependent
//                     byte loads: one-wave workgroups spread the lanes over as many SIMDs as the batch has waves, and
//                     neighbouring lanes decode neighbouring groups of one MCU row -- the nearest thing to equal work.
//                     The Huffman tables are read from the stream pool through the caches.
#include "common.h"
#include "jpeg_huff_core.h"

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_BLOCKS = JP_THREADS / 8;      // 8 x 8 blocks per workgroup pass
constexpr int JP_ROW = 9;                      // LDS row stride of a block, words
constexpr int REC = FV_JPEG_REC_INTS;
constexpr int JP_MAX_MCUS = 8192;              // per axis: 65535 / 8 rounded up

__device__ __forceinline__ long long rec_i64(const int* r, int i) {
  return (long long)(((unsigned long long)(unsigned)r[i + 1] << 32) | (unsigned long long)(unsigned)r[i]);
}

// largest s in [0, batch - 1] with pre[s] <= g
__device__ __forceinline__ int find_sample(const int* pre, int batch, long long g) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)pre[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct Geo {
  int ncomp, cls, hmax, vmax, x0, y0, mw, mh;
  long long off[3];
  int nblk[3];
};

constexpr int KIND_DENSE = 1 << 1, KIND_PACKED = 1 << 2;      // record[0] as a bit

// the record's geometry; false: not a JPEG job of one of `kinds` or not a record the decoder writes
__device__ __forceinline__ bool geometry(const int* r, int kinds, long long cap, Geo& g) {
  g.ncomp = r[3]; g.cls = r[4];
  g.x0 = r[5]; g.y0 = r[6]; g.mw = r[7]; g.mh = r[8];
  if (r[0] < 1 || r[0] > 2 || !((kinds >> r[0]) & 1) || g.cls < 0 || g.cls > 3 || g.ncomp != (g.cls == FV_JPEG_GRAY ? 1 : 3)) return false;
  if (g.x0 < 0 || g.y0 < 0 || g.mw < 1 || g.mh < 1 || g.x0 > JP_MAX_MCUS - g.mw || g.y0 > JP_MAX_MCUS - g.mh) return false;
  g.hmax = (g.cls == FV_JPEG_422 || g.cls == FV_JPEG_420) ? 2 : 1;
  g.vmax = g.cls == FV_JPEG_420 ? 2 : 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g.nblk[c] = c == 0 ? g.mw * g.hmax * g.mh * g.vmax : c < g.ncomp ? g.mw * g.mh : 0;
    g.off[c] = c < g.ncomp ? rec_i64(r, 9 + 2 * c) : 0;
    if (g.off[c] < 0 || (g.off[c] & 7) || g.off[c] > cap - (long long)g.nblk[c] * 64) return false;
  }
  return true;
}

// one pass of jidctint's islow butterfly over eight values
__device__ __forceinline__ void idct8(const int (&in)[8], int (&o)[8], int shift) {
  int z1 = (in[2] + in[6]) * 4433;
  const int tmp2 = z1 - in[6] * 15137;
  const int tmp3 = z1 + in[2] * 6270;
  const int tmp0 = (in[0] + in[4]) << 13;
  const int tmp1 = (in[0] - in[4]) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const int r = 1 << (shift - 1);
  o[0] = (tmp10 + t3 + r) >> shift; o[7] = (tmp10 - t3 + r) >> shift;
  o[1] = (tmp11 + t2 + r) >> shift; o[6] = (tmp11 - t2 + r) >> shift;
  o[2] = (tmp12 + t1 + r) >> shift; o[5] = (tmp12 - t1 + r) >> shift;
  o[3] = (tmp13 + t0 + r) >> shift; o[4] = (tmp13 - t0 + r) >> shift;
}

__device__ __forceinline__ unsigned clamp8(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }

// `src_cap` counts int16 elements of the dense form, bytes of the packed one
template <bool PACKED>
__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const void* __restrict__ src, long long src_cap,
                                                                const int* __restrict__ table, uint8_t* __restrict__ planes,
                                                                long long plane_bytes, int batch) {
  __shared__ int lds[JP_BLOCKS][8 * JP_ROW];
  const int* pre = table + (long long)batch * REC;
  const long long total = pre[batch];
  const int slot = threadIdx.x >> 3, l8 = threadIdx.x & 7;
  const long long cap = PACKED ? plane_bytes : src_cap < plane_bytes ? src_cap : plane_bytes;
  // a workgroup takes one CONTIGUOUS share of the blocks: its sample is searched once and then walked, a step at most
  // every few passes (uniform in the workgroup)
  const long long share = ((total + gridDim.x - 1) / gridDim.x + JP_BLOCKS - 1) / JP_BLOCKS * JP_BLOCKS;
  const long long first = (long long)blockIdx.x * share, last = first + share < total ? first + share : total;
  int s0 = first < last ? find_sample(pre, batch, first) : 0;
  for (long long base = first; base < last; base += JP_BLOCKS) {
    while (s0 < batch - 1 && (long long)pre[s0 + 1] <= base) ++s0;
    const long long gb = base + slot;
    bool valid = gb < last;
    int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long mask = 0;                   // PACKED: the block's non-zero AC terms
    long long dst = 0;       // byte offset of this lane's pixel row in the plane workspace
    if (valid) {
      int s = s0;
      while (s < batch - 1 && (long long)pre[s + 1] <= gb) ++s;
      const int* r = table + (long long)s * REC;
      Geo g;
      long long lb = gb - pre[s];
      const long long ls = lb;                     // the block's number in the sample
      valid = geometry(r, PACKED ? KIND_PACKED : KIND_DENSE, cap, g) && lb >= 0;
      int c = 0;             // the block's component; no runtime index into g.nblk / g.off (they stay in registers)
      if (valid && lb >= g.nblk[0]) {
        lb -= g.nblk[0];
        c = 1;
        if (lb >= g.nblk[1]) {
          lb -= g.nblk[1];
          c = lb >= g.nblk[2] ? 3 : 2;
        }
      }
      valid = valid && c < g.ncomp;
      if (valid) {
        const long long off = c == 0 ? g.off[0] : c == 1 ? g.off[1] : g.off[2];
        const int bw = g.mw * (c == 0 ? g.hmax : 1);
        const int brow = (int)lb / bw, bcol = (int)lb % bw;
        const int4 q0 = *reinterpret_cast<const int4*>(r + 32 + 64 * c + l8 * 8);
        const int4 q1 = *reinterpret_cast<const int4*>(r + 36 + 64 * c + l8 * 8);
        if constexpr (PACKED) {
          // header and values, every byte of them inside [0, src_cap); a block that does not fit is skipped
          const uint8_t* pool = static_cast<const uint8_t*>(src);
          const long long hb = rec_i64(r, 25), vb = rec_i64(r, 27);
          valid = hb >= 0 && (hb & 15) == 0 && vb >= 0 && (vb & 1) == 0 && vb <= src_cap && hb <= src_cap - 16 * (ls + 1);
          if (valid) {
            const uint4 h = *reinterpret_cast<const uint4*>(pool + hb + 16 * ls);
            const unsigned long long m = ((unsigned long long)h.y << 32 | h.x) & ~1ull;
            const int wide = (int)(h.z >> 31);
            const long long vo = vb + (long long)(h.z & 0x7fffffffu);
            // values are read as whole aligned words: they have to lie inside the pool's whole words
            const long long cap4 = src_cap & ~3ll;
            valid = (h.z & 1u) == 0 && vo <= cap4 - ((long long)__popcll(m) << wide);
            if (valid) {
              mask = m;
              const int q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
              const unsigned m8 = (unsigned)(m >> (8 * l8)) & 0xffu;
              // this lane's values: at most 8 (16 bytes) from byte a on.  Five aligned words cover them at any a; all five
              // are loaded without a branch -- one round trip -- and a word past the pool's last is replaced by the last
              // (cap4 >= 16: the header fitted), which no value of this lane lies in
              const long long a = vo + ((long long)__popcll(m & ((1ull << (8 * l8)) - 1ull)) << wide);
              unsigned d[5];
#pragma unroll
              for (int i = 0; i < 5; ++i) {
                const long long at = (a & ~3ll) + 4 * i;
                d[i] = *reinterpret_cast<const unsigned*>(pool + (at > cap4 - 4 ? cap4 - 4 : at));
              }
              const unsigned sh = 8u * ((unsigned)a & 3u);
              unsigned w[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) w[i] = (unsigned)((((unsigned long long)d[i + 1] << 32) | d[i]) >> sh);
              unsigned long long lo = (unsigned long long)w[1] << 32 | w[0], hi = (unsigned long long)w[3] << 32 | w[2];
              const unsigned step = wide ? 16u : 8u;
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const int v = wide ? (int)(int16_t)(lo & 0xffffu) : (int)(int8_t)(lo & 0xffu);
                if ((m8 >> j) & 1u) {
                  x[j] = v * q[j];
                  lo = (lo >> step) | (hi << (64u - step));
                  hi >>= step;
                }
              }
              if (l8 == 0) x[0] = (int)(int16_t)(h.w & 0xffffu) * q[0];
            }
          }
        } else {
          const int4 cv = *reinterpret_cast<const int4*>(static_cast<const int16_t*>(src) + off + lb * 64 + l8 * 8);
          x[0] = (int)(int16_t)(cv.x & 0xffff) * q0.x; x[1] = (cv.x >> 16) * q0.y;
          x[2] = (int)(int16_t)(cv.y & 0xffff) * q0.z; x[3] = (cv.y >> 16) * q0.w;
          x[4] = (int)(int16_t)(cv.z & 0xffff) * q1.x; x[5] = (cv.z >> 16) * q1.y;
          x[6] = (int)(int16_t)(cv.w & 0xffff) * q1.z; x[7] = (cv.w >> 16) * q1.w;
        }
        dst = off + ((long long)brow * 8 + l8) * ((long long)bw * 8) + (long long)bcol * 8;
      }
    }
    bool dc_only;
    if constexpr (PACKED) {
      dc_only = mask == 0;                        // known from the header; the same for the 8 lanes of a block
    } else {
      const int ac = (l8 == 0 ? 0 : x[0]) | x[1] | x[2] | x[3] | x[4] | x[5] | x[6] | x[7];
      const unsigned long long any_ac = __ballot(valid && ac != 0);
      dc_only = ((any_ac >> ((threadIdx.x & 63) & ~7)) & 0xffull) == 0;
    }
    const int dc = __shfl(x[0], 0, 8);
    const bool full = valid && !dc_only;
    int* blk = lds[slot];
    if (full) {
#pragma unroll
      for (int j = 0; j < 8; ++j) blk[l8 * JP_ROW + j] = x[j];
    }
    __syncthreads();
    if (full) {                                   // pass 1: this lane's COLUMN, in place
      int in[8], o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = blk[k * JP_ROW + l8];
      idct8(in, o, 11);
#pragma unroll
      for (int k = 0; k < 8; ++k) blk[k * JP_ROW + l8] = o[k];
    }
    __syncthreads();
    if (valid) {
      unsigned lo, hi;
      if (dc_only) {
        const unsigned v = clamp8(((dc + 4) >> 3) + 128);
        lo = hi = v * 0x01010101u;
      } else {                                    // pass 2: this lane's ROW
        int in[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = blk[l8 * JP_ROW + j];
        idct8(in, o, 18);
        lo = clamp8(o[0] + 128) | clamp8(o[1] + 128) << 8 | clamp8(o[2] + 128) << 16 | clamp8(o[3] + 128) << 24;
        hi = clamp8(o[4] + 128) | clamp8(o[5] + 128) << 8 | clamp8(o[6] + 128) << 16 | clamp8(o[7] + 128) << 24;
      }
      *reinterpret_cast<uint2*>(planes + dst) = make_uint2(lo, hi);
    }
    __syncthreads();                              // the next pass of the loop writes the tile again
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// jdcolor.c: 16 fraction bits
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }
constexpr int CR_R = fix16(1.402), CB_B = fix16(1.772), CB_G = -fix16(0.34414), CR_G = -fix16(0.71414);

__global__ __launch_bounds__(JP_THREADS) void jpeg_rgb_kernel(const uint8_t* __restrict__ planes, long long plane_bytes,
                                                               const int* __restrict__ table, uint8_t* __restrict__ pool,
                                                               long long pool_bytes, int batch) {
  const int* pre = table + (long long)batch * REC + batch + 1;
  const long long total = pre[batch];
  // a workgroup takes one CONTIGUOUS share of the quads, as the blocks above
  const long long share = ((total + gridDim.x - 1) / gridDim.x + JP_THREADS - 1) / JP_THREADS * JP_THREADS;
  const long long first = (long long)blockIdx.x * share, last = first + share < total ? first + share : total;
  int s0 = first < last ? find_sample(pre, batch, first) : 0;
  for (long long base = first; base < last; base += JP_THREADS) {
    while (s0 < batch - 1 && (long long)pre[s0 + 1] <= base) ++s0;
    const long long gq = base + threadIdx.x;
    if (gq >= last) continue;
    int s = s0;                                                   // a crop is thousands of quads: at most a step or two
    while (s < batch - 1 && (long long)pre[s + 1] <= gq) ++s;
    const int* r = table + (long long)s * REC;
    Geo g;
    if (!geometry(r, KIND_DENSE | KIND_PACKED, plane_bytes, g)) continue;
    const int H = r[1], W = r[2], top = r[19], left = r[20], ch = r[21], cw = r[22];
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || top < 0 || left < 0 || ch < 1 || cw < 1 || top > H - ch || left > W - cw) continue;
    const long long npx = (long long)ch * cw, poff = rec_i64(r, 23);
    const long long q = gq - pre[s];
    if (npx > 0x7fffffffll || q < 0 || q * 4 >= npx || poff < 0 || (poff & 3) || poff > pool_bytes - npx * 3) continue;
    // window-local plane extents and the true plane sizes
    const int lw = g.mw * 8 * g.hmax, lh = g.mh * 8 * g.vmax, kw = g.mw * 8, kh = g.mh * 8;
    const int tw = (W + g.hmax - 1) / g.hmax, th = (H + g.vmax - 1) / g.vmax;
    const uint8_t* py = planes + g.off[0];
    unsigned px[4] = {0, 0, 0, 0};
    const int p0 = (int)(q * 4), n = npx - p0 < 4 ? (int)(npx - p0) : 4;
    int yy = p0 / cw, xx = p0 - yy * cw;
#pragma unroll
    for (int j = 0; j < 4; ++j, ++xx) {                    // unrolled: px[] stays in registers
      if (j >= n) break;
      if (xx == cw) { xx = 0; ++yy; }
      const int Y = top + yy, X = left + xx;
      const int lum = py[(long long)clampi(Y - g.y0 * 8 * g.vmax, 0, lh - 1) * lw + clampi(X - g.x0 * 8 * g.hmax, 0, lw - 1)];
      if (g.cls == FV_JPEG_GRAY) {
        px[j] = (unsigned)lum * 0x010101u;
        continue;
      }
      const int cy = Y / g.vmax, cx = X / g.hmax;
      const int ny = g.vmax == 1 ? cy : (Y & 1) ? cy + 1 : cy - 1, nx = g.hmax == 1 ? cx : (X & 1) ? cx + 1 : cx - 1;
      // rows and columns replicated at the TRUE plane edge, then window-local
      const long long r0 = (long long)clampi(clampi(cy, 0, th - 1) - g.y0 * 8, 0, kh - 1) * kw;
      const long long r1 = (long long)clampi(clampi(ny, 0, th - 1) - g.y0 * 8, 0, kh - 1) * kw;
      const int c0 = clampi(clampi(cx, 0, tw - 1) - g.x0 * 8, 0, kw - 1), c1 = clampi(clampi(nx, 0, tw - 1) - g.x0 * 8, 0, kw - 1);
      int cbcr[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint8_t* pc = planes + g.off[1 + k];
        int v;
        if (g.cls == FV_JPEG_444) {
          v = pc[r0 + c0];
        } else if (g.cls == FV_JPEG_422) {
          v = (3 * pc[r0 + c0] + pc[r0 + c1] + ((X & 1) ? 2 : 1)) >> 2;
        } else {
          const int here = 3 * pc[r0 + c0] + pc[r1 + c0], there = 3 * pc[r0 + c1] + pc[r1 + c1];
          v = (3 * here + there + ((X & 1) ? 7 : 8)) >> 4;
        }
        cbcr[k] = v - 128;
      }
      const int cb = cbcr[0], cr = cbcr[1];
      const unsigned R = clamp8(lum + ((CR_R * cr + 32768) >> 16));
      const unsigned G = clamp8(lum + ((CB_G * cb + 32768 + CR_G * cr) >> 16));
      const unsigned B = clamp8(lum + ((CB_B * cb + 32768) >> 16));
      px[j] = R | G << 8 | B << 16;
    }
    uint8_t* dst = pool + poff + (long long)p0 * 3;
    if (n == 4) {                                  // 12 bytes, 4-byte aligned: poff is, and so is 12 q
      unsigned* d = reinterpret_cast<unsigned*>(dst);
      d[0] = px[0] | px[1] << 24;
      d[1] = px[1] >> 8 | px[2] << 16;
      d[2] = px[2] >> 16 | px[3] << 8;
    } else {
      for (int j = 0; j < n; ++j) {
        dst[3 * j] = (uint8_t)px[j];
        dst[3 * j + 1] = (uint8_t)(px[j] >> 8);
        dst[3 * j + 2] = (uint8_t)(px[j] >> 16);
      }
    }
  }
}

constexpr int HUFF_THREADS = 64;
constexpr int SREC = FV_JPEG_STREAM_REC_INTS;
static_assert(fvhuff::ST_CODE == FV_JPEG_ST_CODE && fvhuff::ST_RUN == FV_JPEG_ST_RUN && fvhuff::ST_CAPACITY == FV_JPEG_ST_CAPACITY &&
              fvhuff::ST_RECORD == FV_JPEG_ST_RECORD && fvhuff::SREC_INTS == SREC && fvhuff::MAX_MCUS == JP_MAX_MCUS,
              "the core and the header agree");

__global__ __launch_bounds__(HUFF_THREADS) void jpeg_huff_kernel(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                                  int* __restrict__ stable, int16_t* __restrict__ coef,
                                                                  long long coef_elems, int batch) {
  const int* pre = stable + (long long)batch * SREC;
  const long long total = pre[batch];
  const long long step = (long long)gridDim.x * HUFF_THREADS;
  for (long long g = (long long)blockIdx.x * HUFF_THREADS + threadIdx.x; g < total; g += step) {
    const int s = find_sample(pre, batch, g);
    int* r = stable + (long long)s * SREC;
    if (r[0] != 1) continue;                                    // the prefix sums give such a record no lane
    const int st = fvhuff::run_lane(pool, pool_bytes, r, g - pre[s], coef, coef_elems);
    if (st != fvhuff::ST_OK) r[fvhuff::SREC_STATUS] = st;       // a plain store; lanes that give up may race for it
  }
}

bool batch_ok(int batch) { return batch >= 1 && batch <= 4096; }

// grid of a launch over at most `units` work items, `per` per workgroup pass: from capacities only
int stride_grid(long long units, int per) {
  long long need = (units + per - 1) / per;
  const long long cap = (long long)fv_cu_count() * 8;
  if (need > cap) need = cap;
  return need < 1 ? 1 : (int)need;
}

}  // namespace

extern "C" long long fv_jpeg_table_ints(int batch) {
  return batch_ok(batch) ? (long long)batch * FV_JPEG_REC_INTS + 2 * ((long long)batch + 1) : 0;
}

extern "C" int fv_jpeg_idct(const void* coef, long long coef_elems, const int* table, void* planes, long long plane_bytes,
                            int batch, fv_stream_t stream) {
  FV_CHECK(coef && table && planes, "jpeg_idct: null pointer");
  FV_CHECK(batch_ok(batch), "jpeg_idct: batch %d outside [1, 4096]", batch);
  FV_CHECK(coef_elems >= 0 && plane_bytes >= 0, "jpeg_idct: negative capacity");
  FV_CHECK(((uintptr_t)coef & 15) == 0 && ((uintptr_t)table & 15) == 0 && ((uintptr_t)planes & 7) == 0,
           "jpeg_idct: misaligned buffer (coefficients and table 16 bytes, planes 8)");
  const long long cap = coef_elems < plane_bytes ? coef_elems : plane_bytes;
  hipLaunchKernelGGL(jpeg_idct_kernel<false>, dim3(stride_grid(cap / 64, JP_BLOCKS)), dim3(JP_THREADS), 0, (hipStream_t)stream,
                     coef, coef_elems, table, (uint8_t*)planes, plane_bytes, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_jpeg_idct_packed(const void* pool, long long pool_bytes, const int* table, void* planes,
                                   long long plane_bytes, int batch, fv_stream_t stream) {
  FV_CHECK(pool && table && planes, "jpeg_idct_packed: null pointer");
  FV_CHECK(batch_ok(batch), "jpeg_idct_packed: batch %d outside [1, 4096]", batch);
  FV_CHECK(pool_bytes >= 0 && plane_bytes >= 0, "jpeg_idct_packed: negative capacity");
  FV_CHECK(((uintptr_t)pool & 15) == 0 && ((uintptr_t)table & 15) == 0 && ((uintptr_t)planes & 7) == 0,
           "jpeg_idct_packed: misaligned buffer (pool and table 16 bytes, planes 8)");
  // a block takes a 16-byte header and 64 plane bytes at the least
  const long long cap = pool_bytes / 16 < plane_bytes / 64 ? pool_bytes / 16 : plane_bytes / 64;
  hipLaunchKernelGGL(jpeg_idct_kernel<true>, dim3(stride_grid(cap, JP_BLOCKS)), dim3(JP_THREADS), 0, (hipStream_t)stream, pool,
                     pool_bytes, table, (uint8_t*)planes, plane_bytes, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_jpeg_rgb(const void* planes, long long plane_bytes, const int* table, void* pool, long long pool_bytes,
                           int batch, fv_stream_t stream) {
  FV_CHECK(planes && table && pool, "jpeg_rgb: null pointer");
  FV_CHECK(batch_ok(batch), "jpeg_rgb: batch %d outside [1, 4096]", batch);
  FV_CHECK(plane_bytes >= 0 && pool_bytes >= 0, "jpeg_rgb: negative capacity");
  FV_CHECK(((uintptr_t)table & 3) == 0 && ((uintptr_t)pool & 3) == 0, "jpeg_rgb: misaligned buffer");
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(stride_grid(pool_bytes / 12 + batch, JP_THREADS)), dim3(JP_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)planes, plane_bytes, table, (uint8_t*)pool, pool_bytes, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" long long fv_jpeg_stream_table_ints(int batch) {
  return batch_ok(batch) ? (long long)batch * FV_JPEG_STREAM_REC_INTS + (long long)batch + 1 : 0;
}

extern "C" int fv_jpeg_huff(const void* stream_pool, long long stream_bytes, int* stream_table, void* coef, long long coef_elems,
                            int batch, fv_stream_t stream) {
  FV_CHECK(stream_pool && stream_table && coef, "jpeg_huff: null pointer");
  FV_CHECK(batch_ok(batch), "jpeg_huff: batch %d outside [1, 4096]", batch);
  FV_CHECK(stream_bytes >= 0 && coef_elems >= 0, "jpeg_huff: negative capacity");
  FV_CHECK(((uintptr_t)stream_pool & 15) == 0 && ((uintptr_t)stream_table & 3) == 0 && ((uintptr_t)coef & 15) == 0,
           "jpeg_huff: misaligned buffer (stream pool and coefficients 16 bytes, table 4)");
  // a lane takes a 16-byte entry at the least; one-wave workgroups, at most 32 per CU
  long long need = (stream_bytes / 16 + HUFF_THREADS - 1) / HUFF_THREADS;
  const long long cap = (long long)fv_cu_count() * 32;
  if (need > cap) need = cap;
  hipLaunchKernelGGL(jpeg_huff_kernel, dim3(need < 1 ? 1 : (int)need), dim3(HUFF_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)stream_pool, stream_bytes, stream_table, (int16_t*)coef, coef_elems, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
