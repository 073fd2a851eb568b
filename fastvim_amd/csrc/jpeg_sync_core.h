// The synchronisation core of the INDEX-FREE JPEG path (include/fastvim_hip.h at ENTRIES MADE ON THE DEVICE): the index
// entries fv_jpeg_huff starts its lanes from, found without a serial pass over the file.  Built on jpeg_huff_core.h --
// its Reader, symbol, extend and table layout -- and, like it, one text for hipcc (host and device) and the host compiler.
// jpeg_sync.hip runs it one workgroup per sample; jpeg_host.cpp runs the same passes serially (fv_jpeg_sync_host);
// tools/jpeg_sync_check.cpp runs that under the address and undefined-behaviour sanitizers.
//
// The scan is cut into SUBSEQUENCES of L bytes of the file (a boundary that falls on a stuffed 0x00 lies one byte later,
// so every data byte belongs to exactly one).  A STATE is a symbol boundary: the position (byte, bit) in the index's own
// convention -- here relative to the first staged byte -- the block b within the MCU and the next zigzag position k (0: a
// DC code comes next), or INVALID.  A symbol is a Huffman code with its value bits.  `walk` decodes the symbols whose
// first bit lies inside one subsequence from an entry state and returns the exit state: the start of the first symbol at
// or behind the subsequence's end.  Decoding every subsequence from (its first bit, b = 0, k = 0) and then again from its
// predecessor's exit state until nothing changes reaches the serial decoder's states: subsequence 0 starts from the
// scan's true start, so after round i subsequence i is right.
//
// Nothing trusts the stream, the tables or the job.  `walk` runs at most 8 * (bytes of the subsequence) + 8 symbols, each
// of which consumes a bit; the cursor moves at most 6 bytes per symbol; every stream read is checked against [d, d + n)
// (the Reader's own and the cursor's); a bad code, a run past 63, consumed padding and an entry state outside the
// subsequence give INVALID, and INVALID in gives INVALID out.
#ifndef FASTVIM_JPEG_SYNC_CORE_H
#define FASTVIM_JPEG_SYNC_CORE_H
#include "jpeg_huff_core.h"

namespace fvsync {

constexpr int JOB_INTS = 32, JOB_STATUS = 24, JOB_ROUNDS = 25;      // the sync job (include/fastvim_hip.h)
constexpr int ST_JOB = 5, ST_LOST = 6;                              // statuses of a sample, behind fvhuff's
constexpr int MIN_SUBSEQ = 16, MAX_SUBSEQ = 1024;                   // a symbol is at most 31 bits: 16 bytes hold a start
constexpr long long MAX_SCAN = 1ll << 26;                           // bytes of a staged scan
// Subsequences of a job.  Every round each lane looks at all of its records, so a sample costs up to nsub rounds of
// nsub / 256 record visits per lane and three barriers: the cap keeps the worst launch short on a shared card.
constexpr int MAX_SUBSEQS = 16384;
constexpr uint32_t INVALID = 0xffffffffu;
// One scratch record per subsequence, 32-bit words:
//   [0] [1]  the exit state            [2] [3]  the entry state it was decoded from
//   [4]      MCU starts inside         -- after the scan: the index of its first MCU start
//   [5] [6]  sums of the DC differences inside, as an entry holds predictors  -- after the scan: the predictors at its entry
//   [7]      1: the entry state changed in this round
constexpr int REC_WORDS = 8;

struct State {
  uint32_t byte, w;      // w: bit | b << 3 | k << 8
};
FVH_FN State make(uint32_t byte, int bit, int b, int k) { return State{byte, (uint32_t)bit | (uint32_t)b << 3 | (uint32_t)k << 8}; }
FVH_FN State invalid() { return State{INVALID, 0u}; }
FVH_FN bool same(State a, State b) { return a.byte == b.byte && a.w == b.w; }

struct Sums {
  uint32_t mcus;
  int dc0, dc1, dc2;      // named, not an array: nothing is indexed at run time and the kernel has no scratch
};

// the first byte of subsequence boundary p: p itself, or p + 1 where d[p] is a stuffed 0x00
FVH_FN uint32_t boundary(const uint8_t* d, uint32_t n, unsigned long long p) {
  if (p >= n) return n;
  uint32_t q = (uint32_t)p;
  if (q > 0 && d[q] == 0 && d[q - 1] == 0xFF) ++q;
  return q;
}

// The symbols that start in [lo, hi) of d[0 : n), from the state `in`; nb blocks per MCU, the first nl of them luma.
// `visit(m, byte, bit, sums)` is called at every MCU start inside: its number within the subsequence, its position and the
// DC sums up to it.  Returns the exit state; `sums` holds what was seen up to there, or up to where the walk gave up.
template <class Visit>
FVH_FN State walk(const uint8_t* d, uint32_t n, uint32_t lo, uint32_t hi, State in, const uint32_t* tables, int nb, int nl,
                  Sums& sums, Visit& visit) {
  sums.mcus = 0;
  sums.dc0 = sums.dc1 = sums.dc2 = 0;
  if (in.byte == INVALID || in.byte < lo || in.byte > n || hi > n || lo > hi) return invalid();
  if (in.byte >= hi) return in;
  int bit = (int)(in.w & 7u), b = (int)((in.w >> 3) & 31u), k = (int)(in.w >> 8);
  if (b >= nb || k > 63 || nb < 1 || nb > 6 || nl < 1 || nl > nb) return invalid();
  fvhuff::Reader r;
  fvhuff::start(r, d, n, in.byte, bit);
  uint32_t cur = in.byte, base = 0;      // the data byte the next bit lies in, and the consumed bits at its bit 0
  const uint32_t steps = 8u * (hi - lo) + 8u;
  for (uint32_t it = 0; it < steps && cur < hi; ++it) {
    if (b == 0 && k == 0) {
      visit(sums.mcus, cur, bit, sums);
      ++sums.mcus;
    }
    if (r.bits < 32) fvhuff::fill(r);
    const int c = b < nl ? 0 : b - nl + 1, t = c ? 1 : 0;
    if (k == 0) {
      const int s = fvhuff::symbol(r, tables + t * fvhuff::TABLE_WORDS);
      if (s < 0 || s > 15) return invalid();
      if (s) {
        const int v = (int)fvhuff::peek(r, s);
        r.bits -= s;
        const int diff = fvhuff::extend(v, s);
        if (c == 0) sums.dc0 = (int16_t)(sums.dc0 + diff);
        else if (c == 1) sums.dc1 = (int16_t)(sums.dc1 + diff);
        else sums.dc2 = (int16_t)(sums.dc2 + diff);
      }
      k = 1;
    } else {
      const int rs = fvhuff::symbol(r, tables + (2 + t) * fvhuff::TABLE_WORDS);
      if (rs < 0) return invalid();
      const int run = rs >> 4, s = rs & 15;
      if (s) {
        k += run;
        if (k > 63) return invalid();
        r.bits -= s;
        ++k;
      } else if (run == 15) {
        k += 16;
        if (k > 64) return invalid();
      } else {
        k = 64;
      }
    }
    if (k >= 64) {
      k = 0;
      if (++b == nb) b = 0;
    }
    if (fvhuff::past_end(r)) return invalid();
    // the cursor moves over whole stuffed bytes, as the index builder's does: it never rests on a stuffed 0x00
    const uint32_t used = fvhuff::consumed(r);
    for (int j = 0; j < 6 && used - base >= 8u; ++j) {
      if (cur >= n) return invalid();
      cur += d[cur] == 0xFF ? 2u : 1u;
      base += 8u;
    }
    if (used - base >= 8u) return invalid();
    bit = (int)(used - base);
  }
  if (cur < hi) return invalid();
  return make(cur > n ? n : cur, bit, b, k);
}

struct NoVisit {
  FVH_FN void operator()(uint32_t, uint32_t, int, const Sums&) const {}
};

// the exit state of a subsequence and what it holds
FVH_FN State decode_subseq(const uint8_t* d, uint32_t n, uint32_t lo, uint32_t hi, State in, const uint32_t* tables, int nb, int nl,
                           Sums& sums) {
  NoVisit v;
  return walk(d, n, lo, hi, in, tables, nb, nl, sums, v);
}

// A sync job as the passes read it; `open_job` takes nothing of it on trust.
struct Job {
  int cls, x0, y0, mw, mh, mcus_x, mcus_y, S, gx0, gw, nb, nl, bit0;
  long long soff, eoff, toff, roff;
  uint32_t len, file0, L, nsub;
};

FVH_FN bool open_job(const int* j, long long pool_bytes, long long scratch_records, Job& o) {
  o.cls = j[1]; o.x0 = j[2]; o.y0 = j[3]; o.mw = j[4]; o.mh = j[5]; o.mcus_x = j[6]; o.S = j[7]; o.gx0 = j[8]; o.gw = j[9];
  o.soff = fvhuff::rec64(j, 10); o.bit0 = j[14]; o.eoff = fvhuff::rec64(j, 17); o.toff = fvhuff::rec64(j, 19);
  o.roff = fvhuff::rec64(j, 21); o.mcus_y = j[23];
  const int len = j[12], file0 = j[13], L = j[15], nsub = j[16];
  bool ok = j[0] == 1 && o.cls >= 0 && o.cls <= 3 && o.x0 >= 0 && o.y0 >= 0 && o.mw >= 1 && o.mh >= 1 && o.mcus_x >= 1 &&
            o.mcus_x <= fvhuff::MAX_MCUS && o.mcus_y >= 1 && o.mcus_y <= fvhuff::MAX_MCUS && o.x0 <= o.mcus_x - o.mw &&
            o.y0 <= o.mcus_y - o.mh && o.S >= 1 && o.S <= fvhuff::MAX_S && o.gx0 >= 0 && o.gw >= 1 && o.gw <= fvhuff::MAX_MCUS &&
            o.gx0 <= fvhuff::MAX_MCUS - o.gw;
  ok = ok && (long long)(o.gx0 + o.gw - 1) * o.S < o.mcus_x && o.bit0 >= 0 && o.bit0 <= 7;
  ok = ok && L >= MIN_SUBSEQ && L <= MAX_SUBSEQ && (L & (L - 1)) == 0 && len >= 1 && len <= MAX_SCAN && file0 >= 0 &&
       nsub == (len + L - 1) / L && nsub <= MAX_SUBSEQS;
  ok = ok && o.toff >= 0 && (o.toff & 15) == 0 && o.toff <= pool_bytes - 4ll * fvhuff::TABLES * fvhuff::TABLE_WORDS;
  ok = ok && o.eoff >= 0 && (o.eoff & 15) == 0 && o.eoff <= pool_bytes - 16ll * o.gw * o.mh;
  ok = ok && o.soff >= 0 && o.soff <= pool_bytes - len;
  ok = ok && o.roff >= 0 && o.roff <= scratch_records - nsub;
  if (!ok) return false;
  o.len = (uint32_t)len; o.file0 = (uint32_t)file0; o.L = (uint32_t)L; o.nsub = (uint32_t)nsub;
  const int hmax = (o.cls == 1 || o.cls == 2) ? 2 : 1, vmax = o.cls == 2 ? 2 : 1;
  o.nl = hmax * vmax;
  o.nb = o.cls == 3 ? 1 : o.nl + 2;
  return true;
}

FVH_FN void put_state(uint32_t* rec, int at, State s) { rec[at] = s.byte; rec[at + 1] = s.w; }
FVH_FN State get_state(const uint32_t* rec, int at) { return State{rec[at], rec[at + 1]}; }

// subsequence i from the entry state in its record: the exit state and the sums into the record
FVH_FN void decode_record(const Job& J, const uint8_t* d, const uint32_t* tables, uint32_t* recs, uint32_t i) {
  uint32_t* rec = recs + (size_t)i * REC_WORDS;
  Sums sums;
  const uint32_t lo = boundary(d, J.len, (unsigned long long)i * J.L), hi = boundary(d, J.len, (unsigned long long)(i + 1) * J.L);
  put_state(rec, 0, decode_subseq(d, J.len, lo, hi, get_state(rec, 2), tables, J.nb, J.nl, sums));
  rec[4] = sums.mcus;
  rec[5] = (uint32_t)(uint16_t)sums.dc0 | (uint32_t)(uint16_t)sums.dc1 << 16;
  rec[6] = (uint32_t)(uint16_t)sums.dc2;
}

// THE SPECULATIVE PASS: subsequence i from its first bit, b = 0, k = 0 -- subsequence 0 from the scan's true start
FVH_FN void pass_speculate(const Job& J, const uint8_t* d, const uint32_t* tables, uint32_t* recs, uint32_t i) {
  uint32_t* rec = recs + (size_t)i * REC_WORDS;
  put_state(rec, 2, i == 0 ? make(0u, J.bit0, 0, 0) : make(boundary(d, J.len, (unsigned long long)i * J.L), 0, 0, 0));
  rec[7] = 0;
  decode_record(J, d, tables, recs, i);
}

// A ROUND, first half: the predecessor's exit state becomes the entry state; whether that changed it.  Reads exit states
// and writes entry states only, the second half the other way round: with a barrier between the halves every round sees
// the exit states of the round before, whatever the order of the lanes.
//
// An INVALID exit state is NOT taken: a speculative decode that died says nothing about its successor, whose own
// speculative state stays until the predecessor has a valid exit state.  Exactness does not need it: the first
// subsequence that is not yet right has a predecessor that is right, and on an intact stream that one's exit state is
// valid and is taken.  Where the true exit state is INVALID (a damaged stream), the subsequences behind it keep what they
// have; the scan counts MCU starts only up to the first INVALID exit state (`valid_prefix`).
FVH_FN bool round_take(uint32_t* recs, uint32_t i) {
  if (i == 0) return false;
  uint32_t* rec = recs + (size_t)i * REC_WORDS;
  const State in = get_state(rec - REC_WORDS, 0);
  const bool changed = in.byte != INVALID && !same(in, get_state(rec, 2));
  if (changed) put_state(rec, 2, in);
  rec[7] = changed ? 1u : 0u;
  return changed;
}

// second half: decode again where the entry state changed
FVH_FN void round_decode(const Job& J, const uint8_t* d, const uint32_t* tables, uint32_t* recs, uint32_t i) {
  if (recs[(size_t)i * REC_WORDS + 7]) decode_record(J, d, tables, recs, i);
}

// The MCU starts in front of the first INVALID exit state, that subsequence's own included (they were seen before its walk
// gave up): what is known of a run of subsequences, and how two neighbouring runs join.  Associative, not commutative.
struct Prefix {
  uint32_t n, dead;
};
FVH_FN Prefix prefix_of(const uint32_t* rec) { return Prefix{rec[4], rec[0] == INVALID ? 1u : 0u}; }
FVH_FN Prefix join(Prefix a, Prefix b) { return a.dead ? a : Prefix{a.n + b.n, b.dead}; }

// the MCU start behind which no group start is needed
FVH_FN long long last_needed(const Job& J) { return (long long)(J.y0 + J.mh - 1) * J.mcus_x + (long long)(J.gx0 + J.gw - 1) * J.S; }

struct Emit {
  const Job* J;
  uint8_t* entries;      // pool + eoff: 16 * gw * mh bytes, checked by open_job
  uint32_t first;        // the index of the subsequence's first MCU start
  int pred0, pred1, pred2;      // the predictors at its entry
  FVH_FN void operator()(uint32_t m, uint32_t byte, int bit, const Sums& dc) const {
    const uint32_t at = first + m, my = at / (uint32_t)J->mcus_x, mx = at - my * (uint32_t)J->mcus_x;
    if (my < (uint32_t)J->y0 || my >= (uint32_t)(J->y0 + J->mh) || mx % (uint32_t)J->S) return;
    const uint32_t gx = mx / (uint32_t)J->S;
    if (gx < (uint32_t)J->gx0 || gx >= (uint32_t)(J->gx0 + J->gw)) return;
    uint32_t* e = reinterpret_cast<uint32_t*>(entries + 16ll * ((long long)(my - J->y0) * J->gw + (gx - J->gx0)));
    e[0] = J->file0 + byte;
    e[1] = (uint32_t)bit;
    e[2] = (uint32_t)(uint16_t)(pred0 + dc.dc0) | (uint32_t)(uint16_t)(pred1 + dc.dc1) << 16;
    e[3] = (uint32_t)(uint16_t)(pred2 + dc.dc2);
  }
};

// EMISSION: subsequence i once more from its final entry state; every group start inside that the window needs is
// written where fv_jpeg_huff reads it.  A subsequence whose MCU starts all lie outside the window's rows is not walked.
FVH_FN void pass_emit(const Job& J, const uint8_t* d, const uint32_t* tables, const uint32_t* recs, uint32_t i, uint32_t next_first,
                      uint8_t* pool) {
  const uint32_t* rec = recs + (size_t)i * REC_WORDS;
  const unsigned long long row0 = (unsigned long long)J.y0 * J.mcus_x, row1 = (unsigned long long)(J.y0 + J.mh) * J.mcus_x;
  if (next_first <= rec[4] || next_first <= row0 || rec[4] >= row1) return;
  Emit e;
  e.J = &J; e.entries = pool + J.eoff; e.first = rec[4];
  e.pred0 = (int16_t)(rec[5] & 0xffffu); e.pred1 = (int16_t)(rec[5] >> 16); e.pred2 = (int16_t)(rec[6] & 0xffffu);
  Sums sums;
  const uint32_t lo = boundary(d, J.len, (unsigned long long)i * J.L), hi = boundary(d, J.len, (unsigned long long)(i + 1) * J.L);
  walk(d, J.len, lo, hi, get_state(rec, 2), tables, J.nb, J.nl, sums, e);
}

}  // namespace fvsync
#endif
