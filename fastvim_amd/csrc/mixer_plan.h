// Launch plans of the four row-kernel families of the fused mixer (conv + pool forward / adjoint, combine forward /
// adjoint): which kernel form a shape takes, with how many channels per lane, waves, channel slabs and row groups.
// Pure host code -- no HIP call -- so the same functions serve the launchers, fv_mixer_bwd_blocks,
// fv_mixer_conv_pool_bwd2_ok and the read-only fv_mixer_plan query: a predicate cannot drift from its dispatcher.
//
// A block covers `waves` x 64 lanes x `vec` channels of a token, `row_groups` pooling rows at a time; `slabs` blocks
// (a second / third grid dimension) cover d_inner.  The depthwise conv, the pooling, the D skip and their adjoints never
// mix channels, so the conv + pool families may cut d_inner into slabs (d_inner 2048 = 2 x 1024, 2560 = 2 x 1280 in the
// generic adjoint); the combine families need LayerNorm sums over the whole row and always have slabs == 1.
#pragma once
#include "common.h"

namespace fvplan {

enum Family { CONV_POOL_FWD = 0, COMBINE_FWD = 1, COMBINE_BWD = 2, CONV_POOL_BWD = 3 };
enum Form {
  UNSUPPORTED = 0,
  GENERIC = 1,    // token-tile / streaming kernels of mixer_fwd.hip, mixer_bwd.hip
  ROW = 2,        // whole-row packed-math kernels (14 / 16 columns): convpool_fwd_row.hip, convpool_bwd_row.hip
  CELL = 3,       // 8-token cell walkers (tokens_per_patch 8, or long dense rows), same files
  WAVE = 4,       // wave-per-token combine kernels (combine_wave.hip)
};

struct Plan {
  int form, vec, waves, slabs, row_groups, lds_bytes;
  int dxc2;       // CONV_POOL_BWD: the form takes a second pooled-gradient addend
};

struct Shape {
  int B, rows, cols, tpp, d_in, pool_max, dtype;     // cols = patch columns of a pooling row
};

constexpr int RGMAX = 4;           // row groups per block, at most
constexpr int WAVE_NW = 4;         // waves (= pooling groups in flight) per block of the wave-per-token combine kernels
constexpr int LDS_MAX = 160 * 1024;

// one batch element per buffer descriptor (32-bit byte offsets, fp32 worst case)
inline bool desc_fits(const Shape& s) { return (size_t)s.rows * s.cols * s.tpp * 2 * s.d_in * 4 <= 0xfffff000ull; }

// smallest number of equal slabs that brings `nch` channel waves under `cap`
inline int slabs_for(int nch, int cap) {
  int s = 1;
  while (s < nch && (nch % s || nch / s > cap)) ++s;
  return s;
}

// ------------------------------------------------------------------ conv + pool forward
// cell walkers: the smallest split of d_in / 128 waves into blocks of at most 2 waves.  The waves of a block share
// nothing (each owns 128 channels of the row), so small blocks only help the dispatcher fill the CUs: FastChannelVim-S
// (6 waves of channels) 101.1 us with one 6-wave block per row, 86.9 with three 2-wave blocks; FastVim-B at 2048 px
// (12 waves) 239.6 -> 195.7 us (profiles/r05_ab_chan_block_shapes.log)
inline int fwd_cell_groups(int d_in) {
  static const int t_gq = fv_tune("FASTVIM_FWD_CHAN_GROUPS", 0);   // tuning hook
  const int nw = d_in / 128;
  int gq = (nw + 1) / 2;
  while (nw % gq) ++gq;
  return (t_gq > 0 && nw % t_gq == 0) ? t_gq : gq;
}

// whole-row kernel: channel pairs per lane (0: not served).  One pair per lane measured fastest (12.8 vs 16.5 us with
// three pairs on FastVim-T): more, shorter waves.  The channel groups ride on blockIdx.z, so the width is bounded only
// by what has been run: 24 waves of 128 channels (d_inner 3072).
inline int fwd_row_pairs(int d_in) {
  static const int force = fv_tune("FASTVIM_FWD_NP", 0);   // tuning hook
  if ((force == 0 || force == 1) && d_in % 128 == 0 && d_in <= 24 * 128) return 1;
  if ((force == 0 || force == 2) && d_in % 256 == 0 && d_in <= 8 * 256) return 2;
  return 0;
}

// whole-row kernel: blocks of at most 4 waves (channel groups over blockIdx.z), like the long-row kernel: FastVim-B
// 46.4 -> 43.2 us, FastVim-T (3 waves) unchanged
inline int fwd_row_groups(int d_in, int np) {
  static const int t_gq = fv_tune("FASTVIM_FWD_ROW_GROUPS", 0);   // tuning hook
  const int nw = d_in / (128 * np);
  int gq = (nw + 3) / 4;
  while (nw % gq) ++gq;
  return (t_gq > 0 && nw % t_gq == 0) ? t_gq : gq;
}

inline int fwd_generic_vec(int d_in, int tpp) {
  static const int force = fv_tune("FASTVIM_FWD_VEC", 0);   // tuning hook
  if ((force == 2 || tpp > 1) && d_in % 128 == 0 && d_in <= 8 * 128) return 2;
  if (tpp > 1 && d_in % 256 == 0 && d_in <= 8 * 256) return 4;
  if (tpp > 1) return 1;
  if (d_in % 384 == 0) return 6;
  if (d_in % 256 == 0) return 4;
  return 1;
}

inline Plan conv_pool_fwd(const Shape& s) {
  Plan r{};
  static const bool rowk = (fv_tune("FASTVIM_FWD_ROWK", 1) != 0);   // tuning hooks
  static const bool chan = (fv_tune("FASTVIM_FWD_CHAN", 1) != 0);
  const bool fits = s.d_in % 128 == 0 && desc_fits(s);
  if (rowk && !s.pool_max) {     // mean pooling: the packed-math kernels where the row shape is one they are built for
    const bool chan8 = s.tpp == 8 && s.cols >= 2 && s.d_in <= 8 * 128;
    const bool dense8 = s.tpp == 1 && s.cols % 8 == 0 && s.cols >= 24;     // the 512 / 1024 / 2048 px grids
    if (chan && fits && (chan8 || dense8)) {
      const int gq = fwd_cell_groups(s.d_in);
      r = Plan{CELL, 2, s.d_in / 128 / gq, gq, 1, 0, 0};
      return r;
    }
    const int np = (s.tpp == 1 && (s.cols == 14 || s.cols == 16) && fits) ? fwd_row_pairs(s.d_in) : 0;
    if (np) {
      const int gq = fwd_row_groups(s.d_in, np);
      r = Plan{ROW, 2 * np, s.d_in / (128 * np) / gq, gq, 1, 0, 0};
      return r;
    }
  }
  const int v = fwd_generic_vec(s.d_in, s.tpp);
  const int nch = fv_cdiv(s.d_in, 64 * v);
  const int slabs = slabs_for(nch, v == 1 ? 16 : 8);      // wider rows: channel slabs over blockIdx.z
  const int waves = nch / slabs;
  const size_t lds = (s.tpp > 1 && s.cols > 1) ? (size_t)(s.pool_max ? 4 : 2) * s.tpp * 64 * waves * v * 4 : 0;
  if (lds > (size_t)LDS_MAX) return r;
  r = Plan{GENERIC, v, waves, slabs, 1, (int)lds, 0};
  return r;
}

// ------------------------------------------------------------------ combine (LayerNorm over the whole d_inner row)
inline int combine_wave_mode() {   // tuning hook: 0 = generic kernels only, 1 = wave kernels where a token spans more than one 384-chunk, 2 = wherever they apply
  static const int m = fv_tune("FASTVIM_COMBINE_WAVE", 2);
  return m;
}
inline int combine_wave_chunks(int d_in) {
  if (d_in % 384 != 0 || d_in / 384 > 2) return 0;
  const int nck = d_in / 384;
  return (combine_wave_mode() >= 2 || (combine_wave_mode() == 1 && nck > 1)) ? nck : 0;
}
inline bool combine_wave_wide_fwd(int d_in) { return d_in == 4 * 384 && combine_wave_mode() >= 1; }
inline bool combine_wave_wide_bwd(int d_in) {
  static const bool on = (fv_tune("FASTVIM_COMBINE_WAVE_B", 1) != 0);   // tuning hook
  return on && d_in == 4 * 384 && combine_wave_mode() >= 1;
}

// Generic combine kernels: channels per lane.  A row of up to 8 waves x 6 / 4 / 2 channels, else one channel per lane
// up to 16 waves -- and, past those (d_inner 2560: 40 waves of single channels), 8 channels per lane on up to 8 waves
// (2560 = 5 waves x 64 x 8): two 16-byte accesses per lane and tensor, the row's sums still one LDS exchange.
// The 8-channel kernels are built for tokens_per_patch 1 only.  The un-pooled geometry (one patch column, every token
// its own pooling group: the masked MAE encoders and the un-pooled Vim mixer run as rows x 1 x t) still takes them: with
// one column, rows x 1 x t addresses exactly the memory of rows*t x 1 x 1 -- token i*t + c, yc / dyc row i*t + c -- and
// is launched as that (combine_redescribed).  tokens_per_patch > 1 with more than one patch column (the channel
// models' LDS slot accumulators) stays unsupported at these widths: no reference model has it.
inline int combine_wide8(int d_in, int pcols, int tpp) {
  return (tpp == 1 || pcols == 1) && d_in > 16 * 64 && d_in % 512 == 0 && d_in <= 8 * 512;
}
inline int combine_fwd_vec(int d_in, int pcols, int tpp) {
  const int v = (d_in % 384 == 0 && d_in <= 8 * 384) ? 6 : (d_in % 256 == 0 && d_in <= 8 * 256) ? 4 : (d_in % 128 == 0 && d_in <= 8 * 128) ? 2 : 1;
  return (v == 1 && combine_wide8(d_in, pcols, tpp)) ? 8 : v;
}
inline int combine_bwd_vec(int d_in, int pcols, int tpp) {
  int v;
  if (tpp > 1)      // LDS slot accumulators: keep the per-lane state small
    v = (d_in % 128 == 0 && d_in <= 8 * 128) ? 2 : (d_in % 256 == 0 && d_in <= 8 * 256) ? 4 : 1;
  else
    v = (d_in % 384 == 0 && d_in <= 8 * 384) ? 6 : (d_in % 256 == 0 && d_in <= 8 * 256) ? 4 : 1;
  return (v == 1 && combine_wide8(d_in, pcols, tpp)) ? 8 : v;
}
// the launch walks rows*tpp one-token rows with the tokens_per_patch 1 kernels (natural token order only)
inline bool combine_redescribed(int vec, int pcols, int tpp) { return vec == 8 && pcols == 1 && tpp > 1; }
inline int combine_rg(int d_in, int vec) {
  const int nch = fv_cdiv(d_in, 64 * vec), r = 8 / nch;
  return r < 1 ? 1 : (r > RGMAX ? RGMAX : r);
}

inline Plan combine_fwd(const Shape& s) {
  Plan r{};
  if ((combine_wave_wide_fwd(s.d_in) && desc_fits(s)) || combine_wave_chunks(s.d_in)) {
    r = Plan{WAVE, s.d_in / 64, 1, 1, WAVE_NW, 0, 0};
    return r;
  }
  const int v = combine_fwd_vec(s.d_in, s.cols, s.tpp), nch = fv_cdiv(s.d_in, 64 * v);
  if (nch > (v == 1 ? 16 : 8)) return r;
  const int tt = (s.cols * s.tpp % 2 == 0 && !combine_redescribed(v, s.cols, s.tpp)) ? 2 : 1;
  r = Plan{GENERIC, v, nch, 1, combine_rg(s.d_in, v), RGMAX * tt * 16 * 4, 0};
  return r;
}

inline Plan combine_bwd(const Shape& s) {
  Plan r{};
  if ((combine_wave_wide_bwd(s.d_in) && desc_fits(s)) || combine_wave_chunks(s.d_in)) {
    r = Plan{WAVE, s.d_in / 64, 1, 1, WAVE_NW, 2 * s.d_in * 4, 0};
    return r;
  }
  const int v = combine_bwd_vec(s.d_in, s.cols, s.tpp), nch = fv_cdiv(s.d_in, 64 * v);
  if (nch > (v == 1 ? 16 : 8)) return r;
  const int rg = combine_rg(s.d_in, v), tt = (s.cols * s.tpp % 2 == 0 && !combine_redescribed(v, s.cols, s.tpp)) ? 2 : 1;
  const size_t extra = (s.tpp > 1 && s.cols > 1) ? (size_t)s.tpp * 64 * nch * rg * v : 0;
  if ((RGMAX * 64 + 2 * (size_t)s.d_in + extra) * 4 > 64 * 1024) return r;
  r = Plan{GENERIC, v, nch, 1, rg, (int)((RGMAX * 2 * tt * 16 + 2 * (size_t)s.d_in + extra) * 4), 0};
  return r;
}

// ------------------------------------------------------------------ conv + pool adjoint
// Channels per lane and channel slabs of the streaming kernel: a channel pair per lane up to 12 waves (d_inner 1536), a
// single channel up to 16 waves; wider rows (d_inner 2048, 2560, ... 3072) as two slabs of channel pairs.  A slab is a
// second grid dimension: channel-offset pointers, the full d_inner as the row stride, its own columns of the block's
// gradient partial.
inline void conv_pool_bwd_vec(int d_in, int& vec, int& slabs) {
  vec = (d_in % 128 == 0 && d_in <= 12 * 128) ? 2 : 1;
  slabs = 1;
  if (vec == 1 && fv_cdiv(d_in, 64) > 16) {
    if (d_in % 256 == 0 && d_in <= 2 * 12 * 128) { vec = 2; slabs = 2; }
    else slabs = 0;      // not served
  }
}
inline int conv_pool_bwd_rg(int d_slab, int vec) {
  const int nch = fv_cdiv(d_slab, 64 * vec), r = (vec == 1 ? 16 : 12) / nch;
  return r < 1 ? 1 : (r > RGMAX ? RGMAX : r);
}

// Channel groups (blockIdx.y), waves and row groups per block of the whole-row / cell-walking adjoint kernels
// (convpool_bwd_row.hip), for `nch` waves of 128 channels and `rg` row groups of the persistent grid.
struct BwdRowSplit { int groups, nchg, rgr; bool long_rows, chan8; };
inline BwdRowSplit conv_pool_bwd_row_split(const Shape& s, int nch, int rg) {
  BwdRowSplit q{1, nch, 1, false, false};
  q.chan8 = s.tpp == 8 && s.cols >= 2;
  const bool dense8 = s.tpp == 1 && s.cols % 8 == 0 && s.cols >= 24;      // 512 / 1024 / 2048 px grids
  q.long_rows = q.chan8 || dense8;
  // Long-row kernels (201 VGPRs: 8 waves per CU): blocks of FOUR waves -- at most two waves of channels x two or four
  // rows -- so that two blocks share a CU and the dispatcher has 2-6x as many, lighter blocks to balance (six-wave
  // blocks left a quarter of the wave slots empty): FastChannelVim-S 200.5 -> 173 us, FastVim-B at 2048 px 448.7 ->
  // 385 us (profiles/r05_ab_chan_block_shapes.log)
  static const int t_groups = fv_tune("FASTVIM_BWD_CHAN_GROUPS", 0), t_rg = fv_tune("FASTVIM_BWD_CHAN_RG", 0);   // tuning hooks
  // rows live in registers: whole-row blocks of <= 512 threads (256 VGPRs per wave) for fp32 storage and 16-token rows,
  // <= 768 (168) for the bf16 14-token kernel, i.e. fewer row groups per block than the generic kernel, over the same
  // persistent grid.  The split must not leave wave slots of the CU empty (FastVim-B, 12 waves of channels: two
  // 6-wave blocks 99.5 us, one 12-wave block 73.4, three 4-wave blocks 75.6)
  const int wmax = (q.long_rows || s.dtype == FV_F32 || s.cols > 14) ? 8 : 12;
  if (q.long_rows) {
    q.groups = (nch + 1) / 2;
    while (nch % q.groups) ++q.groups;
    if (t_groups > 0 && nch % t_groups == 0) q.groups = t_groups;
    q.nchg = nch / q.groups;
    q.rgr = t_rg > 0 ? t_rg : 4 / q.nchg;
  } else {
    static const int r_groups = fv_tune("FASTVIM_BWD_ROW_GROUPS", 0), r_rg = fv_tune("FASTVIM_BWD_ROW_RG", 0);   // tuning hooks
    int groups, nchg = nch, rgr = 1;
    for (groups = 1; groups <= nch; ++groups) {
      if (nch % groups) continue;
      nchg = nch / groups;
      if (nchg > wmax) continue;
      rgr = rg < wmax / nchg ? rg : wmax / nchg;
      if (wmax % (nchg * rgr) == 0) break;
    }
    if (groups > nch) { groups = nch; nchg = 1; rgr = 1; }
    if (r_groups > 0 && nch % r_groups == 0) { groups = r_groups; nchg = nch / groups; rgr = rg < wmax / nchg ? rg : (wmax / nchg < 1 ? 1 : wmax / nchg); }
    if (r_rg > 0) rgr = r_rg;
    q.groups = groups; q.nchg = nchg; q.rgr = rgr;
  }
  return q;
}

inline Plan conv_pool_bwd(const Shape& s) {
  Plan r{};
  int v, slabs;
  conv_pool_bwd_vec(s.d_in, v, slabs);
  if (!slabs) return r;
  const int d_slab = s.d_in / slabs;
  const int nch = fv_cdiv(d_slab, 64 * v), rg = conv_pool_bwd_rg(d_slab, v);
  static const bool rowk = (fv_tune("FASTVIM_BWD_ROWK", 1) != 0);   // tuning hooks
  static const bool chan = (fv_tune("FASTVIM_BWD_CHAN", 1) != 0);
  static const bool wide = (fv_tune("FASTVIM_BWD_ROWK_WIDE", 1) != 0);
  // the packed-math kernels: mean pooling, a lane owns a channel pair, d_inner whole waves of 128 channels
  if (rowk && v == 2 && !s.pool_max && s.d_in % 128 == 0 && desc_fits(s) &&
      (size_t)s.B * s.rows * s.d_in * 8 <= 0x7ffff000ull) {      // pooled gradients: one descriptor, int offsets
    const int nw = s.d_in / 128;
    const BwdRowSplit q = conv_pool_bwd_row_split(s, nw, rg);
    // widths the one-slab forms serve keep their launch exactly (a block reserves the whole row's accumulator); the
    // wider ones reserve their own channels' only
    const int nacc = (q.long_rows || s.d_in > 12 * 128) ? q.nchg * 128 : s.d_in;
    if (q.long_rows) {
      if (chan) {
        size_t lds = (size_t)12 * nacc * 4;
        if (q.chan8) lds += (size_t)q.nchg * q.rgr * ((2 * 3 + 2 * 8) * 64) * 8;      // + the waves' parked slot gradients (11 KB per wave)
        r = Plan{CELL, 2, q.nchg, q.groups, q.rgr, (int)lds, 0};
        return r;
      }
    } else if (s.tpp == 1 && (s.cols == 14 || s.cols == 16) && (q.groups == 1 || wide)) {
      r = Plan{ROW, 2, q.nchg, q.groups, q.rgr, 12 * nacc * 4, 1};
      return r;
    }
  }
  const size_t lds = (size_t)12 * d_slab * 4;
  if (lds > (size_t)LDS_MAX) return r;
  r = Plan{GENERIC, v, nch, slabs, rg, (int)lds, 0};
  return r;
}

// row groups of the persistent grid (rows of gradient partials = blocks along x)
inline int conv_pool_bwd_grid_rg(int d_in) {
  int v, slabs;
  conv_pool_bwd_vec(d_in, v, slabs);
  return slabs ? conv_pool_bwd_rg(d_in / slabs, v) : 1;
}

inline Plan plan(int family, const Shape& s) {
  switch (family) {
    case CONV_POOL_FWD: return conv_pool_fwd(s);
    case COMBINE_FWD: return combine_fwd(s);
    case COMBINE_BWD: return combine_bwd(s);
    case CONV_POOL_BWD: return conv_pool_bwd(s);
  }
  return Plan{};
}

}  // namespace fvplan
