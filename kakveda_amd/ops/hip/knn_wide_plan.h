// Host-side plan of the wide exact search, cosine_topk_wide: KMAX < k <=
// KWIDE_MAX results per query. Pure C++ like knn_plan.h (no HIP, no torch), so
// every decision the host takes is checked on the CPU
// (tests/host/knn_wide_plan_test.cpp).
//
// The pipeline is floors -> emission -> wide selection, at every N (the list
// kernels keep KMAX entries per chunk and cannot serve k > KMAX):
//
//   floors     a compact prepass of the 128x128 list kernel over a prefix of
//              the corpus, run WITHOUT a threshold array (its 8-deep list
//              minima bound the 8th best, not the k-th), writes [B][pre_grid]
//              [KMAX] partials: scores of distinct real columns. The k-th
//              largest finite partial of a query lower-bounds its k-th best
//              eligible score. With fewer than k finite partials there is no
//              floor and every eligible row is emitted.
//   emission   the existing kernels, unmodified, over ALL columns (the
//              sample's own top k is unknown, so nothing is seeded or
//              skipped): the streaming kernel for B <= WIDE_GROUP, the 8-phase
//              emission kernel for larger unfiltered batches, and for larger
//              filtered batches (no 8-phase kernel carries the filter) and
//              corpora under MIN_N_8P rows the streaming kernel once per group
//              of WIDE_GROUP queries, each launch reading the corpus again.
//   selection  emit_merge_topk_wide, one block per query.
//
// A query whose candidates exceed `cap`, or an overflowed record segment, is
// answered by the same pipeline over consecutive corpus slices of at most
// `cap` rows (a slice cannot overflow: it emits at most its rows, through the
// streaming kernel, which has no segments), selected across the slices.
#pragma once

#include <algorithm>

#include "knn_plan.h"

namespace kakveda {

constexpr int KWIDE_MAX = 64;          // results per query of the wide path
constexpr int WIDE_GROUP = SMALLB_MAX;  // queries per streaming launch
// Prepass sample: as the emission path's, PREG_EMIT blocks of PRE_TILES
// 128-column tiles (262,144 columns), or the whole corpus where it is smaller.
constexpr int WIDE_PRE_BLOCKS = PREG_EMIT;
// Entries the selection kernel sorts at once (knn_wide_impl.h); the floor
// kernel selects over pre_grid * KMAX <= WIDE_PRE_BLOCKS * KMAX partials.
constexpr int WIDE_SEL_TILE = 1024;

// The k a request is served at: k past KWIDE_MAX returns the top KWIDE_MAX
// (the caller pads), k < 1 is the caller's error and becomes 1 here.
inline int wide_clamp_k(long k) {
  return (int)std::max(1L, std::min(k, (long)KWIDE_MAX));
}

enum class WideMain { Stream, Emit8p, StreamGroups };

struct WideSpan {
  long first, count;
};

struct WidePlan {
  int k;
  WideMain main;
  bool prepass;   // a floor can exist: the partials can hold k finite entries
  int pre_grid;   // prepass grid.x (a multiple of 8), blocks past the corpus idle
  int pre_tiles;  // 128-column tiles per prepass block
  long cap;       // candidates per query
  Chunking ch;    // Emit8p main launch (whole corpus, unseeded)
  long seg;       // Emit8p records per block segment
  int smallb_blocks;  // streaming grid.x
  int groups;         // streaming launches (1 under Stream, 0 under Emit8p)
};

// Finite entries the prepass partials can hold at most: every block keeps
// min(KMAX, its real columns).
inline long wide_partial_slots(long N) {
  const long block_cols = (long)PRE_TILES * BN;
  const long cols = std::min(N, (long)WIDE_PRE_BLOCKS * block_cols);
  const long full = cols / block_cols, rest = cols % block_cols;
  return full * KMAX + std::min(rest, (long)KMAX);
}

// Record segments of the wide 8-phase launch. EMIT_SEG_DEFAULT was sized for
// the 8-deep floor; a k-deep floor lets about k / KMAX times as many records
// through, so the default grows with ceil(k / KMAX). The segments never take
// more bytes than the candidate buffer beside them (both hold 8-byte
// entries): seg * blocks <= B * cap, which needs B * cap >= blocks (plan_wide
// picks the 8-phase kernel only then). `seg_arg` > 0 forces the size, still
// inside the budget.
inline long wide_seg_cap(int B, long cap, const Chunking& ch, int k, long seg_arg) {
  const long blocks = (long)ch.nchunks * ch.row_tiles;
  const long budget = std::max(1L, (long)B * std::max(cap, 0L) / blocks);
  const long want = seg_arg > 0
                        ? seg_arg
                        : EMIT_SEG_DEFAULT * ((wide_clamp_k(k) + KMAX - 1) / KMAX);
  return std::max(1L, std::min(want, budget));
}

// Groups of at most WIDE_GROUP queries for the streaming kernel.
inline int wide_group_count(long B) { return (int)((B + WIDE_GROUP - 1) / WIDE_GROUP); }
inline WideSpan wide_group(long B, int g) {
  const long first = (long)g * WIDE_GROUP;
  return {first, std::max(0L, std::min((long)WIDE_GROUP, B - first))};
}

// Consecutive corpus slices of at most `cap` rows for the overflow fallback.
inline long wide_slice_count(long N, long cap) {
  const long c = std::max(1L, cap);
  return (N + c - 1) / c;
}
inline WideSpan wide_slice(long N, long cap, long s) {
  const long c = std::max(1L, cap);
  const long first = s * c;
  return {first, std::max(0L, std::min(c, N - first))};
}

// `slice`: the plan of one fallback slice (N <= cap): streaming only.
// `seg_arg` / `target` <= 0: the defaults.
inline WidePlan plan_wide(int B, int N, long k, bool filtered, long cap,
                          long seg_arg, long target, bool slice) {
  WidePlan p{};
  p.k = wide_clamp_k(k);
  p.cap = std::max(1L, cap);
  p.prepass = wide_partial_slots(N) >= p.k;
  const long ntiles = ((long)N + BN - 1) / BN;
  const long blocks =
      std::min((ntiles + PRE_TILES - 1) / PRE_TILES, (long)WIDE_PRE_BLOCKS);
  p.pre_grid = (int)((blocks + 7) & ~7L);
  p.pre_tiles = PRE_TILES;
  p.smallb_blocks = (int)std::max(1L, std::min(((long)N + 31) / 32, 8192L));
  p.ch = chunking(B, N, BM8, target > 0 ? target : default_target(BM8));
  const bool fits = (long)B * p.cap >= (long)p.ch.nchunks * p.ch.row_tiles;
  if (B <= WIDE_GROUP) {
    p.main = WideMain::Stream;
    p.groups = 1;
  } else if (!slice && !filtered && N >= MIN_N_8P && fits) {
    p.main = WideMain::Emit8p;
    p.groups = 0;
    p.seg = wide_seg_cap(B, p.cap, p.ch, p.k, seg_arg);
  } else {
    p.main = WideMain::StreamGroups;
    p.groups = wide_group_count(B);
  }
  return p;
}

}  // namespace kakveda
