// Host-side plan for the list-major (batched) routed scan: the geometry of
// ivf_scan_grouped_kernel, the bound on its tile count that needs no device
// read, and the size of its candidate buffer. Pure C++ (no HIP, no torch) so
// it is checked on the CPU (tests/host/ivf_batch_plan_test.cpp).
//
// The B x (nprobe + 1) (query, probe) pairs of a batch - the tail being one
// pseudo-list that every query probes - are grouped by list and cut into
// tiles of at most IVF_BATCH_QTILE queries of one list. One block scans one
// (tile, row slice): the list's rows are gathered once per tile, not once
// per query.
#pragma once

#include <algorithm>
#include <stdexcept>

#include "ivf_plan.h"  // KMAX, IVF_MAX_BLOCKS

namespace kakveda {

// Queries per tile: the N of one mfma_f32_16x16x32_bf16. A 32-query tile
// would halve the gathers of a list 17..32 queries share, but every lane
// then keeps two sorted top-KMAX lists (32 more VGPRs) beside the
// double-buffered row fragments, and below B ~ 1500 at nprobe = 32 the mean
// group (B * nprobe / L) is under 16 queries, so the second half of such a
// tile would mostly score pad lanes.
constexpr int IVF_BATCH_QTILE = 16;
// rows a block takes per iteration: 4 waves x the 16 rows (M) of one MFMA
constexpr int IVF_BATCH_BLOCK_ROWS = 64;
// rows one block should walk before another slice is worth a block: 16
// iterations keep the tile's query gather (QTILE x D bf16 into LDS) and the
// per-query LDS merge a small share of the block's row traffic
constexpr int IVF_BATCH_ROWS_PER_SLICE = 16 * IVF_BATCH_BLOCK_ROWS;
constexpr int IVF_BATCH_MAX_SLICES = 64;
// candidate-buffer bytes of one launch; a batch whose buffer would pass it
// is scanned in chunks of queries
constexpr long IVF_BATCH_MAX_CAND_BYTES = 256L << 20;

// The tile's queries live in LDS at a pitch of 2 D + 16 bytes, beside the
// kernel's 16 KiB of merge lists: 48 KiB keeps the block within the 64 KiB
// a launch gets without opting in to more. The widest D (a multiple of 64)
// that fits is IVF_BATCH_MAX_D; wider rows stay with the per-query scan.
constexpr long IVF_BATCH_MAX_QUERY_LDS = 48 * 1024;
inline long ivf_batch_query_lds(int D) {
  return (long)IVF_BATCH_QTILE * ((long)D * 2 + 16);
}
constexpr int IVF_BATCH_MAX_D = 1472;

struct IvfBatchPlan {
  long pairs;         // P = B * (nprobe + 1)
  long max_tiles;     // grid.y: >= the tile count of any grouping of P pairs
  int slices;         // grid.x: blocks sharing one tile's list
  long slots;         // candidate slots (of KMAX entries) per query
  long cand_entries;  // 64-bit entries per query: slots * KMAX
  long cand_bytes;    // candidate buffer of one launch over B queries
};

// Upper bound on the tiles of P pairs over L lists plus the tail, whatever
// the grouping: sum_l ceil(c_l / QTILE) <= floor(P / QTILE) + (non-empty
// groups), there are at most L + 1 groups, and no tile is empty.
inline long ivf_batch_tile_bound(long P, long L) {
  return std::min(P, P / IVF_BATCH_QTILE + L + 1);
}

// Slice rule: one slice per IVF_BATCH_ROWS_PER_SLICE rows of the longest
// source (list or tail), at most IVF_BATCH_MAX_SLICES, and no more than
// keeps max_tiles * slices within IVF_MAX_BLOCKS (unless one slice per tile
// already passes it). Every tile gets the same slice count; a block whose
// slice starts past the end of its list leaves its preset-empty slots alone.
inline IvfBatchPlan plan_ivf_batch(long max_list_len, long tail_len, int nprobe,
                                   int B, int L) {
  if (nprobe < 0 || B < 1 || L < 0 || max_list_len < 0 || tail_len < 0)
    throw std::invalid_argument("plan_ivf_batch: negative size");
  IvfBatchPlan p;
  p.pairs = (long)B * (nprobe + 1);
  p.max_tiles = ivf_batch_tile_bound(p.pairs, L);
  const long longest = std::max(max_list_len, tail_len);
  long s = (longest + IVF_BATCH_ROWS_PER_SLICE - 1) / IVF_BATCH_ROWS_PER_SLICE;
  s = std::min(s, std::max(1L, IVF_MAX_BLOCKS / p.max_tiles));
  s = std::min<long>(std::max(1L, s), IVF_BATCH_MAX_SLICES);
  p.slices = (int)s;
  p.slots = (long)(nprobe + 1) * p.slices;
  p.cand_entries = p.slots * KMAX;
  p.cand_bytes = (long)B * p.cand_entries * 8;
  return p;
}

// Queries per launch so that the candidate buffer stays within
// IVF_BATCH_MAX_CAND_BYTES (one query's worth may pass it: nprobe <= 65534
// and 64 slices make at most 2 GiB, and a launch needs one query). The
// slice count only falls as B grows, so the bytes per query of a B-query
// launch bound those of every chunk planned with the same B.
inline int ivf_batch_chunk_queries(long max_list_len, long tail_len, int nprobe,
                                   int B, int L) {
  if (B < 1) throw std::invalid_argument("ivf_batch_chunk_queries: negative size");
  const IvfBatchPlan p = plan_ivf_batch(max_list_len, tail_len, nprobe, 1, L);
  const long per_query = p.cand_entries * 8;  // the most slices any B gets
  const long fit = std::max(1L, IVF_BATCH_MAX_CAND_BYTES / per_query);
  return (int)std::min<long>(B, fit);
}

}  // namespace kakveda
