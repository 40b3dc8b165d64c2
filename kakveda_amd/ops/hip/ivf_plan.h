// Host-side plan for the cluster-routed (IVF) search: launch geometry of
// ivf_scan_topk_kernel, the size of its candidate buffer, the row ->
// segment function the kernel and the host share, and the limits a store
// must meet before anything is launched. Pure C++ (no HIP, no torch) so it
// is checked on the CPU (tests/host/ivf_plan_test.cpp).
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>

#include "knn_plan.h"  // KMAX

#if defined(__HIPCC__)
#define IVF_HD __host__ __device__
#else
#define IVF_HD
#endif

namespace kakveda {

constexpr int IVF_MAX_SEGMENTS = 64;  // base pointers passed by value
constexpr int IVF_BLOCK_ROWS = 32;    // rows per block per iteration (4 waves x 8)
// rows one block should walk before another slice is worth a block: 8
// iterations keep the query load (D*2 bytes of LDS fill) and the block's
// tree merge a small share of its row traffic
constexpr int IVF_ROWS_PER_SLICE = 8 * IVF_BLOCK_ROWS;
constexpr int IVF_MAX_SLICES = 64;
// blocks of one launch: past this the grid only queues, and the candidate
// buffer (KMAX * 8 bytes per block) stays within tens of MB
constexpr long IVF_MAX_BLOCKS = 1 << 16;
constexpr int IVF_MAX_GRID_Z = 65535;  // queries per launch (grid.z)

// Row r of a store whose first segment has s0 rows and every later one q.
IVF_HD inline int ivf_segment_of(long r, long s0, long q) {
  return r < s0 ? 0 : 1 + (int)((r - s0) / q);
}
IVF_HD inline long ivf_local_row(long r, long s0, long q) {
  return r < s0 ? r : (r - s0) % q;
}

// The segment layout the kernel's row -> segment function assumes: at most
// IVF_MAX_SEGMENTS segments, every one after the first exactly as long as
// the second. Returns the quantum q (1 for a single segment); throws with
// the reason otherwise.
template <class RowsOf>
long ivf_check_segments(int n_segments, RowsOf&& rows_of) {
  if (n_segments < 1)
    throw std::invalid_argument("routed search needs at least one segment");
  if (n_segments > IVF_MAX_SEGMENTS)
    throw std::invalid_argument(
        "routed search supports at most " + std::to_string(IVF_MAX_SEGMENTS) +
        " store segments, got " + std::to_string(n_segments));
  if (rows_of(0) < 1)
    throw std::invalid_argument("routed search: the first segment is empty");
  if (n_segments == 1) return 1;
  const long q = rows_of(1);
  if (q < 1) throw std::invalid_argument("routed search: empty store segment");
  for (int i = 2; i < n_segments; ++i)
    if (rows_of(i) != q)
      throw std::invalid_argument(
          "routed search needs every store segment after the first to have "
          "the same row count; segment " + std::to_string(i) + " has " +
          std::to_string(rows_of(i)) + ", segment 1 has " + std::to_string(q));
  return q;
}

struct IvfPlan {
  int slices;         // grid.x: blocks sharing one source (list or tail)
  int sources;        // grid.y: nprobe lists + the tail
  long slots;         // candidate slots (of KMAX entries) per query
  long cand_entries;  // 64-bit entries per query: slots * KMAX
};

// slices from what the index knows without a device sync: the longest list
// and the tail length. Every source gets the same slice count (the grid is
// rectangular); a block whose slice starts past the end of its source
// writes an empty slot and exits.
inline IvfPlan plan_ivf_scan(long max_list_len, long tail_len, int nprobe, int B) {
  if (nprobe < 0 || B < 1 || max_list_len < 0 || tail_len < 0)
    throw std::invalid_argument("plan_ivf_scan: negative size");
  IvfPlan p;
  p.sources = nprobe + 1;
  const long longest = std::max(max_list_len, tail_len);
  long s = (longest + IVF_ROWS_PER_SLICE - 1) / IVF_ROWS_PER_SLICE;
  const long per_slice = (long)p.sources * std::min(B, IVF_MAX_GRID_Z);
  s = std::min(s, std::max(1L, IVF_MAX_BLOCKS / per_slice));
  s = std::min<long>(std::max(1L, s), IVF_MAX_SLICES);
  p.slices = (int)s;
  p.slots = (long)p.sources * p.slices;
  p.cand_entries = p.slots * KMAX;
  return p;
}

}  // namespace kakveda
