// List-major (batched) routed scan. Included by kakveda_kernels.hip after
// ivf_impl.h (IvfSegs, IvfFilterArg, bf16x8 / f32x4 / enc_f32 come from there
// and from kernels_impl.h). Nothing here shares a body with the kernels of
// those headers, so their machine code does not move.
//
// ivf_scan_topk_kernel runs one block per (query, probed list, slice): a list
// that 40 queries of a batch probe is gathered 40 times and scored with
// scalar FMAs. Here the (query, probe) pairs arrive grouped by list and cut
// into tiles of <= IVF_BATCH_QTILE queries (ops.ivf_group_probes); a block
// gathers its slice of the list once and scores it against the whole tile
// with mfma_f32_16x16x32_bf16.
#pragma once

#include <hip/hip_runtime.h>
#include "ivf_batch_plan.h"

namespace kakveda {

// rows of 16 bytes (one bf16x8) between two queries of the LDS tile: D / 8
// plus one, so the 16 queries a ds_read_b128 pass touches start 4 banks
// apart and cover the 64 banks once
DEVINL int ivf_batch_qpitch(int D) { return D / 8 + 1; }

constexpr int IVF_BATCH_GROUP_LINES = 4;  // 128-byte lines per load group

// ---------------------------------------------------------------------------
// ivf_scan_grouped_kernel<FILTER>: grid = (slices, tiles), 256 threads,
// dynamic LDS = QTILE * (D*2 + 16) bytes (the tile's queries).
//
// Tile t = (list tile_list[t], pairs [tile_first[t], + tile_count[t])); list
// == L is the tail [tail_lo, tail_hi). Blocks with t >= *n_tiles, an empty
// tile, or a slice that starts past the end of the list exit at once: the
// host presets the whole candidate buffer to 0 (= empty) before the launch,
// and a block that does scan stores KMAX entries to slot (b, y, slice) of
// every pair of its tile, b = pair_query[], y = pair_slot[]. A (b, y, slice)
// slot belongs to one pair, a pair to one tile, so no slot has two writers.
//
// A block walks positions blockIdx.x*64 + 64*slices*i of its list, wave w
// the 16 rows from +16w. Operands of D = A x B, A = 16 rows, B = 16 queries:
// lane l holds A[row l&15][k = 8*(l>>4) + j], j < 8, and the matching B
// fragment of query l&15; the result has col (query) = l&15 and row =
// 4*(l>>4) + reg. The gathered rows go straight from global memory to
// registers in that layout. The k order of the dot product is free as long
// as both operands agree; MFMA step m of a row takes bytes [64m + 16g,
// +16) for lane group g = l>>4. Four lanes of 16 bytes are all a row gets in
// one load instruction, so an instruction covers an aligned 64-byte half
// line per row; steps 2i and 2i+1 are loaded back to back, so the two halves
// of every 128-byte line are requested by consecutive instructions of the
// same wave (D % 64 == 0: a row is whole lines).
//
// Loads are double-buffered in groups of 4 lines (8 x 16 bytes per lane):
// group g+1 - or the first group of the next 16 rows - is in flight while
// group g is multiplied. Lines past the last whole group (D % 256 != 0) are
// loaded and multiplied one at a time.
//
// Top-k: lane (query c, group g) keeps a sorted top-KMAX of packed
// (enc_f32(score) << 32) | (0x7fffffff - row) over the rows 4g..4g+3 of every
// step of its wave; one LDS tree merge per query over its 16 lanes (4 waves
// x 4 groups) leaves the block's top-KMAX for each query.
//
// Guards, as ivf_scan_topk_kernel: list bounds are clamped to [0, n_ids]; a
// row id outside [0, valid_n) is loaded from row 0 and never inserted;
// positions past the end of the list load its last position and are not
// inserted; pad lanes of a short tile hold the tile's first query and store
// nothing. valid_n >= 1 and every row below it lies in a checked segment.
//
// FILTER adds the label predicate of cosine_topk_filtered (row r is eligible
// for query b iff want[b] < 0 || label(r) == want[b]). The tile's wants sit
// in LDS beside pq[]. locate() fetches the row's label with its id (it runs
// one step ahead of the multiply, so neither load is on the critical path;
// a row not to be inserted reads row 0's label), and the shuffle that hands
// rid to the four result rows of a lane carries the label too; eligibility
// is tested per (query, row) at insertion. A tile mixes wants, so row loads
// stay unconditional: a row that no query of the tile wants is still
// gathered and multiplied.
//
// gfx950, hipcc -O3, no spills and no scratch in either instantiation.
// Unfiltered: 116 VGPRs + 4 AGPRs (120 of 512: 4 waves per SIMD); 16,448 B
// static LDS (the merge lists and pq) plus QTILE * (2D + 16) dynamic: 41,280 B
// at D = 768, so LDS sets the occupancy there at 3 blocks = 12 waves per CU
// (3 per SIMD), each with 8 KiB of row loads in flight. Filtered: 120 VGPRs
// + 4 AGPRs (124 of 512, still 4 waves per SIMD); 16,512 B static LDS (pw
// too), 41,344 B at D = 768: the same 3 blocks per CU.
// ---------------------------------------------------------------------------
template <bool FILTER>
__global__ __launch_bounds__(256) void ivf_scan_grouped_kernel(
    const bf16_t* __restrict__ Q, const IvfSegs segs,
    const IvfFilterArg<FILTER> filt, const long* __restrict__ offsets,
    const int* __restrict__ ids, const int* __restrict__ pair_query,
    const int* __restrict__ pair_slot, const int* __restrict__ tile_list,
    const int* __restrict__ tile_first, const int* __restrict__ tile_count,
    const int* __restrict__ n_tiles, int tile0, int B, int sources, int L,
    long n_ids, int D, long valid_n, long tail_lo, long tail_hi, long n_pairs,
    unsigned long long* __restrict__ cand) {
  extern __shared__ char ivf_bq[];  // [QTILE][D/8 + 1] bf16x8: the queries
  __shared__ unsigned long long all[IVF_BATCH_QTILE * 16 * KMAX];
  __shared__ int pq[IVF_BATCH_QTILE];  // query of each pair of the tile
  // FILTER: and the label it wants (< 0: any)
  __shared__ int pw[FILTER ? IVF_BATCH_QTILE : 1];
  const int t = tile0 + blockIdx.y;  // grid.y holds 65535 tiles a launch
  const int tid = threadIdx.x;
  if (t >= *n_tiles) return;
  const int cnt = tile_count[t];
  const int l = tile_list[t];
  const long first = tile_first[t];
  if (cnt < 1 || cnt > IVF_BATCH_QTILE || l < 0 || l > L || first < 0 ||
      first + cnt > n_pairs)
    return;

  long lo, len;
  const bool is_tail = l == L;
  if (is_tail) {
    lo = tail_lo;
    len = tail_hi - tail_lo;
  } else {
    lo = offsets[l];
    long hi = offsets[l + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_ids ? n_ids : hi;
    len = hi - lo;
  }
  // nothing in this slice (block-uniform): the slots stay preset-empty
  if ((long)blockIdx.x * IVF_BATCH_BLOCK_ROWS >= len) return;

  if (tid < IVF_BATCH_QTILE) {
    const int b = pair_query[first + (tid < cnt ? tid : 0)];
    const bool in = b >= 0 && b < B;
    pq[tid] = in ? b : -1;
    if constexpr (FILTER) pw[tid] = in ? filt.want[b] : -1;
  }
  __syncthreads();
  const int pitch = ivf_batch_qpitch(D);
  const int d8 = D / 8;
  for (int i = tid; i < IVF_BATCH_QTILE * d8; i += 256) {
    const int c = i / d8, j = i - c * d8;
    const int b = pq[c] < 0 ? 0 : pq[c];
    ((bf16x8*)ivf_bq)[c * pitch + j] = ((const bf16x8*)(Q + (size_t)b * D))[j];
  }
  __syncthreads();

  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int rr = lane & 15;  // A: row of this wave's 16; B and D: query
  const int g = lane >> 4;   // k group of the operands; D: rows 4g .. 4g+3
  const bf16x8* qrow = (const bf16x8*)ivf_bq + rr * pitch + g;
  const int nlines = D / 64;
  const int ngroups = nlines / IVF_BATCH_GROUP_LINES;
  constexpr int GL = 2 * IVF_BATCH_GROUP_LINES;  // loads (MFMA steps) per group

  // the row position p of this lane: its id (-1: not to be inserted), with
  // FILTER its label (row 0's when not to be inserted), and the address of
  // its row (row 0 when not to be inserted), bf16x8 units
  auto locate = [&](long p, int& rid, int& lab) -> const bf16x8* {
    const long pc = p < len ? p : len - 1;  // clamp loads past the end
    const long r = is_tail ? lo + pc : (long)ids[lo + pc];
    const bool ok = p < len && r >= 0 && r < valid_n;
    const long rc = ok ? r : 0;
    rid = ok ? (int)r : -1;
    const int si = ivf_segment_of(rc, segs.s0, segs.q);
    const long lr = ivf_local_row(rc, segs.s0, segs.q);
    if constexpr (FILTER) lab = filt.labels.base[si][lr];
    return (const bf16x8*)(segs.base[si] + lr * D) + g;
  };

  unsigned long long loc[KMAX];  // sorted desc; 0 = empty
#pragma unroll
  for (int q = 0; q < KMAX; ++q) loc[q] = 0ull;
  const bool live = rr < cnt && pq[rr] >= 0;  // this lane's query is a pair
  int w = -1;                                 // the label that query wants
  if constexpr (FILTER) w = pw[rr];

  const long step = (long)gridDim.x * IVF_BATCH_BLOCK_ROWS;
  long p0 = (long)blockIdx.x * IVF_BATCH_BLOCK_ROWS + wid * 16;
  int rid = -1, rid_next = -1, lab = -1, lab_next = -1;
  const bf16x8* row = locate(p0 + rr, rid, lab);
  bf16x8 cur[GL], nxt[GL];
  if (ngroups > 0) {
#pragma unroll
    for (int v = 0; v < GL; ++v) cur[v] = row[v * 4];
  }
  for (; p0 < len; p0 += step) {
    // the next 16 rows of this wave (a clamped, valid address past the end)
    const bf16x8* row_next = locate(p0 + step + rr, rid_next, lab_next);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int gi = 0; gi < ngroups; ++gi) {
      const bf16x8* src = gi + 1 < ngroups ? row + (gi + 1) * GL * 4 : row_next;
#pragma unroll
      for (int v = 0; v < GL; ++v) nxt[v] = src[v * 4];
#pragma unroll
      for (int v = 0; v < GL; ++v)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            cur[v], qrow[(gi * GL + v) * 4], acc, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < GL; ++v) cur[v] = nxt[v];
    }
    for (int ln = ngroups * IVF_BATCH_GROUP_LINES; ln < nlines; ++ln) {
      const bf16x8 a0 = row[ln * 8], a1 = row[ln * 8 + 4];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qrow[ln * 8], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qrow[ln * 8 + 4], acc, 0,
                                                    0, 0);
    }
    // acc[e]: query rr against row 4g + e of the wave's 16, whose id (and
    // label) lane 4g + e holds
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = __shfl(rid, 4 * g + e, 64);
      const int rl = FILTER ? __shfl(lab, 4 * g + e, 64) : -1;
      const unsigned long long v =
          live && r >= 0 && (w < 0 || rl == w)
              ? ((unsigned long long)enc_f32(acc[e]) << 32) |
                    (unsigned)(0x7fffffff - r)
              : 0ull;
      if (v > loc[KMAX - 1]) {
        loc[KMAX - 1] = v;  // insert at tail, bubble up (array stays sorted)
#pragma unroll
        for (int q = KMAX - 1; q > 0; --q)
          if (loc[q] > loc[q - 1]) {
            const unsigned long long tmp = loc[q];
            loc[q] = loc[q - 1];
            loc[q - 1] = tmp;
          }
      }
    }
    row = row_next;
    rid = rid_next;
    lab = lab_next;
  }

  // per query rr: 16 sorted lists (wave wid, group g) -> the block's top-KMAX
  {
    const int j = wid * 4 + g;
#pragma unroll
    for (int q = 0; q < KMAX; ++q) all[(rr * 16 + j) * KMAX + q] = loc[q];
  }
  __syncthreads();
  for (int stride = 8; stride >= 1; stride >>= 1) {
    if (tid < IVF_BATCH_QTILE * stride) {
      const int c = tid / stride, j = tid - c * stride;
      // two-pointer merge of two sorted-desc KMAX lists -> top KMAX
      // (LDS-indexed, as in emit_merge_topk)
      unsigned long long* pa = all + (size_t)(c * 16 + j) * KMAX;
      const unsigned long long* pb = all + (size_t)(c * 16 + j + stride) * KMAX;
      unsigned long long o[KMAX];
      int ia = 0, ib = 0;
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        const unsigned long long va = pa[ia], vb = pb[ib];
        if (va >= vb) {
          o[q] = va;
          ++ia;
        } else {
          o[q] = vb;
          ++ib;
        }
      }
#pragma unroll
      for (int q = 0; q < KMAX; ++q) pa[q] = o[q];
    }
    __syncthreads();
  }
  if (tid < IVF_BATCH_QTILE * KMAX) {
    const int c = tid / KMAX, e = tid - c * KMAX;
    if (c < cnt && pq[c] >= 0) {
      const int y = pair_slot[first + c];
      if (y >= 0 && y < sources)
        cand[(((size_t)pq[c] * sources + y) * gridDim.x + blockIdx.x) * KMAX + e] =
            all[(size_t)c * 16 * KMAX + e];
    }
  }
}

}  // namespace kakveda
