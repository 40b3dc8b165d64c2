// Kernels of the wide exact search (knn_wide_plan.h): the block-wide
// selection behind emit_merge_topk_wide and the k-th-of-the-partials floor.
//
// Selection. One block of 256 threads per query selects the top k <= 64 of n
// packed entries (order-encoded score << 32 | 0x7fffffff - col: unique per
// column, so descending order of the words is score descending, then column
// ascending; 0 is the empty word). 64 kept entries a thread cannot live in
// registers, so the block sorts tiles of WIDE_SEL_TILE = 1024 words with a
// bitonic network, 4 words a thread (word i of the tile is v[i & 3] of thread
// i >> 2):
//   distance 1, 2      inside the thread's four registers,
//   distance 4..128    between lanes of one wave (lane ^ 1..32): shuffles,
//   distance 256, 512  between waves (thread ^ 64, ^ 128): through 8 KiB of
//                      LDS laid out [register][thread], so every 8-byte access
//                      of a wave is to 64 consecutive words: no bank conflict.
// Three of a sort's 55 steps go through LDS. After the first tile the best 64
// sit in threads 0..15; every further tile keeps them there and loads 960 new
// words into threads 16..255, then sorts again. All register indices are
// compile-time constants: the kernels use no scratch (profiles/wide_topk.md).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_impl.h"
#include "knn_wide_plan.h"

namespace kakveda {

constexpr int WSEL_THREADS = 256;
constexpr int WSEL_PER = WIDE_SEL_TILE / WSEL_THREADS;  // 4 words a thread
constexpr int WSEL_KEEP_THREADS = KWIDE_MAX / WSEL_PER;  // 16 hold the best 64
constexpr int WSEL_FRESH = WIDE_SEL_TILE - KWIDE_MAX;    // 960 new words a tile
static_assert(WSEL_PER == 4 && KWIDE_MAX % WSEL_PER == 0, "4 words a thread");

typedef unsigned long long wsel_t;

// a sits at the lower index of the pair
DEVINL void wsel_cx(wsel_t& a, wsel_t& b, bool desc) {
  const wsel_t hi = a > b ? a : b, lo = a > b ? b : a;
  a = desc ? hi : lo;
  b = desc ? lo : hi;
}

// Sorts the block's 1024 words descending. xch: WIDE_SEL_TILE words of LDS.
// Every thread of the block calls it (it synchronises the block).
DEVINL void wsel_sort_desc(wsel_t (&v)[WSEL_PER], wsel_t* xch, int tid) {
#pragma unroll
  for (int k = 2; k <= WIDE_SEL_TILE; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      // direction of the k-block word tid * 4 + r lies in
      if (j == 1) {
        wsel_cx(v[0], v[1], ((tid * 4) & k) == 0);
        wsel_cx(v[2], v[3], ((tid * 4 + 2) & k) == 0);
      } else if (j == 2) {
        const bool desc = ((tid * 4) & k) == 0;  // k >= 4
        wsel_cx(v[0], v[2], desc);
        wsel_cx(v[1], v[3], desc);
      } else {
        // partner thread tid ^ (j / 4); this thread keeps the larger word
        // iff it is the lower one of a descending pair or the upper one of
        // an ascending pair
        const bool keep_max = (((tid * 4) & k) == 0) == (((tid * 4) & j) == 0);
        wsel_t p[WSEL_PER];
        if (j >= 256) {
          __syncthreads();  // the previous exchange has been read
#pragma unroll
          for (int r = 0; r < WSEL_PER; ++r) xch[r * WSEL_THREADS + tid] = v[r];
          __syncthreads();
#pragma unroll
          for (int r = 0; r < WSEL_PER; ++r)
            p[r] = xch[r * WSEL_THREADS + (tid ^ (j >> 2))];
        } else {
#pragma unroll
          for (int r = 0; r < WSEL_PER; ++r) p[r] = __shfl_xor(v[r], j >> 2, 64);
        }
#pragma unroll
        for (int r = 0; r < WSEL_PER; ++r) {
          const wsel_t hi = v[r] > p[r] ? v[r] : p[r];
          const wsel_t lo = v[r] > p[r] ? p[r] : v[r];
          v[r] = keep_max ? hi : lo;
        }
      }
    }
  }
}

// The best words of load(0..n), sorted descending: afterwards word q of the
// result is v[q & 3] of thread q >> 2 (0 past the n-th). n is block-uniform.
template <class Load>
DEVINL void wsel_select(Load&& load, unsigned n, wsel_t (&v)[WSEL_PER],
                        wsel_t* xch, int tid) {
#pragma unroll
  for (int r = 0; r < WSEL_PER; ++r) {
    const unsigned i = (unsigned)(r * WSEL_THREADS + tid);
    v[r] = i < n ? load(i) : 0ull;
  }
  wsel_sort_desc(v, xch, tid);
  for (unsigned base = WIDE_SEL_TILE; base < n; base += WSEL_FRESH) {
    if (tid >= WSEL_KEEP_THREADS) {
#pragma unroll
      for (int r = 0; r < WSEL_PER; ++r) {
        const unsigned i = base + (unsigned)(r * (WSEL_THREADS - WSEL_KEEP_THREADS) +
                                             tid - WSEL_KEEP_THREADS);
        v[r] = i < n ? load(i) : 0ull;
      }
    }
    wsel_sort_desc(v, xch, tid);
  }
}

// ---------------------------------------------------------------------------
// Wide floor: the k-th largest finite entry of a query's prepass partials
// ([B][entries], entries = pre_grid * KMAX <= 2048; the prepass ran without a
// threshold array, so every entry is the score of a distinct real eligible
// column or the empty (NEG_INF, -1)). Written into rowthr, which the caller
// initialised (init_rowthr): with fewer than k finite entries the row keeps
// that value and the main launch emits every eligible row. grid = B.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(WSEL_THREADS) void wide_floor_kernel(
    const float* __restrict__ ps, const int* __restrict__ pi, int entries, int k,
    unsigned* __restrict__ rowthr) {
  __shared__ wsel_t xch[WIDE_SEL_TILE];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* s = ps + (size_t)row * entries;
  const int* ix = pi + (size_t)row * entries;
  wsel_t v[WSEL_PER];
  wsel_select(
      [&](unsigned i) -> wsel_t {
        const float sc = s[i];
        const int col = ix[i];
        if (col < 0 || !(sc > NEG_INF)) return 0ull;
        return ((wsel_t)enc_f32(sc) << 32) | (unsigned)(0x7fffffff - col);
      },
      (unsigned)entries, v, xch, tid);
#pragma unroll
  for (int r = 0; r < WSEL_PER; ++r)
    if (tid * WSEL_PER + r == k - 1 && v[r] != 0ull)
      rowthr[row] = (unsigned)(v[r] >> 32);
}

// ---------------------------------------------------------------------------
// Wide merge of the emission path: the exact top k <= KWIDE_MAX of a query's
// candidates, score descending then column ascending; ranks past the
// candidates are (-inf, -1). grid = B blocks. cand is [B][stride]; a row has
// ccount[row] entries, or `fixed_cnt` with ccount == nullptr. A row whose
// count exceeds `stride` lost candidates: it is written as pads and the host,
// which reads the largest count back, answers the batch through the sliced
// fallback.
// PACKED writes the packed words instead, columns shifted by col_off (the
// slice's first row), into out_p[row * p_stride + p_off + q]: the sliced
// fallback selects across those with this kernel again.
// ---------------------------------------------------------------------------
template <bool PACKED>
__global__ __launch_bounds__(WSEL_THREADS) void emit_merge_topk_wide(
    const unsigned long long* __restrict__ cand,
    const unsigned* __restrict__ ccount, long stride, unsigned fixed_cnt, int k,
    float* __restrict__ out_s, long* __restrict__ out_i,
    unsigned long long* __restrict__ out_p, long p_stride, long p_off,
    unsigned col_off) {
  __shared__ wsel_t xch[WIDE_SEL_TILE];
  const int row = blockIdx.x, tid = threadIdx.x;
  unsigned cnt = ccount ? ccount[row] : fixed_cnt;
  if (cnt > (unsigned long long)stride) cnt = 0;  // overflowed: all pads
  const unsigned long long* crow = cand + (size_t)row * stride;
  wsel_t v[WSEL_PER];
  wsel_select([&](unsigned i) -> wsel_t { return crow[i]; }, cnt, v, xch, tid);
#pragma unroll
  for (int r = 0; r < WSEL_PER; ++r) {
    const int q = tid * WSEL_PER + r;
    if (q >= k) continue;
    if constexpr (PACKED) {
      // (0x7fffffff - col) - col_off = 0x7fffffff - (col + col_off): no borrow
      out_p[(size_t)row * p_stride + p_off + q] = v[r] ? v[r] - col_off : 0ull;
    } else {
      const bool empty = v[r] == 0ull;
      out_s[(size_t)row * k + q] =
          empty ? -__builtin_inff() : dec_f32((unsigned)(v[r] >> 32));
      out_i[(size_t)row * k + q] =
          empty ? -1L : 0x7fffffffL - (long)(v[r] & 0xffffffffu);
    }
  }
}

}  // namespace kakveda
