// Cluster-routed (IVF) search kernels: centroid scoring and the scan of the
// probed inverted lists. Included by kakveda_kernels.hip after
// kernels_impl.h (bf16x8 / f32x4 / enc_f32 / NEG_INF come from there).
//
// The store's rows stay where they are: a list is a run of row ids in the
// CSR `ids` array and the scan gathers whole rows through it (1,536-B rows
// at D=768; whole-row register gathers of that size read close to the
// streaming rate on CDNA4). Nothing here shares a body with the exact
// kernels, so their machine code does not move.
#pragma once

#include <hip/hip_runtime.h>
#include "ivf_plan.h"

namespace kakveda {

// The store's segments, passed by value: row r lives in segment
// ivf_segment_of(r, s0, q) at local row ivf_local_row(r, s0, q).
struct IvfSegs {
  const bf16_t* base[IVF_MAX_SEGMENTS];
  long s0;  // rows of the first segment
  long q;   // rows of every later segment (1 when there is none)
};

// ---------------------------------------------------------------------------
// ivf_route_scores: dense fp32 scores [B][L] of the queries against the
// bf16 centroids. grid = (ceil(L/32), ceil(B/8)), 256 threads; a block holds
// its <= 8 queries in LDS and streams 32 centroid rows per iteration, 8
// lanes per row (the smallb v4 mapping), then stores every score: plain
// stores, no atomics, no thresholds.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_route_scores(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C,
    float* __restrict__ out, int B, int L, int D) {
  extern __shared__ char ivf_qmem[];  // [nb][D] bf16 queries
  const int b0 = blockIdx.y * 8;
  const int nb = B - b0 < 8 ? B - b0 : 8;
  const bf16x8* qsrc = (const bf16x8*)(Q + (size_t)b0 * D);
  for (int i = threadIdx.x; i < nb * (D / 8); i += 256)
    ((bf16x8*)ivf_qmem)[i] = qsrc[i];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rr = lane >> 3;
  const int ch = lane & 7;
  const int nseg = D / 64;
  for (int r0 = blockIdx.x * 32 + wid * 8; r0 < L; r0 += gridDim.x * 32) {
    const int r = r0 + rr < L ? r0 + rr : L - 1;  // clamp tail loads
    const bf16x8* row = (const bf16x8*)(C + (size_t)r * D);
    f32x4 accv[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) accv[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nseg; ++j) {
      const bf16x8 cv = row[j * 8 + ch];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < nb) {
          const bf16x8 qv =
              ((const bf16x8*)(ivf_qmem + (size_t)b * D * 2))[j * 8 + ch];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            accv[b][e & 3] += (float)cv[e] * (float)qv[e];
        }
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b < nb) {
        float s = (accv[b][0] + accv[b][1]) + (accv[b][2] + accv[b][3]);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (ch == 0 && r0 + rr < L) out[(size_t)(b0 + b) * L + r0 + rr] = s;
      }
    }
  }
}

// The store's per-segment int32 label tensors, parallel to IvfSegs::base and
// addressed by the same ivf_segment_of / ivf_local_row.
struct IvfLabels {
  const int* base[IVF_MAX_SEGMENTS];
};

// The label predicate of a routed scan, passed by value: nothing for the
// unfiltered instantiation, the label tables and the per-query wants (the
// launch's first query first) for the filtered one.
template <bool FILTER> struct IvfFilterArg {};
template <> struct IvfFilterArg<true> {
  IvfLabels labels;
  const int* want;
};

// ---------------------------------------------------------------------------
// ivf_scan_topk_kernel<FILTER>: the routed scan. grid = (slices, nprobe + 1,
// B), 256 threads, D*2 bytes of dynamic LDS (the block's one query).
//
// blockIdx.y < nprobe: the list probes[b][y] (rows ids[offsets[l] ..
// offsets[l+1])); blockIdx.y == nprobe: the contiguous tail [tail_lo,
// tail_hi), the rows appended since the index was built. A block walks its
// source from position blockIdx.x*32 in strides of slices*32, each wave 8
// rows x 8 lanes, so a long list is split over `slices` blocks instead of
// being one wave's whole load.
//
// Every row group keeps a sorted top-KMAX of packed (score bits << 32) |
// (0x7fffffff - row) candidates in registers (its 8 lanes hold the same
// list); one LDS tree merge over the block's 32 groups leaves the block's
// top-KMAX, stored to the block's own slot cand[b][(y*slices + x)*KMAX ..]
// with 0 for "empty". No atomics and no floors: every block writes exactly
// its KMAX entries, and emit_merge_topk (whose empty sentinel is 0) finishes
// over the preset count.
//
// Guards: a probe outside [0, L) is an empty source; list bounds are clamped
// to [0, n_ids]; a row id outside [0, valid_n) is scored from row 0 and never
// inserted (so a snapshot valid_n below some listed ids is safe); positions
// past the end of the source load the source's last position and are not
// inserted. valid_n >= 1 and every row below valid_n lies in a segment the
// host has checked.
//
// FILTER adds the label predicate of cosine_topk_filtered: row r is eligible
// for query b iff want[b] < 0 || label(r) == want[b], and an ineligible row
// is treated exactly as a row id outside [0, valid_n) is: scored from row 0
// if at all, never inserted. want[b] is block-uniform. The id and the label
// of the next iteration's position are fetched while the current rows are
// multiplied, so the chain ids -> label -> row address is off the critical
// path; the label is only read for a position inside the source whose id
// lies in [0, valid_n) (the label tensors have exactly their segments'
// rows). When none of a wave's 8 rows is eligible the wave skips the dot
// product altogether (a wave-uniform branch on the ballot): at 1%
// selectivity 0.99^8 = 92% of the iterations.
//
// gfx950, hipcc -O3, both instantiations: 114 VGPRs, no AGPRs (4 waves per
// SIMD), no spills, no scratch; 2,048 B static LDS (the merge lists) plus
// D*2 dynamic.
// ---------------------------------------------------------------------------
template <bool FILTER>
__global__ __launch_bounds__(256) void ivf_scan_topk_kernel(
    const bf16_t* __restrict__ Q, const IvfSegs segs,
    const IvfFilterArg<FILTER> filt, const long* __restrict__ offsets,
    const int* __restrict__ ids, const int* __restrict__ probes, int nprobe,
    int L, long n_ids, int D, long valid_n, long tail_lo, long tail_hi,
    unsigned long long* __restrict__ cand) {
  extern __shared__ char ivf_qmem[];  // [D] bf16: this block's query
  __shared__ unsigned long long all[32 * KMAX];
  const int b = blockIdx.z;
  const int y = blockIdx.y;
  const int tid = threadIdx.x;
  const bool is_tail = y == nprobe;

  long lo = 0, len = 0;
  if (is_tail) {
    lo = tail_lo;
    len = tail_hi - tail_lo;
  } else {
    const int l = probes[(size_t)b * nprobe + y];
    if (l >= 0 && l < L) {
      lo = offsets[l];
      long hi = offsets[l + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > n_ids ? n_ids : hi;
      len = hi - lo;
    }
  }
  unsigned long long* slot =
      cand + ((size_t)b * gridDim.y * gridDim.x +
              (size_t)y * gridDim.x + blockIdx.x) * KMAX;
  if ((long)blockIdx.x * 32 >= len) {  // nothing in this slice (block-uniform)
    if (tid < KMAX) slot[tid] = 0ull;
    return;
  }
  int w = -1;  // the label this block's query wants (< 0: any)
  if constexpr (FILTER) w = filt.want[b];

  const bf16x8* qsrc = (const bf16x8*)(Q + (size_t)b * D);
  for (int i = tid; i < D / 8; i += 256) ((bf16x8*)ivf_qmem)[i] = qsrc[i];
  __syncthreads();

  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int rr = lane >> 3;  // row within this wave's 8
  const int ch = lane & 7;   // 16-byte chunk within a 128-B segment
  const int nseg = D / 64;
  const bf16x8* qv8 = (const bf16x8*)ivf_qmem;

  // position p of the source: its row id, and whether it is to be inserted
  auto fetch = [&](long p, long& r) -> bool {
    const long pc = p < len ? p : len - 1;  // clamp tail loads
    r = is_tail ? lo + pc : (long)ids[lo + pc];
    bool ok = p < len && r >= 0 && r < valid_n;
    if constexpr (FILTER) {
      if (ok && w >= 0) {
        const int si = ivf_segment_of(r, segs.s0, segs.q);
        ok = filt.labels.base[si][ivf_local_row(r, segs.s0, segs.q)] == w;
      }
    }
    return ok;
  };

  unsigned long long loc[KMAX];  // sorted desc; 0 = empty
#pragma unroll
  for (int q = 0; q < KMAX; ++q) loc[q] = 0ull;

  const long step = (long)gridDim.x * 32;
  long p0 = (long)blockIdx.x * 32 + wid * 8;
  long r = 0, r_next = 0;
  bool ok = false, ok_next = false;
  if constexpr (FILTER) ok = fetch(p0 + rr, r);
  for (; p0 < len; p0 += step) {
    // FILTER: the next iteration's position (clamped, not eligible, past the
    // end); the dot product runs when some row of the wave's 8 is eligible
    if constexpr (FILTER) ok_next = fetch(p0 + step + rr, r_next);
    else ok = fetch(p0 + rr, r);
    if (!FILTER || __ballot(ok) != 0ull) {  // wave-uniform
      const long rc = ok ? r : 0;
      const int si = ivf_segment_of(rc, segs.s0, segs.q);
      const bf16x8* row =
          (const bf16x8*)(segs.base[si] + ivf_local_row(rc, segs.s0, segs.q) * D);
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
      int j = 0;
      for (; j + 4 <= nseg; j += 4) {
        bf16x8 cv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) cv[v] = row[(j + v) * 8 + ch];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const bf16x8 qv = qv8[(j + v) * 8 + ch];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] += (float)cv[v][e] * (float)qv[e];
            acc2[e] += (float)cv[v][e + 4] * (float)qv[e + 4];
          }
        }
      }
      for (; j < nseg; ++j) {  // D % 256 != 0 tail segments
        const bf16x8 cv = row[j * 8 + ch];
        const bf16x8 qv = qv8[j * 8 + ch];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[e] += (float)cv[e] * (float)qv[e];
          acc2[e] += (float)cv[e + 4] * (float)qv[e + 4];
        }
      }
      float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
                ((acc2[0] + acc2[1]) + (acc2[2] + acc2[3]));
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);  // the row group's 8 lanes now agree
      const unsigned long long v =
          ok ? ((unsigned long long)enc_f32(s) << 32) |
                   (unsigned)(0x7fffffff - (int)r)
             : 0ull;
      if (v > loc[KMAX - 1]) {
        loc[KMAX - 1] = v;  // insert at tail, bubble up (array stays sorted)
#pragma unroll
        for (int q = KMAX - 1; q > 0; --q)
          if (loc[q] > loc[q - 1]) {
            const unsigned long long t = loc[q];
            loc[q] = loc[q - 1];
            loc[q - 1] = t;
          }
      }
    }
    if constexpr (FILTER) {
      r = r_next;
      ok = ok_next;
    }
  }

  const int grp = tid >> 3;  // 32 row groups per block
  if (ch == 0) {
#pragma unroll
    for (int q = 0; q < KMAX; ++q) all[grp * KMAX + q] = loc[q];
  }
  __syncthreads();
  for (int stride = 16; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      // two-pointer merge of two sorted-desc KMAX lists -> top KMAX
      // (LDS-indexed, as in emit_merge_topk)
      const unsigned long long* pa = all + (size_t)tid * KMAX;
      const unsigned long long* pb = all + (size_t)(tid + stride) * KMAX;
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
      for (int q = 0; q < KMAX; ++q) all[tid * KMAX + q] = o[q];
    }
    __syncthreads();
  }
  if (tid < KMAX) slot[tid] = all[tid];
}

}  // namespace kakveda
