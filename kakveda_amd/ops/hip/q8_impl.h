// Int8 row mirror: the quantiser and the two kernels of the half-byte exact
// small-batch search (contract: q8_plan.h; host dispatch: kakveda_kernels.hip
// cosine_topk_q8). Pure HIP, no torch. Included after kernels_impl.h, whose
// helpers (enc_f32, streaming_floor, the vector typedefs) it uses.
#pragma once

#include <hip/hip_runtime.h>
#include "kernels_impl.h"
#include "q8_plan.h"

namespace kakveda {

// Segments q8_emit_kernel loads ahead of the FMAs, and the waves per SIMD its
// registers are bounded to. Groups of 4 (v4's) want 256 VGPRs, one wave per
// SIMD, and spill 1.2 KiB per lane under any tighter bound; groups of 2 under
// a rolled outer loop compile to 116 VGPRs, no scratch, 4 waves per SIMD, so
// the loads in flight per SIMD (2 x 4) match v4's (4 x 3 at 134 VGPRs) to
// within a third while every load carries twice the rows' elements.
constexpr int Q8_GROUP = 2;
constexpr int Q8_EMIT_WAVES = 4;

typedef signed char i8x16 __attribute__((ext_vector_type(16)));
typedef signed char i8x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------
// Quantiser: rows [n, D] bf16 -> codes[first_row + i], meta[first_row + i].
// The v4 mapping: a wave covers 8 consecutive rows with 8 lanes per row, lane
// ch owning the 16-byte chunk ch of every 128-byte bf16 segment, so each load
// instruction touches 8 full lines. Three passes over the row (amax, codes,
// residual norm folded into the second); the second read of the 2D-byte row
// hits L2. Bandwidth-bound: 2D bytes read and D + 8 written per row. Tail
// rows are clamped for the loads and guarded at the stores.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_quantize_kernel(
    const bf16_t* __restrict__ rows, long n, int D,
    signed char* __restrict__ codes, float* __restrict__ meta, long first_row) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rr = lane >> 3;
  const int ch = lane & 7;
  const int nseg = D / 64;  // 128-byte bf16 segments
  for (long r0 = (long)blockIdx.x * 32 + wid * 8; r0 < n;
       r0 += (long)gridDim.x * 32) {
    const bool live = r0 + rr < n;
    const long r = live ? r0 + rr : n - 1;
    const bf16x8* row = (const bf16x8*)(rows + r * D);
    float amax = 0.0f;
    for (int j = 0; j < nseg; ++j) {
      const bf16x8 cv = row[j * 8 + ch];
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)cv[e]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
    const Q8Scale qs = q8_scale(amax);
    float ss = 0.0f;
    i8x8* out = (i8x8*)(codes + (first_row + r) * D);
    for (int j = 0; j < nseg; ++j) {
      const bf16x8 cv = row[j * 8 + ch];
      i8x8 nv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float c = (float)cv[e];
        const signed char q = q8_code(c, qs.inv);
        nv[e] = q;
        const float d = fmaf(-qs.scale, (float)q, c);
        ss = fmaf(d, d, ss);
      }
      if (live) out[j * 8 + ch] = nv;
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    ss += __shfl_xor(ss, 4, 64);
    if (live && ch == 0) {
      f32x2 m;
      m[0] = qs.scale;
      m[1] = q8_err(sqrtf(ss), amax, qs.scale, D);
      ((f32x2*)meta)[first_row + r] = m;
    }
  }
}

// ---------------------------------------------------------------------------
// Stage 1 of the q8 search (B <= 8): smallb_emit_kernel_v4 over the int8
// mirror. Same lane mapping (8 consecutive rows per wave, 8 lanes per row);
// a 128-byte segment of an int8 row is 128 codes, 16 per lane, so the scan
// reads D + 8 bytes per row where v4 reads 2D.
//
// Queries sit in LDS as FP32 ([B][D], 24 KiB at B = 8, D = 768). The code is
// converted once per element and shared by the B queries; with bf16 queries
// every (query, element) pair would pay its own bf16 -> fp32 unpack next to
// its FMA, which doubles the VALU work of a loop that is VALU-bound from a
// few queries on. The price is LDS reads of 32 instead of 16 bytes per 8
// elements and query, all of them conflict-free (the 8 lanes of a row read
// 8 x 64 contiguous bytes, the 8 rows of the wave the same addresses).
//
// Emission test and why it loses nothing. Let c be the bf16 row, c^ = scale *
// n its mirror, q a query, floor the streaming floor v4 compares against.
//   (1) |q.c - q.c^| <= ||q|| * ||c - c^|| <= qn * err       (Cauchy-Schwarz;
//       qn >= ||q|| and err >= ||c - c^||, both rounded up)
//   (2) v4's score s4 is an fp32 sum of exact products: s4 <= q.c + D * 2^-24
//       for unit rows (kernels_impl.h streaming_floor).
//   (3) s8 = scale * sum_i q_i n_i: the products q_i n_i are exact in fp32 (8
//       by 7 significant bits), their fp32 sum is within (D - 1) * 2^-24 *
//       sum |q_i n_i| and the multiply adds one rounding, so
//       s8 >= q.c^ - D * 2^-24 * (||q|| * ||c^||) * (1 + 2^-24), and
//       ||c^|| <= 1 + err: s8 >= q.c^ - D * 2^-24 * 1.02 for unit rows.
// So s4 >= floor implies s8 + qn * err + 2.02 * D * 2^-24 >= floor; the test
// adds D * 2^-22 (q8_slack), which also covers the two roundings of its own
// left-hand side. Every row v4 would emit is emitted here; stage 2 replaces
// each candidate's score by v4's own, so what emit_merge_topk sees is a
// superset of v4's candidates with v4's keys.
//
// FILTER, labels, want: as smallb_emit_kernel_v4.
// ---------------------------------------------------------------------------
template <bool FILTER = false>
__global__ __launch_bounds__(256, Q8_EMIT_WAVES) void q8_emit_kernel(
    const bf16_t* __restrict__ Q, const signed char* __restrict__ codes,
    const float* __restrict__ meta, int B, long N, int D,
    const unsigned* __restrict__ rowthr, unsigned long long* __restrict__ cand,
    unsigned* __restrict__ ccount, long ccap,
    const int* __restrict__ labels = nullptr,
    const int* __restrict__ want = nullptr) {
  extern __shared__ char qmem[];  // [B][D] fp32 queries
  __shared__ float fl[8];
  __shared__ float qn[8];
  float* qf = (float*)qmem;
  const int* wl = nullptr;
  (void)wl;
  for (int i = threadIdx.x; i < B * (D / 8); i += 256) {
    const bf16x8 v = ((const bf16x8*)Q)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[i * 8 + e] = (float)v[e];
  }
  if (threadIdx.x < B) fl[threadIdx.x] = streaming_floor(rowthr[threadIdx.x], D);
  if constexpr (FILTER) {
    __shared__ int wls[8];
    if (threadIdx.x < B) wls[threadIdx.x] = want[threadIdx.x];
    wl = wls;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  // qn_b = ||q_b|| rounded up (q8_plan.h q8_roundup: an fp32 norm of D terms)
  for (int b = wid; b < B; b += 4) {
    float ss = 0.0f;
    for (int i = lane; i < D; i += 64) ss = fmaf(qf[b * D + i], qf[b * D + i], ss);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
    if (lane == 0) qn[b] = sqrtf(ss) * q8_roundup(D) + Q8_ERR_ABS;
  }
  __syncthreads();

  const int rr = lane >> 3;  // row within this wave's 8
  const int ch = lane & 7;   // 16-byte chunk within a 128-byte segment
  const int nseg = D / Q8_SEG;
  const float slack = q8_slack(D);
  for (long r0 = (long)blockIdx.x * 32 + wid * 8; r0 < N;
       r0 += (long)gridDim.x * 32) {
    const bool live = r0 + rr < N;
    const long r = live ? r0 + rr : N - 1;  // clamp tail loads
    const i8x16* row = (const i8x16*)(codes + r * D);
    f32x2 m = f32x2{0.f, 0.f};
    int lab = -1;
    (void)lab;
    if (ch == 0) {
      m = ((const f32x2*)meta)[r];
      if constexpr (FILTER) {
        if (live) lab = labels[r];
      }
    }
    f32x4 accv[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) accv[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int j = 0;
#pragma unroll 1
    for (; j + Q8_GROUP <= nseg; j += Q8_GROUP) {
      i8x16 cv[Q8_GROUP];
#pragma unroll
      for (int v = 0; v < Q8_GROUP; ++v) cv[v] = row[(j + v) * 8 + ch];
#pragma unroll
      for (int v = 0; v < Q8_GROUP; ++v) {
        float cf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) cf[e] = (float)cv[v][e];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if (b < B) {
            const f32x4* qb = (const f32x4*)(qf + (size_t)b * D) + ((j + v) * 8 + ch) * 4;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const f32x4 qv = qb[h];
#pragma unroll
              for (int e = 0; e < 4; ++e) accv[b][e] += cf[h * 4 + e] * qv[e];
            }
          }
        }
      }
    }
    for (; j < nseg; ++j) {  // segments past the last whole group
      const i8x16 cv = row[j * 8 + ch];
      float cf[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) cf[e] = (float)cv[e];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < B) {
          const f32x4* qb = (const f32x4*)(qf + (size_t)b * D) + (j * 8 + ch) * 4;
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const f32x4 qv = qb[h];
#pragma unroll
            for (int e = 0; e < 4; ++e) accv[b][e] += cf[h * 4 + e] * qv[e];
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b < B) {
        float s = (accv[b][0] + accv[b][1]) + (accv[b][2] + accv[b][3]);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);  // the row group's 8 lanes now agree
        bool eligible = true;
        if constexpr (FILTER) eligible = wl[b] < 0 || lab == wl[b];
        const float s8 = m[0] * s;
        if (ch == 0 && live && eligible &&
            fmaf(qn[b], m[1], s8) + slack >= fl[b]) {
          const unsigned pos = atomicAdd(&ccount[b], 1u);
          if (pos < (unsigned)ccap)
            cand[(size_t)b * ccap + pos] =
                ((unsigned long long)enc_f32(s8) << 32) |
                (unsigned)(0x7fffffff - (int)(r0 + rr));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Stage 2: rescore every emitted (query, row) pair from the bf16 row with
// smallb_emit_kernel_v4's arithmetic - per lane the same accv[e & 3] chains
// over the same segments in the same order, the same pairwise fold and the
// same shfl_xor 1, 2, 4 reduction over the row's 8 lanes - and overwrite the
// candidate's key with (enc_f32(score), 0x7fffffff - row). No floor test:
// every candidate is rescored, and the merge sees bf16 scores only.
// grid = (blocks, B); a wave takes 8 candidates at a time, 8 lanes each.
// Pairs past min(ccount[b], cap) are not touched; the clamped lanes of a
// partly filled group of 8 reread the last pair and store nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_rescore(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C, int D,
    unsigned long long* __restrict__ cand, const unsigned* __restrict__ ccount,
    long ccap) {
  const int b = blockIdx.y;
  const unsigned total = ccount[b];
  const long cnt = (long)total < ccap ? (long)total : ccap;
  if (cnt <= 0) return;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rr = lane >> 3;
  const int ch = lane & 7;
  const int nseg = D / 64;
  const bf16x8* qb = (const bf16x8*)(Q + (size_t)b * D);
  unsigned long long* crow = cand + (size_t)b * ccap;
  for (long i0 = (long)blockIdx.x * 32 + wid * 8; i0 < cnt;
       i0 += (long)gridDim.x * 32) {
    const bool live = i0 + rr < cnt;
    const long i = live ? i0 + rr : cnt - 1;
    // the low word (the row) only: another group may be storing this key's
    // high word right now when this lane is a clamped one
    const unsigned lo = ((const unsigned*)crow)[2 * i];
    const long r = 0x7fffffffL - (long)lo;
    const bf16x8* row = (const bf16x8*)(C + r * D);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nseg; ++j) {
      const bf16x8 cv = row[j * 8 + ch];
      const bf16x8 qv = qb[j * 8 + ch];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e & 3] += (float)cv[e] * (float)qv[e];
    }
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (live && ch == 0)
      crow[i] = ((unsigned long long)enc_f32(s) << 32) | lo;
  }
}

}  // namespace kakveda
