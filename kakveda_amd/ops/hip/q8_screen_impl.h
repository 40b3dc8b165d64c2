// Int8 screen of the batched exact scan (contract: q8_plan.h "Screening test";
// host dispatch: kakveda_kernels.hip cosine_topk_q8). Pure HIP, no torch.
// Included after kernels_impl.h and q8_impl.h, whose helpers it uses.
//
//   q8_cnorm_kernel          largest row norm of the quantised rows (ingest)
//   q8_screen_prep           per query row: T_r, kappa's term, degenerate flag
//   q8_refresh_floor         between stages: raise the floors, recompute T_r
//   cosine_topk_screen8p_i8  the mode-9 emission kernel over int8 codes
//                            (<false>: without its epilogue, a timing probe)
//   q8_rescore_mfma          bf16 scores of the candidates, bit-equal to the
//                            bf16 emission kernel's
#pragma once

#include <hip/hip_runtime.h>
#include "kernels_impl.h"
#include "q8_impl.h"
#include "q8_plan.h"

namespace kakveda {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Bytes of one wave's (scale, err) slice: 64 columns x 8 bytes.
constexpr int SCREEN_META_WAVE = 512;
// First byte of the slices: past the stashes and the cursor word (32 bytes).
constexpr int SCREEN_META_OFF = ESTASH_OFF + 8 * ESTASH_WAVE + 32;
constexpr int SCREEN_LDS_BYTES = SCREEN_META_OFF + 8 * SCREEN_META_WAVE;
static_assert(SCREEN_LDS_BYTES <= 160 * 1024, "the screen kernel's LDS");
static_assert(SCREEN_META_OFF % 8 == 0, "8-byte reads of the meta slices");

// ---------------------------------------------------------------------------
// cnorm: atomicMax of q8_norm_up(||row||) over rows [0, n) into *cnorm (a
// non-negative float, ordered as its bits). The quantiser's lane mapping: a
// wave covers 8 rows, 8 lanes per row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_cnorm_kernel(
    const bf16_t* __restrict__ rows, long n, int D, float* __restrict__ cnorm) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rr = lane >> 3;
  const int ch = lane & 7;
  const int nseg = D / 64;
  float best = 0.0f;
  for (long r0 = (long)blockIdx.x * 32 + wid * 8; r0 < n;
       r0 += (long)gridDim.x * 32) {
    const long r = r0 + rr < n ? r0 + rr : n - 1;
    const bf16x8* row = (const bf16x8*)(rows + r * D);
    float ss = 0.0f;
    for (int j = 0; j < nseg; ++j) {
      const bf16x8 cv = row[j * 8 + ch];
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = fmaf((float)cv[e], (float)cv[e], ss);
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    ss += __shfl_xor(ss, 4, 64);
    best = fmaxf(best, q8_norm_up(ss, D));
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) best = fmaxf(best, __shfl_xor(best, m, 64));
  if (lane == 0 && best > 0.0f)
    atomicMax((unsigned*)cnorm, __float_as_uint(best));
}

// ---------------------------------------------------------------------------
// Per query row, from its codes and (sq, errq) (q8_quantize_kernel's output)
// and the floor the prepass published: T_r (q8_screen_threshold) into thrT,
// its kappa term into *kappa (atomicMax on the bits of a positive float), and
// a count of degenerate rows (sq == 0) into *degen; such a row gets T = +big
// (it emits nothing: the host sends the batch to the bf16 path). One wave per
// row; *kappa and *degen are zeroed by the host.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_screen_prep(
    const signed char* __restrict__ qcodes, const float* __restrict__ qmeta,
    const unsigned* __restrict__ rowthr, const float* __restrict__ cnorm, int B,
    int D, float* __restrict__ thrT, float* __restrict__ kappa,
    int* __restrict__ degen) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const signed char* row = qcodes + (size_t)r * D;
  int ss = 0;
  for (int i = lane; i < D; i += 64) ss += (int)row[i] * (int)row[i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
  if (lane != 0) return;
  const float sq = qmeta[2 * r], errq = qmeta[2 * r + 1];
  if (!(sq > 0.0f)) {
    thrT[r] = 1e38f;
    atomicAdd(degen, 1);
    return;
  }
  thrT[r] = q8_screen_threshold(dec_f32(rowthr[r]), sq, errq, *cnorm, D);
  atomicMax((unsigned*)kappa,
            __float_as_uint(q8_screen_kappa(q8_code_norm(sq, ss, D), sq)));
}

// ---------------------------------------------------------------------------
// Floor refresh between two stages of the screen (knn_plan.h plan_q8_stages;
// why it stays exact: q8_plan.h "Staged floors"). best_s [B, k] is
// emit_merge_topk's output over every entry the row holds so far, seeds
// included, all with bf16 scores: its last column is the row's k-th best
// exact score. Where that is above the floor, the floor is raised to it;
// T_r is recomputed from the floor in both cases (a degenerate row keeps its
// +big). A row with fewer than k entries, and a row past its capacity (the
// merge wrote no scores for it), reads NEG_INF and raises nothing. kappa and
// the degenerate count do not depend on the floors and stay. One thread per
// row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_refresh_floor(
    const float* __restrict__ best_s, int k, const float* __restrict__ qmeta,
    const float* __restrict__ cnorm, int B, int D,
    unsigned* __restrict__ rowthr, float* __restrict__ thrT) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  unsigned fl = rowthr[r];
  const float kth = best_s[(size_t)r * k + (k - 1)];
  if (kth > NEG_INF && enc_f32(kth) > fl) {
    fl = enc_f32(kth);
    rowthr[r] = fl;
  }
  const float sq = qmeta[2 * r], errq = qmeta[2 * r + 1];
  if (sq > 0.0f)
    thrT[r] = q8_screen_threshold(dec_f32(fl), sq, errq, *cnorm, D);
}

// 16 codes of a staged row: the int8 reading of read_frag's 16 bytes.
DEVINL i32x4 read_frag_i8(const char* lds_tile, int row, int slot) {
  const int s_phys = slot ^ (row & 7);
  return *(const i32x4*)(lds_tile + row * 128 + s_phys * 16);
}

DEVINL void glds4(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

// ---------------------------------------------------------------------------
// The int8 twin of cosine_topk_partial8p_t<9> (kernels_impl.h; its block
// comment holds the schedule and the barrier ledger, which apply here word for
// word). The byte geometry is the parent's: a K window is 128 bytes of a row,
// here 128 codes, so rb = D, nkt = D / 128, and each 16-byte fragment feeds
// one mfma_i32_16x16x64_i8 (A and B use the same lane-to-k mapping and integer
// sums are order-free). Launch geometry, XCD remap, record segments, stash,
// cursor, overflow and poison rules are the parent's; emit_bin consumes the
// segments unchanged.
//
// Epilogue. After the K loop the 128 int32 accumulators are converted in
// place to v = fma(float(acc), sc_c, kappa * err_c) (q8_plan.h
// q8_screen_fast) and the parent's hot sweep and cold path run on v against
// T_r (thrT, q8_screen_prep) in the place of the floors. The record's score
// word carries v; q8_rescore_mfma replaces it.
//
// (scale, err) of the tile's columns. Each wave needs the pairs of its 64
// columns once per column tile. It stages them itself, 512 bytes into a
// private LDS slice behind the cursor word, with two 4-byte global_load_lds
// issued at phase 0 of the tile's LAST window, ahead of that window's A(t+1)
// and B(t+2) pieces. Counted waits: the two loads are older than the window's
// B(t+2) pieces, the newest four outstanding loads at its phase-3
// `vmcnt(4)`, and loads retire in issue order: that wait certifies them, and
// at the chunk tail `vmcnt(0)` does. No other wait is added and no register
// is held across the K loop. The slice is written and read by its own wave
// only: the epilogue's reads are consumed (lgkmcnt) before the wave issues
// the next tile's pair, so it needs no barrier either, and it lies past every
// staging image, stash and the cursor (SCREEN_META_OFF).
// Columns past N - 1 read the pair of column N - 1; the cold path drops them
// as the parent does.
//
// EPILOGUE = true is the production kernel. EPILOGUE = false is the timing
// probe (probe8p_i8 mode 1, the int8 twin of cosine_topk_partial8p_t<1>): the
// same schedule with everything behind the K loop compiled out. It keeps the
// staging, the (scale, err) loads and every wait and barrier, pins the
// accumulators, and writes one zero count per segment and nothing else.
// ---------------------------------------------------------------------------
template <bool EPILOGUE>
__global__ __launch_bounds__(THREADS8, 2) void cosine_topk_screen8p_i8(
    const signed char* __restrict__ Q, const signed char* __restrict__ C,
    const float* __restrict__ meta, const float* __restrict__ thrT,
    const float* __restrict__ kappa, int B, int N, int D, int chunk_tiles,
    int nchunks, unsigned long long* __restrict__ eseg,
    unsigned* __restrict__ esegcnt, long segcap, int tile_first) {
  __shared__ char smem[SCREEN_LDS_BYTES];
  char* const smem0 = smem;
  auto ahalf = [&](int b, int h) -> char* {
    return smem0 + (b * 4 + h) * HALF8;
  };
  auto bhalf = [&](int b, int h) -> char* {
    return smem0 + (b * 4 + 2 + h) * HALF8;
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int wr = wid >> 2;  // row half
  const int wc = wid & 3;   // col quad

  const int nrt = gridDim.y;
  int chunk_id, row_tile;
  if ((gridDim.x & 7) == 0 && gridDim.x * nrt >= 256) {
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = bid & 7;
    const int slot = bid >> 3;
    const int cpx = gridDim.x >> 3;
    chunk_id = xcd * cpx + slot / nrt;
    row_tile = slot % nrt;
  } else {
    chunk_id = blockIdx.x;
    row_tile = blockIdx.y;
  }

  const int row0 = row_tile * BM8;
  const long rb = (long)D;  // bytes of a code row
  const int ntiles_total = (N + BN8 - 1) / BN8;
  const int tile0 = tile_first + chunk_id * chunk_tiles;
  const int tiles_here = min(chunk_tiles, ntiles_total - tile0);
  const int nkt = D / Q8_SEG;  // windows per col tile

  char* const st = smem0 + ESTASH_OFF + wid * ESTASH_WAVE;
  unsigned* const ecursor = (unsigned*)(smem0 + ESTASH_OFF + 8 * ESTASH_WAVE);
  char* const mslice = smem0 + SCREEN_META_OFF + wid * SCREEN_META_WAVE;
  const size_t segid = (size_t)row_tile * nchunks + chunk_id;

  if (tid == 0) *ecursor = 0u;
  __syncthreads();
  if (tiles_here <= 0) {  // padded chunk: an empty segment
    if (tid == 0) esegcnt[segid] = 0u;
    return;
  }

  auto stage_a_piece = [&](int t, int i) {  // i in 0..3
    const int kt = t % nkt;
    const int jt = t / nkt;
    if (jt >= tiles_here) return;
    char* img = ahalf(t & 1, wr);
    const int off = wc * 4096 + i * 1024;
    const int P = off + lane * 16;
    const int r = P >> 7;
    const int s_log = ((P >> 4) & 7) ^ (r & 7);
    const int gr = min(row0 + wr * 128 + r, B - 1);
    glds16((const char*)Q + (size_t)gr * rb + kt * 128 + s_log * 16, img + off);
  };
  auto stage_b_piece = [&](int t, int i) {
    const int kt = t % nkt;
    const int jt = t / nkt;
    if (jt >= tiles_here) return;
    char* img = bhalf(t & 1, wc >> 1);
    const int off = ((wc & 1) * 64 + wr * 32) * 128 + i * 1024;
    const int P = off + lane * 16;
    const int r = P >> 7;
    const int s_log = ((P >> 4) & 7) ^ (r & 7);
    const int col_base = (tile0 + jt) * BN8 + (wc >> 1) * 128;
    const int gr = min(col_base + r, N - 1);
    glds16((const char*)C + (size_t)gr * rb + kt * 128 + s_log * 16, img + off);
  };
  // the (scale, err) pairs of this wave's 64 columns of tile jt: dwords
  // lane and lane + 64 of the 128 (see the block comment)
  auto stage_meta = [&](int jt) {
    const int colw0 = (tile0 + jt) * BN8 + wc * 64;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = h * 64 + lane;
      const int col = min(colw0 + (i >> 1), N - 1);
      glds4(meta + (size_t)col * 2 + (i & 1), mslice + h * 256);
    }
  };

  // ---- prologue: K-tile 0 fully + B(1); then steady schedule ------------
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_a_piece(0, i);
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_b_piece(0, i);
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_b_piece(1, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger (parent's ledger)

  const int total_windows = tiles_here * nkt;

  // T_r of this wave-half's rows (rows beyond B get +big so clamped-row
  // garbage never flags) and kappa, read once per block: both are static
  // under this launch.
  float thr0, thr1;
  {
    const int r0g = row0 + wr * 128 + lane;
    thr0 = (r0g < B) ? thrT[r0g] : 1e38f;
    thr1 = (r0g + 64 < B) ? thrT[r0g + 64] : 1e38f;
  }
  const float kap = *kappa;
  // a use here, right behind the prologue's full drain: the compiler's wait
  // for the three loads lands before the tile loop, not inside it
  asm volatile("" ::"v"(thr0), "v"(thr1), "v"(kap));

  for (int j = 0; j < tiles_here; ++j) {
    const int col0 = (tile0 + j) * BN8;

    i32x4 acc[8][4];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = i32x4{0, 0, 0, 0};

    for (int kt = 0; kt < nkt; ++kt) {
      const int t = j * nkt + kt;  // global window index
      const char* Ai = ahalf(t & 1, wr);
      const char* Bi = bhalf(t & 1, wc >> 1) + ((wc & 1) * 64) * 128;
      i32x4 bf[4][2];
#pragma unroll
      for (int qm = 0; qm < 4; ++qm) {
        i32x4 af[2][2];
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            af[mm][kk] = read_frag_i8(Ai, (qm * 2 + mm) * 16 + cl, kk * 4 + g);
        if (qm == 0) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
              bf[n][kk] = read_frag_i8(Bi, n * 16 + cl, kk * 4 + g);
        }
        // ---- staging issues (the parent's staggered schedule)
        if (qm == 0) {
          // the tile's (scale, err) pairs go first: older than this
          // window's A(t+1) and B(t+2), certified by its phase-3 wait
          if (kt == nkt - 1) stage_meta(j);
          if (t + 1 < total_windows) {
            stage_a_piece(t + 1, 0);
            stage_a_piece(t + 1, 1);
          }
        } else if (qm == 1 && t + 1 < total_windows) {
          stage_a_piece(t + 1, 2);
          stage_a_piece(t + 1, 3);
        } else if (qm == 2 && t + 2 < total_windows) {
          stage_b_piece(t + 2, 0);
          stage_b_piece(t + 2, 1);
        } else if (qm == 3) {
          if (t + 2 < total_windows) {
            stage_b_piece(t + 2, 2);
            stage_b_piece(t + 2, 3);
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int n = 0; n < 4; ++n)
              acc[qm * 2 + mm][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                  af[mm][kk], bf[n][kk], acc[qm * 2 + mm][n], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();  // read-retirement vs next glds
      }
    }
    // group 0's make-up barrier pairs with group 1's last phase barrier
    if (wr == 0 && j == tiles_here - 1) __builtin_amdgcn_s_barrier();

    if constexpr (!EPILOGUE) {
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) asm volatile("" ::"v"(acc[m][n]));
      continue;
    }

    // ---- acc -> v, in place (bits of the float in the int register) ------
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const f32x2 mt = *(const f32x2*)(mslice + (n * 16 + cl) * 8);
      const float sc = mt[0];
      const float ke = kap * mt[1];
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          acc[m][n][reg] =
              __float_as_int(fmaf((float)acc[m][n][reg], sc, ke));
    }
    auto V = [&](int m, int n, int reg) -> float {
      return __int_as_float(acc[m][n][reg]);
    };

    // ---- the parent's threshold-emission epilogue on v against T_r -------
    const int colb = col0 + wc * 64 + cl;
    unsigned qm32 = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rl = m * 16 + g * 4 + reg;  // 0..127 within this half
        const float thr = __shfl(m >= 4 ? thr1 : thr0, rl & 63, 64);
        const float gmax = fmaxf(fmaxf(V(m, 0, reg), V(m, 1, reg)),
                                 fmaxf(V(m, 2, reg), V(m, 3, reg)));
        if (__ballot(gmax >= thr))  // uniform
          qm32 |= 1u << (m * 4 + reg);
      }
    }
    if (__builtin_expect(qm32 != 0, 0)) {  // uniform cold path
      const int rowl0 = wr * 128;               // row within the tile
      const int colc = j * BN8 + wc * 64 + cl;  // column within chunk
      unsigned long long* const seg = eseg + segid * (size_t)segcap;
      unsigned rem = qm32;
      do {
        int ng = 0;
        unsigned gids = 0;  // 5 bits of (m*4+reg) per stashed slot
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const unsigned bit = 1u << (m * 4 + reg);
            if ((rem & bit) && ng < EGCAP) {
              *(f32x4*)(st + ng * 1024 + lane * 16) =
                  f32x4{V(m, 0, reg), V(m, 1, reg), V(m, 2, reg), V(m, 3, reg)};
              gids |= (unsigned)(m * 4 + reg) << (5 * ng);
              rem &= ~bit;
              ++ng;
            }
          }
        }
        for (int i = 0; i < ng; ++i) {
          const int gid = (int)((gids >> (5 * i)) & 31u);
          const int m = gid >> 2, reg = gid & 3;
          const int rl = m * 16 + g * 4 + reg;  // 0..127 within the half
          const float thr = __shfl(m >= 4 ? thr1 : thr0, rl & 63, 64);
          const f32x4 v = *(const f32x4*)(st + i * 1024 + lane * 16);
          const bool rowok = row0 + rowl0 + rl < B;
          const bool q0 = rowok && v[0] >= thr && colb < N;
          const bool q1 = rowok && v[1] >= thr && colb + 16 < N;
          const bool q2 = rowok && v[2] >= thr && colb + 32 < N;
          const bool q3 = rowok && v[3] >= thr && colb + 48 < N;
          const unsigned long long b0 = __ballot(q0), b1 = __ballot(q1),
                                   b2 = __ballot(q2), b3 = __ballot(q3);
          const unsigned c0 = __popcll(b0), c1 = __popcll(b1),
                         c2 = __popcll(b2), c3 = __popcll(b3);
          const unsigned total = c0 + c1 + c2 + c3;
          if (total == 0) continue;  // uniform
          unsigned base = 0;
          if (lane == 0) base = lds_add_rtn(ecursor, total);
          base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
          auto put = [&](bool q, unsigned long long bal, unsigned off, float sc,
                         int n) {
            const unsigned pos =
                base + off +
                __builtin_amdgcn_mbcnt_hi(
                    (unsigned)(bal >> 32),
                    __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
            if (q && pos < (unsigned)segcap)
              seg[pos] = eseg_record(sc, rowl0 + rl, colc + n * 16);
          };
          put(q0, b0, 0u, v[0], 0);
          put(q1, b1, c0, v[1], 1);
          put(q2, b2, c0 + c1, v[2], 2);
          put(q3, b3, c0 + c1 + c2, v[3], 3);
        }
      } while (rem != 0);
    }
  }

  // publish the segment's true record count (it may exceed segcap: emit_bin
  // then poisons the row tile)
  __syncthreads();
  if (tid == 0) esegcnt[segid] = *ecursor;
}

// ---------------------------------------------------------------------------
// Rescore: entries [first[b], min(ccount[b], cap)) of row b of the candidate
// buffer get the bf16 score of (query b, their column), packed as emit_bin
// packs. Entries below first[b] are emit_seed's and already hold bf16 scores.
//
// Bit-equal to cosine_topk_partial8p_t and the prepass: there a score is one
// zero-initialised chain of mfma_f32_16x16x32_bf16 over the K slices of 32 in
// ascending order, the query fragment as A and the corpus fragment as B, lane
// (l & 15, l >> 4) holding elements 8 (l >> 4) .. + 8 of the slice on both
// sides. Here a wave takes 16 candidates of one query: lane (cl, g) feeds the
// same 8 elements of the query as A (every row of the 16 x 16 block is the
// query) and of candidate cl's row as B, gathered from global memory straight
// into the operand registers. Every output row is the wanted score; lanes
// 0..15 (g = 0, register 0: row 0, column cl) store it. The lanes of a partly
// filled group of 16 reread the last candidate and store nothing; only the
// low word (the column) of an entry is read.
// grid = (blocks, B).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q8_rescore_mfma(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C, int N, int D,
    unsigned long long* __restrict__ cand, const unsigned* __restrict__ ccount,
    const unsigned* __restrict__ first, long ccap) {
  const int b = blockIdx.y;
  const long total = (long)ccount[b];
  const long cnt = total < ccap ? total : ccap;
  const long lo0 = first ? (long)first[b] : 0;
  if (cnt <= lo0) return;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int cl = lane & 15;
  const int g = lane >> 4;
  const int nsl = D / 32;  // K slices
  const bf16x8* qb = (const bf16x8*)(Q + (size_t)b * D) + g;
  unsigned long long* crow = cand + (size_t)b * ccap;
  for (long i0 = lo0 + (long)blockIdx.x * 64 + wid * 16; i0 < cnt;
       i0 += (long)gridDim.x * 64) {
    const bool live = i0 + cl < cnt;
    const long i = live ? i0 + cl : cnt - 1;
    const unsigned lo = ((const unsigned*)crow)[2 * i];
    // a row tile poisoned by an overflowed segment counts past its stored
    // entries: what lies there is not a column, so the address is clamped
    // (the batch is answered by the bf16 search anyway)
    long col = 0x7fffffffL - (long)lo;
    col = col < 0 ? 0 : col >= N ? N - 1 : col;
    const bf16x8* row = (const bf16x8*)(C + col * D) + g;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int s = 0; s < nsl; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qb[s * 4], row[s * 4], acc,
                                                    0, 0, 0);
    if (live && g == 0)
      crow[i] = ((unsigned long long)enc_f32(acc[0]) << 32) | lo;
  }
}

}  // namespace kakveda
