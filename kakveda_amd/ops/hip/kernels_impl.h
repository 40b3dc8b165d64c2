// Device-code implementation shared by the torch extension and the
// standalone perf probe (tools/knn_probe.hip). Pure HIP, no torch.
#pragma once
// kakveda-amd CDNA4 (gfx950 / MI355X) kernels.
//
// The hot path of the failure-intelligence engine: batched cosine top-k of
// query fingerprints against the HBM3E-resident GFKB store. Replaces the
// reference's per-request TF-IDF refit + full-corpus cosine
// (reference: services/shared/similarity.py:14-20, services/gfkb/app.py:79-102).
//
// Design (MI355X-first; "guide" tags such as T1, G13 or rule 21 name
// techniques of the CDNA HIP programming guide this was written against):
// - cosine_topk_partial_t: one workgroup owns a (128-query row tile x corpus
//   chunk). Per 128-column tile it runs an MFMA GEMM (mfma_f32_16x16x32_bf16,
//   4 waves x 64x64 output each, BK=64 K-steps, double-buffered LDS staged
//   with global_load_lds_dwordx4) and feeds the scores into an LDS-resident
//   per-row top-k list via a threshold-filtered, wave-serialised insert.
//   The per-chunk top-k lists are written out as partials.
// - topk_merge: per query row, merges the per-chunk partial lists.
// - l2normalize rows, embedding_bag: bandwidth-bound helpers (vectorised
//   bf16x8 loads per guide G13).
//
// Wavefront = 64 everywhere; LDS staging uses the lane-linear glds image
// with the XOR slot swizzle applied on the *source* address and on the
// *read* address (guide rule 21).

#include <hip/hip_runtime.h>
#include <cstdint>
#include "knn_plan.h"  // BM/BN/BM8/BN8/KMAX: shared with the host dispatch plan

#define DEVINL __device__ __forceinline__

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace kakveda {

constexpr int BK = 64;         // K depth per LDS stage
constexpr int THREADS = 256;   // 4 waves
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB (BM==BN)
constexpr float NEG_INF = -1e30f;

DEVINL void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// Order-preserving f32 <-> u32 encoding so float thresholds can be shared
// through u32 atomicMax (x < y  <=>  enc(x) < enc(y)).
DEVINL unsigned enc_f32(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DEVINL float dec_f32(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__global__ void init_rowthr(unsigned* thr, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) thr[i] = enc_f32(NEG_INF);
}

// Lower every published threshold strictly below its value. The list
// kernels prune with a strict `score > threshold`, which is exact while the
// list that backs a published minimum survives: a column tied with that
// minimum is as good as a kept one. The warming prepass's lists do NOT
// survive (the main launch overwrites their partial slots), so after it a
// column EQUAL to the threshold would be in nobody's list: 8 bit-identical
// rows in one prepass list vanished from the result, and 8 distinct
// near-duplicates at k = 8 lost the 8th. The main launch recomputes the
// prepass's scores bit for bit (same kernel, same column -> lane mapping),
// so any strictly lower threshold re-admits them; this steps down by about
// two ulps, and from +-0 to -FLT_MIN (a one-code step from +0 lands on -0,
// which compares equal to +0). NEG_INF (nothing published) stays.
__global__ void relax_rowthr(unsigned* thr, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = dec_f32(thr[i]);
    if (v > NEG_INF)
      thr[i] = enc_f32(v - fmaxf(fabsf(v) * 0x1p-23f, 1.17549435e-38f));
  }
}

// Stage one [128 rows x 64 k] bf16 tile into LDS via global_load_lds.
// LDS image is lane-linear; the 16-byte slot index is XOR-swizzled with
// (row & 7) on the global source so the fragment reads (which apply the
// same XOR) are bank-conflict-reduced (guide T2 / rule 21).
DEVINL void stage_tile(const bf16_t* __restrict__ src, int row0, int row_max,
                       long row_bytes, int ktile_byte, char* lds_tile,
                       int wid, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lds_off = wid * 4096 + i * 1024;
    const int P = lds_off + lane * 16;     // this lane's physical LDS byte
    const int r = P >> 7;                  // tile row (128 B per row)
    const int s_phys = (P >> 4) & 7;       // 16-B slot within the row
    const int s_log = s_phys ^ (r & 7);    // inverse swizzle on the source
    const int gr = min(row0 + r, row_max);
    const char* gaddr =
        (const char*)src + (size_t)gr * row_bytes + ktile_byte + s_log * 16;
    glds16(gaddr, lds_tile + lds_off);
  }
}

// Read an MFMA fragment (8 contiguous bf16 along k) from a staged tile.
// row: tile-local row; slot: logical 16-B k-slot (0..7).
DEVINL bf16x8 read_frag(const char* lds_tile, int row, int slot) {
  const int s_phys = slot ^ (row & 7);
  return *(const bf16x8*)(lds_tile + row * 128 + s_phys * 16);
}

// Extraction for one qualifying (row, col-half): deliberately __noinline__
// so the 16 unrolled epilogue bodies don't get their candidate values
// hoisted live simultaneously (measured: inlining costs 100+ VGPRs and
// ~850 B/lane of scratch spill). Each loop iteration a wave argmax reduce
// picks the group's best remaining candidate; its lane inserts it.
template <bool PUBLISH>
__device__ __noinline__ void topk_extract_group(
    volatile float* vsc, volatile int* vix, int lbase, float rwarm,
    float w0, float w1, float w2, float w3, int colb, int N_unused, int lane,
    int g, unsigned* rowthr, int growp1) {
  float rmin = fmaxf(vsc[lbase], rwarm);
  while (true) {
    float b = w0;
    int bn = 0;
    if (w1 > b) { b = w1; bn = 1; }
    if (w2 > b) { b = w2; bn = 2; }
    if (w3 > b) { b = w3; bn = 3; }
    float mv = (b > rmin) ? b : NEG_INF;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      mv = fmaxf(mv, __shfl_xor(mv, off, 64));
    if (mv <= NEG_INF) break;
    const unsigned long long winners =
        __ballot(b == mv && b > rmin) & (0xFFFFull << (g * 16));
    const int leader = __ffsll(winners) - 1;
    if (lane == leader) {
      float nmn = mv;
      int nmp = 0;
#pragma unroll
      for (int q = 1; q < KMAX; ++q) {
        const float s = vsc[lbase + q];
        if (s < nmn) { nmn = s; nmp = q; }
      }
      const int gcol = colb + bn * 16;
      if (nmp == 0) {
        vsc[lbase] = mv;
        vix[lbase] = gcol;
      } else {
        const int mi2 = vix[lbase + nmp];
        vsc[lbase] = nmn;
        vix[lbase] = mi2;
        vsc[lbase + nmp] = mv;
        vix[lbase + nmp] = gcol;
      }
      if (bn == 0) w0 = NEG_INF;
      else if (bn == 1) w1 = NEG_INF;
      else if (bn == 2) w2 = NEG_INF;
      else w3 = NEG_INF;
      if (PUBLISH && rowthr != nullptr && nmn > NEG_INF && growp1 > 0)
        atomicMax(&rowthr[growp1 - 1], enc_f32(nmn));
    }
    rmin = fmaxf(vsc[lbase], rwarm);  // same-wave LDS order
  }
}

// ---------------------------------------------------------------------------
// Fused score GEMM + per-chunk top-k.
//   grid.x = nchunks, grid.y = ceil(B/128), block = 256 threads.
//   partial_score/partial_idx: [B][nchunks][KMAX]
// ---------------------------------------------------------------------------
// EPI_MODE (numbering is historical; the pruned variants and their
// verdicts are in profiles/knn_kernel_history.md):
//   0  full top-k: volatile-LDS thresholds, call-only extraction
//   1  GEMM-only ablation (tools/knn_probe.hip)
//   4  argmax (k=1 fast path: per-row max, no lists/extraction)
//   8  register-cached thresholds + call-only extraction
//   9  = 8 + inline single-insert fast path
//   11 = 9 with a masked-__ballot pre-check instead of the 4-deep
//      shfl_xor max reduce — the PRODUCTION DEFAULT (754 TF vs 642 for
//      mode 0 at B=4096 x N=2M)
// `stats` is unused (it belonged to a pruned counting mode) and stays in
// the signature so kernarg offsets do not move.
//
// FILTER (mode 11 only) is the label-filtered search: corpus column j is
// eligible for query row b iff want[b] < 0 || labels[j] == want[b]
// (labels i32 [N], want i32 [B]). An ineligible column's score becomes
// NEG_INF exactly where out-of-range columns (col >= N) already do, ahead
// of the ballot pre-check, so the lists only ever hold eligible columns
// and everything downstream (insert, rowthr publish, partial write) is
// unchanged: a full list's minimum is a lower bound of that row's k-th
// best ELIGIBLE score. INVARIANT: every launch that reads or publishes
// rowthr on behalf of a filtered request applies the same (labels, want);
// a threshold published by an unfiltered launch would prune eligible rows.
// labels/want trail the existing arguments (offsets unchanged) and are
// never read by the FILTER=false instantiations.
template <int EPI_MODE, bool FILTER = false>
__global__ __launch_bounds__(THREADS, 2) void cosine_topk_partial_t(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C,
    float* __restrict__ partial_score, int* __restrict__ partial_idx,
    int B, int N, int D, int chunk_tiles, int nchunks,
    unsigned* rowthr = nullptr, unsigned long long* stats = nullptr,
    const int* __restrict__ labels = nullptr,
    const int* __restrict__ want = nullptr) {
  static_assert(!FILTER || EPI_MODE == 11, "only mode 11 has a filtered form");
  constexpr bool REG_THR = EPI_MODE == 8 || EPI_MODE == 9 || EPI_MODE == 11;
  constexpr bool INLINE_INSERT = EPI_MODE == 9 || EPI_MODE == 11;
  constexpr bool BALLOT_CHECK = EPI_MODE == 11;
  // LDS: 4 x 16 KiB staging (A,B double-buffered) + per-(row, col-half)
  // private top-k lists. 80 KiB total -> 2 blocks/CU. The lists are
  // private to the one wave that computes that (row-half, col-half), so
  // the epilogue needs NO barriers and overlaps the next tile's staging.
  constexpr int TB = TILE_BYTES;  // one staged tile
  __shared__ char smem[2 * TB * 2 + 2 * BM * KMAX * 8];
  char* const smem0 = smem;  // avoid static-init addrspacecast of arrays
  auto abuf = [&](int i) -> char* { return smem0 + i * TB; };
  auto bbuf = [&](int i) -> char* { return smem0 + (2 + i) * TB; };
  // list layout: scores[wc][row][KMAX] then idx[wc][row][KMAX];
  // invariant: slot 0 of each list holds that list's MINIMUM.
  float* lsc = (float*)(smem + 4 * TB);
  int* lix = (int*)(smem + 4 * TB + 2 * BM * KMAX * 4);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int g = lane >> 4;        // 16-lane group within the wave
  const int cl = lane & 15;
  const int wr = wid >> 1;        // wave's row half (0/1)
  const int wc = wid & 1;         // wave's col half (0/1)

  // XCD-aware remap (guide T1): the dispatcher places dispatch-index b on
  // XCD b%8. Give each XCD a contiguous span of corpus chunks and iterate
  // row tiles innermost, so the ~64 co-resident blocks of one XCD work on
  // the same 1-2 chunks and the corpus tile stream stays in that XCD's L2
  // instead of being re-fetched from HBM once per query row tile.
  // Requires gridDim.x % 8 == 0 (the host pads nchunks; padded chunks have
  // tiles_here <= 0 and just write -inf partials).
  const int nrt = gridDim.y;
  int chunk_id, row_tile;
  if ((gridDim.x & 7) == 0 && gridDim.x * nrt >= 512) {
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = bid & 7;
    const int slot = bid >> 3;
    const int cpx = gridDim.x >> 3;  // chunks per XCD
    chunk_id = xcd * cpx + slot / nrt;
    row_tile = slot % nrt;
  } else {
    chunk_id = blockIdx.x;
    row_tile = blockIdx.y;
  }

  const int row0 = row_tile * BM;
  const long qrow_bytes = (long)D * 2;
  const int ntiles_total = (N + BN - 1) / BN;
  const int tile0 = chunk_id * chunk_tiles;
  const int tiles_here = min(chunk_tiles, ntiles_total - tile0);
  const int nkt = D / BK;

  // init lists (-inf scores; slot 0 is the min by construction)
  for (int i = tid; i < 2 * BM * KMAX; i += THREADS) {
    lsc[i] = NEG_INF;
    lix[i] = -1;
  }
  __syncthreads();

  // prologue: stage tile 0's first K-tile
  if (tiles_here > 0) {
    stage_tile(Q, row0, B - 1, qrow_bytes, 0, abuf(0), wid, lane);
    stage_tile(C, tile0 * BN, N - 1, qrow_bytes, 0, bbuf(0), wid, lane);
  }
  __syncthreads();
  int cur = 0;

  // REG_THR: per-row pruning threshold cached in a register. Lane
  // l of each wave owns max(list-min, warm) for row wr*64+l of col-half wc,
  // so the pre-check needs no LDS reads at all (the volatile list reads at
  // the 16 unrolled call boundaries otherwise serialize ~70 lgkmcnt(0)
  // waits per tile per wave — measured 650 vs 884 TF full-vs-precheck).
  float rmin_reg = NEG_INF;
  (void)rmin_reg;

  // FILTER: lane l of each wave caches want[] for row wr*64+l for the
  // block's lifetime (-1 = unfiltered, also for the padding rows >= B); the
  // (m, reg) loop broadcasts it with one shfl, as it does rmin_reg.
  int want_reg = -1;
  (void)want_reg;
  if constexpr (FILTER) {
    if (row0 + wr * 64 + lane < B) want_reg = want[row0 + wr * 64 + lane];
  }

  for (int j = 0; j < tiles_here; ++j) {
    const int col0 = (tile0 + j) * BN;

    // per-lane warm thresholds: lane l caches rowthr for row wr*64+l; the
    // pre-check broadcasts the right lane's value with one shfl. Published
    // thresholds from other blocks prune chunk bootstraps to ~nothing.
    float warm = NEG_INF;
    if (EPI_MODE != 1 && rowthr != nullptr && row0 + wr * 64 + lane < B)
      warm = dec_f32(rowthr[row0 + wr * 64 + lane]);
    if constexpr (REG_THR) rmin_reg = fmaxf(rmin_reg, warm);

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nkt; ++kt) {
      // seamless cross-tile pipeline: the last K-step of tile j prefetches
      // tile j+1's first K-tile, so the epilogue below runs while that
      // staging is in flight.
      if (kt + 1 < nkt) {
        const int kb = (kt + 1) * BK * 2;
        stage_tile(Q, row0, B - 1, qrow_bytes, kb, abuf(cur ^ 1), wid, lane);
        stage_tile(C, col0, N - 1, qrow_bytes, kb, bbuf(cur ^ 1), wid, lane);
      } else if (j + 1 < tiles_here) {
        stage_tile(Q, row0, B - 1, qrow_bytes, 0, abuf(cur ^ 1), wid, lane);
        stage_tile(C, col0 + BN, N - 1, qrow_bytes, 0, bbuf(cur ^ 1), wid, lane);
      }
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        bf16x8 afrag[4], bfrag[4];
        const int slot = kk * 4 + g;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          afrag[m] = read_frag(abuf(cur), wr * 64 + m * 16 + cl, slot);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          bfrag[n] = read_frag(bbuf(cur), wc * 64 + n * 16 + cl, slot);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[m], bfrag[n], acc[m][n], 0, 0, 0);
      }
      if (kt + 1 < nkt) {
        __syncthreads();  // drains prefetch glds; guards buffer reuse
        cur ^= 1;
      }
      // after the LAST K-step the barrier is deferred below the epilogue,
      // overlapping list maintenance with the next tile's staging.
    }

    // ---- top-k epilogue (barrier-free) ----------------------------------
    // Each (row, col-half) list is owned by exactly one wave. Per (m,reg)
    // row, a 4-step intra-group shfl computes the row-half max from the
    // accumulators; the (rare) qualifying rows extract their candidates in
    // descending order, one leader lane updating the private LDS list.
    unsigned qmask = 0;
    (void)qmask;
    if constexpr (EPI_MODE == 1) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          asm volatile("" ::"v"(acc[m][n]));
    } else {
      const int colb = col0 + wc * 64 + cl;
      // FILTER: this lane's 4 column labels, loaded once per column tile.
      // (Folding them with the group's 16 wants into two registers of
      // eligibility bits ahead of the loop was tried: 38 spilled VGPRs
      // against 2 for this form; the kernel sits at the 256-VGPR limit.)
      int lab0 = -1, lab1 = -1, lab2 = -1, lab3 = -1;
      (void)lab0; (void)lab1; (void)lab2; (void)lab3;
      if constexpr (FILTER) {
        if (colb + 0 < N) lab0 = labels[colb + 0];
        if (colb + 16 < N) lab1 = labels[colb + 16];
        if (colb + 32 < N) lab2 = labels[colb + 32];
        if (colb + 48 < N) lab3 = labels[colb + 48];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = wr * 64 + m * 16 + g * 4 + reg;
          const int lbase = (wc * BM + row) * KMAX;
          // REG_THR reads the per-row threshold from the register
          // cache (one cross-lane shuffle) instead of a volatile LDS
          // read; the 16 unrolled call-boundary reads otherwise cost
          // ~70 serialized lgkmcnt(0) waits per tile per wave.
          float rwarm, rmin0;
          if constexpr (REG_THR) {
            rwarm = __shfl(rmin_reg, m * 16 + g * 4 + reg, 64);
            rmin0 = rwarm;
          } else {
            rwarm = __shfl(warm, m * 16 + g * 4 + reg, 64);
            rmin0 = fmaxf(lsc[lbase], rwarm);
          }
          float w0 = (colb + 0 < N) ? acc[m][0][reg] : NEG_INF;
          float w1 = (colb + 16 < N) ? acc[m][1][reg] : NEG_INF;
          float w2 = (colb + 32 < N) ? acc[m][2][reg] : NEG_INF;
          float w3 = (colb + 48 < N) ? acc[m][3][reg] : NEG_INF;
          if constexpr (FILTER) {
            const int wt = __shfl(want_reg, m * 16 + g * 4 + reg, 64);
            if (wt >= 0) {
              if (lab0 != wt) w0 = NEG_INF;
              if (lab1 != wt) w1 = NEG_INF;
              if (lab2 != wt) w2 = NEG_INF;
              if (lab3 != wt) w3 = NEG_INF;
            }
          }
          // BALLOT_CHECK: one ballot replaces the 4-deep shfl_xor max
          // reduce in the pre-check (same predicate: does ANY lane of
          // the group beat the threshold) — halves the cross-lane
          // dependency chain of the hot no-candidate path.
          bool qual;
          if constexpr (BALLOT_CHECK) {
            const float lmax = fmaxf(fmaxf(w0, w1), fmaxf(w2, w3));
            qual = (__ballot(lmax > rmin0) & (0xFFFFull << (g * 16))) != 0;
          } else {
            float gmax = fmaxf(fmaxf(w0, w1), fmaxf(w2, w3));
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
              gmax = fmaxf(gmax, __shfl_xor(gmax, off, 64));
            qual = gmax > rmin0;
          }
          if (qual) {
            if constexpr (EPI_MODE == 4) {
              // k=1: group argmax, leader max-merges into list slot 0
              float b = w0;
              int bn = 0;
              if (w1 > b) { b = w1; bn = 1; }
              if (w2 > b) { b = w2; bn = 2; }
              if (w3 > b) { b = w3; bn = 3; }
              float mv = b;
              int mlane = lane;
#pragma unroll
              for (int off = 1; off < 16; off <<= 1) {
                const float ov = __shfl_xor(mv, off, 64);
                const int ol = __shfl_xor(mlane, off, 64);
                if (ov > mv || (ov == mv && ol < mlane)) { mv = ov; mlane = ol; }
              }
              if (lane == mlane && mv > lsc[lbase]) {
                lsc[lbase] = mv;
                lix[lbase] = colb + bn * 16;
              }
            } else if constexpr (INLINE_INSERT) {
              // inline single-insert fast path: the group argmax leader
              // inserts directly (no call, so no callee-entry
              // s_waitcnt vmcnt(0) draining the staging stream); only
              // groups with a SECOND candidate above the new min take
              // the noinline extractor.
              float b = w0;
              int bn = 0;
              if (w1 > b) { b = w1; bn = 1; }
              if (w2 > b) { b = w2; bn = 2; }
              if (w3 > b) { b = w3; bn = 3; }
              float mv = b;
              int mlane = lane;
#pragma unroll
              for (int off = 1; off < 16; off <<= 1) {
                const float ov = __shfl_xor(mv, off, 64);
                const int ol = __shfl_xor(mlane, off, 64);
                if (ov > mv || (ov == mv && ol < mlane)) { mv = ov; mlane = ol; }
              }
              float nmn = mv;  // new list min (valid on the leader lane)
              if (lane == mlane) {
                int nmp = 0;
#pragma unroll
                for (int q = 1; q < KMAX; ++q) {
                  const float sq = lsc[lbase + q];
                  if (sq < nmn) { nmn = sq; nmp = q; }
                }
                const int gcol = colb + bn * 16;
                if (nmp == 0) {
                  lsc[lbase] = mv;
                  lix[lbase] = gcol;
                } else {
                  const int mi2 = lix[lbase + nmp];
                  lsc[lbase] = nmn;
                  lix[lbase] = mi2;
                  lsc[lbase + nmp] = mv;
                  lix[lbase + nmp] = gcol;
                }
                if (bn == 0) w0 = NEG_INF;
                else if (bn == 1) w1 = NEG_INF;
                else if (bn == 2) w2 = NEG_INF;
                else w3 = NEG_INF;
                if (rowthr != nullptr && nmn > NEG_INF && row0 + row < B)
                  atomicMax(&rowthr[row0 + row], enc_f32(nmn));
              }
              qmask = 1;
              // does any remaining candidate still beat the new min?
              const float nmb = fmaxf(__shfl(nmn, mlane, 64), rwarm);
              const float g2l = fmaxf(fmaxf(w0, w1), fmaxf(w2, w3));
              bool more;
              if constexpr (BALLOT_CHECK) {
                more = (__ballot(g2l > nmb) & (0xFFFFull << (g * 16))) != 0;
              } else {
                float g2 = g2l;
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
                  g2 = fmaxf(g2, __shfl_xor(g2, off, 64));
                more = g2 > nmb;
              }
              if (more)
                topk_extract_group<true>(lsc, lix, lbase, rwarm, w0, w1, w2,
                                         w3, colb, N, lane, g, rowthr,
                                         (row0 + row < B) ? row0 + row + 1 : 0);
            } else {
              topk_extract_group<true>(lsc, lix, lbase, rwarm, w0, w1, w2,
                                       w3, colb, N, lane, g, rowthr,
                                       (row0 + row < B) ? row0 + row + 1 : 0);
              if constexpr (EPI_MODE == 8) qmask = 1;
            }
          }
        }
      }
      // refresh the register threshold cache from the settled list minima
      // (wave-local: one coalesced LDS read per lane, before the barrier)
      if constexpr (REG_THR) {
        if (__any(qmask != 0))
          rmin_reg = fmaxf(rmin_reg, lsc[(wc * BM + wr * 64 + lane) * KMAX]);
      }
    }
    __syncthreads();  // next tile's first K-tile staged; lists settled
    cur ^= 1;
  }

  // write partials: [B][nchunks][KMAX]; merge the two col-half lists
  if (tid < BM) {
    const int grow = row0 + tid;
    if (grow < B) {
      const size_t base = ((size_t)grow * nchunks + chunk_id) * KMAX;
      float fs[KMAX];
      int fi[KMAX];
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        fs[q] = lsc[tid * KMAX + q];
        fi[q] = lix[tid * KMAX + q];
      }
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        const float s = lsc[(BM + tid) * KMAX + q];
        const int ix = lix[(BM + tid) * KMAX + q];
        int mp = 0;
        float mn = fs[0];
#pragma unroll
        for (int r = 1; r < KMAX; ++r)
          if (fs[r] < mn) { mn = fs[r]; mp = r; }
        if (s > mn) {
#pragma unroll
          for (int r = 0; r < KMAX; ++r)
            if (r == mp) { fs[r] = s; fi[r] = ix; }
        }
      }
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        partial_score[base + q] = fs[q];
        partial_idx[base + q] = fi[q];
      }
    }
  }
}

// ===========================================================================
// 256x256-tile 8-phase counted-pipeline kernel (guide T3+T4+T5).
//
// Geometry: 512 threads = 8 waves as 2 row-halves (wr) x 4 col-quads (wc);
// output tile 256 queries x 256 corpus rows, per-wave 128x64 (acc 8x4
// fragments of 16x16). K advances in BK=64 "windows" of 4 phases; each
// phase computes one row-quadrant (2 m-frags x 4 n x 2 kk = 16 MFMA). The
// B fragments are read ONCE per window (phase 0) and stay in registers,
// which is what frees the B image bytes early enough that the NEXT
// window's staging can target the LIVE buffer:
//
//   staging schedule (per wave, reader-aligned 1 KiB pieces), LOCKSTEP
//   modes (6, 16):
//     window t, ph0: A(t+1) pieces 0,1      -> buf[(t+1)&1]  (unread now)
//     window t, ph1: A(t+1) 2,3 + B(t+2) 0,1-> B into buf[t&1]: its B bytes
//     window t, ph2: B(t+2) pieces 2,3         were consumed at ph0
//   STAGGERED modes (1, 9, 12, 15): the B issues sit one phase later,
//     window t, ph0: A(t+1) 0,1   ph1: A(t+1) 2,3
//     window t, ph2: B(t+2) 0,1   ph3: B(t+2) 2,3 (before the wait)
//   certification (both): one `s_waitcnt vmcnt(4)` at ph3 (before the
//   barrier) leaves exactly B(t+2)'s 4 glds in flight and proves A(t+1) +
//   B(t+1) (and older) landed -> the pipeline NEVER drains to vmcnt(0)
//   (except the chunk tail, where no B(t+2) exists: vmcnt(0) there).
//
// Each phase p of window t is: issue ds_reads + glds [+ ph3 wait];
// barrier Ba(t,p); lgkmcnt(0); 16 MFMA; barrier Bb(t,p). So a phase's
// ds_reads are ISSUED before its Ba and RETIRED before its Bb.
//
// Staggered wave groups (modes without a barrier/LDS epilogue). Waves w
// and w+4 share a SIMD, i.e. group 0 (wr=0) and group 1 (wr=1) of the same
// wc. Lockstep makes both read together and then compute together, and
// the matrix pipe idles through every read+barrier segment. Group 1
// therefore executes ONE extra s_barrier after the prologue and group 0
// the matching one after the last tile's K loop: between any two
// barriers one wave of each SIMD is in its MFMA segment while its partner
// reads and stages. Barrier counts per wave are equal, so the final
// "write partials" barrier lines up; the padded-chunk return precedes it.
//
// Ledger, in HARDWARE barrier indices n (counted from the first barrier
// after the prologue's __syncthreads). Group 0: Ba(t,p) = 8t+2p,
// Bb(t,p) = 8t+2p+1. Group 1: Ba(t,p) = 8t+2p+1, Bb(t,p) = 8t+2p+2.
//   A-half(wr) [both buffers]: staged by group wr (wave wc stages quarter
//     wc), read by group wr only (phase p reads quarter p). Group-private:
//     all four waves see the same barrier indices, as in lockstep.
//     WAR: A(t+1) overwrites A(t-1); its last reads (window t-1, ph3)
//       retire before the group's Bb(t-1,3); the glds issue after it.
//     RAW: the staging wave's ph3 vmcnt precedes Ba(t,3); group-mates
//       issue their first A(t+1) read after Bb(t,3).
//   B-half(h) rows (wc&1)*64..+64 [both buffers]: read at ph0 only, by
//     waves (0,wc) and (1,wc); each stages the 32 rows wr*32..+32 of it.
//     WAR, B(t+2) over B(t): group 0's reads of B(t) retire before n=8t+1,
//       group 1's before n=8t+2. Earliest B(t+2) issue is ph2: group 0
//       after n=8t+3, group 1 after n=8t+4 — both later than a barrier
//       (8t+2) that every reader reached with its reads retired. (The
//       lockstep ph1 slot is NOT safe here: group 0 would issue between
//       8t+1 and 8t+2 while group 1 is still retiring those bytes.)
//     RAW, B(t+1): group 0 certifies its rows before n=8t+6, group 1
//       before n=8t+7 (each its own Ba(t,3)). Group 0 issues its B(t+1)
//       reads after n=8t+7, group 1 after n=8t+8: each reader has passed
//       a barrier the other group reached after its counted wait ("one
//       barrier more" — exactly enough for group 0, one spare for group 1).
//     vmcnt order at window t ph3: [B(t+1) 0-3 (window t-1 ph2,ph3)],
//       A(t+1) 0-3, B(t+2) 0-3 -> vmcnt(4) leaves only B(t+2).
//   Prologue: A(0), B(0), B(1) certified by vmcnt(0) + __syncthreads
//     before either group's first read.
//   lsc/lix lists: written before the first __syncthreads, read after the
//     final barrier (modes 1, 16); never touched in between. The emission
//     modes (9, 12, 15) have no lists: see the emission ledger below.
// Mode 6 keeps lockstep: its stash/drain epilogue shares LDS and barriers
// across both groups. Mode 16 is mode 1 on the lockstep schedule, kept so
// probe8p can A/B the two sync structures in one process.
//
// Reader-aligned staging makes per-wave vmcnt certification sound: a
// wave stages exactly the quarter of each half-image that it (or its
// barrier-synchronised co-reader) consumes. Two raw barriers per phase:
// the second separates every wave's ds_read retirement (compiler lgkm
// before its MFMAs) from the next phase's glds landing on those bytes.
//
// LDS: 2 buffers x (A[2 halves] + B[2 halves]) x 16 KiB = 128 KiB
// + shared top-k lists 16 KiB = 144 KiB -> 1 block/CU, 2 waves/SIMD.
// Emission modes: 128 KiB + 8 wave stashes x 3 KiB + cursor = 152 KiB.
//
// Emission ledger (modes 9, 15; the cold path of the epilogue):
//   (a) Stash bytes vs staging images. Every glds destination is
//     ahalf(b,h) or bhalf(b,h) + an offset < HALF8, i.e. a byte in
//     [0, 8*HALF8) = [0, 131072). Wave w's stash is [131072 + 3072w,
//     131072 + 3072(w+1)), the cursor word is at 131072 + 24576: both past
//     the last image byte in every window, so no staging write or fragment
//     read can touch them. A stash slice is written and read by its own
//     wave only (LDS serves one wave's accesses in issue order; the reads'
//     results are awaited on lgkmcnt), so it needs no barrier and the
//     staggered groups stay legal. The cursor is shared by the 8 waves
//     through a returning LDS add; it is zeroed before the first
//     __syncthreads and read after the last one.
//   (b) Fire-and-forget record stores vs the counted wait. vmcnt counts
//     loads and stores alike, and loads retire in issue order among
//     themselves. At window t ph3 the newest four LOADS are B(t+2)'s, so
//     after `vmcnt(4)` at most four operations are outstanding and any
//     outstanding load is one of those four: A(t+1) and B(t+1) have landed
//     whatever number of record stores is still in flight. Outstanding
//     stores only make the wait stricter (fewer B(t+2) loads may remain).
//     The chunk-tail `vmcnt(0)` drains everything, stores included, once
//     per block; the block's last `vmcnt(0)` before the count is published
//     is once per block too. Nothing else in the tile loop waits on vmcnt.
//   (c) Nothing in this kernel reads a record or a count back: the
//     segments are consumed by emit_bin, a later launch on the same stream.
// ===========================================================================


constexpr int THREADS8 = 512;
constexpr int HALF8 = 16384;  // one [128][64] bf16 half-image
constexpr int EGCAP = 3;  // emission stash slots per wave (1 KiB each)
constexpr int ESTASH_OFF = 8 * HALF8;        // first byte past the images
constexpr int ESTASH_WAVE = EGCAP * 1024;    // one wave's stash slice, bytes
constexpr int ESEG_COL_BITS = 15;  // column within a chunk: chunk_tiles <= 128

// Emission record (EPI_MODE 9/15 -> emit_bin): order-encoded score in the
// high word; row within the 256-row tile and column within the block's
// chunk in the low word. emit_bin rebuilds (row, global column) from the
// segment's (row_tile, chunk_id).
DEVINL unsigned long long eseg_record(float score, int row_in_tile,
                                      int col_in_chunk) {
  return ((unsigned long long)enc_f32(score) << 32) |
         (unsigned)((row_in_tile << ESEG_COL_BITS) | col_in_chunk);
}

// Returning add on an LDS word, waited for on lgkmcnt alone. Written as
// asm because the compiler puts a vmcnt(0) in front of an LDS atomic in a
// kernel that also stages with global_load_lds (it cannot tell the word
// from a staging destination), which would drain the staging pipeline and
// the epilogue's own fire-and-forget stores.
DEVINL unsigned lds_add_rtn(unsigned* word, unsigned v) {
  const unsigned addr = (unsigned)(__UINTPTR_TYPE__)(
      __attribute__((address_space(3))) unsigned*)word;
  unsigned old;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(old)
               : "v"(addr), "v"(v)
               : "memory");
  return old;
}

// EPI_MODE (numbering is historical; the pruned variants and their
// verdicts are in profiles/knn_kernel_history.md):
//   1  GEMM only (probe8p, tools/knn_probe.hip)
//   6  ballot-skip stash+drain into shared per-row lists: a register
//      ballot pre-check against the rowthr floors marks which waves have
//      ANY qualifying candidate this tile; unflagged waves' stash+drain
//      phases are skipped uniformly (KAKVEDA_KNN_KERNEL=8pbl, 686 TF)
//   9  threshold emission — the PRODUCTION DEFAULT at N >= 64k: no lists,
//      scores >= the prepass floor go to a global candidate buffer
//   12 = 9's hot sweep with the cold path compiled out (probe8p)
//   15 = 9 with block-lifetime packed threshold vectors (=8pe2)
//   16 = 1 on the lockstep schedule (probe8p A/B, tools/knn_probe.hip)
// Modes 1, 9, 12, 15 run their two wave groups staggered by one barrier;
// 6 and 16 run lockstep (ledger in the block comment above).
// eseg/esegcnt/segcap are the emission modes' record segments (they took
// the slots, and types, of the per-row candidate buffer the kernel once
// scattered into itself). `stats`, `slab` and `unused` are unused (they
// belonged to pruned modes and to the global stash) and stay in the
// signature so the kernarg offsets of the others do not move. `tile_first`
// (modes 9/15; the other modes ignore it) is the column tile the launch
// starts at: chunk 0 begins there.
template <int EPI_MODE>
__global__ __launch_bounds__(THREADS8, 2) void cosine_topk_partial8p_t(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C,
    float* __restrict__ partial_score, int* __restrict__ partial_idx,
    int B, int N, int D, int chunk_tiles, int nchunks,
    unsigned* rowthr = nullptr, unsigned long long* stats = nullptr,
    float* __restrict__ slab = nullptr,
    unsigned long long* __restrict__ eseg = nullptr,
    unsigned* __restrict__ esegcnt = nullptr, long segcap = 0,
    char* __restrict__ unused = nullptr, int tile_first = 0) {
  constexpr bool EMIT = EPI_MODE == 9 || EPI_MODE == 12 || EPI_MODE == 15;
  constexpr bool GEMM_ONLY = EPI_MODE == 1 || EPI_MODE == 16;
  // staggered wave groups: only for the modes whose epilogue has no
  // barrier and touches no LDS byte another wave reads or stages (see the
  // ledger above the kernel)
  constexpr bool STAGGER = EPI_MODE == 1 || EMIT;
  // one array: staging images, then (emission) the wave-private stashes and
  // the segment cursor, or (other modes) the shared lists and wave flags
  __shared__ char smem[EMIT ? ESTASH_OFF + 8 * ESTASH_WAVE + 32
                            : 8 * HALF8 + 2 * BM8 * KMAX * 4 + 32];
  char* const smem0 = smem;
  // buffer b in {0,1}: A half h at b*4*HALF8 + h*HALF8; B half h at +2*HALF8
  auto ahalf = [&](int b, int h) -> char* {
    return smem0 + (b * 4 + h) * HALF8;
  };
  auto bhalf = [&](int b, int h) -> char* {
    return smem0 + (b * 4 + 2 + h) * HALF8;
  };
  float* lsc = (float*)(smem + 8 * HALF8);
  int* lix = (int*)(smem + 8 * HALF8 + BM8 * KMAX * 4);
  int* wflags = (int*)(smem + 8 * HALF8 + 2 * BM8 * KMAX * 4);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform for the compiler: wr guards raw s_barriers below, which
  // must sit behind a scalar branch
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
  const long rb = (long)D * 2;
  const int ntiles_total = (N + BN8 - 1) / BN8;
  constexpr bool APPEND = EPI_MODE == 9 || EPI_MODE == 15;
  // the emission main launch starts at column tile `tile_first` (the tiles
  // before it are the prepass sample's: knn_plan.h main_geometry); chunk
  // ids, segments and in-chunk columns count from there. Every other mode
  // scans from tile 0.
  const int tile0 = (APPEND ? tile_first : 0) + chunk_id * chunk_tiles;
  const int tiles_here = min(chunk_tiles, ntiles_total - tile0);
  const int nkt = D / 64;  // windows per col tile

  // emission append state (modes 9/15): this wave's stash slice, the
  // block's record cursor (an LDS word behind the stashes) and the block's
  // segment of the global record buffer, indexed by (row_tile, chunk_id)
  // (lambdas: the other modes' instruction streams must not see them)
  auto estash = [&]() -> char* {
    return smem0 + ESTASH_OFF + wid * ESTASH_WAVE;
  };
  auto ecursor = [&]() -> unsigned* {
    return (unsigned*)(smem0 + ESTASH_OFF + 8 * ESTASH_WAVE);
  };
  auto segid = [&]() -> size_t {
    return (size_t)row_tile * nchunks + chunk_id;
  };

  if constexpr (EMIT) {
    if (tid == 0) *ecursor() = 0u;
  } else {
    for (int i = tid; i < BM8 * KMAX; i += THREADS8) {
      lsc[i] = NEG_INF;
      lix[i] = -1;
    }
  }
  __syncthreads();
  if (tiles_here <= 0) {
    // padded chunk: emit -inf partials (and an empty segment) and exit
    if constexpr (APPEND) {
      if (tid == 0) esegcnt[segid()] = 0u;
    }
    if (tid < BM8 && row0 + tid < B) {
      const size_t base = ((size_t)(row0 + tid) * nchunks + chunk_id) * KMAX;
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        partial_score[base + q] = NEG_INF;
        partial_idx[base + q] = -1;
      }
    }
    return;
  }

  // ---- staging helpers --------------------------------------------------
  // A-share of K-tile t: quarter wc (rows wc*32..+32) of A-half(wr).
  // B-share of K-tile t: rows (wc&1)*64 + wr*32 ..+32 of B-half(wc>>1).
  // piece = 1 KiB = 8 image rows; lane-linear glds dest; swizzled source.
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

  // ---- prologue: K-tile 0 fully + B(1); then steady schedule ------------
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_a_piece(0, i);
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_b_piece(0, i);
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_b_piece(1, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // stagger: group 1 (waves 4-7) runs one barrier behind group 0 from
  // here to the end of the last tile's K loop
  if constexpr (STAGGER) {
    if (wr == 1) __builtin_amdgcn_s_barrier();
  }

  const int total_windows = tiles_here * nkt;

  // EPI_MODE 15: block-lifetime per-lane threshold VECTORS. Under the
  // emission main launch rowthr is static (prepass-published floors; mode
  // 9/15 never write it), so the 32 per-(m,reg) thresholds each lane
  // compares against are constants for the whole block. Mode 9 re-derives
  // them with 32 ds_bpermute + 32 vcc-serialised ballots per TILE; here
  // they are shuffled ONCE into 16 registers as bf16 PAIRS (a full-f32
  // tv[32] spilled 32 B/lane at the 256-VGPR/2-wave cap), rounded toward
  // -inf so the packed floor is <= the exact one. The per-tile hot sweep
  // becomes a pure-VALU running max-diff with a single ballot.
  // Exactness: qualification vs the rounded-DOWN floor is a superset of
  // qualification vs the exact floor, and a hot-sweep positive only opens
  // the cold path, whose per-lane compares in the drain re-check the
  // EXACT thr0/thr1 before any candidate is stored.
  unsigned tvp[16];
  if constexpr (EPI_MODE == 15) {
    const int r0g = row0 + wr * 128 + lane;
    const float t0b =
        (r0g < B) ? (rowthr ? dec_f32(rowthr[r0g]) : NEG_INF) : 1e38f;
    const float t1b = (r0g + 64 < B)
                          ? (rowthr ? dec_f32(rowthr[r0g + 64]) : NEG_INF)
                          : 1e38f;
    // upper-16 f32 bits rounded toward -inf (truncation rounds toward
    // zero, i.e. UP for negatives -> push one ulp down there; a
    // most-negative-finite pushed to 0xff80 = -inf still compares
    // conservatively)
    auto bfloor = [](float f) -> unsigned {
      const unsigned b = __float_as_uint(f);
      unsigned hi = b >> 16;
      if ((b & 0xffffu) && (b >> 31)) ++hi;
      return hi & 0xffffu;
    };
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rl0 = m * 16 + g * 4 + 2 * h;
        const unsigned lo = bfloor(__shfl(m >= 4 ? t1b : t0b, rl0 & 63, 64));
        const unsigned hi =
            bfloor(__shfl(m >= 4 ? t1b : t0b, (rl0 + 1) & 63, 64));
        tvp[m * 2 + h] = lo | (hi << 16);
      }
  }

  // per-lane threshold floors for this wave-half's two rows (rows beyond
  // B get +inf so clamped-row garbage never flags). The emission modes
  // read them ONCE per block: under their launch rowthr is static (the
  // prepass has finished and modes 9/12/15 never write it). Read per tile,
  // each of the two loads cost an L2 round trip behind a vmcnt(0) that also
  // drained the B(t+2) staging the counted wait keeps in flight. Mode 6
  // publishes into rowthr during its launch and keeps the per-tile read.
  auto load_floors = [&](float& t0, float& t1) {
    const int r0g = row0 + wr * 128 + lane;
    t0 = (r0g < B) ? (rowthr ? dec_f32(rowthr[r0g]) : NEG_INF) : 1e38f;
    t1 = (r0g + 64 < B) ? (rowthr ? dec_f32(rowthr[r0g + 64]) : NEG_INF)
                        : 1e38f;
  };
  float thr0 = NEG_INF, thr1 = NEG_INF;
  if constexpr (EMIT) {
    load_floors(thr0, thr1);
    // a use here, right behind the prologue's full drain: the compiler's
    // wait for the two loads lands before the tile loop, not inside it
    asm volatile("" ::"v"(thr0), "v"(thr1));
  }

  for (int j = 0; j < tiles_here; ++j) {
    const int col0 = (tile0 + j) * BN8;

    if constexpr (!GEMM_ONLY && !EMIT) load_floors(thr0, thr1);

    f32x4 acc[8][4];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nkt; ++kt) {
      const int t = j * nkt + kt;  // global window index
      const char* Ai = ahalf(t & 1, wr);
      const char* Bi = bhalf(t & 1, wc >> 1) + ((wc & 1) * 64) * 128;
      bf16x8 bf[4][2];
#pragma unroll
      for (int qm = 0; qm < 4; ++qm) {
        // ---- reads (before barrier; compiler inserts lgkm before MFMA)
        bf16x8 af[2][2];
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            af[mm][kk] = read_frag(Ai, (qm * 2 + mm) * 16 + cl, kk * 4 + g);
        if (qm == 0) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
              bf[n][kk] = read_frag(Bi, n * 16 + cl, kk * 4 + g);
        }
        // ---- staging issues (see schedule above)
        if constexpr (STAGGER) {
          if (qm == 0 && t + 1 < total_windows) {
            stage_a_piece(t + 1, 0);
            stage_a_piece(t + 1, 1);
          } else if (qm == 1 && t + 1 < total_windows) {
            stage_a_piece(t + 1, 2);
            stage_a_piece(t + 1, 3);
          } else if (qm == 2 && t + 2 < total_windows) {
            stage_b_piece(t + 2, 0);
            stage_b_piece(t + 2, 1);
          } else if (qm == 3) {
            // B(t+2) 2,3 go out BEFORE the counted wait, so the newest 4
            // outstanding glds are still exactly B(t+2)'s: vmcnt(4)
            // certifies A(t+1) and B(t+1). Chunk tail: no B(t+2), drain.
            if (t + 2 < total_windows) {
              stage_b_piece(t + 2, 2);
              stage_b_piece(t + 2, 3);
              asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            } else {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
          }
        } else if (qm == 0 && t + 1 < total_windows) {
          stage_a_piece(t + 1, 0);
          stage_a_piece(t + 1, 1);
        } else if (qm == 1) {
          if (t + 1 < total_windows) {
            stage_a_piece(t + 1, 2);
            stage_a_piece(t + 1, 3);
          }
          if (t + 2 < total_windows) {
            stage_b_piece(t + 2, 0);
            stage_b_piece(t + 2, 1);
          }
        } else if (qm == 2 && t + 2 < total_windows) {
          stage_b_piece(t + 2, 2);
          stage_b_piece(t + 2, 3);
        } else if (qm == 3) {
          // certify window t+1's A and B. Steady state: the newest 4
          // outstanding glds are B(t+2)'s, so vmcnt(4) proves A(t+1) and
          // B(t+1) landed. At the chunk tail no B(t+2) was issued, so the
          // newest 4 would be A(t+1) itself -> drain fully there (rare).
          if (t + 2 < total_windows)
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int n = 0; n < 4; ++n)
              acc[qm * 2 + mm][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[mm][kk], bf[n][kk], acc[qm * 2 + mm][n], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();  // read-retirement vs next glds
      }
    }
    // group 0's make-up barrier pairs with group 1's last phase barrier;
    // from here on every wave has executed the same number of barriers
    if constexpr (STAGGER) {
      if (wr == 0 && j == tiles_here - 1) __builtin_amdgcn_s_barrier();
    }

    // ---- top-k epilogue ---------------------------------------------------
    if constexpr (GEMM_ONLY) {
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          asm volatile("" ::"v"(acc[m][n]));
    } else if constexpr (EMIT) {
      // ---- threshold-emission epilogue: no lists, no stash phases, no
      // barriers — the GEMM core's full accumulator sweep is a register
      // compare + rare record append. Exactness: the rowthr floors are
      // the 8th best of a score SUBSET, which lower-bounds the corpus
      // 8th best and hence the true k-th for any k <= 8 — so emitting
      // every score >= floor provably captures the whole top-k. emit_bin
      // scatters the records into the per-row candidate buffer and
      // emit_merge_topk reduces the (expected ~8N/s per row) candidates
      // (a j-th-best floor, j >= k, is as exact and admits j/8 of them:
      // publish_emission_floor takes the depth); per-row counts
      // above the cap, or an overflowed segment, flag a host fallback.
      // Two-phase sweep: the HOT pass is pure compare/shfl/ballot with
      // NO call sites, so the compiler keeps the 128 accumulator VGPRs
      // unspilled (a single-pass sweep with per-group calls pre-spilled
      // 32 regs per tile per wave -> ~27 GB of scratch traffic at the
      // 10M bench). The COLD pass (wave-uniform qmask != 0, ~12% of tiles
      // per wave) stashes the qualifying groups in LDS and drains them
      // inline at ONE site, so no call and no spill either.
      const int colb = col0 + wc * 64 + cl;
      unsigned qm32 = 0;
      if constexpr (EPI_MODE == 15) {
        // mode 15 hot sweep: no shuffles (tv precomputed per block), no
        // per-group ballots — one running max of (gmax - thr) and ONE
        // wave ballot. The per-group qualification bits are only needed
        // on the rare cold path, where they are re-derived with the
        // ballots mode 9 pays unconditionally.
        auto thr_lo = [&](int m, int reg) -> float {
          const unsigned pk = tvp[m * 2 + (reg >> 1)];
          return __uint_as_float((reg & 1) ? (pk & 0xffff0000u) : (pk << 16));
        };
        float run = NEG_INF;
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const float gmax = fmaxf(fmaxf(acc[m][0][reg], acc[m][1][reg]),
                                     fmaxf(acc[m][2][reg], acc[m][3][reg]));
            run = fmaxf(run, gmax - thr_lo(m, reg));
          }
        if (__builtin_expect(__ballot(run >= 0.f) != 0, 0)) {
#pragma unroll
          for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const float gmax = fmaxf(fmaxf(acc[m][0][reg], acc[m][1][reg]),
                                       fmaxf(acc[m][2][reg], acc[m][3][reg]));
              if (__ballot(gmax >= thr_lo(m, reg)))
                qm32 |= 1u << (m * 4 + reg);
            }
        }
      } else {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int rl = m * 16 + g * 4 + reg;  // 0..127 within this half
            const float thr = __shfl(m >= 4 ? thr1 : thr0, rl & 63, 64);
            const float gmax = fmaxf(fmaxf(acc[m][0][reg], acc[m][1][reg]),
                                     fmaxf(acc[m][2][reg], acc[m][3][reg]));
            if (__ballot(gmax >= thr))  // uniform
              qm32 |= 1u << (m * 4 + reg);
          }
        }
      }
      if constexpr (EPI_MODE == 12) {
        // probe-only: hot sweep computed, cold path compiled out — lets
        // the host isolate the sweep's cost from the emission cost
        asm volatile("" ::"s"(qm32));
      } else {
        if (__builtin_expect(qm32 != 0, 0)) {  // uniform cold path
          // Nothing here waits on global memory. Qualifying groups'
          // accumulator quads go to this wave's private LDS stash slice
          // (bytes no staging image ever covers: ledger item (a) above the
          // kernel), written and read back by the same wave, ordered by
          // lgkmcnt alone. The drain compares against the EXACT floors,
          // compacts the qualifying lanes with ballot + mbcnt and appends
          // 8-byte records to the block's segment with plain stores; the
          // segment cursor is an LDS word. The stores are never waited
          // for and never read back by this kernel (ledger (b), (c)).
          // An LDS stash in the "dead" last-window A image once corrupted
          // later tiles' scores (cause never found), so no staging byte
          // is aliased in any window.
          // Correlated query batches (e.g. the bench's template-generated
          // signatures) make qualifying groups BURST on "hot" corpus tiles
          // (dozens of groups at once), so a full stash drains and
          // refills: the stash+drain pass repeats until no group is left.
          const int rowl0 = wr * 128;                 // row within the tile
          const int colc = j * BN8 + wc * 64 + cl;    // column within chunk
          unsigned long long* const seg = eseg + segid() * (size_t)segcap;
          char* const st = estash();
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
                      f32x4{acc[m][0][reg], acc[m][1][reg], acc[m][2][reg],
                            acc[m][3][reg]};
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
              if (lane == 0) base = lds_add_rtn(ecursor(), total);
              base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
              // a segment that would overflow stops storing; the cursor
              // keeps the true count and emit_bin poisons the row tile
              auto put = [&](bool q, unsigned long long bal, unsigned off,
                             float sc, int n) {
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
    } else {
      // ---- EPI_MODE 6 pre-check: one register ballot per (m,reg) row
      // group against the rowthr floors; waves with no qualifying
      // candidate skip their stash+drain phase below (uniformly — the
      // flags live in LDS so every wave takes the same branch).
      unsigned qual = 0;  // per-(m,reg) qualifying bits (my groups)
#pragma unroll
      for (int m = 0; m < 8; ++m) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int rl = m * 16 + g * 4 + reg;  // 0..127 within half
          const float thr = __shfl(m >= 4 ? thr1 : thr0, rl & 63, 64);
          const float lmax = fmaxf(fmaxf(acc[m][0][reg], acc[m][1][reg]),
                                   fmaxf(acc[m][2][reg], acc[m][3][reg]));
          if (__ballot(lmax > thr) & (0xFFFFull << (g * 16)))
            qual |= 1u << (m * 4 + reg);
        }
      }
      if (lane == 0) wflags[wid] = __any(qual != 0) ? 1 : 0;
      __syncthreads();  // flags visible
      // ---- top-k epilogue (stash + lane-parallel register-list drain) --
      // The A images of the LAST window's buffer are dead during the
      // epilogue (A(t+2) staging is only issued at window t+1 phase 0),
      // so each wave stashes its 128x64 score quadrant there and drains
      // it with one lane per two rows: candidates merge into a
      // register-held copy of the row's list (select chains, no calls,
      // no ballots, no volatile round-trips). Col-quad phases serialise
      // writers of the shared per-row lists.
      const int t_last = j * nkt + nkt - 1;
      // 32 KiB ([128][64] f32) of LDS is free during the epilogue (the A
      // images of the last window's buffer). The 8 waves take turns
      // stashing their 128x64 score quadrant there; after each stash ALL
      // waves drain it cooperatively (16 rows per wave, one row per lane,
      // single-writer lists), so the scan latency is hidden by 8-wave TLP
      // instead of being exposed on a lone wave.
      float* stash = (float*)ahalf(t_last & 1, 0);
#pragma unroll
      for (int phw = 0; phw < 8; ++phw) {
        // stashing wave's wid = swr*4 + swc; uniform (flags in LDS)
        if (!wflags[(phw & 1) * 4 + (phw >> 1)]) continue;
        const int swc = phw >> 1, swr = phw & 1;  // stashing wave
        if (wc == swc && wr == swr) {
#pragma unroll
          for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
              for (int reg = 0; reg < 4; ++reg)
                stash[(m * 16 + g * 4 + reg) * 64 + n * 16 + cl] =
                    acc[m][n][reg];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stash visible to every wave

        if (lane < 16) {  // 8 waves x 16 lanes = one drainer per row
          const int rl = wid * 16 + lane;         // 0..127 within half
          const int row = swr * 128 + rl;
          const int grow = row0 + row;
          const int colq = col0 + swc * 64;
          float ls[KMAX];
          int li[KMAX];
#pragma unroll
          for (int q = 0; q < KMAX; ++q) {
            ls[q] = lsc[row * KMAX + q];
            li[q] = lix[row * KMAX + q];
          }
          float rmin = ls[0];
#pragma unroll
          for (int q = 1; q < KMAX; ++q) rmin = fminf(rmin, ls[q]);
          if (rowthr != nullptr && grow < B)
            rmin = fmaxf(rmin, dec_f32(rowthr[grow]));
          bool dirty = false;
          const float* srow = stash + rl * 64;
#pragma unroll 4
          for (int ii = 0; ii < 16; ++ii) {
            const int iv = (ii + rl) & 15;  // bank stagger across rows
            const float4 v4 = *(const float4*)(srow + 4 * iv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = e == 0 ? v4.x : e == 1 ? v4.y : e == 2 ? v4.z : v4.w;
              const int gc = colq + 4 * iv + e;
              if (v > rmin && gc < N) {
                int mp = 0;
                float mn1 = ls[0], mn2 = 1e38f;
#pragma unroll
                for (int q = 1; q < KMAX; ++q) {
                  if (ls[q] < mn1) { mn2 = mn1; mn1 = ls[q]; mp = q; }
                  else if (ls[q] < mn2) { mn2 = ls[q]; }
                }
#pragma unroll
                for (int q = 0; q < KMAX; ++q)
                  if (q == mp) { ls[q] = v; li[q] = gc; }
                rmin = fmaxf(rmin, fminf(mn2, v));
                dirty = true;
              }
            }
          }
          if (dirty) {
            int mp = 0;
            float mn = ls[0];
#pragma unroll
            for (int q = 1; q < KMAX; ++q)
              if (ls[q] < mn) { mn = ls[q]; mp = q; }
            // swap the min into slot 0 (list invariant), then write back
            const float s_mp = ls[mp];
            const int i_mp = li[mp];
            ls[mp] = ls[0];
            li[mp] = li[0];
            ls[0] = s_mp;
            li[0] = i_mp;
#pragma unroll
            for (int q = 0; q < KMAX; ++q) {
              lsc[row * KMAX + q] = ls[q];
              lix[row * KMAX + q] = li[q];
            }
            if (rowthr != nullptr && mn > NEG_INF && grow < B)
              atomicMax(&rowthr[grow], enc_f32(mn));
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // lists settled; stash reusable
      }
      // drain the drains' rowthr publish atomics: they are vmcnt-tracked
      // and must not leak into the next tile's counted staging waits
      // (same audit class as the emission epilogue's vmcnt(0))
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }

  // emission: publish the segment's true record count (it may exceed
  // segcap: emit_bin then poisons the row tile). Every wave's cursor
  // atomics returned before its last readfirstlane, and both wave groups
  // have executed the same number of barriers by now.
  if constexpr (APPEND) {
    __syncthreads();
    if (tid == 0) esegcnt[segid()] = *ecursor();
  }
  // write partials: [B][nchunks][KMAX] (emission modes have no lists —
  // their results went to the record segments)
  if constexpr (!EMIT) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (tid < BM8) {
      const int grow = row0 + tid;
      if (grow < B) {
        const size_t base = ((size_t)grow * nchunks + chunk_id) * KMAX;
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          partial_score[base + q] = lsc[tid * KMAX + q];
          partial_idx[base + q] = lix[tid * KMAX + q];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Publish the merged sample's k-th best as the per-row emission floor.
// After topk_merge over the prepass partials, out_s[row][kth] is the EXACT
// kth-best of the whole sampled column set — a far tighter (still exact)
// lower bound on the corpus kth-best than the per-(row, col-half) list
// minima the prepass publishes on its own (those are 8th-of-512-columns;
// at 10M rows they admitted ~40x more candidates and overflowed).
// ---------------------------------------------------------------------------
__global__ void publish_emission_floor(const float* __restrict__ merged_s,
                                       unsigned* __restrict__ rowthr, int B,
                                       int kth) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < B) {
    const float v = merged_s[(size_t)r * KMAX + kth];
    if (v > NEG_INF) atomicMax(&rowthr[r], enc_f32(v));
  }
}

// ---------------------------------------------------------------------------
// Binning step of the 8-phase emission path: one block per record segment
// (grid = (nchunks, row_tiles), the main launch's logical block ids).
// Rebuilds (row, global column) of every record and scatters the packed
// (order-encoded score << 32) | (0x7fffffff - col) into the per-row
// candidate buffer emit_merge_topk reads. The per-row atomics live here,
// off the GEMM kernel's critical path. A segment whose true count exceeds
// its capacity lost records: it poisons one ccount of its row tile past
// ccap, which the host's single ccount.max() readback turns into the loud
// fallback, exactly as a per-row overflow does.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emit_bin(
    const unsigned long long* __restrict__ eseg,
    const unsigned* __restrict__ esegcnt, int segcap, int chunk_tiles,
    int nchunks, int B, int N, unsigned long long* __restrict__ cand,
    unsigned* __restrict__ ccount, long ccap, int tile_first = 0) {
  const int chunk_id = blockIdx.x, row_tile = blockIdx.y;
  const size_t segid = (size_t)row_tile * nchunks + chunk_id;
  const unsigned cnt = esegcnt[segid];
  if (cnt == 0) return;
  const int row0 = row_tile * BM8;
  // tile_first: the main launch's first column tile (its chunk 0 starts there)
  const int colbase = (tile_first + chunk_id * chunk_tiles) * BN8;
  if (cnt > (unsigned)segcap && threadIdx.x == 0)
    atomicAdd(&ccount[row0], (unsigned)ccap + 1u);
  const unsigned n = min(cnt, (unsigned)segcap);
  const unsigned long long* seg = eseg + segid * (size_t)segcap;
  for (unsigned i = threadIdx.x; i < n; i += 256) {
    const unsigned long long rec = seg[i];
    const unsigned lo = (unsigned)rec;
    const int row = row0 + (int)(lo >> ESEG_COL_BITS);
    const int col = colbase + (int)(lo & ((1u << ESEG_COL_BITS) - 1u));
    if (row >= B || col >= N) continue;  // never emitted; guards the stores
    const unsigned pos = atomicAdd(&ccount[row], 1u);
    if (pos < (unsigned)ccap)
      cand[(size_t)row * ccap + pos] =
          (rec & 0xffffffff00000000ull) | (unsigned)(0x7fffffff - col);
  }
}

// ---------------------------------------------------------------------------
// Seeds each row's candidate list with the sample's top-KMAX (samp_s/samp_i,
// run_emission_floors), packed as emit_bin packs, and sets the row's count
// to the number seeded: the main launch then starts after the sampled
// columns (knn_plan.h main_geometry). Empty slots (-inf, -1: fewer than KMAX
// sampled columns survived) are left out. One thread per row; runs where
// the counts were cleared, ahead of the main launch on the same stream.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emit_seed(
    const float* __restrict__ samp_s, const long* __restrict__ samp_i, int B,
    unsigned long long* __restrict__ cand, unsigned* __restrict__ ccount,
    long ccap) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  unsigned n = 0;
#pragma unroll
  for (int q = 0; q < KMAX; ++q) {
    const float s = samp_s[(size_t)row * KMAX + q];
    const long col = samp_i[(size_t)row * KMAX + q];
    if (col < 0 || !(s > NEG_INF)) continue;
    const unsigned pos = n++;
    if (pos < (unsigned)ccap)
      cand[(size_t)row * ccap + pos] = ((unsigned long long)enc_f32(s) << 32) |
                                       (unsigned)(0x7fffffff - (int)col);
  }
  ccount[row] = n;
}

// The streaming kernels' emission floor was scored by the MFMA prepass, the
// rows they stream by VALU sums in another order. Both add the same exact
// bf16 products in fp32, each within (D-1) * 2^-24 * sum|q_i c_i| of the true
// value, which for UNIT ROWS (the precondition of the search) is
// <= (D-1) * 2^-24: the two scores of one column differ by < D * 2^-23. The
// floor is the 8th best of the sample, so whenever a sampled column is among
// a query's best 8 (always, once the sample covers the corpus; and bit-equal
// duplicates make the 8th best EQUAL the best) that difference can put the
// column's streamed score under its own floor. Every streaming kernel
// therefore compares against the floor lowered by twice the bound. NEG_INF
// (no floor published) absorbs the subtraction.
DEVINL float streaming_floor(unsigned enc_floor, int D) {
  return dec_f32(enc_floor) - (float)D * 0x1p-22f;
}

// ---------------------------------------------------------------------------
// Small-batch streaming emission search (B <= 8): request-level serving.
//
// The MFMA kernels pad tiny query batches to a full 128/256-row tile, so
// a single /warn query pays 128x the GEMM compute (measured p50 6.4 ms
// at B=1 x 10M vs the ~2 ms corpus-stream bound). Here each THREAD
// streams whole corpus rows (64 lanes read 64 consecutive rows — every
// byte of HBM read exactly once, full-bandwidth pattern), keeps B <= 8
// fp32 accumulators in registers against the LDS-resident queries, and
// emits scores >= the per-query prepass floor (lowered: streaming_floor)
// into the same candidate buffer the emission path merges. Exactness = the
// emission argument.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smallb_emit_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C, int B,
    long N, int D, const unsigned* __restrict__ rowthr,
    unsigned long long* __restrict__ cand, unsigned* __restrict__ ccount,
    long ccap) {
  extern __shared__ char qmem[];  // [B][D] bf16 queries
  __shared__ float fl[8];
  for (int i = threadIdx.x; i < B * (D / 8); i += 256)
    ((bf16x8*)qmem)[i] = ((const bf16x8*)Q)[i];
  if (threadIdx.x < B) fl[threadIdx.x] = streaming_floor(rowthr[threadIdx.x], D);
  __syncthreads();

  const int nj = D / 8;  // D % 64 == 0 -> nj % 8 == 0
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < N;
       r += (long)gridDim.x * 256) {
    // 4 independent partial accumulators per query: a single running
    // accumulator serializes a 768-deep FMA dependency chain per row
    // (measured 2.5x slower than the padded MFMA path); 4 chains + the
    // 4-vector load batch restore ILP and memory-level parallelism.
    f32x4 accv[8][2];
#pragma unroll
    for (int b = 0; b < 8; ++b)
      accv[b][0] = accv[b][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16x8* row = (const bf16x8*)(C + r * D);
    for (int j = 0; j < nj; j += 8) {
      bf16x8 cv[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) cv[v] = row[j + v];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < B) {
          const bf16x8* qb = (const bf16x8*)(qmem + (size_t)b * D * 2) + j;
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            const bf16x8 qv = qb[v];
#pragma unroll
            for (int e = 0; e < 8; ++e)
              accv[b][v >> 2][v & 3] += (float)cv[v][e] * (float)qv[e];
          }
        }
      }
    }
    float acc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b)
      acc[b] = ((accv[b][0][0] + accv[b][0][1]) +
                (accv[b][0][2] + accv[b][0][3])) +
               ((accv[b][1][0] + accv[b][1][1]) +
                (accv[b][1][2] + accv[b][1][3]));
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b < B && acc[b] >= fl[b]) {
        const unsigned pos = atomicAdd(&ccount[b], 1u);
        if (pos < (unsigned)ccap)
          cand[(size_t)b * ccap + pos] =
              ((unsigned long long)enc_f32(acc[b]) << 32) |
              (unsigned)(0x7fffffff - (int)r);
      }
    }
  }
}

// v4 lane remap (the serving DEFAULT; KAKVEDA_SMALLB=2 reverts): one
// wave covers 8 CONSECUTIVE rows with 8 lanes per row, so a single load
// instruction touches 8 FULL 128-byte lines, and scores are reduced
// across the 8 chunk lanes with 3 shfl_xor steps at row end; per-lane
// f32x4 sub-chains keep the FMA dependency depth at 2 per segment (the
// v1 lesson). Measured +13% over v2 at B=4 (parity at B=1), and TCC
// counters show WHY (profiles/pmc_round2.md): L2 traffic is identical
// (one request per 128-B line in both mappings — L1 coalesces v2's
// eight same-line 16-B loads), so the win is the leaner inner loop
// (1,587 vs 2,442 instructions) and 134-vs-186 VGPRs = 3-vs-2
// waves/SIMD occupancy, NOT cache behaviour. Exactness: identical
// emission contract to v2 — every score >= the shared prepass floor
// (lowered: streaming_floor) is emitted; tail rows are clamped for the load
// and guarded at emission.
//
// FILTER is the label-filtered form (eligibility rule: see
// cosine_topk_partial_t): want[0..B) sits in LDS beside fl, each row
// group's ch == 0 lane loads its row's label, and a score is emitted only
// when it clears the floor AND its row is eligible for that query. The
// floors it reads must come from a prepass run with the same (labels,
// want). labels/want trail the existing arguments and are never read by
// the FILTER=false instantiation. (A shared __forceinline__ body under two
// plain kernels was tried first: the unfiltered kernel no longer compiled
// to the instructions it had.)
template <bool FILTER = false>
__global__ __launch_bounds__(256) void smallb_emit_kernel_v4(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ C, int B,
    long N, int D, const unsigned* __restrict__ rowthr,
    unsigned long long* __restrict__ cand, unsigned* __restrict__ ccount,
    long ccap, const int* __restrict__ labels = nullptr,
    const int* __restrict__ want = nullptr) {
  extern __shared__ char qmem[];  // [B][D] bf16 queries
  __shared__ float fl[8];
  const int* wl = nullptr;
  (void)wl;
  for (int i = threadIdx.x; i < B * (D / 8); i += 256)
    ((bf16x8*)qmem)[i] = ((const bf16x8*)Q)[i];
  if (threadIdx.x < B) fl[threadIdx.x] = streaming_floor(rowthr[threadIdx.x], D);
  if constexpr (FILTER) {
    __shared__ int wls[8];  // no LDS in the unfiltered kernel
    if (threadIdx.x < B) wls[threadIdx.x] = want[threadIdx.x];
    wl = wls;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int rr = lane >> 3;  // row within this wave's 8
  const int ch = lane & 7;   // 16-byte chunk within a 128-B segment
  const int nseg = D / 64;   // 128-B segments per row (D % 64 == 0)
  for (long r0 = (long)blockIdx.x * 32 + wid * 8; r0 < N;
       r0 += (long)gridDim.x * 32) {
    const long r = r0 + rr < N ? r0 + rr : N - 1;  // clamp tail loads
    const bf16x8* row = (const bf16x8*)(C + r * D);
    int lab = -1;
    (void)lab;
    if constexpr (FILTER) {
      if (ch == 0 && r0 + rr < N) lab = labels[r0 + rr];
    }
    f32x4 accv[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) accv[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j + 4 <= nseg; j += 4) {
      bf16x8 cv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) cv[v] = row[(j + v) * 8 + ch];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < B) {
          const bf16x8* qb = (const bf16x8*)(qmem + (size_t)b * D * 2);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const bf16x8 qv = qb[(j + v) * 8 + ch];
#pragma unroll
            for (int e = 0; e < 8; ++e)
              accv[b][e & 3] += (float)cv[v][e] * (float)qv[e];
          }
        }
      }
    }
    for (; j < nseg; ++j) {  // D % 256 != 0 tail segments
      const bf16x8 cv = row[j * 8 + ch];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < B) {
          const bf16x8 qv =
              ((const bf16x8*)(qmem + (size_t)b * D * 2))[j * 8 + ch];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            accv[b][e & 3] += (float)cv[e] * (float)qv[e];
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
        if (ch == 0 && r0 + rr < N && s >= fl[b] && eligible) {
          const unsigned pos = atomicAdd(&ccount[b], 1u);
          if (pos < (unsigned)ccap)
            cand[(size_t)b * ccap + pos] =
                ((unsigned long long)enc_f32(s) << 32) |
                (unsigned)(0x7fffffff - (int)(r0 + rr));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Companion merge for the emission epilogue (8p EPI_MODE 9): exact top-k
// per row over the emitted (score, col) candidates. grid = B blocks x 256
// threads; each thread keeps a sorted top-KMAX of its strided slice in
// registers, then a log2(256)-step LDS tree merges them. Overflowed rows
// (count > cap: emission skipped stores) write idx[0] = -2 so the host
// falls back to the list-epilogue kernel — the exactness guard.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emit_merge_topk(
    const unsigned long long* __restrict__ cand,
    const unsigned* __restrict__ ccount, float* __restrict__ out_s,
    long* __restrict__ out_i, int B, long cap, int k) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const unsigned cnt = ccount[row];
  if (cnt > (unsigned)cap) {
    if (tid == 0) {
      for (int q = 0; q < k; ++q) {
        out_s[(size_t)row * k + q] = NEG_INF;
        out_i[(size_t)row * k + q] = q == 0 ? -2 : -1;
      }
    }
    return;
  }
  unsigned long long loc[KMAX];  // sorted desc; 0 = empty sentinel
#pragma unroll
  for (int q = 0; q < KMAX; ++q) loc[q] = 0ull;
  const unsigned long long* crow = cand + (size_t)row * cap;
  for (unsigned i = tid; i < cnt; i += 256) {
    const unsigned long long v = crow[i];
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
  __shared__ unsigned long long all[256 * KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) all[tid * KMAX + q] = loc[q];
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      // two-pointer merge of two sorted-desc KMAX lists -> top KMAX
      // (LDS-indexed: a register array would go to scratch)
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
  if (tid == 0) {
    for (int q = 0; q < k; ++q) {
      const unsigned long long v = all[q];
      if (v == 0ull) {
        out_s[(size_t)row * k + q] = NEG_INF;
        out_i[(size_t)row * k + q] = -1;
      } else {
        out_s[(size_t)row * k + q] = dec_f32((unsigned)(v >> 32));
        out_i[(size_t)row * k + q] = 0x7fffffffL - (long)(v & 0xffffffffu);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// k-means centroid update: segmented reduction of bf16 points into
// per-cluster fp32 sums + counts. Grid: (dim-tiles, point-chunks); each
// block accumulates a [C][64]-dim LDS partial over its point chunk, then
// adds it to the global sums once. C <= 512. C <= 128 keeps R = 4 replicas
// of the partial (one per point lane, no atomics), C > 128 keeps R = 1 and
// adds with LDS atomics; LDS = (R*C*64 + C)*4 bytes, the [C] tail being the
// counts partial: 128.5 KiB at C = 128, 130 KiB at C = 512, so the binding raises
// the dynamic LDS cap above 64 KiB when needed. Points whose assignment is
// outside [0, C) are dropped from sums and counts. Points are read exactly once per dim-tile (coalesced 128-B row slices);
// bandwidth-bound by design, replacing torch index_add_ (which was ~30x
// over the I/O floor in benchmarks/kmeans_bench.py).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_update_kernel(
    const bf16_t* __restrict__ points, const int* __restrict__ assign,
    float* __restrict__ sums, float* __restrict__ counts, int N, int D,
    int C, int points_per_chunk) {
  // C <= 128: FOUR replicas of the [C][64] partial, one per point lane, so
  // the inner loop is a plain LDS read+add+write on a slot owned by exactly
  // one thread — the single-replica per-element atomicAdd version measured
  // LDS-atomic-bound (~385 GB/s, 40 ms at 10M x 768). C > 128: one replica
  // with atomics (LDS budget).
  extern __shared__ float part[];  // [R][C][64] sums + [C] counts
  const int R = (C <= 128) ? 4 : 1;
  const int tid = threadIdx.x;
  const int d0 = blockIdx.x * 64;
  const int p0 = blockIdx.y * points_per_chunk;
  const int pend = min(p0 + points_per_chunk, N);

  float* cpart = part + R * C * 64;
  for (int i = tid; i < R * C * 64 + C; i += 256) part[i] = 0.f;
  __syncthreads();

  // thread (pl, d) = (tid>>6, tid&63); 16 points batched per pass so the
  // 2-byte strided loads stack up in flight (the 4-in-flight version was
  // load-latency-bound at ~350 GB/s: each iteration's LDS add depended on
  // its own just-issued load)
  const int pl = tid >> 6;
  const int d = tid & 63;
  float* mypart = part + (R == 4 ? pl * C * 64 : 0);
  constexpr int PU = 16;
  int p = p0 + pl;
  for (; p + 4 * (PU - 1) < pend; p += 4 * PU) {
    float v[PU];
    int a[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int pp = p + 4 * u;
      a[u] = assign[pp];
      v[u] = (float)points[(size_t)pp * D + d0 + d];
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      if (a[u] >= 0 && a[u] < C) {
        if (R == 4)
          mypart[a[u] * 64 + d] += v[u];  // slot owned by this (pl, d) thread
        else
          atomicAdd(&part[a[u] * 64 + d], v[u]);
      }
    }
  }
  for (; p < pend; p += 4) {
    const int a = assign[p];
    const float v = (float)points[(size_t)p * D + d0 + d];
    if (a >= 0 && a < C) {
      if (R == 4)
        mypart[a * 64 + d] += v;
      else
        atomicAdd(&part[a * 64 + d], v);
    }
  }
  __syncthreads();

  for (int i = tid; i < C * 64; i += 256) {
    float v = part[i];
    if (R == 4) v += part[C * 64 + i] + part[2 * C * 64 + i] + part[3 * C * 64 + i];
    if (v != 0.f)
      atomicAdd(&sums[(size_t)(i / 64) * D + d0 + i % 64], v);
  }
  // counts: LDS partial first (the naive global-atomic version costs ~1M
  // contended RMWs per batch), then C adds per chunk
  if (blockIdx.x == 0) {
    for (int p = p0 + tid; p < pend; p += 256) {
      const int a = assign[p];
      if (a >= 0 && a < C) atomicAdd(&cpart[a], 1.0f);
    }
    __syncthreads();
    for (int i = tid; i < C; i += 256)
      if (cpart[i] != 0.f) atomicAdd(&counts[i], cpart[i]);
  }
}

// ---------------------------------------------------------------------------
// Merge per-chunk partial lists -> final sorted top-k per query row.
//   grid = B blocks, 256 threads.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void topk_merge(
    const float* __restrict__ partial_score, const int* __restrict__ partial_idx,
    float* __restrict__ out_score, long* __restrict__ out_idx,
    int nchunks, int k) {
  __shared__ float sc[THREADS * KMAX];
  __shared__ int si[THREADS * KMAX];

  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int total = nchunks * KMAX;
  const size_t base = (size_t)row * total;

  float ls[KMAX];
  int li[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { ls[q] = NEG_INF; li[q] = -1; }
  float lmin = NEG_INF;

  for (int e = tid; e < total; e += THREADS) {
    const float s = partial_score[base + e];
    if (s > lmin) {
      // replace current min
      int mp = 0;
      float mn = ls[0];
#pragma unroll
      for (int q = 1; q < KMAX; ++q)
        if (ls[q] < mn) { mn = ls[q]; mp = q; }
#pragma unroll
      for (int q = 0; q < KMAX; ++q)
        if (q == mp) { ls[q] = s; li[q] = partial_idx[base + e]; }
      lmin = ls[0];
#pragma unroll
      for (int q = 1; q < KMAX; ++q) lmin = fminf(lmin, ls[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < KMAX; ++q) {
    sc[tid * KMAX + q] = ls[q];
    si[tid * KMAX + q] = li[q];
  }
  __syncthreads();

  if (tid == 0) {
    float fs[KMAX];
    int fi[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) { fs[q] = NEG_INF; fi[q] = -1; }
    for (int e = 0; e < THREADS * KMAX; ++e) {
      const float s = sc[e];
      int mp = 0;
      float mn = fs[0];
#pragma unroll
      for (int q = 1; q < KMAX; ++q)
        if (fs[q] < mn) { mn = fs[q]; mp = q; }
      if (s > mn) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q)
          if (q == mp) { fs[q] = s; fi[q] = si[e]; }
      }
    }
    // sort descending (insertion sort, KMAX small)
#pragma unroll
    for (int a = 1; a < KMAX; ++a) {
      const float s = fs[a];
      const int ix = fi[a];
      int b = a - 1;
      for (; b >= 0 && fs[b] < s; --b) { fs[b + 1] = fs[b]; fi[b + 1] = fi[b]; }
      fs[b + 1] = s;
      fi[b + 1] = ix;
    }
    for (int q = 0; q < k; ++q) {
      out_score[(size_t)row * k + q] = fs[q] <= NEG_INF ? -INFINITY : fs[q];
      out_idx[(size_t)row * k + q] = fi[q];
    }
  }
}

// ---------------------------------------------------------------------------
// Small-candidate merge: one THREAD per query row (the block-per-row merge
// above serialises a 2048-entry scan on thread 0, which dominates when B
// is large and nchunks small — e.g. k-means assignment at B=1M, C=64).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_merge_small(
    const float* __restrict__ partial_score, const int* __restrict__ partial_idx,
    float* __restrict__ out_score, long* __restrict__ out_idx, int B,
    int nchunks, int k) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  const int total = nchunks * KMAX;
  const size_t base = (size_t)row * total;
  float ls[KMAX];
  int li[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { ls[q] = NEG_INF; li[q] = -1; }
  float lmin = NEG_INF;
  for (int e = 0; e < total; ++e) {
    const float s = partial_score[base + e];
    if (s > lmin) {
      int mp = 0;
      float mn1 = ls[0], mn2 = 1e38f;
#pragma unroll
      for (int q = 1; q < KMAX; ++q) {
        if (ls[q] < mn1) { mn2 = mn1; mn1 = ls[q]; mp = q; }
        else if (ls[q] < mn2) { mn2 = ls[q]; }
      }
#pragma unroll
      for (int q = 0; q < KMAX; ++q)
        if (q == mp) { ls[q] = s; li[q] = partial_idx[base + e]; }
      lmin = fminf(mn2, s);
    }
  }
  // sort descending (insertion sort over KMAX)
#pragma unroll
  for (int a = 1; a < KMAX; ++a) {
    const float s = ls[a];
    const int ix = li[a];
    int b = a - 1;
    for (; b >= 0 && ls[b] < s; --b) { ls[b + 1] = ls[b]; li[b + 1] = li[b]; }
    ls[b + 1] = s;
    li[b + 1] = ix;
  }
  for (int q = 0; q < k; ++q) {
    out_score[(size_t)row * k + q] = ls[q] <= NEG_INF ? -INFINITY : ls[q];
    out_idx[(size_t)row * k + q] = li[q];
  }
}

// ---------------------------------------------------------------------------
// Row-wise L2 normalisation, in place. One wave per row, bf16x8 loads.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void l2normalize_rows(
    bf16_t* __restrict__ data, int start_row, int nrows, int D) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves_per_grid = gridDim.x * (THREADS / 64);

  for (int r = blockIdx.x * (THREADS / 64) + wave; r < nrows;
       r += waves_per_grid) {
    bf16_t* row = data + (size_t)(start_row + r) * D;
    float ss = 0.f;
    for (int d = lane * 8; d < D; d += 64 * 8) {
      const bf16x8 v = *(const bf16x8*)(row + d);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float f = (float)v[i];
        ss += f * f;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float scale = (ss > 1e-24f) ? rsqrtf(ss) : 0.f;
    for (int d = lane * 8; d < D; d += 64 * 8) {
      bf16x8 v = *(const bf16x8*)(row + d);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (bf16_t)((float)v[i] * scale);
      *(bf16x8*)(row + d) = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Weighted embedding bag: out[b] = sum_l w[b,l] * table[idx[b,l]].
//   table [V][D] bf16, idx [B][L] i32, w [B][L] f32 -> out [B][D] f32.
//   One block per bag; threads stride over D.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void embedding_bag_kernel(
    const bf16_t* __restrict__ table, const int* __restrict__ idx,
    const float* __restrict__ w, float* __restrict__ out, int L, int D,
    int V) {
  __shared__ int s_idx[128];
  __shared__ float s_w[128];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  for (int l = tid; l < L; l += THREADS) {
    s_idx[l] = idx[(size_t)b * L + l];
    s_w[l] = w[(size_t)b * L + l];
  }
  __syncthreads();

  for (int d = tid; d < D; d += THREADS) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
      const float wl = s_w[l];
      if (wl != 0.f) {
        const int ix = s_idx[l];
        if (ix >= 0 && ix < V) acc += wl * (float)table[(size_t)ix * D + d];
      }
    }
    out[(size_t)b * D + d] = acc;
  }
}

// ---------------------------------------------------------------------------
// k-means assignment: N points x C centroids (C <= 64), argmax per point.
//
// The general cosine_topk path is built for huge corpora: at the pattern-
// detector shape (N=10M points as "queries", C=64 centroids as the
// "corpus") its 12-window staged pipeline runs with one 64-valid-column
// tile, nothing to overlap, and a per-block B-restage — measured ~440 GB/s
// effective vs the ~8 TB/s point-stream bound (ROUND2.md). This kernel is
// shaped for that case instead:
//   - centroids are staged into LDS ONCE per block (row-padded pitch so the
//     16-lane fragment reads spread across all 64 banks) and stay resident
//     for every point tile the block processes;
//   - point MFMA A-fragments stream straight from HBM into registers
//     (16 B/lane, sector-coalesced) through a 1-window register prefetch —
//     no LDS staging, no per-window barriers at all;
//   - 8 waves x 32 rows = 256 points per tile, grid-strided so one launch
//     covers any N; the argmax epilogue is pure registers + shfl.
// ---------------------------------------------------------------------------
constexpr int ASSIGN_THREADS = 512;  // 8 waves

// Row pitch for the centroid LDS image: pad so pitch % 256 == 64, which
// makes the 64 lanes of a fragment read (16 rows x 4 slot-groups of 16 B)
// land on 64 distinct banks — the minimum 4 conflict-free phases for a
// 1 KiB ds_read_b128 wave. (A 16 B pad measured as a 4x conflict: lanes
// with equal cl+g collided.)
constexpr __host__ __device__ int assign_pitch(int D) {
  return D * 2 + ((64 - (D * 2) % 256) + 256) % 256;
}

// The 64-row centroid image must fit the 160 KiB of LDS a block can have,
// which bounds D: 1152 is the widest row that fits, 1216 the first that
// does not. ops.kmeans_assign_scored mirrors this rule to send wider rows
// (and C > 64) to the general cosine_topk kernels instead
// (kakveda_amd/ops/__init__.py assign_kernel_fits, pinned by
// tests/test_aux_cases_ref.py).
constexpr int ASSIGN_LDS_BYTES = 160 * 1024;
constexpr __host__ __device__ bool assign_fits_lds(int D) {
  return 64 * assign_pitch(D) <= ASSIGN_LDS_BYTES;
}
constexpr int kmeans_assign_max_d() {
  int d = 64;
  while (assign_fits_lds(d + 64)) d += 64;
  return d;
}
static_assert(kmeans_assign_max_d() == 1152 && !assign_fits_lds(1216),
              "update KMEANS_ASSIGN_MAX_D in kakveda_amd/ops/__init__.py");

__global__ __launch_bounds__(ASSIGN_THREADS, 1) void kmeans_assign_kernel(
    const bf16_t* __restrict__ P, const bf16_t* __restrict__ Cc,
    float* __restrict__ out_score, int* __restrict__ out_idx,
    int N, int D, int C) {
  extern __shared__ char cmem[];  // 64 centroid rows, padded pitch
  const int pitch = assign_pitch(D);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int g = lane >> 4, cl = lane & 15;

  // stage centroids once; rows >= C zero-filled so their MFMAs stay finite
  for (int s = tid; s < 64 * (D / 8); s += ASSIGN_THREADS) {
    const int c = s / (D / 8);
    const int so = s % (D / 8);
    bf16x8 v = {};
    if (c < C)
      v = *(const bf16x8*)((const char*)Cc + ((size_t)c * D + (size_t)so * 8) * 2);
    *(bf16x8*)(cmem + (size_t)c * pitch + so * 16) = v;
  }
  __syncthreads();

  const long prow = (long)D * 2;
  const int nkt = D / 64;
  for (long tile0 = (long)blockIdx.x * 256; tile0 < N;
       tile0 += (long)gridDim.x * 256) {
    const long r0 = tile0 + (long)wid * 32;  // this wave's 32 rows
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A fragments direct global->register. Straight-line, unroll-by-3
    // window loop with THREE named prefetch buffers and 2 windows always
    // in flight: a branchy 1-deep version compiled to a `s_waitcnt
    // vmcnt(0)` before every MFMA phase (the conditional prefetch block
    // defeats counted waits) and measured 153 GB/s; straight-line code
    // lets the compiler emit counted vmcnt waits so the point stream
    // pipelines. Tail rows clamp to the last point (results masked at
    // the write below); past-the-end windows clamp to the last window
    // (redundant re-reads, still straight-line).
    bf16x8 a0[2][2], a1[2][2], a2[2][2];  // [kk][m]
    auto lda = [&](bf16x8 (&dst)[2][2], int kt) {
      if (kt >= nkt) kt = nkt - 1;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          long r = r0 + m * 16 + cl;
          if (r >= N) r = N - 1;
          dst[kk][m] = *(const bf16x8*)((const char*)P + r * prow +
                                        (size_t)(kt * 8 + kk * 4 + g) * 16);
        }
    };
    auto mfma_win = [&](bf16x8 (&src)[2][2], int kt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 bfrag[4];
        const int slot = kt * 8 + kk * 4 + g;
#pragma unroll
        for (int n = 0; n < 4; ++n)
          bfrag[n] =
              *(const bf16x8*)(cmem + (size_t)(n * 16 + cl) * pitch + slot * 16);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                src[kk][m], bfrag[n], acc[m][n], 0, 0, 0);
      }
    };
    lda(a0, 0);
    lda(a1, 1);
    int kt = 0;
    for (; kt + 2 < nkt; kt += 3) {
      lda(a2, kt + 2);
      mfma_win(a0, kt);
      lda(a0, kt + 3);
      mfma_win(a1, kt + 1);
      lda(a1, kt + 4);
      mfma_win(a2, kt + 2);
    }
    if (kt < nkt) mfma_win(a0, kt);
    if (kt + 1 < nkt) mfma_win(a1, kt + 1);

    // argmax per row over 64 cols (cols >= C masked; ties -> lowest col,
    // matching torch.argmax / the CPU reference)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float best = NEG_INF;
        int bcol = 0x7fffffff;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int col = n * 16 + cl;
          const float v = acc[m][n][reg];
          if (col < C && (v > best || (v == best && col < bcol))) {
            best = v;
            bcol = col;
          }
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          const float ov = __shfl_xor(best, off, 64);
          const int oc = __shfl_xor(bcol, off, 64);
          if (ov > best || (ov == best && oc < bcol)) {
            best = ov;
            bcol = oc;
          }
        }
        const long row = r0 + m * 16 + g * 4 + reg;
        if (cl == 0 && row < N) {
          out_score[row] = best;
          out_idx[row] = bcol;
        }
      }
    }
  }
}

}  // namespace kakveda

