// Contract of the int8 row mirror (the kernels are in q8_impl.h, the torch
// reference in ops/__init__.py quantize_rows_q8_ref / cosine_topk_q8_ref).
// Pure C++ (no HIP, no torch): the constants and the serial statement of the
// quantiser, usable from host and device code.
//
// For a row c of D values (bf16 on the device; D % Q8_SEG == 0) the mirror
// holds
//   amax  = max |c_i|
//   scale = amax / 127.0f            (IEEE fp32 divide)
//   inv   = 127.0f / amax
//   n_i   = clamp(rintf(c_i * inv), -127, 127)   as int8: one fp32 multiply,
//           round half to even
//   err  >= || c - scale * n ||_2    evaluated exactly
// stored as int8 [rows, D] codes and float [rows, 2] (scale, err) meta. A row
// with amax < Q8_MIN_AMAX (all-zero rows, and rows so small that inv would
// overflow) is stored as scale = 0, n = 0, err >= ||c||: err = 0 for the
// all-zero row, and nothing is NaN or Inf for any finite row.
//
// err. The kernel evaluates d_i = fma(-scale, n_i, c_i) (c_i, n_i and scale
// are exact fp32 values, so d_i is the real difference rounded once: relative
// error <= u = 2^-24), sums the D squares in fp32 in some order and takes the
// square root. Each square adds one rounding to the two of d_i^2, a sum of D
// non-negative terms is within (D - 1) u relative of its real value in any
// order, and the root halves the relative error of its argument and adds one
// rounding: the computed norm is >= true * (1 - ((D + 2) / 2 + 1) u) to first
// order. Multiplying by 1 + (D + 16) u, itself one rounding, therefore gives
// a value >= the true norm for every D < 2^20 (the second-order terms are
// below 16 u / 2 there). Squares of |d_i| < 2^-63 lose precision to underflow
// or are flushed; together they hide less than sqrt(D) * 2^-63 < 2^-53 of the
// norm, which the additive Q8_ERR_ABS covers. At D = 768 the factor is
// 1 + 4.7e-5: against the 1% the search could tolerate, the stored error is
// as tight as the fp32 norm itself.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define Q8_HD __host__ __device__ inline
#else
#define Q8_HD inline
#endif

namespace kakveda {

constexpr int Q8_SEG = 128;          // codes per 128-byte segment of a row
constexpr float Q8_MIN_AMAX = 0x1p-100f;
constexpr float Q8_ERR_ABS = 0x1p-50f;

Q8_HD bool q8_dim_ok(long D) { return D >= Q8_SEG && D % Q8_SEG == 0 && D < (1L << 20); }

// Factor that rounds an fp32 norm of D terms up past its real value (above).
Q8_HD float q8_roundup(int D) { return 1.0f + (float)(D + 16) * 0x1p-24f; }

struct Q8Scale {
  float scale, inv;
};

// amax -> (scale, inv); (0, 0) for a row stored as zeros.
Q8_HD Q8Scale q8_scale(float amax) {
  if (!(amax >= Q8_MIN_AMAX)) return {0.0f, 0.0f};
  return {amax / 127.0f, 127.0f / amax};
}

// One code. inv == 0 (a row stored as zeros) gives 0.
Q8_HD int8_t q8_code(float c, float inv) {
  const float r = rintf(c * inv);
  return (int8_t)fminf(fmaxf(r, -127.0f), 127.0f);
}

// Stored error from the fp32 norm of the residual (live row) or of the row
// itself bounded by amax * sqrt(D) (row stored as zeros; 0 for amax == 0).
Q8_HD float q8_err(float norm, float amax, float scale, int D) {
  if (scale == 0.0f) return amax * sqrtf((float)D) * q8_roundup(D);
  return norm * q8_roundup(D) + Q8_ERR_ABS;
}

// Slack of the stage-1 emission test, on top of the row's error margin: the
// int8 score and the bf16 score of the streaming kernel are each within
// D * 2^-24 of their real values for unit rows (q8_impl.h); twice that, and
// as much again for the roundings of the test itself.
Q8_HD float q8_slack(int D) { return (float)D * 0x1p-22f; }

// ---------------------------------------------------------------------------
// Screening test of the batched path (kernels: q8_screen_impl.h; torch
// reference: ops/__init__.py q8_screen_mask_ref).
//
// The queries of a call are quantised by the corpus quantiser: q^ = sq * nq,
// errq >= ||q - q^||, and nqh >= ||q^|| = sq * sqrt(sum nq_i^2) (the sum is an
// exact integer below 2^24, the root and the product one rounding each:
// q8_roundup covers them). For a corpus row c with mirror c^ = sc * nc,
//   q.c = q^.c^ + (q - q^).c + q^.(c - c^)
//      <= sq * sc * acc + errq * ||c|| + nqh * err_c          (Cauchy-Schwarz)
// where acc = sum nq_i nc_i is the exact int32 dot of the codes. With cnorm >=
// the largest row norm of the segment (kept by the store, rounded up like err),
// (query r, column c) is a CANDIDATE iff
//   sq_r * sc_c * acc + nqh_r * err_c + errq_r * cnorm + q8_slack(D) >= floor_r
// (q8_screen_ref below). floor_r is the floor the bf16 prepass published; the
// bf16 kernels emit a pair iff their fp32 score reaches it, and that score is
// within D * 2^-24 of q.c for unit rows, the first half of q8_slack. So every
// pair the bf16 search emits is a candidate.
//
// The kernel's form (q8_screen_fast): with kappa >= nqh_r / sq_r for every row
// of the launch and sq_r > 0,
//   v = fma(float(acc), sc_c, kappa * err_c)   >=   T_r
//   T_r <= (floor_r - errq_r * cnorm - q8_slack(D)) / sq_r
// holds for every candidate: dividing the test by sq_r and replacing
// nqh_r / sq_r by the larger kappa only grows the left side. float(acc) is
// exact for |acc| <= D * 127^2 < 2^24, i.e. D <= Q8_SCREEN_MAX_D. The roundings
// of v (two) and of T_r (q8_screen_threshold lowers it explicitly past its
// own) are relative 2^-24 of magnitudes that, times sq_r, stay below 2 for
// unit rows: under 2^-21 in score units against the D * 2^-23 >= 2^-16 the
// second half of q8_slack leaves for them. A query with sq_r == 0 (stored as
// zeros) has no T_r: a batch that holds one takes the bf16 path.
//
// Staged floors (knn_plan.h plan_q8_stages, q8_refresh_floor). The main launch
// runs as stages over disjoint column ranges, and between two stages floor_r
// is raised to the k-th best bf16 score among the entries row r holds so far
// (seeds and rescored candidates; k is the request's). The result stays exact:
// let s_k be the k-th best bf16 score of row r over the whole corpus. Any k
// columns score at most as well as the best k, so the k-th best of ANY subset
// of the columns is <= s_k: every floor a stage reads, the prepass's included,
// is <= s_k. A column of the final top-k scores >= s_k >= that floor, so by
// the argument above it is a candidate of the stage that scans it (or a seed)
// and is rescored. The test is >=, so columns tied with the floor are still
// emitted and the merge breaks the tie by column as before. Stages are
// disjoint and the seeds lie ahead of the first, so no pair is entered twice.
// A row with fewer than k entries, or past its capacity, raises nothing.
// ---------------------------------------------------------------------------
constexpr int Q8_SCREEN_MAX_D = 1024;  // 1024 * 127^2 < 2^24 <= 1152 * 127^2

Q8_HD bool q8_screen_dim_ok(long D) { return q8_dim_ok(D) && D <= Q8_SCREEN_MAX_D; }

// nqh >= ||sq * nq|| from the exact integer sum of the squared codes.
Q8_HD float q8_code_norm(float sq, long sumsq, int D) {
  return sq * sqrtf((float)sumsq) * q8_roundup(D) + Q8_ERR_ABS;
}

// Norm of a row from the fp32 sum of its squares, rounded up (cnorm's terms).
Q8_HD float q8_norm_up(float sumsq, int D) {
  return sqrtf(sumsq) * q8_roundup(D) + Q8_ERR_ABS;
}

// kappa's term of one row: >= nqh / sq (sq > 0).
Q8_HD float q8_screen_kappa(float nqh, float sq) {
  return (nqh / sq) * (1.0f + 0x1p-22f);
}

// T_r, rounded down past the three roundings of its evaluation (sq > 0).
// NEG_INF-like floors (nothing published) give a hugely negative or -inf T:
// every column is then a candidate, as under the bf16 kernels.
Q8_HD float q8_screen_threshold(float floor, float sq, float errq, float cnorm,
                                int D) {
  const float e = errq * cnorm * (1.0f + 0x1p-22f);
  const float mag = fabsf(floor) + e + q8_slack(D);
  const float num = floor - e - q8_slack(D) - mag * 0x1p-21f;
  const float t = num / sq;
  return t - fabsf(t) * 0x1p-22f;
}

// The contract, serially and in double: is (query, column) a candidate?
inline bool q8_screen_ref(long acc, float sq, float sc, float nqh, float err,
                          float errq, float cnorm, float floor, int D) {
  const double lhs = (double)sq * (double)sc * (double)acc +
                     (double)nqh * (double)err + (double)errq * (double)cnorm +
                     (double)q8_slack(D);
  return lhs >= (double)floor;
}

// The kernel's test, as the kernel evaluates it.
Q8_HD bool q8_screen_fast(int acc, float sc, float err, float kappa, float T) {
  return fmaf((float)acc, sc, kappa * err) >= T;
}

}  // namespace kakveda
