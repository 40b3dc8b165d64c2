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

}  // namespace kakveda
