// The device featurizer's contract, host and device: the byte class and
// lower-casing of the tokeniser, the FNV-1a step, the bucket and sign rule,
// the capacity limits, and featurize_one, a plain serial statement of what
// one text's row is (encoder/featurizer.py featurize_batch, restated for
// bytes). The kernel (featurize_impl.h) is built from the same pieces; the
// serial function is checked on the CPU against the Python featurizer
// (tests/host/featurize_plan_test.cpp). Pure C++: no HIP, no torch.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FEAT_HD __host__ __device__
#else
#define FEAT_HD
#endif

namespace kakveda {

// Capacity of one text. Longer texts, and texts with more grams, are not
// featurised on the device: their row is flagged and the host does it.
constexpr int FEATURIZE_MAX_BYTES = 1024;  // bytes per text
constexpr int FEATURIZE_MAX_GRAMS = 256;   // uni+bigrams before de-duplication
// T tokens make 2T-1 grams
constexpr int FEATURIZE_MAX_TOKENS = (FEATURIZE_MAX_GRAMS + 1) / 2;
constexpr int FEATURIZE_MAX_FEATURES = 128;  // embedding_bag's L limit

// status of a row
constexpr int FEATURIZE_OK = 0;
// over capacity: more than FEATURIZE_MAX_BYTES bytes (or offsets that do
// not lie inside the buffer) or more than FEATURIZE_MAX_GRAMS grams
constexpr int FEATURIZE_TOO_MANY_GRAMS = 1;
constexpr int FEATURIZE_TOO_MANY_FEATURES = 2;  // more than max_features buckets

constexpr uint64_t FEAT_FNV_OFFSET = 0xCBF29CE484222325ull;
constexpr uint64_t FEAT_FNV_PRIME = 0x100000001B3ull;
constexpr uint64_t FEAT_SEED_MUL = 0x9E3779B97F4A7C15ull;

// Start state of every gram hash (seed taken mod 2^64).
FEAT_HD inline uint64_t feat_start_state(uint64_t seed) {
  return FEAT_FNV_OFFSET ^ (seed * FEAT_SEED_MUL);
}

// ASCII lower-casing: only A-Z move.
FEAT_HD inline unsigned feat_lower(unsigned b) {
  return (b - 'A' < 26u) ? b + 32u : b;
}

// Token bytes, after lower-casing: a-z 0-9 _ : . -   Everything else is a
// separator, bytes >= 0x80 included. 0 is never a token byte, which lets
// the kernel keep separators as 0 in its lower-cased image.
FEAT_HD inline bool feat_is_token(unsigned c) {
  return (c - 'a' < 26u) || (c - '0' < 10u) || c == '_' || c == ':' || c == '.' ||
         c == '-';
}

FEAT_HD inline uint64_t feat_fnv_step(uint64_t h, unsigned b) {
  return (h ^ (uint64_t)b) * FEAT_FNV_PRIME;
}

FEAT_HD inline int32_t feat_bucket(uint64_t h, uint32_t hash_dim) {
  return (int32_t)(h % (uint64_t)hash_dim);
}

// +1 when bit 62 is set, else -1.
FEAT_HD inline float feat_sign(uint64_t h) {
  return ((h >> 62) & 1ull) ? 1.0f : -1.0f;
}

// One distinct key as a sortable word: bucket in the high half, the bits of
// its term sign * sqrt(count) in the low half. Sorting these words groups
// the buckets ascending and fixes the order their terms are summed in.
FEAT_HD inline uint64_t feat_entry(uint64_t h, uint32_t count, uint32_t hash_dim) {
  const float term = feat_sign(h) * sqrtf((float)count);
  uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
  bits = __float_as_uint(term);
#else
  std::memcpy(&bits, &term, 4);
#endif
  return ((uint64_t)(uint32_t)feat_bucket(h, hash_dim) << 32) | bits;
}

FEAT_HD inline int32_t feat_entry_bucket(uint64_t e) { return (int32_t)(e >> 32); }

FEAT_HD inline float feat_entry_term(uint64_t e) {
  const uint32_t bits = (uint32_t)e;
  float term;
#if defined(__HIP_DEVICE_COMPILE__)
  term = __uint_as_float(bits);
#else
  std::memcpy(&term, &bits, 4);
#endif
  return term;
}

// The row of one text: idx/w get max_features entries each (features sorted
// by bucket, weights L2-normalised, then (0, 0) padding). Returns the row's
// status; a row whose status is not FEATURIZE_OK is all zeros. Serial and
// unhurried: this is the definition the kernel is held to.
inline int featurize_one(const uint8_t* text, long len, uint32_t hash_dim,
                         uint64_t start_state, int max_features, int32_t* idx,
                         float* w) {
  for (int j = 0; j < max_features; ++j) {
    idx[j] = 0;
    w[j] = 0.0f;
  }
  if (len < 0 || len > FEATURIZE_MAX_BYTES) return FEATURIZE_TOO_MANY_GRAMS;

  // tokens -> gram keys; the bigram continues from the state after t_i
  uint64_t keys[FEATURIZE_MAX_GRAMS];
  int n_keys = 0;
  long n_tokens = 0;
  uint64_t prev = 0;  // state after the previous token
  long p = 0;
  while (p < len) {
    if (!feat_is_token(feat_lower(text[p]))) {
      ++p;
      continue;
    }
    uint64_t uni = start_state;
    uint64_t big = n_tokens ? feat_fnv_step(prev, 0x20) : 0;
    for (; p < len && feat_is_token(feat_lower(text[p])); ++p) {
      const unsigned c = feat_lower(text[p]);
      uni = feat_fnv_step(uni, c);
      big = feat_fnv_step(big, c);
    }
    const int grams = n_tokens ? 2 : 1;
    if (n_keys + grams > FEATURIZE_MAX_GRAMS) return FEATURIZE_TOO_MANY_GRAMS;
    keys[n_keys++] = uni;
    if (n_tokens) keys[n_keys++] = big;
    prev = uni;
    ++n_tokens;
  }
  if (n_keys == 0) return FEATURIZE_OK;

  // count per distinct key -> one (bucket, term) entry each
  std::sort(keys, keys + n_keys);
  uint64_t ent[FEATURIZE_MAX_GRAMS];
  int n_ent = 0;
  for (int i = 0; i < n_keys;) {
    int j = i;
    while (j < n_keys && keys[j] == keys[i]) ++j;
    ent[n_ent++] = feat_entry(keys[i], (uint32_t)(j - i), hash_dim);
    i = j;
  }

  // sum per bucket, in entry order
  std::sort(ent, ent + n_ent);
  int32_t fidx[FEATURIZE_MAX_GRAMS];
  float fw[FEATURIZE_MAX_GRAMS];
  int n_feat = 0;
  for (int i = 0; i < n_ent;) {
    float s = 0.0f;
    int j = i;
    for (; j < n_ent && feat_entry_bucket(ent[j]) == feat_entry_bucket(ent[i]); ++j)
      s += feat_entry_term(ent[j]);
    fidx[n_feat] = feat_entry_bucket(ent[i]);
    fw[n_feat++] = s;
    i = j;
  }
  if (n_feat > max_features) return FEATURIZE_TOO_MANY_FEATURES;

  float sq = 0.0f;
  for (int i = 0; i < n_feat; ++i) sq += fw[i] * fw[i];
  const float norm = sqrtf(sq);
  for (int i = 0; i < n_feat; ++i) {
    idx[i] = fidx[i];
    w[i] = norm > 0.0f ? fw[i] / norm : fw[i];
  }
  return FEATURIZE_OK;
}

}  // namespace kakveda
