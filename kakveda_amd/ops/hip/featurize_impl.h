// Device featurizer: raw signature-text bytes -> the padded [B, L] index and
// weight rows of encoder/featurizer.py featurize_batch. Included by
// kakveda_kernels.hip; the contract and every shared piece (byte class, FNV
// step, bucket and sign rule, capacities) live in featurize_plan.h, whose
// serial featurize_one is what this kernel is held to.
//
// One 64-lane wave per text, FEATURIZE_TEXTS_PER_BLOCK texts per block. The
// waves of a block never meet: there is no block barrier, each wave works
// in its own slice of LDS and orders its LDS traffic with feat_wave_sync
// (LDS operations of one wave complete in issue order; the fence only keeps
// the compiler from moving them). Steps of a wave:
//   1. load the text in 64-byte steps, lower-case and classify; keep the
//      lower-cased image in LDS with separators as 0; a ballot per step,
//      with the last lane's class carried into the next step, marks token
//      starts, and a running popcount numbers them;
//   2. one lane per token hashes it (the unigram key) and goes on through
//      0x20 and the next token (the bigram key);
//   3. bitonic sort of the 64-bit keys in LDS, run-length count, one
//      (bucket, sign * sqrt(count)) entry per distinct key;
//   4. bitonic sort of the entries by bucket, sum per bucket;
//   5. squared norm across the wave, then the row goes out with plain
//      vector stores, padded with (0, 0).
// A text over capacity, or with more than max_features buckets, gets a zero
// row and a non-zero status; `flagged` counts those rows (atomicAdd) so the
// host reads one integer when nothing was flagged.
//
// A latency kernel: a typical signature (180 bytes, ~25 tokens) is 3 load
// steps, a 64-key sort and a 64-entry sort. Nothing here is tuned.
#pragma once

#include <hip/hip_runtime.h>
#include "featurize_plan.h"

namespace kakveda {

constexpr int FEATURIZE_TEXTS_PER_BLOCK = 4;

// LDS of one wave
struct FeatWaveLds {
  unsigned long long keys[FEATURIZE_MAX_GRAMS];  // gram keys; later the features
  unsigned long long ent[FEATURIZE_MAX_GRAMS];   // (bucket, term) entries
  unsigned char bytes[FEATURIZE_MAX_BYTES];      // lower-cased image, separators 0
  unsigned short tok_start[FEATURIZE_MAX_TOKENS];
};

__device__ inline void feat_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lanes below this one
__device__ inline unsigned long long feat_lanes_below(int lane) {
  return (1ull << lane) - 1ull;
}

// Ascending bitonic sort of s[0, n), n a power of two <= FEATURIZE_MAX_GRAMS,
// by one wave.
__device__ inline void feat_bitonic_sort(unsigned long long* s, int n, int lane) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < n; i += 64) {
        const int o = i ^ j;
        if (o > i) {
          const unsigned long long a = s[i], b = s[o];
          if ((a > b) == ((i & k) == 0)) {
            s[i] = b;
            s[o] = a;
          }
        }
      }
      feat_wave_sync();
    }
  }
}

__device__ inline int feat_pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

__global__ __launch_bounds__(64 * FEATURIZE_TEXTS_PER_BLOCK) void featurize_bytes_kernel(
    const unsigned char* __restrict__ buf, long buf_len,
    const int* __restrict__ offsets, int B, unsigned hash_dim,
    unsigned long long start_state, int max_features, int* __restrict__ out_idx,
    float* __restrict__ out_w, int* __restrict__ out_status,
    int* __restrict__ flagged) {
  __shared__ FeatWaveLds lds_all[FEATURIZE_TEXTS_PER_BLOCK];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * FEATURIZE_TEXTS_PER_BLOCK + wid;
  if (b >= B) return;  // whole wave; no block barrier anywhere below
  FeatWaveLds& lds = lds_all[wid];

  const long off0 = offsets[b], off1 = offsets[b + 1];
  const bool readable = off0 >= 0 && off1 >= off0 && off1 <= buf_len;
  const int len = readable ? (int)(off1 - off0 < FEATURIZE_MAX_BYTES + 1
                                       ? off1 - off0
                                       : FEATURIZE_MAX_BYTES + 1)
                           : 0;

  int status = FEATURIZE_OK;
  int n_feat = 0;    // features of the row, valid when status stays OK
  float norm = 0.f;  // their L2 norm

  if (!readable || len > FEATURIZE_MAX_BYTES) {
    status = FEATURIZE_TOO_MANY_GRAMS;
  } else {
    // ---- 1. load, classify, number the token starts ----------------------
    int n_tok = 0;                      // wave-uniform
    unsigned long long prev_last = 0;   // class of the previous step's lane 63
    for (int base = 0; base < len; base += 64) {
      const int p = base + lane;
      unsigned c = 0;
      bool tok = false;
      if (p < len) {
        c = feat_lower(buf[off0 + p]);
        tok = feat_is_token(c);
        lds.bytes[p] = (unsigned char)(tok ? c : 0u);
      }
      const unsigned long long m = __ballot(tok);
      const unsigned long long starts = m & ~((m << 1) | prev_last);
      if ((starts >> lane) & 1ull) {
        const int t = n_tok + __popcll(starts & feat_lanes_below(lane));
        if (t < FEATURIZE_MAX_TOKENS) lds.tok_start[t] = (unsigned short)p;
      }
      n_tok += __popcll(starts);
      prev_last = m >> 63;
    }
    feat_wave_sync();

    if (n_tok > FEATURIZE_MAX_TOKENS) {
      status = FEATURIZE_TOO_MANY_GRAMS;
    } else if (n_tok > 0) {
      // ---- 2. gram keys: unigram of token t at t, bigram (t, t+1) at T+t --
      const int n_keys = 2 * n_tok - 1;
      const int n_sort = feat_pow2_at_least(n_keys);
      for (int t = lane; t < n_tok; t += 64) {
        unsigned long long h = start_state;
        for (int p = lds.tok_start[t]; p < len; ++p) {
          const unsigned c = lds.bytes[p];
          if (c == 0u) break;
          h = feat_fnv_step(h, c);
        }
        lds.keys[t] = h;
        if (t + 1 < n_tok) {
          h = feat_fnv_step(h, 0x20u);
          for (int p = lds.tok_start[t + 1]; p < len; ++p) {
            const unsigned c = lds.bytes[p];
            if (c == 0u) break;
            h = feat_fnv_step(h, c);
          }
          lds.keys[n_tok + t] = h;
        }
      }
      // pads sort last: the first n_keys sorted words are the keys
      for (int i = n_keys + lane; i < n_sort; i += 64) lds.keys[i] = ~0ull;
      feat_wave_sync();

      // ---- 3. sort keys, count runs, one entry per distinct key ----------
      feat_bitonic_sort(lds.keys, n_sort, lane);
      int n_ent = 0;  // wave-uniform
      for (int base = 0; base < n_keys; base += 64) {
        const int i = base + lane;
        bool head = false;
        unsigned long long h = 0;
        if (i < n_keys) {
          h = lds.keys[i];
          head = i == 0 || lds.keys[i - 1] != h;
        }
        const unsigned long long hm = __ballot(head);
        if (head) {
          unsigned count = 1;
          while (i + (int)count < n_keys && lds.keys[i + count] == h) ++count;
          lds.ent[n_ent + __popcll(hm & feat_lanes_below(lane))] =
              feat_entry(h, count, hash_dim);
        }
        n_ent += __popcll(hm);
      }
      const int e_sort = feat_pow2_at_least(n_ent);
      // a pad's bucket, 0xFFFFFFFF, is above every real one (< 2^31)
      for (int i = n_ent + lane; i < e_sort; i += 64) lds.ent[i] = ~0ull;
      feat_wave_sync();

      // ---- 4. sort by bucket, sum per bucket ------------------------------
      feat_bitonic_sort(lds.ent, e_sort, lane);
      // the key array is free now: it holds the features from here on
      int* const fidx = (int*)lds.keys;
      float* const fw = (float*)(fidx + FEATURIZE_MAX_GRAMS);
      float sq = 0.f;
      for (int base = 0; base < n_ent; base += 64) {
        const int i = base + lane;
        bool head = false;
        int bucket = 0;
        if (i < n_ent) {
          bucket = feat_entry_bucket(lds.ent[i]);
          head = i == 0 || feat_entry_bucket(lds.ent[i - 1]) != bucket;
        }
        const unsigned long long hm = __ballot(head);
        if (head) {
          float s = 0.f;
          for (int j = i; j < n_ent && feat_entry_bucket(lds.ent[j]) == bucket; ++j)
            s += feat_entry_term(lds.ent[j]);
          const int f = n_feat + __popcll(hm & feat_lanes_below(lane));
          fidx[f] = bucket;
          fw[f] = s;
          sq += s * s;
        }
        n_feat += __popcll(hm);
      }
      feat_wave_sync();

      // ---- 5. norm ---------------------------------------------------------
      if (n_feat > max_features) {
        status = FEATURIZE_TOO_MANY_FEATURES;
      } else {
        for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d, 64);
        norm = sqrtf(sq);
      }
    }
  }

  // ---- the row: features, then (0, 0) padding; all zeros when flagged ----
  const int live = status == FEATURIZE_OK ? n_feat : 0;
  const int* const fidx = (const int*)lds.keys;
  const float* const fw = (const float*)(fidx + FEATURIZE_MAX_GRAMS);
  int* const row_idx = out_idx + b * max_features;
  float* const row_w = out_w + b * max_features;
  for (int j = lane; j < max_features; j += 64) {
    int ix = 0;
    float wt = 0.f;
    if (j < live) {
      ix = fidx[j];
      wt = norm > 0.f ? fw[j] / norm : fw[j];
    }
    row_idx[j] = ix;
    row_w[j] = wt;
  }
  if (lane == 0) {
    out_status[b] = status;
    if (status != FEATURIZE_OK) atomicAdd(flagged, 1);
  }
}

}  // namespace kakveda
