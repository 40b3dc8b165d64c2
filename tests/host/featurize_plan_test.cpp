// Stand-alone check of the device featurizer's contract
// (ops/hip/featurize_plan.h): featurize_one on every case of a case file
// against the rows the Python featurizer gave. Built with the host compiler
// under ASan + UBSan by tests/test_featurize_plan.py, which writes the file:
//
//   <number of cases>
//   then per case
//   <hash_dim> <start_state> <max_features> <status> <n_features> <n_bytes>
//   <n_bytes byte values> <n_features indices> <n_features weights>
//
// A case whose status is not 0 expects that status and an all-zero row.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "featurize_plan.h"

using namespace kakveda;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static void test_pieces() {
  for (unsigned b = 0; b < 256; ++b) {
    const unsigned c = feat_lower(b);
    CHECK(c == ((b >= 'A' && b <= 'Z') ? b + 32 : b));
    const bool tok = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' ||
                     c == ':' || c == '.' || c == '-';
    CHECK(feat_is_token(c) == tok);
    if (b >= 0x80 || b == 0) CHECK(!feat_is_token(c));
  }
  CHECK(feat_start_state(0) == 0xCBF29CE484222325ull);
  // FNV-1a of "a" from the standard offset basis
  CHECK(feat_fnv_step(feat_start_state(0), 'a') == 0xAF63DC4C8601EC8Cull);
  CHECK(feat_sign(1ull << 62) == 1.0f && feat_sign(~(1ull << 62)) == -1.0f);
  CHECK(feat_bucket(0xFFFFFFFFFFFFFFFFull, 1) == 0);
  CHECK(feat_bucket(0xFFFFFFFFFFFFFFFFull, 0x7FFFFFFFu) ==
        (int32_t)(0xFFFFFFFFFFFFFFFFull % 0x7FFFFFFFull));
  const uint64_t e = feat_entry(1ull << 62 | 5, 4, 64);
  CHECK(feat_entry_bucket(e) == 5 && feat_entry_term(e) == 2.0f);
  CHECK(FEATURIZE_MAX_TOKENS * 2 - 1 <= FEATURIZE_MAX_GRAMS);
  CHECK((FEATURIZE_MAX_TOKENS + 1) * 2 - 1 > FEATURIZE_MAX_GRAMS);
}

int main(int argc, char** argv) {
  test_pieces();
  if (argc < 2) {
    std::printf("usage: featurize_plan_test <case file>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  long n_cases = 0;
  in >> n_cases;
  CHECK(in.good() && n_cases > 0);
  const float tol = std::ldexp(1.0f, -18);
  long done = 0;
  for (long c = 0; c < n_cases && in.good(); ++c) {
    uint64_t hash_dim = 0, start_state = 0;
    int max_features = 0, status = 0, n_feat = 0;
    long n_bytes = 0;
    in >> hash_dim >> start_state >> max_features >> status >> n_feat >> n_bytes;
    if (!in.good() || max_features < 1 || max_features > FEATURIZE_MAX_FEATURES ||
        n_feat < 0 || n_feat > max_features || n_bytes < 0) {
      std::printf("FAIL: malformed case %ld\n", c);
      ++failures;
      break;
    }
    // exact-size heap buffers: the sanitizer sees any step outside them
    std::vector<uint8_t> text(n_bytes);
    for (long i = 0; i < n_bytes; ++i) {
      int v = 0;
      in >> v;
      text[i] = (uint8_t)v;
    }
    std::vector<int32_t> want_idx(max_features, 0), idx(max_features, -1);
    std::vector<float> want_w(max_features, 0.0f), w(max_features, -1.0f);
    for (int i = 0; i < n_feat; ++i) in >> want_idx[i];
    for (int i = 0; i < n_feat; ++i) in >> want_w[i];
    if (in.fail()) {
      std::printf("FAIL: truncated case %ld\n", c);
      ++failures;
      break;
    }
    const int got = featurize_one(text.data(), n_bytes, (uint32_t)hash_dim,
                                  start_state, max_features, idx.data(), w.data());
    bool ok = got == status;
    for (int i = 0; i < max_features; ++i)
      ok = ok && idx[i] == want_idx[i] && std::fabs(w[i] - want_w[i]) <= tol;
    if (!ok) {
      std::printf("FAIL: case %ld (hash_dim %llu, %ld bytes): status %d, want %d\n", c,
                  (unsigned long long)hash_dim, n_bytes, got, status);
      ++failures;
    }
    ++done;
  }
  CHECK(done == n_cases);
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all checks passed (%ld cases)\n", done);
  return 0;
}
