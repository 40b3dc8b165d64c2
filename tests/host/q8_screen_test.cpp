// Host check of the batched screen's contract (ops/hip/q8_plan.h "Screening
// test"): rows and queries are quantised serially with the header's own
// pieces; for every (query, row) and a ladder of floors around the pair's
// exact score,
//   - q8_screen_ref never rejects a pair whose exact score reaches the floor,
//   - q8_screen_fast (the kernel's form, with the launch's kappa and the
//     row's q8_screen_threshold) accepts every pair q8_screen_ref accepts.
// Rows: random unit rows, all-zero rows, one-hot rows, rows with one large
// outlier. Queries: random unit rows and rows with a tiny amax. D = 128, 768.
// Built with ASan + UBSan by tests/test_q8_screen.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "q8_plan.h"

using namespace kakveda;

static float to_bf16(float x) {  // round to nearest even, as the device cast
  uint32_t b;
  std::memcpy(&b, &x, 4);
  b += 0x7fffu + ((b >> 16) & 1u);
  b &= 0xffff0000u;
  std::memcpy(&x, &b, 4);
  return x;
}

struct Row {
  std::vector<float> x;
  std::vector<int8_t> n;
  float scale = 0, err = 0, norm_up = 0;
  long sumsq = 0;
};

static Row quantise(std::vector<float> x) {
  const int D = (int)x.size();
  Row r;
  float amax = 0;
  for (float& v : x) {
    v = to_bf16(v);
    amax = std::fmax(amax, std::fabs(v));
  }
  const Q8Scale qs = q8_scale(amax);
  r.scale = qs.scale;
  r.n.resize(D);
  float ss = 0, s2 = 0;
  for (int i = 0; i < D; ++i) {
    r.n[i] = q8_code(x[i], qs.inv);
    const float d = std::fmaf(-qs.scale, (float)r.n[i], x[i]);
    ss = std::fmaf(d, d, ss);
    s2 = std::fmaf(x[i], x[i], s2);
    r.sumsq += (long)r.n[i] * r.n[i];
  }
  r.err = q8_err(std::sqrt(ss), amax, qs.scale, D);
  r.norm_up = q8_norm_up(s2, D);
  r.x = std::move(x);
  return r;
}

static std::vector<float> unit(std::mt19937& g, int D, float norm = 1.0f) {
  std::normal_distribution<float> nd;
  std::vector<float> x(D);
  double s = 0;
  for (float& v : x) {
    v = nd(g);
    s += (double)v * v;
  }
  for (float& v : x) v = (float)(v / std::sqrt(s)) * norm;
  return x;
}

int main() {
  long pairs = 0, tests = 0, fails = 0;
  for (int D : {128, 768}) {
    std::mt19937 g(1234 + D);
    std::vector<Row> rows, qs;
    for (int i = 0; i < 48; ++i) rows.push_back(quantise(unit(g, D)));
    rows.push_back(quantise(std::vector<float>(D, 0.0f)));
    for (int i = 0; i < 4; ++i) {
      std::vector<float> x(D, 0.0f);
      x[(i * 37 + 5) % D] = i & 1 ? -1.0f : 1.0f;
      rows.push_back(quantise(x));
    }
    for (int i = 0; i < 8; ++i) {  // one large outlier over a small background
      std::vector<float> x = unit(g, D, 0.3f);
      x[(i * 53 + 11) % D] = 0.95f;
      rows.push_back(quantise(x));
    }
    for (int i = 0; i < 24; ++i) qs.push_back(quantise(unit(g, D)));
    for (float tiny : {0x1p-20f, 0x1p-60f, 0x1p-90f})  // tiny amax, still live
      qs.push_back(quantise(unit(g, D, tiny)));
    {
      std::vector<float> x = unit(g, D, 0.3f);
      x[7] = -0.95f;
      qs.push_back(quantise(x));
    }

    float cnorm = 0;
    for (const Row& c : rows) cnorm = std::fmax(cnorm, c.norm_up);
    float kappa = 0;
    std::vector<float> nqh(qs.size());
    for (size_t r = 0; r < qs.size(); ++r) {
      if (!(qs[r].scale > 0)) {
        std::printf("FAIL: a test query quantised to zeros (D=%d, q=%zu)\n", D, r);
        return 1;
      }
      nqh[r] = q8_code_norm(qs[r].scale, qs[r].sumsq, D);
      kappa = std::fmax(kappa, q8_screen_kappa(nqh[r], qs[r].scale));
    }

    for (size_t r = 0; r < qs.size(); ++r) {
      const Row& q = qs[r];
      for (const Row& c : rows) {
        long acc = 0;
        long double exact = 0;
        for (int i = 0; i < D; ++i) {
          acc += (long)q.n[i] * c.n[i];
          exact += (long double)q.x[i] * c.x[i];
        }
        ++pairs;
        const float s = (float)exact;
        const float mag = std::fmax(std::fabs(s), 0x1p-120f);
        // floors the exact score reaches (at it, one ulp under, well under)
        // and floors it misses (the screen may accept those, or not)
        const float floors[] = {
            s > (long double)exact ? std::nextafterf(s, -INFINITY) : s,
            std::nextafterf(std::nextafterf(s, -INFINITY), -INFINITY),
            s - mag * 0.25f, s - 0.01f, s - 1.0f, -1e30f,
            s + mag * 0.5f, s + 0.05f, s + 1.0f};
        for (float fl : floors) {
          ++tests;
          const bool reaches = exact >= (long double)fl;
          const bool ref = q8_screen_ref(acc, q.scale, c.scale, nqh[r], c.err,
                                         q.err, cnorm, fl, D);
          const float T = q8_screen_threshold(fl, q.scale, q.err, cnorm, D);
          const bool fast = q8_screen_fast((int)acc, c.scale, c.err, kappa, T);
          if (reaches && !ref) {
            ++fails;
            std::printf("FAIL ref rejects: D=%d q=%zu exact=%.9Lg floor=%.9g\n", D,
                        r, exact, (double)fl);
          }
          if (ref && !fast) {
            ++fails;
            std::printf("FAIL fast rejects what ref accepts: D=%d q=%zu exact=%.9Lg "
                        "floor=%.9g T=%.9g\n", D, r, exact, (double)fl, (double)T);
          }
          if (fails > 20) return 1;
        }
      }
    }
  }
  if (fails) return 1;
  std::printf("all checks passed (%ld pairs, %ld tests)\n", pairs, tests);
  return 0;
}
