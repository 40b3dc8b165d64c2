// Stand-alone check of the stage plan of the batched int8 screen (knn_plan.h:
// plan_q8_stages, stage_model_count, KAKVEDA_Q8_STAGES). Built and run by
// tests/test_q8_stage_plan.py with the host compiler under
// -fsanitize=address,undefined. Expectations are written from the rules: the
// stages partition [skip_tiles, ntiles), every stage is a launch the screen
// kernel takes (a multiple of 8 chunks of 4..128 tiles that cover the stage),
// one stage is the single launch field for field, an unforced plan keeps no
// stage below one round of 256 blocks of 4 tiles, and the modelled candidate
// count falls as n ((N / S)^(1 / n) - 1) against N / S - 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "knn_plan.h"

using namespace kakveda;

using EnvVars = std::vector<std::pair<const char*, const char*>>;

static KnnEnv env_of(const EnvVars& vars) {
  return parse_knn_env([&](const char* name) -> const char* {
    for (const auto& kv : vars)
      if (!std::strcmp(kv.first, name)) return kv.second;
    return nullptr;
  });
}

static int failures = 0;
static int cases = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      ++failures;                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                             \
  } while (0)

static bool same(const Chunking& a, const Chunking& b) {
  return a.row_tiles == b.row_tiles && a.ntiles == b.ntiles &&
         a.chunk_tiles == b.chunk_tiles && a.nchunks == b.nchunks;
}

static bool throws(const EnvVars& vars) {
  try {
    (void)env_of(vars);
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

// The model is sum (first[i + 1] / first[i] - 1). A boundary within 1/64 of
// its geometric place (plus a tile of rounding, which the bound's slack over
// (1 + 1/64)^2 - 1 = 0.0315 covers at these prefixes) moves each of the n
// ratios by at most 3.5%, and the ratios sum to count + n.
static double model_tol(double count, int n) { return 0.035 * (count + n); }

struct Shape {
  int B, N;
  bool skips;  // the main launch starts after the sample
};

static void check_shape(const Shape& sh, const KnnEnv& env) {
  const KnnPlan p = plan_cosine_topk(sh.B, sh.N, 5, env, true);
  CHECK(p.main == MainKernel::Emit8p);
  CHECK((p.skip_tiles > 0) == sh.skips);
  const int ntiles = (sh.N + 255) / 256;
  for (int n = 1; n <= 4; ++n) {
    ++cases;
    const StagePlan s = plan_q8_stages(p, env, n);
    CHECK(s.n == n);  // forced: every shape here has room for four stages
    CHECK(s.first[0] == p.skip_tiles);
    CHECK(s.first[s.n] == ntiles);
    for (int i = 0; i < s.n; ++i) {
      const int tiles = s.first[i + 1] - s.first[i];
      CHECK(tiles >= 1);
      const Chunking& c = s.ch[i];
      CHECK(c.ntiles == tiles);
      CHECK(c.row_tiles == p.ch.row_tiles);
      CHECK(c.nchunks % 8 == 0);
      CHECK(c.chunk_tiles >= 4 && c.chunk_tiles <= 128);
      CHECK((long)c.nchunks * c.chunk_tiles >= tiles);  // the chunks cover it
    }
    if (n == 1) CHECK(same(s.ch[0], p.mch));
    // geometric in the prefix: every interior boundary within 1/64 (the
    // nudge) and one tile (the rounding) of P0 (ntiles / P0)^(i / n)
    if (sh.skips)
      for (int i = 1; i < s.n; ++i) {
        const double g =
            p.skip_tiles * std::pow((double)ntiles / p.skip_tiles, (double)i / n);
        CHECK(std::fabs(s.first[i] - g) <= g / 64 + 1.0);
      }
    // the model: n stages of ratio r let n (r - 1) through
    if (sh.skips) {
      const double ratio = (double)ntiles / p.skip_tiles;
      const double want = n * (std::pow(ratio, 1.0 / n) - 1.0);
      CHECK(std::fabs(stage_model_count(s) - want) <= model_tol(want, n));
    }
  }
}

int main() {
  const KnnEnv env = env_of({});
  // the bench shape, its shards, and the two small shapes of the GPU tests
  const Shape shapes[] = {
      {2048, 10000000, true}, {2048, 5000000, true}, {2048, 2500000, true},
      {2048, 1250000, true},  {300, 70001, false},   {300, 300001, true},
  };
  for (const Shape& sh : shapes) check_shape(sh, env);

  {  // the rule, unforced
    ++cases;
    const KnnPlan bench = plan_cosine_topk(2048, 10000000, 5, env, true);
    const StagePlan s = plan_q8_stages(bench, env, 0);
    CHECK(s.n == Q8_STAGES_DEFAULT);
    for (int i = 0; i < s.n; ++i)
      CHECK((long)(s.first[i + 1] - s.first[i]) * bench.ch.row_tiles >=
            Q8_STAGE_MIN_WORK);
    // 300,001 x 300: 212 tiles x 2 row tiles are left, under one round of
    // 256 blocks of 4 tiles: one stage
    const KnnPlan small = plan_cosine_topk(300, 300001, 5, env, true);
    CHECK((long)(small.ch.ntiles - small.skip_tiles) * small.ch.row_tiles <
          Q8_STAGE_MIN_WORK);
    const StagePlan t = plan_q8_stages(small, env, 0);
    CHECK(t.n == 1 && same(t.ch[0], small.mch));
    // 70,001 x 300: the sample covers the corpus, 548 tile-blocks in all
    const KnnPlan tiny = plan_cosine_topk(300, 70001, 5, env, true);
    CHECK(plan_q8_stages(tiny, env, 0).n == 1);
    // whatever n the rule keeps, no stage is below the floor
    for (int N = 200000; N <= 3000000; N += 137531) {
      const KnnPlan q = plan_cosine_topk(2048, N, 5, env, true);
      const StagePlan u = plan_q8_stages(q, env, 0);
      CHECK(u.n >= 1 && u.n <= Q8_STAGES_DEFAULT);
      if (u.n > 1)
        for (int i = 0; i < u.n; ++i)
          CHECK((long)(u.first[i + 1] - u.first[i]) * q.ch.row_tiles >=
                Q8_STAGE_MIN_WORK);
    }
  }

  {  // a forced n is clamped to one tile a stage and to Q8_MAX_STAGES
    ++cases;
    KnnPlan p = plan_cosine_topk(300, 300001, 5, env, true);
    CHECK(plan_q8_stages(p, env, 9).n == Q8_MAX_STAGES);
    p.skip_tiles = p.ch.ntiles - 2;
    const StagePlan s = plan_q8_stages(p, env, 4);
    CHECK(s.n == 2 && s.first[1] == p.ch.ntiles - 1);
  }

  {  // the bench shape: the modelled count against the single launch's
    ++cases;
    const KnnPlan p = plan_cosine_topk(2048, 10000000, 5, env, true);
    const double one = stage_model_count(plan_q8_stages(p, env, 1));
    CHECK(std::fabs(one - 37.1) < 0.1);  // (39063 - 1024) / 1024
    // the table of the plan's comment: 37 -> 10.4 -> 7.1 -> 5.9
    const double table[] = {37.1, 10.4, 7.1, 5.9};
    // (entries rounded to one decimal: 0.05 more)
    for (int n = 2; n <= 4; ++n)
      CHECK(stage_model_count(plan_q8_stages(p, env, n)) <=
            table[n - 1] + 0.05 + model_tol(table[n - 1], n));
    const StagePlan shipped = plan_q8_stages(p, env, 0);
    const double t = table[shipped.n - 1];
    CHECK(one / stage_model_count(shipped) >=
          (table[0] - 0.05) / (t + 0.05 + model_tol(t, shipped.n)));
  }

  {  // KAKVEDA_Q8_STAGES
    ++cases;
    CHECK(env_of({}).q8_stages == 0);
    CHECK(env_of({{"KAKVEDA_Q8_STAGES", "1"}}).q8_stages == 1);
    CHECK(env_of({{"KAKVEDA_Q8_STAGES", "4"}}).q8_stages == 4);
    CHECK(throws({{"KAKVEDA_Q8_STAGES", "0"}}));
    CHECK(throws({{"KAKVEDA_Q8_STAGES", "5"}}));
    CHECK(throws({{"KAKVEDA_Q8_STAGES", "2x"}}));
    CHECK(throws({{"KAKVEDA_Q8_STAGES", "-1"}}));
  }

  if (failures) {
    std::printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("%d cases passed\n", cases);
  return 0;
}
