// Stand-alone check of the cosine_topk dispatch plan (knn_plan.h).
// Built and run by tests/test_knn_plan.py with the host compiler under
// -fsanitize=address,undefined. The expected values were derived by hand
// from the dispatch logic the plan replaced, not from the plan itself.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
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

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      ++failures;                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
    }                                                                \
  } while (0)

struct Row {
  int B, N, k;
  EnvVars env;
  bool allow_emission;
  MainKernel main;
  int mode, tile, row_tiles, ntiles, chunk_tiles, nchunks, preg;
  bool prepass;
  MergeKernel merge;
};

static void check_row(int i, const Row& r) {
  const KnnPlan p =
      plan_cosine_topk(r.B, r.N, r.k, env_of(r.env), r.allow_emission);
  const bool ok = p.main == r.main && p.mode == r.mode && p.tile == r.tile &&
                  p.ch.row_tiles == r.row_tiles && p.ch.ntiles == r.ntiles &&
                  p.ch.chunk_tiles == r.chunk_tiles &&
                  p.ch.nchunks == r.nchunks && p.preg == r.preg &&
                  p.prepass == r.prepass && p.merge == r.merge &&
                  // only the emission path gives the prepass its own buffer
                  p.prepass_compact ==
                      (r.prepass && r.merge == MergeKernel::Emit);
  if (!ok) {
    ++failures;
    std::printf(
        "FAIL row %d (B=%d N=%d k=%d): main=%d mode=%d tile=%d row_tiles=%d "
        "ntiles=%d chunk_tiles=%d nchunks=%d preg=%d prepass=%d compact=%d "
        "merge=%d\n",
        i, r.B, r.N, r.k, (int)p.main, p.mode, p.tile, p.ch.row_tiles,
        p.ch.ntiles, p.ch.chunk_tiles, p.ch.nchunks, p.preg, (int)p.prepass,
        (int)p.prepass_compact, (int)p.merge);
  }
}

template <class F>
static bool throws_runtime_error(F&& f, std::string* what = nullptr) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (what) *what = e.what();
    return true;
  }
  return false;
}

int main() {
  const auto L = MainKernel::List128;
  const auto A = MainKernel::Argmax128;
  const auto S = MainKernel::Stash8p;
  const auto E = MainKernel::Emit8p;
  const auto SB = MainKernel::SmallB;
  const auto small = MergeKernel::Small;
  const auto merge = MergeKernel::Merge;
  const auto emit = MergeKernel::Emit;
  const EnvVars none;
  auto sel = [](const char* v) { return EnvVars{{"KAKVEDA_KNN_KERNEL", v}}; };

  const Row rows[] = {
      // B, N, k, env, emission allowed | main, mode, tile, row_tiles, ntiles,
      // chunk_tiles, nchunks, preg, prepass, merge
      {1, 100, 5, none, true, L, 11, 128, 1, 1, 4, 8, 8, false, small},
      {256, 8192, 5, none, true, L, 11, 128, 2, 64, 4, 16, 16, false, small},
      {256, 8192, 5, sel("8pbl"), true, S, 6, 256, 1, 32, 4, 8, 8, false, small},
      {256, 4095, 5, sel("8pbl"), true, L, 11, 128, 2, 32, 4, 8, 8, false, small},
      {256, 8192, 5, sel("eager"), true, L, 0, 128, 2, 64, 4, 16, 16, false, small},
      {512, 50000, 1, none, true, A, 4, 128, 4, 391, 4, 104, 64, false, small},
      {300, 200001, 1, none, true, A, 4, 128, 3, 1563, 4, 392, 64, false, merge},
      {300, 200001, 1, sel("8pe"), true, E, 9, 256, 2, 782, 4, 200, 200, true, emit},
      {256, 65535, 5, none, true, L, 11, 128, 2, 512, 4, 128, 64, true, small},
      {256, 65536, 5, none, true, E, 9, 256, 1, 256, 4, 64, 64, true, emit},
      {300, 70000, 5, none, true, E, 9, 256, 2, 274, 4, 72, 72, true, emit},
      {256, 131072, 5, sel("8pe2"), true, E, 15, 256, 1, 512, 4, 128, 128, true, emit},
      {256, 131072, 5, none, false, L, 11, 128, 2, 1024, 4, 256, 64, true, merge},
      {256, 131072, 5, sel("list"), true, L, 11, 128, 2, 1024, 4, 256, 64, true, merge},
      {3, 300000, 5, none, true, SB, 4, 256, 1, 1172, 4, 296, 256, true, emit},
      {3, 300000, 5, {{"KAKVEDA_SMALLB", "2"}}, true, SB, 2, 256, 1, 1172, 4, 296, 256, true, emit},
      {9, 300000, 5, none, true, E, 9, 256, 1, 1172, 4, 296, 256, true, emit},
      {2048, 10000000, 5, none, true, E, 9, 256, 8, 39063, 128, 312, 256, true, emit},
      {2048, 10000000, 5, none, false, L, 11, 128, 16, 78125, 128, 616, 64, false, merge},
      {4096, 2000000, 5, sel("fast"), true, L, 9, 128, 32, 15625, 128, 128, 64, true, small},
      {1024, 1000000, 5, sel("rege"), true, L, 8, 128, 8, 7813, 31, 256, 64, true, merge},
      {1024, 1000000, 5,
       {{"KAKVEDA_KNN_KERNEL", "rege"}, {"KAKVEDA_KNN_PREPASS", "0"}},
       true, L, 8, 128, 8, 7813, 31, 256, 64, false, merge},
  };
  int i = 0;
  for (const Row& r : rows) check_row(i++, r);

  // removed and unknown selections are errors that list the accepted names
  for (const char* bad : {"dfr", "8p", "8pq", "8pv3", "bogus"}) {
    std::string what;
    CHECK(throws_runtime_error([&] { env_of(sel(bad)); }, &what));
    for (const char* name :
         {"list", "eager", "rege", "fast", "8pbl", "8pe", "8pe2"})
      CHECK(what.find(name) != std::string::npos);
  }
  CHECK(throws_runtime_error([&] { env_of({{"KAKVEDA_SMALLB", "v2"}}); }));
  CHECK(!throws_runtime_error([&] { env_of({{"KAKVEDA_SMALLB", "4"}}); }));
  CHECK(!env_of({{"KAKVEDA_SMALLB", "4"}}).smallb_v2);

  // empty selection == unset
  CHECK(env_of(sel("")).sel == KnnSel::Default);
  CHECK(env_of(none).sel == KnnSel::Default);
  CHECK(plan_cosine_topk(256, 65536, 5, env_of(sel("")), true).main == E);

  // smallb grid = min(ceil(N/256), 8192)
  CHECK(plan_cosine_topk(3, 300000, 5, env_of(none), true).smallb_blocks == 1172);
  CHECK(plan_cosine_topk(1, 65536, 5, env_of(none), true).smallb_blocks == 256);
  CHECK(plan_cosine_topk(1, 10000000, 5, env_of(none), true).smallb_blocks == 8192);

  // candidate capacity
  CHECK(plan_cosine_topk(256, 65536, 5, env_of(none), true).cap == 32768);
  CHECK(plan_cosine_topk(256, 65536, 5,
                         env_of({{"KAKVEDA_KNN_EMIT_CAP", "4"}}), true)
            .cap == 4);

  // the prepass samples with the main kernel's mode, except fast (9),
  // which has no prepass instantiation and shares rege's (8)
  CHECK(plan_cosine_topk(256, 65535, 5, env_of(none), true).prepass_mode == 11);
  CHECK(plan_cosine_topk(256, 65535, 5, env_of(sel("eager")), true).prepass_mode == 0);
  CHECK(plan_cosine_topk(256, 65535, 5, env_of(sel("rege")), true).prepass_mode == 8);
  CHECK(plan_cosine_topk(256, 65535, 5, env_of(sel("fast")), true).prepass_mode == 8);

  // chunking() on its own (the probes use it with the default target)
  const Chunking c = chunking(2048, 10000000, BM8, default_target(BM8));
  CHECK(c.row_tiles == 8 && c.ntiles == 39063 && c.chunk_tiles == 128 &&
        c.nchunks == 312);

  // grid.y holds at most 65535 row tiles. 128-row tile: the k = 1 argmax
  // plan of the k-means caller (huge B, a handful of centroids).
  {
    const int fit = MAX_GRID_Y * BM;  // 8 388 480 rows
    const KnnPlan ok = plan_cosine_topk(fit, 200, 1, env_of(none), true);
    CHECK(ok.main == A && ok.tile == 128 && ok.ch.row_tiles == 65535);
    CHECK(plan_fits_grid(ok, fit));
    const KnnPlan over = plan_cosine_topk(fit + 1, 200, 1, env_of(none), true);
    CHECK(over.tile == 128 && over.ch.row_tiles == 65536);
    CHECK(!plan_fits_grid(over, fit + 1));
    // the list kernel at k > 1 on the same tile
    CHECK(plan_fits_grid(plan_cosine_topk(fit, 200, 5, env_of(none), true), fit));
    CHECK(!plan_fits_grid(plan_cosine_topk(fit + 1, 200, 5, env_of(none), true), fit + 1));
  }
  // 256-row tile without a prepass (8pbl): twice as many rows fit
  {
    const int fit = MAX_GRID_Y * BM8;  // 16 776 960 rows
    const KnnPlan ok = plan_cosine_topk(fit, 4096, 5, env_of(sel("8pbl")), true);
    CHECK(ok.main == S && ok.tile == 256 && ok.ch.row_tiles == 65535 && !ok.prepass);
    CHECK(plan_fits_grid(ok, fit));
    const KnnPlan over = plan_cosine_topk(fit + 1, 4096, 5, env_of(sel("8pbl")), true);
    CHECK(over.tile == 256 && over.ch.row_tiles == 65536);
    CHECK(!plan_fits_grid(over, fit + 1));
  }
  // 256-row tile with the emission prepass: the prepass runs on 128-row
  // tiles, so its limit is the 128-row one although the main launch fits
  {
    const int fit = MAX_GRID_Y * BM;
    const KnnPlan ok = plan_cosine_topk(fit, 65536, 5, env_of(none), true);
    CHECK(ok.main == E && ok.tile == 256 && ok.prepass);
    CHECK(plan_fits_grid(ok, fit));
    const KnnPlan over = plan_cosine_topk(fit + 1, 65536, 5, env_of(none), true);
    CHECK(over.main == E && over.prepass && over.ch.row_tiles == 32768);
    CHECK(!plan_fits_grid(over, fit + 1));
  }
  // everyday shapes fit
  CHECK(plan_fits_grid(plan_cosine_topk(1, 100, 5, env_of(none), true), 1));
  CHECK(plan_fits_grid(plan_cosine_topk(2048, 10000000, 5, env_of(none), true), 2048));

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("knn_plan: all checks passed\n");
  return 0;
}
