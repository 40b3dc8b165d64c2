// Stand-alone check of the label-filtered half of the cosine_topk dispatch
// plan (knn_plan.h, plan_cosine_topk(..., filtered = true)). Built and run
// by tests/test_knn_plan_filter.py with the host compiler under
// -fsanitize=address,undefined. Expectations are written from the rule
// ("only the streaming v4 kernel and the 128x128 mode-11 list kernel carry
// the filter"), not read back from the plan.
#include <cstdio>
#include <cstring>
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

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      ++failures;                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                             \
  } while (0)

static bool same_plan(const KnnPlan& a, const KnnPlan& b) {
  return a.main == b.main && a.mode == b.mode && a.tile == b.tile &&
         a.ch.row_tiles == b.ch.row_tiles && a.ch.ntiles == b.ch.ntiles &&
         a.ch.chunk_tiles == b.ch.chunk_tiles && a.ch.nchunks == b.ch.nchunks &&
         a.preg == b.preg && a.prepass == b.prepass &&
         a.prepass_mode == b.prepass_mode &&
         a.prepass_compact == b.prepass_compact && a.cap == b.cap &&
         a.smallb_blocks == b.smallb_blocks && a.merge == b.merge;
}

int main() {
  const int Bs[] = {1, 8, 9, 300, 2048};
  const int Ns[] = {100, 4096, 65535, 65536, 300000, 10000000};
  const int ks[] = {1, 5, 8};
  // every accepted KAKVEDA_KNN_KERNEL / KAKVEDA_SMALLB value (nullptr: unset)
  const char* sels[] = {nullptr, "", "list", "eager", "rege", "fast",
                        "8pbl",  "8pe", "8pe2"};
  const char* smallbs[] = {nullptr, "4", "2"};

  long cases = 0;
  for (int B : Bs)
    for (int N : Ns)
      for (int k : ks)
        for (const char* sel : sels)
          for (const char* sb : smallbs)
            for (bool allow : {true, false}) {
              EnvVars vars;
              if (sel) vars.push_back({"KAKVEDA_KNN_KERNEL", sel});
              if (sb) vars.push_back({"KAKVEDA_SMALLB", sb});
              const KnnEnv env = env_of(vars);
              const KnnPlan p = plan_cosine_topk(B, N, k, env, allow, true);
              ++cases;

              const bool stream = allow && N >= 65536 && B <= 8;
              bool ok = true;
              if (stream) {
                ok = ok && p.main == MainKernel::SmallB && p.mode == 4;
                ok = ok && p.merge == MergeKernel::Emit;
                // the streaming kernel needs the filtered floors
                ok = ok && p.prepass && p.prepass_compact;
              } else {
                ok = ok && p.main == MainKernel::List128 && p.mode == 11;
                ok = ok && p.merge != MergeKernel::Emit && !p.prepass_compact;
              }
              // never a kernel without the filter
              ok = ok && p.main != MainKernel::Emit8p &&
                   p.main != MainKernel::Stash8p &&
                   p.main != MainKernel::Argmax128;
              ok = ok && p.prepass_mode == 11;
              // geometry of the 128-row-tile kernels, default target
              const int ntiles = (N + 127) / 128;
              const int row_tiles = (B + 127) / 128;
              long want = ((long)ntiles * row_tiles + 2047) / 2048;
              if (want < 4) want = 4;
              if (want > 128) want = 128;
              const int nchunks =
                  ((ntiles + (int)want - 1) / (int)want + 7) & ~7;
              ok = ok && p.tile == 128 && p.ch.row_tiles == row_tiles &&
                   p.ch.ntiles == ntiles && p.ch.chunk_tiles == (int)want &&
                   p.ch.nchunks == nchunks;
              // every prepass block has a partial slot and samples 8 tiles
              ok = ok && p.preg <= p.ch.nchunks && p.preg % 8 == 0;
              if (p.prepass) ok = ok && p.preg >= 8;
              if (p.prepass && !stream)
                ok = ok && p.preg * PRE_TILES <= p.ch.ntiles && k > 1;
              // the selections select nothing: same plan as with none set
              ok = ok && same_plan(p, plan_cosine_topk(B, N, k, env_of({}),
                                                       allow, true));
              if (!ok) {
                ++failures;
                std::printf(
                    "FAIL B=%d N=%d k=%d sel=%s smallb=%s allow=%d: main=%d "
                    "mode=%d tile=%d chunks=%d/%d/%d/%d preg=%d prepass=%d/%d/%d "
                    "merge=%d\n",
                    B, N, k, sel ? sel : "-", sb ? sb : "-", (int)allow,
                    (int)p.main, p.mode, p.tile, p.ch.row_tiles, p.ch.ntiles,
                    p.ch.chunk_tiles, p.ch.nchunks, p.preg, (int)p.prepass,
                    p.prepass_mode, (int)p.prepass_compact, (int)p.merge);
              }

              // filtered = false (explicit or defaulted) is today's plan
              CHECK(same_plan(plan_cosine_topk(B, N, k, env, allow),
                              plan_cosine_topk(B, N, k, env, allow, false)));
            }

  // spot values worked out by hand
  {
    const KnnEnv none = env_of({});
    // the overflow-fallback test's shape: 2344 tiles, 592 chunks, and the
    // emission prepass samples 256 chunks x 8 tiles x 128 = 262144 columns
    const KnnPlan p = plan_cosine_topk(4, 300000, 5, none, true, true);
    CHECK(p.main == MainKernel::SmallB && p.ch.ntiles == 2344 &&
          p.ch.chunk_tiles == 4 && p.ch.nchunks == 592 && p.preg == 256 &&
          p.smallb_blocks == 1172 && p.cap == 32768);
    const KnnPlan f = plan_cosine_topk(4, 300000, 5, none, false, true);
    CHECK(f.main == MainKernel::List128 && f.preg == 64 && f.prepass &&
          f.merge == MergeKernel::Merge);
    // unfiltered default at that shape is the streaming kernel on 8p geometry
    CHECK(plan_cosine_topk(4, 300000, 5, none, true).tile == 256);
    // B just over the streaming limit: list kernel where unfiltered is 8p
    CHECK(plan_cosine_topk(9, 70000, 5, none, true, true).main ==
          MainKernel::List128);
    CHECK(plan_cosine_topk(9, 70000, 5, none, true).main == MainKernel::Emit8p);
    // k == 1 has no filtered argmax kernel
    CHECK(plan_cosine_topk(300, 4096, 1, none, true, true).main ==
          MainKernel::List128);
    CHECK(plan_cosine_topk(300, 4096, 1, none, true).main ==
          MainKernel::Argmax128);
    // the geometry knobs still act
    CHECK(plan_cosine_topk(
              4, 300000, 5, env_of({{"KAKVEDA_KNN_EMIT_CAP", "64"}}), true, true)
              .cap == 64);
    CHECK(plan_cosine_topk(4, 300000, 5, env_of({{"KAKVEDA_KNN_PREG", "64"}}),
                           true, true)
              .preg == 64);
  }

  // parsing still validates the selections on the filtered path's env
  bool threw = false;
  try {
    env_of({{"KAKVEDA_KNN_KERNEL", "bogus"}});
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    env_of({{"KAKVEDA_SMALLB", "3"}});
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("knn_plan_filter: all %ld cases passed\n", cases);
  return 0;
}
