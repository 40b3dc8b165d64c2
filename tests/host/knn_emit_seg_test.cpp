// Stand-alone check of the emission record-segment capacity in the
// cosine_topk dispatch plan (knn_plan.h: emit_seg_cap, KnnPlan::seg,
// KAKVEDA_KNN_EMIT_SEG). Built and run by tests/test_knn_emit_seg.py with
// the host compiler under -fsanitize=address,undefined. Expectations are
// written from the rules (default, override, "never more bytes than the
// candidate buffer", "only the 8-phase emission kernel has segments"), not
// read back from the plan.
#include <cstdio>
#include <cstring>
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

int main() {
  long cases = 0;

  // ---- environment parsing ------------------------------------------------
  CHECK(env_of({}).seg == 0);
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_SEG", "1"}}).seg == 1);
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_SEG", "4096"}}).seg == 4096);
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_SEG", "0"}}).seg == 0);
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_SEG", "-3"}}).seg == -3);
  // the other knobs are not disturbed
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_SEG", "7"}}).cap == 32768);
  CHECK(env_of({{"KAKVEDA_KNN_EMIT_CAP", "4"}}).seg == 0);

  // ---- the bench shape: default capacity, bytes within the budget ---------
  {
    const KnnPlan p = plan_cosine_topk(2048, 10000000, 5, env_of({}), true);
    CHECK(p.main == MainKernel::Emit8p);
    CHECK(p.seg == EMIT_SEG_DEFAULT);
    CHECK(p.ch.chunk_tiles <= 128);  // 15 column bits per record
    const long blocks = (long)p.ch.nchunks * p.ch.row_tiles;
    CHECK(blocks * p.seg <= 2048L * p.cap);
  }

  // ---- table: every emission plan, every override --------------------------
  const int Bs[] = {1, 8, 9, 130, 300, 2048, 8192};
  const int Ns[] = {4096, 65535, 65536, 65600, 300000, 10000000};
  const int ks[] = {1, 2, 5, 8};
  const char* sels[] = {nullptr, "list", "8pbl", "8pe", "8pe2"};
  const char* segs[] = {nullptr, "0", "-1", "1", "100", "1000000000"};
  const char* caps[] = {nullptr, "4", "100000"};
  for (int B : Bs)
    for (int N : Ns)
      for (int k : ks)
        for (const char* sel : sels)
          for (const char* seg : segs)
            for (const char* cap : caps)
              for (int allow = 0; allow < 2; ++allow) {
                EnvVars vars;
                if (sel) vars.push_back({"KAKVEDA_KNN_KERNEL", sel});
                if (seg) vars.push_back({"KAKVEDA_KNN_EMIT_SEG", seg});
                if (cap) vars.push_back({"KAKVEDA_KNN_EMIT_CAP", cap});
                const KnnEnv env = env_of(vars);
                const KnnPlan p = plan_cosine_topk(B, N, k, env, allow != 0);
                ++cases;
                if (p.main != MainKernel::Emit8p) {
                  CHECK(p.seg == 0);
                  continue;
                }
                const long capv = cap ? std::atol(cap) : 32768;
                const long blocks = (long)p.ch.nchunks * p.ch.row_tiles;
                const long budget = (long)B * capv / blocks;
                const long asked = seg ? std::atol(seg) : 0;
                const long want = asked > 0 ? asked : EMIT_SEG_DEFAULT;
                CHECK(p.seg >= 1);
                CHECK(p.seg <= want);
                // never more bytes than the candidate buffer beside it,
                // except that a segment holds at least one record
                CHECK(blocks * p.seg <= (long)B * capv || p.seg == 1);
                // and no smaller than asked when the budget allows it
                CHECK(p.seg == want || p.seg == (budget > 1 ? budget : 1));
                CHECK(p.seg <= 2147483647L);  // the kernels take an int
              }
  // filtered plans never run the 8-phase kernel
  for (int B : Bs)
    for (int N : Ns) {
      const KnnPlan p = plan_cosine_topk(
          B, N, 5, env_of({{"KAKVEDA_KNN_EMIT_SEG", "64"}}), true, true);
      ++cases;
      CHECK(p.seg == 0);
    }

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("%ld cases passed\n", cases);
  return 0;
}
