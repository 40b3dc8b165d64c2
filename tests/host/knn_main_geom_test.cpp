// Stand-alone check of the emission main launch geometry in the cosine_topk
// dispatch plan (knn_plan.h: main_geometry, KnnPlan::skip_tiles / mch / mseg,
// KAKVEDA_KNN_SKIP_SAMPLE). Built and run by tests/test_knn_main_geom.py with
// the host compiler under -fsanitize=address,undefined. Expectations are
// written from the rules (the sample is preg * 1024 columns = preg * 4 tiles
// of 256; only the unfiltered 8-phase emission plan skips it, and only where
// it does not cover the corpus; the remaining
// tiles are covered exactly once; the fields that existed before keep their
// values), not read back from the plan.
#include <algorithm>
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

// The whole-corpus chunking rule as it stood before the main launch had a
// geometry of its own (256-column tiles, block target 512 by default).
static Chunking old_chunking8p(int B, int N, long target) {
  Chunking c;
  c.row_tiles = (B + 255) / 256;
  c.ntiles = (N + 255) / 256;
  const long want = ((long)c.ntiles * c.row_tiles + target - 1) / target;
  c.chunk_tiles = (int)std::max(4L, std::min(want, 128L));
  c.nchunks = ((c.ntiles + c.chunk_tiles - 1) / c.chunk_tiles + 7) & ~7;
  return c;
}

// The makespan model of the main launch, in column tiles per CU: one block
// per CU, 32 CUs per XCD, each XCD gets an eighth of the (padded) chunks
// times every row tile, so the busiest XCD runs ceil(ceil(real / 8) *
// row_tiles / 32) rounds of chunk_tiles tiles. Ideal: tiles * row_tiles / 256.
static long makespan(int row_tiles, int ntiles, int chunk_tiles) {
  if (ntiles <= 0) return 0;
  const long real = (ntiles + chunk_tiles - 1) / chunk_tiles;
  const long blocks_per_xcd = (real + 7) / 8 * row_tiles;
  return chunk_tiles * ((blocks_per_xcd + 31) / 32);
}

static bool throws(const EnvVars& vars) {
  try {
    env_of(vars);
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main() {
  long cases = 0;

  // ---- the off switch -------------------------------------------------------
  CHECK(env_of({}).skip_sample);
  CHECK(env_of({{"KAKVEDA_KNN_SKIP_SAMPLE", "1"}}).skip_sample);
  CHECK(!env_of({{"KAKVEDA_KNN_SKIP_SAMPLE", "0"}}).skip_sample);
  CHECK(env_of({{"KAKVEDA_KNN_SKIP_SAMPLE", ""}}).skip_sample);
  CHECK(throws({{"KAKVEDA_KNN_SKIP_SAMPLE", "no"}}));
  CHECK(throws({{"KAKVEDA_KNN_SKIP_SAMPLE", "2"}}));
  CHECK(throws({{"KAKVEDA_KNN_SKIP_SAMPLE", "01"}}));
  CHECK(env_of({{"KAKVEDA_KNN_SKIP_SAMPLE", "0"}}).cap == 32768);

  // ---- the bench shape and its shards ---------------------------------------
  {
    const KnnPlan p = plan_cosine_topk(2048, 10000000, 5, env_of({}), true);
    CHECK(p.main == MainKernel::Emit8p && p.preg == 256);
    CHECK(p.skip_tiles == 1024);
    CHECK(p.mch.ntiles == 39063 - 1024 && p.mch.row_tiles == 8);
    const KnnPlan s = plan_cosine_topk(2048, 1250000, 5, env_of({}), true);
    // 64 chunks of 77 tiles bound the prepass grid: the sample is 64 * 1024
    CHECK(s.preg == 64 && s.skip_tiles == 256 && s.mch.ntiles == 4883 - 256);
    // whole rounds at the four shard shapes of 10M x 2048: the modelled
    // efficiency against the ideal of the tiles actually scanned
    for (int N : {10000000, 5000000, 2500000, 1250000}) {
      const KnnPlan g = plan_cosine_topk(2048, N, 5, env_of({}), true);
      const double ideal = (double)g.mch.ntiles * g.mch.row_tiles / 256.0;
      const long ms = makespan(g.mch.row_tiles, g.mch.ntiles, g.mch.chunk_tiles);
      CHECK(ideal / (double)ms >= 0.98);
      if (ideal / (double)ms < 0.98)
        std::printf("  N=%d: chunk_tiles=%d nchunks=%d makespan=%ld ideal=%.1f\n",
                    N, g.mch.chunk_tiles, g.mch.nchunks, ms, ideal);
    }
    CHECK(p.mch.chunk_tiles == 119 && p.mch.nchunks == 320);
    // the sample is the corpus: the whole-corpus launch stays (a main launch
    // with nothing left would take the segments and their overflow fallback
    // out of every small request's path), so does one tile more
    const KnnPlan c = plan_cosine_topk(256, 65536, 5, env_of({}), true);
    CHECK(c.main == MainKernel::Emit8p && c.prepass && c.preg * 4 == c.ch.ntiles);
    CHECK(c.skip_tiles == 0 && same(c.mch, c.ch) && c.mseg == c.seg);
    const KnnPlan c1 = plan_cosine_topk(256, 65792, 5, env_of({}), true);
    CHECK(c1.preg * 4 > c1.ch.ntiles && c1.skip_tiles == 0 && same(c1.mch, c1.ch));
    const KnnPlan c2 = plan_cosine_topk(130, 262145, 5, env_of({}), true);
    CHECK(c2.skip_tiles == 1024 && c2.mch.ntiles == 1);
  }

  // ---- table ------------------------------------------------------------------
  const int Bs[] = {1, 8, 9, 130, 300, 2048, 8192};
  const int Ns[] = {4096,   65536,   65600,   70000,   262145,
                    300000, 1250000, 2500000, 5000000, 10000000, 100000000};
  const int ks[] = {1, 5, 8};
  const char* sels[] = {nullptr, "list", "8pbl", "8pe", "8pe2"};
  const char* pregs[] = {nullptr, "3", "8", "64", "250", "1000"};
  const char* targets[] = {nullptr, "1", "768", "2560", "100000"};
  const char* caps[] = {nullptr, "4", "100000"};
  for (int B : Bs)
    for (int N : Ns)
      for (int k : ks)
        for (const char* sel : sels)
          for (const char* preg : pregs)
            for (const char* target : targets)
              for (const char* cap : caps)
                for (int variant = 0; variant < 4; ++variant) {
                  // 0: default, 1: fallback replan, 2: filtered, 3: off switch
                  EnvVars vars;
                  if (sel) vars.push_back({"KAKVEDA_KNN_KERNEL", sel});
                  if (preg) vars.push_back({"KAKVEDA_KNN_PREG", preg});
                  if (target) vars.push_back({"KAKVEDA_KNN_TARGET", target});
                  if (cap) vars.push_back({"KAKVEDA_KNN_EMIT_CAP", cap});
                  const KnnEnv env_on = env_of(vars);
                  vars.push_back({"KAKVEDA_KNN_SKIP_SAMPLE", "0"});
                  const KnnEnv env_off = env_of(vars);
                  const bool allow = variant != 1, filtered = variant == 2;
                  const KnnPlan p = plan_cosine_topk(
                      B, N, k, variant == 3 ? env_off : env_on, allow, filtered);
                  const KnnPlan o =
                      plan_cosine_topk(B, N, k, env_off, allow, filtered);
                  ++cases;

                  // the fields that existed before keep their values
                  CHECK(p.main == o.main && p.mode == o.mode && p.tile == o.tile);
                  CHECK(same(p.ch, o.ch) && p.preg == o.preg);
                  CHECK(p.prepass == o.prepass &&
                        p.prepass_mode == o.prepass_mode &&
                        p.prepass_compact == o.prepass_compact);
                  CHECK(p.cap == o.cap && p.seg == o.seg &&
                        p.smallb_blocks == o.smallb_blocks && p.merge == o.merge);
                  const long tgt = target ? std::atol(target) : 512;
                  const long capv = cap ? std::atol(cap) : 32768;
                  if (p.main == MainKernel::Emit8p) {
                    const Chunking oc = old_chunking8p(B, N, tgt);
                    CHECK(same(p.ch, oc));
                    const int want_preg =
                        std::min(preg ? (int)std::atol(preg) : 256, oc.nchunks) & ~7;
                    CHECK(p.preg == want_preg);
                    CHECK(p.prepass == (want_preg >= 8));
                    const long blocks = (long)oc.nchunks * oc.row_tiles;
                    const long budget = std::max(1L, (long)B * capv / blocks);
                    CHECK(p.seg == std::min(8192L, budget));
                  }

                  // who skips: the unfiltered 8-phase emission plan whose
                  // sample leaves at least one tile
                  const bool skips = p.main == MainKernel::Emit8p && p.prepass &&
                                     !filtered && variant != 3 &&
                                     p.preg * 4 < p.ch.ntiles;
                  CHECK(p.skip_tiles >= 0 && p.skip_tiles <= p.ch.ntiles);
                  if (!skips) {
                    CHECK(p.skip_tiles == 0);
                    CHECK(same(p.mch, p.ch));
                    CHECK(p.mseg == p.seg);
                    continue;
                  }
                  CHECK(p.skip_tiles == p.preg * 4);
                  // the skipped tiles are sampled columns, all of them
                  CHECK((long)p.skip_tiles * 256 <= (long)p.preg * 1024);

                  // the rest is covered, every tile by exactly one chunk
                  CHECK(p.mch.row_tiles == p.ch.row_tiles);
                  CHECK(p.skip_tiles + p.mch.ntiles == p.ch.ntiles);
                  CHECK(p.mch.nchunks % 8 == 0 && p.mch.nchunks >= 8);
                  CHECK(p.mch.chunk_tiles >= 4 && p.mch.chunk_tiles <= 128);
                  CHECK(p.mch.ntiles >= 1);
                  long cursor = p.skip_tiles;
                  for (int c = 0; c < p.mch.nchunks; ++c) {
                    const long t0 = p.skip_tiles + (long)c * p.mch.chunk_tiles;
                    const long here = std::max(
                        0L, std::min((long)p.mch.chunk_tiles, p.ch.ntiles - t0));
                    if (here > 0) CHECK(t0 == cursor);
                    cursor += here;
                  }
                  CHECK(cursor == p.ch.ntiles);
                  // never a longer modelled makespan than the whole-corpus
                  // launch of the same input (the same ideal under both:
                  // nowhere a lower modelled efficiency than before)
                  CHECK(makespan(p.mch.row_tiles, p.mch.ntiles, p.mch.chunk_tiles) <=
                        makespan(p.ch.row_tiles, p.ch.ntiles, p.ch.chunk_tiles));
                  // no emptier than the padding to 8 needs
                  CHECK((long)(p.mch.nchunks - 8) * p.mch.chunk_tiles <
                        std::max(1, p.mch.ntiles));

                  // segments: sized from the launched geometry, never more
                  // bytes than the candidate buffer (a segment holds >= 1)
                  {
                    const long blocks = (long)p.mch.nchunks * p.mch.row_tiles;
                    CHECK(p.mseg >= 1 && p.mseg <= 8192);
                    CHECK(blocks * p.mseg <= (long)B * capv || p.mseg == 1);
                    const long budget = std::max(1L, (long)B * capv / blocks);
                    CHECK(p.mseg == std::min(8192L, budget));
                  }
                }

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("%ld cases passed\n", cases);
  return 0;
}
