// Stand-alone check of the prepass launch geometry in the cosine_topk
// dispatch plan (knn_plan.h: prepass_geometry, KnnPlan::pre_grid / pre_tiles,
// KAKVEDA_KNN_PRE_TILES, forced_pre_grid). Built and run by
// tests/test_knn_prepass_geom.py with the host compiler under
// -fsanitize=address,undefined. Expectations are written from the rules (the
// sample stays preg * 8 column tiles; only the compact prepass of the
// emission floors runs longer blocks, in doublings of 8 tiles, while the
// grid stays a multiple of 8 and fills one round of 512 resident blocks; the
// fields that existed before keep the values the earlier rules gave them),
// not read back from the plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
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

static bool same(const Chunking& a, const Chunking& b) {
  return a.row_tiles == b.row_tiles && a.ntiles == b.ntiles &&
         a.chunk_tiles == b.chunk_tiles && a.nchunks == b.nchunks;
}

static bool parse_throws(const char* value) {
  try {
    env_of({{"KAKVEDA_KNN_PRE_TILES", value}});
  } catch (const std::runtime_error& e) {
    return std::strstr(e.what(), "KAKVEDA_KNN_PRE_TILES") != nullptr;
  }
  return false;
}

static bool plan_throws(int B, int N, int k, const KnnEnv& env, bool allow,
                        bool filtered) {
  try {
    plan_cosine_topk(B, N, k, env, allow, filtered);
  } catch (const std::runtime_error& e) {
    return std::strstr(e.what(), "KAKVEDA_KNN_PRE_TILES") != nullptr;
  }
  return false;
}

// ---- the rules as they stood before the prepass had a launch geometry -----
static Chunking old_chunking(int B, int N, int tile, long target) {
  Chunking c;
  c.row_tiles = (B + tile - 1) / tile;
  c.ntiles = (N + tile - 1) / tile;
  const long want = ((long)c.ntiles * c.row_tiles + target - 1) / target;
  c.chunk_tiles = (int)std::max(4L, std::min(want, 128L));
  c.nchunks = ((c.ntiles + c.chunk_tiles - 1) / c.chunk_tiles + 7) & ~7;
  return c;
}

struct OldPlan {
  bool emit, use8p;
  int tile, preg;
  Chunking ch;
  bool prepass, compact;
};

// sel: nullptr, "list", "8pe"; preg_env / target_env: 0 is unset.
static OldPlan old_plan(int B, int N, int k, const char* sel, int preg_env,
                        long target_env, bool allow, bool filtered) {
  OldPlan o;
  if (filtered) {
    o.emit = allow && N >= 65536 && B <= 8;
    o.use8p = false;
  } else {
    const bool want = !sel ? k > 1 : !std::strcmp(sel, "8pe");
    o.emit = want && N >= 65536 && allow;
    o.use8p = o.emit;
  }
  o.tile = o.use8p ? 256 : 128;
  o.ch = old_chunking(B, N, o.tile,
                      target_env > 0 ? target_env : (o.tile == 256 ? 512 : 2048));
  o.preg = std::min(preg_env > 0 ? preg_env : (o.emit ? 256 : 64), o.ch.nchunks) & ~7;
  const bool psmall = o.ch.ntiles <= o.preg * 8 * 32;
  o.prepass = (o.emit || (!o.use8p && k > 1 && o.ch.ntiles >= o.preg * 8 && psmall)) &&
              o.preg >= 8;
  o.compact = o.emit && o.prepass;
  return o;
}

// The geometry rule, from its statement: the largest 8 * 2^j that divides
// the sample into a multiple-of-8 grid of at least 512 blocks in all.
static int rule_pre_tiles(int preg, int B) {
  const long total = (long)preg * 8, row_tiles = (B + 127) / 128;
  int best = 8;
  for (long t = 16; t <= total; t *= 2) {
    if (total % t) continue;
    const long g = total / t;
    if (g % 8 == 0 && g * row_tiles >= 512) best = (int)t;
  }
  return best;
}

int main() {
  long cases = 0;

  // ---- the knob's form ------------------------------------------------------
  CHECK(env_of({}).pre_tiles == 0);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", ""}}).pre_tiles == 0);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "8"}}).pre_tiles == 8);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "16"}}).pre_tiles == 16);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "24"}}).pre_tiles == 24);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "2048"}}).pre_tiles == 2048);
  for (const char* bad : {"0", "-8", "4", "12", "7", "8x", "x", " 8", "8 ", "+8",
                          "1e3", "8.0", "0x10", "99999999999999999999",
                          "100000008"})
    CHECK(parse_throws(bad));
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "16"}}).cap == 32768);
  CHECK(env_of({{"KAKVEDA_KNN_PRE_TILES", "16"}}).skip_sample);

  // ---- forced_pre_grid ------------------------------------------------------
  CHECK(forced_pre_grid(64, 8, "x") == 64);
  CHECK(forced_pre_grid(64, 16, "x") == 32);
  CHECK(forced_pre_grid(64, 64, "x") == 8);
  CHECK(forced_pre_grid(72, 8, "x") == 72);
  CHECK(forced_pre_grid(72, 24, "x") == 24);
  CHECK(forced_pre_grid(8, 8, "x") == 8);
  for (auto bad : {std::pair<int, long>{64, 128}, {64, 512}, {64, 0}, {64, -16},
                   {64, 12}, {72, 16}, {72, 64}, {8, 16}, {64, 24},
                   {64, 1L << 40}}) {
    bool threw = false;
    try {
      forced_pre_grid(bad.first, bad.second, "pre_tiles");
    } catch (const std::runtime_error& e) {
      threw = std::strstr(e.what(), "pre_tiles") != nullptr;
    }
    CHECK(threw);
  }

  // ---- the expected geometries ----------------------------------------------
  {
    const KnnPlan p = plan_cosine_topk(2048, 10000000, 5, env_of({}), true);
    CHECK(p.preg == 256 && p.prepass_compact);
    CHECK(p.pre_grid == 32 && p.pre_tiles == 64);
    CHECK(p.skip_tiles == 1024);  // the sample itself is what it was
    const KnnPlan s = plan_cosine_topk(2048, 1250000, 5, env_of({}), true);
    CHECK(s.preg == 64 && s.pre_grid == 32 && s.pre_tiles == 16);
    const KnnPlan h = plan_cosine_topk(2048, 2500000, 5, env_of({}), true);
    CHECK(h.pre_grid * h.pre_tiles == h.preg * 8 && h.pre_grid % 8 == 0 &&
          h.pre_grid * 16 >= 512 && (h.pre_grid / 2 % 8 != 0 || h.pre_grid * 8 < 512));
    const KnnPlan b256 = plan_cosine_topk(256, 10000000, 5, env_of({}), true);
    CHECK(b256.prepass_compact && b256.pre_grid == b256.preg && b256.pre_tiles == 8);
    for (int B : {1, 4, 8}) {
      const KnnPlan u = plan_cosine_topk(B, 10000000, 5, env_of({}), true);
      CHECK(u.main == MainKernel::SmallB && u.prepass_compact);
      CHECK(u.pre_grid == u.preg && u.pre_tiles == 8);
      const KnnPlan f = plan_cosine_topk(B, 10000000, 5, env_of({}), true, true);
      CHECK(f.main == MainKernel::SmallB && f.prepass_compact);
      CHECK(f.pre_grid == f.preg && f.pre_tiles == 8);
    }
    // the knob forces it, 8 is the launch of one block per sampled chunk
    const KnnPlan f8 = plan_cosine_topk(
        2048, 10000000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "8"}}), true);
    CHECK(f8.pre_grid == 256 && f8.pre_tiles == 8);
    const KnnPlan f128 = plan_cosine_topk(
        2048, 10000000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "128"}}), true);
    CHECK(f128.pre_grid == 16 && f128.pre_tiles == 128);
    const KnnPlan ff = plan_cosine_topk(
        8, 70000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "16"}}), true, true);
    CHECK(ff.prepass_compact && ff.preg == 144 && ff.pre_grid == 72 && ff.pre_tiles == 16);
    // a size the sample does not divide into a multiple-of-8 grid is refused
    CHECK(plan_throws(2048, 10000000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "512"}}), true, false));
    CHECK(plan_throws(2048, 1250000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "128"}}), true, false));
    CHECK(plan_throws(2048, 10000000, 5, env_of({{"KAKVEDA_KNN_PRE_TILES", "24"}}), true, false));
    // ... and only where the compact prepass runs: the fallback replan and
    // the list path do not read it
    const KnnEnv e512 = env_of({{"KAKVEDA_KNN_PRE_TILES", "512"}});
    CHECK(!plan_throws(2048, 10000000, 5, e512, false, false));
    CHECK(!plan_throws(2048, 10000000, 1, e512, true, false));
    CHECK(!plan_throws(300, 70000, 5, e512, true, true));
  }

  // ---- table ------------------------------------------------------------------
  const int Bs[] = {1, 8, 9, 130, 256, 300, 1024, 2048, 4096, 8192};
  const int Ns[] = {4096,    65536,   65600,   70000,   131072,  262145, 300000,
                    1250000, 2500000, 5000000, 10000000, 100000000};
  const int ks[] = {1, 5, 8};
  const char* sels[] = {nullptr, "list", "8pe"};
  const char* pregs[] = {nullptr, "3", "8", "24", "64", "250", "1000"};
  const char* targets[] = {nullptr, "1", "768", "100000"};
  const char* knobs[] = {nullptr, "8", "16", "32", "64", "128", "24"};
  for (int B : Bs)
    for (int N : Ns)
      for (int k : ks)
        for (const char* sel : sels)
          for (const char* preg : pregs)
            for (const char* target : targets)
              for (const char* knob : knobs)
                for (int variant = 0; variant < 3; ++variant) {
                  // 0: default, 1: fallback replan, 2: filtered
                  EnvVars vars;
                  if (sel) vars.push_back({"KAKVEDA_KNN_KERNEL", sel});
                  if (preg) vars.push_back({"KAKVEDA_KNN_PREG", preg});
                  if (target) vars.push_back({"KAKVEDA_KNN_TARGET", target});
                  const KnnEnv env_unset = env_of(vars);
                  if (knob) vars.push_back({"KAKVEDA_KNN_PRE_TILES", knob});
                  const KnnEnv env = env_of(vars);
                  const bool allow = variant != 1, filtered = variant == 2;
                  ++cases;

                  const OldPlan o =
                      old_plan(B, N, k, sel, preg ? std::atoi(preg) : 0,
                               target ? std::atol(target) : 0, allow, filtered);
                  const long total = (long)o.preg * 8;
                  const long kt = knob ? std::atol(knob) : 0;
                  const bool fits =
                      !knob || !o.compact ||
                      (total % kt == 0 && (kt == 8 || total / kt % 8 == 0));
                  if (!fits) {
                    CHECK(plan_throws(B, N, k, env, allow, filtered));
                    continue;
                  }
                  const KnnPlan p = plan_cosine_topk(B, N, k, env, allow, filtered);
                  // the knob moves nothing but the two new fields
                  const KnnPlan u =
                      plan_cosine_topk(B, N, k, env_unset, allow, filtered);
                  CHECK(p.main == u.main && p.mode == u.mode && p.tile == u.tile);
                  CHECK(same(p.ch, u.ch) && p.preg == u.preg);
                  CHECK(p.prepass == u.prepass && p.prepass_mode == u.prepass_mode &&
                        p.prepass_compact == u.prepass_compact);
                  CHECK(p.cap == u.cap && p.seg == u.seg &&
                        p.smallb_blocks == u.smallb_blocks && p.merge == u.merge);
                  CHECK(p.skip_tiles == u.skip_tiles && same(p.mch, u.mch) &&
                        p.mseg == u.mseg);
                  // and they are what the earlier rules gave
                  CHECK(p.tile == o.tile && same(p.ch, o.ch) && p.preg == o.preg);
                  CHECK(p.prepass == o.prepass && p.prepass_compact == o.compact);
                  CHECK(p.cap == 32768);
                  if (p.main == MainKernel::Emit8p) {
                    const long blocks = (long)o.ch.nchunks * o.ch.row_tiles;
                    CHECK(p.seg == std::min(8192L, std::max(1L, (long)B * 32768 / blocks)));
                    const bool skips = p.prepass && o.preg * 4 < o.ch.ntiles;
                    CHECK(p.skip_tiles == (skips ? o.preg * 4 : 0));
                    CHECK(p.skip_tiles + p.mch.ntiles == p.ch.ntiles);
                  } else {
                    CHECK(p.skip_tiles == 0 && same(p.mch, p.ch) && p.mseg == p.seg);
                  }

                  // the new fields
                  CHECK((long)p.pre_grid * p.pre_tiles == total);
                  CHECK(p.pre_tiles >= 8 && p.pre_tiles % 8 == 0);
                  if (p.pre_tiles != 8) CHECK(p.pre_grid % 8 == 0 && p.pre_grid >= 8);
                  if (!o.compact) {
                    CHECK(p.pre_grid == o.preg && p.pre_tiles == 8);
                  } else if (knob) {
                    CHECK(p.pre_tiles == kt && p.pre_grid == total / kt);
                  } else {
                    CHECK(p.pre_tiles == rule_pre_tiles(o.preg, B));
                    const long row_tiles = (B + 127) / 128;
                    if (p.pre_tiles != 8)
                      CHECK(p.pre_grid * row_tiles >= 512);
                    // at most 256 sampled chunks by default: two row tiles
                    // or fewer never fill a round with longer blocks
                    if (!preg && (B <= 256 || filtered)) CHECK(p.pre_tiles == 8);
                  }
                  // every prepass block's partial slot is inside the buffer
                  // its launch writes: [row][pre_grid] of its own (compact) or
                  // [row][ch.nchunks] of the main launch
                  if (p.prepass && !o.compact) CHECK(p.pre_grid <= p.ch.nchunks);
                }

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("%ld cases passed\n", cases);
  return 0;
}
