// Stand-alone check of the list-major routed-scan plan
// (ops/hip/ivf_batch_plan.h): the tile bound against the true tile count of
// adversarial groupings, slice/slot counts, the candidate-byte cap and its
// chunking, refusals. Built with the host compiler under ASan + UBSan by
// tests/test_ivf_batch_plan.py.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "ivf_batch_plan.h"

using namespace kakveda;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// tiles a grouping makes: every non-empty group is cut into QTILE pieces
static long true_tiles(const std::vector<long>& group_sizes) {
  long t = 0;
  for (long c : group_sizes) t += (c + IVF_BATCH_QTILE - 1) / IVF_BATCH_QTILE;
  return t;
}

// groupings of P pairs over L lists + the tail (L + 1 groups; the tail
// always holds B pairs, the rest is spread adversarially)
static void check_bound(int B, int nprobe, int L) {
  const long P = (long)B * (nprobe + 1);
  const long bound = plan_ivf_batch(100, 0, nprobe, B, L).max_tiles;
  CHECK(bound == ivf_batch_tile_bound(P, L));
  CHECK(bound <= P);
  const long rest = P - B;  // the pairs of real lists
  // (a) all pairs of real lists in one list
  if (L >= 1) {
    std::vector<long> g(L + 1, 0);
    g[0] = rest;
    g[L] = B;
    CHECK(true_tiles(g) <= bound);
  }
  // (b) one pair per list as far as the lists go, the remainder in the last
  if (L >= 1) {
    std::vector<long> g(L + 1, 0);
    long left = rest;
    for (int l = 0; l < L && left > 0; ++l) {
      g[l] = 1;
      --left;
    }
    g[L - 1] += left;
    g[L] = B;
    CHECK(true_tiles(g) <= bound);
  }
  // (c) QTILE + 1 pairs per list: every list wastes a nearly empty tile
  if (L >= 1) {
    std::vector<long> g(L + 1, 0);
    long left = rest;
    for (int l = 0; l < L && left > 0; ++l) {
      g[l] = std::min<long>(left, IVF_BATCH_QTILE + 1);
      left -= g[l];
    }
    g[L - 1] += left;
    g[L] = B;
    CHECK(true_tiles(g) <= bound);
  }
  // (d) every probe discarded: only the tail group is left
  {
    std::vector<long> g(L + 1, 0);
    g[L] = B;
    CHECK(true_tiles(g) <= bound);
  }
  // (e) even spread
  if (L >= 1) {
    std::vector<long> g(L + 1, rest / L);
    g[0] += rest % L;
    g[L] = B;
    CHECK(true_tiles(g) <= bound);
  }
}

static void test_tile_bound() {
  for (int B : {1, 3, 15, 16, 17, 100, 2048})
    for (int nprobe : {0, 1, 5, 32, 64})
      for (int L : {0, 1, 2, 18, 64, 3160}) check_bound(B, nprobe, L);
  // P < QTILE: no more tiles than pairs
  CHECK(plan_ivf_batch(10, 0, 2, 1, 3160).max_tiles == 3);
  CHECK(plan_ivf_batch(10, 0, 4, 3, 1).max_tiles == 15 / IVF_BATCH_QTILE + 2);
  // L = 1: P / QTILE + 2
  CHECK(plan_ivf_batch(10, 0, 1, 100, 1).max_tiles == 200 / IVF_BATCH_QTILE + 2);
  CHECK(ivf_batch_tile_bound(0, 5) == 0);
}

static void test_plan() {
  const long lens[] = {0, 1, 63, 64, 65, 1024, 1025, 8192, 1L << 22};
  const long tails[] = {0, 500, 1L << 20};
  for (long len : lens)
    for (long tail : tails)
      for (int nprobe : {0, 1, 8, 32, 64})
        for (int B : {1, 15, 16, 17, 256, 2048})
          for (int L : {1, 18, 3160}) {
            const IvfBatchPlan p = plan_ivf_batch(len, tail, nprobe, B, L);
            CHECK(p.pairs == (long)B * (nprobe + 1));
            CHECK(p.slices >= 1 && p.slices <= IVF_BATCH_MAX_SLICES);
            CHECK(p.slots == (long)(nprobe + 1) * p.slices);
            // slots * KMAX is what the launch allocates per query
            CHECK(p.cand_entries == p.slots * KMAX);
            CHECK(p.cand_bytes == (long)B * p.cand_entries * 8);
            const long longest = len > tail ? len : tail;
            const long want = (longest + IVF_BATCH_ROWS_PER_SLICE - 1) /
                              IVF_BATCH_ROWS_PER_SLICE;
            CHECK(p.slices <= (want > 1 ? want : 1));
            CHECK(p.max_tiles * p.slices <= IVF_MAX_BLOCKS || p.slices == 1);
            // chunking keeps every launch's candidate bytes under the cap
            // (or at one query, which cannot be split)
            const int chunk = ivf_batch_chunk_queries(len, tail, nprobe, B, L);
            CHECK(chunk >= 1 && chunk <= B);
            for (int nb : {chunk, B % chunk ? B % chunk : chunk, 1}) {
              const IvfBatchPlan c = plan_ivf_batch(len, tail, nprobe, nb, L);
              CHECK(c.cand_bytes <= IVF_BATCH_MAX_CAND_BYTES || nb == 1);
            }
          }
  CHECK(plan_ivf_batch(0, 0, 8, 1, 10).slices == 1);
  CHECK(plan_ivf_batch(1024, 0, 8, 1, 10).slices == 1);
  CHECK(plan_ivf_batch(1025, 0, 8, 1, 10).slices == 2);
  CHECK(plan_ivf_batch(0, 1025, 8, 1, 10).slices == 2);  // the tail sizes it too
  CHECK(plan_ivf_batch(1L << 22, 0, 8, 1, 10).slices == IVF_BATCH_MAX_SLICES);
  // block budget: 2048 x 33 pairs over 3160 lists bound 7385 tiles -> 8 slices
  CHECK(plan_ivf_batch(1L << 22, 0, 32, 2048, 3160).max_tiles == 7385);
  CHECK(plan_ivf_batch(1L << 22, 0, 32, 2048, 3160).slices == 8);
  // a batch that must be chunked: 65 sources x 64 slices x 64 B = 266,240 B
  // per query, 1008 queries fit 256 MiB
  CHECK(ivf_batch_chunk_queries(1L << 22, 0, 64, 4096, 3160) == 1008);
  CHECK(ivf_batch_chunk_queries(100, 0, 32, 2048, 3160) == 2048);
  CHECK(throws([] { plan_ivf_batch(-1, 0, 1, 1, 1); }));
  CHECK(throws([] { plan_ivf_batch(0, -1, 1, 1, 1); }));
  CHECK(throws([] { plan_ivf_batch(0, 0, -1, 1, 1); }));
  CHECK(throws([] { plan_ivf_batch(0, 0, 1, 0, 1); }));
  CHECK(throws([] { plan_ivf_batch(0, 0, 1, 1, -1); }));
  CHECK(throws([] { ivf_batch_chunk_queries(0, 0, 1, -1, 1); }));
}

static void test_query_lds() {
  // IVF_BATCH_MAX_D is the widest multiple of 64 whose query tile fits
  static_assert(IVF_BATCH_MAX_D % 64 == 0, "D is a multiple of 64");
  CHECK(ivf_batch_query_lds(IVF_BATCH_MAX_D) <= IVF_BATCH_MAX_QUERY_LDS);
  CHECK(ivf_batch_query_lds(IVF_BATCH_MAX_D + 64) > IVF_BATCH_MAX_QUERY_LDS);
  CHECK(ivf_batch_query_lds(768) == 24832);
  // with the kernel's 16 KiB + 64 B of static LDS: within 64 KiB
  CHECK(ivf_batch_query_lds(IVF_BATCH_MAX_D) + 16448 <= 64 * 1024);
}

int main() {
  test_query_lds();
  test_tile_bound();
  test_plan();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
