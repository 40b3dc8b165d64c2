// Stand-alone check of the routed-search plan (ops/hip/ivf_plan.h): row ->
// segment mapping, slice/slot counts, segment-layout refusals. Built with
// the host compiler under ASan + UBSan by tests/test_ivf_plan.py.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "ivf_plan.h"

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

static void test_row_to_segment() {
  // s0 a multiple of q, and not (1000 vs 2048: the three-segment GPU test)
  const long cases[][2] = {{4096, 4096}, {1000, 2048}, {1, 7}, {2048, 1000}};
  for (auto& c : cases) {
    const long s0 = c[0], q = c[1];
    CHECK(ivf_segment_of(0, s0, q) == 0 && ivf_local_row(0, s0, q) == 0);
    CHECK(ivf_segment_of(s0 - 1, s0, q) == 0);
    CHECK(ivf_local_row(s0 - 1, s0, q) == s0 - 1);
    for (int seg = 1; seg <= 4; ++seg) {
      const long first = s0 + (seg - 1) * q, last = first + q - 1;
      CHECK(ivf_segment_of(first, s0, q) == seg);
      CHECK(ivf_local_row(first, s0, q) == 0);
      CHECK(ivf_segment_of(last, s0, q) == seg);
      CHECK(ivf_local_row(last, s0, q) == q - 1);
      CHECK(ivf_segment_of(first - 1, s0, q) == seg - 1);
    }
  }
  // exhaustive against a walk over a small layout
  const long s0 = 5, q = 3;
  for (long r = 0; r < 40; ++r) {
    int seg = 0;
    long base = 0, rows = s0;
    while (r >= base + rows) {
      base += rows;
      rows = q;
      ++seg;
    }
    CHECK(ivf_segment_of(r, s0, q) == seg);
    CHECK(ivf_local_row(r, s0, q) == r - base);
  }
  // single segment: q == 1 is never used below s0
  CHECK(ivf_segment_of(123456, 1L << 20, 1) == 0);
}

static void test_plan() {
  const long lens[] = {0, 1, 31, 32, 33, 8192};
  const long tails[] = {0, 500};
  for (long len : lens)
    for (long tail : tails)
      for (int nprobe : {1, 8, 32})
        for (int B : {1, 8, 256}) {
          const IvfPlan p = plan_ivf_scan(len, tail, nprobe, B);
          CHECK(p.sources == nprobe + 1);
          CHECK(p.slices >= 1 && p.slices <= IVF_MAX_SLICES);
          CHECK(p.slots == (long)p.sources * p.slices);
          CHECK(p.cand_entries == p.slots * KMAX);
          const long longest = len > tail ? len : tail;
          // no more slices than the longest source has 256-row pieces
          const long want = (longest + IVF_ROWS_PER_SLICE - 1) / IVF_ROWS_PER_SLICE;
          CHECK(p.slices <= (want > 1 ? want : 1));
          // the launch stays within the block budget unless one slice
          // per source already exceeds it
          const long blocks = (long)p.slices * p.sources * B;
          CHECK(blocks <= IVF_MAX_BLOCKS || p.slices == 1);
        }
  CHECK(plan_ivf_scan(0, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(1, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(31, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(32, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(33, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(256, 0, 8, 1).slices == 1);
  CHECK(plan_ivf_scan(257, 0, 8, 1).slices == 2);
  CHECK(plan_ivf_scan(8192, 0, 8, 1).slices == 32);
  CHECK(plan_ivf_scan(0, 500, 8, 1).slices == 2);     // the tail sizes it too
  CHECK(plan_ivf_scan(8192, 500, 8, 1).slices == 32);
  CHECK(plan_ivf_scan(1 << 20, 0, 8, 1).slices == IVF_MAX_SLICES);
  // block budget: 33 sources x 256 queries leave 7 slices
  CHECK(plan_ivf_scan(8192, 0, 32, 256).slices == 7);
  CHECK(plan_ivf_scan(8192, 0, 32, 1 << 20).slices == 1);  // chunked by grid.z
  CHECK(plan_ivf_scan(8192, 0, 0, 1).sources == 1);        // tail only
  CHECK(throws([] { plan_ivf_scan(-1, 0, 1, 1); }));
  CHECK(throws([] { plan_ivf_scan(0, 0, 1, 0); }));
}

static void test_segments() {
  std::vector<long> rows(65, 2048);
  rows[0] = 1000;
  auto of = [&](int i) { return rows[i]; };
  CHECK(ivf_check_segments(1, of) == 1);
  CHECK(ivf_check_segments(2, of) == 2048);
  CHECK(ivf_check_segments(64, of) == 2048);
  CHECK(throws([&] { ivf_check_segments(65, of); }));
  CHECK(throws([&] { ivf_check_segments(0, of); }));
  rows[3] = 2047;  // a later segment off the quantum
  CHECK(ivf_check_segments(3, of) == 2048);
  CHECK(throws([&] { ivf_check_segments(4, of); }));
  rows[3] = 2048;
  rows[0] = 0;
  CHECK(throws([&] { ivf_check_segments(2, of); }));
}

int main() {
  test_row_to_segment();
  test_plan();
  test_segments();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
