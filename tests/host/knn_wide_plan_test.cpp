// Stand-alone check of the host plan of the wide exact search
// (knn_wide_plan.h): the k clamp, whether a floor can exist, the kernel
// choice, the record-segment capacity, the slices of the overflow fallback and
// the grouping of streamed batches. Built and run by
// tests/test_knn_wide_plan.py with the host compiler under
// -fsanitize=address,undefined. Expectations are written from the rules, not
// read back from the plan.
#include <cstdio>

#include "knn_wide_plan.h"

using namespace kakveda;

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

  // ---- the k clamp ----------------------------------------------------------
  CHECK(KWIDE_MAX == 64 && KMAX == 8 && WIDE_GROUP == 8);
  CHECK(wide_clamp_k(-5) == 1 && wide_clamp_k(0) == 1 && wide_clamp_k(1) == 1);
  CHECK(wide_clamp_k(9) == 9 && wide_clamp_k(64) == 64);
  CHECK(wide_clamp_k(65) == 64 && wide_clamp_k(1L << 40) == 64);

  // ---- whether a floor can exist: every prepass block of 1,024 columns keeps
  // 8 entries, so k entries need ceil(k / 8) blocks with 8 columns each -------
  CHECK(wide_partial_slots(1) == 1 && wide_partial_slots(8) == 8);
  CHECK(wide_partial_slots(40) == 8 && wide_partial_slots(1024) == 8);
  CHECK(wide_partial_slots(1025) == 9 && wide_partial_slots(1032) == 16);
  CHECK(wide_partial_slots(4100) == 36);
  CHECK(wide_partial_slots(262144) == 2048 && wide_partial_slots(10000000) == 2048);
  CHECK(!plan_wide(1, 40, 64, false, 32768, 0, 0, false).prepass);
  CHECK(plan_wide(1, 4100, 33, false, 32768, 0, 0, false).prepass);
  CHECK(!plan_wide(1, 4100, 64, false, 32768, 0, 0, false).prepass);
  CHECK(plan_wide(1, 7 * 1024 + 8, 64, false, 32768, 0, 0, false).prepass);
  CHECK(!plan_wide(1, 7 * 1024 + 7, 64, false, 32768, 0, 0, false).prepass);

  // ---- table ------------------------------------------------------------------
  const int Bs[] = {1, 4, 8, 9, 20, 130, 257, 2048, 8192};
  const int Ns[] = {1, 40, 64, 1000, 4095, 4096, 4100, 65536, 65700, 1000000, 10000000};
  const long ks[] = {1, 8, 9, 16, 33, 64, 65, 1000};
  const long caps[] = {1, 128, 4096, 32768, 100000};
  const long segs[] = {0, 1, 100, 1000000000L};
  for (int B : Bs)
    for (int N : Ns)
      for (long cap : caps)
        for (long seg : segs)
          for (int filtered = 0; filtered < 2; ++filtered)
            for (int slice = 0; slice < 2; ++slice) {
              long prev_seg = 0;
              for (long k : ks) {
                const WidePlan p =
                    plan_wide(B, N, k, filtered != 0, cap, seg, 0, slice != 0);
                ++cases;
                CHECK(p.k >= 1 && p.k <= KWIDE_MAX);
                CHECK(p.k == (k > 64 ? 64 : k));
                CHECK(p.cap == cap);
                CHECK(p.prepass == (wide_partial_slots(N) >= p.k));
                // the prepass covers the sample with blocks of PRE_TILES tiles
                CHECK(p.pre_tiles == PRE_TILES && p.pre_grid % 8 == 0);
                CHECK(p.pre_grid >= 8 && p.pre_grid <= WIDE_PRE_BLOCKS);
                CHECK((long)p.pre_grid * PRE_TILES * BN >=
                      (N < WIDE_PRE_BLOCKS * PRE_TILES * BN ? N
                                                            : WIDE_PRE_BLOCKS * PRE_TILES * BN));
                CHECK((long)p.pre_grid * KMAX <= 2 * WIDE_SEL_TILE);
                CHECK(p.smallb_blocks >= 1 && p.smallb_blocks <= 8192);
                // the kernel choice
                if (B <= WIDE_GROUP) {
                  CHECK(p.main == WideMain::Stream && p.groups == 1);
                } else if (p.main == WideMain::Emit8p) {
                  CHECK(!filtered && !slice && N >= MIN_N_8P && p.groups == 0);
                } else {
                  CHECK(p.main == WideMain::StreamGroups);
                  CHECK(p.groups == (B + 7) / 8);
                }
                // a filtered batch and a fallback slice never see a segment
                if (filtered || slice) CHECK(p.main != WideMain::Emit8p);
                // groups are of at most 8 queries and tile the batch
                if (p.main != WideMain::Emit8p) {
                  long next = 0;
                  for (int g = 0; g < p.groups; ++g) {
                    const WideSpan s = wide_group(B, g);
                    CHECK(s.first == next && s.count >= 1 && s.count <= WIDE_GROUP);
                    next += s.count;
                  }
                  CHECK(next == B);
                  CHECK(p.seg == 0);
                  continue;
                }
                // segments: monotone in k, within the candidate buffer's bytes,
                // a forced size honoured where the budget allows
                const long blocks = (long)p.ch.nchunks * p.ch.row_tiles;
                CHECK(p.ch.chunk_tiles >= 4 && p.ch.chunk_tiles <= 128);
                CHECK((long)p.ch.nchunks * p.ch.chunk_tiles >= p.ch.ntiles);
                CHECK(p.ch.row_tiles == (B + BM8 - 1) / BM8);
                CHECK(p.seg >= 1 && p.seg <= 2147483647L);
                CHECK(blocks * p.seg * 8 <= (long)B * cap * 8);
                CHECK(p.seg >= prev_seg);
                prev_seg = p.seg;
                const long budget = (long)B * cap / blocks;
                const long want =
                    seg > 0 ? seg : EMIT_SEG_DEFAULT * ((p.k + KMAX - 1) / KMAX);
                CHECK(p.seg == (want < budget ? want : budget));
              }
            }
  // the default grows with k where the budget leaves room
  CHECK(wide_seg_cap(2048, 32768, chunking(2048, 10000000, BM8, 512), 9, 0) ==
        2 * EMIT_SEG_DEFAULT);
  CHECK(wide_seg_cap(2048, 32768, chunking(2048, 10000000, BM8, 512), 64, 0) >
        wide_seg_cap(2048, 32768, chunking(2048, 10000000, BM8, 512), 16, 0));

  // ---- slices of the fallback: consecutive, never longer than cap, and they
  // tile [0, N) ---------------------------------------------------------------
  for (int N : Ns)
    for (long cap : caps) {
      const long n = wide_slice_count(N, cap);
      long next = 0;
      for (long s = 0; s < n; ++s) {
        const WideSpan sl = wide_slice(N, cap, s);
        CHECK(sl.first == next && sl.count >= 1 && sl.count <= cap);
        next += sl.count;
        ++cases;
      }
      CHECK(next == N);
      CHECK(n == (N + cap - 1) / cap);
    }
  CHECK(wide_slice_count(100, 0) == 100);  // a cap below 1 is 1

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("%ld cases passed\n", cases);
  return 0;
}
