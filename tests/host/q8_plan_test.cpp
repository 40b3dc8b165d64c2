// Stand-alone check of the int8 mirror's contract (ops/hip/q8_plan.h): the
// serial quantiser built from q8_scale / q8_code / q8_err on every row of a
// case file against the codes and scales the torch reference gave. Built with
// the host compiler under ASan + UBSan by tests/test_q8_plan.py, which writes
//
//   <rows> <D>
//   then per row: D values (the bf16 row as floats), D codes, the scale bits
//
// Codes and scale bits must be equal; the error must bound the residual's
// norm (evaluated in double) and stay within 1% + 1e-7 of it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "q8_plan.h"

using namespace kakveda;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static void test_pieces() {
  CHECK(q8_dim_ok(128) && q8_dim_ok(768) && !q8_dim_ok(64) && !q8_dim_ok(192) &&
        !q8_dim_ok(0) && !q8_dim_ok(1L << 20));
  const Q8Scale zero = q8_scale(0.0f);
  CHECK(zero.scale == 0.0f && zero.inv == 0.0f);
  const Q8Scale tiny = q8_scale(0x1p-110f);
  CHECK(tiny.scale == 0.0f && tiny.inv == 0.0f);
  const Q8Scale nan = q8_scale(NAN);
  CHECK(nan.scale == 0.0f && nan.inv == 0.0f);
  const Q8Scale one = q8_scale(127.0f);
  CHECK(one.scale == 1.0f && one.inv == 1.0f);
  // round half to even, clamp to +-127
  CHECK(q8_code(0.5f, 1.0f) == 0 && q8_code(1.5f, 1.0f) == 2 && q8_code(2.5f, 1.0f) == 2);
  CHECK(q8_code(-0.5f, 1.0f) == 0 && q8_code(-1.5f, 1.0f) == -2);
  CHECK(q8_code(1000.0f, 1.0f) == 127 && q8_code(-1000.0f, 1.0f) == -127);
  CHECK(q8_code(3.0f, 0.0f) == 0);
  CHECK(q8_err(0.0f, 0.0f, 0.0f, 768) == 0.0f);
  CHECK(q8_err(1.0f, 1.0f, 1.0f / 127.0f, 768) > 1.0f);
  CHECK(q8_err(1.0f, 1.0f, 1.0f / 127.0f, 768) < 1.0001f);
  CHECK(q8_roundup(768) == 1.0f + 784.0f * 0x1p-24f);
  CHECK(q8_slack(128) == 128.0f * 0x1p-22f);
}

int main(int argc, char** argv) {
  test_pieces();
  if (argc < 2) {
    std::printf("usage: q8_plan_test <case file>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  long rows = 0, D = 0;
  in >> rows >> D;
  CHECK(in.good() && rows > 0 && q8_dim_ok(D));
  std::vector<float> c(D);
  std::vector<int> want(D);
  for (long r = 0; r < rows && failures == 0; ++r) {
    for (long i = 0; i < D; ++i) in >> c[i];
    for (long i = 0; i < D; ++i) in >> want[i];
    uint32_t scale_bits = 0;
    in >> scale_bits;
    CHECK(!in.fail());
    float amax = 0.0f;
    for (long i = 0; i < D; ++i) amax = fmaxf(amax, fabsf(c[i]));
    const Q8Scale qs = q8_scale(amax);
    uint32_t got_bits = 0;
    std::memcpy(&got_bits, &qs.scale, 4);
    CHECK(got_bits == scale_bits);
    float ss = 0.0f;
    double exact = 0.0;
    for (long i = 0; i < D; ++i) {
      const int8_t n = q8_code(c[i], qs.inv);
      CHECK(n >= -127 && n <= 127);
      if (n != want[i]) {
        std::printf("FAIL row %ld element %ld: code %d, reference %d\n", r, i, (int)n, want[i]);
        ++failures;
        break;
      }
      const float d = fmaf(-qs.scale, (float)n, c[i]);
      ss = fmaf(d, d, ss);
      const double dd = (double)c[i] - (double)qs.scale * (double)n;
      exact += dd * dd;
    }
    const float err = q8_err(sqrtf(ss), amax, qs.scale, (int)D);
    const double norm = std::sqrt(exact);
    CHECK(std::isfinite(err));
    CHECK((double)err >= norm);
    CHECK((double)err <= 1.01 * norm + 1e-7);
    if (amax == 0.0f) CHECK(err == 0.0f && qs.scale == 0.0f);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all checks passed (%ld rows)\n", rows);
  return 0;
}
