// Standalone perf probe for the cosine-topk kernel (no torch, no python).
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/knn_probe.hip -o gpurun_out/knn_probe
// Run:    ./knn_probe [B] [N] [iters]
// Times every kept kernel variant interleaved within one process and
// prints ms/iter and effective TFLOP/s of the score GEMM per variant.

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#include "../kakveda_amd/ops/hip/kernels_impl.h"

using namespace kakveda;

#define HIP_CHECK(x)                                                    \
  do {                                                                  \
    hipError_t e = (x);                                                 \
    if (e != hipSuccess) {                                              \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e),  \
              __FILE__, __LINE__);                                      \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

__global__ void fill_rand(bf16_t* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned h = (unsigned)(i * 2654435761u) ^ seed;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    const float f = ((float)(h & 0xFFFF) / 65536.0f - 0.5f) * 0.07217f; // ~unit rows
    p[i] = (bf16_t)f;
  }
}

using K128 = decltype(&cosine_topk_partial_t<11>);
using K8p = decltype(&cosine_topk_partial8p_t<1>);

// One probed variant: exactly one of k128 / k8p is set. A "warm" entry
// keeps rowthr from the entry before it (same data, so the thresholds have
// converged to the exact per-row k-th best): the ideal-threshold-warming
// ceiling. It must directly follow its cold twin.
struct Entry {
  const char* name;
  K128 k128;
  K8p k8p;
  bool warm;
};

static const Entry kTable[] = {
    {"fastbl128", cosine_topk_partial_t<11>, nullptr, false},
    {"fastblwarm128", cosine_topk_partial_t<11>, nullptr, true},
    {"fast128", cosine_topk_partial_t<9>, nullptr, false},
    {"full128", cosine_topk_partial_t<0>, nullptr, false},
    {"gemm128", cosine_topk_partial_t<1>, nullptr, false},
    {"argmax128", cosine_topk_partial_t<4>, nullptr, false},
    {"fastbl8p", nullptr, cosine_topk_partial8p_t<6>, false},
    {"gemm8p", nullptr, cosine_topk_partial8p_t<1>, false},
    {"gemm8plock", nullptr, cosine_topk_partial8p_t<16>, false},
};
constexpr int NE = sizeof(kTable) / sizeof(kTable[0]);

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 4096;
  const long N = argc > 2 ? atol(argv[2]) : 2000000;
  const int iters = argc > 3 ? atoi(argv[3]) : 10;
  const int D = 768;

  bf16_t *Q, *C;
  HIP_CHECK(hipMalloc(&Q, (size_t)B * D * 2));
  HIP_CHECK(hipMalloc(&C, (size_t)N * D * 2));
  hipLaunchKernelGGL(fill_rand, dim3(2048), dim3(256), 0, 0, Q, (size_t)B * D, 1u);
  hipLaunchKernelGGL(fill_rand, dim3(2048), dim3(256), 0, 0, C, (size_t)N * D, 2u);

  // same geometry as the extension's dispatch plan
  const Chunking c128 = chunking(B, (int)N, BM, default_target(BM));
  const Chunking c8p = chunking(B, (int)N, BM8, default_target(BM8));
  const int max_chunks = std::max(c128.nchunks, c8p.nchunks);

  float* pscore;
  int* pidx;
  unsigned* rowthr;
  HIP_CHECK(hipMalloc(&pscore, (size_t)B * max_chunks * KMAX * 4));
  HIP_CHECK(hipMalloc(&pidx, (size_t)B * max_chunks * KMAX * 4));
  HIP_CHECK(hipMalloc(&rowthr, (size_t)B * 4));

  auto run = [&](const Entry& e) {
    if (!e.warm)
      hipLaunchKernelGGL(init_rowthr, dim3((B + 255) / 256), dim3(256), 0, 0,
                         rowthr, B);
    if (e.k128)
      hipLaunchKernelGGL(e.k128, dim3(c128.nchunks, c128.row_tiles),
                         dim3(THREADS), 0, 0, Q, C, pscore, pidx, B, (int)N, D,
                         c128.chunk_tiles, c128.nchunks, rowthr,
                         (unsigned long long*)nullptr, (const int*)nullptr,
                         (const int*)nullptr);  // no label filter
    else
      hipLaunchKernelGGL(e.k8p, dim3(c8p.nchunks, c8p.row_tiles),
                         dim3(THREADS8), 0, 0, Q, C, pscore, pidx, B, (int)N, D,
                         c8p.chunk_tiles, c8p.nchunks, rowthr,
                         (unsigned long long*)nullptr, (float*)nullptr,
                         (unsigned long long*)nullptr, (unsigned*)nullptr, 0L,
                         (char*)nullptr, 0);  // from column tile 0
    hipError_t le = hipGetLastError();
    if (le != hipSuccess)
      fprintf(stderr, "launch error (%s): %s\n", e.name, hipGetErrorString(le));
  };

  for (const Entry& e : kTable) run(e);  // warm-up
  HIP_CHECK(hipDeviceSynchronize());

  std::vector<std::vector<float>> ms(NE);
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  for (int it = 0; it < iters; ++it) {
    for (int i = 0; i < NE; ++i) {
      HIP_CHECK(hipEventRecord(t0));
      run(kTable[i]);
      HIP_CHECK(hipEventRecord(t1));
      HIP_CHECK(hipEventSynchronize(t1));
      float x;
      HIP_CHECK(hipEventElapsedTime(&x, t0, t1));
      ms[i].push_back(x);
    }
  }
  for (int i = 0; i < NE; ++i) {
    std::sort(ms[i].begin(), ms[i].end());
    const float med = ms[i][ms[i].size() / 2];
    const double tf = 2.0 * B * (double)N * D / (med * 1e-3) / 1e12;
    printf("%-15s B=%d N=%ld med=%.3f ms min=%.3f  %.1f TF\n", kTable[i].name,
           B, N, med, ms[i][0], tf);
  }
  return 0;
}
