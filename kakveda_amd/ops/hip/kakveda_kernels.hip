// Torch extension bindings for the kakveda kernels (see kernels_impl.h).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <cstdlib>
#include <string>
#include <vector>
#include "kernels_impl.h"
#include "ivf_impl.h"
#include "ivf_batch_impl.h"
#include "featurize_impl.h"
#include "q8_impl.h"
#include "q8_screen_impl.h"
#include "knn_wide_impl.h"

using namespace kakveda;

static void check_bf16_2d(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), name, " must be contiguous 2-D");
}

namespace {

// The operands every search kernel takes.
struct KnnArgs {
  const bf16_t* q;
  const bf16_t* c;
  int B, N, D;
  hipStream_t stream;
  torch::Device dev;
  torch::TensorOptions f32() const { return torch::TensorOptions().dtype(torch::kFloat32).device(dev); }
  torch::TensorOptions i32() const { return torch::TensorOptions().dtype(torch::kInt32).device(dev); }
  torch::TensorOptions i64() const { return torch::TensorOptions().dtype(torch::kInt64).device(dev); }
};

KnnArgs knn_args(const torch::Tensor& queries, const torch::Tensor& corpus, int N) {
  return {(const bf16_t*)queries.data_ptr(), (const bf16_t*)corpus.data_ptr(),
          (int)queries.size(0), N, (int)queries.size(1),
          c10::hip::getCurrentHIPStream().stream(), queries.device()};
}

// ---- one launch site per kernel template ---------------------------------
using Partial128Fn = decltype(&cosine_topk_partial_t<11>);
Partial128Fn partial128_kernel(int mode) {
  switch (mode) {
    case 0: return cosine_topk_partial_t<0>;
    case 4: return cosine_topk_partial_t<4>;
    case 8: return cosine_topk_partial_t<8>;
    case 9: return cosine_topk_partial_t<9>;
    case 11: return cosine_topk_partial_t<11>;
  }
  TORCH_CHECK(false, "no 128x128 kernel for EPI_MODE ", mode);
}

// The label filter of a cosine_topk_filtered request (null/null: none).
// Every launch of one request gets the same Filter: thresholds published
// under one eligibility rule must not prune under another (kernels_impl.h).
struct Filter {
  const int* labels = nullptr;  // i32 [N]
  const int* want = nullptr;    // i32 [B]
  explicit operator bool() const { return labels != nullptr; }
};

void launch_partial128(int mode, dim3 grid, const KnnArgs& a, float* pscore,
                       int* pidx, int chunk_tiles, int stride, unsigned* rowthr,
                       Filter f = {}) {
  TORCH_CHECK(!f || mode == 11, "the filtered 128x128 kernel is EPI_MODE 11 only");
  const Partial128Fn filtered = cosine_topk_partial_t<11, true>;
  hipLaunchKernelGGL(f ? filtered : partial128_kernel(mode), grid,
                     dim3(THREADS), 0, a.stream, a.q, a.c, pscore, pidx,
                     a.B, a.N, a.D, chunk_tiles, stride, rowthr,
                     (unsigned long long*)nullptr, f.labels, f.want);
}

using Partial8pFn = decltype(&cosine_topk_partial8p_t<9>);
Partial8pFn partial8p_kernel(int mode) {
  switch (mode) {
    case 1: return cosine_topk_partial8p_t<1>;
    case 6: return cosine_topk_partial8p_t<6>;
    case 9: return cosine_topk_partial8p_t<9>;
    case 12: return cosine_topk_partial8p_t<12>;
    case 15: return cosine_topk_partial8p_t<15>;
    case 16: return cosine_topk_partial8p_t<16>;
  }
  TORCH_CHECK(false, "no 256x256 kernel for EPI_MODE ", mode);
}

// eseg/esegcnt/segcap are the emission epilogue's record segments (modes
// 9/15) and null/0 otherwise.
void launch_partial8p(int mode, dim3 grid, const KnnArgs& a, float* pscore,
                      int* pidx, int chunk_tiles, int nchunks, unsigned* rowthr,
                      unsigned long long* eseg, unsigned* esegcnt, long segcap,
                      int tile_first = 0) {
  hipLaunchKernelGGL(partial8p_kernel(mode), grid, dim3(THREADS8), 0, a.stream,
                     a.q, a.c, pscore, pidx, a.B, a.N, a.D, chunk_tiles, nchunks,
                     rowthr, (unsigned long long*)nullptr, (float*)nullptr, eseg,
                     esegcnt, segcap, (char*)nullptr, tile_first);
}

torch::Tensor new_rowthr(const KnnArgs& a) {
  auto rowthr = torch::empty({a.B}, a.i32());
  hipLaunchKernelGGL(init_rowthr, dim3((a.B + 255) / 256), dim3(256), 0,
                     a.stream, (unsigned*)rowthr.data_ptr<int>(), a.B);
  return rowthr;
}

// Emission floors: a prepass over the first pre_grid*pre_tiles column tiles
// (the plan's sample, in the launch geometry of knn_plan.h prepass_geometry)
// writes a COMPACT [B][pre_grid][KMAX] partial buffer of its own (so the floor
// merge scans only what the prepass produced); topk_merge folds it into the
// exact top-8 of the whole sampled column set, whose k-th (k <= KMAX, the
// caller's floor depth: KMAX in production, any k from the debug probes)
// is published as the per-row emission threshold (see
// publish_emission_floor): the k-th best of a subset lower-bounds the
// corpus k-th best just as the 8th does, and admits k/8 of the candidates.
struct Floors {
  torch::Tensor rowthr, samp_s, samp_i;
};

Floors run_emission_floors(const KnnArgs& a, int pre_grid, int pre_tiles,
                           int prepass_mode, int k, Filter flt = {}) {
  Floors f{new_rowthr(a), torch::empty({(long)a.B, (long)KMAX}, a.f32()),
           torch::empty({(long)a.B, (long)KMAX}, a.i64())};
  auto ppre_s = torch::empty({(long)a.B * pre_grid * KMAX}, a.f32());
  auto ppre_i = torch::empty({(long)a.B * pre_grid * KMAX}, a.i32());
  // the prepass always runs the 128-row-tile kernel, also under the
  // 256-row-tile 8p main launch
  launch_partial128(prepass_mode, dim3(pre_grid, (a.B + BM - 1) / BM), a,
                    ppre_s.data_ptr<float>(), ppre_i.data_ptr<int>(), pre_tiles,
                    pre_grid, (unsigned*)f.rowthr.data_ptr<int>(), flt);
  // (filtered: the sample lists hold eligible columns only, so the floor
  // published below is the k-th best ELIGIBLE sampled score; with fewer
  // than k eligible samples that slot is still -inf, nothing is published
  // and the main launch emits every eligible row)
  // block-per-row merge: the thread-per-row variant serial-scanned 2k
  // entries per thread (0.9 ms/step at preg=256)
  hipLaunchKernelGGL(topk_merge, dim3(a.B), dim3(THREADS), 0, a.stream,
                     ppre_s.data_ptr<float>(), ppre_i.data_ptr<int>(),
                     f.samp_s.data_ptr<float>(),
                     (long*)f.samp_i.data_ptr<int64_t>(), pre_grid, KMAX);
  hipLaunchKernelGGL(publish_emission_floor, dim3((a.B + 255) / 256), dim3(256),
                     0, a.stream, f.samp_s.data_ptr<float>(),
                     (unsigned*)f.rowthr.data_ptr<int>(), a.B,
                     std::min(k, KMAX) - 1);
  return f;
}

// Emission outputs: per-row candidate buffer + counts. The 8p main kernel
// (seg > 0) also gets one record segment and one record count per block
// (see kernels_impl.h EPI_MODE 9 and emit_bin); every block writes its
// count, so neither needs clearing. The candidate lists start empty, or,
// given the sample's top-KMAX (`seed`: the main launch will skip the sampled
// columns), hold exactly those: emit_seed then writes every count, in the
// place of the clearing memset.
struct EmitBufs {
  torch::Tensor cand, ccount, eseg, esegcnt;
};

EmitBufs new_emit_bufs(const KnnArgs& a, long cap, const Chunking& ch,
                       long seg = 0, const Floors* seed = nullptr) {
  EmitBufs e{torch::empty({(long)a.B, cap}, a.i64()),
             seed ? torch::empty({a.B}, a.i32()) : torch::zeros({a.B}, a.i32()),
             {}, {}};
  if (seed)
    hipLaunchKernelGGL(emit_seed, dim3((a.B + 255) / 256), dim3(256), 0,
                       a.stream, seed->samp_s.data_ptr<float>(),
                       (const long*)seed->samp_i.data_ptr<int64_t>(), a.B,
                       (unsigned long long*)e.cand.data_ptr<int64_t>(),
                       (unsigned*)e.ccount.data_ptr<int>(), cap);
  if (seg > 0) {
    const long blocks = (long)ch.nchunks * ch.row_tiles;
    e.eseg = torch::empty({blocks, seg}, a.i64());
    e.esegcnt = torch::empty({blocks}, a.i32());
  }
  return e;
}

// The 8p emission main launch and its binning step: afterwards cand/ccount
// hold what the per-row scatter of earlier versions left there (candidate
// order within a row apart, which emit_merge_topk does not depend on).
// `ch` chunks the column tiles from `tile_first` on; pscore/pidx need
// [B][ch.nchunks][KMAX] entries (padded chunks write -inf partials).
void launch_emit8p(int mode, const KnnArgs& a, const Chunking& ch,
                   torch::Tensor& pscore, torch::Tensor& pidx,
                   const torch::Tensor& rowthr, EmitBufs& e, long cap,
                   long seg, int tile_first = 0) {
  TORCH_CHECK(seg > 0 && ch.chunk_tiles <= 128,
              "emission segments need seg > 0 and chunk_tiles <= 128");
  TORCH_CHECK(pscore.numel() >= (long)a.B * ch.nchunks * KMAX &&
                  pidx.numel() >= (long)a.B * ch.nchunks * KMAX,
              "partial buffers are smaller than the main launch's chunks");
  unsigned long long* const eseg = (unsigned long long*)e.eseg.data_ptr<int64_t>();
  unsigned* const esegcnt = (unsigned*)e.esegcnt.data_ptr<int>();
  launch_partial8p(mode, dim3(ch.nchunks, ch.row_tiles), a,
                   pscore.data_ptr<float>(), pidx.data_ptr<int>(),
                   ch.chunk_tiles, ch.nchunks, (unsigned*)rowthr.data_ptr<int>(),
                   eseg, esegcnt, seg, tile_first);
  hipLaunchKernelGGL(emit_bin, dim3(ch.nchunks, ch.row_tiles), dim3(256), 0,
                     a.stream, (const unsigned long long*)eseg,
                     (const unsigned*)esegcnt, (int)seg, ch.chunk_tiles,
                     ch.nchunks, a.B, a.N,
                     (unsigned long long*)e.cand.data_ptr<int64_t>(),
                     (unsigned*)e.ccount.data_ptr<int>(), cap, tile_first);
}

std::tuple<torch::Tensor, torch::Tensor> cosine_topk_impl(
    const torch::Tensor& queries, const torch::Tensor& corpus, int k, int N,
    const KnnEnv& env, bool allow_emission, Filter flt = {}) {
  const KnnArgs a = knn_args(queries, corpus, N);
  const int B = a.B;
  const KnnPlan p = plan_cosine_topk(B, N, k, env, allow_emission, (bool)flt);
  TORCH_CHECK(plan_fits_grid(p, B), "cosine_topk: ", B,
              " query rows need more than ", MAX_GRID_Y, " row tiles of ",
              p.prepass ? BM : p.tile, " rows in one launch; split the batch");
  const Chunking& ch = p.ch;

  // [B][nchunks][KMAX] for whichever launch has more chunks (the emission
  // main launch over p.mch writes only its padded chunks' -inf partials)
  const long pslots = (long)B * std::max(ch.nchunks, p.mch.nchunks) * KMAX;
  auto pscore = torch::empty({pslots}, a.f32());
  auto pidx = torch::empty({pslots}, a.i32());
  auto out_score = torch::empty({B, k}, a.f32());
  auto out_idx = torch::empty({B, k}, a.i64());
  const dim3 grid(ch.nchunks, ch.row_tiles);

  if (p.merge == MergeKernel::Emit) {
    // candidates go to a per-row global buffer sized for ~8N/sample
    // expected emissions with ~25x headroom
    // Floor depth: the 8th best of the sample for every k. Publishing the
    // request's k-th best instead is as exact under the 8p main kernel
    // (its scores are bit-equal to the prepass kernel's) and cuts the
    // candidates to k/8, but measured +0.8..1.4% on the 10M bench, inside
    // the run-to-run band in two of three A/B sets, so it does not ship
    // (profiles/knn_kernel_history.md). The streaming kernels sum in another
    // order and may score the column that set the floor a few ulps lower;
    // they lower the floor they read by the rounding bound of unit rows
    // (kernels_impl.h streaming_floor), whatever the depth published here.
    const int floor_k = KMAX;
    const Floors f =
        p.prepass
            ? run_emission_floors(a, p.pre_grid, p.pre_tiles, p.prepass_mode,
                                  floor_k, flt)
            : Floors{new_rowthr(a), {}, {}};
    // The Emit8p main launch starts after the sampled columns
    // (p.skip_tiles, knn_plan.h main_geometry): the sample's top-KMAX are
    // seeded into the candidate lists in their place.
    const bool seeded = p.skip_tiles > 0;
    EmitBufs e = new_emit_bufs(a, p.cap, p.mch, p.mseg, seeded ? &f : nullptr);
    if (p.main == MainKernel::SmallB && flt) {
      hipLaunchKernelGGL(smallb_emit_kernel_v4<true>, dim3(p.smallb_blocks),
                         dim3(256), (size_t)B * a.D * 2, a.stream, a.q, a.c, B,
                         (long)N, a.D, (const unsigned*)f.rowthr.data_ptr<int>(),
                         (unsigned long long*)e.cand.data_ptr<int64_t>(),
                         (unsigned*)e.ccount.data_ptr<int>(), p.cap, flt.labels,
                         flt.want);
    } else if (p.main == MainKernel::SmallB) {
      // Default: the v4 8-lanes-per-row remap (same-box A/B at 10M:
      // +1.5% at B=1, +13.6% at B=4, exact parity — see
      // profiles/knn_kernel_history.md). KAKVEDA_SMALLB=2 reverts to the
      // per-lane-row streaming kernel (v2).
      if (p.mode == 2)
        hipLaunchKernelGGL(smallb_emit_kernel, dim3(p.smallb_blocks), dim3(256),
                           (size_t)B * a.D * 2, a.stream, a.q, a.c, B, (long)N,
                           a.D, (const unsigned*)f.rowthr.data_ptr<int>(),
                           (unsigned long long*)e.cand.data_ptr<int64_t>(),
                           (unsigned*)e.ccount.data_ptr<int>(), p.cap);
      else
        hipLaunchKernelGGL(smallb_emit_kernel_v4<false>, dim3(p.smallb_blocks),
                           dim3(256), (size_t)B * a.D * 2, a.stream, a.q, a.c,
                           B, (long)N, a.D,
                           (const unsigned*)f.rowthr.data_ptr<int>(),
                           (unsigned long long*)e.cand.data_ptr<int64_t>(),
                           (unsigned*)e.ccount.data_ptr<int>(), p.cap,
                           (const int*)nullptr, (const int*)nullptr);
    } else {
      launch_emit8p(p.mode, a, p.mch, pscore, pidx, f.rowthr, e, p.cap, p.mseg,
                    p.skip_tiles);
    }
    hipLaunchKernelGGL(emit_merge_topk, dim3(B), dim3(256), 0, a.stream,
                       (const unsigned long long*)e.cand.data_ptr<int64_t>(),
                       (const unsigned*)e.ccount.data_ptr<int>(),
                       out_score.data_ptr<float>(),
                       (long*)out_idx.data_ptr<int64_t>(), B, p.cap, k);
    // exactness guard (statistically never taken with prepass floors):
    // an overflowed row means emission skipped stores — rerun the whole
    // batch through the list-epilogue production kernel
    const long mx = (long)e.ccount.max().item<int>();
    if (env.emit_debug) {
      printf("emit: rows=%d max=%ld mean=%.1f cap=%ld%s\n", B, mx,
             e.ccount.to(torch::kFloat32).mean().item<float>(), p.cap,
             mx > p.cap ? "  FALLBACK" : "");
      if (p.prepass)
        printf("emit: prepass pre_grid=%d pre_tiles=%d\n", p.pre_grid,
               p.pre_tiles);
      if (p.mseg > 0)
        printf("emit: segments=%ld max=%d seg=%ld skip_tiles=%d\n",
               (long)e.esegcnt.size(0), e.esegcnt.max().item<int>(), p.mseg,
               p.skip_tiles);
    }
    if (mx > p.cap) {
      static bool warned = false;
      if (!warned) {
        warned = true;
        fprintf(stderr,
                "[kakveda] emission candidate overflow (max=%ld > cap=%ld) — "
                "falling back to the list-epilogue kernel for this batch\n",
                mx, p.cap);
      }
      return cosine_topk_impl(queries, corpus, k, N, env, false, flt);
    }
    return {out_score, out_idx};
  }

  auto rowthr = new_rowthr(a);
  unsigned* const thr = (unsigned*)rowthr.data_ptr<int>();
  // Threshold pre-pass: one cheap launch over the first PRE_TILES*preg
  // column tiles fills each row's lists from a ~4k-column sample and
  // publishes their minima into rowthr, so the main launch's blocks all
  // start with near-converged pruning thresholds instead of each paying
  // the bootstrap insert storm (measured: warm thresholds are worth
  // ~10% end-to-end; the sample scan is ~0.5% extra work, its partial
  // writes land in slots the main launch overwrites). Because they are
  // overwritten, the thresholds they backed must not prune equal scores:
  // relax_rowthr lowers each strictly below its value before the main launch.
  if (p.prepass) {
    launch_partial128(p.prepass_mode, dim3(p.preg, (B + BM - 1) / BM), a,
                      pscore.data_ptr<float>(), pidx.data_ptr<int>(), PRE_TILES,
                      ch.nchunks, thr, flt);
    hipLaunchKernelGGL(relax_rowthr, dim3((B + 255) / 256), dim3(256), 0,
                       a.stream, thr, B);
  }
  if (p.main == MainKernel::Stash8p)
    launch_partial8p(p.mode, grid, a, pscore.data_ptr<float>(),
                     pidx.data_ptr<int>(), ch.chunk_tiles, ch.nchunks, thr,
                     nullptr, nullptr, 0);
  else  // List128, or Argmax128 (k=1: per-row max, no thresholds)
    launch_partial128(p.mode, grid, a, pscore.data_ptr<float>(),
                      pidx.data_ptr<int>(), ch.chunk_tiles, ch.nchunks,
                      p.main == MainKernel::Argmax128 ? nullptr : thr, flt);
  if (p.merge == MergeKernel::Small)
    hipLaunchKernelGGL(topk_merge_small, dim3((B + 255) / 256), dim3(256), 0,
                       a.stream, pscore.data_ptr<float>(), pidx.data_ptr<int>(),
                       out_score.data_ptr<float>(),
                       (long*)out_idx.data_ptr<int64_t>(), B, ch.nchunks, k);
  else
    hipLaunchKernelGGL(topk_merge, dim3(B), dim3(THREADS), 0, a.stream,
                       pscore.data_ptr<float>(), pidx.data_ptr<int>(),
                       out_score.data_ptr<float>(),
                       (long*)out_idx.data_ptr<int64_t>(), ch.nchunks, k);
  return {out_score, out_idx};
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor> cosine_topk(
    torch::Tensor queries, torch::Tensor corpus, int64_t k, int64_t valid_n) {
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const int D = queries.size(1);
  const int N = (int)valid_n;
  TORCH_CHECK(corpus.size(1) == D, "dim mismatch");
  TORCH_CHECK(N >= 1 && N <= corpus.size(0), "valid_n out of range");
  TORCH_CHECK(D % BK == 0, "D must be a multiple of ", BK);
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  // parse -> plan -> allocate -> launch. The KAKVEDA_KNN_* environment is
  // read once per process; an unrecognised selection throws here, before
  // anything is launched (knn_plan.h).
  static const KnnEnv env = parse_knn_env(std::getenv);
  return cosine_topk_impl(queries, corpus, (int)k, N, env, true);
}

std::tuple<torch::Tensor, torch::Tensor> cosine_topk_filtered(
    torch::Tensor queries, torch::Tensor corpus, torch::Tensor labels,
    torch::Tensor want, int64_t k, int64_t valid_n) {
  // cosine_topk restricted, per query row b, to the corpus rows j with
  // want[b] < 0 || labels[j] == want[b]. Rows short of k eligible corpus
  // rows come back padded with the kernels' (-1e30 or -inf, -1) sentinels,
  // which the Python op normalises.
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const int D = queries.size(1);
  const int N = (int)valid_n;
  TORCH_CHECK(corpus.size(1) == D, "dim mismatch");
  TORCH_CHECK(N >= 1 && N <= corpus.size(0), "valid_n out of range");
  TORCH_CHECK(D % BK == 0, "D must be a multiple of ", BK);
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  TORCH_CHECK(labels.is_cuda() && labels.device() == corpus.device() &&
                  labels.scalar_type() == torch::kInt32 && labels.dim() == 1 &&
                  labels.is_contiguous() && labels.size(0) >= N,
              "labels must be contiguous 1-D i32 on the corpus device with at "
              "least valid_n entries");
  TORCH_CHECK(want.is_cuda() && want.device() == queries.device() &&
                  want.scalar_type() == torch::kInt32 && want.dim() == 1 &&
                  want.is_contiguous() && want.size(0) == queries.size(0),
              "want must be contiguous 1-D i32 on the query device with one "
              "entry per query row");
  static const KnnEnv env = parse_knn_env(std::getenv);
  return cosine_topk_impl(queries, corpus, (int)k, N, env, true,
                          Filter{labels.data_ptr<int>(), want.data_ptr<int>()});
}

// ---------------------------------------------------------------------------
// Wide exact search, KMAX < k <= KWIDE_MAX (knn_wide_plan.h, knn_wide_impl.h)
// ---------------------------------------------------------------------------
namespace {

struct WidePass {
  torch::Tensor cand, ccount;  // i64 [B, cap], i32 [B]
};

// Floors and emission of one pass over the a.N corpus rows at a.c: afterwards
// cand / ccount hold, per query, every eligible row scoring at least the
// query's wide floor (every eligible row where it has none).
WidePass run_wide_pass(const KnnArgs& a, const WidePlan& p, Filter flt) {
  // A fresh threshold array that only ever holds the wide floor: the prepass
  // below gets none (its 8-deep list minima bound the 8th best, not the k-th).
  auto rowthr = new_rowthr(a);
  unsigned* const thr = (unsigned*)rowthr.data_ptr<int>();
  if (p.prepass) {
    const long entries = (long)p.pre_grid * KMAX;
    auto ppre_s = torch::empty({(long)a.B * entries}, a.f32());
    auto ppre_i = torch::empty({(long)a.B * entries}, a.i32());
    launch_partial128(11, dim3(p.pre_grid, (a.B + BM - 1) / BM), a,
                      ppre_s.data_ptr<float>(), ppre_i.data_ptr<int>(),
                      p.pre_tiles, p.pre_grid, nullptr, flt);
    hipLaunchKernelGGL(wide_floor_kernel, dim3(a.B), dim3(WSEL_THREADS), 0,
                       a.stream, (const float*)ppre_s.data_ptr<float>(),
                       (const int*)ppre_i.data_ptr<int>(), (int)entries, p.k, thr);
  }
  WidePass w{torch::empty({(long)a.B, p.cap}, a.i64()),
             torch::zeros({(long)a.B}, a.i32())};
  unsigned long long* const cand = (unsigned long long*)w.cand.data_ptr<int64_t>();
  unsigned* const ccount = (unsigned*)w.ccount.data_ptr<int>();
  if (p.main == WideMain::Emit8p) {
    EmitBufs e{w.cand, w.ccount, {}, {}};
    const long blocks = (long)p.ch.nchunks * p.ch.row_tiles;
    e.eseg = torch::empty({blocks, p.seg}, a.i64());
    e.esegcnt = torch::empty({blocks}, a.i32());
    auto pscore = torch::empty({(long)a.B * p.ch.nchunks * KMAX}, a.f32());
    auto pidx = torch::empty({(long)a.B * p.ch.nchunks * KMAX}, a.i32());
    launch_emit8p(9, a, p.ch, pscore, pidx, rowthr, e, p.cap, p.seg);
    return w;
  }
  const auto kernel = flt ? smallb_emit_kernel_v4<true> : smallb_emit_kernel_v4<false>;
  for (int g = 0; g < p.groups; ++g) {
    const WideSpan s = wide_group(a.B, g);
    hipLaunchKernelGGL(kernel, dim3(p.smallb_blocks), dim3(256),
                       (size_t)s.count * a.D * 2, a.stream, a.q + s.first * a.D,
                       a.c, (int)s.count, (long)a.N, a.D,
                       (const unsigned*)thr + s.first, cand + s.first * p.cap,
                       ccount + s.first, p.cap, flt.labels,
                       flt ? flt.want + s.first : nullptr);
  }
  return w;
}

struct WideResult {
  torch::Tensor scores, idx, counts;
  int64_t fallback;
};

WideResult cosine_topk_wide_impl(const torch::Tensor& queries,
                                 const torch::Tensor& corpus, int64_t k,
                                 int64_t valid_n,
                                 const c10::optional<torch::Tensor>& labels,
                                 const c10::optional<torch::Tensor>& want,
                                 int64_t cap, int64_t seg) {
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const int D = queries.size(1);
  const int N = (int)valid_n;
  TORCH_CHECK(corpus.size(1) == D, "dim mismatch");
  TORCH_CHECK(valid_n >= 1 && valid_n <= corpus.size(0) && valid_n <= 0x7fffffffL,
              "valid_n out of range");
  TORCH_CHECK(D % BK == 0, "D must be a multiple of ", BK);
  TORCH_CHECK(k >= 1 && k <= KWIDE_MAX, "k must be in [1,", KWIDE_MAX, "]");
  TORCH_CHECK(cap >= 0 && cap <= (1L << 24) && seg >= 0, "cap or seg out of range");
  TORCH_CHECK((size_t)WIDE_GROUP * D * 2 <= 64 * 1024, "cosine_topk_wide: ",
              WIDE_GROUP, " queries of D = ", D,
              " do not fit the streaming kernel's 64 KiB of LDS");
  TORCH_CHECK(queries.size(0) >= 1 &&
                  (queries.size(0) + BM - 1) / BM <= MAX_GRID_Y,
              "cosine_topk_wide: split the batch");
  TORCH_CHECK(labels.has_value() == want.has_value(), "labels and want go together");
  Filter flt;
  if (labels) {
    const torch::Tensor& l = *labels;
    const torch::Tensor& w = *want;
    TORCH_CHECK(l.is_cuda() && l.device() == corpus.device() &&
                    l.scalar_type() == torch::kInt32 && l.dim() == 1 &&
                    l.is_contiguous() && l.size(0) >= N,
                "labels must be contiguous 1-D i32 on the corpus device with at "
                "least valid_n entries");
    TORCH_CHECK(w.is_cuda() && w.device() == queries.device() &&
                    w.scalar_type() == torch::kInt32 && w.dim() == 1 &&
                    w.is_contiguous() && w.size(0) == queries.size(0),
                "want must be contiguous 1-D i32 on the query device with one "
                "entry per query row");
    flt = Filter{l.data_ptr<int>(), w.data_ptr<int>()};
  }
  static const KnnEnv env = parse_knn_env(std::getenv);
  const KnnArgs a = knn_args(queries, corpus, N);
  const long ccap = cap > 0 ? cap : std::max(1L, env.cap);
  const WidePlan p = plan_wide(a.B, N, k, (bool)flt, ccap, seg > 0 ? seg : env.seg,
                               env.target, false);
  const int kk = p.k;
  WidePass w = run_wide_pass(a, p, flt);
  auto out_score = torch::empty({(long)a.B, (long)kk}, a.f32());
  auto out_idx = torch::empty({(long)a.B, (long)kk}, a.i64());
  hipLaunchKernelGGL(emit_merge_topk_wide<false>, dim3(a.B), dim3(WSEL_THREADS), 0,
                     a.stream, (const unsigned long long*)w.cand.data_ptr<int64_t>(),
                     (const unsigned*)w.ccount.data_ptr<int>(), p.cap, 0u, kk,
                     out_score.data_ptr<float>(), (long*)out_idx.data_ptr<int64_t>(),
                     (unsigned long long*)nullptr, 0L, 0L, 0u);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  // the one readback: a count past cap is a row that lost candidates or a
  // poisoned record segment (emit_bin)
  const long mx = (long)w.ccount.max().item<int>();
  if (env.emit_debug)
    printf("wide: rows=%d k=%d max=%ld mean=%.1f cap=%ld seg=%ld main=%d%s\n", a.B,
           kk, mx, w.ccount.to(torch::kFloat32).mean().item<float>(), p.cap, p.seg,
           (int)p.main, mx > p.cap ? "  FALLBACK" : "");
  if (mx <= p.cap) return {out_score, out_idx, w.ccount, 0};

  static bool warned = false;
  if (!warned) {
    warned = true;
    fprintf(stderr,
            "[kakveda] wide top-k candidate overflow (max=%ld > cap=%ld): "
            "answering this batch over corpus slices of %ld rows\n",
            mx, p.cap, p.cap);
  }
  // Sliced fallback: each slice of at most cap rows through the same
  // pipeline (streaming kernel: no segments, at most its rows emitted), its
  // top k kept as packed words with corpus-wide columns; then one selection
  // across the slices.
  const long slices = wide_slice_count(N, p.cap);
  auto packed = torch::empty({(long)a.B, slices * kk}, a.i64());
  for (long s = 0; s < slices; ++s) {
    const WideSpan sl = wide_slice(N, p.cap, s);
    KnnArgs as = a;
    as.c = a.c + sl.first * (long)D;
    as.N = (int)sl.count;
    Filter fs = flt;
    if (fs) fs.labels = flt.labels + sl.first;
    const WidePlan ps =
        plan_wide(a.B, as.N, kk, (bool)flt, p.cap, 0, env.target, true);
    WidePass ws = run_wide_pass(as, ps, fs);
    hipLaunchKernelGGL(emit_merge_topk_wide<true>, dim3(a.B), dim3(WSEL_THREADS), 0,
                       a.stream,
                       (const unsigned long long*)ws.cand.data_ptr<int64_t>(),
                       (const unsigned*)ws.ccount.data_ptr<int>(), p.cap, 0u, kk,
                       (float*)nullptr, (long*)nullptr,
                       (unsigned long long*)packed.data_ptr<int64_t>(), slices * kk,
                       s * kk, (unsigned)sl.first);
  }
  hipLaunchKernelGGL(emit_merge_topk_wide<false>, dim3(a.B), dim3(WSEL_THREADS), 0,
                     a.stream, (const unsigned long long*)packed.data_ptr<int64_t>(),
                     (const unsigned*)nullptr, slices * kk, (unsigned)(slices * kk),
                     kk, out_score.data_ptr<float>(),
                     (long*)out_idx.data_ptr<int64_t>(),
                     (unsigned long long*)nullptr, 0L, 0L, 0u);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {out_score, out_idx, w.ccount, 1};
}

}  // namespace

// Exact top-k for k up to KWIDE_MAX: (scores f32 [B, k], idx i64 [B, k],
// fallback). labels / want restrict it as cosine_topk_filtered does. cap > 0
// overrides the candidates per query (KAKVEDA_KNN_EMIT_CAP otherwise), seg > 0
// the records per block segment of the 8-phase launch. fallback is 1 when the
// candidates overflowed and the batch was answered slice by slice.
std::tuple<torch::Tensor, torch::Tensor, int64_t> cosine_topk_wide(
    torch::Tensor queries, torch::Tensor corpus, int64_t k, int64_t valid_n,
    c10::optional<torch::Tensor> labels, c10::optional<torch::Tensor> want,
    int64_t cap, int64_t seg) {
  WideResult r =
      cosine_topk_wide_impl(queries, corpus, k, valid_n, labels, want, cap, seg);
  return {r.scores, r.idx, r.fallback};
}

// Benchmark probe: the same request, returning the candidates per query of
// its first pass as well: (scores, idx, fallback, counts i32 [B]).
std::tuple<torch::Tensor, torch::Tensor, int64_t, torch::Tensor> wide_counts_probe(
    torch::Tensor queries, torch::Tensor corpus, int64_t k, int64_t valid_n,
    c10::optional<torch::Tensor> labels, c10::optional<torch::Tensor> want,
    int64_t cap, int64_t seg) {
  WideResult r =
      cosine_topk_wide_impl(queries, corpus, k, valid_n, labels, want, cap, seg);
  return {r.scores, r.idx, r.fallback, r.counts};
}

// ---------------------------------------------------------------------------
// int8 row mirror (q8_plan.h, q8_impl.h)
// ---------------------------------------------------------------------------
namespace {

void check_q8_mirror(const torch::Tensor& codes, const torch::Tensor& meta,
                     const torch::Device& dev, int64_t rows, int64_t D) {
  TORCH_CHECK(q8_dim_ok(D), "the int8 mirror needs D to be a multiple of ",
              Q8_SEG, " (below 2^20), got D = ", D);
  TORCH_CHECK(codes.is_cuda() && codes.device() == dev &&
                  codes.scalar_type() == torch::kInt8 && codes.dim() == 2 &&
                  codes.is_contiguous() && codes.size(1) == D &&
                  codes.size(0) >= rows,
              "codes must be contiguous int8 [>= ", rows, ", ", D,
              "] on the rows' device");
  TORCH_CHECK(meta.is_cuda() && meta.device() == dev &&
                  meta.scalar_type() == torch::kFloat32 && meta.dim() == 2 &&
                  meta.is_contiguous() && meta.size(1) == 2 &&
                  meta.size(0) >= rows,
              "meta must be contiguous fp32 [>= ", rows, ", 2] on the rows' device");
}

void check_q8_cnorm(const torch::Tensor& cnorm, const torch::Device& dev) {
  TORCH_CHECK(cnorm.is_cuda() && cnorm.device() == dev &&
                  cnorm.scalar_type() == torch::kFloat32 && cnorm.numel() == 1 &&
                  cnorm.is_contiguous(),
              "cnorm must be one fp32 value on the rows' device");
}

// Stage 1 of the q8 search into e.cand / e.ccount.
void launch_q8_emit(const KnnArgs& a, const KnnPlan& p, const torch::Tensor& codes,
                    const torch::Tensor& meta, const Floors& f, EmitBufs& e,
                    Filter flt) {
  const size_t lds = (size_t)a.B * a.D * sizeof(float);
  TORCH_CHECK(lds <= 64 * 1024, "cosine_topk_q8: ", a.B, " fp32 queries of D = ",
              a.D, " do not fit the kernel's 64 KiB of LDS");
  const auto kernel = flt ? q8_emit_kernel<true> : q8_emit_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(p.smallb_blocks), dim3(256), lds, a.stream,
                     a.q, (const signed char*)codes.data_ptr<int8_t>(),
                     meta.data_ptr<float>(), a.B, (long)a.N, a.D,
                     (const unsigned*)f.rowthr.data_ptr<int>(),
                     (unsigned long long*)e.cand.data_ptr<int64_t>(),
                     (unsigned*)e.ccount.data_ptr<int>(), p.cap, flt.labels,
                     flt.want);
}

struct Q8Checked {
  int N;
  Filter flt;
};

Q8Checked check_q8_search(const torch::Tensor& queries, const torch::Tensor& corpus,
                          const torch::Tensor& codes, const torch::Tensor& meta,
                          int64_t k, int64_t valid_n,
                          const c10::optional<torch::Tensor>& labels,
                          const c10::optional<torch::Tensor>& want) {
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const int D = queries.size(1);
  const int N = (int)valid_n;
  TORCH_CHECK(corpus.size(1) == D, "dim mismatch");
  TORCH_CHECK(N >= 1 && N <= corpus.size(0), "valid_n out of range");
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  check_q8_mirror(codes, meta, corpus.device(), N, D);
  TORCH_CHECK(labels.has_value() == want.has_value(),
              "labels and want go together");
  Filter flt;
  if (labels) {
    const torch::Tensor& l = *labels;
    const torch::Tensor& w = *want;
    TORCH_CHECK(l.is_cuda() && l.device() == corpus.device() &&
                    l.scalar_type() == torch::kInt32 && l.dim() == 1 &&
                    l.is_contiguous() && l.size(0) >= N,
                "labels must be contiguous 1-D i32 on the corpus device with at "
                "least valid_n entries");
    TORCH_CHECK(w.is_cuda() && w.device() == queries.device() &&
                    w.scalar_type() == torch::kInt32 && w.dim() == 1 &&
                    w.is_contiguous() && w.size(0) == queries.size(0),
                "want must be contiguous 1-D i32 on the query device with one "
                "entry per query row");
    flt = Filter{l.data_ptr<int>(), w.data_ptr<int>()};
  }
  return {N, flt};
}

}  // namespace

void quantize_rows_q8(torch::Tensor rows, torch::Tensor out_codes,
                      torch::Tensor out_meta, int64_t first_row,
                      c10::optional<torch::Tensor> cnorm) {
  check_bf16_2d(rows, "rows");
  const int64_t n = rows.size(0), D = rows.size(1);
  TORCH_CHECK(first_row >= 0, "first_row must be >= 0");
  check_q8_mirror(out_codes, out_meta, rows.device(), first_row + n, D);
  if (cnorm) check_q8_cnorm(*cnorm, rows.device());
  if (n == 0) return;
  const int blocks = (int)std::min((n + 31) / 32, (int64_t)8192);
  hipLaunchKernelGGL(q8_quantize_kernel, dim3(blocks), dim3(256), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     (const bf16_t*)rows.data_ptr(), (long)n, (int)D,
                     (signed char*)out_codes.data_ptr<int8_t>(),
                     out_meta.data_ptr<float>(), (long)first_row);
  // the segment's cnorm (q8_plan.h): raised to the largest norm of these rows
  if (cnorm)
    hipLaunchKernelGGL(q8_cnorm_kernel, dim3(blocks), dim3(256), 0,
                       c10::hip::getCurrentHIPStream().stream(),
                       (const bf16_t*)rows.data_ptr(), (long)n, (int)D,
                       cnorm->data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

namespace {

// The batched int8 screen (q8_screen_impl.h) up to and including the rescore:
// quantise the queries, the unchanged floors and seeds, T_r and kappa, then
// per stage of the plan (knn_plan.h plan_q8_stages) the screen over the
// stage's codes, emit_bin and the bf16 scores of every entry the stage
// emitted, and between two stages the floor refresh (emit_merge_topk into a
// scratch top-k, q8_refresh_floor). Everything runs on the one stream with no
// host synchronisation; a stage's record segments are consumed by its
// emit_bin before the next stage writes them. Afterwards e.cand / e.ccount
// hold every column of the exact top-k (q8_plan.h "Staged floors"), all with
// bf16 scores; with one stage, exactly what the bf16 emission launch leaves
// there plus the screen's false positives.
struct Q8Screen {
  EmitBufs e;
  torch::Tensor first;      // i32 [B]: entries seeded before the screen
  torch::Tensor thrT;       // f32 [B]: T_r (of the last stage)
  torch::Tensor small;      // i32 [2]: bits of kappa, degenerate rows
  torch::Tensor rowthr;     // u32 [B]: the floors, order-encoded (one stage:
                            // the prepass floors)
  torch::Tensor before;     // the candidate buffer ahead of the rescore (probe)
  long cap, seg;
  StagePlan sp;
};

// The stage plan of a request. The boundary search of plan_q8_stages costs a
// few hundred chunkings; a serving process asks for the same few shapes over
// and over, so the last plan is kept per thread.
StagePlan q8_stage_plan(const KnnArgs& a, const KnnPlan& p, const KnnEnv& env,
                        int k, int64_t stages) {
  TORCH_CHECK(stages >= 0 && stages <= Q8_MAX_STAGES,
              "stages must be in [1,", Q8_MAX_STAGES, "], or 0 for the plan's rule");
  const int want = stages > 0 ? (int)stages : env.q8_stages;
  struct Key {
    int B, N, k, want;
  };
  thread_local Key key{-1, -1, -1, -1};
  thread_local StagePlan memo;
  if (key.B != a.B || key.N != a.N || key.k != k || key.want != want) {
    memo = plan_q8_stages(p, env, want);
    key = Key{a.B, a.N, k, want};
  }
  return memo;
}

Q8Screen run_q8_screen(const KnnArgs& a, const KnnPlan& p, const KnnEnv& env,
                       const torch::Tensor& codes, const torch::Tensor& meta,
                       const torch::Tensor& cnorm, long cap_override,
                       bool keep_before, int k, int64_t stages) {
  const auto i8 = torch::TensorOptions().dtype(torch::kInt8).device(a.dev);
  auto qcodes = torch::empty({(long)a.B, (long)a.D}, i8);
  auto qmeta = torch::empty({(long)a.B, 2L}, a.f32());
  hipLaunchKernelGGL(q8_quantize_kernel, dim3((a.B + 31) / 32), dim3(256), 0,
                     a.stream, a.q, (long)a.B, a.D,
                     (signed char*)qcodes.data_ptr<int8_t>(),
                     qmeta.data_ptr<float>(), 0L);
  const Floors f = run_emission_floors(a, p.pre_grid, p.pre_tiles,
                                       p.prepass_mode, KMAX);
  Q8Screen s;
  s.sp = q8_stage_plan(a, p, env, k, stages);
  const StagePlan& sp = s.sp;
  s.rowthr = f.rowthr;
  s.cap = cap_override > 0 ? cap_override : p.cap;
  // one set of record segments, for the stage with the most blocks
  Chunking widest = sp.ch[0];
  for (int i = 1; i < sp.n; ++i)
    if (sp.ch[i].nchunks > widest.nchunks) widest = sp.ch[i];
  s.seg = emit_seg_cap(a.B, s.cap, widest, env.seg);
  s.thrT = torch::empty({(long)a.B}, a.f32());
  s.small = torch::zeros({2L}, a.i32());
  hipLaunchKernelGGL(q8_screen_prep, dim3((a.B + 3) / 4), dim3(256), 0, a.stream,
                     (const signed char*)qcodes.data_ptr<int8_t>(),
                     (const float*)qmeta.data_ptr<float>(),
                     (const unsigned*)f.rowthr.data_ptr<int>(),
                     (const float*)cnorm.data_ptr<float>(), a.B, a.D,
                     s.thrT.data_ptr<float>(), (float*)s.small.data_ptr<int>(),
                     s.small.data_ptr<int>() + 1);
  const bool seeded = p.skip_tiles > 0;
  s.e = new_emit_bufs(a, s.cap, widest, s.seg, seeded ? &f : nullptr);
  // firsts[i]: the rows' counts ahead of stage i (row 0: the seeds)
  auto firsts = torch::empty({(long)sp.n, (long)a.B}, a.i32());
  s.first = firsts[0];
  torch::Tensor best_s, best_i;
  if (sp.n > 1) {
    best_s = torch::empty({(long)a.B, (long)k}, a.f32());
    best_i = torch::empty({(long)a.B, (long)k}, a.i64());
  }
  unsigned long long* const eseg = (unsigned long long*)s.e.eseg.data_ptr<int64_t>();
  unsigned* const esegcnt = (unsigned*)s.e.esegcnt.data_ptr<int>();
  unsigned long long* const cand = (unsigned long long*)s.e.cand.data_ptr<int64_t>();
  unsigned* const ccount = (unsigned*)s.e.ccount.data_ptr<int>();
  for (int i = 0; i < sp.n; ++i) {
    const Chunking& ch = sp.ch[i];
    unsigned* const first = (unsigned*)firsts[i].data_ptr<int>();
    C10_HIP_CHECK(hipMemcpyAsync(first, ccount, (size_t)a.B * sizeof(unsigned),
                                 hipMemcpyDeviceToDevice, a.stream));
    // the stage ends where the next begins: the kernel clamps its loads to
    // n_end - 1 and drops columns at or past n_end, as it does at the corpus end
    const int n_end = (int)std::min((long)a.N, (long)sp.first[i + 1] * BN8);
    const dim3 grid(ch.nchunks, ch.row_tiles);
    hipLaunchKernelGGL(cosine_topk_screen8p_i8<true>, grid, dim3(THREADS8), 0,
                       a.stream, (const signed char*)qcodes.data_ptr<int8_t>(),
                       (const signed char*)codes.data_ptr<int8_t>(),
                       (const float*)meta.data_ptr<float>(),
                       (const float*)s.thrT.data_ptr<float>(),
                       (const float*)s.small.data_ptr<int>(), a.B, n_end, a.D,
                       ch.chunk_tiles, ch.nchunks, eseg, esegcnt, s.seg,
                       sp.first[i]);
    hipLaunchKernelGGL(emit_bin, grid, dim3(256), 0, a.stream,
                       (const unsigned long long*)eseg, (const unsigned*)esegcnt,
                       (int)s.seg, ch.chunk_tiles, ch.nchunks, a.B, n_end, cand,
                       ccount, s.cap, sp.first[i]);
    if (keep_before && i == 0) s.before = s.e.cand.clone();
    hipLaunchKernelGGL(q8_rescore_mfma, dim3(8, a.B), dim3(256), 0, a.stream, a.q,
                       a.c, a.N, a.D, cand, (const unsigned*)ccount,
                       (const unsigned*)first, s.cap);
    if (env.emit_debug)
      printf("q8 screen: stage %d/%d tiles [%d, %d) chunks=%d x %d tiles "
             "segments max=%d mean/row=%.1f\n",
             i + 1, sp.n, sp.first[i], sp.first[i + 1], ch.nchunks,
             ch.chunk_tiles,
             s.e.esegcnt.slice(0, 0, (long)ch.nchunks * ch.row_tiles)
                 .max().item<int>(),
             (s.e.ccount - firsts[i]).to(torch::kFloat32).mean().item<float>());
    if (i + 1 == sp.n) break;
    hipLaunchKernelGGL(emit_merge_topk, dim3(a.B), dim3(256), 0, a.stream,
                       (const unsigned long long*)cand, (const unsigned*)ccount,
                       best_s.data_ptr<float>(),
                       (long*)best_i.data_ptr<int64_t>(), a.B, s.cap, k);
    hipLaunchKernelGGL(q8_refresh_floor, dim3((a.B + 255) / 256), dim3(256), 0,
                       a.stream, (const float*)best_s.data_ptr<float>(), k,
                       (const float*)qmeta.data_ptr<float>(),
                       (const float*)cnorm.data_ptr<float>(), a.B, a.D,
                       (unsigned*)s.rowthr.data_ptr<int>(),
                       s.thrT.data_ptr<float>());
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return s;
}

// Whether the request is the batched int8 screen's: the unfiltered 8-phase
// emission plan, at least min_b queries, a D the screen takes, and not
// switched off (KAKVEDA_Q8_BATCH=0; min_b <= 0: the caller does not want it).
bool q8_screen_in_plan(const KnnArgs& a, const KnnPlan& p, const KnnEnv& env,
                       bool filtered, int64_t min_b) {
  return !filtered && env.q8_batch && min_b > 0 && a.B >= min_b &&
         p.main == MainKernel::Emit8p && p.merge == MergeKernel::Emit &&
         p.prepass && q8_screen_dim_ok(a.D) && p.mch.chunk_tiles <= 128;
}

}  // namespace

// The two-stage exact search over the mirror. Where the plan of the request
// selects the streaming small-batch kernel, stage 1 scans the int8 codes
// (q8_emit_kernel), stage 2 rescores the candidates from the bf16 rows
// (q8_rescore), and the existing merge and overflow check follow. Where it
// selects the 8-phase emission kernel and the batch has at least batch_min_b
// queries (0: never), the int8 screen runs in that kernel's place
// (run_q8_screen: `cnorm` is then required) with the same merge and check.
// Every other request, and an overflowed one, is answered by cosine_topk_impl
// as it is. Returns (scores, idx, fallback, counts): fallback is 1 when the
// candidates overflowed (`cap` > 0 overrides their per-row capacity on the
// batched path), 2 when a query of the batch quantised to zeros, 0 otherwise;
// counts are the per-query stage-1 candidate counts (empty off-plan). `stages`
// forces the stage count of the batched screen (0: KAKVEDA_Q8_STAGES, else
// the plan's rule).
std::tuple<torch::Tensor, torch::Tensor, int64_t, torch::Tensor> cosine_topk_q8(
    torch::Tensor queries, torch::Tensor corpus, torch::Tensor codes,
    torch::Tensor meta, int64_t k, int64_t valid_n,
    c10::optional<torch::Tensor> labels, c10::optional<torch::Tensor> want,
    c10::optional<torch::Tensor> cnorm, int64_t batch_min_b, int64_t cap,
    int64_t stages) {
  const Q8Checked c =
      check_q8_search(queries, corpus, codes, meta, k, valid_n, labels, want);
  TORCH_CHECK(queries.size(1) % BK == 0, "D must be a multiple of ", BK);
  static const KnnEnv env = parse_knn_env(std::getenv);
  const KnnArgs a = knn_args(queries, corpus, c.N);
  const KnnPlan p = plan_cosine_topk(a.B, c.N, (int)k, env, true, (bool)c.flt);
  if (q8_screen_in_plan(a, p, env, (bool)c.flt, batch_min_b)) {
    TORCH_CHECK(cnorm.has_value(), "cosine_topk_q8: the batched screen needs cnorm");
    check_q8_cnorm(*cnorm, corpus.device());
    TORCH_CHECK(plan_fits_grid(p, a.B), "cosine_topk_q8: ", a.B,
                " query rows need more row tiles than one launch holds; split "
                "the batch");
    Q8Screen s = run_q8_screen(a, p, env, codes, meta, *cnorm, cap, false,
                               (int)k, stages);
    auto out_score = torch::empty({a.B, k}, a.f32());
    auto out_idx = torch::empty({a.B, k}, a.i64());
    hipLaunchKernelGGL(emit_merge_topk, dim3(a.B), dim3(256), 0, a.stream,
                       (const unsigned long long*)s.e.cand.data_ptr<int64_t>(),
                       (const unsigned*)s.e.ccount.data_ptr<int>(),
                       out_score.data_ptr<float>(),
                       (long*)out_idx.data_ptr<int64_t>(), a.B, s.cap, (int)k);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    const long mx = (long)s.e.ccount.max().item<int>();
    const int degen = s.small[1].item<int>();
    if (env.emit_debug) {
      printf("q8 screen: rows=%d max=%ld mean=%.1f cap=%ld degenerate=%d%s\n",
             a.B, mx, s.e.ccount.to(torch::kFloat32).mean().item<float>(), s.cap,
             degen, mx > s.cap ? "  FALLBACK" : "");
      printf("q8 screen: segments=%ld seg=%ld skip_tiles=%d stages=%d\n",
             (long)s.e.esegcnt.size(0), s.seg, p.skip_tiles, s.sp.n);
    }
    if (degen > 0 || mx > s.cap) {
      auto [sc, ix] = cosine_topk_impl(queries, corpus, (int)k, c.N, env, true);
      return {sc, ix, degen > 0 ? 2 : 1, s.e.ccount};
    }
    return {out_score, out_idx, 0, s.e.ccount};
  }
  if (p.main != MainKernel::SmallB || p.merge != MergeKernel::Emit) {
    auto [s, i] = cosine_topk_impl(queries, corpus, (int)k, c.N, env, true, c.flt);
    return {s, i, 0, torch::empty({0}, a.i32())};
  }
  const Floors f =
      p.prepass ? run_emission_floors(a, p.pre_grid, p.pre_tiles, p.prepass_mode,
                                      KMAX, c.flt)
                : Floors{new_rowthr(a), {}, {}};
  EmitBufs e = new_emit_bufs(a, p.cap, p.mch);
  launch_q8_emit(a, p, codes, meta, f, e, c.flt);
  hipLaunchKernelGGL(q8_rescore, dim3(64, a.B), dim3(256), 0, a.stream, a.q, a.c,
                     a.D, (unsigned long long*)e.cand.data_ptr<int64_t>(),
                     (const unsigned*)e.ccount.data_ptr<int>(), p.cap);
  auto out_score = torch::empty({a.B, k}, a.f32());
  auto out_idx = torch::empty({a.B, k}, a.i64());
  hipLaunchKernelGGL(emit_merge_topk, dim3(a.B), dim3(256), 0, a.stream,
                     (const unsigned long long*)e.cand.data_ptr<int64_t>(),
                     (const unsigned*)e.ccount.data_ptr<int>(),
                     out_score.data_ptr<float>(),
                     (long*)out_idx.data_ptr<int64_t>(), a.B, p.cap, (int)k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  const long mx = (long)e.ccount.max().item<int>();
  if (mx > p.cap) {
    auto [s, i] = cosine_topk_impl(queries, corpus, (int)k, c.N, env, true, c.flt);
    return {s, i, 1, e.ccount};
  }
  return {out_score, out_idx, 0, e.ccount};
}

// Probe of the batched screen: everything up to the merge, nothing after.
// Returns (counts i32 [B], first i32 [B], before i64 [B, cap], after i64
// [B, cap], T f32 [B], kappa f32 [1], the prepass floors u32 [B],
// order-encoded): per row the entries [0, first) are the
// seeds, [first, min(counts, cap)) the screen's candidates, packed as
// emit_bin packs; `before` carries the screen's own score word, `after` the
// bf16 scores. The request must be one the batched path takes at min_b = 1.
std::vector<torch::Tensor> q8_screen_probe(
    torch::Tensor queries, torch::Tensor corpus, torch::Tensor codes,
    torch::Tensor meta, torch::Tensor cnorm, int64_t k, int64_t valid_n,
    int64_t cap) {
  const Q8Checked c = check_q8_search(queries, corpus, codes, meta, k, valid_n,
                                      c10::nullopt, c10::nullopt);
  check_q8_cnorm(cnorm, corpus.device());
  static const KnnEnv env = parse_knn_env(std::getenv);
  const KnnArgs a = knn_args(queries, corpus, c.N);
  const KnnPlan p = plan_cosine_topk(a.B, c.N, (int)k, env, true, false);
  TORCH_CHECK(q8_screen_in_plan(a, p, env, false, 1) && plan_fits_grid(p, a.B),
              "q8_screen_probe: not a request of the batched int8 screen");
  // one stage: what it returns keeps its meaning (the prepass floors, one T_r)
  Q8Screen s = run_q8_screen(a, p, env, codes, meta, cnorm, cap, true, (int)k, 1);
  return {s.e.ccount, s.first, s.before, s.e.cand, s.thrT,
          s.small.slice(0, 0, 1).view(torch::kFloat32), s.rowthr};
}

// The stage plan of the batched screen for (B, N, k, stages) under this
// process's environment: (first [n + 1], chunk_tiles [n], nchunks [n]); stage
// i scans the 256-column tiles [first[i], first[i + 1]). Host only.
std::tuple<std::vector<int64_t>, std::vector<int64_t>, std::vector<int64_t>>
q8_stage_plan_op(int64_t B, int64_t N, int64_t k, int64_t stages) {
  static const KnnEnv env = parse_knn_env(std::getenv);
  TORCH_CHECK(B >= 1 && N >= 1 && N <= 0x7fffffffL && k >= 1 && k <= KMAX,
              "q8_stage_plan: B, N or k out of range");
  TORCH_CHECK(stages >= 0 && stages <= Q8_MAX_STAGES,
              "stages must be in [1,", Q8_MAX_STAGES, "], or 0 for the plan's rule");
  const KnnPlan p = plan_cosine_topk((int)B, (int)N, (int)k, env, true, false);
  TORCH_CHECK(p.main == MainKernel::Emit8p && p.prepass,
              "q8_stage_plan: not a request of the batched int8 screen");
  const StagePlan sp =
      plan_q8_stages(p, env, stages > 0 ? (int)stages : env.q8_stages);
  std::vector<int64_t> first(sp.first, sp.first + sp.n + 1), ct, nc;
  for (int i = 0; i < sp.n; ++i) {
    ct.push_back(sp.ch[i].chunk_tiles);
    nc.push_back(sp.ch[i].nchunks);
  }
  return {first, ct, nc};
}

// Benchmark probe: the stage-1 candidate counts of one request under both
// arms, from one set of floors: (q8 counts, bf16 counts), i32 [B] each. The
// request must be one the q8 path takes.
std::tuple<torch::Tensor, torch::Tensor> q8_counts_probe(
    torch::Tensor queries, torch::Tensor corpus, torch::Tensor codes,
    torch::Tensor meta, int64_t k, int64_t valid_n,
    c10::optional<torch::Tensor> labels, c10::optional<torch::Tensor> want) {
  const Q8Checked c =
      check_q8_search(queries, corpus, codes, meta, k, valid_n, labels, want);
  static const KnnEnv env = parse_knn_env(std::getenv);
  const KnnArgs a = knn_args(queries, corpus, c.N);
  const KnnPlan p = plan_cosine_topk(a.B, c.N, (int)k, env, true, (bool)c.flt);
  TORCH_CHECK(p.main == MainKernel::SmallB && p.prepass,
              "q8_counts_probe: not a request of the small-batch plan");
  const Floors f = run_emission_floors(a, p.pre_grid, p.pre_tiles,
                                       p.prepass_mode, KMAX, c.flt);
  EmitBufs e8 = new_emit_bufs(a, p.cap, p.mch);
  launch_q8_emit(a, p, codes, meta, f, e8, c.flt);
  EmitBufs e16 = new_emit_bufs(a, p.cap, p.mch);
  const auto v4 = c.flt ? smallb_emit_kernel_v4<true> : smallb_emit_kernel_v4<false>;
  hipLaunchKernelGGL(v4, dim3(p.smallb_blocks), dim3(256), (size_t)a.B * a.D * 2,
                     a.stream, a.q, a.c, a.B, (long)a.N, a.D,
                     (const unsigned*)f.rowthr.data_ptr<int>(),
                     (unsigned long long*)e16.cand.data_ptr<int64_t>(),
                     (unsigned*)e16.ccount.data_ptr<int>(), p.cap, c.flt.labels,
                     c.flt.want);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {e8.ccount, e16.ccount};
}

void l2normalize_(torch::Tensor t, int64_t start_row, int64_t end_row) {
  check_bf16_2d(t, "t");
  const int nrows = (int)(end_row - start_row);
  if (nrows <= 0) return;
  const int D = t.size(1);
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  auto stream = c10::hip::getCurrentHIPStream();
  const int blocks = std::min((nrows + 3) / 4, 2048);
  hipLaunchKernelGGL(l2normalize_rows, dim3(blocks), dim3(THREADS), 0,
                     stream.stream(), (bf16_t*)t.data_ptr(), (int)start_row,
                     nrows, D);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

torch::Tensor embedding_bag(torch::Tensor table, torch::Tensor idx, torch::Tensor w) {
  check_bf16_2d(table, "table");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 && idx.dim() == 2 && idx.is_contiguous(), "idx must be contiguous 2-D i32 on GPU");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kFloat32 && w.is_contiguous(), "w must be contiguous f32 on GPU");
  const int B = idx.size(0);
  const int L = idx.size(1);
  const int D = table.size(1);
  const int V = table.size(0);
  TORCH_CHECK(L <= 128, "L must be <= 128");
  TORCH_CHECK(w.size(0) == B && w.size(1) == L, "w shape mismatch");
  auto out = torch::empty({B, D}, torch::TensorOptions().dtype(torch::kFloat32).device(table.device()));
  if (B == 0 || D == 0) return out;  // nothing to launch
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(embedding_bag_kernel, dim3(B), dim3(THREADS), 0,
                     stream.stream(), (const bf16_t*)table.data_ptr(),
                     idx.data_ptr<int>(), w.data_ptr<float>(),
                     out.data_ptr<float>(), L, D, V);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> kmeans_assign(
    torch::Tensor points, torch::Tensor centroids) {
  // Dedicated C<=64 assignment kernel: LDS-resident centroids, direct
  // global->register point fragments, no per-window barriers
  // (kernels_impl.h kmeans_assign_kernel; ROUND2.md round-2 item).
  check_bf16_2d(points, "points");
  check_bf16_2d(centroids, "centroids");
  const long N = points.size(0);
  const int D = points.size(1);
  const int C = centroids.size(0);
  TORCH_CHECK(centroids.size(1) == D, "dim mismatch");
  TORCH_CHECK(D % 64 == 0, "D must be a multiple of 64");
  TORCH_CHECK(C >= 1 && C <= 64, "kmeans_assign kernel supports C<=64");
  const size_t lds = 64 * (size_t)assign_pitch(D);
  TORCH_CHECK(lds <= ASSIGN_LDS_BYTES, "D too large for LDS-resident centroids");
  auto opts_f = torch::TensorOptions().dtype(torch::kFloat32).device(points.device());
  auto opts_i = torch::TensorOptions().dtype(torch::kInt32).device(points.device());
  auto score = torch::empty({N}, opts_f);
  auto idx = torch::empty({N}, opts_i);
  if (N == 0) return {score, idx};  // nothing to launch
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kmeans_assign_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              ASSIGN_LDS_BYTES);
    attr_set = true;
  }
  const long ntiles = (N + 255) / 256;
  const int grid = (int)std::min<long>(ntiles, 2048);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(grid), dim3(ASSIGN_THREADS),
                     lds, stream.stream(), (const bf16_t*)points.data_ptr(),
                     (const bf16_t*)centroids.data_ptr(),
                     score.data_ptr<float>(), idx.data_ptr<int>(), (int)N, D,
                     C);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {score, idx};
}

std::tuple<torch::Tensor, torch::Tensor> kmeans_update(
    torch::Tensor points, torch::Tensor assign, int64_t n_clusters) {
  check_bf16_2d(points, "points");
  TORCH_CHECK(assign.is_cuda() && assign.scalar_type() == torch::kInt32 &&
                  assign.is_contiguous(),
              "assign must be contiguous i32 on GPU");
  const int N = points.size(0);
  const int D = points.size(1);
  const int C = (int)n_clusters;
  TORCH_CHECK(D % 64 == 0, "D must be a multiple of 64");
  TORCH_CHECK(C >= 1 && C <= 512, "n_clusters must be in [1,512]");
  // replicated partials for C<=128 (4x[C][64]) or single-replica above;
  // either can exceed the 64 KiB default dynamic cap
  const int repl = (C <= 128) ? 4 : 1;
  const size_t lds_upd = ((size_t)repl * C * 64 + C) * 4;
  TORCH_CHECK(lds_upd <= 160 * 1024, "n_clusters LDS overflow");
  if (lds_upd > 64 * 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)kmeans_update_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      attr_set = true;
    }
  }
  auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(points.device());
  auto sums = torch::zeros({C, D}, opts);
  auto counts = torch::zeros({C}, opts);
  if (N == 0) return {sums, counts};  // nothing to launch
  // chunk so the grid oversubscribes the CUs
  const int dim_tiles = D / 64;
  int chunks = std::max(1, 2048 / dim_tiles);
  const int ppc = (N + chunks - 1) / chunks;
  chunks = (N + ppc - 1) / ppc;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(dim_tiles, chunks), dim3(256),
                     lds_upd, stream.stream(),
                     (const bf16_t*)points.data_ptr(), assign.data_ptr<int>(),
                     sums.data_ptr<float>(), counts.data_ptr<float>(), N, D, C,
                     ppc);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {sums, counts};
}

namespace {

// The probes' floors: pregq sampled chunks in blocks of pre_tiles column
// tiles (0: PRE_TILES, one block per chunk; any other value is checked like
// KAKVEDA_KNN_PRE_TILES and refused before anything is launched).
Floors probe_floors(const KnnArgs& a, int64_t pregq, int64_t pre_tiles, int k) {
  const int preg = ((int)pregq) & ~7;
  if (pre_tiles == 0) return run_emission_floors(a, preg, PRE_TILES, 11, k);
  const int pre_grid = forced_pre_grid(preg, pre_tiles, "pre_tiles");
  return run_emission_floors(a, pre_grid, (int)pre_tiles, 11, k);
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> floor_probe(
    torch::Tensor queries, torch::Tensor corpus, int64_t pregq, int64_t k,
    int64_t pre_tiles) {
  // Debug: run ONLY the emission floor pipeline (prepass -> compact
  // partials -> merge -> publish) and return (samp_s [B,KMAX], samp_i,
  // rowthr u32 [B]) for offline comparison against a torch reference. The
  // published floor is the k-th best of the sample (k = 8: the deepest).
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const KnnArgs a = knn_args(queries, corpus, (int)corpus.size(0));
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  const Floors f = probe_floors(a, pregq, pre_tiles, (int)k);
  return {f.samp_s, f.samp_i, f.rowthr};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> emit_counts_probe(
    torch::Tensor queries, torch::Tensor corpus, int64_t pregq, int64_t k,
    int64_t pre_tiles) {
  // Debug: run floors (k-th best of the sample) + the mode-9 emission
  // kernel + the binning step and return the raw per-row candidate counts
  // and candidates (no merge, no fallback) for offline inspection of which
  // rows overcount.
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  const KnnArgs a = knn_args(queries, corpus, (int)corpus.size(0));
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  const Floors f = probe_floors(a, pregq, pre_tiles, (int)k);
  const Chunking ch = chunking(a.B, a.N, BM8, default_target(BM8));
  const long CAP = 32768;
  const long seg = emit_seg_cap(a.B, CAP, ch, 0);
  auto pscore = torch::empty({(long)a.B * ch.nchunks * KMAX}, a.f32());
  auto pidx = torch::empty({(long)a.B * ch.nchunks * KMAX}, a.i32());
  EmitBufs e = new_emit_bufs(a, CAP, ch, seg);
  launch_emit8p(9, a, ch, pscore, pidx, f.rowthr, e, CAP, seg);
  return {e.ccount, e.cand, f.rowthr};
}

double probe8p(torch::Tensor queries, torch::Tensor corpus, int64_t mode,
               int64_t iters) {
  // Timing probe for 8p epilogue isolation (profiles/knn_kernel_history):
  // mode 1 = no epilogue (GEMM core, staggered wave groups), 16 = the same
  // core on the lockstep schedule (A/B of the sync structure in one process
  // on the same buffers), 12 = hot sweep only (worst case: null thresholds
  // make every ballot fire). None touches the emission buffers, so none
  // are passed. Returns ms per launch.
  check_bf16_2d(queries, "queries");
  check_bf16_2d(corpus, "corpus");
  TORCH_CHECK(mode == 1 || mode == 12 || mode == 16,
              "probe8p mode must be 1 (GEMM core), 16 (lockstep GEMM core) or "
              "12 (hot sweep), got ", mode);
  const KnnArgs a = knn_args(queries, corpus, (int)corpus.size(0));
  const Chunking ch = chunking(a.B, a.N, BM8, default_target(BM8));
  auto pscore = torch::empty({(long)a.B * ch.nchunks * KMAX}, a.f32());
  auto pidx = torch::empty({(long)a.B * ch.nchunks * KMAX}, a.i32());
  auto launch = [&] {
    launch_partial8p((int)mode, dim3(ch.nchunks, ch.row_tiles), a,
                     pscore.data_ptr<float>(), pidx.data_ptr<int>(),
                     ch.chunk_tiles, ch.nchunks, nullptr, nullptr, nullptr, 0);
  };
  launch();  // warmup
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0, a.stream);
  for (long i = 0; i < iters; ++i) launch();
  hipEventRecord(e1, a.stream);
  hipEventSynchronize(e1);
  float ms = 0.f;
  hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return (double)ms / (double)iters;
}

double probe8p_i8(torch::Tensor queries, torch::Tensor codes, torch::Tensor meta,
                  int64_t mode, int64_t iters) {
  // Timing probe of the int8 screen kernel, the twin of probe8p: mode 1 = no
  // epilogue (cosine_topk_screen8p_i8<false>: staging, int8 MFMA, waits, barriers
  // only), 12 = the production kernel under T_r = +big (accumulator
  // conversion and hot sweep on every tile, the cold path never taken). Both
  // run the whole-corpus geometry of probe8p over the mirror's rows and emit
  // nothing. Returns ms per launch.
  check_bf16_2d(queries, "queries");
  TORCH_CHECK(mode == 1 || mode == 12,
              "probe8p_i8 mode must be 1 (GEMM core) or 12 (hot sweep), got ", mode);
  TORCH_CHECK(iters >= 1, "iters must be positive");
  const int64_t N = codes.size(0), D = queries.size(1);
  TORCH_CHECK(q8_screen_dim_ok(D), "D must be a multiple of ", Q8_SEG, " up to ",
              Q8_SCREEN_MAX_D);
  TORCH_CHECK(N >= 1 && N <= 0x7fffffffL, "rows out of range");
  check_q8_mirror(codes, meta, queries.device(), N, D);
  const KnnArgs a{(const bf16_t*)queries.data_ptr(), nullptr, (int)queries.size(0),
                  (int)N, (int)D, c10::hip::getCurrentHIPStream().stream(),
                  queries.device()};
  const Chunking ch = chunking(a.B, a.N, BM8, default_target(BM8));
  TORCH_CHECK(ch.row_tiles <= MAX_GRID_Y, "too many query rows for one launch");
  const auto i8 = torch::TensorOptions().dtype(torch::kInt8).device(a.dev);
  auto qcodes = torch::empty({(long)a.B, (long)a.D}, i8);
  auto qmeta = torch::empty({(long)a.B, 2L}, a.f32());
  hipLaunchKernelGGL(q8_quantize_kernel, dim3((a.B + 31) / 32), dim3(256), 0,
                     a.stream, a.q, (long)a.B, a.D,
                     (signed char*)qcodes.data_ptr<int8_t>(),
                     qmeta.data_ptr<float>(), 0L);
  auto thrT = torch::full({(long)a.B}, 1e38f, a.f32());
  auto kappa = torch::ones({1L}, a.f32());
  const long blocks = (long)ch.nchunks * ch.row_tiles;
  auto eseg = torch::empty({blocks}, a.i64());  // one record a segment, unused
  auto esegcnt = torch::empty({blocks}, a.i32());
  const auto kernel =
      mode == 1 ? cosine_topk_screen8p_i8<false> : cosine_topk_screen8p_i8<true>;
  auto launch = [&] {
    hipLaunchKernelGGL(kernel, dim3(ch.nchunks, ch.row_tiles), dim3(THREADS8), 0,
                       a.stream, (const signed char*)qcodes.data_ptr<int8_t>(),
                       (const signed char*)codes.data_ptr<int8_t>(),
                       (const float*)meta.data_ptr<float>(),
                       (const float*)thrT.data_ptr<float>(),
                       (const float*)kappa.data_ptr<float>(), a.B, a.N, a.D,
                       ch.chunk_tiles, ch.nchunks,
                       (unsigned long long*)eseg.data_ptr<int64_t>(),
                       (unsigned*)esegcnt.data_ptr<int>(), 1L, 0);
  };
  launch();  // warmup
  hipEvent_t e0, e1;
  C10_HIP_CHECK(hipEventCreate(&e0));
  C10_HIP_CHECK(hipEventCreate(&e1));
  C10_HIP_CHECK(hipEventRecord(e0, a.stream));
  for (long i = 0; i < iters; ++i) launch();
  C10_HIP_CHECK(hipEventRecord(e1, a.stream));
  C10_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  C10_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  C10_HIP_CHECK(hipEventDestroy(e0));
  C10_HIP_CHECK(hipEventDestroy(e1));
  return (double)ms / (double)iters;
}

// ---- cluster-routed (IVF) search ------------------------------------------

namespace {

void check_i32_gpu(const torch::Tensor& t, int64_t dim, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                  t.dim() == dim && t.is_contiguous(),
              name, " must be contiguous ", dim, "-D i32 on GPU");
}

// The by-value segment table of a routed launch; refuses, before anything
// is launched, a store the kernel's row -> segment function cannot address.
IvfSegs ivf_segs(const std::vector<torch::Tensor>& segments,
                 const torch::Tensor& queries, long valid_n) {
  const int n = (int)segments.size();
  long q = 1;
  try {
    q = ivf_check_segments(n, [&](int i) { return (long)segments[i].size(0); });
  } catch (const std::invalid_argument& e) {
    TORCH_CHECK(false, e.what());
  }
  IvfSegs s{};
  long total = 0;
  for (int i = 0; i < n; ++i) {
    check_bf16_2d(segments[i], "segment");
    TORCH_CHECK(segments[i].device() == queries.device(),
                "segments and queries must be on one device");
    TORCH_CHECK(segments[i].size(1) == queries.size(1), "dim mismatch");
    s.base[i] = (const bf16_t*)segments[i].data_ptr();
    total += segments[i].size(0);
  }
  for (int i = n; i < IVF_MAX_SEGMENTS; ++i) s.base[i] = s.base[0];
  s.s0 = segments[0].size(0);
  s.q = q;
  TORCH_CHECK(valid_n >= 1 && valid_n <= total && valid_n <= 0x7fffffffL,
              "valid_n out of range");
  return s;
}

}  // namespace

torch::Tensor ivf_route_scores_op(torch::Tensor queries, torch::Tensor centroids) {
  check_bf16_2d(queries, "queries");
  check_bf16_2d(centroids, "centroids");
  const int B = queries.size(0), D = queries.size(1), L = centroids.size(0);
  TORCH_CHECK(centroids.device() == queries.device(),
              "centroids and queries must be on one device");
  TORCH_CHECK(centroids.size(1) == D, "dim mismatch");
  TORCH_CHECK(D % 64 == 0 && D >= 64, "D must be a multiple of 64");
  TORCH_CHECK((size_t)8 * D * 2 <= 64 * 1024, "D too large for LDS queries");
  TORCH_CHECK(B >= 1 && L >= 1, "empty queries or centroids");
  TORCH_CHECK((B + 7) / 8 <= 65535, "too many queries for one launch");
  auto out = torch::empty(
      {B, L}, torch::TensorOptions().dtype(torch::kFloat32).device(queries.device()));
  const int gx = std::min((L + 31) / 32, 4096);
  hipLaunchKernelGGL(ivf_route_scores, dim3(gx, (B + 7) / 8), dim3(256),
                     (size_t)std::min(B, 8) * D * 2,
                     c10::hip::getCurrentHIPStream().stream(),
                     (const bf16_t*)queries.data_ptr(),
                     (const bf16_t*)centroids.data_ptr(), out.data_ptr<float>(),
                     B, L, D);
  return out;
}

namespace {

// What both routed scans check before anything is launched.
struct IvfScanArgs {
  IvfSegs segs;
  int B, D, L, nprobe;
};

IvfScanArgs ivf_scan_args(const torch::Tensor& queries,
                          const std::vector<torch::Tensor>& segments,
                          const torch::Tensor& offsets, const torch::Tensor& ids,
                          const torch::Tensor& probes, int64_t k, int64_t valid_n,
                          int64_t tail_lo, int64_t tail_hi, int64_t max_list_len) {
  check_bf16_2d(queries, "queries");
  const int B = queries.size(0), D = queries.size(1);
  const IvfSegs segs = ivf_segs(segments, queries, (long)valid_n);
  TORCH_CHECK(D % 64 == 0 && D >= 64, "D must be a multiple of 64");
  TORCH_CHECK((size_t)D * 2 <= 64 * 1024, "D too large for an LDS query");
  TORCH_CHECK(k >= 1 && k <= KMAX, "k must be in [1,", KMAX, "]");
  TORCH_CHECK(B >= 1, "no queries");
  TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == torch::kInt64 &&
                  offsets.dim() == 1 && offsets.is_contiguous() &&
                  offsets.size(0) >= 1,
              "offsets must be contiguous 1-D i64 on GPU with L+1 entries");
  check_i32_gpu(ids, 1, "ids");
  check_i32_gpu(probes, 2, "probes");
  TORCH_CHECK(offsets.device() == queries.device() &&
                  ids.device() == queries.device() &&
                  probes.device() == queries.device(),
              "offsets, ids, probes and queries must be on one device");
  TORCH_CHECK(probes.size(0) == B, "probes needs one row per query");
  const int L = (int)offsets.size(0) - 1;
  const int nprobe = (int)probes.size(1);
  TORCH_CHECK(nprobe <= 65534, "nprobe too large");
  TORCH_CHECK(tail_lo >= 0 && tail_lo <= tail_hi && tail_hi <= valid_n,
              "tail range must satisfy 0 <= tail_lo <= tail_hi <= valid_n");
  TORCH_CHECK(max_list_len >= 0, "max_list_len must be >= 0");
  return {segs, B, D, L, nprobe};
}

// The label predicate of a filtered routed launch: the by-value table of
// per-segment label pointers and the per-query wants. Refuses, before
// anything is launched, labels the kernels' row -> segment function would
// address out of bounds.
IvfFilterArg<true> ivf_filter(const std::vector<torch::Tensor>& segments,
                              const std::vector<torch::Tensor>& labels,
                              const torch::Tensor& want,
                              const torch::Tensor& queries) {
  TORCH_CHECK(labels.size() == segments.size(), "labels needs one tensor per segment (",
              segments.size(), "), got ", labels.size());
  TORCH_CHECK(!segments.empty() && segments.size() <= (size_t)IVF_MAX_SEGMENTS,
              "routed search supports 1 to ", IVF_MAX_SEGMENTS, " store segments");
  IvfFilterArg<true> f{};
  const int n = (int)labels.size();
  for (int i = 0; i < n; ++i) {
    check_i32_gpu(labels[i], 1, "labels");
    TORCH_CHECK(labels[i].device() == queries.device(),
                "labels and queries must be on one device");
    TORCH_CHECK(segments[i].dim() == 2 && labels[i].size(0) == segments[i].size(0),
                "labels of segment ", i, " must have exactly its ",
                segments[i].dim() == 2 ? segments[i].size(0) : -1, " rows, got ",
                labels[i].size(0));
    f.labels.base[i] = labels[i].data_ptr<int>();
  }
  for (int i = n; i < IVF_MAX_SEGMENTS; ++i) f.labels.base[i] = f.labels.base[0];
  check_i32_gpu(want, 1, "want");
  TORCH_CHECK(want.device() == queries.device(),
              "want and queries must be on one device");
  TORCH_CHECK(queries.dim() == 2 && want.size(0) == queries.size(0),
              "want needs one entry per query");
  f.want = want.data_ptr<int>();
  return f;
}

// The filter of the launch whose first query is b0.
IvfFilterArg<false> ivf_filter_from(IvfFilterArg<false> f, int) { return f; }
IvfFilterArg<true> ivf_filter_from(IvfFilterArg<true> f, int b0) {
  f.want += b0;
  return f;
}

// ivf_scan_topk, and with a filter ivf_scan_topk_filtered: the same plan,
// candidate buffer and merge; FILTER picks the kernel's instantiation.
template <bool FILTER>
std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk_impl(
    const torch::Tensor& queries, const std::vector<torch::Tensor>& segments,
    const torch::Tensor& offsets, const torch::Tensor& ids,
    const torch::Tensor& probes, int64_t k, int64_t valid_n, int64_t tail_lo,
    int64_t tail_hi, int64_t max_list_len, const IvfFilterArg<FILTER>& filter) {
  const IvfScanArgs a = ivf_scan_args(queries, segments, offsets, ids, probes, k,
                                      valid_n, tail_lo, tail_hi, max_list_len);
  const IvfSegs& segs = a.segs;
  const int B = a.B, D = a.D, L = a.L, nprobe = a.nprobe;

  auto dev = queries.device();
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto out_score = torch::empty(
      {B, k}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  auto out_idx =
      torch::empty({B, k}, torch::TensorOptions().dtype(torch::kInt64).device(dev));
  const IvfPlan p =
      plan_ivf_scan((long)max_list_len, (long)(tail_hi - tail_lo), nprobe, B);
  // grid.z holds at most IVF_MAX_GRID_Z queries: chunk the batch
  for (int b0 = 0; b0 < B; b0 += IVF_MAX_GRID_Z) {
    const int nb = std::min(B - b0, IVF_MAX_GRID_Z);
    auto cand = torch::empty(
        {(long)nb, p.cand_entries},
        torch::TensorOptions().dtype(torch::kInt64).device(dev));
    auto ccount = torch::full(
        {(long)nb}, (int64_t)p.cand_entries,
        torch::TensorOptions().dtype(torch::kInt32).device(dev));
    hipLaunchKernelGGL(
        ivf_scan_topk_kernel<FILTER>, dim3(p.slices, p.sources, nb), dim3(256),
        (size_t)D * 2, stream, (const bf16_t*)queries.data_ptr() + (size_t)b0 * D,
        segs, ivf_filter_from(filter, b0),
        (const long*)offsets.data_ptr<int64_t>(), ids.data_ptr<int>(),
        probes.data_ptr<int>() + (size_t)b0 * nprobe, nprobe, L,
        (long)ids.size(0), D, (long)valid_n, (long)tail_lo, (long)tail_hi,
        (unsigned long long*)cand.data_ptr<int64_t>());
    hipLaunchKernelGGL(emit_merge_topk, dim3(nb), dim3(256), 0, stream,
                       (const unsigned long long*)cand.data_ptr<int64_t>(),
                       (const unsigned*)ccount.data_ptr<int>(),
                       out_score.data_ptr<float>() + (size_t)b0 * k,
                       (long*)out_idx.data_ptr<int64_t>() + (size_t)b0 * k, nb,
                       p.cand_entries, (int)k);
  }
  return {out_score, out_idx};
}

// route -> select: score the centroids and take the nprobe best lists per
// query (torch.topk on the tiny [B, L] score tensor).
torch::Tensor ivf_route_probes(const torch::Tensor& queries,
                               const torch::Tensor& centroids,
                               const torch::Tensor& offsets,
                               const torch::Tensor& ids, int64_t nprobe,
                               int64_t n_indexed) {
  TORCH_CHECK(offsets.dim() == 1 && offsets.size(0) == centroids.size(0) + 1,
              "offsets must have L+1 entries for L centroids");
  TORCH_CHECK(ids.dim() == 1 && ids.size(0) == n_indexed,
              "ids must have n_indexed entries");
  TORCH_CHECK(n_indexed >= 0, "n_indexed must be >= 0");
  const int64_t L = centroids.size(0);
  TORCH_CHECK(nprobe >= 1 && nprobe <= L, "nprobe must be in [1, n_lists]");
  auto scores = ivf_route_scores_op(queries, centroids);
  return std::get<1>(scores.topk(nprobe, 1)).to(torch::kInt32).contiguous();
}

}  // namespace

// ---- list-major (batched) routed scan --------------------------------------

std::vector<torch::Tensor> ivf_group_probes_op(torch::Tensor probes,
                                               int64_t n_lists) {
  // The B x (nprobe + 1) (query, probe) pairs - column nprobe being the tail,
  // pseudo-list n_lists - sorted by list and cut into tiles of at most
  // IVF_BATCH_QTILE pairs of one list; probes outside [0, n_lists) form a
  // last group that gets no tile. Returns {pair_query i32 [P], pair_slot
  // i32 [P], tiles i32 [3][T] (list, first pair, pair count; count 0 from
  // the tile count on), n_tiles i32 [1]}, T = ivf_batch_tile_bound(P, L).
  // Torch ops only, none of which reads device memory on the host (the
  // same sequence as ops.ivf_group_probes in Python).
  TORCH_CHECK(probes.dim() == 2 && probes.size(0) >= 1, "probes must be [B, nprobe]");
  TORCH_CHECK(n_lists >= 0, "n_lists must be >= 0");
  const int64_t B = probes.size(0), S = probes.size(1) + 1, P = B * S;
  const int64_t L = n_lists, QT = IVF_BATCH_QTILE;
  const int64_t T = ivf_batch_tile_bound(P, L);
  auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(probes.device());
  auto pl = probes.to(torch::kInt64);
  pl = torch::where((pl >= 0) & (pl < L), pl, torch::full({}, L + 1, i64));
  auto keys = torch::cat({pl, torch::full({B, 1}, L, i64)}, 1).reshape({P});
  auto order = std::get<1>(keys.sort(/*stable=*/true, /*dim=*/0, /*descending=*/false));
  auto counts = torch::zeros({L + 2}, i64)
                    .scatter_add_(0, keys, torch::ones({P}, i64))
                    .slice(0, 0, L + 1);
  auto starts = counts.cumsum(0) - counts;
  auto ntl = (counts + (QT - 1)).floor_divide(QT);
  auto tend = ntl.cumsum(0);
  auto n_tiles = tend.slice(0, L, L + 1);
  auto t = torch::arange(T, i64);
  auto li = torch::searchsorted(tend, t, /*out_int32=*/false, /*right=*/true)
                .clamp_max(L);
  auto within = t - (tend.index_select(0, li) - ntl.index_select(0, li));
  auto live = t < n_tiles;
  auto zero = torch::zeros({}, i64);
  auto tfirst = torch::where(live, starts.index_select(0, li) + within * QT, zero);
  auto tcnt = torch::where(
      live, (counts.index_select(0, li) - within * QT).clamp(0, QT), zero);
  auto tiles = torch::stack({li, tfirst, tcnt}, 0).to(torch::kInt32).contiguous();
  return {order.floor_divide(S).to(torch::kInt32).contiguous(),
          order.remainder(S).to(torch::kInt32).contiguous(), tiles,
          n_tiles.to(torch::kInt32).contiguous()};
}

namespace {

// ivf_scan_topk_batched, and with a filter ivf_scan_topk_batched_filtered:
// the same grouping, plan, candidate buffer and merge; FILTER picks the
// kernel's instantiation.
template <bool FILTER>
std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk_batched_impl(
    const torch::Tensor& queries, const std::vector<torch::Tensor>& segments,
    const torch::Tensor& offsets, const torch::Tensor& ids,
    const torch::Tensor& probes, int64_t k, int64_t valid_n, int64_t tail_lo,
    int64_t tail_hi, int64_t max_list_len, const IvfFilterArg<FILTER>& filter) {
  const IvfScanArgs a = ivf_scan_args(queries, segments, offsets, ids, probes, k,
                                      valid_n, tail_lo, tail_hi, max_list_len);
  const int B = a.B, D = a.D, L = a.L, nprobe = a.nprobe;
  const size_t lds = (size_t)ivf_batch_query_lds(D);
  TORCH_CHECK(D <= IVF_BATCH_MAX_D, "D too large for the LDS query tile (at most ",
              IVF_BATCH_MAX_D, ")");

  auto dev = queries.device();
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto out_score = torch::empty(
      {B, k}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  auto out_idx =
      torch::empty({B, k}, torch::TensorOptions().dtype(torch::kInt64).device(dev));
  const long tail_len = (long)(tail_hi - tail_lo);
  // chunk the batch so that one launch's candidate buffer stays capped
  const int chunk =
      ivf_batch_chunk_queries((long)max_list_len, tail_len, nprobe, B, L);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = std::min(B - b0, chunk);
    const IvfBatchPlan p =
        plan_ivf_batch((long)max_list_len, tail_len, nprobe, nb, L);
    auto grp = ivf_group_probes_op(probes.slice(0, b0, b0 + nb), L);
    const int* tiles = grp[2].data_ptr<int>();
    TORCH_CHECK(grp[2].size(1) == p.max_tiles, "tile table / plan mismatch");
    // preset every slot to 0 (empty): blocks store only what they scanned
    auto cand = torch::zeros(
        {(long)nb, p.cand_entries},
        torch::TensorOptions().dtype(torch::kInt64).device(dev));
    auto ccount = torch::full(
        {(long)nb}, (int64_t)p.cand_entries,
        torch::TensorOptions().dtype(torch::kInt32).device(dev));
    // grid.y holds at most 65535 tiles
    for (long t0 = 0; t0 < p.max_tiles; t0 += 65535) {
      const int nt = (int)std::min(p.max_tiles - t0, 65535L);
      hipLaunchKernelGGL(
          ivf_scan_grouped_kernel<FILTER>, dim3(p.slices, nt), dim3(256), lds,
          stream, (const bf16_t*)queries.data_ptr() + (size_t)b0 * D, a.segs,
          ivf_filter_from(filter, b0),
          (const long*)offsets.data_ptr<int64_t>(), ids.data_ptr<int>(),
          grp[0].data_ptr<int>(), grp[1].data_ptr<int>(), tiles,
          tiles + p.max_tiles, tiles + 2 * p.max_tiles, grp[3].data_ptr<int>(),
          (int)t0, nb, nprobe + 1, L, (long)ids.size(0), D, (long)valid_n,
          (long)tail_lo, (long)tail_hi, p.pairs,
          (unsigned long long*)cand.data_ptr<int64_t>());
    }
    hipLaunchKernelGGL(emit_merge_topk, dim3(nb), dim3(256), 0, stream,
                       (const unsigned long long*)cand.data_ptr<int64_t>(),
                       (const unsigned*)ccount.data_ptr<int>(),
                       out_score.data_ptr<float>() + (size_t)b0 * k,
                       (long*)out_idx.data_ptr<int64_t>() + (size_t)b0 * k, nb,
                       p.cand_entries, (int)k);
  }
  return {out_score, out_idx};
}

// The four searches: route -> select -> scan. Score the centroids, take the
// nprobe best lists per query, scan those lists plus the tail [n_indexed,
// valid_n) (empty when valid_n is a snapshot from before the index was
// built; listed ids >= valid_n are dropped by the scan). `batched` takes the
// list-major scan (-> group -> scan -> merge). The routing does not know
// labels; the caller has checked the filter before the routing kernel runs.
template <bool FILTER>
std::tuple<torch::Tensor, torch::Tensor> ivf_search_impl(
    bool batched, const torch::Tensor& queries,
    const std::vector<torch::Tensor>& segments, const IvfFilterArg<FILTER>& filter,
    const torch::Tensor& centroids, const torch::Tensor& offsets,
    const torch::Tensor& ids, int64_t nprobe, int64_t k, int64_t valid_n,
    int64_t n_indexed, int64_t max_list_len) {
  auto probes = ivf_route_probes(queries, centroids, offsets, ids, nprobe, n_indexed);
  const auto scan =
      batched ? ivf_scan_topk_batched_impl<FILTER> : ivf_scan_topk_impl<FILTER>;
  return scan(queries, segments, offsets, ids, probes, k, valid_n,
              std::min(n_indexed, valid_n), valid_n, max_list_len, filter);
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    torch::Tensor offsets, torch::Tensor ids, torch::Tensor probes, int64_t k,
    int64_t valid_n, int64_t tail_lo, int64_t tail_hi, int64_t max_list_len) {
  // Exact top-k of each query over the rows of its probed lists plus the
  // tail [tail_lo, tail_hi). max_list_len only sizes the grid (any value
  // >= 0 gives the same result); rows short of k candidates come back padded
  // with (NEG_INF, -1), which the Python op normalises.
  return ivf_scan_topk_impl<false>(queries, segments, offsets, ids, probes, k,
                                   valid_n, tail_lo, tail_hi, max_list_len, {});
}

std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk_filtered(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    std::vector<torch::Tensor> labels, torch::Tensor want, torch::Tensor offsets,
    torch::Tensor ids, torch::Tensor probes, int64_t k, int64_t valid_n,
    int64_t tail_lo, int64_t tail_hi, int64_t max_list_len) {
  // ivf_scan_topk over the candidates row r with want[b] < 0 || label(r) ==
  // want[b]; labels: one i32 tensor per segment, want: i32 [B].
  return ivf_scan_topk_impl<true>(queries, segments, offsets, ids, probes, k,
                                  valid_n, tail_lo, tail_hi, max_list_len,
                                  ivf_filter(segments, labels, want, queries));
}

std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk_batched(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    torch::Tensor offsets, torch::Tensor ids, torch::Tensor probes, int64_t k,
    int64_t valid_n, int64_t tail_lo, int64_t tail_hi, int64_t max_list_len) {
  // ivf_scan_topk's contract through the list-major kernel: group the
  // (query, probe) pairs by list, scan every (tile, slice) once with
  // ivf_scan_grouped_kernel, finish with emit_merge_topk.
  return ivf_scan_topk_batched_impl<false>(queries, segments, offsets, ids, probes,
                                           k, valid_n, tail_lo, tail_hi,
                                           max_list_len, {});
}

std::tuple<torch::Tensor, torch::Tensor> ivf_scan_topk_batched_filtered(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    std::vector<torch::Tensor> labels, torch::Tensor want, torch::Tensor offsets,
    torch::Tensor ids, torch::Tensor probes, int64_t k, int64_t valid_n,
    int64_t tail_lo, int64_t tail_hi, int64_t max_list_len) {
  // ivf_scan_topk_filtered's contract through the list-major kernel.
  return ivf_scan_topk_batched_impl<true>(
      queries, segments, offsets, ids, probes, k, valid_n, tail_lo, tail_hi,
      max_list_len, ivf_filter(segments, labels, want, queries));
}

std::tuple<torch::Tensor, torch::Tensor> ivf_search(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    torch::Tensor centroids, torch::Tensor offsets, torch::Tensor ids,
    int64_t nprobe, int64_t k, int64_t valid_n, int64_t n_indexed,
    int64_t max_list_len) {
  return ivf_search_impl<false>(false, queries, segments, {}, centroids, offsets,
                                ids, nprobe, k, valid_n, n_indexed, max_list_len);
}

std::tuple<torch::Tensor, torch::Tensor> ivf_search_batched(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    torch::Tensor centroids, torch::Tensor offsets, torch::Tensor ids,
    int64_t nprobe, int64_t k, int64_t valid_n, int64_t n_indexed,
    int64_t max_list_len) {
  return ivf_search_impl<false>(true, queries, segments, {}, centroids, offsets,
                                ids, nprobe, k, valid_n, n_indexed, max_list_len);
}

std::tuple<torch::Tensor, torch::Tensor> ivf_search_filtered(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    std::vector<torch::Tensor> labels, torch::Tensor want,
    torch::Tensor centroids, torch::Tensor offsets, torch::Tensor ids,
    int64_t nprobe, int64_t k, int64_t valid_n, int64_t n_indexed,
    int64_t max_list_len) {
  return ivf_search_impl<true>(false, queries, segments,
                               ivf_filter(segments, labels, want, queries),
                               centroids, offsets, ids, nprobe, k, valid_n,
                               n_indexed, max_list_len);
}

std::tuple<torch::Tensor, torch::Tensor> ivf_search_batched_filtered(
    torch::Tensor queries, std::vector<torch::Tensor> segments,
    std::vector<torch::Tensor> labels, torch::Tensor want,
    torch::Tensor centroids, torch::Tensor offsets, torch::Tensor ids,
    int64_t nprobe, int64_t k, int64_t valid_n, int64_t n_indexed,
    int64_t max_list_len) {
  return ivf_search_impl<true>(true, queries, segments,
                               ivf_filter(segments, labels, want, queries),
                               centroids, offsets, ids, nprobe, k, valid_n,
                               n_indexed, max_list_len);
}

// ---- device featurizer ------------------------------------------------------

std::vector<torch::Tensor> featurize_bytes(torch::Tensor buf, torch::Tensor offsets,
                                           int64_t hash_dim, uint64_t start_state,
                                           int64_t max_features) {
  // Signature texts as bytes (all texts back to back in `buf`, text b being
  // buf[offsets[b]:offsets[b+1]]) -> {idx i32 [B, max_features], w f32
  // [B, max_features], status i32 [B], flagged i32 [1]}: the rows of
  // featurize_batch (featurize_plan.h states the contract), a zero row and
  // a non-zero status where a text is over capacity or has more than
  // max_features buckets, and the number of such rows.
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == torch::kUInt8 &&
                  buf.dim() == 1 && buf.is_contiguous(),
              "buf must be contiguous 1-D u8 on GPU");
  TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == torch::kInt32 &&
                  offsets.dim() == 1 && offsets.is_contiguous() &&
                  offsets.size(0) >= 1 && offsets.device() == buf.device(),
              "offsets must be contiguous 1-D i32 with B+1 entries on buf's device");
  TORCH_CHECK(hash_dim >= 1 && hash_dim < (int64_t)1 << 31,
              "hash_dim must be in [1, 2^31)");
  TORCH_CHECK(max_features >= 1 && max_features <= FEATURIZE_MAX_FEATURES,
              "max_features must be in [1,", FEATURIZE_MAX_FEATURES, "]");
  const int64_t B = offsets.size(0) - 1;
  auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(buf.device());
  auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(buf.device());
  auto idx = torch::empty({B, max_features}, i32);
  auto w = torch::empty({B, max_features}, f32);
  auto status = torch::empty({B}, i32);
  auto flagged = torch::zeros({1}, i32);
  if (B == 0) return {idx, w, status, flagged};  // nothing to launch
  const int64_t blocks =
      (B + FEATURIZE_TEXTS_PER_BLOCK - 1) / FEATURIZE_TEXTS_PER_BLOCK;
  hipLaunchKernelGGL(featurize_bytes_kernel, dim3((unsigned)blocks),
                     dim3(64 * FEATURIZE_TEXTS_PER_BLOCK), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     (const unsigned char*)buf.data_ptr(), (long)buf.size(0),
                     offsets.data_ptr<int>(), (int)B, (unsigned)hash_dim,
                     (unsigned long long)start_state, (int)max_features,
                     idx.data_ptr<int>(), w.data_ptr<float>(),
                     status.data_ptr<int>(), flagged.data_ptr<int>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {idx, w, status, flagged};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("cosine_topk", &cosine_topk, "fused cosine top-k (MFMA + LDS top-k)");
  m.def("cosine_topk_filtered", &cosine_topk_filtered,
        "cosine top-k over the corpus rows whose label matches each query's");
  m.def("quantize_rows_q8", &quantize_rows_q8,
        "quantise bf16 rows into the int8 mirror (codes, (scale, err))",
        pybind11::arg("rows"), pybind11::arg("out_codes"),
        pybind11::arg("out_meta"), pybind11::arg("first_row"),
        pybind11::arg("cnorm") = pybind11::none());
  m.def("cosine_topk_q8", &cosine_topk_q8,
        "exact top-k over the int8 mirror: int8 scan or screen + bf16 rescore",
        pybind11::arg("queries"), pybind11::arg("corpus"), pybind11::arg("codes"),
        pybind11::arg("meta"), pybind11::arg("k"), pybind11::arg("valid_n"),
        pybind11::arg("labels") = pybind11::none(),
        pybind11::arg("want") = pybind11::none(),
        pybind11::arg("cnorm") = pybind11::none(),
        pybind11::arg("batch_min_b") = (int64_t)0,
        pybind11::arg("cap") = (int64_t)0, pybind11::arg("stages") = (int64_t)0);
  m.def("cosine_topk_wide", &cosine_topk_wide,
        "exact top-k for KMAX < k <= KWIDE_MAX: floors, emission, wide selection",
        pybind11::arg("queries"), pybind11::arg("corpus"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("labels") = pybind11::none(),
        pybind11::arg("want") = pybind11::none(),
        pybind11::arg("cap") = (int64_t)0, pybind11::arg("seg") = (int64_t)0);
  m.def("wide_counts_probe", &wide_counts_probe,
        "cosine_topk_wide plus the candidates per query of its first pass",
        pybind11::arg("queries"), pybind11::arg("corpus"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("labels") = pybind11::none(),
        pybind11::arg("want") = pybind11::none(),
        pybind11::arg("cap") = (int64_t)0, pybind11::arg("seg") = (int64_t)0);
  m.attr("KWIDE_MAX") = KWIDE_MAX;
  m.def("q8_stage_plan", &q8_stage_plan_op,
        "stage plan of the batched int8 screen: tile bounds and chunkings",
        pybind11::arg("B"), pybind11::arg("N"), pybind11::arg("k"),
        pybind11::arg("stages") = (int64_t)0);
  m.def("q8_screen_probe", &q8_screen_probe,
        "batched int8 screen: candidate lists before and after the rescore",
        pybind11::arg("queries"), pybind11::arg("corpus"), pybind11::arg("codes"),
        pybind11::arg("meta"), pybind11::arg("cnorm"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("cap") = (int64_t)0);
  m.def("q8_counts_probe", &q8_counts_probe,
        "stage-1 candidate counts of the int8 and the bf16 arm",
        pybind11::arg("queries"), pybind11::arg("corpus"), pybind11::arg("codes"),
        pybind11::arg("meta"), pybind11::arg("k"), pybind11::arg("valid_n"),
        pybind11::arg("labels") = pybind11::none(),
        pybind11::arg("want") = pybind11::none());
  m.def("l2normalize_", &l2normalize_, "in-place row L2 normalisation");
  m.def("embedding_bag", &embedding_bag, "weighted embedding bag");
  m.def("kmeans_update", &kmeans_update, "segmented centroid sum + counts");
  m.def("kmeans_assign", &kmeans_assign,
        "argmax-cosine assignment, LDS-resident centroids (C<=64)");
  m.def("probe8p", &probe8p, "8p epilogue-isolation timing probe");
  m.def("probe8p_i8", &probe8p_i8, "int8 screen epilogue-isolation timing probe",
        pybind11::arg("queries"), pybind11::arg("codes"), pybind11::arg("meta"),
        pybind11::arg("mode"), pybind11::arg("iters"));
  m.def("floor_probe", &floor_probe, "emission floor pipeline debug probe",
        pybind11::arg("queries"), pybind11::arg("corpus"),
        pybind11::arg("pregq"), pybind11::arg("k") = (int64_t)KMAX,
        pybind11::arg("pre_tiles") = (int64_t)0);
  m.def("emit_counts_probe", &emit_counts_probe,
        "emission per-row count debug probe", pybind11::arg("queries"),
        pybind11::arg("corpus"), pybind11::arg("pregq"),
        pybind11::arg("k") = (int64_t)KMAX,
        pybind11::arg("pre_tiles") = (int64_t)0);
  m.def("ivf_route_scores", &ivf_route_scores_op,
        "dense fp32 scores of queries against IVF centroids");
  m.def("ivf_scan_topk", &ivf_scan_topk,
        "exact top-k over probed inverted lists plus a contiguous tail",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("offsets"), pybind11::arg("ids"), pybind11::arg("probes"),
        pybind11::arg("k"), pybind11::arg("valid_n"), pybind11::arg("tail_lo"),
        pybind11::arg("tail_hi"), pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_search", &ivf_search, "cluster-routed (IVF) top-k search",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("centroids"), pybind11::arg("offsets"),
        pybind11::arg("ids"), pybind11::arg("nprobe"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("n_indexed"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_group_probes", &ivf_group_probes_op,
        "group (query, probe) pairs by list into tiles of IVF_BATCH_QTILE",
        pybind11::arg("probes"), pybind11::arg("n_lists"));
  m.def("ivf_scan_topk_batched", &ivf_scan_topk_batched,
        "ivf_scan_topk through the list-major MFMA scan",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("offsets"), pybind11::arg("ids"), pybind11::arg("probes"),
        pybind11::arg("k"), pybind11::arg("valid_n"), pybind11::arg("tail_lo"),
        pybind11::arg("tail_hi"), pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_search_batched", &ivf_search_batched,
        "cluster-routed (IVF) top-k search through the list-major MFMA scan",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("centroids"), pybind11::arg("offsets"),
        pybind11::arg("ids"), pybind11::arg("nprobe"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("n_indexed"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_scan_topk_filtered", &ivf_scan_topk_filtered,
        "ivf_scan_topk over the rows whose label matches each query's",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("labels"), pybind11::arg("want"),
        pybind11::arg("offsets"), pybind11::arg("ids"), pybind11::arg("probes"),
        pybind11::arg("k"), pybind11::arg("valid_n"), pybind11::arg("tail_lo"),
        pybind11::arg("tail_hi"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_scan_topk_batched_filtered", &ivf_scan_topk_batched_filtered,
        "ivf_scan_topk_filtered through the list-major MFMA scan",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("labels"), pybind11::arg("want"),
        pybind11::arg("offsets"), pybind11::arg("ids"), pybind11::arg("probes"),
        pybind11::arg("k"), pybind11::arg("valid_n"), pybind11::arg("tail_lo"),
        pybind11::arg("tail_hi"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_search_filtered", &ivf_search_filtered,
        "cluster-routed (IVF) top-k search over the rows of each query's label",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("labels"), pybind11::arg("want"),
        pybind11::arg("centroids"), pybind11::arg("offsets"),
        pybind11::arg("ids"), pybind11::arg("nprobe"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("n_indexed"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("ivf_search_batched_filtered", &ivf_search_batched_filtered,
        "ivf_search_filtered through the list-major MFMA scan",
        pybind11::arg("queries"), pybind11::arg("segments"),
        pybind11::arg("labels"), pybind11::arg("want"),
        pybind11::arg("centroids"), pybind11::arg("offsets"),
        pybind11::arg("ids"), pybind11::arg("nprobe"), pybind11::arg("k"),
        pybind11::arg("valid_n"), pybind11::arg("n_indexed"),
        pybind11::arg("max_list_len") = (int64_t)0);
  m.def("featurize_bytes", &featurize_bytes,
        "hash signature-text bytes into padded n-gram feature rows",
        pybind11::arg("buf"), pybind11::arg("offsets"), pybind11::arg("hash_dim"),
        pybind11::arg("start_state"), pybind11::arg("max_features"));
  m.attr("FEATURIZE_MAX_BYTES") = FEATURIZE_MAX_BYTES;
  m.attr("FEATURIZE_MAX_GRAMS") = FEATURIZE_MAX_GRAMS;
  m.attr("FEATURIZE_TEXTS_PER_BLOCK") = FEATURIZE_TEXTS_PER_BLOCK;
  m.attr("KMAX") = KMAX;
  m.attr("IVF_BATCH_QTILE") = IVF_BATCH_QTILE;
  m.attr("IVF_BATCH_MAX_D") = IVF_BATCH_MAX_D;
  // the widest row the C<=64 assignment kernel can keep resident in LDS
  m.attr("KMEANS_ASSIGN_MAX_D") = kmeans_assign_max_d();
}
