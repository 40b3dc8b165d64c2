// Host-side dispatch plan for cosine_topk: which kernels run, with what
// geometry, for a given (B, N, k) and the KAKVEDA_KNN_* environment.
// Pure C++ (no HIP, no torch) so the whole decision table is checked on
// the CPU (tests/host/knn_plan_test.cpp).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace kakveda {

constexpr int BM = 128;   // query rows per block, 128x128 kernels
constexpr int BN = 128;   // corpus cols per tile, 128x128 kernels
constexpr int BM8 = 256;  // 256x256 8-phase kernels
constexpr int BN8 = 256;
constexpr int KMAX = 8;       // top-k list capacity per row
constexpr int PRE_TILES = 8;  // column tiles each prepass block samples
// prepass grid.x (sampled chunks): threshold warming, and the 4x wider
// sample behind the emission floors
constexpr int PREG_WARM = 64;
constexpr int PREG_EMIT = 256;

// Selection thresholds (corpus columns / query rows).
constexpr int MIN_N_8P = 4096;     // 256x256 tiles need a corpus this big
constexpr int MIN_N_EMIT = 65536;  // emission needs a prepass-sized corpus
constexpr int SMALLB_MAX = 8;      // streaming small-batch kernel, B <= 8

enum class KnnSel { Default, List, Eager, Rege, Fast, Bl8p, Emit, Emit2 };

struct KnnEnv {
  KnnSel sel = KnnSel::Default;  // KAKVEDA_KNN_KERNEL
  bool smallb_v2 = false;        // KAKVEDA_SMALLB=2
  int prepass = -1;              // KAKVEDA_KNN_PREPASS: -1 unset, 0 off, 1 on
  int preg = 0;                  // KAKVEDA_KNN_PREG (<= 0: default)
  long target = 0;               // KAKVEDA_KNN_TARGET (<= 0: default)
  long cap = 32768;              // KAKVEDA_KNN_EMIT_CAP
  long seg = 0;                  // KAKVEDA_KNN_EMIT_SEG (<= 0: default)
  bool emit_debug = false;       // KAKVEDA_KNN_EMIT_DEBUG=1
};

// `get` is std::getenv or anything with its signature.
template <class GetEnv>
KnnEnv parse_knn_env(GetEnv&& get) {
  KnnEnv e;
  const char* v = get("KAKVEDA_KNN_KERNEL");
  const std::string s = v ? v : "";
  if (s.empty()) e.sel = KnnSel::Default;
  else if (s == "list") e.sel = KnnSel::List;
  else if (s == "eager") e.sel = KnnSel::Eager;
  else if (s == "rege") e.sel = KnnSel::Rege;
  else if (s == "fast") e.sel = KnnSel::Fast;
  else if (s == "8pbl") e.sel = KnnSel::Bl8p;
  else if (s == "8pe") e.sel = KnnSel::Emit;
  else if (s == "8pe2") e.sel = KnnSel::Emit2;
  else
    throw std::runtime_error(
        "KAKVEDA_KNN_KERNEL='" + s +
        "' is not a kernel selection; accepted: list, eager, rege, fast, "
        "8pbl, 8pe, 8pe2 (or unset for the default)");
  v = get("KAKVEDA_SMALLB");
  const std::string sb = v ? v : "";
  if (sb == "2") e.smallb_v2 = true;
  else if (!sb.empty() && sb != "4")
    throw std::runtime_error("KAKVEDA_SMALLB='" + sb +
                             "' is not a small-batch kernel; accepted: 4 "
                             "(default), 2");
  if ((v = get("KAKVEDA_KNN_PREPASS"))) e.prepass = v[0] == '1';
  if ((v = get("KAKVEDA_KNN_PREG"))) e.preg = (int)std::atol(v);
  if ((v = get("KAKVEDA_KNN_TARGET"))) e.target = std::atol(v);
  if ((v = get("KAKVEDA_KNN_EMIT_CAP"))) e.cap = std::atol(v);
  if ((v = get("KAKVEDA_KNN_EMIT_SEG"))) e.seg = std::atol(v);
  if ((v = get("KAKVEDA_KNN_EMIT_DEBUG"))) e.emit_debug = v[0] == '1';
  return e;
}

// Grid geometry of a main launch: grid = (nchunks, row_tiles), each block
// walks chunk_tiles column tiles.
struct Chunking {
  int row_tiles, ntiles, chunk_tiles, nchunks;
};

// Default block-count target: chunks are sized so the grid comfortably
// oversubscribes 256 CUs (2 blocks/CU at 128x128, 1 block/CU at 256x256).
constexpr long default_target(int tile) { return tile == BM8 ? 512 : 2048; }

inline Chunking chunking(int B, int N, int tile, long target) {
  Chunking c;
  c.row_tiles = (B + tile - 1) / tile;
  c.ntiles = (N + tile - 1) / tile;
  const long want = ((long)c.ntiles * c.row_tiles + target - 1) / target;
  c.chunk_tiles = (int)std::max(4L, std::min(want, 128L));
  // pad the chunk count to a multiple of 8 so the in-kernel XCD remap is
  // bijective; padded chunks have no tiles and emit -inf partials.
  c.nchunks = ((c.ntiles + c.chunk_tiles - 1) / c.chunk_tiles + 7) & ~7;
  return c;
}

// Emission record segments (8-phase emission main kernel): each block
// appends its 8-byte candidate records to a private segment of `seg`
// records; the binning kernel scatters them into the per-row candidate
// buffer. Default capacity: the bench shape (10M x 768, B = 2048, k = 5)
// measured 542 records in the fullest of its 2496 blocks (mean ~260), so
// 8192 is 15x headroom. The segments never take more memory than the
// candidate buffer beside them (both hold 8-byte entries):
// seg <= B * cap / blocks. An overflowed
// segment is not an error, it is the loud fallback (kernels_impl.h
// emit_bin). KAKVEDA_KNN_EMIT_SEG overrides the default.
constexpr long EMIT_SEG_DEFAULT = 8192;

inline long emit_seg_cap(int B, long cap, const Chunking& ch, long env_seg) {
  const long blocks = (long)ch.nchunks * ch.row_tiles;
  const long budget = std::max(1L, (long)B * std::max(cap, 0L) / blocks);
  const long want = env_seg > 0 ? env_seg : EMIT_SEG_DEFAULT;
  return std::max(1L, std::min(want, budget));
}

enum class MainKernel { List128, Argmax128, Stash8p, Emit8p, SmallB };
enum class MergeKernel { Small, Merge, Emit };

struct KnnPlan {
  MainKernel main;
  // EPI_MODE of the main kernel template (List128: 0/8/9/11, Argmax128: 4,
  // Stash8p: 6, Emit8p: 9/15); for SmallB the kernel version (4 or 2)
  int mode;
  int tile;  // 128 or 256
  Chunking ch;
  int preg;              // prepass grid.x (sampled chunks)
  bool prepass;          // run the threshold prepass
  int prepass_mode;      // cosine_topk_partial_t EPI_MODE the prepass runs
  bool prepass_compact;  // prepass writes its own [B][preg][KMAX] buffer
  long cap;              // emission candidates per row
  long seg;              // emission records per block segment (Emit8p)
  int smallb_blocks;     // SmallB grid.x
  MergeKernel merge;
};

// Every main launch and every prepass puts its row tiles on grid.y, which
// the device limits to MAX_GRID_Y blocks. The prepass runs the 128-row-tile
// kernel under either main tile, so it needs ceil(B / BM) rows of blocks
// whatever p.tile is. A plan that does not fit is refused by the caller
// before anything is allocated or launched: a launch over the limit fails
// without running, and its outputs would be returned uninitialised.
constexpr int MAX_GRID_Y = 65535;

inline bool plan_fits_grid(const KnnPlan& p, int B) {
  if (p.ch.row_tiles < 1 || p.ch.row_tiles > MAX_GRID_Y) return false;
  if (p.prepass && ((long)B + BM - 1) / BM > MAX_GRID_Y) return false;
  return true;
}

// Label-filtered search (cosine_topk_filtered). Only two kernels carry the
// filter: the streaming small-batch kernel (v4) and the 128x128 mode-11
// list kernel, which also runs every prepass. So the filtered table is
//   emission allowed, N >= MIN_N_EMIT, B <= SMALLB_MAX -> SmallB (4) + floors
//   everything else, k == 1 included                   -> List128 (11)
// on 128-row tiles throughout. KAKVEDA_KNN_KERNEL and KAKVEDA_SMALLB select
// nothing here (no other kernel applies the filter; parsing still rejects
// bad values); the geometry knobs (TARGET, PREG, PREPASS, EMIT_CAP) act as
// on the unfiltered path. The 8p core has no filtered epilogue.
inline KnnPlan plan_cosine_topk_filtered(int B, int N, int k, const KnnEnv& env,
                                         bool allow_emission) {
  KnnPlan p;
  const bool emit = allow_emission && N >= MIN_N_EMIT && B <= SMALLB_MAX;
  p.tile = BM;
  p.ch = chunking(B, N, BM, env.target > 0 ? env.target : default_target(BM));
  p.preg = std::min(env.preg > 0 ? env.preg : (emit ? PREG_EMIT : PREG_WARM), p.ch.nchunks) & ~7;
  p.prepass_mode = 11;
  const bool psmall = p.ch.ntiles <= p.preg * PRE_TILES * 32;
  p.prepass = (emit || (k > 1 && p.ch.ntiles >= p.preg * PRE_TILES &&
                        (env.prepass >= 0 ? env.prepass == 1 : psmall))) &&
              p.preg >= 8;
  p.prepass_compact = emit && p.prepass;
  p.cap = env.cap;
  p.seg = 0;  // no 8-phase kernel carries the filter
  p.smallb_blocks = (int)std::min((long)((N + 255) / 256), 8192L);
  p.main = emit ? MainKernel::SmallB : MainKernel::List128;
  p.mode = emit ? 4 : 11;
  p.merge = emit                          ? MergeKernel::Emit
            : p.ch.nchunks * KMAX <= 1024 ? MergeKernel::Small
                                          : MergeKernel::Merge;
  return p;
}

// allow_emission=false is the overflow fallback: the same request replanned
// without the emission path. filtered=true plans a label-filtered request
// (above); filtered=false is the unfiltered table, unchanged.
inline KnnPlan plan_cosine_topk(int B, int N, int k, const KnnEnv& env,
                                bool allow_emission, bool filtered = false) {
  if (filtered) return plan_cosine_topk_filtered(B, N, k, env, allow_emission);
  KnnPlan p;
  // Emission (8p GEMM core + threshold-emission epilogue + emit_merge_topk)
  // needs the prepass floors, so only for corpora big enough to carry one.
  // DEFAULT for every N >= 64k with k > 1; any explicit selection other
  // than 8pe/8pe2 disables it.
  const bool emit2 = env.sel == KnnSel::Emit2;
  const bool emit =
      (env.sel == KnnSel::Default ? k > 1 : env.sel == KnnSel::Emit || emit2) &&
      N >= MIN_N_EMIT && allow_emission;
  const bool bl8p = env.sel == KnnSel::Bl8p && N >= MIN_N_8P;
  const bool use8p = emit || bl8p;
  // 128x128 list epilogue: default EPI_MODE 11; eager -> 0, rege -> 8,
  // fast -> 9. The prepass has no mode-9 instantiation of its own: rege
  // and fast both sample with mode 8.
  const int epi = env.sel == KnnSel::Eager  ? 0
                  : env.sel == KnnSel::Rege ? 8
                  : env.sel == KnnSel::Fast ? 9
                                            : 11;
  p.prepass_mode = epi == 11 ? 11 : epi == 0 ? 0 : 8;

  p.tile = use8p ? BM8 : BM;
  p.ch = chunking(B, N, p.tile,
                  env.target > 0 ? env.target : default_target(p.tile));
  // emission floors tighten with sample size (E[emitted/row] ~ 8N/sample):
  // a 4x bigger prepass for the emission path. grid.x must stay <= nchunks
  // so every prepass block's partial slot [row][chunk_id] is in bounds.
  p.preg = std::min(env.preg > 0 ? env.preg : (emit ? PREG_EMIT : PREG_WARM), p.ch.nchunks) & ~7;
  // Pay the prepass only when the sample is a meaningful fraction of the
  // corpus (>= ~3%): below that its published floor is weaker than what
  // the main launch's own publishes converge to almost immediately
  // (measured: +14% at 1M entries, noise-negative at 10M).
  // KAKVEDA_KNN_PREPASS=0/1 forces it off/on. The emission path REQUIRES
  // it: its floors are the exact per-row emission thresholds.
  const bool psmall = p.ch.ntiles <= p.preg * PRE_TILES * 32;
  p.prepass = (emit || (!use8p && k > 1 && p.ch.ntiles >= p.preg * PRE_TILES &&
                        (env.prepass >= 0 ? env.prepass == 1 : psmall))) &&
              p.preg >= 8;
  p.prepass_compact = emit && p.prepass;
  p.cap = env.cap;
  p.seg = emit && B > SMALLB_MAX ? emit_seg_cap(B, env.cap, p.ch, env.seg) : 0;
  p.smallb_blocks = (int)std::min((long)((N + 255) / 256), 8192L);

  if (k == 1 && !use8p) {
    p.main = MainKernel::Argmax128;  // per-row argmax, no lists
    p.mode = 4;
  } else if (emit && B <= SMALLB_MAX) {
    // single-query serving skips the MFMA tile machinery: the streaming
    // kernel reads the corpus once with the same emission floors/merge
    p.main = MainKernel::SmallB;
    p.mode = env.smallb_v2 ? 2 : 4;
  } else if (emit) {
    p.main = MainKernel::Emit8p;
    p.mode = emit2 ? 15 : 9;
  } else if (bl8p) {
    p.main = MainKernel::Stash8p;
    p.mode = 6;
  } else {
    p.main = MainKernel::List128;
    p.mode = epi;
  }
  // few candidates per row: one thread per row beats the block-per-row
  // merge (whose thread-0 serial scan dominates at large B)
  p.merge = emit                             ? MergeKernel::Emit
            : p.ch.nchunks * KMAX <= 1024    ? MergeKernel::Small
                                             : MergeKernel::Merge;
  return p;
}

}  // namespace kakveda
