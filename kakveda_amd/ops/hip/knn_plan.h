// Host-side dispatch plan for cosine_topk: which kernels run, with what
// geometry, for a given (B, N, k) and the KAKVEDA_KNN_* environment.
// Pure C++ (no HIP, no torch) so the whole decision table is checked on
// the CPU (tests/host/knn_plan_test.cpp).
#pragma once

#include <algorithm>
#include <cmath>
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
  bool skip_sample = true;       // KAKVEDA_KNN_SKIP_SAMPLE: 1 (default), 0
  int pre_tiles = 0;             // KAKVEDA_KNN_PRE_TILES (0: the plan's rule)
  bool q8_batch = true;          // KAKVEDA_Q8_BATCH: 1 (default), 0
  int q8_stages = 0;             // KAKVEDA_Q8_STAGES (0: the plan's rule)
};

// A forced size of the compact prepass's blocks, in column tiles (the
// KAKVEDA_KNN_PRE_TILES knob and the probes' pre_tiles argument): a positive
// multiple of PRE_TILES. Whether it divides a given sample is checked where
// the sample is known (forced_pre_grid below).
inline bool pre_tiles_wellformed(long t) {
  return t >= PRE_TILES && t <= (1L << 24) && t % PRE_TILES == 0;
}

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
  v = get("KAKVEDA_KNN_SKIP_SAMPLE");
  const std::string sk = v ? v : "";
  if (sk == "0") e.skip_sample = false;
  else if (!sk.empty() && sk != "1")
    throw std::runtime_error("KAKVEDA_KNN_SKIP_SAMPLE='" + sk +
                             "' is not a setting; accepted: 1 (default: the "
                             "emission main launch starts after the sampled "
                             "columns), 0 (it scans the whole corpus)");
  v = get("KAKVEDA_KNN_PRE_TILES");
  const std::string pt = v ? v : "";
  if (!pt.empty()) {
    char* end = nullptr;
    const long t = std::strtol(pt.c_str(), &end, 10);
    if (pt.find_first_not_of("0123456789") != std::string::npos ||
        pt.size() > 8 || *end != '\0' || !pre_tiles_wellformed(t))
      throw std::runtime_error(
          "KAKVEDA_KNN_PRE_TILES='" + pt +
          "' is not a setting; accepted: a positive multiple of " +
          std::to_string(PRE_TILES) +
          " (column tiles per block of the emission prepass; " +
          std::to_string(PRE_TILES) +
          " is one block per sampled chunk), or unset for the plan's rule");
    e.pre_tiles = (int)t;
  }
  v = get("KAKVEDA_Q8_BATCH");
  const std::string qb = v ? v : "";
  if (qb == "0") e.q8_batch = false;
  else if (!qb.empty() && qb != "1")
    throw std::runtime_error("KAKVEDA_Q8_BATCH='" + qb +
                             "' is not a setting; accepted: 1 (default: "
                             "cosine_topk_q8 screens batches with int8), 0 (it "
                             "answers them with the bf16 search)");
  v = get("KAKVEDA_Q8_STAGES");
  const std::string qs = v ? v : "";
  if (qs == "1" || qs == "2" || qs == "3" || qs == "4") e.q8_stages = qs[0] - '0';
  else if (!qs.empty())
    throw std::runtime_error("KAKVEDA_Q8_STAGES='" + qs +
                             "' is not a setting; accepted: 1 (the batched int8 "
                             "screen runs one main launch), 2, 3, 4 (it "
                             "refreshes its floors between that many stages), "
                             "or unset for the plan's rule");
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

// The same geometry over `ntiles` column tiles.
inline Chunking chunking_tiles(int row_tiles, int ntiles, long target) {
  Chunking c;
  c.row_tiles = row_tiles;
  c.ntiles = ntiles;
  const long want = ((long)c.ntiles * c.row_tiles + target - 1) / target;
  c.chunk_tiles = (int)std::max(4L, std::min(want, 128L));
  // pad the chunk count to a multiple of 8 so the in-kernel XCD remap is
  // bijective; padded chunks have no tiles and emit -inf partials.
  c.nchunks = ((c.ntiles + c.chunk_tiles - 1) / c.chunk_tiles + 7) & ~7;
  return c;
}

inline Chunking chunking(int B, int N, int tile, long target) {
  return chunking_tiles((B + tile - 1) / tile, (N + tile - 1) / tile, target);
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
  // The Emit8p main launch as it is launched (main_geometry below). Under
  // every other main kernel: skip_tiles 0, mch == ch, mseg == seg.
  int skip_tiles;  // leading BN8-column tiles left to the prepass sample
  Chunking mch;    // chunking of the other ntiles - skip_tiles tiles
  long mseg;       // records per block segment of that launch
  // The prepass as it is launched (prepass_geometry below): pre_grid blocks
  // per row tile of pre_tiles column tiles each, over the same sample:
  // pre_grid * pre_tiles == preg * PRE_TILES. preg x PRE_TILES unless the
  // prepass is the compact one.
  int pre_grid;
  int pre_tiles;
};

// Makespan model of an 8-phase main launch, in column tiles per CU. The
// kernel runs one block per CU (its LDS), 32 CUs per XCD, and hands each XCD
// nchunks / 8 consecutive chunks times every row tile (its XCD remap; a grid
// under 256 blocks is dealt round-robin, which spreads chunks the same way).
// nchunks is the real chunk count R rounded up to 8, so fewer than 8 chunks
// are padding and the busiest XCD has ceil(R / 8) real chunks wherever the
// padding falls: it runs ceil(ceil(R / 8) * row_tiles / 32) rounds of
// chunk_tiles tiles. The ideal is ntiles * row_tiles / 256.
inline long model_makespan(const Chunking& c) {
  if (c.ntiles <= 0) return 0;
  const long real = (c.ntiles + c.chunk_tiles - 1) / c.chunk_tiles;
  const long per_xcd = (real + 7) / 8 * c.row_tiles;
  return (long)c.chunk_tiles * ((per_xcd + 31) / 32);
}

// Chunking of the emission main launch over `ntiles` tiles: the chunk size
// in [4, 128] (the record's 15-bit column field caps it) with the smallest
// modelled makespan, so that the last round of blocks is as full as the
// tile count allows. Above ~4M rows the 128 cap, not the target, used to
// decide the block count, and the grid ended in a partly filled round (10M
// x 2048: 312 chunks of 128 = 10 rounds of 128 tiles where 320 chunks of
// 119 are 10 rounds of 119). The search starts at half the chunk size the
// target rule gives (`from` is that rule's chunking of these tiles, `whole`
// the whole-corpus chunking), which bounds the per-block cost the model
// leaves out (prologue, pipeline fill, tail drain: well under one tile);
// both rule sizes are candidates, so the result never models slower than
// either. Ties go to the larger chunk.
inline Chunking balanced_chunking(const Chunking& from, const Chunking& whole) {
  Chunking best = from;
  if (from.ntiles <= 0) return best;
  const int lo = std::max(4, std::min(from.chunk_tiles, whole.chunk_tiles) / 2);
  for (int ct = lo; ct <= 128; ++ct) {
    Chunking c = from;
    c.chunk_tiles = ct;
    c.nchunks = ((c.ntiles + ct - 1) / ct + 7) & ~7;
    const long m = model_makespan(c), b = model_makespan(best);
    if (m < b || (m == b && ct > best.chunk_tiles)) best = c;
  }
  return best;
}

// Main launch geometry of the unfiltered Emit8p plan. The prepass has
// already scored the first preg * PRE_TILES * BN columns, its scores are
// bit-equal to the 8-phase kernel's, and the exact top-KMAX of that sample
// (samp_s/samp_i, whose KMAX-th is the emission floor) is in hand. For
// k <= KMAX the corpus top-k lies in (top-KMAX of the sample) U (unsampled
// columns scoring >= floor), so the main launch starts at the first
// unsampled tile and the host seeds the candidate lists from the sample.
// The remaining tiles are chunked into whole rounds of blocks
// (balanced_chunking above) and the segments are sized from that geometry
// (emit_seg_cap: never more bytes than the candidate buffer).
// Nothing is skipped
//   - when the sample covers the corpus (N <= preg * 1024): the main launch
//     would have nothing left, and with it the record segments, emit_bin and
//     their overflow fallback would leave the path of every request that
//     small; those stay on the whole-corpus launch, second scan included
//     (dropping that launch is left open);
//   - under SmallB: the streaming kernels sum in another order, so their
//     score of a sampled column is not bit-equal to the prepass's (a column
//     could be seeded and emitted, or miss both, at the floor);
//   - on the filtered path, which has no 8-phase kernel;
//   - without a prepass, or with KAKVEDA_KNN_SKIP_SAMPLE=0, which restores
//     the whole-corpus scan over p.ch.
// No field above these three changes with any of this.
inline void main_geometry(KnnPlan& p, int B, const KnnEnv& env) {
  p.skip_tiles = 0;
  p.mch = p.ch;
  p.mseg = p.seg;
  if (p.main != MainKernel::Emit8p || !p.prepass || !env.skip_sample) return;
  const int sampled = p.preg * (PRE_TILES * BN / BN8);
  if (sampled >= p.ch.ntiles) return;
  p.skip_tiles = sampled;
  p.mch = balanced_chunking(
      chunking_tiles(p.ch.row_tiles, p.ch.ntiles - p.skip_tiles,
                     env.target > 0 ? env.target : default_target(BM8)),
      p.ch);
  p.mseg = emit_seg_cap(B, env.cap, p.mch, env.seg);
}

// ---------------------------------------------------------------------------
// Stage plan of the batched int8 screen (kakveda_kernels.hip run_q8_screen).
//
// The screen's floors come from the prepass sample, a prefix of S columns;
// a floor taken from a prefix of P columns lets about k * (N - P) / P of the
// other columns through. The main launch over [skip_tiles, ntiles) is
// therefore cut into n stages [first[i], first[i + 1]) and the floors are
// refreshed between them from the exact scores found so far, so stage i
// screens against a floor taken from the prefix first[i]. With boundaries
// geometric in the prefix, first[i] ~ P0 * (ntiles / P0)^(i / n), every stage
// lets the same share through and the candidates fall from (N - P0) / P0 to
// n * ((N / P0)^(1 / n) - 1) in units of k (stage_model_count): 37 -> 10.4 ->
// 7.1 -> 5.9 for n = 1..4 at N / P0 = 38, the bench shape.
//
// P0 is skip_tiles, or the sample's tile count when nothing is skipped. Where
// that leaves no room (the sample covers the corpus) the stages split
// [0, ntiles) evenly. Each stage is chunked like the single launch, by
// balanced_chunking over its own tiles, and each interior boundary is moved
// by up to 1/64 of its value to where the stage to its right wastes the
// fewest block slots in its last round (right to left: the last stage is the
// longest, the first takes the remainder).
//
// n: `stages` > 0 forces it (KAKVEDA_Q8_STAGES, the op's argument), clamped to
// Q8_MAX_STAGES and to one tile per stage; 0 asks for Q8_STAGES_DEFAULT,
// reduced while the shortest stage is less than one full round of 256 blocks
// of 4 tiles (Q8_STAGE_MIN_WORK tile-blocks): below that a stage cannot fill
// the GPU once, and its boundary costs a drained GPU and four small launches.
// n = 1 is the single launch over p.mch, field for field.
// Measured (profiles/q8_staged_floors.md, 10M x 768, B = 2048, k = 5): 26.16,
// 20.76, 20.31 and 19.94 ms a bench step for n = 1..4, 2,150 -> 289 candidates
// a row at n = 4, hence the default; n = 4 also wins on the 2.5M and 1.25M
// shards, whose shortest stages are 3,376 and 2,200 tile-blocks. The
// Q8_STAGE_MIN_WORK floor itself is the reasoning above, not a measurement.
// ---------------------------------------------------------------------------
constexpr int Q8_MAX_STAGES = 4;
constexpr int Q8_STAGES_DEFAULT = 4;
constexpr long Q8_STAGE_MIN_WORK = 256L * 4;

struct StagePlan {
  int n;
  int prefix;                    // P0, in column tiles
  int first[Q8_MAX_STAGES + 1];  // stage i scans tiles [first[i], first[i+1])
  Chunking ch[Q8_MAX_STAGES];
};

// Interior boundary i of n before any nudge (see above).
inline int stage_boundary(int hi, int prefix, int i, int n) {
  if (prefix >= hi) return (int)((long)hi * i / n);
  return (int)std::lround(prefix * std::pow((double)hi / prefix, (double)i / n));
}

inline StagePlan plan_q8_stages(const KnnPlan& p, const KnnEnv& env, int stages) {
  const int lo = p.skip_tiles, hi = p.ch.ntiles;
  const int sampled = p.preg * (PRE_TILES * BN / BN8);
  StagePlan s{};
  s.prefix = std::max(1, lo > 0 ? lo : sampled);
  int n = stages > 0 ? std::min(stages, Q8_MAX_STAGES) : Q8_STAGES_DEFAULT;
  n = std::max(1, std::min(n, hi - lo));
  if (stages <= 0)
    while (n > 1 && (long)(stage_boundary(hi, s.prefix, 1, n) - lo) *
                            p.ch.row_tiles < Q8_STAGE_MIN_WORK)
      --n;
  s.n = n;
  s.first[0] = lo;
  s.first[n] = hi;
  if (n == 1) {
    s.ch[0] = p.mch;
    return s;
  }
  const long target = env.target > 0 ? env.target : default_target(BM8);
  auto stage_chunking = [&](int tiles) {
    return balanced_chunking(chunking_tiles(p.ch.row_tiles, tiles, target), p.ch);
  };
  for (int i = n - 1; i >= 1; --i) {
    const int next = s.first[i + 1];
    // stages 0..i-1 and stage i keep at least one tile each
    const int tmin = lo + i, tmax = next - 1;
    const int g = std::max(tmin, std::min(stage_boundary(hi, s.prefix, i, n), tmax));
    const int w = g / 64;
    int best = g;
    long best_waste = -1;
    for (int t = std::max(tmin, g - w); t <= std::min(tmax, g + w); ++t) {
      const long waste = model_makespan(stage_chunking(next - t)) * 256 -
                         (long)(next - t) * p.ch.row_tiles;
      if (best_waste < 0 || waste < best_waste ||
          (waste == best_waste && std::abs(t - g) < std::abs(best - g))) {
        best = t;
        best_waste = waste;
      }
    }
    s.first[i] = best;
  }
  for (int i = 0; i < n; ++i) s.ch[i] = stage_chunking(s.first[i + 1] - s.first[i]);
  return s;
}

// Modelled candidates per row in units of the floor depth k: stage i lets
// (its columns) / (the prefix its floors were taken from) through.
inline double stage_model_count(const StagePlan& s) {
  double c = 0.0;
  for (int i = 0; i < s.n; ++i)
    c += (double)(s.first[i + 1] - s.first[i]) /
         (double)(i == 0 ? s.prefix : s.first[i]);
  return c;
}

// Blocks of the 128x128 kernel resident at once: 2 per CU (its 80 KiB of
// LDS), 256 CUs.
constexpr int PREPASS_ROUND = 2 * 256;

// grid.x of a compact prepass forced to `pre_tiles` column tiles per block
// over a sample of preg * PRE_TILES tiles. The size must be well formed,
// divide the sample, and leave a grid that is a multiple of 8 (the in-kernel
// XCD remap is bijective only then) unless it is PRE_TILES itself, the
// launch of one block per sampled chunk.
inline int forced_pre_grid(int preg, long pre_tiles, const char* what) {
  const long total = (long)preg * PRE_TILES;
  if (pre_tiles_wellformed(pre_tiles) && total % pre_tiles == 0 &&
      (pre_tiles == PRE_TILES || (total / pre_tiles) % 8 == 0))
    return (int)(total / pre_tiles);
  throw std::runtime_error(
      std::string(what) + "=" + std::to_string(pre_tiles) +
      " does not fit this request's prepass sample of " +
      std::to_string(total) + " column tiles; accepted: a multiple of " +
      std::to_string(PRE_TILES) +
      " that divides the sample into a multiple of 8 blocks per row tile (" +
      std::to_string(PRE_TILES) + " always fits)");
}

// Launch geometry of the prepass. The sample is preg * PRE_TILES column
// tiles whatever the geometry; a column's score depends only on the K order
// inside its tile, so the sample's exact top-KMAX is the same under any
// split of the sample into blocks.
// Every block bootstraps private top-KMAX lists from empty, through the
// serial insert path, before its thresholds prune anything: a streaming
// top-8 over n columns takes about 8 (1 + ln(n / 8)) inserts, so per query
// row 256 blocks of 8 tiles pay ~21,000 inserts where 32 blocks of 64 tiles
// pay ~3,700. The result needs one top-8 of the sample per row, so the
// COMPACT prepass (the emission floors: it writes a buffer of its own with
// stride pre_grid, and the floor merge shrinks with it) runs the longest
// blocks, in doublings of PRE_TILES, that still
//   - divide the sample,
//   - leave grid.x a multiple of 8 (the in-kernel XCD remap),
//   - fill one whole round of resident blocks (PREPASS_ROUND) with
//     pre_grid * ceil(B / BM) blocks.
// Where no longer block qualifies (B <= 8 serving, B = 256, every filtered
// small-batch plan) the geometry is preg x PRE_TILES. The warming prepass of
// the list path always is: it writes the main launch's [row][chunk_id]
// partial slots. KAKVEDA_KNN_PRE_TILES forces the compact prepass's size
// (forced_pre_grid: a request it does not fit is refused) and acts on
// nothing else. No field above these two changes with any of this.
inline void prepass_geometry(KnnPlan& p, int B, const KnnEnv& env) {
  p.pre_grid = p.preg;
  p.pre_tiles = PRE_TILES;
  if (!p.prepass_compact) return;
  if (env.pre_tiles > 0) {
    p.pre_grid = forced_pre_grid(p.preg, env.pre_tiles, "KAKVEDA_KNN_PRE_TILES");
    p.pre_tiles = env.pre_tiles;
    return;
  }
  const long total = (long)p.preg * PRE_TILES;
  const long row_tiles = ((long)B + BM - 1) / BM;
  for (long t = 2 * PRE_TILES; total % t == 0; t *= 2) {
    const long g = total / t;
    if (g % 8 != 0 || g * row_tiles < PREPASS_ROUND) break;
    p.pre_grid = (int)g;
    p.pre_tiles = (int)t;
  }
}

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
  main_geometry(p, B, env);  // skips nothing: no 8-phase kernel here
  prepass_geometry(p, B, env);
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
  main_geometry(p, B, env);
  prepass_geometry(p, B, env);
  return p;
}

}  // namespace kakveda
