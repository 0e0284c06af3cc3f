// The host planner of the forward convolution: the settings hooks, the analytic plan (choose_plan), the plan cache and the
// autotuner, plan tables, and run_conv, the driver behind frcnn_conv2d_fwd and the data gradient.  It sees the kernels only
// as rows of the tile table (tile_cfg(i).tm / tn / wm / wn / wtm / wtn and the named rows) and launches through launch_gemm /
// launch_winograd / launch_splitk_epilogue.
#include "conv_common.h"

#include <algorithm>
#include <array>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace frcnn::conv;

// test / tuning hook: 0 = the autotuner may pick either form, 1 = implicit GEMM only, 2 = Winograd wherever it applies
std::atomic<int> frcnn::conv::g_algo_mode{0};   // atomic: set from one thread while another may launch
// test / tuning hook (frcnn_conv2d_set_algo bit 4): may the tuner try / forced Winograd use the fused input transform?
std::atomic<int> frcnn::conv::g_wino_fuse{1};
// test / tuning hook (frcnn_conv2d_set_algo bit 6): 1 = the convolution kernels store through the LDS transpose
std::atomic<int> frcnn::conv::g_epi_lds{1};
// test / tuning hook (frcnn_conv2d_set_algo bit 7): 1 = Winograd leaves out the components of partial tiles that feed only
// dropped outputs (wino_geom), 0 = every tile carries all 16 components
std::atomic<int> frcnn::conv::g_wino_trim{1};
// test / tuning hook: force the block tile (0 = automatic choice)
std::atomic<int> frcnn::conv::g_force_tm{0}, frcnn::conv::g_force_tn{0};
// tuning hook: 0 = register-staged kernels only, 1 = LDS-DMA kernel for the 8-wave tiles when C % 32 == 0
std::atomic<int> frcnn::conv::g_use_dma{1};
// test / timing hook (frcnn_conv2d_bf16_set_tile): 0 = bf16_small_tile's rule, 1 = 64x64, 2 = 128x128
std::atomic<int> frcnn::conv::g_bf16_tile{0};
// test hook (frcnn_conv2d_split_bf16_enable): 0 = frcnn_conv2d_split_bf16_wanted answers 0 everywhere
std::atomic<int> frcnn::conv::g_split_bf16{1};
// frcnn_conv2d_set_autotune: see the plan cache below
std::atomic<int> frcnn::conv::g_autotune{0};

namespace {
// ---- per-dispatch timing (frcnn_conv2d_profile_begin / _end) -----------------------------------------------------------
// While a profile is open every kernel of frcnn_conv2d_fwd is launched through hipExtLaunchKernelGGL with its own
// start / stop events: the pair brackets THAT dispatch on the launch stream (begin -> end of the kernel, the quantity
// rocprofv3 --kernel-trace reports), without the event-packet overhead two separately recorded events add around a
// launch.  bench.py's `roofline` is computed from these durations.
struct ProfRec {
  hipEvent_t e0, e1;
  int call, kind;      // frcnn_conv2d_fwd call number since profile_begin; kind 0 = main kernel, 1 = split-K second pass
};
std::vector<ProfRec> g_prof;
}  // namespace
std::atomic<bool> frcnn::conv::g_prof_on{false};
int frcnn::conv::g_prof_call = -1;

bool frcnn::conv::prof_events(int kind, hipEvent_t* e0, hipEvent_t* e1, hipStream_t stream) {
  if (!g_prof_on) return false;
  // a capturing stream cannot take the timed launch form (events would become graph nodes): plain launch, no record
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return false;
  if (hipEventCreate(e0) != hipSuccess) return false;
  if (hipEventCreate(e1) != hipSuccess) { (void)hipEventDestroy(*e0); return false; }
  g_prof.push_back(ProfRec{*e0, *e1, g_prof_call, kind});
  return true;
}

namespace {

// Pick the block tile and the K split that minimise the estimated time on 256 CUs.  Units: MFMA
// issue cycles of one SIMD (64 per v_mfma_f32_32x32x2_f32); a CU runs one workgroup's K-step in
// waves_per_simd * TM*TN*16 MFMAs (co-resident 4-wave workgroups share the SIMDs, which the model
// counts as running one after the other).
Plan choose_plan(int M, int K, int ksteps, int forced_splits) {
  static const int split_cand[] = {1, 2, 3, 4, 6, 8, 12, 16};
  Plan best{kTile128x128, 1, ksteps};
  double best_t = 1e300;
  for (int ci = 0; ci < kNumTiles; ++ci) {
    const TileCfg& c = tile_cfg(ci);
    if (g_force_tm > 0 && (c.tm != g_force_tm || c.tn != g_force_tn)) continue;
    const int bm = 64 * c.tm, bn = 64 * c.tn;
    const long tiles = (long)((M + bm - 1) / bm) * ((K + bn - 1) / bn);
    const int waves_per_simd = c.wm * c.wn / 4;
    for (int sp : split_cand) {
      if (forced_splits > 0 && sp != forced_splits) continue;
      if (forced_splits <= 0 && sp > 1 && ksteps / sp < 4) continue;
      const int sps = (ksteps + sp - 1) / sp;
      const int real_splits = (ksteps + sps - 1) / sps;
      if (real_splits != sp && forced_splits <= 0) continue;
      const long blocks = tiles * real_splits;
      const long rounds = (blocks + NUM_CU - 1) / NUM_CU;
      const double step_cyc = waves_per_simd * c.wtm * c.wtn * 16 * 64 + 300.0;
      double tcyc = rounds * (sps * step_cyc + 5000.0);
      if (real_splits > 1) {
        // slab write + read-back at ~3 TB/s (2.4 GHz -> 1250 B/cycle) + one more launch
        tcyc += (double)M * K * 4.0 * (real_splits + 1) / 1250.0 + 4000.0;
      }
      if (tcyc < best_t) {
        best_t = tcyc;
        best = Plan{ci, real_splits, sps};
      }
    }
  }
  if (forced_splits > 0 && best_t == 1e300) {
    const int sps = (ksteps + forced_splits - 1) / forced_splits;
    int ci = kTile64x64;
    for (int i = kNumTiles - 1; i >= 0; --i)   // first entry with the forced tile (index 6 repeats the 128x128 shape)
      if (g_force_tm > 0 && tile_cfg(i).tm == g_force_tm && tile_cfg(i).tn == g_force_tn) ci = i;
    best = Plan{ci, (ksteps + sps - 1) / sps, sps};
  }
  return best;
}

// ---- plan cache / autotuner -----------------------------------------------------------------------
// The analytic model above ranks (tile, split) pairs well for large GEMMs but not for the small, latency-bound
// layers (layer1..3 at one frame): there the 64x64 tile without a K split usually wins by 10-40 %.  With
// frcnn_conv2d_set_autotune(1) the first call of a shape outside stream capture times every candidate on the
// caller's own tensors (HIP events on the launch stream) and caches the winner; later calls — including the
// captured ones — look the plan up.  Off by default: results for split_k = 0 then depend only on the model.
typedef std::array<int, 10> ShapeKey;
std::map<ShapeKey, Plan> g_plan_cache;
std::mutex g_plan_mutex;
constexpr size_t kTuneWsCap = (size_t)256 << 20;   // candidates whose split-K slabs exceed this are not tried
constexpr size_t kTuneWinoCap = (size_t)768 << 20;  // same for the Winograd workspace (16 x (tiles x (C + K)) floats)

// workspace of a split-K plan: one M x k slab of partial sums per split
size_t splitk_ws_bytes(int splits, long M, int k) { return splits > 1 ? (size_t)splits * M * k * sizeof(float) : 0; }

// The last slot carries the output stride AND whether the call has a residual operand (+ kKeyResidual): a call with a
// residual cannot run as Winograd, so the two kinds of call of one shape are tuned and cached separately (a plan tuned for
// one used to push the other onto the untuned analytic plan for good).
constexpr int kKeyResidual = 256;
ShapeKey shape_key(int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int out_stride,
                   bool has_residual = false) {
  return ShapeKey{n, h, w, c, k, r, s, stride, pad, out_stride + (has_residual ? kKeyResidual : 0)};
}

std::vector<Plan> tune_candidates(long M, int k, int ksteps, bool allow_split) {
  static const int split_cand[] = {1, 2, 3, 4, 6, 8, 12, 16};
  std::vector<Plan> out;
  for (int ci = 0; ci < kNumTiles; ++ci)
    for (int sp : split_cand) {
      if (sp > 1 && (!allow_split || ksteps / sp < 2)) continue;
      const int sps = (ksteps + sp - 1) / sp;
      if ((ksteps + sps - 1) / sps != sp) continue;
      if (splitk_ws_bytes(sp, M, k) > kTuneWsCap) continue;
      out.push_back(Plan{ci, sp, sps});
    }
  return out;
}

// room for every candidate the tuner may try on a shape (wino_bytes: its Winograd workspace, 0 if it has no such form)
size_t tune_ws_bytes(long M, int k, int ksteps, size_t wino_bytes) {
  size_t need = wino_bytes <= kTuneWinoCap ? wino_bytes : 0;
  for (const Plan& cand : tune_candidates(M, k, ksteps, true)) need = std::max(need, splitk_ws_bytes(cand.splits, M, k));
  return need;
}

bool lookup_plan(const ShapeKey& key, Plan* pl) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  auto it = g_plan_cache.find(key);
  if (it == g_plan_cache.end()) return false;
  *pl = it->second;
  return true;
}

}  // namespace

bool frcnn::conv::conv_args_ok(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  return n > 0 && h > 0 && w > 0 && c > 0 && (c % 4) == 0 && k > 0 && r > 0 && s > 0 && stride > 0 && pad >= 0 &&
         (h + 2 * pad - r) >= 0 && (w + 2 * pad - s) >= 0;
}

ConvArgs frcnn::conv::make_conv_params(const float* x, const float* wgt, const float* scale, const float* shift,
                                       const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s,
                                       int stride, int pad, int relu) {
  ConvArgs p;
  p.x = x; p.w = wgt; p.scale = scale; p.shift = shift; p.res = residual; p.y = y;
  p.H = h; p.W = w; p.C = c; p.K = k; p.R = r; p.S = s; p.stride = stride; p.pad = pad;
  p.Ho = (h + 2 * pad - r) / stride + 1;
  p.Wo = (w + 2 * pad - s) / stride + 1;
  p.M = (int)((long)n * p.Ho * p.Wo);
  p.Ktot = r * s * c;
  p.ksteps = (p.Ktot + BK - 1) / BK;
  p.steps_per_split = p.ksteps;
  p.grows[0] = p.grows[1] = p.grows[2] = p.grows[3] = p.M;
  p.relu = relu;
  p.epi_lds = g_epi_lds;
  p.zero = zero_page_address();
  return p;
}

extern "C" int frcnn_conv2d_set_tile(int tm, int tn) {
  bool known = (tm == 0 && tn == 0);
  std::string shapes;
  for (int i = 0; i < kNumShapes; ++i) {
    known = known || (tile_cfg(i).tm == tm && tile_cfg(i).tn == tn);
    shapes += (i ? ",(" : "(") + std::to_string(tile_cfg(i).tm) + "," + std::to_string(tile_cfg(i).tn) + ")";
  }
  FRCNN_REQUIRE(known, "conv2d_set_tile: tiles are 64*tm x 64*tn with (tm,tn) in {%s} ((0,0) = automatic)", shapes.c_str());
  g_force_tm = tm;
  g_force_tn = tn;
  return FRCNN_OK;
}

extern "C" int frcnn_conv2d_set_algo(int mode) {
  FRCNN_REQUIRE(mode >= 0 && (mode & 3) <= 2 && (mode & ~(3 | 16 | 32 | 64 | 128)) == 0,
                "conv2d_set_algo: mode %d (0 auto, 1 implicit GEMM only, 2 Winograd where it applies; +16: never fuse the "
                "Winograd input transform into the GEMM, +32: forced Winograd uses the 64x64 GEMM with the fused transform, +64: the "
                "register-staged kernels store straight from the MFMA layout instead of through the LDS transpose, +128: Winograd "
                "never trims the components of partial tiles)", mode);
  g_algo_mode = mode & 3;
  g_wino_fuse = (mode & 16) ? 0 : ((mode & 32) ? 2 : 1);
  g_epi_lds = (mode & 64) ? 0 : 1;
  g_wino_trim = (mode & 128) ? 0 : 1;
  return FRCNN_OK;
}

extern "C" int frcnn_conv2d_set_staging(int use_lds_dma) {
  FRCNN_REQUIRE(use_lds_dma >= 0 && use_lds_dma <= 3, "conv2d_set_staging: mode %d (0 .. 3)", use_lds_dma);
  g_use_dma = use_lds_dma;
  return FRCNN_OK;
}

extern "C" size_t frcnn_conv2d_fwd_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad,
                                            int split_k) {
  if (!conv_args_ok(n, h, w, c, k, r, s, stride, pad)) return 0;
  const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - s) / stride + 1;
  const long M = (long)n * ho * wo;
  const int ksteps = (r * s * c + BK - 1) / BK;
  // a Winograd plan can only be chosen for a call without a residual; the caller does not say here whether it has one,
  // so the eligible shapes get room for it whenever it may be picked
  const bool wino = winograd_ok(r, s, stride, pad, c, k, 1) && g_algo_mode != 1;
  const size_t wino_bytes = wino ? winograd_ws_bytes(n, h, w, c, k) : 0;
  if (split_k <= 0 && g_force_tm == 0) {
    // the caller does not say whether it has a residual: room for the cached plan of either kind of call.  A shape with
    // only one of the two cached keeps room for whatever the other may still be tuned to (below)
    Plan c0, c1;
    const bool h0 = lookup_plan(shape_key(n, h, w, c, k, r, s, stride, pad, 1, false), &c0);
    const bool h1 = lookup_plan(shape_key(n, h, w, c, k, r, s, stride, pad, 1, true), &c1);
    if (h0 || h1) {
      size_t need = 0;
      for (const Plan* pc : {h0 ? &c0 : nullptr, h1 ? &c1 : nullptr}) {
        if (!pc) continue;
        need = std::max(need, pc->algo == 1 ? wino_bytes : splitk_ws_bytes(pc->splits, M, k));
      }
      if (g_algo_mode == 2) need = std::max(need, wino_bytes);
      if (h0 && h1) return need;
      if (!g_autotune) return need;
      return std::max(need, tune_ws_bytes(M, k, ksteps, wino_bytes));
    }
  }
  if (split_k <= 0 && g_force_tm == 0 && g_autotune) return tune_ws_bytes(M, k, ksteps, wino_bytes);   // not tuned yet
  if (g_algo_mode == 2 && split_k <= 0 && g_force_tm == 0 && wino) return wino_bytes;
  return splitk_ws_bytes(choose_plan((int)M, k, ksteps, split_k).splits, M, k);
}

extern "C" int frcnn_conv2d_plan_algo(int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int has_residual) {
  Plan pl;
  if (!lookup_plan(shape_key(n, h, w, c, k, r, s, stride, pad, 1, has_residual != 0), &pl)) return -1;
  return pl.algo;
}

extern "C" int frcnn_conv2d_set_autotune(int enable) {
  FRCNN_REQUIRE(enable >= 0 && enable <= 2, "conv2d_set_autotune: 0 off, 1 time each candidate alone, 2 time it under load");
  g_autotune = enable;
  return FRCNN_OK;
}

bool frcnn::autotune_enabled() { return g_autotune != 0; }

unsigned long long frcnn::conv_settings_word() {
  return (unsigned long long)g_algo_mode.load() | ((unsigned long long)g_wino_fuse.load() << 4) |
         ((unsigned long long)(g_wino_trim.load() ? 0 : 1) << 6) |
         ((unsigned long long)g_epi_lds.load() << 8) | ((unsigned long long)g_use_dma.load() << 12) |
         ((unsigned long long)g_force_tm.load() << 16) | ((unsigned long long)g_force_tn.load() << 24) |
         ((unsigned long long)g_bf16_tile.load() << 32) | ((unsigned long long)(g_split_bf16.load() ? 0 : 1) << 36);
}

extern "C" int frcnn_conv2d_clear_plans(void) {
  {
    std::lock_guard<std::mutex> lock(g_plan_mutex);
    g_plan_cache.clear();
  }
  frcnn::clear_wgrad_plans();
  return FRCNN_OK;
}

// Plan table as plain ints, 13 per entry: the 10-int shape key, then tile index (+ 16 for a Winograd plan), splits,
// steps per split.
extern "C" int frcnn_conv2d_export_plans(int* out, int capacity_entries) {
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  int n = 0;
  for (const auto& kv : g_plan_cache) {
    if (out && n < capacity_entries) {
      for (int i = 0; i < 10; ++i) out[n * 13 + i] = kv.first[i];
      out[n * 13 + 10] = kv.second.cfg + 16 * (kv.second.algo + kv.second.fuse_in);   // 2 = Winograd with the fused input transform
      out[n * 13 + 11] = kv.second.splits;
      out[n * 13 + 12] = kv.second.steps_per_split;
    }
    ++n;
  }
  return n;   // entries in the cache (may exceed capacity_entries: call again with a larger buffer)
}

extern "C" int frcnn_conv2d_import_plans(const int* in, int entries) {
  FRCNN_REQUIRE(in && entries >= 0, "conv2d_import_plans: null table");
  // every entry is checked before any is inserted: a refused table leaves the cache as it was
  for (int e = 0; e < entries; ++e) {
    const int* row = in + e * 13;
    const int code = row[10] >> 4, cfg = row[10] & 15;
    const int algo = code >= 1 ? 1 : 0, fuse_in = code == 2 ? 1 : 0;
    FRCNN_REQUIRE(row[10] >= 0 && cfg < kNumTiles && code <= 2 && (!fuse_in || (cfg == kTile64x64 && row[3] % BK == 0)) && row[11] >= 1 && row[11] <= 64 && row[12] >= 1 &&
                      (algo == 0 || (row[11] == 1 && winograd_ok(row[5], row[6], row[7], row[8], row[3], row[4], row[9]))),   // a residual key (row[9] >= 256) fails winograd_ok: no Winograd plan for it
                  "conv2d_import_plans: entry %d is not a valid plan (tile %d, splits %d)", e, row[10], row[11]);
    if (algo == 1) continue;   // the Winograd GEMM derives its own K-steps (launch_winograd)
    // the implicit-GEMM kernels run K-steps [z * steps_per_split, min((z + 1) * steps_per_split, ksteps)) in split z: the
    // splits must cover every K-step and none may be empty - the relation choose_plan and tune_candidates obey
    const long ktot = (long)row[5] * row[6] * row[3];
    FRCNN_REQUIRE(row[3] >= 1 && row[5] >= 1 && row[6] >= 1 && ktot <= INT32_MAX,
                  "conv2d_import_plans: entry %d is not a valid plan (filter %dx%d over %d channels)", e, row[5], row[6], row[3]);
    const long ksteps = (ktot + BK - 1) / BK;
    FRCNN_REQUIRE((ksteps + row[12] - 1) / row[12] == row[11],
                  "conv2d_import_plans: entry %d is not a valid plan (%d splits x %d steps per split for %ld K-steps: "
                  "needs ceil(K-steps / steps per split) == splits, else K-steps are dropped or a split is empty)",
                  e, row[11], row[12], ksteps);
  }
  std::lock_guard<std::mutex> lock(g_plan_mutex);
  for (int e = 0; e < entries; ++e) {
    const int* row = in + e * 13;
    const int code = row[10] >> 4, cfg = row[10] & 15;
    const int algo = code >= 1 ? 1 : 0, fuse_in = code == 2 ? 1 : 0;
    ShapeKey key;
    for (int i = 0; i < 10; ++i) key[i] = row[i];
    Plan pl{cfg, row[11], row[12]};
    pl.algo = algo;
    pl.fuse_in = fuse_in;
    g_plan_cache[key] = pl;
  }
  return FRCNN_OK;
}

namespace {

int launch_plan(ConvArgs p, const Plan& pl, long M, int k, const float* scale, const float* shift,
                const float* residual, float* y, int relu, void* ws, hipStream_t stream) {
  if (pl.algo == 1) return launch_winograd(p, pl, scale, shift, y, relu, ws, stream);
  p.partial = pl.splits > 1 ? static_cast<float*>(ws) : nullptr;
  int rc = launch_gemm(p, pl, M, k, 1, stream);
  if (rc != FRCNN_OK) return rc;
  if (pl.splits > 1) return launch_splitk_epilogue(p.partial, pl.splits, M, k, scale, shift, residual, y, relu, p.mask, p.mscale, stream);
  return FRCNN_OK;
}

size_t plan_ws_bytes(const Plan& pl, const ConvArgs& p, long M, int k) {
  if (pl.algo == 1) return winograd_ws_bytes(p.M / (p.Ho * p.Wo), p.H, p.W, p.C, p.K);
  return splitk_ws_bytes(pl.splits, M, k);
}

// frcnn_conv2d_set_autotune(2): candidates are timed UNDER LOAD - kLoadCopies launches of the candidate in flight at once,
// one per stream (the caller's + three of the library's own).  The product keeps four frames in flight on four streams
// (model/frame_graph.FramePool), where what counts is the chip time a plan takes away from the other frames' kernels, not
// the latency of one launch on an idle chip: timed alone, a grid of many small tiles that fills 256 CUs once beats the
// larger tiles whose matrix pipe runs at 1.5x the efficiency; with four copies competing the ranking is by throughput.
// The copies read and write the SAME tensors: they compute identical values, so the races are between equal stores.
constexpr int kLoadCopies = 4;
struct LoadStreams {
  hipStream_t s[kLoadCopies - 1];
  hipEvent_t done[kLoadCopies - 1];
  bool ok = false;
};
LoadStreams& load_streams() {
  static LoadStreams ls;
  static std::once_flag once;
  std::call_once(once, [] {
    bool ok = true;
    for (int j = 0; j < kLoadCopies - 1 && ok; ++j)
      ok = hipStreamCreateWithFlags(&ls.s[j], hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&ls.done[j], hipEventDisableTiming) == hipSuccess;
    ls.ok = ok;
  });
  return ls;
}

// time every candidate plan on the caller's tensors; returns false when tuning is not possible here
bool tune_plan(const ConvArgs& p, long M, int k, const float* scale, const float* shift, const float* residual,
               float* y, int relu, void* ws, size_t ws_bytes, hipStream_t stream, bool allow_split, bool wino, Plan* best) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return false;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return false;
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return false; }
  // two passes over the candidates, each keeps its best time: a one-off disturbance (clock ramp, a neighbour stream)
  // can then neither crown a slow plan nor bury the fast one
  std::vector<Plan> cands;
  if (g_algo_mode != 2 || !wino) cands = tune_candidates(M, k, p.ksteps, allow_split);
  if (wino && g_algo_mode != 1) {
    // Winograd around the grouped GEMM, one candidate per GEMM tile that makes sense for (tiles x C) x (C x K)
    for (int cfg = 0; cfg < kNumTiles; ++cfg) {
      Plan pl{cfg, 1, (p.C + BK - 1) / BK};
      pl.algo = 1;
      cands.push_back(pl);
    }
    if ((p.C % BK) == 0 && g_wino_fuse) {   // the 64x64 GEMM with the input transform in its A-tile load
      Plan pl{kTile64x64, 1, p.C / BK};
      pl.algo = 1;
      pl.fuse_in = 1;
      cands.push_back(pl);
    }
  }
  // Level 1: two passes over all candidates, each timed alone; a candidate keeps its best time (a one-off disturbance can
  // neither crown a slow plan nor bury the fast one).  Level 2: one such pass, then the kLoadFinalists fastest candidates are
  // timed under load (two passes) and ranked by that - every candidate under load would take 4x the tuning time for plans
  // that are already 1.3x off alone.
  std::vector<float> best_of(cands.size(), 1e30f);
  LoadStreams* ls = nullptr;
  if (g_autotune == 2) {
    ls = &load_streams();
    if (!ls->ok) ls = nullptr;     // no extra streams: fall back to timing alone
  }
  auto time_candidate = [&](size_t ci, bool warm, bool loaded) -> float {
    const Plan& pl = cands[ci];
    const size_t need = plan_ws_bytes(pl, p, M, k);
    if (need > ws_bytes || (need > 0 && !ws)) return 1e30f;
    if (warm && launch_plan(p, pl, M, k, scale, shift, residual, y, relu, ws, stream) != FRCNN_OK) return 1e30f;
    (void)hipEventRecord(e0, stream);
    const int reps = 3;
    bool ok = true;
    if (loaded) {
      for (int j = 0; j < kLoadCopies - 1; ++j) (void)hipStreamWaitEvent(ls->s[j], e0, 0);
      for (int i = 0; i < reps && ok; ++i) {
        ok = launch_plan(p, pl, M, k, scale, shift, residual, y, relu, ws, stream) == FRCNN_OK;
        for (int j = 0; j < kLoadCopies - 1 && ok; ++j)
          ok = launch_plan(p, pl, M, k, scale, shift, residual, y, relu, ws, ls->s[j]) == FRCNN_OK;
      }
      for (int j = 0; j < kLoadCopies - 1; ++j) {      // the caller's stream ends the region when every copy is done
        (void)hipEventRecord(ls->done[j], ls->s[j]);
        (void)hipStreamWaitEvent(stream, ls->done[j], 0);
      }
    } else {
      for (int i = 0; i < reps && ok; ++i) ok = launch_plan(p, pl, M, k, scale, shift, residual, y, relu, ws, stream) == FRCNN_OK;
    }
    (void)hipEventRecord(e1, stream);
    if (hipEventSynchronize(e1) != hipSuccess || !ok) return 1e30f;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 1e30f;
    return ms;
  };
  for (int pass = 0; pass < (ls ? 1 : 2); ++pass)
    for (size_t ci = 0; ci < cands.size(); ++ci) best_of[ci] = std::min(best_of[ci], time_candidate(ci, pass == 0, false));
  if (ls) {
    constexpr size_t kLoadFinalists = 6;
    std::vector<size_t> order(cands.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return best_of[a] < best_of[b]; });
    std::vector<float> loaded(cands.size(), 1e30f);
    for (int pass = 0; pass < 2; ++pass)
      for (size_t r = 0; r < std::min(kLoadFinalists, order.size()); ++r) {
        const size_t ci = order[r];
        if (best_of[ci] >= 1e30f) continue;
        loaded[ci] = std::min(loaded[ci], time_candidate(ci, false, true));
      }
    best_of = loaded;
  }
  float best_ms = 1e30f;
  bool found = false;
  for (size_t ci = 0; ci < cands.size(); ++ci)
    if (best_of[ci] < best_ms) { best_ms = best_of[ci]; *best = cands[ci]; found = true; }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return found;
}

}  // namespace

// Shared driver of the forward entry point and of the data-gradient entry point (which is a forward
// convolution of dy with the flipped/transposed filter).  out_stride > 1 scatters the output pixels onto
// a (hy x wy) map at stride out_stride (the map must be zero-filled by the caller); split-K is disabled then.
int frcnn::conv::run_conv(const float* x, const float* wgt, const float* scale, const float* shift, const float* residual,
                          float* y, int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int relu, int split_k,
                          void* ws, size_t ws_bytes, hipStream_t stream, int out_stride, int hy, int wy, const float* u_pre,
                          const float* mask, const float* mscale, bool wino_res) {
  ConvArgs p = make_conv_params(x, wgt, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu);
  p.u_pre = u_pre;
  p.mask = mask;
  p.mscale = mscale;
  const long M = (long)n * p.Ho * p.Wo;
  FRCNN_REQUIRE(M * (long)k < (1L << 31) && (long)n * h * w * c < (1L << 31), "conv2d: tensor too large for int32 indexing");
  p.ys = out_stride; p.Hy = hy; p.Wy = wy;
  {
    const size_t xb = (size_t)n * h * w * c * sizeof(float), wb = (size_t)k * p.Ktot * sizeof(float);
    p.xbytes = xb < ((size_t)1 << 31) ? (unsigned)xb : 0;
    p.wbytes = wb < ((size_t)1 << 31) ? (unsigned)wb : 0;
  }
  if (!p.zero) return frcnn::fail(FRCNN_ERR_LAUNCH, "conv2d: cannot resolve the zero page's device address");
  FRCNN_REQUIRE((long)k * p.Ktot < (1L << 31), "conv2d: filter too large for int32 indexing");
  const bool allow_split = out_stride == 1;
  Plan pl;
  bool have = false;
  if (split_k <= 0 && g_force_tm == 0) {   // cached plans always apply; new shapes are tuned only in autotune mode
    // wino_res (frcnn_conv2d_fwd_wres_pre): the call is planned - looked up, and tuned where a new shape is - as the
    // residual-free call of its shape; a Winograd plan then runs with the residual in its output transform, and any other
    // plan hands the call to the ordinary residual route below
    const bool keyed_res = residual != nullptr && !wino_res;
    const ShapeKey key = shape_key(n, h, w, c, k, r, s, stride, pad, out_stride, keyed_res);
    have = lookup_plan(key, &pl);
    const bool wino = !keyed_res && winograd_ok(r, s, stride, pad, c, k, out_stride);
    // a cached plan of the other form than this call may use (a residual operand, or a forced mode) is left in the cache
    // for the calls it was tuned for; this call runs the analytic plan
    bool keep_cache = false;
    if (have && ((pl.algo == 1 && (!wino || g_algo_mode == 1)) || (pl.algo == 0 && wino && g_algo_mode == 2))) {
      have = false;
      keep_cache = true;
    }
    ConvArgs pt = p;                       // what the tuner times: for a wino_res call the residual-free call itself
    if (!keyed_res) pt.res = nullptr;
    if (!have && !keep_cache && g_autotune && tune_plan(pt, M, k, scale, shift, pt.res, y, relu, ws, ws_bytes, stream, allow_split, wino, &pl)) {
      std::lock_guard<std::mutex> lock(g_plan_mutex);
      g_plan_cache[key] = pl;
      have = true;
    }
  }
  if (!have) {
    pl = choose_plan(p.M, k, p.ksteps, allow_split ? split_k : 1);
    if (g_algo_mode == 2 && split_k <= 0 && g_force_tm == 0 && (residual == nullptr || wino_res) &&
        winograd_ok(r, s, stride, pad, c, k, out_stride)) {
      pl = Plan{M >= 2048 ? kTile128x128 : kTile64x64, 1, (c + BK - 1) / BK};   // forced Winograd without tuning: a mid-size GEMM tile
      pl.algo = 1;
      if (g_wino_fuse == 2 && (c % BK) == 0) { pl.cfg = kTile64x64; pl.fuse_in = 1; }
    }
  }
  if (wino_res && pl.algo != 1)   // the residual-free call would not run Winograd: this is the ordinary call with a residual
    return run_conv(x, wgt, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, split_k, ws, ws_bytes, stream,
                    out_stride, hy, wy, u_pre, mask, mscale, false);
  if (!have && split_k <= 0 && pl.splits > 1 && (!ws || ws_bytes < plan_ws_bytes(pl, p, M, k))) {
    // the workspace was sized for this shape's cached plan, which does not apply to THIS call (a Winograd plan and a call
    // with a residual): run unsplit rather than fail
    pl = choose_plan(p.M, k, p.ksteps, 1);
  }
  {
    const size_t need = plan_ws_bytes(pl, p, M, k);
    if (need > 0 && (!ws || ws_bytes < need))
      return frcnn::fail(FRCNN_ERR_WS, "conv2d: workspace %zu < %zu bytes", ws_bytes, need);
  }
  return launch_plan(p, pl, M, k, scale, shift, residual, y, relu, ws, stream);
}

extern "C" int frcnn_conv2d_fwd(const float* x, const float* wgt, const float* scale, const float* shift,
                                const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s,
                                int stride, int pad, int relu, int split_k, void* ws, size_t ws_bytes,
                                void* stream_) {
  FRCNN_REQUIRE(x && wgt && y, "conv2d_fwd: null tensor");
  FRCNN_REQUIRE(conv_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_fwd: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0)", n, h, w, c,
                k, r, s, stride, pad);
  if (g_prof_on) ++g_prof_call;
  return run_conv(x, wgt, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, split_k, ws, ws_bytes,
                  static_cast<hipStream_t>(stream_), 1, 0, 0);
}

extern "C" int frcnn_conv2d_fwd_pre(const float* x, const float* wgt, const float* w_winograd, const float* scale,
                                    const float* shift, const float* residual, float* y, int n, int h, int w, int c,
                                    int k, int r, int s, int stride, int pad, int relu, int split_k, void* ws,
                                    size_t ws_bytes, void* stream_) {
  FRCNN_REQUIRE(x && wgt && y, "conv2d_fwd_pre: null tensor");
  FRCNN_REQUIRE(conv_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_fwd_pre: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0)", n, h, w, c,
                k, r, s, stride, pad);
  FRCNN_REQUIRE(!w_winograd || winograd_ok(r, s, stride, pad, c, k, 1),
                "conv2d_fwd_pre: a Winograd filter only goes with a 3x3 / stride 1 / pad 1 layer, c%%4 == 0, k%%4 == 0");
  if (g_prof_on) ++g_prof_call;
  return run_conv(x, wgt, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, split_k, ws, ws_bytes,
                  static_cast<hipStream_t>(stream_), 1, 0, 0, w_winograd);
}

extern "C" int frcnn_conv2d_fwd_wres_pre(const float* x, const float* wgt, const float* w_winograd, const float* scale,
                                         const float* shift, const float* residual, float* y, int n, int h, int w, int c,
                                         int k, int r, int s, int stride, int pad, int relu, int split_k, void* ws,
                                         size_t ws_bytes, void* stream_) {
  FRCNN_REQUIRE(x && wgt && y, "conv2d_fwd_wres_pre: null tensor (the (k,3,3,c) filter is needed too: the implicit GEMM reads it)");
  FRCNN_REQUIRE(residual, "conv2d_fwd_wres_pre: null residual (frcnn_conv2d_fwd_pre is the call without one)");
  FRCNN_REQUIRE(conv_args_ok(n, h, w, c, k, r, s, stride, pad) && winograd_ok(r, s, stride, pad, c, k, 1),
                "conv2d_fwd_wres_pre: needs a 3x3 / stride 1 / pad 1 layer with c%%4 == 0 and k%%4 == 0 (n=%d h=%d w=%d c=%d k=%d "
                "r=%d s=%d stride=%d pad=%d)", n, h, w, c, k, r, s, stride, pad);
  if (g_prof_on) ++g_prof_call;
  return run_conv(x, wgt, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, split_k, ws, ws_bytes,
                  static_cast<hipStream_t>(stream_), 1, 0, 0, w_winograd, nullptr, nullptr, true);
}

extern "C" int frcnn_conv2d_profile_begin(void) {
  for (ProfRec& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_prof.clear();
  g_prof_call = -1;
  g_prof_on = true;
  return FRCNN_OK;
}

extern "C" int frcnn_conv2d_profile_end(float* us, int* call, int* kind, int capacity) {
  g_prof_on = false;
  int n = 0;
  for (ProfRec& r : g_prof) {
    float ms = 0.f;
    if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess && n < capacity && us) {
      us[n] = ms * 1e3f;
      call[n] = r.call;
      kind[n] = r.kind;
    }
    ++n;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  return n;      // dispatches recorded (call again with a larger buffer if it exceeds the capacity: the data is gone)
}
