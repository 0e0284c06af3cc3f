// Host side of the filter gradient (kernels: conv_wgrad.hip): the split model, the plans and their cache, the tuner, the rule
// for which plan may run for a call, the workspace layout, the settings and every entry point.  It names no kernel: a plan is
// run through conv_wgrad.h's launch functions.
#include "conv_wgrad.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

namespace {

using namespace frcnn::wgrad;

// Pixel splits for a given tile count: estimated cycles of the slowest CU (two workgroups per CU share the SIMDs)
// plus the reduction pass.  ti scales the per-step MFMA work (TI*TI tiles per wave); mfma_cyc = cycles of one 32 x 32 MFMA
// tile over a step's 32 pixels (fp32: 16 x 64; bf16: 2 x 32, modelled, not tuned).
int choose_splits(int tiles, int steps, int ti, double mfma_cyc = 1024.0) {
  int best = 1;
  double best_t = 1e300;
  const double step_cyc = 2.0 * mfma_cyc * ti * ti;
  for (int sp = 1; sp <= 64; ++sp) {
    const int sps = (steps + sp - 1) / sp;
    const int real = (steps + sps - 1) / sps;
    if (real != sp) continue;
    const long rounds = ((long)tiles * real + 2 * NUM_CU - 1) / (2 * NUM_CU);  // two workgroups per CU
    const double tcyc = rounds * (sps * step_cyc + 6000.0) + (real > 1 ? real * 300.0 : 0.0);
    if (tcyc < best_t) {
      best_t = tcyc;
      best = real;
    }
  }
  return best;
}

std::atomic<int> g_wgrad_variant{0};   // frcnn_conv2d_wgrad_set_variant: 0 = every kernel, 1 = conv_wgrad_f32 only, 2 = DMA only
std::atomic<int> g_wgrad_force_ti{0}, g_wgrad_force_splits{0};   // frcnn_conv2d_wgrad_set_plan (tests): 0 = not forced

// Default plan: the 128 x 128 tile and the modelled split; in autotune mode (frcnn_conv2d_set_autotune, shared with the
// forward kernel) the first call of a shape times both tile sizes around the modelled split and caches the fastest.
typedef std::array<int, 9> WgradKey;
std::map<WgradKey, WgradPlan> g_wgrad_plans;
std::mutex g_wgrad_mutex;

// conv_wgrad_dma_f32 addresses its operands as byte offsets into 2 GB buffers (rows past M included: they must not wrap)
bool dma_ok(const WgradArgs& p) {
  const long lim = (1L << 31) - 64;
  return ((long)p.M + 2 * BR) * p.K * 4 < lim && ((long)p.M + 2 * BR) * p.C * 4 < lim &&
         (long)p.N * p.H * p.W * p.C * 4 < lim;
}

// THE rule for "plan pl may run for this call".  The LDS-DMA kernels (3 / 4) need the operands within a 2 GB buffer and, to
// split, a tile counter per tile from the caller; the variant switch takes out one family - the register-staged one only
// where the other applies.  A forced plan (frcnn_conv2d_wgrad_set_plan) and the launch itself do not heed the switch.
// The bf16 kernel (5) computes something else - products of rounded operands: it runs when, and only when, the caller asks
// for that arithmetic (`bf16`: frcnn_conv2d_bwd_weight_bf16 / _acc_bf16) - never for a tuner, a cached or a forced plan.
bool plan_may_run(const WgradPlan& pl, const WgradArgs& p, bool counters, bool heed_variant = true, bool bf16 = false) {
  if (bf16 || pl.ti == PLAN_BF16) return bf16 && pl.ti == PLAN_BF16;
  const int variant = heed_variant ? g_wgrad_variant.load() : 0;
  if (pl.ti >= 3) return variant != 1 && dma_ok(p) && (pl.splits == 1 || counters);
  return variant != 2 || !dma_ok(p);
}

std::vector<WgradPlan> wgrad_candidates(const WgradArgs& p, bool counters) {
  std::vector<WgradPlan> out;
  for (int ti = 4; ti >= 1; --ti) {
    const int base = choose_splits(tiles_for(p.K, p.Q, ti), p.steps, tile_factor(ti));
    for (int sp : {base, std::max(1, base / 2), std::min(64, base * 2), 1}) {
      const int sps = (p.steps + sp - 1) / sp;
      const int real = (p.steps + sps - 1) / sps;
      bool dup = false;
      for (const WgradPlan& c : out) dup = dup || (c.ti == ti && c.splits == real);
      if (!plan_may_run(WgradPlan{ti, real}, p, counters)) continue;
      if (!dup && (size_t)real * p.K * p.Q * sizeof(float) <= ((size_t)1 << 28)) out.push_back(WgradPlan{ti, real});
    }
  }
  return out;
}

bool wgrad_args_ok(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  return n > 0 && h > 0 && w > 0 && c > 0 && (c % 4) == 0 && k > 0 && (k % 4) == 0 && r > 0 && s > 0 && stride > 0 &&
         pad >= 0 && (h + 2 * pad - r) >= 0 && (w + 2 * pad - s) >= 0;
}

WgradKey wgrad_key(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  return WgradKey{n, h, w, c, k, r, s, stride, pad};
}

bool lookup_wgrad(const WgradKey& key, WgradPlan* pl) {
  std::lock_guard<std::mutex> lock(g_wgrad_mutex);
  auto it = g_wgrad_plans.find(key);
  if (it == g_wgrad_plans.end()) return false;
  *pl = it->second;
  return true;
}

// ---- workspace: the slabs first, 256-aligned, then the bias gradient's partial sums ------------------------------------------
size_t slab_bytes_of(const WgradPlan& pl, int k, int q) {
  return pl.splits > 1 ? (size_t)pl.splits * k * q * sizeof(float) : 0;
}
size_t bias_bytes_of(int k) { return (size_t)BIAS_GROUPS * k * sizeof(float); }
// Where the bias partials begin behind plan pl's slabs (= the bytes a call without bias gradient needs).  The accumulating
// form of plans 1 / 2 reduces from the workspace even when it does not split: at least one slab.
size_t bias_offset_of(const WgradPlan& pl, bool accumulate, int k, int q) {
  size_t slabs = slab_bytes_of(pl, k, q);
  if (accumulate && finishes_through_slabs(pl.ti)) slabs = std::max(slabs, (size_t)k * q * sizeof(float));
  return frcnn::align_up(slabs, 256);
}

// Shape -> kernel parameters (plan-independent part); false when a tensor is too large for the 32-bit indices
bool fill_params(WgradArgs* p, const float* x, const float* dy, int n, int h, int w, int c, int k, int r, int s, int stride,
                 int pad) {
  p->x = x; p->dy = dy; p->out = nullptr; p->target = nullptr; p->counters = nullptr;
  p->H = h; p->W = w; p->C = c; p->K = k; p->R = r; p->S = s; p->stride = stride; p->pad = pad;
  p->Ho = (h + 2 * pad - r) / stride + 1;
  p->Wo = (w + 2 * pad - s) / stride + 1;
  const long M = (long)n * p->Ho * p->Wo;
  if (M * (long)k >= (1L << 31) || (long)n * h * w * c >= (1L << 31)) return false;
  p->M = (int)M;
  p->N = n;
  p->Q = r * s * c;
  p->steps = (p->M + BR - 1) / BR;
  p->steps_per_split = p->steps;
  p->tiles_k = p->tiles_q = 0;
  p->mode = 0; p->c_real = c; p->splits = 1;
  p->xbytes = (unsigned)std::min<long>((long)n * h * w * c * 4, 0x7fffffffL);
  p->dybytes = (unsigned)std::min<long>(M * k * 4, 0x7fffffffL);
  return true;
}

// One plan, start to finish.  mode 0: target = dw [K][R][S][C], overwritten; mode 1: target = the parameter's gradient
// (K, c_real, R, S), accumulated into.  Plans 1 / 2 / 5 need the reduction (mode 0, splits > 1) or accumulation (mode 1) kernel
// behind the main kernel; plans 3 / 4 finish in their own epilogue.  bf16: the caller asked for the bf16 arithmetic.
int run_wgrad(WgradArgs p, const WgradPlan& pl, int mode, float* target, int c_real, void* ws, int* counters,
              hipStream_t stream, bool bf16 = false) {
  if (!plan_may_run(pl, p, counters != nullptr, false, bf16))
    return frcnn::fail(FRCNN_ERR_ARG, "conv_wgrad: plan (%d, %d) may not run for this call (the LDS-DMA kernels need operands "
                       "within 2 GB and, to split, tile counters; the bf16 kernel runs for the bf16 entry points only)",
                       pl.ti, pl.splits);
  set_tiles(p, tile_factor(pl.ti));
  p.steps_per_split = (p.steps + pl.splits - 1) / pl.splits;
  p.splits = pl.splits;
  p.mode = mode;
  p.c_real = c_real;
  if (!finishes_through_slabs(pl.ti)) {
    // (the one limit only the launch ever checked: the kernel addresses its slabs through one buffer, even a single one)
    if ((size_t)pl.splits * p.K * p.Q * sizeof(float) >= ((size_t)1 << 31))
      return frcnn::fail(FRCNN_ERR_ARG, "conv_wgrad_dma_f32: %d slabs of %d x %d floats exceed a 2 GB buffer", pl.splits, p.K, p.Q);
    p.out = static_cast<float*>(ws);
    p.target = target;
    p.counters = counters;
    return launch_gemm(p, pl.ti, stream);
  }
  p.out = (pl.splits > 1 || mode == 1) ? static_cast<float*>(ws) : target;
  const int rc = launch_gemm(p, pl.ti, stream);
  if (rc != FRCNN_OK) return rc;
  if (mode == 1) {
    WgradGroupGrads o{};
    o.grad[0] = target;
    return launch_accumulate(static_cast<const float*>(ws), pl.splits, p, 1, o, 8192, stream);
  }
  if (pl.splits > 1) return launch_reduce(static_cast<const float*>(ws), pl.splits, (size_t)p.K * p.Q / 4, target, stream);
  return rc;
}

// plan without tuning: the 128 x 128 tile and the modelled split - the DMA kernel when it may be used
WgradPlan default_plan(const WgradArgs& p, bool counters) {
  const int sp2 = choose_splits(tiles_for(p.K, p.Q, 2), p.steps, 2);
  return WgradPlan{plan_may_run(WgradPlan{4, sp2}, p, counters) ? 4 : 2, sp2};
}
// the plan of frcnn_conv2d_wgrad_set_plan for this shape (call only while one is forced)
WgradPlan forced_plan(const WgradArgs& p) {
  return WgradPlan{g_wgrad_force_ti.load(), std::max(1, std::min(g_wgrad_force_splits.load(), p.steps))};
}

// Time every candidate twice on the caller's tensors (best-of), outside stream capture only.
bool tune_wgrad(const WgradArgs& p, float* dw, void* ws, size_t ws_avail, int* counters, hipStream_t stream,
                WgradPlan* best) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return false;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return false;
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return false; }
  const std::vector<WgradPlan> cands = wgrad_candidates(p, counters != nullptr);
  std::vector<float> best_of(cands.size(), 1e30f);
  for (int pass = 0; pass < 2; ++pass)
    for (size_t ci = 0; ci < cands.size(); ++ci) {
      if (slab_bytes_of(cands[ci], p.K, p.Q) > ws_avail) continue;
      if (pass == 0 && run_wgrad(p, cands[ci], 0, dw, p.C, ws, counters, stream) != FRCNN_OK) continue;   // warm-up
      (void)hipEventRecord(e0, stream);
      bool ok = true;
      for (int i = 0; i < 3 && ok; ++i) ok = run_wgrad(p, cands[ci], 0, dw, p.C, ws, counters, stream) == FRCNN_OK;
      (void)hipEventRecord(e1, stream);
      float ms = 0.f;
      if (hipEventSynchronize(e1) != hipSuccess || !ok || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) continue;
      best_of[ci] = std::min(best_of[ci], ms);
    }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  float best_ms = 1e30f;
  bool found = false;
  for (size_t ci = 0; ci < cands.size(); ++ci)
    if (best_of[ci] < best_ms) { best_ms = best_of[ci]; *best = cands[ci]; found = true; }
  return found;
}

// shared body of frcnn_conv2d_bwd_weight (mode 0) and frcnn_conv2d_bwd_weight_acc (mode 1)
int bwd_weight(const char* who, int mode, const float* x, const float* dy, float* target, int c_real, float* bias_target, int n,
               int h, int w, int c, int k, int r, int s, int stride, int pad, void* ws, size_t ws_bytes, int* counters,
               hipStream_t stream) {
  WgradArgs p;
  if (!fill_params(&p, x, dy, n, h, w, c, k, r, s, stride, pad)) return frcnn::fail(FRCNN_ERR_ARG, "%s: tensor too large", who);
  const size_t bias_bytes = bias_target ? bias_bytes_of(k) : 0;
  const size_t slab_room = ws_bytes > bias_bytes ? ((ws_bytes - bias_bytes) / 256) * 256 : 0;
  const WgradKey key = wgrad_key(n, h, w, c, k, r, s, stride, pad);
  WgradPlan pl;
  // (a cached plan may not suit this call: the caller may have no counters, the variant switch may have changed)
  bool have = lookup_wgrad(key, &pl) && plan_may_run(pl, p, counters != nullptr);
  if (g_wgrad_force_ti.load()) {
    pl = forced_plan(p);
    if (!plan_may_run(pl, p, counters != nullptr, false))
      return frcnn::fail(FRCNN_ERR_ARG, "%s: the forced plan (%d, %d) does not apply to this call", who, pl.ti, pl.splits);
    have = true;
  }
  if (!have && mode == 0 && frcnn::autotune_enabled() && ws && tune_wgrad(p, target, ws, slab_room, counters, stream, &pl)) {
    std::lock_guard<std::mutex> lock(g_wgrad_mutex);
    g_wgrad_plans[key] = pl;
    have = true;
  }
  if (!have) pl = default_plan(p, counters != nullptr);
  const size_t bias_offset = bias_offset_of(pl, mode == 1, k, p.Q);
  const size_t need = bias_offset + bias_bytes;
  if (need > 0 && (!ws || ws_bytes < need)) return frcnn::fail(FRCNN_ERR_WS, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
  int rc = run_wgrad(p, pl, mode, target, c_real, ws, counters, stream);
  if (rc != FRCNN_OK || !bias_target) return rc;
  return launch_bias_gradient(dy, p.M, k, reinterpret_cast<float*>(static_cast<char*>(ws) + bias_offset), bias_target, mode == 1,
                              stream);
}

// ---- bf16 operands (conv_wgrad_bf16, plan 5) --------------------------------------------------------------------------------
// The plan of a bf16 call: splits > 0 as the caller gives it, clamped to the reduction steps and to the split count that
// leaves no empty range in front of the last (bf16_plan_ok then refuses what a launch cannot hold); 0 = the split model with
// the bf16 step cost, within 256 MB of slabs.
WgradPlan bf16_plan(const WgradArgs& p, int splits) {
  int sp = splits > 0 ? splits : choose_splits(tiles_for(p.K, p.Q, PLAN_BF16), p.steps, 2, 64.0);
  sp = std::max(1, std::min(sp, p.steps));
  while (splits <= 0 && sp > 1 && (size_t)sp * p.K * p.Q * sizeof(float) > ((size_t)1 << 28)) --sp;
  const int sps = (p.steps + sp - 1) / sp;
  return WgradPlan{PLAN_BF16, (p.steps + sps - 1) / sps};
}
// A caller's split count is taken as given, so it is the caller's to keep within what a launch can hold: gridDim.z and the
// 256 MB of slabs the library's own choice stays within.
constexpr int WB_MAX_SPLITS = 65535;
bool bf16_plan_ok(const WgradPlan& pl, const WgradArgs& p) {
  return pl.splits <= WB_MAX_SPLITS && (pl.splits == 1 || (size_t)pl.splits * p.K * p.Q * sizeof(float) <= ((size_t)1 << 28));
}

// shared body of frcnn_conv2d_bwd_weight_bf16 (mode 0) and frcnn_conv2d_bwd_weight_acc_bf16 (mode 1)
int bwd_weight_bf16(const char* who, int mode, const float* x, const float* dy, float* target, int c_real, float* bias_target,
                    int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int splits, void* ws, size_t ws_bytes,
                    hipStream_t stream) {
  WgradArgs p;
  if (!fill_params(&p, x, dy, n, h, w, c, k, r, s, stride, pad)) return frcnn::fail(FRCNN_ERR_ARG, "%s: tensor too large", who);
  const WgradPlan pl = bf16_plan(p, splits);
  if (!bf16_plan_ok(pl, p))
    return frcnn::fail(FRCNN_ERR_ARG, "%s: %d pixel splits of %d x %d floats exceed %d launches in z or 256 MB of slabs", who,
                       pl.splits, p.K, p.Q, WB_MAX_SPLITS);
  const size_t bias_offset = bias_offset_of(pl, mode == 1, k, p.Q);
  const size_t need = bias_offset + (bias_target ? bias_bytes_of(k) : 0);
  if (need > 0 && (!ws || ws_bytes < need)) return frcnn::fail(FRCNN_ERR_WS, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
  const int rc = run_wgrad(p, pl, mode, target, c_real, ws, nullptr, stream, true);
  if (rc != FRCNN_OK || !bias_target) return rc;
  // (the bias gradient has no matrix product: fp32 as in the fp32 entry points)
  return launch_bias_gradient(dy, p.M, k, reinterpret_cast<float*>(static_cast<char*>(ws) + bias_offset), bias_target, mode == 1,
                              stream);
}

}  // namespace

void frcnn::clear_wgrad_plans() {
  std::lock_guard<std::mutex> lock(g_wgrad_mutex);
  g_wgrad_plans.clear();
}

unsigned long long frcnn::wgrad_settings_word() {
  return (unsigned long long)g_wgrad_variant.load() | ((unsigned long long)g_wgrad_force_ti.load() << 4) |
         ((unsigned long long)g_wgrad_force_splits.load() << 8);
}

extern "C" int frcnn_conv2d_wgrad_set_plan(int kernel, int splits) {
  if (kernel < 0 || kernel > 4 || splits < 0 || splits > 64 || (kernel > 0 && splits < 1))
    return frcnn::fail(FRCNN_ERR_ARG, "conv2d_wgrad_set_plan: kernel 0 (not forced) or 1..4, 1..64 pixel splits");
  g_wgrad_force_ti.store(kernel);
  g_wgrad_force_splits.store(kernel ? splits : 0);
  return FRCNN_OK;
}

extern "C" int frcnn_conv2d_wgrad_set_variant(int variant) {
  if (variant < 0 || variant > 2)
    return frcnn::fail(FRCNN_ERR_ARG, "conv2d_wgrad_set_variant: 0 (every kernel), 1 (conv_wgrad_f32 only), 2 (conv_wgrad_dma_f32 where it applies)");
  g_wgrad_variant.store(variant);
  frcnn::clear_wgrad_plans();
  return FRCNN_OK;
}

extern "C" int frcnn_conv2d_bwd_weight_counters(int c, int k, int r, int s) {
  if (c <= 0 || k <= 0 || r <= 0 || s <= 0) return 0;
  return tiles_for(k, r * s * c, 1);
}

extern "C" size_t frcnn_conv2d_bwd_weight_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride,
                                                   int pad) {
  if (!wgrad_args_ok(n, h, w, c, k, r, s, stride, pad)) return 0;
  WgradArgs p;
  if (!fill_params(&p, nullptr, nullptr, n, h, w, c, k, r, s, stride, pad)) return 0;
  // Room for whatever this call may still choose, in either form: the default plans (with and without tile counters - also
  // for when a cached plan is not usable by the caller), the register-staged accumulating form's one slab, a cached or forced
  // plan, and every candidate of a shape that is about to be tuned
  std::vector<WgradPlan> plans = {default_plan(p, true), default_plan(p, false), WgradPlan{2, 1}};
  WgradPlan pl;
  if (lookup_wgrad(wgrad_key(n, h, w, c, k, r, s, stride, pad), &pl)) plans.push_back(pl);
  if (g_wgrad_force_ti.load()) plans.push_back(forced_plan(p));
  if (frcnn::autotune_enabled())
    for (const WgradPlan& cand : wgrad_candidates(p, true)) plans.push_back(cand);
  size_t bias_offset = 0;
  for (const WgradPlan& each : plans) bias_offset = std::max(bias_offset, bias_offset_of(each, true, k, p.Q));
  return bias_offset + bias_bytes_of(k);
}

extern "C" int frcnn_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int n, int h, int w,
                                       int c, int k, int r, int s, int stride, int pad, void* ws, size_t ws_bytes,
                                       int* counters, void* stream_) {
  FRCNN_REQUIRE(x && dy && dw, "conv2d_bwd_weight: null tensor");
  FRCNN_REQUIRE(wgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_weight: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%4==0)",
                n, h, w, c, k, r, s, stride, pad);
  return bwd_weight("conv2d_bwd_weight", 0, x, dy, dw, c, db, n, h, w, c, k, r, s, stride, pad, ws, ws_bytes, counters,
                    static_cast<hipStream_t>(stream_));
}

extern "C" int frcnn_conv2d_bwd_weight_acc(const float* x, const float* dy, float* grad_w, int c_real, float* grad_b, int n,
                                           int h, int w, int c, int k, int r, int s, int stride, int pad, void* ws,
                                           size_t ws_bytes, int* counters, void* stream_) {
  FRCNN_REQUIRE(x && dy && grad_w && c_real > 0 && c_real <= c, "conv2d_bwd_weight_acc: null tensor or c_real out of range");
  FRCNN_REQUIRE(wgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_weight_acc: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%4==0)",
                n, h, w, c, k, r, s, stride, pad);
  return bwd_weight("conv2d_bwd_weight_acc", 1, x, dy, grad_w, c_real, grad_b, n, h, w, c, k, r, s, stride, pad, ws, ws_bytes,
                    counters, static_cast<hipStream_t>(stream_));
}

// Filter gradients of `groups` convolutions of identical shape in one launch: grad_w[g] (K, c_real, R, S) += dW(x[g], dy[g]).
// x / dy / grad_w are HOST arrays of device pointers.  No pixel split, fixed summation order: deterministic.  The LDS-DMA kernel
// adds into the gradients itself; conv_wgrad_grouped_f32 (variant 1, or operands beyond 2 GB) goes through `ws` and
// the accumulation kernel.
extern "C" size_t frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes(int groups, int c, int k, int r, int s) {
  if (groups <= 0 || c <= 0 || k <= 0 || r <= 0 || s <= 0) return 0;
  return frcnn::align_up((size_t)groups * k * r * s * c * sizeof(float), 256);
}

extern "C" int frcnn_conv2d_bwd_weight_acc_grouped(const float* const* x, const float* const* dy, float* const* grad_w,
                                                   int groups, int c_real, int n, int h, int w, int c, int k, int r, int s,
                                                   int stride, int pad, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(x && dy && grad_w && groups > 0 && groups <= WG_MAX_GROUPS && c_real > 0 && c_real <= c,
                "conv2d_bwd_weight_acc_grouped: bad arguments (1..%d groups)", WG_MAX_GROUPS);
  FRCNN_REQUIRE(wgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_weight_acc_grouped: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d", n, h, w, c, k,
                r, s, stride, pad);
  WgradArgs p;
  FRCNN_REQUIRE(fill_params(&p, nullptr, nullptr, n, h, w, c, k, r, s, stride, pad), "conv2d_bwd_weight_acc_grouped: tensor too large");
  WgradGroupOperands g;
  WgradGroupGrads o;
  for (int i = 0; i < WG_MAX_GROUPS; ++i) {
    const int j = i < groups ? i : 0;
    FRCNN_REQUIRE(x[j] && dy[j] && grad_w[j], "conv2d_bwd_weight_acc_grouped: null tensor in group %d", j);
    g.x[i] = x[j]; g.dy[i] = dy[j]; o.grad[i] = grad_w[j];
  }
  // the 128 x 128 tile when the groups together still give every CU a workgroup, else 64 x 64
  const int tf = (long)tiles_for(k, p.Q, 2) * groups >= NUM_CU ? 2 : 1;
  set_tiles(p, tf);
  p.c_real = c_real;
  if (plan_may_run(WgradPlan{tf + 2, 1}, p, false)) {
    p.mode = 1;
    return launch_gemm_grouped(p, tf + 2, groups, g, o, stream);
  }
  const size_t need = frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes(groups, c, k, r, s);
  if (!ws || ws_bytes < need)
    return frcnn::fail(FRCNN_ERR_WS, "conv2d_bwd_weight_acc_grouped: workspace %zu < %zu bytes", ws_bytes, need);
  p.out = static_cast<float*>(ws);
  const int rc = launch_gemm_grouped(p, tf, groups, g, o, stream);
  if (rc != FRCNN_OK) return rc;
  return launch_accumulate(static_cast<const float*>(ws), 1, p, groups, o, 2048, stream);
}

// ---- bf16-operand filter gradient (cfg.TRAIN.CONV_BF16) ----------------------------------------------------------------------
extern "C" size_t frcnn_conv2d_bwd_weight_bf16_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad,
                                                        int splits) {
  if (!wgrad_args_ok(n, h, w, c, k, r, s, stride, pad) || splits < 0) return 0;
  WgradArgs p;
  if (!fill_params(&p, nullptr, nullptr, n, h, w, c, k, r, s, stride, pad)) return 0;
  // either form, with the bias gradient (0 for a split count the call would refuse)
  const WgradPlan pl = bf16_plan(p, splits);
  if (!bf16_plan_ok(pl, p)) return 0;
  return bias_offset_of(pl, true, k, p.Q) + bias_bytes_of(k);
}

extern "C" int frcnn_conv2d_bwd_weight_bf16(const float* x, const float* dy, float* dw, float* db, int n, int h, int w, int c,
                                            int k, int r, int s, int stride, int pad, int splits, void* ws, size_t ws_bytes,
                                            void* stream_) {
  FRCNN_REQUIRE(x && dy && dw && splits >= 0, "conv2d_bwd_weight_bf16: null tensor or negative split count");
  FRCNN_REQUIRE(wgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_weight_bf16: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%4==0)",
                n, h, w, c, k, r, s, stride, pad);
  return bwd_weight_bf16("conv2d_bwd_weight_bf16", 0, x, dy, dw, c, db, n, h, w, c, k, r, s, stride, pad, splits, ws, ws_bytes,
                         static_cast<hipStream_t>(stream_));
}

extern "C" int frcnn_conv2d_bwd_weight_acc_bf16(const float* x, const float* dy, float* grad_w, int c_real, float* grad_b, int n,
                                                int h, int w, int c, int k, int r, int s, int stride, int pad, int splits,
                                                void* ws, size_t ws_bytes, void* stream_) {
  FRCNN_REQUIRE(x && dy && grad_w && c_real > 0 && c_real <= c && splits >= 0,
                "conv2d_bwd_weight_acc_bf16: null tensor, c_real out of range or negative split count");
  FRCNN_REQUIRE(wgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_weight_acc_bf16: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%4==0)",
                n, h, w, c, k, r, s, stride, pad);
  return bwd_weight_bf16("conv2d_bwd_weight_acc_bf16", 1, x, dy, grad_w, c_real, grad_b, n, h, w, c, k, r, s, stride, pad, splits,
                         ws, ws_bytes, static_cast<hipStream_t>(stream_));
}
