// What the two filter-gradient units share: conv_wgrad.hip holds the kernels and the launch functions that name them,
// conv_wgrad_plan.hip the plans, the tuner, the workspace layout, the settings and every entry point.
#pragma once
#include "conv_common.h"   // f32x4, NUM_CU

namespace frcnn {
namespace wgrad {

constexpr int BR = 32;             // pixels per reduction step
constexpr int BIAS_GROUPS = 64;    // rows of the bias gradient's partial sums [BIAS_GROUPS][K]
constexpr int WG_MAX_GROUPS = 24;  // convolutions of one grouped launch

// The argument block of the GEMM kernels, as the host fills it (conv_wgrad_plan.hip: fill_params, run_wgrad) and hands it to
// the launch functions.  The kernels take it under the name WgradParams (conv_wgrad.hip).
struct WgradArgs {
  const float* x;
  const float* dy;
  float* out;  // dw [K][RSC] (splits == 1) or slabs [splits][K][RSC]
  int H, W, C, K, R, S, stride, pad, Ho, Wo;
  int M, Q;  // pixels, R*S*C
  int steps, steps_per_split;
  int tiles_k, tiles_q;
  // conv_wgrad_dma_f32 only
  float* target;     // mode 0: dw [K][RSC], overwritten; mode 1: the parameter's gradient (K, c_real, R, S), accumulated into
  int* counters;     // one per tile, zero on entry and on exit (splits > 1)
  int mode, c_real, N, splits;
  unsigned xbytes, dybytes;
};

// the operands and the parameter gradients of a grouped launch, by group (blockIdx.y)
struct WgradGroupOperands {
  const float* x[WG_MAX_GROUPS];
  const float* dy[WG_MAX_GROUPS];
};
struct WgradGroupGrads {
  float* grad[WG_MAX_GROUPS];
};

// ti: 1 / 2 = conv_wgrad_f32<1 / 2> (+ reduction / accumulation kernels), 3 / 4 = conv_wgrad_dma_f32<1 / 2> (64 / 128 tile,
// reduction and accumulation in its own epilogue), 5 = conv_wgrad_bf16 (bf16 operands, 128 tile, + reduction / accumulation
// kernels like 1 / 2)
struct WgradPlan {
  int ti, splits;
};
constexpr int PLAN_BF16 = 5;
// the main kernel leaves slabs (or, unsplit and overwriting, dw itself) and the reduction / accumulation kernels finish
inline bool finishes_through_slabs(int ti) { return ti <= 2 || ti == PLAN_BF16; }
// tile edge 64 * tile_factor(ti), k rows x q columns
inline int tile_factor(int ti) { return ti == PLAN_BF16 ? 2 : ti >= 3 ? ti - 2 : ti; }
inline int tiles_along(int extent, int tf) { return (extent + 64 * tf - 1) / (64 * tf); }
inline int tiles_for(int k, int q, int ti) { return tiles_along(k, tile_factor(ti)) * tiles_along(q, tile_factor(ti)); }
inline void set_tiles(WgradArgs& p, int tf) {
  p.tiles_k = tiles_along(p.K, tf);
  p.tiles_q = tiles_along(p.Q, tf);
}

// ---- conv_wgrad.hip: the only code that names a kernel -----------------------------------------------------------------------
// The main kernel of plan code `ti` over p.tiles_k x p.tiles_q tiles and p.splits pixel ranges; the caller has filled p for it
// (out / target / counters / mode included).  The grouped form runs `groups` convolutions of p's shape, unsplit.
int launch_gemm(const WgradArgs& p, int ti, hipStream_t stream);
int launch_gemm_grouped(const WgradArgs& p, int ti, int groups, const WgradGroupOperands& g, const WgradGroupGrads& o,
                        hipStream_t stream);
// dw [K][RSC] = sum_z slabs[z], n4 = K * RSC / 4
int launch_reduce(const float* slabs, int splits, size_t n4, float* dw, hipStream_t stream);
// o.grad[g] (K, p.c_real, R, S) += sum_z slabs[g][z] (K, R, S, C), g < groups, on at most max_blocks workgroups per group
int launch_accumulate(const float* slabs, int splits, const WgradArgs& p, int groups, const WgradGroupGrads& o,
                      unsigned max_blocks, hipStream_t stream);
// db[k] = (accumulate: +=) sum_m dy[m][k] through partial [BIAS_GROUPS][k]
int launch_bias_gradient(const float* dy, int M, int k, float* partial, float* db, bool accumulate, hipStream_t stream);

}  // namespace wgrad
}  // namespace frcnn
