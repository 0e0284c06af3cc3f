// What the convolution units (conv_igemm.hip, conv_plan.hip, conv_winograd.hip, conv_bf16.hip, conv_dgrad.hip) share:
// the GEMM kernels' argument block, the plan and tile-table types, the launcher, and the declarations of what one unit
// defines and another one uses.
#pragma once
#include "common.h"

#include <atomic>
#include <hip/hip_ext.h>

namespace frcnn {
namespace conv {

// The argument block of the GEMM kernels, as the host fills it (make_conv_params) and hands it from unit to unit.  The kernels
// take it under the name ConvParams (conv_igemm.hip), which is what comments of the form ConvParams::field refer to.
struct ConvArgs {
  const float* x = nullptr;
  const float* w = nullptr;
  const float* scale = nullptr;
  const float* shift = nullptr;
  const float* res = nullptr;
  float* y = nullptr;
  float* partial = nullptr;  // split-K slabs [splits][M][K] or nullptr
  int H = 0, W = 0, C = 0, K = 0, R = 0, S = 0, stride = 0, pad = 0, Ho = 0, Wo = 0;
  int M = 0;     // N*Ho*Wo
  int Ktot = 0;  // R*S*C
  int ksteps = 0;
  int steps_per_split = 0;
  int tiles_m = 0, tiles_n = 0;
  int relu = 0;
  int ys = 1, Hy = 0, Wy = 0;  // output pixel (ho, wo) is written at (ho*ys, wo*ys) of an Hy x Wy map (ys = 1: dense)
  // grouped launch (blockIdx.y = group): element offsets of a group's activations / filter / output.  Used by the
  // Winograd path (16 independent GEMMs in one launch); 0 for an ordinary convolution (gridDim.y = 1).
  size_t gx = 0, gw = 0, gy = 0;
  // rows of a group's GEMM by the kind of its Winograd component (i, j) = (group >> 2, group & 3): [0] i != 3 and j != 3,
  // [1] i == 3 only, [2] j == 3 only, [3] both (group_rows).  An ordinary convolution is group 0: [0] = M; a Winograd launch
  // that trims the components of partial tiles (launch_winograd) has [1..3] <= [0] = M, an untrimmed one M four times
  int grows[4] = {0, 0, 0, 0};
  // optional activation-backward epilogue (data-gradient calls): y = mask[m][n] > 0 ? y * mscale[n] : 0 - the ReLU /
  // folded-BatchNorm backward of the layer BELOW, applied to this layer's input gradient before it is stored
  const float* mask = nullptr;
  const float* mscale = nullptr;
  const float* u_pre = nullptr;   // host side: Winograd-transformed filter supplied by the caller (frcnn_conv2d_fwd_pre) or nullptr
  // Winograd grouped GEMM with the INPUT TRANSFORM fused into the A-tile load (conv_igemm_f32<..., WINO = true>): x is the
  // layer's NHWC input (wiH x wiW pixels, C channels), GEMM row m is the 2x2-output tile (n, ty, tx) of a wth x wtw grid and
  // blockIdx.y the transform component
  int wiH = 0, wiW = 0, wth = 0, wtw = 0;
  int epi_lds = 0;   // 1: the register-staged kernels transpose their accumulator tiles through LDS before storing (conv_epilogue_lds)
  unsigned xbytes = 0, wbytes = 0;   // byte range of (a group's) activations / filter for the buffer-load kernel (0: range >= 2 GB, kernel not usable)
  const float* zero = nullptr;   // device address of g_zero_page (resolved once on the host: a kernel argument costs no s_getpc / s_load in the K loop)
};

}  // namespace conv
}  // namespace frcnn

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;
constexpr int NUM_CU = 256;

}  // namespace

namespace frcnn {
namespace conv {

struct Plan {
  int cfg, splits, steps_per_split;
  int algo = 0;   // 0 = implicit GEMM; 1 = Winograd F(2x2, 3x3) around a grouped GEMM that uses tile `cfg` (splits = 1)
  int fuse_in = 0;   // algo 1 only: the input transform runs inside the 64x64 GEMM's A-tile load (kTile64x64, C % 32 == 0)
};

// One thin wrapper per kernel family of the implicit GEMM (conv_igemm.hip); p.tiles_m / tiles_n are set by launch_gemm.
typedef int (*ConvLaunch)(const ConvArgs& p, int splits, int groups, hipStream_t stream);

// A row of the tile table kTiles, which a plan names by its index: the block tile (64*tm) x (64*tn) = (32*WTM*WM) x (32*WTN*WN),
// its register-staged kernel, and up to two alternatives tried in order when C % 32 == 0 (conv_igemm.hip: resolve_tile).
struct TileAlt {
  ConvLaunch launch;   // nullptr: none
  unsigned modes;      // bit S: applies in staging mode S
  bool small;          // needs both operands below 2 GB (the buffer-load kernels: ConvParams::xbytes / wbytes)
};
struct TileCfg {
  int tm, tn;            // block tile in units of 64 pixels x 64 channels (the frcnn_conv2d_set_tile key)
  int wm, wn, wtm, wtn;  // wave grid and 32x32 tiles per wave
  ConvLaunch reg[2];     // the register-staged kernel of the tile: [0] any C, [1] C % 32 == 0
  TileAlt alt[2];
};
constexpr int kNumTiles = 14;
// row idx of the tile table (conv_igemm.hip: kTiles), 0 <= idx < kNumTiles
const TileCfg& tile_cfg(int idx);
constexpr int kNumShapes = 6;   // rows 0 .. kNumShapes - 1 hold every tile shape once
// the rows the code names: the mid-size tile (choose_plan's start, forced Winograd) and the small one (the fall-back of a
// forced split, the small forced-Winograd GEMM, the ONLY tile of the fused Winograd input transform)
constexpr int kTile128x128 = 2, kTile64x64 = 5;
constexpr int kTilePersistent = 13;   // (launch_winograd: this row's kernel takes every group's row count from p.M)

// ---- settings (conv_plan.hip: frcnn_conv2d_set_algo / _set_staging / _set_tile / _set_autotune, the bf16 hooks) ----------
extern std::atomic<int> g_algo_mode, g_wino_fuse, g_epi_lds, g_wino_trim, g_use_dma, g_force_tm, g_force_tn, g_bf16_tile,
    g_split_bf16, g_autotune;

// ---- per-dispatch timing (conv_plan.hip) -------------------------------------------------------------------------------
extern std::atomic<bool> g_prof_on;
extern int g_prof_call;
bool prof_events(int kind, hipEvent_t* e0, hipEvent_t* e1, hipStream_t stream);

// ---- launching ---------------------------------------------------------------------------------------------------------
// The one launcher of the convolution units' kernels: the once-per-kernel dynamic-LDS attribute (kernels that ask for LDS at
// launch may need more than the 64 KB granted by default), the timed launch form while a profile is open (`kind` as in
// conv_plan.hip's ProfRec) and the launch check.  `args` must have the kernel's parameter types exactly (hipExtLaunchKernelGGL deduces from them).
template <auto Kernel, typename... Args>
int launch_kernel(const char* name, int kind, dim3 grid, unsigned block, size_t lds, hipStream_t stream, Args... args) {
  static std::atomic<bool> configured{false};   // idempotent attribute call: a race only repeats it
  if (lds > 0 && !configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return frcnn::fail(FRCNN_ERR_LAUNCH, "conv: set LDS size: %s", hipGetErrorString(e));
    configured = true;
  }
  hipEvent_t e0, e1;
  if (prof_events(kind, &e0, &e1, stream)) hipExtLaunchKernelGGL(Kernel, grid, dim3(block), (uint32_t)lds, stream, e0, e1, 0, args...);
  else hipLaunchKernelGGL(Kernel, grid, dim3(block), lds, stream, args...);
  return frcnn::check_launch(name);
}

// launches a 1-D grid kernel, one thread per element (profile kind 2 = Winograd transform)
template <auto Kernel, typename... Args>
int launch_1d(const char* what, size_t threads, hipStream_t stream, Args... args) {
  return launch_kernel<Kernel>(what, 2, dim3((unsigned)((threads + 255) / 256)), 256, 0, stream, args...);
}

// ---- conv_igemm.hip ----------------------------------------------------------------------------------------------------
const float* zero_page_address();
int launch_gemm(ConvArgs p, const Plan& pl, long M, int k, int groups, hipStream_t stream);
int launch_splitk_epilogue(const float* partial, int splits, long M, int k, const float* scale, const float* shift,
                           const float* residual, float* y, int relu, const float* mask, const float* mscale, hipStream_t stream);
// the bf16 GEMM on its 64x64 (small_tile) or 128x128 tile over the packed filter wq; planes = 1, or 3 for the split form
int launch_gemm_bf16(const ConvArgs& p, const unsigned short* wq, bool small_tile, int planes, hipStream_t stream);

// ---- conv_winograd.hip -------------------------------------------------------------------------------------------------
bool winograd_ok(int r, int s, int stride, int pad, int c, int k, int out_stride);
size_t winograd_ws_bytes(int n, int h, int w, int c, int k);
int launch_winograd(const ConvArgs& p, const Plan& pl, const float* scale, const float* shift, float* y, int relu, void* ws,
                    hipStream_t stream);

// ---- conv_plan.hip -----------------------------------------------------------------------------------------------------
bool conv_args_ok(int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
// The fields every caller derives the same way from a convolution's arguments.  A caller adds what is its own (output stride,
// operand byte ranges, activation mask, ...) and makes its own range checks: M is cut to int and `zero` is null where the
// zero page cannot be resolved.
ConvArgs make_conv_params(const float* x, const float* wgt, const float* scale, const float* shift, const float* residual,
                          float* y, int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int relu);
int run_conv(const float* x, const float* wgt, const float* scale, const float* shift, const float* residual, float* y, int n,
             int h, int w, int c, int k, int r, int s, int stride, int pad, int relu, int split_k, void* ws, size_t ws_bytes,
             hipStream_t stream, int out_stride, int hy, int wy, const float* u_pre = nullptr, const float* mask = nullptr,
             const float* mscale = nullptr, bool wino_res = false);

}  // namespace conv
}  // namespace frcnn
