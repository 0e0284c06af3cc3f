// ------------------------------------------------------------------------------------------------
// Data gradient: dx = conv_transpose(dy, w).  For stride 1 this is a forward convolution of dy with the
// filter flipped in (r, s) and transposed in (k, c); a strided 1x1 scatters a 1x1 convolution onto the
// even pixels; a strided RxS first zero-inserts dy.  Replaces autograd's conv backward for the
// trainable part of lib/nets/resnet.py / lib/nets/fpn.py (lib/model/train_val.py:458 -> loss.backward()).
// ------------------------------------------------------------------------------------------------
#include "conv_common.h"

#include <algorithm>

using namespace frcnn::conv;

namespace {
__global__ __launch_bounds__(256) void transpose_filter_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                                              int K, int R, int S, int C) {
  const size_t total = (size_t)K * R * S * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    // i enumerates the OUTPUT [c][r'][s'][k] so that writes are coalesced
    const int k = (int)(i % K);
    size_t t = i / K;
    const int s2 = (int)(t % S);
    t /= S;
    const int r2 = (int)(t % R);
    const int c = (int)(t / R);
    wt[i] = w[(((size_t)k * R + (R - 1 - r2)) * S + (S - 1 - s2)) * C + c];
  }
}

// dyd[n, ho*stride, wo*stride, :] = dy[n, ho, wo, :], zeros elsewhere (Hd x Wd map), 16 B per thread
__global__ __launch_bounds__(256) void dilate_kernel(const float* __restrict__ dy, float* __restrict__ dyd, int N,
                                                    int Ho, int Wo, int K4, int stride, int Hd, int Wd) {
  const size_t total = (size_t)N * Hd * Wd * K4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k4 = (int)(i % K4);
    size_t t = i / K4;
    const int wd = (int)(t % Wd);
    t /= Wd;
    const int hd = (int)(t % Hd);
    const int n = (int)(t / Hd);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (hd % stride == 0 && wd % stride == 0 && hd / stride < Ho && wd / stride < Wo)
      v = reinterpret_cast<const f32x4*>(dy)[(((size_t)n * Ho + hd / stride) * Wo + wd / stride) * K4 + k4];
    reinterpret_cast<f32x4*>(dyd)[i] = v;
  }
}

struct DgradGeom {
  int ho, wo, hd, wd, pad_t;
  bool dilate;
};
DgradGeom dgrad_geom(int h, int w, int r, int s, int stride, int pad) {
  DgradGeom g;
  g.ho = (h + 2 * pad - r) / stride + 1;
  g.wo = (w + 2 * pad - s) / stride + 1;
  g.pad_t = r - 1 - pad;
  g.dilate = stride > 1 && (r > 1 || s > 1);
  // zero-inserted map, extended by the rows/cols the strided forward pass never reached
  g.hd = (g.ho - 1) * stride + 1 + (h + 2 * pad - r) % stride;
  g.wd = (g.wo - 1) * stride + 1 + (w + 2 * pad - s) % stride;
  return g;
}
bool dgrad_args_ok(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  return conv_args_ok(n, h, w, c, k, r, s, stride, pad) && (k % 4) == 0 && r == s && r - 1 - pad >= 0;
}
}  // namespace

extern "C" int frcnn_conv2d_transpose_filter(const float* w_krsc, float* w_crsk_flipped, int k, int r, int s, int c,
                                             void* stream_) {
  FRCNN_REQUIRE(w_krsc && w_crsk_flipped && k > 0 && r > 0 && s > 0 && c > 0, "conv2d_transpose_filter: bad arguments");
  const size_t total = (size_t)k * r * s * c;
  hipLaunchKernelGGL(transpose_filter_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), w_krsc, w_crsk_flipped, k, r, s, c);
  return frcnn::check_launch("transpose_filter_kernel");
}

extern "C" size_t frcnn_conv2d_bwd_data_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride,
                                                 int pad) {
  if (!dgrad_args_ok(n, h, w, c, k, r, s, stride, pad)) return 0;
  const DgradGeom g = dgrad_geom(h, w, r, s, stride, pad);
  if (stride > 1 && !g.dilate) return 0;  // strided 1x1: scattered output, no split-K
  if (!g.dilate) return frcnn_conv2d_fwd_ws_bytes(n, g.ho, g.wo, k, c, r, s, 1, g.pad_t, 0);
  const size_t dil = frcnn::align_up((size_t)n * g.hd * g.wd * k * sizeof(float), 256);
  return dil + frcnn_conv2d_fwd_ws_bytes(n, g.hd, g.wd, k, c, r, s, 1, g.pad_t, 0);
}

extern "C" int frcnn_conv2d_bwd_data_act(const float* dy, const float* w_crsk_flipped, const float* w_winograd,
                                         const float* add, const float* act_y, const float* act_scale, float* dx, int n,
                                         int h, int w, int c, int k, int r, int s, int stride, int pad, void* ws,
                                         size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(!act_scale || act_y, "conv2d_bwd_data_act: act_scale without act_y");
  FRCNN_REQUIRE(!act_y || stride == 1 || (r > 1 || s > 1),
                "conv2d_bwd_data_act: the strided 1x1 data gradient (scattered output) has no activation epilogue");
  FRCNN_REQUIRE(!w_winograd || (stride == 1 && !add && winograd_ok(r, s, 1, r - 1 - pad, k, c, 1)),
                "conv2d_bwd_data_pre: a Winograd filter only goes with a 3x3 / stride 1 / pad 1 layer without `add`");
  FRCNN_REQUIRE(dy && w_crsk_flipped && dx, "conv2d_bwd_data: null tensor");
  FRCNN_REQUIRE(dgrad_args_ok(n, h, w, c, k, r, s, stride, pad),
                "conv2d_bwd_data: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%4==0, "
                "r==s, pad<=r-1)", n, h, w, c, k, r, s, stride, pad);
  const DgradGeom g = dgrad_geom(h, w, r, s, stride, pad);
  const size_t need = frcnn_conv2d_bwd_data_ws_bytes(n, h, w, c, k, r, s, stride, pad);
  if (need > 0 && (!ws || ws_bytes < need))
    return frcnn::fail(FRCNN_ERR_WS, "conv2d_bwd_data: workspace %zu < %zu bytes", ws_bytes, need);
  if (stride == 1)  // dx (n,h,w,c) = conv(dy (n,ho,wo,k), w^T flipped), same-size output
    return run_conv(dy, w_crsk_flipped, nullptr, nullptr, add, dx, n, g.ho, g.wo, k, c, r, s, 1, g.pad_t, 0, 0, ws,
                    ws_bytes, stream, 1, 0, 0, w_winograd, act_y, act_scale);
  if (!g.dilate) {
    // strided 1x1: only pixels (ho*stride, wo*stride) receive a gradient; the rest is `add` (or zero)
    const size_t bytes = (size_t)n * h * w * c * sizeof(float);
    hipError_t e = add ? frcnn::copy_bytes(dx, add, bytes, stream) : frcnn::fill_bytes(dx, 0, bytes, stream);
    if (e != hipSuccess) return frcnn::fail(FRCNN_ERR_LAUNCH, "conv2d_bwd_data: init dx: %s", hipGetErrorString(e));
    return run_conv(dy, w_crsk_flipped, nullptr, nullptr, add, dx, n, g.ho, g.wo, k, c, 1, 1, 1, 0, 0, 1, nullptr, 0,
                    stream, stride, h, w);
  }
  float* dyd = static_cast<float*>(ws);
  const size_t dil = frcnn::align_up((size_t)n * g.hd * g.wd * k * sizeof(float), 256);
  const size_t total = (size_t)n * g.hd * g.wd * (k / 4);
  hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, stream, dy,
                     dyd, n, g.ho, g.wo, k / 4, stride, g.hd, g.wd);
  int rc = frcnn::check_launch("dilate_kernel");
  if (rc != FRCNN_OK) return rc;
  return run_conv(dyd, w_crsk_flipped, nullptr, nullptr, add, dx, n, g.hd, g.wd, k, c, r, s, 1, g.pad_t, 0, 0,
                  static_cast<char*>(ws) + dil, ws_bytes - dil, stream, 1, 0, 0, nullptr, act_y, act_scale);
}

// bf16-operand data gradient (cfg.TRAIN.CONV_BF16): the same two forms - stride 1, and the zero-inserted strided R x S - as
// ONE frcnn_conv2d_fwd_bf16 launch of dy (or the zero-inserted dy) with the bf16 pack of the flipped / transposed filter, `add`
// as that kernel's residual operand.  The act_y mask and act_scale are frcnn_act_bwd in place behind the GEMM (the bf16 kernel's
// store has no mask operand).  The strided 1x1 form writes a scattered output, which the bf16 kernel does not have: FRCNN_ERR_ARG.
extern "C" size_t frcnn_conv2d_bwd_data_bf16_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  if (!dgrad_args_ok(n, h, w, c, k, r, s, stride, pad)) return 0;
  const DgradGeom g = dgrad_geom(h, w, r, s, stride, pad);
  return g.dilate ? frcnn::align_up((size_t)n * g.hd * g.wd * k * sizeof(float), 256) : 0;
}

extern "C" int frcnn_conv2d_bwd_data_bf16(const float* dy, const void* w_crsk_flipped_bf16, const float* add, const float* act_y,
                                          const float* act_scale, float* dx, int n, int h, int w, int c, int k, int r, int s,
                                          int stride, int pad, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(dy && w_crsk_flipped_bf16 && dx, "conv2d_bwd_data_bf16: null tensor");
  FRCNN_REQUIRE(!act_scale || act_y, "conv2d_bwd_data_bf16: act_scale without act_y");
  FRCNN_REQUIRE(dgrad_args_ok(n, h, w, c, k, r, s, stride, pad) && (k % 32) == 0,
                "conv2d_bwd_data_bf16: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%4==0, k%%32==0, "
                "r==s, pad<=r-1)", n, h, w, c, k, r, s, stride, pad);
  FRCNN_REQUIRE(stride == 1 || r > 1, "conv2d_bwd_data_bf16: the strided 1x1 data gradient (scattered output) has no bf16 form");
  const DgradGeom g = dgrad_geom(h, w, r, s, stride, pad);
  const size_t need = frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, s, stride, pad);
  if (need > 0 && (!ws || ws_bytes < need))
    return frcnn::fail(FRCNN_ERR_WS, "conv2d_bwd_data_bf16: workspace %zu < %zu bytes", ws_bytes, need);
  const float* src = dy;
  int hs = g.ho, wsrc = g.wo;
  if (g.dilate) {
    float* dyd = static_cast<float*>(ws);
    const size_t total = (size_t)n * g.hd * g.wd * (k / 4);
    hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, stream, dy,
                       dyd, n, g.ho, g.wo, k / 4, stride, g.hd, g.wd);
    const int rc = frcnn::check_launch("dilate_kernel");
    if (rc != FRCNN_OK) return rc;
    src = dyd;
    hs = g.hd;
    wsrc = g.wd;
  }
  // dx (n,h,w,c) = conv(src (n,hs,wsrc,k), w^T flipped), same-size output
  const int rc = frcnn_conv2d_fwd_bf16(src, w_crsk_flipped_bf16, nullptr, nullptr, add, dx, n, hs, wsrc, k, c, r, s, 1, g.pad_t, 0,
                                       stream_);
  if (rc != FRCNN_OK || !act_y) return rc;
  return frcnn_act_bwd(dx, act_y, act_scale, 1, (int64_t)n * h * w, c, dx, nullptr, stream_);
}

extern "C" int frcnn_conv2d_bwd_data_pre(const float* dy, const float* w_crsk_flipped, const float* w_winograd,
                                         const float* add, float* dx, int n, int h, int w, int c, int k, int r, int s,
                                         int stride, int pad, void* ws, size_t ws_bytes, void* stream_) {
  return frcnn_conv2d_bwd_data_act(dy, w_crsk_flipped, w_winograd, add, nullptr, nullptr, dx, n, h, w, c, k, r, s, stride,
                                   pad, ws, ws_bytes, stream_);
}

extern "C" int frcnn_conv2d_bwd_data(const float* dy, const float* w_crsk_flipped, const float* add, float* dx, int n,
                                     int h, int w, int c, int k, int r, int s, int stride, int pad, void* ws,
                                     size_t ws_bytes, void* stream_) {
  return frcnn_conv2d_bwd_data_pre(dy, w_crsk_flipped, nullptr, add, dx, n, h, w, c, k, r, s, stride, pad, ws, ws_bytes,
                                   stream_);
}
