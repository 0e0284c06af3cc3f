// Entry points of the bf16-operand and split-bf16 forward convolutions (the kernel: conv_igemm_bf16 in conv_igemm.hip) and
// the filter packing that goes with them.
#include "conv_common.h"

using namespace frcnn::conv;

namespace {

// fp32 -> bf16, round to nearest even (the conversion the kernel applies to the activations)
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const __bf16 v = (__bf16)w[i];
  out[i] = __builtin_bit_cast(unsigned short, v);
}

// The one analytic tile rule of the bf16 kernel: the 64x64 tile when 128x128 tiles would leave CUs without a workgroup
bool bf16_small_tile(long M, int k) {
  const int mode = g_bf16_tile;
  if (mode) return mode == 1;
  return ((M + 127) / 128) * ((k + 127) / 128) < NUM_CU;
}

// Split form of pack_bf16_kernel: hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid), each rounded to nearest even;
// both remainders are exact in fp32 and hi + mid + lo == w for finite w whose remainders do not underflow.
__global__ __launch_bounds__(256) void pack_bf16x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float v = w[i];
  const __bf16 hi = (__bf16)v;
  const float r1 = v - (float)hi;
  const __bf16 mid = (__bf16)r1;
  const __bf16 lo = (__bf16)(r1 - (float)mid);
  out[i] = __builtin_bit_cast(unsigned short, hi);
  out[count + i] = __builtin_bit_cast(unsigned short, mid);
  out[2 * count + i] = __builtin_bit_cast(unsigned short, lo);
}

}  // namespace

extern "C" size_t frcnn_conv2d_pack_bf16_bytes(int k, int r, int s, int c) {
  if (k <= 0 || r <= 0 || s <= 0 || c <= 0) return 0;
  return (size_t)k * r * s * c * sizeof(unsigned short);
}

extern "C" int frcnn_conv2d_pack_bf16(const float* w_krsc, void* w_bf16, int k, int r, int s, int c, void* stream_) {
  FRCNN_REQUIRE(w_krsc && w_bf16, "conv2d_pack_bf16: null tensor");
  FRCNN_REQUIRE(k > 0 && r > 0 && s > 0 && c > 0, "conv2d_pack_bf16: bad shape k=%d r=%d s=%d c=%d", k, r, s, c);
  const size_t count = (size_t)k * r * s * c;
  FRCNN_REQUIRE((count + 255) / 256 < ((size_t)1 << 31), "conv2d_pack_bf16: filter too large");
  return launch_kernel<pack_bf16_kernel>("pack_bf16_kernel", 2, dim3((unsigned)((count + 255) / 256)), 256, 0,
                                         static_cast<hipStream_t>(stream_), w_krsc, static_cast<unsigned short*>(w_bf16), count);
}

extern "C" int frcnn_conv2d_bf16_set_tile(int mode) {
  FRCNN_REQUIRE(mode >= 0 && mode <= 2, "conv2d_bf16_set_tile: mode %d (0 = by the number of workgroups, 1 = 64x64, 2 = 128x128)", mode);
  g_bf16_tile = mode;
  return FRCNN_OK;
}

namespace {
int fwd_bf16(int planes, const float* x, const void* w_bf16, const float* scale, const float* shift, const float* residual, float* y, int n,
             int h, int w, int c, int k, int r, int s, int stride, int pad, int relu, void* stream_) {
  FRCNN_REQUIRE(x && w_bf16 && y, "conv2d_fwd_bf16: null tensor");
  FRCNN_REQUIRE(conv_args_ok(n, h, w, c, k, r, s, stride, pad) && (c % BK) == 0,
                "conv2d_fwd_bf16: bad shape n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d (need c%%32==0)", n, h, w, c,
                k, r, s, stride, pad);
  FRCNN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_bf16)) & 15) == 0,
                "conv2d_fwd_bf16: x and w_bf16 must be 16-byte aligned");
  ConvArgs p = make_conv_params(x, nullptr, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu);   // (the filter is wq)
  const long M = (long)n * p.Ho * p.Wo;
  FRCNN_REQUIRE(M * (long)k < (1L << 31) && (long)n * h * w * c < (1L << 31) && M + 128 < (1L << 31),
                "conv2d_fwd_bf16: tensor too large for int32 indexing");
  FRCNN_REQUIRE((long)k * p.Ktot < (1L << 31), "conv2d_fwd_bf16: filter too large for int32 indexing");
  if (!p.zero) return frcnn::fail(FRCNN_ERR_LAUNCH, "conv2d_fwd_bf16: cannot resolve the zero page's device address");
  if (g_prof_on) ++g_prof_call;
  const unsigned short* wq = static_cast<const unsigned short*>(w_bf16);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  return launch_gemm_bf16(p, wq, bf16_small_tile(M, k), planes, stream);
}
}  // namespace

extern "C" int frcnn_conv2d_fwd_bf16(const float* x, const void* w_bf16, const float* scale, const float* shift,
                                     const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s,
                                     int stride, int pad, int relu, void* stream_) {
  return fwd_bf16(1, x, w_bf16, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, stream_);
}

extern "C" int frcnn_conv2d_fwd_bf16x3(const float* x, const void* w_bf16x3, const float* scale, const float* shift,
                                       const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s,
                                       int stride, int pad, int relu, void* stream_) {
  return fwd_bf16(3, x, w_bf16x3, scale, shift, residual, y, n, h, w, c, k, r, s, stride, pad, relu, stream_);
}

extern "C" size_t frcnn_conv2d_pack_bf16x3_bytes(int k, int r, int s, int c) { return 3 * frcnn_conv2d_pack_bf16_bytes(k, r, s, c); }

extern "C" int frcnn_conv2d_pack_bf16x3(const float* w_krsc, void* w_bf16x3, int k, int r, int s, int c, void* stream_) {
  FRCNN_REQUIRE(w_krsc && w_bf16x3, "conv2d_pack_bf16x3: null tensor");
  FRCNN_REQUIRE(k > 0 && r > 0 && s > 0 && c > 0, "conv2d_pack_bf16x3: bad shape k=%d r=%d s=%d c=%d", k, r, s, c);
  const size_t count = (size_t)k * r * s * c;
  FRCNN_REQUIRE((count + 255) / 256 < ((size_t)1 << 31), "conv2d_pack_bf16x3: filter too large");
  return launch_kernel<pack_bf16x3_kernel>("pack_bf16x3_kernel", 2, dim3((unsigned)((count + 255) / 256)), 256, 0,
                                           static_cast<hipStream_t>(stream_), w_krsc, static_cast<unsigned short*>(w_bf16x3), count);
}

extern "C" int frcnn_conv2d_split_bf16_enable(int on) {
  FRCNN_REQUIRE(on == 0 || on == 1, "conv2d_split_bf16_enable: %d (0 or 1)", on);
  g_split_bf16 = on;
  return FRCNN_OK;
}

// The rule, in the GEMM's dimensions M = n*ho*wo, N = k, Ktot = r*s*c (profiles/conv_split_bf16.md): the split kernel
// replaces the fp32 plan where its 128x128 tile applies (at least one workgroup per CU) and the GEMM is long enough in
// both N and Ktot for six bf16 MFMAs per fragment pair to outrun the fp32 pipe - except where fp32 has a Winograd form,
// which measured faster than the split direct convolution.  0 while a hook pins the fp32 kernels.
extern "C" int frcnn_conv2d_split_bf16_wanted(int n, int h, int w, int c, int k, int r, int s, int stride, int pad) {
  // every hook that picks among the fp32 kernels keeps its meaning: forced tile, algorithm mode and flags, staging
  if (!g_split_bf16 || g_force_tm != 0 || g_algo_mode != 0 || g_wino_fuse != 1 || g_epi_lds != 1 || g_wino_trim != 1 || g_use_dma != 1) return 0;
  if (!conv_args_ok(n, h, w, c, k, r, s, stride, pad) || (c % BK) != 0) return 0;
  const long M = (long)n * ((h + 2 * pad - r) / stride + 1) * ((w + 2 * pad - s) / stride + 1);
  const long ktot = (long)r * s * c;
  if (winograd_ok(r, s, stride, pad, c, k, 1)) return 0;   // F(2x2, 3x3) multiplies 2.25 times less: measured faster in fp32
  return ((M + 127) / 128) * ((k + 127) / 128) >= NUM_CU && k >= 512 && ktot >= 512;
}
