// Depthwise 3x3 convolution (groups == C) with a folded BatchNorm / ReLU6 epilogue, and the in-place upper clamp that
// finishes a ReLU6 behind a GEMM convolution: the two streaming kernels of the MobileNet-v1 backbone
// (lib/nets/mobilenet_v1.py:117-123 conv_dw).  NHWC, fp32.
//
// A depthwise convolution moves 8 bytes per 9 multiply-adds: it is bandwidth-bound and no GEMM.  One lane owns ONE float4
// of channels for the whole launch - the channel groups of a pixel lie on neighbouring lanes, so C/4 lanes read 4*C
// contiguous bytes - and keeps its 9 x 4 filter taps, scale and shift in registers.  A work item is a strip of
// FRCNN_DWCONV_STRIP outputs along W: the lane walks the strip's input columns once, reads the three rows of a column and
// adds them into every output of the strip the column is a tap of, so an input float4 is read once per strip, not once
// per tap.  Rows shared by vertically adjacent strips, and the halo columns of neighbouring strips, come from L2.
// The grid is bounded (kMaxBlocks workgroups); every lane walks the strips in a loop.
#include "common.h"

#include <algorithm>

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStrip = FRCNN_DWCONV_STRIP;
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256;      // one workgroup per CU: a lane has 3 * (kStrip * stride + 1) 16-byte loads in flight

__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }
__device__ __forceinline__ f32x4 vmin(f32x4 a, float cap) {
  return f32x4{frcnn::cap_f32(a[0], cap), frcnn::cap_f32(a[1], cap), frcnn::cap_f32(a[2], cap), frcnn::cap_f32(a[3], cap)};
}
__device__ __forceinline__ f32x4 vmax0(f32x4 a) {
  return f32x4{frcnn::relu_f32(a[0]), frcnn::relu_f32(a[1]), frcnn::relu_f32(a[2]), frcnn::relu_f32(a[3])};
}

// lanes: number of working threads, a multiple of C4 (so c4 = thread % C4 is fixed for the launch); items = N * OH * strips.
template <int STRIDE>
__global__ __launch_bounds__(kThreads) void dwconv3x3_nhwc(const float* __restrict__ x, const float* __restrict__ wt,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           float* __restrict__ y, int H, int W, int C4, int OH, int OW,
                                                           int strips, long long items, unsigned lanes, float in_cap,
                                                           float out_cap, int relu) {
  constexpr int COLS = (kStrip - 1) * STRIDE + 3;
  const unsigned t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= lanes) return;
  const int c4 = (int)(t % (unsigned)C4);
  const long long step = lanes / (unsigned)C4;
  const size_t C = (size_t)C4 * 4;

  f32x4 wk[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) wk[i] = *reinterpret_cast<const f32x4*>(wt + (size_t)i * C + (size_t)c4 * 4);
  const f32x4 sc = scale ? *reinterpret_cast<const f32x4*>(scale + (size_t)c4 * 4) : splat(1.f);
  const f32x4 sh = shift ? *reinterpret_cast<const f32x4*>(shift + (size_t)c4 * 4) : splat(0.f);

  for (long long p = t / (unsigned)C4; p < items; p += step) {
    const int st = (int)(p % strips);
    const long long q = p / strips;
    const int oh = (int)(q % OH);
    const long long n = q / OH;
    const int ow0 = st * kStrip;
    const int hi0 = oh * STRIDE - 1, wi0 = ow0 * STRIDE - 1;
    const float* xin = x + (size_t)n * H * W * C + (size_t)c4 * 4;

    // every load is in bounds: a tap outside the image reads the clamped pixel and is replaced by 0 afterwards, so the
    // loads of a strip carry no branch and are all in flight together
    size_t row_off[3];
    bool row_ok[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hi = hi0 + r;
      row_ok[r] = (unsigned)hi < (unsigned)H;
      row_off[r] = (size_t)min(max(hi, 0), H - 1) * W * C;
    }
    f32x4 v[COLS][3];
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
      const int wi = wi0 + j;
      const size_t col_off = (size_t)min(max(wi, 0), W - 1) * C;
#pragma unroll
      for (int r = 0; r < 3; ++r) v[j][r] = *reinterpret_cast<const f32x4*>(xin + row_off[r] + col_off);
    }
    f32x4 acc[kStrip];
#pragma unroll
    for (int o = 0; o < kStrip; ++o) acc[o] = splat(0.f);
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
      const bool col_ok = (unsigned)(wi0 + j) < (unsigned)W;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const f32x4 a = (col_ok && row_ok[r]) ? vmin(v[j][r], in_cap) : splat(0.f);
#pragma unroll
        for (int o = 0; o < kStrip; ++o) {
          const int s = j - o * STRIDE;      // the filter column this input column is for output o of the strip
          if (s >= 0 && s < 3) acc[o] += wk[r * 3 + s] * a;
        }
      }
    }
    float* yout = y + (((size_t)n * OH + oh) * OW + ow0) * C + (size_t)c4 * 4;
#pragma unroll
    for (int o = 0; o < kStrip; ++o) {
      if (ow0 + o < OW) {
        f32x4 r = acc[o] * sc + sh;
        if (relu) r = vmax0(r);
        *reinterpret_cast<f32x4*>(yout + (size_t)o * C) = vmin(r, out_cap);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void clamp_max_kernel(float* __restrict__ x, size_t count, float cap) {
  const size_t vecs = count / 4;
  const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, step = (size_t)gridDim.x * kThreads;
  for (size_t i = tid; i < vecs; i += step) {
    f32x4* p = reinterpret_cast<f32x4*>(x) + i;
    *p = vmin(*p, cap);
  }
  const size_t i = vecs * 4 + tid;      // count % 4 trailing elements
  if (i < count) x[i] = frcnn::cap_f32(x[i], cap);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" int frcnn_dwconv3x3_fwd(const float* x, const float* w_rsc, const float* scale, const float* shift, float* y,
                                   int n, int h, int w, int c, int stride, float in_cap, float out_cap, int relu,
                                   void* stream_) {
  FRCNN_REQUIRE(x && w_rsc && y, "dwconv3x3_fwd: null x / w_rsc / y");
  FRCNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "dwconv3x3_fwd: bad shape n=%d h=%d w=%d c=%d (c%%4==0)",
                n, h, w, c);
  FRCNN_REQUIRE(stride == 1 || stride == 2, "dwconv3x3_fwd: stride %d (1 or 2)", stride);
  FRCNN_REQUIRE(c / 4 <= kMaxBlocks * kThreads, "dwconv3x3_fwd: c=%d above %d", c, 4 * kMaxBlocks * kThreads);
  FRCNN_REQUIRE(aligned16(x) && aligned16(w_rsc) && aligned16(y) && aligned16(scale) && aligned16(shift),
                "dwconv3x3_fwd: pointers must be 16-byte aligned");
  if (n == 0) return FRCNN_OK;
  const int c4 = c / 4;
  const int oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  const int strips = (ow + kStrip - 1) / kStrip;
  const long long items = (long long)n * oh * strips;
  const unsigned long long total = (unsigned long long)items * c4;
  const int blocks = (int)std::min<unsigned long long>((total + kThreads - 1) / kThreads, kMaxBlocks);
  const unsigned lanes = (unsigned)(blocks * kThreads) / (unsigned)c4 * (unsigned)c4;      // >= c4: total >= c4
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (stride == 1)
    hipLaunchKernelGGL(dwconv3x3_nhwc<1>, dim3(blocks), dim3(kThreads), 0, stream, x, w_rsc, scale, shift, y, h, w, c4, oh, ow,
                       strips, items, lanes, in_cap, out_cap, relu);
  else
    hipLaunchKernelGGL(dwconv3x3_nhwc<2>, dim3(blocks), dim3(kThreads), 0, stream, x, w_rsc, scale, shift, y, h, w, c4, oh, ow,
                       strips, items, lanes, in_cap, out_cap, relu);
  return frcnn::check_launch("dwconv3x3_nhwc");
}

extern "C" int frcnn_clamp_max(float* x, int64_t count, float cap, void* stream_) {
  FRCNN_REQUIRE(count >= 0 && (x || count == 0), "clamp_max: bad arguments");
  if (count == 0) return FRCNN_OK;
  FRCNN_REQUIRE(aligned16(x), "clamp_max: x must be 16-byte aligned");
  const size_t work = std::max<size_t>((size_t)count / 4, 4);      // >= 4 threads: the tail has up to 3 elements
  const int blocks = (int)std::min<size_t>((work + kThreads - 1) / kThreads, 2048);
  hipLaunchKernelGGL(clamp_max_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream_), x, (size_t)count,
                     cap);
  return frcnn::check_launch("clamp_max_kernel");
}
