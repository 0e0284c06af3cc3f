// Max-pool 3x3 / stride 2 / pad 1 forward and backward (the ResNet stem), max-pool 2x2 / stride 2 forward and backward (the
// VGG16 body) and the stem's channel padding, NHWC.
#include "common.h"

#include <algorithm>

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// torch's update rule (val > max || isnan(val)), pairwise: a NaN on either side wins
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ f32x4 nan_max4(f32x4 a, f32x4 b) {
  f32x4 m;
  m[0] = nan_max(a[0], b[0]); m[1] = nan_max(a[1], b[1]); m[2] = nan_max(a[2], b[2]); m[3] = nan_max(a[3], b[3]);
  return m;
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// MaxPool 3x3 / stride 2 / pad 1, NHWC (lib/nets/resnet.py:156).  One thread = 4 channels of one
// output pixel; consecutive threads walk the channel dimension -> 16-byte coalesced accesses.
// max is torch's: a NaN in a window makes that output NaN (it beats +inf).
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc(const float* __restrict__ x, float* __restrict__ y, int N,
                                                        int H, int W, int C4, int Ho, int Wo) {
  const size_t total = (size_t)N * Ho * Wo * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    size_t pix = i / C4;
    const int wo = (int)(pix % Wo);
    pix /= Wo;
    const int ho = (int)(pix % Ho);
    const int n = (int)(pix / Ho);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int hi = ho * 2 - 1 + dy;
      if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int wi = wo * 2 - 1 + dx;
        if ((unsigned)wi >= (unsigned)W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + hi) * W + wi) * C4 * 4 + c4 * 4);
        m = nan_max4(m, v);
      }
    }
    *reinterpret_cast<f32x4*>(y + i * 4) = m;
  }
}

__global__ __launch_bounds__(256) void pad_channels_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          size_t pixels, int c, int c_pad) {
  const size_t total = pixels * c_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / c_pad;
    const int ch = (int)(i - pix * c_pad);
    y[i] = ch < c ? x[pix * c + ch] : 0.f;
  }
}
}  // namespace

extern "C" int frcnn_maxpool3x3s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream_) {
  FRCNN_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "maxpool3x3s2_fwd: bad arguments (c%%4==0)");
  const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
  const size_t total = (size_t)n * ho * wo * (c / 4);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048 * 4);
  hipLaunchKernelGGL(maxpool3x3s2_nhwc, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), x, y, n, h, w,
                     c / 4, ho, wo);
  return frcnn::check_launch("maxpool3x3s2_nhwc");
}

// Backward of the 3x3/2 max-pool (autograd of nn.MaxPool2d in the trainable stem, cfg.RESNET.FIXED_BLOCKS == -1):
// gather form, deterministic.  An input pixel lies in at most 2 x 2 windows; it receives dy of a window when it is that
// window's winner in torch's row-major scan (the index its forward stores): an element takes over when val > max ||
// isnan(val) - the FIRST of equal maxima, and the LAST NaN of a window that holds one.
namespace {
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_nhwc(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* __restrict__ dx, int N, int H, int W, int C4, int Ho,
                                                            int Wo) {
  const size_t total = (size_t)N * H * W * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    size_t pix = i / C4;
    const int w = (int)(pix % W);
    pix /= W;
    const int h = (int)(pix % H);
    const int n = (int)(pix / H);
    const f32x4 me = *reinterpret_cast<const f32x4*>(x + i * 4);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    for (int ho = max(0, (h - 1 + 1) / 2); ho <= min(Ho - 1, (h + 1) / 2); ++ho)
      for (int wo = max(0, (w - 1 + 1) / 2); wo <= min(Wo - 1, (w + 1) / 2); ++wo) {
        // is (h, w) the winner of window (ho, wo)?  earlier = strictly before in row-major order.  A finite pixel loses to
        // any NaN (both comparisons are false); a NaN pixel loses only to a later NaN.
        bool first[4] = {true, true, true, true};
        for (int dyy = 0; dyy < 3; ++dyy) {
          const int hi = ho * 2 - 1 + dyy;
          if ((unsigned)hi >= (unsigned)H) continue;
          for (int dxx = 0; dxx < 3; ++dxx) {
            const int wi = wo * 2 - 1 + dxx;
            if ((unsigned)wi >= (unsigned)W || (hi == h && wi == w)) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + hi) * W + wi) * C4 * 4 + c4 * 4);
            const bool earlier = hi < h || (hi == h && wi < w);
            for (int e = 0; e < 4; ++e)
              first[e] = first[e] && (me[e] != me[e] ? (earlier || v[e] == v[e]) : (earlier ? v[e] < me[e] : v[e] <= me[e]));
          }
        }
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((((size_t)n * Ho + ho) * Wo + wo) * C4 + c4) * 4);
        for (int e = 0; e < 4; ++e) g[e] += first[e] ? d[e] : 0.f;
      }
    *reinterpret_cast<f32x4*>(dx + i * 4) = g;
  }
}
}  // namespace

extern "C" int frcnn_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c,
                                      void* stream_) {
  FRCNN_REQUIRE(x && dy && dx && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "maxpool3x3s2_bwd: bad arguments (c%%4==0)");
  const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
  const size_t total = (size_t)n * h * w * (c / 4);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048 * 4);
  hipLaunchKernelGGL(maxpool3x3s2_bwd_nhwc, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), x, dy, dx, n, h,
                     w, c / 4, ho, wo);
  return frcnn::check_launch("maxpool3x3s2_bwd_nhwc");
}

// ------------------------------------------------------------------------------------------------
// MaxPool 2x2 / stride 2, no padding, ceil_mode off, NHWC (lib/nets/vgg16.py:35,46: the 'M' entries of torchvision's
// configuration 'D').  The windows do not overlap: every input float is read once, so the kernel is four 16-byte loads
// per 16-byte store and nothing else.  One lane owns one float4 of channels of one output; neighbouring lanes walk the
// channel axis (a wave reads four runs and writes one run of 1 KB).  The four loads are issued before the first is used.
// The grid is bounded (kPool2MaxBlocks workgroups) and every lane walks the outputs in a grid-stride loop with 64-bit
// offsets.  The last row of an odd H and the last column of an odd W lie in no window and are never read.  max is
// torch's: a NaN in a window makes that output NaN.  (Two outputs per work item measured the same: profiles/vgg16.md.)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int kPool2Threads = 256;
constexpr int kPool2MaxBlocks = FRCNN_MAXPOOL2X2_MAX_LANES / kPool2Threads;   // 8 workgroups per CU

__global__ __launch_bounds__(kPool2Threads) void maxpool2x2s2_nhwc(const f32x4* __restrict__ x, f32x4* __restrict__ y, int H,
                                                                   int W, int C4, int Ho, int Wo, unsigned long long total) {
  const unsigned long long row = (unsigned long long)W * C4;        // float4s of one input row
  for (unsigned long long i = (unsigned long long)blockIdx.x * kPool2Threads + threadIdx.x; i < total;
       i += (unsigned long long)gridDim.x * kPool2Threads) {
    const int c4 = (int)(i % C4);
    unsigned long long p = i / C4;
    const int wo = (int)(p % Wo);
    p /= Wo;
    const int ho = (int)(p % Ho);
    const unsigned long long n = p / Ho;
    const f32x4* src = x + ((n * H + 2 * ho) * W + 2 * wo) * C4 + c4;
    const f32x4 v00 = src[0], v01 = src[C4], v10 = src[row], v11 = src[row + C4];
    y[i] = nan_max4(nan_max4(v00, v01), nan_max4(v10, v11));
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" int frcnn_maxpool2x2s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream_) {
  FRCNN_REQUIRE(x && y, "maxpool2x2s2_fwd: null x / y");
  FRCNN_REQUIRE(n > 0 && h >= 2 && w >= 2 && c > 0 && c % 4 == 0,
                "maxpool2x2s2_fwd: bad shape n=%d h=%d w=%d c=%d (n>0, h>=2, w>=2, c%%4==0)", n, h, w, c);
  FRCNN_REQUIRE(aligned16(x) && aligned16(y), "maxpool2x2s2_fwd: pointers must be 16-byte aligned");
  const int ho = h / 2, wo = w / 2, c4 = c / 4;
  const unsigned long long total = (unsigned long long)n * ho * wo * c4;
  const int blocks = (int)std::min<unsigned long long>((total + kPool2Threads - 1) / kPool2Threads, kPool2MaxBlocks);
  hipLaunchKernelGGL(maxpool2x2s2_nhwc, dim3(blocks), dim3(kPool2Threads), 0, static_cast<hipStream_t>(stream_),
                     reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(y), h, w, c4, ho, wo, total);
  return frcnn::check_launch("maxpool2x2s2_nhwc");
}

// ------------------------------------------------------------------------------------------------
// Backward of the 2x2 / stride 2 max-pool.  The windows do not overlap, so the gradient is a routing: the window's winner
// receives dy, the other three 0.  One lane owns one float4 of channels of one CELL of the ceil(H/2) x ceil(W/2) grid of 2x2
// input blocks: a full cell is a window (four 16-byte loads of x, one of dy, four 16-byte stores), a cell cut by the trailing
// row of an odd H or the trailing column of an odd W lies in no window and its one or two pixels are stored as 0 without a
// load - every element of dx is written by the launch, no memset.  The winner is torch's: scan (0,0), (0,1), (1,0), (1,1),
// an element takes over when val > max || isnan(val) - the first of equal values, the last NaN, (0,0) of four -inf.
// relu_mask: x is the ReLU output of the convolution in front of the pool and dx the gradient of its pre-activation - the
// winner receives dy unless x[winner] <= 0 (act_bwd_kernel's rule: open for a NaN), so no act_bwd pass over dx follows.
// No atomics, no LDS, deterministic; the same bounded grid and 64-bit grid-stride loop as the forward.
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(kPool2Threads) void maxpool2x2s2_bwd_nhwc(const f32x4* __restrict__ x,
                                                                       const f32x4* __restrict__ dy, f32x4* __restrict__ dx,
                                                                       int H, int W, int C4, int Hc, int Wc, int Ho, int Wo,
                                                                       unsigned long long total, int relu_mask) {
  const unsigned long long row = (unsigned long long)W * C4;        // float4s of one input row
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (unsigned long long i = (unsigned long long)blockIdx.x * kPool2Threads + threadIdx.x; i < total;
       i += (unsigned long long)gridDim.x * kPool2Threads) {
    const int c4 = (int)(i % C4);
    unsigned long long p = i / C4;
    const int wc = (int)(p % Wc);
    p /= Wc;
    const int hc = (int)(p % Hc);
    const unsigned long long n = p / Hc;
    const unsigned long long at = ((n * H + 2 * hc) * W + 2 * wc) * C4 + c4;
    const bool has_row = 2 * hc + 1 < H, has_col = 2 * wc + 1 < W;
    if (!(has_row && has_col)) {        // the trailing row / column: in no window
      dx[at] = zero;
      if (has_col) dx[at + C4] = zero;
      if (has_row) dx[at + row] = zero;
      continue;
    }
    const f32x4 v00 = x[at], v01 = x[at + C4], v10 = x[at + row], v11 = x[at + row + C4];
    const f32x4 g = dy[((n * Ho + hc) * Wo + wc) * C4 + c4];
    f32x4 d00, d01, d10, d11;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float m = v00[e];
      int win = 0;
      if (v01[e] > m || v01[e] != v01[e]) { m = v01[e]; win = 1; }
      if (v10[e] > m || v10[e] != v10[e]) { m = v10[e]; win = 2; }
      if (v11[e] > m || v11[e] != v11[e]) { m = v11[e]; win = 3; }
      const float ge = relu_mask ? (frcnn::relu_open(m) ? g[e] : 0.f) : g[e];
      d00[e] = win == 0 ? ge : 0.f;
      d01[e] = win == 1 ? ge : 0.f;
      d10[e] = win == 2 ? ge : 0.f;
      d11[e] = win == 3 ? ge : 0.f;
    }
    dx[at] = d00;
    dx[at + C4] = d01;
    dx[at + row] = d10;
    dx[at + row + C4] = d11;
  }
}
}  // namespace

extern "C" int frcnn_maxpool2x2s2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, int relu_mask,
                                      void* stream_) {
  FRCNN_REQUIRE(x && dy && dx, "maxpool2x2s2_bwd: null x / dy / dx");
  FRCNN_REQUIRE(n > 0 && h >= 2 && w >= 2 && c > 0 && c % 4 == 0,
                "maxpool2x2s2_bwd: bad shape n=%d h=%d w=%d c=%d (n>0, h>=2, w>=2, c%%4==0)", n, h, w, c);
  FRCNN_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx), "maxpool2x2s2_bwd: pointers must be 16-byte aligned");
  const int hc = (h + 1) / 2, wc = (w + 1) / 2, c4 = c / 4;
  const unsigned long long total = (unsigned long long)n * hc * wc * c4;
  const int blocks = (int)std::min<unsigned long long>((total + kPool2Threads - 1) / kPool2Threads, kPool2MaxBlocks);
  hipLaunchKernelGGL(maxpool2x2s2_bwd_nhwc, dim3(blocks), dim3(kPool2Threads), 0, static_cast<hipStream_t>(stream_),
                     reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(dy), reinterpret_cast<f32x4*>(dx), h, w,
                     c4, hc, wc, h / 2, w / 2, total, relu_mask ? 1 : 0);
  return frcnn::check_launch("maxpool2x2s2_bwd_nhwc");
}

extern "C" int frcnn_pad_channels(const float* x, float* y, int64_t pixels, int c, int c_pad, void* stream_) {
  FRCNN_REQUIRE(x && y && pixels > 0 && c > 0 && c_pad >= c, "pad_channels: bad arguments");
  const size_t total = (size_t)pixels * c_pad;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048 * 4);
  hipLaunchKernelGGL(pad_channels_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), x, y,
                     (size_t)pixels, c, c_pad);
  return frcnn::check_launch("pad_channels_kernel");
}
