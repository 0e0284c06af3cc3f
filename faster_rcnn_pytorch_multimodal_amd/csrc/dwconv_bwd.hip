// Gradients of the depthwise 3x3 convolution of csrc/dwconv.hip and the backward of a ReLU6 behind a GEMM convolution: the
// streaming kernels MobileNet-v1 needs under loss.backward() (lib/nets/mobilenet_v1.py:117-123, lib/model/train_val.py:458).
// NHWC, fp32.
//
// Both depthwise gradients read the MASKED upstream gradient dz = dy * scale * m, m = [relu off or not y <= 0] * [not y >= out_cap]
// (hardtanh's backward: zero at both closed ends), computed from dy and the forward's stored output y as they are loaded and
// never stored.  As in the forward, one lane owns ONE float4 of channels for the whole launch and keeps the taps and the
// folded scale in registers, a work item is a strip of FRCNN_DWCONV_STRIP pixels along W, every load is clamped into bounds
// and its value replaced by 0 afterwards, and the grid is bounded: lanes loop over the strips.
//
// Data gradient: GATHER form - a lane sums the (at most 9, at stride 2 at most 4) dz elements its dx pixel was a tap of, so
// every dx element is written once by one lane in a fixed order: no atomics, no zero fill.
// Filter gradient: a reduction over all pixels.  A lane accumulates its 9 x 4 taps over its strips, the lanes of a workgroup
// that own the same channels are summed through LDS in lane order, the workgroup leaves its partial in the caller's workspace,
// and a second small launch sums the partials in workgroup order and writes (or adds into) the parameter's (C,1,3,3) layout.
// No float atomics and no inter-workgroup hand-off inside a launch: two runs are bit-equal.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStrip = FRCNN_DWCONV_STRIP;
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256;      // one workgroup per CU, as the forward
constexpr int kGroupsPerBlock = 32;  // filter gradient: channel groups a workgroup covers - 512 contiguous bytes per pixel
constexpr int kFinalLanes = 16;      // final sum: channel groups per workgroup, and slices of the partials summed side by side
static_assert(kStrip % 2 == 0, "the stride-2 data gradient assumes a strip starts at an even column");
static_assert(kFinalLanes * kFinalLanes == kThreads, "final sum: one workgroup is kFinalLanes x kFinalLanes");

__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }
__device__ __forceinline__ f32x4 vmin(f32x4 a, float cap) {
  return f32x4{frcnn::cap_f32(a[0], cap), frcnn::cap_f32(a[1], cap), frcnn::cap_f32(a[2], cap), frcnn::cap_f32(a[3], cap)};
}
__device__ __forceinline__ float mask1(float g, float y, float cap, int relu) {
  return ((relu && y <= 0.f) || y >= cap) ? 0.f : g;   // hardtanh_backward: open for a NaN y
}
// dz of one float4: g = dy * scale already; y is read only when MASK
template <bool MASK>
__device__ __forceinline__ f32x4 masked(f32x4 g, f32x4 y, float cap, int relu) {
  if (!MASK) return g;
  return f32x4{mask1(g[0], y[0], cap, relu), mask1(g[1], y[1], cap, relu), mask1(g[2], y[2], cap, relu),
               mask1(g[3], y[3], cap, relu)};
}

// lanes: number of working threads, a multiple of C4 (c4 = thread % C4 is fixed for the launch); items = N * H * strips of dx.
template <int STRIDE, bool MASK>
__global__ __launch_bounds__(kThreads) void dwconv3x3_bwd_data_nhwc(const float* __restrict__ dy, const float* __restrict__ y,
                                                                    const float* __restrict__ wt, const float* __restrict__ scale,
                                                                    float* __restrict__ dx, int H, int W, int C4, int OH, int OW,
                                                                    int strips, long long items, unsigned lanes, float out_cap,
                                                                    int relu) {
  // dz columns / rows one strip of dx reads: stride 1 - columns w0-1 .. w0+kStrip, rows h+1, h, h-1 (filter rows 0, 1, 2);
  // stride 2 - columns w0/2 .. w0/2 + kStrip/2; an odd row h is a tap of rows (h+1)/2 (filter row 0) and (h-1)/2 (filter row
  // 2), an even row of h/2 alone (filter row 1)
  constexpr int NC = STRIDE == 1 ? kStrip + 2 : kStrip / 2 + 1;
  constexpr int NR = STRIDE == 1 ? 3 : 2;
  const unsigned t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= lanes) return;
  const int c4 = (int)(t % (unsigned)C4);
  const long long step = lanes / (unsigned)C4;
  const size_t C = (size_t)C4 * 4;

  f32x4 wk[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) wk[i] = *reinterpret_cast<const f32x4*>(wt + (size_t)i * C + (size_t)c4 * 4);
  const f32x4 sc = scale ? *reinterpret_cast<const f32x4*>(scale + (size_t)c4 * 4) : splat(1.f);

  for (long long p = t / (unsigned)C4; p < items; p += step) {
    const int st = (int)(p % strips);
    const long long q = p / strips;
    const int h = (int)(q % H);
    const long long n = q / H;
    const int w0 = st * kStrip;
    const bool odd = (h & 1) != 0;
    const int ow_lo = STRIDE == 1 ? w0 - 1 : w0 / 2;
    const size_t img = (size_t)n * OH * OW * C + (size_t)c4 * 4;

    size_t row_off[NR];
    bool row_ok[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int oh = STRIDE == 1 ? h + 1 - i : (i == 0 ? (h + 1) >> 1 : (h - 1) >> 1);
      row_ok[i] = (unsigned)oh < (unsigned)OH && (STRIDE == 1 || i == 0 || odd);
      row_off[i] = (size_t)min(max(oh, 0), OH - 1) * OW * C;
    }
    // every load is in bounds: a tap outside the map reads the clamped element and is replaced by 0 afterwards
    f32x4 g[NR][NC], yy[NR][NC];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const size_t off = img + row_off[i] + (size_t)min(max(ow_lo + j, 0), OW - 1) * C;
        g[i][j] = *reinterpret_cast<const f32x4*>(dy + off);
        yy[i][j] = MASK ? *reinterpret_cast<const f32x4*>(y + off) : splat(0.f);
      }
    }
    f32x4 dz[NR][NC];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const bool ok = row_ok[i] && (unsigned)(ow_lo + j) < (unsigned)OW;
        dz[i][j] = ok ? masked<MASK>(g[i][j] * sc, yy[i][j], out_cap, relu) : splat(0.f);
      }
    }
    float* out = dx + (((size_t)n * H + h) * W + w0) * C + (size_t)c4 * 4;
#pragma unroll
    for (int o = 0; o < kStrip; ++o) {
      f32x4 acc = splat(0.f);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int d = o + 1 - s;      // dx column w0 + o is tap s of output column (w0 + d) / STRIDE when that divides
          if (STRIDE == 2 && (d & 1)) continue;
          const int j = STRIDE == 1 ? d + 1 : d / 2;
          const f32x4 wv = STRIDE == 1 ? wk[i * 3 + s] : (i == 0 ? (odd ? wk[s] : wk[3 + s]) : wk[6 + s]);
          acc += wv * dz[i][j];
        }
      }
      if (w0 + o < W) *reinterpret_cast<f32x4*>(out + (size_t)o * C) = acc;
    }
  }
}

// Filter gradient, first launch.  A workgroup covers CW = min(C4, kGroupsPerBlock) channel groups (blockIdx.y selects which)
// in S = kThreads / CW pixel slots: thread -> (slot = thread / CW, channel group = thread % CW); threads beyond S * CW idle.
// The slots are summed in LDS, so a workgroup leaves ONE partial per channel group: few channel groups per workgroup mean
// few partials (C = 512: 64 partials of 18 KB instead of 256 of 72 KB with every channel in every workgroup).
// items = N * OH * strips of the OUTPUT map.  ws: [gridDim.x][9][C4] float4 partials.
template <int STRIDE, bool MASK>
__global__ __launch_bounds__(kThreads) void dwconv3x3_bwd_weight_partial(const float* __restrict__ x, const float* __restrict__ dy,
                                                                         const float* __restrict__ y,
                                                                         const float* __restrict__ scale, f32x4* __restrict__ ws,
                                                                         int H, int W, int C4, int OH, int OW, int strips,
                                                                         long long items, int CW, int S, float in_cap,
                                                                         float out_cap, int relu) {
  constexpr int COLS = (kStrip - 1) * STRIDE + 3;
  __shared__ f32x4 red[9][kThreads];
  const int tid = threadIdx.x;
  const int slot = tid / CW;
  const int c4 = blockIdx.y * CW + tid % CW;
  const size_t C = (size_t)C4 * 4;

  f32x4 acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = splat(0.f);
  if (slot < S && c4 < C4) {
    const f32x4 sc = scale ? *reinterpret_cast<const f32x4*>(scale + (size_t)c4 * 4) : splat(1.f);
    const long long step = (long long)gridDim.x * S;
    for (long long p = (long long)blockIdx.x * S + slot; p < items; p += step) {
      const int st = (int)(p % strips);
      const long long q = p / strips;
      const int oh = (int)(q % OH);
      const long long n = q / OH;
      const int ow0 = st * kStrip;
      const int hi0 = oh * STRIDE - 1, wi0 = ow0 * STRIDE - 1;
      const float* xin = x + (size_t)n * H * W * C + (size_t)c4 * 4;
      const size_t orow = (((size_t)n * OH + oh) * OW) * C + (size_t)c4 * 4;

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
        const size_t col_off = (size_t)min(max(wi0 + j, 0), W - 1) * C;
#pragma unroll
        for (int r = 0; r < 3; ++r) v[j][r] = *reinterpret_cast<const f32x4*>(xin + row_off[r] + col_off);
      }
      f32x4 g[kStrip], yy[kStrip];
#pragma unroll
      for (int o = 0; o < kStrip; ++o) {
        const size_t off = orow + (size_t)min(ow0 + o, OW - 1) * C;
        g[o] = *reinterpret_cast<const f32x4*>(dy + off);
        yy[o] = MASK ? *reinterpret_cast<const f32x4*>(y + off) : splat(0.f);
      }
      f32x4 dz[kStrip];
#pragma unroll
      for (int o = 0; o < kStrip; ++o) dz[o] = ow0 + o < OW ? masked<MASK>(g[o] * sc, yy[o], out_cap, relu) : splat(0.f);
#pragma unroll
      for (int j = 0; j < COLS; ++j) {
        const bool col_ok = (unsigned)(wi0 + j) < (unsigned)W;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const f32x4 a = (col_ok && row_ok[r]) ? vmin(v[j][r], in_cap) : splat(0.f);
#pragma unroll
          for (int o = 0; o < kStrip; ++o) {
            const int s = j - o * STRIDE;      // the filter column this input column is for output o of the strip
            if (s >= 0 && s < 3) acc[r * 3 + s] += dz[o] * a;
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) red[i][tid] = acc[i];
  __syncthreads();
  // the slots of a channel group, summed in slot order
  for (int i = tid; i < 9 * CW; i += kThreads) {
    const int tap = i / CW, cw = i % CW;
    const int c = blockIdx.y * CW + cw;
    if (c >= C4) continue;
    f32x4 sum = red[tap][cw];
    for (int s = 1; s < S; ++s) sum += red[tap][s * CW + cw];
    ws[((size_t)blockIdx.x * 9 + tap) * C4 + c] = sum;
  }
}

// Filter gradient, second launch: dw[c,0,r,s] (+)= sum over the `blocks` partials, in a fixed order - kFinalLanes slices of
// the partials (slice i takes partials i, i + kFinalLanes, ...) are summed side by side, then the slices in slice order.
// blockIdx.x: kFinalLanes channel groups, blockIdx.y: the tap.
__global__ __launch_bounds__(kThreads) void dwconv3x3_bwd_weight_final(const f32x4* __restrict__ ws, float* __restrict__ dw, int C4,
                                                                       int blocks, int accumulate) {
  __shared__ f32x4 red[kFinalLanes][kFinalLanes];
  const int cl = threadIdx.x % kFinalLanes, slice = threadIdx.x / kFinalLanes;
  const int tap = blockIdx.y;
  const int c4 = blockIdx.x * kFinalLanes + cl;
  f32x4 sum = splat(0.f);
  if (c4 < C4)
    for (int b = slice; b < blocks; b += kFinalLanes) sum += ws[((size_t)b * 9 + tap) * C4 + c4];
  red[slice][cl] = sum;
  __syncthreads();
  if (slice == 0 && c4 < C4) {
    f32x4 tot = red[0][cl];
    for (int i = 1; i < kFinalLanes; ++i) tot += red[i][cl];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* p = dw + ((size_t)c4 * 4 + j) * 9 + tap;
      *p = accumulate ? *p + tot[j] : tot[j];
    }
  }
}

// d_conv = dy * scale[k] * [y > 0 if relu] * [y < cap] over count = rows * k floats: float4 body, scalar tail.
template <bool MASK>
__global__ __launch_bounds__(kThreads) void act_bwd_cap_kernel(const float* dy, const float* y, const float* __restrict__ scale,
                                                               float* d_conv, size_t count, int k, float cap, int relu) {
  const size_t vecs = count / 4;
  const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, step = (size_t)gridDim.x * kThreads;
  const bool k4 = k % 4 == 0;
  for (size_t i = tid; i < vecs; i += step) {
    f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
    if (scale) {
      if (k4) {
        g *= *reinterpret_cast<const f32x4*>(scale + (i * 4) % (size_t)k);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] *= scale[(i * 4 + j) % (size_t)k];
      }
    }
    f32x4 yy = splat(0.f);
    if (MASK) yy = reinterpret_cast<const f32x4*>(y)[i];
    reinterpret_cast<f32x4*>(d_conv)[i] = masked<MASK>(g, yy, cap, relu);
  }
  const size_t i = vecs * 4 + tid;      // count % 4 trailing elements
  if (i < count) {
    const float g = scale ? dy[i] * scale[i % (size_t)k] : dy[i];
    d_conv[i] = MASK ? mask1(g, y[i], cap, relu) : g;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct WeightPlan {
  int cw, chunks, slots, blocks, strips;
  long long items;
};

// the launch geometry of the filter gradient, shared by the workspace query and the launch
WeightPlan weight_plan(int n, int h, int w, int c, int stride) {
  WeightPlan p;
  const int c4 = c / 4;
  const int oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  p.cw = std::min(c4, kGroupsPerBlock);
  p.chunks = (c4 + p.cw - 1) / p.cw;
  p.slots = kThreads / p.cw;
  p.strips = (ow + kStrip - 1) / kStrip;
  p.items = (long long)n * oh * p.strips;
  const long long want = (p.items + p.slots - 1) / p.slots;
  p.blocks = (int)std::max<long long>(1, std::min<long long>(want, std::max(1, kMaxBlocks / p.chunks)));
  return p;
}

bool shape_ok(int n, int h, int w, int c, int stride) {
  return n >= 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && (stride == 1 || stride == 2) && c / 4 <= kMaxBlocks * kThreads;
}
}  // namespace

extern "C" int frcnn_dwconv3x3_bwd_data(const float* dy, const float* y, const float* w_rsc, const float* scale, float* dx, int n,
                                        int h, int w, int c, int stride, float out_cap, int relu, void* stream_) {
  FRCNN_REQUIRE(dy && w_rsc && dx, "dwconv3x3_bwd_data: null dy / w_rsc / dx");
  FRCNN_REQUIRE(shape_ok(n, h, w, c, stride), "dwconv3x3_bwd_data: bad shape n=%d h=%d w=%d c=%d (c%%4==0) stride=%d (1 or 2)", n,
                h, w, c, stride);
  const bool mask = relu || out_cap < INFINITY;
  FRCNN_REQUIRE(y || !mask, "dwconv3x3_bwd_data: null y with relu or a finite out_cap");
  FRCNN_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(w_rsc) && aligned16(scale) && aligned16(dx),
                "dwconv3x3_bwd_data: pointers must be 16-byte aligned");
  if (n == 0) return FRCNN_OK;
  const int c4 = c / 4;
  const int oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  const int strips = (w + kStrip - 1) / kStrip;
  const long long items = (long long)n * h * strips;
  const unsigned long long total = (unsigned long long)items * c4;
  const int blocks = (int)std::min<unsigned long long>((total + kThreads - 1) / kThreads, kMaxBlocks);
  const unsigned lanes = (unsigned)(blocks * kThreads) / (unsigned)c4 * (unsigned)c4;      // >= c4: total >= c4
  hipStream_t stream = static_cast<hipStream_t>(stream_);
#define FRCNN_DW_BWD_DATA(ST, MK)                                                                                               \
  hipLaunchKernelGGL((dwconv3x3_bwd_data_nhwc<ST, MK>), dim3(blocks), dim3(kThreads), 0, stream, dy, y, w_rsc, scale, dx, h, w, \
                     c4, oh, ow, strips, items, lanes, out_cap, relu)
  if (stride == 1) {
    if (mask) FRCNN_DW_BWD_DATA(1, true); else FRCNN_DW_BWD_DATA(1, false);
  } else {
    if (mask) FRCNN_DW_BWD_DATA(2, true); else FRCNN_DW_BWD_DATA(2, false);
  }
#undef FRCNN_DW_BWD_DATA
  return frcnn::check_launch("dwconv3x3_bwd_data_nhwc");
}

extern "C" size_t frcnn_dwconv3x3_bwd_weight_ws_bytes(int n, int h, int w, int c, int stride) {
  if (!shape_ok(n, h, w, c, stride) || n == 0) return 0;
  return (size_t)weight_plan(n, h, w, c, stride).blocks * 9 * (size_t)(c / 4) * sizeof(f32x4);
}

extern "C" int frcnn_dwconv3x3_bwd_weight(const float* x, const float* dy, const float* y, const float* scale, float* dw, int n,
                                          int h, int w, int c, int stride, float in_cap, float out_cap, int relu, int accumulate,
                                          void* ws, size_t ws_bytes, void* stream_) {
  FRCNN_REQUIRE(x && dy && dw, "dwconv3x3_bwd_weight: null x / dy / dw");
  FRCNN_REQUIRE(shape_ok(n, h, w, c, stride), "dwconv3x3_bwd_weight: bad shape n=%d h=%d w=%d c=%d (c%%4==0) stride=%d (1 or 2)",
                n, h, w, c, stride);
  FRCNN_REQUIRE(accumulate == 0 || accumulate == 1, "dwconv3x3_bwd_weight: accumulate %d (0 or 1)", accumulate);
  const bool mask = relu || out_cap < INFINITY;
  FRCNN_REQUIRE(y || !mask, "dwconv3x3_bwd_weight: null y with relu or a finite out_cap");
  FRCNN_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(scale) && aligned16(dw) && aligned16(ws),
                "dwconv3x3_bwd_weight: pointers must be 16-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n == 0) {
    if (!accumulate && frcnn::fill_bytes(dw, 0, (size_t)c * 9 * sizeof(float), stream) != hipSuccess)
      return frcnn::fail(FRCNN_ERR_LAUNCH, "dwconv3x3_bwd_weight: zero fill failed");
    return FRCNN_OK;
  }
  const size_t need = frcnn_dwconv3x3_bwd_weight_ws_bytes(n, h, w, c, stride);
  FRCNN_REQUIRE(ws && ws_bytes >= need, "dwconv3x3_bwd_weight: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const WeightPlan p = weight_plan(n, h, w, c, stride);
  const int c4 = c / 4;
  const int oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  f32x4* part = static_cast<f32x4*>(ws);
#define FRCNN_DW_BWD_WEIGHT(ST, MK)                                                                                          \
  hipLaunchKernelGGL((dwconv3x3_bwd_weight_partial<ST, MK>), dim3(p.blocks, p.chunks), dim3(kThreads), 0, stream, x, dy, y,  \
                     scale, part, h, w, c4, oh, ow, p.strips, p.items, p.cw, p.slots, in_cap, out_cap, relu)
  if (stride == 1) {
    if (mask) FRCNN_DW_BWD_WEIGHT(1, true); else FRCNN_DW_BWD_WEIGHT(1, false);
  } else {
    if (mask) FRCNN_DW_BWD_WEIGHT(2, true); else FRCNN_DW_BWD_WEIGHT(2, false);
  }
#undef FRCNN_DW_BWD_WEIGHT
  int rc = frcnn::check_launch("dwconv3x3_bwd_weight_partial");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(dwconv3x3_bwd_weight_final, dim3((c4 + kFinalLanes - 1) / kFinalLanes, 9), dim3(kThreads), 0, stream, part,
                     dw, c4, p.blocks, accumulate);
  return frcnn::check_launch("dwconv3x3_bwd_weight_final");
}

extern "C" int frcnn_act_bwd_cap(const float* dy, const float* y, const float* scale, int relu, float cap, int64_t rows, int k,
                                 float* d_conv, void* stream_) {
  FRCNN_REQUIRE(rows >= 0 && k > 0, "act_bwd_cap: bad shape rows=%lld k=%d", (long long)rows, k);
  const size_t count = (size_t)rows * (size_t)k;
  if (count == 0) return FRCNN_OK;
  const bool mask = relu || cap < INFINITY;
  FRCNN_REQUIRE(dy && d_conv, "act_bwd_cap: null dy / d_conv");
  FRCNN_REQUIRE(y || !mask, "act_bwd_cap: null y with relu or a finite cap");
  FRCNN_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(scale) && aligned16(d_conv),
                "act_bwd_cap: pointers must be 16-byte aligned");
  const size_t work = std::max<size_t>(count / 4, 4);      // >= 4 threads: the tail has up to 3 elements
  const int blocks = (int)std::min<size_t>((work + kThreads - 1) / kThreads, 2048);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (mask)
    hipLaunchKernelGGL(act_bwd_cap_kernel<true>, dim3(blocks), dim3(kThreads), 0, stream, dy, y, scale, d_conv, count, k, cap, relu);
  else
    hipLaunchKernelGGL(act_bwd_cap_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream, dy, y, scale, d_conv, count, k, cap,
                       relu);
  return frcnn::check_launch("act_bwd_cap_kernel");
}
