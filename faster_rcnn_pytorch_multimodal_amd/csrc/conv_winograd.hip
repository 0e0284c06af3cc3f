// ------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) for the 3x3 / stride 1 / pad 1 layers with large GEMMs (layer4's conv2 on the 300 RoIs, the RPN
// 3x3): Y = A^T [ (G g G^T) . (B^T d B) ] A per 2x2 output tile, i.e. 16 independent GEMMs over (tiles x C) x (C x K)
// instead of one over (pixels x 9C) x (9C x K): 2.25x fewer multiplications (1.72x on a 7x7 map, whose 4x4 tiles cover
// 8x8).  Same fp32 arithmetic type; the transforms only add and halve, and the reduction is 9x shorter, so the
// rounding error is that of the direct form or smaller (tests/test_gpu_parity.py compares both with float64).
// Four launches: filter transform (stateless ABI: recomputed per call, 16 KC floats), input transform, ONE grouped
// launch of the implicit-GEMM kernels as a 1x1 convolution (blockIdx.y = transform component), output transform with
// the BatchNorm scale / shift, (frcnn_conv2d_fwd_wres_pre only) the residual, and ReLU.  Only the autotuner selects it
// (choose_plan never does).
//
// Trimmed components.  A map with odd H has a last tile row whose second output row falls off the map; in Y = A^T M A,
// A^T = [[1,1,1,0],[0,1,-1,-1]], component row i = 3 feeds nothing but that output row, so the four components (3, j) of
// such a tile are never used - likewise (i, 3) in the last tile column of a map with odd W.  They are not computed: with
// eh = H & 1, ew = W & 1, fh = th - eh, fw = tw - ew the tiles fall into four classes, interior (n fh fw tiles), right edge
// (n fh ew), bottom edge (n eh fw) and corner (n eh ew), and the rows of a component's plane are class-major
// [interior | right | bottom | corner] with the classes that lack the component left out:
//   i != 3, j != 3 (9 components): T rows          i == 3, j != 3 (3): nI + nR rows
//   i != 3, j == 3 (3): nI + nB rows               i == 3, j == 3 (1): nI rows
// so the grouped GEMM runs 9 T + 3 (nI + nR) + 3 (nI + nB) + nI rows instead of 16 T (67 500 instead of 76 800 on the
// 300 RoIs x 7 x 7 of layer4: -12.1 %; nothing changes on an even x even map, where nI = T and this IS the plain tile order),
// and V and M shrink alike.  Planes keep their stride T C / T K (the trimmed ones are sparse at their tail; the workspace
// layout does not change), U stays (16, K, C).  Every surviving M[comp][tile][k] is the same k-ordered fma chain and every
// output the same sum of the same components: no output bit changes.  frcnn_conv2d_set_algo flag 128 turns it off (A/B).
// ------------------------------------------------------------------------------------------------
#include "conv_common.h"

using namespace frcnn::conv;

bool frcnn::conv::winograd_ok(int r, int s, int stride, int pad, int c, int k, int out_stride) {
  return r == 3 && s == 3 && stride == 1 && pad == 1 && (c % 4) == 0 && (k % 4) == 0 && out_stride == 1;
}

namespace {

// tile classes of the trimmed layout, as the transform kernels need them (kernel argument)
struct WinoClasses {
  int fh, fw;        // tile rows / columns whose 2x2 outputs are all inside the map
  int eh, ew;        // 1: a partial last tile row / column exists and its unused components are left out
  long nI, nR, nB;   // interior, right-edge and bottom-edge tiles in the batch (the corner tiles follow them)
};
struct WinoGeom {
  int th, tw;        // 2x2 output tiles per image
  long T;            // tiles in the batch
  size_t u_off, v_off, m_off, bytes;   // workspace layout (bytes)
  WinoClasses cl;
  long rows[4];      // GEMM rows by component kind, the order of ConvParams::grows
};
// trim = false: every tile is an interior tile of the plain (n, ty, tx) order and every component has T rows
WinoGeom wino_geom(int n, int h, int w, int c, int k, bool trim = false) {
  WinoGeom g;
  g.th = (h + 1) / 2;
  g.tw = (w + 1) / 2;
  g.T = (long)n * g.th * g.tw;
  g.cl.eh = trim ? (h & 1) : 0;
  g.cl.ew = trim ? (w & 1) : 0;
  g.cl.fh = g.th - g.cl.eh;
  g.cl.fw = g.tw - g.cl.ew;
  g.cl.nI = (long)n * g.cl.fh * g.cl.fw;
  g.cl.nR = (long)n * g.cl.fh * g.cl.ew;
  g.cl.nB = (long)n * g.cl.eh * g.cl.fw;
  g.rows[0] = g.T;
  g.rows[1] = g.cl.nI + g.cl.nR;
  g.rows[2] = g.cl.nI + g.cl.nB;
  g.rows[3] = g.cl.nI;
  g.u_off = 0;
  g.v_off = frcnn::align_up((size_t)16 * k * c * sizeof(float), 256);
  g.m_off = g.v_off + frcnn::align_up((size_t)16 * g.T * c * sizeof(float), 256);
  g.bytes = g.m_off + frcnn::align_up((size_t)16 * g.T * k * sizeof(float), 256);
  return g;
}

}  // namespace

size_t frcnn::conv::winograd_ws_bytes(int n, int h, int w, int c, int k) { return wino_geom(n, h, w, c, k).bytes; }

namespace {

// U[i*4+j][k][c] = (G g G^T)[i][j],  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]];  one thread per (k, 4 channels)
__global__ __launch_bounds__(256) void wino_filter_kernel(const float* __restrict__ w, float* __restrict__ U, int K,
                                                         int C4) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)K * C4) return;
  const int c4 = (int)(idx % C4);
  const int k = (int)(idx / C4);
  const f32x4* src = reinterpret_cast<const f32x4*>(w) + (size_t)k * 9 * C4 + c4;
  f32x4 g[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) g[r][q] = src[(size_t)(r * 3 + q) * C4];
  f32x4 t[4][3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    t[0][q] = g[0][q];
    t[1][q] = (g[0][q] + g[1][q] + g[2][q]) * 0.5f;
    t[2][q] = (g[0][q] - g[1][q] + g[2][q]) * 0.5f;
    t[3][q] = g[2][q];
  }
  f32x4* dst = reinterpret_cast<f32x4*>(U) + (size_t)k * C4 + c4;
  const size_t plane = (size_t)K * C4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dst[(size_t)(i * 4 + 0) * plane] = t[i][0];
    dst[(size_t)(i * 4 + 1) * plane] = (t[i][0] + t[i][1] + t[i][2]) * 0.5f;
    dst[(size_t)(i * 4 + 2) * plane] = (t[i][0] - t[i][1] + t[i][2]) * 0.5f;
    dst[(size_t)(i * 4 + 3) * plane] = t[i][2];
  }
}

// Row of tile (n, ty, tx) in the planes of the four component kinds (the order of ConvParams::grows), -1 where the tile's
// class lacks the component.  Untrimmed (eh = ew = 0) every tile is interior and all four are the plain tile index.
__device__ __forceinline__ void wino_tile_rows(const WinoClasses& cl, int n, int ty, int tx, long (&row)[4]) {
  const bool be = cl.eh && ty == cl.fh, re = cl.ew && tx == cl.fw;
  if (!be && !re) {
    row[0] = row[1] = row[2] = row[3] = ((long)n * cl.fh + ty) * cl.fw + tx;
  } else if (!be) {                        // right edge: no component (i, 3)
    row[0] = row[1] = cl.nI + (long)n * cl.fh + ty;
    row[2] = row[3] = -1;
  } else if (!re) {                        // bottom edge: no component (3, j)
    row[0] = cl.nI + cl.nR + (long)n * cl.fw + tx;
    row[2] = cl.nI + (long)n * cl.fw + tx;
    row[1] = row[3] = -1;
  } else {                                 // corner: neither
    row[0] = cl.nI + cl.nR + cl.nB + n;
    row[1] = row[2] = row[3] = -1;
  }
}

// V[i*4+j][row][c] = (B^T d B)[i][j] of the 4x4 input patch of tile t (rows 2ty-1.., cols 2tx-1.., zero outside the map);
// B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]].  One thread per (tile, 4 channels): lanes run along the channels.
// Only the components the tile's class has are written, at the tile's row in that component's plane (wino_tile_rows).
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, float* __restrict__ V, int H, int W,
                                                        int C4, int th, int tw, long T, const WinoClasses cl) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)T * C4) return;
  const int c4 = (int)(idx % C4);
  const long t = (long)(idx / C4);
  const int tx = (int)(t % tw);
  const long t2 = t / tw;
  const int ty = (int)(t2 % th);
  const int n = (int)(t2 / th);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 d[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int hi = 2 * ty - 1 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int wi = 2 * tx - 1 + j;
      const bool ok = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
      d[i][j] = ok ? reinterpret_cast<const f32x4*>(x)[((size_t)(n * H + hi) * W + wi) * C4 + c4] : zero;
    }
  }
  f32x4 r[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[0][j] = d[0][j] - d[2][j];
    r[1][j] = d[1][j] + d[2][j];
    r[2][j] = d[2][j] - d[1][j];
    r[3][j] = d[1][j] - d[3][j];
  }
  long row[4];
  wino_tile_rows(cl, n, ty, tx, row);
  f32x4* dst = reinterpret_cast<f32x4*>(V) + c4;
  const size_t plane = (size_t)T * C4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long ra = row[i == 3 ? 1 : 0], rb = row[i == 3 ? 3 : 2];     // components (i, 0..2) and (i, 3)
    if (ra >= 0) {
      dst[(size_t)(i * 4 + 0) * plane + (size_t)ra * C4] = r[i][0] - r[i][2];
      dst[(size_t)(i * 4 + 1) * plane + (size_t)ra * C4] = r[i][1] + r[i][2];
      dst[(size_t)(i * 4 + 2) * plane + (size_t)ra * C4] = r[i][2] - r[i][1];
    }
    if (rb >= 0) dst[(size_t)(i * 4 + 3) * plane + (size_t)rb * C4] = r[i][1] - r[i][3];
  }
}

// y[2ty+a][2tx+b] = act((A^T m A)[a][b] * scale + shift),  A^T = [[1,1,1,0],[0,1,-1,-1]];  one thread per (tile, 4 channels).
// A component the tile's class lacks is NOT loaded (its rows were never written; the workspace may hold anything): the sums
// it would enter (s1 of a bottom tile, column 3 of a right one) feed only the outputs dropped below and are left at zero.
// RES: y = act(v + res) with v = (A^T m A) * scale + shift exactly as without it, ONE rounded add, then the activation - the
// bits of the residual-free call with relu = 0 followed by a float32 add and a ReLU pass.  res is fp32 NHWC of y's shape and
// is read at the address the lane stores to, so only where an output exists (partial tiles of odd maps read nothing else).
template <bool RES>
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ Mo, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, float* __restrict__ y, int H,
                                                         int W, int K4, int th, int tw, long T, int relu,
                                                         const float* __restrict__ mask,
                                                         const float* __restrict__ mscale, const WinoClasses cl,
                                                         const float* __restrict__ res) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)T * K4) return;
  const int k4 = (int)(idx % K4);
  const long t = (long)(idx / K4);
  const int tx = (int)(t % tw);
  const long t2 = t / tw;
  const int ty = (int)(t2 % th);
  const int n = (int)(t2 / th);
  long row[4];
  wino_tile_rows(cl, n, ty, tx, row);
  const f32x4* src = reinterpret_cast<const f32x4*>(Mo) + k4;
  const size_t plane = (size_t)T * K4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s0[4], s1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long ra = row[j == 3 ? 2 : 0], rb = row[j == 3 ? 3 : 1];     // components (0..2, j) and (3, j)
    s0[j] = s1[j] = zero;
    if (ra < 0) continue;
    const f32x4 m0 = src[(size_t)(0 * 4 + j) * plane + (size_t)ra * K4], m1 = src[(size_t)(1 * 4 + j) * plane + (size_t)ra * K4];
    const f32x4 m2 = src[(size_t)(2 * 4 + j) * plane + (size_t)ra * K4];
    s0[j] = m0 + m1 + m2;
    if (rb < 0) continue;
    const f32x4 m3 = src[(size_t)(3 * 4 + j) * plane + (size_t)rb * K4];
    s1[j] = m1 - m2 - m3;
  }
  f32x4 o[2][2];
  o[0][0] = s0[0] + s0[1] + s0[2];
  o[0][1] = s0[1] - s0[2] - s0[3];
  o[1][0] = s1[0] + s1[1] + s1[2];
  o[1][1] = s1[1] - s1[2] - s1[3];
  const f32x4 sc = scale ? reinterpret_cast<const f32x4*>(scale)[k4] : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 sh = shift ? reinterpret_cast<const f32x4*>(shift)[k4] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int ho = 2 * ty + a;
    if (ho >= H) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int wo = 2 * tx + b;
      if (wo >= W) continue;
      f32x4 v = o[a][b] * sc + sh;
      if (RES) v = v + reinterpret_cast<const f32x4*>(res)[((size_t)(n * H + ho) * W + wo) * K4 + k4];   // = `at` below
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = frcnn::relu_f32(v[e]);
      }
      const size_t at = ((size_t)(n * H + ho) * W + wo) * K4 + k4;
      if (mask) {
        const f32x4 mv = reinterpret_cast<const f32x4*>(mask)[at];
        const f32x4 ms = mscale ? reinterpret_cast<const f32x4*>(mscale)[k4] : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = frcnn::relu_open(mv[e]) ? v[e] * ms[e] : 0.f;
      }
      reinterpret_cast<f32x4*>(y)[at] = v;
    }
  }
}

}  // namespace

int frcnn::conv::launch_winograd(const ConvArgs& p, const Plan& pl, const float* scale, const float* shift, float* y, int relu,
                                 void* ws, hipStream_t stream) {
  const int n = p.M / (p.Ho * p.Wo);
  // The fused input transform (conv_igemm_f32<.., WINO>) reads the map in plain tile order and the persistent kernel (tile
  // kTilePersistent) walks p.M rows of every group: plans with either run the untrimmed form, which is bit-identical anyway.
  const bool trim = g_wino_trim && !pl.fuse_in && pl.cfg != kTilePersistent;
  const WinoGeom g = wino_geom(n, p.H, p.W, p.C, p.K, trim);
  char* base = static_cast<char*>(ws);
  float* U = reinterpret_cast<float*>(base + g.u_off);
  float* V = reinterpret_cast<float*>(base + g.v_off);
  float* Mo = reinterpret_cast<float*>(base + g.m_off);
  int rc = FRCNN_OK;
  if (p.u_pre) U = const_cast<float*>(p.u_pre);   // read-only from here on
  else rc = launch_1d<wino_filter_kernel>("wino_filter_kernel", (size_t)p.K * (p.C / 4), stream, p.w, U, p.K, p.C / 4);
  if (rc != FRCNN_OK) return rc;
  if (!pl.fuse_in)
    rc = launch_1d<wino_input_kernel>("wino_input_kernel", (size_t)g.T * (p.C / 4), stream, p.x, V, p.H, p.W, p.C / 4, g.th,
                   g.tw, g.T, g.cl);
  if (rc != FRCNN_OK) return rc;
  // 16 GEMMs  Mo[xi] (T x K) = V[xi] (T x C) . U[xi]^T (K x C)  as ONE grouped 1x1 convolution over a 1 x T "image"
  ConvArgs q;
  q.x = V; q.w = U; q.y = Mo;
  q.H = 1; q.W = (int)g.T; q.C = p.C; q.K = p.K; q.R = 1; q.S = 1; q.stride = 1; q.Ho = 1; q.Wo = (int)g.T;
  q.M = (int)g.T;
  for (int i = 0; i < 4; ++i) q.grows[i] = (int)g.rows[i];
  q.Ktot = p.C;
  q.ksteps = (p.C + BK - 1) / BK;
  q.gx = (size_t)g.T * p.C; q.gw = (size_t)p.K * p.C; q.gy = (size_t)g.T * p.K;
  q.epi_lds = p.epi_lds;
  q.zero = p.zero;
  {
    const size_t xb = q.gx * sizeof(float), wb = q.gw * sizeof(float);   // one transform component's slice
    q.xbytes = xb < ((size_t)1 << 31) ? (unsigned)xb : 0;
    q.wbytes = wb < ((size_t)1 << 31) ? (unsigned)wb : 0;
  }
  Plan gp{pl.cfg, 1, q.ksteps};
  if (pl.fuse_in) {          // the GEMM reads the layer's input itself: no V tensor
    q.x = p.x;
    q.gx = 0;
    q.wiH = p.H; q.wiW = p.W; q.wth = g.th; q.wtw = g.tw;
    gp.fuse_in = 1;
  }
  rc = launch_gemm(q, gp, g.T, p.K, 16, stream);
  if (rc != FRCNN_OK) return rc;
  // p.res: only frcnn_conv2d_fwd_wres_pre plans a call with a residual as Winograd (run_conv)
  if (p.res)
    return launch_1d<wino_output_kernel<true>>("wino_output_kernel<res>", (size_t)g.T * (p.K / 4), stream, (const float*)Mo, scale,
                     shift, y, p.Ho, p.Wo, p.K / 4, g.th, g.tw, g.T, relu, p.mask, p.mscale, g.cl, p.res);
  return launch_1d<wino_output_kernel<false>>("wino_output_kernel", (size_t)g.T * (p.K / 4), stream, (const float*)Mo, scale, shift, y,
                   p.Ho, p.Wo, p.K / 4, g.th, g.tw, g.T, relu, p.mask, p.mscale, g.cl, (const float*)nullptr);
}

extern "C" size_t frcnn_conv2d_winograd_filter_bytes(int k, int c) {
  if (k <= 0 || c <= 0 || (k % 4) || (c % 4)) return 0;
  return (size_t)16 * k * c * sizeof(float);
}

extern "C" long frcnn_conv2d_winograd_rows(int n, int h, int w, long out[4]) {
  if (out) out[0] = out[1] = out[2] = out[3] = 0;
  if (n <= 0 || h <= 0 || w <= 0 || (long)n * ((h + 1) / 2) * ((w + 1) / 2) > INT32_MAX) return 0;
  const WinoGeom g = wino_geom(n, h, w, 4, 4, g_wino_trim != 0);
  if (out)
    for (int i = 0; i < 4; ++i) out[i] = g.rows[i];
  return 9 * g.rows[0] + 3 * g.rows[1] + 3 * g.rows[2] + g.rows[3];
}

extern "C" int frcnn_conv2d_winograd_filter(const float* w_krsc, float* u, int k, int c, void* stream_) {
  FRCNN_REQUIRE(w_krsc && u && k > 0 && c > 0 && (k % 4) == 0 && (c % 4) == 0,
                "conv2d_winograd_filter: need a (k,3,3,c) filter with k%%4 == 0 and c%%4 == 0 (k=%d c=%d)", k, c);
  const size_t threads = (size_t)k * (c / 4);
  hipLaunchKernelGGL(wino_filter_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), w_krsc, u, k, c / 4);
  return frcnn::check_launch("wino_filter_kernel");
}
