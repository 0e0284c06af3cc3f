// Drawing a frame's detections on the device (test_net(draw_det=True); lib/model/test.py:231-242 and the
// draw_and_save_eval of lib/datasets/waymo_imdb.py:190-253, waymo_lidb.py:229-328, kitti_lidb.py:289-378):
//
//   canvas     the frame's own blob back to a uint8 picture: the image blob de-normalised (waymo_imdb.py:200-204) or the
//              BEV blob coloured by height / density / intensity (waymo_lidb.py:240-261, kitti_lidb.py:289-297);
//   plan       the frame's device record (dets (K, max_out, E), counts (K,)) and the ground truth -> a draw list in
//              painter's order: row i is the i-th thing the reference draws (integer geometry, colour, line width);
//   scatter    every outline pixel of row i does atomicMax(owner[pixel], i + 1) on a uint32 plane: where outlines
//              cross, the later row wins whatever the scheduling - an integer maximum does not depend on order;
//   compose    canvas[pixel] = rgb of row owner - 1 where owner != 0.
//
// Every value that decides a byte is formed in float64 (or in integers), each product and sum rounded once
// (-ffp-contract=off), so the picture is a pure function of its inputs and tests/draw_restatement.py restates it
// bit for bit in numpy.  Launches only: the owner plane is cleared by the library's fill kernel, there is no host
// synchronisation and no float atomic, and a stream capture holds kernel nodes only.
// All kernels are bandwidth- or latency-bound passes over at most one canvas; none uses LDS beyond the plan's key table.
#include "common.h"

#include <algorithm>
#include <cmath>

using namespace frcnn;

namespace {

constexpr int ROW = FRCNN_DRAW_ROW_INTS;
constexpr int BEV_MAX_BLOCKS = 256;

// saturating double -> byte: NaN -> 0, below 0 -> 0, above 255 -> 255, else truncation toward zero (astype(uint8) of an
// in-range value; numpy's out-of-range cast is undefined, here it is pinned)
__device__ __forceinline__ unsigned char to_byte(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 255.0) return 255;
  return (unsigned char)(int)v;
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

struct ImageParams {
  double stds[3], means[3];
  int arrange[3];
};

// waymo_imdb.py:200-204: out[y][x][o] = (uint8)(blob[y][x][arrange[o]] * stds[arrange[o]] + means[arrange[o]])
__global__ __launch_bounds__(256) void canvas_image_kernel(const float* __restrict__ blob, ImageParams p, int pixels,
                                                           unsigned char* __restrict__ canvas) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += gridDim.x * blockDim.x) {
    const float* px = blob + (size_t)i * 3;
    const float in[3] = {px[0], px[1], px[2]};
    unsigned char* o = canvas + (size_t)i * 3;
    for (int c = 0; c < 3; ++c) {
      const int s = p.arrange[c];
      const double v = (double)in[s] * p.stds[s] + p.means[s];
      o[c] = to_byte(v);
    }
  }
}

// Height of one BEV cell: the maximum over the height slices; FRCNN_DRAW_BEV_WAYMO adds the slice bias i*0.5 to every
// occupied slice first (waymo_lidb.py:242-245 does it in place on the blob; here the blob is only read).
// A NaN slice is ignored by the maximum (all NaN: the cell counts as height 0).
template <bool WAYMO>
__device__ __forceinline__ double cell_height(const float* __restrict__ cell, int slices) {
  double h = 0.0;
  bool any = false;
  for (int i = 0; i < slices; ++i) {
    double v = (double)cell[i];
    if (WAYMO && fabs(v) > 0.00001) v = v + (double)i * 0.5;
    if (v == v && (!any || v > h)) { h = v; any = true; }
  }
  return h;
}
// waymo_lidb.py:246-248: the extrema are taken over mask * height
template <bool WAYMO>
__device__ __forceinline__ double masked_height(double h) {
  return (WAYMO && !(fabs(h) > 0.00001)) ? 0.0 : h;
}

struct Extrema {
  double hmax, hmin, gmax, bmax;
};
__device__ __forceinline__ void merge(Extrema& a, const Extrema& b) {
  if (b.hmax > a.hmax) a.hmax = b.hmax;
  if (b.hmin < a.hmin) a.hmin = b.hmin;
  if (b.gmax > a.gmax) a.gmax = b.gmax;
  if (b.bmax > a.bmax) a.bmax = b.bmax;
}
__device__ __forceinline__ Extrema block_reduce(Extrema e, Extrema* s /* [4] */) {
  for (int off = 32; off > 0; off >>= 1) {
    Extrema o;
    o.hmax = __shfl_xor(e.hmax, off); o.hmin = __shfl_xor(e.hmin, off);
    o.gmax = __shfl_xor(e.gmax, off); o.bmax = __shfl_xor(e.bmax, off);
    merge(e, o);
  }
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = e;
  __syncthreads();
  e = s[0];
  for (int w = 1; w < 4; ++w) merge(e, s[w]);
  return e;
}
__device__ __forceinline__ Extrema empty_extrema() {
  Extrema e;
  e.hmax = -INFINITY; e.hmin = INFINITY; e.gmax = -INFINITY; e.bmax = -INFINITY;
  return e;
}

// launch 1: one partial per workgroup.  Maxima and minima do not depend on the order they are merged in.
template <bool WAYMO>
__global__ __launch_bounds__(256) void bev_partials_kernel(const float* __restrict__ blob, int cells, int channels, int slices,
                                                           Extrema* __restrict__ partials) {
  __shared__ Extrema s[4];
  Extrema e = empty_extrema();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x) {
    const float* cell = blob + (size_t)i * channels;
    Extrema c;
    c.hmax = c.hmin = masked_height<WAYMO>(cell_height<WAYMO>(cell, slices));
    c.gmax = (double)cell[slices];
    c.bmax = (double)cell[slices + 1];
    merge(e, c);
  }
  e = block_reduce(e, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = e;
}

// launch 2: the finish - merge the partials, form the three scale factors once.  A channel whose range is empty
// (max == min, max == 0, or no finite maximum) gets the factor 0: it is written as 0 (the reference divides by zero).
template <bool WAYMO>
__global__ __launch_bounds__(256) void bev_finish_kernel(const Extrema* __restrict__ partials, int n, double* __restrict__ scales) {
  __shared__ Extrema s[4];
  Extrema e = empty_extrema();
  for (int i = threadIdx.x; i < n; i += blockDim.x) merge(e, partials[i]);
  e = block_reduce(e, s);
  if (threadIdx.x == 0) {
    const double hmax = WAYMO ? e.hmax * 1.5 : e.hmax;
    const double range = hmax - e.hmin;
    const double gnum = WAYMO ? 6.0 * 255.0 : 255.0, bnum = WAYMO ? 2.0 * 255.0 : 255.0;
    const double sr = 255.0 / range, sg = gnum / e.gmax, sb = bnum / e.bmax;
    scales[0] = (range != 0.0 && isfinite(sr)) ? sr : 0.0;
    scales[1] = (e.gmax != 0.0 && isfinite(sg)) ? sg : 0.0;
    scales[2] = (e.bmax != 0.0 && isfinite(sb)) ? sb : 0.0;
  }
}

// launch 3: the colouring (waymo_lidb.py:252-261 / kitti_lidb.py:294-297), saturated to [0, 255]
template <bool WAYMO>
__global__ __launch_bounds__(256) void bev_colour_kernel(const float* __restrict__ blob, int cells, int channels, int slices,
                                                         const double* __restrict__ scales, unsigned char* __restrict__ canvas) {
  const double sr = scales[0], sg = scales[1], sb = scales[2];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x) {
    const float* cell = blob + (size_t)i * channels;
    const double h = cell_height<WAYMO>(cell, slices);
    const bool lit = !WAYMO || fabs(h) > 0.00001;
    unsigned char* o = canvas + (size_t)i * 3;
    o[0] = (lit && sr != 0.0) ? to_byte(h * sr) : 0;
    o[1] = sg != 0.0 ? to_byte((double)cell[slices] * sg) : 0;
    o[2] = sb != 0.0 ? to_byte((double)cell[slices + 1] * sb) : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// plan

struct PlanParams {
  int num_classes, max_out, elem, lidar, key_col, key_cols, limiter0, limiter_resets, num_gt, gt_elem, h, w, capacity;
};

constexpr int PLAN_MAX_OUT = 4096;

__device__ __forceinline__ int rgb_word(int r, int g, int b) { return clamp255(r) | (clamp255(g) << 8) | (clamp255(b) << 16); }

// Pillow's conversion of a float corner (ImageDraw.rectangle -> (int) of a double): truncation toward zero; pinned to
// +-2^30 where the C cast would be undefined
__device__ __forceinline__ int pil_int(double v) {
  if (v >= 1073741824.0) return 1073741824;
  if (v <= -1073741824.0) return -1073741824;
  return (int)v;
}

// one row of the draw list
__device__ __forceinline__ void put_row(int* __restrict__ rows, int seq, int kind, int width, int rgb, const int* g) {
  int* r = rows + (size_t)seq * ROW;
  r[0] = kind; r[1] = width; r[2] = seq; r[3] = rgb;
  for (int k = 0; k < 8; ++k) r[4 + k] = g[k];
}

// axis-aligned box [x1, y1, x2, y2]: kind 1.  A NaN coordinate skips the row (kind 0).
__device__ __forceinline__ void plan_rect(int* rows, int seq, const float* box, int width, int rgb) {
  int g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = true;
  for (int k = 0; k < 4; ++k) {
    const double v = (double)box[k];
    ok = ok && v == v;
    g[k] = ok ? pil_int(v) : 0;
  }
  if (!ok) g[0] = g[1] = g[2] = g[3] = 0;
  put_row(rows, seq, ok ? FRCNN_DRAW_RECT : FRCNN_DRAW_SKIP, width, rgb, g);
}

// rotated footprint of [xc, yc, zc, l, w, h, ry] (bbox_3d_to_bev_4pt / rotate_in_bev, lib/utils/bbox.py:174-233, in
// float64, the corners rounded to float32 like rotate_in_bev's result), clipped to the canvas and truncated
// (draw_bev_bboxes, :346-351): kind 2, corners p0 (x1,y1), p1 (x1,y2), p2 (x2,y2), p3 (x2,y1).
__device__ __forceinline__ void plan_footprint(int* rows, int seq, const float* box, int width, int rgb, int cw, int ch) {
  int g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double xc = box[0], yc = box[1], l = box[3], w = box[4], ry = box[6];
  const bool ok = xc == xc && yc == yc && l == l && w == w && ry == ry;
  if (ok) {
    const double x1 = xc - l / 2, x2 = xc + l / 2, y1 = yc - w / 2, y2 = yc + w / 2;
    const double px[4] = {x1, x1, x2, x2}, py[4] = {y1, y2, y2, y1};
    const double c = cos(ry), s = sin(ry);
    for (int k = 0; k < 4; ++k) {
      const double dx = px[k] - xc, dy = py[k] - yc;
      const double rx = dx * c - dy * s, rr = dx * s + dy * c;
      float fx = (float)(rx + xc), fy = (float)(rr + yc);
      // np.clip(v, 0, n - 1): a NaN (an infinite extent times 0) stays NaN in numpy; here it is pinned to 0
      fx = fx != fx ? 0.f : fminf(fmaxf(fx, 0.f), (float)(cw - 1));
      fy = fy != fy ? 0.f : fminf(fmaxf(fy, 0.f), (float)(ch - 1));
      g[2 * k] = (int)fx;
      g[2 * k + 1] = (int)fy;
    }
  }
  put_row(rows, seq, ok ? FRCNN_DRAW_FOOTPRINT : FRCNN_DRAW_SKIP, width, rgb, g);
}

// the sort key of a detection row: mean of its key columns, fp32 sum in column order / column count (db.py:260-281)
__device__ __forceinline__ float sort_key(const float* row, int key_col, int key_cols) {
  float s = row[key_col];
  for (int c = 1; c < key_cols; ++c) s = s + row[key_col + c];
  return s / (float)key_cols;
}
// does row a (key ka) come before row b (key kb) in np.argsort(-key)?  Descending key, NaN keys last, ties to the lower
// row (numpy's default argsort is not stable: the tie rule is this library's).
__device__ __forceinline__ bool before(float ka, int a, float kb, int b) {
  const bool na = ka != ka, nb = kb != kb;
  if (na != nb) return nb;
  if (!na && ka != kb) return ka > kb;
  return a < b;
}

// block 0: the ground-truth rows and the unused tail of the list; block j >= 1: class j's detections.
__global__ __launch_bounds__(256) void draw_plan_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        const float* __restrict__ gt, const int* __restrict__ gt_labels,
                                                        PlanParams p, int* __restrict__ rows) {
  __shared__ float s_key[PLAN_MAX_OUT];
  const int j = blockIdx.x;
  // detections in front of class j, all detections, and the reference's `limiter` as class j sees it (the value is
  // carried from class to class: waymo_imdb.py:208,220-223 resets it to 15, waymo_lidb.py:265,294-295 only lowers it)
  int before_j = 0, total = 0, limiter = p.limiter0;
  for (int c = 1; c < p.num_classes; ++c) {
    const int n = min(max(counts[c], 0), p.max_out);
    if (c < j) before_j += n;
    total += n;
    if (c <= j && n > 0) {
      if (n < limiter) limiter = n;
      else if (p.limiter_resets) limiter = p.limiter0;
    }
  }
  // image: detections, then ground truth (waymo_imdb.py:211-251); LiDAR: ground truth first (waymo_lidb.py:268-284)
  const int det_base = p.lidar ? p.num_gt : 0, gt_base = p.lidar ? 0 : total;
  if (j == 0) {
    for (int g = threadIdx.x; g < p.num_gt; g += blockDim.x) {
      const float* box = gt + (size_t)g * p.gt_elem;
      if (p.lidar) {
        const int c = gt_labels[g] == 0 ? 127 : 255;
        plan_footprint(rows, gt_base + g, box, 2, rgb_word(c, c, c), p.w, p.h);
      } else {
        const int c = gt_labels[g] == 0 ? 0 : 255;
        plan_rect(rows, gt_base + g, box, 1, rgb_word(c, c, c));
      }
    }
    const int zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = total + p.num_gt + threadIdx.x; r < p.capacity; r += blockDim.x) put_row(rows, r, FRCNN_DRAW_SKIP, 0, 0, zero);
    return;
  }
  const int n = min(max(counts[j], 0), p.max_out);
  const float* cls = dets + (size_t)j * p.max_out * p.elem;
  if (p.key_cols > 0) {
    for (int r = threadIdx.x; r < n; r += blockDim.x) s_key[r] = sort_key(cls + (size_t)r * p.elem, p.key_col, p.key_cols);
    __syncthreads();
  }
  const int score_col = p.lidar ? 7 : 4;
  for (int r = threadIdx.x; r < n; r += blockDim.x) {
    int rank;
    if (p.key_cols > 0) {
      const float k = s_key[r];
      rank = 0;
      for (int m = 0; m < n; ++m) rank += before(s_key[m], m, k, r);
    } else {
      rank = n - 1 - r;                               // np.argsort(-np.arange(n)) (db.py:299-301)
    }
    const float* row = cls + (size_t)r * p.elem;
    const float gf = row[score_col] * 255.0f;
    const int green = gf != gf ? 0 : (gf >= 255.0f ? 255 : gf <= 0.0f ? 0 : (int)gf);
    const int uc = pil_int(((double)(limiter - rank) / (double)limiter) * 255.0);
    const int rgb = rgb_word(0, green, uc);
    const int seq = det_base + before_j + rank;
    if (p.lidar) plan_footprint(rows, seq, row, 2, rgb, p.w, p.h);
    else plan_rect(rows, seq, row, 2, rgb);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// scatter / compose

struct Span {      // an inclusive pixel rectangle, empty when x1 < x0 or y1 < y0
  int x0, y0, x1, y1;
  __device__ int area() const { return (x1 < x0 || y1 < y0) ? 0 : (x1 - x0 + 1) * (y1 - y0 + 1); }
};
__device__ __forceinline__ Span clip_span(int x0, int y0, int x1, int y1, int w, int h) {
  Span s;
  s.x0 = max(x0, 0); s.y0 = max(y0, 0); s.x1 = min(x1, w - 1); s.y1 = min(y1, h - 1);
  return s;
}

// One workgroup per row of the list, one lane per outline pixel (workgroup-strided over the row's pixel count).
//   kind 1, width wd: the pixels of [x0,x1] x [y0,y1] within wd pixels of the border = four strips, each clipped to the
//   canvas BEFORE it is enumerated (a box far outside the canvas costs nothing); the strips overlap at the corners,
//   which an atomic maximum does not mind.
//   kind 2: four edges, corner i -> corner i-1 (draw_polygon, lib/utils/bbox.py:364-379).  Edge pixel t of dmaj + 1:
//   major0 + s_major * t, minor0 + s_minor * ((2*t*dmin + dmaj) / (2*dmaj)) - the closed form of Pillow's Bresenham
//   walk (x is the major axis iff dx > dy); width 2 also paints minor + 1.
__global__ __launch_bounds__(256) void draw_scatter_kernel(const int* __restrict__ rows, int h, int w,
                                                           unsigned* __restrict__ owner) {
  const int* r = rows + (size_t)blockIdx.x * ROW;
  // a list from frcnn_draw_plan keeps its coordinates within +-2^30 and its widths at 1 or 2.  Any other list: rectangle
  // corners and widths are pinned here so that no sum below overflows (the strips are clipped before they are counted);
  // a footprint whose corners or width are out of range is not drawn (below)
  constexpr int PIN = 1 << 30;
  const int kind = r[0], wd = min(r[1], 1 << 20);
  const unsigned tag = blockIdx.x + 1u;
  if (kind == FRCNN_DRAW_RECT) {
    const int x0 = max(r[4], -PIN), y0 = max(r[5], -PIN), x1 = min(r[6], PIN), y1 = min(r[7], PIN);
    if (x1 < x0 || y1 < y0 || wd < 1) return;
    const Span top = clip_span(x0, y0, x1, min(y0 + wd - 1, y1), w, h);
    const Span bottom = clip_span(x0, max(y1 - wd + 1, y0), x1, y1, w, h);
    const Span left = clip_span(x0, y0, min(x0 + wd - 1, x1), y1, w, h);
    const Span right = clip_span(max(x1 - wd + 1, x0), y0, x1, y1, w, h);
    const int a0 = top.area(), a1 = a0 + bottom.area(), a2 = a1 + left.area(), a3 = a2 + right.area();
    for (int t = threadIdx.x; t < a3; t += blockDim.x) {
      const Span s = t < a0 ? top : t < a1 ? bottom : t < a2 ? left : right;
      const int u = t - (t < a0 ? 0 : t < a1 ? a0 : t < a2 ? a1 : a2);
      const int sw = s.x1 - s.x0 + 1;
      const int x = s.x0 + u % sw, y = s.y0 + u / sw;
      atomicMax(owner + (size_t)y * w + x, tag);
    }
  } else if (kind == FRCNN_DRAW_FOOTPRINT) {
    if (wd < 1 || wd > 16) return;                                // 4 edges x (2^21 + 1) pixels x 16 stays below 2^31
    for (int c = 4; c < 12; ++c)
      if (r[c] < -(1 << 20) || r[c] > (1 << 20)) return;          // not a clipped footprint: nothing is drawn
    int end1 = 0, end2 = 0, end3 = 0, end4 = 0;
    for (int e = 0; e < 4; ++e) {
      const int a = e, b = (e + 3) & 3;
      const int dx = abs(r[4 + 2 * b] - r[4 + 2 * a]), dy = abs(r[5 + 2 * b] - r[5 + 2 * a]);
      const int len = (max(dx, dy) + 1) * wd;
      end4 += len;
      if (e < 3) end3 += len;
      if (e < 2) end2 += len;
      if (e < 1) end1 += len;
    }
    for (int t = threadIdx.x; t < end4; t += blockDim.x) {
      const int e = t < end1 ? 0 : t < end2 ? 1 : t < end3 ? 2 : 3;
      const int u = t - (e == 0 ? 0 : e == 1 ? end1 : e == 2 ? end2 : end3);
      const int a = e, b = (e + 3) & 3;
      const int ax = r[4 + 2 * a], ay = r[5 + 2 * a], bx = r[4 + 2 * b], by = r[5 + 2 * b];
      const int dx = abs(bx - ax), dy = abs(by - ay), sx = bx >= ax ? 1 : -1, sy = by >= ay ? 1 : -1;
      const int i = u / wd, side = u % wd;
      int x, y;
      if (dx > dy) {
        x = ax + sx * i;
        y = ay + sy * (int)((2ll * i * dy + dx) / (2ll * dx)) + side;
      } else {
        y = ay + sy * i;
        x = ax + (dy == 0 ? 0 : sx * (int)((2ll * i * dx + dy) / (2ll * dy))) + side;
      }
      if (x >= 0 && x < w && y >= 0 && y < h) atomicMax(owner + (size_t)y * w + x, tag);
    }
  }
}

__global__ __launch_bounds__(256) void draw_compose_kernel(const int* __restrict__ rows, int num_rows,
                                                           const unsigned* __restrict__ owner, int pixels,
                                                           unsigned char* __restrict__ canvas) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += gridDim.x * blockDim.x) {
    const unsigned o = owner[i];
    if (o == 0 || o > (unsigned)num_rows) continue;
    const int rgb = rows[(size_t)(o - 1) * ROW + 3];
    unsigned char* px = canvas + (size_t)i * 3;
    px[0] = (unsigned char)(rgb & 255);
    px[1] = (unsigned char)((rgb >> 8) & 255);
    px[2] = (unsigned char)((rgb >> 16) & 255);
  }
}

unsigned grid_for(size_t work, unsigned cap) { return (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, cap)); }

template <bool WAYMO>
int bev_canvas(const float* blob, int cells, int channels, int slices, unsigned char* canvas, void* ws, hipStream_t stream) {
  Extrema* partials = static_cast<Extrema*>(ws);
  double* scales = reinterpret_cast<double*>(partials + BEV_MAX_BLOCKS);
  const unsigned blocks = grid_for((size_t)cells, BEV_MAX_BLOCKS);
  hipLaunchKernelGGL(bev_partials_kernel<WAYMO>, dim3(blocks), dim3(256), 0, stream, blob, cells, channels, slices, partials);
  hipLaunchKernelGGL(bev_finish_kernel<WAYMO>, dim3(1), dim3(256), 0, stream, partials, (int)blocks, scales);
  hipLaunchKernelGGL(bev_colour_kernel<WAYMO>, dim3(grid_for((size_t)cells, 2048)), dim3(256), 0, stream, blob, cells, channels,
                     slices, scales, canvas);
  return check_launch("frcnn_canvas_from_bev_blob");
}

}  // namespace

extern "C" int frcnn_canvas_from_image_blob(const float* blob, int height, int width, const double* stds_host,
                                            const double* means_host, const int* arrange_host, uint8_t* canvas,
                                            void* stream) {
  FRCNN_REQUIRE(blob && stds_host && means_host && arrange_host && canvas, "canvas_from_image_blob: null argument");
  FRCNN_REQUIRE(height > 0 && width > 0 && (int64_t)height * width < (1ll << 29),
                "canvas_from_image_blob: frame %d x %d", height, width);
  ImageParams p;
  for (int c = 0; c < 3; ++c) {
    FRCNN_REQUIRE(arrange_host[c] >= 0 && arrange_host[c] < 3, "canvas_from_image_blob: channel order entry %d is %d", c,
                  arrange_host[c]);
    FRCNN_REQUIRE(std::isfinite(stds_host[c]) && std::isfinite(means_host[c]),
                  "canvas_from_image_blob: PIXEL_STDDEVS / PIXEL_MEANS entry %d is not finite", c);
    p.stds[c] = stds_host[c];
    p.means[c] = means_host[c];
    p.arrange[c] = arrange_host[c];
  }
  const int pixels = height * width;
  hipLaunchKernelGGL(canvas_image_kernel, dim3(grid_for((size_t)pixels, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), blob, p, pixels, canvas);
  return check_launch("frcnn_canvas_from_image_blob");
}

extern "C" size_t frcnn_canvas_from_bev_blob_ws_bytes(void) { return BEV_MAX_BLOCKS * sizeof(Extrema) + 3 * sizeof(double); }

extern "C" int frcnn_canvas_from_bev_blob(const float* blob, int ny, int nx, int channels, int num_slices, int form,
                                          uint8_t* canvas, void* ws, size_t ws_bytes, void* stream) {
  FRCNN_REQUIRE(blob && canvas && ws, "canvas_from_bev_blob: null argument");
  FRCNN_REQUIRE(ny > 0 && nx > 0 && (int64_t)ny * nx < (1ll << 29), "canvas_from_bev_blob: grid %d x %d", ny, nx);
  FRCNN_REQUIRE(num_slices >= 1 && channels >= num_slices + 2,
                "canvas_from_bev_blob: %d channels cannot hold %d height slices, density and intensity", channels, num_slices);
  FRCNN_REQUIRE((int64_t)ny * nx * channels < (1ll << 31), "canvas_from_bev_blob: blob too large");
  FRCNN_REQUIRE(form == FRCNN_DRAW_BEV_WAYMO || form == FRCNN_DRAW_BEV_KITTI, "canvas_from_bev_blob: form %d", form);
  if (ws_bytes < frcnn_canvas_from_bev_blob_ws_bytes() || (reinterpret_cast<uintptr_t>(ws) & 7))
    return fail(FRCNN_ERR_WS, "canvas_from_bev_blob: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes,
                frcnn_canvas_from_bev_blob_ws_bytes());
  hipStream_t s = static_cast<hipStream_t>(stream);
  return form == FRCNN_DRAW_BEV_WAYMO ? bev_canvas<true>(blob, ny * nx, channels, num_slices, canvas, ws, s)
                                      : bev_canvas<false>(blob, ny * nx, channels, num_slices, canvas, ws, s);
}

extern "C" int frcnn_draw_plan(const float* dets, const int* counts, int num_classes, int max_out, int elem, int lidar,
                               int key_col, int key_cols, int limiter0, int limiter_resets, const float* gt,
                               const int* gt_labels, int num_gt, int canvas_h, int canvas_w, int* rows, int capacity,
                               void* stream) {
  FRCNN_REQUIRE(dets && counts && rows, "draw_plan: null argument");
  FRCNN_REQUIRE(num_classes >= 1 && max_out >= 1 && max_out <= PLAN_MAX_OUT, "draw_plan: %d classes, max_out %d (<= %d)",
                num_classes, max_out, PLAN_MAX_OUT);
  FRCNN_REQUIRE(elem >= (lidar ? 8 : 5), "draw_plan: rows of %d floats", elem);
  FRCNN_REQUIRE(key_cols >= 0 && (key_cols == 0 || (key_col >= 0 && key_col + key_cols <= elem)),
                "draw_plan: key columns %d..%d outside rows of %d floats", key_col, key_col + key_cols, elem);
  FRCNN_REQUIRE(limiter0 >= 1, "draw_plan: limiter %d", limiter0);
  FRCNN_REQUIRE(num_gt >= 0 && (num_gt == 0 || (gt && gt_labels)), "draw_plan: %d ground-truth boxes without data", num_gt);
  FRCNN_REQUIRE(canvas_h > 0 && canvas_w > 0, "draw_plan: canvas %d x %d", canvas_h, canvas_w);
  FRCNN_REQUIRE((int64_t)capacity >= (int64_t)(num_classes - 1) * max_out + num_gt,
                "draw_plan: a list of %d rows cannot hold %d classes x %d detections + %d ground-truth boxes", capacity,
                num_classes - 1, max_out, num_gt);
  PlanParams p = {num_classes, max_out, elem, lidar ? 1 : 0, key_col, key_cols, limiter0, limiter_resets ? 1 : 0,
                  num_gt, lidar ? 7 : 4, canvas_h, canvas_w, capacity};
  hipLaunchKernelGGL(draw_plan_kernel, dim3(num_classes), dim3(256), 0, static_cast<hipStream_t>(stream), dets, counts, gt,
                     gt_labels, p, rows);
  return check_launch("frcnn_draw_plan");
}

extern "C" int frcnn_draw_scatter(const int* rows, int num_rows, uint32_t* owner, int height, int width, void* stream) {
  FRCNN_REQUIRE(owner && (rows || num_rows == 0), "draw_scatter: null argument");
  FRCNN_REQUIRE(num_rows >= 0 && height > 0 && width > 0 && (int64_t)height * width < (1ll << 29),
                "draw_scatter: %d rows on a %d x %d canvas", num_rows, height, width);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = fill_bytes(owner, 0, (size_t)height * width * sizeof(uint32_t), s);
  if (e != hipSuccess) return fail(FRCNN_ERR_LAUNCH, "draw_scatter: clear: %s", hipGetErrorString(e));
  if (num_rows == 0) return FRCNN_OK;
  hipLaunchKernelGGL(draw_scatter_kernel, dim3(num_rows), dim3(256), 0, s, rows, height, width, owner);
  return check_launch("frcnn_draw_scatter");
}

extern "C" int frcnn_draw_compose(const int* rows, int num_rows, const uint32_t* owner, uint8_t* canvas, int height,
                                  int width, void* stream) {
  FRCNN_REQUIRE(owner && canvas && (rows || num_rows == 0), "draw_compose: null argument");
  FRCNN_REQUIRE(num_rows >= 0 && height > 0 && width > 0 && (int64_t)height * width < (1ll << 29),
                "draw_compose: %d rows on a %d x %d canvas", num_rows, height, width);
  if (num_rows == 0) return FRCNN_OK;
  const int pixels = height * width;
  hipLaunchKernelGGL(draw_compose_kernel, dim3(grid_for((size_t)pixels, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rows, num_rows, owner, pixels, canvas);
  return check_launch("frcnn_draw_compose");
}
