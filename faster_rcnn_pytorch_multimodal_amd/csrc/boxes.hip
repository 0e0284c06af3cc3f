// Anchors and the box codec: anchor generators (2-D, 3-D), RPN decode + clip, the *_transform_inv codecs, clip_boxes, the
// FPN level map and the row gathers around the RPN's sort (topk.hip) and NMS (nms.hip).  The per-class detection filter
// is class_filter.hip.  Built with -ffp-contract=off (see box_math.h).
#include "box_math.h"

using namespace frcnn;

namespace {

// ------------------------------------------------------------------------------------------------
// generate_anchors_pre — lib/layer_utils/snippets.py:27-37.  numpy adds the float64 base table to the
// integer shift grid and casts ONCE to float32; do the same (double add, one rounding).
// Layout (H, W, A) flattened, A fastest (snippets.py:35-37).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchors_kernel(const double* __restrict__ base, int A, int H, int W,
                                                     int stride, float* __restrict__ out) {
  const int total = H * W * A;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int a = i % A;
    const int pix = i / A;
    const int x = pix % W, y = pix / W;
    const double sx = (double)(x * stride), sy = (double)(y * stride);
    float4 v;
    v.x = (float)(base[a * 4 + 0] + sx);
    v.y = (float)(base[a * 4 + 1] + sy);
    v.z = (float)(base[a * 4 + 2] + sx);
    v.w = (float)(base[a * 4 + 3] + sy);
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// GridAnchor3dGenerator — lib/layer_utils/generate_3d_anchors.py:15-118, plus the axis-aligned BEV box of
// every 3-D anchor (lib/utils/bbox.py:256-293, clip=False) that the RPN regresses against.
// `base` holds one row per anchor type t = size*R + rot (the order of the meshgrid, rot fastest):
//   [lo_x, lo_y, hi_x, hi_y, z, l, w, h, ry]   lo/hi = float32 BEV half extents of the rotated box.
// Layout (H, W, T): anchors3d[i] = [x, y, z, l, w, h, ry], anchors2d[i] = [lo_x+x, lo_y+y, hi_x+x, hi_y+y]
// with x = float(col*stride), y = float(row*stride) and fp32 adds like the reference's float32 arrays.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchors3d_kernel(const float* __restrict__ base, int T, int H, int W,
                                                       int stride, float* __restrict__ a3, float* __restrict__ a2) {
  const int total = H * W * T;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t = i % T;
    const int pix = i / T;
    const float xc = (float)((pix % W) * stride), yc = (float)((pix / W) * stride);
    const float* b = base + t * 9;
    float* o = a3 + (size_t)i * 7;
    o[0] = xc; o[1] = yc; o[2] = b[4]; o[3] = b[5]; o[4] = b[6]; o[5] = b[7]; o[6] = b[8];
    reinterpret_cast<float4*>(a2)[i] = make_float4(b[0] + xc, b[1] + yc, b[2] + xc, b[3] + yc);
  }
}

// ------------------------------------------------------------------------------------------------
// proposal_layer.py:32-36: fg score, bbox_transform_inv, clip_boxes for anchor i = pix*A + a.
// ------------------------------------------------------------------------------------------------
struct ClipInfo {
  float x_lo, x_hi, y_lo, y_hi;
};

__global__ __launch_bounds__(256) void rpn_decode_clip_kernel(const float* __restrict__ rpn, int ld,
                                                             const float* __restrict__ probs_in,
                                                             const float* __restrict__ deltas_in,
                                                             const float* __restrict__ anchors, ClipInfo clip,
                                                             int total, int A, float* __restrict__ scores,
                                                             float* __restrict__ proposals) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int a = i % A;
    const int pix = i / A;
    float score;
    if (probs_in) {
      score = probs_in[i];
    } else {
      // 2-way softmax over (bg, fg) exactly as torch.softmax: subtract max, exp, divide by the sum
      const float bg = rpn[(size_t)pix * ld + a], fg = rpn[(size_t)pix * ld + A + a];
      const float m = fmaxf(bg, fg);
      const float eb = exp_f32(bg - m), ef = exp_f32(fg - m);
      score = ef / (eb + ef);
    }
    float4 d;
    if (deltas_in) d = reinterpret_cast<const float4*>(deltas_in)[i];
    else {
      const float* p = rpn + (size_t)pix * ld + 2 * A + a * 4;
      d = make_float4(p[0], p[1], p[2], p[3]);
    }
    const float4 an = reinterpret_cast<const float4*>(anchors)[i];
    float o[4];
    decode_box(an.x, an.y, an.z, an.w, d.x, d.y, d.z, d.w, o);
    float4 r;
    r.x = clampf(o[0], clip.x_lo, clip.x_hi);
    r.y = clampf(o[1], clip.y_lo, clip.y_hi);
    r.z = clampf(o[2], clip.x_lo, clip.x_hi);
    r.w = clampf(o[3], clip.y_lo, clip.y_hi);
    scores[i] = score;
    reinterpret_cast<float4*>(proposals)[i] = r;
  }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ rows,
                                                         const int64_t* __restrict__ order,
                                                         const int* __restrict__ count, int max_count, int width,
                                                         float* __restrict__ out) {
  const int cnt = count ? min(*count, max_count) : max_count;
  const int total = max_count * width;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / width, c = i - r * width;
    out[i] = r < cnt ? rows[order[r] * width + c] : 0.f;
  }
}

// The uncertainty columns of a frame's detections (nms_hstack_var_torch, filter_predictions.py:23-43, and the column
// stacking of lib/model/test.py:260-270): out (K, M, D + U) = [dets row | the sources' values of the detection's RoI].
// A per-class source (the box variances) contributes v[roi, j*w:(j+1)*w] for class j, a shared one v[roi, 0:w].  Rows whose
// det_roi is outside [0, R) (-1 marks padding) keep their box columns and get +0.0 in the uncertainty columns.
constexpr int UC_MAX_SOURCES = 8;
struct UcSources {
  const float* ptr[UC_MAX_SOURCES];
  int width[UC_MAX_SOURCES];       // output columns
  int stride[UC_MAX_SOURCES];      // floats per RoI row of the source
  int per_class[UC_MAX_SOURCES];
  int end[UC_MAX_SOURCES];         // first output column after this source
  int count;
};

__global__ __launch_bounds__(256) void uncertainty_columns_kernel(const float* __restrict__ dets,
                                                                 const int* __restrict__ det_roi, UcSources src, int M,
                                                                 int D, int W, int R, size_t total,
                                                                 float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / (size_t)W;          // j * M + m
    const int c = (int)(i - row * (size_t)W);
    if (c < D) {
      out[i] = dets[row * (size_t)D + c];
      continue;
    }
    const int roi = det_roi[row];
    float v = 0.f;
    if (roi >= 0 && roi < R) {
      int q = 0;
      while (q + 1 < src.count && c >= src.end[q]) ++q;
      const int col = c - (src.end[q] - src.width[q]);
      const int j = (int)(row / (size_t)M);
      v = src.ptr[q][(size_t)roi * src.stride[q] + (src.per_class[q] ? j * src.width[q] : 0) + col];
    }
    out[i] = v;
  }
}

__global__ __launch_bounds__(256) void make_rois_kernel(const float* __restrict__ boxes, const float* __restrict__ scs,
                                                       const int64_t* __restrict__ keep_idx,
                                                       const int* __restrict__ keep_count, int max_keep,
                                                       float* __restrict__ rois, float* __restrict__ roi_scores) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= max_keep) return;
  const int cnt = min(*keep_count, max_keep);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  float s = 0.f;
  if (i < cnt) {
    const int64_t k = keep_idx[i];
    b = reinterpret_cast<const float4*>(boxes)[k];
    s = scs[k];
  }
  float* r = rois + (size_t)i * 5;
  r[0] = 0.f; r[1] = b.x; r[2] = b.y; r[3] = b.z; r[4] = b.w;
  if (roi_scores) roi_scores[i] = s;
}

// bbox_transform_inv for (N boxes) x (Kc classes) — lib/model/bbox_transform.py:75-105 — and clip_boxes
// (:235-257) as stand-alone entry points (the proposal / head kernels fuse the same arithmetic).
__global__ __launch_bounds__(256) void bbox_transform_inv_kernel(const float* __restrict__ boxes, int box_ld,
                                                                const float* __restrict__ deltas, int n, int kc,
                                                                float scale, int use_scale,
                                                                float* __restrict__ out) {
  const int total = n * kc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / kc;
    const float* b = boxes + (size_t)r * box_ld;
    float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    if (use_scale) { x1 = x1 / scale; y1 = y1 / scale; x2 = x2 / scale; y2 = y2 / scale; }
    const float4 d = reinterpret_cast<const float4*>(deltas)[i];
    float o[4];
    decode_box(x1, y1, x2, y2, d.x, d.y, d.z, d.w, o);
    reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// lidar_3d_bbox_transform_inv for (N rois) x (Kc classes) — lib/model/bbox_transform.py:174-233.
__global__ __launch_bounds__(256) void lidar_bbox_transform_inv_kernel(const float* __restrict__ rois, int roi_ld,
                                                                      const float* __restrict__ anchors3d,
                                                                      const float* __restrict__ deltas, int n, int kc,
                                                                      float scale, int use_scale,
                                                                      float* __restrict__ out) {
  const int total = n * kc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / kc;
    const float* b = rois + (size_t)r * roi_ld;
    float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    if (use_scale) { x1 = x1 / scale; y1 = y1 / scale; x2 = x2 / scale; y2 = y2 / scale; }
    float d[7], o[7];
    for (int q = 0; q < 7; ++q) d[q] = deltas[(size_t)i * 7 + q];
    decode_box_lidar(x1, y1, x2, y2, anchors3d + (size_t)r * 7, d, o);
    for (int q = 0; q < 7; ++q) out[(size_t)i * 7 + q] = o[q];
  }
}

__global__ __launch_bounds__(256) void clip_boxes_kernel(const float* __restrict__ in, int total, ClipInfo clip,
                                                        float* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float4 b = reinterpret_cast<const float4*>(in)[i];
    b.x = clampf(b.x, clip.x_lo, clip.x_hi);
    b.y = clampf(b.y, clip.y_lo, clip.y_hi);
    b.z = clampf(b.z, clip.x_lo, clip.x_hi);
    b.w = clampf(b.w, clip.y_lo, clip.y_hi);
    reinterpret_cast<float4*>(out)[i] = b;
  }
}

// LevelMapper.__call__ (lib/utils/torchpoolers.py:39-51): FPN level of each RoI from its area (no +1):
// floor(lvl0 + log2(sqrt(area) / s0) + eps) clamped to [k_min, k_max], returned relative to k_min.
__global__ __launch_bounds__(256) void fpn_level_map_kernel(const float* __restrict__ rois, int n, int k_min, int k_max,
                                                           float s0, float lvl0, float eps, int* __restrict__ levels) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* b = rois + (size_t)i * 5 + 1;
    const float area = (b[2] - b[0]) * (b[3] - b[1]);
    const float s = sqrtf(area);
    float lvl = floorf(lvl0 + (float)log2((double)(s / s0)) + eps);
    lvl = fminf(fmaxf(lvl, (float)k_min), (float)k_max);   // NaN (negative area) falls to k_min like clamp(min=...)
    if (!(lvl >= (float)k_min)) lvl = (float)k_min;
    levels[i] = (int)lvl - k_min;
  }
}

}  // namespace

extern "C" int frcnn_generate_anchors(const double* base, int num_base, int height, int width, int feat_stride,
                                      float* anchors, void* stream_) {
  FRCNN_REQUIRE(base && anchors && num_base > 0 && height > 0 && width > 0 && feat_stride > 0,
                "generate_anchors: bad arguments");
  const int total = height * width * num_base;
  hipLaunchKernelGGL(anchors_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), base, num_base, height, width, feat_stride, anchors);
  return check_launch("anchors_kernel");
}

extern "C" int frcnn_rpn_decode_clip(const float* rpn, int ld, const float* probs_in, const float* deltas_in,
                                     const float* anchors, const float* info_host, int hw, int num_anchors,
                                     float* scores, float* proposals, void* stream_) {
  FRCNN_REQUIRE(anchors && info_host && scores && proposals && hw > 0 && num_anchors > 0,
                "rpn_decode_clip: bad arguments");
  FRCNN_REQUIRE((rpn && ld >= 6 * num_anchors) || (probs_in && deltas_in),
                "rpn_decode_clip: need the fused rpn tensor (ld >= 6A) or probs_in + deltas_in");
  FRCNN_REQUIRE(rpn || (probs_in && deltas_in), "rpn_decode_clip: probs_in/deltas_in need each other without rpn");
  // clip_boxes (bbox_transform.py:252-255): x in [info[0], info[1]-1], y in [info[2], info[3]-1], fp32 maths
  ClipInfo clip{info_host[0], info_host[1] - 1.0f, info_host[2], info_host[3] - 1.0f};
  const int total = hw * num_anchors;
  hipLaunchKernelGGL(rpn_decode_clip_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), rpn, ld, probs_in, deltas_in, anchors, clip, total, num_anchors,
                     scores, proposals);
  return check_launch("rpn_decode_clip_kernel");
}

extern "C" int frcnn_gather_rows(const float* rows, const int64_t* order, const int* count, int max_count, int width,
                                 float* rows_out, void* stream_) {
  FRCNN_REQUIRE(rows && order && rows_out && max_count > 0 && width > 0, "gather_rows: bad arguments");
  const int total = max_count * width;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), rows, order, count, max_count, width, rows_out);
  return check_launch("gather_rows_kernel");
}

extern "C" int frcnn_uncertainty_columns(const float* dets, const int* det_roi, int num_classes, int max_out,
                                         int det_width, int num_rois, int num_sources, const float* const* sources_host,
                                         const int* widths_host, const int* per_class_host, float* out, void* stream_) {
  FRCNN_REQUIRE(dets && det_roi && out && sources_host && widths_host && per_class_host,
                "uncertainty_columns: null argument");
  FRCNN_REQUIRE(num_classes > 0 && max_out > 0 && det_width > 0 && num_rois > 0 && num_sources > 0 &&
                    num_sources <= UC_MAX_SOURCES,
                "uncertainty_columns: bad shape (1 <= sources <= %d)", UC_MAX_SOURCES);
  UcSources src{};
  int w = det_width;
  for (int q = 0; q < num_sources; ++q) {
    FRCNN_REQUIRE(sources_host[q] && widths_host[q] > 0, "uncertainty_columns: source %d is null or empty", q);
    src.ptr[q] = sources_host[q];
    src.width[q] = widths_host[q];
    src.per_class[q] = per_class_host[q] ? 1 : 0;
    src.stride[q] = per_class_host[q] ? widths_host[q] * num_classes : widths_host[q];
    w += widths_host[q];
    src.end[q] = w;
  }
  src.count = num_sources;
  const size_t total = (size_t)num_classes * max_out * w;
  hipLaunchKernelGGL(uncertainty_columns_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), dets, det_roi, src, max_out, det_width, w, num_rois, total, out);
  return check_launch("uncertainty_columns_kernel");
}

extern "C" int frcnn_make_rois(const float* sorted_boxes, const float* sorted_scores, const int64_t* keep_idx,
                               const int* keep_count, int max_keep, float* rois, float* roi_scores, void* stream_) {
  FRCNN_REQUIRE(sorted_boxes && sorted_scores && keep_idx && keep_count && rois && max_keep > 0,
                "make_rois: bad arguments");
  hipLaunchKernelGGL(make_rois_kernel, dim3((max_keep + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_),
                     sorted_boxes, sorted_scores, keep_idx, keep_count, max_keep, rois, roi_scores);
  return check_launch("make_rois_kernel");
}

extern "C" int frcnn_generate_anchors_3d(const float* base, int num_types, int height, int width, int feat_stride,
                                         float* anchors_3d, float* anchors_2d, void* stream_) {
  FRCNN_REQUIRE(base && anchors_3d && anchors_2d && num_types > 0 && height > 0 && width > 0 && feat_stride > 0,
                "generate_anchors_3d: bad arguments");
  const int total = height * width * num_types;
  hipLaunchKernelGGL(anchors3d_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), base, num_types, height, width, feat_stride, anchors_3d,
                     anchors_2d);
  return check_launch("anchors3d_kernel");
}

extern "C" int frcnn_bbox_transform_inv(const float* boxes, int box_ld, const float* deltas, int n, int num_classes,
                                        float scale, float* out, void* stream_) {
  FRCNN_REQUIRE(boxes && deltas && out && n > 0 && num_classes > 0 && box_ld >= 4, "bbox_transform_inv: bad arguments");
  const int total = n * num_classes;
  hipLaunchKernelGGL(bbox_transform_inv_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), boxes, box_ld, deltas, n, num_classes, scale, scale > 0.f ? 1 : 0,
                     out);
  return check_launch("bbox_transform_inv_kernel");
}

namespace {
// uncertainty_transform_inv / lidar_3d_uncertainty_transform_inv (lib/model/bbox_transform.py:107-130,132-169): a per-element
// uncertainty of the 7-element deltas [x,y,z,l,w,h,ry] mapped to box space and squared.  lidar == 0: the 4 BEV terms
// [x,y,l,w] -> out (n, 4K); lidar == 1: all 7 -> out (n, 7K).  Centre terms scale with the RoI's +1 sizes (z with the 3-D
// anchor's height), size terms are exp(u) - 1, the yaw term passes through.  The image form as written upstream omits the
// unsqueeze that makes the size factors per-box (see tests/golden/make_golden_uc_inv.py); per-box scaling is implemented.
__global__ __launch_bounds__(256) void uc_transform_inv_kernel(const float* __restrict__ rois, int roi_ld,
                                                              const float* __restrict__ anchors3d,
                                                              const float* __restrict__ uc, int n, int k, float scale,
                                                              int use_scale, int lidar, int is_var,
                                                              float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * k) return;
  const int i = t / k, c = t - i * k;
  const float* r = rois + (size_t)i * roi_ld;
  float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  if (use_scale) { x1 = x1 / scale; y1 = y1 / scale; x2 = x2 / scale; y2 = y2 / scale; }
  const float len = x2 - x1 + 1.f, wid = y2 - y1 + 1.f;
  float u[7];
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const float v = uc[((size_t)i * k + c) * 7 + e];
    u[e] = is_var ? sqrtf(v) : v;          // a variance is turned into the standard deviation the formulas take
  }
  const float ux = u[0] * len, uy = u[1] * wid;
  const float ul = exp_f32(u[3]) - 1.f, uw = exp_f32(u[4]) - 1.f;
  if (!lidar) {
    float* o = out + ((size_t)i * k + c) * 4;
    o[0] = ux * ux; o[1] = uy * uy; o[2] = ul * ul; o[3] = uw * uw;
    return;
  }
  const float ht = anchors3d[(size_t)i * 7 + 5];
  const float uz = u[2] * ht, uh = exp_f32(u[5]) - 1.f, ur = u[6];
  float* o = out + ((size_t)i * k + c) * 7;
  o[0] = ux * ux; o[1] = uy * uy; o[2] = uz * uz; o[3] = ul * ul; o[4] = uw * uw; o[5] = uh * uh; o[6] = ur * ur;
}
}  // namespace

extern "C" int frcnn_uncertainty_transform_inv(const float* rois, int roi_ld, const float* anchors_3d, const float* uncertainty,
                                               int n, int num_classes, float scale, int lidar, int input_is_variance, float* out,
                                               void* stream_) {
  FRCNN_REQUIRE(rois && uncertainty && out && n > 0 && num_classes > 0 && roi_ld >= 4 && (!lidar || anchors_3d),
                "uncertainty_transform_inv: bad arguments");
  const int total = n * num_classes;
  hipLaunchKernelGGL(uc_transform_inv_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_), rois,
                     roi_ld, anchors_3d, uncertainty, n, num_classes, scale, scale > 0.f ? 1 : 0, lidar ? 1 : 0,
                     input_is_variance ? 1 : 0, out);
  return check_launch("uc_transform_inv_kernel");
}

extern "C" int frcnn_lidar_bbox_transform_inv(const float* rois, int roi_ld, const float* anchors_3d,
                                              const float* deltas, int n, int num_classes, float scale, float* out,
                                              void* stream_) {
  FRCNN_REQUIRE(rois && anchors_3d && deltas && out && n > 0 && num_classes > 0 && roi_ld >= 4,
                "lidar_bbox_transform_inv: bad arguments");
  const int total = n * num_classes;
  hipLaunchKernelGGL(lidar_bbox_transform_inv_kernel, dim3(std::min((total + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), rois, roi_ld, anchors_3d, deltas, n, num_classes, scale,
                     scale > 0.f ? 1 : 0, out);
  return check_launch("lidar_bbox_transform_inv_kernel");
}

extern "C" int frcnn_fpn_level_map(const float* rois, int num_rois, int k_min, int k_max, float canonical_scale,
                                   float canonical_level, float eps, int* levels, void* stream_) {
  FRCNN_REQUIRE(rois && levels && num_rois > 0 && k_min <= k_max && canonical_scale > 0.f, "fpn_level_map: bad arguments");
  hipLaunchKernelGGL(fpn_level_map_kernel, dim3(std::min((num_rois + 255) / 256, 1024)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), rois, num_rois, k_min, k_max, canonical_scale, canonical_level, eps,
                     levels);
  return check_launch("fpn_level_map_kernel");
}

extern "C" int frcnn_clip_boxes(const float* boxes, int num_boxes, const float* info_host, float* out, void* stream_) {
  FRCNN_REQUIRE(boxes && out && info_host && num_boxes > 0, "clip_boxes: bad arguments");
  ClipInfo clip{info_host[0], info_host[1] - 1.0f, info_host[2], info_host[3] - 1.0f};
  hipLaunchKernelGGL(clip_boxes_kernel, dim3(std::min((num_boxes + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), boxes, num_boxes, clip, out);
  return check_launch("clip_boxes_kernel");
}

