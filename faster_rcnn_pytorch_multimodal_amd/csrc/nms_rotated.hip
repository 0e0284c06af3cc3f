// Rotated BEV NMS: greedy suppression of yawed 7-DoF boxes [xc,yc,zc,l,w,h,ry] on their ROTATED footprints - the form the
// reference's authors left commented out at lib/utils/filter_predictions.py:56-57 ("Turned off auto rotating"); the
// shipped rule (:55-67) suppresses on the yaw-less rectangle xc -+ l/2, yc -+ w/2 (class_filter.hip, E = 7).
// Opt-in (cfg.TEST.NMS_ROTATED), no default changes.
//
// Contract (utils/bbox.nms_rotated_host is its host statement).  Boxes in (score descending, RoI index ascending) order,
// float32 rows widened to float64 exactly.  For i < j
//     iou(i, j) = frcnn_eval::pair_overlap<EVAL_TYPE_BEV>(det = geom(box_j), gt = geom(box_i))
// which is datasets/waymo_eval.iou(bbgt = box_i[None], bb = box_j, 'bev') term for term (eval_overlap.h, compiled with
// -ffp-contract=off).  Box j is removed when a KEPT i < j has iou >= (double)thresh (frcnn_nms_set_suppress_at_equal(1),
// default) or iou > (double)thresh (0).  A NaN overlap compares false both ways: it never suppresses.  thresh <= 0 is
// refused: disjoint boxes (iou == 0) would suppress each other, and the early-out below relies on thresh > 0.
// Early-out, the only shortcut: a pair whose bounding circles (centre (xc, yc), radius 0.5 hypot(|l|, |w|)) are disjoint
// by a relative margin has an empty clip, iou == +-0 or NaN, and is not clipped.  The test is written `d2 > bound`: a NaN
// or an infinity anywhere makes it false and the pair takes the full computation.
//
// Three launches on the caller's stream, sized by the worst case (n_cap boxes), the live counts read on the device; no
// host synchronisation, no memset / memcpy nodes.  The steps that do not depend on the overlap (select, rank, fixed
// point, positions, cut, write) are those of class_filter.h, shared with the axis-aligned filters.
//   1. stage   one workgroup per class: select_class_keys, rank_sort_keys; write the sorted keys and one staged box
//              (box_geom<EVAL_TYPE_BEV>: corners, edge vectors, area; plus the bounding circle) per box to the
//              workspace.  Stand-alone entry: the boxes arrive sorted, one thread per box.
//   2. pair    grid = classes x 64x64 word tiles (w >= c) of the upper triangle x the 64 boxes j of word w.  One wave:
//              lane = predecessor i of word c, its staged box in registers, box j read as a broadcast, ONE overlap per
//              lane.  Each lane owns two Poly slots as LDS columns (2 x 8 vertices x 2 doubles x 64 lanes = 16 KiB, like
//              frcnn_eval_match_kernel with a quarter of its lanes: up to 10 workgroups per compute unit).  The wave's
//              ballot over its 64 verdicts is the predecessor word P[j][c], stored whole: every word the decide step
//              reads is written exactly once, so P needs no clearing and no atomics.  A clip is a chain of dependent
//              float64 operations, so the phase lasts as long as the clips ONE lane does in turn: one, chosen by
//              measurement against 2, 4 and 8 boxes j per wave (profiles/rotated_nms.md).  300 RoIs are 960 waves per
//              class, 1024 RoIs 8704.
//   3. decide  one workgroup per class: nms_fixed_point ( keep(j) <=> no kept predecessor in P[j] ), kept_positions,
//              cut_at_max_dets (lib/model/test.py:213-221) and write_class_dets.  Up to 1024 boxes P sits in LDS (1024 x
//              16 words = 128 KiB of gfx950's 160 KiB); the stand-alone entry beyond that reads it from the workspace.
// Plain HIP, vector stores only.
#include "class_filter.h"
#include "eval_overlap.h"

#include <algorithm>

using namespace frcnn;
using namespace frcnn_eval;

namespace {

constexpr int ROT_FILTER_MAX = 1024;      // RoIs per frame of the filter (the reference uses 300)
constexpr int ROT_NMS_MAX = 4096;         // boxes of the stand-alone entry
constexpr int ROT_THREADS = 1024;         // stage and decide workgroups
constexpr int ROT_PER = ROT_NMS_MAX / ROT_THREADS;   // boxes per thread of the decide step, at most
constexpr int PAIR_THREADS = 64;
// doubles per staged box: EVAL_GEOM_DOUBLES slots, of which 0-15 corners and edge vectors, 16 area as in eval_match.hip;
// 17-19 (height range and volume there) hold the bounding circle xc, yc, radius here
constexpr int G = EVAL_GEOM_DOUBLES;
constexpr int G_AREA = 16, G_XC = 17, G_YC = 18, G_RAD = 19;
// two circles count as disjoint when centre distance^2 > (r_i + r_j)^2 * this
constexpr double CIRCLE_MARGIN = 1.0 + 1e-6;

// Workspace of one class: staged boxes [G][n_cap] doubles | P [n_cap][nbl] u64 | keys [n_cap] u64 | count (16 bytes).
struct RotLayout {
  size_t geom, pred, keys, count, total;
  int nbl;
};
__host__ __device__ inline RotLayout rot_layout(int n_cap) {
  RotLayout l;
  l.nbl = (n_cap + 63) / 64;
  l.geom = 0;
  l.pred = l.geom + (size_t)G * n_cap * sizeof(double);
  l.keys = l.pred + (size_t)n_cap * l.nbl * sizeof(uint64_t);
  l.count = l.keys + (size_t)n_cap * sizeof(uint64_t);
  l.total = l.count + 16;
  return l;
}

// one box -> its staged form, column `col` of geom[G][n_cap]
__device__ inline void stage_box(const float* __restrict__ b7, double* __restrict__ geom, int n_cap, int col) {
  double b[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) b[q] = (double)b7[q];
  BoxGeom g;
  box_geom<EVAL_TYPE_BEV>(b, g);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    geom[(size_t)k * n_cap + col] = g.cx[k];
    geom[(size_t)(4 + k) * n_cap + col] = g.cy[k];
    geom[(size_t)(8 + k) * n_cap + col] = g.ex[k];
    geom[(size_t)(12 + k) * n_cap + col] = g.ey[k];
  }
  geom[(size_t)G_AREA * n_cap + col] = g.area;
  geom[(size_t)G_XC * n_cap + col] = b[0];
  geom[(size_t)G_YC * n_cap + col] = b[1];
  geom[(size_t)G_RAD * n_cap + col] = 0.5 * hypot(fabs(b[3]), fabs(b[4]));
}

// ---- 1. select and stage ------------------------------------------------------------------------------------------------
// Filter: one workgroup per foreground class (blockIdx.x + 1).  inds = scores[:, c] > thresh (filter_predictions.py:46),
// order (score desc, RoI index asc) by ranking the unique keys.
__global__ __launch_bounds__(ROT_THREADS) void rot_stage_filter_kernel(const float* __restrict__ pred_boxes,
                                                                      const float* __restrict__ cls_prob,
                                                                      const int* __restrict__ roi_count, int num_rois,
                                                                      int num_classes, float thresh,
                                                                      unsigned char* __restrict__ ws, size_t ws_per_class) {
  __shared__ uint64_t raw[ROT_FILTER_MAX];
  __shared__ int s_n;
  const int cls = blockIdx.x + 1, t = threadIdx.x;
  const RotLayout l = rot_layout(num_rois);
  unsigned char* my = ws + (size_t)blockIdx.x * ws_per_class;
  double* geom = reinterpret_cast<double*>(my + l.geom);
  uint64_t* keys = reinterpret_cast<uint64_t*>(my + l.keys);
  const int R = roi_count ? max(0, min(*roi_count, num_rois)) : num_rois;
  const int n = select_class_keys<ROT_THREADS>(cls_prob, R, num_classes, cls, thresh, raw, &s_n);
  rank_sort_keys<ROT_THREADS>(raw, n, [&](int rank, uint64_t key) {
    keys[rank] = key;
    stage_box(pred_boxes + ((size_t)(uint32_t)(key & 0xFFFFFFFFu) * num_classes + cls) * 7, geom, num_rois, rank);
  });
  if (t == 0) *reinterpret_cast<int*>(my + l.count) = n;
}

// Stand-alone: the boxes arrive in descending score order.
__global__ __launch_bounds__(256) void rot_stage_sorted_kernel(const float* __restrict__ boxes7,
                                                              const int* __restrict__ n_dev, int n_max,
                                                              unsigned char* __restrict__ ws) {
  const RotLayout l = rot_layout(n_max);
  const int n = n_dev ? max(0, min(*n_dev, n_max)) : n_max;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *reinterpret_cast<int*>(ws + l.count) = n;
  if (i < n) stage_box(boxes7 + (size_t)i * 7, reinterpret_cast<double*>(ws + l.geom), n_max, i);
}

// ---- 2. pair phase ------------------------------------------------------------------------------------------------------
// blockIdx.x = (tile, box of the tile), blockIdx.y = class.  Tile = (w, c <= w); box j of word w against the 64
// predecessors of word c: lane = predecessor i, its staged box in registers, box j read as a broadcast.  One overlap per
// lane; the wave's ballot IS the predecessor word P[j][c], stored whole by lane 0 - every word the decide step reads
// (j < n, c <= j / 64) is written exactly once, empty or not.
__global__ __launch_bounds__(PAIR_THREADS) void rot_pair_kernel(unsigned char* __restrict__ ws, size_t ws_per_class,
                                                               int n_cap, double thresh, int at_equal) {
  __shared__ double poly[2][2][EVAL_MAX_VERTS][PAIR_THREADS];   // [slot][x / y][vertex][lane]
  const RotLayout l = rot_layout(n_cap);
  unsigned char* my = ws + (size_t)blockIdx.y * ws_per_class;
  const double* __restrict__ geom = reinterpret_cast<const double*>(my + l.geom);
  uint64_t* __restrict__ P = reinterpret_cast<uint64_t*>(my + l.pred);
  const int n = *reinterpret_cast<const int*>(my + l.count);
  const int lane = threadIdx.x;
  int pair = blockIdx.x >> 6, w = 0;
  while (pair > w) { pair -= w + 1; ++w; }
  const int c = pair;
  const int j = w * 64 + (blockIdx.x & 63);
  if (j >= n) return;                                        // not a live box: nobody reads its row
  const int i = c * 64 + lane;
  const bool live = i < n;                                   // n <= n_cap: the loads below stay inside the class's arrays
  BoxGeom gt;
  double xc = 0.0, yc = 0.0, rad = 0.0;
  if (live) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gt.cx[k] = geom[(size_t)k * n_cap + i];
      gt.cy[k] = geom[(size_t)(4 + k) * n_cap + i];
      gt.ex[k] = geom[(size_t)(8 + k) * n_cap + i];
      gt.ey[k] = geom[(size_t)(12 + k) * n_cap + i];
    }
    gt.area = geom[(size_t)G_AREA * n_cap + i];
    xc = geom[(size_t)G_XC * n_cap + i];
    yc = geom[(size_t)G_YC * n_cap + i];
    rad = geom[(size_t)G_RAD * n_cap + i];
  }
  const Poly pa{&poly[0][0][0][lane], &poly[0][1][0][lane], PAIR_THREADS};
  const Poly pb{&poly[1][0][0][lane], &poly[1][1][0][lane], PAIR_THREADS};
  bool hit = false;
  if (live && i < j) {
    const double dx = geom[(size_t)G_XC * n_cap + j] - xc, dy = geom[(size_t)G_YC * n_cap + j] - yc;
    const double rr = geom[(size_t)G_RAD * n_cap + j] + rad;
    if (!(dx * dx + dy * dy > rr * rr * CIRCLE_MARGIN)) {      // NaN / inf: not "disjoint", the pair is clipped
      BoxGeom det;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        det.cx[k] = geom[(size_t)k * n_cap + j];
        det.cy[k] = geom[(size_t)(4 + k) * n_cap + j];
      }
      det.area = geom[(size_t)G_AREA * n_cap + j];
      const double ov = pair_overlap<EVAL_TYPE_BEV>(det, gt, pa, pb);
      hit = at_equal ? ov >= thresh : ov > thresh;
    }
  }
  const unsigned long long word = __ballot(hit);
  if (lane == 0) P[(size_t)j * l.nbl + c] = word;
}

// ---- 3. decide and write ------------------------------------------------------------------------------------------------
// The fixed point over P, the kept boxes' positions, the cut and the outputs: class_filter.h, ROT_PER boxes per thread.
// Filter: one workgroup per class; class 0 (background) writes its empty slice of every output.
__global__ __launch_bounds__(ROT_THREADS) void rot_decide_filter_kernel(
    const float* __restrict__ pred_boxes, const float* __restrict__ cls_prob, int num_rois, int num_classes, int max_dets,
    int max_out, float* __restrict__ dets, int* __restrict__ det_count, int* __restrict__ det_roi,
    const unsigned char* __restrict__ ws, size_t ws_per_class) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rot_smem[];
  __shared__ unsigned long long s_sets[2 * (ROT_NMS_MAX / 64)];
  constexpr int E = 7;
  const int cls = blockIdx.x, t = threadIdx.x;
  if (cls == 0) return fill_background<E, ROT_THREADS>(max_out, dets, det_count, det_roi);
  const RotLayout l = rot_layout(num_rois);
  const unsigned char* my = ws + (size_t)(cls - 1) * ws_per_class;
  const uint64_t* __restrict__ Pg = reinterpret_cast<const uint64_t*>(my + l.pred);
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(my + l.keys);
  const int n = *reinterpret_cast<const int*>(my + l.count);
  const int nbl = (n + 63) / 64;                               // LDS rows are as wide as the live count needs
  uint64_t* P = reinterpret_cast<uint64_t*>(rot_smem);         // [num_rois][<= l.nbl]
  int* order = reinterpret_cast<int*>(P + (size_t)num_rois * l.nbl);   // [num_rois]
  for (int e = t; e < n * nbl; e += ROT_THREADS) {
    const int j = e / nbl, w = e - j * nbl;
    if (w <= (j >> 6)) P[e] = Pg[(size_t)j * l.nbl + w];
  }
  nms_fixed_point<ROT_THREADS, ROT_PER>(P, nbl, n, s_sets, s_sets + ROT_NMS_MAX / 64);
  int kept = kept_positions<ROT_THREADS, ROT_PER>(s_sets, n, order);
  kept = cut_at_max_dets<ROT_THREADS>(keys, order, kept, max_dets, reinterpret_cast<int*>(s_sets + ROT_NMS_MAX / 64));
  write_class_dets<E, ROT_THREADS>(pred_boxes, cls_prob, num_classes, cls, keys, order, kept, max_out, dets, det_count,
                                   det_roi);
}

// Stand-alone: the outputs of frcnn_nms.  P is read from the workspace (up to 4096 boxes x 64 words).
__global__ __launch_bounds__(ROT_THREADS) void rot_decide_sorted_kernel(const unsigned char* __restrict__ ws, int n_max,
                                                                       int max_keep, int64_t* __restrict__ keep_idx,
                                                                       uint8_t* __restrict__ keep_mask,
                                                                       int* __restrict__ keep_count) {
  __shared__ unsigned long long s_sets[2 * (ROT_NMS_MAX / 64)];
  __shared__ int order[ROT_NMS_MAX];
  const RotLayout l = rot_layout(n_max);
  const int n = *reinterpret_cast<const int*>(ws + l.count);
  const int t = threadIdx.x;
  nms_fixed_point<ROT_THREADS, ROT_PER>(reinterpret_cast<const uint64_t*>(ws + l.pred), l.nbl, n, s_sets,
                                        s_sets + ROT_NMS_MAX / 64);
  const int kept = min(kept_positions<ROT_THREADS, ROT_PER>(s_sets, n, order), max_keep);
  for (int i = t; i < max_keep; i += ROT_THREADS) keep_idx[i] = i < kept ? (int64_t)order[i] : 0;
  if (keep_mask) {
    for (int j = t; j < n_max; j += ROT_THREADS) keep_mask[j] = 0;
    __syncthreads();
    for (int i = t; i < kept; i += ROT_THREADS) keep_mask[order[i]] = 1;
  }
  if (t == 0) keep_count[0] = kept;
}

size_t rot_decide_lds(int num_rois) {
  const RotLayout l = rot_layout(num_rois);
  return (size_t)num_rois * l.nbl * sizeof(uint64_t) + (size_t)num_rois * sizeof(int);
}

int rot_launch_pairs(void* ws, size_t ws_per_class, int n_cap, int classes, float thresh, hipStream_t stream) {
  const int nbl = (n_cap + 63) / 64;
  hipLaunchKernelGGL(rot_pair_kernel, dim3(nbl * (nbl + 1) / 2 * 64, classes), dim3(PAIR_THREADS), 0, stream,
                     static_cast<unsigned char*>(ws), ws_per_class, n_cap, (double)thresh,
                     frcnn_nms_get_suppress_at_equal());
  return check_launch("rot_pair_kernel");
}

}  // namespace

extern "C" size_t frcnn_nms_rotated_ws_bytes(int n_max) {
  if (n_max <= 0 || n_max > ROT_NMS_MAX) return 0;
  return rot_layout(n_max).total;
}

extern "C" int frcnn_nms_rotated(const float* boxes7, const int* n_dev, int n_max, float thresh, int max_keep,
                                 int64_t* keep_idx, uint8_t* keep_mask, int* keep_count, void* ws, size_t ws_bytes,
                                 void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(boxes7 && keep_idx && keep_count && n_max > 0 && max_keep > 0, "nms_rotated: bad arguments");
  FRCNN_REQUIRE(n_max <= ROT_NMS_MAX, "nms_rotated: n_max %d > %d", n_max, ROT_NMS_MAX);
  FRCNN_REQUIRE(thresh > 0.f, "nms_rotated: thresh %g must be > 0 (disjoint boxes have IoU 0)", (double)thresh);
  const size_t need = frcnn_nms_rotated_ws_bytes(n_max);
  if (!ws || ws_bytes < need) return fail(FRCNN_ERR_WS, "nms_rotated: workspace %zu < %zu bytes", ws_bytes, need);
  unsigned char* w = static_cast<unsigned char*>(ws);
  hipLaunchKernelGGL(rot_stage_sorted_kernel, dim3((n_max + 255) / 256), dim3(256), 0, stream, boxes7, n_dev, n_max, w);
  int rc = check_launch("rot_stage_sorted_kernel");
  if (rc != FRCNN_OK) return rc;
  rc = rot_launch_pairs(ws, need, n_max, 1, thresh, stream);
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(rot_decide_sorted_kernel, dim3(1), dim3(ROT_THREADS), 0, stream, (const unsigned char*)w, n_max,
                     std::min(max_keep, n_max), keep_idx, keep_mask, keep_count);
  return check_launch("rot_decide_sorted_kernel");
}

extern "C" size_t frcnn_filter_per_class_lidar_rot_ws_bytes(int num_rois, int num_classes) {
  if (num_rois <= 0 || num_rois > ROT_FILTER_MAX || num_classes <= 1) return 0;
  return rot_layout(num_rois).total * (size_t)(num_classes - 1);
}

extern "C" int frcnn_filter_per_class_lidar_rot(const float* pred_boxes, const float* cls_prob, const int* roi_count,
                                                int num_rois, int num_classes, float thresh, float nms_thresh,
                                                int max_dets, int max_out, float* dets, int* det_count, int* det_roi,
                                                void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(pred_boxes && cls_prob && dets && det_count && num_rois > 0 && num_classes > 1 && max_out > 0,
                "filter_per_class_lidar_rot: bad arguments");
  FRCNN_REQUIRE(num_rois <= ROT_FILTER_MAX, "filter_per_class_lidar_rot: num_rois %d > %d", num_rois, ROT_FILTER_MAX);
  FRCNN_REQUIRE(nms_thresh > 0.f, "filter_per_class_lidar_rot: nms_thresh %g must be > 0 (disjoint boxes have IoU 0)",
                (double)nms_thresh);
  const size_t need = frcnn_filter_per_class_lidar_rot_ws_bytes(num_rois, num_classes);
  if (!ws || ws_bytes < need)
    return fail(FRCNN_ERR_WS, "filter_per_class_lidar_rot: workspace %zu < %zu bytes", ws_bytes, need);
  const size_t per_class = rot_layout(num_rois).total;
  unsigned char* w = static_cast<unsigned char*>(ws);
  hipLaunchKernelGGL(rot_stage_filter_kernel, dim3(num_classes - 1), dim3(ROT_THREADS), 0, stream, pred_boxes, cls_prob,
                     roi_count, num_rois, num_classes, thresh, w, per_class);
  int rc = check_launch("rot_stage_filter_kernel");
  if (rc != FRCNN_OK) return rc;
  rc = rot_launch_pairs(ws, per_class, num_rois, num_classes - 1, nms_thresh, stream);
  if (rc != FRCNN_OK) return rc;
  const size_t lds = rot_decide_lds(num_rois);
  rc = ensure_dynamic_lds<&rot_decide_filter_kernel>(lds, "filter_per_class_lidar_rot");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(rot_decide_filter_kernel, dim3(num_classes), dim3(ROT_THREADS), lds, stream, pred_boxes, cls_prob,
                     num_rois, num_classes, max_dets, max_out, dets, det_count, det_roi, (const unsigned char*)w, per_class);
  return check_launch("rot_decide_filter_kernel");
}
