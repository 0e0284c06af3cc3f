// Detection tail: spatial mean (fc7), the two Linear heads, class softmax and test-time box decode,
// fused in one launch (one workgroup per RoI), for up to 12 image / 8 LiDAR classes; for more classes the wide form at the
// end of this file: the heads as an MFMA GEMM on fc7, then softmax and decode.
//
// Reference: _head_to_tail tail `.mean(3).mean(2)` and _region_classification of the missing
// lib/nets/network.py (module names lib/nets/imagenet.py:83-86), test-time de-normalisation with
// cfg.TRAIN.IMAGE.BBOX_NORMALIZE_{STDS,MEANS} (lib/model/config.py:222-223) and
// bbox_transform_inv(rois[:,1:5], deltas, scales=info[6]) (lib/model/bbox_transform.py:75-105;
// evidence lib/model/test.py:75-79, lib/utils/filter_predictions.py:85-91).
// Built with -ffp-contract=off (box_math.h).
#include "common.h"
#include "box_math.h"

using namespace frcnn;

namespace {

constexpr int HEAD_THREADS = 256;
constexpr int MAX_OUT = 64;  // K + 4K <= 64 -> up to 12 classes (8 for LiDAR); more go through the wide form below

struct HeadNorm {
  float stds[7], means[7];
};

// E = 4: image boxes [x1,y1,x2,y2]; E = 7: LiDAR boxes [xc,yc,zc,l,w,h,ry] decoded from the RoI and the
// RoI's 3-D anchor (lib/model/bbox_transform.py:174-233).
template <int E>
__global__ __launch_bounds__(HEAD_THREADS) void head_fc_softmax_decode_kernel(
    const float* __restrict__ x, int P, int C, const float* __restrict__ w_cls, const float* __restrict__ b_cls,
    const float* __restrict__ w_box, const float* __restrict__ b_box, int K, const float* __restrict__ rois,
    const float* __restrict__ roi_anchors, HeadNorm norm, float scale, float* __restrict__ fc7,
    float* __restrict__ cls_score, float* __restrict__ cls_prob, float* __restrict__ bbox_pred,
    float* __restrict__ pred_boxes) {
  extern __shared__ __attribute__((aligned(16))) float head_smem[];  // [C] fc7 + [MAX_OUT] head outputs
  float* s_fc7 = head_smem;
  float* s_out = head_smem + C;
  const int r = blockIdx.x, t = threadIdx.x;
  const int C4 = C / 4;
  const float4* xr = reinterpret_cast<const float4*>(x) + (size_t)r * P * P * C4;
  const float inv = (float)P;
  // fc7 = x.mean(3).mean(2): mean over W inside each row, then mean over the P row means
  for (int c4 = t; c4 < C4; c4 += HEAD_THREADS) {
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = 0; h < P; ++h) {
      float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int w = 0; w < P; ++w) {
        const float4 v = xr[(size_t)(h * P + w) * C4 + c4];
        row.x += v.x; row.y += v.y; row.z += v.z; row.w += v.w;
      }
      tot.x += row.x / inv; tot.y += row.y / inv; tot.z += row.z / inv; tot.w += row.w / inv;
    }
    tot.x /= inv; tot.y /= inv; tot.z /= inv; tot.w /= inv;
    reinterpret_cast<float4*>(s_fc7)[c4] = tot;
    if (fc7) reinterpret_cast<float4*>(fc7)[(size_t)r * C4 + c4] = tot;
  }
  __syncthreads();
  // K class logits + 4K box deltas: one wave per output, 64 lanes stride the channel dimension
  const int lane = t & 63, wave = t >> 6;
  const int n_out = K * (1 + E);
  for (int o = wave; o < n_out; o += HEAD_THREADS / 64) {
    const float* wrow = o < K ? w_cls + (size_t)o * C : w_box + (size_t)(o - K) * C;
    float acc = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
      const float4 a = reinterpret_cast<const float4*>(s_fc7)[c4];
      const float4 b = reinterpret_cast<const float4*>(wrow)[c4];
      acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) s_out[o] = acc + (o < K ? b_cls[o] : b_box[o - K]);
  }
  __syncthreads();
  if (t == 0) {
    // softmax over classes (torch: subtract max, exp, normalise)
    float m = s_out[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, s_out[k]);
    float e[MAX_OUT / 5 + 1], sum = 0.f;  // K <= MAX_OUT / (1 + E) <= MAX_OUT / 5
    for (int k = 0; k < K; ++k) { e[k] = exp_f32(s_out[k] - m); sum += e[k]; }
    for (int k = 0; k < K; ++k) {
      cls_score[(size_t)r * K + k] = s_out[k];
      cls_prob[(size_t)r * K + k] = e[k] / sum;
    }
  }
  if (t < K) {
    // boxes = rois[:,1:5] / scale ; deltas*stds + means ; decode
    const float* roi = rois + (size_t)r * 5;
    const float x1 = roi[1] / scale, y1 = roi[2] / scale, x2 = roi[3] / scale, y2 = roi[4] / scale;
    float d[E];
    for (int q = 0; q < E; ++q) {
      const float raw = s_out[K + t * E + q];
      bbox_pred[(size_t)r * K * E + t * E + q] = raw;
      d[q] = raw * norm.stds[q] + norm.means[q];
    }
    float o[E];
    if (E == 4) {
      decode_box(x1, y1, x2, y2, d[0], d[1], d[2], d[3], o);
    } else {
      float d7[7], o7[7];
      for (int q = 0; q < 7; ++q) d7[q] = d[q < E ? q : 0];
      decode_box_lidar(x1, y1, x2, y2, roi_anchors + (size_t)r * 7, d7, o7);
      for (int q = 0; q < E; ++q) o[q] = o7[q];
    }
    for (int q = 0; q < E; ++q) pred_boxes[(size_t)r * K * E + t * E + q] = o[q];
  }
}

}  // namespace

template <int E>
static int launch_head(const float* x, int num_rois, int pooled, int c, const float* w_cls, const float* b_cls,
                       const float* w_box, const float* b_box, int num_classes, const float* rois,
                       const float* roi_anchors, const float* stds_host, const float* means_host, float scale,
                       float* fc7, float* cls_score, float* cls_prob, float* bbox_pred, float* pred_boxes,
                       void* stream_) {
  FRCNN_REQUIRE(x && w_cls && b_cls && w_box && b_box && rois && stds_host && means_host && cls_score && cls_prob &&
                    bbox_pred && pred_boxes && (E == 4 || roi_anchors),
                "head_fc_softmax_decode: null argument");
  FRCNN_REQUIRE(num_rois > 0 && pooled > 0 && c > 0 && c % 4 == 0 && num_classes >= 2 &&
                    num_classes * (1 + E) <= MAX_OUT && scale > 0.f,
                "head_fc_softmax_decode: bad shape (c%%4==0, 2 <= classes <= %d)", MAX_OUT / (1 + E));
  HeadNorm norm;
  for (int q = 0; q < 7; ++q) { norm.stds[q] = q < E ? stds_host[q] : 1.f; norm.means[q] = q < E ? means_host[q] : 0.f; }
  const size_t lds = ((size_t)c + MAX_OUT) * sizeof(float);
  FRCNN_REQUIRE(lds <= 64 * 1024, "head_fc_softmax_decode: c=%d too large", c);
  hipLaunchKernelGGL(head_fc_softmax_decode_kernel<E>, dim3(num_rois), dim3(HEAD_THREADS), lds,
                     static_cast<hipStream_t>(stream_), x, pooled, c, w_cls, b_cls, w_box, b_box, num_classes, rois,
                     roi_anchors, norm, scale, fc7, cls_score, cls_prob, bbox_pred, pred_boxes);
  return check_launch("head_fc_softmax_decode_kernel");
}

extern "C" int frcnn_head_fc_softmax_decode(const float* x, int num_rois, int pooled, int c, const float* w_cls,
                                            const float* b_cls, const float* w_box, const float* b_box,
                                            int num_classes, const float* rois, const float* stds_host,
                                            const float* means_host, float scale, float* fc7, float* cls_score,
                                            float* cls_prob, float* bbox_pred, float* pred_boxes, void* stream_) {
  return launch_head<4>(x, num_rois, pooled, c, w_cls, b_cls, w_box, b_box, num_classes, rois, nullptr, stds_host,
                        means_host, scale, fc7, cls_score, cls_prob, bbox_pred, pred_boxes, stream_);
}

extern "C" int frcnn_head_fc_softmax_decode_lidar(const float* x, int num_rois, int pooled, int c,
                                                  const float* w_cls, const float* b_cls, const float* w_box,
                                                  const float* b_box, int num_classes, const float* rois,
                                                  const float* roi_anchors_3d, const float* stds_host,
                                                  const float* means_host, float scale, float* fc7,
                                                  float* cls_score, float* cls_prob, float* bbox_pred,
                                                  float* pred_boxes, void* stream_) {
  return launch_head<7>(x, num_rois, pooled, c, w_cls, b_cls, w_box, b_box, num_classes, rois, roi_anchors_3d,
                        stds_host, means_host, scale, fc7, cls_score, cls_prob, bbox_pred, pred_boxes, stream_);
}

// ------------------------------------------------------------------------------------------------
// Wide form of the tail: any class count (PASCAL VOC 21, COCO 81, KITTI's full LiDAR label set 9, ...).
//
// At K(1+E) > MAX_OUT the heads are a GEMM, fc7 (R, C) x [w_cls; w_box]^T (C, K(1+E)), and run as one on
// v_mfma_f32_32x32x2_f32; the one-workgroup-per-RoI kernel above would read both weight matrices once per RoI.  Two launches
// (DESIGN.md section 4.26):
//   1. head_wide_logits_kernel: one workgroup per 32 RoIs x 32 outputs x HALF of the channels (blockIdx.z; the split point
//      depends on C alone).  128 channels of both operands per stage go global -> registers -> LDS, the next stage's loads in
//      flight under this stage's MFMAs (rows past R / past K(1+E) and chunks past the half's end are zero-filled, never
//      read); a stage's channels are split among the four waves (32 each), every wave accumulates a whole 32 x 32 partial
//      tile, and the four partials are added in wave order through LDS.  An output column o reads w_cls[o] (o < K) or
//      w_box[o - K] by its own address: no concatenated copy.  The first half's sums go to cls_score / bbox_pred, the second
//      half's to cls_prob / pred_boxes: the outputs the second launch writes last double as the scratch of the first, so
//      there is no workspace.  The fp32 matrix pipe runs at the vector rate, one 32 x 32 x 2048 tile is ~8 us of MFMA issue on
//      one CU: the split halves that, and two workgroups (66 KB of LDS each) share a CU and fill each other's LDS stalls.
//   2. head_wide_softmax_decode_kernel: one wave per RoI: logit = (first half + second half) + bias, stored, then the
//      arithmetic of the kernel above (maximum, exp_f32(s - m), fp32 sum in class order, divide; raw * std + mean through
//      decode_box / decode_box_lidar).
// The order of every sum depends on C alone, so a RoI's outputs do not depend on R or on the tile it fell into.
// No atomics, no workspace, no host synchronisation.
// ------------------------------------------------------------------------------------------------
namespace {

typedef float wide_f32x4 __attribute__((ext_vector_type(4)));
typedef float wide_f32x16 __attribute__((ext_vector_type(16)));

constexpr int WIDE_THREADS = 256;
constexpr int WIDE_TILE = 32;              // RoIs per workgroup = outputs per workgroup = one MFMA tile
constexpr int WIDE_BK = 128;               // channels per stage, 32 per wave
constexpr int WIDE_LD = WIDE_BK + 4;       // LDS row stride in floats: rows stay 16-byte aligned, 4 banks apart
constexpr int WIDE_CHUNKS = WIDE_BK / 4;   // 16-byte chunks per tile row
constexpr int WIDE_PASSES = WIDE_TILE * WIDE_CHUNKS / WIDE_THREADS;   // chunks per thread, operand and stage
constexpr int WIDE_ROWS_PER_PASS = WIDE_THREADS / WIDE_CHUNKS;
constexpr size_t WIDE_LDS_BYTES = sizeof(float) * 2 * 2 * WIDE_TILE * WIDE_LD;   // 66 KB: two workgroups per CU
constexpr int WIDE_MAX_CLASSES = 4096;
constexpr int WIDE_MAX_ROIS = 1 << 20;

// first channel of the second half: the 16-byte chunks of a row split in two, the odd one to the first half
__host__ __device__ inline int wide_split_point(int C) { return ((C / 4 + 1) / 2) * 4; }

__global__ __launch_bounds__(WIDE_THREADS) void head_wide_logits_kernel(
    const float* __restrict__ fc7, int R, int C, const float* __restrict__ w_cls, const float* __restrict__ w_box, int K,
    int N, float* __restrict__ cls_half0, float* __restrict__ box_half0, float* __restrict__ cls_half1,
    float* __restrict__ box_half1) {
  // [buffer][operand: 0 = fc7 rows, 1 = weight rows][row][channel]; reused for the four partial tiles at the end
  extern __shared__ __attribute__((aligned(16))) float wide_smem[];
  float(*s_tile)[2][WIDE_TILE][WIDE_LD] = reinterpret_cast<float(*)[2][WIDE_TILE][WIDE_LD]>(wide_smem);
  static_assert(WIDE_LDS_BYTES >= sizeof(float) * 4 * WIDE_TILE * (WIDE_TILE + 1), "partial tiles must fit");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * WIDE_TILE, n0 = blockIdx.x * WIDE_TILE;
  const int half = blockIdx.z;
  const int c_begin = half ? wide_split_point(C) : 0, c_end = half ? C : wide_split_point(C);

  // staging: thread t moves 16-byte chunk (t % 32) of tile rows (t / 32) + 8 i, i < 4, of both operands
  const int ch = t % WIDE_CHUNKS, row0 = t / WIDE_CHUNKS;
  const float* pa[WIDE_PASSES];
  const float* pb[WIDE_PASSES];
#pragma unroll
  for (int i = 0; i < WIDE_PASSES; ++i) {
    const int m = m0 + row0 + WIDE_ROWS_PER_PASS * i, o = n0 + row0 + WIDE_ROWS_PER_PASS * i;
    pa[i] = m < R ? fc7 + (size_t)m * C : nullptr;
    pb[i] = o < N ? (o < K ? w_cls + (size_t)o * C : w_box + (size_t)(o - K) * C) : nullptr;
  }
  wide_f32x4 ra[WIDE_PASSES], rb[WIDE_PASSES];
  auto load_stage = [&](int step) {
    const int c = c_begin + step * WIDE_BK + ch * 4;
    const bool c_ok = c < c_end;         // C % 4 == 0 and so is the split point: a chunk is all in or all out
#pragma unroll
    for (int i = 0; i < WIDE_PASSES; ++i) {
      ra[i] = (pa[i] && c_ok) ? *reinterpret_cast<const wide_f32x4*>(pa[i] + c) : wide_f32x4{0.f, 0.f, 0.f, 0.f};
      rb[i] = (pb[i] && c_ok) ? *reinterpret_cast<const wide_f32x4*>(pb[i] + c) : wide_f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < WIDE_PASSES; ++i) {
      *reinterpret_cast<wide_f32x4*>(&s_tile[buf][0][row0 + WIDE_ROWS_PER_PASS * i][ch * 4]) = ra[i];
      *reinterpret_cast<wide_f32x4*>(&s_tile[buf][1][row0 + WIDE_ROWS_PER_PASS * i][ch * 4]) = rb[i];
    }
  };

  wide_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int steps = (c_end - c_begin + WIDE_BK - 1) / WIDE_BK;      // 0 for the second half of C = 4
  load_stage(0);
  store_stage(0);
  __syncthreads();
  int cur = 0;
  for (int step = 0; step < steps; ++step) {
    const bool more = step + 1 < steps;
    if (more) load_stage(step + 1);
    // wave w owns channels 32 w .. 32 w + 31 of the stage; lane half h holds channels 8 q + 4 h + j (j = 0..3) of them, so
    // MFMA (q, j) multiplies channel pair (8 q + j, 8 q + 4 + j): the same fixed order for every row and column
#pragma unroll
    for (int q = 0; q < WIDE_BK / 32; ++q) {
      const int k = (WIDE_BK / 4) * wave + 8 * q + 4 * lh;
      const wide_f32x4 a = *reinterpret_cast<const wide_f32x4*>(&s_tile[cur][0][l31][k]);
      const wide_f32x4 b = *reinterpret_cast<const wide_f32x4*>(&s_tile[cur][1][l31][k]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    if (more) store_stage(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // D: column (lane & 31) = output, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = RoI.  A barrier has passed since the last
  // read of the staging tiles
  float(*s_part)[WIDE_TILE][WIDE_TILE + 1] = reinterpret_cast<float(*)[WIDE_TILE][WIDE_TILE + 1]>(wide_smem);
#pragma unroll
  for (int r = 0; r < 16; ++r) s_part[wave][(r & 3) + 8 * (r >> 2) + 4 * lh][l31] = acc[r];
  __syncthreads();
  float* cls_out = half ? cls_half1 : cls_half0;
  float* box_out = half ? box_half1 : box_half0;
#pragma unroll
  for (int i = 0; i < WIDE_TILE * WIDE_TILE / WIDE_THREADS; ++i) {
    const int idx = t + WIDE_THREADS * i;
    const int row = idx >> 5, col = idx & 31;
    const int m = m0 + row, o = n0 + col;
    if (m >= R || o >= N) continue;
    const float v = ((s_part[0][row][col] + s_part[1][row][col]) + s_part[2][row][col]) + s_part[3][row][col];
    if (o < K)
      cls_out[(size_t)m * K + o] = v;
    else
      box_out[(size_t)m * (N - K) + (o - K)] = v;
  }
}

// On entry cls_score / bbox_pred hold the first half's sums and cls_prob / pred_boxes the second half's.  Every element is
// read, finished and written by the same lane, so the four arrays may not be __restrict__ here.
template <int E>
__global__ __launch_bounds__(WIDE_THREADS) void head_wide_softmax_decode_kernel(
    float* cls_score, float* bbox_pred, int R, int K, const float* __restrict__ b_cls, const float* __restrict__ b_box,
    const float* __restrict__ rois, const float* __restrict__ roi_anchors, HeadNorm norm, float scale, float* cls_prob,
    float* pred_boxes) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (WIDE_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= R) return;                      // whole waves leave; no barrier below
  float* s = cls_score + (size_t)r * K;
  float* prob = cls_prob + (size_t)r * K;
  // logits, and the softmax over classes (torch: subtract max, exp, normalise); the maximum does not depend on the order it
  // is taken in.  Lane l finishes classes l, l + 64, ... and is the only one to read them back
  float m = -INFINITY;
  for (int k = lane; k < K; k += 64) {
    const float v = (s[k] + prob[k]) + b_cls[k];
    s[k] = v;
    m = fmaxf(m, v);
  }
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  // the sum in class order 0..K-1, like the single thread of the kernel above: every lane adds the same K terms
  float sum = 0.f;
  for (int base = 0; base < K; base += 64) {
    const int k = base + lane;
    const float e = k < K ? exp_f32(s[k] - m) : 0.f;
    const int n = K - base < 64 ? K - base : 64;
    for (int j = 0; j < n; ++j) sum += __shfl(e, j);
  }
  for (int k = lane; k < K; k += 64) prob[k] = exp_f32(s[k] - m) / sum;
  // boxes = rois[:,1:5] / scale ; deltas*stds + means ; decode
  const float* roi = rois + (size_t)r * 5;
  const float x1 = roi[1] / scale, y1 = roi[2] / scale, x2 = roi[3] / scale, y2 = roi[4] / scale;
  for (int k = lane; k < K; k += 64) {
    const size_t at = (size_t)r * K * E + (size_t)k * E;
    float d[7], o[7];
    for (int q = 0; q < 7; ++q) d[q] = 0.f;
    for (int q = 0; q < E; ++q) {
      const float raw = (bbox_pred[at + q] + pred_boxes[at + q]) + b_box[k * E + q];
      bbox_pred[at + q] = raw;
      d[q] = raw * norm.stds[q] + norm.means[q];
    }
    if (E == 4)
      decode_box(x1, y1, x2, y2, d[0], d[1], d[2], d[3], o);
    else
      decode_box_lidar(x1, y1, x2, y2, roi_anchors + (size_t)r * 7, d, o);
    for (int q = 0; q < E; ++q) pred_boxes[at + q] = o[q];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

template <int E>
static int launch_head_wide(const float* fc7, int num_rois, int c, const float* w_cls, const float* b_cls,
                            const float* w_box, const float* b_box, int num_classes, const float* rois,
                            const float* roi_anchors, const float* stds_host, const float* means_host, float scale,
                            float* cls_score, float* cls_prob, float* bbox_pred, float* pred_boxes, void* stream_) {
  FRCNN_REQUIRE(fc7 && w_cls && b_cls && w_box && b_box && rois && stds_host && means_host && cls_score && cls_prob &&
                    bbox_pred && pred_boxes && (E == 4 || roi_anchors),
                "head_wide_softmax_decode: null argument");
  FRCNN_REQUIRE(num_rois > 0 && num_rois <= WIDE_MAX_ROIS && c > 0 && c % 4 == 0 && num_classes >= 2 &&
                    num_classes <= WIDE_MAX_CLASSES && scale > 0.f,
                "head_wide_softmax_decode: bad shape (1 <= rois <= %d, c%%4==0, 2 <= classes <= %d, scale > 0)",
                WIDE_MAX_ROIS, WIDE_MAX_CLASSES);
  FRCNN_REQUIRE(aligned16(fc7) && aligned16(w_cls) && aligned16(w_box),
                "head_wide_softmax_decode: fc7, w_cls and w_box must be 16-byte aligned");
  FRCNN_REQUIRE(cls_prob != cls_score && pred_boxes != bbox_pred,
                "head_wide_softmax_decode: cls_prob / pred_boxes hold partial sums between the launches and must not alias "
                "cls_score / bbox_pred");
  HeadNorm norm;
  for (int q = 0; q < 7; ++q) { norm.stds[q] = q < E ? stds_host[q] : 1.f; norm.means[q] = q < E ? means_host[q] : 0.f; }
  const int n_out = num_classes * (1 + E);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 grid((n_out + WIDE_TILE - 1) / WIDE_TILE, (num_rois + WIDE_TILE - 1) / WIDE_TILE, 2);
  int rc = ensure_dynamic_lds<head_wide_logits_kernel>(WIDE_LDS_BYTES, "head_wide_softmax_decode");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(head_wide_logits_kernel, grid, dim3(WIDE_THREADS), WIDE_LDS_BYTES, stream, fc7, num_rois, c, w_cls,
                     w_box, num_classes, n_out, cls_score, bbox_pred, cls_prob, pred_boxes);
  rc = check_launch("head_wide_logits_kernel");
  if (rc != FRCNN_OK) return rc;
  const int waves = WIDE_THREADS / 64;
  hipLaunchKernelGGL(head_wide_softmax_decode_kernel<E>, dim3((num_rois + waves - 1) / waves), dim3(WIDE_THREADS), 0,
                     stream, cls_score, bbox_pred, num_rois, num_classes, b_cls, b_box, rois, roi_anchors, norm, scale,
                     cls_prob, pred_boxes);
  return check_launch("head_wide_softmax_decode_kernel");
}

extern "C" int frcnn_head_wide_softmax_decode(const float* fc7, int num_rois, int c, const float* w_cls,
                                              const float* b_cls, const float* w_box, const float* b_box,
                                              int num_classes, const float* rois, const float* stds_host,
                                              const float* means_host, float scale, float* cls_score, float* cls_prob,
                                              float* bbox_pred, float* pred_boxes, void* stream_) {
  return launch_head_wide<4>(fc7, num_rois, c, w_cls, b_cls, w_box, b_box, num_classes, rois, nullptr, stds_host,
                             means_host, scale, cls_score, cls_prob, bbox_pred, pred_boxes, stream_);
}

extern "C" int frcnn_head_wide_softmax_decode_lidar(const float* fc7, int num_rois, int c, const float* w_cls,
                                                    const float* b_cls, const float* w_box, const float* b_box,
                                                    int num_classes, const float* rois, const float* roi_anchors_3d,
                                                    const float* stds_host, const float* means_host, float scale,
                                                    float* cls_score, float* cls_prob, float* bbox_pred,
                                                    float* pred_boxes, void* stream_) {
  return launch_head_wide<7>(fc7, num_rois, c, w_cls, b_cls, w_box, b_box, num_classes, rois, roi_anchors_3d, stds_host,
                             means_host, scale, cls_score, cls_prob, bbox_pred, pred_boxes, stream_);
}
