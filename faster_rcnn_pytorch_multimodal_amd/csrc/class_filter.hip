// Per-class detection filter on axis-aligned boxes - filter_and_draw_prep, lib/utils/filter_predictions.py:75-130 (+ the
// max_dets cut of test.py:210-221): clamp, threshold, sort, NMS, cut, outputs.  The steps shared with the rotated filter
// are in class_filter.h.  Built with -ffp-contract=off (see box_math.h).
#include "class_filter.h"

#include <algorithm>

using namespace frcnn;

namespace {

// Greedy scan over a precomputed suppression bit-matrix by ONE wave (lane = threadIdx.x & 63).
// mask[i*nb + w] bit b set  <=>  box (w*64+b) has IoU > thresh with box i and (w*64+b) > i.
// Boxes are in descending-score order.  Writes survivors' positions to keep_idx (first max_keep of them)
// and optional per-box bytes to keep_mask (pre-zeroed by the caller).  nb <= 256.
// MaskPtr: `const uint64_t*` (global) or an address_space(3) pointer when the matrix lives in LDS - a generic pointer
// would turn every row fetch into a flat load (40 of the 75 us of the per-class filter kernel were that).
template <typename MaskPtr, typename KeepPtr>
__device__ __forceinline__ int wave_nms_scan(MaskPtr mask, int nb, int n, int max_keep, KeepPtr keep_idx,
                                             uint8_t* keep_mask) {
  const int lane = threadIdx.x & 63;
  uint64_t rm0 = 0, rm1 = 0, rm2 = 0, rm3 = 0;  // removed bits of words lane, lane+64, lane+128, lane+192
  int count = 0;
  // The chain per 64-box chunk is: diagonal word of the 64 rows -> in-register greedy resolve -> rows of the kept boxes
  // OR-ed into the removed set -> next chunk.  Two memory latencies per chunk would sit on that chain; the diagonal
  // word of the NEXT chunk does not depend on anything computed here, so it is fetched one chunk ahead, and the rows
  // of up to four kept boxes are requested together before any of them is consumed.
  uint64_t d_next = (lane < n) ? mask[(size_t)lane * nb] : 0ull;
  for (int c = 0; c < nb && c * 64 < n && count < max_keep; ++c) {
    const int i = c * 64 + lane;
    const uint64_t d = d_next;
    {
      const int in = i + 64;
      d_next = (c + 1 < nb && in < n) ? mask[(size_t)in * nb + (c + 1)] : 0ull;
    }
    const int slot = c >> 6;
    const uint64_t mine = slot == 0 ? rm0 : slot == 1 ? rm1 : slot == 2 ? rm2 : rm3;
    const uint64_t rw = readlane_u64(mine, c & 63);
    const int live = n - c * 64;
    const uint64_t valid = live >= 64 ? ~0ull : ((1ull << live) - 1ull);
    uint64_t alive = ~rw & valid;
    uint64_t kept = 0;
    int nk = 0;
    while (alive != 0 && count + nk < max_keep) {
      const int b = __builtin_ctzll(alive);
      kept |= 1ull << b;
      ++nk;
      const uint64_t db = readlane_u64(d, b);
      alive &= ~(db | (1ull << b));
    }
    if ((kept >> lane) & 1ull) {
      const int pos = count + __builtin_popcountll(kept & ((1ull << lane) - 1ull));
      keep_idx[pos] = i;
      if (keep_mask) keep_mask[i] = 1;
    }
    count += nk;
    if (count >= max_keep) break;
    uint64_t todo = kept;
    while (todo != 0) {
      MaskPtr rows[4];
      int nr = 0;
      for (; nr < 4 && todo != 0; ++nr) {
        rows[nr] = mask + (size_t)(c * 64 + __builtin_ctzll(todo)) * nb;
        todo &= todo - 1ull;
      }
      for (int q = nr; q < 4; ++q) rows[q] = rows[0];      // duplicates: OR is idempotent
      // unconditional loads at a clamped word index (issued back to back), masked afterwards; slots beyond the row
      // length are skipped by a wave-uniform branch
      uint64_t v[4][4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        if (s4 * 64 < nb) {
          const int w = lane + 64 * s4;
          const int wc = min(w, nb - 1);
          const bool ok = w > c && w < nb;
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q][s4] = rows[q][wc];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q][s4] = ok ? v[q][s4] : 0ull;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q][s4] = 0ull;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        rm0 |= v[q][0];
        rm1 |= v[q][1];
        rm2 |= v[q][2];
        rm3 |= v[q][3];
      }
    }
  }
  return count;
}

__global__ __launch_bounds__(256) void clamp_pred_boxes_kernel(float* __restrict__ boxes, int total_boxes, float x_hi,
                                                              float y_hi) {
  // filter_predictions.py:85-91: x1,y1 = clamp_min(0); x2 = clamp_max(frame_w/scale - 1); y2 likewise
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total_boxes; i += gridDim.x * blockDim.x) {
    float4 b = reinterpret_cast<float4*>(boxes)[i];
    b.x = clamp_minf(b.x, 0.f);
    b.y = clamp_minf(b.y, 0.f);
    b.z = clamp_maxf(b.z, x_hi);
    b.w = clamp_maxf(b.w, y_hi);
    reinterpret_cast<float4*>(boxes)[i] = b;
  }
}

constexpr int FILTER_THREADS = 256;

// the rectangle NMS runs on: the image box itself (E = 4) or the yaw-less BEV rectangle of a LiDAR box (E = 7)
template <int E>
__device__ __forceinline__ float4 nms_box(const float* pb) {
  return E == 4 ? make_float4(pb[0], pb[1], pb[2], pb[3])
                : make_float4(pb[0] - pb[3] / 2.0f, pb[1] - pb[4] / 2.0f, pb[0] + pb[3] / 2.0f, pb[1] + pb[4] / 2.0f);
}

// One workgroup per foreground class.  ws per class: sorted boxes [R][4] floats, mask [R][nb] u64,
// keep_idx [R] int64.  E = 4: image boxes; E = 7: LiDAR boxes [xc,yc,zc,l,w,h,ry], suppressed on the
// yaw-less BEV rectangle xc -+ l/2, yc -+ w/2 (filter_predictions.py:55-62,67); rows of dets are E+1 wide.
// Block 0 writes the background class's slice (class_filter.h fill_background).
template <int E>
__global__ __launch_bounds__(FILTER_THREADS) void filter_class_kernel(
    const float* __restrict__ pred_boxes, const float* __restrict__ cls_prob, const int* __restrict__ roi_count,
    int num_rois, int num_classes, float thresh, float nms_thresh, int max_dets, int max_out, int npad, int nb,
    float* __restrict__ dets, int* __restrict__ det_count, int* __restrict__ det_roi, unsigned char* __restrict__ ws,
    size_t ws_per_class) {
  extern __shared__ __attribute__((aligned(16))) unsigned char filt_smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(filt_smem);  // [npad]
  __shared__ int s_n, s_keep;
  const int cls = blockIdx.x, t = threadIdx.x;
  if (cls == 0) return fill_background<E, FILTER_THREADS>(max_out, dets, det_count, det_roi);
  const int R = roi_count ? min(*roi_count, num_rois) : num_rois;
  unsigned char* my = ws + (size_t)(blockIdx.x - 1) * ws_per_class;
  float* sboxes = reinterpret_cast<float*>(my);
  uint64_t* mask = reinterpret_cast<uint64_t*>(my + align_up((size_t)num_rois * 16, 16));
  int64_t* keep_idx = reinterpret_cast<int64_t*>(reinterpret_cast<unsigned char*>(mask) + (size_t)num_rois * nb * 8);
  for (int i = t; i < npad; i += FILTER_THREADS) keys[i] = ~0ull;   // the bitonic sort's padding
  const int n = select_class_keys<FILTER_THREADS>(cls_prob, R, num_classes, cls, thresh, keys, &s_n);
  block_bitonic_sort(keys, npad);  // (score desc, roi index asc)
  for (int i = t; i < n; i += FILTER_THREADS)   // the low word of a key is its RoI
    reinterpret_cast<float4*>(sboxes)[i] = nms_box<E>(pred_boxes + ((size_t)(uint32_t)keys[i] * num_classes + cls) * E);
  __syncthreads();
  // suppression bit-matrix (words on/right of the diagonal)
  const int nbl = (n + 63) / 64;
  for (int wi = t; wi < n * nbl; wi += FILTER_THREADS) {
    const int i = wi / nbl, w = wi - i * nbl;
    if (w < (i >> 6)) continue;
    uint64_t bits = 0;
    const int jn = min(64, n - w * 64);
    for (int b = 0; b < jn; ++b) {
      const int j = w * 64 + b;
      if (j > i && iou_gt(&sboxes[i * 4], &sboxes[j * 4], nms_thresh)) bits |= 1ull << b;
    }
    mask[(size_t)i * nbl + w] = bits;
  }
  __syncthreads();
  if (t < 64) {
    const int cnt = wave_nms_scan(mask, nbl, n, n, keep_idx, nullptr);
    if (t == 0) s_keep = cnt;
  }
  __syncthreads();
  const int kept = cut_at_max_dets<FILTER_THREADS>(keys, keep_idx, s_keep, max_dets, &s_n);
  write_class_dets<E, FILTER_THREADS>(pred_boxes, cls_prob, num_classes, cls, keys, keep_idx, kept, max_out, dets, det_count,
                                      det_roi);
}

// Same per-class filter for num_rois <= 1024 (every detector of the reference: 300 test-time RoIs), entirely in LDS
// with 16 waves.  The general kernel above spent 161 us per frame on ONE workgroup of 4 waves: a 45-stage bitonic
// sort of 512 keys, a suppression matrix with one thread looping over the 64 IoUs of a word, and a greedy scan whose
// row fetches each paid a global-memory round trip.  Here: keys are ranked (unique keys: position = number of smaller
// keys, n broadcast LDS reads per thread, no stage barriers), one WAVE builds a matrix word with one IoU per lane and a
// ballot, and the matrix (n x ceil(n/64) words) stays in LDS for the scan.  Same order, same IoU test, same outputs.
constexpr int FILTER_SMALL_THREADS = 1024, FILTER_SMALL_MAX = 1024;

template <int E>
__global__ __launch_bounds__(FILTER_SMALL_THREADS) void filter_class_small_kernel(
    const float* __restrict__ pred_boxes, const float* __restrict__ cls_prob, const int* __restrict__ roi_count,
    int num_rois, int num_classes, float thresh, float nms_thresh, int max_dets, int max_out, float* __restrict__ dets,
    int* __restrict__ det_count, int* __restrict__ det_roi) {
  extern __shared__ __attribute__((aligned(16))) unsigned char filt_smem[];
  // LDS: raw keys [num_rois] | sorted keys [num_rois] | boxes [num_rois] float4 | keep_idx [num_rois] i64 | mask [n][nbl] u64
  uint64_t* raw = reinterpret_cast<uint64_t*>(filt_smem);
  uint64_t* keys = raw + num_rois;
  float4* sboxes = reinterpret_cast<float4*>(keys + num_rois);
  int64_t* keep_idx = reinterpret_cast<int64_t*>(sboxes + num_rois);
  uint64_t* mask = reinterpret_cast<uint64_t*>(keep_idx + num_rois);
  __shared__ int s_n;
  const int cls = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (cls == 0) return fill_background<E, FILTER_SMALL_THREADS>(max_out, dets, det_count, det_roi);
  const int R = roi_count ? min(*roi_count, num_rois) : num_rois;
  const int n = select_class_keys<FILTER_SMALL_THREADS>(cls_prob, R, num_classes, cls, thresh, raw, &s_n);
  rank_sort_keys<FILTER_SMALL_THREADS>(raw, n, [&](int rank, uint64_t key) {
    keys[rank] = key;
    sboxes[rank] = nms_box<E>(pred_boxes + ((size_t)(uint32_t)(key & 0xFFFFFFFFu) * num_classes + cls) * E);
  });
  __syncthreads();
  // PREDECESSOR matrix P[j] = bits i < j with IoU(i, j) > nms_thresh (boxes in descending-score order): one wave per
  // 64-box word of the upper triangle, one IoU per lane, the hits scattered to the transposed position by LDS atomics
  // (sparse); the greedy rule is then a fixed point over P (class_filter.h nms_fixed_point), which a serial scan paid
  // with 40 of this kernel's 75 us.
  const int nbl = (n + 63) / 64;
  uint64_t* const P = mask;
  __shared__ unsigned long long s_sets[2 * (FILTER_SMALL_MAX / 64)];   // kept set [nbl] | removed set [nbl]
  for (int e = t; e < n * nbl; e += FILTER_SMALL_THREADS) P[e] = 0ull;
  __syncthreads();
  // work unit = (word w of boxes j, chunk c <= w of predecessors i, quarter of the chunk): lane j keeps its box in
  // registers, the 16 predecessor boxes are LDS broadcasts, the hits are collected in a register word - one LDS atomic
  // per lane and unit
  constexpr int PARTS = 4, ROWS = 64 / PARTS;
  const int units = nbl * (nbl + 1) / 2 * PARTS;
  for (int u = wave; u < units; u += FILTER_SMALL_THREADS / 64) {
    int pair = u / PARTS, w = 0;
    const int part = u - pair * PARTS;
    while (pair > w) { pair -= w + 1; ++w; }
    const int c = pair;
    const int j = w * 64 + lane;
    const float4 bj = sboxes[min(j, n - 1)];
    const float b[4] = {bj.x, bj.y, bj.z, bj.w};
    const int i0 = c * 64 + part * ROWS;
    uint64_t word = 0ull;
#pragma unroll 4
    for (int ii = 0; ii < ROWS; ++ii) {
      const int i = i0 + ii;
      if (i >= n) break;
      const float4 bi = sboxes[i];
      const float a[4] = {bi.x, bi.y, bi.z, bi.w};
      if (j < n && j > i && iou_gt_lazy_div(a, b, nms_thresh)) word |= 1ull << (i & 63);
    }
    if (word != 0ull) atomicOr(reinterpret_cast<unsigned long long*>(&P[(size_t)j * nbl + c]), word);
  }
  __syncthreads();
  nms_fixed_point<FILTER_SMALL_THREADS, 1>(P, nbl, n, s_sets, s_sets + FILTER_SMALL_MAX / 64);
  int kept = kept_positions<FILTER_SMALL_THREADS, 1>(s_sets, n, keep_idx);   // survivors in ascending box order
  kept = cut_at_max_dets<FILTER_SMALL_THREADS>(keys, keep_idx, kept, max_dets, &s_n);
  write_class_dets<E, FILTER_SMALL_THREADS>(pred_boxes, cls_prob, num_classes, cls, keys, keep_idx, kept, max_out, dets,
                                            det_count, det_roi);
}

static size_t filter_small_lds(int num_rois) {
  const size_t nb = (size_t)(num_rois + 63) / 64;
  return (size_t)num_rois * (8 + 8 + 16 + 8) + (size_t)num_rois * nb * 8;
}

}  // namespace

// test hook: 0 = automatic (LDS kernel for num_rois <= 1024), 1 = always the general kernel
static int g_filter_variant = 0;
extern "C" int frcnn_filter_set_variant(int v) {
  g_filter_variant = v;
  return FRCNN_OK;
}
// the filter variant in the low word, the rule at IoU == threshold (nms.hip) in the high word
unsigned long long frcnn::boxes_settings_word() {
  return (unsigned long long)(unsigned)g_filter_variant |
         ((unsigned long long)(unsigned)frcnn_nms_get_suppress_at_equal() << 32);
}

static size_t filter_ws_per_class(int num_rois) {
  const size_t nb = (size_t)(num_rois + 63) / 64;
  return align_up(align_up((size_t)num_rois * 16, 16) + (size_t)num_rois * nb * 8 + (size_t)num_rois * 8, 16);
}

extern "C" size_t frcnn_filter_per_class_ws_bytes(int num_rois, int num_classes) {
  if (num_rois <= 0 || num_classes <= 1) return 0;
  return filter_ws_per_class(num_rois) * (size_t)(num_classes - 1);
}

template <int E>
static int launch_filter(float* pred_boxes, const float* cls_prob, const int* roi_count, int num_rois, int num_classes,
                         float frame_w, float frame_h, float scale, float thresh, float nms_thresh, int max_dets,
                         int max_out, float* dets, int* det_count, int* det_roi, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(pred_boxes && cls_prob && dets && det_count && num_rois > 0 && num_classes > 1 && max_out > 0,
                "filter_per_class: bad arguments");
  FRCNN_REQUIRE(num_rois <= 8192, "filter_per_class: num_rois %d > 8192", num_rois);
  const size_t need = frcnn_filter_per_class_ws_bytes(num_rois, num_classes);
  if (!ws || ws_bytes < need) return fail(FRCNN_ERR_WS, "filter_per_class: workspace %zu < %zu bytes", ws_bytes, need);
  nms_thresh = nms_kernel_thresh(nms_thresh);
  if (E == 4) {
    // frame_width/scale - 1 evaluated in fp32 like the numpy float32 scalars of filter_predictions.py:77-91
    const float x_hi = frame_w / scale - 1.0f, y_hi = frame_h / scale - 1.0f;
    const int total_boxes = num_rois * num_classes;
    hipLaunchKernelGGL(clamp_pred_boxes_kernel, dim3(std::min((total_boxes + 255) / 256, 1024)), dim3(256), 0, stream,
                       pred_boxes, total_boxes, x_hi, y_hi);
    int rc = check_launch("clamp_pred_boxes_kernel");
    if (rc != FRCNN_OK) return rc;
  }  // LiDAR boxes are not clamped (filter_predictions.py:92-93)
  if (num_rois <= FILTER_SMALL_MAX && filter_small_lds(num_rois) <= (size_t)150 * 1024 && g_filter_variant != 1) {
    const size_t lds = filter_small_lds(num_rois);
    const int rc = ensure_dynamic_lds<&filter_class_small_kernel<E>>(lds, "filter_per_class");
    if (rc != FRCNN_OK) return rc;
    hipLaunchKernelGGL(filter_class_small_kernel<E>, dim3(num_classes), dim3(FILTER_SMALL_THREADS), lds, stream,
                       pred_boxes, cls_prob, roi_count, num_rois, num_classes, thresh, nms_thresh, max_dets, max_out, dets,
                       det_count, det_roi);
    return check_launch("filter_class_small_kernel");
  }
  const int npad = next_pow2(std::max(num_rois, 2));
  const int nb = (num_rois + 63) / 64;
  const size_t lds = (size_t)npad * 8;
  const int rc = ensure_dynamic_lds<&filter_class_kernel<E>>(lds, "filter_per_class");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(filter_class_kernel<E>, dim3(num_classes), dim3(FILTER_THREADS), lds, stream, pred_boxes,
                     cls_prob, roi_count, num_rois, num_classes, thresh, nms_thresh, max_dets, max_out, npad, nb, dets,
                     det_count, det_roi, static_cast<unsigned char*>(ws), filter_ws_per_class(num_rois));
  return check_launch("filter_class_kernel");
}

extern "C" int frcnn_filter_per_class(float* pred_boxes, const float* cls_prob, const int* roi_count, int num_rois,
                                      int num_classes, float frame_w, float frame_h, float scale, float thresh,
                                      float nms_thresh, int max_dets, int max_out, float* dets, int* det_count,
                                      int* det_roi, void* ws, size_t ws_bytes, void* stream_) {
  return launch_filter<4>(pred_boxes, cls_prob, roi_count, num_rois, num_classes, frame_w, frame_h, scale, thresh,
                          nms_thresh, max_dets, max_out, dets, det_count, det_roi, ws, ws_bytes, stream_);
}

extern "C" int frcnn_filter_per_class_lidar(const float* pred_boxes, const float* cls_prob, const int* roi_count,
                                            int num_rois, int num_classes, float thresh, float nms_thresh,
                                            int max_dets, int max_out, float* dets, int* det_count, int* det_roi,
                                            void* ws, size_t ws_bytes, void* stream_) {
  return launch_filter<7>(const_cast<float*>(pred_boxes), cls_prob, roi_count, num_rois, num_classes, 0.f, 0.f, 1.f,
                          thresh, nms_thresh, max_dets, max_out, dets, det_count, det_roi, ws, ws_bytes, stream_);
}
