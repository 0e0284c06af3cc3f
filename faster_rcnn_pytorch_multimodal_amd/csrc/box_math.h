// Box arithmetic shared by the proposal / detection-tail kernels.  Every translation unit that includes
// this header is compiled with -ffp-contract=off: the reference evaluates these expressions as separate
// torch elementwise ops (one rounding per op), so no mul+add may fuse into an fma here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "common.h"

namespace frcnn {

// exp() rounded once from a double evaluation: within 1 ulp of any faithful fp32 expf (the CPU's
// vectorised expf is not bit-reproducible across ISAs, so this is the best-defined target).
__device__ __forceinline__ float exp_f32(float v) { return (float)exp((double)v); }

// bbox_transform_inv for one (box, delta) pair — lib/model/bbox_transform.py:82-103.
// The codec is non-standard: centre deltas are scaled by the box DIAGONAL sqrt(w^2+h^2) (:84,:94-95),
// widths use the +1 convention (:82-83) and x2 = cx + 0.5*w' (no -1) (:99-103).
__device__ __forceinline__ void decode_box(float x1, float y1, float x2, float y2, float dx, float dy, float dw,
                                           float dh, float out[4]) {
  const float w = x2 - x1 + 1.0f;
  const float h = y2 - y1 + 1.0f;
  const float diag = sqrtf(w * w + h * h);
  const float cx = x1 + 0.5f * w;
  const float cy = y1 + 0.5f * h;
  const float pcx = dx * diag + cx;
  const float pcy = dy * diag + cy;
  const float pw = exp_f32(dw) * w;
  const float ph = exp_f32(dh) * h;
  out[0] = pcx - 0.5f * pw;
  out[1] = pcy - 0.5f * ph;
  out[2] = pcx + 0.5f * pw;
  out[3] = pcy + 0.5f * ph;
}

// lidar_3d_bbox_transform_inv for one (roi, 3-D anchor, delta) triple — lib/model/bbox_transform.py:185-222:
// length/width/centre from the axis-aligned RoI (+1 convention, centre = x1 + len/2), height and z from the
// 3-D anchor, centre deltas scaled by the RoI diagonal, heading = raw delta.
__device__ __forceinline__ void decode_box_lidar(float x1, float y1, float x2, float y2, const float* anchor3d,
                                                 const float d[7], float out[7]) {
  const float ln = x2 - x1 + 1.0f, wd = y2 - y1 + 1.0f, ht = anchor3d[5];
  const float cx = x1 + ln / 2.0f, cy = y1 + wd / 2.0f, cz = anchor3d[2];
  const float diag = sqrtf(ln * ln + wd * wd);
  out[0] = d[0] * diag + cx;
  out[1] = d[1] * diag + cy;
  out[2] = d[2] * ht + cz;
  out[3] = exp_f32(d[3]) * ln;
  out[4] = exp_f32(d[4]) * wd;
  out[5] = exp_f32(d[5]) * ht;
  out[6] = d[6];
}

// torch.clamp(v, lo, hi) = min(max(v, lo), hi), and like torch's it hands a NaN through (fminf / fmaxf would return the
// bound: a NaN coordinate of a diverged regression would silently become a frame edge).  clamp_min / clamp_max likewise.
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clamp_minf(float v, float lo) { return v < lo ? lo : v; }
__device__ __forceinline__ float clamp_maxf(float v, float hi) { return v > hi ? hi : v; }

// What happens when IoU == threshold exactly is a RUN-TIME choice (frcnn_nms_set_suppress_at_equal, csrc/nms.hip; DESIGN.md
// section 1): torchvision 0.4.0 (req.txt:283, not vendored) suppresses on `iou >= threshold` in its CPU kernel and on
// `iou > threshold` in its CUDA kernel.  The default follows the CPU kernel - the path the reference is compared against.
// The kernels below always test `iou > t`; for the inclusive form the entry points hand them t = nextafterf(threshold, -inf):
// no float lies strictly between the two, so `iou > t` IS `iou >= threshold`, bit for bit, NaN included (both false).
inline float nms_kernel_thresh(float thresh) {
  return frcnn_nms_get_suppress_at_equal() ? nextafterf(thresh, -INFINITY) : thresh;
}

// IoU test of torchvision.ops.nms: areas (x2-x1)*(y2-y1) without +1, suppress when iou > thresh (see above).
__device__ __forceinline__ bool iou_gt(const float* a, const float* b, float thresh) {
  const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
  const float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
  const float w = fmaxf(xx2 - xx1, 0.f), h = fmaxf(yy2 - yy1, 0.f);
  const float inter = w * h;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  const float iou = inter / (sa + sb - inter);
  return iou > thresh;
}

// The same predicate, bit for bit, with the IEEE division (~25 instructions) taken only near the threshold: inter against
// thresh * union decides every other pair with a margin (1e-6 relative, against 2^-24 rounding in each of the two
// products and half an ulp in the quotient); degenerate boxes (union <= 0, NaN) always take the division.  Pays where the
// IoU count per lane is small and instruction-bound (the per-class filter); the 64-deep serial loop of nms_mask_kernel
// is faster with the plain form.
__device__ __forceinline__ bool iou_gt_lazy_div(const float* a, const float* b, float thresh) {
  const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
  const float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
  const float w = fmaxf(xx2 - xx1, 0.f), h = fmaxf(yy2 - yy1, 0.f);
  const float inter = w * h;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  const float uni = sa + sb - inter;
  const float tu = thresh * uni;
  const bool sure_yes = inter > tu * 1.000001f, sure_no = inter < tu * 0.999999f;
  bool hit = sure_yes;
  if (!(uni > 0.f) || !(sure_yes || sure_no)) {   // rarely taken (skipped when no lane of the wave needs it)
    const float iou = inter / uni;
    hit = iou > thresh;
  }
  return hit;
}

// fp32 -> u32 key whose ASCENDING order is DESCENDING score (-0 is folded into +0 first).  NaN - with either sign bit - gets
// the smallest key: torch.sort(descending=True) (lib/layer_utils/proposal_layer.py:39) ranks NaN above +Inf, ties by index.
__device__ __forceinline__ uint32_t desc_key(float s) {
  if (s != s) return 0u;
  if (s == 0.f) s = 0.f;
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// In-LDS bitonic sort (ascending) of npad (power of two) u64 keys by the whole workgroup.
__device__ __forceinline__ void block_bitonic_sort(uint64_t* keys, int npad) {
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npad / 2; i += blockDim.x) {
        // pair (a, a+j) where a has bit j clear
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int b = a | j;
        const uint64_t ka = keys[a], kb = keys[b];
        const bool up = (a & k) == 0;
        if ((ka > kb) == up) {
          keys[a] = kb;
          keys[b] = ka;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace frcnn
