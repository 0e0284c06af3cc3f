// COCO bbox matching on the device: what pycocotools' COCOeval.evaluate() does for every (image, category) pair of a
// results file (the call lib/datasets/coco.py:251-258 makes), as ONE launch.  The protocol is restated from its published
// description in datasets/coco_eval.py (PARITY UNPINNED against pycocotools, which is not a dependency); this unit equals
// that module's float64 host path bit for bit (tests/test_coco_eval_device.py).
//
// The host hands in the pairs in CSR form.  Ordering is an input: a pair's detections come in score order, already cut to
// the largest maxDets, its ground truth in annotation order; the thresholds and area ranges are numpy's float64 values
// (np.linspace is never recomputed here).  The device never sorts.
//
// One wavefront per pair, COCO_WAVES pairs per workgroup (the layout of bayes_ce_wide_kernel: pairs differ in size by two
// orders of magnitude, the dispatcher hands a free compute unit the next workgroup, nothing assumes equal work):
//   1. all 64 lanes compute the pair's D x G overlaps once (min / max / + / - / * / one division, float64, no contraction)
//      and store them to the `ious` output and, when D * G <= COCO_LDS_IOUS, to the wave's LDS slice.
//   2. ONE workgroup barrier (taken by every wave, with or without a pair).  Above the LDS budget the walks read the
//      overlaps back from the global output this wave has just written.
//   3. the A x T greedy walks of the pair are independent: lane l runs walk l, l + 64, ... (walk = a * T + t).  A walk
//      visits the detections in order and, per detection, the non-ignored ground truth in annotation order, then - only
//      if that pass matched nothing, which is the protocol's stop rule - the ignored ones.  "Non-ignored first, stable"
//      therefore needs no sort.  `v < best` skips, so an equal overlap replaces: the later box wins a tie.
//      The walk's "already matched" set is a 64-bit register mask for G <= 64 (with the ignore and crowd flags as two more
//      masks), and one byte per box in the caller's workspace, row `walk`, above that.  No per-lane array is indexed at
//      run time, so nothing goes to scratch memory.
//   4. per (box, area range) the ignore byte.
// LDS: COCO_LDS_IOUS = 1024 overlaps = 8 KiB per wave (100 detections x 10 boxes), 32 KiB per workgroup: five workgroups
// fit a compute unit's 160 KiB by LDS.
// Output layouts put the walk index innermost (dt_match / dt_ignore are (num_det, A, T), gt_ignore is (num_gt, A)), so the
// 64 lanes of a wave store one detection's verdicts to consecutive addresses.
// Compiled with -ffp-contract=off like every box-arithmetic unit.  Plain HIP, vector stores only, no atomics.
#include "common.h"

using namespace frcnn;

namespace {

constexpr int COCO_WAVES = FRCNN_COCO_PAIRS_PER_WG;
constexpr int COCO_THREADS = 64 * COCO_WAVES;
constexpr int COCO_LDS_IOUS = FRCNN_COCO_LDS_IOUS;
constexpr int COCO_MASK_GT = FRCNN_COCO_MASK_GT;
constexpr int BOX = 5;                                // x, y, w, h, area

struct CocoArgs {
  const double* det; const int* det_offsets; int num_det;
  const double* gt; const uint8_t* gt_crowd; const int* gt_offsets; int num_gt;
  const long long* iou_offsets; long long num_iou;
  const double* iou_thrs; int num_thr; const double* area_rng; int num_area;
  int num_pairs;
  double* ious; int* dt_match; uint8_t* dt_ignore; uint8_t* gt_ignore;
  uint8_t* ws;                                        // (A * T, num_gt) bytes or nullptr
};

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// datasets/coco_eval.py iou(), term for term
__device__ inline double overlap(const double* d, const double* g, bool crowd) {
  const double dx = d[0], dy = d[1], dw = d[2], dh = d[3];
  const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
  const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double i = iw * ih;
  const double u = crowd ? dw * dh : dw * dh + gw * gh - i;
  return i / u;
}

__global__ __launch_bounds__(COCO_THREADS) void frcnn_coco_match_kernel(CocoArgs a) {
  __shared__ double iou_lds[COCO_WAVES][COCO_LDS_IOUS];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = blockIdx.x * COCO_WAVES + wave;
  const int A = a.num_area, T = a.num_thr, walks = A * T;
  int d0 = 0, g0 = 0, D = 0, G = 0;
  long long io0 = 0;
  bool valid = p < a.num_pairs;
  if (valid) {
    d0 = clampi(a.det_offsets[p], 0, a.num_det);
    D = clampi(a.det_offsets[p + 1], d0, a.num_det) - d0;
    g0 = clampi(a.gt_offsets[p], 0, a.num_gt);
    G = clampi(a.gt_offsets[p + 1], g0, a.num_gt) - g0;
    io0 = a.iou_offsets[p];
    // a pair whose overlaps have no room (or would not index in 32 bits) is left alone
    valid = io0 >= 0 && (long long)D * G <= 0x7fffffffLL && io0 + (long long)D * G <= a.num_iou;
  }
  const int cells = valid ? D * G : 0;
  const bool in_lds = cells <= COCO_LDS_IOUS;
  double* lds = iou_lds[wave];
  double* glob = a.ious + io0;

  for (int c = lane; c < cells; c += 64) {
    const int d = c / G, g = c - d * G;
    const double v = overlap(a.det + (size_t)(d0 + d) * BOX, a.gt + (size_t)(g0 + g) * BOX, a.gt_crowd[g0 + g] != 0);
    glob[c] = v;
    if (in_lds) lds[c] = v;
  }
  __threadfence_block();
  __syncthreads();                                    // the only barrier: every wave of the workgroup arrives
  if (!valid) return;

  for (int c = lane; c < G * A; c += 64) {            // gt_ignore (num_gt, A)
    const int g = c / A, ar = c - g * A;
    const double area = a.gt[(size_t)(g0 + g) * BOX + 4];
    a.gt_ignore[(size_t)(g0 + g) * A + ar] =
        a.gt_crowd[g0 + g] != 0 || area < a.area_rng[2 * ar] || area > a.area_rng[2 * ar + 1];
  }

  const bool masks = G <= COCO_MASK_GT;
  const bool served = masks || a.ws != nullptr;
  for (int w = lane; w < walks; w += 64) {
    const int ar = w / T, t = w - ar * T;
    const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
    const double start = fmin(a.iou_thrs[t], 1.0 - 1e-10);
    if (!served) {                                    // more boxes than the caller's max_gt_per_pair said: not scored
      for (int d = 0; d < D; ++d) {
        a.dt_match[(size_t)(d0 + d) * walks + w] = -2;
        a.dt_ignore[(size_t)(d0 + d) * walks + w] = 0;
      }
      continue;
    }
    if (masks) {
      unsigned long long ign = 0, crowd = 0, matched = 0;
      for (int g = 0; g < G; ++g) {
        const double area = a.gt[(size_t)(g0 + g) * BOX + 4];
        const bool cr = a.gt_crowd[g0 + g] != 0;
        if (cr) crowd |= 1ull << g;
        if (cr || area < lo || area > hi) ign |= 1ull << g;
      }
      for (int d = 0; d < D; ++d) {
        const double* row = in_lds ? lds + d * G : glob + (size_t)d * G;
        double best = start;
        int m = -1;
        const unsigned long long taken = matched & ~crowd;
        for (int g = 0; g < G; ++g) {                 // the non-ignored boxes, annotation order
          if (((ign | taken) >> g) & 1) continue;
          const double v = row[g];
          if (v < best) continue;
          best = v;
          m = g;
        }
        if (m < 0)                                    // stop rule: the ignored boxes only when nothing matched yet
          for (int g = 0; g < G; ++g) {
            if (!((ign & ~taken) >> g & 1)) continue;
            const double v = row[g];
            if (v < best) continue;
            best = v;
            m = g;
          }
        bool dig;
        if (m >= 0) {
          matched |= 1ull << m;
          dig = (ign >> m) & 1;
        } else {
          const double area = a.det[(size_t)(d0 + d) * BOX + 4];
          dig = area < lo || area > hi;
        }
        a.dt_match[(size_t)(d0 + d) * walks + w] = m;
        a.dt_ignore[(size_t)(d0 + d) * walks + w] = dig;
      }
    } else {
      uint8_t* mine = a.ws + (size_t)w * a.num_gt + g0;     // this walk's matched bytes: private to the lane
      for (int g = 0; g < G; ++g) mine[g] = 0;
      for (int d = 0; d < D; ++d) {
        const double* row = in_lds ? lds + d * G : glob + (size_t)d * G;
        double best = start;
        int m = -1;
        bool m_ign = false;
        for (int pass = 0; pass < 2 && m < 0; ++pass)
          for (int g = 0; g < G; ++g) {
            const bool cr = a.gt_crowd[g0 + g] != 0;
            const double area = a.gt[(size_t)(g0 + g) * BOX + 4];
            const bool ig = cr || area < lo || area > hi;
            if (ig != (pass == 1)) continue;
            if (mine[g] && !cr) continue;
            const double v = row[g];
            if (v < best) continue;
            best = v;
            m = g;
            m_ign = ig;
          }
        bool dig = m_ign;
        if (m >= 0) {
          mine[m] = 1;
        } else {
          const double area = a.det[(size_t)(d0 + d) * BOX + 4];
          dig = area < lo || area > hi;
        }
        a.dt_match[(size_t)(d0 + d) * walks + w] = m;
        a.dt_ignore[(size_t)(d0 + d) * walks + w] = dig;
      }
    }
  }
}

}  // namespace

extern "C" size_t frcnn_coco_match_ws_bytes(int num_gt, int max_gt_per_pair, int num_area, int num_thr) {
  if (num_gt <= 0 || max_gt_per_pair <= COCO_MASK_GT || num_area <= 0 || num_thr <= 0) return 0;
  return (size_t)num_area * num_thr * num_gt;
}

extern "C" int frcnn_coco_match(const double* det, const int* det_offsets, int num_det, const double* gt,
                                const uint8_t* gt_crowd, const int* gt_offsets, int num_gt, const int64_t* iou_offsets,
                                int64_t num_iou, int num_pairs, const double* iou_thrs, int num_thr, const double* area_rng,
                                int num_area, int max_gt_per_pair, double* ious, int* dt_match, uint8_t* dt_ignore,
                                uint8_t* gt_ignore, void* ws, size_t ws_bytes, void* stream) {
  FRCNN_REQUIRE(num_pairs >= 0 && num_det >= 0 && num_gt >= 0 && num_iou >= 0 && max_gt_per_pair >= 0,
                "coco_match: negative count");
  FRCNN_REQUIRE(num_thr >= 1 && num_area >= 1 && (long long)num_thr * num_area <= (1 << 20),
                "coco_match: %d thresholds x %d area ranges", num_thr, num_area);
  if (num_pairs == 0) return FRCNN_OK;
  FRCNN_REQUIRE(det_offsets && gt_offsets && iou_offsets, "coco_match: null pair offsets");
  FRCNN_REQUIRE(iou_thrs && area_rng, "coco_match: null thresholds or area ranges");
  FRCNN_REQUIRE(num_det == 0 || (det && dt_match && dt_ignore), "coco_match: null detection array");
  FRCNN_REQUIRE(num_gt == 0 || (gt && gt_crowd && gt_ignore), "coco_match: null ground-truth array");
  FRCNN_REQUIRE(num_iou == 0 || ious, "coco_match: null overlap array");
  const size_t need = frcnn_coco_match_ws_bytes(num_gt, max_gt_per_pair, num_area, num_thr);
  if (need > 0 && (!ws || ws_bytes < need))
    return fail(FRCNN_ERR_WS, "coco_match: workspace of %zu bytes needed (a pair has %d > %d gt boxes), got %zu", need,
                max_gt_per_pair, COCO_MASK_GT, ws_bytes);
  CocoArgs a{det, det_offsets, num_det, gt, gt_crowd, gt_offsets, num_gt,
             reinterpret_cast<const long long*>(iou_offsets), (long long)num_iou, iou_thrs, num_thr, area_rng, num_area,
             num_pairs, ious, dt_match, dt_ignore, gt_ignore, need > 0 ? static_cast<uint8_t*>(ws) : nullptr};
  hipLaunchKernelGGL(frcnn_coco_match_kernel, dim3((num_pairs + COCO_WAVES - 1) / COCO_WAVES), dim3(COCO_THREADS), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("coco_match");
}
