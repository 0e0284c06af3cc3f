// Scoring of a detections file on the device: the overlap and matching loop the three reference evaluators share
// (lib/datasets/waymo_eval.py:131-213, kitti_eval.py:116-215, cadc_eval.py:115-206) for ONE class over the whole
// file, as one launch.  The host hands in the detections and the ground truth grouped by frame (CSR); each detection
// carries its ROW, its rank in the confidence order among detections that have a record (the reference's `idx`).
//
// One workgroup of 256 threads per frame (frames differ in size; the dispatcher hands a free compute unit the next
// frame, so nothing assumes equal work, and the largest frame is the tail):
//   1. best_row[j] = INT_MAX for the frame's gt boxes: in LDS up to EVAL_LDS_GT boxes, else in the caller's workspace.
//   2. Detections in tiles of 256 / L, L lanes per detection (L = the largest power of two <= 64 with n_det * L <= 256, so
//      a frame of 50 detections keeps 200 lanes busy).  The frame's gt boxes go through LDS in chunks of EVAL_CHUNK: ONE
//      thread per box computes corners, edge vectors, area and height range (eval_overlap.h box_geom), all lanes of the
//      tile then read them.  Lane s of a detection takes boxes s, s + L, ... of the chunk and keeps (max overlap, first
//      index); the L partial results are merged by wave shuffles with np.argmax's rule (a later equal overlap does not
//      replace an earlier one).  The don't-care boxes take the same path for their maximum alone.
//      A candidate (ovmax > ovthresh strictly, ovmax_dc < ovthresh_dc) of a non-ignored gt j does atomicMin(best_row[j], row).
//   3. After a barrier every detection reads its verdict: the candidate whose row is best_row[jmax] is the true positive,
//      every other candidate of that gt a duplicate false positive; a candidate of an ignored gt counts for nothing; a
//      non-candidate below the don't-care threshold in a frame that has gt is a false positive at every level.  This is
//      the reference's sequential walk: hit[j] is only ever set by a non-ignored candidate of j and rows are visited in
//      ascending order, so "hit[j] already set" == "a candidate of j with a smaller row exists".
//   4. hit[j] = best_row[j] != INT_MAX.
// The clipped polygon of the 'bev' / '3d' forms sits in a per-lane LDS column (2 slots x 8 vertices x 2 doubles, 64 KiB
// per workgroup): runtime-indexed appends without scratch memory.  With the 10 KiB of staged boxes and 8 KiB of best_row
// that is one workgroup per compute unit; the kernel is a chain of dependent float64 operations per pair and was not
// tuned further (profiles/device_eval.md).
// Compiled with -ffp-contract=off like every box-arithmetic unit.  Plain HIP, vector stores only.
#include "common.h"
#include "eval_overlap.h"

#include <climits>

using namespace frcnn;
using namespace frcnn_eval;

namespace {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_CHUNK = FRCNN_EVAL_CHUNK;      // gt boxes staged in LDS at a time
constexpr int EVAL_LDS_GT = FRCNN_EVAL_LDS_GT;    // gt boxes of a frame whose best_row fits in LDS

struct EvalArgs {
  const double* det_boxes; const int* det_rows; const int* det_offsets; int num_det;
  const double* gt_boxes; const uint8_t* gt_ignore; const int* gt_difficulty; const int* gt_offsets; int num_gt;
  const double* dc_boxes; const int* dc_offsets; int num_dc;
  double ovthresh, ovthresh_dc;
  int* code; int* jmax; double* ovmax; double* ovmax_dc; int* det_difficulty; uint8_t* hit;
  int* ws;                           // num_gt ints or nullptr
};

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (max overlap, first index attaining it) of detection `det` over boxes[begin, end), this lane taking every L-th box
// of each chunk; merged over the detection's L lanes.  Called by the whole workgroup (barriers inside).
template <int TYPE, int E>
__device__ inline void scan_boxes(const double* boxes, int begin, int end, const BoxGeom& det, bool active, int sub, int L,
                                  double (*stage)[EVAL_CHUNK], const Poly& pa, const Poly& pb, double& best, int& best_j) {
  best = -INFINITY;
  best_j = INT_MAX;
  for (int cs = begin; cs < end; cs += EVAL_CHUNK) {
    const int cn = min(EVAL_CHUNK, end - cs);
    __syncthreads();                                  // the previous chunk has been read by everyone
    if ((int)threadIdx.x < cn) {
      BoxGeom g;
      box_geom<TYPE>(boxes + (size_t)(cs + threadIdx.x) * E, g);
      const int t = threadIdx.x;
      stage[0][t] = g.cx[0]; stage[1][t] = g.cx[1]; stage[2][t] = g.cx[2]; stage[3][t] = g.cx[3];
      stage[16][t] = g.area;
      if (TYPE == EVAL_TYPE_BEV || TYPE == EVAL_TYPE_3D) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          stage[4 + k][t] = g.cy[k];
          stage[8 + k][t] = g.ex[k];
          stage[12 + k][t] = g.ey[k];
        }
      }
      if (TYPE == EVAL_TYPE_3D) {
        stage[17][t] = g.zlo; stage[18][t] = g.zhi; stage[19][t] = g.vol;
      }
    }
    __syncthreads();
    if (active) {
      for (int jj = sub; jj < cn; jj += L) {
        BoxGeom g;
        g.cx[0] = stage[0][jj]; g.cx[1] = stage[1][jj]; g.cx[2] = stage[2][jj]; g.cx[3] = stage[3][jj];
        g.area = stage[16][jj];
        if (TYPE == EVAL_TYPE_BEV || TYPE == EVAL_TYPE_3D) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            g.cy[k] = stage[4 + k][jj];
            g.ex[k] = stage[8 + k][jj];
            g.ey[k] = stage[12 + k][jj];
          }
        }
        if (TYPE == EVAL_TYPE_3D) {
          g.zlo = stage[17][jj]; g.zhi = stage[18][jj]; g.vol = stage[19][jj];
        }
        const double ov = pair_overlap<TYPE>(det, g, pa, pb);
        if (ov > best) {                              // ascending index within the lane: strict > keeps the first
          best = ov;
          best_j = cs - begin + jj;
        }
      }
    }
  }
  for (int m = L >> 1; m > 0; m >>= 1) {              // L <= 64 and a power of two: partners share a wave
    const double o = __shfl_xor(best, m, 64);
    const int oj = __shfl_xor(best_j, m, 64);
    if (o > best || (o == best && oj < best_j)) {
      best = o;
      best_j = oj;
    }
  }
}

template <int TYPE, int E>
__global__ __launch_bounds__(EVAL_THREADS) void frcnn_eval_match_kernel(EvalArgs a) {
  __shared__ double poly[2][2][EVAL_MAX_VERTS][EVAL_THREADS];   // [slot][x / y][vertex][lane]
  __shared__ double stage[EVAL_GEOM_DOUBLES][EVAL_CHUNK];
  __shared__ int best_row_lds[EVAL_LDS_GT];

  const int f = blockIdx.x, tid = threadIdx.x;
  const int d0 = clampi(a.det_offsets[f], 0, a.num_det), d1 = clampi(a.det_offsets[f + 1], d0, a.num_det);
  const int g0 = clampi(a.gt_offsets[f], 0, a.num_gt), g1 = clampi(a.gt_offsets[f + 1], g0, a.num_gt);
  const bool has_dc = a.dc_boxes != nullptr && a.dc_offsets != nullptr && a.num_dc > 0;
  const int c0 = has_dc ? clampi(a.dc_offsets[f], 0, a.num_dc) : 0;
  const int c1 = has_dc ? clampi(a.dc_offsets[f + 1], c0, a.num_dc) : 0;
  const int nd = d1 - d0, ng = g1 - g0;
  const bool in_lds = ng <= EVAL_LDS_GT;
  const bool served = in_lds || a.ws != nullptr;      // a frame beyond the LDS count needs the workspace
  int* best_row = a.ws + g0;                          // only dereferenced when !in_lds && served

  if (served)
    for (int j = tid; j < ng; j += EVAL_THREADS) {
      if (in_lds) best_row_lds[j] = INT_MAX;
      else __hip_atomic_store(best_row + j, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  __syncthreads();

  int L = 1;
  while (L < 64 && nd * (2 * L) <= EVAL_THREADS) L *= 2;
  const int tile = EVAL_THREADS / L, group = tid / L, sub = tid % L;
  const Poly pa{&poly[0][0][0][tid], &poly[0][1][0][tid], EVAL_THREADS};
  const Poly pb{&poly[1][0][0][tid], &poly[1][1][0][tid], EVAL_THREADS};

  if (served) {
    for (int tb = 0; tb < nd; tb += tile) {
      const int d = d0 + tb + group;
      const bool active = tb + group < nd;
      BoxGeom det;
      if (active) box_geom<TYPE>(a.det_boxes + (size_t)d * E, det);
      double ov, ov_dc;
      int j, j_dc;
      scan_boxes<TYPE, E>(a.gt_boxes, g0, g1, det, active, sub, L, stage, pa, pb, ov, j);
      scan_boxes<TYPE, E>(a.dc_boxes, c0, c1, det, active, sub, L, stage, pa, pb, ov_dc, j_dc);
      if (active && sub == 0) {
        if (j == INT_MAX) j = 0;                      // no gt: `ovmax, jmax = -np.inf, 0`
        if (c1 == c0) ov_dc = 0.0;                    // `ovmax_dc = 0`
        a.ovmax[d] = ov;
        a.jmax[d] = j;
        a.ovmax_dc[d] = ov_dc;
        if (ov > a.ovthresh && ov_dc < a.ovthresh_dc && !a.gt_ignore[g0 + j]) {
          if (in_lds) atomicMin(&best_row_lds[j], a.det_rows[d]);
          else atomicMin(best_row + j, a.det_rows[d]);
        }
      }
    }
  }
  __threadfence();                                    // the atomics have landed before anyone reads best_row
  __syncthreads();

  for (int tb = 0; tb < nd; tb += tile) {             // the same lane reads back what it wrote
    const int d = d0 + tb + group;
    if (tb + group < nd && sub == 0) {
      int code = served ? 0 : -1, dif = -1;
      if (served) {
        const double ov = a.ovmax[d], ov_dc = a.ovmax_dc[d];
        const int j = a.jmax[d];
        if (ov > a.ovthresh && ov_dc < a.ovthresh_dc) {
          if (!a.gt_ignore[g0 + j]) {
            const int first = in_lds ? best_row_lds[j]
                                     : __hip_atomic_load(best_row + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            code = first == a.det_rows[d] ? 1 : 2;
            dif = a.gt_difficulty[g0 + j];
          }
        } else if (ng > 0 && ov_dc < a.ovthresh_dc) {
          code = 3;
        }
      } else {
        a.ovmax[d] = -INFINITY;
        a.jmax[d] = 0;
        a.ovmax_dc[d] = 0.0;
      }
      a.code[d] = code;
      a.det_difficulty[d] = dif;
    }
  }
  for (int j = tid; j < ng; j += EVAL_THREADS) {
    int first = INT_MAX;
    if (served)
      first = in_lds ? best_row_lds[j] : __hip_atomic_load(best_row + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.hit[g0 + j] = first != INT_MAX;
  }
}

template <int TYPE, int E>
void launch(const EvalArgs& a, int num_frames, hipStream_t stream) {
  hipLaunchKernelGGL((frcnn_eval_match_kernel<TYPE, E>), dim3(num_frames), dim3(EVAL_THREADS), 0, stream, a);
}

}  // namespace

extern "C" size_t frcnn_eval_match_ws_bytes(int num_gt, int max_gt_per_frame) {
  if (num_gt <= 0 || max_gt_per_frame <= EVAL_LDS_GT) return 0;
  return (size_t)num_gt * sizeof(int);
}

extern "C" int frcnn_eval_match(const double* det_boxes, const int* det_rows, const int* det_offsets, int num_det,
                                const double* gt_boxes, const uint8_t* gt_ignore, const int* gt_difficulty,
                                const int* gt_offsets, int num_gt, const double* dc_boxes, const int* dc_offsets, int num_dc,
                                int num_frames, int eval_type, double ovthresh, double ovthresh_dc, int max_gt_per_frame,
                                int* code, int* jmax, double* ovmax, double* ovmax_dc, int* det_difficulty, uint8_t* hit,
                                void* ws, size_t ws_bytes, void* stream) {
  FRCNN_REQUIRE(num_frames >= 0 && num_det >= 0 && num_gt >= 0 && num_dc >= 0 && max_gt_per_frame >= 0,
                "eval_match: negative count");
  FRCNN_REQUIRE(eval_type >= EVAL_TYPE_2D && eval_type <= EVAL_TYPE_3D,
                "eval_match: eval_type %d (0 '2d', 1 'bev_aa', 2 'bev', 3 '3d')", eval_type);
  FRCNN_REQUIRE(ovthresh == ovthresh && ovthresh_dc == ovthresh_dc, "eval_match: NaN threshold");
  if (num_frames == 0) return FRCNN_OK;
  FRCNN_REQUIRE(det_offsets && gt_offsets, "eval_match: null frame offsets");
  FRCNN_REQUIRE(num_det == 0 || (det_boxes && det_rows && code && jmax && ovmax && ovmax_dc && det_difficulty),
                "eval_match: null detection array");
  FRCNN_REQUIRE(num_gt == 0 || (gt_boxes && gt_ignore && gt_difficulty && hit), "eval_match: null ground-truth array");
  FRCNN_REQUIRE(num_dc == 0 || !dc_boxes == !dc_offsets, "eval_match: don't-care boxes and offsets go together");
  const size_t need = frcnn_eval_match_ws_bytes(num_gt, max_gt_per_frame);
  if (need > 0 && (!ws || ws_bytes < need))
    return fail(FRCNN_ERR_WS, "eval_match: workspace of %zu bytes needed (a frame has %d > %d gt boxes), got %zu", need,
                max_gt_per_frame, EVAL_LDS_GT, ws_bytes);
  EvalArgs a{det_boxes, det_rows, det_offsets, num_det, gt_boxes, gt_ignore, gt_difficulty, gt_offsets, num_gt,
             dc_boxes, dc_offsets, num_dc, ovthresh, ovthresh_dc, code, jmax, ovmax, ovmax_dc, det_difficulty, hit,
             need > 0 ? static_cast<int*>(ws) : nullptr};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (eval_type) {
    case EVAL_TYPE_2D: launch<EVAL_TYPE_2D, 4>(a, num_frames, s); break;
    case EVAL_TYPE_BEV_AA: launch<EVAL_TYPE_BEV_AA, 7>(a, num_frames, s); break;
    case EVAL_TYPE_BEV: launch<EVAL_TYPE_BEV, 7>(a, num_frames, s); break;
    default: launch<EVAL_TYPE_3D, 7>(a, num_frames, s); break;
  }
  return check_launch("eval_match");
}
