// The steps of the per-class detection filter (lib/utils/filter_predictions.py:45-72 + the max_dets cut of
// lib/model/test.py:213-221), each written once: select, rank, greedy fixed point, positions, cut, write.  Used by the
// axis-aligned filters (class_filter.hip) and the rotated one (nms_rotated.hip); how the pairwise matrix is produced
// stays with each kernel.  Every function is called by the whole workgroup of THREADS threads and inlined, so the
// address space of each pointer (LDS or global) stays visible to the compiler - no flat loads.
#pragma once
#include "box_math.h"

namespace frcnn {

// inds = scores[:, cls] > thresh (filter_predictions.py:46) as unsorted (desc_key << 32 | roi) keys; returns their number
template <int THREADS>
__device__ __forceinline__ int select_class_keys(const float* __restrict__ cls_prob, int R, int num_classes, int cls,
                                                 float thresh, uint64_t* raw, int* s_n) {
  if (threadIdx.x == 0) *s_n = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += THREADS) {
    const float sc = cls_prob[(size_t)r * num_classes + cls];
    if (sc > thresh) raw[atomicAdd(s_n, 1)] = ((uint64_t)desc_key(sc) << 32) | (uint32_t)r;
  }
  __syncthreads();
  return *s_n;
}

// (score desc, roi index asc): the keys are unique, so the rank of one is the number of smaller keys; store(rank, key)
template <int THREADS, typename Store>
__device__ __forceinline__ void rank_sort_keys(const uint64_t* raw, int n, Store store) {
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const uint64_t mine = raw[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += raw[j] < mine ? 1 : 0;
    store(rank, mine);
  }
}

// Greedy NMS over boxes in descending-score order as the unique fixed point of  keep(j) <=> no kept predecessor in P[j],
// P[j * stride + w] = bits i < j of word w with IoU(i, j) over the threshold.  In every round an undecided box with a
// kept predecessor is removed, one whose predecessors are all removed is kept; both verdicts are final when made, so the
// sets may be read while other threads add to them.  Every round decides at least the first undecided box; a frame's
// boxes take a handful of rounds, against one serial step per kept box in a scan.  Thread t owns boxes t + q * THREADS,
// q < PER.  No mask on the diagonal word: every producer (the small kernel's `j > i`, rot_pair_kernel's `i < j`) sets
// bits i < j only.  P may be LDS or global: the forced inlining lets the compiler see which (through a call it would be
// a generic pointer, every row fetch a flat load).  Leaves the kept set in kept_set, rem_set free; no barrier at the end.
template <int THREADS, int PER, typename PPtr>
__device__ __forceinline__ void nms_fixed_point(PPtr P, int stride, int n, unsigned long long* kept_set,
                                                unsigned long long* rem_set) {
  const int t = threadIdx.x;
  for (int e = t; e < (n + 63) / 64; e += THREADS) kept_set[e] = rem_set[e] = 0ull;
  unsigned undecided = 0u;
#pragma unroll
  for (int q = 0; q < PER; ++q) undecided |= (t + q * THREADS < n) ? 1u << q : 0u;
  for (;;) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      if (!(undecided & (1u << q))) continue;
      const int j = t + q * THREADS;
      bool any_kept = false, all_removed = true;
      for (int w = 0; w <= (j >> 6); ++w) {                 // predecessors of box j live in words 0 .. j / 64
        const uint64_t pre = P[(size_t)j * stride + w];
        any_kept |= (pre & kept_set[w]) != 0ull;
        all_removed &= (pre & ~rem_set[w]) == 0ull;
      }
      if (any_kept) {
        atomicOr(&rem_set[j >> 6], 1ull << (j & 63));
        undecided &= ~(1u << q);
      } else if (all_removed) {
        atomicOr(&kept_set[j >> 6], 1ull << (j & 63));
        undecided &= ~(1u << q);
      }
    }
    if (__syncthreads_count(undecided != 0u ? 1 : 0) == 0) break;
  }
}

// position of every kept box among the kept ones (ascending box order) -> order[pos] = box; returns the kept count
template <int THREADS, int PER, typename OrderPtr>
__device__ __forceinline__ int kept_positions(const unsigned long long* kept_set, int n, OrderPtr order) {
  const int nbl = (n + 63) / 64;
  int total = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int j = threadIdx.x + q * THREADS;
    int before = 0;
    total = 0;
    uint64_t mine = 0ull;
    for (int w = 0; w < nbl; ++w) {
      const uint64_t kw = kept_set[w];
      const int pc = __builtin_popcountll(kw);
      if (w < (j >> 6)) before += pc;
      if (w == (j >> 6)) mine = kw;
      total += pc;
    }
    if (j < n && ((mine >> (j & 63)) & 1ull)) order[before + __builtin_popcountll(mine & ((1ull << (j & 63)) - 1ull))] = j;
  }
  __syncthreads();
  return total;
}

// test.py:213-221: if more than max_dets survive keep score >= the max_dets-th best (ties stay); returns the new count.
// keys[order[.]] ascend (= descending score), so the survivors are a prefix: the ties are counted in parallel into
// *s_ties, any LDS int the caller no longer needs (a bisection needs neither but was measured 0.3 us slower in the
// 300-RoI filter: a chain of dependent LDS reads).  `key <= cut key` IS the reference's `score >= cut score`: desc_key
// folds -0 into +0, is strictly monotone on the other non-NaN floats, and a NaN score never passed `sc > thresh`.
template <int THREADS, typename KeysPtr, typename OrderPtr>
__device__ __forceinline__ int cut_at_max_dets(KeysPtr keys, OrderPtr order, int kept, int max_dets, int* s_ties) {
  if (max_dets <= 0 || kept <= max_dets) return kept;
  const uint32_t cut = (uint32_t)(keys[order[max_dets - 1]] >> 32);     // ascending key = descending score
  if (threadIdx.x == 0) *s_ties = 0;
  __syncthreads();
  for (int m = max_dets + (int)threadIdx.x; m < kept; m += THREADS)
    if ((uint32_t)(keys[order[m]] >> 32) <= cut) atomicAdd(s_ties, 1);   // one LDS atomic per wave after aggregation
  __syncthreads();
  return max_dets + *s_ties;
}

// Rows of class cls: dets[cls][i] = [box (E floats), score] and det_roi[cls][i] = RoI of the i-th kept box, zeros / -1
// from `kept` (cut to max_out) on, det_count[cls].  One output element per thread: coalesced.
template <int E, int THREADS, typename KeysPtr, typename OrderPtr>
__device__ __forceinline__ void write_class_dets(const float* __restrict__ pred_boxes, const float* __restrict__ cls_prob,
                                                 int num_classes, int cls, KeysPtr keys, OrderPtr order, int kept,
                                                 int max_out, float* __restrict__ dets, int* __restrict__ det_count,
                                                 int* __restrict__ det_roi) {
  kept = min(kept, max_out);
  float* out = dets + (size_t)cls * max_out * (E + 1);
  for (int e = threadIdx.x; e < max_out * (E + 1); e += THREADS) {
    const int i = e / (E + 1), q = e - i * (E + 1);
    float v = 0.f;
    int roi = -1;
    if (i < kept) {
      const uint32_t r = (uint32_t)(keys[order[i]] & 0xFFFFFFFFu);
      v = q < E ? pred_boxes[((size_t)r * num_classes + cls) * E + q] : cls_prob[(size_t)r * num_classes + cls];
      roi = (int)r;
    }
    out[e] = v;
    if (det_roi && q == 0) det_roi[(size_t)cls * max_out + i] = roi;
  }
  if (threadIdx.x == 0) det_count[cls] = kept;
}

// Class 0 (background) never has detections (filter_predictions.py:45 loops over classes 1..K-1): block 0 of the filter
// kernels writes that class's slice of every output, so the callers need no zero-filled buffers.
template <int E, int THREADS>
__device__ __forceinline__ void fill_background(int max_out, float* __restrict__ dets, int* __restrict__ det_count,
                                                int* __restrict__ det_roi) {
  for (int e = threadIdx.x; e < max_out * (E + 1); e += THREADS) dets[e] = 0.f;
  if (det_roi)
    for (int e = threadIdx.x; e < max_out; e += THREADS) det_roi[e] = -1;
  if (threadIdx.x == 0) det_count[0] = 0;
}

}  // namespace frcnn
