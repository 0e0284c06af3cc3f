// RPN top-k sort (frcnn_sort_topk_desc): one workgroup in LDS, or several workgroups for large n.  Built with
// -ffp-contract=off like every user of box_math.h.
#include "box_math.h"

#include <algorithm>

using namespace frcnn;

namespace {

// ------------------------------------------------------------------------------------------------
// Top-k of n scores in the total order (score desc, index asc), one 1024-thread workgroup:
//   1. 4-pass 8-bit radix select of the top_n-th key (LDS histogram),
//   2. compaction of keys < kth (any order) and of the lowest-index ties == kth (ordered scan),
//   3. bitonic sort of the <= 16384 u64 (key<<32 | index) candidates in LDS.
// ------------------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 1024;

__global__ __launch_bounds__(SORT_THREADS) void sort_topk_desc_kernel(const float* __restrict__ scores, int n,
                                                                      int top_n, int npad,
                                                                      int64_t* __restrict__ order_out,
                                                                      float* __restrict__ scores_out,
                                                                      int* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(sort_smem);             // [npad]
  uint32_t* hist = reinterpret_cast<uint32_t*>(keys + npad);           // [256]
  uint32_t* scan = hist + 256;                                         // [SORT_THREADS]
  __shared__ uint32_t s_prefix, s_need, s_fill;
  const int t = threadIdx.x;
  const int take = min(n, top_n);

  for (int i = t; i < npad; i += SORT_THREADS) keys[i] = ~0ull;
  if (t == 0) { s_prefix = 0; s_need = (uint32_t)take; s_fill = 0; }
  __syncthreads();

  uint32_t kth = 0xFFFFFFFFu;  // every key <= kth is a candidate when n <= top_n
  uint32_t need_eq = 0;        // how many keys == kth to take (lowest indices first)
  if (n > top_n) {
    // radix select: after the loop s_prefix = kth key, s_need = rank of kth among keys with that value
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = t; i < 256; i += SORT_THREADS) hist[i] = 0;
      __syncthreads();
      const uint32_t prefix = s_prefix;
      const uint32_t himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
      for (int i = t; i < n; i += SORT_THREADS) {
        const uint32_t k = desc_key(scores[i]);
        if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (t == 0) {
        uint32_t need = s_need, acc = 0;
        int b = 0;
        for (; b < 256; ++b) {
          if (acc + hist[b] >= need) break;
          acc += hist[b];
        }
        s_prefix = prefix | ((uint32_t)b << shift);
        s_need = need - acc;
      }
      __syncthreads();
    }
    kth = s_prefix;
    need_eq = s_need;
  }
  __syncthreads();

  // compaction.  Thread t owns the contiguous index range [lo, hi) so ties are taken in index order.
  const int per = (n + SORT_THREADS - 1) / SORT_THREADS;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  uint32_t my_eq = 0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t k = desc_key(scores[i]);
    if (k < kth || (n <= top_n)) {
      const uint32_t pos = atomicAdd(&s_fill, 1u);
      keys[pos] = ((uint64_t)k << 32) | (uint32_t)i;
    } else if (k == kth) {
      ++my_eq;
    }
  }
  scan[t] = my_eq;
  __syncthreads();
  if (n > top_n) {
    // exclusive scan of tie counts (Hillis-Steele in LDS)
    for (int off = 1; off < SORT_THREADS; off <<= 1) {
      const uint32_t v = t >= off ? scan[t - off] : 0u;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    uint32_t rank = scan[t] - my_eq;  // ties before this thread's range
    const uint32_t base = (uint32_t)take - need_eq;  // number of keys < kth
    for (int i = lo; i < hi && rank < need_eq; ++i) {
      const uint32_t k = desc_key(scores[i]);
      if (k == kth) {
        keys[base + rank] = ((uint64_t)k << 32) | (uint32_t)i;
        ++rank;
      }
    }
  }
  __syncthreads();

  block_bitonic_sort(keys, npad);

  for (int i = t; i < take; i += SORT_THREADS) {
    const uint32_t idx = (uint32_t)(keys[i] & 0xFFFFFFFFu);
    order_out[i] = (int64_t)idx;
    scores_out[i] = scores[idx];
  }
  if (t == 0) count_out[0] = take;
}

// ------------------------------------------------------------------------------------------------
// Multi-workgroup form of the same top-k for large n (10^5 .. 10^6 scores: FPN / training RPN).  Same total
// order and the same result as the single-workgroup kernel:
//   3 x { topk_hist_kernel (all CUs: 11/11/10-bit digit histogram of the keys that still match the prefix)
//         topk_pick_kernel (one wave: bucket holding the top_n-th key -> extends the prefix) }
//   topk_count_eq_kernel  per-workgroup count of keys == kth over a contiguous index range
//   topk_compact_kernel   keys < kth (any slot) and the first need_eq ties (ordered slots: ties are taken lowest index
//                         first, each workgroup adds up the counts of the workgroups before it) -> u64 candidates
//   topk_rank_sort_kernel   every CU ranks 32 candidates against all <= 16384 of them; outputs in the canonical order
// ------------------------------------------------------------------------------------------------
constexpr int TOPK_BINS = 2048;
constexpr int TOPK_BLOCK_ITEMS = 4096;  // scores per workgroup (256 threads x 16)

struct TopkState {   // lives at the start of the workspace
  uint32_t prefix;   // digits of the kth key decided so far (high bits)
  uint32_t need;     // rank still to resolve inside the current prefix
  uint32_t fill;     // slots handed out to keys < kth
  uint32_t pad;
  uint32_t hist[TOPK_BINS];
};

__device__ __forceinline__ void topk_pass_bits(int pass, int& shift, int& bits) {
  shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
  bits = pass == 2 ? 10 : 11;
}

__global__ __launch_bounds__(256) void topk_init_kernel(TopkState* st, int take) {
  for (int i = threadIdx.x; i < TOPK_BINS; i += 256) st->hist[i] = 0;
  if (threadIdx.x == 0) { st->prefix = 0; st->need = (uint32_t)take; st->fill = 0; st->pad = 0; }
}

__global__ __launch_bounds__(256) void topk_hist_kernel(const float* __restrict__ scores, int n, int pass,
                                                       TopkState* __restrict__ st) {
  __shared__ uint32_t h[TOPK_BINS];
  for (int i = threadIdx.x; i < TOPK_BINS; i += 256) h[i] = 0;
  __syncthreads();
  int shift, bits;
  topk_pass_bits(pass, shift, bits);
  const uint32_t prefix = st->prefix;
  const uint32_t himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + bits));
  const int lo = blockIdx.x * TOPK_BLOCK_ITEMS, hi = min(lo + TOPK_BLOCK_ITEMS, n);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const uint32_t k = desc_key(scores[i]);
    if ((k & himask) == prefix) atomicAdd(&h[(k >> shift) & ((1u << bits) - 1u)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TOPK_BINS; i += 256)
    if (h[i]) atomicAdd(&st->hist[i], h[i]);
}

__global__ __launch_bounds__(64) void topk_pick_kernel(TopkState* __restrict__ st, int pass) {
  // one wave: lane l owns bins [32l, 32l+32); exclusive prefix over the lanes via shuffles, then the lane that
  // contains the target rank walks its 32 bins
  int shift, bits;
  topk_pass_bits(pass, shift, bits);
  const int lane = threadIdx.x;
  uint32_t mine = 0;
  for (int b = 0; b < 32; ++b) mine += st->hist[lane * 32 + b];
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const uint32_t excl = incl - mine, need = st->need;
  uint32_t new_prefix = 0, new_need = 0;
  const bool owner = need > excl && need <= incl;
  if (owner) {
    uint32_t acc = excl;
    int b = 0;
    for (; b < 32; ++b) {
      const uint32_t c = st->hist[lane * 32 + b];
      if (acc + c >= need) break;
      acc += c;
    }
    new_prefix = st->prefix | ((uint32_t)(lane * 32 + b) << shift);
    new_need = need - acc;
  }
  __syncthreads();   // single wave: orders the reads of hist above against the clears below
  for (int b = 0; b < 32; ++b) st->hist[lane * 32 + b] = 0;
  if (owner) { st->prefix = new_prefix; st->need = new_need; }
}

__global__ __launch_bounds__(256) void topk_count_eq_kernel(const float* __restrict__ scores, int n,
                                                           const TopkState* __restrict__ st,
                                                           uint32_t* __restrict__ block_eq) {
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t kth = st->prefix;
  const int lo = blockIdx.x * TOPK_BLOCK_ITEMS, hi = min(lo + TOPK_BLOCK_ITEMS, n);
  uint32_t c = 0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) c += desc_key(scores[i]) == kth ? 1u : 0u;
  if (c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) block_eq[blockIdx.x] = s_cnt;
}

__global__ __launch_bounds__(256) void topk_compact_kernel(const float* __restrict__ scores, int n, int take,
                                                          TopkState* __restrict__ st,
                                                          const uint32_t* __restrict__ block_eq,
                                                          uint64_t* __restrict__ cand) {
  // thread t owns the contiguous range [lo + 16t, lo + 16t + 16): ties stay in index order.  Slots for the keys < kth
  // are handed out per WORKGROUP (one global atomic each, after a block scan of the per-thread counts) - one atomic per
  // key on a single address was 10 of this kernel's 16 us.
  __shared__ uint32_t scan_lt[256], scan_eq[256];
  __shared__ uint32_t s_before, s_base;
  const uint32_t kth = st->prefix, need_eq = st->need;
  const uint32_t base_eq = (uint32_t)take - need_eq;   // number of keys < kth
  const int lo = blockIdx.x * TOPK_BLOCK_ITEMS + threadIdx.x * 16;
  const int hi = min(lo + 16, min((blockIdx.x + 1) * TOPK_BLOCK_ITEMS, n));
  uint32_t key[16];
  uint32_t my_lt = 0, my_eq = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = lo + q;
    key[q] = i < hi ? desc_key(scores[i]) : 0xFFFFFFFFu;
    if (i < hi) {
      my_lt += key[q] < kth ? 1u : 0u;
      my_eq += key[q] == kth ? 1u : 0u;
    }
  }
  scan_lt[threadIdx.x] = my_lt;
  scan_eq[threadIdx.x] = my_eq;
  if (threadIdx.x == 0) s_before = 0;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t v = threadIdx.x >= off ? scan_lt[threadIdx.x - off] : 0u;
    const uint32_t w = threadIdx.x >= off ? scan_eq[threadIdx.x - off] : 0u;
    __syncthreads();
    scan_lt[threadIdx.x] += v;
    scan_eq[threadIdx.x] += w;
    __syncthreads();
  }
  // ties before this workgroup's range: sum of the earlier workgroups' counts (<= 256 of them; a separate one-workgroup
  // scan kernel did this before, 4.4 us of launch for a handful of adds)
  {
    uint32_t part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) part += block_eq[b];
    if (part) atomicAdd(&s_before, part);
  }
  if (threadIdx.x == 255) s_base = scan_lt[255] ? atomicAdd(&st->fill, scan_lt[255]) : 0u;
  __syncthreads();
  uint32_t pos = s_base + scan_lt[threadIdx.x] - my_lt;
  uint32_t rank = s_before + scan_eq[threadIdx.x] - my_eq;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = lo + q;
    if (i >= hi) break;
    if (key[q] < kth) {
      cand[pos++] = ((uint64_t)key[q] << 32) | (uint32_t)i;
    } else if (key[q] == kth && rank < need_eq) {
      cand[base_eq + rank] = ((uint64_t)key[q] << 32) | (uint32_t)i;
      ++rank;
    }
  }
}

// Final ordering of the <= 16384 selected candidates by RANK: keys are unique (the index is in the low word), so the
// position of a key in the sorted order is the number of candidates smaller than it.  One workgroup ranks 32 keys:
// thread (key k, partition p) counts the keys of partition p below key k against an LDS copy of all candidates
// (32 lanes read the same LDS word: broadcast), the 32 partial counts of a key are summed, and the key is scattered to
// its rank.  6000 candidates: 188 workgroups of 1024 threads, one round on the chip, 188 compares per thread: 12.7 us
// (16 keys x 16 partitions: 375 workgroups in two rounds, 26 us; the round-1 bitonic network in ONE workgroup: 78 us).
constexpr int RANK_KEYS = 32, RANK_PARTS = 32;
__global__ __launch_bounds__(RANK_KEYS * RANK_PARTS) void topk_rank_sort_kernel(const float* __restrict__ scores,
                                                                              const uint64_t* __restrict__ cand, int take,
                                                                              int64_t* __restrict__ order_out,
                                                                              float* __restrict__ scores_out,
                                                                              int* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(sort_smem);          // [take]
  __shared__ uint32_t part[RANK_PARTS][RANK_KEYS];
  for (int i = threadIdx.x; i < take; i += blockDim.x) keys[i] = cand[i];
  __syncthreads();
  const int k = threadIdx.x & (RANK_KEYS - 1), p = threadIdx.x / RANK_KEYS;
  const int ki = blockIdx.x * RANK_KEYS + k;
  const uint64_t mine = ki < take ? keys[ki] : 0ull;
  const int per = (take + RANK_PARTS - 1) / RANK_PARTS;
  const int lo = min(p * per, take), hi = min(lo + per, take);
  uint32_t below = 0;
  for (int j = lo; j < hi; ++j) below += keys[j] < mine ? 1u : 0u;
  part[p][k] = below;
  __syncthreads();
  if (p == 0 && ki < take) {
    uint32_t rank = 0;
#pragma unroll
    for (int q = 0; q < RANK_PARTS; ++q) rank += part[q][k];
    const uint32_t idx = (uint32_t)(mine & 0xFFFFFFFFu);
    order_out[rank] = (int64_t)idx;
    scores_out[rank] = scores[idx];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) count_out[0] = take;
}

}  // namespace

constexpr int TOPK_MULTI_MIN_N = 16384;   // below this one workgroup does everything in LDS

static size_t topk_multi_layout(int n, size_t* off_blocks, size_t* off_cand) {
  const size_t nblocks = ((size_t)n + TOPK_BLOCK_ITEMS - 1) / TOPK_BLOCK_ITEMS;
  size_t o = align_up(sizeof(TopkState), 256);
  *off_blocks = o;
  o = align_up(o + nblocks * sizeof(uint32_t), 256);
  *off_cand = o;
  return o + (size_t)16384 * sizeof(uint64_t);
}

extern "C" size_t frcnn_sort_topk_desc_ws_bytes(int n, int top_n) {
  if (n <= TOPK_MULTI_MIN_N || n <= top_n) return 0;   // everything lives in LDS
  size_t a, b;
  return topk_multi_layout(n, &a, &b);
}

extern "C" int frcnn_sort_topk_desc(const float* scores, int n, int top_n, int64_t* order_out, float* scores_out,
                                    int* count_out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(scores && order_out && scores_out && count_out && n > 0 && top_n > 0, "sort_topk_desc: bad arguments");
  FRCNN_REQUIRE(top_n <= 16384, "sort_topk_desc: top_n %d > 16384", top_n);
  const int take = std::min(n, top_n);
  const int npad = next_pow2(std::max(take, 2));
  if (n > TOPK_MULTI_MIN_N && n > top_n) {
    size_t off_blocks, off_cand;
    const size_t need = topk_multi_layout(n, &off_blocks, &off_cand);
    if (!ws || ws_bytes < need) return fail(FRCNN_ERR_WS, "sort_topk_desc: workspace %zu < %zu bytes", ws_bytes, need);
    char* base = static_cast<char*>(ws);
    TopkState* st = reinterpret_cast<TopkState*>(base);
    uint32_t* block_eq = reinterpret_cast<uint32_t*>(base + off_blocks);
    uint64_t* cand = reinterpret_cast<uint64_t*>(base + off_cand);
    const int nblocks = (n + TOPK_BLOCK_ITEMS - 1) / TOPK_BLOCK_ITEMS;
    hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(256), 0, stream, st, take);
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(topk_hist_kernel, dim3(nblocks), dim3(256), 0, stream, scores, n, pass, st);
      hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(64), 0, stream, st, pass);
    }
    hipLaunchKernelGGL(topk_count_eq_kernel, dim3(nblocks), dim3(256), 0, stream, scores, n, st, block_eq);
    hipLaunchKernelGGL(topk_compact_kernel, dim3(nblocks), dim3(256), 0, stream, scores, n, take, st, block_eq, cand);
    int rc = check_launch("topk multi-workgroup select");
    if (rc != FRCNN_OK) return rc;
    const size_t lds = (size_t)take * 8;
    rc = ensure_dynamic_lds<&topk_rank_sort_kernel>(lds, "sort_topk_desc");
    if (rc != FRCNN_OK) return rc;
    hipLaunchKernelGGL(topk_rank_sort_kernel, dim3((take + RANK_KEYS - 1) / RANK_KEYS), dim3(RANK_KEYS * RANK_PARTS), lds,
                       stream, scores, cand, take, order_out, scores_out, count_out);
    return check_launch("topk_rank_sort_kernel");
  }
  const size_t lds = (size_t)npad * 8 + 256 * 4 + SORT_THREADS * 4;
  const int rc = ensure_dynamic_lds<&sort_topk_desc_kernel>(lds, "sort_topk_desc");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(sort_topk_desc_kernel, dim3(1), dim3(SORT_THREADS), lds, stream, scores, n, top_n, npad, order_out,
                     scores_out, count_out);
  return check_launch("sort_topk_desc_kernel");
}
