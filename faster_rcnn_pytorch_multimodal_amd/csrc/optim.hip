// The solver's weight update (lib/model/train_val.py:207-208 torch.optim.SGD with momentum, :379-382 the step that ends a
// pseudo batch) for ALL trainable parameters of a network in one launch: per-element gradient clip, weight decay,
// momentum, step and (optionally) the clearing of the gradient, in one pass over the flat gradient buffer
// (model/train_val.GradientBucket).  Per element, torch's operations in torch's order, one rounding each (compiled with
// -ffp-contract=off: no fma):
//     g = clamp(g, -clip, +clip)       torch.clamp_: a NaN gradient stays NaN, -0.0 stays -0.0
//     d = g + wd * p                   skipped when wd == 0
//     b = b * momentum + d
//     p = p + (-lr) * b
//     g = +0.0                         only with zero_grads; otherwise the clipped gradient is left in place
//
// Work split: a parameter is a SEGMENT (pointer, offset into the flat buffers, element count, lr, wd - one 32-byte row of
// a device table); segments are cut into chunks of FRCNN_SGD_CHUNK elements and one workgroup owns one chunk (device
// table of (segment, chunk index) pairs, built once by the caller), so every kernel argument is a pointer or a
// launch-invariant scalar and the learning rates can change without a new capture.
//
// Access width: the flat offset of a segment is an arbitrary sum of element counts, so gradient / momentum on one side
// and the parameter on the other can be misaligned against each other by one to three floats.  A chunk is walked as
//     head (0..3 elements, until the GRADIENT address is 16-byte aligned), body (groups of 4), tail (0..3 elements).
// The body moves 16 bytes per lane on all streams: the gradient (and the momentum buffer, which shares the offset)
// at 16-byte aligned addresses, the parameter at whatever alignment is left (a dword-aligned 16-byte access; the
// hardware takes those, see DESIGN.md section 4.17 for the instructions the compiler emits).  The gradient side is the
// one that is aligned because it carries four of the six streams (g read, g clear, b read, b write).
// Purely bandwidth-bound: 5 streams over the parameter count, 6 with the clearing store.
#include "common.h"

#include <cmath>

using namespace frcnn;

namespace {

constexpr int CHUNK = FRCNN_SGD_CHUNK;
constexpr int THREADS = 256;
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of 16-byte groups per thread");
static_assert(sizeof(frcnn_sgd_segment) == 32, "segment rows are 32 bytes");

typedef float vec4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) vec4_dword_aligned { vec4 v; };     // 16 bytes at dword alignment

struct Scalars {
  float momentum, clip;
  int do_clip, zero_grads;
};

__device__ __forceinline__ void update_one(float& p, float& g, float& b, float lr_neg, float wd, const Scalars& s) {
  if (s.do_clip) {                     // comparisons are false for NaN: it passes through, as in torch.clamp_
    g = g < -s.clip ? -s.clip : g;
    g = g > s.clip ? s.clip : g;
  }
  float d = g;
  if (wd != 0.f) d = g + wd * p;
  b = b * s.momentum + d;
  p = p + lr_neg * b;
  if (s.zero_grads) g = 0.f;
}

// the parameter pointer comes out of the segment table: say that it is global memory (global_* instead of flat_* accesses)
#define FRCNN_GLOBAL __attribute__((address_space(1)))
typedef FRCNN_GLOBAL float* gfloat_p;
typedef FRCNN_GLOBAL vec4_dword_aligned* gvec4_dword_aligned_p;

__device__ __forceinline__ void update_scalar(gfloat_p __restrict__ p, float* __restrict__ g, float* __restrict__ b, float lr_neg,
                                              float wd, const Scalars& s) {
  float pv = *p, gv = *g, bv = *b;
  update_one(pv, gv, bv, lr_neg, wd, s);
  *p = pv; *g = gv; *b = bv;
}

__global__ __launch_bounds__(THREADS) void sgd_update_kernel(float* __restrict__ grad, float* __restrict__ mom,
                                                             const frcnn_sgd_segment* __restrict__ segs, int num_segs,
                                                             const int2* __restrict__ chunks, Scalars s) {
  const int2 c = chunks[blockIdx.x];
  if (c.x < 0 || c.x >= num_segs || c.y < 0) return;
  const frcnn_sgd_segment seg = segs[c.x];
  const long long start = (long long)c.y * CHUNK;
  if (start >= seg.count) return;
  const int n = (int)min((long long)CHUNK, seg.count - start);
  gfloat_p __restrict__ p = (gfloat_p)seg.param + start;
  float* __restrict__ g = grad + seg.offset + start;
  float* __restrict__ b = mom + seg.offset + start;
  const float lr_neg = -seg.lr, wd = seg.weight_decay;

  const int head = min(n, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(g) >> 2) & 3u)) & 3u));
  const int groups = (n - head) >> 2;
  const int tail0 = head + groups * 4, tail = n - tail0;
  const int t = threadIdx.x;
  if (t < head) update_scalar(p + t, g + t, b + t, lr_neg, wd, s);
  if (t < tail) update_scalar(p + tail0 + t, g + tail0 + t, b + tail0 + t, lr_neg, wd, s);

#pragma unroll
  for (int k = 0; k < CHUNK / (4 * THREADS); ++k) {
    const int v = k * THREADS + t;
    if (v >= groups) break;
    const int e = head + v * 4;
    vec4* gp = reinterpret_cast<vec4*>(g + e);                                     // 16-byte aligned by the head
    vec4_dword_aligned* bp = reinterpret_cast<vec4_dword_aligned*>(b + e);         // same offset as g: aligned in practice
    gvec4_dword_aligned_p pp = (gvec4_dword_aligned_p)(p + e);
    vec4 gv = *gp, bv = bp->v, pv = pp->v;
    float ga[4] = {gv.x, gv.y, gv.z, gv.w}, ba[4] = {bv.x, bv.y, bv.z, bv.w}, pa[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) update_one(pa[j], ga[j], ba[j], lr_neg, wd, s);
    pv.x = pa[0]; pv.y = pa[1]; pv.z = pa[2]; pv.w = pa[3];
    bv.x = ba[0]; bv.y = ba[1]; bv.z = ba[2]; bv.w = ba[3];
    gv.x = ga[0]; gv.y = ga[1]; gv.z = ga[2]; gv.w = ga[3];
    pp->v = pv;
    bp->v = bv;
    if (s.do_clip || s.zero_grads) *gp = gv;                                       // otherwise the gradient is unchanged
  }
}

}  // namespace

extern "C" int frcnn_sgd_update(float* grad_flat, float* momentum_flat, int64_t flat_elems,
                                const frcnn_sgd_segment* segments_dev, const frcnn_sgd_segment* segments_host,
                                int num_segments, const int* chunks_dev, int64_t num_chunks, float momentum, float clip,
                                int zero_grads, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(num_segments >= 0, "sgd_update: negative segment count %d", num_segments);
  FRCNN_REQUIRE(flat_elems >= 0, "sgd_update: negative flat buffer size %lld", (long long)flat_elems);
  FRCNN_REQUIRE(num_chunks >= 0, "sgd_update: negative chunk count %lld", (long long)num_chunks);
  FRCNN_REQUIRE(zero_grads == 0 || zero_grads == 1, "sgd_update: zero_grads is 0 or 1");
  FRCNN_REQUIRE(!std::isnan(momentum) && !std::isnan(clip), "sgd_update: momentum / clip is NaN");
  if (num_segments == 0) {
    FRCNN_REQUIRE(num_chunks == 0, "sgd_update: %lld chunks for zero segments", (long long)num_chunks);
    return FRCNN_OK;
  }
  FRCNN_REQUIRE(grad_flat && momentum_flat, "sgd_update: null argument (grad_flat / momentum_flat)");
  FRCNN_REQUIRE(segments_dev && segments_host, "sgd_update: null argument (segment table, device / host copy)");
  FRCNN_REQUIRE(grad_flat + flat_elems <= momentum_flat || momentum_flat + flat_elems <= grad_flat,
                "sgd_update: grad_flat and momentum_flat overlap");
  FRCNN_REQUIRE(((reinterpret_cast<uintptr_t>(grad_flat) | reinterpret_cast<uintptr_t>(momentum_flat)) & 3) == 0,
                "sgd_update: flat buffers must be float aligned");
  long long want_chunks = 0;
  for (int i = 0; i < num_segments; ++i) {
    const frcnn_sgd_segment& sg = segments_host[i];
    FRCNN_REQUIRE(sg.param, "sgd_update: null argument (parameter pointer of segment %d)", i);
    FRCNN_REQUIRE((reinterpret_cast<uintptr_t>(sg.param) & 3) == 0, "sgd_update: segment %d: parameter is not float aligned", i);
    FRCNN_REQUIRE(sg.count >= 0 && sg.offset >= 0, "sgd_update: segment %d: negative count %lld / offset %lld", i,
                  (long long)sg.count, (long long)sg.offset);
    FRCNN_REQUIRE(sg.count <= flat_elems && sg.offset <= flat_elems - sg.count,
                  "sgd_update: segment %d (offset %lld, %lld elements) reaches past the flat buffer (%lld elements)", i,
                  (long long)sg.offset, (long long)sg.count, (long long)flat_elems);
    want_chunks += (sg.count + CHUNK - 1) / CHUNK;
  }
  FRCNN_REQUIRE(num_chunks == want_chunks, "sgd_update: %lld chunks given, the segments make %lld of %d elements",
                (long long)num_chunks, want_chunks, CHUNK);
  if (num_chunks == 0) return FRCNN_OK;                                 // only empty segments
  FRCNN_REQUIRE(chunks_dev, "sgd_update: null argument (chunk table)");
  FRCNN_REQUIRE(num_chunks <= 0x7fffffffll, "sgd_update: too many chunks (%lld)", (long long)num_chunks);
  Scalars s;
  s.momentum = momentum;
  s.clip = clip;
  s.do_clip = (clip > 0.f && !std::isinf(clip)) ? 1 : 0;
  s.zero_grads = zero_grads;
  hipLaunchKernelGGL(sgd_update_kernel, dim3((unsigned)num_chunks), dim3(THREADS), 0, stream, grad_flat, momentum_flat,
                     segments_dev, num_segments, reinterpret_cast<const int2*>(chunks_dev), s);
  return check_launch("sgd_update kernel");
}
