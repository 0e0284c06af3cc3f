/*
 * frcnn_hip.h — C ABI of libfrcnn_hip.so, the gfx950 (MI355X) HIP library behind the
 * Faster R-CNN hot path of mathild7/faster_rcnn_pytorch_multimodal.
 *
 * The reference has no FFI of its own (it is 100 % Python on torch / torchvision); each entry
 * point below names the reference call it replaces (path:line under the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch allocates), unless marked host;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), makes no allocation and
 *     no host synchronisation, so a whole frame can be captured in one hipGraph;
 *   - activations are NHWC fp32, filters are KRSC fp32 (K = output channels), both with C % 4 == 0;
 *   - scratch memory comes from the caller: `*_ws_bytes()` says how much `(ws, ws_bytes)` must hold;
 *   - return value 0 = ok, negative = error (frcnn_last_error() gives the message of the calling
 *     thread's last failure). Counts produced on the device (NMS survivors ...) stay on the device.
 */
#ifndef FRCNN_HIP_H_
#define FRCNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_OK 0
#define FRCNN_ERR_ARG (-1)     /* bad shape / null pointer / unsupported configuration */
#define FRCNN_ERR_WS (-2)      /* workspace too small */
#define FRCNN_ERR_LAUNCH (-3)  /* hipLaunch / runtime error */

/* Library version (major*10000 + minor*100 + patch) and last error text of this thread. */
int frcnn_version(void);
/* How the library initialises / copies device memory inside its launch sequences: 0 (default) = its own fill / copy
 * KERNELS, so that a stream capture of any entry point holds kernel nodes only; 1 = hipMemsetAsync / hipMemcpyAsync
 * (memset / memcpy graph nodes).  See DESIGN.md section 4.8 for why the default is 0.  Process-wide, read at call time. */
int frcnn_set_memops_mode(int mode);
int frcnn_get_memops_mode(void);
/* Hash of the CURRENT VALUES of every process-wide switch that selects kernels (frcnn_set_memops_mode, frcnn_conv2d_set_tile /
 * _set_algo / _set_staging / frcnn_conv2d_bf16_set_tile, frcnn_roi_align_set_variant, frcnn_filter_set_variant,
 * frcnn_nms_set_suppress_at_equal; a bf16 tile mode of 0 leaves the hash as it was without that switch): a caller
 * that holds captured hipGraphs of entry points of this library (the reference's per-frame loop lib/model/test.py:183-228
 * replayed by model/frame_graph.FramePool) keys its captures by it - another value means the captures describe other kernels. */
unsigned frcnn_settings_signature(void);
const char* frcnn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Dense backbone: conv + folded BN + residual + ReLU  (lib/nets/resnet.py:98-127 Bottleneck.forward,
 * :24-32 conv3x3/conv1x1, :152-156 stem; lib/nets/fpn.py:33-39 lateral/smoothing convs; RPN convs of
 * the missing lib/nets/network.py).  Implicit GEMM on v_mfma_f32_32x32x2_f32:
 *     y[n,ho,wo,k] = act( (sum_{r,s,c} x[n,ho*stride-pad+r,wo*stride-pad+s,c] * w[k,r,s,c]) * scale[k]
 *                          + shift[k] + residual[n,ho,wo,k] )
 * scale/shift/residual may be NULL (1, 0, 0). relu != 0 applies max(.,0).
 * split_k == 0 lets the library choose; >= 1 forces that many K splits (partials go through ws).
 * ------------------------------------------------------------------------------------------- */
size_t frcnn_conv2d_fwd_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad,
                                 int split_k);
int frcnn_conv2d_fwd(const float* x, const float* wgt, const float* scale, const float* shift,
                     const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s,
                     int stride, int pad, int relu, int split_k, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution backward (autograd of the same nn.Conv2d call sites; lib/model/train_val.py:458 train_step ->
 * loss.backward()).  Gradients w.r.t. the folded-BN scale/shift are not produced: BatchNorm is frozen on
 * this path (lib/nets/imagenet.py:110-116).
 *
 * frcnn_conv2d_transpose_filter: w (K,R,S,C) -> w_t (C,R,S,K) with the taps flipped, the filter of the
 *   data-gradient convolution (prepare once per weight version).
 * frcnn_conv2d_bwd_data: dx (n,h,w,c) = conv_transpose(dy (n,ho,wo,k), w) [+ add (n,h,w,c), may be NULL].
 *   n,h,w,c,k,r,s,stride,pad describe the FORWARD convolution.  Needs k % 4 == 0, r == s, pad <= r-1.
 * frcnn_conv2d_bwd_weight: dw (K,R,S,C) = sum_pixels dy x patch(x); db (K) = sum_pixels dy (db may be NULL).
 * ------------------------------------------------------------------------------------------- */
int frcnn_conv2d_transpose_filter(const float* w_krsc, float* w_crsk_flipped, int k, int r, int s, int c,
                                  void* stream);
size_t frcnn_conv2d_bwd_data_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
int frcnn_conv2d_bwd_data(const float* dy, const float* w_crsk_flipped, const float* add, float* dx, int n, int h,
                          int w, int c, int k, int r, int s, int stride, int pad, void* ws, size_t ws_bytes,
                          void* stream);
/* frcnn_conv2d_bwd_data with the Winograd transform of the data-gradient filter supplied by the caller: w_winograd =
 * frcnn_conv2d_winograd_filter(w_crsk_flipped viewed as a (c,3,3,k) filter), (16,c,k), or NULL.  The weights change once per
 * optimizer step (every cfg.TRAIN.BATCH_SIZE frames, lib/model/train_val.py:379-382), so a caller transforms once per step
 * instead of once per frame.  Only for 3x3 / stride 1 / pad 1 layers and add == NULL. */
int frcnn_conv2d_bwd_data_pre(const float* dy, const float* w_crsk_flipped, const float* w_winograd, const float* add,
                              float* dx, int n, int h, int w, int c, int k, int r, int s, int stride, int pad, void* ws,
                              size_t ws_bytes, void* stream);
/* ... and with the activation backward of the layer BELOW folded into the store: dx = act_y > 0 ? dx * act_scale[c] : 0, i.e.
 * what frcnn_act_bwd(dx, act_y, act_scale, relu = 1) would make of the result in a second pass (act_y = that layer's ReLU
 * output, same shape as dx; act_scale = its folded BatchNorm scale or NULL).  lib/nets/resnet.py:98-127 backward: the data
 * gradient of conv3 directly yields the gradient of conv2's pre-activation output, that of conv2 the one of conv1's.  Not for
 * the strided 1x1 form. */
int frcnn_conv2d_bwd_data_act(const float* dy, const float* w_crsk_flipped, const float* w_winograd, const float* add,
                              const float* act_y, const float* act_scale, float* dx, int n, int h, int w, int c, int k, int r,
                              int s, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
size_t frcnn_conv2d_bwd_weight_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
/* counters: frcnn_conv2d_bwd_weight_counters(c, k, r, s) ints of device memory that are ZERO on entry and are left zero - one
 * per output tile: the workgroups that share a tile's pixel-split sums count themselves there and the last one adds the
 * slabs (in split order: deterministic) and writes / accumulates the result, so no second kernel runs.  Two launches that may
 * be in flight at the same time must not share counters (give each launch of a captured sequence its own range; launches that
 * are ordered on one stream may reuse a range).  NULL: only plans that need no counters are used (the register-staged kernel
 * with its reduction kernels, or an unsplit LDS-DMA launch). */
int frcnn_conv2d_bwd_weight_counters(int c, int k, int r, int s);
int frcnn_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int n, int h, int w, int c, int k,
                            int r, int s, int stride, int pad, void* ws, size_t ws_bytes, int* counters, void* stream);
/* Which filter-gradient kernels may be planned: 0 = all (default), 1 = conv_wgrad_f32 (register-staged, separate reduction /
 * accumulation kernels) only, 2 = conv_wgrad_dma_f32 (LDS-DMA ring, fused reduction + accumulation) wherever it applies
 * (operands < 2 GB).  Forgets the tuned filter-gradient plans.  A/B switch for tests and benchmarks. */
int frcnn_conv2d_wgrad_set_variant(int variant);
/* Force the filter-gradient plan of every following call (tests): kernel 1 / 2 = conv_wgrad_f32 with the 64 / 128 tile,
 * 3 / 4 = conv_wgrad_dma_f32 with the 64 / 128 tile; `splits` pixel ranges (clamped to the number of 32-pixel steps).
 * kernel 0 returns to the tuned / modelled plans.  A call the forced kernel cannot serve fails with FRCNN_ERR_ARG. */
int frcnn_conv2d_wgrad_set_plan(int kernel, int splits);

/* The same filter gradient ACCUMULATED into a parameter's own gradient buffer: grad_w (K, c_real, R, S) += dw (the layout of
 * nn.Conv2d.weight; nn.Linear.weight with R = S = 1), c_real <= c real input channels (c is the padded count of x),
 * grad_b (K) += db (may be NULL).  One pass sums the pixel-split slabs, drops the channel padding, changes the layout and
 * adds - instead of a reduction launch, a permute copy and an add per parameter; with `counters` (see frcnn_conv2d_bwd_weight)
 * that pass is the epilogue of the filter-gradient kernel itself.  Uses the plan frcnn_conv2d_bwd_weight tuned for the shape;
 * workspace of frcnn_conv2d_bwd_weight_ws_bytes. */
int frcnn_conv2d_bwd_weight_acc(const float* x, const float* dy, float* grad_w, int c_real, float* grad_b, int n, int h, int w,
                                int c, int k, int r, int s, int stride, int pad, void* ws, size_t ws_bytes, int* counters,
                                void* stream);
/* The same for `groups` (<= 24) convolutions of IDENTICAL shape in one launch pair: grad_w[g] += dW(x[g], dy[g]).  x, dy, grad_w
 * are HOST arrays of `groups` device pointers.  The repeated Bottlenecks of a ResNet stage (22 of the 23 blocks of layer3,
 * lib/nets/resnet.py:131-240) have identical filter-gradient problems whose outputs are too small to fill the chip one at a
 * time (hence pixel-split slabs and a reduction pass per layer); together they do, so every tile runs the whole pixel loop
 * and nothing is reduced afterwards.  ws: frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes.  Deterministic. */
size_t frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes(int groups, int c, int k, int r, int s);
int frcnn_conv2d_bwd_weight_acc_grouped(const float* const* x, const float* const* dy, float* const* grad_w, int groups,
                                        int c_real, int n, int h, int w, int c, int k, int r, int s, int stride, int pad,
                                        void* ws, size_t ws_bytes, void* stream);

/* bf16-operand gradients of a convolution (cfg.TRAIN.CONV_BF16; not in the reference): both operands of each product are rounded
 * to bf16 (nearest even) and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; every tensor in memory stays fp32.
 *   frcnn_conv2d_bwd_data_bf16: dx = act_bwd(conv_transpose(bf16(dy), w_bf16) [+ add]) - what frcnn_conv2d_bwd_data_act computes, for
 *     the stride-1 form and the zero-inserted strided r x s form (the strided 1x1 form stays fp32: FRCNN_ERR_ARG).  w_crsk_flipped_bf16 =
 *     frcnn_conv2d_pack_bf16 of frcnn_conv2d_transpose_filter's result; needs k % 32 == 0.  act_y / act_scale are applied by an
 *     frcnn_act_bwd pass over dx behind the GEMM.  ws: frcnn_conv2d_bwd_data_bf16_ws_bytes.
 *   frcnn_conv2d_bwd_weight_bf16: dw (k,r,s,c), overwritten = sum over pixels of bf16(dy) * bf16(patch(x)) [db: fp32 column sums of dy].
 *   frcnn_conv2d_bwd_weight_acc_bf16: the same added into the parameter's gradient (k, c_real, r, s) [grad_b].
 *     splits: pixel ranges summed into fp32 slabs that are added in range order (0 = the library's choice; clamped to the number
 *     of 32-pixel steps; a given count beyond 65535 or beyond 256 MB of slabs is FRCNN_ERR_ARG): the result is a fixed function
 *     of the operands and the split count.  No counters, no atomics.
 *     ws: frcnn_conv2d_bwd_weight_bf16_ws_bytes with the same `splits` (covers both forms and the bias gradient). */
size_t frcnn_conv2d_bwd_data_bf16_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
int frcnn_conv2d_bwd_data_bf16(const float* dy, const void* w_crsk_flipped_bf16, const float* add, const float* act_y,
                               const float* act_scale, float* dx, int n, int h, int w, int c, int k, int r, int s, int stride,
                               int pad, void* ws, size_t ws_bytes, void* stream);
size_t frcnn_conv2d_bwd_weight_bf16_ws_bytes(int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int splits);
int frcnn_conv2d_bwd_weight_bf16(const float* x, const float* dy, float* dw, float* db, int n, int h, int w, int c, int k, int r,
                                 int s, int stride, int pad, int splits, void* ws, size_t ws_bytes, void* stream);
int frcnn_conv2d_bwd_weight_acc_bf16(const float* x, const float* dy, float* grad_w, int c_real, float* grad_b, int n, int h,
                                     int w, int c, int k, int r, int s, int stride, int pad, int splits, void* ws, size_t ws_bytes,
                                     void* stream);

/* Tuning / test hook: force the workgroup tile to (64*tm) x (64*tn) output pixels x channels for all
 * following frcnn_conv2d_fwd calls of this process; (tm,tn) in {(4,2),(2,4)} (8 waves, one workgroup per
 * CU), {(2,2),(2,1),(1,2),(1,1)} (4 waves); (0,0) restores the automatic choice. */
int frcnn_conv2d_set_tile(int tm, int tn);
/* Plan autotuner (like a "benchmark mode"): when enabled, the first frcnn_conv2d_fwd / _bwd_data call of a shape
 * OUTSIDE stream capture times every (tile, split-K) candidate on the caller's tensors with HIP events — this
 * synchronises with the host — and caches the fastest; later calls (also captured ones) reuse it.  While enabled,
 * frcnn_conv2d_fwd_ws_bytes returns room for the largest candidate of a not-yet-tuned shape.  Default: off (the
 * analytic model picks).  frcnn_conv2d_bwd_weight follows the same switch with its own cache (tile 128x128 or 64x64 x
 * pixel splits).  frcnn_conv2d_clear_plans forgets both caches.
 * enable == 2: after one pass that times every candidate alone, the six fastest are timed UNDER LOAD - four launches of the
 * candidate in flight at once on four streams (the caller's and three of the library's own; all copies compute the same values
 * into the same tensors) - and ranked by that, i.e. by throughput on a busy chip, which is what a caller that keeps several
 * frames in flight needs (lib/model/test.py:183-228 replayed four frames at a time), instead of by the latency of one launch on
 * an idle chip. */
/* Form of the cached (tuned or imported) plan of a stride-1-output forward call of this shape: -1 none, 0 implicit GEMM,
 * 1 Winograd F(2x2,3x3).  Calls with and without a residual operand are planned separately.  Callers that keep a
 * pre-transformed Winograd filter (frcnn_conv2d_fwd_pre) use this to build it only for layers whose plan reads it. */
int frcnn_conv2d_plan_algo(int n, int h, int w, int c, int k, int r, int s, int stride, int pad, int has_residual);

/* Per-dispatch timing of the kernels frcnn_conv2d_fwd launches (the main implicit-GEMM kernel and, for a split-K
 * plan, the second pass): between _begin and _end every launch gets its own start / stop HIP events on the launch stream
 * (hipExtLaunchKernelGGL), i.e. the begin -> end time of that dispatch.  _end synchronises and fills, per dispatch in
 * launch order, the duration in microseconds, the number of the frcnn_conv2d_fwd call it belongs to (0-based since
 * _begin) and its kind (0 main kernel, 1 second pass).  Returns the number of dispatches recorded.  Not for use during
 * stream capture. */
int frcnn_conv2d_profile_begin(void);
int frcnn_conv2d_profile_end(float* us, int* call, int* kind, int capacity);
int frcnn_conv2d_set_autotune(int enable);
int frcnn_conv2d_clear_plans(void);
/* The plan cache as a table of 13 ints per entry (shape key n,h,w,c,k,r,s,stride,pad,out_stride [+256: call with a residual];
 * tile index [+16: Winograd F(2x2,3x3) around the grouped GEMM, +32: with the input transform fused into the 64x64 GEMM], splits,
 * K-steps per split), so that a tuned table can be saved and replayed (e.g. under a profiler, whose instrumentation would
 * otherwise perturb the tuning; or shipped with a deployment: bench.py loads profiles/r05_plans.json).  Tile indices:
 * 0 256x128, 1 128x256 (8 waves, LDS-DMA three stages), 2 128x128, 3 128x64, 4 64x128, 5 64x64 (register-staged), 6 128x128
 * LDS-DMA two stages, 7 64x64, 8 128x64, 9 64x128, 10 128x128, 11 256x128, 12 128x256 (LDS-DMA through buffer loads, three
 * stages), 13 64x64 with PERSISTENT workgroups (one K-step stream across a workgroup's tiles).  An LDS-DMA index runs its
 * kernel when C % 32 == 0 and frcnn_conv2d_set_staging is not 0 (7 .. 13: and both operands are below 2 GB); otherwise
 * EVERY index, 11 and 12 included, runs the register-staged kernel of its tile shape.  The table these indices select
 * from is kTiles in csrc/conv_igemm.hip.  export returns the number of cached entries (fills at most capacity_entries); import validates
 * every entry, then inserts all or none; an implicit-GEMM entry must split the ceil(r*s*c / 32) K-steps of its shape as
 * ceil(K-steps / steps per split) == splits. */
int frcnn_conv2d_export_plans(int* out, int capacity_entries);
int frcnn_conv2d_import_plans(const int* in, int entries);

/* Tuning / test hook: 1 (default) stages the 8-wave tiles with LDS-DMA (global_load_lds) when C % 32 == 0 (and the
 * autotuner may pick the two-stage LDS-DMA 128x128 tile, plan tile index 6), 0 uses the register-staged kernels
 * everywhere, 2 additionally runs a FORCED 128x128 tile (frcnn_conv2d_set_tile(2, 2)) on the two-stage LDS-DMA kernel,
 * 3 runs FORCED tiles (and plan tile indices 0 .. 5) on the buffer-load LDS-DMA kernel (conv_igemm_buf_f32: plan tile
 * indices 7 .. 12 select it in every mode but 0; needs C % 32 == 0 and operands below 2 GB, else the register-staged kernel
 * - except that indices 0 / 1 in mode 3 with an operand of 2 GB or more stay on their mode-1 LDS-DMA kernel).
 * Results are bit-identical for split_k = 1. */
int frcnn_conv2d_set_staging(int use_lds_dma);

/* Algorithm of the 3x3 / stride 1 / pad 1 convolutions without a residual (lib/nets/resnet.py:119-121 conv2 of a
 * Bottleneck, the RPN 3x3 of the Network):  0 (default) = the autotuner times the implicit GEMM and Winograd F(2x2, 3x3)
 * (same fp32 arithmetic, 2.25x fewer multiplications, four launches) and keeps the faster; without autotuning the
 * implicit GEMM runs;  1 = implicit GEMM only;  2 = Winograd wherever it applies (tests).  A Winograd plan is exported
 * with 16 added to its tile index.
 * Flags (tests, A/B timing): +16 never fuse the Winograd input transform into the GEMM, +32 forced Winograd uses the 64x64
 * GEMM with the fused transform, +64 the register-staged kernels store straight from the MFMA layout, +128 Winograd never
 * trims: by default the transform components of a partial 2x2 tile (last tile row of a map with odd h, last tile column
 * with odd w) that feed only outputs outside the map are neither transformed nor multiplied, which changes no output bit. */
int frcnn_conv2d_set_algo(int mode);
/* Host only: the rows the grouped Winograd GEMM of an n x h x w map executes under the current setting.  With
 * th = (h+1)/2, tw = (w+1)/2, T = n th tw tiles, eh = h & 1, ew = w & 1 and nI = n (th-eh)(tw-ew), nR = n (th-eh) ew,
 * nB = n eh (tw-ew): out[0] = T (each of the 9 components i != 3, j != 3), out[1] = nI + nR (3 components i == 3),
 * out[2] = nI + nB (3 components j == 3), out[3] = nI (component (3,3)); all T with flag 128 set.  Returns the sum over
 * the 16 components, 9 out[0] + 3 out[1] + 3 out[2] + out[3] (0 for a bad shape).  Plans with the fused input transform or the
 * persistent tile (index 13) always run 16 T rows.  out may be NULL. */
long frcnn_conv2d_winograd_rows(int n, int h, int w, long out[4]);

/* The filter side of a Winograd plan is constant while the weights are: U[16][k][c] = G g G^T of a (k,3,3,c) filter,
 * computed once per parameter version by the caller and handed to frcnn_conv2d_fwd_pre, which is frcnn_conv2d_fwd
 * with that one extra operand (NULL = transform inside the call, as frcnn_conv2d_fwd does).  The operand is only read
 * when the layer's plan is a Winograd plan. */
size_t frcnn_conv2d_winograd_filter_bytes(int k, int c);
int frcnn_conv2d_winograd_filter(const float* w_krsc, float* u, int k, int c, void* stream);
int frcnn_conv2d_fwd_pre(const float* x, const float* w_krsc, const float* w_winograd, const float* scale,
                         const float* shift, const float* residual, float* y, int n, int h, int w, int c, int k, int r,
                         int s, int stride, int pad, int relu, int split_k, void* ws, size_t ws_bytes, void* stream);
/* The closing convolution of a BasicBlock (lib/nets/resnet.py:62-69: relu(bn2(conv2(out)) + identity), conv2 3x3 / stride 1 /
 * pad 1) with the residual applied INSIDE a Winograd plan: frcnn_conv2d_fwd keeps its rule that a call with a residual runs
 * the implicit GEMM; this entry plans the call as the RESIDUAL-FREE call of its shape - the cached (tuned or imported) plan
 * under the residual-free key, forced Winograd (frcnn_conv2d_set_algo 2), a new shape tuned with autotuning on exactly as the
 * residual-free call would tune it - and where that plan is a Winograd plan (fused input transform and persistent tile
 * included) its output transform stores
 *     y = act( ((A^T m A) * scale + shift) + residual )
 * with (A^T m A) * scale + shift evaluated as without a residual, one rounded add, then the activation (relu(NaN) = NaN): bit
 * for bit the residual-free call with relu = 0 followed by a float32 add and a ReLU pass.  Where that plan is not a Winograd plan
 * (also: split_k > 0, a forced tile) the call IS frcnn_conv2d_fwd_pre with the residual.  Workspace: frcnn_conv2d_fwd_ws_bytes,
 * as for the residual-free call.  FRCNN_ERR_ARG without a launch: a NULL x / w_krsc / y / residual, and every shape that is not
 * 3x3 / stride 1 / pad 1 with c % 4 == 0 and k % 4 == 0.  w_winograd may be NULL (the filter is then transformed inside the call). */
int frcnn_conv2d_fwd_wres_pre(const float* x, const float* w_krsc, const float* w_winograd, const float* scale,
                              const float* shift, const float* residual, float* y, int n, int h, int w, int c, int k, int r,
                              int s, int stride, int pad, int relu, int split_k, void* ws, size_t ws_bytes, void* stream);

/* Opt-in inference form of frcnn_conv2d_fwd with bf16 OPERANDS on v_mfma_f32_32x32x16_bf16 (fp32 accumulation):
 *     y = act( (sum bf16(x) * bf16(w)) * scale + shift + residual )
 * x, scale, shift, residual and y are fp32 exactly as for frcnn_conv2d_fwd; x is rounded to bf16 (nearest even) inside the
 * kernel.  w_bf16 is the filter packed once per weight version by frcnn_conv2d_pack_bf16: a plain (k,r,s,c) array of 16-bit
 * words, fp32 -> bf16 round to nearest even (+-0 and +-inf kept, NaN stays NaN), frcnn_conv2d_pack_bf16_bytes bytes.
 * Needs c % 32 == 0 (else FRCNN_ERR_ARG) and 16-byte aligned x / w_bf16; any k >= 1.  No split-K, no Winograd, no workspace,
 * no plan-cache entry: one implicit-GEMM launch on a 128x128 tile, or on a 64x64 tile when 128x128 tiles would number fewer
 * than the CUs.  Both tiles give bit-identical results.  frcnn_conv2d_bf16_set_tile is a test / timing hook: 0 = that rule,
 * 1 = 64x64, 2 = 128x128. */
size_t frcnn_conv2d_pack_bf16_bytes(int k, int r, int s, int c);
int frcnn_conv2d_pack_bf16(const float* w_krsc, void* w_bf16, int k, int r, int s, int c, void* stream);
int frcnn_conv2d_fwd_bf16(const float* x, const void* w_bf16, const float* scale, const float* shift,
                          const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s, int stride,
                          int pad, int relu, void* stream);
int frcnn_conv2d_bf16_set_tile(int mode);

/* fp32-accurate form of frcnn_conv2d_fwd on the bf16 matrix pipe (same signature and semantics as frcnn_conv2d_fwd_bf16).
 * Every fp32 operand is the exact sum of three bf16 values hi + mid + lo (hi = bf16(v), mid = bf16(v - hi),
 * lo = bf16(v - hi - mid), round to nearest even); each product x * w is formed as six bf16 products accumulated in fp32,
 * per k = 16 group in the order
 *     x_lo*w_hi, x_hi*w_lo, x_mid*w_mid, x_mid*w_hi, x_hi*w_mid, x_hi*w_hi
 * with the groups in ascending k (taps r, s, then channels, as frcnn_conv2d_fwd_bf16): the first five into one fp32
 * accumulator per output, x_hi*w_hi into a second one, the two added once after the last group (small products added
 * straight into the large sum lose low bits inside the MFMA).  The three terms left out are at most 2^-26 of the
 * product.  Both tiles (frcnn_conv2d_bf16_set_tile applies) give bit-identical results.
 * OPERAND RANGE: finite operands of magnitude below about 2^120.  An infinite operand gives NaN where fp32 gives infinity
 * (its remainder is inf - inf); the remainders of operands within 2^16 of the smallest normal may flush to zero, so those
 * operands are carried with fewer than 24 bits.
 * frcnn_conv2d_pack_bf16x3 writes the filter as three (k,r,s,c) planes of 16-bit words, hi then mid then lo
 * (frcnn_conv2d_pack_bf16x3_bytes bytes), once per weight version; x is split inside the kernel, once per tile element.
 * frcnn_conv2d_split_bf16_wanted: 1 where this kernel is to replace the fp32 plan - a rule in the GEMM's dimensions
 * (M = n*ho*wo, N = k, Ktot = r*s*c): c % 32 == 0, ceil(M/128) * ceil(N/128) >= 256, N >= 512 and Ktot >= 512, and no
 * Winograd form (3x3, stride 1, pad 1 stays with fp32 F(2x2, 3x3), which measured faster).  It answers
 * 0 while frcnn_conv2d_set_tile forces a tile, frcnn_conv2d_set_algo / _set_staging are not at their defaults, or after
 * frcnn_conv2d_split_bf16_enable(0)
 * (test hook, part of frcnn_settings_signature). */
size_t frcnn_conv2d_pack_bf16x3_bytes(int k, int r, int s, int c);
int frcnn_conv2d_pack_bf16x3(const float* w_krsc, void* w_bf16x3, int k, int r, int s, int c, void* stream);
int frcnn_conv2d_fwd_bf16x3(const float* x, const void* w_bf16x3, const float* scale, const float* shift,
                            const float* residual, float* y, int n, int h, int w, int c, int k, int r, int s, int stride,
                            int pad, int relu, void* stream);
int frcnn_conv2d_split_bf16_wanted(int n, int h, int w, int c, int k, int r, int s, int stride, int pad);
int frcnn_conv2d_split_bf16_enable(int on);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1)  (lib/nets/resnet.py:156), NHWC. */
int frcnn_maxpool3x3s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
/* Its backward (trainable stem, cfg.RESNET.FIXED_BLOCKS == -1): dx (n,h,w,c) receives dy of every window whose first
 * maximum (row-major scan, like the index torch stores) is that pixel; gather form, deterministic. */
int frcnn_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, void* stream);

/* nn.MaxPool2d(kernel_size=2, stride=2), no padding, ceil_mode off (lib/nets/vgg16.py:35,46: the 'M' entries of
 * torchvision's VGG configuration 'D'), NHWC fp32: x (n,h,w,c) -> y (n, h/2, w/2, c),
 *   y[n,i,j,ch] = max over dy, dx in {0,1} of x[n, 2i+dy, 2j+dx, ch].
 * The last row of an odd h and the last column of an odd w belong to no window and are never read.  The maximum is exact and
 * follows torch's rule (val > max || isnan(val)): a NaN anywhere in a window makes that output NaN, +-inf behave as numbers.
 * The sign of a zero result is not pinned.  One launch on a bounded grid (at most FRCNN_MAXPOOL2X2_MAX_LANES lanes, each
 * walking the work items - one float4 of channels of one output - in a loop with 64-bit offsets); no
 * workspace, no LDS, no atomics, no host synchronisation: the call captures into a hipGraph.
 * FRCNN_ERR_ARG without a launch: a null x / y, n / c < 1, h < 2 or w < 2 (empty output), c % 4 != 0, a pointer that is not
 * 16-byte aligned. */
#define FRCNN_MAXPOOL2X2_MAX_LANES (2048 * 256)
int frcnn_maxpool2x2s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
/* Its backward: x (n,h,w,c) the pooled input, dy (n, h/2, w/2, c) -> dx (n,h,w,c).  Per window the winner receives dy and the
 * other three elements 0.f; the winner is torch's (scan (0,0), (0,1), (1,0), (1,1); an element takes over when
 * val > max || isnan(val)): the first of equal values, the last NaN, element (0,0) of four -inf.  relu_mask != 0: x is the
 * ReLU output in front of the pool and the winner receives dy only if x[winner] > 0 (frcnn_act_bwd's expression), i.e. dx is
 * the gradient of the ReLU's input.  EVERY element of dx is written by this launch: the trailing row of an odd h and the
 * trailing column of an odd w receive 0.f (they are never read from x) - no memset, no workspace, no LDS, no atomics,
 * deterministic; the call captures into a hipGraph.  Work item: one float4 of channels of one cell of the
 * ceil(h/2) x ceil(w/2) grid, on the forward's bounded grid (FRCNN_MAXPOOL2X2_MAX_LANES).  FRCNN_ERR_ARG without a launch: the
 * forward's rules, for x, dy and dx. */
int frcnn_maxpool2x2s2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, int relu_mask, void* stream);

/* Depthwise 3x3 convolution, pad 1, stride 1 or 2, with the folded BatchNorm and ReLU6 of MobileNet-v1's conv_dw block:
 * nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) -> nn.BatchNorm2d (eval) -> nn.ReLU6
 * (lib/nets/mobilenet_v1.py:117-123).  x (n,h,w,c) NHWC, w_rsc (3,3,c) (the module's (c,1,3,3) weight, channel last),
 * y (n,oh,ow,c) with oh = (h-1)/stride + 1, ow likewise.  Per output element
 *   acc = sum over the taps inside the image of w_rsc[r,s,ch] * min(x[n, oh*stride-1+r, ow*stride-1+s, ch], in_cap)
 *   t = acc * scale[ch] + shift[ch]   (null scale / shift: 1 / 0);   t = max(t, 0) if relu;   y = min(t, out_cap).
 * Zero padding is per image.  in_cap finishes the ReLU6 of the layer that produced x (its kernel applied max(.,0) only),
 * out_cap = 6 with relu = 1 is this layer's own ReLU6; +inf switches a cap off.  What a NaN in x or t becomes under a
 * cap is not pinned.  fp32, products and sums rounded one by one (no fma), taps added in a fixed order: deterministic.
 * FRCNN_ERR_ARG without a launch: c % 4 != 0, stride outside {1,2}, n < 0, h / w / c < 1, c > 262144, a null x / w_rsc /
 * y, a pointer that is not 16-byte aligned.  n == 0: FRCNN_OK, nothing launched.  One launch, no workspace.
 * FRCNN_DWCONV_STRIP: outputs along W one lane produces per work item (widths around its multiples are the kernel's edges). */
#define FRCNN_DWCONV_STRIP 4
int frcnn_dwconv3x3_fwd(const float* x, const float* w_rsc, const float* scale, const float* shift, float* y, int n, int h,
                        int w, int c, int stride, float in_cap, float out_cap, int relu, void* stream);
/* x[i] = min(x[i], cap) in place over count floats: the upper half of an nn.ReLU6 (lib/nets/mobilenet_v1.py:115,131)
 * whose lower half ran in a convolution's epilogue, for the two pointwise outputs no depthwise layer reads.  What a NaN
 * becomes is not pinned.  count == 0: nothing launched.  FRCNN_ERR_ARG: count < 0, null x, x not 16-byte aligned. */
int frcnn_clamp_max(float* x, int64_t count, float cap, void* stream);

/* Gradients of the depthwise convolution above, for training MobileNet-v1: what autograd runs for
 * lib/nets/mobilenet_v1.py:117-123 under loss.backward() (lib/model/train_val.py:458).  In the forward's notation
 * u = min(x, in_cap), t = conv(u) * scale + shift, y = min(relu ? max(t, 0) : t, out_cap), both read the MASKED upstream
 * gradient, computed from dy and the forward's stored y as they are loaded and never stored:
 *   dz[n,oh,ow,ch] = dy[n,oh,ow,ch] * scale[ch] * m,   m = 1 where (relu off or y > 0) and y < out_cap, else 0
 * (hardtanh's backward as torch defines it for nn.ReLU6: zero at both closed ends).  With relu = 0 and out_cap = +inf the
 * mask is 1 and y may be null; a null scale is 1.  fp32, products and sums rounded one by one, fixed order, no atomics:
 * two runs on the same operands are bit-equal.  Argument rules as the forward's (FRCNN_ERR_ARG without a launch: c % 4,
 * stride outside {1,2}, n < 0, h / w / c < 1, a null required pointer, a null y with a mask, a pointer that is not 16-byte
 * aligned); n == 0: FRCNN_OK.
 *
 * bwd_data: the gradient with respect to u, (n,h,w,c):
 *   dx[n,hh,ww,ch] = sum over (r,s) with (hh+1-r), (ww+1-s) divisible by stride and inside (oh,ow) of
 *                    w_rsc[r,s,ch] * dz[n,(hh+1-r)/stride,(ww+1-s)/stride,ch]
 * Gather form, every element of dx written once.  The ReLU6 mask of the layer that produced x (in_cap) belongs to that
 * layer's backward; x is not read.  One launch, no workspace.
 *
 * bwd_weight: the parameter's own (c,1,3,3) layout,
 *   dw[ch,0,r,s] (+)= sum over n,oh,ow of dz[n,oh,ow,ch] * min(x[n,oh*stride-1+r,ow*stride-1+s,ch], in_cap)
 * (taps outside the image contribute 0); accumulate = 1 adds into dw, 0 overwrites (n == 0: dw is zeroed).  Two launches:
 * workgroup partials into ws (the _ws_bytes query, 16-byte aligned), then their sum in a fixed order. */
int frcnn_dwconv3x3_bwd_data(const float* dy, const float* y, const float* w_rsc, const float* scale, float* dx, int n, int h,
                             int w, int c, int stride, float out_cap, int relu, void* stream);
size_t frcnn_dwconv3x3_bwd_weight_ws_bytes(int n, int h, int w, int c, int stride);
int frcnn_dwconv3x3_bwd_weight(const float* x, const float* dy, const float* y, const float* scale, float* dw, int n, int h,
                               int w, int c, int stride, float in_cap, float out_cap, int relu, int accumulate, void* ws,
                               size_t ws_bytes, void* stream);
/* Backward of a ReLU6 behind a GEMM convolution (the pointwise layers, lib/nets/mobilenet_v1.py:117-123 under
 * loss.backward(), lib/model/train_val.py:458): d_conv = dy * scale[k] * [y > 0 if relu] * [y < cap] over rows x k floats,
 * any k >= 1.  The convolution's stored y carries the lower half of the ReLU6 only; 0 < y < cap is the same mask whether or
 * not the upper clamp has been applied to y in place.  Null scale: 1; null y only with relu = 0 and cap = +inf.
 * rows * k == 0: nothing launched.  FRCNN_ERR_ARG: rows < 0, k < 1, a null dy / d_conv, a pointer not 16-byte aligned. */
int frcnn_act_bwd_cap(const float* dy, const float* y, const float* scale, int relu, float cap, int64_t rows, int k,
                      float* d_conv, void* stream);

/* NHWC image/BEV blob (lib/roi_data_layer/minibatch.py:670 layout, (1,H,W,C)) -> NHWC with the channel
 * count padded with zeros to c_pad (multiple of 4) so the stem conv reads 16-byte pixels. */
int frcnn_pad_channels(const float* x, float* y, int64_t pixels, int c, int c_pad, void* stream);

/* Image input producer: prep_im_for_blob + im_list_to_blob (lib/utils/blob.py:16-54) for one frame on
 * the device.  img (h,w,3) uint8 in cv2.imread order -> blob (out_h,out_w,c_out) fp32 with
 * blob[..,c] = (resize(img)[.., arrange[c]] - means[c]) / stddevs[c], c_out = 3 or 4 (4th channel zero).
 * cv2.resize(fx=fy=scale, INTER_LINEAR) semantics restated (cv2 is not vendored by the reference).
 * means / stddevs (3 doubles) and arrange (3 ints) are HOST pointers. */
int frcnn_prep_image_out_size(int h, int w, float scale, int* out_h, int* out_w);
int frcnn_prep_image(const uint8_t* img_hwc3, int h, int w, float scale, const double* means_host,
                     const double* stddevs_host, const int* arrange_host, int c_out, float* blob, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RPN / proposal stage
 * ------------------------------------------------------------------------------------------- */
/* generate_anchors_pre (lib/layer_utils/snippets.py:13-40): anchors[(y*W+x)*A + a] = base[a] + shift.
 * `base` is the (A,4) table of generate_anchors (lib/layer_utils/generate_anchors.py:41-54), computed on
 * the host in float64 (DEVICE pointer to A*4 doubles); the shift is added in float64 and the sum is
 * rounded once to fp32, exactly like the reference's astype(float32). */
int frcnn_generate_anchors(const double* base, int num_base, int height, int width, int feat_stride,
                           float* anchors, void* stream);

/* GridAnchor3dGenerator._generate (lib/layer_utils/generate_3d_anchors.py:15-118) and the axis-aligned BEV
 * box of each 3-D anchor (bbaa_graphics_gems, lib/utils/bbox.py:256-293, clip=False) for the LiDAR RPN.
 * base (DEVICE, num_types x 9 floats), one row per (size, rotation) type, rotation fastest:
 *   [lo_x, lo_y, hi_x, hi_y, z, l, w, h, ry]  (host-computed like generate_3d_anchors.py:37-38,100 and
 *   bbox.py:258-279).  anchors_3d (H*W*T, 7) [x,y,z,l,w,h,ry], anchors_2d (H*W*T, 4), order (H, W, T). */
int frcnn_generate_anchors_3d(const float* base, int num_types, int height, int width, int feat_stride,
                              float* anchors_3d, float* anchors_2d, void* stream);

/* Fused front half of proposal_layer (lib/layer_utils/proposal_layer.py:32-36) on the raw RPN head
 * output `rpn` (H*W, ld) NHWC with channels [0,A) = bg logits, [A,2A) = fg logits, [2A,6A) = deltas:
 *   fg prob of the 2-way softmax, bbox_transform_inv (lib/model/bbox_transform.py:75-105) and
 *   clip_boxes (:235-257, info = [x_min,x_max,y_min,y_max,...]).
 * With probs_in != NULL the logits are ignored and (H*W*A) ready-made fg probabilities are copied
 * (the exact proposal_layer signature, which receives rpn_cls_prob). info is a HOST pointer to 4+ floats. */
int frcnn_rpn_decode_clip(const float* rpn, int ld, const float* probs_in, const float* deltas_in,
                          const float* anchors, const float* info_host, int hw, int num_anchors,
                          float* scores, float* proposals, void* stream);

/* Stand-alone box codec (the proposal and tail kernels fuse the same arithmetic):
 * bbox_transform_inv (lib/model/bbox_transform.py:75-105): boxes rows of box_ld floats whose first 4 are
 * [x1,y1,x2,y2]; deltas/out (n, 4*num_classes); scale > 0 divides the boxes first (:77-78), scale <= 0 = None.
 * clip_boxes (:235-257): num_boxes 4-float boxes; info HOST pointer [x_min,x_max,y_min,y_max]. */
int frcnn_bbox_transform_inv(const float* boxes, int box_ld, const float* deltas, int n, int num_classes,
                             float scale, float* out, void* stream);
int frcnn_clip_boxes(const float* boxes, int num_boxes, const float* info_host, float* out, void* stream);
/* lidar_3d_bbox_transform_inv (lib/model/bbox_transform.py:174-233): rois rows of roi_ld floats whose first 4
 * are [x1,y1,x2,y2]; anchors_3d (n,7); deltas/out (n, 7*num_classes); scale <= 0 = None. */
int frcnn_lidar_bbox_transform_inv(const float* rois, int roi_ld, const float* anchors_3d, const float* deltas,
                                   int n, int num_classes, float scale, float* out, void* stream);

/* uncertainty_transform_inv (lidar == 0) / lidar_3d_uncertainty_transform_inv (lidar != 0), lib/model/bbox_transform.py:
 * 107-130 / 132-169: uncertainty (n, 7K) of the deltas [x,y,z,l,w,h,ry] -> squared box-space terms, out (n, 4K) [x,y,l,w]
 * or (n, 7K).  rois (n rows, first 4 = BEV [x1,y1,x2,y2], divided by scale when scale > 0), anchors_3d (n,7) supplies the
 * height of the z term (may be NULL when lidar == 0).  input_is_variance != 0: the square root of every input element is
 * taken first (Monte-Carlo variances -> standard deviations). */
int frcnn_uncertainty_transform_inv(const float* rois, int roi_ld, const float* anchors_3d, const float* uncertainty, int n,
                                    int num_classes, float scale, int lidar, int input_is_variance, float* out, void* stream);

/* scores.sort(descending=True)[:top_n] (proposal_layer.py:39-42) with the canonical total order
 * (score desc, index asc).  order_out[top_n] int64 source indices, scores_out[top_n];
 * count_out[0] = min(n, top_n).  top_n <= 16384.  n <= 16384: one workgroup in LDS; larger n: multi-workgroup
 * radix select over all CUs (workspace from frcnn_sort_topk_desc_ws_bytes), same result. */
size_t frcnn_sort_topk_desc_ws_bytes(int n, int top_n);
int frcnn_sort_topk_desc(const float* scores, int n, int top_n, int64_t* order_out, float* scores_out,
                         int* count_out, void* ws, size_t ws_bytes, void* stream);

/* rows_out[i,:] = rows[order[i],:]  for i < count (device count), `width` floats per row. */
int frcnn_gather_rows(const float* rows, const int64_t* order, const int* count, int max_count, int width,
                      float* rows_out, void* stream);

/* The uncertainty columns of a frame's detections in one launch (version 124): nms_hstack_var_torch,
 * lib/utils/filter_predictions.py:23-43, plus the column stacking of lib/model/test.py:260-270.
 *   dets (num_classes, max_out, det_width), det_roi (num_classes, max_out) int32 RoI row of each detection, -1 = padding;
 *   out (num_classes, max_out, det_width + sum of widths) = [dets row | source 0 | source 1 | ...].
 * sources_host / widths_host / per_class_host are HOST arrays of num_sources (1..8) entries: a device pointer, the
 * number of output columns, and the kind.  per_class != 0: the source is (num_rois, num_classes * width) and class j
 * takes columns [j*width, (j+1)*width) of its RoI's row (the *bbox_var terms); per_class == 0: the source is
 * (num_rois, width) and every class takes the whole row (entropy, mutual information: width 1; class variances).
 * Valid rows are copies.  Rows with det_roi outside [0, num_rois) keep their box columns and receive +0.0 in the
 * uncertainty columns.  The host arrays are read during the call only; no workspace, no host synchronisation, the launch
 * captures into a hipGraph. */
int frcnn_uncertainty_columns(const float* dets, const int* det_roi, int num_classes, int max_out, int det_width,
                              int num_rois, int num_sources, const float* const* sources_host, const int* widths_host,
                              const int* per_class_host, float* out, void* stream);

/* torchvision.ops.nms at IoU == threshold exactly (proposal_layer.py:46, filter_predictions.py:67-69): on != 0 (default)
 * suppresses the box like torchvision 0.4.0's CPU kernel (`iou >= threshold`), 0 keeps it like its CUDA kernel
 * (`iou > threshold`).  Process-wide, read when frcnn_nms / frcnn_filter_per_class* launch. */
int frcnn_nms_set_suppress_at_equal(int on);
int frcnn_nms_get_suppress_at_equal(void);

/* torchvision.ops.nms (call sites proposal_layer.py:46, filter_predictions.py:67-69) on boxes already
 * sorted by descending score: box j is dropped when IoU(i,j) > thresh for an earlier kept i
 * (areas without +1).  n_dev (device int, may be NULL -> n_max) boxes are live.
 * keep_idx[max_keep] int64 positions of survivors in score order (entries past keep_count are written as 0),
 * keep_mask[n_max] bytes, keep_count[0] = min(#survivors, max_keep). */
size_t frcnn_nms_ws_bytes(int n_max);
int frcnn_nms(const float* boxes, const int* n_dev, int n_max, float thresh, int max_keep,
              int64_t* keep_idx, uint8_t* keep_mask, int* keep_count, void* ws, size_t ws_bytes,
              void* stream);

/* Tail of proposal_layer (proposal_layer.py:50-55): rois[i] = [0, proposals[order... keep[i]]],
 * roi_scores[i]; rows >= keep_count are zero-filled.  sorted_boxes are the score-ordered boxes. */
int frcnn_make_rois(const float* sorted_boxes, const float* sorted_scores, const int64_t* keep_idx,
                    const int* keep_count, int max_keep, float* rois, float* roi_scores, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RoIAlign (torchvision.ops.roi_align 0.4.0 semantics = aligned=False; call sites
 * lib/utils/torchpoolers.py:165-170,194-197 and the _crop_pool_layer of the missing network.py).
 * feat NHWC (n,H,W,C); rois (R,5) [batch,x1,y1,x2,y2]; out (R,P,P,C) NHWC.
 * sampling_ratio <= 0 -> adaptive ceil(roi/P).  roi_count (device int, may be NULL) masks rows
 * >= count to zero.  level_of_roi/level (may be NULL/-1): only rois with level_of_roi[r]==level
 * are written (MultiScaleRoIAlign, torchpoolers.py:187-199).
 * ------------------------------------------------------------------------------------------- */
/* feat holds n images (n,H,W,C).  rois_per_image == 0: the image of a RoI is its batch column and roi_count (may be NULL)
 * is ONE live count; rois_per_image > 0: rows [i*rois_per_image, (i+1)*rois_per_image) belong to image i whatever their
 * batch column says, and roi_count points to n live counts (frames batched into one call).
 * Tuning / test hook: 0 automatic (map-resident kernel when one 16-channel slice of the map fits the LDS: pooled 7,
 * c % 16 == 0, h <= 64, h*w*64 B + 10 KB <= 160 KB; else the planned pair when a workspace is given; else generic),
 * 1 generic kernel, 2 generic with per-XCD channel slices, 3 / 4 planned kernel with 8 / 4 loads in flight per lane,
 * 5 map-resident kernel or an error. */
int frcnn_roi_align_set_variant(int variant);
/* Scratch for the planned kernel pair: the compact work-item list + the per-bin axis weight tables.  Returns 0
 * when the shape has no planned path (pooled != 7).  Passing ws == NULL to frcnn_roi_align_fwd is always valid (the
 * map-resident and the generic kernels need none). */
size_t frcnn_roi_align_fwd_ws_bytes(int h, int w, int c, int num_rois, int pooled);
int frcnn_roi_align_fwd(const float* feat, int n, int h, int w, int c, const float* rois, const int* roi_count,
                        int num_rois, int rois_per_image, int pooled, float spatial_scale, int sampling_ratio,
                        const int* level_of_roi, int level, float* out, void* ws, size_t ws_bytes, void* stream);
/* frcnn_roi_align_fwd with a per-channel epilogue on the pooled value: out = act(pooled * scale[c] + shift[c]) (scale / shift
 * device float[c] or NULL, relu 0/1).  Pooling and a bias-free 1x1 convolution commute (both linear, different axes), so
 * layer4[0].conv1 and layer4[0].downsample[0] - which the reference applies to pool5, lib/nets/resnet.py:98-127 via
 * _head_to_tail - can run on the H x W feature map BEFORE the pooling (6x fewer pixels than 300 x 7 x 7) with their folded
 * BatchNorm + ReLU applied here, after the pooling, where the reference applies them.  Not available with the map-resident
 * kernel (variant 5). */
int frcnn_roi_align_fwd_affine(const float* feat, int n, int h, int w, int c, const float* rois, const int* roi_count,
                               int num_rois, int rois_per_image, int pooled, float spatial_scale, int sampling_ratio,
                               const int* level_of_roi, int level, float* out, const float* scale, const float* shift,
                               int relu, void* ws, size_t ws_bytes, void* stream);
/* One map, two outputs over the channel ranges [0, split_c) and [split_c, c), ONE plan launch: out1 (num_rois,7,7,split_c) =
 * act1(pooled * scale + shift), out2 (num_rois,7,7,c - split_c) likewise (scale / shift: device float[c] or NULL, indexed by
 * the MAP's channel; relu1 / relu2 0/1).  The inference path runs layer4[0].conv1 and layer4[0].downsample[0]
 * (lib/nets/resnet.py:98-127) as one 1x1 convolution with concatenated filters and pools its 512 + 2048 channels here.
 * split_c % 256 == 0; pooled == 7; ws: frcnn_roi_align_fwd_ws_bytes(h, w, 4, num_rois, 7). */
int frcnn_roi_align_fwd_split(const float* feat, int h, int w, int c, const float* rois, const int* roi_count, int num_rois,
                              int pooled, float spatial_scale, int sampling_ratio, int split_c, float* out1, float* out2,
                              const float* scale, const float* shift, int relu1, int relu2, void* ws, size_t ws_bytes,
                              void* stream);

/* LevelMapper (lib/utils/torchpoolers.py:20-51) of MultiScaleRoIAlign: levels[i] = clamp(floor(canonical_level +
 * log2(sqrt(area_i) / canonical_scale) + eps), k_min, k_max) - k_min for rois (n,5); area without +1. */
int frcnn_fpn_level_map(const float* rois, int num_rois, int k_min, int k_max, float canonical_scale,
                        float canonical_level, float eps, int* levels, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Detection tail (_head_to_tail mean + _region_classification + test-time decode of network.py;
 * evidence lib/model/test.py:75-79, lib/model/config.py:219-223):
 *   fc7 = x.mean(3).mean(2); cls_score = fc7 W_c^T + b_c; cls_prob = softmax; deltas = fc7 W_b^T + b_b;
 *   pred_boxes = bbox_transform_inv(rois[:,1:5], deltas*stds+means, scale).
 * x (R,P,P,C) NHWC; w_cls (K,C); w_box (K*4,C); stds/means HOST pointers to 4 floats.
 * Outputs: fc7 (R,C), cls_score (R,K), cls_prob (R,K), bbox_pred (R,4K) raw, pred_boxes (R,4K).
 * ------------------------------------------------------------------------------------------- */
int frcnn_head_fc_softmax_decode(const float* x, int num_rois, int pooled, int c, const float* w_cls,
                                 const float* b_cls, const float* w_box, const float* b_box,
                                 int num_classes, const float* rois, const float* stds_host,
                                 const float* means_host, float scale, float* fc7, float* cls_score,
                                 float* cls_prob, float* bbox_pred, float* pred_boxes, void* stream);

/* LiDAR tail: as above with 7-DoF boxes — bbox_pred (R,7K), pred_boxes = lidar_3d_bbox_transform_inv(
 * rois[:,1:5], roi_anchors_3d, deltas*stds+means, scale) (lib/model/bbox_transform.py:174-233);
 * roi_anchors_3d (R,7) are the 3-D anchors of the RoIs (proposal_layer.py:44,52); stds/means 7 floats. */
int frcnn_head_fc_softmax_decode_lidar(const float* x, int num_rois, int pooled, int c, const float* w_cls,
                                       const float* b_cls, const float* w_box, const float* b_box,
                                       int num_classes, const float* rois, const float* roi_anchors_3d,
                                       const float* stds_host, const float* means_host, float scale, float* fc7,
                                       float* cls_score, float* cls_prob, float* bbox_pred, float* pred_boxes,
                                       void* stream);

/* Wide form of the tail, for class counts past the limits above (num_classes * 5 > 64 for image boxes, * 8 > 64 for LiDAR
 * boxes: PASCAL VOC's 21 of lib/datasets/pascal_voc.py, COCO's 81 of lib/datasets/coco.py, KITTI's full label set).  It
 * replaces the same reference calls on an fc7 that already exists: cls_score = cls_score_net(fc7), cls_prob =
 * softmax(cls_score, 1), bbox_pred = bbox_pred_net(fc7) (_region_classification of network.py; module names
 * lib/nets/imagenet.py:83-86) and pred_boxes = bbox_transform_inv(rois[:,1:5], bbox_pred*stds+means, scale)
 * (lib/model/bbox_transform.py:75-105; lib/model/test.py:75-79).
 * fc7 (R,C) is an INPUT (every caller pools to 1x1 before the heads); w_cls (K,C) and w_box (4K,C) are read by their own
 * addresses, 16-byte aligned like fc7.  The two Linear layers run as one 32 x 32-tiled GEMM on v_mfma_f32_32x32x2_f32 with
 * the channels split over two workgroups; a second launch of one wave per RoI adds the two halves and the bias and does
 * the softmax and the decode with the arithmetic of the fused kernel (class-order fp32 sum).  No workspace: cls_prob and
 * pred_boxes hold the second half's sums between the two launches, so the four outputs must be four distinct buffers.  No
 * atomics, no host synchronisation; a RoI's outputs depend on that RoI's inputs only.  num_rois >= 1, c % 4 == 0, 2 <= num_classes <= 4096 (small class counts are accepted too), scale > 0;
 * anything else returns FRCNN_ERR_ARG and launches nothing.
 * Outputs: cls_score (R,K), cls_prob (R,K), bbox_pred (R,4K) raw, pred_boxes (R,4K). */
int frcnn_head_wide_softmax_decode(const float* fc7, int num_rois, int c, const float* w_cls, const float* b_cls,
                                   const float* w_box, const float* b_box, int num_classes, const float* rois,
                                   const float* stds_host, const float* means_host, float scale, float* cls_score,
                                   float* cls_prob, float* bbox_pred, float* pred_boxes, void* stream);

/* Wide LiDAR tail: as above with 7-DoF boxes - w_box (7K,C), bbox_pred (R,7K), pred_boxes =
 * lidar_3d_bbox_transform_inv(rois[:,1:5], roi_anchors_3d, bbox_pred*stds+means, scale)
 * (lib/model/bbox_transform.py:174-233); roi_anchors_3d (R,7) must not be NULL; stds/means 7 floats. */
int frcnn_head_wide_softmax_decode_lidar(const float* fc7, int num_rois, int c, const float* w_cls, const float* b_cls,
                                         const float* w_box, const float* b_box, int num_classes, const float* rois,
                                         const float* roi_anchors_3d, const float* stds_host, const float* means_host,
                                         float scale, float* cls_score, float* cls_prob, float* bbox_pred,
                                         float* pred_boxes, void* stream);

/* filter_and_draw_prep + nms_hstack_torch + the max_dets cut (lib/utils/filter_predictions.py:75-130,
 * 45-72; lib/model/test.py:210-221) for the image detector, all on the device:
 * clamp to [0, frame/scale-1] in place, per class j>=1 keep score > thresh, NMS(nms_thresh) in
 * descending score order, keep dets with score >= the max_dets-th best.
 * dets (K, max_out, 5) [x1,y1,x2,y2,score], det_count (K) ints: EVERY row is written by the call (rows past a class's
 * count and the whole background class 0 are zero), the caller need not clear them.  roi_count device int or NULL.
 * det_roi (K, max_out) ints or NULL: RoI row of every detection (-1 past det_count) - what nms_hstack_var_torch
 * (filter_predictions.py:23-43) needs to gather the per-RoI uncertainties of the kept detections. */
/* Test hook: 0 = automatic (num_rois <= 1024: LDS-resident kernel), 1 = always the general workspace kernel. */
int frcnn_filter_set_variant(int variant);
size_t frcnn_filter_per_class_ws_bytes(int num_rois, int num_classes);
int frcnn_filter_per_class(float* pred_boxes, const float* cls_prob, const int* roi_count, int num_rois,
                           int num_classes, float frame_w, float frame_h, float scale, float thresh,
                           float nms_thresh, int max_dets, int max_out, float* dets, int* det_count,
                           int* det_roi, void* ws, size_t ws_bytes, void* stream);

/* LiDAR input producer (lib/roi_data_layer/minibatch.py:232-235,434-512): points (num_points, point_stride >= 4)
 * rows [x,y,z,intensity,(elongation)...] in file order -> bev (gy, gx, num_slices + num_meta) fp32, the blob of one
 * frame (already transposed to y-major like the reference's final np.transpose).
 * pc_range_host[6] = [xmin,ymin,zmin,xmax,ymax,zmax] AFTER the reference's shift (zmin = 0, zmax = Z1 - Z0),
 * z_shift = cfg.LIDAR.Z_RANGE[0] (subtracted from every z), voxel_size_host[3]; grid = round((max-min)/size).
 * spconv VoxelGeneratorV2 semantics restated (third party, absent: parity unpinned): voxels numbered by first
 * appearance, at most max_voxels, each keeps its first max_points points.  Height slice = max z - slice*voxel height,
 * evaluated like the reference's numpy expression (minibatch.py:467, int32 * Python float): in float64 from the fp32
 * max z and the DOUBLE voxel height, rounded once to fp32.  frcnn_bev_voxelize_h takes that double (cfg.LIDAR.
 * VOXEL_HEIGHT as the caller holds it; it must round to voxel_size_host[2]) and is exact for every height;
 * frcnn_bev_voxelize is the same call with voxel_height = (double)voxel_size_host[2], which is the configured value
 * only when that is an fp32 number (the default 0.5 is; 0.4 is not).
 * meta channels (density, tanh(mean intensity), tanh(mean elongation) or 0 when elongation_col < 0): the voxel
 * created last in a column wins.  num_voxels (device int, may be NULL) = occupied cells before the max_voxels cap. */
int frcnn_bev_voxelize_grid(const float* pc_range_host, const float* voxel_size_host, int* grid_host);
size_t frcnn_bev_voxelize_ws_bytes(int num_points, const float* pc_range_host, const float* voxel_size_host,
                                   int max_voxels);
int frcnn_bev_voxelize(const float* points, int num_points, int point_stride, const float* pc_range_host,
                       const float* voxel_size_host, float z_shift, int max_points, int max_voxels, int num_slices,
                       int num_meta, int elongation_col, float* bev, int* num_voxels, void* ws, size_t ws_bytes,
                       void* stream);
int frcnn_bev_voxelize_h(const float* points, int num_points, int point_stride, const float* pc_range_host,
                         const float* voxel_size_host, double voxel_height, float z_shift, int max_points,
                         int max_voxels, int num_slices, int num_meta, int elongation_col, float* bev, int* num_voxels,
                         void* ws, size_t ws_bytes, void* stream);

/* LiDAR point-cloud augmentation and test-time rain simulation (lib/roi_data_layer/minibatch.py:274-428), the per-point
 * transforms in front of frcnn_bev_voxelize, one pass in the reference's order: filter_points on the raw point
 * (:232-235,274), Gaussian distortion (:309-319), dropout (:321-325), rotation about z (:330-349,695-714), x/y swap
 * (:351-373), flip y (:375-384), flip x (:386-395), rain (:397-421), test dropout with p_keep 0.8 (:422-425); `flags`
 * selects the steps.  points / out (num_points, point_stride >= 4) rows [x,y,z,intensity,...]; out may be points itself.
 * range_host[6] = [X0,Y0,Z0,X1,Y1,Z1] = cfg.LIDAR.*_RANGE (unshifted).  params_host[FRCNN_AUG_NUM_PARAMS]: indices
 * FRCNN_AUG_P_* (p_keep in (0, 1] always; cos / sin of the angle computed in double and rounded once; rain rate in mm/h
 * and cfg.<DB>.LIDAR_MAX_RANGE in m, read only with FRCNN_AUG_RAIN).  Draws are counter-based, value = f(seed + *seed_dev,
 * stream, row index) (csrc/rng.h; seed_dev device uint32 or NULL): normal01 streams 32, 33, 34 = distortion of x, y, z,
 * 35 = rain shift; uniform01 stream 72 = dropout, 73 = test dropout.  A dropped point keeps its row with x, y, z = NaN
 * (frcnn_bev_voxelize's range test rejects it; row order, hence voxel numbering, is the reference's).  kept_count
 * (device int, written by the call) = surviving points inside range_host, the reference's "no points left" test
 * (:426-432).  max_blocks: 0 = automatic grid, > 0 caps the workgroups (test hook: the result does not depend on it). */
#define FRCNN_AUG_GAUSS 1u
#define FRCNN_AUG_DROPOUT 2u
#define FRCNN_AUG_ROTATE 4u
#define FRCNN_AUG_SWAP_XY 8u
#define FRCNN_AUG_FLIP_Y 16u
#define FRCNN_AUG_FLIP_X 32u
#define FRCNN_AUG_RAIN 64u
#define FRCNN_AUG_TEST_DROPOUT 128u
#define FRCNN_AUG_ALL 255u
#define FRCNN_AUG_P_SIGMA_X 0
#define FRCNN_AUG_P_SIGMA_Y 1
#define FRCNN_AUG_P_SIGMA_Z 2
#define FRCNN_AUG_P_KEEP 3
#define FRCNN_AUG_P_COS 4
#define FRCNN_AUG_P_SIN 5
#define FRCNN_AUG_P_RAIN_RATE 6
#define FRCNN_AUG_P_RAIN_MAX_RANGE 7
#define FRCNN_AUG_NUM_PARAMS 8
int frcnn_lidar_augment(const float* points, int num_points, int point_stride, const float* range_host, unsigned flags,
                        const float* params_host, uint32_t seed, const uint32_t* seed_dev, float* out, int* kept_count,
                        int max_blocks, void* stream);
/* The same pass with the camera field-of-view filter of KITTI / CADC scans (lib/roi_data_layer/minibatch.py:251-268,
 * get_fov_flag :678-693) as its FIRST step, in front of filter_points: no launch of its own.  proj_host[12]: row-major
 * 3x4 double matrix M that takes a homogeneous LiDAR point to the homogeneous pixel (KITTI: P2 [R0 0; 0 1] [Tr; 0 0 0 1];
 * CADC: the first three rows of K4 inv(T_LIDAR_CAM00); roi_data_layer/lidar_calib.py), entries finite; img_h, img_w > 0 =
 * cfg.<DB>.IMG_SIZE.  Per point, in double: h = M [x y z 1]^T, u = h0 / h2, v = h1 / h2 (the DIVISION, like the
 * reference), keep iff 0 <= u < img_w and 0 <= v < img_h.  No depth test, like the reference: a point behind the camera
 * whose quotient lands inside the frame is kept; h2 == 0 and NaN / Inf coordinates fail the comparisons (as in numpy) and
 * are dropped.  A rejected point keeps its row with x, y, z = NaN, columns 3.. untouched.  The draws of the later steps
 * stay indexed by the row in the FILE, so a frame's draws do not depend on how many points the filter removed:
 * the call equals the filter alone (flags 0) followed by frcnn_lidar_augment with the same flags, parameters and seed,
 * bit for bit, kept_count included.  kept_count keeps its meaning (survivors inside range_host after all steps).
 * No allocation, no host synchronisation; kernel launches only. */
int frcnn_lidar_augment_fov(const float* points, int num_points, int point_stride, const float* range_host, unsigned flags,
                            const float* params_host, uint32_t seed, const uint32_t* seed_dev, float* out, int* kept_count,
                            int max_blocks, const double* proj_host, int img_h, int img_w, void* stream);

/* Image augmentation (lib/roi_data_layer/minibatch.py:540-647), the pixel side of the imgaug block in front of
 * frcnn_prep_image: img / out are uint8 (h, w, 3) frames in cv2.imread order.  flip = 1 mirrors the frame left-right first
 * (:549; folded into the first stage's read).  Then num_stages <= FRCNN_IMG_MAX_STAGES stages run in the given order, one
 * launch each, every one uint8 -> uint8 (round half to even, clip); stage k reads stage_codes_host[k] and the
 * FRCNN_IMG_NUM_PARAMS floats at stage_params_host + k * FRCNN_IMG_NUM_PARAMS (unused slots 0):
 *   GAUSS    (:567)     [taps (5, 7 or 9), tap 0 .. tap taps-1]   separable, normalised taps computed by the caller
 *   AVERAGE  (:568)     [k (2 or 3)]                              k = 1 is the identity: do not pass it
 *   MEDIAN   (:569)     []                                        3x3; k = 1 is the identity
 *   SHARPEN  (:570)     [centre weight (1-a) + a(8+l), neighbour weight -a]
 *   NOISE    (:572-575) [scale]                                   normal01 streams 40, 41, 42 = channel 0, 1, 2; index = pixel
 *   HUE_SAT  (:576)     [hue offset on the 0..180 circle, saturation offset on 0..255]   memory channel 0 is taken as R
 *   AFFINE   (:579-586) [m0 .. m5 (output -> source: xs = m0 x + m1 y + m2, ys = m3 x + m4 y + m5), order (0 nearest,
 *                        1 bilinear), border value]
 *   DROPOUT  (:587)     [p, per_channel (0 / 1)]                  uniform01 stream 86; index = pixel, or pixel * 3 + channel
 * Draws are counter-based, value = f(seed + *seed_dev, stream, index) (csrc/rng.h; seed_dev device uint32 or NULL).
 * num_stages == 0: a (mirrored) copy.  scratch (frcnn_image_augment_ws_bytes(h, w) bytes, device) is the ping-pong buffer,
 * read only when num_stages > 1 (may be NULL otherwise).  img, out and scratch must not overlap one another: rejected.
 * Frame size: h, w > 0 and h * w <= 2^29.  A call that holds a stencil stage (GAUSS, AVERAGE, MEDIAN, SHARPEN) further
 * needs h <= 16 * 65535 = 1048560 (one row of workgroups per 16 frame rows, the rule of frcnn_image_spatter with its own
 * tile height): a taller frame is rejected with FRCNN_ERR_ARG before anything is launched.  Calls that hold only the
 * pointwise stages (flip / copy, NOISE, HUE_SAT, AFFINE, DROPOUT) take every admitted size.  The stencil borders are
 * true reflect-101 (replicate for MEDIAN) for every dimension >= 1, also those no larger than the halo.
 * debug_pre (device, h*w*3 floats, usually NULL): with exactly one NOISE or HUE_SAT stage, the values before rounding.
 * No allocation, no host synchronisation; kernel launches only, so a stream capture holds kernel nodes.
 * Operators restated from the published algorithms of imgaug / cv2 / scikit-image (absent: parity unpinned); the
 * conventions are listed in csrc/image_augment.hip. */
#define FRCNN_IMG_COPY 0
#define FRCNN_IMG_GAUSS 1
#define FRCNN_IMG_AVERAGE 2
#define FRCNN_IMG_MEDIAN 3
#define FRCNN_IMG_SHARPEN 4
#define FRCNN_IMG_NOISE 5
#define FRCNN_IMG_HUE_SAT 6
#define FRCNN_IMG_AFFINE 7
#define FRCNN_IMG_DROPOUT 8
#define FRCNN_IMG_MAX_STAGES 8
#define FRCNN_IMG_NUM_PARAMS 12
size_t frcnn_image_augment_ws_bytes(int h, int w);
int frcnn_image_augment(const uint8_t* img_hwc3, int h, int w, int flip, int num_stages, const int* stage_codes_host,
                        const float* stage_params_host, uint32_t seed, const uint32_t* seed_dev, void* scratch,
                        size_t scratch_bytes, uint8_t* out, float* debug_pre, void* stream);

/* Test-time Spatter corruption of a camera frame (lib/roi_data_layer/minibatch.py:648-664, iaa.imgcorruptlike.Spatter
 * behind cfg.TEST.AUGMENT_EN), mud branch of the published ImageNet-C operator, in front of frcnn_prep_image: img / out are
 * uint8 (h, w, 3) frames in cv2.imread order, one fused launch, no workspace.
 *   params_host: FRCNN_SPATTER_NUM_PARAMS floats [loc, scale, sigma1, thr, sigma2] (the operator's constants of a severity).
 *   taps1_host / taps2_host: the normalised Gaussian taps of sigma1 / sigma2, computed by the caller in double;
 *     num_taps = 2 * int(4 sigma + 0.5) + 1 (skimage's radius rule; anything else is rejected), at most
 *     FRCNN_SPATTER_MAX_TAPS1 / FRCNN_SPATTER_MAX_TAPS2, which is what the kernel's halo holds.
 *   liquid = loc + scale * normal01(seed + *seed_dev, stream 44, y * w + x)  (csrc/rng.h; seed_dev device uint32 or NULL)
 *   liquid = blur(liquid, taps1);  b = liquid > thr;  m = blur(b, taps2);  m = m < 0.8 ? 0 : m
 *   out[c] = (uint8) (clip(img[c] / 255 * (1 - m) + mud[c] * m, 0, 1) * 255), truncated; mud = (63, 42, 20) / 255 on memory
 *   channels 0, 1, 2 (the reference hands cv2's BGR frame to an RGB corruption: kept).  Blurs: separable, horizontal then
 *   vertical, fp32, border replicate.  A pixel with m = 0 leaves unchanged.
 * debug_liquid / debug_mask (device, h*w floats each, usually NULL): the field after the first blur, m before the 0.8 cut.
 * FRCNN_ERR_ARG: a null img / out / params / taps pointer, h or w below 1, a tap count above what the kernel holds (or even,
 * or off the radius rule), a non-finite number, out overlapping img.  No allocation, no host synchronisation; one kernel
 * launch.  Restated from the published algorithm (imgaug / imagecorruptions / scikit-image absent: parity unpinned); the
 * conventions are listed in csrc/image_spatter.hip. */
#define FRCNN_SPATTER_NUM_PARAMS 5
#define FRCNN_SPATTER_MAX_TAPS1 9
#define FRCNN_SPATTER_MAX_TAPS2 13
int frcnn_image_spatter(const uint8_t* img_hwc3, int h, int w, const float* params_host, const float* taps1_host, int num_taps1,
                        const float* taps2_host, int num_taps2, uint32_t seed, const uint32_t* seed_dev, uint8_t* out,
                        float* debug_liquid, float* debug_mask, void* stream);

/* Scoring of one class's detections file: the overlap and matching loop the three evaluators share
 * (lib/datasets/waymo_eval.py:131-213, kitti_eval.py:116-215, cadc_eval.py:115-206, and the iou helper of the missing
 * lib/utils/eval_utils.py as restated in datasets/waymo_eval.py), one launch, one workgroup per frame.
 * All arrays are device arrays grouped by frame (CSR): frame f owns detections det_offsets[f] .. det_offsets[f+1]-1, gt
 * boxes gt_offsets[f] .. and don't-care boxes dc_offsets[f] .. (offsets: num_frames + 1 ints, ascending, last = count).
 *   det_boxes (num_det, E) double, E = 4 for FRCNN_EVAL_2D ([x1,y1,x2,y2]) and 7 otherwise ([xc,yc,zc,l,w,h,ry]);
 *   det_rows  (num_det) the detection's rank in the confidence order among detections that have a record (the
 *             reference's idx counter), distinct, and ascending inside a frame;
 *   gt_boxes (num_gt, E) double, gt_ignore (num_gt) bytes, gt_difficulty (num_gt) ints;
 *   dc_boxes (num_dc, E) double; dc_boxes NULL or num_dc 0: don't-care boxes are not consulted (cfg.TEST.IGNORE_DC off).
 * Per detection: ovmax = the largest overlap with the frame's gt boxes (-inf without any), jmax = the FIRST index inside
 * the frame that attains it (np.argmax; 0 without gt), ovmax_dc = the largest overlap with the frame's don't-care boxes
 * (0 without any), det_difficulty = gt_difficulty of jmax for codes 1 and 2 (else -1), and code:
 *   FRCNN_EVAL_NONE    counts for nothing (candidate of an ignored gt; above the don't-care threshold; frame without gt)
 *   FRCNN_EVAL_TP      candidate (ovmax > ovthresh, ovmax_dc < ovthresh_dc) with the smallest row among its gt's candidates
 *   FRCNN_EVAL_DUP_FP  any other candidate of that gt: false positive at the levels of the gt's difficulty
 *   FRCNN_EVAL_FP      no candidate, ovmax_dc < ovthresh_dc, frame has gt: false positive at every level
 * Per gt box: hit = some candidate matched it (what the host loop leaves in rec['hit']).
 * Overlaps are computed in double, term for term as datasets/waymo_eval.py iou (cos / sin of ry are the device's).
 * Box values must be finite and, for the three LiDAR types, l, w, h > 0: the caller checks (datasets/device_eval.py).
 * Any number of boxes per frame; a frame with more than FRCNN_EVAL_LDS_GT gt boxes keeps its per-gt row minimum in ws:
 * pass max_gt_per_frame (the largest gt count of a frame) to both calls, ws_bytes() is 0 below that count.  Frames whose gt
 * count exceeds FRCNN_EVAL_LDS_GT although max_gt_per_frame said otherwise get code -1 and are not scored.
 * gt boxes pass through LDS FRCNN_EVAL_CHUNK at a time.  No allocation, no host synchronisation, one kernel launch. */
#define FRCNN_EVAL_2D 0
#define FRCNN_EVAL_BEV_AA 1
#define FRCNN_EVAL_BEV 2
#define FRCNN_EVAL_3D 3
#define FRCNN_EVAL_NONE 0
#define FRCNN_EVAL_TP 1
#define FRCNN_EVAL_DUP_FP 2
#define FRCNN_EVAL_FP 3
#define FRCNN_EVAL_CHUNK 64
#define FRCNN_EVAL_LDS_GT 2048
size_t frcnn_eval_match_ws_bytes(int num_gt, int max_gt_per_frame);
int frcnn_eval_match(const double* det_boxes, const int* det_rows, const int* det_offsets, int num_det,
                     const double* gt_boxes, const uint8_t* gt_ignore, const int* gt_difficulty, const int* gt_offsets,
                     int num_gt, const double* dc_boxes, const int* dc_offsets, int num_dc, int num_frames, int eval_type,
                     double ovthresh, double ovthresh_dc, int max_gt_per_frame, int* code, int* jmax, double* ovmax,
                     double* ovmax_dc, int* det_difficulty, uint8_t* hit, void* ws, size_t ws_bytes, void* stream);

/* COCO bbox matching of a whole results file: what COCOeval.evaluate() does for every (image, category) pair, the call
 * lib/datasets/coco.py:251-258 makes through pycocotools, as one launch (csrc/coco_match.hip; the protocol is restated in
 * datasets/coco_eval.py, parity against pycocotools unpinned).  One wavefront per pair, FRCNN_COCO_PAIRS_PER_WG pairs per
 * workgroup.  All arrays are device arrays; pair p owns detections det_offsets[p] .. det_offsets[p+1]-1, gt boxes
 * gt_offsets[p] .. and overlaps iou_offsets[p] .. (num_pairs + 1 entries each, ascending, last = count; iou_offsets is the
 * running sum of D * G and 64 bits wide).  Ordering is an input, the device never sorts:
 *   det (num_det, 5) double [x, y, w, h, area], a pair's detections in descending score order, cut to the largest maxDets;
 *   gt (num_gt, 5) double [x, y, w, h, area] in annotation order, gt_crowd (num_gt) bytes;
 *   iou_thrs (num_thr) double and area_rng (num_area, 2) double [lo, hi], as numpy made them.
 * Outputs, per pair:
 *   ious       D x G doubles, row = detection: iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise; 0 if iw <= 0 or ih <= 0, else
 *              iw*ih / (crowd ? dw*dh : dw*dh + gw*gh - iw*ih), each operation rounded once;
 *   gt_ignore  (num_gt, num_area) bytes: crowd, or area < lo, or area > hi;
 *   dt_match   (num_det, num_area, num_thr) ints: the matched box's index inside the pair in annotation order, or -1.
 *              Detections are walked in order; a detection starts from min(thr, 1 - 1e-10), visits the non-ignored boxes
 *              in annotation order and then, only if none of them matched, the ignored ones; a box that is already matched
 *              at this (area range, threshold) is skipped unless it is crowd; a box whose overlap is below the best so far
 *              is skipped, so an overlap equal to the threshold matches and of two equal overlaps the later box wins;
 *   dt_ignore  (num_det, num_area, num_thr) bytes: the matched box's ignore byte, or, unmatched, area < lo or area > hi.
 * Overlaps stay in LDS while D * G <= FRCNN_COCO_LDS_IOUS and are read back from `ious` above that; the per-walk matched
 * set is a register mask up to FRCNN_COCO_MASK_GT boxes and bytes in ws above that: pass max_gt_per_pair (the largest gt
 * count of a pair) to both calls, ws_bytes() is 0 up to that count.  A pair with more boxes than max_gt_per_pair allowed
 * for gets dt_match -2 and is not scored; a pair whose offsets leave no room in `ious` is not written at all.
 * FRCNN_ERR_ARG: a negative count, num_thr or num_area below 1, a null required pointer.  num_pairs == 0 returns without
 * a launch.  No allocation, no host synchronisation, one kernel launch. */
#define FRCNN_COCO_PAIRS_PER_WG 4
#define FRCNN_COCO_LDS_IOUS 1024
#define FRCNN_COCO_MASK_GT 64
size_t frcnn_coco_match_ws_bytes(int num_gt, int max_gt_per_pair, int num_area, int num_thr);
int frcnn_coco_match(const double* det, const int* det_offsets, int num_det, const double* gt, const uint8_t* gt_crowd,
                     const int* gt_offsets, int num_gt, const int64_t* iou_offsets, int64_t num_iou, int num_pairs,
                     const double* iou_thrs, int num_thr, const double* area_rng, int num_area, int max_gt_per_pair,
                     double* ious, int* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, void* ws, size_t ws_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training path (BASELINE config 4: FPN forward + backward of one train_step, lib/model/train_val.py:458)
 * ------------------------------------------------------------------------------------------- */
/* Backward of act(conv*scale + shift + residual): dz = relu ? (y > 0 ? dy : 0) : dy; d_res = dz (may be NULL);
 * d_conv = dz * scale[k] (scale may be NULL).  rows x k fp32, k % 4 == 0.  (F.relu / frozen BatchNorm / the
 * residual add of lib/nets/resnet.py:98-127.) */
int frcnn_act_bwd(const float* dy, const float* y, const float* scale, int relu, int64_t rows, int k,
                  float* d_conv, float* d_res, void* stream);

/* BatchNorm2d with BATCH statistics (module in train() mode; the LiDAR backbone trains layer2/layer3 this way,
 * lib/nets/lidarnet.py:110,152-175; torch.nn.functional.batch_norm(training=True)).  y/out/residual/dout/dy/dres are
 * rows x c fp32 (NHWC activations), c % 4 == 0.
 *   fwd: mean/biased var over the rows -> save_mean, save_invstd = 1/sqrt(var+eps);
 *        out = act((y - mean)*alpha + beta [+ residual]), alpha = gamma*invstd (gamma/beta may be NULL = 1/0);
 *        running_mean/var (may be NULL) <- (1-momentum)*running + momentum*(mean | UNBIASED var).
 *   bwd: g = relu ? (out > 0 ? dout : 0) : dout; dbeta = sum g; dgamma = sum g*xhat;
 *        dy = gamma*invstd*(g - dbeta/rows - xhat*dgamma/rows); dres = g (may be NULL).
 *        accumulate != 0: dgamma / dbeta are the parameters' own gradient buffers and are added into.
 * Column sums are carried in fp64 and added in a fixed order; the summand g*xhat of dgamma is formed in fp64 too
 * (dy's own xhat is fp32).
 * counters: frcnn_bn_train_counters(c) ints, zero on entry and left zero, not shared by launches that can be in flight
 * together (the rule of frcnn_conv2d_bwd_weight's counters): the last workgroup of a 64-channel column block turns the column
 * sums into the statistics / coefficients itself - two launches per call instead of three.  NULL: a separate pass does. */
size_t frcnn_bn_train_ws_bytes(int c);
int frcnn_bn_train_counters(int c);
int frcnn_bn_train_fwd(const float* y, int64_t rows, int c, const float* gamma, const float* beta, float eps,
                       float momentum, float* running_mean, float* running_var, const float* residual, int relu,
                       float* out, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, int* counters,
                       void* stream);
int frcnn_bn_train_bwd(const float* dout, const float* out, const float* y, int64_t rows, int c, const float* gamma,
                       const float* save_mean, const float* save_invstd, int relu, float* dy, float* dres,
                       float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, int* counters,
                       void* stream);

/* fc7 = x.mean(3).mean(2) (_head_to_tail of the non-FPN detector; x (rows,P,P,c) NHWC -> out (rows,c)) and its
 * backward dx = dout / P^2 broadcast over the P x P positions. */
int frcnn_spatial_mean_fwd(const float* x, float* out, int rows, int pooled, int c, void* stream);
int frcnn_spatial_mean_bwd(const float* dout, float* dx, int rows, int pooled, int c, void* stream);

/* fpn._upsample_add (lib/nets/fpn.py:42-45): out (n,out_h,out_w,c) = F.interpolate(x (n,h,w,c), size=(out_h,out_w),
 * mode='bilinear', align_corners=False) + lateral.  Backward: dx = interpolate^T(dout) (deterministic gather);
 * the gradient of `lateral` is dout itself.  The top-down path only enlarges (c5 -> c4 -> c3 -> c2 maps): out_h < h or
 * out_w < w is rejected by both entry points. */
int frcnn_upsample_bilinear_add_fwd(const float* x, const float* lateral, float* out, int n, int h, int w,
                                    int out_h, int out_w, int c, void* stream);
int frcnn_upsample_bilinear_bwd(const float* dout, float* dx, int n, int h, int w, int out_h, int out_w, int c,
                                void* stream);

/* Backward of frcnn_roi_align_fwd: dfeat (1,H,W,C) += scatter(dout (R,P,P,C)); dfeat must be zero-filled by the
 * caller (float atomics: the summation order, hence the last bits, vary from run to run; the same holds for
 * frcnn_roi_align_bwd_planned and frcnn_scatter_add_patches - every other kernel of the library is deterministic). */
int frcnn_roi_align_bwd(const float* dout, int h, int w, int c, const float* rois, const int* roi_count,
                        int num_rois, int pooled, float spatial_scale, int sampling_ratio, const int* level_of_roi,
                        int level, float* dfeat, void* stream);
/* The same gradient through the forward's plan (frcnn_roi_align_fwd_ws_bytes of the shape as workspace; pooled 7, c % 4 == 0):
 * the row bins of a window row are folded in registers first, so ONE atomic is issued per (RoI, window pixel of a column bin,
 * channel) instead of four per sample - 2.5x (2x2 samples per bin) to 10x+ (larger adaptive grids) fewer atomics.  Same sums
 * in another order (float atomics either way). */
int frcnn_roi_align_bwd_planned(const float* dout, int h, int w, int c, const float* rois, const int* roi_count,
                                int num_rois, int pooled, float spatial_scale, int sampling_ratio, const int* level_of_roi,
                                int level, float* dfeat, void* ws, size_t ws_bytes, void* stream);

/* The RPN losses read only the anchors the anchor target layer labelled (<= cfg.TRAIN.RPN_BATCHSIZE,
 * lib/layer_utils/anchor_target_layer.py:91-107), so the gradient of the RPN head is non-zero on at most that many pixels.
 * frcnn_labelled_pixels: labels (hw * A) in (H,W,A) order -> idx[cap] = the pixels with a label != -1, ascending, -1 beyond
 * count[0]; count[0] = min(total, cap), count[1] = total (a caller checks count[1] <= cap where the labels are not its own).
 * frcnn_gather_patches: out (cap, r, s, c) = the r x s window of x (h, w, c) around each listed pixel (zero outside the map and
 * for rows >= count[0]) - the input of a VALID r x s convolution that reproduces the padded convolution at those pixels
 * (lib/nets/network.py rpn_net on net_conv).  frcnn_scatter_add_patches: its adjoint, dx += scatter(d) with float atomics. */
size_t frcnn_labelled_pixels_ws_bytes(int hw);
int frcnn_labelled_pixels(const float* labels, int hw, int num_anchors, int cap, int64_t* idx, int* count, void* ws,
                          size_t ws_bytes, void* stream);
int frcnn_gather_patches(const float* x, int h, int w, int c, const int64_t* idx, const int* count, int cap, int r, int s,
                         int pad, float* out, void* stream);
int frcnn_scatter_add_patches(const float* d, int h, int w, int c, const int64_t* idx, const int* count, int cap, int r, int s,
                              int pad, float* dx, void* stream);

/* RPN losses on the fused head output rpn (hw, ld) = [A bg | A fg | 4A deltas | pad]:
 *   losses[0] = F.cross_entropy over anchors with labels != -1 (mean), losses[1] = smooth_l1_loss('RPN', ...,
 *   dim=[1,2,3]) (lib/utils/loss_utils.py:39-101), losses[2] = number of labelled anchors.
 * labels (hw*A) in (H,W,A) order with values -1/0/1; targets/inside/outside (hw*A, 4).
 * drpn (hw, ld), may be NULL: gradient of grad_ce*losses[0] + grad_box*losses[1]. */
size_t frcnn_rpn_loss_ws_bytes(void);
int frcnn_rpn_loss(const float* rpn, int ld, int num_anchors, int hw, const float* labels, const float* targets,
                   const float* inside, const float* outside, float grad_ce, float grad_box, float* losses,
                   float* drpn, void* ws, size_t ws_bytes, void* stream);

/* Detection losses on the sampled RoIs: losses[0] = F.cross_entropy(cls_score (R,K), labels (R) as floats),
 * losses[1] = smooth_l1_loss('DET', bbox_pred (R,E*K), targets, inside, outside) (image boxes);
 * dcls / dbox (may be NULL): gradients of grad_ce*losses[0] + grad_box*losses[1]. */
int frcnn_det_loss(const float* cls_score, const float* labels, int num_rois, int num_classes,
                   const float* bbox_pred, const float* targets, const float* inside, const float* outside,
                   int bbox_elem, float grad_ce, float grad_box, float* losses, float* dcls, float* dbox,
                   void* stream);

/* bbox_overlaps (lib/utils/bbox.py:5-33): IoU with the +1 area convention; boxes (n rows of box_ld floats, first
 * 4 = [x1,y1,x2,y2]) x query (k rows of query_ld floats) -> overlaps (n,k). */
int frcnn_bbox_overlaps(const float* boxes, int box_ld, int n, const float* query, int query_ld, int k,
                        float* overlaps, void* stream);

/* bbox_transform (lib/model/bbox_transform.py:52-70): regression targets of gt_rois against ex_rois, row by row
 * (n rows of ex_ld / gt_ld floats, first 4 = [x1,y1,x2,y2]) -> targets (n,4) [dx,dy,dw,dh]; dx,dy over the box
 * DIAGONAL, widths with the +1 convention. */
int frcnn_bbox_transform(const float* ex_rois, int ex_ld, const float* gt_rois, int gt_ld, int n, float* targets,
                         void* stream);

/* lidar_3d_bbox_transform (lib/model/bbox_transform.py:16-49): ex_rois (n rows, first 4 = BEV [x1,y1,x2,y2]),
 * ex_anchors_3d (n,7), gt_rois (n rows of gt_ld >= 7 floats [xc,yc,zc,l,w,h,ry]) -> targets (n,7). */
int frcnn_lidar_bbox_transform(const float* ex_rois, int roi_ld, const float* ex_anchors_3d, const float* gt_rois,
                               int gt_ld, int n, float* targets, void* stream);

/* anchor_target_layer_torch (lib/layer_utils/anchor_target_layer.py:22-165; IGNORE_DC off, CLOBBER_POSITIVES off,
 * uniform example weights): anchors (n,4) in (H,W,A) order, gt_boxes (num_gt,5) [x1,y1,x2,y2,cls], info HOST
 * [x_min,x_max,y_min,y_max].  Outputs in anchor order: labels (n) in {-1,0,1}, targets/inside/outside (n,4);
 * counts (2 ints, may be NULL) = fg / bg candidates before sub-sampling.  Sub-sampling to
 * fg_fraction*rpn_batchsize foreground and rpn_batchsize total draws hash keys from `seed` + *seed_dev (seed_dev: device
 * uint32, may be NULL - a launch replayed from a hipGraph keeps its `seed` argument, so per-step seeds come through
 * device memory the caller rewrites before each replay; same for the proposal target layers below). */
size_t frcnn_anchor_target_layer_ws_bytes(int num_anchors_total, int num_gt, int rpn_batchsize);
int frcnn_anchor_target_layer(const float* anchors, int n, const float* gt_boxes, int num_gt,
                              const int* num_gt_dev /* device int or NULL: live rows of a gt buffer padded to num_gt rows
                              (one captured training step serves every number of gt boxes).  REQUIRED: 1 <= *num_gt_dev <=
                              num_gt - the kernels clamp the value into that range, so a 0 would make row 0 of the buffer a
                              ground-truth box; a frame without gt boxes must not be launched (the reference stops on it too,
                              lib/layer_utils/proposal_target_layer.py:232-235) */,
                              const float* info_host, int rpn_batchsize, float fg_fraction, float negative_overlap,
                              float positive_overlap, uint32_t seed, const uint32_t* seed_dev, float* labels,
                              float* targets, float* inside, float* outside, int* counts, void* ws, size_t ws_bytes,
                              void* stream);

/* proposal_target_layer (lib/layer_utils/proposal_target_layer.py:22-262, image detector, USE_GT / IGNORE_DC off):
 * rois (num_rois,5), roi_scores (num_rois) or NULL, roi_count device int or NULL, gt_boxes (num_gt,5).
 * Outputs with rois_per_frame rows (foreground rows first): labels, out_rois (.,5), out_scores, targets / inside /
 * outside (., 4*num_classes; targets normalised with means/stds, HOST 4 floats each), gt_assignment (.) ints,
 * counts[4] = {fg rows, bg rows, fg candidates, bg candidates}.  num_rois <= 4096.
 * skip_mask (num_rois bytes, may be NULL): rows with a non-zero byte are no candidates (TRAIN.IGNORE_DC: proposals whose
 * overlap with a don't-care box reaches DC_THRESH, proposal_target_layer.py:180-191). */
int frcnn_proposal_target_layer(const float* rois, const float* roi_scores, const int* roi_count, int num_rois,
                                const float* gt_boxes, int num_gt, const int* num_gt_dev /* as above */, int num_classes,
                                int rois_per_frame,
                                float fg_fraction, float fg_thresh, float bg_thresh_hi, float bg_thresh_lo,
                                const float* means_host, const float* stds_host, uint32_t seed, const uint32_t* seed_dev,
                                float* labels, float* out_rois, float* out_scores, float* targets, float* inside,
                                float* outside, int* gt_assignment, int* counts, const unsigned char* skip_mask,
                                void* stream);

/* LiDAR form (proposal_target_layer.py:142-154, NET_TYPE 'lidar'): overlaps and labels on the BEV rectangles gt_boxes
 * (num_gt,5); targets = lidar_3d_bbox_transform(roi, the RoI's 3-D anchor, true_gt_boxes (num_gt,8)
 * [xc,yc,zc,l,w,h,ry,cls]) (lib/model/bbox_transform.py:16-49) normalised with 7 means/stds; anchors3d (num_rois,7)
 * follows the RoIs, out_anchors3d (rois_per_frame,7) the sampled rows; targets/inside/outside are (.,7*num_classes). */
int frcnn_proposal_target_layer_lidar(const float* rois, const float* roi_scores, const int* roi_count, int num_rois,
                                      const float* anchors3d, const float* gt_boxes, const float* true_gt_boxes,
                                      int num_gt, const int* num_gt_dev, int num_classes, int rois_per_frame,
                                      float fg_fraction, float fg_thresh, float bg_thresh_hi, float bg_thresh_lo,
                                      const float* means_host,
                                      const float* stds_host, uint32_t seed, const uint32_t* seed_dev, float* labels,
                                      float* out_rois, float* out_scores, float* out_anchors3d, float* targets, float* inside,
                                      float* outside, int* gt_assignment, int* counts, const unsigned char* skip_mask,
                                      void* stream);

/* frcnn_det_loss for the 7-element LiDAR boxes (lib/utils/loss_utils.py:61-77): the yaw difference goes through
 * sin() before the Huber term when ry_sin (cfg.LIDAR.EN_RY_SIN), every element is scaled by reg_loss_weight_host[7]
 * (cfg.LIDAR.REG_LOSS_WEIGHT, NULL = ones). */
int frcnn_det_loss_lidar(const float* cls_score, const float* labels, int num_rois, int num_classes,
                         const float* bbox_pred, const float* targets, const float* inside, const float* outside,
                         const float* reg_loss_weight_host, int ry_sin, float grad_ce, float grad_box, float* losses,
                         float* dcls, float* dbox, void* stream);

/* Uncertainty pieces whose arithmetic IS in the reference snapshot (lib/utils/loss_utils.py):
 *  - frcnn_det_loss with the aleatoric attenuation of loss_utils.py:82-85: bbox_var = predicted log-variance s,
 *    per-element loss (0.5*huber*exp(-s) + 0.5*s)*inside; dvar receives d(loss)/ds.  bbox_elem 4 or 7
 *    (7: sin(ry) + reg_loss_weight_host as in frcnn_det_loss_lidar).
 *  - frcnn_mc_bbox_var: samples (T, elems) -> unbiased variance over the T stochastic passes, clamped at 0
 *    (compute_bbox_var, loss_utils.py:114-120).
 *  - frcnn_mc_cls_stats: cls_score samples (T, num_rois, K) -> mean softmax (num_rois,K), its entropy in bits and the
 *    mutual information H(mean p) - mean H(p) (loss_utils.py:122-141). */
int frcnn_det_loss_aleatoric(const float* cls_score, const float* labels, int num_rois, int num_classes,
                             const float* bbox_pred, const float* bbox_var, const float* targets, const float* inside,
                             const float* outside, int bbox_elem, const float* reg_loss_weight_host, int ry_sin,
                             float grad_ce, float grad_box, float* losses, float* dcls, float* dbox, float* dvar,
                             void* stream);
int frcnn_mc_bbox_var(const float* samples, int num_samples, int64_t elems, float* var, void* stream);
int frcnn_mc_cls_stats(const float* cls_score_samples, int num_samples, int num_rois, int num_classes,
                       float* mean_prob, float* entropy, float* mutual_info, float* prob_var /* (num_rois,K) or NULL:
                       compute_bbox_var of the softmax samples */, void* stream);
/* mean over the T leading samples of a (T, elems) stack (mean logits / mean deltas of the Monte-Carlo passes). */
int frcnn_mc_mean(const float* samples, int num_samples, int64_t elems, float* mean, void* stream);

/* Uncertainty heads (rebuilt from the module names and rates of lib/nets/imagenet.py:52-91 / lidarnet.py:56-102; wiring
 * choices are named constants in nets/network.py).  Random draws are counter-based, value = f(seed, stream_id, index)
 * (csrc/rng.h), so the CPU oracle replays them:
 *  - frcnn_dropout_fwd: nn.Dropout(p) in train() mode on `repeat` stochastic copies of x (elems): y (repeat, elems);
 *    repeat = cfg.UC.E_NUM_SAMPLE starts the Monte-Carlo passes (lib/model/test.py:74-77) from one activation.
 *  - frcnn_dropout_bwd: dx (elems) = sum over the copies of mask * dy / (1 - p).
 *  - frcnn_logit_distort: logit_distort of loss_utils.py:143-147, samples (S, elems) = score + sqrt(var) * N(0,1).
 *  - frcnn_bayesian_cross_entropy: loss_utils.py:149-169 on the same draws: loss[0] = mean over RoIs of
 *    -log(mean_s softmax(score + sqrt(var) eps_s)[label]); per_roi (num_rois) scratch/diagnostic; dscore / dvar
 *    (num_rois, K, may be NULL) receive grad * d loss / d{score, var}.
 *  `seed_dev` (device uint32, may be NULL): the draws use seed + *seed_dev - a launch replayed from a hipGraph keeps its
 *  scalar `seed`, so the per-frame seed of a captured frame / training step comes through device memory (version 107). */
int frcnn_dropout_fwd(const float* x, int64_t elems, int repeat, float p, uint32_t seed, const uint32_t* seed_dev,
                      uint32_t stream_id, float* y, void* stream);
int frcnn_dropout_bwd(const float* dy, int64_t elems, int repeat, float p, uint32_t seed, const uint32_t* seed_dev,
                      uint32_t stream_id, float* dx, void* stream);
int frcnn_logit_distort(const float* score, const float* var, int64_t elems, int num_samples, uint32_t seed,
                        const uint32_t* seed_dev, uint32_t stream_id, int var_is_log /* var holds log-variances */,
                        float* samples, float* var_out /* (elems) exp(var) or var; may be NULL */, void* stream);
int frcnn_bayesian_cross_entropy(const float* cls_score, const float* cls_var, const float* labels, int num_rois,
                                 int num_classes, int num_samples, uint32_t seed, const uint32_t* seed_dev,
                                 uint32_t stream_id, int var_is_log, float grad, float* loss, float* per_roi,
                                 float* dscore, float* dvar, void* stream);
/* The same loss (loss_utils.py:149-169), arguments and draws for 2 <= num_classes <= 1024 (version 124): one wavefront
 * per RoI, lane l owning classes l, l + 64, ...  eps[s][n][k] = normal01(seed + *seed_dev, stream_id, (s*N + n)*K + k)
 * as above.  Every sum keeps the operand order of frcnn_bayesian_cross_entropy (softmax denominator in class order,
 * avg / gradient sums in sample order), so the result does not depend on the launch geometry and equals the entry above
 * wherever both accept num_classes.  No atomics, no workspace; dscore / dvar may be NULL; var == 0 with var_is_log == 0
 * gives dvar = 0.  The host chooses the form (ops.bayes_ce_uses_wide_form: num_classes > 16). */
int frcnn_bayesian_cross_entropy_wide(const float* cls_score, const float* cls_var, const float* labels, int num_rois,
                                      int num_classes, int num_samples, uint32_t seed, const uint32_t* seed_dev,
                                      uint32_t stream_id, int var_is_log, float grad, float* loss, float* per_roi,
                                      float* dscore, float* dvar, void* stream);
/* y = exp(x) elementwise (log-variance heads -> variances at test time). */
int frcnn_exp(const float* x, int64_t elems, float* y, void* stream);

/* LiDAR form (filter_predictions.py:55-62,67, db_type 'lidar'): no clamp, NMS on the yaw-less BEV rectangle
 * xc -+ l/2, yc -+ w/2 of the 7-DoF boxes, dets (K, max_out, 8) [xc,yc,zc,l,w,h,ry,score].
 * Workspace: frcnn_filter_per_class_ws_bytes. */
int frcnn_filter_per_class_lidar(const float* pred_boxes, const float* cls_prob, const int* roi_count,
                                 int num_rois, int num_classes, float thresh, float nms_thresh, int max_dets,
                                 int max_out, float* dets, int* det_count, int* det_roi, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rotated BEV NMS (version 115, opt-in: cfg.TEST.NMS_ROTATED).  The reference suppresses LiDAR detections on the yaw-less
 * rectangle (lib/utils/filter_predictions.py:55-67); its authors left the rotated form commented out at :56-57 ("Turned
 * off auto rotating").  These entries are that form, stated exactly:
 *   boxes are [xc,yc,zc,l,w,h,ry] float32 rows in (score descending, RoI index ascending) order, widened to float64;
 *   for i < j  iou(i, j) = datasets/waymo_eval.iou(bbgt = box_i[None], bb = box_j, 'bev')  - box j's rotated footprint
 *   clipped against box i's (the argument order is part of the contract), over l*w + l*w - intersection, in float64
 *   with one rounding per operation;
 *   box j is removed when a KEPT i < j has iou >= (double)thresh (frcnn_nms_set_suppress_at_equal(1), the default) or
 *   iou > (double)thresh (0).  A NaN overlap never suppresses.
 * thresh <= 0 (or NaN) is refused with FRCNN_ERR_ARG: disjoint boxes have IoU 0 and would suppress each other.
 * Three kernel launches on `stream`, sized by n_max / num_rois; the live counts are read on the device; no host
 * synchronisation, no memset / memcpy nodes: the calls capture into a hipGraph.
 *
 * frcnn_nms_rotated: boxes7 (n_max, 7) already in descending score order, n_dev (device int, may be NULL -> n_max) live.
 * Outputs as frcnn_nms: keep_idx[max_keep] int64 positions of the survivors in score order (entries past keep_count are
 * written as 0), keep_mask[n_max] bytes (may be NULL; 1 for the survivors counted in keep_count), keep_count[0] =
 * min(#survivors, max_keep).  n_max <= 4096, larger is FRCNN_ERR_ARG. */
size_t frcnn_nms_rotated_ws_bytes(int n_max);
int frcnn_nms_rotated(const float* boxes7, const int* n_dev, int n_max, float thresh, int max_keep, int64_t* keep_idx,
                      uint8_t* keep_mask, int* keep_count, void* ws, size_t ws_bytes, void* stream);

/* frcnn_filter_per_class_lidar with the rotated rule in place of filter_predictions.py:55-67's yaw-less one (the
 * commented-out :56-57): same arguments, same outputs - score threshold, order, the max_dets cut with ties
 * (lib/model/test.py:213-221), zero rows past det_count, det_roi -1 there, empty class 0, boxes not clamped.
 * num_rois <= 1024 (the reference uses 300), larger is FRCNN_ERR_ARG.  Workspace: frcnn_filter_per_class_lidar_rot_ws_bytes. */
size_t frcnn_filter_per_class_lidar_rot_ws_bytes(int num_rois, int num_classes);
int frcnn_filter_per_class_lidar_rot(const float* pred_boxes, const float* cls_prob, const int* roi_count, int num_rois,
                                     int num_classes, float thresh, float nms_thresh, int max_dets, int max_out,
                                     float* dets, int* det_count, int* det_roi, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The solver's weight update (lib/model/train_val.py:207-208 torch.optim.SGD(params, momentum=cfg.TRAIN.MOMENTUM) with one
 * param group per parameter, :379-382 the step that ends a pseudo batch; version 114): gradient clip, weight decay,
 * momentum, step and the clearing of the gradients for ALL trainable parameters of a network in ONE launch.
 *   grad_flat, momentum_flat   two flat fp32 device buffers of flat_elems elements with the same layout (the gradients of
 *                              model/train_val.GradientBucket and the momentum buffers next to them); they must not overlap;
 *   segments_dev               device table, one row per parameter: where the parameter lives, where its gradient /
 *                              momentum start in the flat buffers (in elements), how many elements, its learning rate and
 *                              weight decay.  segments_host is a HOST copy of the same rows: every argument check is made
 *                              on it, without a host synchronisation (the caller keeps the two equal);
 *   chunks_dev                 device table of num_chunks (segment, chunk) int pairs: workgroup i updates elements
 *                              chunk * FRCNN_SGD_CHUNK .. of that segment.  Every segment contributes
 *                              ceil(count / FRCNN_SGD_CHUNK) rows, in any order; num_chunks is checked against that sum;
 *   momentum                   torch.optim.SGD's momentum (dampening 0, no Nesterov); the momentum buffers start at zero;
 *   clip                       per-element clamp of the gradient to [-clip, +clip] first; <= 0 or +inf: no clip;
 *   zero_grads                 1: every gradient word is left as +0.0; 0: the (clipped) gradient is left in place.
 * Per element, torch's operations in torch's order, each rounded once (no fma):
 *   g = clamp(g, -clip, clip) (NaN stays NaN);  d = g + wd * p (skipped when wd == 0);  b = b * momentum + d;
 *   p = p + (-lr) * b.
 * Segments may start at any element offset and parameters at any float-aligned address.  Zero segments: nothing is
 * launched, returns FRCNN_OK.  Every kernel argument is a pointer or a launch-invariant scalar (learning rates and weight
 * decays live in the device table).  No allocation, no host synchronisation, one kernel launch. */
#define FRCNN_SGD_CHUNK 4096
typedef struct frcnn_sgd_segment {
  float* param;        /* device pointer of the parameter's first element */
  int64_t offset;      /* first element of its gradient / momentum in the flat buffers */
  int64_t count;       /* elements */
  float lr;
  float weight_decay;
} frcnn_sgd_segment;
int frcnn_sgd_update(float* grad_flat, float* momentum_flat, int64_t flat_elems, const frcnn_sgd_segment* segments_dev,
                     const frcnn_sgd_segment* segments_host, int num_segments, const int* chunks_dev, int64_t num_chunks,
                     float momentum, float clip, int zero_grads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Drawing a frame's detections (version 126; model/test.test_net(draw_det=True), model/draw.render_frame).  Replaces the
 * Pillow / numpy drawing of the reference's draw_and_save_eval (lib/datasets/waymo_imdb.py:190-253, waymo_lidb.py:229-328,
 * kitti_lidb.py:289-378) called at lib/model/test.py:231-242.  Every value that decides a byte is formed in float64 or in
 * integers, one rounding per operation: the outputs are pure functions of the inputs (tests/draw_restatement.py restates
 * them in numpy, bit for bit).  Launches on `stream` only: no host synchronisation, no float atomics, no memset / memcpy
 * nodes - a stream capture holds kernel nodes only.
 *
 * frcnn_canvas_from_image_blob (waymo_imdb.py:200-204): blob (1, height, width, 3) fp32 -> canvas (height, width, 3) uint8,
 *   canvas[y][x][o] = byte((double)blob[y][x][c] * stds_host[c] + means_host[c]) with c = arrange_host[o]
 *   (cfg.PIXEL_STDDEVS, cfg.PIXEL_MEANS, cfg.PIXEL_ARRANGE_BGR).  byte() truncates toward zero like astype(uint8)
 *   (254.99999 -> 254) and - a stated deviation, numpy's out-of-range cast being undefined - saturates to [0, 255], NaN -> 0.
 *
 * frcnn_canvas_from_bev_blob: blob (1, ny, nx, channels) fp32 BEV voxel grid (num_slices height slices, then density, then
 *   intensity) -> canvas (ny, nx, 3) uint8.  The blob is only read.  With height(cell) = max over the slices:
 *   FRCNN_DRAW_BEV_KITTI (kitti_lidb.py:289-297, also CADC's): R = height * (255 / (max height - min height)),
 *     G = density * (255 / max density), B = intensity * (255 / max intensity);
 *   FRCNN_DRAW_BEV_WAYMO (waymo_lidb.py:240-261): slice i of a cell counts as v + i*0.5 where |v| > 1e-5 (formed on the fly:
 *     the reference adds it to the blob in place), mask = |height| > 1e-5, max = 1.5 * max(mask * height),
 *     min = min(mask * height), R = mask * height * (255 / (max - min)), G = density * (6*255 / max density),
 *     B = intensity * (2*255 / max intensity).
 *   Three launches: per-workgroup extrema, their finish (the three factors), the colouring; extrema do not depend on the
 *   order of reduction.  A NaN slice is ignored by the extrema.  Stated deviations: a channel whose range is empty
 *   (max == min, or max == 0) is written as 0 (the reference divides by zero); values are saturated to [0, 255] before
 *   the cast (the reference's green channel reaches 1530 and relies on an undefined cast); the arithmetic is float64
 *   throughout (the reference mixes float32 and float64 by numpy's promotion rules of the day).
 *   Workspace: frcnn_canvas_from_bev_blob_ws_bytes(), 8-byte aligned.
 *
 * frcnn_draw_plan: the device record of a frame -> a draw list in painter's order.  dets (num_classes, max_out, elem) fp32
 *   rows [x1,y1,x2,y2,score,uncertainty...] (lidar == 0) or [xc,yc,zc,l,w,h,ry,score,uncertainty...] in voxel-grid units
 *   (lidar != 0), counts (num_classes) int32, as frcnn_filter_per_class* and frcnn_uncertainty_columns leave them;
 *   gt (num_gt, 4 or 7) fp32 with gt_labels (num_gt) int32 (may be NULL with num_gt == 0).  rows: `capacity` >=
 *   (num_classes - 1) * max_out + num_gt rows of FRCNN_DRAW_ROW_INTS int32:
 *     [kind, line width, sequence number, r | g << 8 | b << 16, g0 .. g7]
 *   FRCNN_DRAW_RECT: g0..g3 = x0,y0,x1,y1 (the float corners truncated toward zero as Pillow's ImageDraw.rectangle
 *   converts them, pinned to +-2^30); FRCNN_DRAW_FOOTPRINT: g0..g7 = x,y of the four corners of bbox_3d_to_bev_4pt /
 *   rotate_in_bev (lib/utils/bbox.py:174-233; float64, rounded to float32 like rotate_in_bev's result), clipped to
 *   [0, canvas_w - 1] x [0, canvas_h - 1] and truncated (draw_bev_bboxes, :346-351); FRCNN_DRAW_SKIP: nothing is drawn
 *   (a row with a NaN coordinate, and every row behind the last one).  Row i has sequence number i.
 *   Order: image frames - per class j >= 1 its detections, then the ground truth (waymo_imdb.py:211-251); LiDAR frames -
 *   the ground truth, then the detections (waymo_lidb.py:268-302).  Inside a class the detections are ordered by
 *   np.argsort(-key) (db.py:283-303), key = mean of the row's columns key_col .. key_col + key_cols - 1 (fp32 sum in
 *   column order / count: _normalize_uncertainties, :260-281); key_cols == 0: key = row index, i.e. reverse row order.
 *   NaN keys last; ties go to the lower row (numpy's default argsort is not stable: the tie rule is this library's).
 *   Colours: detections (0, (int)(score * 255.0f), (int)((limiter - i) / limiter * 255.0)), i the position in the class's
 *   order, limiter starting at limiter0 and carried from class to class: a class with 0 < n < limiter detections sets
 *   limiter = n, any other non-empty class resets it to limiter0 when limiter_resets != 0 (waymo_imdb.py:220-223) and
 *   leaves it otherwise (waymo_lidb.py:294-295); each component clamped to [0, 255] like Pillow; width 2.  Ground truth:
 *   image 0 / 255 for label 0 / other, width 1 (waymo_imdb.py:246-251); LiDAR 127 / 255, width 2 (waymo_lidb.py:277-282).
 *   max_out <= 4096.  One launch.
 *
 * frcnn_draw_scatter: owner (height, width) uint32 is cleared by the library's fill kernel, then every outline pixel of row
 *   i does atomicMax(owner, i + 1): exact painter's order whatever the scheduling.
 *     FRCNN_DRAW_RECT of width w: the pixels of [x0,x1] x [y0,y1] within w pixels of the rectangle's border, clipped to
 *     the canvas; empty when x1 < x0 or y1 < y0.  For boxes at least 2w wide and high this is Pillow's
 *     ImageDraw.rectangle(outline=, width=w); for thinner and degenerate boxes Pillow has quirks (a zero-size box of
 *     width 2 paints 3x4 pixels) and this rule stands.
 *     FRCNN_DRAW_FOOTPRINT: the four edges corner i -> corner i-1 (draw_polygon, lib/utils/bbox.py:364-379).  With
 *     dx = |xb - xa|, dy = |yb - ya|, x the major axis iff dx > dy: for t = 0..dmaj the pixel major_a + s_major * t,
 *     minor_a + s_minor * ((2*t*dmin + dmaj) / (2*dmaj)) in integer division (a zero-length edge: its one pixel) - the
 *     closed form of Pillow's ImageDraw.line(width=1), equal to it pixel for pixel in all eight octants
 *     (tests/test_draw_host.py).  Width 2 also paints the neighbour at +1 along the minor axis, clipped (width w: the
 *     neighbours at +1 .. +w-1; a footprint row with w > 16 or a corner beyond +-2^20 is not drawn).  PARITY
 *     UNPINNED for width 2: the reference asks Pillow for width=2 lines, which Pillow fills as polygons.
 * frcnn_draw_compose: canvas[pixel] = rgb of row owner - 1 where owner != 0.  rows / num_rows as given to
 *   frcnn_draw_scatter. */
#define FRCNN_DRAW_ROW_INTS 12
#define FRCNN_DRAW_SKIP 0
#define FRCNN_DRAW_RECT 1
#define FRCNN_DRAW_FOOTPRINT 2
#define FRCNN_DRAW_BEV_WAYMO 0
#define FRCNN_DRAW_BEV_KITTI 1
int frcnn_canvas_from_image_blob(const float* blob, int height, int width, const double* stds_host,
                                 const double* means_host, const int* arrange_host, uint8_t* canvas, void* stream);
size_t frcnn_canvas_from_bev_blob_ws_bytes(void);
int frcnn_canvas_from_bev_blob(const float* blob, int ny, int nx, int channels, int num_slices, int form, uint8_t* canvas,
                               void* ws, size_t ws_bytes, void* stream);
int frcnn_draw_plan(const float* dets, const int* counts, int num_classes, int max_out, int elem, int lidar, int key_col,
                    int key_cols, int limiter0, int limiter_resets, const float* gt, const int* gt_labels, int num_gt,
                    int canvas_h, int canvas_w, int* rows, int capacity, void* stream);
int frcnn_draw_scatter(const int* rows, int num_rows, uint32_t* owner, int height, int width, void* stream);
int frcnn_draw_compose(const int* rows, int num_rows, const uint32_t* owner, uint8_t* canvas, int height, int width,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_H_ */
