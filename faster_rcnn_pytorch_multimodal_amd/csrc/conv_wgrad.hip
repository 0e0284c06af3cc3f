// Filter gradient of the convolution on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32):
//
//     dw[k][r][s][c] = sum over output pixels m = (n, ho, wo) of  dy[m][k] * x[n, ho*stride-pad+r, wo*stride-pad+s, c]
//
// Replaces autograd's conv weight gradient for the trainable convolutions of lib/nets/resnet.py:98-127,
// lib/nets/fpn.py:33-39 and the RPN / tail layers (lib/model/train_val.py:458 -> loss.backward()).
//
// GEMM view: rows = k (output channels), columns = q = (r*S+s)*C + c, reduction over the M pixels.
// Both operands are contiguous along their ROW/COLUMN index and strided along the reduction index (the
// opposite of the forward kernel), so tiles are staged as [32 pixels][128 k] and [32 pixels][128 q] with
// 16-byte chunks along k / q and the MFMA fragments are ds_read_b32 with the lanes running along k / q
// (32 consecutive floats per half wave: conflict-free without padding).  A thread's q chunk — hence its
// filter tap (r, s) and channel c — is fixed for the whole kernel; only the pixel advances.
// The pixel range is split over gridDim.z; partial sums go to slabs that are added in z order, so the result is
// deterministic.
// Two kernels: conv_wgrad_f32 (rounds 1-4: register-staged tiles, slabs added by wgrad_reduce_kernel / wgrad_accumulate_kernel;
// plans 1 / 2, kept for operands beyond 2 GB, callers without tile counters and A/B) and conv_wgrad_dma_f32 (round 5: LDS-DMA
// ring, ds_read_b64 fragments, the LAST workgroup of a tile adds the slabs and stores / accumulates itself; plans 3 / 4).
// A third, conv_wgrad_bf16 (plan 5), rounds both operands to bf16 and runs on v_mfma_f32_32x32x16_bf16: only for callers that
// ask for that arithmetic (frcnn_conv2d_bwd_weight_bf16 / _acc_bf16).
// This unit holds the kernels and the launch functions that name them; which plan runs for a call, with which workspace, is
// conv_wgrad_plan.hip's business.
#include "conv_wgrad.h"

#include <algorithm>

namespace {

using namespace frcnn::wgrad;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// tile edge BT = 64 * TI (k rows x q columns), 2 x 2 waves each owning TI x TI MFMA tiles of 32 x 32:
//   TI = 2: 128 x 128, the arithmetic-intensity choice for large pixel counts;
//   TI = 1: 64 x 64, four times as many tiles -> fewer pixel splits (less slab traffic, longer K loops) when the
//           filter is small and the pixel count short (layer3 / layer4 of one frame: M = 2394 / 608).

// The kernels' parameter types keep their names in this unit's anonymous namespace (the kernel symbols carry them); the
// fields are conv_wgrad.h's, the launch functions convert at the launch.
struct WgradParams : WgradArgs {};
struct WgradGroups : WgradGroupOperands {};
struct WgradOuts : WgradGroupGrads {};

template <int TI>
__device__ __forceinline__ void conv_wgrad_body(const WgradParams& p, const float* __restrict__ px,
                                                const float* __restrict__ pdy, float* __restrict__ pout) {
  constexpr int BT = 64 * TI;
  constexpr int CH = BT / 4;            // 16-byte chunks per staged pixel row
  constexpr int RP = 256 / CH;          // pixel rows staged per pass
  constexpr int NP = BR / RP;           // passes per reduction step
  __shared__ __attribute__((aligned(16))) float As[2][BR][BT];  // dy tile   [pixel][k]
  __shared__ __attribute__((aligned(16))) float Bs[2][BR][BT];  // x tile    [pixel][q]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int tile_k = blockIdx.x / p.tiles_q, tile_q = blockIdx.x - tile_k * p.tiles_q;
  const int k0 = tile_k * BT, q0 = tile_q * BT;
  const int step_begin = blockIdx.z * p.steps_per_split;
  const int step_end = min(step_begin + p.steps_per_split, p.steps);

  // staging: thread t moves 16-byte chunk (t % CH) of pixel rows (t / CH) + RP*i, i < NP
  const int ch = t % CH, prow = t / CH;
  const int ka = k0 + ch * 4;            // first of this thread's 4 output channels
  const bool ka_ok = ka < p.K;           // K % 4 == 0: a chunk is all in or all out
  const int qb = q0 + ch * 4;            // first of this thread's 4 filter elements
  const bool qb_ok = qb < p.Q;
  const int tap = qb_ok ? qb / p.C : 0;
  const int cb = qb - tap * p.C;
  const int tr = tap / p.S, ts = tap - tr * p.S;

  f32x4 ra[NP], rb[NP];
  auto load_tiles = [&](int step) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int m = step * BR + prow + RP * i;
      const bool m_ok = m < p.M;
      ra[i] = (m_ok && ka_ok) ? *reinterpret_cast<const f32x4*>(pdy + (size_t)m * p.K + ka) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m_ok && qb_ok) {
        const int img = m / (p.Ho * p.Wo);
        const int rem = m - img * p.Ho * p.Wo;
        const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
        const int hi = ho * p.stride - p.pad + tr, wi = wo * p.stride - p.pad + ts;
        if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
          v = *reinterpret_cast<const f32x4*>(px + ((size_t)(img * p.H + hi) * p.W + wi) * p.C + cb);
      }
      rb[i] = v;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      *reinterpret_cast<f32x4*>(&As[buf][prow + RP * i][ch * 4]) = ra[i];
      *reinterpret_cast<f32x4*>(&Bs[buf][prow + RP * i][ch * 4]) = rb[i];
    }
  };

  f32x16 acc[TI][TI];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, lh = lane >> 5;
  if (step_begin < step_end) {
    load_tiles(step_begin);
    store_tiles(0);
  }
  __syncthreads();
  int cur = 0;
  for (int step = step_begin; step < step_end; ++step) {
    const bool more = step + 1 < step_end;
    if (more) load_tiles(step + 1);
#pragma unroll
    for (int kk = 0; kk < BR / 2; ++kk) {
      float a[TI], b[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = As[cur][2 * kk + lh][(wr * TI + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < TI; ++j) b[j] = Bs[cur][2 * kk + lh][(wc * TI + j) * 32 + l31];
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_tiles(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // D: column (lane & 31) = q, row (r&3) + 8*(r>>2) + 4*(lane>>5) = k
  float* out = pout + (size_t)blockIdx.z * p.K * p.Q;
#pragma unroll
  for (int j = 0; j < TI; ++j) {
    const int q = q0 + (wc * TI + j) * 32 + l31;
    if (q >= p.Q) continue;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + (wr * TI + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (k < p.K) out[(size_t)k * p.Q + q] = acc[i][j][r];
      }
  }
}

template <int TI>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f32(const WgradParams p) {
  conv_wgrad_body<TI>(p, p.x, p.dy, p.out);
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA form of the filter gradient (plan codes 3 = 64 x 64 tile, 4 = 128 x 128 tile).
//
// What the register-staged kernel above loses (profiles/r05_train_busy.txt: conv_wgrad_f32<1> 24.8 % MfmaUtil, 5 ms of the
// 18.7 ms of kernel time per training step, + 1.2 ms of wgrad_accumulate_kernel):
//   * its prefetch is ONE reduction step deep (registers), a step of the 64 x 64 tile is 1024 MFMA cycles per wave, a global
//     load under load takes longer: every step waits;
//   * every MFMA of the 64 x 64 tile needs two ds_read_b32 (nothing issues for free beside an fp32 MFMA);
//   * the pixel-split partial sums go through slabs, a reduction kernel and a third kernel that changes the layout and adds
//     into the parameter's gradient.
// Here:
//   * the [32 pixels][BT] tiles of dy and x go global -> LDS by buffer_load_dwordx4 ... lds into a ring (four stages of 16 KB
//     for the 64-tile: three steps in flight; two stages of 32 KB for the 128-tile), one barrier per step.  Rows past M and
//     chunks past K / Q are out of the buffer's range -> zeros, no selects.  dy addresses advance by one v_add per step; x
//     addresses likewise for a 1x1 / stride 1 layer (UNIT), else (img, ho, wo) advance incrementally (no division in the loop);
//   * fragments are ds_read_b64: a lane holds TWO adjacent k (q) per pixel, i.e. MFMA operand t covers rows k = base + 2 i + t.
//     The permutation only moves results between accumulators (undone in the epilogue); one b64 pair feeds four MFMAs.
//     64-tile: every wave computes the WHOLE 64 x 64 tile over a quarter of each step's pixels (LDS bytes are read once
//     instead of twice), the four partial tiles are added in wave order through LDS afterwards.  128-tile: 2 x 2 waves of
//     64 x 64 - the summation order of conv_wgrad_f32<2>, bit-identical to it;
//   * the epilogue goes through LDS to 16-byte chunks and finishes the job: splits == 1 -> store dw or add into the gradient
//     in the parameter's own layout; splits > 1 -> slab, device-scope release, tile counter; the LAST workgroup of a tile
//     adds the slabs in z order (deterministic whoever is last) and does the same.  No second or third kernel.
// ------------------------------------------------------------------------------------------------
constexpr unsigned WG_OOB = 0x80000000u;
constexpr int WG_LDS_FLOATS = 16384;   // 64 KB

template <int TI, bool UNIT>
__device__ __forceinline__ void conv_wgrad_dma_body(const WgradParams& p, const float* __restrict__ px,
                                                    const float* __restrict__ pdy, float* __restrict__ ptarget,
                                                    float* smem) {
  constexpr int BT = 64 * TI;
  constexpr int CH = BT / 4;             // 16-byte chunks per tile row
  constexpr int RPI = 64 / CH;           // tile rows per DMA instruction (1 KB)
  constexpr int PW = BR / RPI / 4;       // DMA instructions per wave, operand and stage
  constexpr int NST = TI == 1 ? 4 : 2;   // ring stages
  constexpr int DIST = NST - 1;          // steps in flight
  constexpr int STAGE = 2 * BR * BT;     // floats per stage: dy tile, then x tile
  constexpr int KK = TI == 1 ? 4 : 16;   // MFMA k-iterations (2 pixels each) per wave and step
  static_assert(NST * STAGE == WG_LDS_FLOATS, "ring = 64 KB");
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef float f32x2 __attribute__((ext_vector_type(2)));

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int tile_k = blockIdx.x / p.tiles_q, tile_q = blockIdx.x - tile_k * p.tiles_q;
  const int k0 = tile_k * BT, q0 = tile_q * BT;
  const int step_begin = blockIdx.z * p.steps_per_split;
  const int step_end = min(step_begin + p.steps_per_split, p.steps);
  const int nsteps = max(step_end - step_begin, 0);

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pdy), 0, (int)p.dybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(px), 0, (int)p.xbytes, 0x00020000);

  // ---- DMA sources: lane i of instruction j of this wave feeds tile row (wave PW + j) RPI + i / CH, chunk i % CH ------------
  const int lrow = lane / CH, lchunk = lane % CH;
  const int ka = k0 + lchunk * 4, qb = q0 + lchunk * 4;
  const bool ka_ok = ka < p.K, qb_ok = qb < p.Q;
  unsigned vA[PW], vB[PW];
  int s_img[PW], s_hi[PW], s_wi[PW], s_off[PW];   // general path: image, input row / column of this lane's tap, byte offset
  const int tap = qb_ok ? qb / p.C : 0;
  const int cb = qb - tap * p.C;
  const int tr = tap / p.S, ts = tap - tr * p.S;
  const int tr_off = tr - p.pad, ts_off = ts - p.pad;
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int m = step_begin * BR + (wave * PW + j) * RPI + lrow;
    vA[j] = ka_ok ? (unsigned)((m * p.K + ka) * 4) : WG_OOB;
    if (UNIT) {
      vB[j] = qb_ok ? (unsigned)((m * p.C + qb) * 4) : WG_OOB;
    } else {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      s_img[j] = img;
      s_hi[j] = ho * p.stride + tr_off;
      s_wi[j] = wo * p.stride + ts_off;
      s_off[j] = (((img * p.H + s_hi[j]) * p.W + s_wi[j]) * p.C + cb) * 4;   // used only where (hi, wi) is inside the image
    }
  }
  const unsigned stepA = (unsigned)(BR * p.K * 4), stepB = (unsigned)(BR * p.C * 4);
  // General path: BR pixels further in (img, ho, wo) is one carry per digit; the input position (hi, wi) and the byte offset
  // are carried along with additions only (the first version recomputed the offset from (img, ho, wo): five quarter-rate
  // integer multiplies per DMA instruction, ~540 of a step's 1900 cycles on a 3x3 layer).
  const int d_img = BR / (p.Ho * p.Wo), d_rem = BR - d_img * p.Ho * p.Wo;
  const int d_ho = d_rem / p.Wo, d_wo = d_rem - d_ho * p.Wo;
  const int dwi = d_wo * p.stride, wrap_w = p.Wo * p.stride, dhi = d_ho * p.stride, wrap_h = p.Ho * p.stride;
  const int wlim = wrap_w + ts_off, hlim = wrap_h + tr_off;             // wo == Wo, ho == Ho in (wi, hi) terms
  const int row_b = p.W * p.C * 4, img_b = p.H * row_b;
  const int o_step = dwi * p.C * 4 + dhi * row_b + d_img * img_b;
  const int o_c1 = p.stride * row_b - wrap_w * p.C * 4;                  // wo wraps: one output row down
  const int o_c2 = img_b - wrap_h * row_b;                               // ho wraps: next image

  auto issue = [&](int stage) {
    float* sA = smem + stage * STAGE + wave * PW * 256;
    float* sB = sA + BR * BT;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr)(sA + j * 256), 16, (int)vA[j], 0, 0, 0);
      vA[j] += stepA;
    }
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      unsigned off;
      if (UNIT) {
        off = vB[j];
        vB[j] += stepB;
      } else {
        const bool ok = qb_ok && s_img[j] < p.N && (unsigned)s_hi[j] < (unsigned)p.H && (unsigned)s_wi[j] < (unsigned)p.W;
        off = ok ? (unsigned)s_off[j] : WG_OOB;
        const int wi = s_wi[j] + dwi;
        const bool c1 = wi >= wlim;
        s_wi[j] = wi - (c1 ? wrap_w : 0);
        const int hi = s_hi[j] + dhi + (c1 ? p.stride : 0);
        const bool c2 = hi >= hlim;
        s_hi[j] = hi - (c2 ? wrap_h : 0);
        s_img[j] += d_img + (c2 ? 1 : 0);
        s_off[j] += o_step + (c1 ? o_c1 : 0) + (c2 ? o_c2 : 0);
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr)(sB + j * 256), 16, (int)off, 0, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment address of k-iteration 0: pixel row (first pixel of this wave) + lh, column pair 2 * l31 of this wave's columns
  const int wr = wave >> 1, wc = wave & 1;
  const int prow0 = TI == 1 ? wave * 8 : 0;
  const int fa = (prow0 + lh) * BT + (TI == 1 ? 0 : wr * 64) + 2 * l31;
  const int fb = BR * BT + (prow0 + lh) * BT + (TI == 1 ? 0 : wc * 64) + 2 * l31;

#pragma unroll
  for (int s = 0; s < DIST; ++s)
    if (s < nsteps) issue(s);
  int stage = 0, fill = DIST % NST;
  for (int s = 0; s < nsteps; ++s) {
    if (DIST > 1 && s + DIST - 1 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PW * (DIST > 1 ? DIST - 1 : 0)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (s + DIST < nsteps) issue(fill);
    const float* base = smem + stage * STAGE;
    f32x2 a2 = *reinterpret_cast<const f32x2*>(base + fa);
    f32x2 b2 = *reinterpret_cast<const f32x2*>(base + fb);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      f32x2 an = a2, bn = b2;
      if (kk + 1 < KK) {
        an = *reinterpret_cast<const f32x2*>(base + fa + (kk + 1) * 2 * BT);
        bn = *reinterpret_cast<const f32x2*>(base + fb + (kk + 1) * 2 * BT);
      }
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[0], b2[0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[0], b2[1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[1], b2[0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[1], b2[1], acc[1][1], 0, 0, 0);
      a2 = an;
      b2 = bn;
    }
    stage = stage + 1 == NST ? 0 : stage + 1;
    fill = fill + 1 == NST ? 0 : fill + 1;
  }

  // ---- epilogue: accumulators -> LDS (tile row k, 16-byte chunks along q) ----------------------------------------------------
  // D of MFMA (ta, tb): column l31 -> q pair member tb of column pair l31, row i = (r & 3) + 8 (r >> 2) + 4 lh -> k = 2 i + ta
  __syncthreads();
  {
    float* P = TI == 1 ? smem + wave * (64 * 64) : smem + (wr * 64) * BT + wc * 64;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
        *reinterpret_cast<f32x2*>(P + (2 * i + ta) * BT + 2 * l31) = f32x2{acc[ta][0][r], acc[ta][1][r]};
      }
  }
  __syncthreads();
  constexpr int NCH = BT * BT / 4 / 256;   // chunks per thread
  const size_t KQ = (size_t)p.K * p.Q;
  auto emit = [&](int k, int q, f32x4 v) {
    if (p.mode == 0) {
      *reinterpret_cast<f32x4*>(ptarget + (size_t)k * p.Q + q) = v;
    } else if (p.R * p.S == 1 && p.c_real == p.C) {
      f32x4* g = reinterpret_cast<f32x4*>(ptarget + (size_t)k * p.C + q);
      f32x4 o = *g;
      o[0] += v[0]; o[1] += v[1]; o[2] += v[2]; o[3] += v[3];
      *g = o;
    } else {
      const int tp = q / p.C, c = q - tp * p.C;
      const int r = tp / p.S, s2 = tp - r * p.S;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < p.c_real) ptarget[(((size_t)k * p.c_real + c + e) * p.R + r) * p.S + s2] += v[e];
    }
  };
  // Slabs travel between workgroups on different XCDs (one L2 each): they are stored and loaded at AGENT scope (sc1: written
  // through / read past the XCD's L2) instead of bracketing plain accesses with device-scope fences - a release fence writes
  // back and an acquire fence invalidates the WHOLE L2 of the XCD, once per workgroup (measured: 24 splits of layer3's
  // 1x1 took 202 us with the fences, the unsplit launch 52 us).
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((size_t)p.splits * KQ * 4), 0x00020000);
  const unsigned zoff = (unsigned)((size_t)blockIdx.z * KQ * 4);
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int c = t + 256 * u;
    const int kl = c / CH, qc = c - kl * CH;
    f32x4 v;
    if (TI == 1) {
      const float* P = smem + kl * 64 + qc * 4;
      v = *reinterpret_cast<const f32x4*>(P);
#pragma unroll
      for (int w2 = 1; w2 < 4; ++w2) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(P + w2 * (64 * 64));
        v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
      }
    } else {
      v = *reinterpret_cast<const f32x4*>(smem + kl * BT + qc * 4);
    }
    const int k = k0 + kl, q = q0 + qc * 4;
    if (k < p.K && q < p.Q) {
      if (p.splits == 1) emit(k, q, v);
      else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rS, zoff + (unsigned)((k * p.Q + q) * 4), 0, 16);
    }
  }
  if (p.splits == 1) return;
  // ---- last arriver of this tile adds the slabs in z order --------------------------------------------------------------------
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's slab stores have reached the coherence point
  __syncthreads();
  if (t == 0) {
    int* ctr = p.counters + blockIdx.x;
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == p.splits - 1;
    if (s_last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero again for the next launch
  }
  __syncthreads();
  if (!s_last) return;
#pragma unroll 1
  for (int u = 0; u < NCH; ++u) {
    const int c = t + 256 * u;
    const int kl = c / CH, qc = c - kl * CH;
    const int k = k0 + kl, q = q0 + qc * 4;
    if (k >= p.K || q >= p.Q) continue;
    const unsigned off = (unsigned)((k * p.Q + q) * 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    // eight slab loads in flight at a time; added in z order
    for (int z0 = 0; z0 < p.splits; z0 += 8) {
      f32x4 o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (z0 + i < p.splits)
          o[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rS, off + (unsigned)((size_t)(z0 + i) * KQ * 4), 0, 16));
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (z0 + i < p.splits) {
          if (z0 + i == 0) v = o[i];
          else { v[0] += o[i][0]; v[1] += o[i][1]; v[2] += o[i][2]; v[3] += o[i][3]; }
        }
    }
    emit(k, q, v);
  }
}

template <int TI, bool UNIT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_dma_f32(const WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float wg_smem[];
  conv_wgrad_dma_body<TI, UNIT>(p, p.x, p.dy, p.target, wg_smem);
}

// Grouped form: blockIdx.y selects one of up to WG_MAX_GROUPS convolutions of IDENTICAL shape (the 22 repeated Bottlenecks
// of layer3, lib/nets/resnet.py:131-240): together they have enough output tiles to fill the chip WITHOUT splitting the
// pixel reduction, so every tile runs the whole M-pixel loop (75 steps instead of ~9) and no slabs are summed afterwards.
// Group g writes its (K, Q) result to p.out + g * K * Q.
template <int TI>
__global__ __launch_bounds__(256, 2) void conv_wgrad_grouped_f32(const WgradParams p, const WgradGroups g) {
  const int grp = blockIdx.y;
  conv_wgrad_body<TI>(p, g.x[grp], g.dy[grp], p.out + (size_t)grp * p.K * p.Q);
}

template <int TI, bool UNIT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_dma_grouped_f32(const WgradParams p, const WgradGroups g, const WgradOuts o) {
  extern __shared__ __attribute__((aligned(16))) float wg_smem[];
  const int grp = blockIdx.y;
  conv_wgrad_dma_body<TI, UNIT>(p, g.x[grp], g.dy[grp], o.grad[grp], wg_smem);
}

// ------------------------------------------------------------------------------------------------
// bf16-operand form of the filter gradient (plan code 5; cfg.TRAIN.CONV_BF16):
//
//     dw[k][q] = sum over pixels m of  bf16(dy)[m][k] * bf16(patch(x))[m][q],   fp32 accumulation
//
// on v_mfma_f32_32x32x16_bf16.  The instruction wants 8 consecutive REDUCTION elements (pixels) per lane, the operands are
// contiguous along k / q: the tiles are transposed on the way into LDS.  A thread loads a 4 pixel x 4 k (q) patch as four
// 16-byte chunks (one per pixel; the eight threads of a pixel group cover 128 contiguous bytes of a pixel row), rounds it to
// bf16 once (nearest even, v_cvt_pk_bf16_f32) and stores it as four 8-byte columns - row k (q), pixels 4 pg .. 4 pg + 3 - of a
// [128 k (q)][32 pixels] bf16 image with the forward bf16 kernel's 80-byte row pitch.  A fragment is then that kernel's
// ds_read_b128: lane l holds row l & 31, pixels 8 (l >> 5) + j of a group of 16.
//   LDS banks: a wave's ds_write_b64 goes to rows 4 ch + e (ch = 8 consecutive chunks) at byte 8 pg: word (4 ch + e) 20 + 2 pg,
//   i.e. bank 16 (ch & 1) + 2 pg + const - all 32 banks, four lanes each: the minimum for 64 lanes x 8 bytes.
//   Pixel addresses of x advance by carries (no division in the loop), as in conv_wgrad_dma_f32.
// One tile: 128 x 128, 2 x 2 waves of 64 x 64, one reduction step (BR = 32 pixels = two MFMA groups) prefetched in registers,
// two LDS stages (40 KB), one barrier per step.  The pixel range is split over gridDim.z into fp32 slabs like conv_wgrad_f32;
// wgrad_reduce_kernel / wgrad_accumulate_kernel add them in z order: the result is a fixed function of the inputs and the
// split count.  No last-arriver epilogue, no grouped form, no counters, no atomics.
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int WB_BT = 128;      // tile edge
constexpr int WB_PITCH = 80;    // bytes per LDS row: 32 pixels of bf16 + 16 B pad (conv_igemm_bf16's BF16_PITCH)
constexpr int WB_STAGE = WB_BT * WB_PITCH;

__global__ __launch_bounds__(256, 2) void conv_wgrad_bf16(const WgradParams p) {
  static_assert(BR == 32, "a reduction step is one 64-byte LDS row of bf16 pixels");
  __shared__ __attribute__((aligned(16))) char As[2 * WB_STAGE];   // dy tile [k][pixel]
  __shared__ __attribute__((aligned(16))) char Bs[2 * WB_STAGE];   // x tile  [q][pixel]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int tile_k = blockIdx.x / p.tiles_q, tile_q = blockIdx.x - tile_k * p.tiles_q;
  const int k0 = tile_k * WB_BT, q0 = tile_q * WB_BT;
  const int step_begin = blockIdx.z * p.steps_per_split;
  const int step_end = min(step_begin + p.steps_per_split, p.steps);

  // staging: thread t moves chunk ch (4 k / 4 q) of the four pixels of group pg
  const int pg = t & 7, ch = t >> 3;
  const int ka = k0 + ch * 4;
  const bool ka_ok = ka < p.K;           // K % 4 == 0: a chunk is all in or all out
  const int qb = q0 + ch * 4;
  const bool qb_ok = qb < p.Q;           // C % 4 == 0: a chunk lies inside one filter tap
  const int tap = qb_ok ? qb / p.C : 0;
  const int cb = qb - tap * p.C;
  const int tr = tap / p.S, ts = tap - tr * p.S;

  // first pixel of this thread in the current step, as (m, img, ho, wo); a step is BR pixels further
  int m = step_begin * BR + pg * 4;
  int img = m / (p.Ho * p.Wo);
  int ho, wo;
  {
    const int rem = m - img * p.Ho * p.Wo;
    ho = rem / p.Wo;
    wo = rem - ho * p.Wo;
  }
  const int d_img = BR / (p.Ho * p.Wo), d_rem = BR - d_img * p.Ho * p.Wo;
  const int d_ho = d_rem / p.Wo, d_wo = d_rem - d_ho * p.Wo;

  f32x4 ra[4], rb[4];
  // (called for consecutive steps: the pixel state advances by one step per call)
  auto load_tiles = [&]() {
    int mi = m, ii = img, hh = ho, ww = wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool m_ok = mi < p.M;
      ra[i] = (m_ok && ka_ok) ? *reinterpret_cast<const f32x4*>(p.dy + (size_t)mi * p.K + ka) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int hi = hh * p.stride - p.pad + tr, wi = ww * p.stride - p.pad + ts;
      if (m_ok && qb_ok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
        v = *reinterpret_cast<const f32x4*>(p.x + ((size_t)(ii * p.H + hi) * p.W + wi) * p.C + cb);
      rb[i] = v;
      ++mi;
      if (++ww == p.Wo) {
        ww = 0;
        if (++hh == p.Ho) { hh = 0; ++ii; }
      }
    }
    m += BR;
    wo += d_wo;
    ho += d_ho;
    img += d_img;
    if (wo >= p.Wo) { wo -= p.Wo; ++ho; }
    if (ho >= p.Ho) { ho -= p.Ho; ++img; }
  };
  // element e of the four chunks = row (ch * 4 + e), pixels 4 pg .. 4 pg + 3
  auto store_tiles = [&](int buf) {
    char* a = As + buf * WB_STAGE + (ch * 4) * WB_PITCH + pg * 8;
    char* b = Bs + buf * WB_STAGE + (ch * 4) * WB_PITCH + pg * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 ca = {ra[0][e], ra[1][e], ra[2][e], ra[3][e]};
      const f32x4 cbv = {rb[0][e], rb[1][e], rb[2][e], rb[3][e]};
      *reinterpret_cast<bf16x4*>(a + e * WB_PITCH) = __builtin_convertvector(ca, bf16x4);
      *reinterpret_cast<bf16x4*>(b + e * WB_PITCH) = __builtin_convertvector(cbv, bf16x4);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment: row l31 of a 32-row block, pixels 8 lh .. 8 lh + 7 of MFMA group kk (16 pixels = 32 bytes)
  const int frag = l31 * WB_PITCH + 16 * lh;
  const int a_frag = (wr * 64) * WB_PITCH + frag;
  const int b_frag = (wc * 64) * WB_PITCH + frag;

  if (step_begin < step_end) {
    load_tiles();
    store_tiles(0);
  }
  __syncthreads();
  int cur = 0;
  for (int step = step_begin; step < step_end; ++step) {
    const bool more = step + 1 < step_end;
    if (more) load_tiles();
    const char* Ab = As + cur * WB_STAGE + a_frag;
    const char* Bb = Bs + cur * WB_STAGE + b_frag;
    bf16x8 fa[2][2], fb[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[kk][i] = *reinterpret_cast<const bf16x8*>(Ab + i * 32 * WB_PITCH + kk * 32);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[kk][j] = *reinterpret_cast<const bf16x8*>(Bb + j * 32 * WB_PITCH + kk * 32);
    }
    // A = dy (row = k), B = x (column = q): D column (lane & 31) = q, D row (register) = k, as in conv_wgrad_f32
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
    if (more) store_tiles(cur ^ 1);   // stage cur ^ 1 was last read before the previous step's barrier
    __syncthreads();
    cur ^= 1;
  }

  float* out = p.out + (size_t)blockIdx.z * p.K * p.Q;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = q0 + (wc * 2 + j) * 32 + l31;
    if (q >= p.Q) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + (wr * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (k < p.K) out[(size_t)k * p.Q + q] = acc[i][j][r];
      }
  }
}

// dw = sum_z slab[z] (z order), 16 bytes per thread
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, int splits, size_t n4,
                                                          float* __restrict__ dw) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 v = reinterpret_cast<const f32x4*>(slabs)[i];
    for (int z = 1; z < splits; ++z) {
      const f32x4 u = reinterpret_cast<const f32x4*>(slabs)[(size_t)z * n4 + i];
      v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
    }
    reinterpret_cast<f32x4*>(dw)[i] = v;
  }
}

// Where element i of a parameter's gradient (K, c_real, R, S) - a Conv2d / Linear parameter's own layout - lies in the
// (K, R, S, C) result of the GEMM.  (The DMA kernels' emit goes the other way, from a 16-byte chunk of the result to four
// gradient elements, and keeps its own arithmetic.)
__device__ __forceinline__ size_t krsc_index(size_t i, int R, int S, int C, int c_real) {
  const int s = (int)(i % S);
  size_t t = i / S;
  const int r = (int)(t % R);
  t /= R;
  const int c = (int)(t % c_real);
  const int k = (int)(t / c_real);
  return (((size_t)k * R + r) * S + s) * C + c;
}

// Slab sum + layout change + accumulation in one pass, for group blockIdx.y of a (grouped) filter gradient: o.grad[g]
// (K, c_real, R, S) += sum_z slabs[g][z] (K, R, S, C) restricted to the real channels.  One thread per OUTPUT element (coalesced
// read-modify-write of the gradient); the slab reads stride by C floats (small tensors).  z ascending: deterministic.
__global__ __launch_bounds__(256) void wgrad_accumulate_kernel(const float* __restrict__ slabs, int splits, int K, int R, int S,
                                                              int C, int c_real, const WgradOuts o) {
  const size_t total = (size_t)K * c_real * R * S, slab = (size_t)K * R * S * C;
  const float* __restrict__ src0 = slabs + (size_t)blockIdx.y * splits * slab;
  float* __restrict__ grad = o.grad[blockIdx.y];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t src = krsc_index(i, R, S, C, c_real);
    float v = src0[src];
    for (int z = 1; z < splits; ++z) v += src0[(size_t)z * slab + src];
    grad[i] += v;
  }
}

// db[k] = sum_m dy[m][k] in two deterministic passes: BIAS_GROUPS x (K/64) workgroups sum interleaved pixel
// subsets (4 waves each) into partial[g][k], then one pass adds the groups in g order.
__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const float* __restrict__ dy, int M, int K,
                                                               float* __restrict__ partial) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (k < K)
    for (int m = blockIdx.y * 4 + wave; m < M; m += 4 * BIAS_GROUPS) s += dy[(size_t)m * K + k];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && k < K)
    partial[(size_t)blockIdx.y * K + k] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}
// db[k] = s or db[k] += 0.f + s, s = the groups' partial sums added in g order from partial[0][k].  The accumulating form used
// to start its sum at 0.f instead: 0.f + s is that sum bit for bit, for s == -0.f (every partial sum a negative zero) too,
// where it is +0.f - and that is the only s for which the two starts differ.
__global__ __launch_bounds__(256) void bias_grad_final_kernel(const float* __restrict__ partial, int K, int accumulate,
                                                             float* __restrict__ db) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  float s = partial[k];
  for (int g = 1; g < BIAS_GROUPS; ++g) s += partial[(size_t)g * K + k];
  db[k] = accumulate ? db[k] + (0.f + s) : s;
}

// ---- launches ------------------------------------------------------------------------------------------------------------
// (not through frcnn::conv::launch_kernel: these launches are no part of the per-dispatch convolution profile)
constexpr size_t WG_LDS_BYTES = (size_t)WG_LDS_FLOATS * sizeof(float);

// one launch form for the four GEMM kernel families; `extra` are a grouped kernel's pointer blocks
template <auto Kernel, typename... Extra>
int launch(const char* name, size_t lds, const WgradArgs& p, dim3 grid, hipStream_t stream, Extra... extra) {
  if (lds > 0) {
    const int rc = frcnn::ensure_dynamic_lds<Kernel>(lds, name);
    if (rc != FRCNN_OK) return rc;
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, stream, WgradParams{p}, extra...);
  return frcnn::check_launch(name);
}

// The one (TI, UNIT) dispatch: f(tile) with tile's TI / UNIT the constants of a tile factor and of "1x1, stride 1, no padding"
// (the register-staged kernels have no UNIT form and take TI alone)
template <int TI_, bool UNIT_>
struct Tile {
  static constexpr int TI = TI_;
  static constexpr bool UNIT = UNIT_;
};
template <typename F>
int for_tile(int tf, bool unit, F f) {
  if (tf == 1) return unit ? f(Tile<1, true>{}) : f(Tile<1, false>{});
  return unit ? f(Tile<2, true>{}) : f(Tile<2, false>{});
}
inline bool unit_conv(const WgradArgs& p) { return p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0; }

}  // namespace

namespace frcnn {
namespace wgrad {

int launch_gemm(const WgradArgs& p, int ti, hipStream_t stream) {
  const dim3 grid(p.tiles_k * p.tiles_q, 1, p.splits);
  if (ti == PLAN_BF16) return launch<conv_wgrad_bf16>("conv_wgrad_bf16", 0, p, grid, stream);
  return for_tile(tile_factor(ti), unit_conv(p), [&](auto t) {
    using T = decltype(t);
    return ti >= 3 ? launch<conv_wgrad_dma_f32<T::TI, T::UNIT>>("conv_wgrad_dma_f32", WG_LDS_BYTES, p, grid, stream)
                   : launch<conv_wgrad_f32<T::TI>>("conv_wgrad_f32", 0, p, grid, stream);
  });
}

int launch_gemm_grouped(const WgradArgs& p, int ti, int groups, const WgradGroupOperands& g, const WgradGroupGrads& o,
                        hipStream_t stream) {
  const dim3 grid(p.tiles_k * p.tiles_q, groups, 1);
  const WgradGroups wg{g};
  return for_tile(tile_factor(ti), unit_conv(p), [&](auto t) {
    using T = decltype(t);
    return ti >= 3 ? launch<conv_wgrad_dma_grouped_f32<T::TI, T::UNIT>>("conv_wgrad_dma_grouped_f32", WG_LDS_BYTES, p, grid, stream,
                                                                       wg, WgradOuts{o})
                   : launch<conv_wgrad_grouped_f32<T::TI>>("conv_wgrad_grouped_f32", 0, p, grid, stream, wg);
  });
}

int launch_reduce(const float* slabs, int splits, size_t n4, float* dw, hipStream_t stream) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 4096)), dim3(256), 0, stream, slabs,
                     splits, n4, dw);
  return frcnn::check_launch("wgrad_reduce_kernel");
}

int launch_accumulate(const float* slabs, int splits, const WgradArgs& p, int groups, const WgradGroupGrads& o,
                      unsigned max_blocks, hipStream_t stream) {
  const size_t total = (size_t)p.K * p.c_real * p.R * p.S;
  hipLaunchKernelGGL(wgrad_accumulate_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, max_blocks), groups), dim3(256),
                     0, stream, slabs, splits, p.K, p.R, p.S, p.C, p.c_real, WgradOuts{o});
  return frcnn::check_launch("wgrad_accumulate_kernel");
}

int launch_bias_gradient(const float* dy, int M, int k, float* partial, float* db, bool accumulate, hipStream_t stream) {
  hipLaunchKernelGGL(bias_grad_partial_kernel, dim3((k + 63) / 64, BIAS_GROUPS), dim3(256), 0, stream, dy, M, k, partial);
  const int rc = frcnn::check_launch("bias_grad_partial_kernel");
  if (rc != FRCNN_OK) return rc;
  hipLaunchKernelGGL(bias_grad_final_kernel, dim3((k + 255) / 256), dim3(256), 0, stream, static_cast<const float*>(partial), k,
                     accumulate ? 1 : 0, db);
  return frcnn::check_launch("bias_grad_final_kernel");
}

}  // namespace wgrad
}  // namespace frcnn

