// Implicit-GEMM convolution forward on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces the ATen/cuDNN conv2d + batch_norm(eval) + add + relu chain of the reference's
// lib/nets/resnet.py:98-127 (Bottleneck.forward), :152-156 (stem), lib/nets/fpn.py:33-39 and the RPN
// convs of the (missing) lib/nets/network.py.
//
// GEMM view:  M = N*Ho*Wo output pixels, N = K output channels, Kdim = R*S*C (tap-major, channel-minor).
// Activations are NHWC and filters KRSC, so both operands are contiguous along Kdim: the global->LDS
// staging moves 16-byte chunks along Kdim and the MFMA fragments are ds_read_b128 along Kdim.
//
// Workgroup = WM x WN waves, each wave owns TM x TN tiles of 32x32 outputs (block tile BM = 32*TM*WM
// pixels, BN = 32*TN*WN channels), BK = 32.  The large-GEMM configuration is 8 waves (two per SIMD)
// on a 256x128 tile, ONE workgroup per CU: both waves of a SIMD belong to the same workgroup, so they
// reach the per-K-step barrier together and the SIMDs carry identical work (two co-resident 4-wave
// workgroups couple through their barriers instead and leave ~20 % of the MFMA slots empty).
// LDS rows are padded to 36 floats: the 16-lane groups of ds_read_b128 then hit 16 distinct 16-byte
// slots (36*m mod 64 = 4*(9m mod 16) is a bijection).
//
// Software pipeline of one K-step (4 groups of k=8, each TM*TN*4 MFMAs per wave):
//   group 0,1 : MFMAs on fragments prefetched one group ahead
//   then      : the register-staged global tile of step s+1 is written to the other LDS buffer
//   group 2   : MFMAs; the global loads of step s+2 are issued (they land ~3/4 step later)
//   barrier   : placed BEFORE the last group, whose fragments are already in registers
//   group 3   : MFMAs, overlapped with the first fragment reads of the next buffer
// so neither the LDS write/barrier/read turn-around nor the HBM/L2 latency is exposed.
//
// The MFMA computes an exact k-ordered fp32 fma chain, so results are deterministic and independent
// of the tile configuration for split_k == 1.
#include "conv_common.h"

#include <type_traits>

#include <algorithm>

using namespace frcnn::conv;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int LDS_PITCH = 36;  // floats per LDS row (32 + 4 pad)

// The kernels' parameter type is ConvArgs under a name of this unit's own, like the kernels themselves: `ConvParams` in an
// anonymous namespace is part of every kernel symbol, and profiles/ and recorded traces name the kernels by their symbols.
struct ConvParams : ConvArgs {};
ConvParams kernel_arg(const ConvArgs& p) { return ConvParams{p}; }

// XCD-aware bijective remap (guide T1): blocks b and b+8 share an XCD; give each XCD a contiguous
// range of logical tiles so neighbouring tiles (shared A rows / B columns) hit the same L2.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = b & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (b >> 3);
}

// Logical tile -> (tile_m, tile_n).  Tiles are walked in column groups of RASTER_GN n-tiles (m fastest inside a
// group): the tiles an XCD works on concurrently (a contiguous range of this order, see xcd_remap) then share at most
// RASTER_GN filter column blocks, so the filter slice they re-read stays inside the XCD's 4 MB L2 instead of the whole
// K x C filter cycling through it once per pixel row.
constexpr int RASTER_GN = 8;
__device__ __forceinline__ void tile_coords(int tile, int tiles_m, int tiles_n, int& tile_m, int& tile_n) {
  const int per_group = RASTER_GN * tiles_m;
  const int group = tile / per_group, within = tile - group * per_group;
  const int gn = min(RASTER_GN, tiles_n - group * RASTER_GN);
  tile_n = group * RASTER_GN + within % gn;
  tile_m = within / gn;
}

// Epilogue shared by the conv kernels.  The MFMA operands are (weights, activations), so D has the PIXEL on the
// lane (col = lane&31) and the CHANNEL in the registers: row = (r&3) + 8*(r>>2) + 4*(lane>>5).  Registers
// 4g..4g+3 are four consecutive channels -> every access is a 16-byte vector per lane, and all residual loads of a
// 32x32 tile are issued before its first store (res may alias nothing we write, but the compiler cannot know:
// batching keeps 4 loads in flight instead of a load->wait->store chain per element).
template <int TM, int TN>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                              int lane, int mrows, int gy = -1, int gz = -1) {   // mrows: group_rows
  if (gy < 0) gy = blockIdx.y;                     // (the persistent kernel walks groups / splits itself)
  if (gz < 0) gz = blockIdx.z;
  const size_t goff = (size_t)gy * p.gy;   // grouped launches have neither a residual nor split-K slabs
  const int mlane = lane & 31, nhalf = 4 * (lane >> 5);
  const bool vec = (p.K & 3) == 0;
  float* const slab = p.partial ? p.partial + (size_t)gz * p.M * p.K : nullptr;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + (wr * TM + i) * 32 + mlane;
    if (m >= mrows) continue;
    size_t orow = (size_t)m * p.K + goff;  // row of y / residual
    if (p.ys != 1) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      orow = ((size_t)(img * p.Hy + ho * p.ys) * p.Wy + wo * p.ys) * p.K + goff;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + (wc * TN + j) * 32 + nhalf;
      const size_t row = (size_t)m * p.K;
      if (vec) {
        if (slab) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int n = nb + 8 * g;
            if (n < p.K)
              *reinterpret_cast<f32x4*>(slab + row + n) =
                  f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          }
          continue;
        }
        f32x4 rv[4], mv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = nb + 8 * g;
          rv[g] = (p.res && n < p.K) ? *reinterpret_cast<const f32x4*>(p.res + orow + n) : f32x4{0.f, 0.f, 0.f, 0.f};
          mv[g] = (p.mask && n < p.K) ? *reinterpret_cast<const f32x4*>(p.mask + orow + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = nb + 8 * g;
          if (n >= p.K) continue;
          const f32x4 sc = p.scale ? *reinterpret_cast<const f32x4*>(p.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
          const f32x4 sh = p.shift ? *reinterpret_cast<const f32x4*>(p.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
          const f32x4 ms = (p.mask && p.mscale) ? *reinterpret_cast<const f32x4*>(p.mscale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float t = acc[i][j][4 * g + e] * sc[e] + sh[e];
            t += rv[g][e];
            t = p.relu ? frcnn::relu_f32(t) : t;
            if (p.mask) t = frcnn::relu_open(mv[g][e]) ? t * ms[e] : 0.f;
            v[e] = t;
          }
          *reinterpret_cast<f32x4*>(p.y + orow + n) = v;
        }
      } else {
        // K % 4 != 0: rows are not 16-byte aligned, element-wise accesses
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = nb + (r & 3) + 8 * (r >> 2);
          if (n >= p.K) continue;
          if (slab) { slab[row + n] = acc[i][j][r]; continue; }
          float t = acc[i][j][r] * (p.scale ? p.scale[n] : 1.f) + (p.shift ? p.shift[n] : 0.f);
          if (p.res) t += p.res[orow + n];
          t = p.relu ? frcnn::relu_f32(t) : t;
          if (p.mask) t = frcnn::relu_open(p.mask[orow + n]) ? t * (p.mscale ? p.mscale[n] : 1.f) : 0.f;
          p.y[orow + n] = t;
        }
      }
    }
  }
}

// The same epilogue with the accumulator tiles TRANSPOSED through LDS first.  In the MFMA layout a lane holds 4 consecutive
// channels of ITS pixel, so a store instruction of conv_epilogue writes 64 pieces of 16 bytes (32 pixels x 2 halves), each in
// a different row of the output - and reads the residual the same way.  Here a wave writes its 32 x 32 tile to a private LDS
// patch (the K loop is over: the staging buffers are free) and reads it back with 8 lanes per pixel: every global access of
// the wave is then 8 rows x 128 contiguous bytes.  Same per-element arithmetic -> bit-identical results.  K % 4 == 0 only.
template <int TM, int TN>
__device__ __forceinline__ void conv_epilogue_lds(const ConvParams& p, f32x16 (&acc)[TM][TN], int m0, int n0, int wr, int wc,
                                                  int lane, int mrows, float* __restrict__ patch, int gy = -1, int gz = -1) {
  if (gy < 0) gy = blockIdx.y;
  if (gz < 0) gz = blockIdx.z;
  const size_t goff = (size_t)gy * p.gy;
  float* const slab = p.partial ? p.partial + (size_t)gz * p.M * p.K : nullptr;
  const int wpix = lane & 31, whalf = 4 * (lane >> 5);       // write phase: MFMA layout
  const int rrow = lane >> 3, rcol = 4 * (lane & 7);         // read phase: 8 lanes x 16 B per pixel row
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(patch + wpix * LDS_PITCH + 8 * g + whalf) =
            f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
      const int n = n0 + (wc * TN + j) * 32 + rcol;
      const bool nok = n < p.K;
      f32x4 v[4], rv[4], mv[4];
      size_t at[4];
      bool ok[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = rrow + 8 * it;
        const int m = m0 + (wr * TM + i) * 32 + row;
        v[it] = *reinterpret_cast<const f32x4*>(patch + row * LDS_PITCH + rcol);
        ok[it] = nok && m < mrows;
        size_t orow = (size_t)m * p.K + goff;
        if (p.ys != 1 && ok[it]) {
          const int img = m / (p.Ho * p.Wo);
          const int rem = m - img * p.Ho * p.Wo;
          const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
          orow = ((size_t)(img * p.Hy + ho * p.ys) * p.Wy + wo * p.ys) * p.K + goff;
        }
        at[it] = slab ? (size_t)m * p.K + n : orow + n;
        rv[it] = (!slab && p.res && ok[it]) ? *reinterpret_cast<const f32x4*>(p.res + at[it]) : f32x4{0.f, 0.f, 0.f, 0.f};
        mv[it] = (!slab && p.mask && ok[it]) ? *reinterpret_cast<const f32x4*>(p.mask + at[it]) : f32x4{1.f, 1.f, 1.f, 1.f};
      }
      if (slab) {
#pragma unroll
        for (int it = 0; it < 4; ++it)
          if (ok[it]) *reinterpret_cast<f32x4*>(slab + at[it]) = v[it];
        continue;
      }
      const f32x4 sc = (p.scale && nok) ? *reinterpret_cast<const f32x4*>(p.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
      const f32x4 sh = (p.shift && nok) ? *reinterpret_cast<const f32x4*>(p.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 ms = (p.mask && p.mscale && nok) ? *reinterpret_cast<const f32x4*>(p.mscale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        if (!ok[it]) continue;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = v[it][e] * sc[e] + sh[e];
          t += rv[it][e];
          t = p.relu ? frcnn::relu_f32(t) : t;
          if (p.mask) t = frcnn::relu_open(mv[it][e]) ? t * ms[e] : 0.f;
          o[e] = t;
        }
        *reinterpret_cast<f32x4*>(p.y + at[it]) = o;
      }
    }
  }
}

// 256 zero bytes: out-of-range lanes (padding taps, M / K tails) load from here instead of branching around the load, so
// every load of a tile is issued unconditionally (and the compiler can count them: partial vmcnt waits)
__device__ float g_zero_page[64];

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* gbl_ptr;

// The LDS image of the four LDS-DMA kernels: a stage is [BM + BN rows][32 floats], 128-byte rows WITHOUT padding, because a
// DMA wave instruction writes lane l at base + 16 l, i.e. 8 whole rows (lane l -> 16-byte slot l & 7 of row l >> 3).  Bank
// conflicts of the ds_read_b128 fragment reads (lane -> row) are removed by an XOR swizzle: logical chunk c of a row lives in
// slot swizzled_chunk(row, c).  The XOR is its own inverse: the DMA side applies the same function to its slot on the per-lane
// SOURCE address, the fragment reads to the LDS address (guide rule 21).
__device__ __forceinline__ int swizzle_key(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swizzled_chunk(int row, int chunk) { return chunk ^ swizzle_key(row); }

// Workgroup `block` of the tile grid -> first pixel m0 and first channel n0 of its BM x BN tile (XCD remap, column-group raster)
template <int BM, int BN>
__device__ __forceinline__ void tile_origin(const ConvParams& p, int block, int& m0, int& n0) {
  int tile_m, tile_n;
  tile_coords(xcd_remap(block, p.tiles_m * p.tiles_n), p.tiles_m, p.tiles_n, tile_m, tile_n);
  m0 = tile_m * BM;
  n0 = tile_n * BN;
}

// Rows of group gy's GEMM (ConvParams::grows); the rows of a tile past them are neither loaded (zero page) nor stored.
__device__ __forceinline__ int group_rows(const ConvParams& p, int gy) {
  const bool i3 = (gy >> 2) == 3, j3 = (gy & 3) == 3;
  return i3 ? (j3 ? p.grows[3] : p.grows[1]) : (j3 ? p.grows[2] : p.grows[0]);
}

// tile_origin for a group of `mrows` <= p.M rows: the group's OWN ceil(mrows / BM) x tiles_n tiles are laid over the first
// workgroups of the grid (which is sized for p.M rows) and the rest return false - before their first barrier, the test is
// uniform.  Remapping p.tiles_m x tiles_n and dropping the tiles past mrows instead would leave the XCDs that own the last
// m-tiles (xcd_remap hands each XCD a contiguous range) without work in the trimmed groups while the first XCD still walks
// all of its tiles: the launch would take as long as the untrimmed one.  mrows == p.M: exactly tile_origin.
template <int BM, int BN>
__device__ __forceinline__ bool group_tile_origin(const ConvParams& p, int block, int mrows, int& m0, int& n0) {
  const int tiles_m = (mrows + BM - 1) / BM, ntiles = tiles_m * p.tiles_n;
  if (block >= ntiles) return false;
  int tile_m, tile_n;
  tile_coords(xcd_remap(block, ntiles), tiles_m, p.tiles_n, tile_m, tile_n);
  m0 = tile_m * BM;
  n0 = tile_n * BN;
  return true;
}

// K-split z reduces the K-steps [begin, begin + returned count); the count is <= 0 for a split past the end
__device__ __forceinline__ int split_range(const ConvParams& p, int z, int& begin) {
  begin = z * p.steps_per_split;
  return min(begin + p.steps_per_split, p.ksteps) - begin;
}

// One group of k = 8: 4 x TM x TN MFMAs.  Operands are (weights, activations): D col (lane) = pixel, D row (register) = channel
template <int TM, int TN>
__device__ __forceinline__ void mma_step(f32x16 (&acc)[TM][TN], const f32x4* fa, const f32x4* fb) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j][q], fa[i][q], acc[i][j], 0, 0, 0);
}

// (the one-accumulator wave of the 64x64 tile is held to 128 VGPRs: four workgroups per CU, as its 36 KB of LDS allow)
template <int WM, int WN, int TM, int TN, bool ALIGNED, bool WINO = false>
__global__ __launch_bounds__(64 * WM * WN, 2) void conv_igemm_f32(const ConvParams p) {
  static_assert(!WINO || ALIGNED, "the fused Winograd input transform needs C % 32 == 0");
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int RPP = NT / 8;                // tile rows staged per pass (8 threads x 16 B cover one row)
  constexpr int PA = BM / RPP, PB = BN / RPP;  // 16-byte chunks per thread per K-step
  static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the staging pass");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                        // [2][BM][36]
  float* Bs = smem + 2 * BM * LDS_PITCH;   // [2][BN][36]

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  const float* const px = p.x + (size_t)blockIdx.y * p.gx;
  const float* const pw = p.w + (size_t)blockIdx.y * p.gw;

  int m0, n0;
  const int mrows = group_rows(p, blockIdx.y);
  if (!group_tile_origin<BM, BN>(p, blockIdx.x, mrows, m0, n0)) return;

  const int step_begin = blockIdx.z * p.steps_per_split;   // (split_range written out: nsteps is formed below, where it is used)
  const int step_end = min(step_begin + p.steps_per_split, p.ksteps);

  // ---- per-thread staging geometry: thread t moves chunk kc of rows (t>>3) + RPP*i ---------------
  const int kc = t & 7, row0 = t >> 3;
  int a_base[PA], a_hi0[PA], a_wi0[PA];
  // WINO: V[xi][tile][c] = (B^T d B)[ci][cj] of the tile's 4x4 input patch d (rows 2ty-1.., cols 2tx-1.., zero outside the
  // map) is a signed sum of FOUR patch pixels: with B^T's rows (1,0,-1,0), (0,1,1,0), (0,-1,1,0), (0,1,0,-1) row ci combines
  // patch rows ra, rb as d[ra] + sr d[rb] and column cj likewise, in the order wino_input_kernel evaluates them
  // (rows first, then columns), so the fused GEMM is bit-identical to the two-launch form.
  constexpr int WPA = WINO ? PA : 1, WQ = WINO ? 4 : 1;
  int w_off[WPA][WQ];      // element offsets of the four pixels (-1: outside the map -> zero page)
  float w_sr = 1.f, w_sc = 1.f;
  if constexpr (WINO) {
    const int xi = blockIdx.y, ci = xi >> 2, cj = xi & 3;
    const int ra = ci == 0 ? 0 : (ci == 2 ? 2 : 1), rb = ci == 2 ? 1 : (ci == 3 ? 3 : 2);
    const int ca = cj == 0 ? 0 : (cj == 2 ? 2 : 1), cb = cj == 2 ? 1 : (cj == 3 ? 3 : 2);
    w_sr = ci == 1 ? 1.f : -1.f;
    w_sc = cj == 1 ? 1.f : -1.f;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const int m = m0 + i * RPP + row0;
      const int tx = m % p.wtw, t2 = m / p.wtw;
      const int ty = t2 % p.wth, img = t2 / p.wth;
      const int hr[2] = {2 * ty - 1 + ra, 2 * ty - 1 + rb}, wc[2] = {2 * tx - 1 + ca, 2 * tx - 1 + cb};
#pragma unroll
      for (int q = 0; q < 4; ++q) {      // q = 0: (ra, ca), 1: (rb, ca), 2: (ra, cb), 3: (rb, cb)
        const int hi = hr[q & 1], wi = wc[q >> 1];
        const bool ok = m < p.M && (unsigned)hi < (unsigned)p.wiH && (unsigned)wi < (unsigned)p.wiW;
        w_off[i][q] = ok ? ((img * p.wiH + hi) * p.wiW + wi) * p.C : -1;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int m = m0 + i * RPP + row0;
    if (!WINO && m < mrows) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      a_hi0[i] = ho * p.stride - p.pad;
      a_wi0[i] = wo * p.stride - p.pad;
      a_base[i] = ((img * p.H + a_hi0[i]) * p.W + a_wi0[i]) * p.C;
    } else {
      a_hi0[i] = -(1 << 20);  // never in range
      a_wi0[i] = 0;
      a_base[i] = 0;
    }
  }

  // two register sets: the tiles of steps s+1 and s+2 are in flight while step s computes
  f32x4 ra[2][PA], rb[2][PB];
  f32x4 rw[2][WPA][WQ];    // WINO: the four raw pixels per A chunk stay in flight; they are combined when the tile is stored
  typedef std::integral_constant<int, 0> Set0;
  typedef std::integral_constant<int, 1> Set1;
  // tap state for the ALIGNED path (C % 32 == 0: a K-step never straddles a tap)
  int tr = 0, ts = 0, tc = 0;
  if (ALIGNED) {
    const int kf = step_begin * BK;
    const int tap = kf / p.C;
    tc = kf - tap * p.C;
    tr = tap / p.S;
    ts = tap - tr * p.S;
  }

  // load_tiles is called for consecutive steps (the ALIGNED tap state advances by one step per call)
  auto load_tiles = [&](int step, auto set) {
    constexpr int SL = decltype(set)::value;
    const int kflat = step * BK + kc * 4;
    if constexpr (WINO) {
      const int koff = tc + kc * 4;          // R = S = 1: a K-step is a channel block
#pragma unroll
      for (int i = 0; i < PA; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          rw[SL][i][q] = *reinterpret_cast<const f32x4*>(w_off[i][q] >= 0 ? px + w_off[i][q] + koff : p.zero);
      tc += BK;
    } else if (ALIGNED) {
      const int koff = (tr * p.W + ts) * p.C + tc + kc * 4;
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const int hi = a_hi0[i] + tr, wi = a_wi0[i] + ts;
        const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        ra[SL][i] = *reinterpret_cast<const f32x4*>(ok ? px + a_base[i] + koff : p.zero);
      }
      tc += BK;
      if (tc == p.C) {
        tc = 0;
        if (++ts == p.S) { ts = 0; ++tr; }
      }
    } else {
      const int tap = kflat / p.C;
      const int c = kflat - tap * p.C;
      const int r = tap / p.S, s = tap - r * p.S;
      const int koff = (r * p.W + s) * p.C + c;
      const bool kok = kflat < p.Ktot;
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const int hi = a_hi0[i] + r, wi = a_wi0[i] + s;
        const bool ok = kok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        ra[SL][i] = *reinterpret_cast<const f32x4*>(ok ? px + a_base[i] + koff : p.zero);
      }
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int n = n0 + j * RPP + row0;
      const bool ok = n < p.K && kflat < p.Ktot;
      rb[SL][j] = *reinterpret_cast<const f32x4*>(ok ? pw + (size_t)n * p.Ktot + kflat : p.zero);
    }
  };
  auto store_tiles = [&](int buf, auto set) {
    constexpr int SL = decltype(set)::value;
    float* a = As + buf * BM * LDS_PITCH + row0 * LDS_PITCH + kc * 4;
    float* b = Bs + buf * BN * LDS_PITCH + row0 * LDS_PITCH + kc * 4;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      if constexpr (WINO) {
        const f32x4 lo = rw[SL][i][0] + w_sr * rw[SL][i][1];      // r[ci][ca] = d[ra][ca] +- d[rb][ca]
        const f32x4 hi = rw[SL][i][2] + w_sr * rw[SL][i][3];      // r[ci][cb]
        *reinterpret_cast<f32x4*>(a + i * RPP * LDS_PITCH) = lo + w_sc * hi;
      } else {
        *reinterpret_cast<f32x4*>(a + i * RPP * LDS_PITCH) = ra[SL][i];
      }
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) *reinterpret_cast<f32x4*>(b + j * RPP * LDS_PITCH) = rb[SL][j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment read offsets: lane (l&31) = row inside the 32x32 tile, (l>>5) selects k in {4h..4h+3}
  const int frag = (lane & 31) * LDS_PITCH + 4 * (lane >> 5);
  const int a_frag = (wr * TM * 32) * LDS_PITCH + frag;
  const int b_frag = (wc * TN * 32) * LDS_PITCH + frag;

  f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];  // two fragment sets: MFMAs on one, LDS reads into the other
  auto read_frags = [&](f32x4* fa, f32x4* fb, int buf, int kk) {
    const float* Ab = As + buf * BM * LDS_PITCH + a_frag + kk * 8;
    const float* Bb = Bs + buf * BN * LDS_PITCH + b_frag + kk * 8;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDS_PITCH);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDS_PITCH);
  };
  auto mma = [&](const f32x4* fa, const f32x4* fb) { mma_step(acc, fa, fb); };

  const int nsteps = step_end - step_begin;
  if (nsteps > 0) {
    load_tiles(step_begin, Set0{});
    store_tiles(0, Set0{});
    if (nsteps > 1) load_tiles(step_begin + 1, Set0{});  // tile t >= 1 waits in set (t - 1) & 1 until step t - 1 stores it
    if (nsteps > 2) load_tiles(step_begin + 2, Set1{});
  }
  __syncthreads();
  if (nsteps > 0) read_frags(fa0, fb0, 0, 0);

  int cur = 0;
  // one K-step; `set` holds tile it + 1 and is refilled with tile it + 3 once that one is in LDS.  STEADY: tiles it+1 and
  // it+3 exist - no conditions around the loads, so the compiler counts them and waits for the OLDER set only.
  auto kstep = [&](int it, auto set, auto steady) {
    constexpr bool STEADY = decltype(steady)::value;
    const bool more = STEADY || it + 1 < nsteps;
    read_frags(fa1, fb1, cur, 1);
    mma(fa0, fb0);
    read_frags(fa0, fb0, cur, 2);
    mma(fa1, fb1);
    if (more) store_tiles(cur ^ 1, set);
    read_frags(fa1, fb1, cur, 3);
    mma(fa0, fb0);
    if (STEADY || it + 3 < nsteps) load_tiles(step_begin + it + 3, set);
    __syncthreads();  // buffer cur^1 complete; every wave has its last fragments of buffer cur in registers
    if (more) read_frags(fa0, fb0, cur ^ 1, 0);
    mma(fa1, fb1);
    cur ^= 1;
  };
  int it = 0;
  for (; it + 4 < nsteps; it += 2) {
    kstep(it, Set0{}, std::true_type{});
    kstep(it + 1, Set1{}, std::true_type{});
  }
  for (; it < nsteps; it += 2) {
    kstep(it, Set0{}, std::false_type{});
    if (it + 1 < nsteps) kstep(it + 1, Set1{}, std::false_type{});
  }

  if (p.epi_lds && (p.K & 3) == 0)   // (uniform branch; every wave is past the K loop's last barrier and reads no LDS any more)
    conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows, smem + wave * 32 * LDS_PITCH);
  else
    conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows);
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant for the 8-wave tiles (C % 32 == 0): the A/B tiles go global -> LDS with
// global_load_lds_dwordx4 (no VGPR staging, no ds_write pass), three LDS stages, loads issued two K-steps
// ahead, ONE raw s_barrier per K-step behind a counted vmcnt.
//   LDS image and swizzle: see swizzled_chunk.  Out-of-range lanes (padding taps, M / K tails) read a zero page instead
//   of branching.
// Numerics are those of conv_igemm_f32 (same k order), so split_k == 1 results are bit-identical.
// ------------------------------------------------------------------------------------------------

template <int WM, int WN>
__global__ __launch_bounds__(512, 2) void conv_igemm_dma_f32(const ConvParams p) {
  constexpr int TM = 2, TN = 2;
  constexpr int BM = 64 * WM, BN = 64 * WN;
  static_assert(WM * WN == 8, "8 waves");
  constexpr int PA = BM / 64, PB = BN / 64;          // LDS-DMA instructions (8 rows each) per wave per K-step
  constexpr int STAGE = (BM + BN) * 32;              // floats per stage
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [3][BM + BN][32]

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  const float* const px = p.x + (size_t)blockIdx.y * p.gx;
  const float* const pw = p.w + (size_t)blockIdx.y * p.gw;
  int m0, n0, step_begin;
  const int mrows = group_rows(p, blockIdx.y);
  if (!group_tile_origin<BM, BN>(p, blockIdx.x, mrows, m0, n0)) return;
  const int nsteps = split_range(p, blockIdx.z, step_begin);

  // ---- per-lane sources: lane i of instruction q feeds row 8q + (i >> 3), physical chunk i & 7 -------------
  const int lrow = lane >> 3, lchunk = lane & 7;
  int a_base[PA], a_hi0[PA], a_wi0[PA], a_swz[PA];
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int row = (wave * PA + j) * 8 + lrow;
    const int m = m0 + row;
    a_swz[j] = swizzled_chunk(row, lchunk) * 4;
    if (m < mrows) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      a_hi0[j] = ho * p.stride - p.pad;
      a_wi0[j] = wo * p.stride - p.pad;
      a_base[j] = ((img * p.H + a_hi0[j]) * p.W + a_wi0[j]) * p.C;
    } else {
      a_hi0[j] = -(1 << 20);
      a_wi0[j] = 0;
      a_base[j] = 0;
    }
  }
  const float* b_src[PB];
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int row = (wave * PB + j) * 8 + lrow;
    const int n = n0 + row;
    b_src[j] = n < p.K ? pw + (size_t)n * p.Ktot + swizzled_chunk(row, lchunk) * 4 : nullptr;
  }
  int tr, ts, tc;
  {
    const int kf = step_begin * BK;
    const int tap = kf / p.C;
    tc = kf - tap * p.C;
    tr = tap / p.S;
    ts = tap - tr * p.S;
  }
  // issue() is called for consecutive steps (the tap state advances by one step per call)
  auto issue = [&](int step, int stage) {
    float* sA = smem + stage * STAGE + (wave * PA) * 8 * 32;
    float* sB = smem + stage * STAGE + BM * 32 + (wave * PB) * 8 * 32;
    const int koff = (tr * p.W + ts) * p.C + tc;
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      const int hi = a_hi0[j] + tr, wi = a_wi0[j] + ts;
      const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      const float* src = ok ? px + a_base[j] + koff + a_swz[j] : p.zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(sA + j * 8 * 32), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const float* src = b_src[j] ? b_src[j] + step * BK : p.zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(sB + j * 8 * 32), 16, 0, 0);
    }
    tc += BK;
    if (tc == p.C) {
      tc = 0;
      if (++ts == p.S) { ts = 0; ++tr; }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment reads: row = tile row of lane & 31, chunk 2*kk + (lane >> 5), XOR-swizzled
  int fa_row[TM], fa_x[TM], fb_row[TN], fb_x[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = (wr * TM + i) * 32 + (lane & 31);
    fa_row[i] = row * 32;
    fa_x[i] = swizzle_key(row);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = (wc * TN + j) * 32 + (lane & 31);
    fb_row[j] = BM * 32 + row * 32;
    fb_x[j] = swizzle_key(row);
  }
  const int lh = lane >> 5;
  f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  auto read_frags = [&](f32x4* fa, f32x4* fb, int stage, int kk) {
    const float* base = smem + stage * STAGE;
    const int c = 2 * kk + lh;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(base + fa_row[i] + ((c ^ fa_x[i]) << 2));
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(base + fb_row[j] + ((c ^ fb_x[j]) << 2));
  };
  auto mma = [&](const f32x4* fa, const f32x4* fb) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j][q], fa[i][q], acc[i][j], 0, 0, 0);
  };

  // Schedule of one K-step (4 groups of 16 MFMAs per wave).  The barrier sits in the MIDDLE of the step:
  //   group 0, 1   on stage s (its group-0 fragments were read at the end of the previous step)
  //   vmcnt + barrier: stage s+1 has landed for every wave, and every wave is past step s-1
  //   issue the loads of step s+2 into the stage step s-1 used
  //   group 2, then the group-0 fragment reads of stage s+1, group 3
  // so neither the barrier nor the first fragment reads of a stage leave the MFMA pipe without queued work.
  if (nsteps > 0) issue(step_begin, 0);
  if (nsteps > 1) issue(step_begin + 1, 1);
  if (nsteps > 0) {
    if (nsteps > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    read_frags(fa0, fb0, 0, 0);
  }
  int stage = 0;
  for (int s = 0; s < nsteps; ++s) {
    const int next = stage == 2 ? 0 : stage + 1;
    read_frags(fa1, fb1, stage, 1);
    mma(fa0, fb0);
    read_frags(fa0, fb0, stage, 2);
    mma(fa1, fb1);
    if (s + 1 < nsteps) {
      // only the loads of step s+1 are outstanding here (step s+2 is issued below)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (s + 2 < nsteps) issue(step_begin + s + 2, stage == 0 ? 2 : stage - 1);
    }
    read_frags(fa1, fb1, stage, 3);
    mma(fa0, fb0);
    if (s + 1 < nsteps) read_frags(fa0, fb0, next, 0);
    mma(fa1, fb1);
    stage = next;
  }
  if (p.epi_lds && (p.K & 3) == 0) {
    __syncthreads();   // the last step has no barrier behind its fragment reads: every wave must be done with the stages
    conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows, smem + wave * 32 * LDS_PITCH);
  } else {
    conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows);
  }
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA 128x128 tile, 4 waves, TWO LDS stages (64 KB): two workgroups per CU.  For the GEMMs with many
// output channels and a short reduction (layer4's 512 -> 2048 / 1024 -> 2048 expansions, the Winograd GEMMs): the
// 64x64 tile the autotuner otherwise picks there pulls 4x the bytes per FLOP from the L2s (6.4 TB/s, 1.88 GB per call),
// the 256x128 tile keeps one workgroup per CU whose epilogue nobody overlaps.  Same operand layout, swizzle, zero page
// and k order as conv_igemm_dma_f32: bit-identical results for split_k == 1.
// ------------------------------------------------------------------------------------------------
template <int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_igemm_dma2_f32(const ConvParams p) {
  constexpr int TM = 2, TN = 2;
  constexpr int BM = 64 * WM, BN = 64 * WN;
  static_assert(WM * WN == 4, "4 waves");
  constexpr int PA = BM / 32, PB = BN / 32;          // LDS-DMA instructions (8 rows each) per wave per K-step
  constexpr int STAGE = (BM + BN) * 32;              // floats per stage
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][BM + BN][32]

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  const float* const px = p.x + (size_t)blockIdx.y * p.gx;
  const float* const pw = p.w + (size_t)blockIdx.y * p.gw;
  int m0, n0, step_begin;
  const int mrows = group_rows(p, blockIdx.y);
  if (!group_tile_origin<BM, BN>(p, blockIdx.x, mrows, m0, n0)) return;
  const int nsteps = split_range(p, blockIdx.z, step_begin);

  // ---- per-lane sources: lane i of instruction q feeds row 8q + (i >> 3), physical chunk i & 7 -------------
  const int lrow = lane >> 3, lchunk = lane & 7;
  int a_base[PA], a_hi0[PA], a_wi0[PA], a_swz[PA];
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int row = (wave * PA + j) * 8 + lrow;
    const int m = m0 + row;
    a_swz[j] = swizzled_chunk(row, lchunk) * 4;
    if (m < mrows) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      a_hi0[j] = ho * p.stride - p.pad;
      a_wi0[j] = wo * p.stride - p.pad;
      a_base[j] = ((img * p.H + a_hi0[j]) * p.W + a_wi0[j]) * p.C;
    } else {
      a_hi0[j] = -(1 << 20);
      a_wi0[j] = 0;
      a_base[j] = 0;
    }
  }
  const float* b_src[PB];
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int row = (wave * PB + j) * 8 + lrow;
    const int n = n0 + row;
    b_src[j] = n < p.K ? pw + (size_t)n * p.Ktot + swizzled_chunk(row, lchunk) * 4 : nullptr;
  }
  int tr, ts, tc;
  {
    const int kf = step_begin * BK;
    const int tap = kf / p.C;
    tc = kf - tap * p.C;
    tr = tap / p.S;
    ts = tap - tr * p.S;
  }
  // issue() is called for consecutive steps (the tap state advances by one step per call)
  auto issue = [&](int step, int stage) {
    float* sA = smem + stage * STAGE + (wave * PA) * 8 * 32;
    float* sB = smem + stage * STAGE + BM * 32 + (wave * PB) * 8 * 32;
    const int koff = (tr * p.W + ts) * p.C + tc;
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      const int hi = a_hi0[j] + tr, wi = a_wi0[j] + ts;
      const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      const float* src = ok ? px + a_base[j] + koff + a_swz[j] : p.zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(sA + j * 8 * 32), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const float* src = b_src[j] ? b_src[j] + step * BK : p.zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(sB + j * 8 * 32), 16, 0, 0);
    }
    tc += BK;
    if (tc == p.C) {
      tc = 0;
      if (++ts == p.S) { ts = 0; ++tr; }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment reads: row = tile row of lane & 31, chunk 2*kk + (lane >> 5), XOR-swizzled
  int fa_row[TM], fa_x[TM], fb_row[TN], fb_x[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = (wr * TM + i) * 32 + (lane & 31);
    fa_row[i] = row * 32;
    fa_x[i] = swizzle_key(row);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = (wc * TN + j) * 32 + (lane & 31);
    fb_row[j] = BM * 32 + row * 32;
    fb_x[j] = swizzle_key(row);
  }
  const int lh = lane >> 5;
  f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  auto read_frags = [&](f32x4* fa, f32x4* fb, int stage, int kk) {
    const float* base = smem + stage * STAGE;
    const int c = 2 * kk + lh;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(base + fa_row[i] + ((c ^ fa_x[i]) << 2));
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(base + fb_row[j] + ((c ^ fb_x[j]) << 2));
  };
  auto mma = [&](const f32x4* fa, const f32x4* fb) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j][q], fa[i][q], acc[i][j], 0, 0, 0);
  };

  // Two stages, one K-step of look-ahead: the barrier at the END of step s says "every wave has its last fragments of
  // stage s in registers and every wave's part of stage s+1 has landed", so the loads of step s+2 may overwrite stage s
  // right after it.  The fragment reads that follow a barrier leave a bubble in this workgroup's MFMA stream; the
  // second workgroup of the CU (64 KB of LDS each) fills it.
  if (nsteps > 0) {
    issue(step_begin, 0);
    if (nsteps > 1) issue(step_begin + 1, 1);
    if (nsteps > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int s = 0; s < nsteps; ++s) {
    const int stage = s & 1;
    read_frags(fa0, fb0, stage, 0);
    read_frags(fa1, fb1, stage, 1);
    mma(fa0, fb0);
    read_frags(fa0, fb0, stage, 2);
    mma(fa1, fb1);
    read_frags(fa1, fb1, stage, 3);
    mma(fa0, fb0);
    if (s + 1 < nsteps) {
      // the last fragments of this stage are in registers (the MFMAs below only read registers): wait for the loads of
      // step s+1 (the only ones outstanding), meet the other waves, refill this stage with step s+2
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (s + 2 < nsteps) issue(step_begin + s + 2, stage);
    }
    mma(fa1, fb1);
  }
  if (p.epi_lds && (p.K & 3) == 0) {
    __syncthreads();
    conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows, smem + wave * 32 * LDS_PITCH);
  } else {
    conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows);
  }
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA through BUFFER loads (buffer_load_dwordx4 ... lds), three stages, any 4- or 8-wave tile: written for the small
// tiles, above all the 64x64 tile whose waves own ONE 32x32 accumulator.
//
// Why (profiles/r05_mfma_chain.txt, profiles/r05_conv_pmc_probe.md): on gfx950 nothing a wave issues hides behind its own
// fp32 MFMAs for free - beside a dependent v_mfma_f32_32x32x2_f32 chain one wave per SIMD pays ~7 cycles per v_fma, ~5 per
// SALU instruction, ~66 per ds_write_b128 and ~85 per global_load_dwordx4 of MFMA time.  The register-staged 64x64 kernel
// issues, per 16 MFMAs (1024 cycles), 4 global loads + 4 ds_write_b128 + ~27 VALU + ~25 SALU instructions: a wave alone on
// its SIMD keeps the matrix pipe busy 53 % of its life, and 2.7 such waves per SIMD only reach 50 %.  This kernel removes the
// instructions instead of rescheduling them:
//   * tiles go global -> LDS by DMA: no VGPR staging, no ds_write pass, no vmcnt -> ds_write dependency;
//   * addresses are  buffer resource (SGPRs) + per-lane byte offset (VGPR, constant while the tap is) + a scalar offset that
//     advances with the K-step: ZERO vector instructions per K-step on a 1x1 layer (a 3x3 layer recomputes its per-lane
//     offsets once per tap, i.e. every C/32 steps);
//   * out-of-range lanes (padding taps, M / K tails) carry the offset 2^31: the buffer's range check returns zeros, no
//     zero page, no select.  (Activation and filter ranges must be < 2 GB: the host falls back to the other kernels.)
// LDS layout, XOR swizzle, k order and epilogue are those of conv_igemm_dma_f32: results are bit-identical to every other
// kernel for split_k == 1.
// ------------------------------------------------------------------------------------------------
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(64 * WM * WN, (TM * TN == 1) ? 3 : 2) void conv_igemm_buf_f32(const ConvParams p) {
  constexpr int NW = WM * WN;
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int PA = BM / (8 * NW), PB = BN / (8 * NW);   // DMA instructions (8 rows of 128 bytes each) per wave per K-step
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile rows must be a multiple of the DMA pass");
  constexpr int STAGE = (BM + BN) * 32;                   // floats per stage
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [3][BM + BN][32]

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  int m0, n0, step_begin;
  const int mrows = group_rows(p, blockIdx.y);
  if (!group_tile_origin<BM, BN>(p, blockIdx.x, mrows, m0, n0)) return;
  const int nsteps = split_range(p, blockIdx.z, step_begin);

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x + (size_t)blockIdx.y * p.gx), 0, (int)p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.w + (size_t)blockIdx.y * p.gw), 0, (int)p.wbytes, 0x00020000);

  // ---- per-lane sources: lane i of instruction j feeds row 8 (wave PA + j) + (i >> 3), physical chunk i & 7 -------------
  const int lrow = lane >> 3, lchunk = lane & 7;
  int a_pix[PA], a_hi0[PA], a_wi0[PA];      // byte offset of pixel (img, hi0, wi0), -1 for a row past M
  unsigned a_swz[PA], vA[PA], vB[PB];
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int row = (wave * PA + j) * 8 + lrow;
    const int m = m0 + row;
    a_swz[j] = (unsigned)(swizzled_chunk(row, lchunk) * 16);
    if (m < mrows) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      a_hi0[j] = ho * p.stride - p.pad;
      a_wi0[j] = wo * p.stride - p.pad;
      a_pix[j] = ((img * p.H + a_hi0[j]) * p.W + a_wi0[j]) * p.C * 4;
    } else {
      a_hi0[j] = -(1 << 20);
      a_wi0[j] = 0;
      a_pix[j] = 0;
    }
    vA[j] = OOB;
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int row = (wave * PB + j) * 8 + lrow;
    const int n = n0 + row;
    vB[j] = n < p.K ? (unsigned)(n * p.Ktot * 4 + swizzled_chunk(row, lchunk) * 16) : OOB;
  }
  int tr, ts, tc;
  {
    const int kf = step_begin * BK;
    const int tap = kf / p.C;
    tc = kf - tap * p.C;
    tr = tap / p.S;
    ts = tap - tr * p.S;
  }
  bool new_tap = true;
  // issue() is called for consecutive steps (the tap state advances by one step per call)
  auto issue = [&](int step, int stage) {
    float* sA = smem + stage * STAGE + (wave * PA) * 8 * 32;
    float* sB = smem + stage * STAGE + BM * 32 + (wave * PB) * 8 * 32;
    if (new_tap) {                          // uniform: once per tap (once per kernel on a 1x1 layer)
      const int toff = (tr * p.W + ts) * p.C * 4;
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        const int hi = a_hi0[j] + tr, wi = a_wi0[j] + ts;
        const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        vA[j] = ok ? (unsigned)(a_pix[j] + toff) + a_swz[j] : OOB;
      }
    }
    const int sa = tc * 4, sb = step * (BK * 4);
#pragma unroll
    for (int j = 0; j < PA; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr)(sA + j * 8 * 32), 16, (int)vA[j], sa, 0, 0);
#pragma unroll
    for (int j = 0; j < PB; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr)(sB + j * 8 * 32), 16, (int)vB[j], sb, 0, 0);
    tc += BK;
    new_tap = tc == p.C;
    if (new_tap) {
      tc = 0;
      if (++ts == p.S) { ts = 0; ++tr; }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment reads: row = tile row of lane & 31, logical chunk 2 kk + (lane >> 5), XOR-swizzled; the four chunk offsets of a
  // row are kept in registers (no address arithmetic in the loop)
  const int lh = lane >> 5;
  int fa_off[TM][4], fb_off[TN][4];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = (wr * TM + i) * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) fa_off[i][kk] = row * 32 + (swizzled_chunk(row, 2 * kk + lh) << 2);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = (wc * TN + j) * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) fb_off[j][kk] = BM * 32 + row * 32 + (swizzled_chunk(row, 2 * kk + lh) << 2);
  }
  f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  auto read_frags = [&](f32x4* fa, f32x4* fb, int stage, int kk) {
    const float* base = smem + stage * STAGE;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(base + fa_off[i][kk]);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(base + fb_off[j][kk]);
  };
  auto mma = [&](const f32x4* fa, const f32x4* fb) { mma_step(acc, fa, fb); };

  // Schedule of one K-step as in conv_igemm_dma_f32: the barrier sits in the MIDDLE of the step (stage s+1 has landed for
  // every wave and every wave is past step s-1), the loads of step s+2 are issued right behind it.
  if (nsteps > 0) issue(step_begin, 0);
  if (nsteps > 1) issue(step_begin + 1, 1);
  if (nsteps > 0) {
    if (nsteps > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    read_frags(fa0, fb0, 0, 0);
  }
  int stage = 0;
  for (int s = 0; s < nsteps; ++s) {
    const int next = stage == 2 ? 0 : stage + 1;
    read_frags(fa1, fb1, stage, 1);
    mma(fa0, fb0);
    read_frags(fa0, fb0, stage, 2);
    mma(fa1, fb1);
    if (s + 1 < nsteps) {
      // only the loads of step s+1 are outstanding here (step s+2 is issued below)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (s + 2 < nsteps) issue(step_begin + s + 2, stage == 0 ? 2 : stage - 1);
    }
    read_frags(fa1, fb1, stage, 3);
    mma(fa0, fb0);
    if (s + 1 < nsteps) read_frags(fa0, fb0, next, 0);
    mma(fa1, fb1);
    stage = next;
  }
  if (p.epi_lds && (p.K & 3) == 0) {
    __syncthreads();   // the last step has no barrier behind its fragment reads: every wave must be done with the stages
    conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows, smem + wave * 32 * LDS_PITCH);
  } else {
    conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, mrows);
  }
}

// ------------------------------------------------------------------------------------------------
// PERSISTENT form of the buffer-load LDS-DMA kernel for the 64x64 tile (plan tile index 13).
//
// Section 4.10 of DESIGN.md: a 64x64 tile of a short reduction (layer1-3: 2-16 K-steps, ~1-8 us of MFMA work) is launched,
// computes its addresses, waits for its first two DMA round trips, runs its K loop, stores and exits - the skeleton costs
// as much as the loop, and co-resident workgroups only partly cover each other's skeletons.  Here a workgroup is resident for
// the whole launch (grid = 2 workgroups per CU at most) and walks its WORK ITEMS (tile x group x K-split, item i, i + grid,
// ...) as ONE stream of K-steps through the same three-stage LDS ring: while the last K-steps of an item compute, the DMA of the
// next item's first steps is already in flight (a producer cursor runs two steps ahead of the consumer cursor, across item
// boundaries), so from its second item on a workgroup pays neither dispatch nor address set-up nor a cold first load before
// its MFMAs - only the epilogue (LDS transpose in a patch of its own, stores) sits between two items' MFMAs.
// Same LDS image, k order and epilogue arithmetic as conv_igemm_buf_f32: bit-identical for split_k == 1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void conv_igemm_pbuf_f32(const ConvParams p, int groups, int splits) {
  constexpr int WN = 2, TM = 1, TN = 1;
  constexpr int BM = 64, BN = 64, PA = 2, PB = 2;       // 4 waves x 8 rows per DMA instruction: 2 + 2 instructions per wave and step
  constexpr int STAGE = (BM + BN) * 32;                 // floats per stage
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [3][BM + BN][32] ring + [4 waves][32][36] epilogue patches
  float* const patch = smem + 3 * STAGE + (threadIdx.x >> 6) * 32 * LDS_PITCH;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  const int ntiles = p.tiles_m * p.tiles_n;
  const int total = ntiles * groups * splits;
  const int stride = gridDim.x;

  // item -> (tile, group, split); tiles in the XCD-aware raster order of the other kernels
  auto item_coords = [&](int item, int& m0, int& n0, int& g, int& z) {
    const int tl = item % ntiles, gz = item / ntiles;
    g = gz % groups;
    z = gz / groups;
    tile_origin<BM, BN>(p, tl, m0, n0);
  };

  // ---- producer cursor: the item / step whose tiles are issued next ------------------------------------------------------
  const int lrow = lane >> 3, lchunk = lane & 7;
  int p_item = blockIdx.x, p_step = 0, p_nst = 0, p_begin = 0, p_stage = 0;
  int a_pix[PA], a_hi0[PA], a_wi0[PA];
  unsigned a_swz[PA], vA[PA], vB[PB];
  int tr = 0, ts = 0, tc = 0;
  bool new_tap = true;
  __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.xbytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)p.wbytes, 0x00020000);
  auto producer_setup = [&]() {                        // geometry of item p_item (uniform: p_item < total)
    int m0, n0, g, z;
    item_coords(p_item, m0, n0, g, z);
    p_nst = split_range(p, z, p_begin);
    p_step = 0;
    rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x + (size_t)g * p.gx), 0, (int)p.xbytes, 0x00020000);
    rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w + (size_t)g * p.gw), 0, (int)p.wbytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      const int row = (wave * PA + j) * 8 + lrow;
      const int m = m0 + row;
      a_swz[j] = (unsigned)(swizzled_chunk(row, lchunk) * 16);
      if (m < p.M) {
        const int img = m / (p.Ho * p.Wo);
        const int rem = m - img * p.Ho * p.Wo;
        const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
        a_hi0[j] = ho * p.stride - p.pad;
        a_wi0[j] = wo * p.stride - p.pad;
        a_pix[j] = ((img * p.H + a_hi0[j]) * p.W + a_wi0[j]) * p.C * 4;
      } else {
        a_hi0[j] = -(1 << 20);
        a_wi0[j] = 0;
        a_pix[j] = 0;
      }
      vA[j] = OOB;
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int row = (wave * PB + j) * 8 + lrow;
      const int n = n0 + row;
      vB[j] = n < p.K ? (unsigned)(n * p.Ktot * 4 + swizzled_chunk(row, lchunk) * 16) : OOB;
    }
    const int kf = p_begin * BK;
    const int tap = kf / p.C;
    tc = kf - tap * p.C;
    tr = tap / p.S;
    ts = tap - tr * p.S;
    new_tap = true;
  };
  // issues the tiles of the producer's step into the producer's stage and advances the cursor; false when the stream is over
  auto issue_next = [&]() -> bool {
    if (p_item >= total) return false;
    float* sA = smem + p_stage * STAGE + (wave * PA) * 8 * 32;
    float* sB = smem + p_stage * STAGE + BM * 32 + (wave * PB) * 8 * 32;
    if (new_tap) {
      const int toff = (tr * p.W + ts) * p.C * 4;
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        const int hi = a_hi0[j] + tr, wi = a_wi0[j] + ts;
        const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        vA[j] = ok ? (unsigned)(a_pix[j] + toff) + a_swz[j] : OOB;
      }
    }
    const int sa = tc * 4, sb = (p_begin + p_step) * (BK * 4);
#pragma unroll
    for (int j = 0; j < PA; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr)(sA + j * 8 * 32), 16, (int)vA[j], sa, 0, 0);
#pragma unroll
    for (int j = 0; j < PB; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr)(sB + j * 8 * 32), 16, (int)vB[j], sb, 0, 0);
    tc += BK;
    new_tap = tc == p.C;
    if (new_tap) {
      tc = 0;
      if (++ts == p.S) { ts = 0; ++tr; }
    }
    p_stage = p_stage == 2 ? 0 : p_stage + 1;
    if (++p_step == p_nst) {
      p_item += stride;
      if (p_item < total) producer_setup();
    }
    return true;
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  const int lh = lane >> 5;
  int fa_off[4], fb_off[4];   // (must match swizzle_key / swizzled_chunk; spelled out here: through the function this kernel takes 116 VGPRs, not 114)
  {
    const int rowa = wr * 32 + (lane & 31), rowb = wc * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      fa_off[kk] = rowa * 32 + (((2 * kk + lh) ^ ((rowa >> 1) & 7)) << 2);
      fb_off[kk] = BM * 32 + rowb * 32 + (((2 * kk + lh) ^ ((rowb >> 1) & 7)) << 2);
    }
  }
  f32x4 fa0, fb0, fa1, fb1;
  auto read_frags = [&](f32x4& fa, f32x4& fb, int stage, int kk) {
    const float* base = smem + stage * STAGE;
    fa = *reinterpret_cast<const f32x4*>(base + fa_off[kk]);
    fb = *reinterpret_cast<const f32x4*>(base + fb_off[kk]);
  };
  auto mma = [&](const f32x4& fa, const f32x4& fb) { mma_step(acc, &fa, &fb); };

  if (blockIdx.x >= total) return;                     // (uniform) more workgroups than items: nothing to do
  // The stream: step g of this workgroup's items lives in stage g % 3.  `ahead` = steps issued - steps consumed (1 or 2 at the
  // top of a step): ahead >= 2 <=> a next step exists.
  producer_setup();
  issue_next();                                        // stream step 0
  int ahead = issue_next() ? 2 : 1;                    // stream step 1
  if (ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  read_frags(fa0, fb0, 0, 0);
  int stage = 0;
  for (int item = blockIdx.x; item < total; item += stride) {
    int m0, n0, g, z, begin;
    item_coords(item, m0, n0, g, z);
    const int nst = split_range(p, z, begin);
    for (int s = 0; s < nst; ++s) {
      const int next = stage == 2 ? 0 : stage + 1;
      const bool more = ahead >= 2;
      read_frags(fa1, fb1, stage, 1);
      mma(fa0, fb0);
      read_frags(fa0, fb0, stage, 2);
      mma(fa1, fb1);
      if (more) {
        // everything this wave has issued is waited for: the DMA of the next stream step and, behind an item boundary, the
        // previous item's stores (issued half a K-step ago)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (issue_next()) ++ahead;                     // stream step + 2 goes into the stage step - 1 used
      }
      read_frags(fa1, fb1, stage, 3);
      mma(fa0, fb0);
      if (more) read_frags(fa0, fb0, next, 0);
      mma(fa1, fb1);
      stage = next;
      --ahead;
    }
    if (p.epi_lds && (p.K & 3) == 0) conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, p.M, patch, g, z);
    else conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, p.M, g, z);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  }
}

// Split-K second pass: y = act((sum_z partial[z]) * scale + shift + res), slabs summed in z order.
__global__ __launch_bounds__(256) void conv_splitk_epilogue(const float* __restrict__ partial, int splits,
                                                           size_t mk, int K, const float* scale,
                                                           const float* shift, const float* res, float* y,
                                                           int relu, const float* mask, const float* mscale) {
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < mk; o += (size_t)gridDim.x * blockDim.x) {
    float v = partial[o];
    for (int z = 1; z < splits; ++z) v += partial[(size_t)z * mk + o];
    const int n = (int)(o % K);
    v = v * (scale ? scale[n] : 1.f) + (shift ? shift[n] : 0.f);
    if (res) v += res[o];
    if (relu) v = frcnn::relu_f32(v);
    if (mask) v = frcnn::relu_open(mask[o]) ? v * (mscale ? mscale[n] : 1.f) : 0.f;
    y[o] = v;
  }
}

// ---- launching ---------------------------------------------------------------------------------------------------------
// One thin wrapper per kernel family of the implicit GEMM: its LDS bytes, its block size and, for the persistent kernel,
// its grid and two extra arguments.  p.tiles_m / tiles_n are set by launch_gemm.
dim3 tile_grid(const ConvArgs& p, int splits, int groups) { return dim3(p.tiles_m * p.tiles_n, groups, splits); }

template <int WM, int WN, int TM, int TN, bool ALIGNED, bool WINO = false>
int launch_reg(const ConvArgs& p, int splits, int groups, hipStream_t stream) {   // register-staged, two stages of padded rows
  constexpr size_t lds = (size_t)2 * 32 * (TM * WM + TN * WN) * LDS_PITCH * sizeof(float);
  return launch_kernel<conv_igemm_f32<WM, WN, TM, TN, ALIGNED, WINO>>("conv_igemm_f32", 0, tile_grid(p, splits, groups), 64 * WM * WN,
                                                                      lds, stream, kernel_arg(p));
}
template <int WM, int WN>
int launch_dma(const ConvArgs& p, int splits, int groups, hipStream_t stream) {   // LDS-DMA, three stages, 8 waves of 2x2 tiles
  constexpr size_t lds = (size_t)3 * 64 * (WM + WN) * 32 * sizeof(float);
  return launch_kernel<conv_igemm_dma_f32<WM, WN>>("conv_igemm_dma_f32", 0, tile_grid(p, splits, groups), 512, lds, stream, kernel_arg(p));
}
int launch_dma2(const ConvArgs& p, int splits, int groups, hipStream_t stream) {   // LDS-DMA, two stages, 128x128
  constexpr size_t lds = (size_t)2 * (128 + 128) * 32 * sizeof(float);
  return launch_kernel<conv_igemm_dma2_f32<2, 2>>("conv_igemm_dma2_f32", 0, tile_grid(p, splits, groups), 256, lds, stream, kernel_arg(p));
}
template <int WM, int WN, int TM, int TN>
int launch_buf(const ConvArgs& p, int splits, int groups, hipStream_t stream) {   // LDS-DMA through buffer loads, three stages
  constexpr size_t lds = (size_t)3 * 32 * (TM * WM + TN * WN) * 32 * sizeof(float);
  return launch_kernel<conv_igemm_buf_f32<WM, WN, TM, TN>>("conv_igemm_buf_f32", 0, tile_grid(p, splits, groups), 64 * WM * WN, lds,
                                                           stream, kernel_arg(p));
}
int launch_pbuf(const ConvArgs& p, int splits, int groups, hipStream_t stream) {   // the same, 64x64, persistent workgroups
  constexpr size_t lds = ((size_t)3 * (64 + 64) * 32 + (size_t)4 * 32 * LDS_PITCH) * sizeof(float);
  const long total = (long)p.tiles_m * p.tiles_n * groups * splits;
  const dim3 grid((unsigned)std::min<long>(total, 2L * NUM_CU));      // two resident workgroups per CU (66 KB of LDS each)
  return launch_kernel<conv_igemm_pbuf_f32>("conv_igemm_pbuf_f32", 0, grid, 256, lds, stream, kernel_arg(p), groups, splits);
}

// ---- plan tiles --------------------------------------------------------------------------------------------------------
// A plan names its kernel by an index into kTiles.  The indices are the serialised form of plan tables (frcnn_conv2d_export_plans),
// so rows are appended, never moved.  A row: the block tile (64*tm) x (64*tn) = (32*WTM*WM) x (32*WTN*WN), its register-staged
// kernel, and up to two alternatives tried in order when C % 32 == 0 - the first one whose staging-mode set holds the current
// frcnn_conv2d_set_staging mode and whose operand bound is met runs instead of the register-staged kernel (resolve_tile).
constexpr unsigned kModes123 = 0xE, kMode2 = 1u << 2, kMode3 = 1u << 3;
template <int WM, int WN, int TM, int TN>
constexpr TileCfg tile_row(TileAlt a0, TileAlt a1 = TileAlt{nullptr, 0, false}) {
  return TileCfg{WM * TM / 2, WN * TN / 2, WM, WN, TM, TN, {launch_reg<WM, WN, TM, TN, false>, launch_reg<WM, WN, TM, TN, true>}, {a0, a1}};
}
constexpr TileCfg kTiles[kNumTiles] = {
    // 0 .. 5, the six tile shapes - all that choose_plan or a forced tile selects: the buffer-load kernel in staging mode 3, else
    tile_row<4, 2, 2, 2>({launch_buf<4, 2, 2, 2>, kMode3, true}, {launch_dma<4, 2>, kModes123, false}),  // 256x128, 8 waves, one workgroup per CU: LDS-DMA
    tile_row<2, 4, 2, 2>({launch_buf<2, 4, 2, 2>, kMode3, true}, {launch_dma<2, 4>, kModes123, false}),  // 128x256, 8 waves: LDS-DMA
    tile_row<2, 2, 2, 2>({launch_buf<2, 2, 2, 2>, kMode3, true}, {launch_dma2, kMode2, false}),  // 128x128, 4 waves, two workgroups per CU (mode 2: test hook)
    tile_row<2, 2, 2, 1>({launch_buf<2, 2, 2, 1>, kMode3, true}),     // 128x64
    tile_row<2, 2, 1, 2>({launch_buf<2, 2, 1, 2>, kMode3, true}),     // 64x128
    tile_row<2, 2, 1, 1>({launch_buf<2, 2, 1, 1>, kMode3, true}),     // 64x64
    // 6 .. 13, LDS-DMA variants the autotuner times next to them, in every staging mode but 0
    tile_row<2, 2, 2, 2>({launch_dma2, kModes123, false}),            // 128x128, two stages: two workgroups per CU
    tile_row<2, 2, 1, 1>({launch_buf<2, 2, 1, 1>, kModes123, true}),  // 64x64, through buffer loads, three stages
    tile_row<2, 2, 2, 1>({launch_buf<2, 2, 2, 1>, kModes123, true}),  // 128x64, the same kernel
    tile_row<2, 2, 1, 2>({launch_buf<2, 2, 1, 2>, kModes123, true}),  // 64x128
    tile_row<2, 2, 2, 2>({launch_buf<2, 2, 2, 2>, kModes123, true}),  // 128x128, 96 KB of LDS: one workgroup per CU
    tile_row<4, 2, 2, 2>({launch_buf<4, 2, 2, 2>, kModes123, true}),  // 256x128, 8 waves (else register-staged, unlike index 0)
    tile_row<2, 4, 2, 2>({launch_buf<2, 4, 2, 2>, kModes123, true}),  // 128x256, 8 waves (likewise, unlike index 1)
    tile_row<2, 2, 1, 1>({launch_pbuf, kModes123, true}),             // 64x64, PERSISTENT workgroups walking their tiles as one K-step stream
};
static_assert(kTiles[kTile128x128].tm == 2 && kTiles[kTile128x128].tn == 2 && kTiles[kTile64x64].tm == 1 && kTiles[kTile64x64].tn == 1 &&
              kTile128x128 < kNumShapes && kTile64x64 < kNumShapes, "the named rows are the register-staged 128x128 and 64x64 tiles");

// the launch function of plan tile `idx`: aligned = C % 32 == 0, staging = the frcnn_conv2d_set_staging mode, small = both operands < 2 GB
constexpr ConvLaunch resolve_tile(int idx, bool aligned, int staging, bool small) {
  if (aligned)
    for (const TileAlt& a : kTiles[idx].alt)
      if (a.launch && ((a.modes >> staging) & 1) && (small || !a.small)) return a.launch;
  return kTiles[idx].reg[aligned];
}

// What every index runs, pinned at compile time.  tile_is: `dflt` with aligned, small operands in the default staging mode 1;
// the tile's register-staged kernel in staging mode 0 and for every unaligned C.
template <int WM, int WN, int TM, int TN>
constexpr bool tile_is(int idx, ConvLaunch dflt) {
  bool ok = resolve_tile(idx, true, 1, true) == dflt;
  for (int s = 0; s < 4; ++s)
    for (int small = 0; small < 2; ++small)
      ok = ok && resolve_tile(idx, false, s, small) == launch_reg<WM, WN, TM, TN, false> &&
           resolve_tile(idx, true, 0, small) == launch_reg<WM, WN, TM, TN, true>;
  return ok;
}
static_assert(kNumTiles == 14 && tile_is<4, 2, 2, 2>(0, launch_dma<4, 2>) && tile_is<2, 4, 2, 2>(1, launch_dma<2, 4>) &&
              tile_is<2, 2, 2, 2>(kTile128x128, launch_reg<2, 2, 2, 2, true>) && tile_is<2, 2, 2, 1>(3, launch_reg<2, 2, 2, 1, true>) &&
              tile_is<2, 2, 1, 2>(4, launch_reg<2, 2, 1, 2, true>) && tile_is<2, 2, 1, 1>(kTile64x64, launch_reg<2, 2, 1, 1, true>) &&
              tile_is<2, 2, 2, 2>(6, launch_dma2) && tile_is<2, 2, 1, 1>(7, launch_buf<2, 2, 1, 1>) &&
              tile_is<2, 2, 2, 1>(8, launch_buf<2, 2, 2, 1>) && tile_is<2, 2, 1, 2>(9, launch_buf<2, 2, 1, 2>) &&
              tile_is<2, 2, 2, 2>(10, launch_buf<2, 2, 2, 2>) && tile_is<4, 2, 2, 2>(11, launch_buf<4, 2, 2, 2>) &&
              tile_is<2, 4, 2, 2>(12, launch_buf<2, 4, 2, 2>) && tile_is<2, 2, 1, 1>(13, launch_pbuf),
              "plan tile indices are serialised (profiles/, exported tables): index -> kernel must stay as listed");
static_assert(resolve_tile(0, true, 3, true) == launch_buf<4, 2, 2, 2> && resolve_tile(0, true, 3, false) == launch_dma<4, 2> &&
              resolve_tile(0, true, 1, false) == launch_dma<4, 2> && resolve_tile(kTile128x128, true, 2, false) == launch_dma2 &&
              resolve_tile(kTile128x128, true, 3, true) == launch_buf<2, 2, 2, 2> &&
              resolve_tile(kTile128x128, true, 3, false) == launch_reg<2, 2, 2, 2, true> &&
              resolve_tile(kTile64x64, true, 3, true) == launch_buf<2, 2, 1, 1> && resolve_tile(6, true, 3, false) == launch_dma2 &&
              resolve_tile(11, true, 1, false) == launch_reg<4, 2, 2, 2, true> && resolve_tile(12, true, 3, false) == launch_reg<2, 4, 2, 2, true> &&
              resolve_tile(13, true, 2, false) == launch_reg<2, 2, 1, 1, true> && resolve_tile(13, true, 3, true) == launch_pbuf,
              "fall-backs: index 0 / 1 fall back to LDS-DMA, 11 / 12 to the register-staged kernel");
}  // namespace

const TileCfg& frcnn::conv::tile_cfg(int idx) { return kTiles[idx]; }

// device address of g_zero_page, resolved once (hipGetSymbolAddress is a host-side lookup: legal during stream capture)
const float* frcnn::conv::zero_page_address() {
  static std::atomic<const float*> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  const float* z = cached[dev].load();
  if (!z) {
    void* ptr = nullptr;
    if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_zero_page)) != hipSuccess) return nullptr;
    z = static_cast<const float*>(ptr);
    cached[dev].store(z);
  }
  return z;
}

// launch the GEMM kernel of one plan: the tile's kernel for this C, staging mode and operand size (resolve_tile)
int frcnn::conv::launch_gemm(ConvArgs p, const Plan& pl, long M, int k, int groups, hipStream_t stream) {
  const TileCfg& tc = kTiles[pl.cfg];
  p.steps_per_split = pl.steps_per_split;
  const int bm = 64 * tc.tm, bn = 64 * tc.tn;
  p.tiles_m = (p.M + bm - 1) / bm;
  p.tiles_n = (k + bn - 1) / bn;
  const bool aligned = (p.C % BK) == 0;
  if (pl.fuse_in) {
    if (pl.cfg != kTile64x64 || !aligned) return frcnn::fail(FRCNN_ERR_ARG, "conv2d: fused Winograd input needs the 64x64 tile and C %% 32 == 0");
    return launch_reg<2, 2, 1, 1, true, true>(p, 1, groups, stream);
  }
  return resolve_tile(pl.cfg, aligned, g_use_dma, p.xbytes && p.wbytes)(p, pl.splits, groups, stream);
}

// the second pass of a split-K plan over the slabs launch_gemm wrote (profile kind 1)
int frcnn::conv::launch_splitk_epilogue(const float* partial, int splits, long M, int k, const float* scale, const float* shift,
                                        const float* residual, float* y, int relu, const float* mask, const float* mscale,
                                        hipStream_t stream) {
  const size_t mk = (size_t)M * k;
  const int blocks = (int)std::min<size_t>((mk + 255) / 256, 2048);
  return launch_kernel<conv_splitk_epilogue>("conv_splitk_epilogue", 1, dim3(blocks), 256, 0, stream, partial, splits,
                                             mk, k, scale, shift, residual, y, relu, mask, mscale);
}

// ------------------------------------------------------------------------------------------------
// bf16-operand forward convolution (frcnn_conv2d_fwd_bf16): the GEMM of conv_igemm_f32<..., ALIGNED = true> on
// v_mfma_f32_32x32x16_bf16 - sixteen k per instruction, fp32 accumulation.  Activations and outputs stay fp32 NHWC in
// HBM: an activation chunk is rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) between its global load and its LDS
// store; the filter arrives packed (frcnn_conv2d_pack_bf16, KRSC 16-bit words).  A K-step is 32 channels of one tap
// (C % 32 == 0) = two MFMA groups of k = 16.
//   LDS: rows of 32 bf16 at an 80-byte pitch, two stages.  A fragment is one ds_read_b128: lane l holds row l & 31,
//   k = 8 (l >> 5) + j; the sixteen lanes of a read group hit sixteen distinct 16-byte slots (5 m mod 16 is a bijection).
//   The C/D lane map is the fp32 instruction's, so tile_origin, the zero page and both epilogues are shared as they are.
// 4 waves on a 128x128 (TM = TN = 2) or 64x64 (TM = TN = 1) tile; both walk K in the same order with the same
// instruction, so their results are bit-identical.
// The kernel lives beside the fp32 kernels whose device helpers it shares (its entry points: conv_bf16.hip).  In a unit of its
// own the compiler's whole-module passes see fewer callers of those helpers and the epilogue comes out scheduled differently
// (profiles/conv_units.md).
// ------------------------------------------------------------------------------------------------
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // eight packed bf16 in flight between the global load and the LDS store
constexpr int BF16_PITCH = 80;   // bytes per LDS row (32 bf16 + 16 B pad)
// split form: (activation plane, filter plane) of the six products of a k-group in issue order; 0 = hi, 1 = mid, 2 = lo.
// The three left out (mid*lo, lo*mid, lo*lo) are at most 2^-26 of the product.  The first five (at most 2^-8 of hi*hi) are
// summed in an accumulator of their own and added to the hi*hi accumulator once, after the K loop: the MFMA aligns its
// addends to the largest one and cuts what falls below, so small products added straight into the large sum lose their
// low bits at every instruction - measured, 1.15 to 2 times the fp32 kernel's error and a bias of its own
// (profiles/conv_split_bf16.md); apart, the result carries the hi*hi chain's error only, 0.34 to 0.70 of the fp32 kernel's.
constexpr int kSplitTerms[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};

// NP = 3 is the split form (frcnn_conv2d_fwd_bf16x3, see below the kernel): three bf16 planes per operand.
template <int TM, int TN, int DEPTH, int NP>
__global__ __launch_bounds__(256, (NP == 3 && TM * TN > 1) ? 1 : 2) void conv_igemm_bf16(const ConvParams p, const unsigned short* __restrict__ wq) {
  static_assert(DEPTH >= 1 && DEPTH <= 4, "register sets of the staging ring");
  static_assert(NP == 1 || NP == 3, "one bf16 plane per operand, or hi / mid / lo");
  constexpr int WN = 2;
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int PA = BM / 32;   // A: 8 threads x 4 floats cover a row's K-step, 32 rows per pass
  constexpr int PB = BN / 64;   // B: 4 threads x 8 bf16 cover a row's K-step, 64 rows per pass
  static_assert(2 * (BM + BN) * BF16_PITCH >= 4 * 32 * LDS_PITCH * (int)sizeof(float), "the epilogue's patches fit the stages");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* const As = reinterpret_cast<char*>(smem);   // [2][NP][BM][80 B]
  char* const Bs = As + 2 * NP * BM * BF16_PITCH;   // [2][NP][BN][80 B]
  const size_t w_plane = (size_t)p.K * p.Ktot;      // NP == 3: the filter's planes are whole KRSC arrays, hi then mid then lo

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave / WN, wc = wave % WN;
  int m0, n0;
  tile_origin<BM, BN>(p, blockIdx.x, m0, n0);

  const int kc = t & 7, row0 = t >> 3;
  int a_base[PA], a_hi0[PA], a_wi0[PA];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int m = m0 + i * 32 + row0;
    if (m < p.M) {
      const int img = m / (p.Ho * p.Wo);
      const int rem = m - img * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      a_hi0[i] = ho * p.stride - p.pad;
      a_wi0[i] = wo * p.stride - p.pad;
      a_base[i] = ((img * p.H + a_hi0[i]) * p.W + a_wi0[i]) * p.C;
    } else {
      a_hi0[i] = -(1 << 20);  // never in range
      a_wi0[i] = 0;
      a_base[i] = 0;
    }
  }
  const int kb = t & 3, rowb = t >> 2;
  const unsigned short* b_src[PB];
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int n = n0 + j * 64 + rowb;
    b_src[j] = n < p.K ? wq + (size_t)n * p.Ktot + kb * 8 : nullptr;
  }

  // DEPTH register sets: tile t waits in set t % DEPTH from its global load until step t - 1 stores it to LDS, so the tiles
  // of steps s+1 .. s+DEPTH are in flight while step s computes.  A step's MFMAs are an eighth of the fp32 kernel's for the
  // same tile: with one tile ahead a lone 64x64 workgroup pays the HBM / L2 latency once per K-step (DEPTH = 4 there); the
  // 128x128 tile keeps one set - 154 VGPRs, three workgroups per CU - because a deeper ring costs it the third workgroup.
  f32x4 ra[DEPTH][PA];
  u32x4 rb[DEPTH][PB * NP];
  typedef std::integral_constant<int, 0> Set0;
  typedef std::integral_constant<int, 1 % DEPTH> Set1;   // SetN: the set of tile N
  typedef std::integral_constant<int, 2 % DEPTH> Set2;
  typedef std::integral_constant<int, 3 % DEPTH> Set3;
  int tr = 0, ts = 0, tc = 0;   // tap state: a K-step never straddles a tap
  // load_tiles is called for consecutive steps (the tap state advances by one step per call)
  auto load_tiles = [&](int step, auto set) {
    constexpr int SL = decltype(set)::value;
    const int koff = (tr * p.W + ts) * p.C + tc + kc * 4;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const int hi = a_hi0[i] + tr, wi = a_wi0[i] + ts;
      const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      ra[SL][i] = *reinterpret_cast<const f32x4*>(ok ? p.x + a_base[i] + koff : p.zero);
    }
    tc += BK;
    if (tc == p.C) {
      tc = 0;
      if (++ts == p.S) { ts = 0; ++tr; }
    }
#pragma unroll
    for (int j = 0; j < PB; ++j)
#pragma unroll
      for (int q = 0; q < NP; ++q)
        rb[SL][j * NP + q] = *reinterpret_cast<const u32x4*>(b_src[j] ? reinterpret_cast<const void*>(b_src[j] + q * w_plane + step * BK)
                                                                      : reinterpret_cast<const void*>(p.zero));
  };
  auto store_tiles = [&](int buf, auto set) {
    constexpr int SL = decltype(set)::value;
    char* a = As + (buf * NP * BM + row0) * BF16_PITCH + kc * 8;
    char* b = Bs + (buf * NP * BN + rowb) * BF16_PITCH + kb * 16;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const bf16x4 hi = __builtin_convertvector(ra[SL][i], bf16x4);
      *reinterpret_cast<bf16x4*>(a + i * 32 * BF16_PITCH) = hi;
      if constexpr (NP == 3) {   // split_bf16x3's chain, once per tile element: both remainders are exact in fp32
        const f32x4 r1 = ra[SL][i] - __builtin_convertvector(hi, f32x4);
        const bf16x4 mid = __builtin_convertvector(r1, bf16x4);
        const f32x4 r2 = r1 - __builtin_convertvector(mid, f32x4);
        *reinterpret_cast<bf16x4*>(a + (BM + i * 32) * BF16_PITCH) = mid;
        *reinterpret_cast<bf16x4*>(a + (2 * BM + i * 32) * BF16_PITCH) = __builtin_convertvector(r2, bf16x4);
      }
    }
#pragma unroll
    for (int j = 0; j < PB; ++j)
#pragma unroll
      for (int q = 0; q < NP; ++q) *reinterpret_cast<u32x4*>(b + (q * BN + j * 64) * BF16_PITCH) = rb[SL][j * NP + q];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // split form: the five small products of every k-group go to an accumulator of their own (see kSplitTerms)
  f32x16 low[TM][TN];   // (unused, and removed by the compiler, when NP == 1)
  if constexpr (NP == 3) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) low[i][j][r] = 0.f;
  }

  // fragment read offsets: lane (l&31) = row inside the 32x32 tile, (l>>5) selects k in {8h..8h+7} of a group of 16
  const int frag = (lane & 31) * BF16_PITCH + 16 * (lane >> 5);
  const int a_frag = (wr * TM * 32) * BF16_PITCH + frag;
  const int b_frag = (wc * TN * 32) * BF16_PITCH + frag;

  const int nsteps = p.ksteps;   // >= 1
  load_tiles(0, Set0{});
  if (DEPTH > 1 && nsteps > 1) load_tiles(1, Set1{});
  if (DEPTH > 2 && nsteps > 2) load_tiles(2, Set2{});
  if (DEPTH > 3 && nsteps > 3) load_tiles(3, Set3{});
  store_tiles(0, Set0{});
  if (nsteps > DEPTH) load_tiles(DEPTH, Set0{});
  __syncthreads();
  int cur = 0;
  // split form only: the fragments of a step's two k-groups, three planes per operand
  bf16x8 ga[2][TM][NP], gb[2][TN][NP];
  auto read_frags = [&](int stage, int kk, auto which) {
    constexpr int G = decltype(which)::value;
    const char* Ab = As + stage * NP * BM * BF16_PITCH + a_frag + kk * 32;
    const char* Bb = Bs + stage * NP * BN * BF16_PITCH + b_frag + kk * 32;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
#pragma unroll
      for (int i = 0; i < TM; ++i) ga[G][i][q] = *reinterpret_cast<const bf16x8*>(Ab + (q * BM + i * 32) * BF16_PITCH);
#pragma unroll
      for (int j = 0; j < TN; ++j) gb[G][j][q] = *reinterpret_cast<const bf16x8*>(Bb + (q * BN + j * 32) * BF16_PITCH);
    }
  };
  // a k = 16 group: six products in kSplitTerms' order, the five small ones into `low`, hi*hi into `acc`; consecutive MFMAs
  // go to different outputs' accumulators, each accumulator sees its terms in this order and the groups in ascending k.
  // (A generic lambda: instantiated only where it is called, under NP == 3.  On the 64x64 tile, TM = TN = 1, the five
  // `low` MFMAs of a group depend on each other back to back; the rule never gives that tile a layer of the frame.)
  auto mma_group = [&](auto which) {
    constexpr int G = decltype(which)::value;
#pragma unroll
    for (int term = 0; term < 6; ++term)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          f32x16& to = term < 5 ? low[i][j] : acc[i][j];
          to = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gb[G][j][kSplitTerms[term][1]], ga[G][i][kSplitTerms[term][0]], to, 0, 0, 0);
        }
  };
  // one K-step; `set` = (s + 1) % DEPTH holds tile s + 1 and is refilled with tile s + 1 + DEPTH once that one is in LDS.
  // STEADY: both exist - no conditions around the loads, so the compiler counts them and waits for the oldest set only.
  auto kstep = [&](int s, auto set, auto steady) {
    constexpr bool STEADY = decltype(steady)::value;
    // operands are (weights, activations) as in mma_step: D col (lane) = pixel, D row (register) = channel
    if constexpr (NP == 1) {
      const char* Ab = As + cur * BM * BF16_PITCH + a_frag;
      const char* Bb = Bs + cur * BN * BF16_PITCH + b_frag;
      bf16x8 fa[2][TM], fb[2][TN];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[kk][i] = *reinterpret_cast<const bf16x8*>(Ab + i * 32 * BF16_PITCH + kk * 32);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[kk][j] = *reinterpret_cast<const bf16x8*>(Bb + j * 32 * BF16_PITCH + kk * 32);
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[kk][j], fa[kk][i], acc[i][j], 0, 0, 0);
    } else {
      read_frags(cur, 0, std::integral_constant<int, 0>{});
      read_frags(cur, 1, std::integral_constant<int, 1>{});
      mma_group(std::integral_constant<int, 0>{});
      mma_group(std::integral_constant<int, 1>{});
    }
    if (STEADY || s + 1 < nsteps) store_tiles(cur ^ 1, set);   // stage cur^1 was last read before the previous step's barrier
    if (STEADY || s + 1 + DEPTH < nsteps) load_tiles(s + 1 + DEPTH, set);
    __syncthreads();
    cur ^= 1;
  };
  // DEPTH consecutive steps from s, a multiple of DEPTH: step s + i refills the set of tile s + i + 1
  auto round = [&](int s, auto steady) {
    constexpr bool STEADY = decltype(steady)::value;
    kstep(s, Set1{}, steady);
    if (DEPTH > 1 && (STEADY || s + 1 < nsteps)) kstep(s + 1, Set2{}, steady);
    if (DEPTH > 2 && (STEADY || s + 2 < nsteps)) kstep(s + 2, Set3{}, steady);
    if (DEPTH > 3 && (STEADY || s + 3 < nsteps)) kstep(s + 3, Set0{}, steady);
  };
  int s = 0;
  for (; s + 2 * DEPTH < nsteps; s += DEPTH) round(s, std::true_type{});
  for (; s < nsteps; s += DEPTH) round(s, std::false_type{});

  if constexpr (NP == 3) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] += low[i][j];
  }
  if (p.epi_lds && (p.K & 3) == 0)   // (uniform branch; every wave is past the K loop's last barrier and reads no LDS any more)
    conv_epilogue_lds<TM, TN>(p, acc, m0, n0, wr, wc, lane, p.M, smem + wave * 32 * LDS_PITCH, 0, 0);
  else
    conv_epilogue<TM, TN>(p, acc, m0, n0, wr, wc, lane, p.M, 0, 0);
}

// LDS of a workgroup: two stages x NP planes x (BM + BN) rows of 80 B.  NP = 3: 60 KB on the 64x64 tile (two workgroups
// per CU, the staging ring stays four deep) and 120 KB on the 128x128 tile - one workgroup per CU, so the kernel is built
// for one wave per SIMD (512 registers) and keeps two tiles in flight.
template <int TM, int TN, int NP>
int launch_bf16(ConvArgs p, const unsigned short* wq, hipStream_t stream) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr size_t lds = (size_t)2 * NP * (BM + BN) * BF16_PITCH;
  static_assert(lds <= 160 * 1024, "LDS of a gfx950 CU");
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.K + BN - 1) / BN;
  constexpr int DEPTH = TM * TN == 1 ? 4 : (NP == 3 ? 2 : 1);   // (see the kernel's staging ring)
  return launch_kernel<conv_igemm_bf16<TM, TN, DEPTH, NP>>(NP == 3 ? "conv_igemm_bf16x3" : "conv_igemm_bf16", 0, dim3(p.tiles_m * p.tiles_n),
                                                           256, lds, stream, kernel_arg(p), wq);
}

}  // namespace

int frcnn::conv::launch_gemm_bf16(const ConvArgs& p, const unsigned short* wq, bool small_tile, int planes, hipStream_t stream) {
  if (planes == 3) return small_tile ? launch_bf16<1, 1, 3>(p, wq, stream) : launch_bf16<2, 2, 3>(p, wq, stream);
  return small_tile ? launch_bf16<1, 1, 1>(p, wq, stream) : launch_bf16<2, 2, 1>(p, wq, stream);
}
