// Image augmentation on the device (lib/roi_data_layer/minibatch.py:540-647): the pixel side of the block the reference
// runs with imgaug between cv2.imread and prep_im_for_blob.  uint8 HWC3 in, uint8 HWC3 out (what frcnn_prep_image
// consumes); the decisions and the gt boxes stay on the host (roi_data_layer/image_augment.py).  A call is an optional
// horizontal flip (:549) followed by up to FRCNN_IMG_MAX_STAGES stages in the caller's order; EVERY stage takes uint8
// and leaves uint8 (imgaug's augmenters round and clip before the next one), one launch per stage, ping-pong between
// `scratch` and `out` so that the last one writes `out`.  The flip is folded into the read of the first stage (a
// mirrored copy when there is no stage).
//
// imgaug, cv2 and scikit-image are not vendored: the operators are restated from the published algorithms, PARITY
// UNPINNED (like prep.hip's resize).  Conventions chosen here (tests/test_image_augment.py restates them in numpy):
//   * rounding: every stage ends with rintf (round half to even) and a clip to [0, 255].
//   * GAUSS (:567): separable, 5 / 7 / 9 normalised taps computed by the caller in double and passed as fp32 (no expf
//     here); horizontal pass then vertical pass, each acc = t0*p0, acc += tk*pk in tap order, fp32, no rounding between
//     the passes; border reflect-101.
//   * reflect-101 everywhere means np.pad(mode='reflect') for ANY frame dimension n >= 1: the index is folded with
//     period 2n - 2, so a dimension no larger than the halo (n <= 4 under 9 taps) reflects as often as it takes, and
//     n == 1 repeats the only sample.
//   * AVERAGE (:568): k = 2 or 3, integer window sum, round-half-even of sum / k^2; the window of k = 2 covers
//     offsets {-1, 0} (cv2's anchor k / 2); border reflect-101.
//   * MEDIAN (:569): 3x3 per channel, border replicate; exchange network on integers (sort the three columns, then
//     med3(max of mins, med of meds, min of maxes)).
//   * SHARPEN (:570): centre weight wc = (1 - a) + a (8 + l) and neighbour weight wn = -a computed by the caller in
//     double; value = wc * centre + wn * (integer sum of the 8 neighbours); border reflect-101.
//   * NOISE (:572-575): px + s * normal01(seed, stream 40 + channel, pixel index row-major).
//   * HUE_SAT (:576): the frame is cv2's BGR and imgaug reads it as RGB - kept: memory channel 0 plays "R".  RGB -> HSV by
//     cv2's formulas in fp32 (H in [0, 180) = degrees / 2, S = 255 (V - min) / V, V = max), NOT quantised to 8 bits in
//     between; H' = (H + dh) wrapped into [0, 180), S' = clip(S + ds, 0, 255); the caller passes dh = trunc(v_h / 255 * 90)
//     (imgaug's scaling of the [-255, 255] convention to the hue circle, integer) and ds = v_s; HSV -> RGB by sectors of 30.
//   * AFFINE (:579-586): inverse map, six fp32 numbers computed by the caller in double, source = (m0 x + m1 y) + m2;
//     nearest = rintf of the source coordinate; bilinear = floorf + fraction, horizontal blend first, every tap outside
//     the frame reads the border value; output size = input size.
//   * DROPOUT (:587): uniform01(seed, stream 86, index) < p -> 0; index = pixel (one mask for the three channels) or
//     sample (pixel * 3 + channel).
// Draws are counter-based on the OUTPUT index of their stage (rng.h), so a frame is a pure function of (record, seed).
// Compiled with -ffp-contract=off: one rounding per operation, like the float32 numpy restatement.
//
// Stencil stages: a 256-thread workgroup stages a 64x16-pixel tile plus halo (<= 4 pixels) once in LDS as bytes (row
// pitch 320 B: the two 16-lane quarters of a half-wave that straddle a row then fall on disjoint banks), every thread
// produces 4 consecutive bytes of a row per item and stores them as one dword when the address allows.  The Gaussian
// keeps its horizontal pass in LDS as fp32 (read back as 16-byte rows).  Pointwise stages: 4 pixels = 3 dwords per thread.
// HBM-bound: one read and one write of H*W*3 bytes per stage.
#include "common.h"
#include "rng.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace frcnn;

namespace {

constexpr uint32_t IA_NORMAL_NOISE = 40;      // +channel: reads the uniform streams 80..85
constexpr uint32_t IA_UNIFORM_DROPOUT = 86;

constexpr int TILE_W = 64, TILE_H = 16, MAX_R = 4;
constexpr int TILE_BYTES = TILE_W * 3;                       // 192 output bytes per tile row
constexpr int LDS_PITCH = 320;                               // >= (TILE_W + 2 * MAX_R) * 3 = 216
constexpr int LDS_ROWS = TILE_H + 2 * MAX_R;

struct StageParams {
  int code, h, w, flip;
  float p[FRCNN_IMG_NUM_PARAMS];
};

// BORDER_REFLECT_101 (np.pad mode='reflect') for any n >= 1 and any i: the pattern 0 1 .. n-1 n-2 .. 1 has period 2n - 2
// and is even about 0, so a halo wider than the frame folds as often as it takes.  n == 1: the only sample.
__device__ __forceinline__ int reflect101(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i = (i < 0 ? -i : i) % period;
  return i < n ? i : period - i;
}
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f); }
__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// source byte of sample (y, x, c) of the (flipped) input frame
__device__ __forceinline__ int src_px(const uint8_t* __restrict__ in, const StageParams& s, int y, int x, int c) {
  const int xs = s.flip ? s.w - 1 - x : x;
  return in[((size_t)y * s.w + xs) * 3 + c];
}

// ------------------------------------------------------------------------------------------------------------------
// stencils
// ------------------------------------------------------------------------------------------------------------------
template <int CODE>
__global__ __launch_bounds__(256) void image_stencil_kernel(const uint8_t* __restrict__ in, StageParams s,
                                                           uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[LDS_ROWS * LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float hpass[CODE == FRCNN_IMG_GAUSS ? LDS_ROWS * TILE_BYTES : 4];
  const int r = CODE == FRCNN_IMG_GAUSS ? (int)s.p[0] / 2 : 1;       // halo
  const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
  const int rows = TILE_H + 2 * r, row_bytes = (TILE_W + 2 * r) * 3;
  // stage the tile + halo once; border pixels are resolved here, so the passes below never test coordinates
  for (int e = threadIdx.x; e < rows * row_bytes; e += 256) {
    const int ry = e / row_bytes, rb = e - ry * row_bytes, rx = rb / 3, c = rb - rx * 3;
    int y = y0 - r + ry, x = x0 - r + rx;
    if (CODE == FRCNN_IMG_MEDIAN) {
      y = min(max(y, 0), s.h - 1);
      x = min(max(x, 0), s.w - 1);
    } else {
      y = reflect101(y, s.h);
      x = reflect101(x, s.w);
    }
    tile[ry * LDS_PITCH + rb] = (uint8_t)src_px(in, s, y, x, c);
  }
  __syncthreads();
  constexpr int GROUPS = TILE_BYTES / 4;                             // 48 four-byte items per tile row
  if (CODE == FRCNN_IMG_GAUSS) {
    const int taps = 2 * r + 1;
    for (int it = threadIdx.x; it < rows * GROUPS; it += 256) {
      const int ry = it / GROUPS, b = (it - ry * GROUPS) * 4;
      const uint8_t* src = tile + ry * LDS_PITCH + b;
      float acc[4];
      for (int j = 0; j < 4; ++j) acc[j] = s.p[1] * (float)src[j];
      for (int k = 1; k < taps; ++k)
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + s.p[1 + k] * (float)src[3 * k + j];
      *reinterpret_cast<float4*>(hpass + ry * TILE_BYTES + b) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();
  }
  const size_t row_stride = (size_t)s.w * 3;
  const int valid_bytes = min(TILE_W, s.w - x0) * 3;
  for (int it = threadIdx.x; it < TILE_H * GROUPS; it += 256) {
    const int ty = it / GROUPS, b = (it - ty * GROUPS) * 4;
    if (y0 + ty >= s.h || b >= valid_bytes) continue;
    uint8_t o[4];
    if (CODE == FRCNN_IMG_GAUSS) {
      const int taps = 2 * r + 1;
      float4 v = *reinterpret_cast<const float4*>(hpass + ty * TILE_BYTES + b);
      float acc[4] = {s.p[1] * v.x, s.p[1] * v.y, s.p[1] * v.z, s.p[1] * v.w};
      for (int k = 1; k < taps; ++k) {
        v = *reinterpret_cast<const float4*>(hpass + (ty + k) * TILE_BYTES + b);
        acc[0] = acc[0] + s.p[1 + k] * v.x; acc[1] = acc[1] + s.p[1 + k] * v.y;
        acc[2] = acc[2] + s.p[1 + k] * v.z; acc[3] = acc[3] + s.p[1 + k] * v.w;
      }
      for (int j = 0; j < 4; ++j) o[j] = to_u8(acc[j]);
    } else {
      for (int j = 0; j < 4; ++j) {
        const uint8_t* c = tile + (ty + 1) * LDS_PITCH + 3 + b + j;  // centre sample (halo 1)
        const int p00 = c[-LDS_PITCH - 3], p01 = c[-LDS_PITCH], p02 = c[-LDS_PITCH + 3];
        const int p10 = c[-3], p11 = c[0], p12 = c[3];
        const int p20 = c[LDS_PITCH - 3], p21 = c[LDS_PITCH], p22 = c[LDS_PITCH + 3];
        if (CODE == FRCNN_IMG_AVERAGE) {
          const int k = (int)s.p[0], n = k * k;
          const int sum = k == 3 ? ((p00 + p01 + p02) + (p10 + p11 + p12)) + (p20 + p21 + p22) : (p00 + p01) + (p10 + p11);
          const int q = sum / n, rem = sum - q * n;
          o[j] = (uint8_t)(q + ((2 * rem > n) || (2 * rem == n && (q & 1))));
        } else if (CODE == FRCNN_IMG_MEDIAN) {
          const int lo0 = min(min(p00, p10), p20), lo1 = min(min(p01, p11), p21), lo2 = min(min(p02, p12), p22);
          const int hi0 = max(max(p00, p10), p20), hi1 = max(max(p01, p11), p21), hi2 = max(max(p02, p12), p22);
          const int md0 = med3i(p00, p10, p20), md1 = med3i(p01, p11, p21), md2 = med3i(p02, p12, p22);
          o[j] = (uint8_t)med3i(max(max(lo0, lo1), lo2), med3i(md0, md1, md2), min(min(hi0, hi1), hi2));
        } else {                                                     // FRCNN_IMG_SHARPEN
          const int neigh = ((p00 + p01 + p02) + (p10 + p12)) + (p20 + p21 + p22);
          o[j] = to_u8(s.p[0] * (float)p11 + s.p[1] * (float)neigh);
        }
      }
    }
    uint8_t* dst = out + (size_t)(y0 + ty) * row_stride + (size_t)x0 * 3 + b;
    if (b + 4 <= valid_bytes && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
    } else {
      for (int j = 0; j < 4 && b + j < valid_bytes; ++j) dst[j] = o[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// pointwise stages and the warp
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float affine_tap(const uint8_t* __restrict__ in, const StageParams& s, int y, int x, int c,
                                            float cval) {
  return (x >= 0 && x < s.w && y >= 0 && y < s.h) ? (float)src_px(in, s, y, x, c) : cval;
}

// One output pixel i (row-major).  px[3] holds the (flipped) input pixel for the stages that read it in place.
// pre (debug, may be null): the value before rounding, H*W*3 floats (NOISE and HUE_SAT only).
template <int CODE>
__device__ __forceinline__ void point_pixel(const uint8_t* __restrict__ in, const StageParams& s, uint32_t seed, int i,
                                            const int px[3], uint8_t o[3], float* __restrict__ pre) {
  if (CODE == FRCNN_IMG_COPY) {
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)px[c];
  } else if (CODE == FRCNN_IMG_NOISE) {
    for (int c = 0; c < 3; ++c) {
      const float v = (float)px[c] + s.p[0] * normal01(seed, IA_NORMAL_NOISE + c, (uint32_t)i);
      if (pre) pre[(size_t)i * 3 + c] = v;
      o[c] = to_u8(v);
    }
  } else if (CODE == FRCNN_IMG_DROPOUT) {
    const bool per_channel = s.p[1] != 0.f;
    const bool shared_drop = uniform01(seed, IA_UNIFORM_DROPOUT, (uint32_t)i) < s.p[0];
    for (int c = 0; c < 3; ++c) {
      const bool drop = per_channel ? uniform01(seed, IA_UNIFORM_DROPOUT, (uint32_t)i * 3u + c) < s.p[0] : shared_drop;
      o[c] = drop ? 0 : (uint8_t)px[c];
    }
  } else if (CODE == FRCNN_IMG_HUE_SAT) {
    const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
    const float v = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b), d = v - mn;
    float sat = v > 0.f ? 255.f * d / v : 0.f, hue = 0.f;
    if (d > 0.f) {
      if (v == r) hue = 60.f * (g - b) / d;
      else if (v == g) hue = 120.f + 60.f * (b - r) / d;
      else hue = 240.f + 60.f * (r - g) / d;
      if (hue < 0.f) hue = hue + 360.f;
      hue = hue * 0.5f;
    }
    hue = hue + s.p[0];
    if (hue < 0.f) hue = hue + 180.f;
    if (hue >= 180.f) hue = hue - 180.f;
    sat = fminf(fmaxf(sat + s.p[1], 0.f), 255.f) / 255.f;
    const float h6 = hue / 30.f, sector = floorf(h6), f = h6 - sector;
    const float p = v * (1.f - sat), q = v * (1.f - sat * f), t = v * (1.f - sat * (1.f - f));
    float rgb[3];
    switch ((int)sector) {
      case 0: rgb[0] = v; rgb[1] = t; rgb[2] = p; break;
      case 1: rgb[0] = q; rgb[1] = v; rgb[2] = p; break;
      case 2: rgb[0] = p; rgb[1] = v; rgb[2] = t; break;
      case 3: rgb[0] = p; rgb[1] = q; rgb[2] = v; break;
      case 4: rgb[0] = t; rgb[1] = p; rgb[2] = v; break;
      default: rgb[0] = v; rgb[1] = p; rgb[2] = q; break;
    }
    for (int c = 0; c < 3; ++c) {
      if (pre) pre[(size_t)i * 3 + c] = rgb[c];
      o[c] = to_u8(rgb[c]);
    }
  } else {                                                           // FRCNN_IMG_AFFINE
    const float x = (float)(i % s.w), y = (float)(i / s.w);
    const float xs = (s.p[0] * x + s.p[1] * y) + s.p[2], ys = (s.p[3] * x + s.p[4] * y) + s.p[5];
    const float cval = s.p[7];
    if (s.p[6] == 0.f) {
      const float xr = rintf(xs), yr = rintf(ys);
      const bool inside = xr >= 0.f && xr < (float)s.w && yr >= 0.f && yr < (float)s.h;   // also false for NaN
      for (int c = 0; c < 3; ++c) o[c] = inside ? (uint8_t)src_px(in, s, (int)yr, (int)xr, c) : (uint8_t)cval;
    } else {
      // far outside the frame every tap is the border value; clamp so that the int conversion is defined
      const float xf = floorf(fminf(fmaxf(xs, -2.f), (float)s.w + 1.f)), yf = floorf(fminf(fmaxf(ys, -2.f), (float)s.h + 1.f));
      const float fx = fminf(fmaxf(xs, -2.f), (float)s.w + 1.f) - xf, fy = fminf(fmaxf(ys, -2.f), (float)s.h + 1.f) - yf;
      const int xi = (int)xf, yi = (int)yf;
      for (int c = 0; c < 3; ++c) {
        const float top = affine_tap(in, s, yi, xi, c, cval) * (1.f - fx) + affine_tap(in, s, yi, xi + 1, c, cval) * fx;
        const float bot = affine_tap(in, s, yi + 1, xi, c, cval) * (1.f - fx) + affine_tap(in, s, yi + 1, xi + 1, c, cval) * fx;
        o[c] = to_u8(top * (1.f - fy) + bot * fy);
      }
    }
  }
}

template <int CODE>
__global__ __launch_bounds__(256) void image_point_kernel(const uint8_t* __restrict__ in, StageParams s, uint32_t seed,
                                                         const uint32_t* __restrict__ seed_dev, uint8_t* __restrict__ out,
                                                         float* __restrict__ pre) {
  if (seed_dev) seed += *seed_dev;
  const int total = s.h * s.w, quads = (total + 3) / 4;
  const bool words = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
    const int i0 = q * 4;
    const bool full = words && i0 + 4 <= total;
    uint8_t ib[12] = {}, ob[12];
    if (CODE != FRCNN_IMG_AFFINE) {                                  // the stages that read their own pixel
      if (full && !s.flip) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(in + (size_t)i0 * 3);
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        memcpy(ib, &w0, 4); memcpy(ib + 4, &w1, 4); memcpy(ib + 8, &w2, 4);
      } else {
        for (int j = 0; j < 4 && i0 + j < total; ++j) {
          const int i = i0 + j, y = i / s.w, x = i - y * s.w;
          for (int c = 0; c < 3; ++c) ib[j * 3 + c] = (uint8_t)src_px(in, s, y, x, c);
        }
      }
    }
    for (int j = 0; j < 4 && i0 + j < total; ++j) {
      const int px[3] = {ib[j * 3], ib[j * 3 + 1], ib[j * 3 + 2]};
      point_pixel<CODE>(in, s, seed, i0 + j, px, ob + j * 3, pre);
    }
    if (full) {
      uint32_t w0, w1, w2;
      memcpy(&w0, ob, 4); memcpy(&w1, ob + 4, 4); memcpy(&w2, ob + 8, 4);
      uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)i0 * 3);
      dst[0] = w0; dst[1] = w1; dst[2] = w2;
    } else {
      for (int j = 0; j < 4 && i0 + j < total; ++j)
        for (int c = 0; c < 3; ++c) out[(size_t)(i0 + j) * 3 + c] = ob[j * 3 + c];
    }
  }
}

template <int CODE>
void launch_stencil(const uint8_t* in, const StageParams& s, uint8_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(image_stencil_kernel<CODE>, dim3((s.w + TILE_W - 1) / TILE_W, (s.h + TILE_H - 1) / TILE_H), dim3(256), 0,
                     stream, in, s, out);
}
template <int CODE>
void launch_point(const uint8_t* in, const StageParams& s, uint32_t seed, const uint32_t* seed_dev, uint8_t* out, float* pre,
                  hipStream_t stream) {
  const long long quads = ((long long)s.h * s.w + 3) / 4;
  hipLaunchKernelGGL(image_point_kernel<CODE>, dim3((unsigned)std::min<long long>((quads + 255) / 256, 8192)), dim3(256), 0,
                     stream, in, s, seed, seed_dev, out, pre);
}

bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

extern "C" size_t frcnn_image_augment_ws_bytes(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return align_up((size_t)h * (size_t)w * 3, 256);
}

extern "C" int frcnn_image_augment(const uint8_t* img_hwc3, int h, int w, int flip, int num_stages, const int* stage_codes_host,
                                   const float* stage_params_host, uint32_t seed, const uint32_t* seed_dev, void* scratch,
                                   size_t scratch_bytes, uint8_t* out, float* debug_pre, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(img_hwc3 && out, "image_augment: null argument (img / out)");
  FRCNN_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1ll << 29), "image_augment: bad frame size %d x %d", h, w);
  FRCNN_REQUIRE(flip == 0 || flip == 1, "image_augment: flip is 0 or 1");
  FRCNN_REQUIRE(num_stages >= 0 && num_stages <= FRCNN_IMG_MAX_STAGES, "image_augment: num_stages %d outside [0, %d]", num_stages,
                FRCNN_IMG_MAX_STAGES);
  FRCNN_REQUIRE(num_stages == 0 || (stage_codes_host && stage_params_host), "image_augment: null argument (stage codes / parameters)");
  const size_t bytes = (size_t)h * w * 3;
  const uint8_t* sc = static_cast<const uint8_t*>(scratch);
  FRCNN_REQUIRE(out + bytes <= img_hwc3 || img_hwc3 + bytes <= out, "image_augment: out must not overlap img");
  if (num_stages > 1) {
    FRCNN_REQUIRE(scratch, "image_augment: null argument (scratch is needed for more than one stage)");
    FRCNN_REQUIRE(scratch_bytes >= frcnn_image_augment_ws_bytes(h, w), "image_augment: scratch too small (%zu < %zu bytes)",
                  scratch_bytes, frcnn_image_augment_ws_bytes(h, w));
    FRCNN_REQUIRE((sc + bytes <= img_hwc3 || img_hwc3 + bytes <= sc) && (sc + bytes <= out || out + bytes <= sc),
                  "image_augment: scratch must not overlap img or out");
  }
  StageParams st[FRCNN_IMG_MAX_STAGES + 1];
  for (int k = 0; k < num_stages; ++k) {
    StageParams& s = st[k];
    s.code = stage_codes_host[k];
    s.h = h; s.w = w; s.flip = (k == 0) ? flip : 0;
    const float* p = stage_params_host + (size_t)k * FRCNN_IMG_NUM_PARAMS;
    for (int j = 0; j < FRCNN_IMG_NUM_PARAMS; ++j) s.p[j] = p[j];
    FRCNN_REQUIRE(finite_all(p, FRCNN_IMG_NUM_PARAMS), "image_augment: stage %d has a non-finite parameter", k);
    // a stencil stage launches one row of workgroups per TILE_H frame rows (grid y <= 65535, the rule of image_spatter);
    // the pointwise stages run on a capped 1-D grid and take any admitted frame
    if (s.code == FRCNN_IMG_GAUSS || s.code == FRCNN_IMG_AVERAGE || s.code == FRCNN_IMG_MEDIAN || s.code == FRCNN_IMG_SHARPEN)
      FRCNN_REQUIRE((h + TILE_H - 1) / TILE_H <= 65535,
                    "image_augment: stage %d: bad frame size %d x %d for a stencil stage (at most %d rows)", k, h, w,
                    65535 * TILE_H);
    switch (s.code) {
      case FRCNN_IMG_GAUSS:
        FRCNN_REQUIRE(p[0] == 5.f || p[0] == 7.f || p[0] == 9.f, "image_augment: stage %d: gaussian taps must be 5, 7 or 9", k);
        break;
      case FRCNN_IMG_AVERAGE:
        FRCNN_REQUIRE(p[0] == 2.f || p[0] == 3.f, "image_augment: stage %d: average k must be 2 or 3 (1 is the identity)", k);
        break;
      case FRCNN_IMG_MEDIAN:
      case FRCNN_IMG_SHARPEN:
        break;
      case FRCNN_IMG_NOISE:
        FRCNN_REQUIRE(p[0] >= 0.f, "image_augment: stage %d: negative noise scale", k);
        break;
      case FRCNN_IMG_HUE_SAT:
        FRCNN_REQUIRE(std::fabs(p[0]) <= 90.f && std::fabs(p[1]) <= 255.f, "image_augment: stage %d: hue / saturation offset out of range", k);
        break;
      case FRCNN_IMG_AFFINE:
        FRCNN_REQUIRE((p[6] == 0.f || p[6] == 1.f) && p[7] >= 0.f && p[7] <= 255.f && p[7] == std::floor(p[7]),
                      "image_augment: stage %d: affine order is 0 or 1, border value an integer in [0, 255]", k);
        break;
      case FRCNN_IMG_DROPOUT:
        FRCNN_REQUIRE(p[0] >= 0.f && p[0] <= 1.f && (p[1] == 0.f || p[1] == 1.f), "image_augment: stage %d: dropout p outside [0, 1]", k);
        break;
      default:
        return fail(FRCNN_ERR_ARG, "image_augment: stage %d: unknown stage code %d", k, s.code);
    }
  }
  int n = num_stages;
  if (n == 0) {                                                      // flip alone (or a plain copy)
    st[0].code = FRCNN_IMG_COPY;
    st[0].h = h; st[0].w = w; st[0].flip = flip;
    for (int j = 0; j < FRCNN_IMG_NUM_PARAMS; ++j) st[0].p[j] = 0.f;
    n = 1;
  }
  if (debug_pre)
    FRCNN_REQUIRE(n == 1 && (st[0].code == FRCNN_IMG_NOISE || st[0].code == FRCNN_IMG_HUE_SAT),
                  "image_augment: debug_pre needs exactly one NOISE or HUE_SAT stage");
  uint8_t* buf = static_cast<uint8_t*>(scratch);
  const uint8_t* src = img_hwc3;
  for (int k = 0; k < n; ++k) {
    uint8_t* dst = ((n - 1 - k) % 2 == 0) ? out : buf;               // the last stage writes `out`
    const StageParams& s = st[k];
    switch (s.code) {
      case FRCNN_IMG_GAUSS: launch_stencil<FRCNN_IMG_GAUSS>(src, s, dst, stream); break;
      case FRCNN_IMG_AVERAGE: launch_stencil<FRCNN_IMG_AVERAGE>(src, s, dst, stream); break;
      case FRCNN_IMG_MEDIAN: launch_stencil<FRCNN_IMG_MEDIAN>(src, s, dst, stream); break;
      case FRCNN_IMG_SHARPEN: launch_stencil<FRCNN_IMG_SHARPEN>(src, s, dst, stream); break;
      case FRCNN_IMG_NOISE: launch_point<FRCNN_IMG_NOISE>(src, s, seed, seed_dev, dst, debug_pre, stream); break;
      case FRCNN_IMG_HUE_SAT: launch_point<FRCNN_IMG_HUE_SAT>(src, s, seed, seed_dev, dst, debug_pre, stream); break;
      case FRCNN_IMG_AFFINE: launch_point<FRCNN_IMG_AFFINE>(src, s, seed, seed_dev, dst, nullptr, stream); break;
      case FRCNN_IMG_DROPOUT: launch_point<FRCNN_IMG_DROPOUT>(src, s, seed, seed_dev, dst, nullptr, stream); break;
      default: launch_point<FRCNN_IMG_COPY>(src, s, seed, seed_dev, dst, nullptr, stream); break;
    }
    const int rc = check_launch("image_augment stage kernel");
    if (rc != FRCNN_OK) return rc;
    src = dst;
  }
  return FRCNN_OK;
}
