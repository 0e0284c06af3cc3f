// Test-time Spatter corruption of a camera frame on the device (lib/roi_data_layer/minibatch.py:648-664, behind
// cfg.TEST.AUGMENT_EN): the mud branch (severities 4 and 5) of the published ImageNet-C `spatter`, which the reference
// reaches as iaa.imgcorruptlike.Spatter(severity=5).  uint8 HWC3 in, uint8 HWC3 out (what frcnn_prep_image consumes).
//
// imgaug, imagecorruptions, scikit-image and scipy are not vendored: the operator and its constants are restated from
// the published code, PARITY UNPINNED (like image_augment.hip and prep.hip's resize).  Conventions chosen here
// (tests/test_image_spatter.py restates them in float64 numpy):
//   * field: liquid[y, x] = loc + scale * normal01(seed, stream 44, y * W + x) (rng.h; reads the uniform streams 88, 89).
//   * blurs: skimage / scipy's gaussian: radius int(4 sigma + 0.5) (9 taps for sigma 1, 13 for sigma 1.5), taps
//     exp(-x^2 / 2 sigma^2) normalised, computed by the caller in double and passed as fp32 (no expf here); border
//     replicate ("nearest"), for EACH blur on the field it reads; horizontal pass then vertical pass, each
//     acc = t0*p0, acc += tk*pk in tap order, fp32.
//   * b = liquid > thr ? 1 : 0 (the published code zeroes the values below thr and then tests > thr: the same thing);
//     m = gaussian(b, sigma2); m = m < 0.8 ? 0 : m.
//   * blend per memory channel c: x = px / 255, v = clip(x (1 - m) + col[c] m, 0, 1) * 255, out = (uint8) v TRUNCATED
//     (np.uint8(...) of the published corrupt()).  px / 255 * 255 is px again in fp32 for all 256 values, so a pixel with
//     m = 0 leaves as it came.
//   * mud colour (63, 42, 20) / 255 on memory channels 0, 1, 2 in that order: the frame is cv2's BGR and the corruption
//     reads it as RGB - kept, exactly as the HUE_SAT stage of image_augment.hip keeps it.
// Severities 1-3 (the water branch: Canny edges, distance transform) are not built; the Python layer refuses them.
// A frame is a pure function of (pixels, severity, seed).  Compiled with -ffp-contract=off: one rounding per operation.
//
// One fused launch.  A 256-thread workgroup owns a 64x32-pixel output tile and regenerates the draws of the tile plus
// a halo of 4 + 6 pixels from the counter-based generator (84 x 52 = 4368 draws, 2.1 per output pixel; the 64x16 tile of
// image_augment.hip would pay 2.95, and the draws - two hashes, logf, sqrtf, cosf each - are what the kernel spends its
// time on), so no field ever goes to HBM.  Both separable blurs and both cuts run in LDS as fp32, in two buffers that
// the five passes reuse in turn (17.1 + 15.4 KiB: four workgroups = 16 waves per CU).  A halo position outside the frame
// takes the value of the clamped coordinate - the clamped draw before the first blur, the clamped column / row of the
// first blur before the second - which is replicate padding of the full field for each blur (the clamped position always
// lies inside the tile's own region).  Every LDS pass walks a dense row-major index, so a wave reads consecutive dwords.
// The frame is read once and written once, 4 bytes per item as one dword when the address allows.
#include "common.h"
#include "rng.h"

#include <cmath>

using namespace frcnn;

namespace {

constexpr uint32_t SP_NORMAL_FIELD = 44;                      // reads the uniform streams 88, 89
constexpr int SP_R1 = FRCNN_SPATTER_MAX_TAPS1 / 2, SP_R2 = FRCNN_SPATTER_MAX_TAPS2 / 2, SP_HALO = SP_R1 + SP_R2;
constexpr int SP_TILE_W = 64, SP_TILE_H = 32;
constexpr int SP_A_W = SP_TILE_W + 2 * SP_HALO, SP_A_H = SP_TILE_H + 2 * SP_HALO;     // draws: 84 x 52
constexpr int SP_C_W = SP_TILE_W + 2 * SP_R2, SP_C_H = SP_TILE_H + 2 * SP_R2;         // first blur, b: 76 x 44
constexpr int SP_TILE_BYTES = SP_TILE_W * 3, SP_GROUPS = SP_TILE_BYTES / 4;           // 48 four-byte items per tile row
constexpr float SP_MASK_CUT = 0.8f;

struct SpatterParams {
  int h, w;
  float loc, scale, thr;
  float col[3];
  float t1[FRCNN_SPATTER_MAX_TAPS1], t2[FRCNN_SPATTER_MAX_TAPS2];   // centred, zero-filled: a zero tap adds an exact 0
};

__global__ __launch_bounds__(256) void image_spatter_kernel(const uint8_t* __restrict__ in, SpatterParams s, uint32_t seed,
                                                           const uint32_t* __restrict__ seed_dev, uint8_t* __restrict__ out,
                                                           float* __restrict__ debug_liquid, float* __restrict__ debug_mask) {
  __shared__ __attribute__((aligned(16))) float buf_a[SP_A_H * SP_A_W];   // draws -> b -> m
  __shared__ __attribute__((aligned(16))) float buf_b[SP_A_H * SP_C_W];   // horizontal pass 1 -> horizontal pass 2
  if (seed_dev) seed += *seed_dev;
  const int x0 = blockIdx.x * SP_TILE_W, y0 = blockIdx.y * SP_TILE_H;
  // 1. the draws of the tile + halo, at the clamped coordinate
  for (int e = threadIdx.x; e < SP_A_H * SP_A_W; e += 256) {
    const int ry = e / SP_A_W, rx = e - ry * SP_A_W;
    const int y = min(max(y0 - SP_HALO + ry, 0), s.h - 1), x = min(max(x0 - SP_HALO + rx, 0), s.w - 1);
    buf_a[e] = s.loc + s.scale * normal01(seed, SP_NORMAL_FIELD, (uint32_t)(y * s.w + x));
  }
  __syncthreads();
  // 2. first blur, horizontal: every row of the draws, the columns the second blur reads (clamped into the frame)
  for (int it = threadIdx.x; it < SP_A_H * SP_C_W; it += 256) {
    const int ry = it / SP_C_W, cx = it - ry * SP_C_W;
    const int lx = min(max(x0 - SP_R2 + cx, 0), s.w - 1) - (x0 - SP_R2);
    const float* src = buf_a + ry * SP_A_W + lx;
    float acc = s.t1[0] * src[0];
    for (int k = 1; k < FRCNN_SPATTER_MAX_TAPS1; ++k) acc = acc + s.t1[k] * src[k];
    buf_b[it] = acc;
  }
  __syncthreads();
  // 3. first blur, vertical (rows clamped into the frame), and the first cut
  for (int it = threadIdx.x; it < SP_C_H * SP_C_W; it += 256) {
    const int cy = it / SP_C_W, cx = it - cy * SP_C_W;
    const int ly = min(max(y0 - SP_R2 + cy, 0), s.h - 1) - (y0 - SP_R2);
    const float* src = buf_b + ly * SP_C_W + cx;
    float acc = s.t1[0] * src[0];
    for (int k = 1; k < FRCNN_SPATTER_MAX_TAPS1; ++k) acc = acc + s.t1[k] * src[k * SP_C_W];
    buf_a[it] = acc > s.thr ? 1.f : 0.f;
    const int y = y0 - SP_R2 + cy, x = x0 - SP_R2 + cx;
    if (debug_liquid && cy >= SP_R2 && cy < SP_R2 + SP_TILE_H && cx >= SP_R2 && cx < SP_R2 + SP_TILE_W && y < s.h && x < s.w)
      debug_liquid[(size_t)y * s.w + x] = acc;
  }
  __syncthreads();
  // 4. second blur, horizontal
  for (int it = threadIdx.x; it < SP_C_H * SP_TILE_W; it += 256) {
    const int cy = it / SP_TILE_W, tx = it - cy * SP_TILE_W;
    const float* src = buf_a + cy * SP_C_W + tx;
    float acc = s.t2[0] * src[0];
    for (int k = 1; k < FRCNN_SPATTER_MAX_TAPS2; ++k) acc = acc + s.t2[k] * src[k];
    buf_b[it] = acc;
  }
  __syncthreads();
  // 5. second blur, vertical, and the second cut
  for (int it = threadIdx.x; it < SP_TILE_H * SP_TILE_W; it += 256) {
    const int ty = it / SP_TILE_W, tx = it - ty * SP_TILE_W;
    const float* src = buf_b + it;
    float acc = s.t2[0] * src[0];
    for (int k = 1; k < FRCNN_SPATTER_MAX_TAPS2; ++k) acc = acc + s.t2[k] * src[k * SP_TILE_W];
    buf_a[it] = acc < SP_MASK_CUT ? 0.f : acc;
    if (debug_mask && y0 + ty < s.h && x0 + tx < s.w) debug_mask[(size_t)(y0 + ty) * s.w + x0 + tx] = acc;
  }
  __syncthreads();
  // 6. blend: the frame is read once and written once
  const size_t row_stride = (size_t)s.w * 3;
  const int valid_bytes = min(SP_TILE_W, s.w - x0) * 3;
  for (int it = threadIdx.x; it < SP_TILE_H * SP_GROUPS; it += 256) {
    const int ty = it / SP_GROUPS, b = (it - ty * SP_GROUPS) * 4;
    if (y0 + ty >= s.h || b >= valid_bytes) continue;
    const size_t off = (size_t)(y0 + ty) * row_stride + (size_t)x0 * 3 + b;
    const uint8_t* src = in + off;
    uint8_t* dst = out + off;
    const bool word = b + 4 <= valid_bytes && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) == 0;
    uint32_t pw = 0;
    if (word) {
      pw = *reinterpret_cast<const uint32_t*>(src);
    } else {
      for (int j = 0; j < 4 && b + j < valid_bytes; ++j) pw |= (uint32_t)src[j] << (8 * j);
    }
    uint32_t ow = 0;
    for (int j = 0; j < 4; ++j) {
      const int px = (b + j) / 3, c = (b + j) - px * 3;
      const float m = buf_a[ty * SP_TILE_W + min(px, SP_TILE_W - 1)];
      const float x = (float)((pw >> (8 * j)) & 255u) / 255.f;
      const float v = fminf(fmaxf(x * (1.f - m) + s.col[c] * m, 0.f), 1.f) * 255.f;
      ow |= (uint32_t)(uint8_t)v << (8 * j);
    }
    if (word) {
      *reinterpret_cast<uint32_t*>(dst) = ow;
    } else {
      for (int j = 0; j < 4 && b + j < valid_bytes; ++j) dst[j] = (uint8_t)(ow >> (8 * j));
    }
  }
}

// centre `n` (odd) taps in a zero-filled array of `cap`
void centre_taps(const float* taps, int n, float* dst, int cap) {
  for (int k = 0; k < cap; ++k) dst[k] = 0.f;
  for (int k = 0; k < n; ++k) dst[(cap - n) / 2 + k] = taps[k];
}

bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

extern "C" int frcnn_image_spatter(const uint8_t* img_hwc3, int h, int w, const float* params_host, const float* taps1_host,
                                   int num_taps1, const float* taps2_host, int num_taps2, uint32_t seed, const uint32_t* seed_dev,
                                   uint8_t* out, float* debug_liquid, float* debug_mask, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(img_hwc3 && out && params_host && taps1_host && taps2_host,
                "image_spatter: null argument (img / out / parameters / taps)");
  FRCNN_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1ll << 29) && (h + SP_TILE_H - 1) / SP_TILE_H <= 65535,
                "image_spatter: bad frame size %d x %d", h, w);
  FRCNN_REQUIRE(num_taps1 >= 1 && num_taps1 <= FRCNN_SPATTER_MAX_TAPS1 && num_taps1 % 2 == 1,
                "image_spatter: first blur: %d taps, the kernel holds an odd count up to %d", num_taps1, FRCNN_SPATTER_MAX_TAPS1);
  FRCNN_REQUIRE(num_taps2 >= 1 && num_taps2 <= FRCNN_SPATTER_MAX_TAPS2 && num_taps2 % 2 == 1,
                "image_spatter: second blur: %d taps, the kernel holds an odd count up to %d", num_taps2, FRCNN_SPATTER_MAX_TAPS2);
  FRCNN_REQUIRE(finite_all(params_host, FRCNN_SPATTER_NUM_PARAMS) && finite_all(taps1_host, num_taps1) &&
                    finite_all(taps2_host, num_taps2),
                "image_spatter: non-finite parameter or tap");
  const float sigma1 = params_host[2], sigma2 = params_host[4];
  FRCNN_REQUIRE(params_host[1] >= 0.f && sigma1 > 0.f && sigma2 > 0.f, "image_spatter: negative scale or sigma");
  FRCNN_REQUIRE(num_taps1 == 2 * (int)(4.0 * sigma1 + 0.5) + 1 && num_taps2 == 2 * (int)(4.0 * sigma2 + 0.5) + 1,
                "image_spatter: tap counts (%d, %d) do not follow the radius rule int(4 sigma + 0.5) for sigma (%g, %g)", num_taps1,
                num_taps2, (double)sigma1, (double)sigma2);
  const size_t bytes = (size_t)h * w * 3;
  FRCNN_REQUIRE(out + bytes <= img_hwc3 || img_hwc3 + bytes <= out, "image_spatter: out must not overlap img");
  SpatterParams s;
  s.h = h; s.w = w;
  s.loc = params_host[0]; s.scale = params_host[1]; s.thr = params_host[3];
  s.col[0] = (float)(63.0 / 255.0); s.col[1] = (float)(42.0 / 255.0); s.col[2] = (float)(20.0 / 255.0);
  centre_taps(taps1_host, num_taps1, s.t1, FRCNN_SPATTER_MAX_TAPS1);
  centre_taps(taps2_host, num_taps2, s.t2, FRCNN_SPATTER_MAX_TAPS2);
  hipLaunchKernelGGL(image_spatter_kernel, dim3((w + SP_TILE_W - 1) / SP_TILE_W, (h + SP_TILE_H - 1) / SP_TILE_H), dim3(256), 0,
                     stream, img_hwc3, s, seed, seed_dev, out, debug_liquid, debug_mask);
  return check_launch("image_spatter kernel");
}
