// LiDAR point-cloud augmentation and rain simulation on the device (lib/roi_data_layer/minibatch.py:274-428): the
// per-point transforms the reference applies in numpy between reading a scan and voxelising it, as ONE pass, one
// thread per point, in the reference's order:
//
//  -1. camera field of view of KITTI / CADC scans (:251-268,678-693; frcnn_lidar_augment_fov only): in double,
//      h = M [x y z 1]^T, u = h0 / h2, v = h1 / h2, keep iff 0 <= u < img_w and 0 <= v < img_h.  The quotient is formed
//      (not multiplied through by h2) and there is no depth test, like get_fov_flag: a point BEHIND the camera whose
//      quotient lands inside the frame is kept; h2 == 0 and NaN / Inf coordinates fail the comparisons and are dropped.
//   0. filter_points on the raw point (:232-235,274): a point outside cfg.LIDAR.*_RANGE is dropped before any transform
//   1. Gaussian distortion (:309-319)            x += sx*n0, y += sy*n1, z += sz*n2
//   2. dropout (:321-325)                        keep iff u < p_keep
//   3. rotation about z (:330-349, :695-714)     x' = c*x - s*y, y' = s*x + c*y   (c, s rounded once on the host)
//   4. x/y swap (:351-373)                       x' = y - Y0, y' = x - (X1 - X0)/2   (the reference's offsets, literally)
//   5. flip y (:375-384), flip x (:386-395)      y' = -y;  x' = -x + X1
//   6. test-time rain (:397-421)                 range r = |p|, sigma = 0.02 r (1 - e^-R)^2, shift = sigma*n,
//                                                p.xyz += shift/3, r += shift, delta = exp(-0.02 R^0.6 r),
//                                                intensity *= delta, keep iff rho/(r^2 + eps)*delta >= rho/(pi r_max^2)
//   7. test-time dropout (:422-425)              keep iff u < 0.8
//
// Every draw is a pure function of (seed, stream, row index of the point IN THE FILE) (rng.h), so the launch does not
// depend on the grid shape, nor on how many points the field-of-view step removed, and the CPU oracle replays it.
// A dropped point KEEPS ITS ROW: x, y, z become NaN.  The voxeliser's range test (voxelize.hip, vox_cell_kernel)
// rejects NaN, and voxel numbering / the first-max_points rule only look at surviving points in ascending row order,
// so this equals the reference's order-preserving compaction (the reference's points[fov_flag] too) without a scan.
// The surviving points that also pass the reference's final filter_points (:426) are counted (one atomic per
// workgroup) so the host can skip a frame without points (:428-432).
// Compiled with -ffp-contract=off: each product and sum above rounds once, like the numpy expression it restates.
// HBM-bound: 2 * N * F * 4 bytes moved once.
#include "common.h"
#include "rng.h"

#include <algorithm>
#include <cmath>

using namespace frcnn;

namespace {

// stream numbers of the draws (normal01 stream k reads the uniform streams 2k, 2k + 1: 64..71; the two keep masks
// read the uniform streams 72 and 73)
constexpr uint32_t LA_NORMAL_GAUSS = 32;     // +0 x, +1 y, +2 z
constexpr uint32_t LA_NORMAL_RAIN = 35;
constexpr uint32_t LA_UNIFORM_DROPOUT = 72;
constexpr uint32_t LA_UNIFORM_TEST_DROPOUT = 73;

constexpr unsigned LA_MAX_BLOCKS = 2048;

struct AugParams {
  float lo[3], hi[3];          // cfg.LIDAR.{X,Y,Z}_RANGE
  unsigned flags;              // FRCNN_AUG_*
  float sigma[3], p_keep, cosa, sina;
  float swap_x_off, swap_y_off, flip_x_off;
  float rain_sigma_k, rain_att_k, rain_rho, rain_p_min, test_p_keep;
  int n, f;
};

// camera of the field-of-view step: row-major 3x4 M (LiDAR point -> homogeneous pixel) and the frame size, all double
struct FovParams {
  double m[12];
  double img_w, img_h;
};

// get_fov_flag (:678-693) on one point.  Each product and sum rounds once (no fma: -ffp-contract=off), the divisions stay.
__device__ __forceinline__ bool in_fov(const FovParams& c, float xf, float yf, float zf) {
  const double x = xf, y = yf, z = zf;
  const double h0 = ((c.m[0] * x + c.m[1] * y) + c.m[2] * z) + c.m[3];
  const double h1 = ((c.m[4] * x + c.m[5] * y) + c.m[6] * z) + c.m[7];
  const double h2 = ((c.m[8] * x + c.m[9] * y) + c.m[10] * z) + c.m[11];
  const double u = h0 / h2, v = h1 / h2;
  return u >= 0.0 && u < c.img_w && v >= 0.0 && v < c.img_h;             // NaN / +-Inf quotients fail
}

__device__ __forceinline__ bool in_range(const AugParams& p, float x, float y, float z) {
  return x >= p.lo[0] && y >= p.lo[1] && z >= p.lo[2] && x < p.hi[0] && y < p.hi[1] && z < p.hi[2];
}

// One point: returns false when the point is dropped.
__device__ __forceinline__ bool augment_point(const AugParams& p, uint32_t seed, uint32_t i, float& x, float& y, float& z,
                                              float& intensity) {
  if (!in_range(p, x, y, z)) return false;
  if (p.flags & FRCNN_AUG_GAUSS) {
    x += p.sigma[0] * normal01(seed, LA_NORMAL_GAUSS + 0, i);
    y += p.sigma[1] * normal01(seed, LA_NORMAL_GAUSS + 1, i);
    z += p.sigma[2] * normal01(seed, LA_NORMAL_GAUSS + 2, i);
  }
  if ((p.flags & FRCNN_AUG_DROPOUT) && !(uniform01(seed, LA_UNIFORM_DROPOUT, i) < p.p_keep)) return false;
  if (p.flags & FRCNN_AUG_ROTATE) {
    const float xr = p.cosa * x - p.sina * y, yr = p.sina * x + p.cosa * y;
    x = xr; y = yr;
  }
  if (p.flags & FRCNN_AUG_SWAP_XY) {
    const float xs = y - p.swap_x_off, ys = x - p.swap_y_off;
    x = xs; y = ys;
  }
  if (p.flags & FRCNN_AUG_FLIP_Y) y = -y;
  if (p.flags & FRCNN_AUG_FLIP_X) x = -x + p.flip_x_off;
  if (p.flags & FRCNN_AUG_RAIN) {
    float r = sqrtf((x * x + y * y) + z * z);
    const float shift = (p.rain_sigma_k * r) * normal01(seed, LA_NORMAL_RAIN, i);
    const float third = shift / 3.0f;
    x += third; y += third; z += third;
    r += shift;
    const float delta = expf(-(p.rain_att_k * r));
    intensity *= delta;
    const float p_n = p.rain_rho / (r * r + 2.220446049250313e-16f) * delta;
    if (!(p_n >= p.rain_p_min)) return false;                 // attenuated away (a NaN power is dropped too)
  }
  if ((p.flags & FRCNN_AUG_TEST_DROPOUT) && !(uniform01(seed, LA_UNIFORM_TEST_DROPOUT, i) < p.test_p_keep)) return false;
  return true;
}

struct NoFov {};
__device__ __forceinline__ bool in_fov(const NoFov&, float, float, float) { return true; }

// VEC4: rows of exactly four floats, both pointers 16-byte aligned -> one 16-byte load and store per point.
// Cam = FovParams: the field-of-view step runs first; Cam = NoFov: the step and its arguments are compiled out.
template <bool VEC4, typename Cam>
__global__ __launch_bounds__(256) void frcnn_lidar_augment_kernel(const float* in, AugParams p, Cam cam, uint32_t seed,
                                                                 const uint32_t* __restrict__ seed_dev, float* out,
                                                                 int* __restrict__ kept) {   // out may be `in` (in place)
  if (seed_dev) seed += *seed_dev;      // per-frame seed from device memory (a replayed hipGraph keeps `seed` itself)
  const float nan = __uint_as_float(0x7FC00000u);
  int alive = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gridDim.x * blockDim.x) {
    float x, y, z, w;
    if (VEC4) {
      const float4 q = reinterpret_cast<const float4*>(in)[i];
      x = q.x; y = q.y; z = q.z; w = q.w;
    } else {
      const float* q = in + (size_t)i * p.f;
      x = q[0]; y = q[1]; z = q[2]; w = q[3];
    }
    const bool keep = in_fov(cam, x, y, z) && augment_point(p, seed, (uint32_t)i, x, y, z, w);
    if (!keep) x = y = z = nan;
    alive += keep && in_range(p, x, y, z);                    // the reference's second filter_points (:426)
    if (VEC4) {
      reinterpret_cast<float4*>(out)[i] = make_float4(x, y, z, w);
    } else {
      float* o = out + (size_t)i * p.f;
      if (o != in + (size_t)i * p.f)
        for (int c = 4; c < p.f; ++c) o[c] = in[(size_t)i * p.f + c];
      o[0] = x; o[1] = y; o[2] = z; o[3] = w;
    }
  }
  // surviving points: ONE global atomic per workgroup (the atl_label_kernel pattern); integer sum, any order
  __shared__ int s_cnt[4];
  for (int off = 32; off > 0; off >>= 1) alive += __shfl_xor(alive, off);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = alive;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
    if (total) atomicAdd(kept, total);
  }
}

template <typename Cam>
void launch(unsigned blocks, bool vec4, hipStream_t stream, const float* points, const AugParams& p, const Cam& cam,
            uint32_t seed, const uint32_t* seed_dev, float* out, int* kept_count) {
  if (vec4)
    hipLaunchKernelGGL((frcnn_lidar_augment_kernel<true, Cam>), dim3(blocks), dim3(256), 0, stream, points, p, cam, seed,
                       seed_dev, out, kept_count);
  else
    hipLaunchKernelGGL((frcnn_lidar_augment_kernel<false, Cam>), dim3(blocks), dim3(256), 0, stream, points, p, cam, seed,
                       seed_dev, out, kept_count);
}

// both entries; proj_host == nullptr: no field-of-view step
int lidar_augment(const float* points, int num_points, int point_stride, const float* range_host, unsigned flags,
                  const float* params_host, uint32_t seed, const uint32_t* seed_dev, float* out, int* kept_count,
                  int max_blocks, const double* proj_host, int img_h, int img_w, hipStream_t stream) {
  FRCNN_REQUIRE(points && range_host && params_host && out && kept_count, "lidar_augment: null argument");
  FRCNN_REQUIRE(num_points > 0 && point_stride >= 4,
                "lidar_augment: bad arguments (points are num_points > 0 rows of >= 4 floats x,y,z,intensity)");
  const size_t span = (size_t)num_points * point_stride;
  FRCNN_REQUIRE(out == points || out + span <= points || points + span <= out,
                "lidar_augment: out must be the input itself (in place) or not overlap it");
  FRCNN_REQUIRE((flags & ~(unsigned)FRCNN_AUG_ALL) == 0, "lidar_augment: unknown flag bits 0x%x", flags);
  FRCNN_REQUIRE(max_blocks >= 0, "lidar_augment: max_blocks %d < 0", max_blocks);
  AugParams p;
  for (int j = 0; j < 3; ++j) {
    p.lo[j] = range_host[j];
    p.hi[j] = range_host[3 + j];
    FRCNN_REQUIRE(p.hi[j] > p.lo[j], "lidar_augment: empty range on axis %d", j);
    p.sigma[j] = params_host[FRCNN_AUG_P_SIGMA_X + j];
  }
  p.flags = flags;
  p.p_keep = params_host[FRCNN_AUG_P_KEEP];
  p.cosa = params_host[FRCNN_AUG_P_COS];
  p.sina = params_host[FRCNN_AUG_P_SIN];
  if (flags & FRCNN_AUG_GAUSS)
    FRCNN_REQUIRE(p.sigma[0] >= 0.f && p.sigma[1] >= 0.f && p.sigma[2] >= 0.f, "lidar_augment: negative sigma");
  FRCNN_REQUIRE(p.p_keep > 0.f && p.p_keep <= 1.f, "lidar_augment: p_keep %g outside (0, 1]", (double)p.p_keep);
  if (flags & FRCNN_AUG_ROTATE)
    FRCNN_REQUIRE(std::fabs(p.cosa) <= 1.f && std::fabs(p.sina) <= 1.f, "lidar_augment: cos / sin outside [-1, 1]");
  // the reference's offsets, evaluated in double like its Python floats and rounded once (:353,361,369-370,389)
  p.swap_x_off = range_host[1];
  p.swap_y_off = (float)(((double)range_host[3] - (double)range_host[0]) / 2.0);
  p.flip_x_off = range_host[3];
  p.rain_sigma_k = p.rain_att_k = p.rain_rho = p.rain_p_min = 0.f;
  if (flags & FRCNN_AUG_RAIN) {
    const double rate = params_host[FRCNN_AUG_P_RAIN_RATE], r_max = params_host[FRCNN_AUG_P_RAIN_MAX_RANGE];
    FRCNN_REQUIRE(rate > 0.0 && r_max > 0.0, "lidar_augment: rain needs rain_rate > 0 and max_range > 0 (got %g, %g)", rate,
                  r_max);
    const double pi = 3.14159265358979323846, rho = 0.9 / pi;
    p.rain_sigma_k = (float)(0.02 * std::pow(1.0 - std::exp(-rate), 2.0));
    p.rain_att_k = (float)(2.0 * 0.01 * std::pow(rate, 0.6));
    p.rain_rho = (float)rho;
    p.rain_p_min = (float)(rho / (pi * r_max * r_max));
  }
  p.test_p_keep = 0.8f;
  p.n = num_points;
  p.f = point_stride;
  FovParams cam = {};
  if (proj_host) {
    FRCNN_REQUIRE(img_h > 0 && img_w > 0, "lidar_augment_fov: image size %d x %d", img_h, img_w);
    for (int j = 0; j < 12; ++j) {
      FRCNN_REQUIRE(std::isfinite(proj_host[j]), "lidar_augment_fov: projection entry %d is not finite", j);
      cam.m[j] = proj_host[j];
    }
    cam.img_w = img_w;
    cam.img_h = img_h;
  }
  hipError_t e = fill_bytes(kept_count, 0, sizeof(int), stream);
  if (e != hipSuccess) return fail(FRCNN_ERR_LAUNCH, "lidar_augment: memset: %s", hipGetErrorString(e));
  unsigned blocks = (unsigned)std::min<size_t>(((size_t)num_points + 255) / 256, LA_MAX_BLOCKS);
  if (max_blocks > 0) blocks = std::min<unsigned>(blocks, (unsigned)max_blocks);
  const bool vec4 = point_stride == 4 && (reinterpret_cast<uintptr_t>(points) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (proj_host)
    launch(blocks, vec4, stream, points, p, cam, seed, seed_dev, out, kept_count);
  else
    launch(blocks, vec4, stream, points, p, NoFov{}, seed, seed_dev, out, kept_count);
  return check_launch("frcnn_lidar_augment_kernel");
}

}  // namespace

extern "C" int frcnn_lidar_augment(const float* points, int num_points, int point_stride, const float* range_host,
                                   unsigned flags, const float* params_host, uint32_t seed, const uint32_t* seed_dev,
                                   float* out, int* kept_count, int max_blocks, void* stream) {
  return lidar_augment(points, num_points, point_stride, range_host, flags, params_host, seed, seed_dev, out, kept_count,
                       max_blocks, nullptr, 0, 0, static_cast<hipStream_t>(stream));
}

extern "C" int frcnn_lidar_augment_fov(const float* points, int num_points, int point_stride, const float* range_host,
                                       unsigned flags, const float* params_host, uint32_t seed, const uint32_t* seed_dev,
                                       float* out, int* kept_count, int max_blocks, const double* proj_host, int img_h,
                                       int img_w, void* stream) {
  FRCNN_REQUIRE(proj_host, "lidar_augment_fov: null projection matrix");
  return lidar_augment(points, num_points, point_stride, range_host, flags, params_host, seed, seed_dev, out, kept_count,
                       max_blocks, proj_host, img_h, img_w, static_cast<hipStream_t>(stream));
}
