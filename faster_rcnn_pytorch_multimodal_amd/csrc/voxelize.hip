// LiDAR input producer on the device: point cloud -> bird's-eye-view blob (lib/roi_data_layer/minibatch.py:434-512,
// SURVEY.md 8f-1).  The reference voxelises on the CPU with spconv.utils.VoxelGeneratorV2 (third party, not vendored:
// PARITY UNPINNED - its published points_to_voxel loop is restated) and scatters with numpy:
//
//   for each point in file order: cell = floor((p - range_min) / voxel_size) (fp32), dropped when outside the grid;
//   a cell seen for the first time becomes voxel number `voxel_num` unless max_voxels voxels already exist (then the
//   point is skipped); a voxel keeps its first max_points points.
//   bev[x, y, z]            = max z of the voxel's points - z * VOXEL_HEIGHT                    (height slices;
//                             int32 * Python float: float64, rounded once on the store into the fp32 map)
//   bev[x, y, NUM_SLICES]   = num_points / MAX_PTS_PER_VOXEL                                     (density)
//   bev[x, y, NUM_SLICES+1] = tanh(sum(intensity) / num_points)       (+2: same for elongation, or tanh(0) = 0)
//   the meta channels are written per VOXEL into the (x, y) column, so the voxel created last in a column wins;
//   finally the map is transposed to (y, x, c).
//
// Order-dependent parts and how they are made parallel yet exact: "voxel number" = rank of the voxel's first point
// index (atomicMin per cell, then an exclusive scan over the points); "first max_points points" = the max_points
// smallest point indices of the cell (per-voxel segments filled in arbitrary order, then one wave per voxel extracts
// the smallest indices one by one); "last voxel of a column wins" = atomicMax of the voxel number per column.
// Sums run in ascending point order, so the output does not depend on the order in which atomics land.
// HBM/latency-bound integer work; the dense cell table (gx*gy*gz int32, 27 MB at 0.1 m voxels) lives in HBM.
#include "common.h"

#include <algorithm>

using namespace frcnn;

namespace {

struct VoxParams {
  float rmin[3], vsize[3];
  float fmin[3], fmax[3];   // filter_points (minibatch.py:232-235) on the raw coordinates: fmin <= p < fmax
  int grid[3];        // gx, gy, gz
  float z_shift;      // source_bin[:, 2] -= cfg.LIDAR.Z_RANGE[0]
  int n, f, max_points, max_voxels, num_slices, num_meta, elong_col;
  double voxel_height;      // cfg.LIDAR.VOXEL_HEIGHT as the caller holds it; vsize[2] is its fp32 rounding
};

constexpr int NO_POINT = 0x7F7F7F7F;   // hipMemset pattern of the cell table

__global__ __launch_bounds__(256) void vox_cell_kernel(const float* __restrict__ pts, VoxParams p, int* __restrict__ cell,
                                                      int* __restrict__ first) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gridDim.x * blockDim.x) {
    const float* q = pts + (size_t)i * p.f;
    const float v[3] = {q[0], q[1], q[2] - p.z_shift};
    int c[3];
    bool ok = q[0] >= p.fmin[0] && q[1] >= p.fmin[1] && q[2] >= p.fmin[2] && q[0] < p.fmax[0] && q[1] < p.fmax[1] &&
              q[2] < p.fmax[2];
    for (int j = 0; j < 3; ++j) {
      const float t = floorf((v[j] - p.rmin[j]) / p.vsize[j]);
      ok = ok && t >= 0.f && t < (float)p.grid[j];
      c[j] = (int)t;
    }
    int id = -1;
    if (ok) {
      id = (c[2] * p.grid[1] + c[1]) * p.grid[0] + c[0];
      atomicMin(first + id, i);
    }
    cell[i] = id;
  }
}

__global__ __launch_bounds__(256) void vox_flag_kernel(const int* __restrict__ cell, const int* __restrict__ first, int n,
                                                      int* __restrict__ flag) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    flag[i] = (cell[i] >= 0 && first[cell[i]] == i) ? 1 : 0;
}

// out[i] = sum(in[0..i)), *total = sum(in[0..n)); one workgroup walks the array in tiles of 4096 consecutive items
// (4 per thread, coalesced), scanning each tile through the waves (shuffle scan + 16 wave totals in LDS) and carrying
// the running sum.
__global__ __launch_bounds__(1024) void scan_excl_kernel(const int* __restrict__ in, int n, int* __restrict__ out,
                                                        int* __restrict__ total) {
  __shared__ int wave_sum[16];
  __shared__ int carry_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 4096) {
    const int i = base + 4 * t;
    int v[4];
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? in[i + e] : 0;
    const int mine = (v[0] + v[1]) + (v[2] + v[3]);
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int run = carry_s + incl - mine;
    for (int w = 0; w < wave; ++w) run += wave_sum[w];
    for (int e = 0; e < 4; ++e) {
      if (i + e < n) out[i + e] = run;
      run += v[e];
    }
    __syncthreads();
    if (t == 1023) carry_s = run;
    __syncthreads();
  }
  if (t == 0 && total) *total = carry_s;
}

__global__ __launch_bounds__(256) void vox_count_kernel(const int* __restrict__ cell, const int* __restrict__ first,
                                                       const int* __restrict__ prank, const int* __restrict__ flag, int n,
                                                       int max_voxels, int* __restrict__ vox_of_point,
                                                       int* __restrict__ cnt, int* __restrict__ vcell) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int v = -1;
    if (cell[i] >= 0) {
      v = prank[first[cell[i]]];
      if (v >= max_voxels) v = -1;          // the voxel table was already full when this cell first appeared
      else {
        atomicAdd(cnt + v, 1);
        if (flag[i]) vcell[v] = cell[i];
      }
    }
    vox_of_point[i] = v;
  }
}

__global__ __launch_bounds__(256) void vox_fill_kernel(const int* __restrict__ vox_of_point, const int* __restrict__ off,
                                                      int n, int* __restrict__ cursor, int* __restrict__ seg) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int v = vox_of_point[i];
    if (v >= 0) seg[off[v] + atomicAdd(cursor + v, 1)] = i;
  }
}

__device__ __forceinline__ int wave_min_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// One wave per voxel: the max_points smallest point indices of the segment in ascending order, then the features.
__global__ __launch_bounds__(256) void vox_feature_kernel(const float* __restrict__ pts, VoxParams p,
                                                         const int* __restrict__ total_voxels,
                                                         const int* __restrict__ cnt, const int* __restrict__ off,
                                                         const int* __restrict__ seg, const int* __restrict__ vcell,
                                                         int* __restrict__ col_last, float* __restrict__ vfeat,
                                                         float* __restrict__ bev) {
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int V = min(*total_voxels, p.max_voxels);
  if (v >= V) return;
  const int n = cnt[v], base = off[v];
  const int keep = min(n, p.max_points);
  // np.amax over the zero-initialised (max_points, F) voxel buffer: a voxel that is not full has rows of zeros
  float zmax = keep < p.max_points ? 0.f : -INFINITY;
  float isum = 0.f, esum = 0.f;
  int prev = -1;
  for (int k = 0; k < keep; ++k) {
    int best = NO_POINT;
    for (int j = lane; j < n; j += 64) {
      const int idx = seg[base + j];
      if (idx > prev) best = min(best, idx);
    }
    best = wave_min_i32(best);
    prev = best;
    const float* q = pts + (size_t)best * p.f;
    zmax = fmaxf(zmax, q[2] - p.z_shift);
    isum += q[3];
    if (p.elong_col >= 0) esum += q[p.elong_col];
  }
  if (lane != 0) return;
  const int id = vcell[v];
  const int cx = id % p.grid[0], cy = (id / p.grid[0]) % p.grid[1], cz = id / (p.grid[0] * p.grid[1]);
  const int C = p.num_slices + p.num_meta;
  float* px = bev + ((size_t)cy * p.grid[0] + cx) * C;          // (y, x, c): the reference's final transpose
  if (cz < p.num_slices) px[cz] = (float)((double)zmax - (double)cz * p.voxel_height);   // the reference's float64
  atomicMax(col_last + cy * p.grid[0] + cx, v);
  vfeat[(size_t)v * 4 + 0] = (float)((double)keep / (double)p.max_points);
  vfeat[(size_t)v * 4 + 1] = (float)tanh((double)isum / (double)keep);
  vfeat[(size_t)v * 4 + 2] = p.elong_col >= 0 ? (float)tanh((double)esum / (double)keep) : 0.f;
}

__global__ __launch_bounds__(256) void vox_meta_kernel(VoxParams p, const int* __restrict__ total_voxels,
                                                      const int* __restrict__ vcell, const int* __restrict__ col_last,
                                                      const float* __restrict__ vfeat, float* __restrict__ bev) {
  const int V = min(*total_voxels, p.max_voxels);
  const int C = p.num_slices + p.num_meta;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    const int id = vcell[v];
    const int cx = id % p.grid[0], cy = (id / p.grid[0]) % p.grid[1];
    if (col_last[cy * p.grid[0] + cx] != v) continue;
    float* px = bev + ((size_t)cy * p.grid[0] + cx) * C;
    for (int m = 0; m < p.num_meta && m < 3; ++m) px[p.num_slices + m] = vfeat[(size_t)v * 4 + m];
  }
}

struct VoxLayout {
  size_t cell, first, flag, prank, total, vox_of_point, cnt, off, cursor, vcell, seg, col_last, vfeat, bytes;
};
VoxLayout vox_layout(int n, long cells, long cols, int max_voxels) {
  VoxLayout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  l.cell = take((size_t)n * 4);
  l.first = take((size_t)cells * 4);
  l.flag = take((size_t)n * 4);
  l.prank = take((size_t)n * 4);
  l.total = take(16);
  l.vox_of_point = take((size_t)n * 4);
  l.cnt = take((size_t)max_voxels * 4);
  l.off = take((size_t)max_voxels * 4);
  l.cursor = take((size_t)max_voxels * 4);
  l.vcell = take((size_t)max_voxels * 4);
  l.seg = take((size_t)n * 4);
  l.col_last = take((size_t)cols * 4);
  l.vfeat = take((size_t)max_voxels * 16);
  l.bytes = o;
  return l;
}

bool grid_of(const float* range, const float* vsize, int* grid) {
  for (int j = 0; j < 3; ++j) {
    if (!(vsize[j] > 0.f) || !(range[3 + j] > range[j])) return false;
    grid[j] = (int)lrintf((range[3 + j] - range[j]) / vsize[j]);     // spconv: np.round((max - min) / voxel_size)
    if (grid[j] <= 0) return false;
  }
  return (long)grid[0] * grid[1] * grid[2] < (1L << 30);
}

unsigned blocks_for(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, 4096)); }

}  // namespace

extern "C" int frcnn_bev_voxelize_grid(const float* pc_range_host, const float* voxel_size_host, int* grid_host) {
  FRCNN_REQUIRE(pc_range_host && voxel_size_host && grid_host, "bev_voxelize_grid: null argument");
  FRCNN_REQUIRE(grid_of(pc_range_host, voxel_size_host, grid_host), "bev_voxelize_grid: empty or oversized grid");
  return FRCNN_OK;
}

extern "C" size_t frcnn_bev_voxelize_ws_bytes(int num_points, const float* pc_range_host, const float* voxel_size_host,
                                              int max_voxels) {
  int g[3];
  if (num_points <= 0 || max_voxels <= 0 || !pc_range_host || !voxel_size_host ||
      !grid_of(pc_range_host, voxel_size_host, g))
    return 0;
  return vox_layout(num_points, (long)g[0] * g[1] * g[2], (long)g[0] * g[1], max_voxels).bytes;
}

extern "C" int frcnn_bev_voxelize_h(const float* points, int num_points, int point_stride, const float* pc_range_host,
                                    const float* voxel_size_host, double voxel_height, float z_shift, int max_points,
                                    int max_voxels, int num_slices, int num_meta, int elongation_col, float* bev,
                                    int* num_voxels, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FRCNN_REQUIRE(points && pc_range_host && voxel_size_host && bev && num_points > 0 && point_stride >= 4 &&
                    max_points > 0 && max_voxels > 0 && num_slices > 0 && num_meta >= 0 && num_meta <= 3 &&
                    elongation_col < point_stride,
                "bev_voxelize: bad arguments (points are rows of >= 4 floats x,y,z,intensity)");
  FRCNN_REQUIRE((float)voxel_height == voxel_size_host[2],
                "bev_voxelize: voxel_height %.17g is not the double that voxel_size[2] = %.9g was rounded from",
                voxel_height, (double)voxel_size_host[2]);
  VoxParams p;
  FRCNN_REQUIRE(grid_of(pc_range_host, voxel_size_host, p.grid), "bev_voxelize: empty or oversized grid");
  FRCNN_REQUIRE(p.grid[2] <= num_slices, "bev_voxelize: %d z cells but %d height slices", p.grid[2], num_slices);
  for (int j = 0; j < 3; ++j) { p.rmin[j] = pc_range_host[j]; p.vsize[j] = voxel_size_host[j]; }
  p.z_shift = z_shift;
  p.fmin[0] = pc_range_host[0]; p.fmin[1] = pc_range_host[1]; p.fmin[2] = pc_range_host[2] + z_shift;
  p.fmax[0] = pc_range_host[3]; p.fmax[1] = pc_range_host[4]; p.fmax[2] = pc_range_host[5] + z_shift;
  p.n = num_points; p.f = point_stride; p.max_points = max_points; p.max_voxels = max_voxels;
  p.num_slices = num_slices; p.num_meta = num_meta; p.elong_col = elongation_col;
  p.voxel_height = voxel_height;
  const long cells = (long)p.grid[0] * p.grid[1] * p.grid[2], cols = (long)p.grid[0] * p.grid[1];
  const VoxLayout l = vox_layout(num_points, cells, cols, max_voxels);
  if (!ws || ws_bytes < l.bytes) return fail(FRCNN_ERR_WS, "bev_voxelize: workspace %zu < %zu bytes", ws_bytes, l.bytes);
  char* w = static_cast<char*>(ws);
  auto ip = [&](size_t o) { return reinterpret_cast<int*>(w + o); };
  const int C = num_slices + num_meta;
  hipError_t e = fill_bytes(bev, 0, (size_t)cols * C * sizeof(float), stream);
  if (e == hipSuccess) e = fill_bytes(ip(l.first), 0x7F, (size_t)cells * 4, stream);
  if (e == hipSuccess) e = fill_bytes(ip(l.cnt), 0, l.vcell - l.cnt, stream);          // cnt, off, cursor
  if (e == hipSuccess) e = fill_bytes(ip(l.col_last), 0xFF, (size_t)cols * 4, stream);
  if (e != hipSuccess) return fail(FRCNN_ERR_LAUNCH, "bev_voxelize: memset: %s", hipGetErrorString(e));
  const unsigned pb = blocks_for(num_points);
  hipLaunchKernelGGL(vox_cell_kernel, dim3(pb), dim3(256), 0, stream, points, p, ip(l.cell), ip(l.first));
  hipLaunchKernelGGL(vox_flag_kernel, dim3(pb), dim3(256), 0, stream, ip(l.cell), ip(l.first), num_points, ip(l.flag));
  hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, stream, ip(l.flag), num_points, ip(l.prank), ip(l.total));
  hipLaunchKernelGGL(vox_count_kernel, dim3(pb), dim3(256), 0, stream, ip(l.cell), ip(l.first), ip(l.prank), ip(l.flag),
                     num_points, max_voxels, ip(l.vox_of_point), ip(l.cnt), ip(l.vcell));
  hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, stream, ip(l.cnt), max_voxels, ip(l.off),
                     static_cast<int*>(nullptr));
  hipLaunchKernelGGL(vox_fill_kernel, dim3(pb), dim3(256), 0, stream, ip(l.vox_of_point), ip(l.off), num_points,
                     ip(l.cursor), ip(l.seg));
  hipLaunchKernelGGL(vox_feature_kernel, dim3((max_voxels + 3) / 4), dim3(256), 0, stream, points, p, ip(l.total),
                     ip(l.cnt), ip(l.off), ip(l.seg), ip(l.vcell), ip(l.col_last),
                     reinterpret_cast<float*>(w + l.vfeat), bev);
  hipLaunchKernelGGL(vox_meta_kernel, dim3(blocks_for(max_voxels)), dim3(256), 0, stream, p, ip(l.total), ip(l.vcell),
                     ip(l.col_last), reinterpret_cast<const float*>(w + l.vfeat), bev);
  int rc = check_launch("bev_voxelize kernels");
  if (rc != FRCNN_OK) return rc;
  if (num_voxels) {
    e = copy_bytes(num_voxels, ip(l.total), sizeof(int), stream);
    if (e != hipSuccess) return fail(FRCNN_ERR_LAUNCH, "bev_voxelize: copy voxel count: %s", hipGetErrorString(e));
  }
  return FRCNN_OK;
}

extern "C" int frcnn_bev_voxelize(const float* points, int num_points, int point_stride, const float* pc_range_host,
                                  const float* voxel_size_host, float z_shift, int max_points, int max_voxels,
                                  int num_slices, int num_meta, int elongation_col, float* bev, int* num_voxels,
                                  void* ws, size_t ws_bytes, void* stream) {
  FRCNN_REQUIRE(voxel_size_host, "bev_voxelize: bad arguments (null voxel size)");
  return frcnn_bev_voxelize_h(points, num_points, point_stride, pc_range_host, voxel_size_host,
                              (double)voxel_size_host[2], z_shift, max_points, max_voxels, num_slices, num_meta,
                              elongation_col, bev, num_voxels, ws, ws_bytes, stream);
}
