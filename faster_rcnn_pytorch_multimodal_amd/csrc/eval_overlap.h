// Overlap of one detection with one ground-truth box, the four forms of datasets/waymo_eval.py iou() restated term for
// term in double, in the same order of operations (compile with -ffp-contract=off: every product and sum rounds once,
// like the Python / numpy expression it restates).  Host and device: the host build is what a CPU check links.
//
//   '2d'      [x1,y1,x2,y2], VOC +1 pixel convention            (waymo_eval.py iou, '2d' branch)
//   'bev_aa'  [xc,yc,zc,l,w,h,ry] as yaw-less rectangles         ('bev_aa' branch)
//   'bev'     rotated rectangles: the detection's four counter-clockwise corners clipped against the gt's four edges
//             (Sutherland-Hodgman, _poly_clip), shoelace area (_poly_area)
//   '3d'      the 'bev' intersection area times the height overlap
//
// A box is split into what depends on it alone (BoxGeom: corners, edge vectors, areas, height range), computed ONCE per
// box, and the pair step, which reads two BoxGeoms.  The clipped polygon (at most 8 vertices for convex input) lives in
// a caller-supplied strided slot, `Poly`: on the device a per-lane LDS column, so its runtime-indexed appends cost no
// scratch memory.  Appends past EVAL_MAX_VERTS are dropped (never stored): memory safety for sign patterns that only a
// numerically degenerate (zero-size) box could produce.
#pragma once
#include <cmath>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define EVAL_TYPE_2D 0
#define EVAL_TYPE_BEV_AA 1
#define EVAL_TYPE_BEV 2
#define EVAL_TYPE_3D 3
#define EVAL_MAX_VERTS 8
// doubles per staged box: corners x[4] y[4], edge vectors ex[4] ey[4], area, zlo, zhi, volume
#define EVAL_GEOM_DOUBLES 20

namespace frcnn_eval {

// Python's max(a, b) / min(a, b) on floats: the first argument unless the second is strictly greater / smaller.
__host__ __device__ inline double py_max(double a, double b) { return b > a ? b : a; }
__host__ __device__ inline double py_min(double a, double b) { return b < a ? b : a; }

// What one box contributes to every pair it takes part in.  For '2d' cx[0..3] hold x1,y1,x2,y2 and for 'bev_aa' the
// rectangle gx1,gy1,gx2,gy2; `area` is the box's own term of the union.
struct BoxGeom {
  double cx[4], cy[4], ex[4], ey[4];
  double area, zlo, zhi, vol;
};

template <int TYPE>
__host__ __device__ inline void box_geom(const double* b, BoxGeom& g) {
  if (TYPE == EVAL_TYPE_2D) {
    g.cx[0] = b[0]; g.cx[1] = b[1]; g.cx[2] = b[2]; g.cx[3] = b[3];
    g.area = (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0);
    return;
  }
  if (TYPE == EVAL_TYPE_BEV_AA) {
    g.cx[0] = b[0] - b[3] / 2; g.cx[1] = b[1] - b[4] / 2; g.cx[2] = b[0] + b[3] / 2; g.cx[3] = b[1] + b[4] / 2;
    g.area = (g.cx[2] - g.cx[0]) * (g.cx[3] - g.cx[1]);
    return;
  }
  // _bev_corners: (l/2, w/2), (-l/2, w/2), (-l/2, -w/2), (l/2, -w/2) turned by ry about (xc, yc)
  const double xc = b[0], yc = b[1], hl = b[3] / 2, hw = b[4] / 2;
  const double c = cos(b[6]), s = sin(b[6]);
  const double px[4] = {hl, -hl, -hl, hl}, py[4] = {hw, hw, -hw, -hw};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.cx[k] = xc + c * px[k] - s * py[k];
    g.cy[k] = yc + s * px[k] + c * py[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {            // edge a -> b of _poly_clip: a = corner k, b = corner k + 1
    g.ex[k] = g.cx[(k + 1) & 3] - g.cx[k];
    g.ey[k] = g.cy[(k + 1) & 3] - g.cy[k];
  }
  g.area = b[3] * b[4];
  if (TYPE == EVAL_TYPE_3D) {
    g.zlo = b[2] - b[5] / 2;
    g.zhi = b[2] + b[5] / 2;
    g.vol = g.area * b[5];
  }
}

// A polygon of up to EVAL_MAX_VERTS vertices in strided storage: vertex k at x[k * stride], y[k * stride].
struct Poly {
  double* x;
  double* y;
  int stride;
  __host__ __device__ inline void put(int k, double vx, double vy) const {
    if (k < EVAL_MAX_VERTS) {
      x[k * stride] = vx;
      y[k * stride] = vy;
    }
  }
};

// One vertex p -> q step of _poly_clip against the edge (ax, ay) + t (ex, ey); returns the new vertex count.
__host__ __device__ inline int clip_step(const Poly& out, int n, double p0, double p1, double q0, double q1, double ax,
                                         double ay, double ex, double ey) {
  const double side_p = ex * (p1 - ay) - ey * (p0 - ax);
  const double side_q = ex * (q1 - ay) - ey * (q0 - ax);
  if (side_p >= 0) {
    out.put(n, p0, p1);
    ++n;
  }
  if ((side_p >= 0) != (side_q >= 0)) {
    const double t = side_p / (side_p - side_q);
    out.put(n, p0 + t * (q0 - p0), p1 + t * (q1 - p1));
    ++n;
  }
  return n;
}

// Area of (detection polygon) clipped by (gt polygon): _poly_area(_poly_clip(det corners, gt corners)).  a and b are two
// polygon slots of the caller that are used in turn.
__host__ __device__ inline double clip_area(const BoxGeom& det, const BoxGeom& gt, const Poly& a, const Poly& b) {
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)                       // edge 0: the subject is the detection's corners, in registers
    n = clip_step(a, n, det.cx[j], det.cy[j], det.cx[(j + 1) & 3], det.cy[(j + 1) & 3], gt.cx[0], gt.cy[0], gt.ex[0],
                  gt.ey[0]);
  n = n < EVAL_MAX_VERTS ? n : EVAL_MAX_VERTS;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const Poly& in = (i & 1) ? a : b;
    const Poly& out = (i & 1) ? b : a;
    if (n == 0) break;                              // `if not inp: break`
    int m = 0;
    double p0 = in.x[0], p1 = in.y[0];
    const double f0 = p0, f1 = p1;
    for (int j = 0; j < n; ++j) {
      const bool last = j + 1 == n;
      const double q0 = last ? f0 : in.x[(j + 1) * in.stride], q1 = last ? f1 : in.y[(j + 1) * in.stride];
      m = clip_step(out, m, p0, p1, q0, q1, gt.cx[i], gt.cy[i], gt.ex[i], gt.ey[i]);
      p0 = q0;
      p1 = q1;
    }
    n = m < EVAL_MAX_VERTS ? m : EVAL_MAX_VERTS;
  }
  if (n < 3) return 0.0;
  const Poly& r = b;                                // edges 1, 2, 3 end in b; n == 0 after edge 0 returned above
  // np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)), each dot summed left to right
  const double x0 = r.x[0], y0 = r.y[0];
  double xp = x0, yp = y0, d1 = 0.0, d2 = 0.0;
  for (int k = 1; k <= n; ++k) {
    const double xk = k == n ? x0 : r.x[k * r.stride], yk = k == n ? y0 : r.y[k * r.stride];
    const double t1 = xp * yk, t2 = yp * xk;
    d1 = k == 1 ? t1 : d1 + t1;
    d2 = k == 1 ? t2 : d2 + t2;
    xp = xk;
    yp = yk;
  }
  return 0.5 * fabs(d1 - d2);
}

template <int TYPE>
__host__ __device__ inline double pair_overlap(const BoxGeom& det, const BoxGeom& gt, const Poly& a, const Poly& b) {
  if (TYPE == EVAL_TYPE_2D) {
    const double ixmin = fmax(gt.cx[0], det.cx[0]), iymin = fmax(gt.cx[1], det.cx[1]);
    const double ixmax = fmin(gt.cx[2], det.cx[2]), iymax = fmin(gt.cx[3], det.cx[3]);
    const double iw = fmax(ixmax - ixmin + 1.0, 0.0), ih = fmax(iymax - iymin + 1.0, 0.0);
    const double inters = iw * ih;
    return inters / (det.area + gt.area - inters);
  }
  if (TYPE == EVAL_TYPE_BEV_AA) {
    const double iw = fmax(fmin(gt.cx[2], det.cx[2]) - fmax(gt.cx[0], det.cx[0]), 0.0);
    const double ih = fmax(fmin(gt.cx[3], det.cx[3]) - fmax(gt.cx[1], det.cx[1]), 0.0);
    const double inters = iw * ih;
    return inters / (gt.area + det.area - inters);
  }
  const double inter = clip_area(det, gt, a, b);
  if (TYPE == EVAL_TYPE_BEV) return inter / (det.area + gt.area - inter);
  const double zlo = py_max(det.zlo, gt.zlo), zhi = py_min(det.zhi, gt.zhi);
  const double vol = inter * py_max(zhi - zlo, 0.0);
  return vol / (det.vol + gt.vol - vol);
}

}  // namespace frcnn_eval
