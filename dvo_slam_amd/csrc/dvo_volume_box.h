// The frustum box of dvo_amd_volume's integration (include/dvo_amd.h, "A truncated signed-distance volume"): a conservative
// inclusive index box of (a frame's frustum between near_z and z_max = far_z + trunc) intersected with the volume.  Host code only,
// in double, no HIP: tests/volume_box_main.cpp compiles it alone and tests/volume_ref.py restates it operation by operation.
//
// The kernel decides in fp32 which voxels a frame updates; this box may only contain more.  Three things make it so:
//  - the frustum is the convex hull of eight corners (tangent bounds at z = near_z and z = z_max), an affine map keeps hulls, and
//    the axis-aligned box of the mapped corners holds the mapped hull;
//  - the tangent bounds lie a whole pixel outside the pixels the rule accepts (pu in 0..w-1 means px in [-0.5, w-0.5));
//  - the box grows by one voxel plus 1e-5 of the largest coordinate involved, in voxels: fifty times what the fp32 rounding of
//    the voxel position and of the transformation can move a point.
// The corners go back through the exact inverse of the matrix the kernel uses (the float entries, as doubles); a matrix that is
// not finite or far from a rotation (|det| outside [0.5, 2]), or any non-finite input, gives the whole volume.
#ifndef DVO_VOLUME_BOX_H
#define DVO_VOLUME_BOX_H

#include <cmath>

namespace dvo_amd {
namespace volume_box {

struct Box {
  int lo[3], hi[3];  // inclusive; empty: hi[a] < lo[a] on every axis ({0,0,0}, {-1,-1,-1})
};

inline Box whole(const int n[3]) {
  Box b;
  for (int a = 0; a < 3; ++a) b.lo[a] = 0, b.hi[a] = n[a] - 1;
  return b;
}

inline Box none() {
  Box b;
  for (int a = 0; a < 3; ++a) b.lo[a] = 0, b.hi[a] = -1;
  return b;
}

inline bool is_empty(const Box &b) { return b.hi[0] < b.lo[0] || b.hi[1] < b.lo[1] || b.hi[2] < b.lo[2]; }

// M: rows 0..2 of world -> camera, row-major (the kernel's floats); n: the volume's dimensions (each >= 1)
inline Box frustum_box(const double M[12], double fx, double fy, double ox, double oy, int w, int h, double near_z, double z_max,
                       const double origin[3], double voxel, const int n[3]) {
  const Box all = whole(n);
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(M[i])) return all;
  if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(ox) && std::isfinite(oy) && std::isfinite(near_z) && std::isfinite(z_max) &&
        std::isfinite(voxel) && std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
    return all;
  if (!(fx > 0.0 && fy > 0.0 && voxel > 0.0 && near_z > 0.0)) return all;
  if (!(z_max >= near_z)) return none();
  // the inverse of the 3x3 part by cofactors
  const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], hh = M[9], k = M[10];
  const double c00 = e * k - f * hh, c01 = c * hh - b * k, c02 = b * f - c * e;
  const double c10 = f * g - d * k, c11 = a * k - c * g, c12 = c * d - a * f;
  const double c20 = d * hh - e * g, c21 = b * g - a * hh, c22 = a * e - b * d;
  const double det = (a * c00 + b * c10) + c * c20;
  if (!(std::fabs(det) >= 0.5 && std::fabs(det) <= 2.0)) return all;
  const double inv[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
  const double tx[2] = {(-1.5 - ox) / fx, ((double)w + 0.5 - ox) / fx};
  const double ty[2] = {(-1.5 - oy) / fy, ((double)h + 0.5 - oy) / fy};
  const double zs[2] = {near_z, z_max};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  double scale = std::fmax(std::fmax(std::fabs(M[3]), std::fabs(M[7])), std::fabs(M[11]));
  for (int iz = 0; iz < 2; ++iz)
    for (int iy = 0; iy < 2; ++iy)
      for (int ix = 0; ix < 2; ++ix) {
        const double q[3] = {tx[ix] * zs[iz] - M[3], ty[iy] * zs[iz] - M[7], zs[iz] - M[11]};
        for (int r = 0; r < 3; ++r) {
          const double p = (inv[r * 3 + 0] * q[0] + inv[r * 3 + 1] * q[1]) + inv[r * 3 + 2] * q[2];
          if (!std::isfinite(p)) return all;
          lo[r] = std::fmin(lo[r], p), hi[r] = std::fmax(hi[r], p);
          scale = std::fmax(scale, std::fabs(p));
        }
      }
  for (int r = 0; r < 3; ++r) {
    scale = std::fmax(scale, std::fabs(origin[r]));
    scale = std::fmax(scale, std::fabs(origin[r] + (double)(n[r] - 1) * voxel));
  }
  const double margin = 1.0 + 1e-5 * (scale / voxel);
  if (!std::isfinite(margin)) return all;
  Box out;
  for (int r = 0; r < 3; ++r) {
    double g0 = std::floor((lo[r] - origin[r]) / voxel - margin), g1 = std::ceil((hi[r] - origin[r]) / voxel + margin);
    if (!std::isfinite(g0) || !std::isfinite(g1)) return all;
    const double last = (double)(n[r] - 1);
    if (g0 > last || g1 < 0.0) return none();
    if (g0 < 0.0) g0 = 0.0;   // (clamped in double: the conversions below are in range)
    if (g1 > last) g1 = last;
    out.lo[r] = (int)g0, out.hi[r] = (int)g1;
  }
  return out;
}

// the smallest box that holds both (an empty box adds nothing)
inline Box unite(const Box &p, const Box &q) {
  if (is_empty(p)) return q;
  if (is_empty(q)) return p;
  Box u;
  for (int a = 0; a < 3; ++a) u.lo[a] = p.lo[a] < q.lo[a] ? p.lo[a] : q.lo[a], u.hi[a] = p.hi[a] > q.hi[a] ? p.hi[a] : q.hi[a];
  return u;
}

}  // namespace volume_box
}  // namespace dvo_amd
#endif
