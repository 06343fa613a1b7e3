// Device-side rules the feature kernels share, each stated once.  The library is built with -ffp-contract=off and the tests compare
// bit patterns: every helper below is one expression tree, and a kernel calls it only where the text it replaces was that tree.
// (dvo_kernels.hip keeps its own forms: its sigma is (0.0019f * s) * s, another tree.)
#pragma once
#include <hip/hip_runtime.h>

// Pointers read from a record in memory are generic ("flat") to the compiler, and a flat access counts as an LDS access too: a
// wait for one gather would be a wait for all.  The planes live in device global memory: say so.
#define DVO_DEVICE_GLOBAL __attribute__((address_space(1)))

namespace dvo_amd {
namespace rules {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }  // (false for NaN)

// the sensor's depth noise at z (the reference's depthStdDevZ)
__device__ __forceinline__ float depth_sigma(float z) { return 0.0012f + 0.0019f * ((z - 0.4f) * (z - 0.4f)); }

// rows 0..2 of a row-major transformation applied to a point
__device__ __forceinline__ void transform_rows(const float *M, float x, float y, float z, float &qx, float &qy, float &qz) {
  qx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  qy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  qz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

// the pixel nearest to the projection of q, in float ...
__device__ __forceinline__ void nearest_pixel(float qx, float qy, float qz, float fx, float fy, float ox, float oy, float &pu, float &pv) {
  pu = floorf(((qx * fx) / qz + ox) + 0.5f);
  pv = floorf(((qy * fy) / qz + oy) + 0.5f);
}
// ... whether a w x h plane holds it (false for NaN), and its offset there: 0 <= pu <= w-1, 0 <= pv <= h-1 are tested in float
__device__ __forceinline__ bool pixel_inside(float pu, float pv, int w, int h) {
  return pu >= 0.0f && pu <= (float)(w - 1) && pv >= 0.0f && pv <= (float)(h - 1);
}
__device__ __forceinline__ size_t pixel_offset(float pu, float pv, int w) { return (size_t)(int)pv * (size_t)w + (size_t)(int)pu; }

// the pixel of a w x h plane nearest to the projection of q: 1 behind near_z, 2 outside the plane, else 0 and its offset in `at`
__device__ __forceinline__ int project_nearest(float qx, float qy, float qz, float near_z, float fx, float fy, float ox, float oy, int w,
                                               int h, size_t &at) {
  if (!(qz >= near_z)) return 1;
  float pu, pv;
  nearest_pixel(qx, qy, qz, fx, fy, ox, oy, pu, pv);
  if (!pixel_inside(pu, pv, w, h)) return 2;
  at = pixel_offset(pu, pv, w);
  return 0;
}

// a point at depth qz against the depth zs its pixel holds: 3 no depth there, 4 consistent, 5 occluded, 6 seen through
__device__ __forceinline__ int classify_depth(float zs, float qz, float sigmas) {
  if (!(zs == zs)) return 3;
  const float tol = sigmas * depth_sigma(qz);
  const float d = zs - qz;
  return d < -tol ? 5 : (d > tol ? 6 : 4);
}

// The covisibility rule (include/dvo_amd.h, dvo_amd_mask_warp) for a pixel of depth z and rays (tx, ty): -1 no depth, 1 behind,
// 2 outside, else classify_depth against `plane`, a w x h depth plane with the intrinsics given, `at` being where the pixel lands
// (set for the classes 3..6).  A caller that reads the rays only where there is a depth tests finite_f(z) itself first: the test
// here then folds away.  (project_nearest's steps written out, nested: the gather stays inside the branch that needs it.)
__device__ __forceinline__ int classify_covisible(float z, float tx, float ty, const float *T, float near_z, float sigmas, const float *plane,
                                                  int w, int h, float fx, float fy, float ox, float oy, size_t &at) {
  int cls = -1;
  if (finite_f(z)) {
    float qx, qy, qz, pu, pv;
    transform_rows(T, tx * z, ty * z, z, qx, qy, qz);
    if (!(qz >= near_z)) {
      cls = 1;
    } else {
      nearest_pixel(qx, qy, qz, fx, fy, ox, oy, pu, pv);
      if (!pixel_inside(pu, pv, w, h)) {
        cls = 2;
      } else {
        at = pixel_offset(pu, pv, w);
        cls = classify_depth(plane[at], qz, sigmas);
      }
    }
  }
  return cls;
}

// the sum of v over the wave, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a depth buffer's word keeps the minimum.  The stale value a plain load may return is never smaller than the word in memory:
// skipping the atomic on it is exact
__device__ __forceinline__ void depth_min(unsigned *z, unsigned word) {
  if (*z > word) atomicMin(z, word);
}
__device__ __forceinline__ void depth_min(unsigned long long *z, unsigned long long word) {
  if (*z > word) atomicMin(z, word);
}

// One axis of what a splatted point covers (dvo_amd.h: rule 5 of dvo_amd_map_render, the registration's and the forward warp's
// splat rule), in float: lo..hi before clamping.  kFootprintFill falls back to the nearest pixel where the footprint holds none.
enum { kFootprintNearest = 0, kFootprintFloor = 1, kFootprintFill = 2 };
__device__ __forceinline__ void footprint_span(float c, float half, int mode, float &lo, float &hi) {
  if (mode == kFootprintFloor) {
    lo = hi = floorf(c);
  } else if (mode == kFootprintNearest) {
    lo = hi = floorf(c + 0.5f);
  } else {
    lo = ceilf(c - half), hi = floorf(c + half);
    if (hi < lo) lo = hi = floorf(c + 0.5f);
  }
}
// ... and clamped to an axis of `size` pixels, compared in float before any conversion to int; false: no pixel is covered
__device__ __forceinline__ bool footprint_axis(float c, float half, int mode, int size, int &lo, int &hi) {
  float a, b;
  footprint_span(c, half, mode, a, b);
  const float last = (float)(size - 1);
  if (!(b >= 0.0f && a <= last)) return false;
  lo = a > 0.0f ? (int)a : 0;
  hi = b < last ? (int)b : size - 1;
  return true;
}

// Exclusive scan of one value per thread over a block of kWaves waves; *total = the block's sum.  The barrier in front keeps a
// wave from writing s_wave while another still reads what an earlier call left: safe for repeated calls in one kernel.
template <int kWaves>
__device__ unsigned block_exclusive_scan(unsigned v, unsigned *total) {
  __shared__ unsigned s_wave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned before = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const unsigned s = s_wave[w];
    if (w < wave) before += s;
    all += s;
  }
  *total = all;
  return before + inc - v;
}

}  // namespace rules
}  // namespace dvo_amd
