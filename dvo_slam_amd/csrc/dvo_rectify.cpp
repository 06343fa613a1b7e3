// Rectification at ingest: what image_proc does in front of the reference (cv::initUndistortRectifyMap + cv::remap on the CPU;
// camera_keyframe_tracking.cpp:89 takes its intrinsics from CameraInfo::P, the projection matrix of the RECTIFIED image) as
// device-resident remap tables and a resampling frame ingest.  The two rules are pinned operation by operation in
// include/dvo_amd.h; tests/rectify_ref.py restates them.
//   k_undistort_map   one lane per 4 consecutive output pixels: the five-coefficient model in fp32, two float4 stores; the
//                     pixels whose source position lies inside the source are counted per wave (ballots) with one integer
//                     atomic per wave
//   k_count_inside    the same count for a map pair that came from the host
//   k_grey_plane      a BGR source as a 1 B/px grey plane (k_ingest's integer rule): bit-identical to converting every tap,
//                     a third of the bytes the gather touches, and each source pixel is converted once instead of up to four times
//   k_ingest_remap    one lane per 4 output pixels of a row: two 16-byte map loads, four bilinear intensity taps and one
//                     nearest depth tap per pixel, two float4 stores -- the two base planes of level 0 as k_ingest writes
//                     them.  No atomics: every output has one writer, the result cannot depend on the launch geometry.
#include "dvo_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dvo_amd {
namespace rectify {

struct UndistortArgs {
  float fx, fy, ox, oy;              // k_out
  float fxs, fys, oxs, oys;          // k_src
  float k1, k2, two_p1, two_p2, k3;  // dist, the tangential pair doubled (2.0f * p: exact)
  float p1, p2;
};

// the sampling rule's step 1: in float, before any conversion to int (false for NaN, +-inf and anything an int cannot hold)
__device__ __forceinline__ bool inside_source(float sx, float sy, float wmax, float hmax) {
  return sx >= 0.0f && sx < wmax && sy >= 0.0f && sy < hmax;
}

// what the four pixels of every lane of a wave add to the count: one integer atomic per wave
__device__ __forceinline__ void count_inside(const bool in[4], int *n_inside) {
  unsigned cnt = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt += (unsigned)__popcll(__ballot(in[k]));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_inside, (int)cnt);
}

__global__ void __launch_bounds__(256) k_undistort_map(UndistortArgs A, int w, int n, float wmax, float hmax,
                                                       float *__restrict__ map_x, float *__restrict__ map_y,
                                                       int *__restrict__ n_inside) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;  // four pixels of one row (w % 4 == 0)
  const bool active = q * 4 < n;                         // (no early return: every lane takes part in the ballots)
  bool in[4] = {false, false, false, false};
  if (active) {
    const int v = (q * 4) / w, u0 = q * 4 - v * w;
    const float y = ((float)v - A.oy) / A.fy, yy = y * y;
    float mx[4], my[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = ((float)(u0 + k) - A.ox) / A.fx;
      const float xx = x * x, r2 = xx + yy, xy = x * y;
      const float rad = ((A.k3 * r2 + A.k2) * r2 + A.k1) * r2 + 1.0f;
      const float xd = x * rad + ((A.two_p1 * xy) + A.p2 * (r2 + (xx + xx)));
      const float yd = y * rad + (A.p1 * (r2 + (yy + yy)) + (A.two_p2 * xy));
      mx[k] = xd * A.fxs + A.oxs, my[k] = yd * A.fys + A.oys;
      in[k] = inside_source(mx[k], my[k], wmax, hmax);
    }
    *(float4 *)(map_x + (size_t)q * 4) = make_float4(mx[0], mx[1], mx[2], mx[3]);
    *(float4 *)(map_y + (size_t)q * 4) = make_float4(my[0], my[1], my[2], my[3]);
  }
  count_inside(in, n_inside);
}

__global__ void __launch_bounds__(256) k_count_inside(const float *__restrict__ map_x, const float *__restrict__ map_y, int n,
                                                      float wmax, float hmax, int *__restrict__ n_inside) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  bool in[4] = {false, false, false, false};
  if (q * 4 < n) {
    const float4 mx = *(const float4 *)(map_x + (size_t)q * 4), my = *(const float4 *)(map_y + (size_t)q * 4);
    in[0] = inside_source(mx.x, my.x, wmax, hmax), in[1] = inside_source(mx.y, my.y, wmax, hmax);
    in[2] = inside_source(mx.z, my.z, wmax, hmax), in[3] = inside_source(mx.w, my.w, wmax, hmax);
  }
  count_inside(in, n_inside);
}

// BGR -> grey, four source pixels per lane; the grey plane's rows are padded to a multiple of 4 bytes (grey_stride), so every
// lane stores one aligned word; the source width is any number >= 2, so the last lane of a row may hold fewer than 4 pixels
__global__ void __launch_bounds__(64) k_grey_plane(const unsigned char *__restrict__ img, int img_stride_bytes, int sw, int sh,
                                                   unsigned char *__restrict__ grey, int grey_stride) {
  const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
  if (x >= sw || y >= sh) return;
  const unsigned char *ip = img + (size_t)y * img_stride_bytes + (size_t)x * 3;
  unsigned char px[12];
  if (x + 4 <= sw && (((size_t)ip) & 3) == 0) {
    const unsigned *ip4 = (const unsigned *)ip;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned v = ip4[k];
      px[4 * k] = (unsigned char)v, px[4 * k + 1] = (unsigned char)(v >> 8), px[4 * k + 2] = (unsigned char)(v >> 16),
             px[4 * k + 3] = (unsigned char)(v >> 24);
    }
  } else {
    const int nb = 3 * min(4, sw - x);
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k] = k < nb ? ip[k] : (unsigned char)0;
  }
  unsigned out = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int b = px[3 * k], g = px[3 * k + 1], r = px[3 * k + 2];
    out |= (unsigned)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14) << (8 * k);
  }
  *(unsigned *)(grey + (size_t)y * grey_stride + x) = out;
}

// `grey` is a 1 B/px plane: the caller's own image for a 1-channel source, k_grey_plane's output for a BGR one.
// kDepth = false writes the intensity plane alone (the registered ingest, dvo_register.cpp: its depth does not go through the map).
template <bool kDepth>
__global__ void __launch_bounds__(64) k_ingest_remap(const float *__restrict__ map_x, const float *__restrict__ map_y,
                                                     const unsigned char *__restrict__ grey, int grey_stride,
                                                     const unsigned short *__restrict__ raw_z, int z_stride, float z_scale,
                                                     float wmax, float hmax, float *__restrict__ i_plane,
                                                     float *__restrict__ z_plane, int w, int h) {
  const int x4 = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x4 * 4 >= w || y >= h) return;
  const size_t o = (size_t)y * w + (size_t)x4 * 4;
  const float4 mx4 = *(const float4 *)(map_x + o), my4 = *(const float4 *)(map_y + o);
  const float mx[4] = {mx4.x, mx4.y, mx4.z, mx4.w}, my[4] = {my4.x, my4.y, my4.z, my4.w};
  float I[4], Z[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float sx = mx[k], sy = my[k];
    I[k] = 0.0f, Z[k] = __builtin_nanf("");
    if (inside_source(sx, sy, wmax, hmax)) {
      // 0 <= sx < sw - 1 and 0 <= sy < sh - 1 were tested in float: x0 + 1 <= sw - 1, y0 + 1 <= sh - 1, and the nearest tap
      // floorf(s + 0.5f) <= s - 1 + 1 lies in the source as well (sw, sh <= 2^20: the sums are exact to half a pixel)
      const float x0 = floorf(sx), y0 = floorf(sy);
      const float ax = sx - x0, ay = sy - y0;
      const unsigned char *t = grey + (size_t)(int)y0 * grey_stride + (int)x0;
      const float g00 = (float)t[0], g01 = (float)t[1], g10 = (float)t[grey_stride], g11 = (float)t[grey_stride + 1];
      const float top = g00 + ax * (g01 - g00), bot = g10 + ax * (g11 - g10);
      I[k] = top + ay * (bot - top);
      if (kDepth) {
        const float px = floorf(sx + 0.5f), py = floorf(sy + 0.5f);
        const unsigned short zr = raw_z[(size_t)(int)py * z_stride + (int)px];
        if (zr != 0) Z[k] = (float)zr * z_scale;
      }
    }
  }
  *(float4 *)(i_plane + o) = make_float4(I[0], I[1], I[2], I[3]);
  if (kDepth) *(float4 *)(z_plane + o) = make_float4(Z[0], Z[1], Z[2], Z[3]);
}

}  // namespace rectify

namespace host {

namespace {

constexpr int kMaxSourceSide = 1 << 20;  // (float)(s - 1) and s + 0.5f are exact below 2^23; a side this long is no camera's

int check_output_size(const char *entry, int width, int height) {
  if (check_levels(entry, width, height, 1)) return invalid(entry, "the output must be at least 4x2 with a width that is a multiple of 4");
  if ((long long)width * height > (1ll << 30)) return invalid(entry, "the output holds more than 2^30 pixels");
  return DVO_AMD_OK;
}

int check_source_size(const char *entry, int src_width, int src_height) {
  if (src_width < 2 || src_height < 2) return invalid(entry, "the source must be at least 2x2");
  if (src_width > kMaxSourceSide || src_height > kMaxSourceSide) return invalid(entry, "a source side is longer than 2^20 pixels");
  return DVO_AMD_OK;
}

// the remap object with its two planes allocated and the counter cleared (on the prep stream); the caller fills the planes
int remap_alloc(const char *entry, int device, int width, int height, int src_width, int src_height, dvo_amd_remap **out,
                hipStream_t *st) {
  int ndev = 0;
  int rc = have_device(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(entry, "no such device");
  HIP_TRY(hipSetDevice(device));
  rc = device_prep_stream(device, st);
  if (rc) return rc;
  const size_t n = (size_t)width * height, plane = align_up(sizeof(float) * n, 256);
  void *mem = nullptr;
  const hipError_t e = hipMalloc(&mem, 2 * plane + 256);
  if (e == hipErrorOutOfMemory) return DVO_AMD_ERR_OUT_OF_MEMORY;
  if (e != hipSuccess) return fail_hip("hipMalloc (remap)", e);
  dvo_amd_remap *r = new dvo_amd_remap();
  r->device = device, r->w = width, r->h = height, r->sw = src_width, r->sh = src_height;
  r->mem = mem, r->map_x = (float *)mem, r->map_y = (float *)((char *)mem + plane), r->counter = (int *)((char *)mem + 2 * plane);
  const hipError_t em = hipMemsetAsync(r->counter, 0, sizeof(int), *st);
  if (em != hipSuccess) {
    (void)hipFree(mem);
    delete r;
    return fail_hip("remap counter", em);
  }
  *out = r;
  return DVO_AMD_OK;
}

// n_inside to the host and the stream drained; on failure the remap is gone
int remap_finish(dvo_amd_remap *r, hipError_t e, hipStream_t st, dvo_amd_remap **out) {
  if (e == hipSuccess) e = hipMemcpyAsync(&r->n_inside, r->counter, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(r->mem);
    delete r;
    return fail_hip("remap build", e);
  }
  *out = r;
  return DVO_AMD_OK;
}

}  // namespace

// Level 0's base planes from a raw frame in device memory through a remap, enqueued on `st` (ingest_level0 calls this in place of
// launch_ingest); z_plane == nullptr: the intensity plane alone, d_z is not read
int launch_remap_ingest(const dvo_amd_remap *r, const unsigned char *d_img, int channels, int img_stride, unsigned char *grey,
                        int grey_stride, const unsigned short *d_z, int z_stride, float z_scale, float *i_plane, float *z_plane,
                        hipStream_t st) {
  hipError_t e = hipSuccess;
  if (channels == 3) {
    hipLaunchKernelGGL(rectify::k_grey_plane, dim3((unsigned)((grey_stride / 4 + 63) / 64), (unsigned)r->sh), dim3(64), 0, st, d_img,
                       img_stride, r->sw, r->sh, grey, grey_stride);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip("k_grey_plane", e);
    d_img = grey, img_stride = grey_stride;
  }
  const dim3 grid((unsigned)((r->w / 4 + 63) / 64), (unsigned)r->h);
  if (z_plane)
    hipLaunchKernelGGL(rectify::k_ingest_remap<true>, grid, dim3(64), 0, st, r->map_x, r->map_y, d_img, img_stride, d_z, z_stride,
                       z_scale, (float)(r->sw - 1), (float)(r->sh - 1), i_plane, z_plane, r->w, r->h);
  else
    hipLaunchKernelGGL(rectify::k_ingest_remap<false>, grid, dim3(64), 0, st, r->map_x, r->map_y, d_img, img_stride,
                       (const unsigned short *)nullptr, 0, 0.0f, (float)(r->sw - 1), (float)(r->sh - 1), i_plane, (float *)nullptr,
                       r->w, r->h);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip("k_ingest_remap", e);
  return DVO_AMD_OK;
}

}  // namespace host
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;

extern "C" {

int dvo_amd_remap_create(int device, int width, int height, const float *map_x, const float *map_y, int stride, int src_width,
                         int src_height, dvo_amd_remap **out) {
  static const char *entry = "dvo_amd_remap_create";
  if (out) *out = nullptr;
  if (!out || !map_x || !map_y) return invalid(entry, "a NULL pointer");
  int rc = check_output_size(entry, width, height);
  if (!rc) rc = check_source_size(entry, src_width, src_height);
  if (rc) return rc;
  if (stride < width) return invalid(entry, "stride < width");
  dvo_amd_remap *r = nullptr;
  hipStream_t st;
  rc = remap_alloc(entry, device, width, height, src_width, src_height, &r, &st);
  if (rc) return rc;
  const size_t row = sizeof(float) * (size_t)width;
  hipError_t e = hipMemcpy2DAsync(r->map_x, row, map_x, sizeof(float) * (size_t)stride, row, height, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpy2DAsync(r->map_y, row, map_y, sizeof(float) * (size_t)stride, row, height, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const int n = width * height;
    hipLaunchKernelGGL(rectify::k_count_inside, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, (const float *)r->map_x,
                       (const float *)r->map_y, n, (float)(src_width - 1), (float)(src_height - 1), r->counter);
    e = hipGetLastError();
  }
  return remap_finish(r, e, st, out);
}

int dvo_amd_remap_create_undistort(int device, int width, int height, const float k_out[4], int src_width, int src_height,
                                   const float k_src[4], const float dist[5], dvo_amd_remap **out) {
  static const char *entry = "dvo_amd_remap_create_undistort";
  if (out) *out = nullptr;
  if (!out || !k_out || !k_src || !dist) return invalid(entry, "a NULL pointer");
  int rc = check_output_size(entry, width, height);
  if (!rc) rc = check_source_size(entry, src_width, src_height);
  if (rc) return rc;
  if (!finite_all(k_out, 4) || !finite_all(k_src, 4) || !finite_all(dist, 5)) return invalid(entry, "a non-finite intrinsic or coefficient");
  if (!(k_out[0] > 0.0f && k_out[1] > 0.0f && k_src[0] > 0.0f && k_src[1] > 0.0f)) return invalid(entry, "fx and fy of both cameras must be positive");
  dvo_amd_remap *r = nullptr;
  hipStream_t st;
  rc = remap_alloc(entry, device, width, height, src_width, src_height, &r, &st);
  if (rc) return rc;
  rectify::UndistortArgs A;
  A.fx = k_out[0], A.fy = k_out[1], A.ox = k_out[2], A.oy = k_out[3];
  A.fxs = k_src[0], A.fys = k_src[1], A.oxs = k_src[2], A.oys = k_src[3];
  A.k1 = dist[0], A.k2 = dist[1], A.p1 = dist[2], A.p2 = dist[3], A.k3 = dist[4];
  A.two_p1 = 2.0f * dist[2], A.two_p2 = 2.0f * dist[3];
  const int n = width * height;
  hipLaunchKernelGGL(rectify::k_undistort_map, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, A, width, n,
                     (float)(src_width - 1), (float)(src_height - 1), r->map_x, r->map_y, r->counter);
  return remap_finish(r, hipGetLastError(), st, out);
}

void dvo_amd_remap_retain(dvo_amd_remap *r) {
  if (r) r->refs.fetch_add(1);
}

void dvo_amd_remap_release(dvo_amd_remap *r) {
  if (!r) return;
  if (r->refs.fetch_sub(1) != 1) return;
  (void)hipSetDevice(r->device);
  (void)hipFree(r->mem);
  delete r;
}

int dvo_amd_remap_info(const dvo_amd_remap *r, int *width, int *height, int *src_width, int *src_height, int *n_inside) {
  if (!r) return invalid("dvo_amd_remap_info", "the remap is NULL");
  if (width) *width = r->w;
  if (height) *height = r->h;
  if (src_width) *src_width = r->sw;
  if (src_height) *src_height = r->sh;
  if (n_inside) *n_inside = r->n_inside;
  return DVO_AMD_OK;
}

int dvo_amd_remap_download(const dvo_amd_remap *r, float *map_x, float *map_y) {
  if (!r || !map_x || !map_y) return invalid("dvo_amd_remap_download", "a NULL pointer");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st;
  const int rc = device_prep_stream(r->device, &st);
  if (rc) return rc;
  const size_t bytes = sizeof(float) * (size_t)r->w * r->h;
  HIP_TRY(hipMemcpyAsync(map_x, r->map_x, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(map_y, r->map_y, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DVO_AMD_OK;
}

}  // extern "C"
