// Depth-to-colour registration at ingest: what depth_image_proc/register does on the CPU in front of the reference
// (dvo_ros/src/camera_base.cpp:31-33 subscribes to camera/depth_registered/image_rect_raw) as a forward splat of the raw depth
// frame of the depth camera into level 0's depth plane of the colour camera.  The rule is pinned operation by operation in
// include/dvo_amd.h; tests/register_ref.py restates it.
//   hipMemsetD32Async   the depth plane to NaN 0x7FC00000, which as an unsigned word lies above every finite positive float
//   k_register_splat    one lane per depth pixel: scale, back-project, transform, cull, project, footprint; the footprint's
//                       pixels keep the minimum of bits(cz) with one 32-bit unsigned-min atomic each.  Every kept cz is > 0, so
//                       its bit pattern orders like its value: the plane holds the nearest depth itself and needs no resolve.
//   k_register_count    the pixels of the plane that something covered
// The minimum does not depend on the order the atomics land in and the words only decrease: the plane and the counters are a
// function of the frame and the registration alone.
#include "dvo_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dvo_amd {
namespace registration {

constexpr int kBlock = 256;
constexpr unsigned kEmptyWord = 0x7FC00000u;
constexpr int kMaxBlocks = 256;     // of k_register_splat (a quarter of it for k_register_count): see register_level0
constexpr int kSmallFootprint = 4;  // pixels a lane splats by itself; larger footprints are walked by the whole wave

struct View {
  int w, h;
  float fx, fy, ox, oy;
};

struct Ctrl {
  unsigned long long behind, outside, drawn, covered;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one axis of the footprint (dvo_amd.h: rule 5 of the registration, which is rule 5 of dvo_amd_map_render), compared in float
// before any conversion to int; false: no pixel of the axis is covered
__device__ __forceinline__ bool footprint_axis(float c, float half, bool fill, int size, int &lo, int &hi) {
  float a = ceilf(c - half), b = floorf(c + half);
  if (!fill || b < a) a = b = floorf(c + 0.5f);
  const float last = (float)(size - 1);
  if (!(b >= 0.0f && a <= last)) return false;
  lo = a > 0.0f ? (int)a : 0;
  hi = b < last ? (int)b : size - 1;
  return true;
}

// the stale value a plain load may return is never smaller than the word in memory: skipping the atomic on it is exact
__device__ __forceinline__ void depth_min(unsigned *z, unsigned word) {
  if (*z > word) atomicMin(z, word);
}

__global__ void __launch_bounds__(kBlock) k_register_splat(const unsigned short *__restrict__ raw_z, int z_stride, float z_scale,
                                                           Registration R, View V, unsigned *zbuf, Ctrl *ctrl) {
  const int lane = threadIdx.x & 63;
  unsigned behind = 0, outside = 0, drawn = 0;
  // both loops are uniform over the block: no lane leaves before the ballots
  for (int v = blockIdx.y; v < R.dh; v += gridDim.y) {
    const float ry = ((float)v - R.oyd) / R.fyd;
    for (int ub = blockIdx.x * kBlock; ub < R.dw; ub += gridDim.x * kBlock) {
      const int u = ub + threadIdx.x;
      int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
      unsigned word = kEmptyWord;
      bool draw = false;
      const unsigned short d = u < R.dw ? raw_z[(size_t)v * z_stride + u] : (unsigned short)0;
      if (d != 0) {
        const float z = (float)d * z_scale;
        const float rx = ((float)u - R.oxd) / R.fxd;
        const float X = rx * z, Y = ry * z;
        const float *T = R.T;
        const float cx = ((T[0] * X + T[1] * Y) + T[2] * z) + T[3];
        const float cy = ((T[4] * X + T[5] * Y) + T[6] * z) + T[7];
        const float cz = ((T[8] * X + T[9] * Y) + T[10] * z) + T[11];
        if (!(cz > R.min_z)) {
          ++behind;
        } else {
          const float uc = (cx * V.fx) / cz + V.ox, vc = (cy * V.fy) / cz + V.oy;
          const float s = z / cz;
          const float hx = fminf(0.5f * (R.mx * s), 4.0f), hy = fminf(0.5f * (R.my * s), 4.0f);
          const bool in_x = footprint_axis(uc, hx, R.fill != 0, V.w, x0, x1), in_y = footprint_axis(vc, hy, R.fill != 0, V.h, y0, y1);
          draw = in_x && in_y;
          if (draw) ++drawn, word = __float_as_uint(cz);
          else ++outside;
        }
      }
      const int fw = draw ? x1 - x0 + 1 : 0, fh = draw ? y1 - y0 + 1 : 0;  // (each at most 9: the 4.0 cap)
      const bool some = fw > 0 && fh > 0;
      const bool small = some && fw * fh <= kSmallFootprint;
      if (small)
        for (int yy = y0; yy <= y1; ++yy)
          for (int xx = x0; xx <= x1; ++xx) depth_min(zbuf + (size_t)yy * V.w + xx, word);
      // the larger footprints of the wave, one after the other: a lane per pixel along the rows
      unsigned long long todo = __ballot(some && !small);
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sfw = __shfl(fw, src, 64), sfh = __shfl(fh, src, 64);
        const unsigned sword = __shfl(word, src, 64);
        const int npx = sfw * sfh;  // (at most 81)
        for (int p = lane; p < npx; p += 64) {
          const int row = p / sfw, col = p - row * sfw;
          depth_min(zbuf + (size_t)(sy0 + row) * V.w + (sx0 + col), sword);
        }
      }
    }
  }
  const unsigned long long b = wave_sum(behind), o = wave_sum(outside), dr = wave_sum(drawn);
  if (lane == 0) {
    if (b) atomicAdd(&ctrl->behind, b);
    if (o) atomicAdd(&ctrl->outside, o);
    if (dr) atomicAdd(&ctrl->drawn, dr);
  }
}

// four pixels per lane (a level's pixel count is a multiple of 4)
__global__ void __launch_bounds__(kBlock) k_register_count(const uint4 *__restrict__ zbuf, unsigned long long n4, Ctrl *ctrl) {
  unsigned covered = 0;
  for (unsigned long long p = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; p < n4; p += (unsigned long long)gridDim.x * kBlock) {
    const uint4 q = zbuf[p];
    covered += (q.x != kEmptyWord) + (q.y != kEmptyWord) + (q.z != kEmptyWord) + (q.w != kEmptyWord);
  }
  const unsigned long long c = wave_sum(covered);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctrl->covered, c);
}

}  // namespace registration

namespace host {

namespace {

constexpr int kMaxDepthSide = 1 << 20;  // (float)u is exact far beyond it; a side this long is no camera's

int invalid(const char *entry, const std::string &why) {
  g_last_error = std::string(entry) + ": " + why;
  return DVO_AMD_ERR_INVALID_ARGUMENT;
}

bool finite_all(const float *v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

// Level 0's two base planes of a registered frame (pyramid_build calls this in place of launch_ingest): the intensity plane as
// the plain or the remapped ingest writes it, the depth plane by the registration rule.  `ctrl` is device memory of the
// pyramid's own (4 words: behind, outside, drawn, covered).  Everything is enqueued on `st`, the device's prep stream, with the
// device's mutex held from the first upload to the last launch, as in rectify_level0.
int register_level0(int device, const RawFrame &raw, bool on_device, float *i_plane, float *z_plane, int width, int height,
                    float fx, float fy, float ox, float oy, unsigned long long *ctrl, hipStream_t st) {
  const Registration &R = *raw.reg;
  std::lock_guard<std::mutex> lk(device_mutex(device));
  Staging &S = staging(device);
  hipError_t e = hipSuccess;
  if (raw.remap) {
    const int rc = rectify_level0_locked(device, raw, on_device, i_plane, nullptr, st);
    if (rc) return rc;
  } else {
    const unsigned char *d_img = raw.image;
    int img_stride = raw.image_stride_bytes;
    if (!on_device) {
      const size_t row_img = (size_t)width * raw.channels;
      const int rc = staging_grow(&S.img, &S.img_bytes, row_img * height);
      if (rc) return rc;
      e = hipMemcpy2DAsync(S.img, row_img, raw.image, (size_t)raw.image_stride_bytes, row_img, height, hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return fail_hip("raw image upload", e);
      d_img = (const unsigned char *)S.img, img_stride = (int)row_img;
    }
    e = launch_ingest_intensity(d_img, raw.channels, img_stride, i_plane, width, height, st);
    if (e != hipSuccess) return fail_hip("k_ingest", e);
  }
  const unsigned short *d_z = raw.depth;
  int z_stride = raw.depth_stride;
  if (!on_device) {
    const size_t row_z = sizeof(unsigned short) * (size_t)R.dw;
    const int rc = staging_grow(&S.z, &S.z_bytes, row_z * R.dh);
    if (rc) return rc;
    e = hipMemcpy2DAsync(S.z, row_z, raw.depth, sizeof(unsigned short) * (size_t)raw.depth_stride, row_z, R.dh, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail_hip("raw depth upload", e);
    d_z = (const unsigned short *)S.z, z_stride = R.dw;
  }
  const size_t n = (size_t)width * height;
  e = hipMemsetD32Async((hipDeviceptr_t)z_plane, (int)registration::kEmptyWord, n, st);
  if (e == hipSuccess) e = hipMemsetAsync(ctrl, 0, sizeof(registration::Ctrl), st);
  if (e != hipSuccess) return fail_hip("registration clear", e);
  const registration::View V{width, height, fx, fy, ox, oy};
  // About one block per compute unit, and the kernel strides over the rest: every wave ends with up to three atomic adds on one
  // cache line, which the memory side serialises at about 12 ns each (measured: a block per 256 pixels, 4800 waves at 640x480,
  // spent 61 us in the splat).
  const unsigned gx = (unsigned)std::min(registration::kMaxBlocks, (R.dw + registration::kBlock - 1) / registration::kBlock);
  const unsigned gy = (unsigned)std::min<long long>(R.dh, std::max(1u, (unsigned)registration::kMaxBlocks / gx));
  hipLaunchKernelGGL(registration::k_register_splat, dim3(gx, gy), dim3(registration::kBlock), 0, st, d_z, z_stride, raw.depth_scale, R, V,
                     (unsigned *)z_plane, (registration::Ctrl *)ctrl);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip("k_register_splat", e);
  const unsigned long long n4 = n / 4;
  const unsigned gc = (unsigned)std::min<unsigned long long>(registration::kMaxBlocks / 4, std::max<unsigned long long>(1, (n4 + registration::kBlock - 1) / registration::kBlock));
  hipLaunchKernelGGL(registration::k_register_count, dim3(gc), dim3(registration::kBlock), 0, st, (const uint4 *)z_plane, n4, (registration::Ctrl *)ctrl);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip("k_register_count", e);
  return DVO_AMD_OK;
}

}  // namespace host
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;

extern "C" {

void dvo_amd_default_registration(dvo_amd_registration *reg) {
  if (!reg) return;
  std::memset(reg, 0, sizeof(*reg));
  reg->T[0] = reg->T[5] = reg->T[10] = reg->T[15] = 1.0;
}

int dvo_amd_pyramid_create_raw_registered(int device, const unsigned char *image, int channels, int image_stride_bytes,
                                          const unsigned short *depth, int depth_stride, float depth_scale, int on_device,
                                          const dvo_amd_registration *reg, const dvo_amd_remap *remap, int width, int height,
                                          float fx, float fy, float ox, float oy, int levels, double timestamp,
                                          dvo_amd_pyramid **out, dvo_amd_registration_stats *stats) {
  static const char *entry = "dvo_amd_pyramid_create_raw_registered";
  if (out) *out = nullptr;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!out || !image || !depth || !reg) return invalid(entry, "a NULL pointer");
  if (channels != 1 && channels != 3) return invalid(entry, "channels must be 1 or 3");
  if (!(depth_scale > 0.0f)) return invalid(entry, "depth_scale must be > 0");
  if (reg->depth_width < 1 || reg->depth_height < 1 || reg->depth_width > kMaxDepthSide || reg->depth_height > kMaxDepthSide)
    return invalid(entry, "a side of the depth frame is outside 1..2^20");
  if (depth_stride < reg->depth_width) return invalid(entry, "depth_stride < depth_width");
  const float k[4] = {fx, fy, ox, oy};
  float T[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[4 * r + c] = (float)reg->T[4 * c + r];  // column-major double -> row-major float
  if (!finite_all(reg->k_depth, 4) || !finite_all(T, 12) || !finite_all(k, 4))
    return invalid(entry, "a non-finite intrinsic or entry of the transform");
  if (!(reg->k_depth[0] > 0.0f && reg->k_depth[1] > 0.0f && fx > 0.0f && fy > 0.0f))
    return invalid(entry, "fx and fy of both cameras must be positive");
  if (!(reg->min_z >= 0.0f) || !std::isfinite(reg->min_z)) return invalid(entry, "min_z must be finite and >= 0");
  if (reg->fill != 0 && reg->fill != 1) return invalid(entry, "fill must be 0 or 1");
  if (remap && (remap->w != width || remap->h != height)) return invalid(entry, "the remap's output size differs from width x height");
  const int image_width = remap ? remap->sw : width;
  if ((long long)image_stride_bytes < (long long)image_width * channels)
    return invalid(entry, "the image stride is smaller than the row it must hold");
  if (levels < 1 || levels > DVO_AMD_MAX_LEVELS) return invalid(entry, "levels must be 1.." + std::to_string(DVO_AMD_MAX_LEVELS));
  if ((long long)width * height > (1ll << 30)) return invalid(entry, "the pyramid's level 0 holds more than 2^30 pixels");
  for (int l = 0, w = width, h = height; l < levels; ++l, w /= 2, h /= 2)
    if (w < 4 || h < 2 || (w % 4) != 0)
      return invalid(entry, "level " + std::to_string(l) + " would not be at least 4x2 with a width that is a multiple of 4");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DVO_AMD_ERR_NO_DEVICE;
  if (remap && remap->device != device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  unsigned long long counts[4] = {0, 0, 0, 0};
  Registration R;
  R.dw = reg->depth_width, R.dh = reg->depth_height;
  R.fxd = reg->k_depth[0], R.fyd = reg->k_depth[1], R.oxd = reg->k_depth[2], R.oyd = reg->k_depth[3];
  std::memcpy(R.T, T, sizeof(T));
  R.min_z = reg->min_z, R.mx = fx / R.fxd, R.my = fy / R.fyd, R.fill = reg->fill, R.counts = counts;
  RawFrame raw{image, channels, image_stride_bytes, depth, depth_stride, depth_scale, remap, &R};
  const int rc = pyramid_build(device, nullptr, nullptr, &raw, on_device != 0, width, height, width, fx, fy, ox, oy, levels,
                               timestamp, out);
  if (rc == DVO_AMD_OK && stats) {
    stats->behind = (long long)counts[0], stats->outside = (long long)counts[1], stats->drawn = (long long)counts[2];
    stats->measurements = stats->behind + stats->outside + stats->drawn;
    stats->covered_pixels = (long long)counts[3];
  }
  return rc;
}

}  // extern "C"
