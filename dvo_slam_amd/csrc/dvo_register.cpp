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
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dvo_amd {
namespace registration {

constexpr int kBlock = 256;
constexpr unsigned kEmptyWord = 0x7FC00000u;
constexpr int kMaxBlocks = 256;     // of k_register_splat (a quarter of it for k_register_count): see launch_register_depth
constexpr int kSmallFootprint = 4;  // pixels a lane splats by itself; larger footprints are walked by the whole wave

struct View {
  int w, h;
  float fx, fy, ox, oy;
};

struct Ctrl {
  unsigned long long behind, outside, drawn, covered;
};

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
          const int mode = R.fill != 0 ? rules::kFootprintFill : rules::kFootprintNearest;
          const bool in_x = rules::footprint_axis(uc, hx, mode, V.w, x0, x1), in_y = rules::footprint_axis(vc, hy, mode, V.h, y0, y1);
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
          for (int xx = x0; xx <= x1; ++xx) rules::depth_min(zbuf + (size_t)yy * V.w + xx, word);
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
          rules::depth_min(zbuf + (size_t)(sy0 + row) * V.w + (sx0 + col), sword);
        }
      }
    }
  }
  const unsigned long long b = rules::wave_sum((unsigned long long)behind), o = rules::wave_sum((unsigned long long)outside),
                           dr = rules::wave_sum((unsigned long long)drawn);
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
  const unsigned long long c = rules::wave_sum((unsigned long long)covered);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctrl->covered, c);
}

}  // namespace registration

namespace host {

// Level 0's depth plane of a registered frame from raw depth in device memory, enqueued on `st` (ingest_level0 calls this after the
// intensity plane is on its way).  `ctrl` is device memory of the pyramid's own (4 words: behind, outside, drawn, covered).
int launch_register_depth(const Registration &R, const unsigned short *d_z, int z_stride, float z_scale, float *z_plane,
                          const PyramidSpec &view, unsigned long long *ctrl, hipStream_t st) {
  const size_t n = (size_t)view.width * view.height;
  hipError_t e = hipMemsetD32Async((hipDeviceptr_t)z_plane, (int)registration::kEmptyWord, n, st);
  if (e == hipSuccess) e = hipMemsetAsync(ctrl, 0, sizeof(registration::Ctrl), st);
  if (e != hipSuccess) return fail_hip("registration clear", e);
  const registration::View V{view.width, view.height, view.fx, view.fy, view.ox, view.oy};
  // About one block per compute unit, and the kernel strides over the rest: every wave ends with up to three atomic adds on one
  // cache line, which the memory side serialises at about 12 ns each (measured: a block per 256 pixels, 4800 waves at 640x480,
  // spent 61 us in the splat).
  const unsigned gx = (unsigned)std::min(registration::kMaxBlocks, (R.dw + registration::kBlock - 1) / registration::kBlock);
  const unsigned gy = (unsigned)std::min<long long>(R.dh, std::max(1u, (unsigned)registration::kMaxBlocks / gx));
  hipLaunchKernelGGL(registration::k_register_splat, dim3(gx, gy), dim3(registration::kBlock), 0, st, d_z, z_stride, z_scale, R, V,
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

}  // extern "C"
