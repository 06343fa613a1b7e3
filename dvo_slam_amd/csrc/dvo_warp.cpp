// A frame resampled into another camera's pixels, on the device: RgbdImage::warpIntensity / warpIntensitySse (inverse: a gather
// over the fixed frame's pixels) and warpIntensityForward / warpDepthForward / warpDepthForwardAdvanced (forward: a scatter of
// the moving frame's pixels), rgbd_image.cpp:545-781.  The plane entries hand host planes back, the pyramid entries hand the
// result to the ordinary builder: the output is an ordinary pyramid.  The rules are pinned in include/dvo_amd.h ("Frame
// warps"); tests/warp_ref.py restates them in numpy.
//
//   k_warp_inverse   ONE launch over all pairs of a call: blockIdx.y walks the pair records, striding by gridDim.y, blockIdx.x
//                    a chunk of the fixed level.  A lane owns four consecutive fixed pixels of one row (widths are multiples
//                    of 4): one float4 depth load, the point, the projection, then the four taps of the moving level as
//                    data-dependent gathers.  A tap reads the grey value and the depth with ONE 8-byte load from the level's
//                    interleaved gather layout {I, Z, Ix, Iy}, whose first two words are the bits of the two base planes.
//                    One float4 store per requested plane.
//   k_warp_clear     the 64-bit depth buffers of all items of a call (they lie next to each other) to all ones
//   k_warp_splat     ONE launch over all items: a lane owns one moving pixel; point, transformation, cull, projection,
//                    footprint; every covered pixel keeps the minimum of (bits(cz) << 32) | r with one 64-bit unsigned-min
//                    atomic.  Footprints of up to four pixels are drawn by their lane, larger ones by the whole wave.
//   k_warp_resolve   ONE launch over all items: a lane owns one pixel of the view: the winner's depth, its grey value and index
// Counts: ballots and popcounts per wave, LDS per block, one integer atomicAdd per non-zero count -- integers and 64-bit minima
// only, so nothing depends on the launch geometry or on the order atomics land in.  Everything runs on the device's prep stream
// with scratch from the slab pool and one synchronisation per call; the pyramid forms then run pyramid_build per item.
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>

namespace dvo_amd {
namespace warp {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLanePixels = 4;                // inverse: pixels per lane
constexpr int kChunk = kBlock * kLanePixels;  // ... and per block
constexpr int kInvCounts = DVO_AMD_WARP_INVERSE_COUNTS;  // valid, behind, outside, border, hidden, warped, partial, no_depth
constexpr int kFwdCounts = DVO_AMD_WARP_FORWARD_COUNTS;  // valid, behind, outside, too_large, drawn, covered_pixels, no_depth
constexpr unsigned kNaN = 0x7FC00000u;
constexpr unsigned long long kEmptyWord = ~0ull;
constexpr int kSmallFootprint = 4;  // pixels a lane splats by itself; larger footprints are walked by the whole wave
static_assert(kInvCounts == 8 && kFwdCounts == 7, "the records of include/dvo_amd.h");

// ---- inverse

// one pair as the kernel reads it (block-uniform)
struct InverseRecord {
  const float *zf, *txf, *tyf;  // fixed: depth plane and rays of the level
  const float4 *cam;            // moving: {I, Z, Ix, Iy} per pixel of the level
  float *i_out, *z_out;         // the planes on the fixed level's pixels (either may be null)
  unsigned *counts;             // [kInvCounts]
  int wf, nf;                   // fixed: width, pixels
  int wm, hm;                   // moving: size
  float fx, fy, ox, oy;         // moving: intrinsics
  float M[12];                  // rows 0..2 of fixed camera -> moving camera, row-major
};

__global__ void __launch_bounds__(kBlock) k_warp_inverse(const InverseRecord *__restrict__ records, int n_records, float near_z,
                                                         float margin, int depth_fixed, int empty_all, float fill) {
  __shared__ unsigned s_cnt[kWaves][kInvCounts];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float nan = __uint_as_float(kNaN);
  for (int rec = blockIdx.y; rec < n_records; rec += gridDim.y) {
    const InverseRecord R = records[rec];        // uniform over the block
    if (blockIdx.x * kChunk >= R.nf) continue;   // (block-uniform: no barrier is skipped by part of a block)
    const float wm = (float)R.wm, hm = (float)R.hm;
    const int p0 = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
    const bool live = p0 < R.nf;  // (nf is a multiple of 4: four pixels or none, all in one row)
    float z4[kLanePixels] = {0.f, 0.f, 0.f, 0.f};
    int u0 = 0;
    float ty = 0.f;
    if (live) {
      const float4 z = *(const float4 *)(R.zf + p0);
      z4[0] = z.x, z4[1] = z.y, z4[2] = z.z, z4[3] = z.w;
      const int v = p0 / R.wf;
      u0 = p0 - v * R.wf;
      ty = R.tyf[v];
    }
    unsigned cnt[kInvCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    float io[kLanePixels], zo[kLanePixels];
#pragma unroll
    for (int k = 0; k < kLanePixels; ++k) {
      int cls = -1;  // -1: no pixel; 7 no depth; else the index of the outcome's count (1 behind .. 5 warped)
      bool partial = false;
      float iv = nan, zv = nan;
      if (live) {
        const float z = z4[k];
        cls = 7;
        if (rules::finite_f(z)) {
          float qx, qy, qz;
          rules::transform_rows(R.M, R.txf[u0 + k] * z, ty * z, z, qx, qy, qz);
          if (!(qz >= near_z)) {
            cls = 1;
          } else {
            const float px = (qx * R.fx) / qz + R.ox, py = (qy * R.fy) / qz + R.oy;
            if (!(px >= 0.0f && px < wm && py >= 0.0f && py < hm)) {
              cls = 2;
            } else {
              zv = depth_fixed ? z : qz;
              const float x0 = floorf(px), y0 = floorf(py);
              if (x0 + 1.0f >= wm || y0 + 1.0f >= hm) {
                cls = 3;
              } else {
                const float a = px - x0, b = py - y0, wa = 1.0f - a, wb = 1.0f - b;
                // 0 <= x0 <= wm-2, 0 <= y0 <= hm-2: tested in float above
                const size_t at = (size_t)(int)y0 * (size_t)R.wm + (size_t)(int)x0;
                const float2 t00 = *(const float2 *)(R.cam + at), t01 = *(const float2 *)(R.cam + at + 1);
                const float2 t10 = *(const float2 *)(R.cam + at + (size_t)R.wm), t11 = *(const float2 *)(R.cam + at + (size_t)R.wm + 1);
                const float thr = qz - margin;
                float val = 0.0f, sum = 0.0f;
                int taps = 0;
                auto tap = [&](const float2 t, float w) {
                  if (rules::finite_f(t.y) && t.y > thr) {
                    val = val + w * t.x;
                    sum = sum + w;
                    ++taps;
                  }
                };
                tap(t00, wa * wb), tap(t01, a * wb), tap(t10, wa * b), tap(t11, a * b);
                if (sum > 0.0f) {
                  cls = 5;
                  iv = val / sum;
                  partial = taps < 4;
                } else {
                  cls = 4;
                }
              }
            }
          }
        }
      }
      if (empty_all) {  // the pyramid form: a pixel that is not warped is empty in both planes
        if (cls != 5) iv = fill, zv = nan;
      }
      io[k] = iv, zo[k] = zv;
      cnt[0] += (unsigned)__popcll(__ballot(cls >= 1 && cls <= 5));
#pragma unroll
      for (int c = 1; c <= 5; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
      cnt[6] += (unsigned)__popcll(__ballot(partial));
      cnt[7] += (unsigned)__popcll(__ballot(cls == 7));
    }
    if (live) {
      if (R.i_out) *(float4 *)(R.i_out + p0) = make_float4(io[0], io[1], io[2], io[3]);
      if (R.z_out) *(float4 *)(R.z_out + p0) = make_float4(zo[0], zo[1], zo[2], zo[3]);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kInvCounts; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < kInvCounts) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
      if (sum) atomicAdd(R.counts + threadIdx.x, sum);
    }
    __syncthreads();  // s_cnt is written again for the block's next record
  }
}

// ---- forward

// one item as the kernels read it (block-uniform)
struct ForwardRecord {
  const float *z, *i, *tx, *ty;  // moving: depth and intensity planes and rays of the level
  unsigned long long *zbuf;      // the view's depth buffer
  float *z_out, *i_out;          // the view's planes (any may be null)
  int *idx_out;
  unsigned *counts;              // [kFwdCounts]
  int w, n;                      // moving: width, pixels
  int vw, vh, vn;                // the view: size, pixels
  float fx, fy, ox, oy, near_z;  // the view
  float fxm, fym;                // moving: focal lengths of the level
  float T[12];                   // rows 0..2 of moving camera -> fixed camera, row-major
};

__global__ void __launch_bounds__(kBlock) k_warp_clear(ulonglong2 *z, unsigned long long n2) {
  for (unsigned long long p = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; p < n2; p += (unsigned long long)gridDim.x * kBlock)
    z[p] = make_ulonglong2(kEmptyWord, kEmptyWord);
}

static_assert(DVO_AMD_WARP_SPLAT_NEAREST == rules::kFootprintNearest && DVO_AMD_WARP_SPLAT_FLOOR == rules::kFootprintFloor &&
                  DVO_AMD_WARP_SPLAT_FOOTPRINT == rules::kFootprintFill,
              "the splat modes of include/dvo_amd.h are the footprint modes of dvo_device_rules.h");

__global__ void __launch_bounds__(kBlock) k_warp_splat(const ForwardRecord *__restrict__ records, int n_records, int splat) {
  __shared__ unsigned s_cnt[kWaves][kFwdCounts];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rec = blockIdx.y; rec < n_records; rec += gridDim.y) {
    const ForwardRecord R = records[rec];        // uniform over the block
    if (blockIdx.x * kBlock >= R.n) continue;    // (block-uniform)
    const int r = blockIdx.x * kBlock + threadIdx.x;
    int cls = -1;  // -1: no pixel; 6 no depth; 1 behind, 2 outside, 3 too large, 4 drawn
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    unsigned long long word = kEmptyWord;
    if (r < R.n) {
      const float z = R.z[r];
      cls = 6;
      if (rules::finite_f(z)) {
        const int v = r / R.w, u = r - v * R.w;
        float cx, cy, cz;
        rules::transform_rows(R.T, R.tx[u] * z, R.ty[v] * z, z, cx, cy, cz);
        if (!(cz >= R.near_z)) {
          cls = 1;
        } else {
          const float pu = (cx * R.fx) / cz + R.ox, pv = (cy * R.fy) / cz + R.oy;
          const float hx = 0.5f * (((z / R.fxm) * R.fx) / cz), hy = 0.5f * (((z / R.fym) * R.fy) / cz);
          float a0, a1, b0, b1;
          // (the span of either axis first: a footprint that is too large is counted before one that is outside)
          rules::footprint_span(pu, hx, splat, a0, a1);
          rules::footprint_span(pv, hy, splat, b0, b1);
          const float wlast = (float)(R.vw - 1), hlast = (float)(R.vh - 1);
          if (a1 - a0 > (float)(DVO_AMD_WARP_MAX_FOOTPRINT - 1) || b1 - b0 > (float)(DVO_AMD_WARP_MAX_FOOTPRINT - 1)) {
            cls = 3;
          } else if (!(a1 >= 0.0f && a0 <= wlast && b1 >= 0.0f && b0 <= hlast)) {
            cls = 2;
          } else {
            cls = 4;
            x0 = a0 > 0.0f ? (int)a0 : 0, x1 = a1 < wlast ? (int)a1 : R.vw - 1;
            y0 = b0 > 0.0f ? (int)b0 : 0, y1 = b1 < hlast ? (int)b1 : R.vh - 1;
            word = ((unsigned long long)__float_as_uint(cz) << 32) | (unsigned)r;
          }
        }
      }
    }
    const bool draw = cls == 4;
    const int fw = draw ? x1 - x0 + 1 : 0, fh = draw ? y1 - y0 + 1 : 0;  // (each at most 16)
    const bool some = fw > 0 && fh > 0;
    const bool small = some && fw * fh <= kSmallFootprint;
    if (small)
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) rules::depth_min(R.zbuf + (size_t)yy * R.vw + xx, word);
    // the larger footprints of the wave, one after the other: a lane per pixel along the rows
    unsigned long long todo = __ballot(some && !small);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sfw = __shfl(fw, src, 64), sfh = __shfl(fh, src, 64);
      const unsigned wlo = __shfl((unsigned)word, src, 64), whi = __shfl((unsigned)(word >> 32), src, 64);
      const unsigned long long sword = ((unsigned long long)whi << 32) | wlo;
      const int npx = sfw * sfh;  // (at most 256)
      for (int p = lane; p < npx; p += 64) {
        const int row = p / sfw, col = p - row * sfw;
        rules::depth_min(R.zbuf + (size_t)(sy0 + row) * R.vw + (sx0 + col), sword);
      }
    }
    unsigned cnt[kFwdCounts];
    cnt[0] = (unsigned)__popcll(__ballot(cls >= 1 && cls <= 4));
#pragma unroll
    for (int c = 1; c <= 4; ++c) cnt[c] = (unsigned)__popcll(__ballot(cls == c));
    cnt[5] = 0u;  // (covered_pixels: k_warp_resolve)
    cnt[6] = (unsigned)__popcll(__ballot(cls == 6));
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kFwdCounts; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < kFwdCounts) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
      if (sum) atomicAdd(R.counts + threadIdx.x, sum);
    }
    __syncthreads();  // s_cnt is written again for the block's next record
  }
}

__global__ void __launch_bounds__(kBlock) k_warp_resolve(const ForwardRecord *__restrict__ records, int n_records, float empty_intensity) {
  __shared__ unsigned s_cnt[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rec = blockIdx.y; rec < n_records; rec += gridDim.y) {
    const ForwardRecord R = records[rec];         // uniform over the block
    if (blockIdx.x * kBlock >= R.vn) continue;    // (block-uniform)
    const int p = blockIdx.x * kBlock + threadIdx.x;
    bool covered = false;
    if (p < R.vn) {
      const unsigned long long w = R.zbuf[p];
      const unsigned r = (unsigned)w;
      float d = __uint_as_float(kNaN), g = empty_intensity;
      int at = -1;
      if (w != kEmptyWord && r < (unsigned)R.n) {  // (r < n always: the indices k_warp_splat wrote)
        d = __uint_as_float((unsigned)(w >> 32));
        g = R.i[r];
        at = (int)r;
        covered = true;
      }
      if (R.z_out) R.z_out[p] = d;
      if (R.i_out) R.i_out[p] = g;
      if (R.idx_out) R.idx_out[p] = at;
    }
    const unsigned c = (unsigned)__popcll(__ballot(covered));
    if (lane == 0) s_cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_cnt[w];
      if (sum) atomicAdd(R.counts + 5, sum);
    }
    __syncthreads();  // s_cnt is written again for the block's next record
  }
}

}  // namespace warp
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::warp;

namespace {

// dvo_amd_debug_warp_timing: what the last call on the device launched and waited for (the warp's own kernels and its own
// synchronisation, not pyramid_build's), and (when asked for) two events around its launches on the prep stream
DeviceTiming g_timing[kMaxDevices];

int check_options(const char *entry, const dvo_amd_warp_options *opt) {
  if (!std::isfinite(opt->near_z) || !(opt->near_z > 0.0f)) return invalid(entry, "near_z must be finite and positive");
  if (!(opt->occlusion_margin >= 0.0f)) return invalid(entry, "occlusion_margin must be >= 0 (+inf: no depth-buffer test)");
  if (opt->depth != DVO_AMD_WARP_DEPTH_TRANSFORMED && opt->depth != DVO_AMD_WARP_DEPTH_FIXED)
    return invalid(entry, "depth must be DVO_AMD_WARP_DEPTH_TRANSFORMED or DVO_AMD_WARP_DEPTH_FIXED");
  if (opt->splat != DVO_AMD_WARP_SPLAT_NEAREST && opt->splat != DVO_AMD_WARP_SPLAT_FLOOR && opt->splat != DVO_AMD_WARP_SPLAT_FOOTPRINT)
    return invalid(entry, "splat must be DVO_AMD_WARP_SPLAT_NEAREST, _FLOOR or _FOOTPRINT");
  if (!std::isfinite(opt->fill_intensity)) return invalid(entry, "fill_intensity must be finite");
  return DVO_AMD_OK;
}

// dvo_amd_map_render's checks of a view, without the one that needs a map's leaf size
int check_view(const char *entry, const std::string &item, const dvo_amd_view *v) {
  if (v->width < 1 || v->height < 1 || (long long)v->width * v->height > (1ll << 26))
    return invalid(entry, item + ": the view's width and height must be >= 1 and width*height <= 2^26");
  if (!(std::isfinite(v->fx) && v->fx > 0.0f && std::isfinite(v->fy) && v->fy > 0.0f))
    return invalid(entry, item + ": the view's fx and fy must be finite and positive");
  if (!std::isfinite(v->ox) || !std::isfinite(v->oy)) return invalid(entry, item + ": the view's ox and oy must be finite");
  if (!std::isfinite(v->near_z) || !(v->near_z > 0.0f)) return invalid(entry, item + ": the view's near_z must be finite and positive");
  return DVO_AMD_OK;
}

void release_all(dvo_amd_pyramid **out, int n) {
  for (int k = 0; k < n; ++k)
    if (out[k]) dvo_amd_pyramid_release(out[k]), out[k] = nullptr;
}

// level < 0: the pyramid form (level 0, `out` receives n pyramids); else the plane form (host planes, any may be null)
int inverse_many(const char *entry, int n, const dvo_amd_pyramid *const *fixed, const dvo_amd_pyramid *const *moving, const double *T,
                 int level, const dvo_amd_warp_options *opt, float *const *intensity_out, float *const *depth_out,
                 dvo_amd_pyramid **out, long long *counts) {
  const bool as_pyramid = level < 0;
  if (as_pyramid && out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative count");
  if (!fixed || !moving || !T || !opt || (as_pyramid && !out)) return invalid(entry, "a NULL pointer");
  const int lv = as_pyramid ? 0 : level;
  for (int k = 0; k < n; ++k) {
    const std::string pair = "pair " + std::to_string(k);
    if (!fixed[k] || !moving[k]) return invalid(entry, pair + ": a NULL pyramid");
    if (lv >= fixed[k]->n_levels || lv >= moving[k]->n_levels)
      return invalid(entry, pair + ": level " + std::to_string(lv) + " is beyond a pyramid of " +
                                std::to_string(std::min(fixed[k]->n_levels, moving[k]->n_levels)) + " levels");
    if (!finite_all(T + 16 * (size_t)k, 16)) return invalid(entry, pair + ": the transformation has a non-finite entry");
  }
  int rc = check_options(entry, opt);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    if (fixed[k]->device != fixed[0]->device || moving[k]->device != fixed[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  const int device = fixed[0]->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  // the call's scratch: the record table, the counts, then the planes anybody wants
  const size_t table_bytes = align_up(sizeof(InverseRecord) * (size_t)n, 256);
  const size_t count_bytes = align_up(sizeof(unsigned) * kInvCounts * (size_t)n, 256);
  std::vector<size_t> i_at((size_t)n, 0), z_at((size_t)n, 0);
  std::vector<char> want_i((size_t)n, 0), want_z((size_t)n, 0);
  size_t scratch_bytes = table_bytes + count_bytes;
  int max_n = 1;
  for (int k = 0; k < n; ++k) {
    const size_t plane = align_up(sizeof(float) * (size_t)fixed[k]->lv[lv].n, 256);
    want_i[(size_t)k] = as_pyramid || (intensity_out && intensity_out[k]);
    want_z[(size_t)k] = as_pyramid || (depth_out && depth_out[k]);
    if (want_i[(size_t)k]) i_at[(size_t)k] = scratch_bytes, scratch_bytes += plane;
    if (want_z[(size_t)k]) z_at[(size_t)k] = scratch_bytes, scratch_bytes += plane;
    max_n = std::max(max_n, fixed[k]->lv[lv].n);
  }
  Scratch S;  // (every return below stands behind a synchronisation of the stream)
  rc = S.take(device, scratch_bytes);
  if (rc) return rc;
  char *base = S.base();
  unsigned *d_counts = (unsigned *)(base + table_bytes);
  std::vector<InverseRecord> table((size_t)n);
  for (int k = 0; k < n; ++k) {
    const LevelData &A = fixed[k]->lv[lv], &B = moving[k]->lv[lv];
    InverseRecord &R = table[(size_t)k];
    R.zf = A.z_plane, R.txf = A.tx, R.tyf = A.ty, R.cam = B.c_a;
    R.i_out = want_i[(size_t)k] ? (float *)(base + i_at[(size_t)k]) : nullptr;
    R.z_out = want_z[(size_t)k] ? (float *)(base + z_at[(size_t)k]) : nullptr;
    R.counts = d_counts + (size_t)kInvCounts * (size_t)k;
    R.wf = A.w, R.nf = A.n, R.wm = B.w, R.hm = B.h;
    R.fx = B.fx, R.fy = B.fy, R.ox = B.ox, R.oy = B.oy;
    inverse_rows(T + 16 * (size_t)k, R.M);
  }
  std::vector<unsigned> h_counts((size_t)kInvCounts * (size_t)n);
  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemcpyAsync(base, table.data(), sizeof(InverseRecord) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    const unsigned gx = (unsigned)((max_n + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(k_warp_inverse, dim3(gx, grid_rows(n, gx, kBlock)), dim3(kBlock), 0, st, (const InverseRecord *)base, n, opt->near_z,
                       opt->occlusion_margin, opt->depth == DVO_AMD_WARP_DEPTH_FIXED ? 1 : 0, as_pyramid ? 1 : 0, opt->fill_intensity);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), d_counts, sizeof(unsigned) * h_counts.size(), hipMemcpyDeviceToHost, st);
  if (!as_pyramid)
    for (int k = 0; k < n && e == hipSuccess; ++k) {
      const size_t bytes = sizeof(float) * (size_t)fixed[k]->lv[lv].n;
      if (intensity_out && intensity_out[k]) e = hipMemcpyAsync(intensity_out[k], base + i_at[(size_t)k], bytes, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && depth_out && depth_out[k]) e = hipMemcpyAsync(depth_out[k], base + z_at[(size_t)k], bytes, hipMemcpyDeviceToHost, st);
    }
  // the warp's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("inverse warp", e);
  bracket.read(1, 1);
  if (as_pyramid)
    for (int k = 0; k < n; ++k) {
      const dvo_amd_pyramid *f = fixed[k];
      const LevelData &L = f->lv[0];
      const PyramidSpec spec{L.w, L.h, L.fx, L.fy, L.ox, L.oy, f->n_levels, f->timestamp};
      const Level0Source src{(const float *)(base + i_at[(size_t)k]), (const float *)(base + z_at[(size_t)k]), L.w, nullptr, true};
      rc = pyramid_build(device, spec, src, &out[k]);
      if (rc) {
        out[k] = nullptr;
        release_all(out, n);
        return rc;
      }
    }
  if (counts)
    for (size_t i = 0; i < h_counts.size(); ++i) counts[i] = (long long)h_counts[i];
  return DVO_AMD_OK;
}

// level < 0: the pyramid form (level 0, `out` receives n pyramids); else the plane form (host planes, any may be null)
int forward_many(const char *entry, int n, const dvo_amd_pyramid *const *moving, const double *T, const dvo_amd_view *views, int level,
                 const dvo_amd_warp_options *opt, float *const *depth_out, float *const *intensity_out, int *const *index_out,
                 dvo_amd_pyramid **out, long long *counts) {
  const bool as_pyramid = level < 0;
  if (as_pyramid && out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative count");
  if (!moving || !T || !opt || (as_pyramid && !out)) return invalid(entry, "a NULL pointer");
  const int lv = as_pyramid ? 0 : level;
  for (int k = 0; k < n; ++k) {
    const std::string item = "item " + std::to_string(k);
    if (!moving[k]) return invalid(entry, item + ": a NULL pyramid");
    if (lv >= moving[k]->n_levels)
      return invalid(entry, item + ": level " + std::to_string(lv) + " is beyond a pyramid of " + std::to_string(moving[k]->n_levels) + " levels");
    if (!finite_all(T + 16 * (size_t)k, 16)) return invalid(entry, item + ": the transformation has a non-finite entry");
  }
  int rc = check_options(entry, opt);
  if (rc) return rc;
  if (views)
    for (int k = 0; k < n; ++k) {
      rc = check_view(entry, "item " + std::to_string(k), views + k);
      // dvo_amd_pyramid_create_from_device's rule for the pyramid a view becomes
      if (!rc && as_pyramid) rc = check_levels(entry, views[k].width, views[k].height, moving[k]->n_levels, " of the levels asked of the view");
      if (rc) return rc;
    }
  for (int k = 0; k < n; ++k)
    if (moving[k]->device != moving[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  const int device = moving[0]->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  // the view of every item: the caller's, or the moving level's own camera
  std::vector<dvo_amd_view> V((size_t)n);
  for (int k = 0; k < n; ++k) {
    const LevelData &L = moving[k]->lv[lv];
    V[(size_t)k] = views ? views[k] : dvo_amd_view{L.w, L.h, L.fx, L.fy, L.ox, L.oy, opt->near_z};
  }
  // the call's scratch: the record table, the counts, the depth buffers next to each other, then the planes anybody wants
  const size_t table_bytes = align_up(sizeof(ForwardRecord) * (size_t)n, 256);
  const size_t count_bytes = align_up(sizeof(unsigned) * kFwdCounts * (size_t)n, 256);
  std::vector<size_t> buf_at((size_t)n), z_at((size_t)n, 0), i_at((size_t)n, 0), x_at((size_t)n, 0);
  std::vector<char> want_z((size_t)n, 0), want_i((size_t)n, 0), want_x((size_t)n, 0);
  size_t scratch_bytes = table_bytes + count_bytes;
  const size_t zbuf_first = scratch_bytes;
  int max_n = 1, max_vn = 1;
  for (int k = 0; k < n; ++k) {
    const size_t vn = (size_t)V[(size_t)k].width * (size_t)V[(size_t)k].height;
    buf_at[(size_t)k] = scratch_bytes, scratch_bytes += align_up(sizeof(unsigned long long) * vn, 256);
    max_n = std::max(max_n, moving[k]->lv[lv].n), max_vn = std::max(max_vn, (int)vn);
  }
  const size_t zbuf_bytes = scratch_bytes - zbuf_first;  // (a multiple of 256: cleared 16 bytes at a time)
  for (int k = 0; k < n; ++k) {
    const size_t plane = align_up(sizeof(float) * (size_t)V[(size_t)k].width * (size_t)V[(size_t)k].height, 256);
    want_z[(size_t)k] = as_pyramid || (depth_out && depth_out[k]);
    want_i[(size_t)k] = as_pyramid || (intensity_out && intensity_out[k]);
    want_x[(size_t)k] = !as_pyramid && index_out && index_out[k];
    if (want_z[(size_t)k]) z_at[(size_t)k] = scratch_bytes, scratch_bytes += plane;
    if (want_i[(size_t)k]) i_at[(size_t)k] = scratch_bytes, scratch_bytes += plane;
    if (want_x[(size_t)k]) x_at[(size_t)k] = scratch_bytes, scratch_bytes += plane;
  }
  Scratch S;  // (every return below stands behind a synchronisation of the stream)
  rc = S.take(device, scratch_bytes);
  if (rc) return rc;
  char *base = S.base();
  unsigned *d_counts = (unsigned *)(base + table_bytes);
  std::vector<ForwardRecord> table((size_t)n);
  for (int k = 0; k < n; ++k) {
    const LevelData &L = moving[k]->lv[lv];
    const dvo_amd_view &v = V[(size_t)k];
    const double *Tk = T + 16 * (size_t)k;
    ForwardRecord &R = table[(size_t)k];
    R.z = L.z_plane, R.i = L.i_plane, R.tx = L.tx, R.ty = L.ty;
    R.zbuf = (unsigned long long *)(base + buf_at[(size_t)k]);
    R.z_out = want_z[(size_t)k] ? (float *)(base + z_at[(size_t)k]) : nullptr;
    R.i_out = want_i[(size_t)k] ? (float *)(base + i_at[(size_t)k]) : nullptr;
    R.idx_out = want_x[(size_t)k] ? (int *)(base + x_at[(size_t)k]) : nullptr;
    R.counts = d_counts + (size_t)kFwdCounts * (size_t)k;
    R.w = L.w, R.n = L.n;
    R.vw = v.width, R.vh = v.height, R.vn = v.width * v.height;
    R.fx = v.fx, R.fy = v.fy, R.ox = v.ox, R.oy = v.oy, R.near_z = v.near_z;
    R.fxm = L.fx, R.fym = L.fy;
    rows_from_column_major(Tk, R.T);
  }
  std::vector<unsigned> h_counts((size_t)kFwdCounts * (size_t)n);
  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemcpyAsync(base, table.data(), sizeof(ForwardRecord) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    const unsigned long long n2 = zbuf_bytes / sizeof(ulonglong2);
    const unsigned gc = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((n2 + kBlock - 1) / kBlock, 4096));
    hipLaunchKernelGGL(k_warp_clear, dim3(gc), dim3(kBlock), 0, st, (ulonglong2 *)(base + zbuf_first), n2);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    const unsigned gx = (unsigned)((max_n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_warp_splat, dim3(gx, grid_rows(n, gx, kBlock)), dim3(kBlock), 0, st, (const ForwardRecord *)base, n, opt->splat);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    const unsigned gx = (unsigned)((max_vn + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_warp_resolve, dim3(gx, grid_rows(n, gx, kBlock)), dim3(kBlock), 0, st, (const ForwardRecord *)base, n,
                       as_pyramid ? opt->fill_intensity : __builtin_nanf(""));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), d_counts, sizeof(unsigned) * h_counts.size(), hipMemcpyDeviceToHost, st);
  if (!as_pyramid)
    for (int k = 0; k < n && e == hipSuccess; ++k) {
      const size_t bytes = sizeof(float) * (size_t)V[(size_t)k].width * (size_t)V[(size_t)k].height;
      if (want_z[(size_t)k]) e = hipMemcpyAsync(depth_out[k], base + z_at[(size_t)k], bytes, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && want_i[(size_t)k]) e = hipMemcpyAsync(intensity_out[k], base + i_at[(size_t)k], bytes, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && want_x[(size_t)k]) e = hipMemcpyAsync(index_out[k], base + x_at[(size_t)k], bytes, hipMemcpyDeviceToHost, st);
    }
  // the warp's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("forward warp", e);
  bracket.read(3, 1);
  if (as_pyramid)
    for (int k = 0; k < n; ++k) {
      const dvo_amd_view &v = V[(size_t)k];
      const PyramidSpec spec{v.width, v.height, v.fx, v.fy, v.ox, v.oy, moving[k]->n_levels, moving[k]->timestamp};
      const Level0Source src{(const float *)(base + i_at[(size_t)k]), (const float *)(base + z_at[(size_t)k]), v.width, nullptr, true};
      rc = pyramid_build(device, spec, src, &out[k]);
      if (rc) {
        out[k] = nullptr;
        release_all(out, n);
        return rc;
      }
    }
  if (counts)
    for (size_t i = 0; i < h_counts.size(); ++i) counts[i] = (long long)h_counts[i];
  return DVO_AMD_OK;
}

int check_level(const char *entry, int level) {
  return level < 0 ? invalid(entry, "a negative level") : (int)DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_warp_options(dvo_amd_warp_options *opt) {
  if (!opt) return;
  opt->near_z = 0.1f, opt->occlusion_margin = 0.05f;
  opt->depth = DVO_AMD_WARP_DEPTH_TRANSFORMED, opt->splat = DVO_AMD_WARP_SPLAT_NEAREST;
  opt->fill_intensity = 0.0f;
}

int dvo_amd_warp_inverse_many(int n, const dvo_amd_pyramid *const *fixed, const dvo_amd_pyramid *const *moving, const double *T, int level,
                              const dvo_amd_warp_options *opt, float *const *intensity_out, float *const *depth_out, long long *counts) {
  static const char *entry = "dvo_amd_warp_inverse_many";
  const int rc = check_level(entry, level);
  return rc ? rc : inverse_many(entry, n, fixed, moving, T, level, opt, intensity_out, depth_out, nullptr, counts);
}

int dvo_amd_warp_inverse(const dvo_amd_pyramid *fixed, const dvo_amd_pyramid *moving, const double *T, int level,
                         const dvo_amd_warp_options *opt, float *intensity_out, float *depth_out, long long *counts) {
  static const char *entry = "dvo_amd_warp_inverse";
  if (!fixed || !moving || !T || !opt) return invalid(entry, "a NULL pointer");
  const int rc = check_level(entry, level);
  return rc ? rc : inverse_many(entry, 1, &fixed, &moving, T, level, opt, &intensity_out, &depth_out, nullptr, counts);
}

int dvo_amd_pyramid_warp_inverse_many(int n, const dvo_amd_pyramid *const *fixed, const dvo_amd_pyramid *const *moving, const double *T,
                                      const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts) {
  return inverse_many("dvo_amd_pyramid_warp_inverse_many", n, fixed, moving, T, -1, opt, nullptr, nullptr, out, counts);
}

int dvo_amd_pyramid_warp_inverse(const dvo_amd_pyramid *fixed, const dvo_amd_pyramid *moving, const double *T,
                                 const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts) {
  static const char *entry = "dvo_amd_pyramid_warp_inverse";
  if (out) *out = nullptr;
  if (!fixed || !moving || !T || !opt || !out) return invalid(entry, "a NULL pointer");
  return inverse_many(entry, 1, &fixed, &moving, T, -1, opt, nullptr, nullptr, out, counts);
}

int dvo_amd_warp_forward_many(int n, const dvo_amd_pyramid *const *moving, const double *T, const dvo_amd_view *views, int level,
                              const dvo_amd_warp_options *opt, float *const *depth_out, float *const *intensity_out, int *const *index_out,
                              long long *counts) {
  static const char *entry = "dvo_amd_warp_forward_many";
  const int rc = check_level(entry, level);
  return rc ? rc : forward_many(entry, n, moving, T, views, level, opt, depth_out, intensity_out, index_out, nullptr, counts);
}

int dvo_amd_warp_forward(const dvo_amd_pyramid *moving, const double *T, const dvo_amd_view *view, int level, const dvo_amd_warp_options *opt,
                         float *depth_out, float *intensity_out, int *index_out, long long *counts) {
  static const char *entry = "dvo_amd_warp_forward";
  if (!moving || !T || !opt) return invalid(entry, "a NULL pointer");
  const int rc = check_level(entry, level);
  return rc ? rc : forward_many(entry, 1, &moving, T, view, level, opt, &depth_out, &intensity_out, &index_out, nullptr, counts);
}

int dvo_amd_pyramid_warp_forward_many(int n, const dvo_amd_pyramid *const *moving, const double *T, const dvo_amd_view *views,
                                      const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts) {
  return forward_many("dvo_amd_pyramid_warp_forward_many", n, moving, T, views, -1, opt, nullptr, nullptr, nullptr, out, counts);
}

int dvo_amd_pyramid_warp_forward(const dvo_amd_pyramid *moving, const double *T, const dvo_amd_view *view, const dvo_amd_warp_options *opt,
                                 dvo_amd_pyramid **out, long long *counts) {
  static const char *entry = "dvo_amd_pyramid_warp_forward";
  if (out) *out = nullptr;
  if (!moving || !T || !opt || !out) return invalid(entry, "a NULL pointer");
  return forward_many(entry, 1, &moving, T, view, -1, opt, nullptr, nullptr, nullptr, out, counts);
}

/* instrumentation: *launches / *synchronisations (may be NULL) receive what the most recent successful warp entry on `device`
 * enqueued of its own (1 / 1 for an inverse warp, 3 / 1 for a forward warp, whatever n is; a pyramid form's builder comes on top);
 * with enable != 0 the launches of every later call are bracketed by two events on the prep stream and *last_ms (may be NULL)
 * receives the device time of the most recent bracketed call */
int dvo_amd_debug_warp_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms) {
  return timing_entry(g_timing, device, enable, launches, synchronisations, last_ms);
}

}  // extern "C"
