// Depth fusion on the device: the frames tracked against a keyframe each measured the keyframe's surfaces again, and their poses
// relative to it are what match() returned.  dvo_amd_pyramid_fuse_depth / _many carry every frame's level-0 depth onto the
// keyframe's pixels by dvo_amd_covisibility's rule, average what agrees with inverse-variance weights and hand the result to the
// ordinary builder: the output is an ordinary pyramid.  The rule is pinned in include/dvo_amd.h ("Depth fusion");
// tests/depth_fusion_ref.py restates it in numpy.
//
//   k_fuse_depth     ONE launch over all keyframes of a call: blockIdx.y walks the keyframe records, striding by gridDim.y,
//                    blockIdx.x a chunk of the keyframe's level 0.  A lane owns two consecutive pixels of one row (widths are
//                    multiples of 4: one 8-byte load, one 8-byte store, one 16-bit store of two observation bytes) and walks
//                    the keyframe's frames IN ORDER, so the order of a pixel's fp32 sums is the rule's and not the launch's.
//                    (Four pixels per lane made a 640x480 keyframe 1 200 waves on 1 024 SIMDs; two measured faster from
//                    eight frames on: DESIGN.md 4.16.)  A frame's record (M, intrinsics, size, plane) is read at a
//                    block-uniform index: scalar loads into scalar registers.  The walk is pipelined by one frame: the
//                    projections and the depth gathers of frame k + 1 (eight per lane with the bilinear sample) are issued
//                    before frame k's are consumed.  A gather's address is clamped to the plane's first pixel where the
//                    projection is not inside, so that every load is unconditional and in bounds.
// The eight counts per frame and the four per keyframe: ballots and popcounts per wave, integer adds into LDS per block
// (kFrameBatch frames between two barriers), one integer atomicAdd per non-zero count -- integers only, no float atomic
// anywhere, so nothing depends on the launch geometry or on the order atomics land in.  One synchronisation for the fusion on
// the device's prep stream, then pyramid_build's own per keyframe.
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>

namespace dvo_amd {
namespace fuse {

constexpr int kBlock = 256;
constexpr int kLanePixels = 2;                // pixels per lane
constexpr int kChunk = kBlock * kLanePixels;  // ... and per block
constexpr int kFrameCounts = DVO_AMD_FUSE_FRAME_COUNTS;  // valid, behind, outside, no_depth, consistent, occluded, seen_through, fused
constexpr int kKeyCounts = DVO_AMD_FUSE_KEYFRAME_COUNTS;  // with_depth, confirmed, unconfirmed_kept, unconfirmed_dropped
constexpr int kFrameBatch = kBlock / kFrameCounts;  // frames whose counts a block gathers in LDS between two barriers
static_assert(kFrameBatch * kFrameCounts == kBlock, "a thread per (frame of the batch, count) clears and flushes the LDS counts");
static_assert(DVO_AMD_FUSE_MAX_FRAMES <= 255, "a pixel's observations fit a byte");

// (The planes are read through DVO_DEVICE_GLOBAL: with flat loads, the scalar load of the next frame's record would wait for every
// gather in flight.)
typedef float vpf __attribute__((ext_vector_type(kLanePixels)));  // a lane's pixels (a plain vector type: loadable from any address space)
typedef std::conditional<kLanePixels == 4, unsigned, unsigned short>::type obs_word;  // ... and their observation bytes
static_assert(kLanePixels == 2 || kLanePixels == 4, "a lane's pixels are one load, and they divide every width (a multiple of 4)");

// one frame of one keyframe as the kernel reads it (block-uniform: scalar registers)
struct FrameRecord {
  const float *z;     // level-0 depth plane
  unsigned *counts;   // [kFrameCounts]
  int w, h;
  float fx, fy, ox, oy;
  float M[12];        // rows 0..2 of keyframe camera -> frame camera, row-major
};

// one keyframe
struct KeyRecord {
  const float *z, *tx, *ty;  // level 0: depth plane and rays
  float *out;                // the fused plane
  unsigned char *obs;        // the observation bytes (null: nobody asked)
  unsigned *counts;          // [kKeyCounts]
  int w, n;                  // width, pixels
  int first, count;          // its frames in the frame table
};

// a pixel's sample of one frame between issue and consumption
template <bool kNearest>
struct Sample {
  float qz, a, b;
  float z[kNearest ? 1 : 4];  // Zs, or z00, z10, z01, z11
  int cls;                    // -1 no pixel or no depth; 0 sampled, to be classified; 1 behind; 2 outside
};

// one integer add to a count in global memory (a flat atomic would count as an LDS access too and, while one is in flight, make
// every wait for a gather a wait for all of them)
__device__ __forceinline__ void add_global(unsigned *p, unsigned v) {
  (void)__hip_atomic_fetch_add((DVO_DEVICE_GLOBAL unsigned *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// steps 3a..3e for one pixel and one frame: the point, the projection, the gathers (issued, not waited for)
template <bool kNearest>
__device__ __forceinline__ void issue(const FrameRecord &F, float near_z, bool has, float x, float y, float z0, Sample<kNearest> &S) {
  float qx, qy, qz;
  rules::transform_rows(F.M, x, y, z0, qx, qy, qz);
  S.qz = qz, S.a = 0.f, S.b = 0.f;
  int cls = has ? 0 : -1;
  if (has && !(qz >= near_z)) cls = 1;
  const float px = (qx * F.fx) / qz + F.ox, py = (qy * F.fy) / qz + F.oy;
  const DVO_DEVICE_GLOBAL float *Z = (const DVO_DEVICE_GLOBAL float *)F.z;
  size_t at = 0;  // (the plane's first pixel where nothing is sampled: every load below is unconditional and in bounds)
  if constexpr (kNearest) {
    const float pu = floorf(px + 0.5f), pv = floorf(py + 0.5f);
    // (rules::pixel_inside's test, kept as a value of its own: the select below is part of the branchless form)
    const bool inside = pu >= 0.0f && pu <= (float)(F.w - 1) && pv >= 0.0f && pv <= (float)(F.h - 1);
    if (cls == 0 && !inside) cls = 2;
    if (cls == 0) at = rules::pixel_offset(pu, pv, F.w);
    S.z[0] = Z[at];
  } else {
    const float x0 = floorf(px), y0 = floorf(py);
    const bool inside = x0 >= 0.0f && x0 <= (float)(F.w - 2) && y0 >= 0.0f && y0 <= (float)(F.h - 2);
    if (cls == 0 && !inside) cls = 2;
    if (cls == 0) at = (size_t)(int)y0 * (size_t)F.w + (size_t)(int)x0;  // 0 <= x0 <= w-2, 0 <= y0 <= h-2: tested in float above
    S.a = px - x0, S.b = py - y0;
    // (a frame is at least 4x2: with at == 0 the four addresses are inside the plane too)
    S.z[0] = Z[at], S.z[1] = Z[at + 1], S.z[2] = Z[at + (size_t)F.w], S.z[3] = Z[at + (size_t)F.w + 1];
  }
  S.cls = cls;
}

// the rest of step 3: the class of the sample (1..6, -1) and, where it is fused, the pixel's sums
template <bool kNearest>
__device__ __forceinline__ int consume(const FrameRecord &F, const Sample<kNearest> &S, float sigmas, float min_cos, float tx, float ty,
                                       float z0, float &sw, float &swz, int &n_obs, bool &fused) {
  // Without a branch: every lane forms every value and the outcome selects.  A branch around the first use of the gathered depths
  // would leave a path on which they are never waited for, and the wait before the next frame's gathers would then be for all of
  // them (vmcnt(0)) instead of for this frame's alone.  (So not rules::classify_covisible, which branches: its parts only.)
  float Zs;
  bool nan;
  if constexpr (kNearest) {
    Zs = S.z[0];
    nan = !(Zs == Zs);
  } else {
    const float z00 = S.z[0], z10 = S.z[1], z01 = S.z[2], z11 = S.z[3];
    nan = !(z00 == z00) || !(z10 == z10) || !(z01 == z01) || !(z11 == z11);
    const float top = z00 + S.a * (z10 - z00);
    const float bot = z01 + S.a * (z11 - z01);
    Zs = top + S.b * (bot - top);
  }
  const float d = Zs - S.qz;
  const float tol = sigmas * rules::depth_sigma(S.qz);
  const float c = (F.M[8] * tx + F.M[9] * ty) + F.M[10];
  const float z_obs = z0 + d / c;
  const float sg = rules::depth_sigma(Zs);
  const float w = 1.0f / (sg * sg);
  const bool sampled = S.cls == 0 && !nan;
  const int cls = S.cls != 0 ? S.cls : nan ? 3 : d < -tol ? 5 : d > tol ? 6 : 4;
  fused = sampled && cls == 4 && c >= min_cos;
  sw = fused ? sw + w : sw;
  swz = fused ? swz + w * z_obs : swz;
  n_obs += fused ? 1 : 0;
  return cls;
}

template <bool kNearest>
__global__ void __launch_bounds__(kBlock) k_fuse_depth(const KeyRecord *__restrict__ keys, int n_keys, const FrameRecord *__restrict__ frames,
                                                       float near_z, float sigmas, float min_cos, int min_observations, int drop_unconfirmed) {
  __shared__ unsigned s_frame[kFrameBatch * kFrameCounts];
  __shared__ unsigned s_key[kKeyCounts];
  const int lane = threadIdx.x & 63;
  for (int key = blockIdx.y; key < n_keys; key += gridDim.y) {
    const KeyRecord K = keys[key];                 // uniform over the block
    if (blockIdx.x * kChunk >= K.n) continue;      // (block-uniform: no barrier is skipped by part of a block)
    const FrameRecord *__restrict__ Fs = frames + K.first;
    const int nf = K.count;
    const int p0 = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
    const bool live = p0 < K.n;  // (w and n are multiples of 4: all of a lane's pixels or none, all in one row)
    float z0[kLanePixels], tx[kLanePixels], x[kLanePixels], y[kLanePixels], sw[kLanePixels], swz[kLanePixels];
    int n_obs[kLanePixels];
    bool has[kLanePixels];
    float ty = 0.f;
    {
      vpf z = 0.f, t = 0.f;
      if (live) {
        z = *(const DVO_DEVICE_GLOBAL vpf *)(K.z + p0);
        const int v = p0 / K.w, u0 = p0 - v * K.w;
        t = *(const DVO_DEVICE_GLOBAL vpf *)(K.tx + u0);  // (u0 is a multiple of kLanePixels and the ray plane is 256-byte aligned)
        ty = ((const DVO_DEVICE_GLOBAL float *)K.ty)[v];
      }
#pragma unroll
      for (int i = 0; i < kLanePixels; ++i) z0[i] = z[i], tx[i] = t[i];
    }
#pragma unroll
    for (int i = 0; i < kLanePixels; ++i) {
      has[i] = live && rules::finite_f(z0[i]);
      x[i] = tx[i] * z0[i], y[i] = ty * z0[i];
      const float sg = rules::depth_sigma(z0[i]);
      const float w = 1.0f / (sg * sg);
      sw[i] = w, swz[i] = w * z0[i], n_obs[i] = 0;
    }
    if (threadIdx.x < kKeyCounts) s_key[threadIdx.x] = 0u;  // (flushed by the same threads at the end of the block's last keyframe)
    if (nf == 0) __syncthreads();                            // (with frames, the first batch's barrier below)

    // two sets of samples, taken in turns: no sample is moved between registers, so nothing waits for a gather before its use
    Sample<kNearest> even[kLanePixels], odd[kLanePixels];
    if (nf > 0) {
      const FrameRecord F = Fs[0];
#pragma unroll
      for (int i = 0; i < kLanePixels; ++i) issue<kNearest>(F, near_z, has[i], x[i], y[i], z0[i], even[i]);
    }
    auto step = [&](int k, Sample<kNearest> (&cur)[kLanePixels], Sample<kNearest> (&nxt)[kLanePixels]) {
      const int kb = k % kFrameBatch;
      if (kb == 0) {
        // a thread per (frame of the batch, count): what the batch before left goes out, the slot is cleared (both by this thread)
        if (k > 0) {
          __syncthreads();
          const unsigned v = s_frame[threadIdx.x];
          if (v) add_global(Fs[k - kFrameBatch + (int)(threadIdx.x / kFrameCounts)].counts + threadIdx.x % kFrameCounts, v);
        }
        s_frame[threadIdx.x] = 0u;
        __syncthreads();
      }
      const FrameRecord F = Fs[k];
      if (k + 1 < nf) {  // frame k + 1's gathers are in flight while frame k is consumed
        const FrameRecord G = Fs[k + 1];
#pragma unroll
        for (int i = 0; i < kLanePixels; ++i) issue<kNearest>(G, near_z, has[i], x[i], y[i], z0[i], nxt[i]);
      }
      unsigned cnt[kFrameCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < kLanePixels; ++i) {
        bool fused;
        const int cls = consume<kNearest>(F, cur[i], sigmas, min_cos, tx[i], ty, z0[i], sw[i], swz[i], n_obs[i], fused);
        cnt[0] += (unsigned)__popcll(__ballot(cls >= 0));
#pragma unroll
        for (int c = 1; c < 7; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
        cnt[7] += (unsigned)__popcll(__ballot(fused));
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kFrameCounts; ++c)
          if (cnt[c]) atomicAdd(&s_frame[kb * kFrameCounts + c], cnt[c]);
      }
    };
    for (int k = 0; k < nf; k += 2) {  // (nf is block-uniform: every thread reaches every barrier of a step)
      step(k, even, odd);
      if (k + 1 < nf) step(k + 1, odd, even);
    }

    // step 4
    float o[kLanePixels];
    unsigned word = 0u;
    unsigned kc[kKeyCounts] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kLanePixels; ++i) {
      const float fusedz = swz[i] / sw[i];
      const bool confirmed = has[i] && n_obs[i] >= min_observations;
      const bool dropped = has[i] && !confirmed && drop_unconfirmed != 0;
      o[i] = has[i] && !dropped ? fusedz : __builtin_nanf("");
      word |= has[i] ? ((unsigned)n_obs[i] << (8 * i)) : 0u;
      kc[0] += (unsigned)__popcll(__ballot(has[i]));
      kc[1] += (unsigned)__popcll(__ballot(confirmed));
      kc[2] += (unsigned)__popcll(__ballot(has[i] && !confirmed && !dropped));
      kc[3] += (unsigned)__popcll(__ballot(dropped));
    }
    if (live) {
      vpf fused;
#pragma unroll
      for (int i = 0; i < kLanePixels; ++i) fused[i] = o[i];
      *(DVO_DEVICE_GLOBAL vpf *)(K.out + p0) = fused;
      if (K.obs) *(DVO_DEVICE_GLOBAL obs_word *)(K.obs + p0) = (obs_word)word;
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kKeyCounts; ++c)
        if (kc[c]) atomicAdd(&s_key[c], kc[c]);
    }
    __syncthreads();
    if (nf > 0) {
      const int k0 = (nf - 1) / kFrameBatch * kFrameBatch;
      const int f = k0 + (int)(threadIdx.x / kFrameCounts);
      const unsigned v = s_frame[threadIdx.x];
      if (f < nf && v) add_global(Fs[f].counts + threadIdx.x % kFrameCounts, v);
    }
    if (threadIdx.x < kKeyCounts) {
      const unsigned v = s_key[threadIdx.x];
      if (v) add_global(K.counts + threadIdx.x, v);
    }
    __syncthreads();  // s_frame and s_key are written again for the block's next keyframe
  }
}

}  // namespace fuse
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::fuse;

namespace {

// dvo_amd_debug_fuse_timing: two events around the fusion launch of a call on the prep stream (off unless asked for)
DeviceTiming g_timing[kMaxDevices];

// the record tables and the counts of the call in flight (grown to the largest call and kept; used with the device's mutex held
// from the tables' upload to the last thing enqueued that touches the area)
DeviceBuf g_area[kMaxDevices];

int check_options(const char *entry, const dvo_amd_fuse_options *opt) {
  if (!std::isfinite(opt->near_z) || !(opt->near_z > 0.0f)) return invalid(entry, "near_z must be finite and positive");
  if (!std::isfinite(opt->depth_sigmas) || opt->depth_sigmas < 0.0f) return invalid(entry, "depth_sigmas must be finite and >= 0");
  if (!std::isfinite(opt->min_cos) || !(opt->min_cos > 0.0f)) return invalid(entry, "min_cos must be finite and positive");
  if (opt->sample != DVO_AMD_FUSE_BILINEAR && opt->sample != DVO_AMD_FUSE_NEAREST)
    return invalid(entry, "sample must be DVO_AMD_FUSE_BILINEAR or DVO_AMD_FUSE_NEAREST");
  if (opt->min_observations < 0 || opt->min_observations > DVO_AMD_FUSE_MAX_FRAMES)
    return invalid(entry, "min_observations is outside 0.." + std::to_string(DVO_AMD_FUSE_MAX_FRAMES));
  return DVO_AMD_OK;
}

int fuse_many(const char *entry, int nk, const dvo_amd_pyramid *const *keyframes, const int *offsets,
              const dvo_amd_pyramid *const *frames, const double *T, const dvo_amd_fuse_options *opt, dvo_amd_pyramid **out,
              long long *frame_counts, long long *keyframe_counts, unsigned char *const *observations) {
  if (out && nk > 0)
    for (int k = 0; k < nk; ++k) out[k] = nullptr;
  if (nk < 0) return invalid(entry, "a negative keyframe count");
  if (!keyframes || !offsets || !opt || !out) return invalid(entry, "a NULL pointer");
  if (offsets[0] != 0) return invalid(entry, "the frame offsets do not start at 0");
  for (int k = 0; k < nk; ++k) {
    const long long n = (long long)offsets[k + 1] - (long long)offsets[k];
    if (n < 0) return invalid(entry, nk == 1 ? std::string("a negative frame count") : "the frame offsets decrease at keyframe " + std::to_string(k));
    if (n > DVO_AMD_FUSE_MAX_FRAMES)
      return invalid(entry, (nk == 1 ? std::string("") : "keyframe " + std::to_string(k) + ": ") + "more than " +
                                std::to_string(DVO_AMD_FUSE_MAX_FRAMES) + " frames");
  }
  const int total = nk > 0 ? offsets[nk] : 0;
  if (total > 0 && (!frames || !T)) return invalid(entry, "a NULL pointer");
  for (int k = 0; k < nk; ++k)
    if (!keyframes[k]) return invalid(entry, "keyframe " + std::to_string(k) + " is NULL");
  for (int f = 0; f < total; ++f) {
    if (!frames[f]) return invalid(entry, "frame " + std::to_string(f) + " is NULL");
    if (!finite_all(T + 16 * (size_t)f, 16)) return invalid(entry, "frame " + std::to_string(f) + ": the transformation has a non-finite entry");
  }
  int rc = check_options(entry, opt);
  if (rc) return rc;
  for (int k = 0; k < nk; ++k)
    if (keyframes[k]->device != keyframes[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  for (int f = 0; f < total; ++f)
    if (frames[f]->device != keyframes[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (nk == 0) return DVO_AMD_OK;

  const int device = keyframes[0]->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  // the call's own scratch: a fused plane per keyframe, and the observation bytes of the keyframes that ask for them
  std::vector<size_t> plane_at((size_t)nk), obs_at((size_t)nk, 0);
  size_t scratch_bytes = 0;
  int max_n = 1;
  for (int k = 0; k < nk; ++k) {
    const LevelData &L = keyframes[k]->lv[0];
    plane_at[(size_t)k] = scratch_bytes;
    scratch_bytes += align_up(sizeof(float) * (size_t)L.n, 256);
    max_n = std::max(max_n, L.n);
  }
  for (int k = 0; k < nk; ++k)
    if (observations && observations[k]) {
      obs_at[(size_t)k] = scratch_bytes;
      scratch_bytes += align_up((size_t)keyframes[k]->lv[0].n, 256);
    }
  // (given back when the call ends: every return below stands before anything is enqueued or behind a synchronisation of the stream)
  Scratch S;
  rc = S.take(device, scratch_bytes);
  if (rc) return rc;
  void *const scratch = S.mem;

  const size_t key_bytes = align_up(sizeof(KeyRecord) * (size_t)nk, 256);
  const size_t frame_bytes = align_up(sizeof(FrameRecord) * (size_t)std::max(total, 1), 256);
  const size_t n_counts = (size_t)kFrameCounts * (size_t)total + (size_t)kKeyCounts * (size_t)nk;
  const size_t count_bytes = sizeof(unsigned) * n_counts;
  std::vector<KeyRecord> key_table((size_t)nk);
  std::vector<FrameRecord> frame_table((size_t)total);
  std::vector<unsigned> h_counts(n_counts);

  Bracket bracket(g_timing[device]);
  // The tables and the counts live in the device's one fuse area, which the next call overwrites: the device's mutex is held from
  // the upload to the last thing enqueued that reads or writes the area (dvo_amd_mask_warp_many does the same for its table).
  std::unique_lock<std::mutex> area_lock(device_mutex(device));
  DeviceBuf &area = g_area[device];
  rc = grow(area, key_bytes + frame_bytes + count_bytes, 1 << 16, "fuse tables");
  if (rc) return rc;  // (nothing has been enqueued)
  KeyRecord *d_keys = (KeyRecord *)area.p;
  FrameRecord *d_frames = (FrameRecord *)((char *)area.p + key_bytes);
  unsigned *d_counts = (unsigned *)((char *)area.p + key_bytes + frame_bytes);
  unsigned *d_key_counts = d_counts + (size_t)kFrameCounts * (size_t)total;
  for (int k = 0; k < nk; ++k) {
    const LevelData &L = keyframes[k]->lv[0];
    KeyRecord &K = key_table[(size_t)k];
    K.z = L.z_plane, K.tx = L.tx, K.ty = L.ty;
    K.out = (float *)((char *)scratch + plane_at[(size_t)k]);
    K.obs = observations && observations[k] ? (unsigned char *)scratch + obs_at[(size_t)k] : nullptr;
    K.counts = d_key_counts + (size_t)kKeyCounts * (size_t)k;
    K.w = L.w, K.n = L.n, K.first = offsets[k], K.count = offsets[k + 1] - offsets[k];
  }
  for (int f = 0; f < total; ++f) {
    const LevelData &L = frames[f]->lv[0];
    FrameRecord &F = frame_table[(size_t)f];
    F.z = L.z_plane, F.counts = d_counts + (size_t)kFrameCounts * (size_t)f;
    F.w = L.w, F.h = L.h, F.fx = L.fx, F.fy = L.fy, F.ox = L.ox, F.oy = L.oy;
    inverse_rows(T + 16 * (size_t)f, F.M);
  }
  hipError_t e = hipMemcpyAsync(d_keys, key_table.data(), sizeof(KeyRecord) * (size_t)nk, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && total > 0)
    e = hipMemcpyAsync(d_frames, frame_table.data(), sizeof(FrameRecord) * (size_t)total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    const unsigned gx = (unsigned)((max_n + kChunk - 1) / kChunk);
    const unsigned gy = grid_rows(nk, gx, kBlock);  // a block takes further keyframes in steps of gridDim.y
    if (opt->sample == DVO_AMD_FUSE_NEAREST)
      hipLaunchKernelGGL(k_fuse_depth<true>, dim3(gx, gy), dim3(kBlock), 0, st, (const KeyRecord *)d_keys, nk, (const FrameRecord *)d_frames,
                         opt->near_z, opt->depth_sigmas, opt->min_cos, opt->min_observations, opt->drop_unconfirmed);
    else
      hipLaunchKernelGGL(k_fuse_depth<false>, dim3(gx, gy), dim3(kBlock), 0, st, (const KeyRecord *)d_keys, nk, (const FrameRecord *)d_frames,
                         opt->near_z, opt->depth_sigmas, opt->min_cos, opt->min_observations, opt->drop_unconfirmed);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && (frame_counts || keyframe_counts)) e = hipMemcpyAsync(h_counts.data(), d_counts, count_bytes, hipMemcpyDeviceToHost, st);
  for (int k = 0; k < nk && e == hipSuccess; ++k)
    if (observations && observations[k])
      e = hipMemcpyAsync(observations[k], (const char *)scratch + obs_at[(size_t)k], (size_t)keyframes[k]->lv[0].n, hipMemcpyDeviceToHost, st);
  area_lock.unlock();
  // the fusion's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("depth fusion", e);
  bracket.read();
  // every keyframe's pyramid from its own intensity plane and its fused plane, by the builder every pyramid comes from
  for (int k = 0; k < nk; ++k) {
    const dvo_amd_pyramid *kf = keyframes[k];
    const LevelData &L = kf->lv[0];
    const PyramidSpec spec{L.w, L.h, L.fx, L.fy, L.ox, L.oy, kf->n_levels, kf->timestamp};
    const Level0Source src{L.i_plane, (const float *)((const char *)scratch + plane_at[(size_t)k]), L.w, nullptr, true};
    rc = pyramid_build(device, spec, src, &out[k]);
    if (rc) {
      for (int j = 0; j < k; ++j) dvo_amd_pyramid_release(out[j]), out[j] = nullptr;
      out[k] = nullptr;
      return rc;
    }
  }
  // (pyramid_build drained the stream: nothing reads the scratch any more when S goes out of scope)
  if (frame_counts)
    for (size_t i = 0; i < (size_t)kFrameCounts * (size_t)total; ++i) frame_counts[i] = (long long)h_counts[i];
  if (keyframe_counts)
    for (size_t i = 0; i < (size_t)kKeyCounts * (size_t)nk; ++i) keyframe_counts[i] = (long long)h_counts[(size_t)kFrameCounts * (size_t)total + i];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_fuse_options(dvo_amd_fuse_options *opt) {
  if (!opt) return;
  opt->near_z = 0.1f, opt->depth_sigmas = 5.0f, opt->min_cos = 0.5f;
  opt->sample = DVO_AMD_FUSE_BILINEAR, opt->min_observations = 0, opt->drop_unconfirmed = 0;
}

int dvo_amd_pyramid_fuse_depth_many(int n_keyframes, const dvo_amd_pyramid *const *keyframes, const int *frame_offsets,
                                    const dvo_amd_pyramid *const *frames, const double *T, const dvo_amd_fuse_options *opt,
                                    dvo_amd_pyramid **out, long long *frame_counts, long long *keyframe_counts,
                                    unsigned char *const *observations) {
  return fuse_many("dvo_amd_pyramid_fuse_depth_many", n_keyframes, keyframes, frame_offsets, frames, T, opt, out, frame_counts,
                   keyframe_counts, observations);
}

int dvo_amd_pyramid_fuse_depth(const dvo_amd_pyramid *keyframe, int n, const dvo_amd_pyramid *const *frames, const double *T,
                               const dvo_amd_fuse_options *opt, dvo_amd_pyramid **out, long long *frame_counts, long long *keyframe_counts,
                               unsigned char *observations) {
  static const char *entry = "dvo_amd_pyramid_fuse_depth";
  if (out) *out = nullptr;
  if (!keyframe || !opt || !out) return invalid(entry, "a NULL pointer");
  const int offsets[2] = {0, n};
  return fuse_many(entry, 1, &keyframe, offsets, frames, T, opt, out, frame_counts, keyframe_counts, observations ? &observations : nullptr);
}

/* instrumentation: with enable != 0 the fusion launch of every later dvo_amd_pyramid_fuse_depth / _many on `device` is bracketed by
 * two events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent bracketed launch */
int dvo_amd_debug_fuse_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
