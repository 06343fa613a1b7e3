// Loop-closure candidates: the reference's radius search on keyframe translations (NearestNeighborConstraintSearch::
// findPossibleConstraints, keyframe_constraint_search.cpp:41-72) and, beyond the reference, the view overlap of ordered keyframe
// pairs counted on the device (dvo_amd_covisibility), by which dvo_amd_find_constraint_candidates can prune the radius
// candidates before any alignment runs.  The rule is pinned in include/dvo_amd.h; tests/covisibility_ref.py restates it.
//   k_covis   blockIdx.y = the pair, blockIdx.x = a chunk of a's pixels; every pixel of a with a depth is moved into b's frame,
//             projected and classified against b's depth plane; the seven counts are reduced per wave (ballots), per block (LDS)
//             and added to the pair's record with one integer atomic per non-zero count
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace dvo_amd {
namespace covis {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSteps = 4;                   // pixels per lane: a wave walks kSteps runs of 64 consecutive pixels
constexpr int kChunk = kBlock * kSteps;     // pixels of a per block
constexpr int kCounts = 7;                  // valid, behind, outside, no_depth, consistent, occluded, seen_through

// one ordered pair (a, b) as the kernel reads it
struct Pair {
  const float *za, *txa, *tya;  // a: depth plane and rays of the level
  const float *zb;              // b: depth plane of the level
  int wa, na;                   // a: width, pixels
  int wb, hb;                   // b: size
  float fx, fy, ox, oy;         // b: intrinsics
  float T[12];                  // rows 0..2 of pose_b^-1 * pose_a, row-major
};

__global__ void __launch_bounds__(kBlock) k_covis(const Pair *__restrict__ pairs, int n_pairs, float near_z, float sigmas,
                                                  unsigned *__restrict__ out) {
  __shared__ unsigned s_cnt[kWaves][kCounts + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int pair = blockIdx.y; pair < n_pairs; pair += gridDim.y) {
    const Pair P = pairs[pair];  // uniform over the block: scalar loads, once per pair
    const int na = P.na;
    const int base = blockIdx.x * kChunk + wave * (kSteps * 64);
    if (blockIdx.x * kChunk >= na) continue;  // (block-uniform: no barrier is skipped by part of a block)
    unsigned cnt[kCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      const int p = base + k * 64 + lane;
      int cls = -1;  // -1: no pixel or no depth; else the index of the outcome's count
      if (p < na) {
        const float z = P.za[p];
        if (rules::finite_f(z)) {
          const int v = p / P.wa, u = p - v * P.wa;
          size_t at;
          cls = rules::classify_covisible(z, P.txa[u], P.tya[v], P.T, near_z, sigmas, P.zb, P.wb, P.hb, P.fx, P.fy, P.ox, P.oy, at);
        }
      }
      cnt[0] += (unsigned)__popcll(__ballot(cls >= 0));
#pragma unroll
      for (int c = 1; c < kCounts; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kCounts; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < kCounts) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
      if (sum) atomicAdd(out + (size_t)pair * 8 + threadIdx.x, sum);
    }
    __syncthreads();  // s_cnt is written again for the block's next pair
  }
}

}  // namespace covis

namespace host {

struct CovisWorkspace {
  DeviceBuf pairs, out;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double device_ms = 0.0;
};

namespace {

// (a buffer that has to grow at least doubles)
int grow_covis(DeviceBuf &b, size_t bytes) {
  return grow(b, bytes <= b.bytes ? bytes : std::max(bytes, 2 * b.bytes), 1 << 16, "covisibility workspace");
}

int check_options(const char *entry, const dvo_amd_covisibility_options *opt) {
  if (!opt) return invalid(entry, "the options are NULL");
  if (opt->level < 0) return invalid(entry, "level must be >= 0");
  if (!std::isfinite(opt->depth_sigmas) || opt->depth_sigmas < 0.0f) return invalid(entry, "depth_sigmas must be finite and >= 0");
  if (!std::isfinite(opt->near_z) || !(opt->near_z > 0.0f)) return invalid(entry, "near_z must be finite and positive");
  return DVO_AMD_OK;
}

// the checks of dvo_amd_covisibility that need no device
int check_pairs(const char *entry, int n_keyframes, const dvo_amd_keyframe *keyframes, const dvo_amd_covisibility_options *opt,
                int n_pairs, const int *pair_a, const int *pair_b, const dvo_amd_covisibility_counts *out) {
  if (n_pairs < 0 || n_keyframes < 0) return invalid(entry, "a negative count");
  if (n_pairs > 0 && (!keyframes || !pair_a || !pair_b || !out)) return invalid(entry, "a NULL array with n_pairs > 0");
  for (int i = 0; i < n_pairs; ++i) {
    for (const int k : {pair_a[i], pair_b[i]}) {
      if (k < 0 || k >= n_keyframes) return invalid(entry, "pair " + std::to_string(i) + " names keyframe " + std::to_string(k) + " out of range");
      if (!keyframes[k].image) return invalid(entry, "keyframe " + std::to_string(k) + " has no image");
      if (!finite_all(keyframes[k].pose, 16)) return invalid(entry, "keyframe " + std::to_string(k) + " has a non-finite pose entry");
    }
  }
  return n_pairs > 0 || opt ? check_options(entry, opt) : DVO_AMD_OK;
}

int covisibility(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes, const dvo_amd_covisibility_options *opt,
                 int n_pairs, const int *pair_a, const int *pair_b, dvo_amd_covisibility_counts *out, const char *entry) {
  int rc = check_pairs(entry, n_keyframes, keyframes, opt, n_pairs, pair_a, pair_b, out);
  if (rc) return rc;
  rc = have_device();
  if (rc) return rc;
  if (!ctx) return invalid(entry, "the context is NULL");
  for (int i = 0; i < n_pairs; ++i)
    if (keyframes[pair_a[i]].image->device != ctx->device || keyframes[pair_b[i]].image->device != ctx->device)
      return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = queue_must_be_idle(ctx, entry);
  if (rc) return rc;
  if (n_pairs == 0) return DVO_AMD_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->covis_ws) {
    ctx->covis_ws = new CovisWorkspace();
    for (hipEvent_t &e : ctx->covis_ws->ev) HIP_TRY(hipEventCreate(&e));
  }
  CovisWorkspace &W = *ctx->covis_ws;
  for (hipEvent_t &e : W.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  std::vector<covis::Pair> table((size_t)n_pairs);
  int max_na = 1;
  for (int i = 0; i < n_pairs; ++i) {
    const dvo_amd_keyframe &ka = keyframes[pair_a[i]], &kb = keyframes[pair_b[i]];
    const int l = std::min(opt->level, std::min(ka.image->n_levels, kb.image->n_levels) - 1);
    const LevelData &A = ka.image->lv[l], &B = kb.image->lv[l];
    covis::Pair &P = table[(size_t)i];
    P.za = A.z_plane, P.txa = A.tx, P.tya = A.ty, P.zb = B.z_plane;
    P.wa = A.w, P.na = A.w * A.h, P.wb = B.w, P.hb = B.h;
    P.fx = B.fx, P.fy = B.fy, P.ox = B.ox, P.oy = B.oy;
    relative_rows(ka.pose, kb.pose, P.T);
    max_na = std::max(max_na, P.na);
  }
  const size_t out_bytes = sizeof(dvo_amd_covisibility_counts) * (size_t)n_pairs;
  rc = grow_covis(W.pairs, sizeof(covis::Pair) * (size_t)n_pairs);
  if (!rc) rc = grow_covis(W.out, out_bytes);
  if (rc) return rc;
  const hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(W.pairs.p, table.data(), sizeof(covis::Pair) * (size_t)n_pairs, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(W.out.p, 0, out_bytes, st));
  const unsigned gx = (unsigned)((max_na + covis::kChunk - 1) / covis::kChunk);
  const unsigned gy = grid_rows(n_pairs, gx, covis::kBlock);  // a block takes further pairs in steps of gridDim.y
  HIP_TRY(hipEventRecord(W.ev[0], st));
  hipLaunchKernelGGL(covis::k_covis, dim3(gx, gy), dim3(covis::kBlock), 0, st, (const covis::Pair *)W.pairs.p, n_pairs, opt->near_z,
                     opt->depth_sigmas, (unsigned *)W.out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(W.ev[1], st));
  HIP_TRY(hipMemcpyAsync(out, W.out.p, out_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
  W.device_ms = ms;
  return DVO_AMD_OK;
}

double overlap_of(const dvo_amd_covisibility_counts &c) { return c.valid ? (double)c.consistent / (double)c.valid : 0.0; }

}  // namespace

void covis_workspace_release(dvo_amd_context *ctx) {
  CovisWorkspace *w = ctx->covis_ws;
  if (!w) return;
  if (w->pairs.p) (void)hipFree(w->pairs.p);
  if (w->out.p) (void)hipFree(w->out.p);
  for (hipEvent_t e : w->ev)
    if (e) (void)hipEventDestroy(e);
  delete w;
  ctx->covis_ws = nullptr;
}

}  // namespace host
}  // namespace dvo_amd

extern "C" {

void dvo_amd_default_covisibility_options(dvo_amd_covisibility_options *opt) {
  if (!opt) return;
  opt->level = 3, opt->near_z = 0.1f, opt->depth_sigmas = 20.0f;
}

int dvo_amd_covisibility(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes,
                         const dvo_amd_covisibility_options *opt, int n_pairs, const int *pair_a, const int *pair_b,
                         dvo_amd_covisibility_counts *out) {
  return host::covisibility(ctx, n_keyframes, keyframes, opt, n_pairs, pair_a, pair_b, out, "dvo_amd_covisibility");
}

/* instrumentation: milliseconds k_covis took in the context's last dvo_amd_covisibility call (between two events) */
int dvo_amd_debug_covisibility_ms(const dvo_amd_context *ctx, double *device_ms) {
  if (!ctx || !device_ms) return DVO_AMD_ERR_INVALID_ARGUMENT;
  *device_ms = ctx->covis_ws ? ctx->covis_ws->device_ms : 0.0;
  return DVO_AMD_OK;
}

int dvo_amd_find_constraint_candidates(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes, int keyframe,
                                       float max_distance, double min_overlap, const dvo_amd_covisibility_options *opt,
                                       int *candidates, double *overlap, int capacity, int *n_out) {
  static const char *entry = "dvo_amd_find_constraint_candidates";
  if (n_out) *n_out = 0;
  if (!n_out || !keyframes || n_keyframes <= 0) return host::invalid(entry, "keyframes and n_out must be given");
  if (keyframe < 0 || keyframe >= n_keyframes) return host::invalid(entry, "the query keyframe is out of range");
  if (capacity < 0 || (capacity > 0 && !candidates)) return host::invalid(entry, "capacity without a candidate array");
  if (!std::isfinite(max_distance) || max_distance < 0.0f) return host::invalid(entry, "max_distance must be finite and >= 0");
  if (std::isnan(min_overlap)) return host::invalid(entry, "min_overlap is NaN");
  for (int k = 0; k < n_keyframes; ++k)
    if (!host::finite_all(keyframes[k].pose, 16)) return host::invalid(entry, "keyframe " + std::to_string(k) + " has a non-finite pose entry");
  const bool prune = min_overlap > 0.0;
  if (prune) {
    const int rc = host::check_options(entry, opt);
    if (rc) return rc;
  }
  // the radius stage: translations as floats (pcl::PointXYZ), d2 = ((dx dx + dy dy) + dz dz) <= r r in fp32, ascending index
  const double *Q = keyframes[keyframe].pose;
  const float qx = (float)Q[12], qy = (float)Q[13], qz = (float)Q[14];
  const float r2 = max_distance * max_distance;
  std::vector<int> found;
  for (int k = 0; k < n_keyframes; ++k) {
    const float dx = (float)keyframes[k].pose[12] - qx, dy = (float)keyframes[k].pose[13] - qy, dz = (float)keyframes[k].pose[14] - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 <= r2) found.push_back(k);
  }
  std::vector<double> best(found.size(), std::numeric_limits<double>::quiet_NaN());
  if (prune) {
    const size_t m = found.size();
    std::vector<int> pa(2 * m), pb(2 * m);
    for (size_t i = 0; i < m; ++i) pa[2 * i] = keyframe, pb[2 * i] = found[i], pa[2 * i + 1] = found[i], pb[2 * i + 1] = keyframe;
    std::vector<dvo_amd_covisibility_counts> counts(2 * m);
    const int rc = host::covisibility(ctx, n_keyframes, keyframes, opt, (int)(2 * m), pa.data(), pb.data(), counts.data(), entry);
    if (rc) return rc;
    size_t kept = 0;
    for (size_t i = 0; i < m; ++i) {
      const double o = std::max(host::overlap_of(counts[2 * i]), host::overlap_of(counts[2 * i + 1]));
      if (o >= min_overlap) found[kept] = found[i], best[kept] = o, ++kept;
    }
    found.resize(kept);
  }
  *n_out = (int)found.size();
  if ((int)found.size() > capacity) return DVO_AMD_ERR_CAPACITY;
  for (size_t i = 0; i < found.size(); ++i) {
    candidates[i] = found[i];
    if (overlap) overlap[i] = best[i];
  }
  return DVO_AMD_OK;
}

}  // extern "C"
