// Exposure compensation on the device: the gain and bias between two frames of an auto-exposing camera, fitted over the pixels
// both frames see, and a frame's intensity adjusted by them.
//   dvo_amd_estimate_exposure / _many          I_ref ~ gain * I_cur + bias at ONE level of a (reference, current) pair, by trimmed
//                                              least squares over exact integer sums
//   dvo_amd_pyramid_adjust_intensity / _many   a new ordinary pyramid whose level-0 intensity is (gain * I) + bias
// The rule is pinned operation by operation in include/dvo_amd.h ("Exposure compensation"); tests/exposure_ref.py restates it.
//
//   k_exposure   ONE launch per pass over all pairs of a call: blockIdx.y = the pair, blockIdx.x = a chunk of the reference level's
//                pixels.  Every pixel with a depth is moved into the current frame and classified against the current's depth
//                plane -- dvo_amd_mask_warp's rule, operation for operation --, a consistent pixel reads its mask byte, its own
//                intensity and the current's at the landing pixel (a nearest gather), and a candidate that the pass uses adds its
//                quantised pair to the lane's 64-bit integer sums.  Counts are ballots and popcounts per wave; the five sums are
//                reduced over the wave by shuffles, over the block through LDS, and go out as one 64-bit integer vector atomic per
//                non-zero word and block.  Integers only: no value depends on the geometry or on the order the atomics land in.
//   k_adjust     ONE launch over all pyramids of a call, four pixels per thread; a block finds its pyramid by its index in the
//                records' block ranges (block-uniform).
// The host solves each pass from the six sums in 128-bit integers (dvo_exposure_solve.h) and hands gain and bias, as floats, to the
// next pass: a call is refits_max + 1 launches and as many synchronisations, whatever number of pairs it holds.
#include "dvo_internal.h"
#include "dvo_device_rules.h"
#include "dvo_exposure_solve.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

namespace dvo_amd {
namespace exposure {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSteps = 4;                // pixels per lane: a wave walks kSteps runs of 64 consecutive pixels
constexpr int kChunk = kBlock * kSteps;  // pixels of the reference level per block
// the words of one (pass, pair): the seven covisibility counts, masked, saturated, candidates, trimmed, then n, sx, sy, sxx, sxy, syy
constexpr int kCounts = 12;  // ... of which the first twelve are counts of pixels (n, the pixels the pass uses, is the twelfth)
constexpr int kWords = 17;
constexpr int kWordsPad = 24;
constexpr int kAdjustPixels = 4;
static_assert(kBlock % 64 == 0, "whole waves");
static_assert(DVO_AMD_EXPOSURE_MAX_REFITS == 8, "the header's bound: gain_pass[9]");


// one pair as the kernel reads it (uniform over the block: scalar registers)
struct Pair {
  const float *zr, *txr, *tyr, *ir;  // reference: depth plane, rays and intensity plane of the level
  const float *zc, *ic;              // current: depth and intensity plane of the level
  const unsigned char *mask;         // the mask's plane of the level on the reference's pixels, or null
  int wr, nr;                        // reference: width, pixels
  int wc, hc;                        // current: size
  float fx, fy, ox, oy;              // current: intrinsics
  float T[12];                       // rows 0..2 of reference -> current, row-major, cast from double
  float near_z, sigmas, lo, hi, scale, trim;
};

// what a pass knows of a pair: whether the pair takes part in it, and the fit of the pass before it
struct PassState {
  float gain, bias;
  int active, trimming;
};

__global__ void __launch_bounds__(kBlock) k_exposure(const Pair *__restrict__ pairs, const PassState *__restrict__ states, int n_pairs,
                                                     unsigned long long *__restrict__ out) {
  __shared__ unsigned long long s_v[kWaves][kWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int pair = blockIdx.y; pair < n_pairs; pair += gridDim.y) {
    const PassState S = states[pair];
    if (!S.active) continue;  // (block-uniform: no barrier is skipped by part of a block)
    const Pair P = pairs[pair];
    if (blockIdx.x * kChunk >= P.nr) continue;
    const int base = blockIdx.x * kChunk + wave * (kSteps * 64);
    unsigned cnt[kCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    long long sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      const int p = base + k * 64 + lane;
      int cls = -1;  // -1: no pixel or no depth; 1..6 the outcome's count; 7 masked, 8 saturated, 9 candidate
      bool trimmed = false, used = false;
      if (p < P.nr) {
        const float z = P.zr[p];
        size_t at;
        if (rules::finite_f(z)) {
          const int v = p / P.wr, u = p - v * P.wr;
          cls = rules::classify_covisible(z, P.txr[u], P.tyr[v], P.T, P.near_z, P.sigmas, P.zc, P.wc, P.hc, P.fx, P.fy, P.ox, P.oy, at);
        }
        if (cls == 4) {
          if (P.mask && P.mask[p] == 0) {
            cls = 7;
          } else {
            const float iy = P.ir[p], ix = P.ic[at];
            if (!(ix >= P.lo && ix <= P.hi && iy >= P.lo && iy <= P.hi)) {  // (false for a NaN)
              cls = 8;
            } else {
              cls = 9;
              used = !S.trimming || fabsf((S.gain * ix + S.bias) - iy) <= P.trim;
              trimmed = !used;
              if (used) {
                const long long X = (long long)rintf(ix * P.scale), Y = (long long)rintf(iy * P.scale);
                sx += X, sy += Y, sxx += X * X, sxy += X * Y, syy += Y * Y;
              }
            }
          }
        }
      }
      cnt[0] += (unsigned)__popcll(__ballot(cls >= 0));
#pragma unroll
      for (int c = 1; c <= 3; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
      cnt[4] += (unsigned)__popcll(__ballot(cls == 4 || cls >= 7));  // consistent: whatever happens to the pixel afterwards
      cnt[5] += (unsigned)__popcll(__ballot(cls == 5));
      cnt[6] += (unsigned)__popcll(__ballot(cls == 6));
      cnt[7] += (unsigned)__popcll(__ballot(cls == 7));
      cnt[8] += (unsigned)__popcll(__ballot(cls == 8));
      cnt[9] += (unsigned)__popcll(__ballot(cls == 9));
      cnt[10] += (unsigned)__popcll(__ballot(trimmed));
      cnt[11] += (unsigned)__popcll(__ballot(used));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      sx += __shfl_xor(sx, m, 64), sy += __shfl_xor(sy, m, 64);
      sxx += __shfl_xor(sxx, m, 64), sxy += __shfl_xor(sxy, m, 64), syy += __shfl_xor(syy, m, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kCounts; ++c) s_v[wave][c] = cnt[c];
      // (a negative sum travels as its two's complement: 64-bit adds wrap the same way signed or unsigned)
      s_v[wave][12] = (unsigned long long)sx, s_v[wave][13] = (unsigned long long)sy, s_v[wave][14] = (unsigned long long)sxx;
      s_v[wave][15] = (unsigned long long)sxy, s_v[wave][16] = (unsigned long long)syy;
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
      unsigned long long sum = 0ull;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_v[w][threadIdx.x];
      if (sum)
        (void)__hip_atomic_fetch_add((DVO_DEVICE_GLOBAL unsigned long long *)out + (size_t)pair * kWordsPad + threadIdx.x, sum, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();  // s_v is written again for the block's next pair
  }
}

// one pyramid of an adjust call as the kernel reads it (block-uniform)
struct AdjustRecord {
  const float *in;  // level 0's intensity plane (n pixels, tight rows; n is a multiple of 4)
  float *out;
  int n;
  int block_first, block_end;  // the pyramid's blocks are [block_first, block_end) of the launch
  float gain, bias;
  int pad;
};

__global__ void __launch_bounds__(kBlock) k_adjust(const AdjustRecord *__restrict__ records, int n_records) {
  int lo = 0, hi = n_records - 1;  // the first record whose block range ends behind this block (block-uniform)
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if ((int)blockIdx.x >= records[mid].block_end)
      lo = mid + 1;
    else
      hi = mid;
  }
  const AdjustRecord R = records[lo];
  const int p0 = (((int)blockIdx.x - R.block_first) * kBlock + (int)threadIdx.x) * kAdjustPixels;
  if (p0 >= R.n) return;  // (n is a multiple of 4: four pixels or none)
  const float4 i = *(const float4 *)(R.in + p0);
  float4 o;
  o.x = (R.gain * i.x) + R.bias, o.y = (R.gain * i.y) + R.bias, o.z = (R.gain * i.z) + R.bias, o.w = (R.gain * i.w) + R.bias;
  *(float4 *)(R.out + p0) = o;
}

}  // namespace exposure
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::exposure;

static_assert(sizeof(dvo_amd_exposure_estimate) == 392, "the record as include/dvo_amd.h lays it out");

namespace {

constexpr long long kMaxPixels = 1ll << 22;      // of the reference's level: sxx <= 2^22 * (2^20)^2 = 2^62
constexpr double kMaxQuantised = 1048576.0;      // |intensity bound| * scale <= 2^20

// dvo_amd_debug_exposure_timing: two events around every launch of a call on the prep stream, when asked for; a call's launches
// are added up
DeviceTiming g_timing[kMaxDevices];

int check_options(const char *entry, const std::string &pair, const dvo_amd_exposure_options &o) {
  if (!std::isfinite(o.near_z) || !(o.near_z > 0.0f)) return invalid(entry, pair + ": near_z must be finite and positive");
  if (!std::isfinite(o.depth_sigmas) || o.depth_sigmas < 0.0f) return invalid(entry, pair + ": depth_sigmas must be finite and >= 0");
  if (!std::isfinite(o.scale) || !(o.scale > 0.0f)) return invalid(entry, pair + ": scale must be finite and positive");
  if (!std::isfinite(o.min_intensity) || !std::isfinite(o.max_intensity) || !(o.min_intensity <= o.max_intensity))
    return invalid(entry, pair + ": min_intensity and max_intensity must be finite with min <= max");
  if (std::fabs((double)o.min_intensity) * (double)o.scale > kMaxQuantised || std::fabs((double)o.max_intensity) * (double)o.scale > kMaxQuantised)
    return invalid(entry, pair + ": an intensity bound times scale is beyond 2^20");
  if (!(o.trim > 0.0f)) return invalid(entry, pair + ": trim must be > 0 (+inf: no trimming)");
  if (o.refits < 0 || o.refits > DVO_AMD_EXPOSURE_MAX_REFITS)
    return invalid(entry, pair + ": refits is outside 0.." + std::to_string(DVO_AMD_EXPOSURE_MAX_REFITS));
  if (o.min_pairs < 2) return invalid(entry, pair + ": min_pairs must be at least 2");
  if (!std::isfinite(o.min_gain) || !std::isfinite(o.max_gain) || !(o.min_gain > 0.0) || !(o.min_gain <= o.max_gain))
    return invalid(entry, pair + ": min_gain and max_gain must be finite with 0 < min <= max");
  return DVO_AMD_OK;
}

int estimate_many(const char *entry, dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                  const dvo_amd_pyramid *const *currents, const double *T, const dvo_amd_mask *const *masks,
                  const dvo_amd_exposure_options *opts, dvo_amd_exposure_estimate *out) {
  if (n < 0) return invalid(entry, "a negative count (n < 0)");
  if (!ctx || !references || !currents || !opts || !out) return invalid(entry, "a NULL pointer");
  bool mismatch = false;
  int passes_max = 0;
  for (int k = 0; k < n; ++k) {
    const std::string pair = "pair " + std::to_string(k);
    const dvo_amd_pyramid *ref = references[k], *cur = currents[k];
    if (!ref || !cur) return invalid(entry, pair + ": a NULL pyramid");
    const dvo_amd_exposure_options &o = opts[k];
    const int l = o.level;
    if (l < 0 || l >= DVO_AMD_MAX_LEVELS || l >= ref->n_levels || l >= cur->n_levels)
      return invalid(entry, pair + ": level " + std::to_string(l) + " is out of range (the reference has " + std::to_string(ref->n_levels) +
                                " levels, the current " + std::to_string(cur->n_levels) + ")");
    if ((long long)ref->lv[l].w * ref->lv[l].h > kMaxPixels)
      return invalid(entry, pair + ": level " + std::to_string(l) + " of the reference is larger than 2^22 pixels");
    int rc = check_options(entry, pair, o);
    if (rc) return rc;
    if (T && !finite_all(T + 16 * (size_t)k, 16)) return invalid(entry, pair + ": the transformation has a non-finite entry");
    rc = mask_fits(entry, ref, masks ? masks[k] : nullptr);
    if (rc == DVO_AMD_ERR_INVALID_ARGUMENT) return rc;
    if (rc == DVO_AMD_ERR_DEVICE_MISMATCH || ref->device != ctx->device || cur->device != ctx->device) mismatch = true;
    passes_max = std::max(passes_max, o.refits + 1);
  }
  if (mismatch) return DVO_AMD_ERR_DEVICE_MISMATCH;
  int rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  const int device = ctx->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  // the call's own scratch: the pair table, the pass states, and one zeroed block of words per (pass, pair)
  const size_t pairs_bytes = align_up(sizeof(Pair) * (size_t)n, 256), states_bytes = align_up(sizeof(PassState) * (size_t)n, 256);
  const size_t pass_words = (size_t)kWordsPad * (size_t)n;
  const size_t sums_bytes = sizeof(unsigned long long) * pass_words * (size_t)passes_max;
  const size_t scratch_bytes = pairs_bytes + states_bytes + sums_bytes;
  std::vector<Pair> table((size_t)n);
  int max_nr = 1;
  for (int k = 0; k < n; ++k) {
    const dvo_amd_exposure_options &o = opts[k];
    const LevelData &A = references[k]->lv[o.level], &B = currents[k]->lv[o.level];
    Pair &P = table[(size_t)k];
    P.zr = A.z_plane, P.txr = A.tx, P.tyr = A.ty, P.ir = A.i_plane;
    P.zc = B.z_plane, P.ic = B.i_plane;
    P.mask = masks && masks[k] ? masks[k]->plane[o.level] : nullptr;
    P.wr = A.w, P.nr = A.w * A.h, P.wc = B.w, P.hc = B.h;
    P.fx = B.fx, P.fy = B.fy, P.ox = B.ox, P.oy = B.oy;
    rows_from_column_major(T ? T + 16 * (size_t)k : nullptr, P.T);  // (no T: the identity)
    P.near_z = o.near_z, P.sigmas = o.depth_sigmas, P.lo = o.min_intensity, P.hi = o.max_intensity, P.scale = o.scale, P.trim = o.trim;
    max_nr = std::max(max_nr, P.nr);
  }
  Scratch scratch;  // (every return below stands behind a synchronisation of the stream)
  rc = scratch.take(device, scratch_bytes);
  if (rc) return rc;
  char *base = scratch.base();
  const Pair *d_pairs = (const Pair *)base;
  PassState *d_states = (PassState *)(base + pairs_bytes);
  unsigned long long *d_sums = (unsigned long long *)(base + pairs_bytes + states_bytes);

  const unsigned gx = (unsigned)((max_nr + kChunk - 1) / kChunk);
  const unsigned gy = grid_rows(n, gx, kBlock);  // a block takes further pairs in steps of gridDim.y
  Bracket bracket(g_timing[device]);
  double device_ms = 0.0;

  std::vector<dvo_amd_exposure_estimate> made((size_t)n);  // (the outputs stay untouched until nothing can fail any more)
  std::vector<PassState> states((size_t)n);
  std::vector<char> done((size_t)n, 0);
  std::vector<unsigned long long> words(pass_words);
  for (int k = 0; k < n; ++k) {
    made[(size_t)k] = dvo_amd_exposure_estimate{};
    made[(size_t)k].gain = 1.0;
    states[(size_t)k] = PassState{1.0f, 0.0f, 1, 0};
  }
  hipError_t e = hipMemcpyAsync(base, table.data(), sizeof(Pair) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_sums, 0, sums_bytes, st);
  for (int pass = 0; pass < passes_max && e == hipSuccess; ++pass) {
    bool any = false;
    for (int k = 0; k < n; ++k) {
      PassState &S = states[(size_t)k];
      S.active = !done[(size_t)k] && pass <= opts[k].refits;
      S.trimming = pass > 0;
      any = any || S.active;
    }
    if (!any) break;
    unsigned long long *d_pass = d_sums + pass_words * (size_t)pass;
    e = hipMemcpyAsync(d_states, states.data(), sizeof(PassState) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = bracket.begin(st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_exposure, dim3(gx, gy), dim3(kBlock), 0, st, d_pairs, (const PassState *)d_states, n, d_pass);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = bracket.end(st);
    if (e == hipSuccess) e = hipMemcpyAsync(words.data(), d_pass, sizeof(unsigned long long) * pass_words, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the pass's one synchronisation
    if (e != hipSuccess) break;
    double pass_ms = 0.0;
    if (bracket.elapsed(&pass_ms)) device_ms += pass_ms;
    for (int k = 0; k < n; ++k) {
      if (!states[(size_t)k].active) continue;
      const unsigned long long *w = words.data() + (size_t)kWordsPad * (size_t)k;
      const dvo_amd_exposure_options &o = opts[k];
      dvo_amd_exposure_estimate &R = made[(size_t)k];
      if (pass == 0) {
        R.valid = (long long)w[0], R.behind = (long long)w[1], R.outside = (long long)w[2], R.no_depth = (long long)w[3];
        R.consistent = (long long)w[4], R.occluded = (long long)w[5], R.seen_through = (long long)w[6];
        R.masked = (long long)w[7], R.saturated = (long long)w[8], R.candidates = (long long)w[9];
      }
      R.trimmed = (long long)w[10], R.used = (long long)w[11];
      R.n = (long long)w[11], R.sx = (long long)w[12], R.sy = (long long)w[13], R.sxx = (long long)w[14], R.sxy = (long long)w[15];
      R.syy = (long long)w[16];
      const Fit f = solve(Sums{R.n, R.sx, R.sy, R.sxx, R.sxy, R.syy}, o.min_pairs, o.min_gain, o.max_gain, (double)o.scale);
      R.gain = f.gain, R.bias = f.bias, R.r2 = f.r2, R.degenerate = f.degenerate, R.passes = pass + 1;
      R.gain_pass[pass] = f.gain, R.bias_pass[pass] = f.bias, R.used_pass[pass] = R.used;
      if (f.degenerate) done[(size_t)k] = 1;
      states[(size_t)k].gain = (float)f.gain, states[(size_t)k].bias = (float)f.bias;
    }
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);  // (whatever failed, the stream is drained before the scratch goes back to the pool)
    return fail_hip("exposure estimate", e);
  }
  if (bracket.timed) bracket.store(device_ms);
  for (int k = 0; k < n; ++k) out[k] = made[(size_t)k];
  return DVO_AMD_OK;
}

int adjust_many(const char *entry, int n, const dvo_amd_pyramid *const *p, const double *gain, const double *bias, dvo_amd_pyramid **out) {
  if (out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative pyramid count (n < 0)");
  if (!p || !gain || !bias || !out) return invalid(entry, "a NULL pointer");
  for (int k = 0; k < n; ++k) {
    if (!p[k]) return invalid(entry, "pyramid " + std::to_string(k) + " is NULL");
    if (!std::isfinite(gain[k]) || !std::isfinite(bias[k])) return invalid(entry, "item " + std::to_string(k) + ": gain and bias must be finite");
  }
  for (int k = 0; k < n; ++k)
    if (p[k]->device != p[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  int rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  const size_t record_bytes = align_up(sizeof(AdjustRecord) * (size_t)n, 256);
  std::vector<size_t> plane_at((size_t)n);
  std::vector<AdjustRecord> table((size_t)n);
  size_t scratch_bytes = record_bytes;
  long long n_blocks = 0;
  for (int k = 0; k < n; ++k) {
    const LevelData &L = p[k]->lv[0];
    if ((long long)L.w * L.h > (1ll << 30)) return invalid(entry, "pyramid " + std::to_string(k) + ": level 0 is larger than 2^30 pixels");
    plane_at[(size_t)k] = scratch_bytes;
    scratch_bytes += align_up(sizeof(float) * (size_t)L.n, 256);
    AdjustRecord &R = table[(size_t)k];
    R = AdjustRecord{};
    R.n = L.w * L.h;
    R.block_first = (int)n_blocks;
    n_blocks += ((long long)R.n + kBlock * kAdjustPixels - 1) / (kBlock * kAdjustPixels);
    if (n_blocks > (1ll << 30)) return invalid(entry, "the call holds more than 2^30 blocks");
    R.block_end = (int)n_blocks;
    R.gain = (float)gain[k], R.bias = (float)bias[k];
  }
  const int device = p[0]->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  Scratch scratch;  // (every return below stands behind a synchronisation of the stream: the adjust's own, then pyramid_build's)
  rc = scratch.take(device, scratch_bytes);
  if (rc) return rc;
  char *base = scratch.base();
  for (int k = 0; k < n; ++k) {
    table[(size_t)k].in = p[k]->lv[0].i_plane;
    table[(size_t)k].out = (float *)(base + plane_at[(size_t)k]);
  }
  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemcpyAsync(base, table.data(), sizeof(AdjustRecord) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_adjust, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, (const AdjustRecord *)base, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  // the adjust's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("intensity adjustment", e);
  bracket.read();
  // every pyramid from its adjusted intensity plane and its own depth plane, by the builder every pyramid comes from
  for (int k = 0; k < n; ++k) {
    const LevelData &L = p[k]->lv[0];
    const PyramidSpec spec{L.w, L.h, L.fx, L.fy, L.ox, L.oy, p[k]->n_levels, p[k]->timestamp};
    const Level0Source src{(const float *)(base + plane_at[(size_t)k]), L.z_plane, L.w, nullptr, true};
    rc = pyramid_build(device, spec, src, &out[k]);
    if (rc) {
      for (int j = 0; j < k; ++j) dvo_amd_pyramid_release(out[j]), out[j] = nullptr;
      out[k] = nullptr;
      return rc;
    }
  }
  return DVO_AMD_OK;  // (pyramid_build drained the stream: nothing reads the scratch any more)
}

}  // namespace

extern "C" {

void dvo_amd_default_exposure_options(dvo_amd_exposure_options *opt) {
  if (!opt) return;
  opt->level = 0;
  opt->near_z = 0.1f, opt->depth_sigmas = 20.0f;
  opt->min_intensity = 4.0f, opt->max_intensity = 251.0f;
  opt->scale = 16.0f;
  opt->trim = 12.0f;
  opt->refits = 4;
  opt->min_pairs = 64;
  opt->min_gain = 0.25, opt->max_gain = 4.0;
}

int dvo_amd_estimate_exposure_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                                   const dvo_amd_pyramid *const *currents, const double *T, const dvo_amd_mask *const *masks,
                                   const dvo_amd_exposure_options *opts, dvo_amd_exposure_estimate *out) {
  return estimate_many("dvo_amd_estimate_exposure_many", ctx, n, references, currents, T, masks, opts, out);
}

int dvo_amd_estimate_exposure(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current, const double *T,
                              const dvo_amd_mask *mask, const dvo_amd_exposure_options *opt, dvo_amd_exposure_estimate *out) {
  static const char *entry = "dvo_amd_estimate_exposure";
  if (!ctx || !reference || !current || !opt || !out) return invalid(entry, "a NULL pointer");
  return estimate_many(entry, ctx, 1, &reference, &current, T, mask ? &mask : nullptr, opt, out);
}

int dvo_amd_pyramid_adjust_intensity_many(int n, const dvo_amd_pyramid *const *p, const double *gain, const double *bias,
                                          dvo_amd_pyramid **out) {
  return adjust_many("dvo_amd_pyramid_adjust_intensity_many", n, p, gain, bias, out);
}

int dvo_amd_pyramid_adjust_intensity(const dvo_amd_pyramid *p, double gain, double bias, dvo_amd_pyramid **out) {
  static const char *entry = "dvo_amd_pyramid_adjust_intensity";
  if (out) *out = nullptr;
  if (!p || !out) return invalid(entry, "a NULL pointer");
  return adjust_many(entry, 1, &p, &gain, &bias, out);
}

/* instrumentation: with enable != 0 every launch of a later dvo_amd_estimate_exposure / _many or dvo_amd_pyramid_adjust_intensity /
 * _many on `device` is bracketed by two events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent
 * bracketed call, its launches added up */
int dvo_amd_debug_exposure_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
