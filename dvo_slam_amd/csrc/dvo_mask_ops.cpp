// Operations on selection masks, all on the device: a mask from one or two masks (dvo_amd_mask_combine), from a mask grown or
// shrunk by a square window (dvo_amd_mask_morph), and from a mask carried onto another frame's pixels through the two frames'
// depth (dvo_amd_mask_warp / _warp_many).  The third producer of masks next to dvo_mask.cpp and dvo_budget.cpp: every result is
// an ordinary dvo_amd_mask (mask_alloc / mask_finish), the inputs are only read.  The rules are pinned in include/dvo_amd.h;
// tests/mask_ops_ref.py restates them in numpy.
//
//   k_mask_combine   ONE launch over all levels: blockIdx.y = the level, a lane owns four consecutive bytes (a level's pixel
//                    count is a multiple of 4 and its plane is 256-byte aligned), one 32-bit load per input and one 32-bit store
//   k_mask_morph     ONE launch over all levels (blockIdx.z = the level, each with its own radius), no scratch plane and no LDS:
//                    both axes of the window in one pass.  A block owns a tile of 64 columns x 64 rows, a wave 16 of
//                    its rows.  A wave reads the rows its window reaches, row by row; the 64 pixels of a row under the wave and
//                    the 64 on either side become three 64-bit ballots, of which every lane tests the bits of its own clipped
//                    row window (radius <= 64: never beyond the neighbouring 64).  The row answers of a lane's column pile up as
//                    bits of a 192-bit string in the lane's registers (16 + 2 * 64 rows at most), and an output pixel is a range
//                    test on that string.  Erode is dilate of the complement: input and output bits are flipped, and a pixel
//                    outside the plane is 0 in either form -- it has no vote.
//   k_mask_warp      ONE launch over all (pair, level) records of a call: blockIdx.y walks the records, striding by gridDim.y,
//                    blockIdx.x a chunk of the target level.  A lane owns four consecutive target pixels (one row: widths are
//                    multiples of 4): one float4 depth load, k_covis's arithmetic per pixel, the source depth and the source
//                    mask byte as data-dependent gathers, one 32-bit store of four mask bytes.
// kept[] and the warp's eight counts: ballots and popcounts per wave, LDS per block, one integer atomicAdd per non-zero count --
// integers only, so nothing depends on the launch geometry or on the order atomics land in.  One synchronisation per call
// (mask_finish's), on the device's prep stream.
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>

namespace dvo_amd {
namespace mask_ops {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLanePixels = 4;                  // combine, warp: pixels per lane
constexpr int kChunk = kBlock * kLanePixels;    // ... and per block
constexpr int kMorphCols = 64;                  // morph: a wave's columns
constexpr int kMorphWaveRows = 16;              // ... and rows
constexpr int kMorphRows = kMorphWaveRows * kWaves;
static_assert(kMorphWaveRows + 2 * DVO_AMD_MASK_MAX_RADIUS <= 192, "a lane's column string holds the rows a wave's window reaches");
static_assert(DVO_AMD_MASK_MAX_RADIUS <= 64, "a row window reaches no further than the neighbouring 64 pixels");
constexpr int kWarpCounts = 8;  // valid, behind, outside, no_depth, consistent, occluded, seen_through, dropped_by_source

// ---- combine

struct CombineLevels {
  const unsigned char *a[DVO_AMD_MAX_LEVELS], *b[DVO_AMD_MAX_LEVELS];  // b: null for NOT
  unsigned char *out[DVO_AMD_MAX_LEVELS];
  int n[DVO_AMD_MAX_LEVELS];
  int *kept;  // [levels]
};

// every non-zero byte of a word as 1
__device__ __forceinline__ unsigned normalised(unsigned v) {
  v |= v >> 4, v |= v >> 2, v |= v >> 1;
  return v & 0x01010101u;
}

// the kept pixels of four bytes of 0 / 1 per lane: a ballot per byte, one integer atomic per wave (every lane gets here)
__device__ __forceinline__ void count_kept4(unsigned word, int *kept) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c += __popcll(__ballot((word >> (8 * k)) & 1u));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(kept, c);
}

__global__ void __launch_bounds__(kBlock) k_mask_combine(CombineLevels L, int op) {
  const int l = blockIdx.y;
  const int n = L.n[l];
  if (blockIdx.x * kChunk >= n) return;  // (block-uniform)
  const int i = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
  unsigned r = 0u;
  if (i < n) {
    const unsigned a = normalised(*(const unsigned *)(L.a[l] + i));
    const unsigned b = op == DVO_AMD_MASK_NOT ? 0u : normalised(*(const unsigned *)(L.b[l] + i));
    r = op == DVO_AMD_MASK_AND ? (a & b) : op == DVO_AMD_MASK_OR ? (a | b) : op == DVO_AMD_MASK_ANDNOT ? (a & ~b) : (~a & 0x01010101u);
    *(unsigned *)(L.out[l] + i) = r;
  }
  count_kept4(r, L.kept + l);
}

// ---- morph

// bits lo..hi of a 64-bit word (any ints: an empty or outlying range is 0)
__device__ __forceinline__ unsigned long long bit_range(int lo, int hi) {
  if (hi < 0 || lo > 63 || hi < lo) return 0ull;
  lo = lo < 0 ? 0 : lo, hi = hi > 63 ? 63 : hi;
  return (~0ull >> (63 - hi)) & (~0ull << lo);
}

struct MorphLevels {
  const unsigned char *src[DVO_AMD_MAX_LEVELS];
  unsigned char *dst[DVO_AMD_MAX_LEVELS];
  int w[DVO_AMD_MAX_LEVELS], h[DVO_AMD_MAX_LEVELS], r[DVO_AMD_MAX_LEVELS];
  int *kept;  // [levels]
};

__global__ void __launch_bounds__(kBlock) k_mask_morph(MorphLevels L, int erode) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = blockIdx.z;  // the grid is level 0's: a coarser level leaves the blocks beyond its tiles idle
  const int w = L.w[l], h = L.h[l], r = L.r[l];
  const unsigned char *__restrict__ src = L.src[l];
  unsigned char *__restrict__ dst = L.dst[l];
  const int x0 = blockIdx.x * kMorphCols, y0 = blockIdx.y * kMorphRows + wave * kMorphWaveRows;
  if (x0 >= w || y0 >= h) return;  // (the whole wave: no barrier in this kernel)
  const int x = x0 + lane;
  // the lane's row window in the 192 pixels x0 - 64 .. x0 + 127, of which the lane is pixel 64 + lane
  const unsigned long long m_left = bit_range(lane - r + 64, lane + r + 64), m_mid = bit_range(lane - r, lane + r),
                           m_right = bit_range(lane - r - 64, lane + r - 64);
  const int j0 = y0 - r;  // the row that is bit 0 of the column string
  const int jlo = j0 < 0 ? 0 : j0;
  const int jhi = y0 + kMorphWaveRows - 1 + r < h - 1 ? y0 + kMorphWaveRows - 1 + r : h - 1;
  unsigned long long c0 = 0ull, c1 = 0ull, c2 = 0ull;
  for (int j = jlo; j <= jhi; ++j) {  // (wave-uniform bounds: every lane reaches every ballot)
    const unsigned char *row = src + (size_t)j * (size_t)w;
    const bool mid = x < w && (row[x] != 0) != (erode != 0);
    bool left = false, right = false;
    if (r > 0) {
      left = x - 64 >= 0 && x - 64 < w && (row[x - 64] != 0) != (erode != 0);
      right = x + 64 < w && (row[x + 64] != 0) != (erode != 0);
    }
    const unsigned long long b_mid = __ballot(mid), b_left = __ballot(left), b_right = __ballot(right);
    const unsigned long long any = ((b_left & m_left) | (b_mid & m_mid) | (b_right & m_right)) != 0ull ? 1ull : 0ull;
    const int t = j - j0;  // 0 .. kMorphWaveRows - 1 + 2 r
    const unsigned long long bit = any << (t & 63);
    if (t < 64) c0 |= bit;
    else if (t < 128) c1 |= bit;
    else c2 |= bit;
  }
  int count = 0;
  for (int t = 0; t < kMorphWaveRows; ++t) {
    const int y = y0 + t;
    if (y >= h) break;  // (wave-uniform)
    const int lo = t, hi = t + 2 * r;
    const bool any = ((c0 & bit_range(lo, hi)) | (c1 & bit_range(lo - 64, hi - 64)) | (c2 & bit_range(lo - 128, hi - 128))) != 0ull;
    const bool keep = x < w && any != (erode != 0);
    if (x < w) dst[(size_t)y * (size_t)w + x] = keep ? 1 : 0;
    count += __popcll(__ballot(keep));
  }
  if (lane == 0 && count) atomicAdd(L.kept + l, count);
}

// ---- warp

// one (pair, level) as the kernel reads it
struct WarpRecord {
  const float *zt, *txt, *tyt;   // target: depth plane and rays of the level
  const float *zs;               // source: depth plane of the level
  const unsigned char *ms;       // the mask's plane of the level (on the source's pixels)
  unsigned char *out;            // the result's plane of the level (on the target's pixels)
  int *kept;                     // the result's counter of the level
  unsigned *counts;              // [kWarpCounts]
  int wt, nt;                    // target: width, pixels
  int ws, hs;                    // source: size
  float fx, fy, ox, oy;          // source: intrinsics
  float T[12];                   // rows 0..2 of the transformation target -> source, row-major
};

__global__ void __launch_bounds__(kBlock) k_mask_warp(const WarpRecord *__restrict__ records, int n_records, float near_z, float sigmas,
                                                      int unseen_keep, int inconsistent_keep) {
  __shared__ unsigned s_cnt[kWaves][kWarpCounts + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rec = blockIdx.y; rec < n_records; rec += gridDim.y) {
    const WarpRecord R = records[rec];  // uniform over the block
    if (blockIdx.x * kChunk >= R.nt) continue;  // (block-uniform: no barrier is skipped by part of a block)
    const int p0 = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
    const bool live = p0 < R.nt;  // (nt is a multiple of 4: four pixels or none, all in one row)
    float z4[kLanePixels] = {0.f, 0.f, 0.f, 0.f};
    int v = 0, u0 = 0;
    float ty = 0.f;
    if (live) {
      const float4 z = *(const float4 *)(R.zt + p0);
      z4[0] = z.x, z4[1] = z.y, z4[2] = z.z, z4[3] = z.w;
      v = p0 / R.wt, u0 = p0 - v * R.wt;
      ty = R.tyt[v];
    }
    unsigned cnt[kWarpCounts + 1] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    unsigned word = 0u;
#pragma unroll
    for (int k = 0; k < kLanePixels; ++k) {
      int cls = -1;  // -1: no pixel or no depth; else the index of the outcome's count
      bool keep = false, dropped = false;
      if (live) {
        const float z = z4[k];
        keep = unseen_keep != 0;  // (what is not seen: no depth here, behind, outside, no depth there)
        size_t at;
        if (rules::finite_f(z))
          cls = rules::classify_covisible(z, R.txt[u0 + k], ty, R.T, near_z, sigmas, R.zs, R.ws, R.hs, R.fx, R.fy, R.ox, R.oy, at);
        if (cls == 4) {
          keep = R.ms[at] != 0;
          dropped = !keep;
        } else if (cls >= 5) {
          keep = inconsistent_keep != 0;
        }
      }
      word |= keep ? (1u << (8 * k)) : 0u;
      cnt[0] += (unsigned)__popcll(__ballot(cls >= 0));
#pragma unroll
      for (int c = 1; c < 7; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
      cnt[7] += (unsigned)__popcll(__ballot(dropped));
      cnt[8] += (unsigned)__popcll(__ballot(keep));
    }
    if (live) *(unsigned *)(R.out + p0) = word;
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c <= kWarpCounts; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x <= kWarpCounts) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
      if (sum) {
        if (threadIdx.x < kWarpCounts) atomicAdd(R.counts + threadIdx.x, sum);
        else atomicAdd(R.kept, (int)sum);
      }
    }
    __syncthreads();  // s_cnt is written again for the block's next record
  }
}

}  // namespace mask_ops
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::mask_ops;

namespace {

// dvo_amd_debug_mask_ops_timing: two events around the launches of a call on the prep stream (off unless asked for)
DeviceTiming g_timing[kMaxDevices];

// dvo_amd_mask_warp_many: the record table and the counts of the call in flight (grown to the largest call and kept; used with
// the device's mutex held from the table's upload to the last thing enqueued that touches it)
DeviceBuf g_warp_area[kMaxDevices];

void drop(dvo_amd_mask *m) {
  (void)hipFree(m->mem);
  delete m;
}

int check_warp_options(const char *entry, const dvo_amd_mask_warp_options *opt) {
  if (!opt) return invalid(entry, "the options are NULL");
  if (!std::isfinite(opt->near_z) || !(opt->near_z > 0.0f)) return invalid(entry, "near_z must be finite and positive");
  if (!std::isfinite(opt->depth_sigmas) || opt->depth_sigmas < 0.0f) return invalid(entry, "depth_sigmas must be finite and >= 0");
  return DVO_AMD_OK;
}

int warp_many(const char *entry, int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *sources,
              const dvo_amd_pyramid *const *targets, const double *T, const dvo_amd_mask_warp_options *opt, dvo_amd_mask **out,
              long long *counts) {
  if (out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative count");
  if (!masks || !sources || !targets || !T || !opt || !out) return invalid(entry, "a NULL pointer");
  int rc = check_warp_options(entry, opt);
  if (rc) return rc;
  size_t n_records = 0;
  for (int k = 0; k < n; ++k) {
    const std::string pair = "pair " + std::to_string(k);
    if (!masks[k] || !sources[k] || !targets[k]) return invalid(entry, pair + ": a NULL mask or pyramid");
    if (!finite_all(T + 16 * (size_t)k, 16)) return invalid(entry, pair + ": the transformation has a non-finite entry");
    if (sources[k]->n_levels < targets[k]->n_levels)
      return invalid(entry, pair + ": the source has " + std::to_string(sources[k]->n_levels) + " levels but the target has " +
                                std::to_string(targets[k]->n_levels));
    rc = mask_fits(entry, sources[k], masks[k]);
    if (rc == DVO_AMD_ERR_INVALID_ARGUMENT) return rc;
    rc = check_mask_size(entry, targets[k]->lv[0].w, targets[k]->lv[0].h, targets[k]->n_levels);
    if (rc) return rc;
    n_records += (size_t)targets[k]->n_levels;
  }
  for (int k = 0; k < n; ++k)
    if (masks[k]->device != targets[0]->device || sources[k]->device != targets[0]->device || targets[k]->device != targets[0]->device)
      return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;
  if (n_records > (size_t)(1 << 24)) return invalid(entry, "more than 2^24 (pair, level) records");

  const int device = targets[0]->device;
  std::vector<dvo_amd_mask *> made((size_t)n, nullptr);
  hipStream_t st = nullptr;
  auto unwind = [&](int status) {
    if (st) (void)hipStreamSynchronize(st);
    for (dvo_amd_mask *m : made)
      if (m) drop(m);
    return status;
  };
  Bracket bracket(g_timing[device]);
  for (int k = 0; k < n; ++k) {
    const dvo_amd_pyramid *t = targets[k];
    rc = mask_alloc(entry, device, t->lv[0].w, t->lv[0].h, t->n_levels, &made[(size_t)k], &st);
    if (rc) return unwind(rc);
  }
  // The record table and the counts live in the device's one warp area, which the next call overwrites: the device's mutex is held
  // from the upload to the last thing enqueued that reads or writes the area, so that two threads' calls reach the prep stream one
  // after the other (pyramid_build_batch does the same for its frame table).  mask_alloc above took and released it on its own.
  const size_t table_bytes = align_up(sizeof(WarpRecord) * n_records, 256), count_bytes = sizeof(unsigned) * kWarpCounts * n_records;
  std::unique_lock<std::mutex> area_lock(device_mutex(device));
  DeviceBuf &area = g_warp_area[device];
  rc = grow(area, table_bytes + count_bytes, 1 << 16, "warp table");
  if (rc) {
    area_lock.unlock();
    return unwind(rc);
  }
  void *scratch = area.p;
  unsigned *d_counts = (unsigned *)((char *)scratch + table_bytes);
  hipError_t e = hipSuccess;
  std::vector<WarpRecord> table(n_records);
  int max_nt = 1;
  size_t r = 0;
  for (int k = 0; k < n; ++k) {
    const double *Tk = T + 16 * (size_t)k;
    for (int l = 0; l < targets[k]->n_levels; ++l, ++r) {
      const LevelData &A = targets[k]->lv[l], &B = sources[k]->lv[l];
      WarpRecord &R = table[r];
      R.zt = A.z_plane, R.txt = A.tx, R.tyt = A.ty, R.zs = B.z_plane;
      R.ms = masks[k]->plane[l], R.out = made[(size_t)k]->plane[l], R.kept = made[(size_t)k]->counters + l;
      R.counts = d_counts + kWarpCounts * r;
      R.wt = A.w, R.nt = A.w * A.h, R.ws = B.w, R.hs = B.h;
      R.fx = B.fx, R.fy = B.fy, R.ox = B.ox, R.oy = B.oy;
      rows_from_column_major(Tk, R.T);
      max_nt = std::max(max_nt, R.nt);
    }
  }
  std::vector<unsigned> h_counts(counts ? kWarpCounts * n_records : 0);
  std::vector<int> h_kept((size_t)n * DVO_AMD_MAX_LEVELS, 0);
  e = bracket.begin(st);
  if (e == hipSuccess) e = hipMemcpyAsync(scratch, table.data(), sizeof(WarpRecord) * n_records, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) {
    const unsigned gx = (unsigned)((max_nt + kChunk - 1) / kChunk);
    const unsigned gy = grid_rows((long long)n_records, gx, kBlock);  // a block takes further records in steps of gridDim.y
    hipLaunchKernelGGL(k_mask_warp, dim3(gx, gy), dim3(kBlock), 0, st, (const WarpRecord *)scratch, (int)n_records, opt->near_z,
                       opt->depth_sigmas, opt->unseen_keep, opt->inconsistent_keep);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), d_counts, count_bytes, hipMemcpyDeviceToHost, st);
  // every mask but the last hands its counters over here; the last goes through mask_finish, which drains the stream for all
  for (int k = 0; k + 1 < n && e == hipSuccess; ++k)
    e = hipMemcpyAsync(h_kept.data() + (size_t)k * DVO_AMD_MAX_LEVELS, made[(size_t)k]->counters, sizeof(int) * made[(size_t)k]->levels,
                       hipMemcpyDeviceToHost, st);
  area_lock.unlock();
  dvo_amd_mask *last = made[(size_t)n - 1];
  made[(size_t)n - 1] = nullptr;  // (mask_finish owns it from here: on failure it is gone)
  dvo_amd_mask *finished = nullptr;
  rc = mask_finish(last, e, st, &finished);
  if (rc) return unwind(rc);
  made[(size_t)n - 1] = finished;
  bracket.read();
  for (int k = 0; k + 1 < n; ++k)
    for (int l = 0; l < made[(size_t)k]->levels; ++l) made[(size_t)k]->kept[l] = h_kept[(size_t)k * DVO_AMD_MAX_LEVELS + l];
  if (counts)
    for (size_t i = 0; i < h_counts.size(); ++i) counts[i] = (long long)h_counts[i];
  for (int k = 0; k < n; ++k) out[k] = made[(size_t)k];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

int dvo_amd_mask_combine(const dvo_amd_mask *a, const dvo_amd_mask *b, int op, dvo_amd_mask **out) {
  static const char *entry = "dvo_amd_mask_combine";
  if (out) *out = nullptr;
  if (!a || !out) return invalid(entry, "a NULL pointer");
  if (op != DVO_AMD_MASK_AND && op != DVO_AMD_MASK_OR && op != DVO_AMD_MASK_ANDNOT && op != DVO_AMD_MASK_NOT)
    return invalid(entry, "op must be DVO_AMD_MASK_AND, _OR, _ANDNOT or _NOT");
  if (op == DVO_AMD_MASK_NOT && b) return invalid(entry, "b must be NULL for DVO_AMD_MASK_NOT");
  if (op != DVO_AMD_MASK_NOT && !b) return invalid(entry, "b is NULL");
  if (b) {
    if (a->w != b->w || a->h != b->h)
      return invalid(entry, "a is " + std::to_string(a->w) + "x" + std::to_string(a->h) + " but b is " + std::to_string(b->w) + "x" +
                                std::to_string(b->h));
    if (a->levels != b->levels)
      return invalid(entry, "a has " + std::to_string(a->levels) + " levels but b has " + std::to_string(b->levels));
    if (a->device != b->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  }
  dvo_amd_mask *m = nullptr;
  hipStream_t st;
  const int rc = mask_alloc(entry, a->device, a->w, a->h, a->levels, &m, &st);
  if (rc) return rc;
  Bracket bracket(g_timing[a->device]);
  CombineLevels L = {};
  for (int l = 0; l < a->levels; ++l) {
    L.a[l] = a->plane[l], L.b[l] = b ? b->plane[l] : nullptr, L.out[l] = m->plane[l];
    L.n[l] = (a->w >> l) * (a->h >> l);
  }
  L.kept = m->counters;
  hipError_t e = bracket.begin(st);
  if (e == hipSuccess) {
    // (level 0 is the largest: at most 2^30 pixels, 2^20 blocks)
    hipLaunchKernelGGL(k_mask_combine, dim3((unsigned)((L.n[0] + kChunk - 1) / kChunk), (unsigned)a->levels), dim3(kBlock), 0, st, L, op);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  const int status = mask_finish(m, e, st, out);
  if (!status) bracket.read();
  return status;
}

int dvo_amd_mask_morph(const dvo_amd_mask *mask, int op, const int *radius, dvo_amd_mask **out) {
  static const char *entry = "dvo_amd_mask_morph";
  if (out) *out = nullptr;
  if (!mask || !radius || !out) return invalid(entry, "a NULL pointer");
  if (op != DVO_AMD_MASK_DILATE && op != DVO_AMD_MASK_ERODE) return invalid(entry, "op must be DVO_AMD_MASK_DILATE or DVO_AMD_MASK_ERODE");
  for (int l = 0; l < mask->levels; ++l)
    if (radius[l] < 0 || radius[l] > DVO_AMD_MASK_MAX_RADIUS)
      return invalid(entry, "radius[" + std::to_string(l) + "] is outside 0.." + std::to_string(DVO_AMD_MASK_MAX_RADIUS));
  dvo_amd_mask *m = nullptr;
  hipStream_t st;
  const int rc = mask_alloc(entry, mask->device, mask->w, mask->h, mask->levels, &m, &st);
  if (rc) return rc;
  Bracket bracket(g_timing[mask->device]);
  MorphLevels L = {};
  for (int l = 0; l < mask->levels; ++l) {
    L.src[l] = mask->plane[l], L.dst[l] = m->plane[l];
    L.w[l] = mask->w >> l, L.h[l] = mask->h >> l, L.r[l] = radius[l];
  }
  L.kept = m->counters;
  hipError_t e = bracket.begin(st);
  if (e == hipSuccess) {
    // (level 0 is the largest; its height is at most 65535 rows: check_mask_size)
    hipLaunchKernelGGL(k_mask_morph,
                       dim3((unsigned)((mask->w + kMorphCols - 1) / kMorphCols), (unsigned)((mask->h + kMorphRows - 1) / kMorphRows),
                            (unsigned)mask->levels),
                       dim3(kBlock), 0, st, L, op == DVO_AMD_MASK_ERODE ? 1 : 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  const int status = mask_finish(m, e, st, out);
  if (!status) bracket.read();
  return status;
}

void dvo_amd_default_mask_warp_options(dvo_amd_mask_warp_options *opt) {
  if (!opt) return;
  opt->near_z = 0.1f, opt->depth_sigmas = 20.0f, opt->unseen_keep = 1, opt->inconsistent_keep = 1;
}

int dvo_amd_mask_warp_many(int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *sources,
                           const dvo_amd_pyramid *const *targets, const double *T, const dvo_amd_mask_warp_options *opt,
                           dvo_amd_mask **out, long long *counts) {
  return warp_many("dvo_amd_mask_warp_many", n, masks, sources, targets, T, opt, out, counts);
}

int dvo_amd_mask_warp(const dvo_amd_mask *mask, const dvo_amd_pyramid *source, const dvo_amd_pyramid *target, const double *T,
                      const dvo_amd_mask_warp_options *opt, dvo_amd_mask **out, long long *counts) {
  static const char *entry = "dvo_amd_mask_warp";
  if (out) *out = nullptr;
  if (!mask || !source || !target || !T || !opt || !out) return invalid(entry, "a NULL pointer");
  return warp_many(entry, 1, &mask, &source, &target, T, opt, out, counts);
}

/* instrumentation: with enable != 0 every later dvo_amd_mask_combine / _morph / _warp / _warp_many on `device` is bracketed by two
 * events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent bracketed call */
int dvo_amd_debug_mask_ops_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
