// Point-budget selection masks: a dvo_amd_mask built on the device from a resident pyramid, by one of two rules
//   TOPK   level l keeps its budget[l] strongest candidates
//   GRID   level l keeps the strongest candidate of every cell[l] x cell[l] cell
// "strongest" by the saliency s = Ix^2 + Iy^2 (+ depth_weight * (Zx^2 + Zy^2)), ordered by (bits(s) descending, pixel index
// ascending): a total order, so both rules are exact and the planes are a function of the pyramid and the options alone.  The
// rules are pinned in include/dvo_amd.h; tests/budget_selection_cases.py restates them in numpy.  The result is an ordinary mask
// (dvo_mask.cpp) and enters where every mask enters, the select kernel.
//
// Per level, on the device's prep stream:
//   k_budget_keys     28 B/px in (z, c_a, c_b; + 1 B/px of `within`), 4 B/px out: the key plane, kNoKey where no candidate
//   TOPK  4 x { k_budget_hist: the histogram of one 8-bit digit over the keys that share the digits found so far (LDS integer
//                              atomics per block, then the block's non-empty bins into the level's histogram, integer atomics)
//               k_budget_pick: one block: the digit in which the K-th largest key lies; the remaining count goes forward }
//         -> T, the K-th largest key, and r, how many pixels with key == T are kept
//         k_budget_ties / k_budget_ties_prefix / k_budget_topk_plane: keep key > T and the first r pixels with key == T in scan
//         order -- per-block tie counts and an exclusive prefix over them, the k_select / k_select_prefix / k_compact pattern
//         (dvo_kernels.hip); no atomic decides an order
//   GRID  k_budget_grid_lanes (cell <= kLaneCell: a lane per cell) or k_budget_grid_blocks (a block per cell: 256 lanes walk the
//         cell's rows, shuffle and LDS reduce the 64-bit (key, ~index) maximum) onto a zeroed plane
// 12 launches per level for TOPK, 2 for GRID; all counts are integers, so nothing depends on the launch geometry or on the order
// atomics land in.  K never meets |C| on the host: k_budget_pick of the first digit clamps it, so "every candidate" (K < 0,
// K >= |C|) is the ordinary path with T = the smallest key.  One synchronisation, mask_finish's.
#include "dvo_internal.h"

#include <cmath>
#include <string>

namespace dvo_amd {
namespace budget {

constexpr int kBlock = 256;
constexpr unsigned kNoKey = 0xffffffffu;  // a NaN's bit pattern: no saliency has it (a NaN saliency is no candidate)
constexpr int kMaxHistBlocks = 2048;      // k_budget_hist walks the level grid-stride beyond that
constexpr int kLaneCell = 8;              // GRID: cells up to this edge are walked by one lane each, larger ones by a block each
constexpr int kDigits = 4;                // 4 x 8 bits, most significant first

// the radix select's state of one level (device; zeroed before the level's first launch)
struct SelectState {
  unsigned hist[kDigits][256];
  unsigned prefix;     // the digits found so far, in place; after the last pick: T
  unsigned remaining;  // how many of the keys that share `prefix` are still to keep; after the last pick: r
  unsigned none;       // K clamped to 0: nothing is kept (T = kNoKey, r = 0)
  unsigned pad;
};

__device__ __forceinline__ int lane_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the kept pixels of a plane: one integer atomic per wave (every lane of the wave gets here)
__device__ __forceinline__ void count_kept(bool keep, int *kept) {
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(kept, __popcll(m));
}

__global__ __launch_bounds__(kBlock) void k_budget_keys(const float *__restrict__ zp, const float4 *__restrict__ c_a,
                                                        const float2 *__restrict__ c_b, const unsigned char *__restrict__ within,
                                                        int n, float ti, float td, float dw, unsigned *__restrict__ keys) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    const float z = zp[i];
    const float4 a = c_a[i];  // I, Z, Ix, Iy
    const float2 b = c_b[i];  // Zx, Zy
    bool ok = (z == z) && (b.x == b.x) && (b.y == b.y) &&
              (__builtin_fabsf(a.z) > ti || __builtin_fabsf(a.w) > ti || __builtin_fabsf(b.x) > td || __builtin_fabsf(b.y) > td);
    if (within) ok = ok && within[i] != 0;
    float s = a.z * a.z + a.w * a.w;                   // (-ffp-contract=off: every product and sum rounds by itself)
    if (dw != 0.0f) s = s + dw * (b.x * b.x + b.y * b.y);
    ok = ok && (s == s);
    keys[i] = ok ? __float_as_uint(s) : kNoKey;
  }
}

// digit `pass` (0: bits 31..24) of the keys whose higher digits are st->prefix's
__global__ __launch_bounds__(kBlock) void k_budget_hist(const unsigned *__restrict__ keys, int n, int pass, SelectState *st) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned prefix = st->prefix;
  for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
    const int i = base + threadIdx.x;
    if (i < n) {
      const unsigned k = keys[i];
      // (the first digit of kNoKey is 0xff and a key's is at most 0x7f: from the second pass on the prefix excludes it)
      const bool in = pass == 0 ? k != kNoKey : ((k ^ prefix) >> (shift + 8)) == 0u;
      if (in) atomicAdd(&sh[(k >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const unsigned c = sh[threadIdx.x];
  if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);
}

// one block: the digit d with  #(keys above d) < k <= #(keys at or above d)  among the keys that share the prefix
__global__ __launch_bounds__(kBlock) void k_budget_pick(SelectState *st, int pass, unsigned budget) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = st->hist[pass][threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned k = st->remaining;
    if (pass == 0) {  // the bins of the first digit hold every candidate: K meets |C| here, not on the host
      unsigned total = 0;
      for (int d = 0; d < 256; ++d) total += sh[d];
      k = budget < total ? budget : total;
      if (k == 0u) st->none = 1u, st->prefix = kNoKey, st->remaining = 0u;
    }
    if (!st->none) {
      unsigned above = 0;
      int d = 255;
      for (; d > 0; --d) {
        if (above + sh[d] >= k) break;
        above += sh[d];
      }
      st->prefix |= (unsigned)d << (24 - 8 * pass);
      st->remaining = k - above;
    }
  }
}

// pixels with key == T per 256-pixel block
__global__ __launch_bounds__(kBlock) void k_budget_ties(const unsigned *__restrict__ keys, int n, const SelectState *__restrict__ st,
                                                        int *__restrict__ ties) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned T = st->prefix;
  const bool tie = i < n && keys[i] == T;
  __shared__ int sh_cnt[4];
  const unsigned long long m = __ballot(tie);
  if ((threadIdx.x & 63) == 0) sh_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) ties[blockIdx.x] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}

// one block: the exclusive prefix of the per-block tie counts, in place
__global__ __launch_bounds__(kBlock) void k_budget_ties_prefix(int *ties, int n_blocks) {
  const int chunk = (n_blocks + kBlock - 1) / kBlock;
  const int b0 = (int)threadIdx.x * chunk < n_blocks ? (int)threadIdx.x * chunk : n_blocks;
  const int b1 = b0 + chunk < n_blocks ? b0 + chunk : n_blocks;
  int c = 0;
  for (int b = b0; b < b1; ++b) c += ties[b];
  __shared__ int sh[kBlock];
  sh[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < kBlock; ++t) {
      const int v = sh[t];
      sh[t] = run, run += v;
    }
  }
  __syncthreads();
  int run = sh[threadIdx.x];
  for (int b = b0; b < b1; ++b) {
    const int v = ties[b];
    ties[b] = run, run += v;
  }
}

__global__ __launch_bounds__(kBlock) void k_budget_topk_plane(const unsigned *__restrict__ keys, int n,
                                                              const SelectState *__restrict__ st, const int *__restrict__ ties_before,
                                                              unsigned char *__restrict__ plane, int *__restrict__ kept) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned T = st->prefix;
  const int r = (int)st->remaining;
  const unsigned k = i < n ? keys[i] : kNoKey;
  const bool cand = k != kNoKey;
  const bool tie = cand && k == T;
  __shared__ int sh_cnt[4];
  const unsigned long long m = __ballot(tie);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = ties_before[blockIdx.x];
  for (int w = 0; w < wave; ++w) before += sh_cnt[w];
  const bool keep = cand && (k > T || (tie && before + lane_rank(m) < r));
  if (i < n) plane[i] = keep ? 1 : 0;
  count_kept(keep, kept);
}

// (key, lowest index first) as one 64-bit maximum; 0: no candidate (an index is below 2^30, so ~index is never 0)
__device__ __forceinline__ unsigned long long pack(unsigned key, int i) {
  return key == kNoKey ? 0ull : ((unsigned long long)key << 32) | (unsigned long long)(~(unsigned)i);
}

// GRID, small cells: a lane per cell, a row of cells along x
__global__ __launch_bounds__(kBlock) void k_budget_grid_lanes(const unsigned *__restrict__ keys, int w, int h, int cell, int cells_x,
                                                              unsigned char *__restrict__ plane, int *__restrict__ kept) {
  const int cx = blockIdx.x * kBlock + threadIdx.x, cy = blockIdx.y;
  unsigned long long best = 0ull;
  if (cx < cells_x) {
    const int x0 = cx * cell, y0 = cy * cell;
    const int x1 = x0 + cell < w ? x0 + cell : w, y1 = y0 + cell < h ? y0 + cell : h;
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) {
        const int i = y * w + x;
        const unsigned long long p = pack(keys[i], i);
        best = p > best ? p : best;
      }
    if (best) plane[~(unsigned)best] = 1;
  }
  count_kept(best != 0ull, kept);
}

// GRID, large cells (up to the whole level): a block per cell
__global__ __launch_bounds__(kBlock) void k_budget_grid_blocks(const unsigned *__restrict__ keys, int w, int h, int cell,
                                                               unsigned char *__restrict__ plane, int *__restrict__ kept) {
  const int x0 = blockIdx.x * cell, y0 = blockIdx.y * cell;
  const int cw = (x0 + cell < w ? x0 + cell : w) - x0, ch = (y0 + cell < h ? y0 + cell : h) - y0;
  unsigned long long best = 0ull;
  // a wave reads 64 consecutive pixels of a row where the cell is that wide; a narrower cell wraps into its next rows
  const int px = cw * ch;  // (at most 2^30)
  for (int p = threadIdx.x; p < px; p += kBlock) {
    const int row = p / cw, col = p - row * cw;
    const int i = (y0 + row) * w + (x0 + col);
    const unsigned long long v = pack(keys[i], i);
    best = v > best ? v : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(best, o, 64);
    best = v > best ? v : best;
  }
  __shared__ unsigned long long sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  bool won = false;
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) best = sh[k] > best ? sh[k] : best;
    won = best != 0ull;
    if (won) plane[~(unsigned)best] = 1;
  }
  count_kept(won, kept);
}

}  // namespace budget
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::budget;

namespace {

// level l of `p` behind the options into the mask's plane l
hipError_t budget_level(const dvo_amd_pyramid *p, const dvo_amd_budget_options &o, int l, unsigned *keys, int *ties, SelectState *st,
                        dvo_amd_mask *m, hipStream_t s) {
  const LevelData &L = p->lv[l];
  const int n = L.n, n_blocks = (n + kBlock - 1) / kBlock;
  const unsigned char *within = o.within ? o.within->plane[l] : nullptr;
  hipLaunchKernelGGL(k_budget_keys, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, L.z_plane, L.c_a, L.c_b, within, n,
                     o.intensity_threshold, o.depth_threshold, o.depth_weight, keys);
  if (o.rule == DVO_AMD_BUDGET_TOPK) {
    // (a budget a level cannot hold, or a negative one, is "every candidate": the clamp against |C| is k_budget_pick's)
    const unsigned budget = o.budget[l] < 0 || o.budget[l] > (long long)n ? (unsigned)n : (unsigned)o.budget[l];
    const int hist_blocks = n_blocks < kMaxHistBlocks ? n_blocks : kMaxHistBlocks;
    for (int pass = 0; pass < kDigits; ++pass) {
      hipLaunchKernelGGL(k_budget_hist, dim3((unsigned)hist_blocks), dim3(kBlock), 0, s, (const unsigned *)keys, n, pass, st);
      hipLaunchKernelGGL(k_budget_pick, dim3(1), dim3(kBlock), 0, s, st, pass, budget);
    }
    hipLaunchKernelGGL(k_budget_ties, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, (const unsigned *)keys, n, (const SelectState *)st, ties);
    hipLaunchKernelGGL(k_budget_ties_prefix, dim3(1), dim3(kBlock), 0, s, ties, n_blocks);
    hipLaunchKernelGGL(k_budget_topk_plane, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, (const unsigned *)keys, n, (const SelectState *)st,
                       (const int *)ties, m->plane[l], m->counters + l);
  } else {
    const int cell = o.cell[l] < (L.w > L.h ? L.w : L.h) ? o.cell[l] : (L.w > L.h ? L.w : L.h);  // (one cell already)
    const int cells_x = (L.w + cell - 1) / cell, cells_y = (L.h + cell - 1) / cell;
    const hipError_t e = hipMemsetAsync(m->plane[l], 0, (size_t)n, s);
    if (e != hipSuccess) return e;
    if (cell <= kLaneCell)
      hipLaunchKernelGGL(k_budget_grid_lanes, dim3((unsigned)((cells_x + kBlock - 1) / kBlock), (unsigned)cells_y), dim3(kBlock), 0, s,
                         (const unsigned *)keys, L.w, L.h, cell, cells_x, m->plane[l], m->counters + l);
    else  // (cell > 8: at most w / 9 cells along x, and cells_y <= h <= 65535 as check_mask_size has it)
      hipLaunchKernelGGL(k_budget_grid_blocks, dim3((unsigned)cells_x, (unsigned)cells_y), dim3(kBlock), 0, s, (const unsigned *)keys,
                         L.w, L.h, cell, m->plane[l], m->counters + l);
  }
  return hipGetLastError();
}

}  // namespace

extern "C" {

void dvo_amd_default_budget_options(dvo_amd_budget_options *opt) {
  if (!opt) return;
  opt->rule = DVO_AMD_BUDGET_TOPK;
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) opt->budget[l] = -1, opt->cell[l] = 1;
  opt->intensity_threshold = 0.0f, opt->depth_threshold = 0.0f, opt->depth_weight = 0.0f;
  opt->within = nullptr;
}

int dvo_amd_mask_create_budget(dvo_amd_pyramid *p, const dvo_amd_budget_options *opt, dvo_amd_mask **out) {
  static const char *entry = "dvo_amd_mask_create_budget";
  if (out) *out = nullptr;
  if (!p || !opt || !out) return invalid(entry, "a NULL pointer");
  const dvo_amd_budget_options o = *opt;
  if (o.rule != DVO_AMD_BUDGET_TOPK && o.rule != DVO_AMD_BUDGET_GRID)
    return invalid(entry, "rule must be DVO_AMD_BUDGET_TOPK or DVO_AMD_BUDGET_GRID");
  if (o.rule == DVO_AMD_BUDGET_GRID)
    for (int l = 0; l < p->n_levels; ++l)
      if (o.cell[l] < 1) return invalid(entry, "cell[" + std::to_string(l) + "] < 1");
  if (!std::isfinite(o.intensity_threshold) || !std::isfinite(o.depth_threshold)) return invalid(entry, "a threshold is not finite");
  if (!std::isfinite(o.depth_weight) || o.depth_weight < 0.0f) return invalid(entry, "depth_weight must be finite and >= 0");
  int rc = mask_fits(entry, p, o.within);
  if (rc) return rc;
  const int w = p->lv[0].w, h = p->lv[0].h, levels = p->n_levels;
  rc = check_mask_size(entry, w, h, levels);
  if (rc) return rc;

  dvo_amd_mask *m = nullptr;
  hipStream_t st;
  rc = mask_alloc(entry, p->device, w, h, levels, &m, &st);
  if (rc) return rc;
  // scratch of the call: the select states, then the key plane and the tie counts of the largest level
  const size_t n0 = (size_t)p->lv[0].n, blocks0 = (n0 + kBlock - 1) / kBlock;
  const size_t state_bytes = align_up(sizeof(SelectState) * (size_t)levels, 256), key_bytes = align_up(4 * n0, 256);
  void *scratch = nullptr;
  hipError_t e = hipMalloc(&scratch, state_bytes + key_bytes + 4 * blocks0);
  if (e != hipSuccess) {
    (void)hipFree(m->mem);
    delete m;
    return e == hipErrorOutOfMemory ? (int)DVO_AMD_ERR_OUT_OF_MEMORY : fail_hip("hipMalloc (budget scratch)", e);
  }
  SelectState *states = (SelectState *)scratch;
  unsigned *keys = (unsigned *)((char *)scratch + state_bytes);
  int *ties = (int *)((char *)scratch + state_bytes + key_bytes);
  e = hipMemsetAsync(states, 0, state_bytes, st);
  for (int l = 0; l < levels && e == hipSuccess; ++l) e = budget_level(p, o, l, keys, ties, states + l, m, st);
  rc = mask_finish(m, e, st, out);  // (drains the stream: the scratch is idle behind it)
  (void)hipFree(scratch);
  return rc;
}

}  // extern "C"
