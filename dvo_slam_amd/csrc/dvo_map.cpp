// The keyframe map's point cloud (dvo_amd.h: dvo_amd_point_cloud, dvo_amd_map_cloud, dvo_amd_voxel_downsample):
//   k_cloud        one pass over a level's depth / intensity planes and rays: the organized cloud at a pose, 16-B stores
//   k_map_keys     the same points (one shared device function) straight into the aggregate: finite and in-range points are
//                  compacted with their 63-bit voxel key; counts and the min / max voxel index per thread, one integer atomic
//                  per wave at the end
//   k_rekey        63-bit key -> the dense key of the bits actually present (order preserving)
//   k_radix_*      stable LSD radix sort of (key, point index), 8-bit digits: per-block digit histograms, an exclusive scan of
//                  the [digit][block] table, a stable scatter (ranks within a wave by ballots, across waves through LDS)
//   k_heads        first position of every run of equal keys -> (scan) the voxel index of every sorted position
//   k_accum        runs of a sorted chunk summed in registers, flushed into the voxel's integer sums with u64 atomics
//   k_voxel_out    centroid and colour of every voxel from its integer sums
// The map kept on the device (dvo_amd_map_*): the same input stage and sort with a sign per image, then
//   k_delta_keys   the 63-bit key of every voxel of the sorted, signed delta
//   k_merge        merge path over (store, delta), both in key order: sums of equal keys added, voxels left without points flagged
//   k_compact      the flagged positions into the other store buffer
//   k_box_flags / k_box_compact   the box rule of dvo_amd_map_extract on the output points, order kept
//   k_render_clear / k_render_splat / k_render_resolve   the store forward-projected into a camera view with a nearest-depth
//                  test (dvo_amd_map_render): a 64-bit unsigned-min atomic per covered pixel, then one pass over the pixels
// Every sum is an integer sum: the result does not depend on the order points arrive in, on the compaction order or on the
// launch geometry -- bit for bit.
#include <climits>
#include <cmath>
#include <cstring>

#include "dvo_internal.h"
#include "dvo_device_rules.h"

namespace dvo_amd {
namespace map {

constexpr int kBlock = 256;
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kSortItems = 16;                    // items per thread of a radix tile
constexpr int kSortTile = kBlock * kSortItems;    // 4096 items per radix block
constexpr int kScanTile = kBlock * 16;            // items per block of the generic exclusive scan
constexpr int kAccumChunk = 16;                   // sorted positions one k_accum thread sums before it flushes
constexpr int kIndexBias = 1 << 20;               // voxel index range [-2^20, 2^20)
constexpr double kFix = 16777216.0;               // 2^24: the fixed point of the centroid sums
constexpr unsigned kNegBit = 0x80000000u;         // top bit of a value index: the point counts with sign -1 (k_accum)
constexpr int kMergeItems = 8;                    // merged entries per thread of a merge tile
constexpr int kMergeTile = kBlock * kMergeItems;  // 2048 entries of store + delta per k_merge block
// At most 2^31 points per call: every position the kernels form in 32 bits (a radix tile's t0 + c * 256 + tid, a k_accum
// chunk's start) then stays below 2^31 + 2^16 and cannot wrap.

// one image of a map call, as the kernels read it
struct MapImage {
  const float *z, *i, *tx, *ty;
  const unsigned char *bgr;  // device, tight (w * 3 bytes per row); null: grey from the intensity plane
  int w, h;
  float T[12];               // rows 0..2 of (float)pose, row-major
  unsigned neg;              // 0, or kNegBit: the image's points are subtracted (the delta of a persistent map)
};

struct MapCtrl {
  unsigned long long kept, finite, out_of_range;
  int mn[3], mx[3];
  unsigned voxels, pad;
};

struct VoxelAcc {
  unsigned long long count, s[3], c[3], pad;
};

__device__ __forceinline__ unsigned grey8(float v) {
  if (!(v == v)) return 0u;
  return (unsigned)fminf(fmaxf(v, 0.0f), 255.0f);
}

// the point of pixel (u, v): camera point (tx[u] z, ty[v] z, z), transformed in the order the header pins, coloured
__device__ __forceinline__ float4 image_point(const MapImage &im, int u, int v) {
  const size_t p = (size_t)v * im.w + u;
  const float z = im.z[p];
  const float x = im.tx[u] * z, y = im.ty[v] * z;
  const float *T = im.T;
  const float wx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  const float wy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  const float wz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
  unsigned rgb;
  if (im.bgr) {
    const unsigned char *c = im.bgr + p * 3;
    rgb = ((unsigned)c[2] << 16) | ((unsigned)c[1] << 8) | (unsigned)c[0];
  } else {
    const unsigned g = grey8(im.i[p]);
    rgb = (g << 16) | (g << 8) | g;
  }
  return make_float4(wx, wy, wz, __uint_as_float(rgb));
}

__global__ void __launch_bounds__(kBlock) k_cloud(MapImage im, float4 *out) {
  const long long n = (long long)im.w * im.h;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock) {
    const int v = (int)(p / im.w), u = (int)(p - (long long)v * im.w);
    out[p] = image_point(im, u, v);
  }
}

__device__ __forceinline__ unsigned long long lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// what a thread of an input stage has counted over its points; flushed once per wave at the end of the kernel
struct Counts {
  unsigned long long finite = 0, out_of_range = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
};

// voxel of one point: kept (finite and in range) with its 63-bit key
__device__ __forceinline__ void key_and_count(const float4 pt, float inv, bool active, Counts &cnt, bool &keep,
                                              unsigned long long &key) {
  const bool finite = active && isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z);
  float f[3] = {floorf(pt.x * inv), floorf(pt.y * inv), floorf(pt.z * inv)};
  bool in = finite;
  int idx[3] = {0, 0, 0};
  for (int a = 0; a < 3; ++a) {
    in = in && f[a] >= -(float)kIndexBias && f[a] < (float)kIndexBias;
    idx[a] = in ? (int)f[a] : 0;
  }
  keep = in;
  key = ((unsigned long long)(idx[0] + kIndexBias) << 42) | ((unsigned long long)(idx[1] + kIndexBias) << 21) |
        (unsigned long long)(idx[2] + kIndexBias);
  cnt.finite += finite ? 1 : 0;
  cnt.out_of_range += (finite && !in) ? 1 : 0;
  if (in)
    for (int a = 0; a < 3; ++a) cnt.mn[a] = min(cnt.mn[a], idx[a]), cnt.mx[a] = max(cnt.mx[a], idx[a]);
}

// every lane of the wave must call it
__device__ __forceinline__ void flush_counts(Counts &cnt, MapCtrl *ctrl) {
  const unsigned long long fin = rules::wave_sum(cnt.finite), oor = rules::wave_sum(cnt.out_of_range);
  int mn[3], mx[3];
  for (int a = 0; a < 3; ++a) mn[a] = wave_min(cnt.mn[a]), mx[a] = wave_max(cnt.mx[a]);
  if ((threadIdx.x & 63) == 0) {
    if (fin) atomicAdd(&ctrl->finite, fin);
    if (oor) atomicAdd(&ctrl->out_of_range, oor);
    if (fin != oor)
      for (int a = 0; a < 3; ++a) atomicMin(&ctrl->mn[a], mn[a]), atomicMax(&ctrl->mx[a], mx[a]);
  }
}

// compaction slot of a kept point (wave-aggregated atomic: the order of the compacted points is not deterministic, nothing
// downstream depends on it)
__device__ __forceinline__ unsigned long long compact_slot(bool keep, MapCtrl *ctrl) {
  const unsigned long long bk = __ballot(keep);
  unsigned long long base = 0;
  if ((threadIdx.x & 63) == 0 && bk) base = atomicAdd(&ctrl->kept, (unsigned long long)__popcll(bk));
  base = __shfl(base, 0, 64);
  return base + __popcll(bk & lanemask_lt());
}

// aggregate input from images: grid (blocks over the largest image, images)
__global__ void __launch_bounds__(kBlock) k_map_keys(const MapImage *images, int image0, float inv, float4 *pts,
                                                     unsigned long long *keys, unsigned *vals, MapCtrl *ctrl,
                                                     unsigned long long *per_image) {
  const MapImage im = images[image0 + blockIdx.y];
  const long long n = (long long)im.w * im.h;
  Counts cnt;
  for (long long p0 = (long long)blockIdx.x * kBlock; p0 < n; p0 += (long long)gridDim.x * kBlock) {
    const long long p = p0 + threadIdx.x;
    const bool active = p < n;
    float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
      const int v = (int)(p / im.w), u = (int)(p - (long long)v * im.w);
      pt = image_point(im, u, v);
    }
    bool keep;
    unsigned long long key;
    key_and_count(pt, inv, active, cnt, keep, key);
    const unsigned long long slot = compact_slot(keep, ctrl);
    if (keep) pts[slot] = pt, keys[slot] = key, vals[slot] = (unsigned)slot | im.neg;
  }
  if (per_image) {  // (finite, out of range) of every image on its own: the totals a persistent map keeps per keyframe
    const unsigned long long fin = rules::wave_sum(cnt.finite), oor = rules::wave_sum(cnt.out_of_range);
    if ((threadIdx.x & 63) == 0) {
      if (fin) atomicAdd(&per_image[2 * (size_t)(image0 + blockIdx.y)], fin);
      if (oor) atomicAdd(&per_image[2 * (size_t)(image0 + blockIdx.y) + 1], oor);
    }
  }
  flush_counts(cnt, ctrl);
}

// aggregate input from a point array (already on the device); vals index the array itself
__global__ void __launch_bounds__(kBlock) k_points_keys(const float4 *in, unsigned long long n, float inv,
                                                        unsigned long long *keys, unsigned *vals, MapCtrl *ctrl) {
  Counts cnt;
  for (unsigned long long p0 = (unsigned long long)blockIdx.x * kBlock; p0 < n; p0 += (unsigned long long)gridDim.x * kBlock) {
    const unsigned long long p = p0 + threadIdx.x;
    const bool active = p < n;
    const float4 pt = active ? in[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep;
    unsigned long long key;
    key_and_count(pt, inv, active, cnt, keep, key);
    const unsigned long long slot = compact_slot(keep, ctrl);
    if (keep) keys[slot] = key, vals[slot] = (unsigned)p;
  }
  flush_counts(cnt, ctrl);
}

struct Rekey {
  int mn[3];
  int sh_i, sh_j;  // bits of the j and k fields, of the k field
};

__global__ void __launch_bounds__(kBlock) k_rekey(unsigned long long *keys, unsigned long long n, Rekey r) {
  for (unsigned long long p = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (unsigned long long)gridDim.x * kBlock) {
    const unsigned long long k = keys[p];
    const unsigned long long i = ((k >> 42) & 0x1FFFFF) - (unsigned long long)(r.mn[0] + kIndexBias);
    const unsigned long long j = ((k >> 21) & 0x1FFFFF) - (unsigned long long)(r.mn[1] + kIndexBias);
    const unsigned long long kk = (k & 0x1FFFFF) - (unsigned long long)(r.mn[2] + kIndexBias);
    keys[p] = (i << r.sh_i) | (j << r.sh_j) | kk;
  }
}

// per-block digit histogram of a radix tile -> counts[digit * n_blocks + block]
__global__ void __launch_bounds__(kBlock) k_radix_hist(const unsigned long long *keys, unsigned n, int shift, unsigned *counts) {
  __shared__ unsigned hist[kRadix];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned t0 = blockIdx.x * kSortTile;
  for (int c = 0; c < kSortItems; ++c) {
    const unsigned p = t0 + c * kBlock + threadIdx.x;
    if (p < n) atomicAdd(&hist[(unsigned)(keys[p] >> shift) & (kRadix - 1)], 1u);
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

// stable scatter of a radix tile: items in tile order (chunk, wave, lane); offsets = the scanned counts
__global__ void __launch_bounds__(kBlock) k_radix_scatter(const unsigned long long *keys_in, const unsigned *vals_in,
                                                          unsigned long long *keys_out, unsigned *vals_out, unsigned n,
                                                          int shift, const unsigned *offsets) {
  __shared__ unsigned base[kRadix];
  __shared__ unsigned wcnt[kBlock / 64][kRadix];
  const int wave = threadIdx.x >> 6;
  base[threadIdx.x] = offsets[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
  const unsigned t0 = blockIdx.x * kSortTile;
  for (int c = 0; c < kSortItems; ++c) {
    for (int w = 0; w < kBlock / 64; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const unsigned p = t0 + c * kBlock + threadIdx.x;
    const bool active = p < n;
    const unsigned long long k = active ? keys_in[p] : 0ull;
    const unsigned v = active ? vals_in[p] : 0u;
    const unsigned d = (unsigned)(k >> shift) & (kRadix - 1);
    unsigned long long peers = __ballot(active);
    for (int b = 0; b < kRadixBits; ++b) {
      const unsigned long long bal = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const unsigned rank = __popcll(peers & lanemask_lt());
    if (active && rank == 0) wcnt[wave][d] = __popcll(peers);  // the first lane of each digit group writes its count
    __syncthreads();
    if (active) {
      unsigned off = base[d] + rank;
      for (int w = 0; w < wave; ++w) off += wcnt[w][d];
      if (off < n) keys_out[off] = k, vals_out[off] = v;  // (always: the offsets are a permutation of [0, n))
    }
    __syncthreads();
    unsigned add = 0;
    for (int w = 0; w < kBlock / 64; ++w) add += wcnt[w][threadIdx.x];
    base[threadIdx.x] += add;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock) k_scan_reduce(const unsigned *a, unsigned n, unsigned *bsum) {
  const unsigned t0 = blockIdx.x * kScanTile;
  unsigned s = 0;
  for (int c = 0; c < kScanTile / kBlock; ++c) {
    const unsigned p = t0 + c * kBlock + threadIdx.x;
    if (p < n) s += a[p];
  }
  unsigned total;
  (void)rules::block_exclusive_scan<kBlock / 64>(s, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: exclusive scan of the block sums in place; *grand = the sum of all
__global__ void __launch_bounds__(kBlock) k_scan_blocks(unsigned *bsum, unsigned nb, unsigned *grand) {
  unsigned carry = 0;
  for (unsigned c0 = 0; c0 < nb; c0 += kBlock) {
    const unsigned p = c0 + threadIdx.x;
    const unsigned v = p < nb ? bsum[p] : 0u;
    unsigned total;
    const unsigned ex = rules::block_exclusive_scan<kBlock / 64>(v, &total);
    if (p < nb) bsum[p] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0 && grand) *grand = carry;
}

__global__ void __launch_bounds__(kBlock) k_scan_apply(unsigned *a, unsigned n, const unsigned *bsum) {
  const unsigned t0 = blockIdx.x * kScanTile;
  unsigned carry = bsum[blockIdx.x];
  for (int c = 0; c < kScanTile / kBlock; ++c) {
    const unsigned p = t0 + c * kBlock + threadIdx.x;
    const unsigned v = p < n ? a[p] : 0u;
    unsigned total;
    const unsigned ex = rules::block_exclusive_scan<kBlock / 64>(v, &total);
    if (p < n) a[p] = carry + ex;
    carry += total;
  }
}

__global__ void __launch_bounds__(kBlock) k_heads(const unsigned long long *keys, unsigned n, unsigned *flags) {
  for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock)
    flags[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}

__device__ __forceinline__ void flush(VoxelAcc *acc, unsigned n_vox, unsigned v, unsigned long long cnt,
                                      const unsigned long long s[3], const unsigned long long c[3]) {
  if (v >= n_vox) return;  // (never: v < the number of heads)
  VoxelAcc *a = acc + v;
  atomicAdd(&a->count, cnt);
  for (int q = 0; q < 3; ++q) atomicAdd(&a->s[q], s[q]), atomicAdd(&a->c[q], c[q]);
}

// vidx = the exclusive scan of the head flags: the voxel of sorted position p is vidx[p] + flag(p) - 1; sums wrap modulo 2^64.
// A value index with kNegBit set subtracts its point: the count and every sum take the sign in integers (modulo 2^64).
__global__ void __launch_bounds__(kBlock) k_accum(const unsigned long long *keys, const unsigned *vals, const unsigned *vidx,
                                                  unsigned n, const float4 *pts, VoxelAcc *acc, unsigned n_vox) {
  const unsigned p0 = (blockIdx.x * kBlock + threadIdx.x) * kAccumChunk;
  if (p0 >= n) return;
  const unsigned p1 = min(n, p0 + kAccumChunk);
  unsigned long long key = keys[p0];
  unsigned vox = vidx[p0] + ((p0 == 0 || keys[p0 - 1] != key) ? 1u : 0u) - 1u;
  unsigned long long cnt = 0, c[3] = {0, 0, 0}, s[3] = {0, 0, 0};
  for (unsigned p = p0; p < p1; ++p) {
    const unsigned long long k = keys[p];
    if (k != key) {
      flush(acc, n_vox, vox, cnt, s, c);
      key = k, ++vox, cnt = 0;
      for (int q = 0; q < 3; ++q) s[q] = 0, c[q] = 0;
    }
    const unsigned val = vals[p];
    const float4 pt = pts[val & ~kNegBit];
    const unsigned rgb = __float_as_uint(pt.w);
    const unsigned long long q[3] = {(unsigned long long)llrint((double)pt.x * kFix), (unsigned long long)llrint((double)pt.y * kFix),
                                     (unsigned long long)llrint((double)pt.z * kFix)};
    const unsigned long long ch[3] = {(rgb >> 16) & 0xFF, (rgb >> 8) & 0xFF, rgb & 0xFF};
    if (val & kNegBit) {
      for (int a = 0; a < 3; ++a) s[a] -= q[a], c[a] -= ch[a];
      --cnt;
    } else {
      for (int a = 0; a < 3; ++a) s[a] += q[a], c[a] += ch[a];
      ++cnt;
    }
  }
  flush(acc, n_vox, vox, cnt, s, c);
}

__global__ void __launch_bounds__(kBlock) k_voxel_out(const VoxelAcc *acc, unsigned n_vox, float4 *out) {
  for (unsigned v = blockIdx.x * kBlock + threadIdx.x; v < n_vox; v += gridDim.x * kBlock) {
    const VoxelAcc a = acc[v];
    const double den = (double)a.count * kFix;
    float xyz[3];
    unsigned ch[3];
    for (int q = 0; q < 3; ++q) {
      xyz[q] = (float)((double)(long long)a.s[q] / den);
      ch[q] = (unsigned)((a.c[q] + a.count / 2) / a.count);
    }
    out[v] = make_float4(xyz[0], xyz[1], xyz[2], __uint_as_float((ch[0] << 16) | (ch[1] << 8) | ch[2]));
  }
}

// ---- the persistent keyframe map (dvo_amd_map_*) ---------------------------------------------------------------------------
// The store holds the occupied voxels in ascending 63-bit key order: keys[n], VoxelAcc[n].  One call's delta (signed points
// through k_map_keys, the sort, k_accum) is one signed VoxelAcc per touched voxel in key order; k_merge merges the two sorted
// sequences, k_compact drops the voxels whose count has become 0.

// the 63-bit key of every voxel of a sorted delta, from the dense key of its first point
__global__ void __launch_bounds__(kBlock) k_delta_keys(const unsigned long long *keys, const unsigned *vidx, unsigned n, Rekey r,
                                                       unsigned long long *vkeys, unsigned n_vox) {
  for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    const unsigned long long k = keys[p];
    if (p != 0 && keys[p - 1] == k) continue;
    const unsigned v = vidx[p];  // heads before p
    if (v >= n_vox) continue;    // (never)
    const unsigned long long i = k >> r.sh_i, j = (k >> r.sh_j) & ((1ull << (r.sh_i - r.sh_j)) - 1ull), kk = k & ((1ull << r.sh_j) - 1ull);
    vkeys[v] = ((i + (unsigned long long)(r.mn[0] + kIndexBias)) << 42) | ((j + (unsigned long long)(r.mn[1] + kIndexBias)) << 21) |
               (kk + (unsigned long long)(r.mn[2] + kIndexBias));
  }
}

// merge path: how many of the first d merged entries come from a (ties: a first)
__device__ __forceinline__ unsigned merge_split(const unsigned long long *a, unsigned na, const unsigned long long *b, unsigned nb,
                                                unsigned d) {
  unsigned lo = d > nb ? d - nb : 0u, hi = min(d, na);
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (a[mid] <= b[d - mid - 1]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

constexpr unsigned kNoMatch = 0xFFFFFFFFu, kDead = 0xFFFFFFFEu;

// Merges the store (ka, va: na entries) and the delta (kb, vb: nb entries), both in ascending order of distinct keys, into
// na + nb merged positions.  A store entry takes the sums of the delta entry of its key (the next merged position); that delta
// entry is dead.  flags[o] = 1 where position o holds a voxel with a count other than 0.  Every position has one writer: the
// block whose tile it lies in, found by a binary search along the tile's diagonals; no atomics.  Four lanes move one 64-byte
// entry, 16 bytes each.
__global__ void __launch_bounds__(kBlock) k_merge(const unsigned long long *ka, const VoxelAcc *va, unsigned na,
                                                  const unsigned long long *kb, const VoxelAcc *vb, unsigned nb,
                                                  unsigned long long *ko, VoxelAcc *vo, unsigned *flags) {
  __shared__ unsigned long long sk[kMergeTile + 2];  // a[a0 - 1] | a[a0, a1) | b[b0, b1) | b[b1]
  __shared__ unsigned s_src[kMergeTile], s_match[kMergeTile], s_split[2];
  const unsigned total = na + nb;
  const unsigned d0 = blockIdx.x * (unsigned)kMergeTile, d1 = min(total, d0 + (unsigned)kMergeTile);
  if (threadIdx.x < 2) s_split[threadIdx.x] = merge_split(ka, na, kb, nb, threadIdx.x ? d1 : d0);
  __syncthreads();
  const unsigned a0 = s_split[0], a1 = s_split[1], b0 = d0 - a0, b1 = d1 - a1;
  const unsigned la = a1 - a0, lb = b1 - b0, len = d1 - d0;
  unsigned long long *sa = sk + 1, *sb = sk + 1 + la;
  for (unsigned e = threadIdx.x; e < la; e += kBlock) sa[e] = ka[a0 + e];
  for (unsigned e = threadIdx.x; e < lb; e += kBlock) sb[e] = kb[b0 + e];
  if (threadIdx.x == 0) {
    sk[0] = a0 > 0 ? ka[a0 - 1] : ~0ull;      // (~0 is no key: keys have 63 bits)
    sb[lb] = b1 < nb ? kb[b1] : ~0ull;
  }
  __syncthreads();
  const unsigned dl = min(threadIdx.x * (unsigned)kMergeItems, len);
  unsigned a = merge_split(sa, la, sb, lb, dl), b = dl - a;
  for (int it = 0; it < kMergeItems; ++it) {
    const unsigned o = dl + it;
    if (o >= len) break;
    if (a < la && (b >= lb || sa[a] <= sb[b])) {
      s_src[o] = a0 + a;
      s_match[o] = sb[b] == sa[a] ? b0 + b : kNoMatch;  // sb[lb]: the first delta key of the next tile
      ++a;
    } else {
      s_src[o] = (b0 + b) | kNegBit;
      s_match[o] = sa[(int)a - 1] == sb[b] ? kDead : kNoMatch;  // sa[-1]: the last store key of the tile before
      ++b;
    }
  }
  __syncthreads();
  const unsigned part = threadIdx.x & 3;
  for (unsigned e = threadIdx.x >> 2; e < len; e += kBlock / 4) {
    const unsigned src = s_src[e], mt = s_match[e], o = d0 + e;
    if (mt == kDead) {
      if (part == 0) flags[o] = 0u;
      continue;
    }
    const bool from_b = (src & kNegBit) != 0;
    const unsigned at = src & ~kNegBit;
    ulonglong2 v = ((const ulonglong2 *)(from_b ? vb + at : va + at))[part];
    if (mt != kNoMatch) {
      const ulonglong2 w = ((const ulonglong2 *)(vb + mt))[part];
      v.x += w.x, v.y += w.y;
    }
    ((ulonglong2 *)(vo + o))[part] = v;
    if (part == 0) {
      flags[o] = v.x != 0ull ? 1u : 0u;  // v.x: the count
      ko[o] = from_b ? sb[at - b0] : sa[at - a0];
    }
  }
}

// ex = the exclusive scan of k_merge's flags, *grand its total: the flagged positions move to ex[o] of the other store buffer
__global__ void __launch_bounds__(kBlock) k_compact(const unsigned long long *ki, const VoxelAcc *vi, const unsigned *ex,
                                                    const unsigned *grand, unsigned total, unsigned long long *ko, VoxelAcc *vo) {
  const unsigned part = threadIdx.x & 3;
  for (unsigned long long t = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; t < 4ull * total;
       t += (unsigned long long)gridDim.x * kBlock) {
    const unsigned o = (unsigned)(t >> 2);
    const unsigned at = ex[o], next = o + 1 < total ? ex[o + 1] : *grand;
    if (next == at || at >= total) continue;
    ((ulonglong2 *)(vo + at))[part] = ((const ulonglong2 *)(vi + o))[part];
    if (part == 0) ko[at] = ki[o];
  }
}

struct Box {
  float mn[3], mx[3];
};

// the box rule of dvo_amd_map_extract on the output points
__global__ void __launch_bounds__(kBlock) k_box_flags(const float4 *pts, unsigned n, Box box, unsigned *flags) {
  for (unsigned v = blockIdx.x * kBlock + threadIdx.x; v < n; v += gridDim.x * kBlock) {
    const float4 c = pts[v];
    const bool in = c.x >= box.mn[0] && c.x < box.mx[0] && c.y >= box.mn[1] && c.y < box.mx[1] && c.z >= box.mn[2] && c.z < box.mx[2];
    flags[v] = in ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(kBlock) k_box_compact(const float4 *pts, const unsigned *ex, const unsigned *grand, unsigned n,
                                                        float4 *out) {
  for (unsigned v = blockIdx.x * kBlock + threadIdx.x; v < n; v += gridDim.x * kBlock) {
    const unsigned at = ex[v], next = v + 1 < n ? ex[v + 1] : *grand;
    if (next != at && at < n) out[at] = pts[v];
  }
}

// ---- the map rendered into a camera view (dvo_amd_map_render, dvo_amd_map_render_pyramid) ------------------------------------
//   k_render_clear    the z-buffer (one 64-bit word per pixel) to all ones
//   k_render_splat    every voxel of the store: centroid, world -> camera, cull, project, footprint; the footprint's pixels keep
//                     the minimum of (bits(cz) << 32) | rank with one 64-bit unsigned-min atomic each
//   k_render_resolve  per pixel: the winner's depth, colour, grey value and rank into the requested planes
// The minimum does not depend on the order the atomics land in, and the words only decrease: the planes are a function of the
// store and the view alone.

struct RenderView {
  int w, h;
  float fx, fy, ox, oy, near_z, leaf;
  float T[12];  // rows 0..2 of the float inverse pose (world -> camera), row-major
};

struct RenderCtrl {
  unsigned long long behind_near, outside, drawn, covered;
};

constexpr unsigned long long kEmptyWord = ~0ull;
constexpr int kSmallFootprint = 4;  // pixels a lane splats by itself; larger footprints are walked by the whole wave

__global__ void __launch_bounds__(kBlock) k_render_clear(ulonglong2 *z, unsigned long long n2) {
  for (unsigned long long p = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; p < n2; p += (unsigned long long)gridDim.x * kBlock)
    z[p] = make_ulonglong2(kEmptyWord, kEmptyWord);
}

__global__ void __launch_bounds__(kBlock) k_render_splat(const VoxelAcc *acc, unsigned n_vox, RenderView V, unsigned long long *zbuf,
                                                         RenderCtrl *ctrl) {
  const int lane = threadIdx.x & 63;
  unsigned long long behind = 0, outside = 0, drawn = 0;
  for (unsigned base = blockIdx.x * kBlock; base < n_vox; base += gridDim.x * kBlock) {  // (uniform over the wave: ballots below)
    const unsigned r = base + threadIdx.x;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    unsigned long long word = kEmptyWord;
    bool draw = false;
    if (r < n_vox) {
      const ulonglong2 *a = (const ulonglong2 *)(acc + r);
      const ulonglong2 a0 = a[0], a1 = a[1];  // count, s[0] | s[1], s[2]
      const double den = (double)a0.x * kFix;  // k_voxel_out's centroid
      const float x = (float)((double)(long long)a0.y / den), y = (float)((double)(long long)a1.x / den),
                  z = (float)((double)(long long)a1.y / den);
      const float *T = V.T;
      const float cx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
      const float cy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
      const float cz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
      if (!(cz >= V.near_z)) {
        ++behind;
      } else {
        const float u = (cx * V.fx) / cz + V.ox, v = (cy * V.fy) / cz + V.oy;
        const float hx = 0.5f * ((V.leaf * V.fx) / cz), hy = 0.5f * ((V.leaf * V.fy) / cz);
        const bool in_x = rules::footprint_axis(u, hx, rules::kFootprintFill, V.w, x0, x1),
                   in_y = rules::footprint_axis(v, hy, rules::kFootprintFill, V.h, y0, y1);
        draw = in_x && in_y;
        if (draw) ++drawn, word = ((unsigned long long)__float_as_uint(cz) << 32) | r;
        else ++outside;
      }
    }
    const int fw = draw ? x1 - x0 + 1 : 0, fh = draw ? y1 - y0 + 1 : 0;  // (either may be < 1 past 2^24 pixels a side: nothing drawn)
    const bool some = fw > 0 && fh > 0;
    const bool small = some && (long long)fw * fh <= kSmallFootprint;
    if (small)
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) rules::depth_min(zbuf + (size_t)yy * V.w + xx, word);
    // the larger footprints of the wave, one after the other: a lane per pixel along the rows, so one atomic instruction
    // touches runs of adjacent words
    unsigned long long todo = __ballot(some && !small);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sfw = __shfl(fw, src, 64), sfh = __shfl(fh, src, 64);
      const unsigned wlo = __shfl((unsigned)word, src, 64), whi = __shfl((unsigned)(word >> 32), src, 64);
      const unsigned long long sword = ((unsigned long long)whi << 32) | wlo;
      const int npx = sfw * sfh;  // (at most the view: 2^26)
      for (int p = lane; p < npx; p += 64) {
        const int row = p / sfw, col = p - row * sfw;
        rules::depth_min(zbuf + (size_t)(sy0 + row) * V.w + (sx0 + col), sword);
      }
    }
  }
  const unsigned long long b = rules::wave_sum(behind), o = rules::wave_sum(outside), d = rules::wave_sum(drawn);
  if (lane == 0) {
    if (b) atomicAdd(&ctrl->behind_near, b);
    if (o) atomicAdd(&ctrl->outside, o);
    if (d) atomicAdd(&ctrl->drawn, d);
  }
}

// any of the planes may be null
__global__ void __launch_bounds__(kBlock) k_render_resolve(const unsigned long long *zbuf, unsigned long long n_px, const VoxelAcc *acc,
                                                           unsigned n_vox, float *depth, unsigned *rgb, float *intensity, int *index,
                                                           RenderCtrl *ctrl) {
  unsigned long long covered = 0;
  for (unsigned long long p0 = (unsigned long long)blockIdx.x * kBlock; p0 < n_px; p0 += (unsigned long long)gridDim.x * kBlock) {
    const unsigned long long p = p0 + threadIdx.x;
    if (p >= n_px) continue;
    const unsigned long long w = zbuf[p];
    const unsigned r = (unsigned)w;
    float d = __uint_as_float(0x7FC00000u), g = 0.0f;
    unsigned c = 0;
    int at = -1;
    if (w != kEmptyWord && r < n_vox) {  // (r < n_vox always: the ranks k_render_splat wrote)
      const unsigned long long *a = (const unsigned long long *)(acc + r);
      const unsigned long long cnt = a[0];
      unsigned ch[3];
      for (int q = 0; q < 3; ++q) ch[q] = (unsigned)((a[4 + q] + cnt / 2) / cnt);  // k_voxel_out's colour
      d = __uint_as_float((unsigned)(w >> 32));
      c = (ch[0] << 16) | (ch[1] << 8) | ch[2];
      g = (float)((1868u * (c & 0xFF) + 9617u * ((c >> 8) & 0xFF) + 4899u * ((c >> 16) & 0xFF) + 8192u) >> 14);  // the ingest's grey
      at = (int)r;
      ++covered;
    }
    if (depth) depth[p] = d;
    if (rgb) rgb[p] = c;
    if (intensity) intensity[p] = g;
    if (index) index[p] = at;
  }
  covered = rules::wave_sum(covered);
  if ((threadIdx.x & 63) == 0 && covered) atomicAdd(&ctrl->covered, covered);
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------

unsigned grid_for(unsigned long long n, unsigned per_block, unsigned cap = 4096) {
  const unsigned long long b = (n + per_block - 1) / per_block;
  return (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(b, cap));
}

}  // namespace map

namespace host {

// device buffers of the map entries: grown to the largest call, kept by the context (nothing is allocated once warm)
struct MapWorkspace {
  typedef DeviceBuf Buf;  // (grown in 64 KiB steps: grow_ws)
  Buf pts, keys[2], vals[2], flags, counts, bsum, acc, out, bgr, images, ctrl;
  Buf zbuf, planes;  // a render: the 64-bit z-buffer, then depth | rgb | intensity | index of the view
  hipEvent_t ev[8] = {};  // input stage, sort, reduction, output copy: begin / end each
  double device_ms = 0.0, copy_ms = 0.0;  // the last map call: kernels (three timed segments), the output copy
  long long points = 0;
};

namespace {

int grow_ws(DeviceBuf &b, size_t bytes) { return grow(b, bytes, 1 << 16, "map workspace"); }

int workspace(dvo_amd_context *ctx, MapWorkspace **out) {
  if (!ctx->map_ws) {
    MapWorkspace *w = new MapWorkspace();
    for (hipEvent_t &e : w->ev) {
      const hipError_t he = hipEventCreate(&e);
      if (he != hipSuccess) {
        ctx->map_ws = w;
        return fail_hip("hipEventCreate (map workspace)", he);
      }
    }
    ctx->map_ws = w;
  }
  *out = ctx->map_ws;
  return DVO_AMD_OK;
}

bool valid_leaf(float leaf) { return std::isfinite(leaf) && leaf > 0.0f && leaf <= 65536.0f; }

void float_pose(const double *pose, float T[12]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T[r * 4 + c] = pose ? (float)pose[c * 4 + r] : (r == c ? 1.0f : 0.0f);
}

int bits_for(int span) {
  int b = 0;
  while (b < 31 && (1u << b) <= (unsigned)span) ++b;
  return b;
}

// exclusive scan of a[0..n) in place on the stream; grand (device, may be null) = the total
int scan(MapWorkspace &W, unsigned *a, unsigned n, unsigned *grand, hipStream_t st) {
  const unsigned nb = std::max(1u, (n + map::kScanTile - 1) / map::kScanTile);
  int rc = grow_ws(W.bsum, sizeof(unsigned) * nb);
  if (rc) return rc;
  unsigned *bsum = (unsigned *)W.bsum.p;
  hipLaunchKernelGGL(map::k_scan_reduce, dim3(nb), dim3(map::kBlock), 0, st, a, n, bsum);
  hipLaunchKernelGGL(map::k_scan_blocks, dim3(1), dim3(map::kBlock), 0, st, bsum, nb, grand);
  hipLaunchKernelGGL(map::k_scan_apply, dim3(nb), dim3(map::kBlock), 0, st, a, n, bsum);
  HIP_TRY(hipGetLastError());
  return DVO_AMD_OK;
}

// Sorts the m points the input stage left in keys[0] / vals[0] (c: the control block it filled, read back) by voxel key and
// finds the voxels: *cur = the buffer pair that holds the sorted (dense key, value), W.flags = the voxel index of every sorted
// position (k_accum), *n_vox = the voxels, *rk = how the dense keys were formed.  Events 2..3 time the segment.
int sort_voxels(MapWorkspace &W, const map::MapCtrl &c, hipStream_t st, int *cur_out, unsigned *n_vox, map::Rekey *rk) {
  const unsigned m = (unsigned)c.kept;
  // the bits present: fields i | j | k of (index - min), packed densely -- order preserving
  const int bi = bits_for(c.mx[0] - c.mn[0]), bj = bits_for(c.mx[1] - c.mn[1]), bk = bits_for(c.mx[2] - c.mn[2]);
  map::Rekey r = {{c.mn[0], c.mn[1], c.mn[2]}, bj + bk, bk};
  const int passes = (bi + bj + bk + map::kRadixBits - 1) / map::kRadixBits;
  const unsigned nb = (m + map::kSortTile - 1) / map::kSortTile;
  int rc = grow_ws(W.counts, sizeof(unsigned) * map::kRadix * (size_t)nb);
  // the scan scratch for the larger of the two scans (the digit table, the head flags), before anything is enqueued
  if (!rc) rc = grow_ws(W.bsum, sizeof(unsigned) * (std::max<size_t>((size_t)map::kRadix * nb, m) / map::kScanTile + 1));
  if (rc) return rc;
  unsigned long long *keys[2] = {(unsigned long long *)W.keys[0].p, (unsigned long long *)W.keys[1].p};
  unsigned *vals[2] = {(unsigned *)W.vals[0].p, (unsigned *)W.vals[1].p};
  unsigned *counts = (unsigned *)W.counts.p;
  map::MapCtrl *dctrl = (map::MapCtrl *)W.ctrl.p;
  HIP_TRY(hipEventRecord(W.ev[2], st));
  hipLaunchKernelGGL(map::k_rekey, dim3(map::grid_for(m, map::kBlock)), dim3(map::kBlock), 0, st, keys[0], (unsigned long long)m, r);
  int cur = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = pass * map::kRadixBits;
    hipLaunchKernelGGL(map::k_radix_hist, dim3(nb), dim3(map::kBlock), 0, st, keys[cur], m, shift, counts);
    rc = scan(W, counts, map::kRadix * nb, nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(map::k_radix_scatter, dim3(nb), dim3(map::kBlock), 0, st, keys[cur], vals[cur], keys[cur ^ 1],
                       vals[cur ^ 1], m, shift, (const unsigned *)counts);
    cur ^= 1;
  }
  unsigned *flags = (unsigned *)W.flags.p;
  hipLaunchKernelGGL(map::k_heads, dim3(map::grid_for(m, map::kBlock)), dim3(map::kBlock), 0, st, keys[cur], m, flags);
  rc = scan(W, flags, m, &dctrl->voxels, st);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(W.ev[3], st));
  HIP_TRY(hipMemcpyAsync(n_vox, &dctrl->voxels, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *cur_out = cur, *rk = r;
  return DVO_AMD_OK;
}

// The aggregate of the m points the input stage left in keys[0] / vals[0] (c: the control block it filled, read back): sorts,
// finds the voxels, checks the capacity, reduces and copies the voxels to `out`.  Events 2..5 time the two kernel segments.
int reduce_voxels(MapWorkspace &W, const map::MapCtrl &c, const float4 *pts, dvo_amd_point *out, long long capacity,
                  dvo_amd_cloud_stats *stats, hipStream_t st) {
  const unsigned m = (unsigned)c.kept;
  unsigned n_vox = 0;
  if (m > 0) {
    int cur = 0;
    map::Rekey r;
    int rc = sort_voxels(W, c, st, &cur, &n_vox, &r);
    if (rc) return rc;
    const unsigned long long *const keys[2] = {(unsigned long long *)W.keys[0].p, (unsigned long long *)W.keys[1].p};
    const unsigned *const vals[2] = {(unsigned *)W.vals[0].p, (unsigned *)W.vals[1].p};
    const unsigned *flags = (unsigned *)W.flags.p;
    if ((long long)n_vox <= capacity && out) {
      rc = grow_ws(W.acc, sizeof(map::VoxelAcc) * (size_t)n_vox);
      if (!rc) rc = grow_ws(W.out, sizeof(float4) * (size_t)n_vox);
      if (rc) return rc;
      map::VoxelAcc *acc = (map::VoxelAcc *)W.acc.p;
      HIP_TRY(hipEventRecord(W.ev[4], st));
      HIP_TRY(hipMemsetAsync(acc, 0, sizeof(map::VoxelAcc) * (size_t)n_vox, st));
      const unsigned long long threads = ((unsigned long long)m + map::kAccumChunk - 1) / map::kAccumChunk;
      hipLaunchKernelGGL(map::k_accum, dim3((unsigned)((threads + map::kBlock - 1) / map::kBlock)), dim3(map::kBlock), 0, st,
                         keys[cur], vals[cur], flags, m, pts, acc, n_vox);
      hipLaunchKernelGGL(map::k_voxel_out, dim3(map::grid_for(n_vox, map::kBlock)), dim3(map::kBlock), 0, st, acc, n_vox,
                         (float4 *)W.out.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(W.ev[5], st));
    }
  }
  if (stats) stats->voxels = n_vox;
  if ((long long)n_vox > capacity) {
    g_last_error = "voxel aggregate: " + std::to_string(n_vox) + " voxels, capacity " + std::to_string(capacity);
    return DVO_AMD_ERR_CAPACITY;
  }
  if (n_vox > 0) {
    HIP_TRY(hipEventRecord(W.ev[6], st));
    HIP_TRY(hipMemcpyAsync(out, W.out.p, sizeof(float4) * (size_t)n_vox, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(W.ev[7], st));
    HIP_TRY(hipStreamSynchronize(st));
    float a = 0.f, b = 0.f, d = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, W.ev[2], W.ev[3]));
    HIP_TRY(hipEventElapsedTime(&b, W.ev[4], W.ev[5]));
    HIP_TRY(hipEventElapsedTime(&d, W.ev[6], W.ev[7]));
    W.device_ms += a + b;
    W.copy_ms = d;
  }
  return DVO_AMD_OK;
}

// the control block before an input stage, and its read-back into the stats
int start_ctrl(MapWorkspace &W, hipStream_t st) {
  int rc = grow_ws(W.ctrl, sizeof(map::MapCtrl));
  if (rc) return rc;
  map::MapCtrl c;
  std::memset(&c, 0, sizeof(c));
  for (int a = 0; a < 3; ++a) c.mn[a] = INT_MAX, c.mx[a] = INT_MIN;
  HIP_TRY(hipMemcpyAsync(W.ctrl.p, &c, sizeof(c), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(W.ev[0], st));
  return DVO_AMD_OK;
}

int read_ctrl(MapWorkspace &W, map::MapCtrl *c, long long points_in, dvo_amd_cloud_stats *stats, hipStream_t st) {
  HIP_TRY(hipEventRecord(W.ev[1], st));
  HIP_TRY(hipMemcpyAsync(c, W.ctrl.p, sizeof(*c), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
  W.device_ms = ms, W.copy_ms = 0.0, W.points = points_in;
  if (stats) {
    stats->points_in = points_in;
    stats->finite = (long long)c->finite;
    stats->out_of_range = (long long)c->out_of_range;
    stats->voxels = 0;
  }
  return DVO_AMD_OK;
}

// the per-point buffers of the sort for n points
int grow_points(MapWorkspace &W, size_t n, bool pts) {
  int rc = DVO_AMD_OK;
  for (int b = 0; b < 2 && !rc; ++b) rc = grow_ws(W.keys[b], 8 * n), rc = rc ? rc : grow_ws(W.vals[b], 4 * n);
  if (!rc) rc = grow_ws(W.flags, 4 * n);
  if (!rc && pts) rc = grow_ws(W.pts, 16 * n);
  return rc;
}

// the image descriptors of a call (and its BGR planes, packed to w * 3 bytes per row) on the device
int upload_images(MapWorkspace &W, int n, dvo_amd_pyramid *const *images, int level, const double *poses, int pose_stride,
                  const unsigned char *const *bgrs, const int *bgr_strides, std::vector<map::MapImage> &host, hipStream_t st) {
  host.resize((size_t)n);
  size_t bgr_bytes = 0;
  for (int k = 0; k < n; ++k) {
    const LevelData &L = images[k]->lv[level];
    map::MapImage &im = host[(size_t)k];
    im.z = L.z_plane, im.i = L.i_plane, im.tx = L.tx, im.ty = L.ty, im.bgr = nullptr, im.w = L.w, im.h = L.h, im.neg = 0;
    float_pose(poses ? poses + (size_t)pose_stride * k : nullptr, im.T);
    if (bgrs && bgrs[k]) bgr_bytes += (size_t)L.w * L.h * 3;
  }
  int rc = grow_ws(W.images, sizeof(map::MapImage) * std::max(1, n));
  if (!rc && bgr_bytes) rc = grow_ws(W.bgr, bgr_bytes);
  if (rc) return rc;
  size_t at = 0;
  for (int k = 0; k < n; ++k) {
    if (!bgrs || !bgrs[k]) continue;
    map::MapImage &im = host[(size_t)k];
    unsigned char *dst = (unsigned char *)W.bgr.p + at;
    const int stride = bgr_strides ? bgr_strides[k] : im.w * 3;
    if (stride < im.w * 3) return DVO_AMD_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)im.w * 3, bgrs[k], (size_t)stride, (size_t)im.w * 3, im.h, hipMemcpyHostToDevice, st));
    im.bgr = dst;
    at += (size_t)im.w * im.h * 3;
  }
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(W.images.p, host.data(), sizeof(map::MapImage) * n, hipMemcpyHostToDevice, st));
  return DVO_AMD_OK;
}

int check_images(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *images, int level) {
  for (int k = 0; k < n; ++k) {
    if (!images[k]) return DVO_AMD_ERR_INVALID_ARGUMENT;
    if (level >= images[k]->n_levels) return DVO_AMD_ERR_TOO_FEW_LEVELS;
    if (images[k]->device != ctx->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  }
  return DVO_AMD_OK;
}

}  // namespace

void map_workspace_release(dvo_amd_context *ctx) {
  MapWorkspace *w = ctx->map_ws;
  if (!w) return;
  for (MapWorkspace::Buf *b : {&w->pts, &w->keys[0], &w->keys[1], &w->vals[0], &w->vals[1], &w->flags, &w->counts, &w->bsum,
                               &w->acc, &w->out, &w->bgr, &w->images, &w->ctrl, &w->zbuf, &w->planes})
    if (b->p) (void)hipFree(b->p);
  for (hipEvent_t e : w->ev)
    if (e) (void)hipEventDestroy(e);
  delete w;
  ctx->map_ws = nullptr;
}

}  // namespace host
}  // namespace dvo_amd

// ---- the persistent keyframe map ------------------------------------------------------------------------------------------

struct dvo_amd_map {
  struct Keyframe {
    int id = 0;
    dvo_amd_pyramid *pyr = nullptr;  // retained
    float T[12] = {};                // the pose its contribution was generated at
    void *bgr = nullptr;             // device, tight rows; null: grey
    long long points = 0, finite = 0, out_of_range = 0;
  };
  using Buf = dvo_amd::host::MapWorkspace::Buf;
  dvo_amd_context *ctx = nullptr;
  float leaf = 0.0f;
  std::vector<Keyframe> kfs;
  Buf keys[2], acc[2];             // the store, double-buffered: keys[cur] / acc[cur] hold n voxels in ascending key order
  Buf tkeys, tacc, flags;          // the merged sequence before compaction, its flags (and the box flags of an extract)
  Buf dkeys, counts, images;       // the delta's keys; (finite, out of range) per image; the image descriptors
  int cur = 0;
  unsigned n = 0;
  hipEvent_t ev[4] = {};
  double device_ms = 0.0, copy_ms = 0.0;  // the last call
  long long delta_points = 0, delta_voxels = 0;
};

namespace dvo_amd {
namespace host {
namespace {

// one image of an update: a keyframe at a pose, added or subtracted
struct DeltaItem {
  const dvo_amd_map::Keyframe *kf;
  float T[12];
  bool negative;
  int stats_of;  // index into the next keyframe list whose totals this pass produces; -1: none
};

// the store buffers grow geometrically: a session that gains a keyframe at a time reallocates O(log) times
int grow_store(MapWorkspace::Buf &b, size_t bytes) { return bytes <= b.bytes ? DVO_AMD_OK : grow_ws(b, std::max(bytes, 2 * b.bytes)); }

int find_keyframe(const dvo_amd_map *M, int id) {
  for (size_t k = 0; k < M->kfs.size(); ++k)
    if (M->kfs[k].id == id) return (int)k;
  return -1;
}

int entry_checks(const dvo_amd_map *M, const char *what) {
  int rc = have_device();
  if (rc) return rc;
  if (!M) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = queue_must_be_idle(M->ctx, what);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(M->ctx->device));
  return DVO_AMD_OK;
}

// The merge of an update, enqueued on the stream: k_merge over the store (ka, va: na entries) and the delta (kb, vb: nb entries)
// into the na + nb merged positions (kt, vt, flags), the scan of the flags (their total lands in the control block's voxels)
// and k_compact into (ko, vo).  W.ctrl and W.bsum must already hold the control block and the scan scratch of na + nb entries.
int merge_launches(MapWorkspace &W, const unsigned long long *ka, const map::VoxelAcc *va, unsigned na,
                   const unsigned long long *kb, const map::VoxelAcc *vb, unsigned nb, unsigned long long *kt, map::VoxelAcc *vt,
                   unsigned *flags, unsigned long long *ko, map::VoxelAcc *vo, hipStream_t st) {
  const unsigned long long merged = (unsigned long long)na + nb;
  map::MapCtrl *dctrl = (map::MapCtrl *)W.ctrl.p;
  hipLaunchKernelGGL(map::k_merge, dim3((unsigned)((merged + map::kMergeTile - 1) / map::kMergeTile)), dim3(map::kBlock), 0, st,
                     ka, va, na, kb, vb, nb, kt, vt, flags);
  const int rc = scan(W, flags, (unsigned)merged, &dctrl->voxels, st);
  if (rc) return rc;
  hipLaunchKernelGGL(map::k_compact, dim3(map::grid_for(4 * merged, map::kBlock)), dim3(map::kBlock), 0, st,
                     (const unsigned long long *)kt, (const map::VoxelAcc *)vt, (const unsigned *)flags,
                     (const unsigned *)&dctrl->voxels, (unsigned)merged, ko, vo);
  HIP_TRY(hipGetLastError());
  return DVO_AMD_OK;
}

// Applies the items to the store (from_scratch: to an empty store) and, when everything succeeded, makes `next` the keyframe
// list.  Until then the map is untouched: the merge writes the other store buffer.
int apply_delta(dvo_amd_map *M, const std::vector<DeltaItem> &items, bool from_scratch, std::vector<dvo_amd_map::Keyframe> &next) {
  dvo_amd_context *ctx = M->ctx;
  MapWorkspace *Wp = nullptr;
  int rc = workspace(ctx, &Wp);
  if (rc) return rc;
  MapWorkspace &W = *Wp;
  const hipStream_t st = ctx->stream;
  unsigned long long total = 0;
  int max_px = 1;
  for (const DeltaItem &it : items) {
    total += (unsigned long long)it.kf->points;
    max_px = (int)std::max<long long>(max_px, it.kf->points);
  }
  if (total > (1ull << 31)) {
    g_last_error = "keyframe map: more than 2^31 points in one update";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  const unsigned n_store = from_scratch ? 0u : M->n;
  unsigned n_delta = 0, n_new = n_store;
  double device_ms = 0.0;
  const int n_items = (int)items.size();
  if (n_items > 0) {
    rc = grow_points(W, std::max<size_t>(1, total), true);
    if (!rc) rc = grow_ws(M->images, sizeof(map::MapImage) * (size_t)n_items);
    if (!rc) rc = grow_ws(M->counts, 2 * sizeof(unsigned long long) * (size_t)n_items);
    if (rc) return rc;
    std::vector<map::MapImage> im((size_t)n_items);
    for (int k = 0; k < n_items; ++k) {
      const LevelData &L = items[(size_t)k].kf->pyr->lv[0];
      map::MapImage &d = im[(size_t)k];
      d.z = L.z_plane, d.i = L.i_plane, d.tx = L.tx, d.ty = L.ty, d.bgr = (const unsigned char *)items[(size_t)k].kf->bgr;
      d.w = L.w, d.h = L.h, d.neg = items[(size_t)k].negative ? map::kNegBit : 0u;
      std::memcpy(d.T, items[(size_t)k].T, sizeof(d.T));
    }
    HIP_TRY(hipMemcpyAsync(M->images.p, im.data(), sizeof(map::MapImage) * (size_t)n_items, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(M->counts.p, 0, 2 * sizeof(unsigned long long) * (size_t)n_items, st));
    rc = start_ctrl(W, st);
    if (rc) return rc;
    const float inv = 1.0f / M->leaf;
    for (int k0 = 0; k0 < n_items; k0 += 65535) {
      const int nk = std::min(65535, n_items - k0);
      hipLaunchKernelGGL(map::k_map_keys, dim3(map::grid_for(max_px, map::kBlock, 64), nk), dim3(map::kBlock), 0, st,
                         (const map::MapImage *)M->images.p, k0, inv, (float4 *)W.pts.p, (unsigned long long *)W.keys[0].p,
                         (unsigned *)W.vals[0].p, (map::MapCtrl *)W.ctrl.p, (unsigned long long *)M->counts.p);
    }
    HIP_TRY(hipGetLastError());
    map::MapCtrl c;
    rc = read_ctrl(W, &c, (long long)total, nullptr, st);
    if (rc) return rc;
    device_ms = W.device_ms;
    std::vector<unsigned long long> counts(2 * (size_t)n_items);
    HIP_TRY(hipMemcpyAsync(counts.data(), M->counts.p, sizeof(unsigned long long) * counts.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n_items; ++k) {
      const int at = items[(size_t)k].stats_of;
      if (at < 0) continue;
      next[(size_t)at].finite = (long long)counts[2 * (size_t)k];
      next[(size_t)at].out_of_range = (long long)counts[2 * (size_t)k + 1];
    }
    if (c.kept > 0) {
      int cur = 0;
      map::Rekey r;
      rc = sort_voxels(W, c, st, &cur, &n_delta, &r);
      if (!rc) rc = grow_ws(W.acc, sizeof(map::VoxelAcc) * (size_t)n_delta);
      if (!rc) rc = grow_ws(M->dkeys, sizeof(unsigned long long) * (size_t)n_delta);
      if (rc) return rc;
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, W.ev[2], W.ev[3]));
      device_ms += ms;
      const unsigned m = (unsigned)c.kept;
      map::VoxelAcc *acc = (map::VoxelAcc *)W.acc.p;
      HIP_TRY(hipEventRecord(M->ev[0], st));
      HIP_TRY(hipMemsetAsync(acc, 0, sizeof(map::VoxelAcc) * (size_t)n_delta, st));
      const unsigned long long threads = ((unsigned long long)m + map::kAccumChunk - 1) / map::kAccumChunk;
      hipLaunchKernelGGL(map::k_accum, dim3((unsigned)((threads + map::kBlock - 1) / map::kBlock)), dim3(map::kBlock), 0, st,
                         (const unsigned long long *)W.keys[cur].p, (const unsigned *)W.vals[cur].p, (const unsigned *)W.flags.p, m,
                         (const float4 *)W.pts.p, acc, n_delta);
      hipLaunchKernelGGL(map::k_delta_keys, dim3(map::grid_for(m, map::kBlock)), dim3(map::kBlock), 0, st,
                         (const unsigned long long *)W.keys[cur].p, (const unsigned *)W.flags.p, m, r,
                         (unsigned long long *)M->dkeys.p, n_delta);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(M->ev[1], st));
    }
  }
  const unsigned long long merged = (unsigned long long)n_store + n_delta;
  if (merged >= (1ull << 31)) {
    g_last_error = "keyframe map: 2^31 voxels or more";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  const bool merge = n_delta > 0;
  if (merge) {
    const int other = M->cur ^ 1;
    rc = grow_store(M->keys[other], 8 * (size_t)merged);
    if (!rc) rc = grow_store(M->acc[other], sizeof(map::VoxelAcc) * (size_t)merged);
    if (!rc) rc = grow_store(M->tkeys, 8 * (size_t)merged);
    if (!rc) rc = grow_store(M->tacc, sizeof(map::VoxelAcc) * (size_t)merged);
    if (!rc) rc = grow_store(M->flags, 4 * (size_t)merged);
    if (!rc) rc = grow_ws(W.bsum, sizeof(unsigned) * ((size_t)merged / map::kScanTile + 1));
    if (rc) return rc;
    map::MapCtrl *dctrl = (map::MapCtrl *)W.ctrl.p;
    HIP_TRY(hipEventRecord(M->ev[2], st));
    rc = merge_launches(W, (const unsigned long long *)M->keys[M->cur].p, (const map::VoxelAcc *)M->acc[M->cur].p, n_store,
                        (const unsigned long long *)M->dkeys.p, (const map::VoxelAcc *)W.acc.p, n_delta,
                        (unsigned long long *)M->tkeys.p, (map::VoxelAcc *)M->tacc.p, (unsigned *)M->flags.p,
                        (unsigned long long *)M->keys[other].p, (map::VoxelAcc *)M->acc[other].p, st);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(M->ev[3], st));
    HIP_TRY(hipMemcpyAsync(&n_new, &dctrl->voxels, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, M->ev[0], M->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, M->ev[2], M->ev[3]));
    device_ms += a + b;
    M->cur = other;
  } else if (from_scratch) {
    n_new = 0;
  }
  M->n = n_new;
  M->kfs.swap(next);
  M->device_ms = device_ms, M->copy_ms = 0.0, M->delta_points = (long long)total, M->delta_voxels = n_delta;
  return DVO_AMD_OK;
}

// the device planes of a rendered view (null where not asked for)
struct RenderPlanes {
  float *depth = nullptr;
  unsigned *rgb = nullptr;
  float *intensity = nullptr;
  int *index = nullptr;
};

// the world -> camera transform of a view as the device takes it (dvo_amd.h, rule 2): the inverse of a rigid pose in double,
// every product and sum rounded on its own, then cast to float
void inverse_pose(const double *pose, float T[12]) {
  static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double *P = pose ? pose : kIdentity;  // column-major: R[i][j] = P[j * 4 + i], t[i] = P[12 + i]
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)P[r * 4 + c];  // Ri[r][c] = R[c][r]
    T[r * 4 + 3] = (float)-((P[r * 4 + 0] * P[12] + P[r * 4 + 1] * P[13]) + P[r * 4 + 2] * P[14]);
  }
}

int check_view(const dvo_amd_map *M, const double *pose, const dvo_amd_view *v, const char *what) {
  const char *why = nullptr;
  if (!v) return DVO_AMD_ERR_INVALID_ARGUMENT;
  if (v->width < 1 || v->height < 1 || (long long)v->width * v->height > (1ll << 26)) why = "width and height must be >= 1 and width*height <= 2^26";
  else if (!(std::isfinite(v->fx) && v->fx > 0.0f && std::isfinite(v->fy) && v->fy > 0.0f)) why = "fx and fy must be finite and positive";
  else if (!std::isfinite(v->ox) || !std::isfinite(v->oy)) why = "ox and oy must be finite";
  else if (!std::isfinite(v->near_z) || !(v->near_z > 0.0f)) why = "near_z must be finite and positive";
  else if (pose && !finite_all(pose, 16)) why = "the pose has a non-finite entry";
  else if (v->near_z < (M->leaf * std::max(v->fx, v->fy)) / 32.0f)
    why = "near_z is below leaf_size * max(fx, fy) / 32: a voxel at near_z would cover more than 32 pixels a side";
  if (!why) return DVO_AMD_OK;
  g_last_error = std::string(what) + ": " + why;
  return DVO_AMD_ERR_INVALID_ARGUMENT;
}

// Enqueues a render on the context's stream: clear, splat, resolve into the workspace's planes (`want`: bit 0 depth, 1 rgb,
// 2 intensity, 3 index), the control block into *ctrl.  The caller synchronises.  M->ev[0..1] time the kernels.
int render_launches(dvo_amd_map *M, const double *pose, const dvo_amd_view *view, unsigned want, RenderPlanes *planes,
                    map::RenderCtrl *ctrl) {
  MapWorkspace *Wp = nullptr;
  int rc = workspace(M->ctx, &Wp);
  if (rc) return rc;
  MapWorkspace &W = *Wp;
  const size_t n_px = (size_t)view->width * view->height;
  rc = grow_ws(W.zbuf, 8 * (n_px + 1));  // (cleared 16 bytes at a time)
  if (!rc) rc = grow_ws(W.planes, 16 * n_px);
  if (!rc) rc = grow_ws(W.ctrl, std::max(sizeof(map::MapCtrl), sizeof(map::RenderCtrl)));
  if (rc) return rc;
  map::RenderView V;
  V.w = view->width, V.h = view->height, V.fx = view->fx, V.fy = view->fy, V.ox = view->ox, V.oy = view->oy;
  V.near_z = view->near_z, V.leaf = M->leaf;
  inverse_pose(pose, V.T);
  float *base = (float *)W.planes.p;
  if (want & 1u) planes->depth = base;
  if (want & 2u) planes->rgb = (unsigned *)(base + n_px);
  if (want & 4u) planes->intensity = base + 2 * n_px;
  if (want & 8u) planes->index = (int *)(base + 3 * n_px);
  const hipStream_t st = M->ctx->stream;
  unsigned long long *zbuf = (unsigned long long *)W.zbuf.p;
  map::RenderCtrl *dctrl = (map::RenderCtrl *)W.ctrl.p;
  const map::VoxelAcc *acc = (const map::VoxelAcc *)M->acc[M->cur].p;
  HIP_TRY(hipEventRecord(M->ev[0], st));
  HIP_TRY(hipMemsetAsync(dctrl, 0, sizeof(map::RenderCtrl), st));
  hipLaunchKernelGGL(map::k_render_clear, dim3(map::grid_for((n_px + 1) / 2, map::kBlock)), dim3(map::kBlock), 0, st, (ulonglong2 *)zbuf,
                     (unsigned long long)((n_px + 1) / 2));
  if (M->n > 0)
    hipLaunchKernelGGL(map::k_render_splat, dim3(map::grid_for(M->n, map::kBlock)), dim3(map::kBlock), 0, st, acc, M->n, V, zbuf, dctrl);
  hipLaunchKernelGGL(map::k_render_resolve, dim3(map::grid_for(n_px, map::kBlock)), dim3(map::kBlock), 0, st,
                     (const unsigned long long *)zbuf, (unsigned long long)n_px, acc, M->n, planes->depth, planes->rgb,
                     planes->intensity, planes->index, dctrl);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(M->ev[1], st));
  HIP_TRY(hipMemcpyAsync(ctrl, dctrl, sizeof(*ctrl), hipMemcpyDeviceToHost, st));
  return DVO_AMD_OK;
}

void render_stats(const dvo_amd_map *M, const map::RenderCtrl &c, dvo_amd_render_stats *stats) {
  if (!stats) return;
  stats->voxels = M->n;
  stats->behind_near = (long long)c.behind_near, stats->outside = (long long)c.outside, stats->drawn = (long long)c.drawn;
  stats->covered_pixels = (long long)c.covered;
}

}  // namespace
}  // namespace host
}  // namespace dvo_amd

extern "C" {

int dvo_amd_map_create(dvo_amd_context *ctx, float leaf_size, dvo_amd_map **out) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx || !out || !host::valid_leaf(leaf_size)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  dvo_amd_map *M = new dvo_amd_map();
  M->ctx = ctx, M->leaf = leaf_size;
  for (hipEvent_t &e : M->ev) {
    const hipError_t he = hipEventCreate(&e);
    if (he != hipSuccess) {
      dvo_amd_map_destroy(M);
      return host::fail_hip("hipEventCreate (keyframe map)", he);
    }
  }
  *out = M;
  return DVO_AMD_OK;
}

void dvo_amd_map_destroy(dvo_amd_map *M) {
  if (!M) return;
  (void)hipSetDevice(M->ctx->device);
  (void)hipStreamSynchronize(M->ctx->stream);
  for (dvo_amd_map::Keyframe &k : M->kfs) {
    if (k.bgr) (void)hipFree(k.bgr);
    dvo_amd_pyramid_release(k.pyr);
  }
  for (dvo_amd_map::Buf *b : {&M->keys[0], &M->keys[1], &M->acc[0], &M->acc[1], &M->tkeys, &M->tacc, &M->flags, &M->dkeys, &M->counts,
                              &M->images})
    if (b->p) (void)hipFree(b->p);
  for (hipEvent_t e : M->ev)
    if (e) (void)hipEventDestroy(e);
  delete M;
}

int dvo_amd_map_insert(dvo_amd_map *M, int id, dvo_amd_pyramid *image, const double *pose, const unsigned char *bgr,
                       int bgr_stride_bytes) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!M || !image) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = host::check_images(M->ctx, 1, &image, 0);
  if (!rc) rc = host::entry_checks(M, "dvo_amd_map_insert");
  if (rc) return rc;
  if (host::find_keyframe(M, id) >= 0) {
    g_last_error = "dvo_amd_map_insert: keyframe id " + std::to_string(id) + " is already in the map";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  if (pose && !host::finite_all(pose, 16)) {
    g_last_error = "dvo_amd_map_insert: the pose of keyframe " + std::to_string(id) + " has a non-finite entry";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  const LevelData &L = image->lv[0];
  const int stride = bgr_stride_bytes > 0 ? bgr_stride_bytes : L.w * 3;
  if (bgr && stride < L.w * 3) {
    g_last_error = "dvo_amd_map_insert: bgr_stride_bytes is smaller than a row";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  dvo_amd_map::Keyframe kf;
  kf.id = id, kf.pyr = image, kf.points = (long long)L.w * L.h;
  host::float_pose(pose, kf.T);
  const hipStream_t st = M->ctx->stream;
  if (bgr) {
    const hipError_t e = hipMalloc(&kf.bgr, (size_t)L.w * L.h * 3);
    if (e == hipErrorOutOfMemory) return DVO_AMD_ERR_OUT_OF_MEMORY;
    if (e != hipSuccess) return host::fail_hip("hipMalloc (keyframe map, bgr)", e);
    const hipError_t c = hipMemcpy2DAsync(kf.bgr, (size_t)L.w * 3, bgr, (size_t)stride, (size_t)L.w * 3, L.h, hipMemcpyHostToDevice, st);
    if (c != hipSuccess) {
      (void)hipFree(kf.bgr);
      return host::fail_hip("hipMemcpy2DAsync (keyframe map, bgr)", c);
    }
  }
  std::vector<dvo_amd_map::Keyframe> next = M->kfs;
  next.push_back(kf);
  std::vector<host::DeltaItem> items(1);
  items[0].kf = &kf, items[0].negative = false, items[0].stats_of = (int)next.size() - 1;
  std::memcpy(items[0].T, kf.T, sizeof(kf.T));
  rc = host::apply_delta(M, items, false, next);
  if (rc) {
    (void)hipStreamSynchronize(st);  // the copy of the caller's image may still be in flight
    if (kf.bgr) (void)hipFree(kf.bgr);
    return rc;
  }
  dvo_amd_pyramid_retain(image);
  return DVO_AMD_OK;
}

int dvo_amd_map_set_poses(dvo_amd_map *M, int n, const int *ids, const double *poses) {
  int rc = host::entry_checks(M, "dvo_amd_map_set_poses");
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!ids || !poses))) return DVO_AMD_ERR_INVALID_ARGUMENT;
  std::vector<dvo_amd_map::Keyframe> next = M->kfs;
  std::vector<int> moved;
  std::vector<char> seen(next.size(), 0);
  long long moved_points = 0, all_points = 0;
  for (const dvo_amd_map::Keyframe &k : next) all_points += k.points;
  for (int q = 0; q < n; ++q) {
    const int at = host::find_keyframe(M, ids[q]);
    if (at < 0 || seen[(size_t)at] || !host::finite_all(poses + 16 * (size_t)q, 16)) {
      g_last_error = "dvo_amd_map_set_poses: keyframe id " + std::to_string(ids[q]) +
                     (at < 0 ? " is not in the map" : seen[(size_t)at] ? " is given twice" : " has a non-finite pose entry");
      return DVO_AMD_ERR_INVALID_ARGUMENT;
    }
    seen[(size_t)at] = 1;
    float T[12];
    host::float_pose(poses + 16 * (size_t)q, T);
    if (std::memcmp(T, next[(size_t)at].T, sizeof(T)) == 0) continue;  // the same float pose: the same contribution
    std::memcpy(next[(size_t)at].T, T, sizeof(T));
    moved.push_back(at);
    moved_points += next[(size_t)at].points;
  }
  if (moved.empty()) return DVO_AMD_OK;
  // a delta of more points than the whole map holds: build the store again from every keyframe instead
  const bool rebuild = 2 * moved_points > all_points;
  std::vector<host::DeltaItem> items;
  if (rebuild) {
    for (size_t k = 0; k < next.size(); ++k) {
      host::DeltaItem it;
      it.kf = &M->kfs[k], it.negative = false, it.stats_of = (int)k;
      std::memcpy(it.T, next[k].T, sizeof(it.T));
      items.push_back(it);
    }
  } else {
    for (int at : moved) {
      host::DeltaItem it;
      it.kf = &M->kfs[(size_t)at], it.negative = true, it.stats_of = -1;
      std::memcpy(it.T, M->kfs[(size_t)at].T, sizeof(it.T));
      items.push_back(it);
      it.negative = false, it.stats_of = at;
      std::memcpy(it.T, next[(size_t)at].T, sizeof(it.T));
      items.push_back(it);
    }
  }
  return host::apply_delta(M, items, rebuild, next);
}

int dvo_amd_map_remove(dvo_amd_map *M, int n, const int *ids) {
  int rc = host::entry_checks(M, "dvo_amd_map_remove");
  if (rc) return rc;
  if (n < 0 || (n > 0 && !ids)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  std::vector<char> gone(M->kfs.size(), 0);
  std::vector<host::DeltaItem> items;
  for (int q = 0; q < n; ++q) {
    const int at = host::find_keyframe(M, ids[q]);
    if (at < 0 || gone[(size_t)at]) {
      g_last_error = "dvo_amd_map_remove: keyframe id " + std::to_string(ids[q]) + (at < 0 ? " is not in the map" : " is given twice");
      return DVO_AMD_ERR_INVALID_ARGUMENT;
    }
    gone[(size_t)at] = 1;
    host::DeltaItem it;
    it.kf = &M->kfs[(size_t)at], it.negative = true, it.stats_of = -1;
    std::memcpy(it.T, M->kfs[(size_t)at].T, sizeof(it.T));
    items.push_back(it);
  }
  if (items.empty()) return DVO_AMD_OK;
  std::vector<dvo_amd_map::Keyframe> next, removed;
  for (size_t k = 0; k < M->kfs.size(); ++k) (gone[k] ? removed : next).push_back(M->kfs[k]);
  rc = host::apply_delta(M, items, false, next);  // (on success `next` holds the old list: the items stay valid throughout)
  if (rc) return rc;
  for (dvo_amd_map::Keyframe &k : removed) {
    if (k.bgr) (void)hipFree(k.bgr);
    dvo_amd_pyramid_release(k.pyr);
  }
  return DVO_AMD_OK;
}

int dvo_amd_map_stats(const dvo_amd_map *M, dvo_amd_cloud_stats *stats, int *n_keyframes) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!M) return DVO_AMD_ERR_INVALID_ARGUMENT;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    for (const dvo_amd_map::Keyframe &k : M->kfs)
      stats->points_in += k.points, stats->finite += k.finite, stats->out_of_range += k.out_of_range;
    stats->voxels = M->n;
  }
  if (n_keyframes) *n_keyframes = (int)M->kfs.size();
  return DVO_AMD_OK;
}

int dvo_amd_map_extract(dvo_amd_map *M, const float *box, dvo_amd_point *out, long long capacity, long long *n_out) {
  int rc = host::entry_checks(M, "dvo_amd_map_extract");
  if (rc) return rc;
  if (capacity < 0 || (capacity > 0 && !out)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  map::Box bx = {};
  if (box) {
    for (int a = 0; a < 3; ++a) {
      if (!(box[a] < box[a + 3])) {  // NaN included
        g_last_error = "dvo_amd_map_extract: the box needs min < max on every axis";
        return DVO_AMD_ERR_INVALID_ARGUMENT;
      }
      bx.mn[a] = box[a], bx.mx[a] = box[a + 3];
    }
  }
  if (n_out) *n_out = 0;
  M->device_ms = 0.0, M->copy_ms = 0.0, M->delta_points = 0, M->delta_voxels = 0;
  const unsigned n = M->n;
  if (n == 0) return DVO_AMD_OK;
  if (!box && (long long)n > capacity) {
    if (n_out) *n_out = n;
    g_last_error = "dvo_amd_map_extract: " + std::to_string(n) + " voxels, capacity " + std::to_string(capacity);
    return DVO_AMD_ERR_CAPACITY;
  }
  host::MapWorkspace *W = nullptr;
  rc = host::workspace(M->ctx, &W);
  if (!rc) rc = host::grow_ws(W->out, sizeof(float4) * (size_t)n);
  if (!rc && box) rc = host::grow_ws(W->pts, sizeof(float4) * (size_t)n);
  if (!rc && box) rc = host::grow_store(M->flags, 4 * (size_t)n);
  if (!rc && box) rc = host::grow_ws(W->ctrl, sizeof(map::MapCtrl));
  if (!rc && box) rc = host::grow_ws(W->bsum, sizeof(unsigned) * ((size_t)n / map::kScanTile + 1));
  if (rc) return rc;
  const hipStream_t st = M->ctx->stream;
  const float4 *src = (const float4 *)W->out.p;
  unsigned n_ret = n;
  HIP_TRY(hipEventRecord(M->ev[0], st));
  hipLaunchKernelGGL(map::k_voxel_out, dim3(map::grid_for(n, map::kBlock)), dim3(map::kBlock), 0, st,
                     (const map::VoxelAcc *)M->acc[M->cur].p, n, (float4 *)W->out.p);
  if (box) {
    map::MapCtrl *dctrl = (map::MapCtrl *)W->ctrl.p;
    hipLaunchKernelGGL(map::k_box_flags, dim3(map::grid_for(n, map::kBlock)), dim3(map::kBlock), 0, st, src, n, bx,
                       (unsigned *)M->flags.p);
    rc = host::scan(*W, (unsigned *)M->flags.p, n, &dctrl->voxels, st);
    if (rc) return rc;
    hipLaunchKernelGGL(map::k_box_compact, dim3(map::grid_for(n, map::kBlock)), dim3(map::kBlock), 0, st, src,
                       (const unsigned *)M->flags.p, (const unsigned *)&dctrl->voxels, n, (float4 *)W->pts.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(M->ev[1], st));
    HIP_TRY(hipMemcpyAsync(&n_ret, &dctrl->voxels, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    src = (const float4 *)W->pts.p;
    if ((long long)n_ret > capacity) {
      if (n_out) *n_out = n_ret;
      g_last_error = "dvo_amd_map_extract: " + std::to_string(n_ret) + " voxels in the box, capacity " + std::to_string(capacity);
      return DVO_AMD_ERR_CAPACITY;
    }
  } else {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(M->ev[1], st));
  }
  HIP_TRY(hipEventRecord(M->ev[2], st));
  if (n_ret > 0) HIP_TRY(hipMemcpyAsync(out, src, sizeof(float4) * (size_t)n_ret, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(M->ev[3], st));
  HIP_TRY(hipStreamSynchronize(st));
  float a = 0.f, b = 0.f;
  HIP_TRY(hipEventElapsedTime(&a, M->ev[0], M->ev[1]));
  HIP_TRY(hipEventElapsedTime(&b, M->ev[2], M->ev[3]));
  M->device_ms = a, M->copy_ms = b;
  if (n_out) *n_out = n_ret;
  return DVO_AMD_OK;
}

int dvo_amd_map_render(dvo_amd_map *M, const double *pose, const dvo_amd_view *view, float *depth, unsigned int *rgb, float *intensity,
                       int *index, dvo_amd_render_stats *stats) {
  int rc = host::entry_checks(M, "dvo_amd_map_render");
  if (!rc) rc = host::check_view(M, pose, view, "dvo_amd_map_render");
  if (rc) return rc;
  M->device_ms = 0.0, M->copy_ms = 0.0, M->delta_points = 0, M->delta_voxels = 0;
  host::RenderPlanes P;
  map::RenderCtrl c;
  rc = host::render_launches(M, pose, view, (depth ? 1u : 0u) | (rgb ? 2u : 0u) | (intensity ? 4u : 0u) | (index ? 8u : 0u), &P, &c);
  if (rc) return rc;
  const hipStream_t st = M->ctx->stream;
  const size_t bytes = sizeof(float) * (size_t)view->width * view->height;
  HIP_TRY(hipEventRecord(M->ev[2], st));
  if (depth) HIP_TRY(hipMemcpyAsync(depth, P.depth, bytes, hipMemcpyDeviceToHost, st));
  if (rgb) HIP_TRY(hipMemcpyAsync(rgb, P.rgb, bytes, hipMemcpyDeviceToHost, st));
  if (intensity) HIP_TRY(hipMemcpyAsync(intensity, P.intensity, bytes, hipMemcpyDeviceToHost, st));
  if (index) HIP_TRY(hipMemcpyAsync(index, P.index, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(M->ev[3], st));
  HIP_TRY(hipStreamSynchronize(st));
  float a = 0.f, b = 0.f;
  HIP_TRY(hipEventElapsedTime(&a, M->ev[0], M->ev[1]));
  HIP_TRY(hipEventElapsedTime(&b, M->ev[2], M->ev[3]));
  M->device_ms = a, M->copy_ms = b;
  host::render_stats(M, c, stats);
  return DVO_AMD_OK;
}

int dvo_amd_map_render_pyramid(dvo_amd_map *M, const double *pose, const dvo_amd_view *view, int levels, double timestamp,
                               dvo_amd_pyramid **out, dvo_amd_render_stats *stats) {
  int rc = host::entry_checks(M, "dvo_amd_map_render_pyramid");
  if (rc) return rc;
  if (!out) return DVO_AMD_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  rc = host::check_view(M, pose, view, "dvo_amd_map_render_pyramid");
  if (rc) return rc;
  // dvo_amd_pyramid_create_from_device's rule, before anything is rendered
  rc = host::check_levels("dvo_amd_map_render_pyramid", view->width, view->height, levels, " of the levels asked of the view");
  if (rc) return rc;
  M->device_ms = 0.0, M->copy_ms = 0.0, M->delta_points = 0, M->delta_voxels = 0;
  host::RenderPlanes P;
  map::RenderCtrl c;
  rc = host::render_launches(M, pose, view, 1u | 4u, &P, &c);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(M->ctx->stream));
  float a = 0.f;
  HIP_TRY(hipEventElapsedTime(&a, M->ev[0], M->ev[1]));
  M->device_ms = a;
  // the pyramid copies the two planes device to device and builds its levels from them: the workspace is free again on return
  rc = dvo_amd_pyramid_create_from_device(M->ctx->device, P.intensity, P.depth, view->width, view->height, view->width, view->fx,
                                          view->fy, view->ox, view->oy, levels, timestamp, out);
  if (rc) return rc;
  host::render_stats(M, c, stats);
  return DVO_AMD_OK;
}

int dvo_amd_debug_keyframe_map_timing(const dvo_amd_map *M, double *device_ms, double *copy_ms, long long *delta_points,
                                      long long *delta_voxels, int *merge_tile) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!M) return DVO_AMD_ERR_INVALID_ARGUMENT;
  if (device_ms) *device_ms = M->device_ms;
  if (copy_ms) *copy_ms = M->copy_ms;
  if (delta_points) *delta_points = M->delta_points;
  if (delta_voxels) *delta_voxels = M->delta_voxels;
  if (merge_tile) *merge_tile = map::kMergeTile;
  return DVO_AMD_OK;
}

namespace {

// device buffers of one dvo_amd_debug_map_merge call: freed when the call returns, whichever way
struct MergeProbeBuffers {
  host::MapWorkspace::Buf ka, va, kb, vb, kt, vt, flags, ko, vo;
  ~MergeProbeBuffers() {
    for (host::MapWorkspace::Buf *b : {&ka, &va, &kb, &vb, &kt, &vt, &flags, &ko, &vo})
      if (b->p) (void)hipFree(b->p);
  }
};

// ascending, distinct, 63 bits
bool merge_probe_keys_ok(long long n, const unsigned long long *k) {
  for (long long e = 0; e < n; ++e)
    if ((k[e] >> 63) != 0 || (e > 0 && k[e] <= k[e - 1])) return false;
  return true;
}

}  // namespace

int dvo_amd_debug_map_merge(dvo_amd_context *ctx, long long na, const unsigned long long *keys_a, const unsigned long long *acc_a,
                            long long nb, const unsigned long long *keys_b, const unsigned long long *acc_b,
                            unsigned long long *keys_out, unsigned long long *acc_out, long long *n_out) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx || !n_out || na < 0 || nb < 0 || (na > 0 && (!keys_a || !acc_a)) || (nb > 0 && (!keys_b || !acc_b)) ||
      (na + nb > 0 && (!keys_out || !acc_out)))
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if ((unsigned long long)na + (unsigned long long)nb >= (1ull << 31)) {
    g_last_error = "dvo_amd_debug_map_merge: 2^31 entries or more";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  if (!merge_probe_keys_ok(na, keys_a) || !merge_probe_keys_ok(nb, keys_b)) {
    g_last_error = "dvo_amd_debug_map_merge: the keys of each side must be ascending, distinct and below 2^63";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  rc = queue_must_be_idle(ctx, "dvo_amd_debug_map_merge");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n_store = (unsigned)na, n_delta = (unsigned)nb, merged = n_store + n_delta;
  if (merged == 0) return DVO_AMD_OK;
  host::MapWorkspace *W = nullptr;
  rc = host::workspace(ctx, &W);
  MergeProbeBuffers B;
  const size_t acc_bytes = sizeof(map::VoxelAcc);
  if (!rc) rc = host::grow_ws(B.ka, 8 * (size_t)n_store);
  if (!rc) rc = host::grow_ws(B.va, acc_bytes * n_store);
  if (!rc) rc = host::grow_ws(B.kb, 8 * (size_t)n_delta);
  if (!rc) rc = host::grow_ws(B.vb, acc_bytes * n_delta);
  if (!rc) rc = host::grow_ws(B.kt, 8 * (size_t)merged);
  if (!rc) rc = host::grow_ws(B.vt, acc_bytes * merged);
  if (!rc) rc = host::grow_ws(B.flags, 4 * (size_t)merged);
  if (!rc) rc = host::grow_ws(B.ko, 8 * (size_t)merged);
  if (!rc) rc = host::grow_ws(B.vo, acc_bytes * merged);
  if (!rc) rc = host::grow_ws(W->ctrl, sizeof(map::MapCtrl));
  if (!rc) rc = host::grow_ws(W->bsum, sizeof(unsigned) * ((size_t)merged / map::kScanTile + 1));
  if (rc) return rc;
  const hipStream_t st = ctx->stream;
  if (n_store > 0) {
    HIP_TRY(hipMemcpyAsync(B.ka.p, keys_a, 8 * (size_t)n_store, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(B.va.p, acc_a, acc_bytes * n_store, hipMemcpyHostToDevice, st));
  }
  if (n_delta > 0) {
    HIP_TRY(hipMemcpyAsync(B.kb.p, keys_b, 8 * (size_t)n_delta, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(B.vb.p, acc_b, acc_bytes * n_delta, hipMemcpyHostToDevice, st));
  }
  // the launches of an update's merge (host::apply_delta), on the probe's buffers
  map::MapCtrl *dctrl = (map::MapCtrl *)W->ctrl.p;
  rc = host::merge_launches(*W, (const unsigned long long *)B.ka.p, (const map::VoxelAcc *)B.va.p, n_store,
                            (const unsigned long long *)B.kb.p, (const map::VoxelAcc *)B.vb.p, n_delta, (unsigned long long *)B.kt.p,
                            (map::VoxelAcc *)B.vt.p, (unsigned *)B.flags.p, (unsigned long long *)B.ko.p, (map::VoxelAcc *)B.vo.p, st);
  if (rc) {
    (void)hipStreamSynchronize(st);  // before the buffers go
    return rc;
  }
  unsigned n_new = 0;
  hipError_t e = hipMemcpyAsync(&n_new, &dctrl->voxels, sizeof(unsigned), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // before the buffers go, whatever happened
  if (e != hipSuccess || es != hipSuccess) return host::fail_hip("dvo_amd_debug_map_merge", e != hipSuccess ? e : es);
  n_new = std::min(n_new, merged);  // (always: the flags are 0 or 1)
  if (n_new > 0) {
    HIP_TRY(hipMemcpy(keys_out, B.ko.p, 8 * (size_t)n_new, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(acc_out, B.vo.p, acc_bytes * n_new, hipMemcpyDeviceToHost));
  }
  *n_out = n_new;
  return DVO_AMD_OK;
}


int dvo_amd_point_cloud(dvo_amd_context *ctx, dvo_amd_pyramid *image, int level, const double *pose, const unsigned char *bgr,
                        int bgr_stride_bytes, dvo_amd_point *out) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx || !image || !out || level < 0) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = host::check_images(ctx, 1, &image, level);
  if (rc) return rc;
  rc = queue_must_be_idle(ctx, "dvo_amd_point_cloud");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  host::MapWorkspace *W = nullptr;
  rc = host::workspace(ctx, &W);
  if (rc) return rc;
  const hipStream_t st = ctx->stream;
  std::vector<map::MapImage> im;
  const unsigned char *const bgrs[1] = {bgr};
  const int strides[1] = {bgr_stride_bytes};
  rc = host::upload_images(*W, 1, &image, level, pose, 16, bgr ? bgrs : nullptr, strides, im, st);
  if (rc) return rc;
  const size_t n = (size_t)im[0].w * im[0].h;
  rc = host::grow_ws(W->out, 16 * n);
  if (rc) return rc;
  hipLaunchKernelGGL(map::k_cloud, dim3(map::grid_for(n, map::kBlock)), dim3(map::kBlock), 0, st, im[0], (float4 *)W->out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, W->out.p, 16 * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DVO_AMD_OK;
}

int dvo_amd_map_cloud(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *images, const double *poses,
                      const unsigned char *const *bgrs, const int *bgr_strides, float leaf_size, dvo_amd_point *out,
                      long long capacity, dvo_amd_cloud_stats *stats) {
  int rc = host::have_device();
  if (rc) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!ctx || n < 0 || (n > 0 && (!images || !poses)) || capacity < 0 || (capacity > 0 && !out) || !host::valid_leaf(leaf_size))
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = host::check_images(ctx, n, images, 0);
  if (rc) return rc;
  rc = queue_must_be_idle(ctx, "dvo_amd_map_cloud");
  if (rc) return rc;
  unsigned long long total = 0;
  int max_px = 1;
  for (int k = 0; k < n; ++k) {
    total += (unsigned long long)images[k]->lv[0].n;
    max_px = std::max(max_px, images[k]->lv[0].n);
  }
  if (total > (1ull << 31)) {
    g_last_error = "dvo_amd_map_cloud: more than 2^31 points in one call";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  host::MapWorkspace *W = nullptr;
  rc = host::workspace(ctx, &W);
  if (!rc) rc = host::grow_points(*W, std::max<size_t>(1, total), true);
  if (rc) return rc;
  const hipStream_t st = ctx->stream;
  std::vector<map::MapImage> im;
  rc = host::upload_images(*W, n, images, 0, poses, 16, bgrs, bgr_strides, im, st);
  if (!rc) rc = host::start_ctrl(*W, st);
  if (rc) return rc;
  const float inv = 1.0f / leaf_size;
  for (int k0 = 0; k0 < n; k0 += 65535) {
    const int nk = std::min(65535, n - k0);
    hipLaunchKernelGGL(map::k_map_keys, dim3(map::grid_for(max_px, map::kBlock, 64), nk), dim3(map::kBlock), 0, st,
                       (const map::MapImage *)W->images.p, k0, inv, (float4 *)W->pts.p, (unsigned long long *)W->keys[0].p,
                       (unsigned *)W->vals[0].p, (map::MapCtrl *)W->ctrl.p, (unsigned long long *)nullptr);
  }
  HIP_TRY(hipGetLastError());
  map::MapCtrl c;
  rc = host::read_ctrl(*W, &c, (long long)total, stats, st);
  if (rc) return rc;
  return host::reduce_voxels(*W, c, (const float4 *)W->pts.p, out, capacity, stats, st);
}

int dvo_amd_voxel_downsample(dvo_amd_context *ctx, long long n, const dvo_amd_point *in, float leaf_size, dvo_amd_point *out,
                             long long capacity, dvo_amd_cloud_stats *stats) {
  int rc = host::have_device();
  if (rc) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!ctx || n < 0 || (n > 0 && !in) || capacity < 0 || (capacity > 0 && !out) || !host::valid_leaf(leaf_size))
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  if ((unsigned long long)n > (1ull << 31)) {
    g_last_error = "dvo_amd_voxel_downsample: more than 2^31 points in one call";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  rc = queue_must_be_idle(ctx, "dvo_amd_voxel_downsample");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  host::MapWorkspace *W = nullptr;
  rc = host::workspace(ctx, &W);
  if (!rc) rc = host::grow_points(*W, std::max<long long>(1, n), true);
  if (rc) return rc;
  const hipStream_t st = ctx->stream;
  if (n > 0) HIP_TRY(hipMemcpyAsync(W->pts.p, in, 16 * (size_t)n, hipMemcpyHostToDevice, st));
  rc = host::start_ctrl(*W, st);
  if (rc) return rc;
  if (n > 0)
    hipLaunchKernelGGL(map::k_points_keys, dim3(map::grid_for(n, map::kBlock, 2048)), dim3(map::kBlock), 0, st,
                       (const float4 *)W->pts.p, (unsigned long long)n, 1.0f / leaf_size, (unsigned long long *)W->keys[0].p,
                       (unsigned *)W->vals[0].p, (map::MapCtrl *)W->ctrl.p);
  HIP_TRY(hipGetLastError());
  map::MapCtrl c;
  rc = host::read_ctrl(*W, &c, n, stats, st);
  if (rc) return rc;
  return host::reduce_voxels(*W, c, (const float4 *)W->pts.p, out, capacity, stats, st);
}

int dvo_amd_debug_map_timing(dvo_amd_context *ctx, double *device_ms, double *copy_ms, long long *points) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const host::MapWorkspace *W = ctx->map_ws;
  if (device_ms) *device_ms = W ? W->device_ms : 0.0;
  if (copy_ms) *copy_ms = W ? W->copy_ms : 0.0;
  if (points) *points = W ? W->points : 0;
  return DVO_AMD_OK;
}

}  // extern "C"
