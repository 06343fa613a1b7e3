// A truncated signed-distance volume resident on one device: keyframes fused into a dense voxel grid of integer sums, raycast
// into a model view, surface points pulled out of it.  The rules are pinned in include/dvo_amd.h ("A truncated signed-distance
// volume"); tests/volume_ref.py restates them in numpy.  Context-free: the device's prep stream, scratch from the slab pool.
//
// The store: two planes of 8 bytes per voxel, a = {w_sum, sd_sum} and b = {iw_sum, i_sum}, index L = (iz*ny + iy)*nx + ix: a tap of
// the raycast is one 8-byte load.  All sums are unsigned words, i.e. modulo 2^32.
//
//   k_volume_integrate  ONE launch per call, whatever the number of frames: a lane owns one voxel of the union of the frames' index
//                       boxes (dvo_volume_box.h), walks the call's frame records (block-uniform), accumulates the four deltas in
//                       registers and reads and writes each plane once.  A move is two records, -1 at the old pose and +1 at the new.
//                       Counts: ballots per wave, LDS per block, one integer atomicAdd per non-zero count.
//   k_volume_raycast    ONE launch: a wave owns an 8x8 tile of the view, so neighbouring rays read neighbouring voxels; a lane
//                       marches its ray with the fixed step; every corner address comes from a float comparison made before the
//                       conversion to int (g < n-1 is strict: corner +1 is in range).
//   k_volume_count / k_volume_scan / k_volume_write   the surface: crossings per tile of voxels, an exclusive scan of the tile
//                       totals by one block, then every tile recounts, scans inside the block and writes its points in
//                       ascending 3*L + a.  No per-voxel count array exists: a tile is counted twice instead.
//   k_volume_gather / k_volume_scatter   the public records of an index box, packed for the copy to the host and back
//   k_mesh_*            the surface as an indexed triangle mesh (surface nets): see "the mesh" below
#include "dvo_internal.h"
#include "dvo_device_rules.h"
#include "dvo_volume_box.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

namespace dvo_amd {
namespace volume {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kVoxelsPerLane = 8;                  // surface kernels: consecutive voxels a lane walks
constexpr int kTile = kBlock * kVoxelsPerLane;     // ... and a block
constexpr unsigned kNaN = 0x7FC00000u;

struct Geom {
  int nx, ny, nz;
  float voxel, o[3], trunc, near_z, far_z;
  int weight;
};

// one frame of a call as the kernel reads it (block-uniform)
struct FrameRecord {
  const float *z, *i;    // the level's depth and intensity planes
  int w, h;
  float fx, fy, ox, oy;
  float M[12];           // rows 0..2 of world -> camera, row-major
  int lo[3], hi[3];      // the frame's index box, inclusive
  int sign;              // +1 / -1
  int slot;              // where its two counts go (near, free), -1: nowhere
};

using rules::finite_f;

__global__ void __launch_bounds__(kBlock) k_volume_integrate(uint2 *__restrict__ pa, uint2 *__restrict__ pb, Geom G,
                                                             const FrameRecord *__restrict__ records, int n_records, int3 lo, int3 ext,
                                                             unsigned total, unsigned *__restrict__ counts) {
  __shared__ unsigned s_cnt[kWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  const bool live = idx < total;
  int ix = 0, iy = 0, iz = 0;
  if (live) {
    const unsigned row = idx / (unsigned)ext.x;
    ix = lo.x + (int)(idx - row * (unsigned)ext.x);
    const unsigned slab = row / (unsigned)ext.y;
    iy = lo.y + (int)(row - slab * (unsigned)ext.y);
    iz = lo.z + (int)slab;  // (slab < ext.z: idx < total = ext.x*ext.y*ext.z)
  }
  // the voxel's centre, from the indices
  const float x = G.o[0] + (float)ix * G.voxel, y = G.o[1] + (float)iy * G.voxel, z = G.o[2] + (float)iz * G.voxel;
  unsigned dw = 0u, dsd = 0u, diw = 0u, di = 0u;
  bool touched = false;
  for (int rec = 0; rec < n_records; ++rec) {
    const FrameRecord &R = records[rec];  // uniform over the block
    bool is_near = false, is_free = false;
    if (live && ix >= R.lo[0] && ix <= R.hi[0] && iy >= R.lo[1] && iy <= R.hi[1] && iz >= R.lo[2] && iz <= R.hi[2]) {
      float cx, cy, cz;
      rules::transform_rows(R.M, x, y, z, cx, cy, cz);
      {
        size_t at;
        if (rules::project_nearest(cx, cy, cz, G.near_z, R.fx, R.fy, R.ox, R.oy, R.w, R.h, at) == 0) {
          const float Zs = R.z[at], Is = R.i[at];
          if (finite_f(Zs) && finite_f(Is) && Zs <= G.far_z) {
            const float d = Zs - cz;
            if (!(d < -G.trunc)) {
              is_near = d <= G.trunc;
              is_free = !is_near;
              const float dc = fminf(d, G.trunc);
              const int q = (int)rintf((dc / G.trunc) * 2047.0f);
              int wgt = 1;
              if (G.weight == DVO_AMD_VOLUME_WEIGHT_SENSOR) {
                const float s = rules::depth_sigma(Zs);
                wgt = (int)fminf(fmaxf(rintf(256.0f * ((0.0012f * 0.0012f) / (s * s))), 1.0f), 256.0f);
              }
              const int g = (int)fminf(fmaxf(rintf(Is * 16.0f), 0.0f), 4080.0f);
              const int sw = R.sign * wgt;  // |sw| <= 256, |q| <= 2047, g <= 4080: the products fit an int
              dw += (unsigned)sw, dsd += (unsigned)(sw * q);
              if (is_near) diw += (unsigned)sw, di += (unsigned)(sw * g);
              touched = true;
            }
          }
        }
      }
    }
    if (R.slot >= 0) {  // (block-uniform: no barrier is skipped by part of a block)
      const unsigned cn = (unsigned)__popcll(__ballot(is_near)), cf = (unsigned)__popcll(__ballot(is_free));
      if (lane == 0) s_cnt[wave][0] = cn, s_cnt[wave][1] = cf;
      __syncthreads();
      if (threadIdx.x < 2) {
        unsigned sum = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
        if (sum) atomicAdd(counts + 2 * (size_t)R.slot + threadIdx.x, sum);
      }
      __syncthreads();  // s_cnt is written again for the next record
    }
  }
  if (touched) {  // (live: a lane that is not live touches nothing)
    const size_t L = ((size_t)iz * (size_t)G.ny + (size_t)iy) * (size_t)G.nx + (size_t)ix;
    uint2 a = pa[L], b = pb[L];
    a.x += dw, a.y += dsd, b.x += diw, b.y += di;
    pa[L] = a, pb[L] = b;
  }
}

// ---- raycast

struct RayParams {
  float P[12];  // rows 0..2 of camera -> world, row-major
  int width, height;
  float fx, fy, ox, oy, near_z;
  float step;
  int min_weight;
  int empty_all;  // the pyramid form: a pixel that is not hit and coloured is empty in both planes
  float fill;
};

struct Sample {
  bool inside;      // step 4's inequalities
  size_t base;      // L of corner (0,0,0)
  float fr[3];
  bool nearest[3];  // fr >= 0.5
};

__device__ __forceinline__ Sample sample_at(const Geom &G, const RayParams &V, float rx, float ry, float t) {
  Sample S;
  float p0, p1, p2;
  rules::transform_rows(V.P, rx * t, ry * t, t, p0, p1, p2);
  const float g0 = (p0 - G.o[0]) / G.voxel, g1 = (p1 - G.o[1]) / G.voxel, g2 = (p2 - G.o[2]) / G.voxel;
  S.inside = g0 >= 0.0f && g0 < (float)(G.nx - 1) && g1 >= 0.0f && g1 < (float)(G.ny - 1) && g2 >= 0.0f && g2 < (float)(G.nz - 1);
  S.base = 0;
  S.fr[0] = S.fr[1] = S.fr[2] = 0.0f;
  S.nearest[0] = S.nearest[1] = S.nearest[2] = false;
  if (S.inside) {
    const float f0 = floorf(g0), f1 = floorf(g1), f2 = floorf(g2);
    // 0 <= f_a <= n_a - 2: tested in float above, so every corner +1 is a voxel of the volume
    S.base = ((size_t)(int)f2 * (size_t)G.ny + (size_t)(int)f1) * (size_t)G.nx + (size_t)(int)f0;
    S.fr[0] = g0 - f0, S.fr[1] = g1 - f1, S.fr[2] = g2 - f2;
    S.nearest[0] = S.fr[0] >= 0.5f, S.nearest[1] = S.fr[1] >= 0.5f, S.nearest[2] = S.fr[2] >= 0.5f;
  }
  return S;
}

// the trilinear blend of the eight corners' ratios y/x of a plane; false unless every corner has x >= floor_x (as an int)
__device__ __forceinline__ bool blend(const uint2 *__restrict__ plane, const Geom &G, const Sample &S, int floor_x, float *out) {
  const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * (size_t)G.ny;
  const uint2 t000 = plane[S.base], t100 = plane[S.base + 1];
  const uint2 t010 = plane[S.base + sy], t110 = plane[S.base + sy + 1];
  const uint2 t001 = plane[S.base + sz], t101 = plane[S.base + sz + 1];
  const uint2 t011 = plane[S.base + sz + sy], t111 = plane[S.base + sz + sy + 1];
  const bool ok = (int)t000.x >= floor_x && (int)t100.x >= floor_x && (int)t010.x >= floor_x && (int)t110.x >= floor_x &&
                  (int)t001.x >= floor_x && (int)t101.x >= floor_x && (int)t011.x >= floor_x && (int)t111.x >= floor_x;
  if (!ok) return false;
  auto ratio = [](const uint2 t) { return (float)(int)t.y / (float)(int)t.x; };
  const float F000 = ratio(t000), F100 = ratio(t100), F010 = ratio(t010), F110 = ratio(t110);
  const float F001 = ratio(t001), F101 = ratio(t101), F011 = ratio(t011), F111 = ratio(t111);
  const float c00 = F000 + S.fr[0] * (F100 - F000), c10 = F010 + S.fr[0] * (F110 - F010);
  const float c01 = F001 + S.fr[0] * (F101 - F001), c11 = F011 + S.fr[0] * (F111 - F011);
  const float c0 = c00 + S.fr[1] * (c10 - c00), c1 = c01 + S.fr[1] * (c11 - c01);
  *out = c0 + S.fr[2] * (c1 - c0);
  return true;
}

__global__ void __launch_bounds__(kBlock) k_volume_raycast(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, RayParams V,
                                                           float *__restrict__ depth, float *__restrict__ inten, int *__restrict__ weight,
                                                           unsigned *__restrict__ stats) {
  __shared__ unsigned s_cnt[kWaves][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (V.width + 7) >> 3, tiles_y = (V.height + 7) >> 3;
  const int tile = blockIdx.x * kWaves + wave;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int u = txi * 8 + (lane & 7), v = tyi * 8 + (lane >> 3);
  const bool live = tyi < tiles_y && u < V.width && v < V.height;
  const float nan = __uint_as_float(kNaN);
  int cls = 0;  // 0: no pixel; 1 hit, 2 backface, 3 missed
  bool coloured = false;
  float d_out = nan, i_out = nan;
  int w_out = 0;
  if (live) {
    const float rx = ((float)u - V.ox) / V.fx, ry = ((float)v - V.oy) / V.fy;
    bool have_prev = false;
    float f_prev = 0.0f, t_prev = 0.0f;
    cls = 3;
    for (int k = 0; k <= DVO_AMD_VOLUME_MAX_STEPS + 1; ++k) {  // (the bound is never the one that ends a ray: the entry checks the step)
      const float t = V.near_z + (float)k * V.step;
      if (!(t <= G.far_z)) break;
      const Sample S = sample_at(G, V, rx, ry, t);
      float f = 0.0f;
      const bool known = S.inside && blend(pa, G, S, V.min_weight, &f);
      if (known && have_prev) {
        if (f_prev > 0.0f && f <= 0.0f) {
          cls = 1;
          d_out = t_prev + V.step * (f_prev / (f_prev - f));
          break;
        }
        if (f_prev < 0.0f && f > 0.0f) {
          cls = 2;
          break;
        }
      }
      have_prev = known, f_prev = f, t_prev = t;
    }
    if (cls == 1) {
      const Sample S = sample_at(G, V, rx, ry, d_out);
      if (S.inside) {
        float gval = 0.0f;
        if (blend(pb, G, S, 1, &gval)) coloured = true, i_out = gval * 0.0625f;
        const size_t at = S.base + (S.nearest[0] ? 1 : 0) + (S.nearest[1] ? (size_t)G.nx : 0) + (S.nearest[2] ? (size_t)G.nx * (size_t)G.ny : 0);
        w_out = (int)pa[at].x;
      }
    }
    if (V.empty_all) {
      if (!(cls == 1 && coloured)) d_out = nan, i_out = V.fill;
    }
    const size_t p = (size_t)v * (size_t)V.width + (size_t)u;
    if (depth) depth[p] = d_out;
    if (inten) inten[p] = i_out;
    if (weight) weight[p] = w_out;
  }
  unsigned cnt[4];
#pragma unroll
  for (int c = 0; c < 3; ++c) cnt[c] = (unsigned)__popcll(__ballot(cls == c + 1));
  cnt[3] = (unsigned)__popcll(__ballot(cls == 1 && !coloured));
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s_cnt[wave][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned sum = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][threadIdx.x];
    if (sum) atomicAdd(stats + threadIdx.x, sum);
  }
}

// ---- the surface

// the crossings of voxel L = (ix,iy,iz) along the three axes: bit a of the result; `emit` receives (a, point, coloured)
template <typename Emit>
__device__ __forceinline__ int crossings(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, const Geom &G, int min_weight, size_t L,
                                         int ix, int iy, int iz, Emit emit) {
  const uint2 ta = pa[L];
  if ((int)ta.x < min_weight) return 0;
  const float Fa = (float)(int)ta.y / (float)(int)ta.x;
  const size_t stride[3] = {1, (size_t)G.nx, (size_t)G.nx * (size_t)G.ny};
  const bool has[3] = {ix + 1 < G.nx, iy + 1 < G.ny, iz + 1 < G.nz};
  int found = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!has[a]) continue;
    const size_t Lb = L + stride[a];
    const uint2 tb = pa[Lb];
    if ((int)tb.x < min_weight) continue;
    const float Fb = (float)(int)tb.y / (float)(int)tb.x;
    if (!((Fa > 0.0f && Fb <= 0.0f) || (Fa <= 0.0f && Fb > 0.0f))) continue;
    found |= 1 << a;
    emit(a, Fa, Fb, Lb);
  }
  return found;
}

__device__ __forceinline__ void voxel_of(const Geom &G, size_t L, int &ix, int &iy, int &iz) {
  const size_t row = L / (size_t)G.nx;
  ix = (int)(L - row * (size_t)G.nx);
  iz = (int)(row / (size_t)G.ny);
  iy = (int)(row - (size_t)iz * (size_t)G.ny);
}

__global__ void __launch_bounds__(kBlock) k_volume_count(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, int min_weight,
                                                         size_t n_vox, unsigned long long *__restrict__ tile_sums) {
  const size_t first = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kVoxelsPerLane;
  unsigned mine = 0u;
  for (int j = 0; j < kVoxelsPerLane; ++j) {
    const size_t L = first + j;
    if (L >= n_vox) break;
    int ix, iy, iz;
    voxel_of(G, L, ix, iy, iz);
    mine += (unsigned)__popc(crossings(pa, pb, G, min_weight, L, ix, iy, iz, [](int, float, float, size_t) {}));
  }
  unsigned total = 0u;
  (void)rules::block_exclusive_scan<kWaves>(mine, &total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one block: the exclusive scan of the tile totals in place; *grand = the sum of all
__device__ __forceinline__ void scan_tile_sums(unsigned long long *__restrict__ tile_sums, unsigned n_tiles,
                                               unsigned long long *__restrict__ grand) {
  unsigned long long carry = 0ull;
  for (unsigned base = 0; base < n_tiles; base += kBlock) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < n_tiles ? (unsigned)tile_sums[i] : 0u;  // (a tile holds at most 3 * kTile crossings)
    unsigned total = 0u;
    const unsigned ex = rules::block_exclusive_scan<kWaves>(v, &total);  // (a chunk's sum is at most 256 * 3 * kTile < 2^32)
    if (i < n_tiles) tile_sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *grand = carry;
}

__global__ void __launch_bounds__(kBlock) k_volume_scan(unsigned long long *__restrict__ tile_sums, unsigned n_tiles,
                                                        unsigned long long *__restrict__ grand) {
  scan_tile_sums(tile_sums, n_tiles, grand);
}

__global__ void __launch_bounds__(kBlock) k_volume_write(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, int min_weight,
                                                         size_t n_vox, const unsigned long long *__restrict__ tile_offsets,
                                                         dvo_amd_point *__restrict__ out, unsigned long long capacity,
                                                         unsigned *__restrict__ uncoloured) {
  __shared__ unsigned s_unc[kWaves];
  const size_t first = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kVoxelsPerLane;
  unsigned mine = 0u;
  for (int j = 0; j < kVoxelsPerLane; ++j) {
    const size_t L = first + j;
    if (L >= n_vox) break;
    int ix, iy, iz;
    voxel_of(G, L, ix, iy, iz);
    mine += (unsigned)__popc(crossings(pa, pb, G, min_weight, L, ix, iy, iz, [](int, float, float, size_t) {}));
  }
  unsigned total = 0u;
  unsigned long long at = tile_offsets[blockIdx.x] + rules::block_exclusive_scan<kWaves>(mine, &total);
  unsigned unc = 0u;
  for (int j = 0; j < kVoxelsPerLane; ++j) {
    const size_t L = first + j;
    if (L >= n_vox) break;
    int ix, iy, iz;
    voxel_of(G, L, ix, iy, iz);
    const float c[3] = {G.o[0] + (float)ix * G.voxel, G.o[1] + (float)iy * G.voxel, G.o[2] + (float)iz * G.voxel};
    const int idx[3] = {ix, iy, iz};
    const uint2 ga = pb[L];
    (void)crossings(pa, pb, G, min_weight, L, ix, iy, iz, [&](int a, float Fa, float Fb, size_t Lb) {
      const float s = Fa / (Fa - Fb);
      dvo_amd_point p;
      p.x = c[0], p.y = c[1], p.z = c[2];
      const float along = G.o[a] + ((float)idx[a] + s) * G.voxel;
      if (a == 0) p.x = along;
      if (a == 1) p.y = along;
      if (a == 2) p.z = along;
      const uint2 gb = pb[Lb];
      p.rgb = 0u;
      if ((int)ga.x > 0 && (int)gb.x > 0) {
        const float Ga = (float)(int)ga.y / (float)(int)ga.x, Gb = (float)(int)gb.y / (float)(int)gb.x;
        const unsigned grey = (unsigned)(int)fminf(fmaxf(rintf((Ga + s * (Gb - Ga)) * 0.0625f), 0.0f), 255.0f);
        p.rgb = (grey << 16) | (grey << 8) | grey;
      } else {
        ++unc;
      }
      if (at < capacity) out[at] = p;  // (the host launches this kernel only with room for every point)
      ++at;
    });
  }
  // the uncoloured points: per wave, per block, one atomic
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) unc += __shfl_down(unc, o, 64);
  if (lane == 0) s_unc[wave] = unc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_unc[w];
    if (sum) atomicAdd(uncoloured, sum);
  }
}

// the public records of count voxels of an index box, from position `first` of the box's own order (x fastest)
__global__ void __launch_bounds__(kBlock) k_volume_gather(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, int3 lo, int3 ext,
                                                          unsigned long long first, unsigned count, uint4 *__restrict__ out) {
  const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (i >= count) return;
  const unsigned long long idx = first + i;
  const unsigned long long row = idx / (unsigned)ext.x;
  const int ix = lo.x + (int)(idx - row * (unsigned)ext.x);
  const unsigned long long slab = row / (unsigned)ext.y;
  const int iy = lo.y + (int)(row - slab * (unsigned)ext.y), iz = lo.z + (int)slab;
  const size_t L = ((size_t)iz * (size_t)G.ny + (size_t)iy) * (size_t)G.nx + (size_t)ix;  // (inside the volume: the host checks the box)
  const uint2 a = pa[L], b = pb[L];
  out[i] = make_uint4(a.x, a.y, b.x, b.y);
}

// ... and the way back: the packed records of the same stretch of a box into the two planes
__global__ void __launch_bounds__(kBlock) k_volume_scatter(uint2 *__restrict__ pa, uint2 *__restrict__ pb, Geom G, int3 lo, int3 ext,
                                                           unsigned long long first, unsigned count, const uint4 *__restrict__ in) {
  const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (i >= count) return;
  const unsigned long long idx = first + i;
  const unsigned long long row = idx / (unsigned)ext.x;
  const int ix = lo.x + (int)(idx - row * (unsigned)ext.x);
  const unsigned long long slab = row / (unsigned)ext.y;
  const int iy = lo.y + (int)(row - slab * (unsigned)ext.y), iz = lo.z + (int)slab;
  const size_t L = ((size_t)iz * (size_t)G.ny + (size_t)iy) * (size_t)G.nx + (size_t)ix;  // (inside the volume: the host checks the box)
  const uint4 r = in[i];
  pa[L] = make_uint2(r.x, r.y), pb[L] = make_uint2(r.z, r.w);
}

// ---- the mesh (include/dvo_amd.h, "The mesh"): naive surface nets, one vertex per active cell, one quad per crossing edge
//
// Cells are indexed Lc = (cz*(ny-1) + cy)*(nx-1) + cx.  What a cell's rank among the active ones is, is never stored per cell:
//   k_mesh_cells     a lane walks kCellsPerLane consecutive cells and keeps the four taps of the face it shares with the next one
//                    (they are consecutive along x until a row ends: 4 loads per cell instead of 8); eight lanes' bytes make one
//                    64-bit activity word, the block scans its 32 words and leaves word, offset of the word inside the tile, tile total
//   k_mesh_edges     the faces per tile of voxels: crossings() whose four cells exist and are active (a cell around a crossing
//                    edge is active iff it is known); the open ones are counted, one integer atomic per block
//   k_mesh_scan      one block: both lists of tile totals
//   k_mesh_vertices  a lane takes its byte of the activity word and computes the vertices of its active cells at their rank
//   k_mesh_faces     every tile of voxels recounts, scans inside the block and writes two triangles per face from the four ranks
// rank(Lc) = tile_offset[Lc / kCellTile] + word_offset[Lc / 64] + popcll(word[Lc / 64] & below(Lc % 64)).
constexpr int kCellsPerLane = 8;
constexpr int kCellTile = kBlock * kCellsPerLane;
constexpr int kWordsPerTile = kCellTile / 64;
static_assert(kCellsPerLane == 8 && kWordsPerTile * 64 == kCellTile, "eight lanes' bytes make one 64-bit word");

struct Cells {
  int nx, ny, nz;  // cells along each axis: the volume's dimensions minus one
  size_t n;
  const unsigned long long *word;     // [tiles * kWordsPerTile] activity bits
  const unsigned *word_offset;        // the active cells of the tile before the word
  const unsigned long long *tile_offset;
};

__device__ __forceinline__ bool cell_active(const Cells &C, int cx, int cy, int cz) {
  const size_t Lc = ((size_t)cz * (size_t)C.ny + (size_t)cy) * (size_t)C.nx + (size_t)cx;
  return (C.word[Lc >> 6] >> (Lc & 63)) & 1ull;
}

__device__ __forceinline__ int cell_rank(const Cells &C, size_t Lc) {
  const size_t w = Lc >> 6;
  const unsigned long long below = C.word[w] & ((1ull << (Lc & 63)) - 1ull);
  return (int)(C.tile_offset[Lc / kCellTile] + C.word_offset[w] + (unsigned)__popcll(below));  // (< 2^30 cells)
}

// the four cells q0..q3 around the crossing edge of voxel (ix,iy,iz) along a, counter-clockwise seen from +a; false: one of them
// does not exist or is not active
__device__ __forceinline__ bool quad_cells(const Cells &C, int a, int ix, int iy, int iz, size_t q[4]) {
  // (b,c) = (y,z), (z,x), (x,y) for a = x, y, z; selects, not indexed arrays: a is not a constant everywhere this is inlined
  const int ib = a == 0 ? iy : a == 1 ? iz : ix, ic = a == 0 ? iz : a == 1 ? ix : iy;
  const int nb = a == 0 ? C.ny : a == 1 ? C.nz : C.nx, nc = a == 0 ? C.nz : a == 1 ? C.nx : C.ny;
  if (ib < 1 || ib > nb - 1 || ic < 1 || ic > nc - 1) return false;  // (cells i-1 and i: 1 <= i <= cells - 1)
  bool all = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cb = ib - (k == 0 || k == 3 ? 1 : 0), cc = ic - (k < 2 ? 1 : 0);
    const int cx = a == 0 ? ix : a == 1 ? cc : cb, cy = a == 0 ? cb : a == 1 ? iy : cc, cz = a == 0 ? cc : a == 1 ? cb : iz;
    q[k] = ((size_t)cz * (size_t)C.ny + (size_t)cy) * (size_t)C.nx + (size_t)cx;
    all = all && cell_active(C, cx, cy, cz);
  }
  return all;
}

__global__ void __launch_bounds__(kBlock) k_mesh_cells(const uint2 *__restrict__ pa, Geom G, int min_weight, size_t n_cells,
                                                       unsigned long long *__restrict__ word, unsigned *__restrict__ word_offset,
                                                       unsigned long long *__restrict__ tile_sums) {
  const int ncx = G.nx - 1, ncy = G.ny - 1;
  const size_t first = (size_t)blockIdx.x * kCellTile + (size_t)threadIdx.x * kCellsPerLane;
  const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * (size_t)G.ny;
  // the four taps of a cell's face at x: bit dy + 2*dz of `known` and of `inside`
  auto face = [&](size_t L, unsigned &known, unsigned &inside) {
    known = inside = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint2 t = pa[L + (k & 1 ? sy : 0) + (k & 2 ? sz : 0)];
      const bool ok = (int)t.x >= min_weight;
      known |= (ok ? 1u : 0u) << k;
      inside |= (ok && (float)(int)t.y / (float)(int)t.x <= 0.0f ? 1u : 0u) << k;
    }
  };
  unsigned byte = 0u, k_lo = 0u, i_lo = 0u;
  bool have = false;
  int cx = 0, cy = 0, cz = 0;
  for (int j = 0; j < kCellsPerLane; ++j) {
    const size_t Lc = first + j;
    if (Lc >= n_cells) break;
    if (j == 0) {
      const size_t row = Lc / (size_t)ncx;
      cx = (int)(Lc - row * (size_t)ncx);
      cz = (int)(row / (size_t)ncy);
      cy = (int)(row - (size_t)cz * (size_t)ncy);
    } else if (++cx == ncx) {  // the row ends: the next cell shares no face with this one
      cx = 0, have = false;
      if (++cy == ncy) cy = 0, ++cz;
    }
    const size_t L = ((size_t)cz * (size_t)G.ny + (size_t)cy) * (size_t)G.nx + (size_t)cx;  // corner 0; cx + 1 <= nx - 1 and alike
    if (!have) face(L, k_lo, i_lo);
    unsigned k_hi, i_hi;
    face(L + 1, k_hi, i_hi);
    const unsigned in = i_lo | (i_hi << 4);
    const bool active = k_lo == 15u && k_hi == 15u && in != 0u && in != 255u;
    byte |= (active ? 1u : 0u) << j;
    k_lo = k_hi, i_lo = i_hi, have = true;
  }
  // eight lanes' bytes are one word
  unsigned long long m = (unsigned long long)byte << (8 * (threadIdx.x & 7));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m |= __shfl_xor(m, o, 64);
  const bool writer = (threadIdx.x & 7) == 0;
  unsigned total = 0u;
  const unsigned ex = rules::block_exclusive_scan<kWaves>(writer ? (unsigned)__popcll(m) : 0u, &total);
  if (writer) {
    const size_t w = (size_t)blockIdx.x * kWordsPerTile + (threadIdx.x >> 3);
    word[w] = m, word_offset[w] = ex;
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// the faces of a lane's voxels; *open: the crossings that yield none
__device__ __forceinline__ unsigned lane_faces(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, const Geom &G, const Cells &C,
                                               int min_weight, size_t first, size_t n_vox, unsigned *open) {
  unsigned faces = 0u, none = 0u;
  for (int j = 0; j < kVoxelsPerLane; ++j) {
    const size_t L = first + j;
    if (L >= n_vox) break;
    int ix, iy, iz;
    voxel_of(G, L, ix, iy, iz);
    const int found = crossings(pa, pb, G, min_weight, L, ix, iy, iz, [](int, float, float, size_t) {});
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((found >> a) & 1)) continue;
      size_t q[4];
      if (quad_cells(C, a, ix, iy, iz, q))
        ++faces;
      else
        ++none;
    }
  }
  *open = none;
  return faces;
}

__global__ void __launch_bounds__(kBlock) k_mesh_edges(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, Cells C,
                                                       int min_weight, size_t n_vox, unsigned long long *__restrict__ tile_sums,
                                                       unsigned *__restrict__ open_edges) {
  const size_t first = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kVoxelsPerLane;
  unsigned open = 0u;
  const unsigned faces = lane_faces(pa, pb, G, C, min_weight, first, n_vox, &open);
  unsigned total = 0u, total_open = 0u;
  (void)rules::block_exclusive_scan<kWaves>(faces, &total);
  (void)rules::block_exclusive_scan<kWaves>(open, &total_open);
  if (threadIdx.x == 0) {
    tile_sums[blockIdx.x] = total;
    if (total_open) atomicAdd(open_edges, total_open);
  }
}

// one block: grand[0] = the vertices, grand[1] = the faces (quads)
__global__ void __launch_bounds__(kBlock) k_mesh_scan(unsigned long long *__restrict__ cell_sums, unsigned n_cell_tiles,
                                                      unsigned long long *__restrict__ face_sums, unsigned n_voxel_tiles,
                                                      unsigned long long *__restrict__ grand) {
  scan_tile_sums(cell_sums, n_cell_tiles, grand);
  scan_tile_sums(face_sums, n_voxel_tiles, grand + 1);
}

// counts[0]: uncoloured, counts[1]: flat
__global__ void __launch_bounds__(kBlock) k_mesh_vertices(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, Cells C,
                                                          dvo_amd_point *__restrict__ out, float *__restrict__ normals,
                                                          unsigned long long capacity, unsigned *__restrict__ counts) {
  __shared__ unsigned s_cnt[kWaves][2];
  const size_t w = (size_t)blockIdx.x * kWordsPerTile + (threadIdx.x >> 3);
  const unsigned long long m = C.word[w];
  const int shift = 8 * (threadIdx.x & 7);
  unsigned byte = (unsigned)(m >> shift) & 255u;
  unsigned long long at = C.tile_offset[blockIdx.x] + C.word_offset[w] + (unsigned)__popcll(m & ((1ull << shift) - 1ull));
  const size_t first = (size_t)blockIdx.x * kCellTile + (size_t)threadIdx.x * kCellsPerLane;
  const size_t stride[3] = {1, (size_t)G.nx, (size_t)G.nx * (size_t)G.ny};
  unsigned unc = 0u, flat = 0u;
  while (byte) {
    const int j = __ffs(byte) - 1;
    byte &= byte - 1u;
    const size_t Lc = first + j;  // (< cells: a bit beyond them is never set)
    const size_t row = Lc / (size_t)C.nx;
    int cc[3];
    cc[0] = (int)(Lc - row * (size_t)C.nx);
    cc[2] = (int)(row / (size_t)C.ny);
    cc[1] = (int)(row - (size_t)cc[2] * (size_t)C.ny);
    const size_t L = ((size_t)cc[2] * (size_t)G.ny + (size_t)cc[1]) * (size_t)G.nx + (size_t)cc[0];
    float Fk[8], Gk[8];
    bool col[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const size_t Lk = L + (k & 1 ? stride[0] : 0) + (k & 2 ? stride[1] : 0) + (k & 4 ? stride[2] : 0);
      const uint2 ta = pa[Lk], tb = pb[Lk];
      Fk[k] = (float)(int)ta.y / (float)(int)ta.x;  // (an active cell: every corner has w_sum >= min_weight >= 1)
      col[k] = (int)tb.x > 0;
      Gk[k] = (float)(int)tb.y / (float)(int)tb.x;  // (used where col[k])
    }
    float S[3] = {0.0f, 0.0f, 0.0f}, grad[3] = {0.0f, 0.0f, 0.0f}, grey_sum = 0.0f;
    int n_cross = 0, n_grey = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int db = e & 1, dc = e >> 1;
        const int lo = (db << b) | (dc << c), hi = lo | (1 << a);
        const float Fa = Fk[lo], Fb = Fk[hi];
        grad[a] = grad[a] + (Fb - Fa);
        if (!((Fa > 0.0f && Fb <= 0.0f) || (Fa <= 0.0f && Fb > 0.0f))) continue;
        const float s = Fa / (Fa - Fb);
        float pt[3];
        pt[a] = s, pt[b] = (float)db, pt[c] = (float)dc;
        S[0] = S[0] + pt[0], S[1] = S[1] + pt[1], S[2] = S[2] + pt[2];
        ++n_cross;
        if (col[lo] && col[hi]) {
          grey_sum = grey_sum + (Gk[lo] + s * (Gk[hi] - Gk[lo]));
          ++n_grey;
        }
      }
    }
    dvo_amd_point p;
    const float mf = (float)n_cross;
    p.x = G.o[0] + ((float)cc[0] + S[0] / mf) * G.voxel;
    p.y = G.o[1] + ((float)cc[1] + S[1] / mf) * G.voxel;
    p.z = G.o[2] + ((float)cc[2] + S[2] / mf) * G.voxel;
    p.rgb = 0u;
    if (n_grey > 0) {
      const unsigned grey = (unsigned)(int)fminf(fmaxf(rintf((grey_sum / (float)n_grey) * 0.0625f), 0.0f), 255.0f);
      p.rgb = (grey << 16) | (grey << 8) | grey;
    } else {
      ++unc;
    }
    const float len = sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (len == 0.0f)
      ++flat;
    else
      nrm[0] = grad[0] / len, nrm[1] = grad[1] / len, nrm[2] = grad[2] / len;
    if (at < capacity) {  // (the host launches this kernel only with room for every vertex)
      out[at] = p;
      if (normals) normals[3 * at] = nrm[0], normals[3 * at + 1] = nrm[1], normals[3 * at + 2] = nrm[2];
    }
    ++at;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) unc += __shfl_down(unc, o, 64), flat += __shfl_down(flat, o, 64);
  if (lane == 0) s_cnt[wave][0] = unc, s_cnt[wave][1] = flat;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned sum = 0u;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) sum += s_cnt[v][threadIdx.x];
    if (sum) atomicAdd(counts + threadIdx.x, sum);
  }
}

__global__ void __launch_bounds__(kBlock) k_mesh_faces(const uint2 *__restrict__ pa, const uint2 *__restrict__ pb, Geom G, Cells C,
                                                       int min_weight, size_t n_vox, const unsigned long long *__restrict__ tile_offsets,
                                                       int *__restrict__ out, unsigned long long capacity) {
  const size_t first = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kVoxelsPerLane;
  unsigned open = 0u, total = 0u;
  const unsigned mine = lane_faces(pa, pb, G, C, min_weight, first, n_vox, &open);
  unsigned long long at = tile_offsets[blockIdx.x] + rules::block_exclusive_scan<kWaves>(mine, &total);  // in faces
  if (!mine) return;  // (behind the block's last barrier)
  for (int j = 0; j < kVoxelsPerLane; ++j) {
    const size_t L = first + j;
    if (L >= n_vox) break;
    int ix, iy, iz;
    voxel_of(G, L, ix, iy, iz);
    int faces_up = 0;  // bit a: Fb > 0, the surface faces +a
    const int found = crossings(pa, pb, G, min_weight, L, ix, iy, iz, [&](int a, float, float Fb, size_t) { faces_up |= (Fb > 0.0f ? 1 : 0) << a; });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      size_t q[4];
      if (!((found >> a) & 1) || !quad_cells(C, a, ix, iy, iz, q)) continue;
      const int v0 = cell_rank(C, q[0]), v1 = cell_rank(C, q[1]), v2 = cell_rank(C, q[2]), v3 = cell_rank(C, q[3]);
      const bool up = (faces_up >> a) & 1;
      if (2ull * at + 2ull <= capacity) {  // (the host launches this kernel only with room for every triangle)
        int *t = out + 6ull * at;
        t[0] = v0, t[1] = up ? v1 : v2, t[2] = up ? v2 : v1;
        t[3] = v0, t[4] = up ? v2 : v3, t[5] = up ? v3 : v2;
      }
      ++at;
    }
  }
}

}  // namespace volume
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::volume;

struct dvo_amd_volume {
  int device = 0;
  dvo_amd_volume_options opt{};
  Geom geom{};
  size_t n_vox = 0;
  uint2 *a = nullptr, *b = nullptr;  // device, [n_vox] each
  struct Keyframe {
    dvo_amd_pyramid *pyramid;  // retained
    int level;
    float M[12];               // the float inverse pose it is integrated at
    long long updated;         // its `updated` count there
  };
  std::map<int, Keyframe> keyframes;
};

namespace {

// dvo_amd_debug_volume_timing: what the last call on the device launched and waited for, and (when asked for) two events around
// its launches on the prep stream
DeviceTiming g_timing[kMaxDevices];

// one frame of an integration call on the host
struct Item {
  const dvo_amd_pyramid *pyramid;
  int level;
  float M[12];
  int sign;
  int slot;  // index into the call's counts, -1: not counted
};

// ONE launch and ONE synchronisation for all items; near_free: 2 words per slot (may be empty when no item has a slot)
int run_integration(dvo_amd_volume *vol, const std::vector<Item> &items, int n_slots, std::vector<unsigned> &near_free) {
  near_free.assign((size_t)2 * (size_t)std::max(n_slots, 0), 0u);
  if (items.empty()) {  // nothing moves: nothing is launched
    g_timing[vol->device].count(0, 0);
    return DVO_AMD_OK;
  }
  const int device = vol->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  int rc = device_prep_stream(device, &st);
  if (rc) return rc;
  const dvo_amd_volume_options &o = vol->opt;
  const int dims[3] = {o.nx, o.ny, o.nz};
  const double origin[3] = {(double)o.origin[0], (double)o.origin[1], (double)o.origin[2]};
  const double z_max = (double)(o.far_z + o.trunc);
  std::vector<FrameRecord> table(items.size());
  volume_box::Box uni = volume_box::none();
  for (size_t k = 0; k < items.size(); ++k) {
    const Item &it = items[k];
    const LevelData &L = it.pyramid->lv[it.level];
    FrameRecord &R = table[k];
    R.z = L.z_plane, R.i = L.i_plane, R.w = L.w, R.h = L.h;
    R.fx = L.fx, R.fy = L.fy, R.ox = L.ox, R.oy = L.oy;
    double Md[12];
    for (int i = 0; i < 12; ++i) R.M[i] = it.M[i], Md[i] = (double)it.M[i];
    const volume_box::Box box = volume_box::frustum_box(Md, (double)L.fx, (double)L.fy, (double)L.ox, (double)L.oy, L.w, L.h,
                                                        (double)o.near_z, z_max, origin, (double)o.voxel, dims);
    for (int a = 0; a < 3; ++a) R.lo[a] = box.lo[a], R.hi[a] = box.hi[a];
    R.sign = it.sign, R.slot = it.slot;
    uni = volume_box::unite(uni, box);
  }
  const bool nothing = volume_box::is_empty(uni);
  const int3 lo = make_int3(nothing ? 0 : uni.lo[0], nothing ? 0 : uni.lo[1], nothing ? 0 : uni.lo[2]);
  const int3 ext = make_int3(nothing ? 1 : uni.hi[0] - uni.lo[0] + 1, nothing ? 1 : uni.hi[1] - uni.lo[1] + 1, nothing ? 1 : uni.hi[2] - uni.lo[2] + 1);
  const unsigned total = nothing ? 0u : (unsigned)((size_t)ext.x * (size_t)ext.y * (size_t)ext.z);  // (<= 2^30)

  const size_t table_bytes = align_up(sizeof(FrameRecord) * table.size(), 256);
  const size_t count_bytes = align_up(sizeof(unsigned) * std::max<size_t>(near_free.size(), 1), 256);
  Scratch S;
  rc = S.take(device, table_bytes + count_bytes, true);
  if (rc) return rc;
  char *base = (char *)S.mem;
  unsigned *d_counts = (unsigned *)(base + table_bytes);
  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemcpyAsync(base, table.data(), sizeof(FrameRecord) * table.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  int launches = 0;
  if (e == hipSuccess && total > 0u) {
    const unsigned blocks = (total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_volume_integrate, dim3(blocks), dim3(kBlock), 0, st, vol->a, vol->b, vol->geom, (const FrameRecord *)base,
                       (int)table.size(), lo, ext, total, d_counts);
    e = hipGetLastError();
    launches = 1;
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && !near_free.empty())
    e = hipMemcpyAsync(near_free.data(), d_counts, sizeof(unsigned) * near_free.size(), hipMemcpyDeviceToHost, st);
  // the call's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume integration", e);
  bracket.read(launches, 1);
  return DVO_AMD_OK;
}

int check_frames(const char *entry, int n, const dvo_amd_pyramid *const *pyramids, int level, const double *poses) {
  if (level < 0) return invalid(entry, "a negative level");
  for (int k = 0; k < n; ++k) {
    const std::string item = "frame " + std::to_string(k);
    if (!pyramids[k]) return invalid(entry, item + ": a NULL pyramid");
    if (level >= pyramids[k]->n_levels)
      return invalid(entry, item + ": level " + std::to_string(level) + " is beyond a pyramid of " + std::to_string(pyramids[k]->n_levels) + " levels");
    if (poses && !finite_all(poses + 16 * (size_t)k, 16)) return invalid(entry, item + ": the pose has a non-finite entry");
  }
  return DVO_AMD_OK;
}

int check_ids(const char *entry, const dvo_amd_volume *vol, int n, const int *ids, bool present) {
  for (int k = 0; k < n; ++k) {
    for (int j = 0; j < k; ++j)
      if (ids[j] == ids[k]) return invalid(entry, "id " + std::to_string(ids[k]) + " appears twice in the call");
    const bool have = vol->keyframes.count(ids[k]) != 0;
    if (have && !present) return invalid(entry, "id " + std::to_string(ids[k]) + " is already in the volume");
    if (!have && present) return invalid(entry, "id " + std::to_string(ids[k]) + " is not in the volume");
  }
  return DVO_AMD_OK;
}

void to_counts(const std::vector<unsigned> &near_free, int slot, dvo_amd_volume_counts *c) {
  c->near = (long long)near_free[2 * (size_t)slot], c->free = (long long)near_free[2 * (size_t)slot + 1];
  c->updated = c->near + c->free;
}

int check_raycast(const char *entry, const dvo_amd_volume *vol, const double *pose, const dvo_amd_view *v, const dvo_amd_volume_raycast_options *opt,
                  float *step_out) {
  if (!opt || !v) return invalid(entry, "a NULL pointer");
  if (!(opt->step_fraction > 0.0f && opt->step_fraction <= 1.0f)) return invalid(entry, "step_fraction must be in (0, 1]");
  if (opt->min_weight < 1) return invalid(entry, "min_weight must be >= 1");
  if (!std::isfinite(opt->fill_intensity)) return invalid(entry, "fill_intensity must be finite");
  if (v->width < 1 || v->height < 1 || (long long)v->width * v->height > (1ll << 26))
    return invalid(entry, "the view's width and height must be >= 1 and width*height <= 2^26");
  if (!(std::isfinite(v->fx) && v->fx > 0.0f && std::isfinite(v->fy) && v->fy > 0.0f))
    return invalid(entry, "the view's fx and fy must be finite and positive");
  if (!std::isfinite(v->ox) || !std::isfinite(v->oy)) return invalid(entry, "the view's ox and oy must be finite");
  if (!std::isfinite(v->near_z) || !(v->near_z > 0.0f)) return invalid(entry, "the view's near_z must be finite and positive");
  if (pose && !finite_all(pose, 16)) return invalid(entry, "the pose has a non-finite entry");
  if (!vol) return invalid(entry, "a NULL volume");
  const float step = opt->step_fraction * vol->opt.trunc;
  if (!(step > 0.0f) || !((vol->opt.far_z - v->near_z) / step <= (float)DVO_AMD_VOLUME_MAX_STEPS))
    return invalid(entry, "(far_z - near_z) / (step_fraction * trunc) must not exceed " + std::to_string(DVO_AMD_VOLUME_MAX_STEPS));
  *step_out = step;
  return DVO_AMD_OK;
}

// levels < 0: the plane form (host planes, any may be null); else the pyramid form
int raycast(const char *entry, dvo_amd_volume *vol, const double *pose, const dvo_amd_view *view, const dvo_amd_volume_raycast_options *opt,
            int levels, double timestamp, float *depth, float *intensity, int *weight, dvo_amd_pyramid **out,
            dvo_amd_volume_raycast_stats *stats) {
  const bool as_pyramid = levels >= 0;
  float step = 0.0f;
  int rc = check_raycast(entry, vol, pose, view, opt, &step);
  if (rc) return rc;
  if (as_pyramid) {
    rc = check_levels(entry, view->width, view->height, levels, " of the levels asked of the view");
    if (rc) return rc;
  }
  rc = have_device();
  if (rc) return rc;
  const int device = vol->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  RayParams V;
  if (pose) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) V.P[r * 4 + c] = (float)pose[c * 4 + r];  // column-major in, rows 0..2 out
  } else {
    for (int i = 0; i < 12; ++i) V.P[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  }
  V.width = view->width, V.height = view->height;
  V.fx = view->fx, V.fy = view->fy, V.ox = view->ox, V.oy = view->oy, V.near_z = view->near_z;
  V.step = step, V.min_weight = opt->min_weight, V.empty_all = as_pyramid ? 1 : 0, V.fill = opt->fill_intensity;

  const size_t n_px = (size_t)view->width * (size_t)view->height;
  const size_t plane = align_up(sizeof(float) * n_px, 256);
  const bool want_z = as_pyramid || depth, want_i = as_pyramid || intensity, want_w = !as_pyramid && weight;
  Scratch S;
  // the stats, then the planes anybody wants
  size_t need = 256;
  const size_t z_at = need;
  if (want_z) need += plane;
  const size_t i_at = need;
  if (want_i) need += plane;
  const size_t w_at = need;
  if (want_w) need += plane;
  rc = S.take(device, need, true);
  if (rc) return rc;
  char *base = (char *)S.mem;
  unsigned *d_stats = (unsigned *)base;
  float *d_z = want_z ? (float *)(base + z_at) : nullptr;
  float *d_i = want_i ? (float *)(base + i_at) : nullptr;
  int *d_w = want_w ? (int *)(base + w_at) : nullptr;
  unsigned h_stats[4] = {0u, 0u, 0u, 0u};
  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemsetAsync(d_stats, 0, 256, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    const unsigned tiles = (unsigned)(((view->width + 7) / 8) * (size_t)((view->height + 7) / 8));
    hipLaunchKernelGGL(k_volume_raycast, dim3((tiles + kWaves - 1) / kWaves), dim3(kBlock), 0, st, (const uint2 *)vol->a, (const uint2 *)vol->b,
                       vol->geom, V, d_z, d_i, d_w, d_stats);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st);
  if (!as_pyramid) {
    if (e == hipSuccess && depth) e = hipMemcpyAsync(depth, d_z, sizeof(float) * n_px, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && intensity) e = hipMemcpyAsync(intensity, d_i, sizeof(float) * n_px, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && weight) e = hipMemcpyAsync(weight, d_w, sizeof(int) * n_px, hipMemcpyDeviceToHost, st);
  }
  const hipError_t es = hipStreamSynchronize(st);  // the raycast's one synchronisation
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume raycast", e);
  bracket.read(1, 1);
  if (as_pyramid) {
    const PyramidSpec spec{view->width, view->height, view->fx, view->fy, view->ox, view->oy, levels, timestamp};
    const Level0Source src{d_i, d_z, view->width, nullptr, true};
    rc = pyramid_build(device, spec, src, out);
    if (rc) {
      *out = nullptr;
      return rc;
    }
  }
  if (stats) {
    stats->hit = h_stats[0], stats->backface = h_stats[1], stats->missed = h_stats[2], stats->uncoloured = h_stats[3];
    stats->pixels = stats->hit + stats->backface + stats->missed;
  }
  return DVO_AMD_OK;
}

void release_keyframes(dvo_amd_volume *vol) {
  for (auto &kv : vol->keyframes) dvo_amd_pyramid_release(kv.second.pyramid);
  vol->keyframes.clear();
}

}  // namespace

extern "C" {

void dvo_amd_default_volume_options(dvo_amd_volume_options *opt) {
  if (!opt) return;
  opt->nx = opt->ny = opt->nz = 64;
  opt->voxel = 0.05f;
  opt->origin[0] = -1.6f, opt->origin[1] = -1.6f, opt->origin[2] = 0.4f;
  opt->trunc = 0.15f, opt->near_z = 0.4f, opt->far_z = 5.0f;
  opt->weight = DVO_AMD_VOLUME_WEIGHT_SENSOR;
}

void dvo_amd_default_volume_raycast_options(dvo_amd_volume_raycast_options *opt) {
  if (!opt) return;
  opt->step_fraction = 0.5f, opt->min_weight = 1, opt->fill_intensity = 0.0f;
}

int dvo_amd_volume_create(int device, const dvo_amd_volume_options *opt, dvo_amd_volume **out) {
  static const char *entry = "dvo_amd_volume_create";
  if (out) *out = nullptr;
  if (!opt || !out) return invalid(entry, "a NULL pointer");
  const int dims[3] = {opt->nx, opt->ny, opt->nz};
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 2 || dims[a] > 2048) return invalid(entry, "nx, ny and nz must be in 2..2048");
  if ((long long)opt->nx * opt->ny * opt->nz > (1ll << 30)) return invalid(entry, "nx*ny*nz must not exceed 2^30");
  const float positive[4] = {opt->voxel, opt->trunc, opt->near_z, opt->far_z};
  for (float v : positive)
    if (!std::isfinite(v) || !(v > 0.0f)) return invalid(entry, "voxel, trunc, near_z and far_z must be finite and positive");
  if (opt->trunc < opt->voxel) return invalid(entry, "trunc must be >= voxel");
  if (opt->far_z <= opt->near_z) return invalid(entry, "far_z must be > near_z");
  if (!finite_all(opt->origin, 3)) return invalid(entry, "the origin has a non-finite entry");
  if (opt->weight != DVO_AMD_VOLUME_WEIGHT_CONSTANT && opt->weight != DVO_AMD_VOLUME_WEIGHT_SENSOR)
    return invalid(entry, "weight must be DVO_AMD_VOLUME_WEIGHT_CONSTANT or DVO_AMD_VOLUME_WEIGHT_SENSOR");
  int ndev = 0;
  int rc = have_device(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(entry, "no such device");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  dvo_amd_volume *vol = new dvo_amd_volume();
  vol->device = device, vol->opt = *opt;
  vol->geom = Geom{opt->nx, opt->ny, opt->nz, opt->voxel, {opt->origin[0], opt->origin[1], opt->origin[2]}, opt->trunc, opt->near_z, opt->far_z, opt->weight};
  vol->n_vox = (size_t)opt->nx * (size_t)opt->ny * (size_t)opt->nz;
  void *mem = nullptr;
  if (hipMalloc(&mem, 2 * sizeof(uint2) * vol->n_vox) != hipSuccess) {
    (void)hipGetLastError();
    delete vol;
    return DVO_AMD_ERR_OUT_OF_MEMORY;
  }
  vol->a = (uint2 *)mem, vol->b = vol->a + vol->n_vox;
  hipError_t e = hipMemsetAsync(mem, 0, 2 * sizeof(uint2) * vol->n_vox, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    (void)hipFree(mem);
    delete vol;
    return fail_hip("clearing a new volume", e);
  }
  *out = vol;
  return DVO_AMD_OK;
}

void dvo_amd_volume_destroy(dvo_amd_volume *vol) {
  if (!vol) return;
  release_keyframes(vol);
  if (hipSetDevice(vol->device) == hipSuccess && vol->a) (void)hipFree(vol->a);  // (hipFree waits for whatever still uses the memory)
  delete vol;
}

int dvo_amd_volume_clear(dvo_amd_volume *vol) {
  static const char *entry = "dvo_amd_volume_clear";
  if (!vol) return invalid(entry, "a NULL pointer");
  const int rc = have_device();
  if (rc) return rc;
  HIP_TRY(hipSetDevice(vol->device));
  hipStream_t st = nullptr;
  const int rs = device_prep_stream(vol->device, &st);
  if (rs) return rs;
  hipError_t e = hipMemsetAsync(vol->a, 0, 2 * sizeof(uint2) * vol->n_vox, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("clearing a volume", e);
  release_keyframes(vol);
  return DVO_AMD_OK;
}

int dvo_amd_volume_options_get(const dvo_amd_volume *vol, dvo_amd_volume_options *opt) {
  if (!vol || !opt) return invalid("dvo_amd_volume_options_get", "a NULL pointer");
  *opt = vol->opt;
  return DVO_AMD_OK;
}

int dvo_amd_volume_integrate(dvo_amd_volume *vol, int n, const dvo_amd_pyramid *const *pyramids, int level, const double *poses, int sign,
                             dvo_amd_volume_counts *counts) {
  static const char *entry = "dvo_amd_volume_integrate";
  if (n < 0) return invalid(entry, "a negative count");
  if (!vol || (n > 0 && !pyramids)) return invalid(entry, "a NULL pointer");
  if (sign != 1 && sign != -1) return invalid(entry, "sign must be +1 or -1");
  int rc = check_frames(entry, n, pyramids, level, poses);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    if (pyramids[k]->device != vol->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  std::vector<Item> items((size_t)n);
  for (int k = 0; k < n; ++k) {
    items[(size_t)k].pyramid = pyramids[k], items[(size_t)k].level = level, items[(size_t)k].sign = sign, items[(size_t)k].slot = k;
    inverse_rows(poses ? poses + 16 * (size_t)k : nullptr, items[(size_t)k].M);
  }
  std::vector<unsigned> near_free;
  rc = run_integration(vol, items, n, near_free);
  if (rc) return rc;
  if (counts)
    for (int k = 0; k < n; ++k) to_counts(near_free, k, counts + k);
  return DVO_AMD_OK;
}

int dvo_amd_volume_insert(dvo_amd_volume *vol, int n, const int *ids, dvo_amd_pyramid *const *pyramids, int level, const double *poses,
                          dvo_amd_volume_counts *counts) {
  static const char *entry = "dvo_amd_volume_insert";
  if (n < 0) return invalid(entry, "a negative count");
  if (!vol || (n > 0 && (!pyramids || !ids))) return invalid(entry, "a NULL pointer");
  int rc = check_frames(entry, n, pyramids, level, poses);
  if (!rc) rc = check_ids(entry, vol, n, ids, false);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    if (pyramids[k]->device != vol->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  std::vector<Item> items((size_t)n);
  for (int k = 0; k < n; ++k) {
    items[(size_t)k].pyramid = pyramids[k], items[(size_t)k].level = level, items[(size_t)k].sign = 1, items[(size_t)k].slot = k;
    inverse_rows(poses ? poses + 16 * (size_t)k : nullptr, items[(size_t)k].M);
  }
  std::vector<unsigned> near_free;
  rc = run_integration(vol, items, n, near_free);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    dvo_amd_volume_counts c;
    to_counts(near_free, k, &c);
    if (counts) counts[k] = c;
    dvo_amd_volume::Keyframe kf;
    kf.pyramid = pyramids[k], kf.level = level, kf.updated = c.updated;
    std::memcpy(kf.M, items[(size_t)k].M, sizeof(kf.M));
    dvo_amd_pyramid_retain(pyramids[k]);
    vol->keyframes[ids[k]] = kf;
  }
  return DVO_AMD_OK;
}

int dvo_amd_volume_set_poses(dvo_amd_volume *vol, int n, const int *ids, const double *poses) {
  static const char *entry = "dvo_amd_volume_set_poses";
  if (n < 0) return invalid(entry, "a negative count");
  if (!vol || (n > 0 && (!ids || !poses))) return invalid(entry, "a NULL pointer");
  int rc = check_ids(entry, vol, n, ids, true);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    if (!finite_all(poses + 16 * (size_t)k, 16)) return invalid(entry, "keyframe " + std::to_string(k) + ": the pose has a non-finite entry");
  rc = have_device();
  if (rc) return rc;
  // a moved keyframe: -1 at the float inverse pose it is stored with, +1 at the new one, in the same launch
  std::vector<Item> items;
  std::vector<int> moved;
  std::vector<std::array<float, 12>> Ms;
  for (int k = 0; k < n; ++k) {
    const dvo_amd_volume::Keyframe &kf = vol->keyframes[ids[k]];
    std::array<float, 12> M;
    inverse_rows(poses + 16 * (size_t)k, M.data());
    if (std::memcmp(M.data(), kf.M, sizeof(kf.M)) == 0) continue;  // the same floats: nothing moves
    Item sub{kf.pyramid, kf.level, {}, -1, -1}, add{kf.pyramid, kf.level, {}, 1, (int)moved.size()};
    std::memcpy(sub.M, kf.M, sizeof(kf.M)), std::memcpy(add.M, M.data(), sizeof(kf.M));
    items.push_back(sub), items.push_back(add);
    moved.push_back(ids[k]), Ms.push_back(M);
  }
  std::vector<unsigned> near_free;
  rc = run_integration(vol, items, (int)moved.size(), near_free);
  if (rc) return rc;
  for (size_t m = 0; m < moved.size(); ++m) {
    dvo_amd_volume::Keyframe &kf = vol->keyframes[moved[m]];
    dvo_amd_volume_counts c;
    to_counts(near_free, (int)m, &c);
    std::memcpy(kf.M, Ms[m].data(), sizeof(kf.M));
    kf.updated = c.updated;
  }
  return DVO_AMD_OK;
}

int dvo_amd_volume_remove(dvo_amd_volume *vol, int n, const int *ids) {
  static const char *entry = "dvo_amd_volume_remove";
  if (n < 0) return invalid(entry, "a negative count");
  if (!vol || (n > 0 && !ids)) return invalid(entry, "a NULL pointer");
  int rc = check_ids(entry, vol, n, ids, true);
  if (rc) return rc;
  rc = have_device();
  if (rc) return rc;
  std::vector<Item> items((size_t)n);
  for (int k = 0; k < n; ++k) {
    const dvo_amd_volume::Keyframe &kf = vol->keyframes[ids[k]];
    items[(size_t)k].pyramid = kf.pyramid, items[(size_t)k].level = kf.level, items[(size_t)k].sign = -1, items[(size_t)k].slot = -1;
    std::memcpy(items[(size_t)k].M, kf.M, sizeof(kf.M));
  }
  std::vector<unsigned> near_free;
  rc = run_integration(vol, items, 0, near_free);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    dvo_amd_pyramid_release(vol->keyframes[ids[k]].pyramid);
    vol->keyframes.erase(ids[k]);
  }
  return DVO_AMD_OK;
}

int dvo_amd_volume_stats(const dvo_amd_volume *vol, int *n_keyframes, long long *updated_total) {
  if (!vol) return invalid("dvo_amd_volume_stats", "a NULL pointer");
  long long total = 0;
  for (const auto &kv : vol->keyframes) total += kv.second.updated;
  if (n_keyframes) *n_keyframes = (int)vol->keyframes.size();
  if (updated_total) *updated_total = total;
  return DVO_AMD_OK;
}

int dvo_amd_volume_download(dvo_amd_volume *vol, const int *box, dvo_amd_volume_voxel *records, long long capacity, long long *n_out) {
  static const char *entry = "dvo_amd_volume_download";
  if (n_out) *n_out = 0;
  if (!vol || !n_out) return invalid(entry, "a NULL pointer");
  if (capacity < 0 || (capacity > 0 && !records)) return invalid(entry, "a negative capacity, or a capacity without records");
  const int dims[3] = {vol->opt.nx, vol->opt.ny, vol->opt.nz};
  int b[6] = {0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] - 1};
  if (box)
    for (int a = 0; a < 3; ++a) {
      if (!(0 <= box[a] && box[a] <= box[3 + a] && box[3 + a] < dims[a])) return invalid(entry, "the box must satisfy 0 <= lo <= hi < n on every axis");
      b[a] = box[a], b[3 + a] = box[3 + a];
    }
  const int3 lo = make_int3(b[0], b[1], b[2]), ext = make_int3(b[3] - b[0] + 1, b[4] - b[1] + 1, b[5] - b[2] + 1);
  const unsigned long long need = (unsigned long long)ext.x * (unsigned long long)ext.y * (unsigned long long)ext.z;
  int rc = have_device();
  if (rc) return rc;
  *n_out = (long long)need;
  if ((unsigned long long)capacity < need) return DVO_AMD_ERR_CAPACITY;
  HIP_TRY(hipSetDevice(vol->device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(vol->device, &st);
  if (rc) return rc;
  const unsigned long long chunk = std::min<unsigned long long>(need, 1ull << 21);  // 32 MiB of records at a time
  Scratch S;
  rc = S.take(vol->device, sizeof(uint4) * (size_t)chunk, true);
  if (rc) return rc;
  for (unsigned long long first = 0; first < need; first += chunk) {
    const unsigned count = (unsigned)std::min<unsigned long long>(chunk, need - first);
    hipLaunchKernelGGL(k_volume_gather, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint2 *)vol->a, (const uint2 *)vol->b,
                       vol->geom, lo, ext, first, count, (uint4 *)S.mem);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(records + first, S.mem, sizeof(uint4) * (size_t)count, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail_hip("volume download", e);
  }
  return DVO_AMD_OK;
}

int dvo_amd_volume_raycast(dvo_amd_volume *vol, const double *pose, const dvo_amd_view *view, const dvo_amd_volume_raycast_options *opt,
                           float *depth, float *intensity, int *weight, dvo_amd_volume_raycast_stats *stats) {
  return raycast("dvo_amd_volume_raycast", vol, pose, view, opt, -1, 0.0, depth, intensity, weight, nullptr, stats);
}

int dvo_amd_volume_raycast_pyramid(dvo_amd_volume *vol, const double *pose, const dvo_amd_view *view,
                                   const dvo_amd_volume_raycast_options *opt, int levels, double timestamp, dvo_amd_pyramid **out,
                                   dvo_amd_volume_raycast_stats *stats) {
  static const char *entry = "dvo_amd_volume_raycast_pyramid";
  if (out) *out = nullptr;
  if (!out) return invalid(entry, "a NULL pointer");
  if (levels < 0) return invalid(entry, "a negative level count");
  return raycast(entry, vol, pose, view, opt, levels, timestamp, nullptr, nullptr, nullptr, out, stats);
}

int dvo_amd_volume_extract(dvo_amd_volume *vol, int min_weight, dvo_amd_point *out, long long capacity, long long *n_out,
                           dvo_amd_volume_extract_counts *counts) {
  static const char *entry = "dvo_amd_volume_extract";
  if (n_out) *n_out = 0;
  if (!vol || !n_out) return invalid(entry, "a NULL pointer");
  if (min_weight < 1) return invalid(entry, "min_weight must be >= 1");
  if (capacity < 0 || (capacity > 0 && !out)) return invalid(entry, "a negative capacity, or a capacity without points");
  int rc = have_device();
  if (rc) return rc;
  const int device = vol->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  const unsigned n_tiles = (unsigned)((vol->n_vox + kTile - 1) / kTile);
  const size_t sums_bytes = align_up(sizeof(unsigned long long) * (size_t)n_tiles, 256);
  Scratch S;
  rc = S.take(device, sums_bytes + 256, true);
  if (rc) return rc;
  unsigned long long *d_sums = (unsigned long long *)S.mem;
  unsigned long long *d_grand = (unsigned long long *)((char *)S.mem + sums_bytes);
  unsigned *d_unc = (unsigned *)(d_grand + 1);
  Bracket bracket(g_timing[device]);
  unsigned long long grand = 0ull;
  hipError_t e = hipMemsetAsync(d_grand, 0, 256, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_volume_count, dim3(n_tiles), dim3(kBlock), 0, st, (const uint2 *)vol->a, (const uint2 *)vol->b, vol->geom, min_weight,
                       vol->n_vox, d_sums);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_volume_scan, dim3(1), dim3(kBlock), 0, st, d_sums, n_tiles, d_grand);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&grand, d_grand, sizeof(grand), hipMemcpyDeviceToHost, st);
  hipError_t es = hipStreamSynchronize(st);  // the total decides whether anything is written
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume extract (count)", e);
  *n_out = (long long)grand;
  if ((unsigned long long)capacity < grand) {
    if (bracket.timed) (void)bracket.end(st), (void)hipStreamSynchronize(st);
    bracket.read(2, 1);
    return DVO_AMD_ERR_CAPACITY;
  }
  Scratch P;
  unsigned h_unc = 0u;
  if (grand > 0ull) {
    rc = P.take(device, sizeof(dvo_amd_point) * (size_t)grand, true);
    if (rc) return rc;
    hipLaunchKernelGGL(k_volume_write, dim3(n_tiles), dim3(kBlock), 0, st, (const uint2 *)vol->a, (const uint2 *)vol->b, vol->geom, min_weight,
                       vol->n_vox, (const unsigned long long *)d_sums, (dvo_amd_point *)P.mem, grand, d_unc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && grand > 0ull) e = hipMemcpyAsync(out, P.mem, sizeof(dvo_amd_point) * (size_t)grand, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_unc, d_unc, sizeof(h_unc), hipMemcpyDeviceToHost, st);
  es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume extract (write)", e);
  bracket.read(grand > 0ull ? 3 : 2, 2);
  if (counts) counts->points = (long long)grand, counts->uncoloured = (long long)h_unc;
  return DVO_AMD_OK;
}

int dvo_amd_volume_upload(dvo_amd_volume *vol, const int *box, const dvo_amd_volume_voxel *records, long long n) {
  static const char *entry = "dvo_amd_volume_upload";
  if (n < 0) return invalid(entry, "a negative count");
  if (!vol || !records) return invalid(entry, "a NULL pointer");
  const int dims[3] = {vol->opt.nx, vol->opt.ny, vol->opt.nz};
  int b[6] = {0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] - 1};
  if (box)
    for (int a = 0; a < 3; ++a) {
      if (!(0 <= box[a] && box[a] <= box[3 + a] && box[3 + a] < dims[a])) return invalid(entry, "the box must satisfy 0 <= lo <= hi < n on every axis");
      b[a] = box[a], b[3 + a] = box[3 + a];
    }
  const int3 lo = make_int3(b[0], b[1], b[2]), ext = make_int3(b[3] - b[0] + 1, b[4] - b[1] + 1, b[5] - b[2] + 1);
  const unsigned long long need = (unsigned long long)ext.x * (unsigned long long)ext.y * (unsigned long long)ext.z;
  if (n < 0 || (unsigned long long)n != need) return invalid(entry, "n is " + std::to_string(n) + ", the box holds " + std::to_string(need) + " records");
  if (!vol->keyframes.empty())
    return invalid(entry, "the volume holds " + std::to_string(vol->keyframes.size()) + " keyframes of the tracked form: remove them or clear first");
  int rc = have_device();
  if (rc) return rc;
  HIP_TRY(hipSetDevice(vol->device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(vol->device, &st);
  if (rc) return rc;
  const unsigned long long chunk = std::min<unsigned long long>(need, 1ull << 21);  // 32 MiB of records at a time
  Scratch S;
  rc = S.take(vol->device, sizeof(uint4) * (size_t)chunk, true);
  if (rc) return rc;
  for (unsigned long long first = 0; first < need; first += chunk) {
    const unsigned count = (unsigned)std::min<unsigned long long>(chunk, need - first);
    hipError_t e = hipMemcpyAsync(S.mem, records + first, sizeof(uint4) * (size_t)count, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_volume_scatter, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, vol->a, vol->b, vol->geom, lo, ext, first,
                         count, (const uint4 *)S.mem);
      e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(st);  // (the scratch is filled again for the next stretch)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail_hip("volume upload", e);
  }
  return DVO_AMD_OK;
}

int dvo_amd_volume_mesh(dvo_amd_volume *vol, int min_weight, dvo_amd_point *vertices, float *normals, long long vertex_capacity, int *triangles,
                        long long triangle_capacity, dvo_amd_volume_mesh_counts *counts) {
  static const char *entry = "dvo_amd_volume_mesh";
  if (counts) *counts = dvo_amd_volume_mesh_counts{0, 0, 0, 0, 0};
  if (min_weight < 1) return invalid(entry, "min_weight must be >= 1");
  if (vertex_capacity < 0 || (vertex_capacity > 0 && !vertices)) return invalid(entry, "a negative vertex capacity, or a capacity without vertices");
  if (triangle_capacity < 0 || (triangle_capacity > 0 && !triangles))
    return invalid(entry, "a negative triangle capacity, or a capacity without triangles");
  if (!vol || !counts) return invalid(entry, "a NULL pointer");
  int rc = have_device();
  if (rc) return rc;
  const int device = vol->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  const Geom &G = vol->geom;
  Cells C;
  C.nx = G.nx - 1, C.ny = G.ny - 1, C.nz = G.nz - 1;
  C.n = (size_t)C.nx * (size_t)C.ny * (size_t)C.nz;
  const unsigned cell_tiles = (unsigned)((C.n + kCellTile - 1) / kCellTile), voxel_tiles = (unsigned)((vol->n_vox + kTile - 1) / kTile);
  const size_t n_words = (size_t)cell_tiles * kWordsPerTile;
  // the scratch: words, their offsets, the two lists of tile totals, then {vertices, faces} and {open, uncoloured, flat}
  const size_t word_bytes = align_up(sizeof(unsigned long long) * n_words, 256), offset_bytes = align_up(sizeof(unsigned) * n_words, 256);
  const size_t cell_bytes = align_up(sizeof(unsigned long long) * (size_t)cell_tiles, 256);
  const size_t face_bytes = align_up(sizeof(unsigned long long) * (size_t)voxel_tiles, 256);
  Scratch S;
  rc = S.take(device, word_bytes + offset_bytes + cell_bytes + face_bytes + 256, true);
  if (rc) return rc;
  char *base = (char *)S.mem;
  unsigned long long *d_word = (unsigned long long *)base;
  unsigned *d_offset = (unsigned *)(base + word_bytes);
  unsigned long long *d_cell_sums = (unsigned long long *)(base + word_bytes + offset_bytes);
  unsigned long long *d_face_sums = (unsigned long long *)(base + word_bytes + offset_bytes + cell_bytes);
  unsigned long long *d_grand = (unsigned long long *)(base + word_bytes + offset_bytes + cell_bytes + face_bytes);
  unsigned *d_cnt = (unsigned *)(d_grand + 2);  // open, uncoloured, flat
  C.word = d_word, C.word_offset = d_offset, C.tile_offset = d_cell_sums;
  const uint2 *pa = vol->a, *pb = vol->b;
  Bracket bracket(g_timing[device]);
  unsigned long long grand[2] = {0ull, 0ull};
  unsigned h_cnt[3] = {0u, 0u, 0u};
  hipError_t e = hipMemsetAsync(d_grand, 0, 256, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_mesh_cells, dim3(cell_tiles), dim3(kBlock), 0, st, pa, G, min_weight, C.n, d_word, d_offset, d_cell_sums);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_mesh_edges, dim3(voxel_tiles), dim3(kBlock), 0, st, pa, pb, G, C, min_weight, vol->n_vox, d_face_sums, d_cnt);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, d_cell_sums, cell_tiles, d_face_sums, voxel_tiles, d_grand);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(grand, d_grand, sizeof(grand), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, sizeof(unsigned), hipMemcpyDeviceToHost, st);
  hipError_t es = hipStreamSynchronize(st);  // the totals decide whether anything is written
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume mesh (count)", e);
  const unsigned long long n_vertices = grand[0], n_triangles = 2ull * grand[1];
  counts->vertices = (long long)n_vertices, counts->triangles = (long long)n_triangles, counts->open_edges = (long long)h_cnt[0];
  if ((unsigned long long)vertex_capacity < n_vertices || (unsigned long long)triangle_capacity < n_triangles) {
    if (bracket.timed) (void)bracket.end(st), (void)hipStreamSynchronize(st);
    bracket.read(3, 1);
    return DVO_AMD_ERR_CAPACITY;
  }
  Scratch P;
  int launches = 3;
  const size_t vertex_bytes = align_up(sizeof(dvo_amd_point) * (size_t)n_vertices, 256);
  const size_t normal_bytes = normals ? align_up(3 * sizeof(float) * (size_t)n_vertices, 256) : 0;
  const size_t triangle_bytes = align_up(3 * sizeof(int) * (size_t)n_triangles, 256);
  dvo_amd_point *d_vertices = nullptr;
  float *d_normals = nullptr;
  int *d_triangles = nullptr;
  if (n_vertices > 0ull) {  // (no vertex: no face either)
    rc = P.take(device, vertex_bytes + normal_bytes + triangle_bytes, true);
    if (rc) return rc;
    d_vertices = (dvo_amd_point *)P.mem;
    if (normals) d_normals = (float *)((char *)P.mem + vertex_bytes);
    d_triangles = (int *)((char *)P.mem + vertex_bytes + normal_bytes);
    hipLaunchKernelGGL(k_mesh_vertices, dim3(cell_tiles), dim3(kBlock), 0, st, pa, pb, G, C, d_vertices, d_normals, n_vertices, d_cnt + 1);
    e = hipGetLastError();
    launches = 4;
    if (e == hipSuccess && n_triangles > 0ull) {
      hipLaunchKernelGGL(k_mesh_faces, dim3(voxel_tiles), dim3(kBlock), 0, st, pa, pb, G, C, min_weight, vol->n_vox,
                         (const unsigned long long *)d_face_sums, d_triangles, n_triangles);
      e = hipGetLastError();
      launches = 5;
    }
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && n_vertices > 0ull) e = hipMemcpyAsync(vertices, d_vertices, sizeof(dvo_amd_point) * (size_t)n_vertices, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_vertices > 0ull && normals)
    e = hipMemcpyAsync(normals, d_normals, 3 * sizeof(float) * (size_t)n_vertices, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_triangles > 0ull) e = hipMemcpyAsync(triangles, d_triangles, 3 * sizeof(int) * (size_t)n_triangles, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st);
  es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("volume mesh (write)", e);
  bracket.read(launches, 2);
  counts->uncoloured = (long long)h_cnt[1], counts->flat = (long long)h_cnt[2];
  return DVO_AMD_OK;
}

int dvo_amd_write_ply(const char *path, const dvo_amd_point *vertices, const float *normals, long long n_vertices, const int *triangles,
                      long long n_triangles) {
  static const char *entry = "dvo_amd_write_ply";
  if (!path || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) return invalid(entry, "a NULL pointer");
  if (n_vertices < 0 || n_triangles < 0) return invalid(entry, "a negative count");
  for (long long i = 0; i < 3 * n_triangles; ++i)
    if (triangles[i] < 0 || triangles[i] >= n_vertices)
      return invalid(entry, "triangle " + std::to_string(i / 3) + " names vertex " + std::to_string(triangles[i]) + " of " + std::to_string(n_vertices));
  std::FILE *f = std::fopen(path, "wb");
  if (!f) return DVO_AMD_ERR_IO;
  bool ok = std::fprintf(f,
                         "ply\nformat binary_little_endian 1.0\ncomment dvo_amd_volume_mesh\nelement vertex %lld\n"
                         "property float x\nproperty float y\nproperty float z\n%s"
                         "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                         "element face %lld\nproperty list uchar int vertex_indices\nend_header\n",
                         n_vertices, normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", n_triangles) > 0;
  // records are packed by hand: 15 or 27 bytes a vertex, 13 a face (the values are little-endian as the host is)
  std::vector<unsigned char> rows;
  const size_t vertex_size = normals ? 27 : 15;
  const long long batch = 1 << 14;
  for (long long at = 0; ok && at < n_vertices; at += batch) {
    const size_t k = (size_t)std::min<long long>(batch, n_vertices - at);
    rows.resize(k * vertex_size);
    unsigned char *w = rows.data();
    for (size_t i = 0; i < k; ++i) {
      const dvo_amd_point &p = vertices[at + (long long)i];
      std::memcpy(w, &p.x, 12), w += 12;
      if (normals) std::memcpy(w, normals + 3 * (at + (long long)i), 12), w += 12;
      *w++ = (unsigned char)(p.rgb >> 16), *w++ = (unsigned char)(p.rgb >> 8), *w++ = (unsigned char)p.rgb;
    }
    ok = std::fwrite(rows.data(), vertex_size, k, f) == k;
  }
  for (long long at = 0; ok && at < n_triangles; at += batch) {
    const size_t k = (size_t)std::min<long long>(batch, n_triangles - at);
    rows.resize(k * 13);
    unsigned char *w = rows.data();
    for (size_t i = 0; i < k; ++i) {
      *w++ = 3;
      std::memcpy(w, triangles + 3 * (at + (long long)i), 12), w += 12;
    }
    ok = std::fwrite(rows.data(), 13, k, f) == k;
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? DVO_AMD_OK : DVO_AMD_ERR_IO;
}

int dvo_amd_debug_volume_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms) {
  return timing_entry(g_timing, device, enable, launches, synchronisations, last_ms);
}

}  // extern "C"
