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
//   k_volume_gather     the public records of an index box, packed for the copy to the host
#include "dvo_internal.h"
#include "dvo_device_rules.h"
#include "dvo_volume_box.h"

#include <algorithm>
#include <array>
#include <cmath>
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
__global__ void __launch_bounds__(kBlock) k_volume_scan(unsigned long long *__restrict__ tile_sums, unsigned n_tiles,
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

int dvo_amd_debug_volume_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms) {
  return timing_entry(g_timing, device, enable, launches, synchronisations, last_ms);
}

}  // extern "C"
