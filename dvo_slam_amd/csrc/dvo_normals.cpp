// Surface normals on the device: which way the surface under a pixel faces, from the pyramid's own depth planes and rays.
//   dvo_amd_pyramid_normals       one level's normal plane (float4) and facing plane to the host
//   dvo_amd_mask_from_normals     an ordinary mask of the pixels that face the camera well enough, every level in ONE launch
//   dvo_amd_point_cloud_normals   dvo_amd_point_cloud plus every point's normal in the pose's frame
// The rule is RgbdImage::calculateNormals (rgbd_image.cpp:502-532) -- the cross product of the one-pixel central differences of
// the back-projected points -- summed un-normalised over a (2r+1)^2 window of pixels at about the centre's depth.  It is pinned
// operation by operation in include/dvo_amd.h ("Surface normals"); tests/normals_ref.py restates it in numpy.
//
//   k_normals   ONE launch over all levels of a call.  A level is cut into kTileW x kTileH tiles, one block each, a thread per
//               pixel; a block finds its level by its index in the records' block ranges (block-uniform: scalar registers).
//               r > 0: the depth tile with its r + 1 halo goes to LDS, the cross products of the tile and its r halo are
//               formed ONCE per block into LDS (a NaN x marks "not a member": outside the plane or not usable), and every
//               thread sums its window from LDS in the pinned order, dv outer, du inner.  Planes are stored component by
//               component, so that the 32 lanes of a tile row read 32 consecutive banks.
//               r = 0: a thread forms its own cross product from the four neighbours in global memory; no LDS, no barrier.
//               The tile shape does not show in the result: every pixel's sum runs over the same members in the same order
//               wherever the tile borders fall.
// Counts (defined, undefined, kept) are ballots and popcounts per wave, integer adds into LDS per block and one integer
// atomicAdd per non-zero count and block: integers only, no float atomic anywhere.
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <mutex>
#include <string>

namespace dvo_amd {
namespace normals {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kBlock = kTileW * kTileH;
constexpr int kMaxR = DVO_AMD_NORMAL_MAX_RADIUS;
constexpr int kCW = kTileW + 2 * kMaxR, kCH = kTileH + 2 * kMaxR;  // the cross products a block forms, at most
constexpr int kZW = kCW + 2, kZH = kCH + 2;                        // the depths it stages, at most
static_assert(kBlock == 256 && kBlock % 64 == 0, "four waves per block");
static_assert(DVO_AMD_NORMAL_MAX_RADIUS == 8, "the header's bound");

typedef float v4f __attribute__((ext_vector_type(4)));  // a normal (a plain vector type: storable to any address space)

// one level of one call as the kernel reads it (block-uniform: scalar registers)
struct Record {
  const float *z, *tx, *ty;  // the level's depth plane (w * h, tight rows) and rays
  float4 *normals;           // null: nobody asked
  float *facing;             // null: nobody asked
  unsigned char *mask;       // null: no mask is built
  int *kept;                 // the mask's counter of this level (with mask)
  unsigned *counts;          // {defined, undefined}
  int w, h, r;
  int tiles_x, block_first, block_end;  // the level's blocks are [block_first, block_end) of the launch
  float ratio, min_facing;
  int facing_kind, toward_camera, undefined_keep, rotate;
  float R[9];                // (rotate) row-major rotation applied to a defined normal
};


// steps 4..7 for a pixel whose window sum is (mx, my, mz) over `have` members, and its outputs
struct Pixel {
  float nx, ny, nz, nw, facing;
  bool defined;
};

__device__ __forceinline__ Pixel finish(const Record &L, bool have, float mx, float my, float mz, float px, float py, float pz) {
  const float nan = __builtin_nanf("");
  Pixel o;
  const float s = (mx * mx + my * my) + mz * mz;
  o.defined = have && s >= 1e-30f;  // (false for NaN)
  const float len = sqrtf(s);
  float nx = mx / len, ny = my / len, nz = mz / len;
  const float d = (nx * px + ny * py) + nz * pz;
  if (L.toward_camera != 0 && d > 0.0f) nx = -nx, ny = -ny, nz = -nz;
  float f;
  if (L.facing_kind == DVO_AMD_NORMAL_FACING_AXIS) {
    f = fabsf(nz);
  } else {
    const float pp = (px * px + py * py) + pz * pz;
    f = pp > 0.0f ? fabsf(d) / sqrtf(pp) : nan;
  }
  if (f != f) f = nan;  // (one NaN: the quiet one with a clear sign and payload)
  o.nx = o.defined ? nx : nan, o.ny = o.defined ? ny : nan, o.nz = o.defined ? nz : nan, o.nw = o.defined ? 0.0f : nan;
  o.facing = o.defined ? f : nan;
  return o;
}

__global__ void __launch_bounds__(kBlock) k_normals(const Record *__restrict__ records, int n_records) {
  __shared__ float s_z[kZW * kZH];
  __shared__ float s_cx[kCW * kCH], s_cy[kCW * kCH], s_cz[kCW * kCH];
  __shared__ float s_tx[kZW], s_ty[kZH];
  __shared__ unsigned s_cnt[3];

  int rec = 0;
  while (rec + 1 < n_records && (int)blockIdx.x >= records[rec].block_end) ++rec;  // (block-uniform)
  const Record L = records[rec];
  const int tile = (int)blockIdx.x - L.block_first;
  const int x0 = (tile % L.tiles_x) * kTileW, y0 = (tile / L.tiles_x) * kTileH;
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int u = x0 + lx, v = y0 + ly;
  const bool live = u < L.w && v < L.h;
  const int w = L.w, h = L.h, r = L.r;
  const DVO_DEVICE_GLOBAL float *Z = (const DVO_DEVICE_GLOBAL float *)L.z;
  const DVO_DEVICE_GLOBAL float *TX = (const DVO_DEVICE_GLOBAL float *)L.tx;
  const DVO_DEVICE_GLOBAL float *TY = (const DVO_DEVICE_GLOBAL float *)L.ty;
  const float nan = __builtin_nanf("");

  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;

  bool have = false;
  float mx = 0.f, my = 0.f, mz = 0.f, z = nan, px = 0.f, py = 0.f;
  if (r == 0) {
    // the reference's rule, a thread on its own: the four clamped neighbours straight from the plane
    if (live) {
      const int up = min(u + 1, w - 1), um = max(u - 1, 0), vp = min(v + 1, h - 1), vm = max(v - 1, 0);
      const size_t row = (size_t)v * (size_t)w;
      z = Z[row + (size_t)u];
      const float zp = Z[row + (size_t)up], zm = Z[row + (size_t)um];
      const float zq = Z[(size_t)vp * (size_t)w + (size_t)u], zn = Z[(size_t)vm * (size_t)w + (size_t)u];
      const float txu = TX[u], txp = TX[up], txm = TX[um], tyv = TY[v], tyq = TY[vp], tyn = TY[vm];
      const float ax = txp * zp - txm * zm, ay = tyv * zp - tyv * zm, az = zp - zm;
      const float bx = txu * zq - txu * zn, by = tyq * zq - tyn * zn, bz = zq - zn;
      const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      px = txu * z, py = tyv * z;
      const bool usable = rules::finite_f(cx) && rules::finite_f(cy) && rules::finite_f(cz);
      const bool near = !(L.ratio > 0.0f) || fabsf(z - z) <= L.ratio * z;
      have = rules::finite_f(z) && usable && near;
      mx = cx, my = cy, mz = cz;
    }
    __syncthreads();  // (s_cnt is cleared)
  } else {
    const int zw = kTileW + 2 * r + 2, zh = kTileH + 2 * r + 2;  // the staged depths: the tile and its r + 1 halo
    const int cw = kTileW + 2 * r, ch = kTileH + 2 * r;          // the cross products: the tile and its r halo
    const int zx0 = x0 - r - 1, zy0 = y0 - r - 1;
    for (int i = threadIdx.x; i < zw * zh; i += kBlock) {
      const int gx = zx0 + i % zw, gy = zy0 + i / zw;
      const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
      s_z[i] = in ? Z[(size_t)gy * (size_t)w + (size_t)gx] : nan;
    }
    if ((int)threadIdx.x < zw) {
      const int gx = zx0 + (int)threadIdx.x;
      s_tx[threadIdx.x] = gx >= 0 && gx < w ? TX[gx] : 0.0f;
    } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < zh) {
      const int gy = zy0 + (int)threadIdx.x - 64;
      s_ty[threadIdx.x - 64] = gy >= 0 && gy < h ? TY[gy] : 0.0f;
    }
    __syncthreads();
    // step 2 once per block: member (i, j) of the cross-product region is pixel (x0 - r + i, y0 - r + j), at (i + 1, j + 1) of
    // the depth region; its clamped neighbours are pixels of the plane within one step: inside the depth region
    for (int k = threadIdx.x; k < cw * ch; k += kBlock) {
      const int i = k % cw, j = k / cw;
      const int gx = x0 - r + i, gy = y0 - r + j;
      float cx = nan, cy = nan, cz = nan;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const int ip = min(gx + 1, w - 1) - zx0, im = max(gx - 1, 0) - zx0, iu = i + 1;
        const int jq = min(gy + 1, h - 1) - zy0, jn = max(gy - 1, 0) - zy0, jv = j + 1;
        const float zp = s_z[jv * zw + ip], zm = s_z[jv * zw + im], zq = s_z[jq * zw + iu], zn = s_z[jn * zw + iu];
        const float txu = s_tx[iu], txp = s_tx[ip], txm = s_tx[im], tyv = s_ty[jv], tyq = s_ty[jq], tyn = s_ty[jn];
        const float ax = txp * zp - txm * zm, ay = tyv * zp - tyv * zm, az = zp - zm;
        const float bx = txu * zq - txu * zn, by = tyq * zq - tyn * zn, bz = zq - zn;
        cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        if (!(rules::finite_f(cx) && rules::finite_f(cy) && rules::finite_f(cz))) cx = nan;  // not usable: never a member
      }
      s_cx[k] = cx, s_cy[k] = cy, s_cz[k] = cz;
    }
    __syncthreads();
    // step 3: the window of pixel (lx, ly) is rows ly .. ly + 2r, columns lx .. lx + 2r of the cross-product region
    z = s_z[(ly + r + 1) * zw + lx + r + 1];
    px = s_tx[lx + r + 1] * z, py = s_ty[ly + r + 1] * z;
    const float tol = L.ratio * z;
    const bool test = L.ratio > 0.0f;
    if (live && rules::finite_f(z)) {
      for (int dv = 0; dv <= 2 * r; ++dv) {
        const int crow = (ly + dv) * cw + lx, zrow = (ly + dv + 1) * zw + lx + 1;
        for (int du = 0; du <= 2 * r; ++du) {
          const float cx = s_cx[crow + du], cy = s_cy[crow + du], cz = s_cz[crow + du], zm = s_z[zrow + du];
          const bool add = cx == cx && (!test || fabsf(zm - z) <= tol);
          mx = add ? (have ? mx + cx : cx) : mx;
          my = add ? (have ? my + cy : cy) : my;
          mz = add ? (have ? mz + cz : cz) : mz;
          have = have || add;
        }
      }
    }
  }

  Pixel o = finish(L, have, mx, my, mz, px, py, z);
  bool keep = false;
  if (L.mask) keep = o.defined ? o.facing >= L.min_facing : L.undefined_keep != 0;  // (a NaN facing: false)
  if (L.rotate && o.defined) {
    const float nx = o.nx, ny = o.ny, nz = o.nz;
    o.nx = (L.R[0] * nx + L.R[1] * ny) + L.R[2] * nz;
    o.ny = (L.R[3] * nx + L.R[4] * ny) + L.R[5] * nz;
    o.nz = (L.R[6] * nx + L.R[7] * ny) + L.R[8] * nz;
  }
  if (live) {
    const size_t at = (size_t)v * (size_t)w + (size_t)u;
    if (L.normals) {
      v4f n4;
      n4[0] = o.nx, n4[1] = o.ny, n4[2] = o.nz, n4[3] = o.nw;
      ((DVO_DEVICE_GLOBAL v4f *)L.normals)[at] = n4;  // (one 16-byte store)
    }
    if (L.facing) ((DVO_DEVICE_GLOBAL float *)L.facing)[at] = o.facing;
    if (L.mask) ((DVO_DEVICE_GLOBAL unsigned char *)L.mask)[at] = keep ? 1 : 0;
  }
  const unsigned n_def = (unsigned)__popcll(__ballot(live && o.defined));
  const unsigned n_und = (unsigned)__popcll(__ballot(live && !o.defined));
  const unsigned n_keep = (unsigned)__popcll(__ballot(live && keep));
  if ((threadIdx.x & 63) == 0) {
    if (n_def) atomicAdd(&s_cnt[0], n_def);
    if (n_und) atomicAdd(&s_cnt[1], n_und);
    if (n_keep) atomicAdd(&s_cnt[2], n_keep);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned c = s_cnt[threadIdx.x];
    if (c) (void)__hip_atomic_fetch_add((DVO_DEVICE_GLOBAL unsigned *)L.counts + threadIdx.x, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (threadIdx.x == 2 && L.mask) {
    const unsigned c = s_cnt[2];
    if (c) (void)__hip_atomic_fetch_add((DVO_DEVICE_GLOBAL int *)L.kept, (int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace normals
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::normals;

namespace {

// dvo_amd_debug_normals_timing: what the last call on the device launched and waited for, and (when asked for) two events
// around its launch on the prep stream
DeviceTiming g_timing[kMaxDevices];

int check_options(const char *entry, const dvo_amd_pyramid *p, const dvo_amd_normal_options *opt) {
  for (int l = 0; l < p->n_levels && l < DVO_AMD_MAX_LEVELS; ++l)
    if (opt->radius[l] < 0 || opt->radius[l] > DVO_AMD_NORMAL_MAX_RADIUS)
      return invalid(entry, "radius[" + std::to_string(l) + "] is outside 0.." + std::to_string(DVO_AMD_NORMAL_MAX_RADIUS));
  if (!std::isfinite(opt->depth_step_ratio) || opt->depth_step_ratio < 0.0f)
    return invalid(entry, "depth_step_ratio must be finite and >= 0");
  if (opt->facing != DVO_AMD_NORMAL_FACING_AXIS && opt->facing != DVO_AMD_NORMAL_FACING_RAY)
    return invalid(entry, "facing must be DVO_AMD_NORMAL_FACING_AXIS or DVO_AMD_NORMAL_FACING_RAY");
  return DVO_AMD_OK;
}

// what every output of a level shares: where the level lies and how its pixels are judged
void fill_record(Record &R, const LevelData &L, int level, const dvo_amd_normal_options *opt, int &next_block) {
  R = Record{};
  R.z = L.z_plane, R.tx = L.tx, R.ty = L.ty;
  R.w = L.w, R.h = L.h, R.r = opt->radius[level];
  R.tiles_x = (L.w + kTileW - 1) / kTileW;
  R.block_first = next_block;
  next_block += R.tiles_x * ((L.h + kTileH - 1) / kTileH);
  R.block_end = next_block;
  R.ratio = opt->depth_step_ratio;
  R.facing_kind = opt->facing, R.toward_camera = opt->toward_camera;
}

// the call's own scratch on the device: the records and the counts in front, then whatever planes the call wants
struct CallScratch : Scratch {
  Record *records = nullptr;
  unsigned *counts = nullptr;  // [DVO_AMD_MAX_LEVELS][2]
  char *planes = nullptr;
};
constexpr size_t kRecordBytes = (sizeof(Record) * DVO_AMD_MAX_LEVELS + 255) / 256 * 256;
constexpr size_t kCountBytes = 256;
static_assert(sizeof(unsigned) * 2 * DVO_AMD_MAX_LEVELS <= kCountBytes, "two counts per level");

int scratch_alloc(CallScratch &S, int device, size_t plane_bytes) {
  const int rc = S.take(device, kRecordBytes + kCountBytes + plane_bytes);
  if (rc) return rc;
  S.records = (Record *)S.mem;
  S.counts = (unsigned *)(S.base() + kRecordBytes);
  S.planes = S.base() + kRecordBytes + kCountBytes;
  return DVO_AMD_OK;
}

// the records up, the counts cleared, the one launch (bracketed by the device's two events when timing is on)
hipError_t launch(const CallScratch &S, const Record *table, int n_records, int n_blocks, Bracket &bracket, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(S.records, table, sizeof(Record) * (size_t)n_records, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(S.counts, 0, kCountBytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_normals, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, (const Record *)S.records, n_records);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  return e;
}

// one level's planes into host memory; rotation: null, or nine floats applied to every defined normal
int level_to_host(const char *entry, const dvo_amd_pyramid *p, int level, const dvo_amd_normal_options *opt, const float *rotation,
                  float *normals, float *facing, long long *counts) {
  const int device = p->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  int rc = device_prep_stream(device, &st);
  if (rc) return rc;
  const LevelData &L = p->lv[level];
  if ((long long)L.w * L.h > (1ll << 30)) return invalid(entry, "the level is larger than 2^30 pixels");
  const size_t n = (size_t)L.n;
  const size_t normal_bytes = normals ? align_up(16 * n, 256) : 0, facing_bytes = facing ? align_up(4 * n, 256) : 0;
  CallScratch S;
  rc = scratch_alloc(S, device, normal_bytes + facing_bytes);
  if (rc) return rc;
  Record R;
  int n_blocks = 0;
  fill_record(R, L, level, opt, n_blocks);
  R.normals = normals ? (float4 *)S.planes : nullptr;
  R.facing = facing ? (float *)(S.planes + normal_bytes) : nullptr;
  R.counts = S.counts;
  if (rotation) {
    R.rotate = 1;
    for (int i = 0; i < 9; ++i) R.R[i] = rotation[i];
  }
  Bracket bracket(g_timing[device]);
  unsigned h_counts[2] = {0u, 0u};
  hipError_t e = launch(S, &R, 1, n_blocks, bracket, st);
  if (e == hipSuccess && normals) e = hipMemcpyAsync(normals, R.normals, 16 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && facing) e = hipMemcpyAsync(facing, R.facing, 4 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts, S.counts, sizeof(h_counts), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // the call's one synchronisation (before the scratch goes back, whatever failed)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("surface normals", e);
  bracket.read(1, 1);
  if (counts) counts[0] = h_counts[0], counts[1] = h_counts[1];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_normal_options(dvo_amd_normal_options *opt) {
  if (!opt) return;
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) opt->radius[l] = 0;
  opt->depth_step_ratio = 0.0f;
  opt->facing = DVO_AMD_NORMAL_FACING_AXIS, opt->toward_camera = 0;
}

int dvo_amd_pyramid_normals(const dvo_amd_pyramid *p, int level, const dvo_amd_normal_options *opt, float *normals, float *facing,
                            long long *counts) {
  static const char *entry = "dvo_amd_pyramid_normals";
  if (!p || !opt) return invalid(entry, "a NULL pointer");
  if (level < 0 || level >= p->n_levels) return invalid(entry, "no such level");
  int rc = check_options(entry, p, opt);
  if (rc) return rc;
  rc = have_device();
  if (rc) return rc;
  return level_to_host(entry, p, level, opt, nullptr, normals, facing, counts);
}

int dvo_amd_mask_from_normals(const dvo_amd_pyramid *p, const dvo_amd_normal_options *opt, const float *min_facing, int undefined_keep,
                              dvo_amd_mask **out, long long *counts) {
  static const char *entry = "dvo_amd_mask_from_normals";
  if (out) *out = nullptr;
  if (!p || !opt || !min_facing || !out) return invalid(entry, "a NULL pointer");
  int rc = check_options(entry, p, opt);
  if (rc) return rc;
  for (int l = 0; l < p->n_levels && l < DVO_AMD_MAX_LEVELS; ++l)
    if (min_facing[l] != min_facing[l]) return invalid(entry, "min_facing[" + std::to_string(l) + "] is NaN");
  rc = have_device();
  if (rc) return rc;
  const int levels = p->n_levels, device = p->device;
  rc = check_mask_size(entry, p->lv[0].w, p->lv[0].h, levels);
  if (rc) return rc;
  dvo_amd_mask *m = nullptr;
  hipStream_t st = nullptr;
  rc = mask_alloc(entry, device, p->lv[0].w, p->lv[0].h, levels, &m, &st);
  if (rc) return rc;
  CallScratch S;
  rc = scratch_alloc(S, device, 0);
  if (rc) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(m->mem);
    delete m;
    return rc;
  }
  Record table[DVO_AMD_MAX_LEVELS];
  int n_blocks = 0;
  for (int l = 0; l < levels; ++l) {
    Record &R = table[l];
    fill_record(R, p->lv[l], l, opt, n_blocks);
    R.mask = m->plane[l], R.kept = m->counters + l, R.counts = S.counts + 2 * l;
    R.min_facing = min_facing[l], R.undefined_keep = undefined_keep;
  }
  Bracket bracket(g_timing[device]);
  unsigned h_counts[2 * DVO_AMD_MAX_LEVELS] = {};
  hipError_t e = launch(S, table, levels, n_blocks, bracket, st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts, S.counts, sizeof(unsigned) * 2 * (size_t)levels, hipMemcpyDeviceToHost, st);
  rc = mask_finish(m, e, st, out);  // the call's one synchronisation; on failure the mask is gone (and the stream drained)
  if (rc) {
    *out = nullptr;
    return rc;
  }
  bracket.read(1, 1);
  if (counts)
    for (int l = 0; l < levels; ++l) counts[3 * l] = h_counts[2 * l], counts[3 * l + 1] = h_counts[2 * l + 1], counts[3 * l + 2] = (*out)->kept[l];
  return DVO_AMD_OK;
}

int dvo_amd_point_cloud_normals(dvo_amd_context *ctx, dvo_amd_pyramid *image, int level, const double *pose, const unsigned char *bgr,
                                int bgr_stride_bytes, const dvo_amd_normal_options *opt, dvo_amd_point *out, float *normals) {
  static const char *entry = "dvo_amd_point_cloud_normals";
  if (!ctx || !image || !opt || !out || !normals) return invalid(entry, "a NULL pointer");
  if (level < 0 || level >= image->n_levels) return invalid(entry, "no such level");
  if (pose && !finite_all(pose, 16)) return invalid(entry, "the pose has a non-finite entry");
  int rc = check_options(entry, image, opt);
  if (rc) return rc;
  if (ctx->device != image->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  rc = dvo_amd_point_cloud(ctx, image, level, pose, bgr, bgr_stride_bytes, out);
  if (rc) return rc;
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (pose)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (float)pose[4 * c + r];  // (column-major)
  return level_to_host(entry, image, level, opt, R, normals, nullptr, nullptr);
}

int dvo_amd_write_pcd_normals(const char *path, const dvo_amd_point *points, const float *normals, long long n, int width, int height) {
  static const char *entry = "dvo_amd_write_pcd_normals";
  if (!path || (n > 0 && (!points || !normals))) return invalid(entry, "a NULL pointer");
  if (n < 0 || width < 0 || height < 0 || (long long)width * height != n) return invalid(entry, "width * height is not the point count");
  std::FILE *f = std::fopen(path, "wb");
  if (!f) return DVO_AMD_ERR_IO;
  // pcl::PCDWriter::generateHeader for PointXYZRGBNormal; the binary block holds the eight fields packed, 32 bytes per point
  const int h = std::fprintf(f,
                             "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n"
                             "FIELDS x y z rgb normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4 4\n"
                             "TYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT %d\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %lld\n"
                             "DATA binary\n",
                             width, height, n);
  bool ok = h > 0;
  struct Rec {
    dvo_amd_point p;
    float normal[3], curvature;
  };
  static_assert(sizeof(Rec) == 32, "a PointXYZRGBNormal record of the file is 32 bytes");
  std::vector<Rec> rows((size_t)std::min<long long>(n, 1 << 14));
  for (long long at = 0; ok && at < n; at += (long long)rows.size()) {
    const size_t k = (size_t)std::min<long long>((long long)rows.size(), n - at);
    for (size_t i = 0; i < k; ++i) {
      Rec &r = rows[i];
      r.p = points[at + (long long)i];
      for (int c = 0; c < 3; ++c) r.normal[c] = normals[4 * (at + (long long)i) + c];
      r.curvature = 0.0f;
    }
    ok = std::fwrite(rows.data(), sizeof(Rec), k, f) == k;
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? DVO_AMD_OK : DVO_AMD_ERR_IO;
}

/* instrumentation: *launches / *synchronisations (may be NULL) receive what the most recent dvo_amd_pyramid_normals,
 * dvo_amd_mask_from_normals or normal pass of dvo_amd_point_cloud_normals on `device` launched and waited for; with enable != 0
 * the launch of every later call is bracketed by two events on the prep stream and *last_ms (may be NULL) receives the device
 * time of the most recent bracketed launch */
int dvo_amd_debug_normals_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms) {
  return timing_entry(g_timing, device, enable, launches, synchronisations, last_ms);
}

}  // extern "C"
