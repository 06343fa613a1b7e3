// Depth filtering on the device: one frame's level-0 depth denoised by an edge-preserving filter whose range scale is the sensor's
// own noise model, unsupported (flying) pixels dropped, small holes filled from the farthest surface around them.
//   dvo_amd_pyramid_filter_depth        a new ordinary pyramid whose level-0 depth is the filtered plane
//   dvo_amd_pyramid_filter_depth_many   the same for n pyramids, of any sizes, in ONE launch and one synchronisation
// The rule is pinned operation by operation in include/dvo_amd.h ("Depth filtering"); tests/depth_filter_ref.py restates it.
//
//   k_depth_filter   ONE launch over all pyramids of a call.  Level 0 of each is cut into kTileW x kTileH tiles, one block each, a
//                    thread per pixel; a block finds its pyramid by its index in the records' block ranges (block-uniform: scalar
//                    registers).  The depth tile with a halo of max(radius, fill_radius) goes to LDS, NaN outside the plane, and
//                    every thread sums its window from LDS in the pinned order, dy outer, dx inner; the loop bounds and the
//                    spatial weights (a table the host fills once per call) are block-uniform.  With both radii 0 a thread works
//                    on its own pixel alone: no LDS plane, one barrier (for the counts).
//                    Only the input plane is read and every pixel's sums run over the same members in the same order wherever the
//                    tile borders fall: the tile shape does not show in the result.
// Counts (with_depth, kept, dropped, holes, filled) are ballots and popcounts per wave, integer adds into LDS per block and one
// integer atomicAdd per non-zero count and block: integers only, no float atomic anywhere.
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

namespace dvo_amd {
namespace depth_filter {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kBlock = kTileW * kTileH;
constexpr int kMaxR = DVO_AMD_DEPTH_FILTER_MAX_RADIUS;
constexpr int kZW = kTileW + 2 * kMaxR, kZH = kTileH + 2 * kMaxR;  // the depths a block stages, at most
constexpr int kCounts = DVO_AMD_DEPTH_FILTER_COUNTS;
constexpr int kSide = 2 * kMaxR + 1;
constexpr int kTable = kSide * kSide;  // the spatial weights of one window, at most
static_assert(kBlock == 256 && kBlock % 64 == 0, "four waves per block");
static_assert(DVO_AMD_DEPTH_FILTER_MAX_RADIUS == 8 && DVO_AMD_DEPTH_FILTER_COUNTS == 5, "the header's bounds");


// one pyramid of one call as the kernel reads it (block-uniform: scalar registers)
struct Record {
  const float *z;           // level 0's depth plane (w * h, tight rows)
  float *out;               // the filtered plane
  unsigned short *support;  // null: nobody asked
  unsigned *counts;         // {with_depth, kept, dropped, holes, filled}
  int w, h;
  int tiles_x, block_first, block_end;  // the pyramid's blocks are [block_first, block_end) of the launch
  int pad;
};

// what every pyramid of a call shares
struct Params {
  int radius, fill_radius, min_support, min_fill_support;
  float range_sigmas;
};


// ws: (2 radius + 1)^2 weights of the filter window, then (2 fill_radius + 1)^2 of the fill window, rows dy, columns dx
__global__ void __launch_bounds__(kBlock) k_depth_filter(const Record *__restrict__ records, int n_records, const float *__restrict__ ws,
                                                         Params P) {
  __shared__ float s_z[kZW * kZH];
  __shared__ unsigned s_cnt[kCounts];

  int lo = 0, hi = n_records - 1;  // the first record whose block range ends behind this block (block-uniform)
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if ((int)blockIdx.x >= records[mid].block_end)
      lo = mid + 1;
    else
      hi = mid;
  }
  const Record L = records[lo];
  const int tile = (int)blockIdx.x - L.block_first;
  const int x0 = (tile % L.tiles_x) * kTileW, y0 = (tile / L.tiles_x) * kTileH;
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int u = x0 + lx, v = y0 + ly;
  const int w = L.w, h = L.h;
  const bool live = u < w && v < h;
  const int r = P.radius, fr = P.fill_radius;
  const int halo = max(r, fr);
  const DVO_DEVICE_GLOBAL float *Z = (const DVO_DEVICE_GLOBAL float *)L.z;
  const DVO_DEVICE_GLOBAL float *WS = (const DVO_DEVICE_GLOBAL float *)ws;
  const float nan = __builtin_nanf("");

  if (threadIdx.x < kCounts) s_cnt[threadIdx.x] = 0u;

  const int zw = kTileW + 2 * halo;
  float zc = nan;
  if (halo == 0) {
    if (live) zc = Z[(size_t)v * (size_t)w + (size_t)u];
  } else {
    const int zh = kTileH + 2 * halo;
    const int zx0 = x0 - halo, zy0 = y0 - halo;
    for (int i = threadIdx.x; i < zw * zh; i += kBlock) {
      const int gx = zx0 + i % zw, gy = zy0 + i / zw;
      const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
      s_z[i] = in ? Z[(size_t)gy * (size_t)w + (size_t)gx] : nan;
    }
  }
  __syncthreads();  // (s_cnt is cleared; the tile is staged)
  if (halo != 0) zc = s_z[(ly + halo) * zw + lx + halo];  // (NaN for a thread outside the plane)

  const bool has = live && rules::finite_f(zc);
  float out = nan;
  int n = 0;
  bool kept = false, filled = false;
  if (has) {
    // steps 1 and 2: the members of the window are the positions within s of the centre; a position outside the plane holds NaN
    const float s = P.range_sigmas * rules::depth_sigma(zc);
    const float ss = s * s;
    float sw = 0.0f, swd = 0.0f;
    if (halo == 0) {
      const float d = zc - zc;
      if (fabsf(d) <= s) {
        const float wr = 1.0f - (d * d) / ss;
        const float wt = WS[0] * wr;
        sw = sw + wt, swd = swd + wt * d, n = 1;
      }
    } else {
      const int off = halo - r, side = 2 * r + 1;
      for (int dy = 0; dy < side; ++dy) {
        const int row = (ly + off + dy) * zw + lx + off;
        for (int dx = 0; dx < side; ++dx) {
          const float zm = s_z[row + dx];
          const float d = zm - zc;
          const bool member = fabsf(d) <= s;  // (false for a NaN zm)
          const float wr = 1.0f - (d * d) / ss;
          const float wt = WS[dy * side + dx] * wr;
          sw = member ? sw + wt : sw;
          swd = member ? swd + wt * d : swd;
          n += member ? 1 : 0;
        }
      }
    }
    kept = n >= P.min_support;
    out = kept ? zc + swd / sw : nan;
  } else if (live && fr > 0) {
    // step 3: a hole takes the weighted mean of the farthest surface in its window
    const int off = halo - fr, side = 2 * fr + 1;
    const DVO_DEVICE_GLOBAL float *WF = WS + (2 * r + 1) * (2 * r + 1);
    float zfar = nan;
    for (int dy = 0; dy < side; ++dy) {
      const int row = (ly + off + dy) * zw + lx + off;
      for (int dx = 0; dx < side; ++dx) {
        const float zm = s_z[row + dx];
        if (rules::finite_f(zm) && !(zfar >= zm)) zfar = zm;  // (the first finite one, then every larger one)
      }
    }
    if (rules::finite_f(zfar)) {
      const float s = P.range_sigmas * rules::depth_sigma(zfar);
      float sw = 0.0f, swd = 0.0f;
      for (int dy = 0; dy < side; ++dy) {
        const int row = (ly + off + dy) * zw + lx + off;
        for (int dx = 0; dx < side; ++dx) {
          const float zm = s_z[row + dx];
          const bool member = rules::finite_f(zm) && zfar - zm <= s;
          const float wt = WF[dy * side + dx];
          sw = member ? sw + wt : sw;
          swd = member ? swd + wt * (zm - zfar) : swd;
          n += member ? 1 : 0;
        }
      }
      filled = n >= P.min_fill_support;
      out = filled ? zfar + swd / sw : nan;
    }
  }

  if (live) {
    const size_t at = (size_t)v * (size_t)w + (size_t)u;
    ((DVO_DEVICE_GLOBAL float *)L.out)[at] = out;
    if (L.support) ((DVO_DEVICE_GLOBAL unsigned short *)L.support)[at] = (unsigned short)(has ? n : 0);
  }
  const unsigned n_has = (unsigned)__popcll(__ballot(has));
  const unsigned n_kept = (unsigned)__popcll(__ballot(has && kept));
  const unsigned n_holes = (unsigned)__popcll(__ballot(live && !has));
  const unsigned n_filled = (unsigned)__popcll(__ballot(filled));
  if ((threadIdx.x & 63) == 0) {
    if (n_has) atomicAdd(&s_cnt[0], n_has);
    if (n_kept) atomicAdd(&s_cnt[1], n_kept);
    if (n_has - n_kept) atomicAdd(&s_cnt[2], n_has - n_kept);
    if (n_holes) atomicAdd(&s_cnt[3], n_holes);
    if (n_filled) atomicAdd(&s_cnt[4], n_filled);
  }
  __syncthreads();
  if (threadIdx.x < kCounts) {
    const unsigned c = s_cnt[threadIdx.x];
    if (c) (void)__hip_atomic_fetch_add((DVO_DEVICE_GLOBAL unsigned *)L.counts + threadIdx.x, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace depth_filter
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::depth_filter;

namespace {

// dvo_amd_debug_depth_filter_timing: two events around the filter launch on the prep stream, when asked for
DeviceTiming g_timing[kMaxDevices];

int check_options(const char *entry, const dvo_amd_depth_filter_options *opt) {
  const std::string top = std::to_string(DVO_AMD_DEPTH_FILTER_MAX_RADIUS);
  if (opt->radius < 0 || opt->radius > DVO_AMD_DEPTH_FILTER_MAX_RADIUS) return invalid(entry, "radius is outside 0.." + top);
  if (opt->fill_radius < 0 || opt->fill_radius > DVO_AMD_DEPTH_FILTER_MAX_RADIUS) return invalid(entry, "fill_radius is outside 0.." + top);
  if (!std::isfinite(opt->range_sigmas) || !(opt->range_sigmas > 0.0f)) return invalid(entry, "range_sigmas must be finite and positive");
  const int window = (2 * opt->radius + 1) * (2 * opt->radius + 1);
  if (opt->min_support < 1 || opt->min_support > window) return invalid(entry, "min_support is outside 1.." + std::to_string(window));
  const int fill_window = (2 * opt->fill_radius + 1) * (2 * opt->fill_radius + 1);
  if (opt->fill_radius > 0 && (opt->min_fill_support < 1 || opt->min_fill_support > fill_window))
    return invalid(entry, "min_fill_support is outside 1.." + std::to_string(fill_window));
  return DVO_AMD_OK;
}

// ws(dy, dx) = B_r[dy] * B_r[dx] with B_r[d] = (float) C(2r, r + d): (2r + 1)^2 floats, rows dy, one rounded product each
void binomial_window(int r, float *ws) {
  float B[kSide];
  double c = 1.0;  // C(2r, k), exact: at most C(16, 8) = 12870
  for (int k = 0; k <= 2 * r; ++k) {
    B[k] = (float)c;
    c = c * (double)(2 * r - k) / (double)(k + 1);
  }
  const int side = 2 * r + 1;
  for (int dy = 0; dy < side; ++dy)
    for (int dx = 0; dx < side; ++dx) ws[dy * side + dx] = B[dy] * B[dx];
}

int filter_many(const char *entry, int n, const dvo_amd_pyramid *const *p, const dvo_amd_depth_filter_options *opt, dvo_amd_pyramid **out,
                long long *counts, unsigned short *const *support) {
  if (out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative pyramid count");
  if (!p || !opt || !out) return invalid(entry, "a NULL pointer");
  for (int k = 0; k < n; ++k)
    if (!p[k]) return invalid(entry, "pyramid " + std::to_string(k) + " is NULL");
  int rc = check_options(entry, opt);
  if (rc) return rc;
  for (int k = 0; k < n; ++k)
    if (p[k]->device != p[0]->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  // the geometry of the one launch, and the call's own scratch: the records, the two weight windows and the counts in front, then a
  // filtered plane per pyramid and the support planes of the pyramids that ask for them
  const size_t record_bytes = align_up(sizeof(Record) * (size_t)n, 256);
  const size_t table_bytes = align_up(sizeof(float) * 2 * (size_t)kTable, 256);
  const size_t count_bytes = align_up(sizeof(unsigned) * (size_t)kCounts * (size_t)n, 256);
  std::vector<size_t> plane_at((size_t)n), support_at((size_t)n, 0);
  std::vector<Record> table((size_t)n);
  size_t scratch_bytes = record_bytes + table_bytes + count_bytes;
  long long n_blocks = 0;
  for (int k = 0; k < n; ++k) {
    const LevelData &L = p[k]->lv[0];
    if ((long long)L.w * L.h > (1ll << 30)) return invalid(entry, "pyramid " + std::to_string(k) + ": level 0 is larger than 2^30 pixels");
    plane_at[(size_t)k] = scratch_bytes;
    scratch_bytes += align_up(sizeof(float) * (size_t)L.n, 256);
    Record &R = table[(size_t)k];
    R = Record{};
    R.w = L.w, R.h = L.h;
    R.tiles_x = (L.w + kTileW - 1) / kTileW;
    R.block_first = (int)n_blocks;
    n_blocks += (long long)R.tiles_x * ((L.h + kTileH - 1) / kTileH);
    if (n_blocks > (1ll << 30)) return invalid(entry, "the call holds more than 2^30 tiles");
    R.block_end = (int)n_blocks;
  }
  for (int k = 0; k < n; ++k)
    if (support && support[k]) {
      support_at[(size_t)k] = scratch_bytes;
      scratch_bytes += align_up(sizeof(unsigned short) * (size_t)p[k]->lv[0].n, 256);
    }

  const int device = p[0]->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  Scratch scratch;  // (every return below stands behind a synchronisation of the stream: the filter's own, then pyramid_build's)
  rc = scratch.take(device, scratch_bytes);
  if (rc) return rc;
  char *base = scratch.base();
  Record *d_records = (Record *)base;
  float *d_ws = (float *)(base + record_bytes);
  unsigned *d_counts = (unsigned *)(base + record_bytes + table_bytes);
  for (int k = 0; k < n; ++k) {
    Record &R = table[(size_t)k];
    R.z = p[k]->lv[0].z_plane;
    R.out = (float *)(base + plane_at[(size_t)k]);
    R.support = support && support[k] ? (unsigned short *)(base + support_at[(size_t)k]) : nullptr;
    R.counts = d_counts + (size_t)kCounts * (size_t)k;
  }
  float h_ws[2 * kTable] = {};
  const int window = (2 * opt->radius + 1) * (2 * opt->radius + 1), fill_window = (2 * opt->fill_radius + 1) * (2 * opt->fill_radius + 1);
  binomial_window(opt->radius, h_ws);
  binomial_window(opt->fill_radius, h_ws + window);
  std::vector<unsigned> h_counts((size_t)kCounts * (size_t)n);
  const Params P{opt->radius, opt->fill_radius, opt->min_support, opt->min_fill_support, opt->range_sigmas};

  Bracket bracket(g_timing[device]);
  hipError_t e = hipMemcpyAsync(d_records, table.data(), sizeof(Record) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_ws, h_ws, sizeof(float) * (size_t)(window + fill_window), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = bracket.begin(st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_depth_filter, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, (const Record *)d_records, n, (const float *)d_ws, P);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), d_counts, sizeof(unsigned) * h_counts.size(), hipMemcpyDeviceToHost, st);
  for (int k = 0; k < n && e == hipSuccess; ++k)
    if (support && support[k])
      e = hipMemcpyAsync(support[k], base + support_at[(size_t)k], sizeof(unsigned short) * (size_t)p[k]->lv[0].n, hipMemcpyDeviceToHost, st);
  // the filter's one synchronisation (whatever failed, the stream is drained before the scratch goes back to the pool)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("depth filtering", e);
  bracket.read();
  // every pyramid from its own intensity plane and its filtered plane, by the builder every pyramid comes from
  for (int k = 0; k < n; ++k) {
    const LevelData &L = p[k]->lv[0];
    const PyramidSpec spec{L.w, L.h, L.fx, L.fy, L.ox, L.oy, p[k]->n_levels, p[k]->timestamp};
    const Level0Source src{L.i_plane, (const float *)(base + plane_at[(size_t)k]), L.w, nullptr, true};
    rc = pyramid_build(device, spec, src, &out[k]);
    if (rc) {
      for (int j = 0; j < k; ++j) dvo_amd_pyramid_release(out[j]), out[j] = nullptr;
      out[k] = nullptr;
      return rc;
    }
  }
  // (pyramid_build drained the stream: nothing reads the scratch any more when it goes out of scope)
  if (counts)
    for (size_t i = 0; i < h_counts.size(); ++i) counts[i] = (long long)h_counts[i];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_depth_filter_options(dvo_amd_depth_filter_options *opt) {
  if (!opt) return;
  opt->radius = 2, opt->range_sigmas = 3.0f, opt->min_support = 1, opt->fill_radius = 0, opt->min_fill_support = 3;
}

int dvo_amd_pyramid_filter_depth_many(int n, const dvo_amd_pyramid *const *p, const dvo_amd_depth_filter_options *opt, dvo_amd_pyramid **out,
                                      long long *counts, unsigned short *const *support) {
  return filter_many("dvo_amd_pyramid_filter_depth_many", n, p, opt, out, counts, support);
}

int dvo_amd_pyramid_filter_depth(const dvo_amd_pyramid *p, const dvo_amd_depth_filter_options *opt, dvo_amd_pyramid **out, long long *counts,
                                 unsigned short *support) {
  static const char *entry = "dvo_amd_pyramid_filter_depth";
  if (out) *out = nullptr;
  if (!p || !opt || !out) return invalid(entry, "a NULL pointer");
  return filter_many(entry, 1, &p, opt, out, counts, support ? &support : nullptr);
}

/* instrumentation: with enable != 0 the filter launch of every later dvo_amd_pyramid_filter_depth / _many on `device` is bracketed
 * by two events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent bracketed launch */
int dvo_amd_debug_depth_filter_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
