// Device pools, pyramid construction and point selection: RgbdCameraPyramid / RgbdImagePyramid / PointSelection of the reference
// (rgbd_image.cpp:38-55,127-172,186-296,419-543, rgbd_image_sse.cpp:241-284, point_selection.cpp:68-152) as device-resident,
// immutable handles, and the dvo_amd_pyramid_* entries of the C ABI.
#include <dlfcn.h>
#include <emmintrin.h>  // the host side of the record hand-off takes 16 bytes at a time (x86-64 hosts)

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dvo_internal.h"

namespace dvo_amd {
namespace host {

// ---- per-device shared state: a prep stream and a pool of pyramid slabs ------------------------------------------
// Level descriptors (pointers + intrinsics of a pyramid level, ~1 KB per pyramid) are read by every block of every launch
// before it can touch a pixel.  Inside a pyramid's own 20 MB slab they would be a cold line in HBM each time a pair comes
// back to it; kept together in a small arena per device they stay in L2 / Infinity Cache.
constexpr size_t kDescEntryBytes = 1024;
constexpr size_t kDescChunkEntries = 256;
constexpr size_t kRefDesc0Offset = 640;  // where the first selection's descriptors start inside a pyramid's entry
struct DeviceState {
  std::mutex mu;
  hipStream_t prep_stream = nullptr;
  std::vector<std::pair<size_t, void *>> free_slabs;
  std::vector<void *> desc_chunks, desc_free;
  // dvo_amd_debug_ingest_timing: two events around a build's work on the prep stream (off unless asked for)
  std::atomic<bool> timing{false};
  hipEvent_t ev[2] = {nullptr, nullptr};
  double last_ms = 0.0;
  // pyramid_build_batch: the frame table and the counters of the call in flight (grown to the largest call and kept; used with
  // `mu` held from the table's upload to the last thing enqueued that touches it), and what the most recent call enqueued
  void *batch_area = nullptr;
  size_t batch_bytes = 0;
  int batch_launches = 0, batch_copies = 0, batch_syncs = 0;
};
DeviceState g_dev[kMaxDevices];

int device_prep_stream(int device, hipStream_t *s) {
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  if (!d.prep_stream) HIP_TRY(hipStreamCreateWithFlags(&d.prep_stream, hipStreamNonBlocking));
  *s = d.prep_stream;
  return DVO_AMD_OK;
}

std::mutex &device_mutex(int device) { return g_dev[device].mu; }

int ingest_timing(int device, int enable, double *last_ms) {
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  if (enable && !d.ev[0]) {
    HIP_TRY(hipSetDevice(device));
    for (hipEvent_t &e : d.ev) HIP_TRY(hipEventCreate(&e));
  }
  d.timing = enable != 0;
  if (last_ms) *last_ms = d.last_ms;
  return DVO_AMD_OK;
}

int slab_alloc(int device, size_t bytes, void **out) {
  DeviceState &d = g_dev[device];
  {
    std::lock_guard<std::mutex> lk(d.mu);
    for (size_t i = 0; i < d.free_slabs.size(); ++i)
      if (d.free_slabs[i].first == bytes) {
        *out = d.free_slabs[i].second;
        d.free_slabs.erase(d.free_slabs.begin() + (long)i);
        return DVO_AMD_OK;
      }
  }
  HIP_TRY(hipMalloc(out, bytes));
  return DVO_AMD_OK;
}

int desc_alloc(int device, void **out) {
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.desc_free.empty()) {
    void *chunk = nullptr;
    HIP_TRY(hipMalloc(&chunk, kDescEntryBytes * kDescChunkEntries));
    d.desc_chunks.push_back(chunk);
    for (size_t i = kDescChunkEntries; i-- > 0;) d.desc_free.push_back((char *)chunk + i * kDescEntryBytes);
  }
  *out = d.desc_free.back();
  d.desc_free.pop_back();
  return DVO_AMD_OK;
}

void desc_free(int device, void *p) {
  if (!p) return;
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  d.desc_free.push_back(p);
}

void slab_free(int device, size_t bytes, void *p) {
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.free_slabs.size() < 64) {
    d.free_slabs.emplace_back(bytes, p);
  } else {
    (void)hipFree(p);
  }
}


size_t pyramid_layout(dvo_amd_pyramid *p, char *base) {
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    char *ptr = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return ptr;
  };
  for (int l = 0; l < p->n_levels; ++l) {
    LevelData &L = p->lv[l];
    L.i_plane = (float *)carve(sizeof(float) * L.n);
    L.z_plane = (float *)carve(sizeof(float) * L.n);
    L.c_a = (float4 *)carve(sizeof(float4) * L.n);
    L.c_b = (float2 *)carve(sizeof(float2) * L.n);
    L.r_i = (float *)carve(sizeof(float) * L.n_pad);
    L.r_ix = (float *)carve(sizeof(float) * L.n_pad);
    L.r_iy = (float *)carve(sizeof(float) * L.n_pad);
    L.zsel0 = (float *)carve(sizeof(float) * L.n_pad);
    L.pts0 = carve(kCompactBytesPerPoint * L.n_pad);
    L.tx = (float *)carve(sizeof(float) * L.w);
    L.ty = (float *)carve(sizeof(float) * L.h);
  }
  p->counters = (int *)carve(sizeof(int) * 2 * DVO_AMD_MAX_LEVELS);
  p->sel_partials = (int2 *)carve(sizeof(int2) * (size_t)(p->lv[0].n_pad / 256 + 1));
  p->sel_prefix = (int *)carve(sizeof(int) * (size_t)(p->lv[0].n_pad / 256 + 1));
  static_assert(sizeof(CurLevelDesc) * DVO_AMD_MAX_LEVELS <= kRefDesc0Offset &&
                    kRefDesc0Offset + sizeof(RefLevelDesc) * DVO_AMD_MAX_LEVELS <= kDescEntryBytes,
                "a pyramid's level descriptors fit one arena entry");
  return off;
}

// a pyramid's geometry, its slab and its descriptor entry, from the device's pools; nothing is enqueued
static int pyramid_alloc(int device, const PyramidSpec &spec, dvo_amd_pyramid **out) {
  const int levels = spec.levels;
  dvo_amd_pyramid *p = new dvo_amd_pyramid();
  p->device = device;
  p->n_levels = levels;
  p->timestamp = spec.timestamp;
  for (int l = 0; l < levels; ++l) {
    LevelData &L = p->lv[l];
    if (l == 0) {
      L.w = spec.width, L.h = spec.height, L.fx = spec.fx, L.fy = spec.fy, L.ox = spec.ox, L.oy = spec.oy;
    } else {
      // RgbdCameraPyramid::build (rgbd_image.cpp:283-296) with IntrinsicMatrix::scale(0.5f) (intrinsic_matrix.cpp:90-93)
      const LevelData &P = p->lv[l - 1];
      L.w = P.w / 2, L.h = P.h / 2;
      L.fx = P.fx * 0.5f, L.fy = P.fy * 0.5f, L.ox = P.ox * 0.5f, L.oy = P.oy * 0.5f;
    }
    L.n = L.w * L.h;
    L.n_pad = (int)align_up((size_t)L.n, kPlanePad);
  }
  p->slab_bytes = pyramid_layout(p, nullptr);
  int rc = slab_alloc(device, p->slab_bytes, &p->slab);
  if (rc) {
    delete p;
    return rc;
  }
  pyramid_layout(p, (char *)p->slab);
  rc = desc_alloc(device, &p->desc_entry);
  if (rc) {
    slab_free(device, p->slab_bytes, p->slab);
    delete p;
    return rc;
  }
  p->cur_desc = (CurLevelDesc *)p->desc_entry;
  p->ref_desc0 = (RefLevelDesc *)((char *)p->desc_entry + kRefDesc0Offset);
  *out = p;
  return DVO_AMD_OK;
}

// a pyramid nobody has seen yet back to the pools (the stream is drained: nothing is on its way into the slab any more)
static void pyramid_discard(dvo_amd_pyramid *p) {
  slab_free(p->device, p->slab_bytes, p->slab);
  desc_free(p->device, p->desc_entry);
  delete p;
}

// the current side's level descriptors as the host fills them
static void cur_level_descs(const dvo_amd_pyramid *p, CurLevelDesc *cur_host) {
  std::memset(cur_host, 0, sizeof(CurLevelDesc) * DVO_AMD_MAX_LEVELS);
  for (int l = 0; l < p->n_levels; ++l) {
    const LevelData &C = p->lv[l];
    CurLevelDesc &d = cur_host[l];
    d.c_a = C.c_a, d.c_b = C.c_b, d.w = C.w, d.h = C.h;
    // wcur / wref, dense_tracking.cpp:215-220
    const float wcur_id = 0.5f, wref_id = 0.5f, wcur_zd = 1.0f;
    d.wc[0] = 1.0f / 255.0f, d.wc[1] = 1.0f;
    d.wc[2] = wcur_id * C.fx / 255.0f, d.wc[3] = wcur_id * C.fy / 255.0f;
    d.wc[4] = wcur_zd * C.fx, d.wc[5] = wcur_zd * C.fy;
    d.wr[0] = -1.0f / 255.0f, d.wr[1] = -1.0f;
    d.wr[2] = wref_id * C.fx / 255.0f, d.wr[3] = wref_id * C.fy / 255.0f;
    d.ub_x = (float)(size_t)(C.w - 2), d.ub_y = (float)(size_t)(C.h - 2);
  }
}

// the arguments are the entries' business (dvo_ingest.cpp): nothing is checked again here
int pyramid_build(int device, const PyramidSpec &spec, const Level0Source &src, dvo_amd_pyramid **out) {
  *out = nullptr;
  const int levels = spec.levels;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st;
  int rc = device_prep_stream(device, &st);
  if (rc) return rc;
  dvo_amd_pyramid *p = nullptr;
  rc = pyramid_alloc(device, spec, &p);
  if (rc) return rc;

  // everything below is enqueued on the device's prep stream, and whatever fails, the stream is drained before the slab goes
  // back to the pool: a copy or a launch may still be on its way into it
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(st);
    pyramid_discard(p);
    return code;
  };
  hipError_t e;
  DeviceState &dev = g_dev[device];
  const bool timed = dev.timing.load();
  if (timed && (e = hipEventRecord(dev.ev[0], st)) != hipSuccess) return bail(fail_hip("ingest timing", e));
  // (a registration's four counters live in the room of the first selection's descriptors, which nothing writes before this
  // build returns)
  rc = ingest_level0(device, spec, src, p->lv[0], (unsigned long long *)p->ref_desc0, st);
  if (rc) return bail(rc);
  for (int l = 0; l < levels; ++l) {
    LevelData &L = p->lv[l];
    if (l > 0) {
      const LevelData &P = p->lv[l - 1];
      e = launch_pyr_down(P.i_plane, P.z_plane, P.w, L.i_plane, L.z_plane, L.w, L.h, st);
      if (e != hipSuccess) return bail(fail_hip("pyr_down", e));
    }
    e = launch_level_planes(L.i_plane, L.z_plane, L.w, L.h, L.n_pad, L.fx, L.fy, L.ox, L.oy, L.c_a, L.c_b, L.r_i, L.r_ix,
                            L.r_iy, L.tx, L.ty, L.h, st);
    if (e != hipSuccess) return bail(fail_hip("level_planes", e));
  }
  CurLevelDesc cur_host[DVO_AMD_MAX_LEVELS];
  cur_level_descs(p, cur_host);
  e = hipMemcpyAsync(p->cur_desc, cur_host, sizeof(CurLevelDesc) * levels, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return bail(fail_hip("pyramid descriptors", e));
  if (src.raw && src.raw->reg) {
    e = hipMemcpyAsync(src.raw->reg->counts, p->ref_desc0, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return bail(fail_hip("registration counters", e));
  }
  if (timed && (e = hipEventRecord(dev.ev[1], st)) != hipSuccess) return bail(fail_hip("ingest timing", e));
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return bail(fail_hip("pyramid build", e));
  if (timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]) == hipSuccess) dev.last_ms = ms;
  }
  *out = p;
  return DVO_AMD_OK;
}

static CompactLevel compact_at(char *base, int n_pad) {
  CompactLevel c;
  float *f = (float *)base;
  c.z = f, c.i = f + n_pad, c.ix = f + 2 * (size_t)n_pad, c.iy = f + 3 * (size_t)n_pad, c.tx = f + 4 * (size_t)n_pad,
  c.ty = f + 5 * (size_t)n_pad, c.pix = (int *)(f + 6 * (size_t)n_pad);
  return c;
}

// a pyramid's first selection lives in the pyramid's own slab and descriptor entry
static void selection_in_slab(dvo_amd_pyramid *p, Selection &s) {
  for (int l = 0; l < p->n_levels; ++l) s.zsel[l] = p->lv[l].zsel0, s.pts[l] = compact_at(p->lv[l].pts0, p->lv[l].n_pad);
  s.ref_desc = p->ref_desc0;
}

// the reference side's level descriptors of a selection as the host fills them
static void ref_level_descs(const dvo_amd_pyramid *p, const Selection &s, RefLevelDesc *ref_host) {
  std::memset(ref_host, 0, sizeof(RefLevelDesc) * DVO_AMD_MAX_LEVELS);
  for (int l = 0; l < p->n_levels; ++l) {
    ref_host[l].r_zsel = s.pts[l].z;
    ref_host[l].r_i = s.pts[l].i, ref_host[l].r_ix = s.pts[l].ix, ref_host[l].r_iy = s.pts[l].iy;
    ref_host[l].tx = s.pts[l].tx, ref_host[l].ty = s.pts[l].ty;
  }
}

// PointSelection::select for every level, cached per threshold pair (the reference caches per PointSelection object until
// setRgbdImagePyramid, point_selection.cpp:51-59,100; pyramids are immutable here, so the cache never goes stale)
// A selection mask (dvo_mask.cpp) is the third part of the key, by its serial (0: no mask): a released mask's address may come
// back, its serial never does.  The selection holds planes, not the mask: once built it stays valid for the life of the pyramid
// whatever becomes of the mask.  At most DVO_AMD_MAX_MASKED_SELECTIONS masked selections per pyramid; unmasked ones are not counted.
int mask_fits(const char *entry, const dvo_amd_pyramid *p, const dvo_amd_mask *mask) {
  if (!mask) return DVO_AMD_OK;
  if (mask->w != p->lv[0].w || mask->h != p->lv[0].h)
    return invalid(entry, "the mask is " + std::to_string(mask->w) + "x" + std::to_string(mask->h) + " but the pyramid is " +
                              std::to_string(p->lv[0].w) + "x" + std::to_string(p->lv[0].h));
  if (mask->levels < p->n_levels)
    return invalid(entry, "the mask has " + std::to_string(mask->levels) + " levels but the pyramid has " + std::to_string(p->n_levels));
  if (mask->device != p->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  return DVO_AMD_OK;
}

int pyramid_selection(dvo_amd_pyramid *p, float ti, float td, const dvo_amd_mask *mask, const Selection **out) {
  int rc = mask_fits("point selection", p, mask);
  if (rc) return rc;
  const unsigned long long serial = mask ? mask->serial : 0ull;
  std::lock_guard<std::mutex> lk(p->mu);
  int masked = 0;
  for (size_t i = 0; i < p->selections.size(); ++i) {
    if (p->selections[i]->ti == ti && p->selections[i]->td == td && p->selections[i]->mask_serial == serial) {
      *out = p->selections[i].get();
      return DVO_AMD_OK;
    }
    if (p->selections[i]->mask_serial) ++masked;
  }
  if (mask && masked >= DVO_AMD_MAX_MASKED_SELECTIONS) {
    g_last_error = "point selection: the pyramid already caches " + std::to_string(DVO_AMD_MAX_MASKED_SELECTIONS) + " masked selections";
    return DVO_AMD_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st;
  rc = device_prep_stream(p->device, &st);
  if (rc) return rc;
  std::unique_ptr<Selection> sp(new Selection());
  Selection &s = *sp;
  s.ti = ti, s.td = td, s.mask_serial = serial, s.extra_slab = nullptr, s.extra_bytes = 0;
  if (p->selections.empty()) {
    selection_in_slab(p, s);
  } else {
    size_t bytes = 0;
    for (int l = 0; l < p->n_levels; ++l) bytes += align_up((sizeof(float) + kCompactBytesPerPoint) * p->lv[l].n_pad, 256);
    rc = desc_alloc(p->device, &s.desc_entry);
    if (rc) return rc;
    const hipError_t em = hipMalloc(&s.extra_slab, bytes);
    if (em != hipSuccess) {
      desc_free(p->device, s.desc_entry);
      return fail_hip("selection planes", em);
    }
    s.extra_bytes = bytes;
    s.ref_desc = (RefLevelDesc *)s.desc_entry;
    size_t off = 0;
    for (int l = 0; l < p->n_levels; ++l) {
      s.zsel[l] = (float *)((char *)s.extra_slab + off);
      s.pts[l] = compact_at((char *)s.extra_slab + off + sizeof(float) * p->lv[l].n_pad, p->lv[l].n_pad);
      off += align_up((sizeof(float) + kCompactBytesPerPoint) * p->lv[l].n_pad, 256);
    }
  }
  // any failure below must not leak the selection's own allocation
  auto fail = [&](const char *what, hipError_t e) {
    (void)hipStreamSynchronize(st);
    if (s.extra_slab) (void)hipFree(s.extra_slab);
    desc_free(p->device, s.desc_entry);
    return fail_hip(what, e);
  };
  RefLevelDesc ref_host[DVO_AMD_MAX_LEVELS];
  ref_level_descs(p, s, ref_host);
  // (dvo_amd_debug_ingest_timing brackets a selection's build like a pyramid's: that a cached selection costs nothing shows there)
  DeviceState &dev = g_dev[p->device];
  const bool timed = dev.timing.load();
  hipError_t e = timed ? hipEventRecord(dev.ev[0], st) : hipSuccess;
  if (e != hipSuccess) return fail("ingest timing", e);
  e = hipMemcpyAsync(s.ref_desc, ref_host, sizeof(RefLevelDesc) * p->n_levels, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail("selection descriptors", e);
  for (int l = 0; l < p->n_levels; ++l) {
    const LevelData &L = p->lv[l];
    // (a pair without a mask takes the path it always took: the unmasked kernel, the same launches)
    e = mask ? launch_select_masked(L.z_plane, L.c_a, L.c_b, mask->plane[l], L.n, L.n_pad, ti, td, s.zsel[l], p->counters + 2 * l,
                                    p->sel_partials, st)
             : launch_select(L.z_plane, L.c_a, L.c_b, L.n, L.n_pad, ti, td, s.zsel[l], p->counters + 2 * l, p->sel_partials, st);
    if (e != hipSuccess) return fail("select", e);
    // (the partials and the prefix are scratch of the pyramid shared by its levels: the prep stream runs them in order)
    e = launch_compact(s.zsel[l], L.r_i, L.r_ix, L.r_iy, L.tx, L.ty, L.w, L.n, L.n_pad, p->sel_partials, p->sel_prefix, p->counters + 2 * l,
                       s.pts[l].z, s.pts[l].i, s.pts[l].ix, s.pts[l].iy, s.pts[l].tx, s.pts[l].ty, s.pts[l].pix, st);
    if (e != hipSuccess) return fail("compact", e);
  }
  int host_counters[2 * DVO_AMD_MAX_LEVELS];
  e = hipMemcpyAsync(host_counters, p->counters, sizeof(int) * 2 * p->n_levels, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return fail("selection counters", e);
  if (timed && (e = hipEventRecord(dev.ev[1], st)) != hipSuccess) return fail("ingest timing", e);
  e = hipStreamSynchronize(st);  // (also keeps ref_host alive until the copy has read it)
  if (e != hipSuccess) return fail("selection", e);
  if (timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]) == hipSuccess) dev.last_ms = ms;
  }
  for (int l = 0; l < p->n_levels; ++l) s.count[l] = host_counters[2 * l], s.n_pts[l] = s.count[l] & ~1, s.last[l] = host_counters[2 * l + 1];
  p->selections.push_back(std::move(sp));
  *out = p->selections.back().get();
  return DVO_AMD_OK;
}


// ---- N pyramids in one call (dvo_amd_pyramid_create_raw_batch) --------------------------------------------------------------
// What pyramid_build and the first pyramid_selection enqueue for one frame -- a dozen dependent launches for the pyramid, four per
// level for the selection, three small copies and two synchronisations -- is enqueued once for all N frames of the call: one
// launch per stage and level with the frame as the grid's y dimension (dvo_kernels.hip, "N frames per launch"), one upload of the
// frame table, one copy of every frame's counters back, one synchronisation.  All slabs of a call have one layout, so the kernels
// take a level as offsets from a slab's base (BatchLevel) and a frame as a row of the table (BatchFrame).

static BatchLevel batch_level(const dvo_amd_pyramid *p, int l) {
  const LevelData &L = p->lv[l];
  const char *base = (const char *)p->slab;
  auto off = [&](const void *q) { return (size_t)((const char *)q - base); };
  BatchLevel B;
  B.i_plane = off(L.i_plane), B.z_plane = off(L.z_plane), B.c_a = off(L.c_a), B.c_b = off(L.c_b);
  B.r_i = off(L.r_i), B.r_ix = off(L.r_ix), B.r_iy = off(L.r_iy), B.tx = off(L.tx), B.ty = off(L.ty);
  const CompactLevel c = compact_at(L.pts0, L.n_pad);
  B.zsel = off(L.zsel0);
  B.pts[0] = off(c.z), B.pts[1] = off(c.i), B.pts[2] = off(c.ix), B.pts[3] = off(c.iy), B.pts[4] = off(c.tx), B.pts[5] = off(c.ty),
  B.pts[6] = off(c.pix);
  B.counters = off(p->counters + 2 * l), B.partials = off(p->sel_partials), B.prefix = off(p->sel_prefix);
  B.w = L.w, B.h = L.h, B.n = L.n, B.n_pad = L.n_pad;
  B.fx = L.fx, B.fy = L.fy, B.ox = L.ox, B.oy = L.oy;
  return B;
}

template <typename T>
static void rebase(const T *&q, const char *base) {
  q = (const T *)((const char *)q - base);
}

// the level descriptors of pyramid `p` with every pointer as its distance from the slab's base: the same for every frame of a call
static void batch_descs(dvo_amd_pyramid *p, bool with_ref, BatchDescs &D) {
  static_assert(kBatchMaxLevels == DVO_AMD_MAX_LEVELS, "BatchDescs holds a pyramid's levels");
  const char *base = (const char *)p->slab;
  cur_level_descs(p, D.cur);
  Selection s;
  selection_in_slab(p, s);
  ref_level_descs(p, s, D.ref);
  for (int l = 0; l < p->n_levels; ++l) {
    rebase(D.cur[l].c_a, base), rebase(D.cur[l].c_b, base);
    RefLevelDesc &r = D.ref[l];
    rebase(r.r_zsel, base), rebase(r.r_i, base), rebase(r.r_ix, base), rebase(r.r_iy, base), rebase(r.tx, base), rebase(r.ty, base);
  }
  D.levels = p->n_levels, D.with_ref = with_ref ? 1 : 0, D.ref_offset = (unsigned)kRefDesc0Offset;
}

// the arguments are the entry's business (dvo_ingest.cpp): nothing is checked again here.  out: b.count entries, all NULL on entry
// and again after any failure
int pyramid_build_batch(int device, const dvo_amd_raw_batch &b, dvo_amd_pyramid **out) {
  const int count = b.count, levels = b.levels;
  const bool with_sel = b.build_selection != 0;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st;
  int rc = device_prep_stream(device, &st);
  if (rc) return rc;
  DeviceState &dev = g_dev[device];
  std::vector<dvo_amd_pyramid *> pyr;
  pyr.reserve((size_t)count);
  // Whatever fails, at whichever frame: the stream is drained -- a copy or a launch may still be on its way into a slab --, every
  // slab and descriptor entry taken so far goes back to its pool, and the caller's array stays all NULL
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(st);
    for (dvo_amd_pyramid *p : pyr) pyramid_discard(p);
    return code;
  };
  for (int f = 0; f < count; ++f) {
    dvo_amd_pyramid *p = nullptr;
    rc = pyramid_alloc(device, PyramidSpec{b.width, b.height, b.fx, b.fy, b.ox, b.oy, levels, b.timestamps ? b.timestamps[f] : 0.0}, &p);
    if (rc) return bail(rc);
    pyr.push_back(p);
  }
  int launches = 0, copies = 0;
  hipError_t e;
  const bool timed = dev.timing.load();
  if (timed && (e = hipEventRecord(dev.ev[0], st)) != hipSuccess) return bail(fail_hip("ingest timing", e));
  // A host frame's bytes are staged where pyramid_build stages them: in the frame's own level-0 gather plane, which only
  // launch_level_planes_batch writes, further down the same stream.  No lock: the room is the pyramid's own.
  const size_t n0 = (size_t)pyr[0]->lv[0].n;
  const size_t row_img = (size_t)b.width * b.channels, row_z = sizeof(unsigned short) * (size_t)b.width;
  const size_t z_room = align_up(n0 * b.channels, 256);
  std::vector<BatchFrame> table((size_t)count);
  for (int f = 0; f < count; ++f) {
    BatchFrame &F = table[(size_t)f];
    F.slab = (char *)pyr[f]->slab, F.desc = (char *)pyr[f]->desc_entry, F.img = b.images[f], F.z = b.depths[f];
    if (b.on_device) continue;
    char *room = (char *)pyr[f]->lv[0].c_a;
    e = hipMemcpy2DAsync(room, row_img, b.images[f], (size_t)b.image_stride_bytes, row_img, (size_t)b.height, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(room + z_room, row_z, b.depths[f], sizeof(unsigned short) * (size_t)b.depth_stride, row_z, (size_t)b.height,
                           hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return bail(fail_hip("raw frame upload", e));
    copies += 2;
    F.img = (const unsigned char *)room, F.z = (const unsigned short *)(room + z_room);
  }
  const int img_stride = b.on_device ? b.image_stride_bytes : (int)row_img, z_stride = b.on_device ? b.depth_stride : b.width;
  BatchLevel lv[DVO_AMD_MAX_LEVELS];
  for (int l = 0; l < levels; ++l) lv[l] = batch_level(pyr[0], l);
  BatchDescs descs;
  batch_descs(pyr[0], with_sel, descs);
  const size_t table_bytes = align_up(sizeof(BatchFrame) * (size_t)count, 256);
  const size_t counter_ints = 2 * (size_t)levels * (size_t)count;
  std::vector<int> host_counters(with_sel ? counter_ints : 0);
  // (a failure inside leaves the mutex before the unwind below takes it again for the pools)
  rc = [&]() -> int {
    // The table and the counters live in the device's one batch area, which the next call overwrites: the device's mutex is held
    // from the upload to the last thing enqueued that reads or writes the area, so that two threads' calls reach the stream one
    // after the other (ingest_raw does the same for its staging area).  The pools above took and released the mutex on their own.
    std::lock_guard<std::mutex> lk(dev.mu);
    const size_t need = table_bytes + sizeof(int) * counter_ints;
    if (need > dev.batch_bytes) {
      if (dev.batch_area) (void)hipFree(dev.batch_area), dev.batch_area = nullptr, dev.batch_bytes = 0;  // (waits for its readers)
      const size_t grown = align_up(need, 1 << 16);
      e = hipMalloc(&dev.batch_area, grown);
      if (e == hipErrorOutOfMemory) return DVO_AMD_ERR_OUT_OF_MEMORY;
      if (e != hipSuccess) return fail_hip("hipMalloc (batch table)", e);
      dev.batch_bytes = grown;
    }
    const BatchFrame *frames = (const BatchFrame *)dev.batch_area;
    int *all_counters = (int *)((char *)dev.batch_area + table_bytes);
    e = hipMemcpyAsync(dev.batch_area, table.data(), sizeof(BatchFrame) * (size_t)count, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail_hip("batch table", e);
    copies += 1;
    e = launch_ingest_batch(frames, count, b.channels, img_stride, z_stride, b.depth_scale, lv[0], st, &launches);
    if (e != hipSuccess) return fail_hip("k_ingest_batch", e);
    for (int l = 0; l < levels; ++l) {
      if (l > 0 && (e = launch_pyr_down_batch(frames, count, lv[l - 1], lv[l], st, &launches)) != hipSuccess)
        return fail_hip("pyr_down_batch", e);
      e = launch_level_planes_batch(frames, count, lv[l], st, &launches);
      if (e != hipSuccess) return fail_hip("level_planes_batch", e);
    }
    e = launch_batch_descs(frames, count, descs, st, &launches);
    if (e != hipSuccess) return fail_hip("batch descriptors", e);
    if (with_sel) {
      for (int l = 0; l < levels; ++l) {
        e = launch_select_batch(frames, count, lv[l], b.intensity_threshold, b.depth_threshold, all_counters, l, levels, st, &launches);
        if (e != hipSuccess) return fail_hip("select_batch", e);
        // (the partials and the prefix are scratch of each pyramid shared by its levels: the prep stream runs them in order)
        e = launch_compact_batch(frames, count, lv[l], st, &launches);
        if (e != hipSuccess) return fail_hip("compact_batch", e);
      }
      e = hipMemcpyAsync(host_counters.data(), all_counters, sizeof(int) * counter_ints, hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) return fail_hip("selection counters", e);
      copies += 1;
    }
    if (timed && (e = hipEventRecord(dev.ev[1], st)) != hipSuccess) return fail_hip("ingest timing", e);
    return DVO_AMD_OK;
  }();
  if (rc) return bail(rc);
  e = hipStreamSynchronize(st);  // the call's one synchronisation (also keeps `table` alive until the copy has read it)
  if (e != hipSuccess) return bail(fail_hip("batched pyramid build", e));
  if (with_sel)
    for (int f = 0; f < count; ++f) {
      std::unique_ptr<Selection> sp(new Selection());
      Selection &s = *sp;
      s.ti = b.intensity_threshold, s.td = b.depth_threshold, s.extra_slab = nullptr, s.extra_bytes = 0;
      selection_in_slab(pyr[f], s);
      const int *c = host_counters.data() + 2 * (size_t)levels * (size_t)f;
      for (int l = 0; l < levels; ++l) s.count[l] = c[2 * l], s.n_pts[l] = s.count[l] & ~1, s.last[l] = c[2 * l + 1];
      pyr[f]->selections.push_back(std::move(sp));
    }
  {
    std::lock_guard<std::mutex> lk(dev.mu);
    float ms = 0.f;
    if (timed && hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]) == hipSuccess) dev.last_ms = ms;
    dev.batch_launches = launches, dev.batch_copies = copies, dev.batch_syncs = 1;
  }
  for (int f = 0; f < count; ++f) out[f] = pyr[f];
  return DVO_AMD_OK;
}

int batch_build_stats(int device, int *kernel_launches, int *copies, int *synchronisations) {
  DeviceState &d = g_dev[device];
  std::lock_guard<std::mutex> lk(d.mu);
  if (kernel_launches) *kernel_launches = d.batch_launches;
  if (copies) *copies = d.batch_copies;
  if (synchronisations) *synchronisations = d.batch_syncs;
  return DVO_AMD_OK;
}

}  // namespace host
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;

extern "C" {

void dvo_amd_pyramid_retain(dvo_amd_pyramid *p) {
  if (p) p->refs.fetch_add(1);
}

void dvo_amd_pyramid_release(dvo_amd_pyramid *p) {
  if (!p) return;
  if (p->refs.fetch_sub(1) != 1) return;
  (void)hipSetDevice(p->device);
  for (auto &s : p->selections) {
    if (s->extra_slab) (void)hipFree(s->extra_slab);
    desc_free(p->device, s->desc_entry);
  }
  desc_free(p->device, p->desc_entry);
  slab_free(p->device, p->slab_bytes, p->slab);
  delete p;
}

int dvo_amd_pyramid_levels(const dvo_amd_pyramid *p) { return p ? p->n_levels : 0; }
double dvo_amd_pyramid_timestamp(const dvo_amd_pyramid *p) { return p ? p->timestamp : 0.0; }

int dvo_amd_pyramid_level_info(const dvo_amd_pyramid *p, int level, int *width, int *height, float k[4]) {
  if (!p || level < 0 || level >= p->n_levels) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const LevelData &L = p->lv[level];
  if (width) *width = L.w;
  if (height) *height = L.h;
  if (k) k[0] = L.fx, k[1] = L.fy, k[2] = L.ox, k[3] = L.oy;
  return DVO_AMD_OK;
}

int dvo_amd_pyramid_download_plane(const dvo_amd_pyramid *p, int level, int plane, float *dst) {
  if (!p || !dst || level < 0 || level >= p->n_levels || plane < 0 || plane > 5) return DVO_AMD_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st;
  int rc = device_prep_stream(p->device, &st);
  if (rc) return rc;
  const LevelData &L = p->lv[level];
  float *tmp = nullptr;
  HIP_TRY(hipMalloc((void **)&tmp, sizeof(float) * L.n));
  hipError_t e = launch_unpack_plane(L.c_a, L.c_b, plane, L.n, tmp, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dst, tmp, sizeof(float) * L.n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail_hip("download_plane", e);
  return DVO_AMD_OK;
}

// dvo_amd_pyramid_select and dvo_amd_pyramid_select_masked (sel_mask == nullptr: the former)
static int select_entry(dvo_amd_pyramid *p, int level, float ti, float td, const dvo_amd_mask *sel_mask, int *count, unsigned char *mask) {
  if (!p || level < 0 || level >= p->n_levels) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const Selection *sp = nullptr;
  int rc = pyramid_selection(p, ti, td, sel_mask, &sp);
  if (rc) return rc;
  const Selection &s = *sp;
  if (count) *count = s.count[level];
  if (mask) {
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st;
    rc = device_prep_stream(p->device, &st);
    if (rc) return rc;
    const LevelData &L = p->lv[level];
    unsigned char *tmp = nullptr;
    HIP_TRY(hipMalloc((void **)&tmp, L.n));
    const int dropped = (s.count[level] & 1) ? s.last[level] : -1;
    hipError_t e = launch_mask_from_zsel(s.zsel[level], L.n, dropped, tmp, st);
    if (e == hipSuccess) e = hipMemcpyAsync(mask, tmp, L.n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail_hip("select mask", e);
  }
  return DVO_AMD_OK;
}

int dvo_amd_pyramid_select(dvo_amd_pyramid *p, int level, float ti, float td, int *count, unsigned char *mask) {
  return select_entry(p, level, ti, td, nullptr, count, mask);
}

int dvo_amd_pyramid_select_masked(dvo_amd_pyramid *p, int level, float ti, float td, const dvo_amd_mask *mask, int *count,
                                  unsigned char *out_mask) {
  return select_entry(p, level, ti, td, mask, count, out_mask);
}

}  // extern "C"
