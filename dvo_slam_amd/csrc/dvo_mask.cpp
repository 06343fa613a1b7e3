// Selection masks: which reference pixels may take part in an alignment, as a device-resident, immutable, refcounted pyramid of
// byte planes (1 = keep, 0 = drop), one per pyramid level.  The reference lets a caller decide this with any
// PointSelectionPredicate (point_selection.h:32-37: isPointOk sees the pixel's position, so a predicate can cut out a region or
// follow a segmentation); here the decision arrives as a mask and enters in exactly one place, the select kernel
// (k_select_masked, dvo_kernels.hip) -- everything behind the selection walks the selected pixels only and stays what it is.
//   level 0       given by the caller, in host or in device memory (a segmentation network's output), any non-zero byte = keep
//   levels 1..    derived on the device, ALL or ANY of the four pixels under a pixel (k_mask_down), or given level by level
// A mask carries a process-wide serial number, never 0 and never reused: its identity in a pyramid's selection cache
// (pyramid_selection, dvo_pyramid.cpp).  The rules are pinned in include/dvo_amd.h.
#include "dvo_internal.h"

#include <atomic>
#include <string>

namespace dvo_amd {
namespace host {

namespace {

std::atomic<unsigned long long> g_mask_serial{0};

}  // namespace

// the geometry a mask may have: a pyramid's (check_levels), within what one launch's grid holds
int check_mask_size(const char *entry, int width, int height, int levels) {
  const int rc = check_levels(entry, width, height, levels, " of the mask");
  if (rc) return rc;
  if (height > 65535 || (long long)width * height > (1ll << 30)) return invalid(entry, "the mask is larger than 2^30 pixels or 65535 rows");
  return DVO_AMD_OK;
}

// the mask object with its planes allocated and its counters cleared (on the prep stream); the caller fills the planes
int mask_alloc(const char *entry, int device, int width, int height, int levels, dvo_amd_mask **out, hipStream_t *st) {
  int ndev = 0;
  int rc = have_device(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(entry, "no such device");
  HIP_TRY(hipSetDevice(device));
  rc = device_prep_stream(device, st);
  if (rc) return rc;
  size_t bytes = 0;
  for (int l = 0; l < levels; ++l) bytes += align_up((size_t)(width >> l) * (size_t)(height >> l), 256);
  void *mem = nullptr;
  const hipError_t e = hipMalloc(&mem, bytes + 256);
  if (e == hipErrorOutOfMemory) return DVO_AMD_ERR_OUT_OF_MEMORY;
  if (e != hipSuccess) return fail_hip("hipMalloc (mask)", e);
  dvo_amd_mask *m = new dvo_amd_mask();
  m->device = device, m->w = width, m->h = height, m->levels = levels, m->mem = mem;
  m->serial = g_mask_serial.fetch_add(1) + 1;
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    m->plane[l] = (unsigned char *)mem + off;
    off += align_up((size_t)(width >> l) * (size_t)(height >> l), 256);
  }
  m->counters = (int *)((char *)mem + off);
  static_assert(sizeof(int) * DVO_AMD_MAX_LEVELS <= 256, "a mask's counters fit the room behind its planes");
  const hipError_t em = hipMemsetAsync(m->counters, 0, sizeof(int) * levels, *st);
  if (em != hipSuccess) {
    (void)hipFree(mem);
    delete m;
    return fail_hip("mask counters", em);
  }
  *out = m;
  return DVO_AMD_OK;
}

// level l as the caller gave it into the mask's plane, normalised and counted: one launch, wherever the bytes come from (a host
// plane is copied into the mask's own plane first and normalised in place)
hipError_t mask_level_in(dvo_amd_mask *m, int l, const unsigned char *src, int stride, bool on_device, hipStream_t st) {
  const int w = m->w >> l, h = m->h >> l;
  if (!on_device) {
    const hipError_t e = hipMemcpy2DAsync(m->plane[l], (size_t)w, src, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    src = m->plane[l], stride = w;
  }
  return launch_mask_plane(src, stride, m->plane[l], w, h, m->counters + l, st);
}

// the kept counts to the host and the stream drained; on failure the mask is gone
int mask_finish(dvo_amd_mask *m, hipError_t e, hipStream_t st, dvo_amd_mask **out) {
  int kept[DVO_AMD_MAX_LEVELS] = {};
  if (e == hipSuccess) e = hipMemcpyAsync(kept, m->counters, sizeof(int) * m->levels, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(m->mem);
    delete m;
    return fail_hip("mask build", e);
  }
  for (int l = 0; l < m->levels; ++l) m->kept[l] = kept[l];
  *out = m;
  return DVO_AMD_OK;
}

}  // namespace host
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;

extern "C" {

int dvo_amd_mask_create(int device, int width, int height, int levels, const unsigned char *mask0, int stride, int on_device, int rule,
                        dvo_amd_mask **out) {
  static const char *entry = "dvo_amd_mask_create";
  if (out) *out = nullptr;
  if (!out || !mask0) return invalid(entry, "a NULL pointer");
  int rc = check_mask_size(entry, width, height, levels);
  if (rc) return rc;
  if (stride < width) return invalid(entry, "stride < width");
  if (rule != DVO_AMD_MASK_ALL && rule != DVO_AMD_MASK_ANY) return invalid(entry, "rule must be DVO_AMD_MASK_ALL or DVO_AMD_MASK_ANY");
  dvo_amd_mask *m = nullptr;
  hipStream_t st;
  rc = mask_alloc(entry, device, width, height, levels, &m, &st);
  if (rc) return rc;
  // one launch per level: the given level, then every derived level from the one above it
  hipError_t e = mask_level_in(m, 0, mask0, stride, on_device != 0, st);
  for (int l = 1; l < levels && e == hipSuccess; ++l)
    e = launch_mask_down(m->plane[l - 1], width >> (l - 1), m->plane[l], width >> l, height >> l, rule == DVO_AMD_MASK_ANY ? 1 : 0,
                         m->counters + l, st);
  return mask_finish(m, e, st, out);
}

int dvo_amd_mask_create_levels(int device, int width, int height, int levels, const unsigned char *const *planes, const int *strides,
                               int on_device, dvo_amd_mask **out) {
  static const char *entry = "dvo_amd_mask_create_levels";
  if (out) *out = nullptr;
  if (!out || !planes || !strides) return invalid(entry, "a NULL pointer");
  int rc = check_mask_size(entry, width, height, levels);
  if (rc) return rc;
  for (int l = 0; l < levels; ++l) {
    if (!planes[l]) return invalid(entry, "planes[" + std::to_string(l) + "] is NULL");
    if (strides[l] < (width >> l)) return invalid(entry, "strides[" + std::to_string(l) + "] < the width of level " + std::to_string(l));
  }
  dvo_amd_mask *m = nullptr;
  hipStream_t st;
  rc = mask_alloc(entry, device, width, height, levels, &m, &st);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  for (int l = 0; l < levels && e == hipSuccess; ++l) e = mask_level_in(m, l, planes[l], strides[l], on_device != 0, st);
  return mask_finish(m, e, st, out);
}

void dvo_amd_mask_retain(dvo_amd_mask *m) {
  if (m) m->refs.fetch_add(1);
}

void dvo_amd_mask_release(dvo_amd_mask *m) {
  if (!m) return;
  if (m->refs.fetch_sub(1) != 1) return;
  (void)hipSetDevice(m->device);
  (void)hipFree(m->mem);
  delete m;
}

int dvo_amd_mask_info(const dvo_amd_mask *m, int *width, int *height, int *levels, long long *kept) {
  if (!m) return invalid("dvo_amd_mask_info", "the mask is NULL");
  if (width) *width = m->w;
  if (height) *height = m->h;
  if (levels) *levels = m->levels;
  if (kept)
    for (int l = 0; l < m->levels; ++l) kept[l] = m->kept[l];
  return DVO_AMD_OK;
}

int dvo_amd_mask_download(const dvo_amd_mask *m, int level, unsigned char *dst) {
  if (!m || !dst) return invalid("dvo_amd_mask_download", "a NULL pointer");
  if (level < 0 || level >= m->levels) return invalid("dvo_amd_mask_download", "no such level");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st;
  const int rc = device_prep_stream(m->device, &st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(dst, m->plane[level], (size_t)(m->w >> level) * (size_t)(m->h >> level), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DVO_AMD_OK;
}

}  // extern "C"
