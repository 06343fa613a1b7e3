// Where level 0 of a pyramid comes from.  Five sources -- float planes in host or device memory, a raw sensor frame as it is,
// resampled through a remap (dvo_rectify.cpp), or with its depth registered from another camera (dvo_register.cpp) -- are one
// description (Level0Source, dvo_internal.h) and go through one driver, ingest_level0, which owns everything that is not a kernel:
// the per-device staging area of host raw frames, the span of the device's mutex over it, and the row upload.  The five
// single-frame dvo_amd_pyramid_create* entries stand side by side below it and check their arguments through the same helpers; so does
// the batched raw entry, whose driver (pyramid_build_batch, dvo_pyramid.cpp) stages its host frames the way ingest_raw does.
#include "dvo_internal.h"

#include <cstring>

namespace dvo_amd {
namespace host {

namespace {

// The per-device staging area of host raw frames and of the grey plane of BGR sources that go through a remap: grown to the
// largest seen and kept; used with the device's mutex held.
struct Staging {
  DeviceBuf img, z, grey;
};
Staging g_stage[kMaxDevices];

int staging_grow(DeviceBuf &a, size_t bytes) { return grow(a, bytes, 1 << 16, "ingest staging"); }

// `rows` rows of `row_bytes` from host memory, `src_stride_bytes` apart, packed into `dst`
hipError_t upload_rows(void *dst, const void *src, size_t row_bytes, size_t src_stride_bytes, int rows, hipStream_t st) {
  return hipMemcpy2DAsync(dst, row_bytes, src, src_stride_bytes, row_bytes, (size_t)rows, hipMemcpyHostToDevice, st);
}

int ingest_planes(const PyramidSpec &spec, const Level0Source &src, const LevelData &L0, hipStream_t st) {
  const int w = spec.width, h = spec.height;
  const float *from[2] = {src.intensity, src.depth};
  float *to[2] = {L0.i_plane, L0.z_plane};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    if (!src.on_device)
      e = upload_rows(to[k], from[k], sizeof(float) * (size_t)w, sizeof(float) * (size_t)src.stride, h, st);
    else if (src.stride == w)
      e = hipMemcpyAsync(to[k], from[k], sizeof(float) * L0.n, hipMemcpyDeviceToDevice, st);
    else
      e = launch_copy_strided(from[k], src.stride, to[k], w, h, st);
  }
  return e == hipSuccess ? DVO_AMD_OK : fail_hip("pyramid upload", e);
}

int ingest_raw(int device, const PyramidSpec &spec, const RawFrame &raw, bool on_device, const LevelData &L0,
               unsigned long long *ctrl, hipStream_t st) {
  const dvo_amd_remap *rm = raw.remap;
  const Registration *reg = raw.reg;
  const int w = spec.width, h = spec.height;
  const int iw = rm ? rm->sw : w, ih = rm ? rm->sh : h;          // the image as it arrives
  const int zw = reg ? reg->dw : iw, zh = reg ? reg->dh : ih;    // ... and the depth frame
  // The plain frame stages its bytes (5 B/px instead of 8 B/px of float planes over PCIe) in level 0's gather plane, which is
  // only written by launch_level_planes further down the same stream, and takes no lock.  The other two read their source at
  // scattered positions, so it has a size of its own: they share the device's staging area, under the device's mutex from here
  // to the last launch that reads the area, so that two threads' uses reach the stream one after the other.
  Staging *shared = rm || reg ? &g_stage[device] : nullptr;
  std::unique_lock<std::mutex> lk;
  if (shared) lk = std::unique_lock<std::mutex>(device_mutex(device));
  const unsigned char *d_img = raw.image;
  const unsigned short *d_z = raw.depth;
  int img_stride = raw.image_stride_bytes, z_stride = raw.depth_stride, rc = DVO_AMD_OK;
  hipError_t e = hipSuccess;
  const size_t row_img = (size_t)iw * raw.channels, row_z = sizeof(unsigned short) * (size_t)zw;
  if (!on_device) {
    void *dst = L0.c_a;
    if (shared && (rc = staging_grow(shared->img, row_img * ih))) return rc;
    if (shared) dst = shared->img.p;
    e = upload_rows(dst, raw.image, row_img, (size_t)raw.image_stride_bytes, ih, st);
    if (e != hipSuccess) return fail_hip("raw frame upload", e);
    d_img = (const unsigned char *)dst, img_stride = (int)row_img;
  }
  auto stage_depth = [&]() -> int {
    if (on_device) return DVO_AMD_OK;
    void *dst = (char *)L0.c_a + align_up((size_t)L0.n * raw.channels, 256);
    if (shared && (rc = staging_grow(shared->z, row_z * zh))) return rc;
    if (shared) dst = shared->z.p;
    e = upload_rows(dst, raw.depth, row_z, sizeof(unsigned short) * (size_t)raw.depth_stride, zh, st);
    if (e != hipSuccess) return fail_hip("raw frame upload", e);
    d_z = (const unsigned short *)dst, z_stride = zw;
    return DVO_AMD_OK;
  };
  if (!reg && (rc = stage_depth())) return rc;  // (a registered frame's depth follows its intensity plane)
  if (rm) {
    const int grey_stride = (int)align_up((size_t)rm->sw, 4);
    if (raw.channels == 3 && (rc = staging_grow(shared->grey, (size_t)grey_stride * rm->sh))) return rc;
    rc = launch_remap_ingest(rm, d_img, raw.channels, img_stride, (unsigned char *)shared->grey.p, grey_stride, d_z, z_stride,
                             raw.depth_scale, L0.i_plane, reg ? nullptr : L0.z_plane, st);
    if (rc) return rc;
  } else {
    e = reg ? launch_ingest_intensity(d_img, raw.channels, img_stride, L0.i_plane, w, h, st)
            : launch_ingest(d_img, raw.channels, img_stride, d_z, z_stride, raw.depth_scale, L0.i_plane, L0.z_plane, w, h, st);
    if (e != hipSuccess) return fail_hip("k_ingest", e);
  }
  if (!reg) return DVO_AMD_OK;
  if ((rc = stage_depth())) return rc;
  return launch_register_depth(*reg, d_z, z_stride, raw.depth_scale, L0.z_plane, spec, ctrl, st);
}

// ---- the argument checks the entries share ----------------------------------------------------------------------------------------

// what every raw entry asks of its frame; the two widths are those of the rows the strides must hold, the two sentences what to say
int check_raw(const char *entry, const RawFrame &raw, int image_width, int depth_width, const char *image_why, const char *depth_why) {
  if (raw.channels != 1 && raw.channels != 3) return invalid(entry, "channels must be 1 or 3");
  if (!(raw.depth_scale > 0.0f)) return invalid(entry, "depth_scale must be > 0");
  if ((long long)raw.image_stride_bytes < (long long)image_width * raw.channels) return invalid(entry, image_why);
  if (raw.depth_stride < depth_width) return invalid(entry, depth_why);
  return DVO_AMD_OK;
}

// after every INVALID_ARGUMENT the arguments alone can earn: is there a device, is it the remap's, does it exist
int check_device(int device, const dvo_amd_remap *remap) {
  int ndev = 0;
  const int rc = have_device(&ndev);
  if (rc) return rc;
  if (remap && remap->device != device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return DVO_AMD_ERR_INVALID_ARGUMENT;
  return DVO_AMD_OK;
}

int create_from_planes(const char *entry, int device, const float *intensity, const float *depth, bool on_device, int stride,
                       const PyramidSpec &spec, dvo_amd_pyramid **out) {
  if (out) *out = nullptr;
  if (!out || !intensity || !depth) return invalid(entry, "a NULL pointer");
  if (stride < spec.width) return invalid(entry, "stride < width");
  int rc = check_levels(entry, spec.width, spec.height, spec.levels);
  if (!rc) rc = check_device(device, nullptr);
  if (rc) return rc;
  return pyramid_build(device, spec, Level0Source{intensity, depth, stride, nullptr, on_device}, out);
}

}  // namespace

int check_levels(const char *entry, int w, int h, int levels, const char *of) {
  if (levels < 1 || levels > DVO_AMD_MAX_LEVELS) return invalid(entry, "levels must be 1.." + std::to_string(DVO_AMD_MAX_LEVELS));
  for (int l = 0; l < levels; ++l, w /= 2, h /= 2)
    if (w < 4 || h < 2 || (w % 4) != 0)
      return invalid(entry, "level " + std::to_string(l) + of + " would not be at least 4x2 with a width that is a multiple of 4");
  return DVO_AMD_OK;
}

int ingest_level0(int device, const PyramidSpec &spec, const Level0Source &src, const LevelData &L0, unsigned long long *ctrl,
                  hipStream_t st) {
  return src.raw ? ingest_raw(device, spec, *src.raw, src.on_device, L0, ctrl, st) : ingest_planes(spec, src, L0, st);
}

}  // namespace host
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;

extern "C" {

int dvo_amd_pyramid_create(int device, const float *intensity, const float *depth, int width, int height, int stride,
                           float fx, float fy, float ox, float oy, int levels, double timestamp, dvo_amd_pyramid **out) {
  return create_from_planes("dvo_amd_pyramid_create", device, intensity, depth, false, stride,
                            PyramidSpec{width, height, fx, fy, ox, oy, levels, timestamp}, out);
}

int dvo_amd_pyramid_create_from_device(int device, const float *d_intensity, const float *d_depth, int width, int height,
                                       int stride, float fx, float fy, float ox, float oy, int levels, double timestamp,
                                       dvo_amd_pyramid **out) {
  return create_from_planes("dvo_amd_pyramid_create_from_device", device, d_intensity, d_depth, true, stride,
                            PyramidSpec{width, height, fx, fy, ox, oy, levels, timestamp}, out);
}

int dvo_amd_pyramid_create_raw(int device, const unsigned char *image, int channels, int image_stride_bytes,
                               const unsigned short *depth, int depth_stride, float depth_scale, int on_device, int width,
                               int height, float fx, float fy, float ox, float oy, int levels, double timestamp,
                               dvo_amd_pyramid **out) {
  static const char *entry = "dvo_amd_pyramid_create_raw";
  if (out) *out = nullptr;
  if (!out || !image || !depth) return invalid(entry, "a NULL pointer");
  const RawFrame raw{image, channels, image_stride_bytes, depth, depth_stride, depth_scale, nullptr, nullptr};
  int rc = check_raw(entry, raw, width, width, "the image stride is smaller than the row it must hold", "depth_stride < width");
  if (!rc) rc = check_levels(entry, width, height, levels);
  if (!rc) rc = check_device(device, nullptr);
  if (rc) return rc;
  return pyramid_build(device, PyramidSpec{width, height, fx, fy, ox, oy, levels, timestamp},
                       Level0Source{nullptr, nullptr, 0, &raw, on_device != 0}, out);
}

int dvo_amd_pyramid_create_raw_batch(int device, const dvo_amd_raw_batch *batch, dvo_amd_pyramid **out) {
  static const char *entry = "dvo_amd_pyramid_create_raw_batch";
  if (out && batch)
    for (int f = 0; f < batch->count; ++f) out[f] = nullptr;
  if (!out || !batch) return invalid(entry, "a NULL pointer");
  const dvo_amd_raw_batch &b = *batch;
  if (b.count < 1) return invalid(entry, "count must be >= 1");
  if (!b.images || !b.depths) return invalid(entry, "a NULL pointer");
  for (int f = 0; f < b.count; ++f)
    if (!b.images[f] || !b.depths[f]) return invalid(entry, "a NULL pointer at frame " + std::to_string(f) + " of images or depths");
  const RawFrame raw{b.images[0], b.channels, b.image_stride_bytes, b.depths[0], b.depth_stride, b.depth_scale, nullptr, nullptr};
  int rc = check_raw(entry, raw, b.width, b.width, "the image stride is smaller than the row it must hold", "depth_stride < width");
  if (rc) return rc;
  if (b.build_selection != 0 && b.build_selection != 1) return invalid(entry, "build_selection must be 0 or 1");
  if (b.build_selection && !(std::isfinite(b.intensity_threshold) && std::isfinite(b.depth_threshold)))
    return invalid(entry, "a non-finite selection threshold");
  rc = check_levels(entry, b.width, b.height, b.levels);
  if (!rc) rc = check_device(device, nullptr);
  if (rc) return rc;
  return pyramid_build_batch(device, b, out);
}

int dvo_amd_pyramid_create_raw_remapped(int device, const unsigned char *image, int channels, int image_stride_bytes,
                                        const unsigned short *depth, int depth_stride, float depth_scale, int on_device,
                                        const dvo_amd_remap *remap, float fx, float fy, float ox, float oy, int levels,
                                        double timestamp, dvo_amd_pyramid **out) {
  static const char *entry = "dvo_amd_pyramid_create_raw_remapped";
  static const char *stride_why = "a stride of the raw frame is smaller than the remap's source row";
  if (out) *out = nullptr;
  if (!out || !image || !depth || !remap) return invalid(entry, "a NULL pointer");
  const RawFrame raw{image, channels, image_stride_bytes, depth, depth_stride, depth_scale, remap, nullptr};
  int rc = check_raw(entry, raw, remap->sw, remap->sw, stride_why, stride_why);
  if (!rc) rc = check_levels(entry, remap->w, remap->h, levels, " of the remap's output");
  if (!rc) rc = check_device(device, remap);
  if (rc) return rc;
  return pyramid_build(device, PyramidSpec{remap->w, remap->h, fx, fy, ox, oy, levels, timestamp},
                       Level0Source{nullptr, nullptr, 0, &raw, on_device != 0}, out);
}

int dvo_amd_pyramid_create_raw_registered(int device, const unsigned char *image, int channels, int image_stride_bytes,
                                          const unsigned short *depth, int depth_stride, float depth_scale, int on_device,
                                          const dvo_amd_registration *reg, const dvo_amd_remap *remap, int width, int height,
                                          float fx, float fy, float ox, float oy, int levels, double timestamp,
                                          dvo_amd_pyramid **out, dvo_amd_registration_stats *stats) {
  static const char *entry = "dvo_amd_pyramid_create_raw_registered";
  constexpr int kMaxDepthSide = 1 << 20;  // (float)u is exact far beyond it; a side this long is no camera's
  if (out) *out = nullptr;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!out || !image || !depth || !reg) return invalid(entry, "a NULL pointer");
  Registration R;
  const RawFrame raw{image, channels, image_stride_bytes, depth, depth_stride, depth_scale, remap, &R};
  int rc = check_raw(entry, raw, remap ? remap->sw : width, reg->depth_width, "the image stride is smaller than the row it must hold",
                     "depth_stride < depth_width");
  if (rc) return rc;
  if (reg->depth_width < 1 || reg->depth_height < 1 || reg->depth_width > kMaxDepthSide || reg->depth_height > kMaxDepthSide)
    return invalid(entry, "a side of the depth frame is outside 1..2^20");
  const float k[4] = {fx, fy, ox, oy};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) R.T[4 * r + c] = (float)reg->T[4 * c + r];  // column-major double -> row-major float
  if (!finite_all(reg->k_depth, 4) || !finite_all(R.T, 12) || !finite_all(k, 4))
    return invalid(entry, "a non-finite intrinsic or entry of the transform");
  if (!(reg->k_depth[0] > 0.0f && reg->k_depth[1] > 0.0f && fx > 0.0f && fy > 0.0f))
    return invalid(entry, "fx and fy of both cameras must be positive");
  if (!(reg->min_z >= 0.0f) || !std::isfinite(reg->min_z)) return invalid(entry, "min_z must be finite and >= 0");
  if (reg->fill != 0 && reg->fill != 1) return invalid(entry, "fill must be 0 or 1");
  if (remap && (remap->w != width || remap->h != height)) return invalid(entry, "the remap's output size differs from width x height");
  if ((long long)width * height > (1ll << 30)) return invalid(entry, "the pyramid's level 0 holds more than 2^30 pixels");
  rc = check_levels(entry, width, height, levels);
  if (!rc) rc = check_device(device, remap);
  if (rc) return rc;
  unsigned long long counts[4] = {0, 0, 0, 0};
  R.dw = reg->depth_width, R.dh = reg->depth_height;
  R.fxd = reg->k_depth[0], R.fyd = reg->k_depth[1], R.oxd = reg->k_depth[2], R.oyd = reg->k_depth[3];
  R.min_z = reg->min_z, R.mx = fx / R.fxd, R.my = fy / R.fyd, R.fill = reg->fill, R.counts = counts;
  rc = pyramid_build(device, PyramidSpec{width, height, fx, fy, ox, oy, levels, timestamp},
                     Level0Source{nullptr, nullptr, 0, &raw, on_device != 0}, out);
  if (rc == DVO_AMD_OK && stats) {
    stats->behind = (long long)counts[0], stats->outside = (long long)counts[1], stats->drawn = (long long)counts[2];
    stats->measurements = stats->behind + stats->outside + stats->drawn;
    stats->covered_pixels = (long long)counts[3];
  }
  return rc;
}

/* instrumentation: with enable != 0 every later pyramid build on `device` is bracketed by two events on the prep stream;
 * *last_ms (may be NULL) receives the device time of the most recent bracketed build */
int dvo_amd_debug_ingest_timing(int device, int enable, double *last_ms) {
  if (device < 0 || device >= kMaxDevices) return DVO_AMD_ERR_INVALID_ARGUMENT;
  return ingest_timing(device, enable, last_ms);
}

/* instrumentation: what the most recent batched build on `device` enqueued */
int dvo_amd_debug_batch_build_stats(int device, int *kernel_launches, int *copies, int *synchronisations) {
  if (device < 0 || device >= kMaxDevices) return DVO_AMD_ERR_INVALID_ARGUMENT;
  return batch_build_stats(device, kernel_launches, copies, synchronisations);
}

}  // extern "C"
