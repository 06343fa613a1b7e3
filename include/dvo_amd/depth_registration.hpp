// depth_registration.hpp -- header-only C++ adaptor over the registered frame ingest of the C ABI
// (dvo_amd_pyramid_create_raw_registered).
//
// The reference has no class for this: it subscribes to camera/depth_registered/image_rect_raw (dvo_ros/src/camera_base.cpp:31-33)
// and leaves the registration to depth_image_proc/register, on the CPU upstream.  dvo::core::DepthRegistration is that step for
// a caller that holds the sensor's own two streams: a value type -- the depth camera's size and intrinsics, the transform from
// the depth camera to the colour camera, the near cull and the footprint switch -- whose create() takes a raw colour image and a
// raw depth frame of the depth camera to an RgbdImagePyramid of the colour camera, next to Rectification::create; with a
// Rectification the image goes through its table on the way (the depth never does).  The rule is pinned in dvo_amd.h.
#ifndef DVO_AMD_DEPTH_REGISTRATION_HPP_
#define DVO_AMD_DEPTH_REGISTRATION_HPP_

#include "rectification.hpp"

namespace dvo {
namespace core {

class DepthRegistration {
 public:
  typedef dvo_amd_registration_stats Stats;  // measurements == behind + outside + drawn; covered_pixels

  DepthRegistration() { dvo_amd_default_registration(&reg_); }  // identity, no size: create() is refused until one is set
  DepthRegistration(int depth_width, int depth_height, const IntrinsicMatrix &depth_camera, const AffineTransformd &depth_to_colour,
                    float min_z = 0.0f, bool fill = false) {
    dvo_amd_default_registration(&reg_);
    reg_.depth_width = depth_width, reg_.depth_height = depth_height;
    reg_.k_depth[0] = depth_camera.fx(), reg_.k_depth[1] = depth_camera.fy(), reg_.k_depth[2] = depth_camera.ox(), reg_.k_depth[3] = depth_camera.oy();
    std::memcpy(reg_.T, data(depth_to_colour), sizeof(reg_.T));
    reg_.min_z = min_z, reg_.fill = fill ? 1 : 0;
  }

  int depthWidth() const { return reg_.depth_width; }
  int depthHeight() const { return reg_.depth_height; }
  float minZ() const { return reg_.min_z; }
  bool fill() const { return reg_.fill != 0; }
  void setMinZ(float min_z) { reg_.min_z = min_z; }
  void setFill(bool fill) { reg_.fill = fill ? 1 : 0; }
  const dvo_amd_registration &c() const { return reg_; }

  // A raw image of the colour camera (width x height, `camera`) and a raw depth frame of the depth camera -> the pyramid of the
  // colour camera.  image: uint8, 1 channel (grey) or 3 (B, G, R), image_stride_bytes 0 = packed; depth: uint16, 0 = no
  // measurement, depth_stride in elements, 0 = packed; on_device: both pointers are device memory of `device`.
  RgbdImagePyramidPtr create(int width, int height, const IntrinsicMatrix &camera, const unsigned char *image, int channels,
                             int image_stride_bytes, const unsigned short *depth, int depth_stride, float depth_scale, int levels,
                             double timestamp = 0.0, Stats *stats = nullptr, bool on_device = false, int device = 0) const {
    return build(nullptr, device, width, height, width, camera, image, channels, image_stride_bytes, depth, depth_stride, depth_scale,
                 levels, timestamp, stats, on_device);
  }

  // The same with the image taken through `rect` on the way: the image has rect's source size, the pyramid its output size and
  // its rectified camera.
  RgbdImagePyramidPtr create(const Rectification &rect, const unsigned char *image, int channels, int image_stride_bytes,
                             const unsigned short *depth, int depth_stride, float depth_scale, int levels, double timestamp = 0.0,
                             Stats *stats = nullptr, bool on_device = false) const {
    const Rectification::Info i = rect.info();
    return build(rect.handle(), rect.device(), i.width, i.height, i.src_width, rect.intrinsics(), image, channels, image_stride_bytes,
                 depth, depth_stride, depth_scale, levels, timestamp, stats, on_device);
  }
#ifdef DVO_AMD_HAVE_OPENCV
  // CV_8UC1 or CV_8UC3 image of the colour camera, CV_16UC1 depth of the depth camera's size
  RgbdImagePyramidPtr create(const IntrinsicMatrix &camera, const cv::Mat &image, const cv::Mat &depth, float depth_scale, int levels,
                             double timestamp = 0.0, Stats *stats = nullptr) const {
    if ((image.type() != CV_8UC1 && image.type() != CV_8UC3) || depth.type() != CV_16UC1 || depth.cols != reg_.depth_width ||
        depth.rows != reg_.depth_height)
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "DepthRegistration::create");
    return create(image.cols, image.rows, camera, image.ptr<unsigned char>(), image.channels(), (int)image.step,
                  depth.ptr<unsigned short>(), (int)(depth.step / sizeof(unsigned short)), depth_scale, levels, timestamp, stats);
  }
#endif

 private:
  RgbdImagePyramidPtr build(const dvo_amd_remap *remap, int device, int width, int height, int image_width, const IntrinsicMatrix &K,
                            const unsigned char *image, int channels, int image_stride_bytes, const unsigned short *depth,
                            int depth_stride, float depth_scale, int levels, double timestamp, Stats *stats, bool on_device) const {
    dvo_amd_pyramid *p = nullptr;
    detail::check(dvo_amd_pyramid_create_raw_registered(device, image, channels, image_stride_bytes ? image_stride_bytes : image_width * channels,
                                                        depth, depth_stride ? depth_stride : reg_.depth_width, depth_scale, on_device ? 1 : 0,
                                                        &reg_, remap, width, height, K.fx(), K.fy(), K.ox(), K.oy(), levels, timestamp, &p,
                                                        stats),
                  "DepthRegistration::create");
    return RgbdImagePyramidPtr(new RgbdImagePyramid(p, width, height, K, device, timestamp));
  }
  dvo_amd_registration reg_;
};

}  // namespace core
}  // namespace dvo

#endif
