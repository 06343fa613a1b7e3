// rectification.hpp -- header-only C++ adaptor over the remap entries of the C ABI (dvo_amd_remap_*,
// dvo_amd_pyramid_create_raw_remapped).
//
// The reference has no class for this: it tracks on rectified images and leaves the rectification to image_proc
// (camera_keyframe_tracking.cpp:89 reads CameraInfo::P; cv::initUndistortRectifyMap + cv::remap run upstream, on the CPU).
// dvo::core::Rectification is that step for a caller that holds the sensor's own frames: made once per camera -- from the
// five lens coefficients (undistort) or from any pair of CV_32FC1 maps (fromMaps) --, shared by value (shared ownership of one
// device table), and applied by create(), which takes a raw frame to an RgbdImagePyramid of the rectified camera the way
// RgbdCameraPyramid::create takes two float planes to one.  The rules are pinned in dvo_amd.h.  No PCL, no OpenCV in the
// signatures; cv::Mat overloads where OpenCV is present, as in dense_tracking.hpp.
#ifndef DVO_AMD_RECTIFICATION_HPP_
#define DVO_AMD_RECTIFICATION_HPP_

#include <memory>
#include <vector>

#include "dense_tracking.hpp"

namespace dvo {
namespace core {

class Rectification {
 public:
  Rectification() {}  // empty: valid() is false, create() throws

  // k1, k2, p1, p2, k3 in OpenCV's order; `camera` is the rectified camera (cv::initUndistortRectifyMap's newCameraMatrix with
  // R = I) of width x height pixels, `source` the real one of src_width x src_height
  static Rectification undistort(int width, int height, const IntrinsicMatrix &camera, int src_width, int src_height,
                                 const IntrinsicMatrix &source, const float dist[5], int device = 0) {
    const float k_out[4] = {camera.fx(), camera.fy(), camera.ox(), camera.oy()};
    const float k_src[4] = {source.fx(), source.fy(), source.ox(), source.oy()};
    dvo_amd_remap *r = nullptr;
    detail::check(dvo_amd_remap_create_undistort(device, width, height, k_out, src_width, src_height, k_src, dist, &r),
                  "Rectification::undistort");
    return Rectification(r, camera, device);
  }

  // any map: map_x, map_y hold width x height source positions (cv::remap's CV_32FC1 pair), stride in floats (0: width)
  static Rectification fromMaps(int width, int height, const IntrinsicMatrix &camera, const float *map_x, const float *map_y,
                                int stride, int src_width, int src_height, int device = 0) {
    dvo_amd_remap *r = nullptr;
    detail::check(dvo_amd_remap_create(device, width, height, map_x, map_y, stride ? stride : width, src_width, src_height, &r),
                  "Rectification::fromMaps");
    return Rectification(r, camera, device);
  }
#ifdef DVO_AMD_HAVE_OPENCV
  // the two outputs of cv::initUndistortRectifyMap(..., CV_32FC1, map1, map2)
  static Rectification fromMaps(const cv::Mat &map_x, const cv::Mat &map_y, const IntrinsicMatrix &camera, int src_width,
                                int src_height, int device = 0) {
    if (map_x.type() != CV_32FC1 || map_y.type() != CV_32FC1 || map_x.size() != map_y.size())
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "Rectification::fromMaps");
    if (map_x.step != map_y.step) {
      cv::Mat x = map_x.clone(), y = map_y.clone();
      return fromMaps(x.cols, x.rows, camera, x.ptr<float>(), y.ptr<float>(), (int)(x.step / sizeof(float)), src_width, src_height, device);
    }
    return fromMaps(map_x.cols, map_x.rows, camera, map_x.ptr<float>(), map_y.ptr<float>(), (int)(map_x.step / sizeof(float)),
                    src_width, src_height, device);
  }
#endif

  bool valid() const { return (bool)handle_; }
  dvo_amd_remap *handle() const { return handle_.get(); }
  const IntrinsicMatrix &intrinsics() const { return K_; }  // of the rectified camera: what the pyramids carry
  int device() const { return device_; }

  struct Info {
    int width, height, src_width, src_height, n_inside;  // n_inside: output pixels that see the source (the others are 0 / NaN)
  };
  Info info() const {
    Info i = {0, 0, 0, 0, 0};
    detail::check(dvo_amd_remap_info(need(), &i.width, &i.height, &i.src_width, &i.src_height, &i.n_inside), "Rectification::info");
    return i;
  }
  void download(std::vector<float> &map_x, std::vector<float> &map_y) const {
    const Info i = info();
    map_x.resize((size_t)i.width * i.height), map_y.resize((size_t)i.width * i.height);
    detail::check(dvo_amd_remap_download(need(), map_x.data(), map_y.data()), "Rectification::download");
  }

  // A raw frame of the source camera -> the pyramid of the rectified camera (dvo_amd_pyramid_create_raw_remapped), next to
  // RgbdCameraPyramid::create.  image: uint8, 1 channel (grey) or 3 (B, G, R), image_stride_bytes 0 = packed; depth: uint16,
  // 0 = no measurement, depth_stride in elements, 0 = packed; on_device: both pointers are device memory of device().
  RgbdImagePyramidPtr create(const unsigned char *image, int channels, int image_stride_bytes, const unsigned short *depth,
                             int depth_stride, float depth_scale, int levels, double timestamp = 0.0, bool on_device = false) const {
    const Info i = info();
    dvo_amd_pyramid *p = nullptr;
    detail::check(dvo_amd_pyramid_create_raw_remapped(device_, image, channels, image_stride_bytes ? image_stride_bytes : i.src_width * channels,
                                                      depth, depth_stride ? depth_stride : i.src_width, depth_scale, on_device ? 1 : 0,
                                                      handle_.get(), K_.fx(), K_.fy(), K_.ox(), K_.oy(), levels, timestamp, &p),
                  "Rectification::create");
    return RgbdImagePyramidPtr(new RgbdImagePyramid(p, i.width, i.height, K_, device_, timestamp));
  }
#ifdef DVO_AMD_HAVE_OPENCV
  // CV_8UC1 or CV_8UC3 image, CV_16UC1 depth, both of the source camera's size
  RgbdImagePyramidPtr create(const cv::Mat &image, const cv::Mat &depth, float depth_scale, int levels, double timestamp = 0.0) const {
    const Info i = info();
    if ((image.type() != CV_8UC1 && image.type() != CV_8UC3) || depth.type() != CV_16UC1 || image.size() != depth.size() ||
        image.cols != i.src_width || image.rows != i.src_height)
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "Rectification::create");
    return create(image.ptr<unsigned char>(), image.channels(), (int)image.step, depth.ptr<unsigned short>(),
                  (int)(depth.step / sizeof(unsigned short)), depth_scale, levels, timestamp);
  }
#endif

 private:
  struct Release {
    void operator()(dvo_amd_remap *r) const { dvo_amd_remap_release(r); }
  };
  Rectification(dvo_amd_remap *r, const IntrinsicMatrix &K, int device) : handle_(r, Release()), K_(K), device_(device) {}
  dvo_amd_remap *need() const {
    if (!handle_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "Rectification: empty");
    return handle_.get();
  }
  std::shared_ptr<dvo_amd_remap> handle_;
  IntrinsicMatrix K_;
  int device_ = 0;
};

}  // namespace core
}  // namespace dvo

#endif
