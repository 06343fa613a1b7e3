// dense_tracking.hpp -- header-only C++ adaptor over the C ABI (include/dvo_amd.h).
//
// Re-declares, name for name, the part of dvo_core's interface that callers of the dense-tracking hot path use:
//   dvo::core::IntrinsicMatrix        dvo_core/include/dvo/core/intrinsic_matrix.h:33-64
//   dvo::core::RgbdCameraPyramid      dvo_core/include/dvo/core/rgbd_image.h:127-144
//   dvo::core::RgbdImagePyramid       dvo_core/include/dvo/core/rgbd_image.h:242-262
//   dvo::core::RgbdImage (level(i))   dvo_core/include/dvo/core/rgbd_image.h:146-240 (what callers of the hot path touch)
//   dvo::core::PointSelection + predicates   dvo_core/include/dvo/core/point_selection.h:32-117
//   dvo::DenseTracker {Config, TerminationCriteria, IterationStats, LevelStats, Stats, Result, configure, match x4,
//                      computeIntensityErrorImage}
//                                     dvo_core/include/dvo/dense_tracking.h:39-213
// so that dvo_ros / dvo_slam / dvo_benchmark call sites (camera_dense_tracking.cpp:243-276, local_tracker.cpp:157-213,
// constraint_proposal_validator.cpp:132-166, benchmark_slam.cpp:352-547) compile against it unchanged apart from the
// include path.  Where <Eigen/Geometry> / <opencv2/core/core.hpp> are on the include path the Eigen and cv::Mat
// signatures of the reference are used; otherwise minimal stand-in value types with the same accessors are provided
// (this image has neither, which is what the CPU compile check in tests/ exercises).
//
// All compute happens in libdvo_amd.so on the GPU.  Errors that the reference signals with assert() are thrown as
// dvo::DvoAmdError; the failure modes the reference reports through its Result (NaN, TooFewConstraints) are preserved.
#ifndef DVO_AMD_DENSE_TRACKING_HPP_
#define DVO_AMD_DENSE_TRACKING_HPP_

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../dvo_amd.h"

#define DVO_AMD_MAX_DEVICES_FOR_CLOUDS 16

#if !defined(DVO_AMD_NO_EIGEN) && defined(__has_include)
#if __has_include(<Eigen/Geometry>)
#include <Eigen/Geometry>
#define DVO_AMD_HAVE_EIGEN 1
#endif
#endif
#if !defined(DVO_AMD_NO_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#define DVO_AMD_HAVE_OPENCV 1
#endif
#endif

namespace dvo {

class DvoAmdError : public std::runtime_error {
 public:
  DvoAmdError(int status, const std::string &where)
      : std::runtime_error(where + ": " + dvo_amd_status_string(status) + " [" + dvo_amd_last_error() + "]"), status_(status) {}
  int status() const { return status_; }

 private:
  int status_;
};

namespace detail {
inline void check(int status, const char *where) {
  if (status != DVO_AMD_OK) throw DvoAmdError(status, where);
}
}  // namespace detail

namespace core {

#ifdef DVO_AMD_HAVE_EIGEN
typedef Eigen::Affine3d AffineTransformd;
typedef Eigen::Matrix<double, 6, 6> Matrix6d;
typedef Eigen::Matrix<double, 6, 1> Vector6d;
typedef Eigen::Matrix2d Matrix2d;
typedef Eigen::Vector2d Vector2d;
inline const double *data(const AffineTransformd &T) { return T.matrix().data(); }
inline double *data(AffineTransformd &T) { return T.matrix().data(); }
inline double *data(Matrix6d &m) { return m.data(); }
#else
// column-major stand-ins with the accessors the call sites use
template <int R, int C>
struct Mat {
  double m[R * C];
  Mat() { std::memset(m, 0, sizeof(m)); }
  double &operator()(int r, int c) { return m[c * R + r]; }
  double operator()(int r, int c) const { return m[c * R + r]; }
  double &operator()(int i) { return m[i]; }
  double operator()(int i) const { return m[i]; }
  double *data() { return m; }
  const double *data() const { return m; }
  void setZero() { std::memset(m, 0, sizeof(m)); }
  void setIdentity() {
    setZero();
    for (int i = 0; i < (R < C ? R : C); ++i) (*this)(i, i) = 1.0;
  }
  void setConstant(double v) { std::fill(m, m + R * C, v); }
  double sum() const {
    double s = 0;
    for (int i = 0; i < R * C; ++i) s += m[i];
    return s;
  }
};
typedef Mat<6, 6> Matrix6d;
typedef Mat<6, 1> Vector6d;
typedef Mat<2, 2> Matrix2d;
typedef Mat<2, 1> Vector2d;
struct AffineTransformd {
  Mat<4, 4> mat;
  AffineTransformd() { mat.setIdentity(); }
  Mat<4, 4> &matrix() { return mat; }
  const Mat<4, 4> &matrix() const { return mat; }
  void setIdentity() { mat.setIdentity(); }
  double &operator()(int r, int c) { return mat(r, c); }
  double operator()(int r, int c) const { return mat(r, c); }
};
inline const double *data(const AffineTransformd &T) { return T.mat.data(); }
inline double *data(AffineTransformd &T) { return T.mat.data(); }
inline double *data(Matrix6d &m) { return m.data(); }
#endif

// weight_calculation.h:107-119,191-203.  DenseTracker::configure stores these in Config and match() never reads them (the
// bivariate t-distribution with 5 degrees of freedom is hard-coded); they exist here so that
// dvo_ros' updateConfigFromDynamicReconfigure (configtools.h:34-79) and the Config stream operator compile unchanged.
struct ScaleEstimators {
  typedef enum { Unit, NormalDistribution, TDistribution, MAD } enum_t;
  static const char *str(enum_t type) {  // weight_calculation.cpp:255-273
    switch (type) {
      case Unit: return "Unit";
      case TDistribution: return "TDistribution";
      case MAD: return "MAD";
      case NormalDistribution: return "NormalDistribution";
      default: break;
    }
    return "";
  }
};
struct InfluenceFunctions {
  typedef enum { Unit, Tukey, TDistribution, Huber } enum_t;
  static const char *str(enum_t type) {  // weight_calculation.cpp:373-391
    switch (type) {
      case Unit: return "Unit";
      case TDistribution: return "TDistribution";
      case Tukey: return "Tukey";
      case Huber: return "Huber";
      default: break;
    }
    return "";
  }
};
// TDistributionScaleEstimator::DEFAULT_DOF / TDistributionInfluenceFunction::DEFAULT_DOF (weight_calculation.cpp)
static const float kTDistributionDefaultDof = 5.0f;

namespace linalg {
// eigenvalues of a symmetric 6x6 matrix (column-major) in ascending order by cyclic Jacobi rotations: what
// Eigen::EigenSolver + std::sort give DenseTracker::IterationStats::InformationEigenValues (dense_tracking_config.cpp:123-128)
// for the symmetric EstimateInformation
inline void symmetric_eigenvalues6(const double *A_colmajor, double ev[6]) {
  double a[6][6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) a[r][c] = 0.5 * (A_colmajor[c * 6 + r] + A_colmajor[r * 6 + c]);
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) (r == c ? diag : off) += a[r][c] * a[r][c];
    if (off <= 1e-30 * diag || off == 0.0) break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {  // columns p, q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq, a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {  // rows p, q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk, a[q][k] = s * apk + c * aqk;
        }
      }
  }
  for (int i = 0; i < 6; ++i) ev[i] = a[i][i];
  std::sort(ev, ev + 6);
}
}  // namespace linalg

// intrinsic_matrix.h:33-64
class IntrinsicMatrix {
 public:
  IntrinsicMatrix() : fx_(0), fy_(0), ox_(0), oy_(0) {}
  static IntrinsicMatrix create(float fx, float fy, float ox, float oy) {
    IntrinsicMatrix k;
    k.fx_ = fx, k.fy_ = fy, k.ox_ = ox, k.oy_ = oy;
    return k;
  }
  float fx() const { return fx_; }
  float fy() const { return fy_; }
  float ox() const { return ox_; }
  float oy() const { return oy_; }
  void invertOffset() { ox_ *= -1, oy_ *= -1; }
  void scale(float factor) { fx_ *= factor, fy_ *= factor, ox_ *= factor, oy_ *= factor; }

 private:
  float fx_, fy_, ox_, oy_;
};

class RgbdCameraPyramid;
class RgbdImagePyramid;

// rgbd_image.h:146-240, as far as callers of the hot path use it: LocalTracker::update pre-builds the point cloud and the
// 8-channel acceleration structure of every level (local_tracker.cpp:163-169).  Here every level, its derivative planes,
// rays and gather layout are built on the GPU by RgbdImagePyramid::build, so these members have nothing left to do.
// RgbdImage::pointcloud (rgbd_image.h: Eigen::Matrix<float, 4, Dynamic>): the level's points (x, y, z, 1) at the identity pose,
// column-major 4 x (width * height), NaN points included.  Filled by dvo_amd_point_cloud on the first access and kept: a
// caller that never reads it costs nothing.  The accessors the reference's readers use; no Eigen expression support.
class PointCloudMatrix {
 public:
  PointCloudMatrix() : owner_(nullptr), level_(0), filled_(false) {}
  long rows() const { return 4; }
  inline long cols() const;
  inline const float *data() const;
  float operator()(long r, long c) const { return data()[c * 4 + r]; }

 private:
  friend class RgbdImagePyramid;
  inline void fill() const;
  const RgbdImagePyramid *owner_;
  int level_;
  mutable bool filled_;
  mutable std::vector<float> xyzw_;
};

// RgbdImage::normals / RgbdImage::angles without OpenCV (rgbd_image.h: cv::Mat CV_32FC4 / CV_32FC1): a level's normal plane
// (x, y, z, 0 per pixel, four NaNs where the surface has no normal) and |n.z| per pixel, row-major.  Filled by
// dvo_amd_pyramid_normals with the default options -- RgbdImage::calculateNormals' own rule (dvo_amd.h, "Surface normals") -- on
// the first access and kept, like PointCloudMatrix.
class NormalPlane {
 public:
  explicit NormalPlane(int channels) : owner_(nullptr), level_(0), channels_(channels), filled_(false) {}
  inline long rows() const;
  inline long cols() const;
  int channels() const { return channels_; }
  inline const float *data() const;
  float operator()(long row, long col, int channel = 0) const { return data()[((size_t)row * (size_t)cols() + (size_t)col) * channels_ + channel]; }

 private:
  friend class RgbdImagePyramid;
  inline void fill() const;
  const RgbdImagePyramid *owner_;
  int level_, channels_;
  mutable bool filled_;
  mutable long rows_ = 0, cols_ = 0;
  mutable std::vector<float> values_;
};

class RgbdImage {
 public:
#ifdef DVO_AMD_HAVE_OPENCV
  RgbdImage() : width(0), height(0), owner_(nullptr), level_(0) {}
#else
  RgbdImage() : width(0), height(0), normals(4), angles(1), owner_(nullptr), level_(0) {}
#endif
  size_t width, height;
  IntrinsicMatrix intrinsics;  // of this level (RgbdCamera::intrinsics())
  // the colour image callers attach (camera_keyframe_tracking.cpp:252): float B, G, R in 0..255, width * height pixels.  Read
  // by AsyncPointCloudBuilder::BuildJob (include/dvo_amd/point_cloud.hpp), converted to 8 bits by the rule of dvo_amd.h
  // (clamped to [0, 255], truncated, NaN -> 0); empty: grey from the intensity plane.
#ifdef DVO_AMD_HAVE_OPENCV
  cv::Mat rgb;  // CV_32FC3
#else
  std::vector<float> rgb;  // interleaved B, G, R
#endif
  PointCloudMatrix pointcloud;
  // rgbd_image.cpp:502-532: the surface normal of every pixel (CV_32FC4: x, y, z, 0) and `angles`, |n.z| (CV_32FC1), computed on
  // the device by the reference's own rule (dvo_amd_pyramid_normals with the default options).  With OpenCV the two members are
  // the reference's cv::Mat, filled by calculateNormals(); without, they fill themselves on first access and calculateNormals()
  // only forces that.
#ifdef DVO_AMD_HAVE_OPENCV
  cv::Mat normals, angles;
#else
  NormalPlane normals, angles;
#endif
  inline void calculateNormals();
  void initialize() {}
  void calculateDerivatives() {}
  bool calculateIntensityDerivatives() { return false; }
  void calculateDepthDerivatives() {}
  void buildPointCloud() {}  // no-op: `pointcloud` fills itself on first access
  void buildAccelerationStructure() {}
  // host copy of one plane of this level: 0 intensity, 1 depth, 2 intensity_dx, 3 intensity_dy, 4 depth_dx, 5 depth_dy
  inline std::vector<float> plane(int which) const;
  const RgbdImagePyramid *pyramid() const { return owner_; }  // (not in the reference) the pyramid this level belongs to
  int level() const { return level_; }                        // ... and its index there

 private:
  friend class RgbdImagePyramid;
  const RgbdImagePyramid *owner_;
  int level_;
};

class SelectionMask;

// (not in the reference) Exposure compensation (dvo_amd.h, "Exposure compensation"): the options of the gain and bias fit with their
// defaults, and the record one estimate returns
struct ExposureOptions : dvo_amd_exposure_options {
  ExposureOptions() { dvo_amd_default_exposure_options(this); }
};
typedef dvo_amd_exposure_estimate ExposureEstimate;

// rgbd_image.h:242-262.  The reference extends a pyramid lazily, level by level; here the base planes are kept on the host
// until the first build(n), then the device pyramid is (re)built with max(n, levels so far) levels in one go.
class RgbdImagePyramid {
 public:
  typedef std::shared_ptr<RgbdImagePyramid> Ptr;

  RgbdImagePyramid(int width, int height, const IntrinsicMatrix &K, const float *intensity, const float *depth, int stride,
                   int device, double timestamp)
      : width_(width), height_(height), K_(K), device_(device), timestamp_(timestamp), handle_(nullptr), levels_(0) {
    intensity_.resize((size_t)width * height);
    depth_.resize((size_t)width * height);
    for (int y = 0; y < height; ++y) {
      std::memcpy(&intensity_[(size_t)y * width], intensity + (size_t)y * stride, sizeof(float) * width);
      std::memcpy(&depth_[(size_t)y * width], depth + (size_t)y * stride, sizeof(float) * width);
    }
  }
  // adopts a pyramid that was built on the device (visualization::KeyframeMap::renderPyramid): no host planes are kept; a
  // later build() of more levels downloads level 0 once and rebuilds from it
  RgbdImagePyramid(dvo_amd_pyramid *adopted, int width, int height, const IntrinsicMatrix &K, int device, double timestamp)
      : width_(width), height_(height), K_(K), device_(device), timestamp_(timestamp), handle_(adopted),
        levels_(dvo_amd_pyramid_levels(adopted)) {}
  // (not in the reference) the raw frames of one camera -- uint8 grey or B,G,R, uint16 depth with 0 = no measurement -- as
  // `levels`-level pyramids built in ONE call (dvo_amd_pyramid_create_raw_batch): the frames share every kernel launch, so a
  // recorded sequence or a burst of frames costs a few dozen launches instead of a few dozen per frame.  A stride of 0 means
  // packed rows; timestamps: one per frame, or null for 0.0.  With with_selection every pyramid leaves the call with the point
  // selection for the two thresholds already built (pass DenseTracker::Config's IntensityDerivativeThreshold and
  // DepthDerivativeThreshold: the first match() then builds none).  Each result is what the single-frame raw create makes.
  static std::vector<Ptr> createRawBatch(int width, int height, const IntrinsicMatrix &K, const std::vector<const unsigned char *> &images,
                                         int channels, int image_stride_bytes, const std::vector<const unsigned short *> &depths,
                                         int depth_stride, float depth_scale, int levels, const double *timestamps = nullptr,
                                         bool with_selection = false, float intensity_threshold = 0.0f, float depth_threshold = 0.0f,
                                         int device = 0, bool on_device = false) {
    if (images.empty() || images.size() != depths.size()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImagePyramid::createRawBatch");
    dvo_amd_raw_batch b;
    std::memset(&b, 0, sizeof(b));
    b.count = (int)images.size(), b.images = images.data(), b.depths = depths.data(), b.timestamps = timestamps;
    b.channels = channels, b.image_stride_bytes = image_stride_bytes ? image_stride_bytes : width * channels;
    b.depth_stride = depth_stride ? depth_stride : width, b.depth_scale = depth_scale, b.on_device = on_device ? 1 : 0;
    b.width = width, b.height = height, b.fx = K.fx(), b.fy = K.fy(), b.ox = K.ox(), b.oy = K.oy(), b.levels = levels;
    b.build_selection = with_selection ? 1 : 0, b.intensity_threshold = intensity_threshold, b.depth_threshold = depth_threshold;
    std::vector<dvo_amd_pyramid *> handles(images.size(), nullptr);
    detail::check(dvo_amd_pyramid_create_raw_batch(device, &b, handles.data()), "RgbdImagePyramid::createRawBatch");
    std::vector<Ptr> out;
    size_t adopted = 0;
    try {
      out.reserve(handles.size());
      for (; adopted < handles.size(); ++adopted) {
        RgbdImagePyramid *p = new RgbdImagePyramid(handles[adopted], width, height, K, device, timestamps ? timestamps[adopted] : 0.0);
        handles[adopted] = nullptr;  // p owns it now (releasing NULL is a no-op)
        out.push_back(Ptr(p));
      }
    } catch (...) {
      for (size_t f = adopted; f < handles.size(); ++f) dvo_amd_pyramid_release(handles[f]);
      throw;
    }
    return out;
  }
  ~RgbdImagePyramid() { dvo_amd_pyramid_release(handle_); }
  RgbdImagePyramid(const RgbdImagePyramid &) = delete;
  RgbdImagePyramid &operator=(const RgbdImagePyramid &) = delete;

  void compute(const size_t num_levels) { build(num_levels); }  // deprecated spelling kept by the reference (:252)

  void build(const size_t num_levels) {
    if ((size_t)levels_ >= num_levels && handle_) return;
    const int want = (int)std::max<size_t>(num_levels, (size_t)levels_);
    if (intensity_.empty() && handle_) {  // an adopted pyramid: its level 0 is the base
      intensity_.resize((size_t)width_ * height_), depth_.resize((size_t)width_ * height_);
      detail::check(dvo_amd_pyramid_download_plane(handle_, 0, 0, intensity_.data()), "RgbdImagePyramid::build");
      detail::check(dvo_amd_pyramid_download_plane(handle_, 0, 1, depth_.data()), "RgbdImagePyramid::build");
    }
    dvo_amd_pyramid *fresh = nullptr;
    detail::check(dvo_amd_pyramid_create(device_, intensity_.data(), depth_.data(), width_, height_, width_, K_.fx(), K_.fy(),
                                         K_.ox(), K_.oy(), want, timestamp_, &fresh),
                  "RgbdImagePyramid::build");
    dvo_amd_pyramid_release(handle_);
    handle_ = fresh;
    levels_ = want;
  }

  // rgbd_image.h:256: builds up to idx + 1 levels on demand, like the reference
  RgbdImage &level(size_t idx) {
    if (idx >= (size_t)DVO_AMD_MAX_LEVELS) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImagePyramid::level");
    build(idx + 1);
    RgbdImage &img = level_views_[idx];  // fixed storage: a reference handed out stays valid, as in the reference
    if (img.owner_ != this || img.level_ != (int)idx || img.width == 0) {
      int w = 0, h = 0;
      float k[4];
      detail::check(dvo_amd_pyramid_level_info(handle_, (int)idx, &w, &h, k), "RgbdImagePyramid::level");
      img.width = (size_t)w, img.height = (size_t)h;
      img.intrinsics = IntrinsicMatrix::create(k[0], k[1], k[2], k[3]);
      img.owner_ = this, img.level_ = (int)idx;
      img.pointcloud.owner_ = this, img.pointcloud.level_ = (int)idx, img.pointcloud.filled_ = false;
#ifndef DVO_AMD_HAVE_OPENCV
      img.normals.owner_ = img.angles.owner_ = this, img.normals.level_ = img.angles.level_ = (int)idx;
      img.normals.filled_ = img.angles.filled_ = false;
#endif
    }
    return img;
  }

  // (not in the reference, which tracks against the raw keyframe) This keyframe with the level-0 depth of the frames tracked
  // against it averaged into its own, on the device (dvo_amd.h, "Depth fusion"): a new pyramid of this one's size, intrinsics,
  // level count and timestamp; this one and the frames are only read.  transformations[k]: for tracker.match(*this, *frames[k],
  // result) that is result.Transformation as returned.  All pyramids must hold their levels (RgbdImagePyramid::build; a match has
  // built them).  frame_counts: one record per frame; keyframe_counts: one record; observations: width * height bytes.
  struct FuseOptions : dvo_amd_fuse_options {
    FuseOptions() { dvo_amd_default_fuse_options(this); }
  };
  struct FuseFrameCounts {
    long long valid, behind, outside, no_depth, consistent, occluded, seen_through, fused;
  };
  struct FuseKeyframeCounts {
    long long with_depth, confirmed, unconfirmed_kept, unconfirmed_dropped;
  };
  Ptr fuseDepth(const std::vector<Ptr> &frames, const std::vector<AffineTransformd> &transformations,
                const FuseOptions &options = FuseOptions(), std::vector<FuseFrameCounts> *frame_counts = nullptr,
                FuseKeyframeCounts *keyframe_counts = nullptr, std::vector<unsigned char> *observations = nullptr) const {
    static_assert(sizeof(FuseFrameCounts) == DVO_AMD_FUSE_FRAME_COUNTS * sizeof(long long) &&
                      sizeof(FuseKeyframeCounts) == DVO_AMD_FUSE_KEYFRAME_COUNTS * sizeof(long long),
                  "the count records are dvo_amd_pyramid_fuse_depth's");
    const char *where = "RgbdImagePyramid::fuseDepth";
    if (frames.size() != transformations.size() || frames.size() > (size_t)DVO_AMD_FUSE_MAX_FRAMES)
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
    std::vector<const dvo_amd_pyramid *> handles(frames.size());
    std::vector<double> T(16 * frames.size());
    for (size_t k = 0; k < frames.size(); ++k) {
      if (!frames[k]) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
      handles[k] = frames[k]->handle();
      std::memcpy(&T[16 * k], data(transformations[k]), 16 * sizeof(double));  // column-major
    }
    std::vector<FuseFrameCounts> records(frames.size() + 1);
    FuseKeyframeCounts key_record;
    if (observations) observations->assign((size_t)width_ * height_, 0);
    dvo_amd_pyramid *fused = nullptr;
    detail::check(dvo_amd_pyramid_fuse_depth(handle_, (int)frames.size(), handles.data(), T.data(), &options, &fused, &records[0].valid,
                                             &key_record.with_depth, observations ? observations->data() : nullptr),
                  where);
    Ptr out;
    try {
      out = Ptr(new RgbdImagePyramid(fused, width_, height_, K_, device_, timestamp_));
    } catch (...) {
      dvo_amd_pyramid_release(fused);
      throw;
    }
    if (frame_counts) frame_counts->assign(records.begin(), records.end() - 1);
    if (keyframe_counts) *keyframe_counts = key_record;
    return out;
  }

  // (not in the reference, which tracks raw sensor depth) This frame with its level-0 depth filtered on the device (dvo_amd.h,
  // "Depth filtering"): an edge-preserving filter whose range scale is the sensor's noise model, unsupported pixels dropped, small
  // holes filled.  A new pyramid of this one's size, intrinsics, level count and timestamp; this one is only read and must hold
  // its levels (RgbdImagePyramid::build; a match has built them).  counts: one record; support: width * height window members.
  struct DepthFilterOptions : dvo_amd_depth_filter_options {
    DepthFilterOptions() { dvo_amd_default_depth_filter_options(this); }
  };
  struct DepthFilterCounts {
    long long with_depth, kept, dropped, holes, filled;
  };
  Ptr filterDepth(const DepthFilterOptions &options = DepthFilterOptions(), DepthFilterCounts *counts = nullptr,
                  std::vector<unsigned short> *support = nullptr) const {
    static_assert(sizeof(DepthFilterCounts) == DVO_AMD_DEPTH_FILTER_COUNTS * sizeof(long long),
                  "the count record is dvo_amd_pyramid_filter_depth's");
    const char *where = "RgbdImagePyramid::filterDepth";
    DepthFilterCounts record;
    if (support) support->assign((size_t)width_ * height_, 0);
    dvo_amd_pyramid *filtered = nullptr;
    detail::check(dvo_amd_pyramid_filter_depth(handle_, &options, &filtered, &record.with_depth, support ? support->data() : nullptr), where);
    Ptr out;
    try {
      out = Ptr(new RgbdImagePyramid(filtered, width_, height_, K_, device_, timestamp_));
    } catch (...) {
      dvo_amd_pyramid_release(filtered);
      throw;
    }
    if (counts) *counts = record;
    return out;
  }

  // (not in the reference, which assumes constant brightness) The gain and bias with which THIS frame, the current one, looks like
  // `reference`: I_ref ~ gain * I_cur + bias over the pixels both see, by trimmed least squares on the device (dvo_amd.h, "Exposure
  // compensation").  estimate: reference -> current, what computeIntensityErrorImage takes and the inverse of what match() returns;
  // null is the identity.  mask: on the reference's pixels, or null.  Both pyramids are built up to options.level.  context: a
  // tracker's (DenseTracker::handle()), which gives its device and nothing else; null takes the shared one of the point clouds.
  ExposureEstimate estimateExposure(RgbdImagePyramid &reference, const AffineTransformd *estimate = nullptr, const SelectionMask *mask = nullptr,
                                    const ExposureOptions &options = ExposureOptions(), dvo_amd_context *context = nullptr);

  // This frame with level 0's intensity mapped to (gain * I) + bias, not clamped, on the device: a new pyramid of this one's depth,
  // size, intrinsics, level count and timestamp; this one is only read and must hold its levels (RgbdImagePyramid::build).
  Ptr adjustIntensity(double gain, double bias) const {
    dvo_amd_pyramid *made = nullptr;
    detail::check(dvo_amd_pyramid_adjust_intensity(handle_, gain, bias, &made), "RgbdImagePyramid::adjustIntensity");
    try {
      return Ptr(new RgbdImagePyramid(made, width_, height_, K_, device_, timestamp_));
    } catch (...) {
      dvo_amd_pyramid_release(made);
      throw;
    }
  }

  // RgbdImage::warpIntensity / warpIntensitySse and warpIntensityForward / warpDepthForward / warpDepthForwardAdvanced
  // (rgbd_image.cpp:545-781) on the device, operation by operation as dvo_amd.h pins them ("Frame warps").  THIS frame is the
  // moving one, whose grey values travel.  transformation: moving camera -> fixed camera; for tracker.match(fixed, *this, result)
  // that is result.Transformation as returned.  All pyramids must hold their levels (RgbdImagePyramid::build; a match has built
  // them).
  struct WarpOptions : dvo_amd_warp_options {
    WarpOptions() { dvo_amd_default_warp_options(this); }
  };
  struct WarpInverseCounts {
    long long valid, behind, outside, border, hidden, warped, partial, no_depth;
  };
  struct WarpForwardCounts {
    long long valid, behind, outside, too_large, drawn, covered_pixels, no_depth;
  };
  // one level's planes, row-major; index only from warpForward (-1: empty; empty intensity and depth are NaN)
  struct WarpedPlanes {
    int width, height;
    std::vector<float> intensity, depth;
    std::vector<int> index;
  };
  // the inverse warp (a gather): this frame's grey values on the pixels of level `level` of `fixed`
  WarpedPlanes warpInverse(const RgbdImagePyramid &fixed, const AffineTransformd &transformation, int level,
                           const WarpOptions &options = WarpOptions(), WarpInverseCounts *counts = nullptr) const {
    static_assert(sizeof(WarpInverseCounts) == DVO_AMD_WARP_INVERSE_COUNTS * sizeof(long long), "the count record is dvo_amd_warp_inverse's");
    const char *where = "RgbdImagePyramid::warpInverse";
    WarpedPlanes out;
    float k[4];
    detail::check(dvo_amd_pyramid_level_info(fixed.handle_, level, &out.width, &out.height, k), where);
    out.intensity.resize((size_t)out.width * out.height), out.depth.resize((size_t)out.width * out.height);
    WarpInverseCounts record;
    detail::check(dvo_amd_warp_inverse(fixed.handle_, handle_, data(transformation), level, &options, out.intensity.data(), out.depth.data(),
                                       &record.valid),
                  where);
    if (counts) *counts = record;
    return out;
  }
  // ... as a pyramid like `fixed` (its size, intrinsics, level count and timestamp) in which only warped pixels have a depth
  Ptr warpInverse(const RgbdImagePyramid &fixed, const AffineTransformd &transformation, const WarpOptions &options = WarpOptions(),
                  WarpInverseCounts *counts = nullptr) const {
    WarpInverseCounts record;
    dvo_amd_pyramid *made = nullptr;
    detail::check(dvo_amd_pyramid_warp_inverse(fixed.handle_, handle_, data(transformation), &options, &made, &record.valid),
                  "RgbdImagePyramid::warpInverse");
    if (counts) *counts = record;
    try {
      return Ptr(new RgbdImagePyramid(made, fixed.width_, fixed.height_, fixed.K_, device_, fixed.timestamp_));
    } catch (...) {
      dvo_amd_pyramid_release(made);
      throw;
    }
  }
  // the forward warp (a scatter with a nearest-depth test): this frame's level `level` drawn into `view` (null: this frame's own
  // camera at that level)
  WarpedPlanes warpForward(const AffineTransformd &transformation, const dvo_amd_view *view, int level,
                           const WarpOptions &options = WarpOptions(), WarpForwardCounts *counts = nullptr) const {
    static_assert(sizeof(WarpForwardCounts) == DVO_AMD_WARP_FORWARD_COUNTS * sizeof(long long), "the count record is dvo_amd_warp_forward's");
    const char *where = "RgbdImagePyramid::warpForward";
    WarpedPlanes out;
    if (view) {
      out.width = view->width > 0 ? view->width : 0, out.height = view->height > 0 ? view->height : 0;  // (the library refuses the rest)
    } else {
      float k[4];
      detail::check(dvo_amd_pyramid_level_info(handle_, level, &out.width, &out.height, k), where);
    }
    const size_t n = (size_t)out.width * out.height;
    out.intensity.resize(n), out.depth.resize(n), out.index.resize(n);
    WarpForwardCounts record;
    detail::check(dvo_amd_warp_forward(handle_, data(transformation), view, level, &options, out.depth.data(), out.intensity.data(),
                                       out.index.data(), &record.valid),
                  where);
    if (counts) *counts = record;
    return out;
  }
  // ... as a pyramid of the view with this frame's level count and timestamp
  Ptr warpForward(const AffineTransformd &transformation, const dvo_amd_view *view = nullptr, const WarpOptions &options = WarpOptions(),
                  WarpForwardCounts *counts = nullptr) const {
    WarpForwardCounts record;
    dvo_amd_pyramid *made = nullptr;
    detail::check(dvo_amd_pyramid_warp_forward(handle_, data(transformation), view, &options, &made, &record.valid),
                  "RgbdImagePyramid::warpForward");
    if (counts) *counts = record;
    try {
      return view ? Ptr(new RgbdImagePyramid(made, view->width, view->height, IntrinsicMatrix::create(view->fx, view->fy, view->ox, view->oy),
                                             device_, timestamp_))
                  : Ptr(new RgbdImagePyramid(made, width_, height_, K_, device_, timestamp_));
    } catch (...) {
      dvo_amd_pyramid_release(made);
      throw;
    }
  }

  double timestamp() const { return timestamp_; }
  int device() const { return device_; }
  int width() const { return width_; }
  int height() const { return height_; }
  dvo_amd_pyramid *handle() const { return handle_; }

 private:
  int width_, height_;
  IntrinsicMatrix K_;
  int device_;
  double timestamp_;
  std::vector<float> intensity_, depth_;
  dvo_amd_pyramid *handle_;
  int levels_;
  RgbdImage level_views_[DVO_AMD_MAX_LEVELS];
};
typedef RgbdImagePyramid::Ptr RgbdImagePyramidPtr;

inline std::vector<float> RgbdImage::plane(int which) const {
  if (!owner_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::plane");
  std::vector<float> out(width * height);
  detail::check(dvo_amd_pyramid_download_plane(owner_->handle(), level_, which, out.data()), "RgbdImage::plane");
  return out;
}

namespace cloud {
// The context the adaptor's point-cloud calls run in when the caller has no DenseTracker to hand (RgbdImage::pointcloud, the
// map builder of point_cloud.hpp): one per device, created on first use and kept for the life of the process with the buffers
// of the largest cloud it built.  A context is not thread-safe: callers hold the returned lock for the duration of the call.
inline dvo_amd_context *context(int device, std::unique_lock<std::mutex> &lock) {
  static std::mutex mu;
  static dvo_amd_context *ctx[DVO_AMD_MAX_DEVICES_FOR_CLOUDS] = {};
  if (device < 0 || device >= DVO_AMD_MAX_DEVICES_FOR_CLOUDS) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "cloud_context");
  lock = std::unique_lock<std::mutex>(mu);
  if (!ctx[device]) ::dvo::detail::check(dvo_amd_context_create(device, nullptr, &ctx[device]), "cloud_context");
  return ctx[device];
}
}  // namespace cloud

inline long PointCloudMatrix::cols() const {
  fill();
  return (long)(xyzw_.size() / 4);
}
inline const float *PointCloudMatrix::data() const {
  fill();
  return xyzw_.data();
}
inline void PointCloudMatrix::fill() const {
  if (filled_) return;
  if (!owner_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::pointcloud");
  int w = 0, h = 0;
  ::dvo::detail::check(dvo_amd_pyramid_level_info(owner_->handle(), level_, &w, &h, nullptr), "RgbdImage::pointcloud");
  std::vector<dvo_amd_point> pts((size_t)w * h);
  {
    std::unique_lock<std::mutex> lock;
    dvo_amd_context *ctx = cloud::context(owner_->device(), lock);
    ::dvo::detail::check(dvo_amd_point_cloud(ctx, owner_->handle(), level_, nullptr, nullptr, 0, pts.data()), "RgbdImage::pointcloud");
  }
  xyzw_.resize(pts.size() * 4);
  for (size_t p = 0; p < pts.size(); ++p)
    xyzw_[4 * p] = pts[p].x, xyzw_[4 * p + 1] = pts[p].y, xyzw_[4 * p + 2] = pts[p].z, xyzw_[4 * p + 3] = 1.0f;
  filled_ = true;
}

inline void NormalPlane::fill() const {
  if (filled_) return;
  if (!owner_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::normals");
  int w = 0, h = 0;
  ::dvo::detail::check(dvo_amd_pyramid_level_info(owner_->handle(), level_, &w, &h, nullptr), "RgbdImage::normals");
  values_.resize((size_t)w * h * channels_);
  dvo_amd_normal_options o;
  dvo_amd_default_normal_options(&o);
  ::dvo::detail::check(dvo_amd_pyramid_normals(owner_->handle(), level_, &o, channels_ == 4 ? values_.data() : nullptr,
                                               channels_ == 4 ? nullptr : values_.data(), nullptr),
                       "RgbdImage::calculateNormals");
  rows_ = h, cols_ = w;
  filled_ = true;
}
inline long NormalPlane::rows() const {
  fill();
  return rows_;
}
inline long NormalPlane::cols() const {
  fill();
  return cols_;
}
inline const float *NormalPlane::data() const {
  fill();
  return values_.data();
}
inline void RgbdImage::calculateNormals() {
#ifdef DVO_AMD_HAVE_OPENCV
  if (!owner_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::calculateNormals");
  if (!normals.empty() && !angles.empty()) return;  // (rgbd_image.cpp:504: computed once)
  cv::Mat n((int)height, (int)width, CV_MAKETYPE(CV_32F, 4)), a((int)height, (int)width, CV_MAKETYPE(CV_32F, 1));
  dvo_amd_normal_options o;
  dvo_amd_default_normal_options(&o);
  ::dvo::detail::check(dvo_amd_pyramid_normals(owner_->handle(), level_, &o, n.ptr<float>(), a.ptr<float>(), nullptr),
                       "RgbdImage::calculateNormals");
  normals = n, angles = a;
#else
  (void)normals.data(), (void)angles.data();
#endif
}

// rgbd_image.h:39-89: the 48-byte record PointSelection::select hands out ({x, y, z, 1; I, Z, Ix, Iy, Zx, Zy, 0, 0})
struct PointWithIntensityAndDepth {
  union Point {
    float data[4];
    struct {
      float x, y, z;
    };
  };
  union IntensityAndDepth {
    float data[8];
    struct {
      float i, z, idx, idy, zdx, zdy, time_interpolation;
    };
  };
  typedef std::vector<PointWithIntensityAndDepth> VectorType;
  Point point;
  IntensityAndDepth intensity_and_depth;
};

// (not in the reference) A selection mask on the device (dvo_amd_mask): which reference pixels may take part, one byte plane per
// pyramid level, 1 = keep.  RAII over the C ABI, shared by value (shared ownership of one device object, like
// dvo::core::Rectification): a predicate hands one out through deviceMask(), a selection built behind it outlives it.
class SelectionMask {
 public:
  enum Rule { All = DVO_AMD_MASK_ALL, Any = DVO_AMD_MASK_ANY };
  SelectionMask() : device_(0) {}  // empty: valid() is false

  // level 0 given (stride in bytes, 0 = packed; on_device: device memory of `device`, e.g. a segmentation network's output), the
  // coarser levels derived on the device: a pixel is kept iff all (All) or any (Any) of the four pixels under it are kept
  static SelectionMask fromLevel0(int width, int height, int levels, const unsigned char *mask0, int stride = 0, Rule rule = All,
                                  int device = 0, bool on_device = false) {
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_create(device, width, height, levels, mask0, stride ? stride : width, on_device ? 1 : 0, (int)rule, &m),
                  "SelectionMask::fromLevel0");
    return SelectionMask(m, device);
  }
  // every level given: planes[l] holds (width >> l) x (height >> l) bytes, packed
  static SelectionMask fromLevels(int width, int height, const std::vector<std::vector<unsigned char> > &planes, int device = 0) {
    std::vector<const unsigned char *> ptr(planes.size());
    std::vector<int> strides(planes.size());
    for (size_t l = 0; l < planes.size(); ++l) {
      if (planes[l].size() != (size_t)(width >> l) * (size_t)(height >> l))
        throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SelectionMask::fromLevels");
      ptr[l] = planes[l].data(), strides[l] = width >> l;
    }
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_create_levels(device, width, height, (int)planes.size(), ptr.data(), strides.data(), 0, &m),
                  "SelectionMask::fromLevels");
    return SelectionMask(m, device);
  }

  // A point budget, ranked on the device from the resident pyramid (dvo_amd_mask_create_budget; the rules are pinned in
  // dvo_amd.h).  A candidate passes the threshold predicate and, if given, `within`; its strength is
  // Ix^2 + Iy^2 + depth_weight * (Zx^2 + Zy^2), ties go to the lowest pixel index.
  //   topK   level l keeps its budgets[l] strongest candidates (negative, or no entry for the level: every candidate)
  //   grid   level l keeps the strongest candidate of every cells[l] x cells[l] cell (no entry for the level: 1, every candidate)
  // The pyramid is built to at least budgets.size() / cells.size() levels first (RgbdImagePyramid::build); the mask has the
  // levels the pyramid has then, so build the levels the tracker will use before asking for the mask.
  static SelectionMask topK(RgbdImagePyramid &pyramid, const std::vector<long long> &budgets, float intensity_threshold = 0.0f,
                            float depth_threshold = 0.0f, float depth_weight = 0.0f, const SelectionMask *within = nullptr) {
    dvo_amd_budget_options o;
    dvo_amd_default_budget_options(&o);
    o.rule = DVO_AMD_BUDGET_TOPK;
    for (size_t l = 0; l < budgets.size() && l < (size_t)DVO_AMD_MAX_LEVELS; ++l) o.budget[l] = budgets[l];
    pyramid.build(std::max<size_t>(budgets.size(), 1));
    return budget(pyramid, o, intensity_threshold, depth_threshold, depth_weight, within, "SelectionMask::topK");
  }
  static SelectionMask grid(RgbdImagePyramid &pyramid, const std::vector<int> &cells, float intensity_threshold = 0.0f,
                            float depth_threshold = 0.0f, float depth_weight = 0.0f, const SelectionMask *within = nullptr) {
    dvo_amd_budget_options o;
    dvo_amd_default_budget_options(&o);
    o.rule = DVO_AMD_BUDGET_GRID;
    for (size_t l = 0; l < cells.size() && l < (size_t)DVO_AMD_MAX_LEVELS; ++l) o.cell[l] = cells[l];
    pyramid.build(std::max<size_t>(cells.size(), 1));
    return budget(pyramid, o, intensity_threshold, depth_threshold, depth_weight, within, "SelectionMask::grid");
  }

  // Masks from masks, on the device (dvo_amd.h, "Mask operations"): every result is a new mask, the operands are only read.
  //   a & b, a | b, ~a, a.andNot(b)   level by level; a and b of one size and level count
  //   dilated(r) / eroded(r)          by the square of edge 2 r + 1 clipped to the plane; r in pixels of level 0 (level l gets
  //                                   r / 2^l rounded up) or one radius per level; every level on its own
  //   warped(source, target, T)       this mask, on the pixels of `source`, carried onto the pixels of `target`: T maps points of
  //                                   the target camera frame into the source camera frame -- for tracker.match(source, target,
  //                                   result) that is result.Transformation as returned.  Both pyramids must hold their levels
  //                                   (RgbdImagePyramid::build; a match has built them); the result has the target's.
  SelectionMask operator&(const SelectionMask &other) const { return combine(&other, DVO_AMD_MASK_AND, "SelectionMask::operator&"); }
  SelectionMask operator|(const SelectionMask &other) const { return combine(&other, DVO_AMD_MASK_OR, "SelectionMask::operator|"); }
  SelectionMask operator~() const { return combine(nullptr, DVO_AMD_MASK_NOT, "SelectionMask::operator~"); }
  SelectionMask andNot(const SelectionMask &other) const { return combine(&other, DVO_AMD_MASK_ANDNOT, "SelectionMask::andNot"); }
  SelectionMask dilated(int radius) const { return morph(DVO_AMD_MASK_DILATE, levelRadii(radius), "SelectionMask::dilated"); }
  SelectionMask dilated(const std::vector<int> &radii) const { return morph(DVO_AMD_MASK_DILATE, radii, "SelectionMask::dilated"); }
  SelectionMask eroded(int radius) const { return morph(DVO_AMD_MASK_ERODE, levelRadii(radius), "SelectionMask::eroded"); }
  SelectionMask eroded(const std::vector<int> &radii) const { return morph(DVO_AMD_MASK_ERODE, radii, "SelectionMask::eroded"); }

  struct WarpOptions : dvo_amd_mask_warp_options {
    WarpOptions() { dvo_amd_default_mask_warp_options(this); }
  };
  struct WarpCounts {  // one level's record
    long long valid, behind, outside, no_depth, consistent, occluded, seen_through, dropped_by_source;
  };
  SelectionMask warped(const RgbdImagePyramid &source, const RgbdImagePyramid &target, const AffineTransformd &transformation,
                       const WarpOptions &options = WarpOptions(), std::vector<WarpCounts> *counts = nullptr) const {
    static_assert(sizeof(WarpCounts) == 8 * sizeof(long long), "a WarpCounts is one record of dvo_amd_mask_warp's counts");
    WarpCounts records[DVO_AMD_MAX_LEVELS];
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_warp(need(), source.handle(), target.handle(), data(transformation), &options, &m, &records[0].valid),
                  "SelectionMask::warped");
    SelectionMask out(m, target.device());
    if (counts) counts->assign(records, records + out.info().levels);
    return out;
  }

  // A mask from what the tracker itself knows (dvo_amd.h, "Residual masks"): the pixels of `reference` whose residuals against
  // `current` are inliers of the t-distribution -- valid, and with a Mahalanobis distance of at most maxDistance (default: the
  // 99 % point of chi-square with two degrees of freedom) under the level's precision -- at the estimate of
  // tracker.match(reference, current, result).  match() returns the inverse of its estimate (dense_tracking.cpp:371), so the
  // estimate passed on is the rigid inverse of result.Transformation (rigidInverse below).  The precision of level l is the
  // TDistributionPrecision of the last iteration of that level in result.Statistics; a level the match did not run (level 0
  // under the default configuration) takes the nearest level that ran, ties to the finer one.  Throws INVALID_ARGUMENT if the
  // result holds no iteration at all.  Both pyramids hold their levels (the match has built them); the mask has the reference's.
  // Tracker: dvo::DenseTracker, MatchResult: dvo::DenseTracker::Result (templates only because both are declared further down).
  struct ResidualCounts {  // one level's record
    long long evaluated, invalid, inlier, outlier, kept;
  };
  template <class Tracker, class MatchResult>
  static SelectionMask fromResiduals(const Tracker &tracker, const RgbdImagePyramid &reference, const RgbdImagePyramid &current,
                                     const MatchResult &result, float maxDistance = 9.2103f, bool invalidKeep = false,
                                     bool unevaluatedKeep = false, std::vector<ResidualCounts> *counts = nullptr) {
    static_assert(sizeof(ResidualCounts) == DVO_AMD_RESIDUAL_MASK_COUNTS * sizeof(long long),
                  "a ResidualCounts is one record of dvo_amd_mask_from_residuals' counts");
    const char *where = "SelectionMask::fromResiduals";
    dvo_amd_residual_mask_options o;
    dvo_amd_default_residual_mask_options(&o);
    const int levels = dvo_amd_pyramid_levels(reference.handle());
    for (int l = 0; l < levels && l < DVO_AMD_MAX_LEVELS; ++l) {
      long best = -1, best_distance = 0;
      for (size_t i = 0; i < result.Statistics.Levels.size(); ++i) {
        if (result.Statistics.Levels[i].Iterations.empty()) continue;
        const long id = (long)result.Statistics.Levels[i].Id, distance = id > l ? id - l : l - id;
        if (best < 0 || distance < best_distance || (distance == best_distance && id < (long)result.Statistics.Levels[(size_t)best].Id))
          best = (long)i, best_distance = distance;
      }
      if (best < 0) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
      const Matrix2d &P = result.Statistics.Levels[(size_t)best].Iterations.back().TDistributionPrecision;
      for (int i = 0; i < 4; ++i) o.precision[l][i] = (float)P(i % 2, i / 2);  // column-major
      o.max_distance[l] = maxDistance;
    }
    o.invalid_keep = invalidKeep ? 1 : 0, o.unevaluated_keep = unevaluatedKeep ? 1 : 0;
    const AffineTransformd estimate = rigidInverse(result.Transformation);
    ResidualCounts records[DVO_AMD_MAX_LEVELS];
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_from_residuals(tracker.handle(), reference.handle(), current.handle(), data(estimate), &o, &m,
                                              &records[0].evaluated, nullptr),
                  where);
    SelectionMask out(m, reference.device());
    if (counts) counts->assign(records, records + out.info().levels);
    return out;
  }
  // A mask from which way the surfaces face (dvo_amd.h, "Surface normals"): the pixels of `pyramid` whose normal is defined and
  // whose facing value is at least minFacing[l] on level l (no entry for the level: the last entry); a pixel without a normal is
  // kept iff undefinedKeep.  The pixels it drops are the ones seen at a grazing angle, where depth noise and flying pixels are
  // worst.  The pyramid holds its levels (RgbdImagePyramid::build); the mask has the pyramid's, every level from one launch.
  struct NormalOptions : dvo_amd_normal_options {
    NormalOptions() { dvo_amd_default_normal_options(this); }
  };
  struct NormalCounts {  // one level's record
    long long defined, undefined, kept;
  };
  static SelectionMask fromNormals(const RgbdImagePyramid &pyramid, const std::vector<float> &minFacing,
                                   const NormalOptions &options = NormalOptions(), bool undefinedKeep = false,
                                   std::vector<NormalCounts> *counts = nullptr) {
    static_assert(sizeof(NormalCounts) == 3 * sizeof(long long), "a NormalCounts is one record of dvo_amd_mask_from_normals' counts");
    if (minFacing.empty()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SelectionMask::fromNormals");
    float min_facing[DVO_AMD_MAX_LEVELS];
    for (size_t l = 0; l < (size_t)DVO_AMD_MAX_LEVELS; ++l) min_facing[l] = minFacing[std::min(l, minFacing.size() - 1)];
    NormalCounts records[DVO_AMD_MAX_LEVELS];
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_from_normals(pyramid.handle(), &options, min_facing, undefinedKeep ? 1 : 0, &m, &records[0].defined),
                  "SelectionMask::fromNormals");
    SelectionMask out(m, pyramid.device());
    if (counts) counts->assign(records, records + out.info().levels);
    return out;
  }
  // Connected components (dvo_amd.h, "Mask components"): what tells a 3-pixel speckle from a 3000-pixel object.
  //   filterComponents(options, depth, seeds)   the components of this mask -- cut further by the depth rule where `depth` is
  //                                             given -- that pass the options' area band, touch `seeds` where given and are
  //                                             among the keep_largest largest where asked
  //   reconstruct(seeds)                        the components `seeds` still touches: with seeds = eroded(r), an erosion's speckle
  //                                             removal without its loss of shape
  //   components(level, labels, ...)            one level's records in ascending root order, and its label plane (root + 1, 0 =
  //                                             background) where `labels` is given
  //   depthComponents(pyramid, options, seeds)  the mask-less form: the depth-connected surfaces of a pyramid
  // A pyramid holds its levels (RgbdImagePyramid::build; a match has built them).
  struct ComponentOptions : dvo_amd_component_options {
    ComponentOptions() { dvo_amd_default_component_options(this); }
    // an area in pixels of level 0 on every level, max(1, ceil(a0 / 4^l)): level l has a quarter of the pixels of level l - 1
    static int levelArea(int a0, int level) {
      const long long q = 1ll << (2 * level), a = ((long long)a0 + q - 1) / q;
      return a < 1 ? 1 : (int)a;
    }
    ComponentOptions &minArea(int a0) {
      for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) min_area[l] = levelArea(a0, l);
      return *this;
    }
    ComponentOptions &maxArea(int a0) {
      for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) max_area[l] = levelArea(a0, l);
      return *this;
    }
  };
  struct ComponentCounts {  // one level's record
    long long foreground, components, kept_components, kept_pixels, largest_area, edges_cut;
  };
  typedef dvo_amd_component Component;
  SelectionMask filterComponents(const ComponentOptions &options = ComponentOptions(), const RgbdImagePyramid *depth = nullptr,
                                 const SelectionMask *seeds = nullptr, std::vector<ComponentCounts> *counts = nullptr) const {
    return filtered(need(), depth, seeds, options, device_, counts, "SelectionMask::filterComponents");
  }
  SelectionMask reconstruct(const SelectionMask &seeds) const {
    return filtered(need(), nullptr, &seeds, ComponentOptions(), device_, nullptr, "SelectionMask::reconstruct");
  }
  static SelectionMask depthComponents(const RgbdImagePyramid &pyramid, const ComponentOptions &options = ComponentOptions(),
                                       const SelectionMask *seeds = nullptr, std::vector<ComponentCounts> *counts = nullptr) {
    return filtered(nullptr, &pyramid, seeds, options, pyramid.device(), counts, "SelectionMask::depthComponents");
  }
  std::vector<Component> components(int level, std::vector<int> *labels = nullptr, const ComponentOptions &options = ComponentOptions(),
                                    const RgbdImagePyramid *depth = nullptr, const SelectionMask *seeds = nullptr) const {
    const char *where = "SelectionMask::components";
    const Info i = info();
    if (level < 0 || level >= i.levels) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
    if (labels) labels->assign((size_t)(i.width >> level) * (size_t)(i.height >> level), 0);
    // one call with room for 4096 records; a second one, for the records alone, only when the level has more components
    std::vector<Component> records(4096);
    int n = 0;
    detail::check(dvo_amd_mask_components(need(), depth ? depth->handle() : nullptr, seeds ? seeds->need() : nullptr, &options, level,
                                          labels ? labels->data() : nullptr, records.data(), (int)records.size(), &n),
                  where);
    if ((size_t)n > records.size()) {
      records.resize((size_t)n);
      detail::check(dvo_amd_mask_components(need(), depth ? depth->handle() : nullptr, seeds ? seeds->need() : nullptr, &options, level,
                                            nullptr, records.data(), n, &n),
                    where);
    }
    records.resize((size_t)n);
    return records;
  }

  // (R^T, -R^T t) of a rigid transformation, every sum in this order: the inverse the Python binding and the C example form too,
  // so that all three hand the library the same sixteen doubles
  static AffineTransformd rigidInverse(const AffineTransformd &transformation) {
    const double *t = data(transformation);  // column-major
    AffineTransformd inverse;
    inverse.setIdentity();
    double *o = data(inverse);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) o[j * 4 + i] = t[i * 4 + j];
      o[12 + i] = -((t[i * 4 + 0] * t[12] + t[i * 4 + 1] * t[13]) + t[i * 4 + 2] * t[14]);
    }
    return inverse;
  }

  bool valid() const { return (bool)handle_; }
  dvo_amd_mask *handle() const { return handle_.get(); }
  int device() const { return device_; }

  struct Info {
    int width, height, levels;
    long long kept[DVO_AMD_MAX_LEVELS];  // kept pixels per level
  };
  Info info() const {
    Info i;
    std::memset(&i, 0, sizeof(i));
    detail::check(dvo_amd_mask_info(need(), &i.width, &i.height, &i.levels, i.kept), "SelectionMask::info");
    return i;
  }
  std::vector<unsigned char> download(int level) const {
    const Info i = info();
    if (level < 0 || level >= i.levels) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SelectionMask::download");
    std::vector<unsigned char> out((size_t)(i.width >> level) * (size_t)(i.height >> level));
    detail::check(dvo_amd_mask_download(need(), level, out.data()), "SelectionMask::download");
    return out;
  }

 private:
  struct Release {
    void operator()(dvo_amd_mask *m) const { dvo_amd_mask_release(m); }
  };
  SelectionMask(dvo_amd_mask *m, int device) : handle_(m, Release()), device_(device) {}
  static SelectionMask budget(const RgbdImagePyramid &pyramid, dvo_amd_budget_options &o, float intensity_threshold,
                              float depth_threshold, float depth_weight, const SelectionMask *within, const char *where) {
    o.intensity_threshold = intensity_threshold, o.depth_threshold = depth_threshold, o.depth_weight = depth_weight;
    o.within = within ? within->need() : nullptr;
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_create_budget(pyramid.handle(), &o, &m), where);
    return SelectionMask(m, pyramid.device());
  }
  static SelectionMask filtered(const dvo_amd_mask *mask, const RgbdImagePyramid *depth, const SelectionMask *seeds,
                                const ComponentOptions &options, int device, std::vector<ComponentCounts> *counts, const char *where) {
    static_assert(sizeof(ComponentCounts) == DVO_AMD_COMPONENTS_COUNTS * sizeof(long long),
                  "a ComponentCounts is one record of dvo_amd_mask_filter_components' counts");
    ComponentCounts records[DVO_AMD_MAX_LEVELS];
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_filter_components(mask, depth ? depth->handle() : nullptr, seeds ? seeds->need() : nullptr, &options, &m,
                                                 &records[0].foreground),
                  where);
    SelectionMask out(m, device);
    if (counts) counts->assign(records, records + out.info().levels);
    return out;
  }
  SelectionMask combine(const SelectionMask *other, int op, const char *where) const {
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_combine(need(), other ? other->need() : nullptr, op, &m), where);
    return SelectionMask(m, device_);
  }
  SelectionMask morph(int op, const std::vector<int> &radii, const char *where) const {
    int r[DVO_AMD_MAX_LEVELS] = {0};
    if (radii.size() < (size_t)info().levels) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
    for (size_t l = 0; l < radii.size() && l < (size_t)DVO_AMD_MAX_LEVELS; ++l) r[l] = radii[l];
    dvo_amd_mask *m = nullptr;
    detail::check(dvo_amd_mask_morph(need(), op, r, &m), where);
    return SelectionMask(m, device_);
  }
  // a radius in pixels of level 0 on every level: (r0 + (1 << l) - 1) >> l
  static std::vector<int> levelRadii(int r0) {
    std::vector<int> r(DVO_AMD_MAX_LEVELS);
    for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) r[l] = (r0 + (1 << l) - 1) >> l;
    return r;
  }
  dvo_amd_mask *need() const {
    if (!handle_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SelectionMask: empty");
    return handle_.get();
  }
  std::shared_ptr<dvo_amd_mask> handle_;
  int device_;
};

// point_selection.h:32-67.  The selection runs on the GPU.  A predicate says how in one of three ways:
//   deviceThresholds()   the two gradient thresholds of the reference's own predicates: evaluated by the select kernel
//   deviceMask()         a SelectionMask the predicate holds (next to its thresholds, or -1 / -1 if it has none): the kernel
//                        keeps a pixel iff the mask does and the threshold predicate does
//   neither              any user-defined predicate, as a caller of the reference writes it.  PointSelection then evaluates
//                        isPointOk(x, y, z, idx, idy, zdx, zdy) itself, on the host: once per pyramid and per level in use it
//                        downloads the level's six planes, calls the predicate for every pixel in scan order, and uploads the
//                        answers as a mask (dvo_amd_mask_create_levels) that it keeps until setRgbdImagePyramid / recycle --
//                        when the reference drops its own cache.  The cost is that host pass over the planes, once per
//                        pyramid; the alignment itself runs on the device as always, behind that mask with thresholds -1 / -1.
// One deviation, for the two mask forms: a pixel with NaN z, zdx or zdy is never selected, whatever the predicate says (the
// reference would put a point its predicate admits into the point list, NaN or not).
class PointSelectionPredicate {
 public:
  virtual ~PointSelectionPredicate() {}
  virtual bool isPointOk(const size_t &x, const size_t &y, const float &z, const float &idx, const float &idy, const float &zdx,
                         const float &zdy) const = 0;
  virtual bool deviceThresholds(float &intensity_threshold, float &depth_threshold) const {
    (void)intensity_threshold, (void)depth_threshold;
    return false;
  }
  virtual const SelectionMask *deviceMask() const { return nullptr; }
};

class ValidPointPredicate : public PointSelectionPredicate {
 public:
  virtual ~ValidPointPredicate() {}
  virtual bool isPointOk(const size_t &, const size_t &, const float &z, const float &, const float &, const float &zdx,
                         const float &zdy) const {
    return z == z && zdx == zdx && zdy == zdy;
  }
  // |zdx| > -1 holds for every non-NaN zdx: thresholds of -1 leave exactly the validity part of the test
  virtual bool deviceThresholds(float &ti, float &td) const {
    ti = -1.0f, td = -1.0f;
    return true;
  }
};

class ValidPointAndGradientThresholdPredicate : public PointSelectionPredicate {
 public:
  float intensity_threshold;
  float depth_threshold;
  ValidPointAndGradientThresholdPredicate() : intensity_threshold(0.0f), depth_threshold(0.0f) {}
  virtual ~ValidPointAndGradientThresholdPredicate() {}
  virtual bool isPointOk(const size_t &, const size_t &, const float &z, const float &idx, const float &idy, const float &zdx,
                         const float &zdy) const {
    return z == z && zdx == zdx && zdy == zdy &&
           (std::abs(idx) > intensity_threshold || std::abs(idy) > intensity_threshold || std::abs(zdx) > depth_threshold ||
            std::abs(zdy) > depth_threshold);
  }
  virtual bool deviceThresholds(float &ti, float &td) const {
    ti = intensity_threshold, td = depth_threshold;
    return true;
  }
};

// (not in the reference) a device mask and the two gradient thresholds: keep = mask && ValidPointAndGradientThresholdPredicate.
// isPointOk is the threshold part alone -- the call does not say which level a pixel belongs to, so the mask part exists on the
// device only; PointSelection never calls it for a predicate that has a device form.
class MaskedGradientThresholdPredicate : public ValidPointAndGradientThresholdPredicate {
 public:
  SelectionMask mask;
  MaskedGradientThresholdPredicate() {}
  explicit MaskedGradientThresholdPredicate(const SelectionMask &m, float intensity = 0.0f, float depth = 0.0f) : mask(m) {
    intensity_threshold = intensity, depth_threshold = depth;
  }
  virtual ~MaskedGradientThresholdPredicate() {}
  virtual const SelectionMask *deviceMask() const { return mask.valid() ? &mask : nullptr; }
};

// point_selection.h:70-117.  The reference caches the compacted 48-byte records per level until setRgbdImagePyramid(); here
// the selection lives with the device pyramid (a NaN-masked depth plane per threshold pair, cached for the pyramid's
// lifetime), so this class only carries the pyramid pointer and the predicate -- and, for a predicate without a device form,
// the predicate's answers as a device mask (hostMask).  select() materialises host records for callers that want to look at
// them; match() never does.
class PointSelection {
 public:
  typedef PointWithIntensityAndDepth::VectorType PointVector;
  typedef PointVector::iterator PointIterator;

  explicit PointSelection(const PointSelectionPredicate &predicate) : pyramid_(nullptr), predicate_(predicate), debug_(false) {}
  PointSelection(RgbdImagePyramid &pyramid, const PointSelectionPredicate &predicate)
      : pyramid_(&pyramid), predicate_(predicate), debug_(false) {}
  virtual ~PointSelection() {}

  RgbdImagePyramid &getRgbdImagePyramid() {
    if (!pyramid_) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "PointSelection::getRgbdImagePyramid");  // assert(pyramid_ != 0)
    return *pyramid_;
  }
  void setRgbdImagePyramid(RgbdImagePyramid &pyramid) {
    pyramid_ = &pyramid;
    storage_.clear();  // point_selection.cpp:51-59: the cache belongs to the previous pyramid
    host_mask_ = SelectionMask(), host_planes_.clear(), host_mask_of_ = nullptr;  // ... and so does a host-evaluated mask
  }
  void recycle(RgbdImagePyramid &pyramid) { setRgbdImagePyramid(pyramid); }

  // point_selection.cpp:68-71
  size_t getMaximumNumberOfPoints(const size_t &level) {
    RgbdImagePyramid &p = getRgbdImagePyramid();
    return size_t((double)((size_t)p.width() * (size_t)p.height()) * std::pow(0.25, double(level)));
  }

  // the thresholds of a predicate that is its two thresholds and nothing else (throws for any other: see deviceForm)
  void thresholds(float &ti, float &td) const {
    if (predicate_.deviceMask() || !predicate_.deviceThresholds(ti, td))
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "PointSelection: predicate is not a threshold pair (deviceForm)");
  }

  // What the device selection of levels first_level..last_level of the pyramid runs with: a mask (null: none) and the two
  // thresholds.  A predicate without a device form is evaluated here, on the host, for the levels asked for that have not been
  // evaluated for this pyramid yet (PointSelectionPredicate's comment); the pyramid must hold the levels already.
  void deviceForm(size_t first_level, size_t last_level, const SelectionMask *&mask, float &ti, float &td) {
    mask = predicate_.deviceMask();
    if (predicate_.deviceThresholds(ti, td)) return;
    ti = -1.0f, td = -1.0f;
    if (mask) return;
    mask = &hostMask(first_level, last_level);
  }

  // number of selected pixels of a level (the distance last_point - first_point of select())
  size_t size(const size_t &level) {
    RgbdImagePyramid &p = getRgbdImagePyramid();
    p.build(level + 1);
    const SelectionMask *m;
    float ti, td;
    deviceForm(level, level, m, ti, td);
    int count = 0;
    detail::check(dvo_amd_pyramid_select_masked(p.handle(), (int)level, ti, td, m ? m->handle() : nullptr, &count, nullptr),
                  "PointSelection::size");
    return (size_t)count;
  }

  // point_selection.cpp:89-152: row-major scan, predicate, 48-byte records.  Host copy, built on demand and cached per level.
  void select(const size_t &level, PointIterator &first_point, PointIterator &last_point) {
    RgbdImagePyramid &p = getRgbdImagePyramid();
    RgbdImage &img = p.level(level);
    if (storage_.size() < level + 1) storage_.resize(level + 1);
    Storage &st = storage_[level];
    if (!st.is_cached || debug_) {
      const SelectionMask *m;
      float ti, td;
      deviceForm(level, level, m, ti, td);
      const size_t n = img.width * img.height;
      std::vector<unsigned char> mask(n);
      int count = 0;
      detail::check(dvo_amd_pyramid_select_masked(p.handle(), (int)level, ti, td, m ? m->handle() : nullptr, &count, mask.data()),
                    "PointSelection::select");
      std::vector<float> pl[6];
      for (int k = 0; k < 6; ++k) pl[k] = img.plane(k);
      st.points.assign((size_t)count, PointWithIntensityAndDepth());
      const float fx = img.intrinsics.fx(), fy = img.intrinsics.fy(), ox = img.intrinsics.ox(), oy = img.intrinsics.oy();
      size_t o = 0;
      for (size_t y = 0; y < img.height; ++y)
        for (size_t x = 0; x < img.width; ++x) {
          const size_t i = y * img.width + x;
          if (!mask[i]) continue;
          PointWithIntensityAndDepth &q = st.points[o++];
          const float z = pl[1][i];
          // RgbdCamera's ray template ((x - ox) / fx, (y - oy) / fy, 1, 0) times depth, w = 1 (rgbd_image.cpp:198-199,245-262)
          q.point.data[0] = (((float)x - ox) / fx) * z, q.point.data[1] = (((float)y - oy) / fy) * z;
          q.point.data[2] = z, q.point.data[3] = 1.0f;
          for (int k = 0; k < 6; ++k) q.intensity_and_depth.data[k] = pl[k][i];
          q.intensity_and_depth.data[6] = q.intensity_and_depth.data[7] = 0.0f;
        }
      if (debug_) st.debug_idx.swap(mask);
      st.is_cached = true;
    }
    first_point = st.points.begin();
    last_point = st.points.end();
  }

  // point_selection.cpp:74-86 (a row-major 0/1 byte per pixel instead of a cv::Mat)
  bool getDebugIndex(const size_t &level, std::vector<unsigned char> &dbg_idx) {
    if (debug_ && storage_.size() > level) {
      dbg_idx = storage_[level].debug_idx;
      return !dbg_idx.empty();
    }
    return false;
  }
  void debug(bool v) { debug_ = v; }
  bool debug() const { return debug_; }

 private:
  struct Storage {
    PointVector points;
    bool is_cached;
    std::vector<unsigned char> debug_idx;
    Storage() : is_cached(false) {}
  };
  // The predicate's answers for levels first..last of the pyramid as a device mask.  A level is evaluated once per pyramid;
  // levels nobody has asked for yet are all-drop planes.  Asking for a further level later evaluates that one and uploads a new
  // mask -- a new identity in the pyramid's selection cache (at most DVO_AMD_MAX_MASKED_SELECTIONS of them per pyramid), so a
  // caller does well to ask for the levels it tracks over in one go, as DenseTracker::match does.
  const SelectionMask &hostMask(size_t first_level, size_t last_level) {
    RgbdImagePyramid &p = getRgbdImagePyramid();
    p.build(last_level + 1);
    const size_t levels = (size_t)dvo_amd_pyramid_levels(p.handle());
    if (host_mask_of_ != p.handle() || host_planes_.size() != levels) {  // (the pyramid was rebuilt with more levels)
      host_mask_ = SelectionMask(), host_mask_of_ = p.handle();
      host_planes_.assign(levels, std::vector<unsigned char>());
      host_done_.assign(levels, false);
    }
    bool fresh = !host_mask_.valid();
    for (size_t l = first_level; l <= last_level && l < levels; ++l) {
      if (host_done_[l]) continue;
      RgbdImage &img = p.level(l);
      std::vector<float> pl[6];
      for (int k = 1; k < 6; ++k) pl[k] = img.plane(k);  // (isPointOk does not see the intensity itself)
      std::vector<unsigned char> &out = host_planes_[l];
      out.assign(img.width * img.height, 0);
      for (size_t y = 0; y < img.height; ++y)
        for (size_t x = 0; x < img.width; ++x) {
          const size_t i = y * img.width + x;
          out[i] = predicate_.isPointOk(x, y, pl[1][i], pl[2][i], pl[3][i], pl[4][i], pl[5][i]) ? 1 : 0;
        }
      host_done_[l] = true, fresh = true;
    }
    if (fresh) {
      for (size_t l = 0; l < levels; ++l)
        if (host_planes_[l].empty()) host_planes_[l].assign((size_t)(p.width() >> l) * (size_t)(p.height() >> l), 0);
      host_mask_ = SelectionMask::fromLevels(p.width(), p.height(), host_planes_, p.device());
    }
    return host_mask_;
  }

  RgbdImagePyramid *pyramid_;
  std::vector<Storage> storage_;
  const PointSelectionPredicate &predicate_;
  bool debug_;
  SelectionMask host_mask_;                               // a predicate without a device form, evaluated on the host ...
  std::vector<std::vector<unsigned char> > host_planes_;  // ... its answers per level (all-drop where not evaluated yet)
  std::vector<bool> host_done_;
  const dvo_amd_pyramid *host_mask_of_ = nullptr;         // ... and the device pyramid they belong to
};

// surface_pyramid.h:34-49 / surface_pyramid.cpp:44-105: uint16 raw depth -> float metres, 0 -> NaN, one fp32 multiply per pixel.
// Host-side shim for callers that build the float depth image themselves (camera_dense_tracking.cpp:233-236); the same
// conversion runs on the GPU when a pyramid is created straight from the raw frame (dvo_amd_pyramid_create_raw).  Both reference entry points give the same values; the Sse one needs 16-byte aligned rows of a
// multiple of 8 pixels, which this shim does not.
class SurfacePyramid {
 public:
  static void convertRawDepthImage(const unsigned short *input, float *output, size_t n_pixels, float scale) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < n_pixels; ++i) output[i] = input[i] == 0 ? nan : (float)input[i] * scale;
  }
  static void convertRawDepthImageSse(const unsigned short *input, float *output, size_t n_pixels, float scale) {
    convertRawDepthImage(input, output, n_pixels, scale);
  }
#ifdef DVO_AMD_HAVE_OPENCV
  static void convertRawDepthImage(const cv::Mat &input, cv::Mat &output, float scale) {
    output.create(input.rows, input.cols, CV_32FC1);
    for (int y = 0; y < input.rows; ++y) convertRawDepthImage(input.ptr<unsigned short>(y), output.ptr<float>(y), (size_t)input.cols, scale);
  }
  static void convertRawDepthImageSse(const cv::Mat &input, cv::Mat &output, float scale) { convertRawDepthImage(input, output, scale); }
#endif
  SurfacePyramid() {}
  virtual ~SurfacePyramid() {}
};

// rgbd_image.h:127-144
class RgbdCameraPyramid {
 public:
  RgbdCameraPyramid(size_t base_width, size_t base_height, const IntrinsicMatrix &base_intrinsics, int device = 0)
      : width_((int)base_width), height_((int)base_height), K_(base_intrinsics), device_(device) {}

  // raw planes: intensity 0..255, depth metres with NaN = invalid, stride in floats
  RgbdImagePyramidPtr create(const float *base_intensity, const float *base_depth, int stride = 0, double timestamp = 0.0) {
    return RgbdImagePyramidPtr(new RgbdImagePyramid(width_, height_, K_, base_intensity, base_depth, stride ? stride : width_,
                                                    device_, timestamp));
  }
#ifdef DVO_AMD_HAVE_OPENCV
  // RgbdCameraPyramid::create(const cv::Mat&, const cv::Mat&), rgbd_image.h:135: CV_32FC1 planes
  RgbdImagePyramidPtr create(const cv::Mat &base_intensity, const cv::Mat &base_depth) {
    if (base_intensity.type() != CV_32FC1 || base_depth.type() != CV_32FC1 || base_intensity.size() != base_depth.size() ||
        base_intensity.cols != width_ || base_intensity.rows != height_)
      throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdCameraPyramid::create");
    if (base_intensity.step != base_depth.step) {
      cv::Mat d = base_depth.clone(), i = base_intensity.clone();
      return create(i.ptr<float>(), d.ptr<float>(), (int)(i.step / sizeof(float)));
    }
    return create(base_intensity.ptr<float>(), base_depth.ptr<float>(), (int)(base_intensity.step / sizeof(float)));
  }
#endif
  void build(size_t) {}  // camera levels are derived together with the image levels
  const IntrinsicMatrix &intrinsics() const { return K_; }

 private:
  int width_, height_;
  IntrinsicMatrix K_;
  int device_;
};
typedef std::shared_ptr<RgbdCameraPyramid> RgbdCameraPyramidPtr;

inline ExposureEstimate RgbdImagePyramid::estimateExposure(RgbdImagePyramid &reference, const AffineTransformd *estimate, const SelectionMask *mask,
                                                           const ExposureOptions &options, dvo_amd_context *context) {
  if (options.level >= 0 && options.level < DVO_AMD_MAX_LEVELS) {
    reference.build((size_t)options.level + 1);
    build((size_t)options.level + 1);
  }
  ExposureEstimate out;
  std::unique_lock<std::mutex> lock;
  if (!context) context = cloud::context(device_, lock);
  detail::check(dvo_amd_estimate_exposure(context, reference.handle(), handle_, estimate ? data(*estimate) : nullptr,
                                          mask ? mask->handle() : nullptr, &options, &out),
                "RgbdImagePyramid::estimateExposure");
  return out;
}

}  // namespace core

// dense_tracking.h:39-213
class DenseTracker {
 public:
  struct Config {
    int FirstLevel, LastLevel;
    int MaxIterationsPerLevel;
    double Precision;
    double Mu;
    bool UseInitialEstimate;
    // The next six fields are declared by the reference (dense_tracking.h:51-60), assigned by its callers (configtools.h:70-79)
    // and never read by match(): kept so that those call sites compile; they do not cross the C ABI.
    bool UseWeighting;
    bool UseParallel;  // (not even initialised by the reference's constructor; false here)
    core::InfluenceFunctions::enum_t InfluenceFuntionType;  // [sic]
    float InfluenceFunctionParam;
    core::ScaleEstimators::enum_t ScaleEstimatorType;
    float ScaleEstimatorParam;
    float IntensityDerivativeThreshold;
    float DepthDerivativeThreshold;
    // NOT a field of the reference: dvo_amd_config::segment_geometry (DVO_AMD_GEOMETRY_THROUGHPUT, the default, or
    // DVO_AMD_GEOMETRY_LATENCY for the shortest single match()); callers of the reference never touch it
    int SegmentGeometry;

    Config() {  // dense_tracking_config.cpp:27-42
      dvo_amd_config c;
      dvo_amd_default_config(&c);
      FirstLevel = c.first_level, LastLevel = c.last_level, MaxIterationsPerLevel = c.max_iterations_per_level;
      Precision = c.precision, Mu = c.mu, UseInitialEstimate = c.use_initial_estimate != 0, UseWeighting = true;
      UseParallel = false;
      InfluenceFuntionType = core::InfluenceFunctions::TDistribution, InfluenceFunctionParam = core::kTDistributionDefaultDof;
      ScaleEstimatorType = core::ScaleEstimators::TDistribution, ScaleEstimatorParam = core::kTDistributionDefaultDof;
      IntensityDerivativeThreshold = c.intensity_derivative_threshold;
      DepthDerivativeThreshold = c.depth_derivative_threshold;
      SegmentGeometry = c.segment_geometry;
    }
    size_t getNumLevels() const { return (size_t)FirstLevel + 1; }
    bool UseEstimateSmoothing() const { return Mu > 1e-6; }
    bool IsSane() const { return FirstLevel >= LastLevel; }
  };

  struct TerminationCriteria {
    enum Enum { IterationsExceeded, IncrementTooSmall, LogLikelihoodDecreased, TooFewConstraints, NumCriteria };
  };

  struct IterationStats {
    size_t Id, ValidConstraints;
    double TDistributionLogLikelihood;
    core::Vector2d TDistributionMean;
    core::Matrix2d TDistributionPrecision;
    double PriorLogLikelihood;
    core::Vector6d EstimateIncrement;
    core::Matrix6d EstimateInformation;

    // dense_tracking_config.cpp:123-136 (caller: keyframe_graph.cpp:370-371)
    void InformationEigenValues(core::Vector6d &eigenvalues) const {
      double ev[6];
      core::linalg::symmetric_eigenvalues6(EstimateInformation.data(), ev);
      for (int i = 0; i < 6; ++i) eigenvalues(i) = ev[i];
    }
    double InformationConditionNumber() const {
      core::Vector6d ev;
      InformationEigenValues(ev);
      return std::abs(ev(5) / ev(0));
    }
  };
  typedef std::vector<IterationStats> IterationStatsVector;

  struct LevelStats {
    size_t Id, MaxValidPixels, ValidPixels;
    TerminationCriteria::Enum TerminationCriterion;
    IterationStatsVector Iterations;

    bool HasIterationWithIncrement() const {  // dense_tracking_config.cpp:129-134
      const size_t min = (TerminationCriterion == TerminationCriteria::LogLikelihoodDecreased ||
                          TerminationCriterion == TerminationCriteria::TooFewConstraints)
                             ? 2
                             : 1;
      return Iterations.size() >= min;
    }
    // dense_tracking_config.cpp:138-172 (the reference prints "awkward" + the level and asserts; no assert crosses this adaptor)
    const IterationStats &LastIterationWithIncrement() const {
      if (!HasIterationWithIncrement()) throw std::logic_error("LevelStats: no iteration with an increment");
      return TerminationCriterion == TerminationCriteria::LogLikelihoodDecreased ? Iterations[Iterations.size() - 2]
                                                                                  : Iterations[Iterations.size() - 1];
    }
    IterationStats &LastIterationWithIncrement() {
      return const_cast<IterationStats &>(static_cast<const LevelStats *>(this)->LastIterationWithIncrement());
    }
    const IterationStats &LastIteration() const { return Iterations.back(); }
    IterationStats &LastIteration() { return Iterations.back(); }
  };
  typedef std::vector<LevelStats> LevelStatsVector;

  struct Stats {
    LevelStatsVector Levels;
  };

  struct Result {
    core::AffineTransformd Transformation;
    core::Matrix6d Information;
    double LogLikelihood;
    Stats Statistics;

    Result() : LogLikelihood(std::numeric_limits<double>::max()) {  // dense_tracking_config.cpp:101-108
      const double nan = std::numeric_limits<double>::quiet_NaN();
      double *t = core::data(Transformation);
      for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) t[c * 4 + r] = nan;
      Information.setIdentity();
    }
    bool isNaN() const {  // dense_tracking_config.cpp:96-99
      const double *t = core::data(Transformation);
      double s = 0;
      for (int i = 0; i < 16; ++i) s += t[i];
      return !std::isfinite(s) || !std::isfinite(Information.sum());
    }
    void setIdentity() {
      Transformation.setIdentity();
      Information.setIdentity();
      LogLikelihood = 0.0;
    }
    void clearStatistics() { Statistics.Levels.clear(); }
  };

  static const Config &getDefaultConfig() {
    static Config c;
    return c;
  }

  explicit DenseTracker(const Config &config = getDefaultConfig(), int device = 0)
      : ctx_(nullptr), device_(device), reference_selection_(selection_predicate_) {
    dvo_amd_config c = to_c(config);
    detail::check(dvo_amd_context_create(device, &c, &ctx_), "DenseTracker::DenseTracker");
    cfg = config;
    selection_predicate_.intensity_threshold = cfg.IntensityDerivativeThreshold;
    selection_predicate_.depth_threshold = cfg.DepthDerivativeThreshold;
  }
  DenseTracker(const DenseTracker &other) : ctx_(nullptr), device_(other.device_), reference_selection_(selection_predicate_) {
    dvo_amd_config c = to_c(other.cfg);
    detail::check(dvo_amd_context_create(device_, &c, &ctx_), "DenseTracker::DenseTracker");
    cfg = other.cfg;
    selection_predicate_.intensity_threshold = cfg.IntensityDerivativeThreshold;
    selection_predicate_.depth_threshold = cfg.DepthDerivativeThreshold;
  }
  DenseTracker &operator=(const DenseTracker &) = delete;
  ~DenseTracker() { dvo_amd_context_destroy(ctx_); }

  const Config &configuration() const { return cfg; }

  void configure(const Config &config) {
    dvo_amd_config c = to_c(config);
    detail::check(dvo_amd_configure(ctx_, &c), "DenseTracker::configure");  // assert(config.IsSane()) in the reference
    cfg = config;
    selection_predicate_.intensity_threshold = cfg.IntensityDerivativeThreshold;  // dense_tracking.cpp:76-77
    selection_predicate_.depth_threshold = cfg.DepthDerivativeThreshold;
  }

  // dense_tracking.cpp:99-109
  bool match(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current, core::AffineTransformd &transformation) {
    Result result;
    result.Transformation = transformation;
    const bool success = match(reference, current, result);
    transformation = result.Transformation;
    return success;
  }

  // dense_tracking.cpp:111-121
  bool match(core::PointSelection &reference, core::RgbdImagePyramid &current, core::AffineTransformd &transformation) {
    Result result;
    result.Transformation = transformation;
    const bool success = match(reference, current, result);
    transformation = result.Transformation;
    return success;
  }

  // dense_tracking.cpp:123-129
  bool match(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current, Result &result) {
    reference.compute(cfg.getNumLevels());
    reference_selection_.setRgbdImagePyramid(reference);
    return match(reference_selection_, current, result);
  }

  // dense_tracking.cpp:131-376: the reference pixels are the ones `reference`'s predicate keeps
  bool match(core::PointSelection &reference, core::RgbdImagePyramid &current, Result &result) {
    core::RgbdImagePyramid &ref_pyramid = reference.getRgbdImagePyramid();
    ref_pyramid.compute(cfg.getNumLevels());
    current.compute(cfg.getNumLevels());
    // the predicate's device form for the levels this match walks (a user-defined predicate is evaluated on the host here, once
    // per pyramid); a predicate of two thresholds takes the path it always took (mask == NULL is dvo_amd_match_selection)
    const core::SelectionMask *mask = nullptr;
    float ti = 0.0f, td = 0.0f;
    reference.deviceForm((size_t)cfg.LastLevel, (size_t)cfg.FirstLevel, mask, ti, td);
    const int cap = (cfg.FirstLevel - cfg.LastLevel + 1) * (cfg.MaxIterationsPerLevel + 1);
    std::vector<dvo_amd_iteration_stats> its((size_t)cap);
    dvo_amd_result r;
    std::memset(&r, 0, sizeof(r));
    r.iterations = its.data();
    r.iterations_capacity = cap;
    double T0[16];
    std::memcpy(T0, core::data(result.Transformation), sizeof(T0));
    detail::check(dvo_amd_match_masked(ctx_, ref_pyramid.handle(), mask ? mask->handle() : nullptr, ti, td, current.handle(),
                                       cfg.UseInitialEstimate ? T0 : nullptr, &r),
                  "DenseTracker::match");
    std::memcpy(core::data(result.Transformation), r.transformation, sizeof(r.transformation));
    std::memcpy(core::data(result.Information), r.information, sizeof(r.information));
    result.LogLikelihood = r.loglik;
    result.Statistics.Levels.clear();
    for (int l = 0; l < r.n_levels; ++l) {
      LevelStats ls;
      ls.Id = (size_t)r.levels[l].id;
      ls.MaxValidPixels = (size_t)r.levels[l].max_valid_pixels;
      ls.ValidPixels = (size_t)r.levels[l].valid_pixels;
      ls.TerminationCriterion = (TerminationCriteria::Enum)r.levels[l].termination;
      for (int k = 0; k < r.levels[l].n_iterations; ++k) {
        const dvo_amd_iteration_stats &s = its[(size_t)(r.levels[l].first_iteration + k)];
        IterationStats is;
        is.Id = (size_t)s.id, is.ValidConstraints = (size_t)s.valid_constraints;
        is.TDistributionLogLikelihood = s.tdist_loglik;
        for (int i = 0; i < 2; ++i) is.TDistributionMean(i) = s.tdist_mean[i];
        for (int i = 0; i < 4; ++i) is.TDistributionPrecision(i % 2, i / 2) = s.tdist_precision[i];
        is.PriorLogLikelihood = s.prior_loglik;
        for (int i = 0; i < 6; ++i) is.EstimateIncrement(i) = s.increment[i];
        for (int i = 0; i < 36; ++i) is.EstimateInformation(i % 6, i / 6) = s.information[i];
        ls.Iterations.push_back(is);
      }
      result.Statistics.Levels.push_back(ls);
    }
    return true;  // the reference's `success` is constant true (dense_tracking.cpp:135,375)
  }

  // (not in the reference) match() behind an exposure compensation of the current frame (dvo_amd.h, "Exposure compensation"): the
  // gain and bias of `current` against `reference` are estimated at the start -- result.Transformation on entry with
  // UseInitialEstimate, else the identity --, `current` is adjusted by them and the adjusted pyramid is matched.  Every further
  // round estimates again at the result, adjusts the ORIGINAL frame and matches from the result (with UseInitialEstimate; without,
  // match() starts from the identity as always).  match() itself is untouched; `current` is only read.  estimates: one record per
  // round; adjusted: the adjusted pyramid of the last round.
  bool matchCompensated(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current, Result &result,
                        const core::ExposureOptions &options = core::ExposureOptions(), int rounds = 1,
                        std::vector<core::ExposureEstimate> *estimates = nullptr, core::RgbdImagePyramidPtr *adjusted = nullptr) {
    if (rounds < 1) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "DenseTracker::matchCompensated");
    reference.compute(cfg.getNumLevels());
    current.compute(cfg.getNumLevels());
    core::AffineTransformd start;  // the identity
    if (cfg.UseInitialEstimate) start = result.Transformation;
    if (estimates) estimates->clear();
    bool success = true;
    for (int round = 0; round < rounds; ++round) {
      const core::ExposureEstimate e = current.estimateExposure(reference, &start, nullptr, options, ctx_);
      core::RgbdImagePyramidPtr made = current.adjustIntensity(e.gain, e.bias);
      Result r;
      r.Transformation = start;
      success = match(reference, *made, r);
      result = r;
      if (estimates) estimates->push_back(e);
      if (adjusted) *adjusted = made;
      if (r.isNaN()) break;
      start = core::SelectionMask::rigidInverse(r.Transformation);
    }
    return success;
  }

  // dense_tracking.cpp:378-444 (caller: keyframe_graph.cpp:354): |intensity residual| per reference pixel of `level`, 0 where
  // the pixel is not selected or its warp is invalid; CV_32FC1 where OpenCV is available, else ErrorImage
  struct ErrorImage {
    int rows, cols;
    std::vector<float> data;
    float &at(int y, int x) { return data[(size_t)y * cols + x]; }
    float at(int y, int x) const { return data[(size_t)y * cols + x]; }
  };
  ErrorImage computeIntensityErrorImageRaw(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current,
                                           const core::AffineTransformd &transformation, size_t level = 0) {
    reference.compute(level + 1);
    current.compute(level + 1);
    core::RgbdImage &img = reference.level(level);
    ErrorImage out;
    out.rows = (int)img.height, out.cols = (int)img.width;
    out.data.resize(img.width * img.height);
    detail::check(dvo_amd_error_image(ctx_, reference.handle(), current.handle(), core::data(transformation), (int)level,
                                      out.data.data()),
                  "DenseTracker::computeIntensityErrorImage");
    return out;
  }
#ifdef DVO_AMD_HAVE_OPENCV
  cv::Mat computeIntensityErrorImage(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current,
                                     const core::AffineTransformd &transformation, size_t level = 0) {
    ErrorImage e = computeIntensityErrorImageRaw(reference, current, transformation, level);
    cv::Mat m(e.rows, e.cols, CV_32FC1);
    for (int y = 0; y < e.rows; ++y) std::memcpy(m.ptr<float>(y), &e.data[(size_t)y * e.cols], sizeof(float) * (size_t)e.cols);
    return m;
  }
#else
  ErrorImage computeIntensityErrorImage(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current,
                                        const core::AffineTransformd &transformation, size_t level = 0) {
    return computeIntensityErrorImageRaw(reference, current, transformation, level);
  }
#endif

  // Pose scoring (dvo_amd.h, "Pose scoring"): one record per hypothesis of the pair at options.level -- the counts of the four
  // outcomes, the integer cost and the total a ranking goes by.  transformations: reference -> current, the ESTIMATE (what
  // computeIntensityErrorImage takes; the inverse of what match() returns).  Both pyramids are built up to the level.  The call
  // holds no tracker state and refines nothing: the best hypotheses are starts for match() or the proposal validator.
  struct PoseScoreOptions : dvo_amd_pose_score_options {
    explicit PoseScoreOptions(int level_ = 0) {
      dvo_amd_default_pose_score_options(this);
      level = level_;
    }
    // the level's precision as SelectionMask::fromResiduals takes it: the last iteration of the nearest level that ran
    PoseScoreOptions(int level_, const Result &result) {
      dvo_amd_default_pose_score_options(this);
      level = level_;
      long best = -1, best_distance = 0;
      for (size_t i = 0; i < result.Statistics.Levels.size(); ++i) {
        if (result.Statistics.Levels[i].Iterations.empty()) continue;
        const long id = (long)result.Statistics.Levels[i].Id, distance = id > level_ ? id - level_ : level_ - id;
        if (best < 0 || distance < best_distance || (distance == best_distance && id < (long)result.Statistics.Levels[(size_t)best].Id))
          best = (long)i, best_distance = distance;
      }
      if (best < 0) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "DenseTracker::PoseScoreOptions");
      const core::Matrix2d &P = result.Statistics.Levels[(size_t)best].Iterations.back().TDistributionPrecision;
      for (int i = 0; i < 4; ++i) precision[i] = (float)P(i % 2, i / 2);  // column-major
    }
  };
  typedef dvo_amd_pose_score PoseScore;
  std::vector<PoseScore> scorePoses(core::RgbdImagePyramid &reference, core::RgbdImagePyramid &current,
                                    const std::vector<core::AffineTransformd> &transformations, const PoseScoreOptions &options) {
    if (options.level >= 0 && options.level < DVO_AMD_MAX_LEVELS) {
      reference.compute((size_t)options.level + 1);
      current.compute((size_t)options.level + 1);
    }
    std::vector<double> T(16 * transformations.size());
    for (size_t j = 0; j < transformations.size(); ++j) std::memcpy(&T[16 * j], core::data(transformations[j]), sizeof(double) * 16);
    std::vector<PoseScore> scores(transformations.size());
    detail::check(dvo_amd_score_poses(ctx_, reference.handle(), current.handle(), (int)transformations.size(), T.data(), &options,
                                      scores.data()),
                  "DenseTracker::scorePoses");
    return scores;
  }
  // the min(k, scores.size()) indices of smallest total, smallest first, ties to the lower index (dvo_amd_rank_poses)
  static std::vector<int> rankPoses(const std::vector<PoseScore> &scores, int k) {
    std::vector<int> order((size_t)std::max(0, std::min(k, (int)scores.size())) + 1);
    int n = 0;
    detail::check(dvo_amd_rank_poses(scores.data(), (int)scores.size(), k, order.data(), &n), "DenseTracker::rankPoses");
    order.resize((size_t)n);
    return order;
  }
  // Exp(xi) * centre over a grid of xi = (vx, vy, vz, wx, wy, wz), wz fastest; the middle entry is the centre itself (dvo_amd_pose_grid)
  static std::vector<core::AffineTransformd> poseGrid(const dvo_amd_pose_grid_options &grid, const core::AffineTransformd &centre) {
    int n = 0;
    detail::check(dvo_amd_pose_grid(&grid, core::data(centre), nullptr, 0, &n), "DenseTracker::poseGrid");
    std::vector<double> T(16 * (size_t)n);
    detail::check(dvo_amd_pose_grid(&grid, core::data(centre), T.data(), n, &n), "DenseTracker::poseGrid");
    std::vector<core::AffineTransformd> out((size_t)n);
    for (int j = 0; j < n; ++j) std::memcpy(core::data(out[(size_t)j]), &T[16 * (size_t)j], sizeof(double) * 16);
    return out;
  }

  dvo_amd_context *handle() const { return ctx_; }

 private:
  static dvo_amd_config to_c(const Config &c) {
    dvo_amd_config o;
    o.first_level = c.FirstLevel, o.last_level = c.LastLevel, o.max_iterations_per_level = c.MaxIterationsPerLevel;
    o.precision = c.Precision, o.mu = c.Mu, o.use_initial_estimate = c.UseInitialEstimate ? 1 : 0;
    o.intensity_derivative_threshold = c.IntensityDerivativeThreshold;
    o.depth_derivative_threshold = c.DepthDerivativeThreshold;
    o.segment_geometry = c.SegmentGeometry, o.reserved = 0;
    return o;
  }

  Config cfg;
  dvo_amd_context *ctx_;
  int device_;
  core::ValidPointAndGradientThresholdPredicate selection_predicate_;  // dense_tracking.h:199-200
  core::PointSelection reference_selection_;
};

}  // namespace dvo

// dense_tracking.h:215-237
template <typename CharT, typename Traits>
std::ostream &operator<<(std::basic_ostream<CharT, Traits> &out, const dvo::DenseTracker::Config &config) {
  out << "First Level = " << config.FirstLevel << ", Last Level = " << config.LastLevel
      << ", Max Iterations per Level = " << config.MaxIterationsPerLevel << ", Precision = " << config.Precision
      << ", Mu = " << config.Mu << ", Use Initial Estimate = " << (config.UseInitialEstimate ? "true" : "false")
      << ", Use Weighting = " << (config.UseWeighting ? "true" : "false")
      << ", Scale Estimator = " << dvo::core::ScaleEstimators::str(config.ScaleEstimatorType)
      << ", Scale Estimator Param = " << config.ScaleEstimatorParam
      << ", Influence Function = " << dvo::core::InfluenceFunctions::str(config.InfluenceFuntionType)
      << ", Influence Function Param = " << config.InfluenceFunctionParam
      << ", Intensity Derivative Threshold = " << config.IntensityDerivativeThreshold
      << ", Depth Derivative Threshold = " << config.DepthDerivativeThreshold;
  return out;
}

// dense_tracking.h:239-245
template <typename CharT, typename Traits>
std::ostream &operator<<(std::basic_ostream<CharT, Traits> &o, const dvo::DenseTracker::IterationStats &s) {
  o << "Iteration: " << s.Id << " ValidConstraints: " << s.ValidConstraints << " DataLogLikelihood: " << s.TDistributionLogLikelihood
    << " PriorLogLikelihood: " << s.PriorLogLikelihood << std::endl;
  return o;
}

// dense_tracking.h:247-279
template <typename CharT, typename Traits>
std::ostream &operator<<(std::basic_ostream<CharT, Traits> &o, const dvo::DenseTracker::LevelStats &s) {
  std::string termination;
  switch (s.TerminationCriterion) {
    case dvo::DenseTracker::TerminationCriteria::IterationsExceeded: termination = "IterationsExceeded"; break;
    case dvo::DenseTracker::TerminationCriteria::IncrementTooSmall: termination = "IncrementTooSmall"; break;
    case dvo::DenseTracker::TerminationCriteria::LogLikelihoodDecreased: termination = "LogLikelihoodDecreased"; break;
    case dvo::DenseTracker::TerminationCriteria::TooFewConstraints: termination = "TooFewConstraints"; break;
    default: break;
  }
  o << "Level: " << s.Id << " Pixel: " << s.ValidPixels << "/" << s.MaxValidPixels << " Termination: " << termination
    << " Iterations: " << s.Iterations.size() << std::endl;
  for (dvo::DenseTracker::IterationStatsVector::const_iterator it = s.Iterations.begin(); it != s.Iterations.end(); ++it) o << *it;
  return o;
}

// dense_tracking.h:281-291
template <typename CharT, typename Traits>
std::ostream &operator<<(std::basic_ostream<CharT, Traits> &o, const dvo::DenseTracker::Stats &s) {
  o << s.Levels.size() << " levels" << std::endl;
  for (dvo::DenseTracker::LevelStatsVector::const_iterator it = s.Levels.begin(); it != s.Levels.end(); ++it) o << *it;
  return o;
}

#endif  // DVO_AMD_DENSE_TRACKING_HPP_
