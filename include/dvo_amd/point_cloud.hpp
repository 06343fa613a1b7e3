// point_cloud.hpp -- header-only C++ adaptor of the keyframe map's point cloud over the C ABI (include/dvo_amd.h):
//   dvo::visualization::AsyncPointCloudBuilder::{PointCloud, BuildJob}   dvo_core/include/dvo/visualization/async_point_cloud_builder.h
//   dvo::visualization::PointCloudAggregator                             dvo_core/include/dvo/visualization/point_cloud_aggregator.h
//   dvo::visualization::KeyframeMap                                      (no counterpart: the map kept on the device, dvo_amd_map_*)
// PCL-free: PointCloud holds PointXYZRGB records with the members callers read (points, width, height, push_back, size,
// reserve).  A BuildJob's cloud is dvo_amd_point_cloud at the job's pose; PointCloudAggregator::build keeps the reference's
// std::map name order and its max(n / 50, 1) step and aggregates the clouds it picks in ONE call on the GPU: dvo_amd_map_cloud
// when every picked entry is a job on a level-0 image, dvo_amd_voxel_downsample of all of them otherwise (the same result: the
// aggregate of the concatenated clouds).  The aggregate is dvo_amd.h's one-point-per-voxel grid, not ApproximateVoxelGrid's
// order-dependent hash.
#ifndef DVO_AMD_POINT_CLOUD_HPP_
#define DVO_AMD_POINT_CLOUD_HPP_

#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "dense_tracking.hpp"

namespace dvo {
namespace visualization {

// pcl::PointXYZRGB as far as the map's readers use it (default: the origin, black -- what PCL's constructor gives)
struct PointXYZRGB {
  float x, y, z;
  std::uint8_t r, g, b;
  PointXYZRGB() : x(0.0f), y(0.0f), z(0.0f), r(0), g(0), b(0) {}
};

// pcl::PointXYZRGBNormal as far as a mesher or a shader reads it: the point, its colour, its surface normal (NaN where the
// surface has none) and PCL's curvature, which is not computed here (0)
struct PointXYZRGBNormal : PointXYZRGB {
  float normal_x, normal_y, normal_z, curvature;
  PointXYZRGBNormal() : normal_x(0.0f), normal_y(0.0f), normal_z(0.0f), curvature(0.0f) {}
};

namespace detail {
inline PointXYZRGB from_record(const dvo_amd_point &p) {
  PointXYZRGB q;
  q.x = p.x, q.y = p.y, q.z = p.z;
  q.r = (std::uint8_t)((p.rgb >> 16) & 0xFF), q.g = (std::uint8_t)((p.rgb >> 8) & 0xFF), q.b = (std::uint8_t)(p.rgb & 0xFF);
  return q;
}
inline dvo_amd_point to_record(const PointXYZRGB &q) {
  dvo_amd_point p;
  p.x = q.x, p.y = q.y, p.z = q.z;
  p.rgb = ((unsigned)q.r << 16) | ((unsigned)q.g << 8) | (unsigned)q.b;
  return p;
}
// dvo_amd.h's colour rule: clamped to [0, 255], truncated, NaN -> 0
inline unsigned char to8(float v) {
  if (!(v == v)) return 0;
  return (unsigned char)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}
// the image's float BGR as the 8-bit BGR the C ABI takes (empty: no colour image, grey from the intensity plane)
inline std::vector<unsigned char> bgr8(const core::RgbdImage &image) {
  std::vector<unsigned char> out;
  const size_t w = image.width, h = image.height;
#ifdef DVO_AMD_HAVE_OPENCV
  if (image.rgb.empty()) return out;
  if (image.rgb.type() != CV_MAKETYPE(CV_32F, 3) || (size_t)image.rgb.cols != w || (size_t)image.rgb.rows != h)
    throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::rgb (CV_32FC3 of the image's size)");
  out.resize(w * h * 3);
  for (size_t y = 0; y < h; ++y) {
    const float *row = image.rgb.ptr<float>((int)y);
    for (size_t x = 0; x < w * 3; ++x) out[y * w * 3 + x] = to8(row[x]);
  }
#else
  if (image.rgb.empty()) return out;
  if (image.rgb.size() != w * h * 3) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "RgbdImage::rgb (width * height * 3)");
  out.resize(w * h * 3);
  for (size_t i = 0; i < out.size(); ++i) out[i] = to8(image.rgb[i]);
#endif
  return out;
}
}  // namespace detail

class AsyncPointCloudBuilder {
 public:
  struct PointCloud {
    typedef PointXYZRGB PointType;
    typedef std::shared_ptr<PointCloud> Ptr;
    std::vector<PointXYZRGB> points;
    std::uint32_t width, height;
    PointCloud() : width(0), height(1) {}
    void push_back(const PointXYZRGB &p) {
      points.push_back(p);
      width = (std::uint32_t)points.size(), height = 1;
    }
    size_t size() const { return points.size(); }
    void reserve(size_t n) { points.reserve(n); }
  };

  // async_point_cloud_builder.h:43-54: the cloud of one image at a pose (RgbdCamera::buildPointCloud, transformed and coloured)
  struct BuildJob {
    typedef std::shared_ptr<BuildJob> Ptr;
    const core::RgbdImage &image;
    core::AffineTransformd pose;

    BuildJob(const core::RgbdImage &image, const core::AffineTransformd pose = core::AffineTransformd()) : image(image), pose(pose) {}

    // the organized cloud: width x height points in scan order, NaN points included (async_point_cloud_builder.cpp:61-110)
    PointCloud::Ptr build() const {
      std::vector<dvo_amd_point> pts;
      records(pts);
      PointCloud::Ptr cloud(new PointCloud);
      cloud->points.reserve(pts.size());
      for (size_t i = 0; i < pts.size(); ++i) cloud->points.push_back(detail::from_record(pts[i]));
      cloud->width = (std::uint32_t)image.width, cloud->height = (std::uint32_t)image.height;
      return cloud;
    }

    // the same cloud as the C ABI's records
    void records(std::vector<dvo_amd_point> &out) const {
      const core::RgbdImagePyramid *pyr = owner();
      const std::vector<unsigned char> bgr = detail::bgr8(image);
      out.resize(image.width * image.height);
      std::unique_lock<std::mutex> lock;
      dvo_amd_context *ctx = core::cloud::context(pyr->device(), lock);
      ::dvo::detail::check(dvo_amd_point_cloud(ctx, pyr->handle(), level(), core::data(pose), bgr.empty() ? nullptr : bgr.data(),
                                               (int)image.width * 3, out.data()),
                           "AsyncPointCloudBuilder::BuildJob::build");
    }

    // (not in the reference) the same cloud with every point's surface normal in the pose's frame (dvo_amd_point_cloud_normals;
    // the rule is pinned in dvo_amd.h under "Surface normals"): `options` default to RgbdImage::calculateNormals' own rule
    struct NormalCloud {
      typedef PointXYZRGBNormal PointType;
      typedef std::shared_ptr<NormalCloud> Ptr;
      std::vector<PointXYZRGBNormal> points;
      std::uint32_t width, height;
      NormalCloud() : width(0), height(1) {}
      size_t size() const { return points.size(); }
    };
    NormalCloud::Ptr buildWithNormals(const core::SelectionMask::NormalOptions &options = core::SelectionMask::NormalOptions()) const {
      std::vector<dvo_amd_point> pts;
      std::vector<float> normals;
      recordsWithNormals(pts, normals, options);
      NormalCloud::Ptr cloud(new NormalCloud);
      cloud->points.resize(pts.size());
      for (size_t i = 0; i < pts.size(); ++i) {
        PointXYZRGBNormal &q = cloud->points[i];
        static_cast<PointXYZRGB &>(q) = detail::from_record(pts[i]);
        q.normal_x = normals[4 * i], q.normal_y = normals[4 * i + 1], q.normal_z = normals[4 * i + 2];
      }
      cloud->width = (std::uint32_t)image.width, cloud->height = (std::uint32_t)image.height;
      return cloud;
    }
    // ... as the C ABI's records and four floats per point (what dvo_amd_write_pcd_normals takes)
    void recordsWithNormals(std::vector<dvo_amd_point> &out, std::vector<float> &normals,
                            const core::SelectionMask::NormalOptions &options = core::SelectionMask::NormalOptions()) const {
      const core::RgbdImagePyramid *pyr = owner();
      const std::vector<unsigned char> bgr = detail::bgr8(image);
      out.resize(image.width * image.height);
      normals.resize(image.width * image.height * 4);
      std::unique_lock<std::mutex> lock;
      dvo_amd_context *ctx = core::cloud::context(pyr->device(), lock);
      ::dvo::detail::check(dvo_amd_point_cloud_normals(ctx, pyr->handle(), level(), core::data(pose), bgr.empty() ? nullptr : bgr.data(),
                                                       (int)image.width * 3, &options, out.data(), normals.data()),
                           "AsyncPointCloudBuilder::BuildJob::buildWithNormals");
    }

    const core::RgbdImagePyramid *owner() const {
      if (!image.pyramid()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "BuildJob: an image that is not a pyramid level");
      return image.pyramid();
    }
    int level() const { return image.level(); }
  };
};

// point_cloud_aggregator.h:36-55 / point_cloud_aggregator.cpp:74-109
class PointCloudAggregator {
 public:
  typedef AsyncPointCloudBuilder::PointCloud PointCloud;
  typedef AsyncPointCloudBuilder::BuildJob BuildJob;

  explicit PointCloudAggregator(float leaf_size = 0.01f) : leaf_(leaf_size) {}

  void add(const std::string &name, const BuildJob &job) {
    std::lock_guard<std::mutex> g(mu_);
    entries_[name] = Entry(std::make_shared<BuildJob>(job), PointCloud::Ptr());
  }
  void add(const std::string &name, const PointCloud::Ptr &cloud) {
    std::lock_guard<std::mutex> g(mu_);
    entries_[name] = Entry(BuildJob::Ptr(), cloud);
  }
  void remove(const std::string &name) {
    std::lock_guard<std::mutex> g(mu_);
    entries_.erase(name);
  }

  PointCloud::Ptr build() {
    std::map<std::string, Entry> local;
    {
      std::lock_guard<std::mutex> g(mu_);
      local = entries_;
    }
    PointCloud::Ptr out(new PointCloud);
    if (local.empty()) {  // the reference's single default point
      out->push_back(PointXYZRGB());
      return out;
    }
    const size_t step = std::max(local.size() / size_t(50), size_t(1));
    std::vector<const Entry *> picked;
    bool all_jobs = true;
    size_t k = 0;
    for (std::map<std::string, Entry>::const_iterator it = local.begin(); it != local.end(); ++it, ++k)
      if (k % step == 0) {
        picked.push_back(&it->second);
        all_jobs = all_jobs && it->second.first && it->second.first->level() == 0;
      }
    int device = 0;
    for (size_t i = 0; i < picked.size(); ++i)
      if (picked[i]->first) device = picked[i]->first->owner()->device();
    std::vector<dvo_amd_point> voxels;
    dvo_amd_cloud_stats stats;
    if (all_jobs) {
      std::vector<dvo_amd_pyramid *> pyrs;
      std::vector<double> poses;
      std::vector<std::vector<unsigned char> > bgr(picked.size());
      std::vector<const unsigned char *> bgr_ptr;
      std::vector<int> strides;
      for (size_t i = 0; i < picked.size(); ++i) {
        const BuildJob &j = *picked[i]->first;
        pyrs.push_back(j.owner()->handle());
        poses.insert(poses.end(), core::data(j.pose), core::data(j.pose) + 16);
        bgr[i] = detail::bgr8(j.image);
        bgr_ptr.push_back(bgr[i].empty() ? nullptr : bgr[i].data());
        strides.push_back((int)j.image.width * 3);
      }
      aggregate(device, "PointCloudAggregator::build", voxels, stats, [&](dvo_amd_context *ctx, dvo_amd_point *o, long long cap,
                                                                          dvo_amd_cloud_stats *st) {
        return dvo_amd_map_cloud(ctx, (int)pyrs.size(), pyrs.data(), poses.data(), bgr_ptr.data(), strides.data(), leaf_, o, cap,
                                 st);
      });
    } else {
      std::vector<dvo_amd_point> all, one;
      for (size_t i = 0; i < picked.size(); ++i) {
        if (picked[i]->first) {
          picked[i]->first->records(one);
          all.insert(all.end(), one.begin(), one.end());
        } else if (picked[i]->second) {
          const std::vector<PointXYZRGB> &p = picked[i]->second->points;
          for (size_t q = 0; q < p.size(); ++q) all.push_back(detail::to_record(p[q]));
        }
      }
      aggregate(device, "PointCloudAggregator::build", voxels, stats, [&](dvo_amd_context *ctx, dvo_amd_point *o, long long cap,
                                                                          dvo_amd_cloud_stats *st) {
        return dvo_amd_voxel_downsample(ctx, (long long)all.size(), all.data(), leaf_, o, cap, st);
      });
    }
    out->reserve(voxels.size());
    for (size_t i = 0; i < voxels.size(); ++i) out->points.push_back(detail::from_record(voxels[i]));
    out->width = (std::uint32_t)voxels.size(), out->height = 1;
    return out;
  }

 private:
  typedef std::pair<BuildJob::Ptr, PointCloud::Ptr> Entry;

  // one aggregate call, the output grown once on DVO_AMD_ERR_CAPACITY
  template <typename Call>
  static void aggregate(int device, const char *where, std::vector<dvo_amd_point> &out, dvo_amd_cloud_stats &stats, Call call) {
    std::unique_lock<std::mutex> lock;
    dvo_amd_context *ctx = core::cloud::context(device, lock);
    out.resize(1 << 16);
    int rc = call(ctx, out.data(), (long long)out.size(), &stats);
    if (rc == DVO_AMD_ERR_CAPACITY) {
      out.resize((size_t)stats.voxels);
      rc = call(ctx, out.data(), (long long)out.size(), &stats);
    }
    ::dvo::detail::check(rc, where);
    out.resize((size_t)stats.voxels);
  }

  float leaf_;
  std::mutex mu_;
  std::map<std::string, Entry> entries_;
};

// The keyframe map kept on the device (dvo_amd.h: dvo_amd_map_*): insert / move / remove keyframes one event at a time;
// extract() always equals one dvo_amd_map_cloud over the keyframes now in the map, bit for bit, without the rebuild.  This is
// what replaces calling PointCloudAggregator::build() after every event.  Level-0 jobs only.  The map lives in
// the shared cloud context of `device` (core::cloud::context), which outlives it; calls are serialised by that context's lock.
class KeyframeMap {
 public:
  typedef AsyncPointCloudBuilder::PointCloud PointCloud;
  typedef AsyncPointCloudBuilder::BuildJob BuildJob;

  // a rendered view (dvo_amd.h: dvo_amd_map_render): width * height values per plane, row-major; empty pixels hold depth NaN,
  // rgb 0, intensity 0, index -1
  struct View {
    int width, height;
    std::vector<float> depth, intensity;
    std::vector<unsigned int> rgb;
    std::vector<int> index;
    dvo_amd_render_stats stats;
  };

  explicit KeyframeMap(float leaf_size = 0.01f, int device = 0) : device_(device), map_(nullptr), leaf_(leaf_size) {
    std::unique_lock<std::mutex> lock;
    dvo_amd_context *ctx = core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_create(ctx, leaf_size, &map_), "KeyframeMap");
  }
  ~KeyframeMap() {
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    dvo_amd_map_destroy(map_);
  }
  KeyframeMap(const KeyframeMap &) = delete;
  KeyframeMap &operator=(const KeyframeMap &) = delete;

  // the job's image (level 0 of its pyramid) at the job's pose; the map keeps the pyramid and a copy of the colour image
  void insert(int id, const BuildJob &job) {
    if (job.level() != 0) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "KeyframeMap::insert: a level-0 image");
    const std::vector<unsigned char> bgr = detail::bgr8(job.image);
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_insert(map_, id, job.owner()->handle(), core::data(job.pose), bgr.empty() ? nullptr : bgr.data(),
                                            (int)job.image.width * 3),
                         "KeyframeMap::insert");
  }
  void set_poses(const std::vector<int> &ids, const std::vector<core::AffineTransformd> &poses) {
    if (ids.size() != poses.size()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "KeyframeMap::set_poses: one pose per id");
    std::vector<double> flat;
    for (size_t i = 0; i < poses.size(); ++i) flat.insert(flat.end(), core::data(poses[i]), core::data(poses[i]) + 16);
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_set_poses(map_, (int)ids.size(), ids.data(), flat.data()), "KeyframeMap::set_poses");
  }
  void set_pose(int id, const core::AffineTransformd &pose) {
    set_poses(std::vector<int>(1, id), std::vector<core::AffineTransformd>(1, pose));
  }
  void remove(const std::vector<int> &ids) {
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_remove(map_, (int)ids.size(), ids.data()), "KeyframeMap::remove");
  }
  void remove(int id) { remove(std::vector<int>(1, id)); }

  dvo_amd_cloud_stats stats(int *n_keyframes = nullptr) const {
    dvo_amd_cloud_stats st;
    ::dvo::detail::check(dvo_amd_map_stats(map_, &st, n_keyframes), "KeyframeMap::stats");
    return st;
  }

  // the voxels in key order; box: null, or {xmin, ymin, zmin, xmax, ymax, zmax}
  void records(std::vector<dvo_amd_point> &out, const float *box = nullptr) {
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    dvo_amd_cloud_stats st;
    ::dvo::detail::check(dvo_amd_map_stats(map_, &st, nullptr), "KeyframeMap::extract");
    long long n = 0;
    out.resize((size_t)(box ? 0 : st.voxels));
    int rc = dvo_amd_map_extract(map_, box, out.data(), (long long)out.size(), &n);
    if (rc == DVO_AMD_ERR_CAPACITY) {
      out.resize((size_t)n);
      rc = dvo_amd_map_extract(map_, box, out.data(), (long long)out.size(), &n);
    }
    ::dvo::detail::check(rc, "KeyframeMap::extract");
    out.resize((size_t)n);
  }
  PointCloud::Ptr extract(const float *box = nullptr) {
    std::vector<dvo_amd_point> voxels;
    records(voxels, box);
    PointCloud::Ptr out(new PointCloud);
    out->reserve(voxels.size());
    for (size_t i = 0; i < voxels.size(); ++i) out->points.push_back(detail::from_record(voxels[i]));
    out->width = (std::uint32_t)voxels.size(), out->height = 1;
    return out;
  }

  // near_z <= 0: max(0.1, leaf * max(fx, fy) / 32), the closest the render rule admits
  dvo_amd_view view(const core::IntrinsicMatrix &K, int width, int height, float near_z = 0.0f) const {
    dvo_amd_view v;
    v.width = width, v.height = height, v.fx = K.fx(), v.fy = K.fy(), v.ox = K.ox(), v.oy = K.oy();
    v.near_z = near_z > 0.0f ? near_z : std::max(0.1f, (leaf_ * std::max(K.fx(), K.fy())) / 32.0f);
    return v;
  }
  // the map seen from `pose` (camera -> world) through K: every voxel splatted over a square of its own size with a
  // nearest-depth test, what RgbdImage::warpDepthForward / warpIntensityForward do with a point list (rgbd_image.cpp:604-781)
  void render(const core::AffineTransformd &pose, const core::IntrinsicMatrix &K, int width, int height, View &out, float near_z = 0.0f) {
    const dvo_amd_view v = view(K, width, height, near_z);
    const size_t n = width > 0 && height > 0 ? (size_t)width * (size_t)height : 0;
    out.width = width, out.height = height;
    out.depth.resize(n), out.intensity.resize(n), out.rgb.resize(n), out.index.resize(n);
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_render(map_, core::data(pose), &v, out.depth.data(), out.rgb.data(), out.intensity.data(),
                                            out.index.data(), &out.stats),
                         "KeyframeMap::render");
  }
  // the same view as a pyramid built on the device from the rendered planes: a reference any tracker entry accepts
  core::RgbdImagePyramidPtr renderPyramid(const core::AffineTransformd &pose, const core::IntrinsicMatrix &K, int width, int height,
                                          int levels, float near_z = 0.0f, double timestamp = 0.0) {
    const dvo_amd_view v = view(K, width, height, near_z);
    dvo_amd_pyramid *pyr = nullptr;
    std::unique_lock<std::mutex> lock;
    (void)core::cloud::context(device_, lock);
    ::dvo::detail::check(dvo_amd_map_render_pyramid(map_, core::data(pose), &v, levels, timestamp, &pyr, nullptr),
                         "KeyframeMap::renderPyramid");
    return core::RgbdImagePyramidPtr(new core::RgbdImagePyramid(pyr, width, height, K, device_, timestamp));
  }

  dvo_amd_map *handle() const { return map_; }

 private:
  int device_;
  dvo_amd_map *map_;
  float leaf_;
};

// The signed-distance volume kept on the device (dvo_amd.h: dvo_amd_volume_*), next to KeyframeMap: keyframes are fused into a
// dense grid of integer sums -- inserted, moved and removed exactly --, raycast() gives a hole-free model view, raycastPyramid()
// the same view as a reference any tracker entry accepts, extract() the surface crossings as a cloud.  Context-free: it needs no
// tracker; calls on one volume are serialised by the caller.
class SurfaceVolume {
 public:
  typedef AsyncPointCloudBuilder::PointCloud PointCloud;

  // a raycast view: width * height values per plane, row-major; empty pixels hold NaN (weight 0)
  struct View {
    int width, height;
    std::vector<float> depth, intensity;
    std::vector<int> weight;
    dvo_amd_volume_raycast_stats stats;
  };

  static dvo_amd_volume_options defaultOptions() {
    dvo_amd_volume_options o;
    dvo_amd_default_volume_options(&o);
    return o;
  }
  static dvo_amd_volume_raycast_options defaultRaycastOptions() {
    dvo_amd_volume_raycast_options o;
    dvo_amd_default_volume_raycast_options(&o);
    return o;
  }

  explicit SurfaceVolume(const dvo_amd_volume_options &options = defaultOptions(), int device = 0)
      : device_(device), volume_(nullptr), options_(options) {
    ::dvo::detail::check(dvo_amd_volume_create(device, &options, &volume_), "SurfaceVolume");
  }
  ~SurfaceVolume() { dvo_amd_volume_destroy(volume_); }
  SurfaceVolume(const SurfaceVolume &) = delete;
  SurfaceVolume &operator=(const SurfaceVolume &) = delete;

  const dvo_amd_volume_options &options() const { return options_; }

  // the anonymous form: `level` of every frame at its pose (camera -> world), added (sign +1) or subtracted (-1) in one launch
  std::vector<dvo_amd_volume_counts> integrate(const std::vector<core::RgbdImagePyramid *> &frames,
                                               const std::vector<core::AffineTransformd> &poses, int level = 0, int sign = 1) {
    std::vector<dvo_amd_pyramid *> handles;
    std::vector<double> flat;
    pack("SurfaceVolume::integrate", frames, poses, level, handles, flat);
    std::vector<dvo_amd_volume_counts> counts(frames.size());
    ::dvo::detail::check(dvo_amd_volume_integrate(volume_, (int)frames.size(), handles.data(), level, flat.data(), sign, counts.data()),
                         "SurfaceVolume::integrate");
    return counts;
  }
  // the tracked form: the volume retains the pyramids until remove()
  std::vector<dvo_amd_volume_counts> insert(const std::vector<int> &ids, const std::vector<core::RgbdImagePyramid *> &frames,
                                            const std::vector<core::AffineTransformd> &poses, int level = 0) {
    if (ids.size() != frames.size()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SurfaceVolume::insert: one id per frame");
    std::vector<dvo_amd_pyramid *> handles;
    std::vector<double> flat;
    pack("SurfaceVolume::insert", frames, poses, level, handles, flat);
    std::vector<dvo_amd_volume_counts> counts(frames.size());
    ::dvo::detail::check(dvo_amd_volume_insert(volume_, (int)frames.size(), ids.data(), handles.data(), level, flat.data(), counts.data()),
                         "SurfaceVolume::insert");
    return counts;
  }
  void set_poses(const std::vector<int> &ids, const std::vector<core::AffineTransformd> &poses) {
    if (ids.size() != poses.size()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, "SurfaceVolume::set_poses: one pose per id");
    std::vector<double> flat;
    for (size_t i = 0; i < poses.size(); ++i) flat.insert(flat.end(), core::data(poses[i]), core::data(poses[i]) + 16);
    ::dvo::detail::check(dvo_amd_volume_set_poses(volume_, (int)ids.size(), ids.data(), flat.data()), "SurfaceVolume::set_poses");
  }
  void remove(const std::vector<int> &ids) {
    ::dvo::detail::check(dvo_amd_volume_remove(volume_, (int)ids.size(), ids.data()), "SurfaceVolume::remove");
  }
  void clear() { ::dvo::detail::check(dvo_amd_volume_clear(volume_), "SurfaceVolume::clear"); }
  long long stats(int *n_keyframes = nullptr) const {
    long long updated = 0;
    ::dvo::detail::check(dvo_amd_volume_stats(volume_, n_keyframes, &updated), "SurfaceVolume::stats");
    return updated;
  }

  // the records of the inclusive index box {x0,y0,z0,x1,y1,z1} (null: the whole volume), x fastest
  void download(std::vector<dvo_amd_volume_voxel> &out, const int *box = nullptr) {
    long long n = 0;
    int rc = dvo_amd_volume_download(volume_, box, nullptr, 0, &n);
    if (rc == DVO_AMD_ERR_CAPACITY) {
      out.resize((size_t)n);
      rc = dvo_amd_volume_download(volume_, box, out.data(), (long long)out.size(), &n);
    }
    ::dvo::detail::check(rc, "SurfaceVolume::download");
    out.resize((size_t)n);
  }

  // near_z <= 0: the volume's near_z
  dvo_amd_view view(const core::IntrinsicMatrix &K, int width, int height, float near_z = 0.0f) const {
    dvo_amd_view v;
    v.width = width, v.height = height, v.fx = K.fx(), v.fy = K.fy(), v.ox = K.ox(), v.oy = K.oy();
    v.near_z = near_z > 0.0f ? near_z : options_.near_z;
    return v;
  }
  void raycast(const core::AffineTransformd &pose, const core::IntrinsicMatrix &K, int width, int height, View &out, float near_z = 0.0f,
               const dvo_amd_volume_raycast_options &options = defaultRaycastOptions()) {
    const dvo_amd_view v = view(K, width, height, near_z);
    const size_t n = width > 0 && height > 0 ? (size_t)width * (size_t)height : 0;
    out.width = width, out.height = height;
    out.depth.resize(n), out.intensity.resize(n), out.weight.resize(n);
    ::dvo::detail::check(dvo_amd_volume_raycast(volume_, core::data(pose), &v, &options, out.depth.data(), out.intensity.data(),
                                                out.weight.data(), &out.stats),
                         "SurfaceVolume::raycast");
  }
  core::RgbdImagePyramidPtr raycastPyramid(const core::AffineTransformd &pose, const core::IntrinsicMatrix &K, int width, int height,
                                           int levels, float near_z = 0.0f,
                                           const dvo_amd_volume_raycast_options &options = defaultRaycastOptions(), double timestamp = 0.0,
                                           dvo_amd_volume_raycast_stats *stats = nullptr) {
    const dvo_amd_view v = view(K, width, height, near_z);
    dvo_amd_pyramid *pyr = nullptr;
    ::dvo::detail::check(dvo_amd_volume_raycast_pyramid(volume_, core::data(pose), &v, &options, levels, timestamp, &pyr, stats),
                         "SurfaceVolume::raycastPyramid");
    try {
      return core::RgbdImagePyramidPtr(new core::RgbdImagePyramid(pyr, width, height, K, device_, timestamp));
    } catch (...) {  // (the adopting object was never made: the handle is still ours)
      dvo_amd_pyramid_release(pyr);
      throw;
    }
  }

  // the surface crossings in ascending 3*L + a
  void records(std::vector<dvo_amd_point> &out, int min_weight = 1, dvo_amd_volume_extract_counts *counts = nullptr) {
    long long n = 0;
    int rc = dvo_amd_volume_extract(volume_, min_weight, nullptr, 0, &n, counts);
    if (rc == DVO_AMD_ERR_CAPACITY) {
      out.resize((size_t)n);
      rc = dvo_amd_volume_extract(volume_, min_weight, out.data(), (long long)out.size(), &n, counts);
    }
    ::dvo::detail::check(rc, "SurfaceVolume::extract");
    out.resize((size_t)n);
  }
  PointCloud::Ptr extract(int min_weight = 1) {
    std::vector<dvo_amd_point> points;
    records(points, min_weight);
    PointCloud::Ptr out(new PointCloud);
    out->reserve(points.size());
    for (size_t i = 0; i < points.size(); ++i) out->points.push_back(detail::from_record(points[i]));
    out->width = (std::uint32_t)points.size(), out->height = 1;
    return out;
  }

  // the surface as an indexed triangle mesh (dvo_amd_volume_mesh: surface nets, one vertex per active cell, two triangles per
  // crossing edge whose four cells are known); normals: 3 floats per vertex, triangles: 3 vertex indices each
  struct Mesh {
    std::vector<dvo_amd_point> vertices;
    std::vector<float> normals;
    std::vector<int> triangles;
    dvo_amd_volume_mesh_counts counts;
  };
  void extractMesh(Mesh &out, int min_weight = 1, bool with_normals = true) {
    int rc = dvo_amd_volume_mesh(volume_, min_weight, nullptr, nullptr, 0, nullptr, 0, &out.counts);
    if (rc == DVO_AMD_ERR_CAPACITY) {
      out.vertices.resize((size_t)out.counts.vertices), out.triangles.resize(3 * (size_t)out.counts.triangles);
      out.normals.resize(with_normals ? 3 * (size_t)out.counts.vertices : 0);
      rc = dvo_amd_volume_mesh(volume_, min_weight, out.vertices.data(), with_normals ? out.normals.data() : nullptr,
                               (long long)out.vertices.size(), out.triangles.data(), (long long)(out.triangles.size() / 3), &out.counts);
    }
    ::dvo::detail::check(rc, "SurfaceVolume::extractMesh");
    out.vertices.resize((size_t)out.counts.vertices), out.triangles.resize(3 * (size_t)out.counts.triangles);
    out.normals.resize(with_normals ? 3 * (size_t)out.counts.vertices : 0);
  }
  // a mesh as a binary little-endian PLY file (dvo_amd_write_ply), with normals when the mesh holds them
  static void writePly(const std::string &path, const Mesh &mesh) {
    ::dvo::detail::check(dvo_amd_write_ply(path.c_str(), mesh.vertices.data(), mesh.normals.empty() ? nullptr : mesh.normals.data(),
                                           (long long)mesh.vertices.size(), mesh.triangles.data(), (long long)(mesh.triangles.size() / 3)),
                         "SurfaceVolume::writePly");
  }
  // the inverse of download(): the records of the box (null: the whole volume) are overwritten; refused while keyframes are held
  void upload(const std::vector<dvo_amd_volume_voxel> &records, const int *box = nullptr) {
    ::dvo::detail::check(dvo_amd_volume_upload(volume_, box, records.data(), (long long)records.size()), "SurfaceVolume::upload");
  }

  dvo_amd_volume *handle() const { return volume_; }

 private:
  static void pack(const char *where, const std::vector<core::RgbdImagePyramid *> &frames, const std::vector<core::AffineTransformd> &poses,
                   int level, std::vector<dvo_amd_pyramid *> &handles, std::vector<double> &flat) {
    if (frames.size() != poses.size()) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
    for (size_t i = 0; i < frames.size(); ++i) {
      if (!frames[i]) throw DvoAmdError(DVO_AMD_ERR_INVALID_ARGUMENT, where);
      frames[i]->build((size_t)(level < 0 ? 0 : level) + 1);
      handles.push_back(frames[i]->handle());
      flat.insert(flat.end(), core::data(poses[i]), core::data(poses[i]) + 16);
    }
    if (flat.empty()) flat.resize(16);  // (n == 0: the entries still want arrays)
  }

  int device_;
  dvo_amd_volume *volume_;
  dvo_amd_volume_options options_;
};

}  // namespace visualization
}  // namespace dvo

#endif  // DVO_AMD_POINT_CLOUD_HPP_
