// dvo::visualization::KeyframeMap (include/dvo_amd/point_cloud.hpp) the way a viewer of a running SLAM session uses it: a
// keyframe is inserted when it is created, moved when the graph optimizer has moved it, removed when it is dropped, and the
// map is extracted after each event -- without PointCloudAggregator::build()'s rebuild.  Synthetic frames, no input files.
//   g++ -std=c++11 -Iinclude/dvo_amd_compat -Iinclude examples/keyframe_map_adaptor_example.cpp -Ldvo_slam_amd -ldvo_amd
#include <dvo/core/rgbd_image.h>
#include <dvo/visualization/point_cloud_aggregator.h>

#include <cstdio>
#include <vector>

int main() try {
  using namespace dvo;
  typedef visualization::KeyframeMap Map;
  const int w = 160, h = 120;
  core::IntrinsicMatrix K = core::IntrinsicMatrix::create(131.25f, 131.25f, 79.5f, 59.5f);
  core::RgbdCameraPyramid camera(w, h, K);
  std::vector<core::RgbdImagePyramidPtr> frames;
  Map map(0.02f);
  core::AffineTransformd identity;
  identity.setIdentity();  // (Eigen's default constructor leaves the matrix unset)
  for (int k = 0; k < 3; ++k) {
    std::vector<float> grey((size_t)w * h), depth((size_t)w * h);
    for (int v = 0; v < h; ++v)
      for (int u = 0; u < w; ++u) grey[(size_t)v * w + u] = (float)((u + v + 10 * k) % 256), depth[(size_t)v * w + u] = 1.5f + 0.002f * u + 0.1f * k;
    frames.push_back(camera.create(grey.data(), depth.data()));
    map.insert(k, Map::BuildJob(frames.back()->level(0), identity));
    std::printf("insert %d: %zu points\n", k, map.extract()->size());
  }
  core::AffineTransformd moved = identity;
  core::data(moved)[12] = 0.05;  // a translation along x (column-major)
  map.set_pose(1, moved);
  std::printf("move 1: %zu points\n", map.extract()->size());
  map.remove(0);
  const float box[6] = {-0.5f, -0.5f, 0.0f, 0.5f, 0.5f, 3.0f};
  std::printf("remove 0: %zu points, %zu in the box, %lld voxels\n", map.extract()->size(), map.extract(box)->size(), map.stats().voxels);
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "%s\n", e.what());
  return 1;
}
