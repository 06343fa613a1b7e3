// dvo::visualization::KeyframeMap::render / renderPyramid (include/dvo_amd/point_cloud.hpp): the device map seen from a pose,
// as planes on the host and as a pyramid a tracker can align a live frame to.  The wrapper's planes are compared with the C
// ABI's for the same view: the same bytes.  Synthetic frames, no input files.
//   g++ -std=c++11 -Iinclude/dvo_amd_compat -Iinclude examples/map_render_adaptor_example.cpp -Ldvo_slam_amd -ldvo_amd
#include <dvo/core/rgbd_image.h>
#include <dvo/visualization/point_cloud_aggregator.h>

#include <cstdio>
#include <cstring>
#include <vector>

int main() try {
  using namespace dvo;
  typedef visualization::KeyframeMap Map;
  const int w = 160, h = 120;
  core::IntrinsicMatrix K = core::IntrinsicMatrix::create(131.25f, 131.25f, 79.5f, 59.5f);
  core::RgbdCameraPyramid camera(w, h, K);
  std::vector<core::RgbdImagePyramidPtr> frames;
  Map map(0.02f);
  core::AffineTransformd pose;
  pose.setIdentity();
  for (int k = 0; k < 3; ++k) {
    std::vector<float> grey((size_t)w * h), depth((size_t)w * h);
    for (int v = 0; v < h; ++v)
      for (int u = 0; u < w; ++u) grey[(size_t)v * w + u] = (float)((u + v + 10 * k) % 256), depth[(size_t)v * w + u] = 1.5f + 0.002f * u + 0.1f * k;
    frames.push_back(camera.create(grey.data(), depth.data()));
    core::data(pose)[12] = 0.05 * k;  // a translation along x (column-major)
    map.insert(k, Map::BuildJob(frames.back()->level(0), pose));
  }
  core::data(pose)[12] = 0.07;  // between the second and the third keyframe
  Map::View view;
  map.render(pose, K, w, h, view);
  std::printf("render: %lld voxels, %lld drawn, %lld pixels covered\n", view.stats.voxels, view.stats.drawn, view.stats.covered_pixels);

  // the C ABI on the same map and view
  const dvo_amd_view v = map.view(K, w, h);
  const size_t n = (size_t)w * h;
  std::vector<float> depth(n), intensity(n);
  std::vector<unsigned int> rgb(n);
  std::vector<int> index(n);
  dvo_amd_render_stats st;
  ::dvo::detail::check(dvo_amd_map_render(map.handle(), core::data(pose), &v, depth.data(), rgb.data(), intensity.data(), index.data(), &st),
                       "dvo_amd_map_render");
  bool same = std::memcmp(&st, &view.stats, sizeof(st)) == 0 && std::memcmp(depth.data(), view.depth.data(), 4 * n) == 0 &&
              std::memcmp(rgb.data(), view.rgb.data(), 4 * n) == 0 && std::memcmp(intensity.data(), view.intensity.data(), 4 * n) == 0 &&
              std::memcmp(index.data(), view.index.data(), 4 * n) == 0;

  core::RgbdImagePyramidPtr model = map.renderPyramid(pose, K, w, h, 3, 0.0f, 2.5);
  std::vector<float> plane(n);
  ::dvo::detail::check(dvo_amd_pyramid_download_plane(model->handle(), 0, 0, plane.data()), "download_plane");
  same = same && std::memcmp(plane.data(), intensity.data(), 4 * n) == 0;
  ::dvo::detail::check(dvo_amd_pyramid_download_plane(model->handle(), 0, 1, plane.data()), "download_plane");
  same = same && std::memcmp(plane.data(), depth.data(), 4 * n) == 0;
  std::printf("pyramid: %d levels, level 2 is %zu x %zu, timestamp %.1f\n", dvo_amd_pyramid_levels(model->handle()), model->level(2).width,
              model->level(2).height, model->timestamp());
  model->build(4);  // more levels than were rendered: rebuilt from the adopted level 0
  ::dvo::detail::check(dvo_amd_pyramid_download_plane(model->handle(), 0, 1, plane.data()), "download_plane");
  same = same && dvo_amd_pyramid_levels(model->handle()) == 4 && std::memcmp(plane.data(), depth.data(), 4 * n) == 0;
  std::printf("equal to the C ABI: %d\n", same ? 1 : 0);
  return same ? 0 : 1;
} catch (const std::exception &e) {
  std::fprintf(stderr, "%s\n", e.what());
  return 1;
}
