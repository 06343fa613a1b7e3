// The keyframe map as dvo_slam builds it, written against the adaptor: every keyframe's image at its (optimised) pose goes into
// a PointCloudAggregator as a BuildJob under its name (graph_visualizer.cpp:255), build() picks every max(n / 50, 1)-th of
// them in name order and aggregates them (point_cloud_aggregator.cpp:74-109).  Colour images are attached the way
// camera_keyframe_tracking.cpp:252 does (float BGR).  Also prints RgbdImage::pointcloud of the first keyframe.
//
// usage: map_cloud_example W H fx fy ox oy N frames.bin out.bin
//   frames.bin: intensity f32 [N][H][W], depth f32 [N][H][W], poses f64 [N][16] (column-major), BGR f32 [N][H][W][3];
//               keyframes with an odd index get no colour image
//   out.bin:    u64 V, V x {f32 x, y, z; u8 r, g, b, 0}; u64 C, C x 4 f32 (pointcloud of keyframe 0, level 0)
#include <dvo/core/rgbd_image.h>
#include <dvo/visualization/async_point_cloud_builder.h>
#include <dvo/visualization/point_cloud_aggregator.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

int main(int argc, char **argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s W H fx fy ox oy N frames.bin out.bin\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[7]);
  const size_t px = (size_t)w * h;
  std::vector<float> I(px * n), Z(px * n), bgr(px * 3 * n);
  std::vector<double> poses(16 * (size_t)n);
  std::FILE *f = std::fopen(argv[8], "rb");
  if (!f || std::fread(I.data(), 4, I.size(), f) != I.size() || std::fread(Z.data(), 4, Z.size(), f) != Z.size() ||
      std::fread(poses.data(), 8, poses.size(), f) != poses.size() || std::fread(bgr.data(), 4, bgr.size(), f) != bgr.size()) {
    std::fprintf(stderr, "cannot read %s\n", argv[8]);
    return 1;
  }
  std::fclose(f);
  try {
    dvo::core::RgbdCameraPyramid camera(w, h, dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]),
                                                                               (float)std::atof(argv[5]), (float)std::atof(argv[6])));
    std::vector<dvo::core::RgbdImagePyramidPtr> keyframes;
    dvo::visualization::PointCloudAggregator aggregator;
    for (int k = 0; k < n; ++k) {
      keyframes.push_back(camera.create(&I[px * k], &Z[px * k]));
      dvo::core::RgbdImage &image = keyframes.back()->level(0);
      if (k % 2 == 0) {  // camera_keyframe_tracking.cpp:252: the colour image as float
#ifdef DVO_AMD_HAVE_OPENCV
        image.rgb.create(h, w, CV_MAKETYPE(CV_32F, 3));
        for (int y = 0; y < h; ++y) std::memcpy(image.rgb.ptr<float>(y), &bgr[(px * k + (size_t)y * w) * 3], sizeof(float) * 3 * w);
#else
        image.rgb.assign(bgr.begin() + px * 3 * k, bgr.begin() + px * 3 * (k + 1));
#endif
      }
      dvo::core::AffineTransformd pose;
      std::memcpy(dvo::core::data(pose), &poses[16 * (size_t)k], sizeof(double) * 16);
      aggregator.add(std::to_string(k), dvo::visualization::AsyncPointCloudBuilder::BuildJob(image, pose));
    }
    dvo::visualization::AsyncPointCloudBuilder::PointCloud::Ptr map = aggregator.build();
    const dvo::core::RgbdImage &first = keyframes.front()->level(0);
    std::FILE *o = std::fopen(argv[9], "wb");
    if (!o) return 1;
    const std::uint64_t v = map->size(), c = (std::uint64_t)first.pointcloud.cols();
    std::fwrite(&v, 8, 1, o);
    for (size_t i = 0; i < map->points.size(); ++i) {
      const dvo::visualization::PointXYZRGB &p = map->points[i];
      const unsigned char rgb[4] = {p.r, p.g, p.b, 0};
      std::fwrite(&p.x, 4, 1, o), std::fwrite(&p.y, 4, 1, o), std::fwrite(&p.z, 4, 1, o), std::fwrite(rgb, 1, 4, o);
    }
    std::fwrite(&c, 8, 1, o);
    std::fwrite(first.pointcloud.data(), 4, 4 * c, o);
    std::fclose(o);
    dvo::visualization::PointCloudAggregator empty;
    std::printf("voxels %llu pointcloud %llu x %ld empty %zu\n", (unsigned long long)v, (unsigned long long)c, first.pointcloud.rows(),
                empty.build()->size());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
