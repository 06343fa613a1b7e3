// Surface normals through the C++ adaptor: which way the surfaces of a keyframe face, and what that is good for.
//   normals   RgbdImage::calculateNormals(), RgbdImage::normals and RgbdImage::angles of level 0: the reference's members
//   facing    dvo::core::SelectionMask::fromNormals: the pixels whose windowed normal looks at the camera, every level at once
//   track     the mask eroded by a pixel, the next frame tracked behind it as a PointSelection like any other
//   cloud     AsyncPointCloudBuilder::BuildJob::buildWithNormals: the keyframe's cloud as PointXYZRGBNormal
// Prints the counts, the kept pixels and a checksum of the pose -- what examples/normals_example.c does through the C ABI -- and
// writes level 0's normals, its angles and the facing mask's planes to `out`.  Input files: float32 planes without a header, as
// tests/test_normals_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <dvo/visualization/async_point_cloud_builder.h>

#include "dvo_amd/dense_tracking.hpp"

static std::vector<float> read_plane(const char *path, size_t n) {
  std::vector<float> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

int main(int argc, char **argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z out.bin\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  std::vector<dvo::core::RgbdImagePyramidPtr> frame;
  for (int k = 0; k < 2; ++k) {
    std::vector<float> i = read_plane(argv[7 + 2 * k], n), z = read_plane(argv[8 + 2 * k], n);
    frame.push_back(camera.create(i.data(), z.data()));
  }
  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  dvo::DenseTracker tracker(cfg);
  const size_t levels = cfg.getNumLevels();
  frame[0]->build(levels), frame[1]->build(levels);

  // the reference's members, used the way the reference's callers use them
  dvo::core::RgbdImage &image = frame[0]->level(0);
  image.calculateNormals();
  std::vector<float> normals(4 * n), angles(n);
#ifdef DVO_AMD_HAVE_OPENCV
  for (int y = 0; y < h; ++y) {
    const float *nr = image.normals.ptr<float>(y), *ar = image.angles.ptr<float>(y);
    for (int x = 0; x < w; ++x) {
      for (int c = 0; c < 4; ++c) normals[4 * ((size_t)y * w + x) + c] = nr[4 * x + c];
      angles[(size_t)y * w + x] = ar[x];
    }
  }
#else
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      for (int c = 0; c < 4; ++c) normals[4 * ((size_t)y * w + x) + c] = image.normals(y, x, c);
      angles[(size_t)y * w + x] = image.angles(y, x);
    }
#endif
  long long defined = 0;
  for (size_t p = 0; p < n; ++p) defined += normals[4 * p + 3] == 0.0f ? 1 : 0;  // (NaN where there is no normal)
  std::printf("normals counts %lld %lld\n", defined, (long long)n - defined);

  // a 7x7 window on level 0, smaller ones above it, members within 2 % of the centre's depth; facing = cosine to the viewing ray
  dvo::core::SelectionMask::NormalOptions options;
  for (size_t l = 0; l < levels; ++l) options.radius[l] = l < 3 ? 3 - (int)l : 0;
  options.depth_step_ratio = 0.02f, options.facing = DVO_AMD_NORMAL_FACING_RAY, options.toward_camera = 1;
  std::vector<dvo::core::SelectionMask::NormalCounts> counts;
  const dvo::core::SelectionMask facing = dvo::core::SelectionMask::fromNormals(*frame[0], std::vector<float>(1, 0.5f), options, false, &counts);
  for (size_t l = 0; l < counts.size(); ++l)
    std::printf("mask counts %zu %lld %lld %lld\n", l, counts[l].defined, counts[l].undefined, counts[l].kept);
  const dvo::core::SelectionMask eroded = facing.eroded(1);
  const dvo::core::SelectionMask::Info info = eroded.info();
  for (size_t l = 0; l < levels; ++l) std::printf("eroded kept %zu %lld\n", l, info.kept[l]);

  dvo::core::MaskedGradientThresholdPredicate predicate(eroded, cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold);
  dvo::core::PointSelection selection(*frame[0], predicate);
  dvo::DenseTracker::Result result;
  tracker.match(selection, *frame[1], result);
  const double *T = dvo::core::data(result.Transformation);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("track checksum %.17g isnan %d\n", sum, result.isNaN() ? 1 : 0);

  FILE *out = std::fopen(argv[11], "wb");
  if (!out || std::fwrite(normals.data(), 16, n, out) != n || std::fwrite(angles.data(), 4, n, out) != n) return 2;
  for (size_t l = 0; l < levels; ++l) {
    const std::vector<unsigned char> bytes = facing.download((int)l);
    if (std::fwrite(bytes.data(), 1, bytes.size(), out) != bytes.size()) return 2;
  }
  // the keyframe's cloud with the windowed normals: x y z, colour, normal per point
  dvo::core::AffineTransformd identity;
  identity.setIdentity();  // (an Eigen transform is not initialised by its constructor)
  dvo::visualization::AsyncPointCloudBuilder::BuildJob job(image, identity);
  const dvo::visualization::AsyncPointCloudBuilder::BuildJob::NormalCloud::Ptr cloud = job.buildWithNormals(options);
  std::vector<float> cloud_normals(3 * cloud->size());
  for (size_t p = 0; p < cloud->size(); ++p)
    cloud_normals[3 * p] = cloud->points[p].normal_x, cloud_normals[3 * p + 1] = cloud->points[p].normal_y,
                      cloud_normals[3 * p + 2] = cloud->points[p].normal_z;
  if (std::fwrite(cloud_normals.data(), 12, cloud->size(), out) != cloud->size() || std::fclose(out) != 0) return 2;
  std::printf("cloud points %zu\n", cloud->size());
  return 0;
}
