// The signed-distance volume through the C++ adaptor (dvo::visualization::SurfaceVolume, next to KeyframeMap): two frames fused
// into a volume, the volume raycast and its surface pulled.
//   match     the second frame aligned against the first: the transformation, as returned, is the second frame's pose in the
//             first frame's world
//   insert    both frames as keyframes 0 and 1 in one call: the counts of each
//   raycast   the volume seen from the first frame's camera: stats and a checksum of the depth plane
//   extract   the surface crossings
//   track     the same view as a pyramid (raycastPyramid), the second frame tracked against the model
// Prints counts and checksums -- what examples/volume_example.c prints through the C ABI.  Input files: float32 planes without a
// header, as tests/test_volume_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvo_amd/dense_tracking.hpp"
#include "dvo_amd/point_cloud.hpp"

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
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy first_i first_z second_i second_z\n", argv[0]);
    return 2;
  }
  typedef dvo::core::RgbdImagePyramid Pyramid;
  typedef dvo::visualization::SurfaceVolume Volume;
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
  dvo::DenseTracker::Result result;
  tracker.match(*frame[0], *frame[1], result);

  Volume volume;
  std::vector<int> ids;
  std::vector<Pyramid *> frames;
  std::vector<dvo::core::AffineTransformd> poses(2);
  poses[0].setIdentity();
  poses[1] = result.Transformation;
  for (int k = 0; k < 2; ++k) ids.push_back(k), frames.push_back(frame[k].get());
  const std::vector<dvo_amd_volume_counts> counts = volume.insert(ids, frames, poses);
  std::printf("insert counts %lld %lld %lld %lld %lld %lld\n", counts[0].updated, counts[0].near, counts[0].free, counts[1].updated,
              counts[1].near, counts[1].free);

  Volume::View view;
  volume.raycast(poses[0], K, w, h, view);
  std::printf("raycast stats %lld %lld %lld %lld %lld\n", view.stats.pixels, view.stats.hit, view.stats.backface, view.stats.missed,
              view.stats.uncoloured);
  double sum = 0.0;
  for (size_t i = 0; i < view.depth.size(); ++i)
    if (view.depth[i] == view.depth[i]) sum += view.depth[i];  // (NaN: not hit)
  std::printf("raycast checksum %.17g\n", sum);

  std::vector<dvo_amd_point> points;
  dvo_amd_volume_extract_counts ec;
  volume.records(points, 1, &ec);
  sum = 0.0;
  for (size_t i = 0; i < points.size(); ++i) sum += points[i].x;
  std::printf("extract counts %lld %lld checksum %.17g\n", ec.points, ec.uncoloured, sum);

  const int levels = (int)cfg.FirstLevel + 1;
  const dvo::core::RgbdImagePyramidPtr model =
      volume.raycastPyramid(poses[0], K, w, h, levels, 0.0f, Volume::defaultRaycastOptions(), 2.0);
  dvo::DenseTracker::Result left;
  tracker.match(*model, *frame[1], left);
  const double *T = dvo::core::data(left.Transformation);
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("track checksum %.17g isnan %d\n", sum, left.isNaN() ? 1 : 0);
  return 0;
}
