// Residual masks through the C++ adaptor: what the tracker down-weights in one alignment is cut out of the next one.
//   match     frame 1 aligned against the keyframe
//   inliers   the keyframe's pixels whose residuals at the estimate are inliers of the t-distribution
//             (dvo::core::SelectionMask::fromResiduals: the precisions come from the result's statistics)
//   eroded    ... shrunk by one pixel
//   warped    ... carried onto frame 1, the next keyframe, with the pose the match returned
//   track     frame 2 tracked against frame 1 behind the warped mask, as a PointSelection like any other
// Prints the kept pixels per level of the three masks and a checksum of the pose -- what examples/residual_mask_example.c does
// through the C ABI.  Input files: float32 planes without a header, as tests/test_residual_mask_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static void report_kept(const char *tag, const dvo::core::SelectionMask &mask, size_t levels) {
  const dvo::core::SelectionMask::Info info = mask.info();
  for (size_t l = 0; l < levels; ++l) std::printf("%s kept %zu %lld\n", tag, l, info.kept[l]);
}

int main(int argc, char **argv) {
  if (argc < 13) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z f2_i f2_z\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  std::vector<dvo::core::RgbdImagePyramidPtr> frame;
  for (int k = 0; k < 3; ++k) {
    std::vector<float> i = read_plane(argv[7 + 2 * k], n), z = read_plane(argv[8 + 2 * k], n);
    frame.push_back(camera.create(i.data(), z.data()));
  }

  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();  // level 0 is not run by default
  dvo::DenseTracker tracker(cfg);
  const size_t levels = cfg.getNumLevels();

  // the alignment whose residuals are judged (it builds both pyramids' levels)
  dvo::DenseTracker::Result first;
  tracker.match(*frame[0], *frame[1], first);
  std::vector<dvo::core::SelectionMask::ResidualCounts> counts;
  const dvo::core::SelectionMask inliers =
      dvo::core::SelectionMask::fromResiduals(tracker, *frame[0], *frame[1], first, 9.2103f, false, false, &counts);
  for (size_t l = 0; l < counts.size(); ++l)
    std::fprintf(stderr, "level %zu: evaluated %lld invalid %lld inlier %lld outlier %lld kept %lld\n", l, counts[l].evaluated,
                 counts[l].invalid, counts[l].inlier, counts[l].outlier, counts[l].kept);
  const dvo::core::SelectionMask eroded = inliers.eroded(1);
  // onto the next keyframe: source = keyframe, target = frame 1, and the transformation as the match returned it
  const dvo::core::SelectionMask warped = eroded.warped(*frame[0], *frame[1], first.Transformation);
  report_kept("inliers", inliers, levels);
  report_kept("eroded", eroded, levels);
  report_kept("warped", warped, levels);

  dvo::core::MaskedGradientThresholdPredicate predicate(warped, cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold);
  dvo::core::PointSelection selection(*frame[1], predicate);
  dvo::DenseTracker::Result result;
  tracker.match(selection, *frame[2], result);
  const double *T = dvo::core::data(result.Transformation);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("track checksum %.17g isnan %d\n", sum, result.isNaN() ? 1 : 0);
  return 0;
}
