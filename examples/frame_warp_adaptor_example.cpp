// Frame warps through the C++ adaptor: a frame resampled into another frame's pixels, in both directions.
//   match     the moving frame aligned against the fixed frame: the transformation, as returned, is what both warps take
//   inverse   the moving frame's grey values gathered onto the fixed frame's pixels (dvo::core::RgbdImagePyramid::warpInverse)
//   forward   the moving frame's pixels drawn into the fixed camera with a nearest-depth test (::warpForward)
//   track     the inverse warp as a pyramid with the fixed camera's depth (DVO_AMD_WARP_DEPTH_FIXED), tracked against the fixed
//             frame: what is left of the motion once the frame has been carried over
// Prints the counts and a checksum of each direction and a checksum of the pose -- what examples/frame_warp_example.c does through
// the C ABI.  Input files: float32 planes without a header, as tests/test_frame_warp_adaptor.py writes them.
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

int main(int argc, char **argv) {
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy fixed_i fixed_z moving_i moving_z\n", argv[0]);
    return 2;
  }
  typedef dvo::core::RgbdImagePyramid Pyramid;
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
  Pyramid &fixed = *frame[0], &moving = *frame[1];

  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  dvo::DenseTracker tracker(cfg);
  dvo::DenseTracker::Result result;
  tracker.match(fixed, moving, result);  // (it builds the pyramids' levels)

  Pyramid::WarpInverseCounts ic;
  const Pyramid::WarpedPlanes inverse = moving.warpInverse(fixed, result.Transformation, 0, Pyramid::WarpOptions(), &ic);
  std::printf("inverse counts %lld %lld %lld %lld %lld %lld %lld %lld\n", ic.valid, ic.behind, ic.outside, ic.border, ic.hidden, ic.warped,
              ic.partial, ic.no_depth);
  double sum = 0.0;
  for (size_t i = 0; i < inverse.intensity.size(); ++i)
    if (inverse.intensity[i] == inverse.intensity[i]) sum += inverse.intensity[i];  // (NaN: not warped)
  std::printf("inverse checksum %.17g\n", sum);

  Pyramid::WarpOptions footprint;
  footprint.splat = DVO_AMD_WARP_SPLAT_FOOTPRINT;
  Pyramid::WarpForwardCounts fc;
  const Pyramid::WarpedPlanes forward = moving.warpForward(result.Transformation, nullptr, 0, footprint, &fc);
  std::printf("forward counts %lld %lld %lld %lld %lld %lld %lld\n", fc.valid, fc.behind, fc.outside, fc.too_large, fc.drawn, fc.covered_pixels,
              fc.no_depth);
  sum = 0.0;
  long long index_sum = 0;
  for (size_t i = 0; i < forward.index.size(); ++i)
    if (forward.index[i] >= 0) sum += forward.depth[i], index_sum += forward.index[i];
  std::printf("forward checksum %.17g %lld\n", sum, index_sum);

  Pyramid::WarpOptions in_fixed_geometry;
  in_fixed_geometry.depth = DVO_AMD_WARP_DEPTH_FIXED;
  const dvo::core::RgbdImagePyramidPtr warped = moving.warpInverse(fixed, result.Transformation, in_fixed_geometry);
  dvo::DenseTracker::Result left;
  tracker.match(fixed, *warped, left);
  const double *T = dvo::core::data(left.Transformation);
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("track checksum %.17g isnan %d\n", sum, left.isNaN() ? 1 : 0);
  return 0;
}
