// Depth filtering through the C++ adaptor: two frames' depth is denoised on the device before they are tracked.
//   filter    dvo::core::RgbdImagePyramid::filterDepth on both frames: a 5x5 edge-preserving filter whose range scale is the
//             sensor's noise model, pixels fewer than four window members agree with dropped, one-pixel holes filled
//   track     the filtered frame tracked against the filtered keyframe, pyramids like any other
// Prints each frame's counts, a checksum of the keyframe's filtered depth and a checksum of the pose -- what
// examples/depth_filter_example.c does through the C ABI -- and writes the keyframe's filtered plane and its support plane to
// `out`.  Input files: float32 planes without a header, as tests/test_depth_filter_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <exception>
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

static int run(char **argv) {
  const int frames = 2;  // the keyframe and the frame tracked against it
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  std::vector<dvo::core::RgbdImagePyramidPtr> frame;
  for (int k = 0; k < frames; ++k) {
    std::vector<float> i = read_plane(argv[7 + 2 * k], n), z = read_plane(argv[8 + 2 * k], n);
    frame.push_back(camera.create(i.data(), z.data()));
  }
  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  dvo::DenseTracker tracker(cfg);

  dvo::core::RgbdImagePyramid::DepthFilterOptions options;
  options.min_support = 4, options.fill_radius = 1;
  std::vector<dvo::core::RgbdImagePyramidPtr> filtered;
  std::vector<unsigned short> support;
  for (int k = 0; k < frames; ++k) {
    frame[k]->build(cfg.getNumLevels());  // (the filter reads the pyramid the device holds)
    dvo::core::RgbdImagePyramid::DepthFilterCounts c;
    filtered.push_back(frame[k]->filterDepth(options, &c, k == 0 ? &support : nullptr));
    std::printf("filter counts %d %lld %lld %lld %lld %lld\n", k, c.with_depth, c.kept, c.dropped, c.holes, c.filled);
  }

  const std::vector<float> depth = filtered[0]->level(0).plane(1);
  double sum = 0.0;
  for (size_t i = 0; i < depth.size(); ++i)
    if (depth[i] == depth[i]) sum += depth[i];  // (NaN: no depth)
  std::printf("filtered checksum %.17g\n", sum);

  dvo::DenseTracker::Result result;
  tracker.match(*filtered[0], *filtered[1], result);
  const double *T = dvo::core::data(result.Transformation);
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("track checksum %.17g isnan %d\n", sum, result.isNaN() ? 1 : 0);

  FILE *out = std::fopen(argv[7 + 2 * frames], "wb");
  if (!out || std::fwrite(depth.data(), 4, n, out) != n || std::fwrite(support.data(), 2, n, out) != n || std::fclose(out) != 0) return 2;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z out.bin\n", argv[0]);
    return 2;
  }
  try {
    return run(argv);
  } catch (const std::exception &e) {  // (a DvoAmdError carries the entry, the status and the library's reason)
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
