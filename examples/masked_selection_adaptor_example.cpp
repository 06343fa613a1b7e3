// Masked point selections through the C++ adaptor, two ways.
//   user    a user-defined PointSelectionPredicate written the way a caller of the reference writes one
//           (point_selection.h:32-37): isPointOk sees the pixel's position and drops a rectangle.  It has no device form, so
//           PointSelection evaluates it on the host once per pyramid and tracks behind the resulting device mask.
//   masked  dvo::core::MaskedGradientThresholdPredicate: a device mask whose level 0 drops the same rectangle (the coarser
//           levels derived on the device, conservative rule) next to the two gradient thresholds -- what
//           examples/masked_selection_example.c does through the C ABI.
// Prints the selected pixels per level and a checksum of the pose for both.  Input files: float32 planes without a header, as
// tests/test_selection_mask_adaptor.py writes them.
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

// a valid point outside the rectangle [x0, x1) x [y0, y1) -- in the pixel coordinates of whichever level is being selected, as
// in the reference, which calls the predicate per level with that level's x and y
class OutsideRectanglePredicate : public dvo::core::PointSelectionPredicate {
 public:
  size_t x0, y0, x1, y1;
  OutsideRectanglePredicate(size_t x0_, size_t y0_, size_t x1_, size_t y1_) : x0(x0_), y0(y0_), x1(x1_), y1(y1_) {}
  virtual ~OutsideRectanglePredicate() {}
  virtual bool isPointOk(const size_t &x, const size_t &y, const float &z, const float &, const float &, const float &zdx,
                         const float &zdy) const {
    const bool inside = x >= x0 && x < x1 && y >= y0 && y < y1;
    return z == z && zdx == zdx && zdy == zdy && !inside;
  }
};

static void report(const char *tag, dvo::core::PointSelection &selection, const dvo::DenseTracker::Result &result, size_t levels) {
  for (size_t l = 0; l < levels; ++l) std::printf("%s count %zu %zu\n", tag, l, selection.size(l));
  const double *T = dvo::core::data(result.Transformation);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("%s checksum %.17g isnan %d\n", tag, sum, result.isNaN() ? 1 : 0);
}

int main(int argc, char **argv) {
  if (argc < 15) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z x0 y0 x1 y1\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));
  std::vector<float> ri = read_plane(argv[7], n), rz = read_plane(argv[8], n), ci = read_plane(argv[9], n), cz = read_plane(argv[10], n);
  const int x0 = std::atoi(argv[11]), y0 = std::atoi(argv[12]), x1 = std::atoi(argv[13]), y1 = std::atoi(argv[14]);

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  dvo::core::RgbdImagePyramidPtr reference = camera.create(ri.data(), rz.data());
  dvo::core::RgbdImagePyramidPtr current = camera.create(ci.data(), cz.data());

  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  cfg.LastLevel = 0;
  dvo::DenseTracker tracker(cfg);
  const size_t levels = cfg.getNumLevels();

  {
    OutsideRectanglePredicate predicate((size_t)x0, (size_t)y0, (size_t)x1, (size_t)y1);
    dvo::core::PointSelection selection(*reference, predicate);
    dvo::DenseTracker::Result result;
    tracker.match(selection, *current, result);
    report("user", selection, result, levels);
  }
  {
    std::vector<unsigned char> keep(n);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) keep[(size_t)y * w + x] = !(x >= x0 && x < x1 && y >= y0 && y < y1);
    dvo::core::MaskedGradientThresholdPredicate predicate(
        dvo::core::SelectionMask::fromLevel0(w, h, (int)levels, keep.data(), 0, dvo::core::SelectionMask::All),
        cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold);
    dvo::core::PointSelection selection(*reference, predicate);
    dvo::DenseTracker::Result result;
    tracker.match(selection, *current, result);
    report("masked", selection, result, levels);
  }
  return 0;
}
