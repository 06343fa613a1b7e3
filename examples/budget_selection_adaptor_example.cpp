// Point-budget selections through the C++ adaptor: dvo::core::SelectionMask::topK and ::grid rank the reference pixels on the
// device and return the SelectionMask a MaskedGradientThresholdPredicate holds, so a budgeted alignment is a PointSelection like
// any other.
//   plain  the tracker's own selection
//   topk   the k0 strongest points of level 0, a quarter of the budget on every coarser level
//   grid   one point per cell x cell cell on every level
// Prints the selected pixels per level and a checksum of the pose for each -- what examples/budget_selection_example.c does
// through the C ABI.  Input files: float32 planes without a header, as tests/test_budget_selection_adaptor.py writes them.
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

static void report(const char *tag, const dvo::DenseTracker::Result &result) {
  const double *T = dvo::core::data(result.Transformation);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("%s checksum %.17g isnan %d\n", tag, sum, result.isNaN() ? 1 : 0);
}

static void track(const char *tag, dvo::DenseTracker &tracker, dvo::core::RgbdImagePyramid &reference,
                  dvo::core::RgbdImagePyramid &current, const dvo::core::SelectionMask &mask, size_t levels) {
  const dvo::DenseTracker::Config &cfg = tracker.configuration();
  const dvo::core::SelectionMask::Info info = mask.info();
  for (size_t l = 0; l < levels; ++l) std::printf("%s kept %zu %lld\n", tag, l, info.kept[l]);
  dvo::core::MaskedGradientThresholdPredicate predicate(mask, cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold);
  dvo::core::PointSelection selection(reference, predicate);
  dvo::DenseTracker::Result result;
  tracker.match(selection, current, result);
  report(tag, result);
}

int main(int argc, char **argv) {
  if (argc < 13) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z k0 cell\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));
  std::vector<float> ri = read_plane(argv[7], n), rz = read_plane(argv[8], n), ci = read_plane(argv[9], n), cz = read_plane(argv[10], n);
  const long long k0 = std::atoll(argv[11]);
  const int cell = std::atoi(argv[12]);

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  dvo::core::RgbdImagePyramidPtr reference = camera.create(ri.data(), rz.data());
  dvo::core::RgbdImagePyramidPtr current = camera.create(ci.data(), cz.data());

  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  cfg.LastLevel = 0;
  dvo::DenseTracker tracker(cfg);
  const size_t levels = cfg.getNumLevels();

  {
    dvo::DenseTracker::Result result;
    tracker.match(*reference, *current, result);
    report("plain", result);
  }
  // the candidates are what the tracker's own thresholds select; the budget thins them
  std::vector<long long> budgets(levels);
  for (size_t l = 0; l < levels; ++l) budgets[l] = k0 >> (2 * l);
  track("topk", tracker, *reference, *current,
        dvo::core::SelectionMask::topK(*reference, budgets, cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold), levels);
  track("grid", tracker, *reference, *current,
        dvo::core::SelectionMask::grid(*reference, std::vector<int>(levels, cell), cfg.IntensityDerivativeThreshold,
                                       cfg.DepthDerivativeThreshold),
        levels);
  return 0;
}
