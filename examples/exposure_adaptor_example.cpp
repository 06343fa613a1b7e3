// Exposure compensation through the C++ adaptor: a current frame whose camera changed its exposure is aligned against a reference.
//   plain        dvo::DenseTracker::match on the frame as it is
//   estimate     dvo::core::RgbdImagePyramid::estimateExposure on the current frame, at the identity: I_ref ~ gain * I_cur + bias
//   compensated  dvo::DenseTracker::matchCompensated: estimate, RgbdImagePyramid::adjustIntensity, match -- one round
// Prints the estimate with its sums and a checksum of both poses -- what examples/exposure_example.c does through the C ABI.
// Input files: float32 planes without a header, as tests/test_exposure_adaptor.py writes them.
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

static double checksum(const dvo::core::AffineTransformd &T) {
  const double *t = dvo::core::data(T);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += t[k];
  return sum;
}

static int run(char **argv) {
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
  dvo::DenseTracker tracker(dvo::DenseTracker::getDefaultConfig());

  dvo::DenseTracker::Result plain;
  tracker.match(*frame[0], *frame[1], plain);
  std::printf("plain checksum %.17g isnan %d\n", checksum(plain.Transformation), plain.isNaN() ? 1 : 0);

  // the estimate on its own (no transformation: the identity; no mask), in the tracker's context
  const dvo::core::ExposureEstimate e = frame[1]->estimateExposure(*frame[0], nullptr, nullptr, dvo::core::ExposureOptions(), tracker.handle());
  std::printf("estimate gain %.17g bias %.17g r2 %.17g passes %d degenerate %d\n", e.gain, e.bias, e.r2, e.passes, e.degenerate);
  std::printf("counts valid %lld consistent %lld masked %lld saturated %lld candidates %lld used %lld trimmed %lld\n", e.valid, e.consistent,
              e.masked, e.saturated, e.candidates, e.used, e.trimmed);
  std::printf("sums n %lld sx %lld sy %lld sxx %lld sxy %lld syy %lld\n", e.n, e.sx, e.sy, e.sxx, e.sxy, e.syy);

  dvo::DenseTracker::Result compensated;
  std::vector<dvo::core::ExposureEstimate> estimates;
  dvo::core::RgbdImagePyramidPtr adjusted;
  tracker.matchCompensated(*frame[0], *frame[1], compensated, dvo::core::ExposureOptions(), 1, &estimates, &adjusted);
  if (estimates.size() != 1 || estimates[0].gain != e.gain || estimates[0].bias != e.bias || !adjusted) return 3;
  std::printf("compensated checksum %.17g isnan %d\n", checksum(compensated.Transformation), compensated.isNaN() ? 1 : 0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z\n", argv[0]);
    return 2;
  }
  try {
    return run(argv);
  } catch (const std::exception &e) {  // (a DvoAmdError carries the entry, the status and the library's reason)
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
