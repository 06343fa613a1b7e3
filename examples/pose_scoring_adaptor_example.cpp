// Pose scoring through the C++ adaptor: a start for an alignment whose relative pose is not known.
//   first     the current frame aligned against the reference from the identity: whatever pose it ends at, its coarsest level
//             holds a precision of the residuals (dvo::DenseTracker::PoseScoreOptions takes it from the result's statistics)
//   grid      15 hypotheses around the identity: five yaws in steps of 5 degrees, three shifts along x in steps of 10 cm
//   scores    dvo::DenseTracker::scorePoses at the coarsest level, rankPoses for the three of smallest total
//   seeds     dvo_slam::seedProposals for the same pair as keyframes: its proposal carries the top hypothesis
//   seeded    the alignment again, started from the best hypothesis
// Prints the three ranked hypotheses with their sums and a checksum of the seeded pose -- what examples/pose_scoring_example.c
// does through the C ABI.  Input files: float32 planes without a header, as tests/test_pose_scoring_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvo_amd/constraints.hpp"
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
    std::fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z\n", argv[0]);
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
  const int coarsest = cfg.FirstLevel;

  dvo::DenseTracker::Result first;
  tracker.match(*frame[0], *frame[1], first);
  const dvo::DenseTracker::PoseScoreOptions options(coarsest, first);

  dvo_amd_pose_grid_options axes;
  for (int a = 0; a < 6; ++a) axes.count[a] = 1, axes.step[a] = 0.0;
  axes.count[0] = 3, axes.step[0] = 0.1;                                   // vx
  axes.count[4] = 5, axes.step[4] = 5.0 * 3.14159265358979323846 / 180.0;  // wy: yaw
  dvo::core::AffineTransformd identity;
  identity.setIdentity();
  const std::vector<dvo::core::AffineTransformd> grid = dvo::DenseTracker::poseGrid(axes, identity);

  const std::vector<dvo::DenseTracker::PoseScore> scores = tracker.scorePoses(*frame[0], *frame[1], grid, options);
  const std::vector<int> order = dvo::DenseTracker::rankPoses(scores, 3);
  for (size_t r = 0; r < order.size(); ++r) {
    const dvo::DenseTracker::PoseScore &s = scores[(size_t)order[r]];
    std::printf("rank %zu hypothesis %d evaluated %lld invalid %lld inlier %lld outlier %lld cost %llu total %llu\n", r, order[r],
                s.evaluated, s.invalid, s.inlier, s.outlier, s.cost, s.total);
  }

  // the same pair as keyframes: the proposal the validator would be handed starts at the top hypothesis
  dvo_slam::KeyframeVector keyframes;
  for (int k = 0; k < 2; ++k) {
    dvo_slam::KeyframePtr kf(new dvo_slam::Keyframe());
    kf->id(k).image(frame[(size_t)k]).pose(identity);
    keyframes.push_back(kf);
  }
  const dvo_slam::constraints::ConstraintProposalVector seeds =
      dvo_slam::seedProposals(tracker, keyframes[0], dvo_slam::KeyframeVector(1, keyframes[1]), grid, options, 1);
  if (seeds.size() != 1 || std::memcmp(dvo::core::data(seeds[0]->InitialTransformation), dvo::core::data(grid[(size_t)order[0]]),
                                       sizeof(double) * 16) != 0) {
    std::fprintf(stderr, "seedProposals does not carry the top hypothesis\n");
    return 1;
  }

  cfg.UseInitialEstimate = true;
  tracker.configure(cfg);
  dvo::DenseTracker::Result seeded;
  seeded.Transformation = seeds[0]->InitialTransformation;
  tracker.match(*frame[0], *frame[1], seeded);
  const double *T = dvo::core::data(seeded.Transformation);
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  std::printf("seeded checksum %.17g isnan %d\n", sum, seeded.isNaN() ? 1 : 0);
  return 0;
}
