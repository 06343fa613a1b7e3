// Loop-closure candidates by appearance through the C++ adaptor: dvo_slam::AppearanceConstraintSearch stands where
// keyframe_graph.cpp:158 puts a NearestNeighborConstraintSearch, and asks for no pose.
//   findPossibleConstraints   the keyframes that look most like keyframe 0
//   findForFrame              ... and most like a frame that is no keyframe (relocalisation)
//   dots                      the exact int32 dot products behind the scores, through the search's index
// Prints what examples/place_index_example.c prints through the C ABI.  Input files: float32 planes without a header, as
// tests/test_place_index_adaptor.py writes them; the last pair is the frame.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvo_amd/constraints.hpp"

using namespace dvo_slam;

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

static void print_found(const char *what, const KeyframeVector &found, const std::vector<double> &scores) {
  std::printf("%s:", what);
  for (size_t t = 0; t < found.size(); ++t) std::printf(" %d:%.17g", found[t]->id(), scores[t]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  const int n_files = argc - 7;
  if (argc < 7 + 4 || n_files % 2 != 0) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy kf0_i kf0_z [kf1_i kf1_z ...] frame_i frame_z\n", argv[0]);
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n_keyframes = n_files / 2 - 1;
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));
  dvo::core::RgbdCameraPyramid camera(w, h, K);

  KeyframeVector all;
  dvo::core::RgbdImagePyramid::Ptr frame;
  for (int k = 0; k <= n_keyframes; ++k) {
    std::vector<float> i = read_plane(argv[7 + 2 * k], n), z = read_plane(argv[8 + 2 * k], n);
    dvo::core::RgbdImagePyramid::Ptr image = camera.create(i.data(), z.data());
    if (k == n_keyframes) {
      frame = image;
      break;
    }
    KeyframePtr kf(new Keyframe());
    kf->id(k).image(image);  // (the pose stays unset: nothing below reads it)
    all.push_back(kf);
  }

  AppearanceConstraintSearch *appearance = new AppearanceConstraintSearch(3);
  KeyframeConstraintSearchInterfacePtr search(appearance);  // keyframe_graph.cpp:158
  KeyframeVector found;
  search->findPossibleConstraints(all, all[0], found);  // keyframe_graph.cpp:456
  int size = 0, dim = 0;
  dvo::detail::check(dvo_amd_place_index_info(appearance->index(), &size, nullptr, nullptr, &dim), "dvo_amd_place_index_info");
  std::printf("index size %d dim %d first %d\n", size, dim, 0);
  print_found("keyframe 0", found, appearance->scores());
  found.clear();
  appearance->findForFrame(all, *frame, found);
  print_found("frame", found, appearance->scores());

  std::vector<int> dots((size_t)size);
  const int keyframe = 0;
  dvo::detail::check(dvo_amd_place_scores(appearance->index(), 1, &keyframe, 0, size, dots.data()), "dvo_amd_place_scores");
  std::printf("dots:");
  for (int j = 0; j < size; ++j) std::printf(" %d", dots[(size_t)j]);
  std::printf("\n");
  return 0;
}
