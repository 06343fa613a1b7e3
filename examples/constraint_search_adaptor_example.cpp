// The loop-closure candidate search written the way dvo_slam/src/keyframe_graph.cpp:158,233,456 uses the reference API:
// a KeyframeConstraintSearchInterface that is a NearestNeighborConstraintSearch, asked for the candidates of one keyframe.
// Without arguments: the reference's radius search on keyframes without images (needs no GPU).  With "overlap": the same
// keyframes with synthetic images (a tilted wall; keyframe 8 looks the other way) and minOverlap(0.3): this library's extension.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dvo_amd/constraints.hpp"

using namespace dvo_slam;

enum { W = 160, H = 120, N = 6, TURNED = 4 };
static const float FX = 131.25f, FY = 131.25f, OX = 79.5f, OY = 59.5f;

static void wall(double cx, std::vector<float> &grey, std::vector<float> &depth) {
  grey.resize((size_t)W * H), depth.resize((size_t)W * H);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      const double rx = (u - OX) / FX, ry = (v - OY) / FY;
      const double z = (2.0 + 0.2 * cx) / (1.0 - 0.2 * rx);
      const double x = cx + rx * z, y = ry * z;
      const int cell = ((int)(x * 8.0 + 64.0) + (int)(y * 8.0 + 64.0)) & 1;
      grey[(size_t)v * W + u] = (float)(60 + 120 * cell + (int)(40.0 * (x - (int)x)));
      depth[(size_t)v * W + u] = (float)z;
    }
}

static void print(const char *what, const KeyframeVector &found) {
  std::printf("%s:", what);
  for (size_t i = 0; i < found.size(); ++i) std::printf(" %d", found[i]->id());
  std::printf("\n");
}

int main(int argc, char **argv) {
  const bool with_overlap = argc > 1 && std::string(argv[1]) == "overlap";
  static const double place[N] = {0.0, 0.04, 0.08, 0.12, 0.06, 3.0};
  dvo::core::RgbdCameraPyramid camera(W, H, dvo::core::IntrinsicMatrix::create(FX, FY, OX, OY));
  KeyframeVector all;
  for (int k = 0; k < N; ++k) {
    KeyframePtr kf(new Keyframe());
    dvo::core::AffineTransformd pose;
    pose.setIdentity();
    double *T = dvo::core::data(pose);  // column-major
    T[12] = place[k];
    if (k == TURNED) T[0] = T[10] = -1.0;  // a half turn about y
    kf->id(2 * k).pose(pose);
    if (with_overlap) {
      std::vector<float> grey, depth;
      wall(place[k], grey, depth);
      kf->image(camera.create(grey.data(), depth.data()));
    }
    all.push_back(kf);
  }

  NearestNeighborConstraintSearch *nearest = new NearestNeighborConstraintSearch(1.0f);
  KeyframeConstraintSearchInterfacePtr search(nearest);  // keyframe_graph.cpp:158
  KeyframeVector found;
  search->findPossibleConstraints(all, all[0], found);  // keyframe_graph.cpp:456
  print("within 1 m", found);
  nearest->maxDistance(0.05f);
  found.clear();
  search->findPossibleConstraints(all, all[2], found);
  std::printf("maxDistance %.2f, minOverlap %.2f\n", nearest->maxDistance(), nearest->minOverlap());
  print("within 0.05 m of keyframe 4", found);
  if (with_overlap) {
    nearest->maxDistance(1.0f);
    nearest->minOverlap(0.3);
    found.clear();
    search->findPossibleConstraints(all, all[0], found);
    print("within 1 m and overlapping", found);
    for (size_t i = 0; i < found.size(); ++i) std::printf("  %d: %.3f\n", found[i]->id(), nearest->overlaps()[i]);
  }
  return 0;
}
