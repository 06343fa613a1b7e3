// The frustum box of the signed-distance volume (dvo_slam_amd/csrc/dvo_volume_box.h) as a stand-alone program: host code only,
// built by tests/test_volume.py with -fsanitize=undefined -fno-sanitize-recover=all.  Every line of standard input holds
//   M[0..11] fx fy ox oy w h near_z z_max origin[0..2] voxel nx ny nz
// (doubles as strtod reads them: hex floats, "nan", "inf"; w, h and the dimensions as integers); the answer is one line
//   lo0 lo1 lo2 hi0 hi1 hi2
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dvo_volume_box.h"

int main() {
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    double v[27];
    char *at = line;
    int got = 0;
    for (; got < 27; ++got) {
      char *end = nullptr;
      v[got] = std::strtod(at, &end);
      if (end == at) break;
      at = end;
    }
    if (got == 0) continue;
    if (got != 27) {
      std::fprintf(stderr, "a line with %d of 27 values\n", got);
      return 2;
    }
    const double origin[3] = {v[20], v[21], v[22]};
    const int n[3] = {(int)v[24], (int)v[25], (int)v[26]};
    const dvo_amd::volume_box::Box b =
        dvo_amd::volume_box::frustum_box(v, v[12], v[13], v[14], v[15], (int)v[16], (int)v[17], v[18], v[19], origin, v[23], n);
    std::printf("%d %d %d %d %d %d\n", b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
  }
  return 0;
}
