// dvo::core::Rectification (include/dvo_amd/rectification.hpp): the lens undistortion as a device table made once per camera,
// and raw frames of the real camera taken through it into RgbdImagePyramids of the rectified camera.  The same synthetic frame
// and camera as examples/rectified_ingest_example.c, and the same lines; then the table once more through fromMaps, which
// must give the same pyramid.
//   g++ -std=c++11 -Iinclude/dvo_amd_compat -Iinclude examples/rectified_ingest_adaptor_example.cpp -Ldvo_slam_amd -ldvo_amd
#include <dvo/core/rgbd_image.h>
#include <dvo_amd/rectification.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned checksum(const std::vector<float> &plane) {
  unsigned h = 0u;
  for (size_t i = 0; i < plane.size(); ++i) {
    unsigned word;
    std::memcpy(&word, &plane[i], 4);
    if (plane[i] != plane[i]) word = 0x7fc00000u;
    h = h * 31u + word;
  }
  return h;
}

int main() try {
  using namespace dvo::core;
  const int SW = 80, SH = 60, W = 72, H = 50, LEVELS = 2;
  std::vector<unsigned char> bgr((size_t)SW * SH * 3);
  std::vector<unsigned short> depth((size_t)SW * SH);
  for (int v = 0; v < SH; ++v)
    for (int u = 0; u < SW; ++u) {
      unsigned char *px = &bgr[((size_t)v * SW + u) * 3];
      px[0] = (unsigned char)((3 * u + 5 * v) % 256), px[1] = (unsigned char)((7 * u + v) % 256), px[2] = (unsigned char)((u + 11 * v) % 256);
      depth[(size_t)v * SW + u] = (unsigned short)((u + 2 * v) % 9 == 0 ? 0 : 5000 + 13 * u + 7 * v);
    }
  const IntrinsicMatrix camera = IntrinsicMatrix::create(60.0f, 60.0f, 35.5f, 24.5f), source = IntrinsicMatrix::create(64.0f, 64.0f, 39.5f, 29.5f);
  const float dist[5] = {0.1f, -0.05f, 0.002f, -0.001f, 0.01f};
  Rectification rect = Rectification::undistort(W, H, camera, SW, SH, source, dist);
  const Rectification::Info info = rect.info();
  std::printf("remap: %d x %d from %d x %d, %d inside\n", info.width, info.height, info.src_width, info.src_height, info.n_inside);

  RgbdImagePyramidPtr pyr = rect.create(bgr.data(), 3, 0, depth.data(), 0, 1.0f / 5000.0f, LEVELS);
  std::vector<unsigned> sums;
  for (int l = 0; l < LEVELS; ++l) {
    RgbdImage &img = pyr->level((size_t)l);
    sums.push_back(checksum(img.plane(0))), sums.push_back(checksum(img.plane(1)));
    std::printf("level %d: %zu x %zu intensity %08x depth %08x\n", l, img.width, img.height, sums[2 * l], sums[2 * l + 1]);
  }

  // a copy shares the table; the table again from its own download, as any map would come in
  std::vector<float> map_x, map_y;
  Rectification shared = rect;
  rect = Rectification();
  shared.download(map_x, map_y);
  Rectification again = Rectification::fromMaps(W, H, camera, map_x.data(), map_y.data(), 0, SW, SH);
  shared = Rectification();  // the last owner of the first table lets go; `pyr` lives on
  RgbdImagePyramidPtr pyr2 = again.create(bgr.data(), 3, 3 * SW, depth.data(), SW, 1.0f / 5000.0f, LEVELS, 1.5);
  bool same = again.info().n_inside == info.n_inside && pyr2->timestamp() == 1.5 && !rect.valid() && again.valid();
  for (int l = 0; l < LEVELS; ++l)
    same = same && checksum(pyr2->level((size_t)l).plane(0)) == sums[2 * l] && checksum(pyr2->level((size_t)l).plane(1)) == sums[2 * l + 1] &&
           checksum(pyr->level((size_t)l).plane(1)) == sums[2 * l + 1];
  std::printf("fromMaps gives the same pyramid: %d\n", same ? 1 : 0);
  return same ? 0 : 1;
} catch (const std::exception &e) {
  std::fprintf(stderr, "%s\n", e.what());
  return 1;
}
