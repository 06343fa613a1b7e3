// dvo::core::DepthRegistration (include/dvo_amd/depth_registration.hpp): raw depth of the depth camera and a raw colour image
// taken into RgbdImagePyramids of the colour camera, without and with a Rectification of the image.  The same synthetic frames
// and cameras as examples/registered_ingest_example.c, and the same lines.
//   g++ -std=c++11 -Iinclude/dvo_amd_compat -Iinclude examples/registered_ingest_adaptor_example.cpp -Ldvo_slam_amd -ldvo_amd
#include <dvo/core/rgbd_image.h>
#include <dvo_amd/depth_registration.hpp>

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

static void report(const char *what, dvo::core::RgbdImagePyramid &pyr, const dvo::core::DepthRegistration::Stats &st, int levels) {
  std::printf("%s: %lld measurements, %lld behind, %lld outside, %lld drawn, %lld covered\n", what, st.measurements, st.behind, st.outside,
              st.drawn, st.covered_pixels);
  for (int l = 0; l < levels; ++l) {
    dvo::core::RgbdImage &img = pyr.level((size_t)l);
    std::printf("level %d: %zu x %zu intensity %08x depth %08x\n", l, img.width, img.height, checksum(img.plane(0)), checksum(img.plane(1)));
  }
}

int main() try {
  using namespace dvo::core;
  const int SW = 80, SH = 60, W = 72, H = 50, DW = 40, DH = 30, LEVELS = 2;
  std::vector<unsigned char> bgr((size_t)SW * SH * 3);
  std::vector<unsigned short> depth((size_t)DW * DH);
  for (int v = 0; v < SH; ++v)
    for (int u = 0; u < SW; ++u) {
      unsigned char *px = &bgr[((size_t)v * SW + u) * 3];
      px[0] = (unsigned char)((3 * u + 5 * v) % 256), px[1] = (unsigned char)((7 * u + v) % 256), px[2] = (unsigned char)((u + 11 * v) % 256);
    }
  for (int v = 0; v < DH; ++v)
    for (int u = 0; u < DW; ++u)
      depth[(size_t)v * DW + u] = (unsigned short)((u + 2 * v) % 9 == 0 ? 0 : (u + v) % 17 == 0 ? 1000 : 5000 + 130 * u + 70 * v);
  const IntrinsicMatrix colour = IntrinsicMatrix::create(60.0f, 60.0f, 35.5f, 24.5f), ir = IntrinsicMatrix::create(26.0f, 26.0f, 19.5f, 14.5f);
  AffineTransformd T;
  T.setIdentity();  // (Eigen's default constructor leaves the matrix unset)
  double *t = data(T);  // column-major: a small rotation about y and the baseline
  t[0] = 0.9998, t[2] = -0.02, t[8] = 0.02, t[10] = 0.9998, t[12] = 0.025, t[13] = 0.001, t[14] = -0.004;
  DepthRegistration reg(DW, DH, ir, T, 0.3f, true);

  DepthRegistration::Stats st;
  RgbdImagePyramidPtr pyr = reg.create(W, H, colour, bgr.data(), 3, 3 * SW, depth.data(), 0, 1.0f / 5000.0f, LEVELS, 0.0, &st);
  report("registered", *pyr, st, LEVELS);

  const IntrinsicMatrix source = IntrinsicMatrix::create(64.0f, 64.0f, 39.5f, 29.5f);
  const float dist[5] = {0.1f, -0.05f, 0.002f, -0.001f, 0.01f};
  Rectification rect = Rectification::undistort(W, H, colour, SW, SH, source, dist);
  DepthRegistration single = reg;  // a value: the copy is changed, `reg` is not
  single.setFill(false);
  RgbdImagePyramidPtr pyr2 = single.create(rect, bgr.data(), 3, 0, depth.data(), DW, 1.0f / 5000.0f, LEVELS, 1.5, &st);
  rect = Rectification();  // the pyramid holds planes: it needs neither the table nor the registration any more
  report("registered and rectified", *pyr2, st, LEVELS);
  return reg.fill() && !single.fill() && pyr2->timestamp() == 1.5 ? 0 : 1;
} catch (const std::exception &e) {
  std::fprintf(stderr, "%s\n", e.what());
  return 1;
}
