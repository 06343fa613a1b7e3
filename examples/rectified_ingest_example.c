/* Rectification at ingest through the C ABI (C99): a remap table from the five lens coefficients, made once on the device, and
 * raw frames of the real camera taken through it into pyramids of the rectified camera -- what image_proc's
 * initUndistortRectifyMap + remap do on the CPU in front of the reference.  Synthetic frame, no input files.  Prints the
 * remap's sizes and n_inside and a checksum of the two base planes of every level (tests/test_rectify_adaptor.py compares them
 * with the Python binding's).
 *   cc -std=c99 -Iinclude examples/rectified_ingest_example.c -Ldvo_slam_amd -ldvo_amd */
#include <dvo_amd.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    int rc_ = (call);                                                                                 \
    if (rc_ != DVO_AMD_OK) {                                                                          \
      fprintf(stderr, "%s: %s [%s]\n", #call, dvo_amd_status_string(rc_), dvo_amd_last_error());      \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

enum { SW = 80, SH = 60, W = 72, H = 50, LEVELS = 2 };

/* h <- 31 h + word over the plane in scan order; every NaN counts as the word 0x7fc00000 */
static unsigned checksum(const float *plane, int n) {
  unsigned h = 0u;
  for (int i = 0; i < n; ++i) {
    unsigned word;
    memcpy(&word, &plane[i], 4);
    if (plane[i] != plane[i]) word = 0x7fc00000u;
    h = h * 31u + word;
  }
  return h;
}

int main(void) {
  static unsigned char bgr[SH][SW][3];
  static unsigned short depth[SH][SW];
  static float plane[W * H];
  for (int v = 0; v < SH; ++v)
    for (int u = 0; u < SW; ++u) {
      bgr[v][u][0] = (unsigned char)((3 * u + 5 * v) % 256), bgr[v][u][1] = (unsigned char)((7 * u + v) % 256);
      bgr[v][u][2] = (unsigned char)((u + 11 * v) % 256);
      depth[v][u] = (unsigned short)((u + 2 * v) % 9 == 0 ? 0 : 5000 + 13 * u + 7 * v);
    }
  const float k_out[4] = {60.0f, 60.0f, 35.5f, 24.5f}, k_src[4] = {64.0f, 64.0f, 39.5f, 29.5f};
  const float dist[5] = {0.1f, -0.05f, 0.002f, -0.001f, 0.01f};
  dvo_amd_remap *remap = NULL;
  CHECK(dvo_amd_remap_create_undistort(0, W, H, k_out, SW, SH, k_src, dist, &remap));
  int w, h, sw, sh, n_inside;
  CHECK(dvo_amd_remap_info(remap, &w, &h, &sw, &sh, &n_inside));
  printf("remap: %d x %d from %d x %d, %d inside\n", w, h, sw, sh, n_inside);

  dvo_amd_pyramid *pyr = NULL;
  CHECK(dvo_amd_pyramid_create_raw_remapped(0, &bgr[0][0][0], 3, 3 * SW, &depth[0][0], SW, 1.0f / 5000.0f, 0, remap, k_out[0], k_out[1],
                                            k_out[2], k_out[3], LEVELS, 0.0, &pyr));
  dvo_amd_remap_release(remap); /* the pyramid holds planes, not positions: it does not need the remap any more */
  for (int l = 0; l < LEVELS; ++l) {
    int lw, lh;
    unsigned sums[2];
    CHECK(dvo_amd_pyramid_level_info(pyr, l, &lw, &lh, NULL));
    for (int p = 0; p < 2; ++p) {
      CHECK(dvo_amd_pyramid_download_plane(pyr, l, p, plane));
      sums[p] = checksum(plane, lw * lh);
    }
    printf("level %d: %d x %d intensity %08x depth %08x\n", l, lw, lh, sums[0], sums[1]);
  }
  dvo_amd_pyramid_release(pyr);
  return 0;
}
