/* Depth-to-colour registration at ingest through the C ABI (C99): a raw depth frame of the depth camera -- beside the colour
 * camera, with other intrinsics and half its resolution -- and a raw colour image taken straight into a pyramid of the colour
 * camera, what depth_image_proc/register does on the CPU in front of the reference.  Once with the image as it is, once with
 * the image of a real lens through a remap.  Synthetic frames, no input files.  Prints the five counters and a checksum of the
 * two base planes of every level (tests/test_register_adaptor.py compares them with the Python binding's).
 *   cc -std=c99 -Iinclude examples/registered_ingest_example.c -Ldvo_slam_amd -ldvo_amd */
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

enum { SW = 80, SH = 60, W = 72, H = 50, DW = 40, DH = 30, LEVELS = 2 };

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

static int report(const char *what, dvo_amd_pyramid *pyr, const dvo_amd_registration_stats *st) {
  static float plane[W * H];
  printf("%s: %lld measurements, %lld behind, %lld outside, %lld drawn, %lld covered\n", what, st->measurements, st->behind,
         st->outside, st->drawn, st->covered_pixels);
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
  return 0;
}

int main(void) {
  static unsigned char bgr[SH][SW][3];
  static unsigned short depth[DH][DW];
  for (int v = 0; v < SH; ++v)
    for (int u = 0; u < SW; ++u) {
      bgr[v][u][0] = (unsigned char)((3 * u + 5 * v) % 256), bgr[v][u][1] = (unsigned char)((7 * u + v) % 256);
      bgr[v][u][2] = (unsigned char)((u + 11 * v) % 256);
    }
  for (int v = 0; v < DH; ++v)
    for (int u = 0; u < DW; ++u) /* holes, a few measurements nearer than min_z, a slanted surface */
      depth[v][u] = (unsigned short)((u + 2 * v) % 9 == 0 ? 0 : (u + v) % 17 == 0 ? 1000 : 5000 + 130 * u + 70 * v);
  const float k_colour[4] = {60.0f, 60.0f, 35.5f, 24.5f};
  dvo_amd_registration reg;
  dvo_amd_default_registration(&reg);
  reg.depth_width = DW, reg.depth_height = DH;
  reg.k_depth[0] = 26.0f, reg.k_depth[1] = 26.0f, reg.k_depth[2] = 19.5f, reg.k_depth[3] = 14.5f;
  /* column-major: a small rotation about y and the baseline between the two cameras */
  reg.T[0] = 0.9998, reg.T[2] = -0.02, reg.T[8] = 0.02, reg.T[10] = 0.9998;
  reg.T[12] = 0.025, reg.T[13] = 0.001, reg.T[14] = -0.004;
  reg.min_z = 0.3f, reg.fill = 1;

  /* the image as it is: the top left W x H pixels of the frame, rows SW pixels apart */
  dvo_amd_pyramid *pyr = NULL;
  dvo_amd_registration_stats st;
  CHECK(dvo_amd_pyramid_create_raw_registered(0, &bgr[0][0][0], 3, 3 * SW, &depth[0][0], DW, 1.0f / 5000.0f, 0, &reg, NULL, W, H,
                                              k_colour[0], k_colour[1], k_colour[2], k_colour[3], LEVELS, 0.0, &pyr, &st));
  if (report("registered", pyr, &st)) return 1;
  dvo_amd_pyramid_release(pyr);

  /* the image of a real lens: the whole SW x SH frame through a remap; the depth does not go through it */
  const float k_src[4] = {64.0f, 64.0f, 39.5f, 29.5f}, dist[5] = {0.1f, -0.05f, 0.002f, -0.001f, 0.01f};
  dvo_amd_remap *remap = NULL;
  CHECK(dvo_amd_remap_create_undistort(0, W, H, k_colour, SW, SH, k_src, dist, &remap));
  reg.fill = 0;
  CHECK(dvo_amd_pyramid_create_raw_registered(0, &bgr[0][0][0], 3, 3 * SW, &depth[0][0], DW, 1.0f / 5000.0f, 0, &reg, remap, W, H,
                                              k_colour[0], k_colour[1], k_colour[2], k_colour[3], LEVELS, 0.0, &pyr, &st));
  dvo_amd_remap_release(remap);
  if (report("registered and rectified", pyr, &st)) return 1;
  dvo_amd_pyramid_release(pyr);
  return 0;
}
