/* Mask operations through the C ABI, from C99: a region of interest drawn on a keyframe follows the camera.
 *   rect      a rectangle mask on the keyframe (the middle of the image)
 *   warped    the rectangle carried onto the next frame with the pose a match of (keyframe, frame 1) returned
 *   eroded    ... shrunk by one pixel, because its border is only as exact as the depth
 *   combined  ... AND a GRID budget of frame 1: one point per cell x cell cell inside the region
 *   track     frame 2 tracked against frame 1 behind the combined mask
 * Every mask is made on the device; nothing but the rectangle is uploaded and nothing is downloaded.  Prints the kept pixels per
 * level of the four masks and a checksum of the pose.  Input files: float32 planes without a header, as
 * tests/test_mask_ops_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/mask_ops_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvo_amd.h"

static void *read_file(const char *path, size_t bytes) {
  void *p = malloc(bytes);
  FILE *f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return p;
}

#define CHECK(call)                                                                                         \
  do {                                                                                                      \
    int rc_ = (call);                                                                                       \
    if (rc_ != DVO_AMD_OK) {                                                                                \
      fprintf(stderr, "%s: %s [%s]\n", #call, dvo_amd_status_string(rc_), dvo_amd_last_error());             \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

static int report_kept(const char *tag, const dvo_amd_mask *mask, int levels) {
  long long kept[DVO_AMD_MAX_LEVELS];
  CHECK(dvo_amd_mask_info(mask, NULL, NULL, NULL, kept));
  for (int l = 0; l < levels; ++l) printf("%s kept %d %lld\n", tag, l, kept[l]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 14) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z f2_i f2_z cell\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const int cell = atoi(argv[13]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[6];
  for (int k = 0; k < 6; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  cfg.last_level = 0;
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frame[3] = {NULL, NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < 3; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  /* the region of interest, on the keyframe's pixels */
  unsigned char *roi = calloc(n, 1);
  if (!roi) return 2;
  for (int y = h / 4; y < (3 * h) / 4; ++y)
    for (int x = w / 4; x < (3 * w) / 4; ++x) roi[(size_t)y * (size_t)w + (size_t)x] = 1;
  dvo_amd_mask *rect = NULL, *warped = NULL, *eroded = NULL, *budget = NULL, *combined = NULL;
  CHECK(dvo_amd_mask_create(0, w, h, levels, roi, w, 0, DVO_AMD_MASK_ALL, &rect));

  /* match(reference = keyframe, current = frame 1) returns the transformation that takes points of frame 1 into the keyframe:
   * what dvo_amd_mask_warp asks for with source = keyframe and target = frame 1 */
  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frame[0], frame[1], NULL, &res));
  dvo_amd_mask_warp_options wopt;
  dvo_amd_default_mask_warp_options(&wopt);
  CHECK(dvo_amd_mask_warp(rect, frame[0], frame[1], res.transformation, &wopt, &warped, NULL));

  int radius[DVO_AMD_MAX_LEVELS];
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) radius[l] = (1 + (1 << l) - 1) >> l; /* one pixel of level 0, rounded up */
  CHECK(dvo_amd_mask_morph(warped, DVO_AMD_MASK_ERODE, radius, &eroded));

  dvo_amd_budget_options bopt;
  dvo_amd_default_budget_options(&bopt);
  bopt.rule = DVO_AMD_BUDGET_GRID;
  bopt.intensity_threshold = cfg.intensity_derivative_threshold, bopt.depth_threshold = cfg.depth_derivative_threshold;
  for (int l = 0; l < levels; ++l) bopt.cell[l] = cell;
  CHECK(dvo_amd_mask_create_budget(frame[1], &bopt, &budget));
  CHECK(dvo_amd_mask_combine(eroded, budget, DVO_AMD_MASK_AND, &combined));

  if (report_kept("rect", rect, levels) || report_kept("warped", warped, levels) || report_kept("eroded", eroded, levels) ||
      report_kept("combined", combined, levels))
    return 1;
  /* the operands may go: the result is a mask of its own */
  dvo_amd_mask_release(rect);
  dvo_amd_mask_release(warped);
  dvo_amd_mask_release(eroded);
  dvo_amd_mask_release(budget);

  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, frame[1], combined, bopt.intensity_threshold, bopt.depth_threshold, frame[2], NULL, &res));
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_mask_release(combined);
  for (int k = 0; k < 3; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 6; ++k) free(planes[k]);
  free(roi);
  return 0;
}
