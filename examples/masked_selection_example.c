/* A masked point selection through the C ABI, from C99: the reference pixels inside a rectangle of level 0 (a moving object, the
 * robot's own arm, a timestamp overlay) take no part in the alignment.  Level 0 of the mask is given, the coarser levels are
 * derived on the device by the conservative rule (DVO_AMD_MASK_ALL).  Prints the selected pixels per level and a checksum of
 * the pose.  Input files: float32 planes without a header, as tests/test_selection_mask_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/masked_selection_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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

int main(int argc, char **argv) {
  if (argc < 15) {
    fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z x0 y0 x1 y1\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const int x0 = atoi(argv[11]), y0 = atoi(argv[12]), x1 = atoi(argv[13]), y1 = atoi(argv[14]);
  const size_t n = (size_t)w * (size_t)h;
  float *ri = read_file(argv[7], 4 * n), *rz = read_file(argv[8], 4 * n), *ci = read_file(argv[9], 4 * n), *cz = read_file(argv[10], 4 * n);

  /* 1 = keep, 0 = drop: everything but the rectangle [x0, x1) x [y0, y1) of level 0 */
  unsigned char *keep = malloc(n);
  if (!keep) return 2;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) keep[(size_t)y * (size_t)w + (size_t)x] = (unsigned char)!(x >= x0 && x < x1 && y >= y0 && y < y1);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  cfg.last_level = 0;
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *ref = NULL, *cur = NULL;
  dvo_amd_mask *mask = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_pyramid_create(0, ri, rz, w, h, w, fx, fy, ox, oy, levels, 0.0, &ref));
  CHECK(dvo_amd_pyramid_create(0, ci, cz, w, h, w, fx, fy, ox, oy, levels, 0.0, &cur));
  CHECK(dvo_amd_mask_create(0, w, h, levels, keep, w, 0, DVO_AMD_MASK_ALL, &mask));

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, ref, mask, cfg.intensity_derivative_threshold, cfg.depth_derivative_threshold, cur, NULL, &res));
  /* the selections are the pyramid's now: the mask may go, the counts below come from the cache */
  for (int l = 0; l < levels; ++l) {
    int count = 0;
    CHECK(dvo_amd_pyramid_select_masked(ref, l, cfg.intensity_derivative_threshold, cfg.depth_derivative_threshold, mask, &count, NULL));
    printf("count %d %d\n", l, count);
  }
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_mask_release(mask);
  dvo_amd_pyramid_release(ref);
  dvo_amd_pyramid_release(cur);
  dvo_amd_context_destroy(ctx);
  free(ri), free(rz), free(ci), free(cz), free(keep);
  return 0;
}
