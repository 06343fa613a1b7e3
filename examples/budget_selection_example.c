/* Point-budget selection masks through the C ABI, from C99: track a pair with the k0 strongest points of level 0 (a quarter of the
 * budget on every coarser level), and with one point per cell x cell cell, spread over the image.  Both masks are ranked on the
 * device from the resident reference pyramid (dvo_amd_mask_create_budget).  Prints the kept pixels per level of both masks and a
 * checksum of the pose of the plain match and of the two budgeted ones.  Input files: float32 planes without a header, as
 * tests/test_budget_selection_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/budget_selection_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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

static void report(const char *tag, const dvo_amd_result *res) {
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res->transformation[k];
  printf("%s checksum %.17g isnan %d\n", tag, sum, res->is_nan);
}

int main(int argc, char **argv) {
  if (argc < 13) {
    fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z k0 cell\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const long long k0 = atoll(argv[11]);
  const int cell = atoi(argv[12]);
  const size_t n = (size_t)w * (size_t)h;
  float *ri = read_file(argv[7], 4 * n), *rz = read_file(argv[8], 4 * n), *ci = read_file(argv[9], 4 * n), *cz = read_file(argv[10], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  cfg.last_level = 0;
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *ref = NULL, *cur = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_pyramid_create(0, ri, rz, w, h, w, fx, fy, ox, oy, levels, 0.0, &ref));
  CHECK(dvo_amd_pyramid_create(0, ci, cz, w, h, w, fx, fy, ox, oy, levels, 0.0, &cur));

  /* the candidates are what the tracker's own thresholds select; the budget thins them */
  dvo_amd_budget_options opt;
  dvo_amd_mask *topk = NULL, *grid = NULL;
  dvo_amd_default_budget_options(&opt);
  opt.intensity_threshold = cfg.intensity_derivative_threshold, opt.depth_threshold = cfg.depth_derivative_threshold;
  opt.rule = DVO_AMD_BUDGET_TOPK;
  for (int l = 0; l < levels; ++l) opt.budget[l] = k0 >> (2 * l);
  CHECK(dvo_amd_mask_create_budget(ref, &opt, &topk));
  opt.rule = DVO_AMD_BUDGET_GRID;
  for (int l = 0; l < levels; ++l) opt.cell[l] = cell;
  CHECK(dvo_amd_mask_create_budget(ref, &opt, &grid));

  long long kept[DVO_AMD_MAX_LEVELS];
  CHECK(dvo_amd_mask_info(topk, NULL, NULL, NULL, kept));
  for (int l = 0; l < levels; ++l) printf("topk kept %d %lld\n", l, kept[l]);
  CHECK(dvo_amd_mask_info(grid, NULL, NULL, NULL, kept));
  for (int l = 0; l < levels; ++l) printf("grid kept %d %lld\n", l, kept[l]);

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, ref, cur, NULL, &res));
  report("plain", &res);
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, ref, topk, opt.intensity_threshold, opt.depth_threshold, cur, NULL, &res));
  report("topk", &res);
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, ref, grid, opt.intensity_threshold, opt.depth_threshold, cur, NULL, &res));
  report("grid", &res);

  dvo_amd_mask_release(topk);
  dvo_amd_mask_release(grid);
  dvo_amd_pyramid_release(ref);
  dvo_amd_pyramid_release(cur);
  dvo_amd_context_destroy(ctx);
  free(ri), free(rz), free(ci), free(cz);
  return 0;
}
