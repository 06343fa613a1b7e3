/* Mask components through the C ABI, from C99: the speckle of a residual mask removed without eroding its shape, and a frame's
 * depth despeckled.
 *   match          frame 1 aligned against the keyframe, with per-iteration statistics (they hold each level's precision)
 *   inliers        the keyframe's pixels whose residuals at the estimate are inliers of the t-distribution: isolated outliers are
 *                  scattered over good surfaces, isolated inliers over bad ones
 *   eroded         ... shrunk by one pixel: the speckle is gone, and so is a rim of every true region
 *   reconstructed  the components of `inliers` that `eroded` still touches: the speckle is gone, the regions keep their shape
 *   warped         ... carried onto frame 1, the next keyframe, with the pose the match returned
 *   track          frame 2 tracked against frame 1 behind the warped mask
 *   despeckled     frame 1's depth-connected surfaces of at least 10 pixels of level 0 (the mask-less form): floating blobs go
 * Nothing leaves the device between the steps.  Prints the kept pixels per level of the masks and a checksum of the pose.  Input
 * files: float32 planes without a header, as tests/test_mask_components_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/mask_components_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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

/* precision[l] = tdist_precision of the last iteration of level l; a level the match did not run (level 0 under the default
 * configuration) takes the nearest level that ran, ties to the finer one */
static int precisions_from_result(const dvo_amd_result *res, int levels, dvo_amd_residual_mask_options *opt) {
  for (int l = 0; l < levels; ++l) {
    int best = -1, best_distance = 0;
    for (int i = 0; i < res->n_levels; ++i) {
      const dvo_amd_level_stats *L = &res->levels[i];
      if (L->n_iterations < 1) continue;
      const int distance = L->id > l ? L->id - l : l - L->id;
      if (best < 0 || distance < best_distance || (distance == best_distance && L->id < res->levels[best].id))
        best = i, best_distance = distance;
    }
    if (best < 0) return 1;
    const dvo_amd_iteration_stats *last = &res->iterations[res->levels[best].first_iteration + res->levels[best].n_iterations - 1];
    for (int k = 0; k < 4; ++k) opt->precision[l][k] = (float)last->tdist_precision[k];
  }
  return 0;
}

/* (R^T, -R^T t) of a rigid transformation, column-major */
static void rigid_inverse(const double *t, double *o) {
  memset(o, 0, 16 * sizeof(double));
  o[15] = 1.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[j * 4 + i] = t[i * 4 + j];
    o[12 + i] = -((t[i * 4 + 0] * t[12] + t[i * 4 + 1] * t[13]) + t[i * 4 + 2] * t[14]);
  }
}

int main(int argc, char **argv) {
  if (argc < 13) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z f2_i f2_z\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[6];
  for (int k = 0; k < 6; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg); /* levels first_level .. last_level: level 0 is not run by default */
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frame[3] = {NULL, NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < 3; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  /* the alignment whose residuals are judged */
  const int capacity = levels * (cfg.max_iterations_per_level + 1);
  dvo_amd_iteration_stats *iterations = calloc((size_t)capacity, sizeof(*iterations));
  if (!iterations) return 2;
  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  res.iterations = iterations, res.iterations_capacity = capacity;
  CHECK(dvo_amd_match(ctx, frame[0], frame[1], NULL, &res));

  /* dvo_amd_match returns the inverse of its estimate; the residuals are taken at the estimate (keyframe -> frame 1) */
  dvo_amd_residual_mask_options ropt;
  dvo_amd_default_residual_mask_options(&ropt);
  if (precisions_from_result(&res, levels, &ropt)) {
    fprintf(stderr, "the match recorded no iteration\n");
    return 1;
  }
  double estimate[16];
  rigid_inverse(res.transformation, estimate);
  dvo_amd_mask *inliers = NULL, *eroded = NULL, *reconstructed = NULL, *warped = NULL, *despeckled = NULL;
  long long counts[DVO_AMD_MAX_LEVELS * DVO_AMD_RESIDUAL_MASK_COUNTS];
  CHECK(dvo_amd_mask_from_residuals(ctx, frame[0], frame[1], estimate, &ropt, &inliers, counts, NULL));
  for (int l = 0; l < levels; ++l) {
    const long long *c = counts + DVO_AMD_RESIDUAL_MASK_COUNTS * l;
    fprintf(stderr, "level %d: evaluated %lld invalid %lld inlier %lld outlier %lld kept %lld\n", l, c[0], c[1], c[2], c[3], c[4]);
  }

  int radius[DVO_AMD_MAX_LEVELS];
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) radius[l] = (1 + (1 << l) - 1) >> l; /* one pixel of level 0, rounded up */
  CHECK(dvo_amd_mask_morph(inliers, DVO_AMD_MASK_ERODE, radius, &eroded));

  /* reconstruction from seeds: the defaults (8-connected, no area band) and the eroded mask as seeds */
  dvo_amd_component_options copt;
  dvo_amd_default_component_options(&copt);
  long long ccounts[DVO_AMD_MAX_LEVELS * DVO_AMD_COMPONENTS_COUNTS];
  CHECK(dvo_amd_mask_filter_components(inliers, NULL, eroded, &copt, &reconstructed, ccounts));
  for (int l = 0; l < levels; ++l) {
    const long long *c = ccounts + DVO_AMD_COMPONENTS_COUNTS * l;
    fprintf(stderr, "level %d: foreground %lld components %lld kept %lld (%lld pixels) largest %lld\n", l, c[0], c[1], c[2], c[3], c[4]);
  }

  /* onto the next keyframe: source = keyframe, target = frame 1, and the transformation as the match returned it */
  dvo_amd_mask_warp_options wopt;
  dvo_amd_default_mask_warp_options(&wopt);
  CHECK(dvo_amd_mask_warp(reconstructed, frame[0], frame[1], res.transformation, &wopt, &warped, NULL));

  /* a depth despeckle: no mask, the pyramid's depth alone; an area of 10 pixels of level 0 is max(1, ceil(10 / 4^l)) on level l */
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) {
    const int q = 1 << (2 * l), a = (10 + q - 1) / q;
    copt.min_area[l] = a < 1 ? 1 : a;
  }
  CHECK(dvo_amd_mask_filter_components(NULL, frame[1], NULL, &copt, &despeckled, NULL));

  if (report_kept("inliers", inliers, levels) || report_kept("eroded", eroded, levels) ||
      report_kept("reconstructed", reconstructed, levels) || report_kept("warped", warped, levels) ||
      report_kept("despeckled", despeckled, levels))
    return 1;
  dvo_amd_mask_release(inliers);
  dvo_amd_mask_release(eroded);
  dvo_amd_mask_release(reconstructed);
  dvo_amd_mask_release(despeckled);

  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, frame[1], warped, cfg.intensity_derivative_threshold, cfg.depth_derivative_threshold, frame[2], NULL,
                             &res));
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_mask_release(warped);
  for (int k = 0; k < 3; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 6; ++k) free(planes[k]);
  free(iterations);
  return 0;
}
