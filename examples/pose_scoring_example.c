/* Pose scoring through the C ABI, from C99: a start for an alignment whose relative pose is not known.
 *   first     the current frame aligned against the reference from the identity, with per-iteration statistics: whatever pose it
 *             ends at, its coarsest level holds a precision of the residuals
 *   grid      15 hypotheses around the identity: five yaws in steps of 5 degrees, three shifts along x in steps of 10 cm
 *   scores    every hypothesis scored at the coarsest level in one call (two kernel launches)
 *   rank      the three of smallest total
 *   seeded    the alignment again, started from the best hypothesis
 * Prints the three ranked hypotheses with their sums and a checksum of the seeded pose.  Input files: float32 planes without a
 * header, as tests/test_pose_scoring_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/pose_scoring_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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

#define HYPOTHESES 15
#define KEEP 3

int main(int argc, char **argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: %s w h fx fy ox oy ref_i ref_z cur_i cur_z\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[4];
  for (int k = 0; k < 4; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  const int levels = cfg.first_level + 1, coarsest = cfg.first_level;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frame[2] = {NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < 2; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  /* from the identity: the pose may be wrong, the precision of the coarsest level is what is taken from it */
  const int capacity = levels * (cfg.max_iterations_per_level + 1);
  dvo_amd_iteration_stats *iterations = calloc((size_t)capacity, sizeof(*iterations));
  if (!iterations) return 2;
  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  res.iterations = iterations, res.iterations_capacity = capacity;
  CHECK(dvo_amd_match(ctx, frame[0], frame[1], NULL, &res));
  dvo_amd_pose_score_options sopt;
  dvo_amd_default_pose_score_options(&sopt);
  sopt.level = coarsest;
  int found = 0;
  for (int i = 0; i < res.n_levels; ++i)
    if (res.levels[i].id == coarsest && res.levels[i].n_iterations > 0) {
      const dvo_amd_iteration_stats *last = &res.iterations[res.levels[i].first_iteration + res.levels[i].n_iterations - 1];
      for (int k = 0; k < 4; ++k) sopt.precision[k] = (float)last->tdist_precision[k];
      found = 1;
    }
  if (!found) {
    fprintf(stderr, "the match recorded no iteration at level %d\n", coarsest);
    return 1;
  }

  dvo_amd_pose_grid_options grid;
  for (int a = 0; a < 6; ++a) grid.count[a] = 1, grid.step[a] = 0.0;
  grid.count[0] = 3, grid.step[0] = 0.1;                         /* vx */
  grid.count[4] = 5, grid.step[4] = 5.0 * 3.14159265358979323846 / 180.0; /* wy: yaw */
  double identity[16], T[16 * HYPOTHESES];
  memset(identity, 0, sizeof(identity));
  identity[0] = identity[5] = identity[10] = identity[15] = 1.0;
  int n_hypotheses = 0;
  CHECK(dvo_amd_pose_grid(&grid, identity, T, HYPOTHESES, &n_hypotheses));

  dvo_amd_pose_score scores[HYPOTHESES];
  CHECK(dvo_amd_score_poses(ctx, frame[0], frame[1], n_hypotheses, T, &sopt, scores));
  int order[KEEP], kept = 0;
  CHECK(dvo_amd_rank_poses(scores, n_hypotheses, KEEP, order, &kept));
  for (int r = 0; r < kept; ++r) {
    const dvo_amd_pose_score *s = &scores[order[r]];
    printf("rank %d hypothesis %d evaluated %lld invalid %lld inlier %lld outlier %lld cost %llu total %llu\n", r, order[r], s->evaluated,
           s->invalid, s->inlier, s->outlier, s->cost, s->total);
  }

  /* the alignment again, from the best hypothesis (reference -> current: what T_init takes) */
  cfg.use_initial_estimate = 1;
  CHECK(dvo_amd_configure(ctx, &cfg));
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frame[0], frame[1], T + 16 * order[0], &res));
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("seeded checksum %.17g isnan %d\n", sum, res.is_nan);

  for (int k = 0; k < 2; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  free(iterations);
  return 0;
}
