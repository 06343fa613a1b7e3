/* The loop-closure back end from C99, from the search to the constraints: dvo_amd_find_constraint_candidates picks the
 * keyframes near a query keyframe (the reference's radius search, pruned by view overlap on the device),
 * dvo_amd_proposals_for_candidates turns them into proposals and dvo_amd_validate_proposals aligns and votes on them.
 * The frames are synthetic (a tilted, textured wall seen from places along x); no input files.  Keyframe 8 stands next to the
 * others but looks the other way: the radius search proposes it, the overlap stage drops it before any alignment runs.
 *   cc -std=c99 -Iinclude examples/constraint_search_example.c -Ldvo_slam_amd -ldvo_amd -lm -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvo_amd.h"

#define CHECK(call)                                                                                         \
  do {                                                                                                      \
    int rc_ = (call);                                                                                       \
    if (rc_ != DVO_AMD_OK) {                                                                                \
      fprintf(stderr, "%s: %s [%s]\n", #call, dvo_amd_status_string(rc_), dvo_amd_last_error());             \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

enum { W = 160, H = 120, N = 6, LEVELS = 4, TURNED = 4, FAR_AWAY = 5 };
static const float FX = 131.25f, FY = 131.25f, OX = 79.5f, OY = 59.5f;

/* the wall z = 2 + 0.2 x (world) seen from (cx, 0, 0) looking along z: intensity and depth of every pixel */
static void wall(double cx, float *grey, float *depth) {
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      const double rx = (u - OX) / FX, ry = (v - OY) / FY;
      const double z = (2.0 + 0.2 * cx) / (1.0 - 0.2 * rx); /* z = 2 + 0.2 (cx + rx z) */
      const double x = cx + rx * z, y = ry * z;
      const int cell = ((int)(x * 8.0 + 64.0) + (int)(y * 8.0 + 64.0)) & 1;
      grey[v * W + u] = (float)(60 + 120 * cell + (int)(40.0 * (x - (int)x)));
      depth[v * W + u] = (float)z;
    }
}

/* camera -> world, column-major: at (x, 0, 0), looking along +z, or along -z when turned (a half turn about y) */
static void pose_at(double *T, double x, int turned) {
  memset(T, 0, 16 * sizeof(double));
  T[0] = T[10] = turned ? -1.0 : 1.0;
  T[5] = T[15] = 1.0;
  T[12] = x;
}

int main(void) {
  static float grey[H * W], depth[H * W];
  static const double place[N] = {0.0, 0.04, 0.08, 0.12, 0.06, 3.0};
  dvo_amd_config cfg;
  dvo_amd_context *ctx = NULL;
  dvo_amd_keyframe keyframes[N];
  dvo_amd_default_config(&cfg);
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  memset(keyframes, 0, sizeof(keyframes));
  for (int k = 0; k < N; ++k) {
    dvo_amd_result first;
    wall(place[k], grey, depth); /* (the turned keyframe sees a wall of its own on the other side) */
    CHECK(dvo_amd_pyramid_create(0, grey, depth, W, H, W, FX, FY, OX, OY, LEVELS, (double)k, &keyframes[k].image));
    keyframes[k].id = 2 * k; /* not neighbours in id: the odometry voter rejects |id - id| <= 1 */
    pose_at(keyframes[k].pose, place[k], k == TURNED);
    /* the evaluation every keyframe carries (keyframe_tracker.cpp:88-96 seeds it from its first odometry result; here: the
     * keyframe against itself) */
    memset(&first, 0, sizeof(first));
    CHECK(dvo_amd_match(ctx, keyframes[k].image, keyframes[k].image, NULL, &first));
    keyframes[k].evaluation_kind = DVO_AMD_EVAL_LOGLIKELIHOOD;
    keyframes[k].evaluation_average = -first.loglik, keyframes[k].evaluation_n = 1.0;
  }

  /* 1. the search, for keyframe 0: the reference's radius search first, then the same with the overlap stage */
  const int query = 0;
  int radius[N], candidates[N], n_radius = 0, n = 0;
  double overlap[N];
  dvo_amd_covisibility_options opt;
  dvo_amd_default_covisibility_options(&opt);
  CHECK(dvo_amd_find_constraint_candidates(NULL, N, keyframes, query, 1.0f, 0.0, NULL, radius, NULL, N, &n_radius));
  printf("within 1 m of keyframe %d:", keyframes[query].id);
  for (int i = 0; i < n_radius; ++i) printf(" %d", keyframes[radius[i]].id);
  printf("\n");
  CHECK(dvo_amd_find_constraint_candidates(ctx, N, keyframes, query, 1.0f, 0.3, &opt, candidates, overlap, N, &n));
  printf("... of which overlap its view by 0.3 or more:");
  for (int i = 0; i < n; ++i) printf(" %d (%.3f)", keyframes[candidates[i]].id, overlap[i]);
  printf("\n");

  /* 2. two proposals per candidate, 3. the two-stage validation (thresholds that let every sound alignment through) */
  dvo_amd_constraint_proposal *proposals = (dvo_amd_constraint_proposal *)calloc((size_t)(2 * N), sizeof(*proposals));
  dvo_amd_validator_stage stages[2];
  int n_valid = 0;
  if (!proposals) return 1;
  CHECK(dvo_amd_proposals_for_candidates(keyframes, query, n, candidates, proposals));
  dvo_amd_default_validator_stages(&cfg, 0.0, -1e300, -1e300, stages);
  CHECK(dvo_amd_validate_proposals(ctx, N, keyframes, 2, stages, 2 * n, proposals, &n_valid, 0));
  printf("validated: %d constraints from %d proposals\n", n_valid, 2 * n);
  for (int i = 0; i < n_valid; ++i) {
    const double *T = proposals[i].tracking_result.transformation;
    printf("  %d -> %d: t = (%.4f %.4f %.4f)\n", keyframes[proposals[i].reference].id, keyframes[proposals[i].current].id, T[12], T[13],
           T[14]);
  }

  free(proposals);
  for (int k = 0; k < N; ++k) dvo_amd_pyramid_release(keyframes[k].image);
  dvo_amd_context_destroy(ctx);
  return 0;
}
