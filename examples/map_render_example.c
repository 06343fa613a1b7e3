/* Frame-to-model tracking from C99: three keyframes go into the device map, the map is rendered into a camera view between
 * them, the view becomes a pyramid on the device, and a live frame is aligned to it with the ordinary dvo_amd_match.
 * The frames are synthetic (a tilted, textured wall seen from places along x); no input files.
 *   cc -std=c99 -Iinclude examples/map_render_example.c -Ldvo_slam_amd -ldvo_amd -lm -Wl,-rpath,$PWD/dvo_slam_amd */
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

enum { W = 160, H = 120, N = 3, LEVELS = 3 };
static const float LEAF = 0.02f;
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

static void translation(double *T, double x) {
  memset(T, 0, 16 * sizeof(double));
  T[0] = T[5] = T[10] = T[15] = 1.0;
  T[12] = x;
}

static void print_pose(const char *what, const double *T) {
  printf("%s: t = (%.4f %.4f %.4f), R diagonal = (%.4f %.4f %.4f)\n", what, T[12], T[13], T[14], T[0], T[5], T[10]);
}

int main(void) {
  static float grey[H * W], depth[H * W];
  dvo_amd_config cfg;
  dvo_amd_context *ctx = NULL;
  dvo_amd_map *map = NULL;
  dvo_amd_pyramid *kf = NULL, *model = NULL, *live = NULL;
  double pose[16];
  dvo_amd_default_config(&cfg);
  cfg.first_level = LEVELS - 1, cfg.last_level = 0;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_map_create(ctx, LEAF, &map));
  for (int k = 0; k < N; ++k) { /* keyframes at x = 0, 0.1, 0.2 */
    wall(0.1 * k, grey, depth);
    CHECK(dvo_amd_pyramid_create(0, grey, depth, W, H, W, FX, FY, OX, OY, 1, (double)k, &kf));
    translation(pose, 0.1 * k);
    CHECK(dvo_amd_map_insert(map, k, kf, pose, NULL, 0));
    dvo_amd_pyramid_release(kf); /* the map keeps it */
  }

  /* the model seen from x = 0.14, between the second and the third keyframe */
  const dvo_amd_view view = {W, H, FX, FY, OX, OY, 0.1f};
  dvo_amd_render_stats st;
  static float model_depth[H * W];
  static int model_index[H * W];
  translation(pose, 0.14);
  CHECK(dvo_amd_map_render(map, pose, &view, model_depth, NULL, NULL, model_index, &st));
  printf("render: %lld voxels, %lld behind near_z, %lld outside, %lld drawn, %lld of %d pixels covered\n", st.voxels, st.behind_near,
         st.outside, st.drawn, st.covered_pixels, W * H);
  CHECK(dvo_amd_map_render_pyramid(map, pose, &view, LEVELS, 0.0, &model, NULL));

  /* a live frame from x = 0.15: where is it relative to the model view? */
  wall(0.15, grey, depth);
  CHECK(dvo_amd_pyramid_create(0, grey, depth, W, H, W, FX, FY, OX, OY, LEVELS, 1.0, &live));
  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, model, live, NULL, &res));
  print_pose("model view (camera -> world)", pose);
  print_pose("live frame relative to the model view (estimated; 0.01 along x in truth)", res.transformation);

  dvo_amd_pyramid_release(live);
  dvo_amd_pyramid_release(model);
  dvo_amd_map_destroy(map);
  dvo_amd_context_destroy(ctx);
  return 0;
}
