/* The keyframe map kept on the device, from C99: insert three keyframes, move one, remove one, write the map as a PCD.
 * After every event the map is compared with one dvo_amd_map_cloud over the keyframes it holds: the two are the same bytes.
 * The frames are synthetic (a tilted wall seen from three places); no input files.
 *   cc -std=c99 -Iinclude examples/keyframe_map_example.c -Ldvo_slam_amd -ldvo_amd -lm -Wl,-rpath,$PWD/dvo_slam_amd
 *   ./a.out map.pcd */
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

enum { W = 160, H = 120, N = 3 };
static const float LEAF = 0.02f;

/* column-major 4x4: a translation */
static void translation(double *T, double x, double y, double z) {
  memset(T, 0, 16 * sizeof(double));
  T[0] = T[5] = T[10] = T[15] = 1.0;
  T[12] = x, T[13] = y, T[14] = z;
}

/* the map against the rebuild over the same keyframes: 1 when every byte agrees */
static int same_as_rebuild(dvo_amd_context *ctx, dvo_amd_map *map, int n, dvo_amd_pyramid *const *pyr, const double *poses,
                           const unsigned char *const *bgr, dvo_amd_point *a, dvo_amd_point *b, long long cap, long long *n_out) {
  dvo_amd_cloud_stats st, ms;
  long long got = 0;
  if (dvo_amd_map_cloud(ctx, n, pyr, poses, bgr, NULL, LEAF, a, cap, &st) != DVO_AMD_OK) return 0;
  if (dvo_amd_map_extract(map, NULL, b, cap, &got) != DVO_AMD_OK) return 0;
  if (dvo_amd_map_stats(map, &ms, NULL) != DVO_AMD_OK) return 0;
  *n_out = got;
  return got == st.voxels && memcmp(&st, &ms, sizeof(st)) == 0 && memcmp(a, b, (size_t)got * sizeof(*a)) == 0;
}

int main(int argc, char **argv) {
  const char *path = argc > 1 ? argv[1] : "keyframe_map.pcd";
  const float fx = 131.25f, fy = 131.25f, ox = 79.5f, oy = 59.5f;
  static unsigned char bgr[N][H * W * 3];
  static unsigned short depth[H * W];
  dvo_amd_context *ctx = NULL;
  dvo_amd_map *map = NULL;
  dvo_amd_pyramid *pyr[N] = {NULL, NULL, NULL};
  double poses[N * 16];
  CHECK(dvo_amd_context_create(0, NULL, &ctx));
  CHECK(dvo_amd_map_create(ctx, LEAF, &map));
  for (int k = 0; k < N; ++k) {
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        /* a wall at 1.5 m, tilted, with a hole of missing depth; 1/5000 m units */
        const int hole = (u - 40 - 20 * k) * (u - 40 - 20 * k) + (v - 60) * (v - 60) < 100;
        depth[v * W + u] = hole ? 0 : (unsigned short)(7500 + 10 * u + 5 * v + 100 * k);
        bgr[k][(v * W + u) * 3 + 0] = (unsigned char)(u + 30 * k);
        bgr[k][(v * W + u) * 3 + 1] = (unsigned char)(v * 2);
        bgr[k][(v * W + u) * 3 + 2] = (unsigned char)(((u / 8 + v / 8) & 1) * 200);
      }
    CHECK(dvo_amd_pyramid_create_raw(0, bgr[k], 3, 3 * W, depth, W, 1.0f / 5000.0f, 0, W, H, fx, fy, ox, oy, 1, (double)k, &pyr[k]));
    translation(poses + 16 * k, 0.05 * k, -0.02 * k, 0.01 * k);
  }
  const long long cap = (long long)N * W * H;
  dvo_amd_point *a = malloc((size_t)cap * sizeof(*a)), *b = malloc((size_t)cap * sizeof(*b));
  const unsigned char *colour[N] = {bgr[0], NULL, bgr[2]}; /* the second keyframe is grey */
  if (!a || !b) return 2;
  long long n = 0;
  int ok = 1;

  for (int k = 0; k < N; ++k) {
    CHECK(dvo_amd_map_insert(map, 100 + k, pyr[k], poses + 16 * k, colour[k], 3 * W));
    ok &= same_as_rebuild(ctx, map, k + 1, pyr, poses, colour, a, b, cap, &n);
    printf("insert %d: %lld voxels\n", 100 + k, n);
  }
  /* the map holds the pyramids and copies of the images: the caller's handles can go (kept here for the rebuilds) */

  /* a loop closure moves the second keyframe */
  const int moved = 101;
  translation(poses + 16, 0.08, -0.01, 0.03);
  CHECK(dvo_amd_map_set_poses(map, 1, &moved, poses + 16));
  ok &= same_as_rebuild(ctx, map, N, pyr, poses, colour, a, b, cap, &n);
  printf("move %d: %lld voxels\n", moved, n);

  /* the first keyframe is dropped */
  const int dropped = 100;
  CHECK(dvo_amd_map_remove(map, 1, &dropped));
  ok &= same_as_rebuild(ctx, map, N - 1, pyr + 1, poses + 16, colour + 1, a, b, cap, &n);
  printf("remove %d: %lld voxels\n", dropped, n);

  /* the part of the map in a box */
  const float box[6] = {-0.2f, -0.2f, 0.0f, 0.2f, 0.2f, 3.0f};
  long long in_box = 0;
  CHECK(dvo_amd_map_extract(map, box, a, cap, &in_box));
  printf("box: %lld voxels\n", in_box);

  CHECK(dvo_amd_map_extract(map, NULL, b, cap, &n));
  CHECK(dvo_amd_write_pcd(path, b, n, (int)n, 1));
  printf("wrote %lld points to %s; equal to the rebuild after every event: %d\n", n, path, ok);

  dvo_amd_map_destroy(map);
  for (int k = 0; k < N; ++k) dvo_amd_pyramid_release(pyr[k]);
  dvo_amd_context_destroy(ctx);
  free(a), free(b);
  return ok ? 0 : 1;
}
