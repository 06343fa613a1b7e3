/* The signed-distance volume through the C ABI, from C99: two frames fused into a volume, the volume raycast and its surface pulled.
 *   match     the second frame aligned against the first: the transformation, as returned, is the second frame's pose in the
 *             first frame's world
 *   insert    both frames as keyframes 0 and 1 in one call (dvo_amd_volume_insert): the counts of each
 *   raycast   the volume seen from the first frame's camera (dvo_amd_volume_raycast): stats and a checksum of the depth plane
 *   extract   the surface crossings (dvo_amd_volume_extract), written as a PCD file when a path is given
 *   track     the same view as a pyramid (dvo_amd_volume_raycast_pyramid), the second frame tracked against the model
 * Prints counts and checksums -- what examples/volume_adaptor_example.cpp prints through the C++ adaptor.  Input files: float32
 * planes without a header, as tests/test_volume_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/volume_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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
  if (argc < 11) {
    fprintf(stderr, "usage: %s w h fx fy ox oy first_i first_z second_i second_z [surface.pcd]\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[4];
  for (int k = 0; k < 4; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frames[2] = {NULL, NULL}, *model = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_pyramid_create(0, planes[0], planes[1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frames[0]));
  CHECK(dvo_amd_pyramid_create(0, planes[2], planes[3], w, h, w, fx, fy, ox, oy, levels, 1.0, &frames[1]));

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frames[0], frames[1], NULL, &res));

  dvo_amd_volume_options vopt;
  dvo_amd_default_volume_options(&vopt);
  dvo_amd_volume *vol = NULL;
  CHECK(dvo_amd_volume_create(0, &vopt, &vol));
  double poses[32];
  memset(poses, 0, sizeof(poses));
  poses[0] = poses[5] = poses[10] = poses[15] = 1.0;
  memcpy(poses + 16, res.transformation, 16 * sizeof(double));
  const int ids[2] = {0, 1};
  dvo_amd_volume_counts counts[2];
  CHECK(dvo_amd_volume_insert(vol, 2, ids, frames, 0, poses, counts));
  printf("insert counts %lld %lld %lld %lld %lld %lld\n", counts[0].updated, counts[0].near, counts[0].free, counts[1].updated, counts[1].near,
         counts[1].free);

  const dvo_amd_view view = {w, h, fx, fy, ox, oy, vopt.near_z};
  dvo_amd_volume_raycast_options ropt;
  dvo_amd_default_volume_raycast_options(&ropt);
  float *depth = malloc(4 * n);
  if (!depth) return 2;
  dvo_amd_volume_raycast_stats st;
  CHECK(dvo_amd_volume_raycast(vol, poses, &view, &ropt, depth, NULL, NULL, &st));
  printf("raycast stats %lld %lld %lld %lld %lld\n", st.pixels, st.hit, st.backface, st.missed, st.uncoloured);
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (depth[i] == depth[i]) sum += depth[i]; /* (NaN: not hit) */
  printf("raycast checksum %.17g\n", sum);

  long long n_points = 0;
  dvo_amd_volume_extract_counts ec;
  int rc = dvo_amd_volume_extract(vol, 1, NULL, 0, &n_points, &ec);
  if (rc != DVO_AMD_OK && rc != DVO_AMD_ERR_CAPACITY) CHECK(rc);
  dvo_amd_point *points = malloc(sizeof(dvo_amd_point) * (size_t)(n_points > 0 ? n_points : 1));
  if (!points) return 2;
  CHECK(dvo_amd_volume_extract(vol, 1, points, n_points, &n_points, &ec));
  sum = 0.0;
  for (long long i = 0; i < n_points; ++i) sum += points[i].x;
  printf("extract counts %lld %lld checksum %.17g\n", ec.points, ec.uncoloured, sum);
  if (argc > 11) CHECK(dvo_amd_write_pcd(argv[11], points, n_points, (int)n_points, 1));

  CHECK(dvo_amd_volume_raycast_pyramid(vol, poses, &view, &ropt, levels, 2.0, &model, NULL));
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, model, frames[1], NULL, &res));
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_pyramid_release(model);
  dvo_amd_volume_destroy(vol);
  dvo_amd_pyramid_release(frames[0]);
  dvo_amd_pyramid_release(frames[1]);
  dvo_amd_context_destroy(ctx);
  free(points), free(depth);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  return 0;
}
