/* Surface normals through the C ABI, from C99: which way the surfaces of a keyframe face, and what that is good for.
 *   normals   level 0's normal plane and the reference's `angles` by RgbdImage::calculateNormals' own rule (default options)
 *   facing    a mask of the pixels whose windowed normal looks at the camera (cosine to the viewing ray >= 0.5) on every level,
 *             from ONE kernel launch (dvo_amd_mask_from_normals): surfaces seen at a grazing angle, where depth noise and flying
 *             pixels are worst, are dropped
 *   track     the mask eroded by a pixel, the next frame tracked behind it: mask -> erode -> dvo_amd_match_masked
 *   cloud     the keyframe's cloud with normals, written as a PointXYZRGBNormal PCD file a mesher can read
 * Nothing but the results leaves the device.  Prints the counts, the kept pixels and a checksum of the pose; writes level 0's
 * normals (w*h*4 floats), its angles (w*h floats) and the facing mask's planes to `out`.  Input files: float32 planes without a
 * header, as tests/test_normals_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/normals_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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
  if (argc < 13) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z out.bin cloud.pcd\n", argv[0]);
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
  dvo_amd_pyramid *frame[2] = {NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < 2; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  /* the reference's members: normals (x, y, z, 0; four NaNs where there is none) and angles (|n.z|) */
  dvo_amd_normal_options plain;
  dvo_amd_default_normal_options(&plain);
  float *normals = malloc(16 * n), *angles = malloc(4 * n);
  if (!normals || !angles) return 2;
  long long counts[2];
  CHECK(dvo_amd_pyramid_normals(frame[0], 0, &plain, normals, angles, counts));
  printf("normals counts %lld %lld\n", counts[0], counts[1]);

  /* a 7x7 window on level 0, smaller ones above it, members within 2 % of the centre's depth; facing = cosine to the viewing ray */
  dvo_amd_normal_options opt;
  dvo_amd_default_normal_options(&opt);
  for (int l = 0; l < levels; ++l) opt.radius[l] = l < 3 ? 3 - l : 0;
  opt.depth_step_ratio = 0.02f, opt.facing = DVO_AMD_NORMAL_FACING_RAY, opt.toward_camera = 1;
  float min_facing[DVO_AMD_MAX_LEVELS];
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) min_facing[l] = 0.5f;
  dvo_amd_mask *facing = NULL, *eroded = NULL;
  long long mask_counts[3 * DVO_AMD_MAX_LEVELS];
  CHECK(dvo_amd_mask_from_normals(frame[0], &opt, min_facing, 0, &facing, mask_counts));
  for (int l = 0; l < levels; ++l)
    printf("mask counts %d %lld %lld %lld\n", l, mask_counts[3 * l], mask_counts[3 * l + 1], mask_counts[3 * l + 2]);

  int radius[DVO_AMD_MAX_LEVELS];
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) radius[l] = (1 + (1 << l) - 1) >> l; /* one pixel of level 0, rounded up */
  CHECK(dvo_amd_mask_morph(facing, DVO_AMD_MASK_ERODE, radius, &eroded));
  long long kept[DVO_AMD_MAX_LEVELS];
  CHECK(dvo_amd_mask_info(eroded, NULL, NULL, NULL, kept));
  for (int l = 0; l < levels; ++l) printf("eroded kept %d %lld\n", l, kept[l]);

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match_masked(ctx, frame[0], eroded, cfg.intensity_derivative_threshold, cfg.depth_derivative_threshold, frame[1], NULL, &res));
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  FILE *out = fopen(argv[11], "wb");
  if (!out || fwrite(normals, 16, n, out) != n || fwrite(angles, 4, n, out) != n) return 2;
  unsigned char *bytes = malloc(n);
  if (!bytes) return 2;
  for (int l = 0; l < levels; ++l) {
    const size_t nl = (size_t)(w >> l) * (size_t)(h >> l);
    CHECK(dvo_amd_mask_download(facing, l, bytes));
    if (fwrite(bytes, 1, nl, out) != nl) return 2;
  }
  if (fclose(out) != 0) return 2;

  /* the keyframe's cloud with the windowed normals, at the identity pose, grey from the intensity plane */
  dvo_amd_point *points = malloc(n * sizeof(*points));
  if (!points) return 2;
  CHECK(dvo_amd_point_cloud_normals(ctx, frame[0], 0, NULL, NULL, 0, &opt, points, normals));
  CHECK(dvo_amd_write_pcd_normals(argv[12], points, normals, (long long)n, w, h));
  printf("cloud points %lld\n", (long long)n);

  dvo_amd_mask_release(facing);
  dvo_amd_mask_release(eroded);
  for (int k = 0; k < 2; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  free(normals), free(angles), free(bytes), free(points);
  return 0;
}
