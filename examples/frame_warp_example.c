/* Frame warps through the C ABI, from C99: a frame resampled into another frame's pixels, in both directions.
 *   match     the moving frame aligned against the fixed frame: the transformation, as returned, is what both warps take
 *   inverse   the moving frame's grey values gathered onto the fixed frame's pixels (dvo_amd_warp_inverse): host planes
 *   forward   the moving frame's pixels drawn into the fixed camera with a nearest-depth test (dvo_amd_warp_forward)
 *   track     the inverse warp as a pyramid (dvo_amd_pyramid_warp_inverse) with the fixed camera's depth
 *             (DVO_AMD_WARP_DEPTH_FIXED), tracked against the fixed frame: what is left of the motion once the frame has been
 *             carried over.  (With the default, the reference's transformed depth, the depth plane still shows the moving camera's
 *             geometry and the tracker finds that motion again.)
 * Prints the counts and a checksum of each direction and a checksum of the pose.  Input files: float32 planes without a header, as
 * tests/test_frame_warp_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/frame_warp_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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
    fprintf(stderr, "usage: %s w h fx fy ox oy fixed_i fixed_z moving_i moving_z\n", argv[0]);
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
  dvo_amd_pyramid *fixed = NULL, *moving = NULL, *warped = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_pyramid_create(0, planes[0], planes[1], w, h, w, fx, fy, ox, oy, levels, 0.0, &fixed));
  CHECK(dvo_amd_pyramid_create(0, planes[2], planes[3], w, h, w, fx, fy, ox, oy, levels, 1.0, &moving));

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, fixed, moving, NULL, &res));

  dvo_amd_warp_options opt;
  dvo_amd_default_warp_options(&opt);
  float *intensity = malloc(4 * n), *depth = malloc(4 * n);
  int *index = malloc(sizeof(int) * n);
  if (!intensity || !depth || !index) return 2;

  long long ic[DVO_AMD_WARP_INVERSE_COUNTS];
  CHECK(dvo_amd_warp_inverse(fixed, moving, res.transformation, 0, &opt, intensity, depth, ic));
  printf("inverse counts %lld %lld %lld %lld %lld %lld %lld %lld\n", ic[0], ic[1], ic[2], ic[3], ic[4], ic[5], ic[6], ic[7]);
  double sum = 0.0, before = 0.0, after = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (intensity[i] == intensity[i]) { /* (NaN: not warped) */
      sum += intensity[i];
      const double a = (double)planes[0][i] - (double)intensity[i], b = (double)planes[0][i] - (double)planes[2][i];
      after += a < 0 ? -a : a, before += b < 0 ? -b : b;
    }
  printf("inverse checksum %.17g\n", sum);
  if (ic[5] > 0)
    fprintf(stderr, "mean |I_fixed - I_moving| over the warped pixels: %.3f as recorded, %.3f warped\n", before / (double)ic[5], after / (double)ic[5]);

  long long fc[DVO_AMD_WARP_FORWARD_COUNTS];
  opt.splat = DVO_AMD_WARP_SPLAT_FOOTPRINT;
  CHECK(dvo_amd_warp_forward(moving, res.transformation, NULL, 0, &opt, depth, intensity, index, fc));
  printf("forward counts %lld %lld %lld %lld %lld %lld %lld\n", fc[0], fc[1], fc[2], fc[3], fc[4], fc[5], fc[6]);
  sum = 0.0;
  long long index_sum = 0;
  for (size_t i = 0; i < n; ++i)
    if (index[i] >= 0) sum += depth[i], index_sum += index[i];
  printf("forward checksum %.17g %lld\n", sum, index_sum);

  dvo_amd_default_warp_options(&opt);
  opt.depth = DVO_AMD_WARP_DEPTH_FIXED;
  CHECK(dvo_amd_pyramid_warp_inverse(fixed, moving, res.transformation, &opt, &warped, NULL));
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, fixed, warped, NULL, &res));
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_pyramid_release(warped);
  dvo_amd_pyramid_release(moving);
  dvo_amd_pyramid_release(fixed);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  free(intensity), free(depth), free(index);
  return 0;
}
