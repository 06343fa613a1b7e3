/* Depth filtering through the C ABI, from C99: two frames' depth is denoised on the device before they are tracked.
 *   filter    both frames in ONE call (dvo_amd_pyramid_filter_depth_many): a 5x5 edge-preserving filter whose range scale is the
 *             sensor's noise model, pixels fewer than four window members agree with dropped, one-pixel holes filled; two new
 *             ordinary pyramids, the inputs are only read
 *   track     the filtered frame tracked against the filtered keyframe
 * Nothing leaves the device between the steps.  Prints each frame's counts, a checksum of the keyframe's filtered depth and a
 * checksum of the pose, and writes the keyframe's filtered plane and its support plane to `out`.  Input files: float32 planes
 * without a header, as tests/test_depth_filter_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/depth_filter_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvo_amd.h"

#define FRAMES 2 /* the keyframe and the frame tracked against it */

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
  if (argc < 8 + 2 * FRAMES) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z out.bin\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[2 * FRAMES];
  for (int k = 0; k < 2 * FRAMES; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frame[FRAMES] = {NULL, NULL}, *filtered[FRAMES] = {NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < FRAMES; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  dvo_amd_depth_filter_options opt;
  dvo_amd_default_depth_filter_options(&opt);
  opt.min_support = 4, opt.fill_radius = 1;
  long long counts[FRAMES * DVO_AMD_DEPTH_FILTER_COUNTS];
  unsigned short *support = malloc(2 * n);
  float *depth = malloc(4 * n);
  if (!support || !depth) return 2;
  unsigned short *supports[FRAMES] = {NULL, NULL};
  supports[0] = support; /* the keyframe's only */
  const dvo_amd_pyramid *inputs[FRAMES];
  for (int k = 0; k < FRAMES; ++k) inputs[k] = frame[k];
  CHECK(dvo_amd_pyramid_filter_depth_many(FRAMES, inputs, &opt, filtered, counts, supports));
  for (int k = 0; k < FRAMES; ++k) {
    const long long *c = counts + DVO_AMD_DEPTH_FILTER_COUNTS * k;
    printf("filter counts %d %lld %lld %lld %lld %lld\n", k, c[0], c[1], c[2], c[3], c[4]);
  }

  CHECK(dvo_amd_pyramid_download_plane(filtered[0], 0, 1, depth));
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (depth[i] == depth[i]) sum += depth[i]; /* (NaN: no depth) */
  printf("filtered checksum %.17g\n", sum);

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, filtered[0], filtered[1], NULL, &res));
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  FILE *out = fopen(argv[7 + 2 * FRAMES], "wb");
  if (!out || fwrite(depth, 4, n, out) != n || fwrite(support, 2, n, out) != n || fclose(out) != 0) return 2;

  for (int k = 0; k < FRAMES; ++k) dvo_amd_pyramid_release(filtered[k]), dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 2 * FRAMES; ++k) free(planes[k]);
  free(depth), free(support);
  return 0;
}
