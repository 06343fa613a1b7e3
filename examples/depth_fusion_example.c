/* Depth fusion through the C ABI, from C99: the frames tracked against a keyframe are averaged into its depth before it is used again.
 *   match     frames 1, 2 and 3 aligned against the keyframe
 *   fused     the keyframe with the three frames' depth carried onto its pixels by the poses the matches returned and averaged
 *             into its own (dvo_amd_pyramid_fuse_depth): a new ordinary pyramid, the keyframe itself is only read
 *   track     frame 4 tracked against the fused keyframe
 * Nothing leaves the device between the steps.  Prints the keyframe counts, a checksum of the fused depth and a checksum of the
 * pose.  Input files: float32 planes without a header, as tests/test_depth_fusion_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/depth_fusion_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvo_amd.h"

#define FRAMES 5 /* the keyframe, three frames to fuse, one to track */

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
  if (argc < 7 + 2 * FRAMES) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf_i kf_z f1_i f1_z f2_i f2_z f3_i f3_z f4_i f4_z\n", argv[0]);
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
  dvo_amd_pyramid *frame[FRAMES] = {NULL, NULL, NULL, NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < FRAMES; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  /* the three alignments against the keyframe: their transformations, as returned, are what the fusion takes */
  double T[3 * 16];
  const dvo_amd_pyramid *tracked[3];
  for (int k = 0; k < 3; ++k) {
    dvo_amd_result res;
    memset(&res, 0, sizeof(res));
    CHECK(dvo_amd_match(ctx, frame[0], frame[1 + k], NULL, &res));
    memcpy(T + 16 * k, res.transformation, sizeof(res.transformation));
    tracked[k] = frame[1 + k];
  }

  dvo_amd_fuse_options opt;
  dvo_amd_default_fuse_options(&opt);
  dvo_amd_pyramid *fused = NULL;
  long long frame_counts[3 * DVO_AMD_FUSE_FRAME_COUNTS], keyframe_counts[DVO_AMD_FUSE_KEYFRAME_COUNTS];
  CHECK(dvo_amd_pyramid_fuse_depth(frame[0], 3, tracked, T, &opt, &fused, frame_counts, keyframe_counts, NULL));
  for (int k = 0; k < 3; ++k) {
    const long long *c = frame_counts + DVO_AMD_FUSE_FRAME_COUNTS * k;
    fprintf(stderr, "frame %d: valid %lld behind %lld outside %lld no_depth %lld consistent %lld occluded %lld seen_through %lld fused %lld\n",
            k + 1, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
  }
  printf("fused counts %lld %lld %lld %lld\n", keyframe_counts[0], keyframe_counts[1], keyframe_counts[2], keyframe_counts[3]);

  float *depth = malloc(4 * n);
  if (!depth) return 2;
  CHECK(dvo_amd_pyramid_download_plane(fused, 0, 1, depth));
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (depth[i] == depth[i]) sum += depth[i]; /* (NaN: no depth) */
  printf("fused checksum %.17g\n", sum);

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, fused, frame[4], NULL, &res));
  sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += res.transformation[k];
  printf("track checksum %.17g isnan %d\n", sum, res.is_nan);

  dvo_amd_pyramid_release(fused);
  for (int k = 0; k < FRAMES; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 2 * FRAMES; ++k) free(planes[k]);
  free(depth);
  return 0;
}
