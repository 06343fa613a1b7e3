/* Loop-closure candidates by appearance through the C ABI, from C99: no pose is asked for anywhere.
 *   index     one int8 descriptor per keyframe on the device (dvo_amd_place_index_add: one launch for all of them)
 *   query     the keyframes that look most like keyframe 0 (dvo_amd_place_query), and most like a frame that is no keyframe
 *             (dvo_amd_place_query_frames: relocalisation)
 *   dots      the exact int32 dot products behind the scores (dvo_amd_place_scores)
 * The candidates feed dvo_amd_proposals_for_candidates like the radius search's (examples/constraint_search_example.c).
 * Input files: float32 planes without a header, as tests/test_place_index_adaptor.py writes them; the last pair is the frame.
 *   cc -std=c99 -Iinclude examples/place_index_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>

#include "dvo_amd.h"

#define MAX_FRAMES 64
#define K 3

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

static void print_found(const char *what, const int *ids, const double *scores, int count) {
  printf("%s:", what);
  for (int t = 0; t < count; ++t) printf(" %d:%.17g", ids[t], scores[t]);
  printf("\n");
}

int main(int argc, char **argv) {
  const int n_files = argc - 7;
  if (argc < 7 + 4 || n_files % 2 != 0 || n_files / 2 > MAX_FRAMES) {
    fprintf(stderr, "usage: %s w h fx fy ox oy kf0_i kf0_z [kf1_i kf1_z ...] frame_i frame_z\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), n_keyframes = n_files / 2 - 1;
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;

  dvo_amd_place_options opt;
  dvo_amd_default_place_options(&opt);
  const dvo_amd_pyramid *pyramid[MAX_FRAMES];
  dvo_amd_pyramid *owned[MAX_FRAMES];
  for (int k = 0; k <= n_keyframes; ++k) {
    float *intensity = read_file(argv[7 + 2 * k], 4 * n), *depth = read_file(argv[8 + 2 * k], 4 * n);
    CHECK(dvo_amd_pyramid_create(0, intensity, depth, w, h, w, fx, fy, ox, oy, opt.level + 1, 0.0, &owned[k]));
    pyramid[k] = owned[k];
    free(intensity);
    free(depth);
  }

  dvo_amd_place_index *index = NULL;
  int first = -1, size = 0, dim = 0;
  CHECK(dvo_amd_place_index_create(0, &opt, &index));
  CHECK(dvo_amd_place_index_add(index, n_keyframes, pyramid, &first));
  CHECK(dvo_amd_place_index_info(index, &size, NULL, NULL, &dim));
  printf("index size %d dim %d first %d\n", size, dim, first);

  dvo_amd_place_query_options query;
  dvo_amd_default_place_query_options(&query);
  query.k = K;
  int ids[K], count = 0;
  double scores[K];
  const int keyframe = 0;
  CHECK(dvo_amd_place_query(index, 1, &keyframe, &query, ids, scores, &count));
  print_found("keyframe 0", ids, scores, count);
  CHECK(dvo_amd_place_query_frames(index, 1, &pyramid[n_keyframes], &query, ids, scores, &count));
  print_found("frame", ids, scores, count);

  int dots[MAX_FRAMES];
  CHECK(dvo_amd_place_scores(index, 1, &keyframe, 0, size, dots));
  printf("dots:");
  for (int j = 0; j < size; ++j) printf(" %d", dots[j]);
  printf("\n");

  dvo_amd_place_index_destroy(index);
  for (int k = 0; k <= n_keyframes; ++k) dvo_amd_pyramid_release(owned[k]);
  return 0;
}
