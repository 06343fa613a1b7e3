/* Exposure compensation through the C ABI, from C99: a current frame whose camera changed its exposure is aligned against a
 * reference.
 *   plain      the current frame aligned as it is
 *   estimate   the gain and bias with which the current frame looks like the reference, fitted on the device at the identity (what
 *              a tracker has before its first match): I_ref ~ gain * I_cur + bias
 *   adjust     the current frame with that model applied: a new pyramid, depth untouched
 *   match      the adjusted frame aligned against the reference
 * Prints the estimate with its sums, and a checksum of both poses.  Input files: float32 planes without a header, as
 * tests/test_exposure_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/exposure_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
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

static double checksum(const double *T) {
  double sum = 0.0;
  for (int k = 0; k < 16; ++k) sum += T[k];
  return sum;
}

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
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frame[2] = {NULL, NULL}, *adjusted = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  for (int k = 0; k < 2; ++k)
    CHECK(dvo_amd_pyramid_create(0, planes[2 * k], planes[2 * k + 1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frame[k]));

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frame[0], frame[1], NULL, &res));
  printf("plain checksum %.17g isnan %d\n", checksum(res.transformation), res.is_nan);

  /* no transformation: the identity; no mask: every pixel of the reference */
  dvo_amd_exposure_options opt;
  dvo_amd_default_exposure_options(&opt);
  dvo_amd_exposure_estimate e;
  CHECK(dvo_amd_estimate_exposure(ctx, frame[0], frame[1], NULL, NULL, &opt, &e));
  printf("estimate gain %.17g bias %.17g r2 %.17g passes %d degenerate %d\n", e.gain, e.bias, e.r2, e.passes, e.degenerate);
  printf("counts valid %lld consistent %lld masked %lld saturated %lld candidates %lld used %lld trimmed %lld\n", e.valid, e.consistent,
         e.masked, e.saturated, e.candidates, e.used, e.trimmed);
  printf("sums n %lld sx %lld sy %lld sxx %lld sxy %lld syy %lld\n", e.n, e.sx, e.sy, e.sxx, e.sxy, e.syy);

  CHECK(dvo_amd_pyramid_adjust_intensity(frame[1], e.gain, e.bias, &adjusted));
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frame[0], adjusted, NULL, &res));
  printf("compensated checksum %.17g isnan %d\n", checksum(res.transformation), res.is_nan);

  dvo_amd_pyramid_release(adjusted);
  for (int k = 0; k < 2; ++k) dvo_amd_pyramid_release(frame[k]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  return 0;
}
