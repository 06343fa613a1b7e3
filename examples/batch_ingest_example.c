/* Frame-to-frame odometry over a short recorded sequence from C99: N raw frames (uint8 BGR + uint16 depth) become N pyramids in
 * ONE call, each with its point selection already built, and one dvo_amd_match_batch aligns the N - 1 consecutive pairs.  The
 * frames are synthetic -- a textured, tilted plane that slides sideways from frame to frame -- so the example needs no files.
 *   cc -std=c99 -Iinclude examples/batch_ingest_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <string.h>

#include "dvo_amd.h"

enum { W = 160, H = 120, N = 6, LEVELS = 3 };

static unsigned char bgr[N][H][W][3];
static unsigned short depth[N][H][W];

#define CHECK(call)                                                                                         \
  do {                                                                                                      \
    int rc_ = (call);                                                                                       \
    if (rc_ != DVO_AMD_OK) {                                                                                \
      fprintf(stderr, "%s: %s [%s]\n", #call, dvo_amd_status_string(rc_), dvo_amd_last_error());             \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

int main(void) {
  const unsigned char *images[N];
  const unsigned short *depths[N];
  double stamps[N];
  for (int f = 0; f < N; ++f) {
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int s = u + 2 * f; /* the scene moves two pixels per frame */
        bgr[f][v][u][0] = (unsigned char)(128 + 60 * ((s / 8 + v / 8) % 2) + (s * 3 + v * 5) % 23);
        bgr[f][v][u][1] = (unsigned char)(100 + (s * 7 + v) % 90);
        bgr[f][v][u][2] = (unsigned char)(90 + (s + v * 11) % 110);
        depth[f][v][u] = (u + v) % 37 == 0 ? 0 : (unsigned short)(7000 + 12 * s + 9 * v); /* 0 = no measurement */
      }
    images[f] = &bgr[f][0][0][0], depths[f] = &depth[f][0][0], stamps[f] = 0.033 * f;
  }

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  cfg.first_level = LEVELS - 1, cfg.last_level = 0;
  dvo_amd_context *ctx = NULL;
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));

  dvo_amd_raw_batch batch;
  memset(&batch, 0, sizeof(batch));
  batch.count = N, batch.images = images, batch.depths = depths, batch.timestamps = stamps;
  batch.channels = 3, batch.image_stride_bytes = 3 * W, batch.depth_stride = W, batch.depth_scale = 1.0f / 5000.0f;
  batch.on_device = 0, batch.width = W, batch.height = H;
  batch.fx = 140.0f, batch.fy = 140.0f, batch.ox = 79.5f, batch.oy = 59.5f, batch.levels = LEVELS;
  /* the tracker's own thresholds: the selections the matches below ask for are the ones the batch leaves behind */
  batch.build_selection = 1;
  batch.intensity_threshold = cfg.intensity_derivative_threshold, batch.depth_threshold = cfg.depth_derivative_threshold;
  dvo_amd_pyramid *pyr[N];
  CHECK(dvo_amd_pyramid_create_raw_batch(0, &batch, pyr));

  /* pair k: frame k is the reference, frame k + 1 the current image */
  dvo_amd_result res[N - 1];
  memset(res, 0, sizeof(res));
  CHECK(dvo_amd_match_batch(ctx, N - 1, pyr, pyr + 1, NULL, res));
  for (int k = 0; k < N - 1; ++k)
    printf("pair %d -> %d (t = %.3f s): isnan %d, translation %.6f %.6f %.6f\n", k, k + 1, dvo_amd_pyramid_timestamp(pyr[k + 1]),
           res[k].is_nan, res[k].transformation[12], res[k].transformation[13], res[k].transformation[14]);

  for (int f = 0; f < N; ++f) dvo_amd_pyramid_release(pyr[f]);
  dvo_amd_context_destroy(ctx);
  return 0;
}
