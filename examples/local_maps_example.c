/* Three local maps optimized in one call through the C ABI (dvo_amd_optimize_graphs_batch), the way LocalMap::optimize runs
 * Levenberg on each of them: a fixed keyframe, one vertex per frame, an odometry edge and a keyframe edge per frame.
 * Plain C99:  cc -std=c99 -Iinclude examples/local_maps_example.c -Ldvo_slam_amd -ldvo_amd -lm */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "dvo_amd.h"

#define N_MAPS 3
#define MAX_FRAMES 12

/* column-major 4x4: rotation about z by a, then translation t */
static void pose_z(double a, double tx, double ty, double *T) {
  memset(T, 0, 16 * sizeof(double));
  T[0] = cos(a);
  T[1] = sin(a);
  T[4] = -sin(a);
  T[5] = cos(a);
  T[10] = 1.0;
  T[12] = tx;
  T[13] = ty;
  T[15] = 1.0;
}

/* C = A^-1 B for rigid transforms */
static void relative(const double *A, const double *B, double *C) {
  double Ai[16];
  int r, c, k;
  memset(Ai, 0, sizeof(Ai));
  for (r = 0; r < 3; ++r)
    for (c = 0; c < 3; ++c) Ai[c * 4 + r] = A[r * 4 + c];
  for (r = 0; r < 3; ++r) Ai[12 + r] = -(Ai[r] * A[12] + Ai[4 + r] * A[13] + Ai[8 + r] * A[14]);
  Ai[15] = 1.0;
  for (r = 0; r < 4; ++r)
    for (c = 0; c < 4; ++c) {
      double s = 0.0;
      for (k = 0; k < 4; ++k) s += Ai[k * 4 + r] * B[c * 4 + k];
      C[c * 4 + r] = s;
    }
}

static void set_edge(dvo_amd_graph_edge *e, int from, int to, double truth[][16]) {
  int i;
  e->from = from;
  e->to = to;
  relative(truth[from], truth[to], e->measurement);
  memset(e->information, 0, sizeof(e->information));
  for (i = 0; i < 6; ++i) e->information[i * 7] = i < 3 ? 400.0 : 2500.0;
}

int main(void) {
  static double truth[N_MAPS][MAX_FRAMES + 1][16], poses[N_MAPS][MAX_FRAMES + 1][16];
  static int fixed[N_MAPS][MAX_FRAMES + 1];
  static dvo_amd_graph_edge edges[N_MAPS][2 * MAX_FRAMES];
  const int frames[N_MAPS] = {6, 9, MAX_FRAMES}; /* the maps differ in size */
  dvo_amd_graph_batch_item items[N_MAPS];
  dvo_amd_graph_options opt;
  dvo_amd_context *ctx = NULL;
  int g, i, rc, ok = 1;

  for (g = 0; g < N_MAPS; ++g) {
    int n_edges = 0;
    for (i = 0; i <= frames[g]; ++i) { /* vertex 0 is the keyframe; the frames move along an arc */
      const double a = 0.05 * i + 0.3 * g;
      pose_z(a, 2.0 * cos(a), 2.0 * sin(a), truth[g][i]);
      /* the estimate drifts: 1 cm and 0.3 degrees more per frame */
      pose_z(a + 0.005 * i, (2.0 + 0.01 * i) * cos(a), (2.0 + 0.01 * i) * sin(a), poses[g][i]);
      fixed[g][i] = i == 0;
    }
    for (i = 1; i <= frames[g]; ++i) {
      set_edge(&edges[g][n_edges++], i - 1, i, truth[g]);        /* odometry */
      if (i > 1) set_edge(&edges[g][n_edges++], 0, i, truth[g]); /* the keyframe's edge */
    }
    memset(&items[g], 0, sizeof(items[g]));
    items[g].n_vertices = frames[g] + 1;
    items[g].poses = &poses[g][0][0];
    items[g].fixed = fixed[g];
    items[g].n_edges = n_edges;
    items[g].edges = edges[g];
  }

  if (dvo_amd_device_count() < 1) {
    printf("no HIP device\n");
    return 0;
  }
  rc = dvo_amd_context_create(0, NULL, &ctx);
  if (rc != DVO_AMD_OK) return 1;
  dvo_amd_default_graph_options(DVO_AMD_GRAPH_LEVENBERG, &opt);
  rc = dvo_amd_optimize_graphs_batch(ctx, N_MAPS, items, &opt);
  if (rc == DVO_AMD_OK) {
    for (g = 0; g < N_MAPS; ++g) {
      const dvo_amd_graph_stats *s = &items[g].stats;
      printf("local map %d: %d free vertices, %d iterations, termination %d, F %.6g -> %.6g\n", g, s->n_free, s->iterations,
             s->termination, s->initial_objective, s->final_objective);
      ok = ok && s->final_objective < s->initial_objective;
    }
  } else {
    printf("dvo_amd_optimize_graphs_batch: %s (%s)\n", dvo_amd_status_string(rc), dvo_amd_last_error());
  }
  dvo_amd_context_destroy(ctx);
  return rc == DVO_AMD_OK && ok ? 0 : 1;
}
