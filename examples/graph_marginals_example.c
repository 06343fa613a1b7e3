/* A loop-closed ring of keyframes optimized with dogleg, then the marginal covariance of every keyframe
 * (dvo_amd_graph_marginals, the role of g2o's computeMarginals): the trace of each vertex's positional covariance grows with
 * the distance from the fixed keyframe and shrinks at the loop closures.
 * Plain C99:  cc -std=c99 -Iinclude examples/graph_marginals_example.c -Ldvo_slam_amd -ldvo_amd -lm */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "dvo_amd.h"

#define N_VERTICES 12

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

int main(void) {
  double truth[N_VERTICES][16], poses[N_VERTICES][16];
  int fixed[N_VERTICES] = {1};
  dvo_amd_graph_edge edges[N_VERTICES + 2];
  dvo_amd_graph_options opt;
  dvo_amd_graph_stats stats;
  dvo_amd_graph_marginal_stats mstats;
  int block_a[N_VERTICES], block_b[N_VERTICES];
  double blocks[N_VERTICES][36];
  dvo_amd_context *ctx = NULL;
  int i, k, n_edges = 0, rc;
  const double pi = 3.14159265358979323846;

  for (i = 0; i < N_VERTICES; ++i) {
    const double a = 2.0 * pi * i / N_VERTICES;
    pose_z(a, 2.0 * cos(a), 2.0 * sin(a), truth[i]);
    /* the estimate drifts: 2 cm and 0.5 degrees more per keyframe */
    pose_z(a + 0.0087 * i, (2.0 + 0.02 * i) * cos(a), (2.0 + 0.02 * i) * sin(a), poses[i]);
  }
  for (i = 0; i < N_VERTICES; ++i) { /* odometry ring, then two loop closures */
    edges[n_edges].from = i;
    edges[n_edges].to = (i + 1) % N_VERTICES;
    ++n_edges;
  }
  edges[n_edges].from = 0, edges[n_edges].to = N_VERTICES / 2, ++n_edges;
  edges[n_edges].from = 3, edges[n_edges].to = 9, ++n_edges;
  for (k = 0; k < n_edges; ++k) {
    relative(truth[edges[k].from], truth[edges[k].to], edges[k].measurement);
    memset(edges[k].information, 0, sizeof(edges[k].information));
    for (i = 0; i < 6; ++i) edges[k].information[i * 7] = i < 3 ? 100.0 : 1000.0;
  }

  if (dvo_amd_device_count() < 1) {
    printf("no HIP device\n");
    return 0;
  }
  rc = dvo_amd_context_create(0, NULL, &ctx);
  if (rc != DVO_AMD_OK) return 1;
  dvo_amd_default_graph_options(DVO_AMD_GRAPH_DOGLEG, &opt);
  rc = dvo_amd_optimize_graph(ctx, N_VERTICES, &poses[0][0], fixed, n_edges, edges, &opt, NULL, NULL, 0, NULL, &stats);
  if (rc == DVO_AMD_OK) {
    printf("dogleg: %d iterations, F %.6g -> %.6g\n", stats.iterations, stats.initial_objective, stats.final_objective);
    for (i = 0; i < N_VERTICES; ++i) block_a[i] = block_b[i] = i; /* a == b: the vertex's own 6 x 6 covariance */
    rc = dvo_amd_graph_marginals(ctx, N_VERTICES, &poses[0][0], fixed, n_edges, edges, &opt, N_VERTICES, block_a, block_b,
                                 &blocks[0][0], &mstats);
  }
  if (rc == DVO_AMD_OK) {
    printf("%d free vertices, factorized %d\n", mstats.n_free, mstats.factorized);
    for (i = 0; i < N_VERTICES; ++i) /* column-major: entry (r, c) at c * 6 + r; the fixed keyframe's block is zeros */
      printf("vertex %2d: trace of the positional covariance %.6g m^2\n", i, blocks[i][0] + blocks[i][7] + blocks[i][14]);
  } else {
    printf("%s\n", dvo_amd_status_string(rc));
  }
  dvo_amd_context_destroy(ctx);
  return rc == DVO_AMD_OK ? 0 : 1;
}
